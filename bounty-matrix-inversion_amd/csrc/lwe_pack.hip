// Compression of output ciphertexts (2^64 torus, k = 1): up to N big-key LWE ciphertexts are packed into the N coefficients of one
// GLWE ciphertext by a packing keyswitch, and the GLWE words are modulus-switched to log_modulus bits each (TFHE-rs' compressed
// ciphertext list).  Plain u64 wrap-around arithmetic throughout; include/bmi_tfhe.h states the scheme, tests/compress_cases.py
// restates it in numpy.
//
// The compression key is the matrix KEY[K = N L rows][2N columns]: row j L + l = [A | B], a GLWE encryption of the constant
// polynomial S_j 2^(64 - b (l + 1)) under the context's GLWE key (the standard layout IS the layout of the product's loads).
// A block of m <= N ciphertexts (a_i, b_i) goes through four kernels, slice by slice of at most `slice` ciphertexts so that the
// scratch stays bounded:
//   k_pack_digits    D[i][j L + l] = d[i][j][l] + 2^(b-1), the digits of a_i[j] by the oracle's rule (ora_decompose: centred lift,
//                    round half up to the top L b bits, balanced digits from the least significant, the top digit absorbs the
//                    carry), staged UNSIGNED in [0, 2^b] (the top digit reaches +2^(b-1): no int16) like the keyswitch's;
//   k_pack_product   T[i][col] = (col == N ? b_i : 0) + BIAS[col] - sum_k D[i][k] KEY[k][col],  BIAS[col] = 2^(b-1) sum_k KEY[k][col]:
//                    a register-tiled integer matrix product - a workgroup of 256 threads owns 64 ciphertexts x 64 columns, a thread
//                    4 x 4 sums of 64 bits; digits and key words of 16 rows at a time are staged in LDS (the next 16 rows are
//                    requested before the current ones are multiplied), so every key word serves 4 ciphertexts and every digit 4
//                    columns per LDS read;
//   k_pack_rotate    ACC[comp][c] (+)= sum_i X^i T_i: coefficient c receives +T_i[c - i] for i <= c and -T_i[N + c - i] for i > c;
//   k_pack_switch    the centred modulus switch of modswitch_centre.hip carried over to a polynomial, one workgroup per block: with
//                    Sh = 64 - log_modulus, e_j = ((A_j + 2^(Sh-1)) mod 2^Sh) - 2^(Sh-1), P_x = sum_{j<=x} e_j (workgroup-wide
//                    inclusive prefix sum, int64), E = P_{N-1}, B'_x = B_x - ((2 P_x - E) >> 1) (arithmetic shift), and the outputs
//                    ((A_j + 2^(Sh-1)) >> Sh) and ((B'_x + 2^(Sh-1)) >> Sh) as uint32: N mask values, then m body values.
//                    (|2 P_x - E| <= N 2^(Sh-1): no int64 overflow for log_modulus > log2 N; below that the sums wrap, as the numpy
//                    restatement's do - such widths carry no message anyway.)
// Partial tiles are predicated: a ciphertext row past m is neither read nor written.
#include <hip/hip_runtime.h>

#include "bmi_internal.hpp"

namespace {

using bmi::i64;
using bmi::u64;

constexpr int PK_BM = 64, PK_BN = 64, PK_BK = 16;   // tile of the product: ciphertexts x columns, key rows per LDS stage
constexpr int PK_DPITCH = PK_BM + 4;                // digit rows in LDS: 16-byte aligned, staggered over the banks
constexpr int PK_ROT = 64;                          // threads (= coefficients) per workgroup of the rotation
constexpr int PK_SW = 1024;                         // threads of the switch's workgroup

// cts = the slice's ciphertexts [m][N + 1]; digits = [m][N * levels]
__global__ void __launch_bounds__(256)
    k_pack_digits(const u64 *__restrict__ cts, uint32_t *__restrict__ digits, uint32_t m, uint32_t N, uint32_t levels, uint32_t base_log) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)m * N) return;
    const uint32_t i = (uint32_t)(idx / N), j = (uint32_t)(idx % N);
    const i64 c = (i64)cts[(size_t)i * (N + 1) + j];
    const uint32_t shift = 64 - levels * base_log;   // >= 1
    i64 r = (c >> shift) + ((c >> (shift - 1)) & 1);
    const i64 B = (i64)1 << base_log, half = B >> 1;
    uint32_t *d = digits + ((size_t)i * N + j) * levels;
    for (uint32_t lev = levels - 1; lev >= 1; lev--) {
        i64 v = r & (B - 1);
        r >>= base_log;
        if (v >= half) {
            v -= B;
            r += 1;
        }
        d[lev] = (uint32_t)(v + half);
    }
    d[0] = (uint32_t)(r + half);
}

__global__ void __launch_bounds__(256)
    k_pack_product(const uint32_t *__restrict__ digits, const u64 *__restrict__ key, const u64 *__restrict__ bias,
                   const u64 *__restrict__ cts, u64 *__restrict__ T, uint32_t m, uint32_t N, uint32_t K) {
    __shared__ __attribute__((aligned(16))) uint32_t sd[PK_BK][PK_DPITCH];
    __shared__ __attribute__((aligned(16))) u64 sk[PK_BK][PK_BN];
    const uint32_t tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const uint32_t row0 = blockIdx.y * PK_BM, col0 = blockIdx.x * PK_BN;
    const size_t W = (size_t)2 * N;
    // staging roles: 4 digits of one ciphertext (16 bytes), 4 words of one key row (32 bytes)
    const uint32_t d_i = threadIdx.x >> 2, d_k = (threadIdx.x & 3) * 4;
    const uint32_t k_r = threadIdx.x >> 4, k_c = (threadIdx.x & 15) * 4;
    const bool d_live = row0 + d_i < m;
    const uint32_t *d_src = digits + (size_t)(d_live ? row0 + d_i : 0) * K + d_k;
    const u64 *k_src = key + (size_t)k_r * W + col0 + k_c;
    u64 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = 0;
    uint4 dq = d_live ? *reinterpret_cast<const uint4 *>(d_src) : make_uint4(0, 0, 0, 0);
    ulonglong2 kq0 = *reinterpret_cast<const ulonglong2 *>(k_src), kq1 = *reinterpret_cast<const ulonglong2 *>(k_src + 2);
    for (uint32_t k0 = 0; k0 < K; k0 += PK_BK) {
        __syncthreads();   // the previous stage has been multiplied
        sd[d_k + 0][d_i] = dq.x;
        sd[d_k + 1][d_i] = dq.y;
        sd[d_k + 2][d_i] = dq.z;
        sd[d_k + 3][d_i] = dq.w;
        *reinterpret_cast<ulonglong2 *>(&sk[k_r][k_c]) = kq0;
        *reinterpret_cast<ulonglong2 *>(&sk[k_r][k_c + 2]) = kq1;
        __syncthreads();
        if (k0 + PK_BK < K) {   // the next stage's words, requested under this stage's products
            if (d_live) dq = *reinterpret_cast<const uint4 *>(d_src + k0 + PK_BK);
            const u64 *nx = k_src + (size_t)(k0 + PK_BK) * W;
            kq0 = *reinterpret_cast<const ulonglong2 *>(nx);
            kq1 = *reinterpret_cast<const ulonglong2 *>(nx + 2);
        }
#pragma unroll 4   // (whole: 256 registers, one wavefront per SIMD; 4 under the default scheduler: 100)
        for (int kk = 0; kk < PK_BK; kk++) {
            const uint4 d = *reinterpret_cast<const uint4 *>(&sd[kk][ty * 4]);
            const ulonglong2 w0 = *reinterpret_cast<const ulonglong2 *>(&sk[kk][tx * 4]);
            const ulonglong2 w1 = *reinterpret_cast<const ulonglong2 *>(&sk[kk][tx * 4 + 2]);
            const uint32_t dv[4] = {d.x, d.y, d.z, d.w};
            const u64 wv[4] = {w0.x, w0.y, w1.x, w1.y};
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) acc[a][b] += (u64)dv[a] * wv[b];
        }
    }
    const uint32_t col = col0 + tx * 4;
    const ulonglong2 b0 = *reinterpret_cast<const ulonglong2 *>(bias + col), b1 = *reinterpret_cast<const ulonglong2 *>(bias + col + 2);
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const uint32_t i = row0 + ty * 4 + a;
        if (i >= m) continue;
        ulonglong2 o0, o1;
        o0.x = b0.x - acc[a][0];
        o0.y = b0.y - acc[a][1];
        o1.x = b1.x - acc[a][2];
        o1.y = b1.y - acc[a][3];
        if (col == N) o0.x += cts[(size_t)i * (N + 1) + N];   // the body b_i X^0 (column N is the first of its quad)
        u64 *dst = T + (size_t)i * W + col;
        *reinterpret_cast<ulonglong2 *>(dst) = o0;
        *reinterpret_cast<ulonglong2 *>(dst + 2) = o1;
    }
}

// T = the slice's rows [m][2N], ciphertext r of the slice is ciphertext first + r of its block; acc = [2][N]
__global__ void __launch_bounds__(PK_ROT)
    k_pack_rotate(const u64 *__restrict__ T, u64 *__restrict__ acc, uint32_t m, uint32_t first, uint32_t N, int init) {
    const uint32_t c = blockIdx.x * PK_ROT + threadIdx.x, comp = blockIdx.y;
    const size_t W = (size_t)2 * N;
    const u64 *src = T + (size_t)comp * N;
    u64 s = init ? 0 : acc[(size_t)comp * N + c];
#pragma unroll 8
    for (uint32_t r = 0; r < m; r++) {
        const uint32_t i = first + r;
        const u64 v = src[r * W + ((c - i) & (N - 1))];
        s += i <= c ? v : (u64)0 - v;
    }
    acc[(size_t)comp * N + c] = s;
}

// acc = [A: N][B: N] of one block; out = N mask values, then m body values.  PER = N / PK_SW coefficients per thread, contiguous.
template <int PER>
__global__ void __launch_bounds__(PK_SW)
    k_pack_switch(const u64 *__restrict__ acc, uint32_t *__restrict__ out, uint32_t m, uint32_t log_modulus) {
    __shared__ u64 wave_sum[PK_SW / 64];
    constexpr uint32_t N = PER * PK_SW;
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t Sh = 64 - log_modulus;
    const u64 half = (u64)1 << (Sh - 1), mask = ((u64)1 << Sh) - 1, omask = ((u64)1 << log_modulus) - 1;
    // the int64 sums of the definition are carried as u64 words (two's complement: the same bits, and wrap-around is defined);
    // only the arithmetic shift below reads one as signed
    u64 p[PER];
    u64 run = 0;
#pragma unroll
    for (int e = 0; e < PER; e++) {
        const u64 a = acc[t * PER + e];
        out[t * PER + e] = (uint32_t)(((a + half) >> Sh) & omask);
        run += ((a + half) & mask) - half;
        p[e] = run;
    }
    u64 scan = run;   // inclusive scan of the threads' totals within the wavefront ...
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 up = __shfl_up((unsigned long long)scan, off);
        if (lane >= (uint32_t)off) scan += up;
    }
    if (lane == 63) wave_sum[wave] = scan;
    __syncthreads();
    u64 before = 0, total = 0;   // ... and the wavefronts before this one
#pragma unroll
    for (int w = 0; w < PK_SW / 64; w++) {
        const u64 s = wave_sum[w];
        if ((uint32_t)w < wave) before += s;
        total += s;
    }
    const u64 base = before + scan - run;   // sum of the coefficients before this thread's
#pragma unroll
    for (int e = 0; e < PER; e++) {
        const uint32_t x = t * PER + e;
        if (x >= m) continue;
        const u64 P = base + p[e];
        const u64 b = acc[N + x] - (u64)((i64)(2 * P - total) >> 1);
        out[N + x] = (uint32_t)(((b + half) >> Sh) & omask);
    }
}

}  // namespace

namespace bmit {

uint32_t pack_slice(uint32_t N) { return (uint32_t)(((size_t)16 << 20) / ((size_t)2 * N * 8)); }

int launch_pack_slice(const u64 *cts, const u64 *key, const u64 *bias, uint32_t *digits, u64 *T, u64 *acc, uint32_t m, uint32_t first,
                      uint32_t N, uint32_t levels, uint32_t base_log, hipStream_t s) {
    if (m == 0) return 0;
    if ((N != 1024 && N != 2048 && N != 4096) || m > pack_slice(N) || first + m > N || levels == 0 || levels > 4 || base_log == 0 ||
        base_log > 16 || levels * base_log > 63)
        return (int)hipErrorInvalidValue;
    const uint32_t K = N * levels;
    hipLaunchKernelGGL(k_pack_digits, dim3((uint32_t)(((size_t)m * N + 255) / 256)), dim3(256), 0, s, cts, digits, m, N, levels, base_log);
    BMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pack_product, dim3(2 * N / PK_BN, (m + PK_BM - 1) / PK_BM), dim3(256), 0, s, digits, key, bias, cts, T, m, N, K);
    BMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pack_rotate, dim3(N / PK_ROT, 2), dim3(PK_ROT), 0, s, T, acc, m, first, N, first == 0 ? 1 : 0);
    BMI_LAUNCH_CHECK();
    return 0;
}

int launch_pack_switch(const u64 *acc, uint32_t *out, uint32_t m, uint32_t N, uint32_t log_modulus, hipStream_t s) {
    if (m == 0) return 0;
    if (m > N || log_modulus < 2 || log_modulus > 32) return (int)hipErrorInvalidValue;
    if (N == 1024) hipLaunchKernelGGL((k_pack_switch<1>), dim3(1), dim3(PK_SW), 0, s, acc, out, m, log_modulus);
    else if (N == 2048) hipLaunchKernelGGL((k_pack_switch<2>), dim3(1), dim3(PK_SW), 0, s, acc, out, m, log_modulus);
    else if (N == 4096) hipLaunchKernelGGL((k_pack_switch<4>), dim3(1), dim3(PK_SW), 0, s, acc, out, m, log_modulus);
    else return (int)hipErrorInvalidValue;
    BMI_LAUNCH_CHECK();
    return 0;
}

}  // namespace bmit
