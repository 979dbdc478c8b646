// Decompression of compressed ciphertexts back to big-key LWE ciphertexts (2^64 torus, k = 1): the inverse direction of lwe_pack.hip,
// and it needs no key.  The packing key encrypts under the context's own GLWE key and the centred switch has folded its mean
// correction into the body values, so position i of a block is recovered by the negacyclic sample extraction of coefficient i, shifted
// back up from log_modulus bits to 2^64 (include/bmi_tfhe.h states the rule, tests/decompress_cases.py restates it in numpy):
//   with Sh = 64 - log_modulus, i = idx[r] mod N and A^ / B^ the mask and body values of block idx[r] / N (taken mod 2^log_modulus),
//   out[r][j] = A^[i - j] << Sh for j <= i,   0 - (A^[N + i - j] << Sh) for i < j < N,   out[r][N] = B^[i] << Sh.
// The LWE phase of out[r] under sk_big is bit for bit what bmi_phase_compressed gives for position idx[r].
//
// Pure data movement: rows * (N + 1) * 8 bytes written, and per block at most 4N bytes of mask values read over and over (they
// stay in the caches).  The kernel is therefore laid out over the OUTPUT: the rows have a pitch of N + 1 words and start on 8-byte
// boundaries only, so a thread owns one 16-byte ALIGNED pair of the flat word sequence out[0 .. rows * (N + 1)), whichever rows the
// two words belong to, and a wavefront stores 1 KiB of consecutive bytes with one instruction.  Where the base itself sits on an odd
// 8-byte boundary (head = 1) the pairs start one word earlier: the first pair then holds word 0 alone, and whichever pair reaches
// rows * (N + 1) holds its first word alone; those two are 8-byte stores.  Every word is written exactly once and nothing outside.
#include <hip/hip_runtime.h>

#include "bmi_internal.hpp"

namespace {

using bmi::u64;

constexpr uint32_t UP_THREADS = 256;

// word j of output row r
template <uint32_t N>
__device__ __forceinline__ u64 unpack_word(const uint32_t *__restrict__ in, const uint32_t *__restrict__ index, uint32_t r, uint32_t j,
                                           uint32_t Sh, uint32_t omask) {
    const uint32_t idx = index ? index[r] : r;
    const uint32_t *blk = in + (size_t)(idx / N) * 2 * N;   // a block before the last is full: N mask and N body values
    const uint32_t i = idx & (N - 1);
    const uint32_t v = (j == N ? blk[N + i] : blk[(i - j) & (N - 1)]) & omask;
    const u64 x = (u64)v << Sh;
    return j > i && j < N ? (u64)0 - x : x;
}

// total = rows * (N + 1) words; head = 1 where out sits on an odd 8-byte boundary.  Thread p of the grid owns the words
// 2 p - head and 2 p + 1 - head.
template <uint32_t N>
__global__ void __launch_bounds__(UP_THREADS)
    k_unpack(const uint32_t *__restrict__ in, const uint32_t *__restrict__ index, u64 *__restrict__ out, u64 total, uint32_t head,
             uint32_t log_modulus) {
    constexpr uint32_t W = N + 1;
    const uint32_t Sh = 64 - log_modulus, omask = 0xFFFFFFFFu >> (32 - log_modulus);
    // the workgroup's first word -> (row, word in row) once, by a 64-bit division; the thread's own offset by a 32-bit one
    const u64 wb = (u64)blockIdx.x * (2 * UP_THREADS);
    const uint32_t rb = (uint32_t)(wb / W), jb = (uint32_t)(wb % W);
    const u64 w1 = wb + 2 * threadIdx.x + 1 - head;   // the pair's second word; the first is w1 - 1 (which word 0 of head = 1 lacks)
    if (w1 > total) return;
    const uint32_t t1 = jb + 2 * threadIdx.x + 1 - head;
    const uint32_t r1 = rb + t1 / W, j1 = t1 % W;
    const bool has0 = w1 >= 1, has1 = w1 < total;
    u64 v0 = 0, v1 = 0;
    if (has0) v0 = j1 ? unpack_word<N>(in, index, r1, j1 - 1, Sh, omask) : unpack_word<N>(in, index, r1 - 1, N, Sh, omask);
    if (has1) v1 = unpack_word<N>(in, index, r1, j1, Sh, omask);
    if (has0 && has1) {
        ulonglong2 q;
        q.x = v0;
        q.y = v1;
        *reinterpret_cast<ulonglong2 *>(out + (w1 - 1)) = q;
    } else if (has0) {
        out[w1 - 1] = v0;
    } else if (has1) {
        out[w1] = v1;
    }
}

}  // namespace

namespace bmit {

int launch_unpack(const uint32_t *in, const uint32_t *index, u64 *out, uint32_t count, uint32_t rows, uint32_t N, uint32_t log_modulus,
                  hipStream_t s) {
    if (rows == 0) return 0;
    if (count == 0 || log_modulus < 2 || log_modulus > 32 || (!index && rows != count) || ((uintptr_t)out & 7)) return (int)hipErrorInvalidValue;
    const u64 total = (u64)rows * (N + 1);
    const uint32_t head = (uint32_t)(((uintptr_t)out >> 3) & 1);
    const u64 pairs = (total - 1 + head) / 2 + 1, groups = (pairs + UP_THREADS - 1) / UP_THREADS;
    if (groups > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    const dim3 grid((uint32_t)groups), block(UP_THREADS);
    if (N == 1024) hipLaunchKernelGGL((k_unpack<1024>), grid, block, 0, s, in, index, out, total, head, log_modulus);
    else if (N == 2048) hipLaunchKernelGGL((k_unpack<2048>), grid, block, 0, s, in, index, out, total, head, log_modulus);
    else if (N == 4096) hipLaunchKernelGGL((k_unpack<4096>), grid, block, 0, s, in, index, out, total, head, log_modulus);
    else return (int)hipErrorInvalidValue;
    BMI_LAUNCH_CHECK();
    return 0;
}

}  // namespace bmit
