// Centred modulus switch (TFHE-rs' "centred mean" variant): halves the variance of the rounding that takes the n mask words of a
// small-key ciphertext to the 2N positions of the circle, without key material and without touching a rotation kernel.
//
// The rotation kernels round every word of a small ciphertext (a_0 .. a_{n-1}, b) by themselves (t64::modswitch resp.
// f49::modswitch).  With e_i the rounding error of mask word i and e_b that of the body, the switched phase is off by
//      sum_i s_i e_i - e_b  =  sum_i e_i / 2  +  sum_i (s_i - 1/2) e_i  -  e_b            (binary key s).
// The first sum is public: this kernel subtracts it from the BODY, before the body is rounded.  What remains has the variance
// sum e_i^2 / 4 ~ n / 48 positions^2 whatever the key's weight, against hw(s) / 12 ~ n / 24 of the standard switch.
//
// Exact integer definitions (restated in tests/test_centred_modswitch_model.py):
//   2^64 torus, L = log2(2N), S = 64 - L:   e_i = ((a_i + 2^(S-1)) mod 2^S) - 2^(S-1)   in [-2^(S-1), 2^(S-1)),
//       T = sum_{i<n} e_i  (int64; |T| <= n 2^(S-1) <= 2^62 for n <= 1024, N >= 1024),   b' = b - (T >> 1) mod 2^64;
//   49-bit field, q = 2^49 - 720895:   A_i = floor((a_i 2N + (q >> 1)) / q) (f49::modswitch before its mask),
//       E_i = a_i 2N - A_i q,   T = sum E_i  (|T| < 2^59),   b' = (b - floor(T / 4N)) mod q.
//
// k_modswitch_centre: one wavefront per ciphertext, MSC_WAVES per workgroup.  Lane l owns the mask words l + 64 t (a step of the
// wavefront reads 512 contiguous bytes; rows are 8-byte aligned only: n + 1 is odd for the shipped n), keeps an int64 partial
// sum, the lanes are reduced with __shfl_xor and lane 0 writes the body.  Where out is another buffer than in, the mask words
// are copied unchanged.  No LDS, no atomics; a wavefront past `count` does nothing.
#include <hip/hip_runtime.h>

#include "bmi_internal.hpp"
#include "field49.hpp"

namespace {

using bmi::i64;
using bmi::u64;

constexpr int MSC_WAVES = 4;

// in and out may be the same buffer: no __restrict__
template <bool TORUS>
__global__ void __launch_bounds__(64 * MSC_WAVES)
    k_modswitch_centre(const u64 *in, u64 *out, uint32_t count, uint32_t n, uint32_t log_2N) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.x * MSC_WAVES + (threadIdx.x >> 6);
    if (c >= count) return;   // a whole wavefront leaves: no barrier below
    const u64 *src = in + (size_t)c * (n + 1);
    u64 *dst = out + (size_t)c * (n + 1);
    const bool copy = dst != src;
    const uint32_t S = 64 - log_2N;
    const u64 half = (u64)1 << (S - 1), mask = ((u64)1 << S) - 1;
    i64 t = 0;
    for (uint32_t i = lane; i < n; i += 64) {
        const u64 a = src[i];
        if (TORUS) {
            t += (i64)((a + half) & mask) - (i64)half;
        } else {
            const u64 scaled = a << log_2N;   // a < 2^49, log_2N <= 13: no overflow
            t += (i64)scaled - (i64)(((scaled + (f49::Q >> 1)) / f49::Q) * f49::Q);
        }
        if (copy) dst[i] = a;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off);
    if (lane != 0) return;
    const u64 b = src[n];
    if (TORUS) {
        dst[n] = b - (u64)(t >> 1);
    } else {
        const i64 d = t >> (log_2N + 1);   // floor(T / 4N), |d| < 2^47 < q
        const u64 bq = b % f49::Q;
        dst[n] = d >= 0 ? f49::subq(bq, (u64)d) : f49::addq(bq, (u64)(-d));
    }
}

}  // namespace

namespace bmi {

int launch_modswitch_centre(const u64 *in, u64 *out, uint32_t count, uint32_t n, uint32_t log_N, bool torus, hipStream_t s) {
    if (count == 0) return 0;
    if (n == 0 || n > BMI_MAX_LWE_N || log_N < 10 || log_N > 12) return (int)hipErrorInvalidValue;
    const dim3 grid((count + MSC_WAVES - 1) / MSC_WAVES), block(64 * MSC_WAVES);
    if (torus) hipLaunchKernelGGL((k_modswitch_centre<true>), grid, block, 0, s, in, out, count, n, log_N + 1);
    else hipLaunchKernelGGL((k_modswitch_centre<false>), grid, block, 0, s, in, out, count, n, log_N + 1);
    BMI_LAUNCH_CHECK();
    return 0;
}

}  // namespace bmi
