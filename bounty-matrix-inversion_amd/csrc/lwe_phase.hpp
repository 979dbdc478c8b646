// Phase and decryption of big-key LWE ciphertexts on the device, shared by the three ciphertext moduli (policy F, as in
// ks_lincomb.hpp).  F provides, on canonical 64-bit words:
//   static u64 sub(u64, u64), mul_small(i64 coef, u64 v), reduce128(u64 hi, u64 lo);  static i64 centered(u64)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmi_internal.hpp"   // BMI_LAUNCH_CHECK

namespace lwp {

typedef uint64_t u64;
typedef int64_t i64;

// phase[i] = body - sum_x key[x] * ct[i][x] mod q for `count` ciphertexts of big_n + 1 words (big_n a multiple of 64).
// One wavefront per ciphertext, LWP_WAVES per workgroup; lane L owns the words x = L + 64 t, so a step of the wavefront reads
// 512 contiguous bytes (rows are 8-byte aligned only: the width is odd) and lane 0 takes the body.  The secret key is a bit
// mask of big_n / 64 words: word t is the same for the whole wavefront (a uniform load), bit L selects lane L's word.
// The selected words are summed exactly, as a low word and a count of carries (up to 4,096 words below 2^64), reduced
// across the lanes and passed through F::reduce128 once (the torus keeps the low word: its sum wraps).
// msgs (may be null): the message at delta_log by the host's rule (bmi_decrypt): v = centred(phase),
//   m = (v >> dl) + ((v >> (dl - 1)) & 1) with arithmetic shifts;
// err (may be null, needs msgs): centred(phase - e * 2^dl), e = expected[i] if expected is given, else m.
constexpr int LWP_WAVES = 4;

template <class F>
__global__ void __launch_bounds__(64 * LWP_WAVES)
    k_lwe_phase(const u64 *__restrict__ ct, const u64 *__restrict__ key_mask, u64 *__restrict__ phase,
                const i64 *__restrict__ expected, i64 *__restrict__ msgs, i64 *__restrict__ err, uint32_t count,
                uint32_t big_n, uint32_t delta_log) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * LWP_WAVES + (threadIdx.x >> 6);
    if (i >= count) return;   // a whole wavefront leaves: no barrier below
    const u64 *row = ct + (size_t)i * (big_n + 1);
    const uint32_t steps = big_n >> 6;
    u64 lo = 0, hi = 0;
#pragma unroll 8
    for (uint32_t t = 0; t < steps; t++) {
        const u64 v = row[lane + 64 * t];
        const u64 sel = (key_mask[t] >> lane) & 1 ? v : 0;
        lo += sel;
        hi += lo < sel;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const u64 olo = __shfl_xor(lo, off), ohi = __shfl_xor(hi, off);
        lo += olo;
        hi += ohi + (lo < olo);
    }
    if (lane != 0) return;
    const u64 ph = F::sub(row[big_n], F::reduce128(hi, lo));
    if (phase) phase[i] = ph;
    if (!msgs) return;
    const i64 v = F::centered(ph);
    const i64 m = (v >> delta_log) + ((v >> (delta_log - 1)) & 1);
    msgs[i] = m;
    if (err) err[i] = F::centered(F::sub(ph, F::mul_small(expected ? expected[i] : m, (u64)1 << delta_log)));
}

template <class F>
int launch_lwe_phase(const u64 *ct, const u64 *key_mask, u64 *phase, const i64 *expected, i64 *msgs, i64 *err,
                     uint32_t count, uint32_t big_n, uint32_t delta_log, hipStream_t s) {
    if (count == 0) return 0;
    hipLaunchKernelGGL((k_lwe_phase<F>), dim3((count + LWP_WAVES - 1) / LWP_WAVES), dim3(64 * LWP_WAVES), 0, s, ct, key_mask,
                       phase, expected, msgs, err, count, big_n, delta_log);
    BMI_LAUNCH_CHECK();
    return 0;
}

}  // namespace lwp
