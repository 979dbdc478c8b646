// The steps the N = 1024 half-transform torus blind rotations state the same way (gfx950): k_blind_rotate_lat_t64f (plain key,
// bmi_kernels_t64f.hip), k_blind_rotate_lat2u_t64f and k_blind_rotate_tp2u_t64f (unrolled key, one and two ciphertexts per
// workgroup, bmi_kernels_t64fu.hip), and the key conversion all three read, k_bsk_to_latf_t64.  Built like t64_wide_steps.hpp, by
// the same rules: force-inlined functions on the caller's compile-time constants, no state, no barrier, pin() or phase mark (where
// a step stands relative to those distinguishes the kernels and stays in their step loops, as do the LDS maps); phase B helpers
// take tile and table words as VALUES the caller has read from its `extern __shared__` array.  A step is here if at least two of
// the four kernels call it with their machine code unchanged, instruction for instruction (tools/isa_diff.py; the record is
// profiles/half_steps_ab.txt); a kernel whose schedule or register numbering a helper changes keeps the step written out and says
// so in one line.  Four steps stay written out in every kernel and are not here: the start accumulator, the accumulator's digits,
// the tile store behind a forward half, and the inverse half with its atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "bmi_internal.hpp"
#include "fft_half_f64.hpp"
#include "t64_common.hpp"

namespace t64h {

using ffth::C;
using fftw::static_for;
using t64::mod_ab;

// ---- the family's constants and the accumulator's layout ----
constexpr int HN = ffth::N, HLOG = 10;
constexpr int H_THREADS = 1024;        // 16 wavefronts
constexpr int H_MAX_L = 3;
constexpr int H_HALF = HN / 2;         // accumulator words per parity; complex words of a row's two half tiles
constexpr int H_RECENTRE = 8;          // steps between reductions of the accumulator mod 2^AB
// accumulator words are kept split by parity (a lane's four points are 128 coefficients apart and of one parity)
constexpr t64::ResidueSlot<HN, 1> acc_slot{};
// keeps the magnitude of BLOCKS x 1,024 accumulator words (2: one ciphertext, 4: two) below 2^51
template <int AB, int BLOCKS>
__device__ __forceinline__ void recentre(double *acc, int tid) {
    static_for<0, BLOCKS>([&](auto Q) { acc[tid + H_THREADS * Q] = mod_ab<AB>(acc[tid + H_THREADS * Q]); });
}
// the forward half of the wavefront's parity h
__device__ __forceinline__ void forward_half_of(int h, const double (&re)[4], const double (&im)[4], C (&v)[4], int lane, const double *lds) {
    if (h) ffth::forward_half<1>(re, im, v, lane, lds);
    else ffth::forward_half<0>(re, im, v, lane, lds);
}

// ---- phase B: thread = (limb mj, output polynomial mo, slot mq) ----
// A row's transform at the slot's two frequencies is E + O' (F_k) and E - O' (F_{k+256}), e and od the slot's words of the row's
// two half tiles: ylo += (E + O') klo, yhi += (E - O') khi, klo / khi this thread's key words of the row.
__device__ __forceinline__ void mac_pair(C &ylo, C &yhi, const double2 e, const double2 od, const double2 klo, const double2 khi) {
    const double lr = e.x + od.x, li = e.y + od.y, hr = e.x - od.x, hi = e.y - od.y;
    ylo.r = __builtin_fma(lr, klo.x, __builtin_fma(-li, klo.y, ylo.r));
    ylo.i = __builtin_fma(lr, klo.y, __builtin_fma(li, klo.x, ylo.i));
    yhi.r = __builtin_fma(hr, khi.x, __builtin_fma(-hi, khi.y, yhi.r));
    yhi.i = __builtin_fma(hr, khi.y, __builtin_fma(hi, khi.x, yhi.i));
}
// what the inverse halves start from: the sum slo + shi and the twisted difference (slo - shi) conj w, w = the slot's word of
// the table HT_W, into sd = [S, D][256 slots] of the thread's (limb, output)
__device__ __forceinline__ void sum_diff_store(double2 *sd, int mq, const C &slo, const C &shi, const double2 w) {
    const C d = ffth::cmul<true>(C{slo.r - shi.r, slo.i - shi.i}, w.x, w.y);
    sd[mq] = double2{slo.r + shi.r, slo.i + shi.i};
    sd[H_HALF / 2 + mq] = double2{d.r, d.i};
}

// ---- the unrolled key: [pair][key 3][row 2L][output 2][limb][256 slots][F_k, F_{k+256}], read in chunks of L rows (half a key) ----
// the pair's exponents c = (a + a', a, a') of the three keys (an odd n is completed by a' = 0: at[n] is the body)
__device__ __forceinline__ void pair_exponents(uint32_t (&cj)[3], const uint16_t *at, uint32_t ip, uint32_t n) {
    const uint32_t a1 = at[2 * ip], a2 = (2 * ip + 1 < n) ? at[2 * ip + 1] : 0u;
    cj[0] = (a1 + a2) & (2 * HN - 1);
    cj[1] = a1;
    cj[2] = a2;
}
// this thread's words of chunk t = (key t / 2, rows (t & 1) L .. + L) of pair ip, and their request (2 CH double2)
template <int L, int LIMBS>
__device__ __forceinline__ const double2 *chunk_ptr(const double *bsk3_latf, uint32_t ip, int t, int mo, int mj, int mq) {
    const int key = t >> 1, r0 = (t & 1) * L;
    return reinterpret_cast<const double2 *>(bsk3_latf + (((size_t)ip * 3 + key) * 2 * L + r0) * 2 * LIMBS * HN) +
           ((size_t)mo * LIMBS + mj) * (HN / 2) + 2 * mq;
}
template <int CH, int LIMBS>
__device__ __forceinline__ void request(double2 (&dst)[CH][2], const double2 *p) {
    static_for<0, CH>([&](auto R) {
        dst[R][0] = p[(size_t)R * 2 * LIMBS * (HN / 2)];
        dst[R][1] = p[(size_t)R * 2 * LIMBS * (HN / 2) + 1];
    });
}
// a complete key's sums scaled by X^c - 1 at the slot's two roots and added: w = zeta^((4k+1) c) for F_k (each kernel's own table
// look-up), its negative (c odd) for F_{k+256}; the key's sums start over
__device__ __forceinline__ void scale_add(C &slo, C &shi, C &ylo, C &yhi, const double2 w, uint32_t c) {
    const double wlr = w.x - 1.0, wli = w.y;
    const double whr = ((c & 1) ? -w.x : w.x) - 1.0, whi = (c & 1) ? -w.y : w.y;
    slo.r += __builtin_fma(ylo.r, wlr, -(ylo.i * wli));
    slo.i += __builtin_fma(ylo.r, wli, ylo.i * wlr);
    shi.r += __builtin_fma(yhi.r, whr, -(yhi.i * whi));
    shi.i += __builtin_fma(yhi.r, whi, yhi.i * whr);
    ylo = yhi = C{0.0, 0.0};
}

// an inverse task's 256 sums (h = 0) or twisted differences (h = 1)
__device__ __forceinline__ void read_sums(C (&v)[4], const double2 *sd, int lane) {
    static_for<0, 4>([&](auto R) {
        const double2 t = sd[R * 64 + lane];
        v[R] = C{t.x, t.y};
    });
}

}  // namespace t64h
