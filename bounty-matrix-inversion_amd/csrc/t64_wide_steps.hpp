// The steps the four N = 2048 torus blind rotations state the same way (gfx950):
//
//   k_blind_rotate_w_t64f    bmi_kernels_t64w.hip    plain key,    one ciphertext per workgroup
//   k_blind_rotate_w2_t64f   bmi_kernels_t64w2.hip   plain key,    two ciphertexts per workgroup
//   k_blind_rotate_wu_t64f   bmi_kernels_t64wu.hip   unrolled key, one ciphertext per workgroup
//   k_blind_rotate_wu2_t64f  bmi_kernels_t64wu2.hip  unrolled key, two ciphertexts per workgroup
//
// and the two key conversions k_bsk_to_w_t64, k_bsk_to_w2_t64.  Force-inlined functions on the caller's compile-time constants,
// no state.  What distinguishes the kernels - the LDS map, the step loop with its barriers, its pin()s and its phase marks, the
// key prefetch schedule - is in the kernel files: no helper here holds a barrier, a pin() or a PH_MARK.  Helpers of phase B take
// table and tile words as VALUES, read by the caller from its `extern __shared__` array: read through a pointer handed to a
// helper, the same two words come as one ds_read_b128 instead of ds_read2_b64 (the alignment the compiler knows differs).
//
// The rule for what is here: a step at least two of the kernels can call with their machine code unchanged, instruction for
// instruction (tools/isa_diff.py against the written-out text; the record is profiles/wide_steps_ab.txt).  A force-inlined helper
// is inlined before the optimizer runs, a lambda body after: where that order changes the schedule or the register numbering of a
// kernel, the kernel keeps the step written out and says so in one line.  Steps every kernel keeps written out for that reason
// (the forward task's quarter transform and tile store, the epilogue) are not here.
#pragma once
#include <hip/hip_runtime.h>

#include "bmi_internal.hpp"
#include "fft_quarter_f64.hpp"
#include "lane_transpose.hpp"
#include "t64_common.hpp"

namespace t64w {

using fftq::C;
using fftq::static_for;
using t64::i64;
using t64::mod_ab;
using t64::u64;

// ---- the family's constants and the accumulator's layout ----
constexpr int WN = 2048, WLOG = 11;
constexpr int WQ = fftq::QUARTER;      // complex points (= slots) of a quarter transform
constexpr int W_THREADS = 1024;        // 16 wavefronts
constexpr int W_MAX_L = 3;
constexpr int W_RECENTRE = 8;          // steps between reductions of the accumulator mod 2^AB
constexpr int W_RES = WN / 4;          // accumulator words per residue class mod 4
constexpr int W_ZO = WN / 4;           // the unrolled kernels' octant: zeta^x for x in [0, W_ZO], zeta = exp(i pi / 2048)
constexpr int W_ZO_WORDS = 2 * (W_ZO + 1);
// accumulator words are kept split by residue mod 4 (a lane's points of a quarter are 256 coefficients apart and of one residue):
// a polynomial is [4 residues][512], an accumulator [2 components] of those
constexpr t64::ResidueSlot<WN, 2> acc_slot{};

// ---- key conversion, first half ----
// Limb j of the words of standard-domain polynomial `poly` that quarter h's lane holds -> forward quarter -> tile [h][256 slots].
// The callers combine the four quarters (radix 4) after a barrier, each into its own order of the key copy.
__device__ __forceinline__ void key_limb_to_tile(double2 *tile, const u64 *std_polys, uint32_t poly, int j, int prec, int h, int lane, const double *lds) {
    double re[4], im[4];
    static_for<0, 4>([&](auto R) {
        const uint32_t m = 4 * (lane + 64 * R) + h;
        re[R] = (double)t64::limb_of((i64)std_polys[(size_t)poly * WN + m], j, prec);
        im[R] = (double)t64::limb_of((i64)std_polys[(size_t)poly * WN + m + WN / 2], j, prec);
    });
    C v[4];
    fftq::forward_quarter(h, re, im, v, lane, lds);
    static_for<0, 4>([&](auto R) { tile[h * WQ + R * 64 + lane] = double2{v[R].r, v[R].i}; });
}

// ---- forward task of the plain step: digits `lev` of X^a ACC - ACC ----
// Quarter h's lane holds the coefficients m_J = 4 (lane + 64 (J & 3)) + h + 1024 (J >> 2), J = 0 .. 7, of polynomial `ac`; x[J] is
// re[J] of the quarter transform for J < 4, im[J - 4] above.  This is the group J = 4 G .. 4 G + 3: the callers fence the two
// groups with pin() (with the key registers in flight all eight at once do not fit).  The rotated source of m_J is
// e_J = m_J - a_t mod 2N: a quarter of it is t0 + 64 (J & 3) + 256 (J >> 2) - the low 9 bits are the slot inside the residue
// block, bit 9 is the sign.
template <int L, int BG, int AB, int G>
__device__ __forceinline__ void rotated_diff_digits(double (&x)[8], const double *ac, int h, int lane, uint32_t a_t, int lev) {
    const uint32_t e0 = (4 * lane + h + 2 * WN - a_t) & (2 * WN - 1);
    const uint32_t t0 = e0 >> 2, pbase = (e0 & 3) * W_RES;
    double vr[4], vs[4];
    static_for<0, 4>([&](auto J4) {
        constexpr int J = G * 4 + J4;
        const uint32_t t = t0 + 64 * (J & 3) + 256 * (J >> 2);
        vr[J4] = ac[pbase + (t & (W_RES - 1))];
        vs[J4] = ac[h * W_RES + lane + 64 * (J & 3) + 256 * (J >> 2)];
    });
    static_for<0, 4>([&](auto J4) {
        constexpr int J = G * 4 + J4;
        const uint32_t t = t0 + 64 * (J & 3) + 256 * (J >> 2);
        const double dd = mod_ab<AB>(((t >> 9) & 1) ? -vr[J4] - vs[J4] : vr[J4] - vs[J4]);   // the centred lift of the u64 difference, / 2^PRE
        x[J] = t64::digit<L, BG, AB>(dd, lev);
    });
}

// ---- phase B by lane pairs: thread = (output polynomial mo, slot mq = 32 w8 + (lane & 31), tp = lane >> 5) ----
// A pair of lanes 32 apart shares a slot.  Lane tp reads quarters tp (`lo`) and tp + 2 (`hi`) of a row's tiles, half a radix-4
// butterfly each -  tp = 0: (q0 + q2, q0 - q2);  tp = 1: (q1 + q3, i (q1 - q3))  - and ONE 2 x 2 transpose on lane bit 5
// (v_permlane32_swap) completes it -  tp = 0: (a, cc),  tp = 1: (b, d)  - : the row's transform at the thread's two frequencies
// a0 = A_{kappa + 256 tp}, a1 = A_{kappa + 256 (tp + 2)}.
__device__ __forceinline__ void forward_half_butterfly(const double2 lo, const double2 hi, int tp, int lane, C &a0, C &a1) {
    C u{lo.x + hi.x, lo.y + hi.y};
    const C dl{lo.x - hi.x, lo.y - hi.y};
    C w{tp ? -dl.i : dl.r, tp ? dl.r : dl.i};   // tp ? i dl : dl, a select per part (as one of the pair the four selects come in another order)
    lanetr::tr_double<5>(u.r, w.r, lane);
    lanetr::tr_double<5>(u.i, w.i, lane);
    a0 = u + w;
    a1 = u - w;
}
// y[f] += a_f k[f] at the two frequencies, k one limb's words of a key row (request_row below)
__device__ __forceinline__ void cmac2(C (&y)[2], const C &a0, const C &a1, const double2 (&k)[2]) {
    const double2 k0 = k[0], k1 = k[1];
    y[0].r = __builtin_fma(a0.r, k0.x, __builtin_fma(-a0.i, k0.y, y[0].r));
    y[0].i = __builtin_fma(a0.r, k0.y, __builtin_fma(a0.i, k0.x, y[0].i));
    y[1].r = __builtin_fma(a1.r, k1.x, __builtin_fma(-a1.i, k1.y, y[1].r));
    y[1].i = __builtin_fma(a1.r, k1.y, __builtin_fma(a1.i, k1.x, y[1].i));
}
// The inverse butterfly the same way back -  tp = 0: (Y0 + Y2, Y0 - Y2);  tp = 1: (Y1 + Y3, -i (Y1 - Y3));  transpose;
// S_tp = u + w, S_{tp+2} = u - w  - times conj W_h: s_lo = S_tp conj W_tp, s_hi = S_{tp+2} conj W_{tp+2} at slot mq.  The caller
// reads wl and wh, once per step, at the double2 indices below: branch-free - a conditional read would split the block and let
// the compiler sink every product below it; W_0 = 1 is the first word of the omega_64 table.
__device__ __forceinline__ int conj_w_lo_index(int tp, int mq) { return tp ? fftq::QT_W1 / 2 + mq : ffth::HT_T2 / 2; }
__device__ __forceinline__ int conj_w_hi_index(int tp, int mq) { return (tp ? fftq::QT_W3 : fftq::QT_W2) / 2 + mq; }
__device__ __forceinline__ void inverse_half_butterfly(const C y0, const C y1, int tp, int lane, const double2 wl, const double2 wh, C &s_lo, C &s_hi) {
    C u = y0 + y1;
    const C dl = y0 - y1;
    C w = tp ? C{dl.i, -dl.r} : dl;
    lanetr::tr_double<5>(u.r, w.r, lane);
    lanetr::tr_double<5>(u.i, w.i, lane);
    s_lo = fftq::cmul<true>(u + w, wl.x, wl.y);
    s_hi = fftq::cmul<true>(u - w, wh.x, wh.y);
}
// s_lo, s_hi of one (limb, output) -> the thread's slot of the sums' tile, sd = [4 quarters][256 slots] + mq (over the forward tiles)
__device__ __forceinline__ void store_sums(double2 *sd, int tp, const C &s_lo, const C &s_hi) {
    sd[tp * WQ] = double2{s_lo.r, s_lo.i};
    sd[(tp + 2) * WQ] = double2{s_hi.r, s_hi.i};
}

// ---- key rows of the per-polynomial key copy (launch_bsk_to_wide): [step][row ROWS][output 2][limb][f 2][64 w8 + lane] ----
// complex words, f the thread's two frequencies: a wavefront's request is 1 KiB contiguous.  ROWS = 2 L, of the unrolled key 3 x 2 L.
template <int ROWS, int LIMBS>
__device__ __forceinline__ const double2 *key_ptr(const double *bsk, uint32_t step, int mo, int w8, int lane) {
    return reinterpret_cast<const double2 *>(bsk + (size_t)step * ROWS * 2 * LIMBS * WN) + (size_t)mo * LIMBS * (WN / 2) + (w8 * 64 + lane);
}
template <int LIMBS>
__device__ __forceinline__ void request_row(double2 (&dst)[LIMBS][2], const double2 *kth, const int row) {
    static_for<0, LIMBS>([&](auto J) {
        dst[J][0] = kth[((size_t)row * 2 * LIMBS + J) * (WN / 2)];
        dst[J][1] = kth[((size_t)row * 2 * LIMBS + J) * (WN / 2) + WN / 4];
    });
}

// ---- the unrolled key's powers of zeta ----
// zeta^x, x in [0, 4096), from the octant ZO = zeta^[0, 512]: r = x mod 1024 folded at 512 (zeta^(1024 - r) = i conj(zeta^r): real
// and imaginary parts swapped), the quadrant a multiplication by i^q.  The symmetries are exact: every factor is ONE table entry.
__device__ __forceinline__ double2 zeta_pow(const double2 *ZO, uint32_t x) {
    const uint32_t r = x & 1023, fold = r > (uint32_t)W_ZO;
    const double2 w = ZO[fold ? 1024 - r : r];
    const double cr = fold ? w.y : w.x, ci = fold ? w.x : w.y;
    const uint32_t quad = (x >> 10) & 3;
    const double sr = (quad & 1) ? -ci : cr, si = (quad & 1) ? cr : ci;         // times i for odd quadrants
    return double2{(quad & 2) ? -sr : sr, (quad & 2) ? -si : si};               // times -1 for quadrants 2, 3
}

// ---- inverse task, one limb j per pass (the two-ciphertext kernels: all 16 wavefronts run a task per limb) ----
// v = that limb's sums of (output, quarter h), already times conj W_h -> inverse quarter -> nearest integers, limb 1 shifted into
// place -> a plain read-modify-write of the wavefront's 512 coefficients of accumulator polynomial `poly`
template <int AB, int LB, bool STATS>
__device__ __forceinline__ void inverse_task_limb(double *poly, int h, C (&v)[4], int j, int lane, const double *lds, double &dev) {
    double re[4], im[4];
    fftq::inverse_quarter(v, re, im, lane, lds);
    double *ao = poly + h * W_RES + lane;
    static_for<0, 4>([&](auto R) {
        ao[64 * R] += t64::place_limb<AB, LB, STATS>(re[R], j, dev);              // coefficient 4 (lane + 64 R) + h
        ao[64 * R + 256] += t64::place_limb<AB, LB, STATS>(im[R], j, dev);        // ... + 1024
    });
}

// ---- prologue and re-centring (the barriers between them are the kernels') ----
// the start accumulator (0, X^bt tv) of ciphertext ct, bt = at[n] its mod-switched body
template <int PRE>
__device__ __forceinline__ void load_start_acc(double *acc, const u64 *luts, const uint32_t *lut_ids, uint32_t ct, const uint16_t *at, uint32_t n, int tid) {
    const u64 *tv = luts + (size_t)(lut_ids[ct] & (BMI_LUT_CAP - 1)) * WN;
    const uint32_t bt = at[n];
    static_for<0, 2>([&](auto Q) { t64::load_test_poly<WN, PRE>(acc, acc_slot, tv, bt, tid + W_THREADS * Q); });
}
// keeps the magnitude of BLOCKS x 1,024 accumulator words (4: one ciphertext, 8: two) below 2^51
template <int AB, int BLOCKS>
__device__ __forceinline__ void recentre(double *acc, int tid) {
    static_for<0, BLOCKS>([&](auto Q) { acc[tid + W_THREADS * Q] = mod_ab<AB>(acc[tid + W_THREADS * Q]); });
}
// the two ciphertexts cts[] of workgroup `wg` (an odd batch: the last workgroup runs its one ciphertext twice and writes it once);
// returns whether the second is live
__device__ __forceinline__ bool ciphertext_pair(uint32_t (&cts)[2], uint32_t wg, uint32_t count) {
    const uint32_t ct0 = wg * 2;
    const bool live1 = ct0 + 1 < count;
    cts[0] = ct0;
    cts[1] = live1 ? ct0 + 1 : ct0;
    return live1;
}

// ---- an empty statement that reads and writes every element of an array of sums ----
// They must be in registers there: the branches of the next level's forward task would otherwise let the compiler sink the
// multiply-adds of all levels below them, their operands waiting in scratch (1.4 - 1.6 KB per lane in the unrolled kernel).
__device__ __forceinline__ void keep(C &c) { asm volatile("" : "+v"(c.r), "+v"(c.i)); }
template <typename T, int K>
__device__ __forceinline__ void keep(T (&a)[K]) {
#pragma unroll
    for (int k = 0; k < K; k++) keep(a[k]);
}

}  // namespace t64w
