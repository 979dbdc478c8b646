// 2^64 TORUS at N = 2048 (the secure128_torus set: n 742, k 1, l 3, Bg 2^10), UNROLLED blind rotation (two LWE coefficients per
// step) with the exact limb products carried by the floating-point transform of fft_quarter_f64.hpp (gfx950): the structure of
// bmi_kernels_t64w.hip (one workgroup of 16 wavefronts per ciphertext, quarter transforms, phase B by lane pairs 32 apart, both
// limbs in the inverse tasks, plain read-modify-write of the f64 accumulator) running the step of bmi_kernels_t64fu.hip
// (oracle/tfhe_oracle.c ora_blind_rotate_extract_unrolled):
//
//     ACC <- ACC + sum_{j<3} (X^(c_j) - 1) (K3[i][j] [.] ACC),   c = (a + a', a, a'),
//     K3[i] = GGSW(s s'), GGSW(s (1 - s')), GGSW((1 - s) s')   of the key bits (s, s') = (s_2i, s_2i+1),
//
// one decomposition of ACC itself and one set of forward transforms per PAIR of coefficients, three GGSW products scaled by
// X^c - 1 in the transform domain: X^c at the root zeta^(4k+1) of frequency k is zeta^((4k+1) c), zeta = exp(i pi / 2048).
//
// Exactness.  A limb's inverse transform returns  sum_j (X^(c_j) - 1) sum_rows digit x limb : three keys, each scaled by a factor
// of magnitude <= 2 - six times the plain step's sum.  The unrolled key is therefore stored at 40 bits of precision (two balanced
// 20-bit limbs, words rounded to multiples of 2^24; the rounded key IS the key: exported, given to the oracle):
// |sum| < 6 * 2 l N 2^9 2^19 = 2^44.2 < 2^45, and the a-priori bound of the transform's error is 0.38 < 1/2
// (tools/fft_bound.py unrolled_limb_sum_bound: six times fft_quarter_f64.hpp's formula for a plain limb sum, 0.052 x 6 = 0.31,
// with the scaling by zeta^(..c) - 1 counted as a multiplication stage of its own, n = 12, and its factor's error - a table
// entry minus one - as beta = 1.5 e), so the nearest integer of the inverse transform is the exact sum and the words equal the
// oracle's integer arithmetic on the same key (tests/test_gpu_torus_wide_unrolled.py).  21-bit limbs would give 0.76 (0.62
// before the scaling stage is counted): not certified, hence 40 bits and not 42.
//
// The powers of zeta.  A full table of 2,048 complex powers is 32 KB and does not fit beside the tiles (the plain kernel uses 151
// of the 160 KB).  The kernel keeps ONE OCTANT, zeta^x for x in [0, 512] (513 complex words, 8 KB + one entry), in LDS and folds
// the exponent by the table's symmetries: zeta^(1024 - x) = i conj(zeta^x) (real and imaginary parts swapped), zeta^(x + 1024) =
// i zeta^x.  The symmetries are exact, so every factor is a table entry rounded once from long double - no product of two
// entries, nothing added to the `beta` of the bound.
//
// Per step (a pair with a = a' = 0 is skipped, uniformly over the workgroup; an odd n is completed by a' = 0):
//   A  8 l forward tasks (input polynomial c, level, quarter h) over the 16 wavefronts: decompose 512 coefficients of the
//      accumulator itself (no rotation), forward quarter -> tile (slot order, times W_h)
//   B  all 1,024 threads = (output polynomial o, slot, tp), lanes 32 apart sharing a slot as in the plain kernel: for each of the
//      three keys the 2 l rows' radix-4 butterfly (one 2 x 2 transpose on lane bit 5, v_permlane32_swap) and multiply-accumulates
//      with both limbs' key words at the two frequencies kappa + 256 tp and kappa + 256 (tp + 2); the key's sums scaled by
//      zeta^((4k+1) c_j) - 1 at those frequencies (the second is the first times (-1)^c) and added; the 6 l key rows of a step
//      are one contiguous run, requested BMI_T64WU_KEY_ROWS_AHEAD rows ahead (the first during the step before); then the
//      inverse butterfly, times conj W_h -> the sums S_h (over the tiles, after a barrier)
//   C  8 inverse tasks (o, quarter) on wavefronts 8 .. 15: the inverse quarters of both limbs, nearest integers, limb 1 shifted
//      into place, one plain read-modify-write per coefficient of the accumulator; re-centred mod 2^40 every 8 steps taken
#include <hip/hip_runtime.h>

#include "bmi_internal.hpp"
#include "fft_quarter_f64.hpp"
#include "pair_sync.hpp"
#include "t64_common.hpp"
#include "t64_wide_steps.hpp"

using t64::i64;
using t64::u64;

namespace {

using namespace t64w;   // the N = 2048 family's constants (WN, WQ, W_*) and shared steps: t64_wide_steps.hpp
using t64::Scheme;

#ifndef BMI_T64WU_KEY_ROWS_AHEAD
#define BMI_T64WU_KEY_ROWS_AHEAD 2   // key rows (of the 6 l of a step) a thread holds in registers
#endif
constexpr int WU_TILE_CPLX = 2 * W_MAX_L * 4 * WQ;            // complex words of the forward tiles (the sums S overlay them)
// LDS (doubles): tables | accumulator [2 components][4 residues][512] | tiles | mod-switched LWE words | octant of zeta powers
constexpr int WU_LDS_WORDS = fftq::QT_WORDS + 2 * WN + 2 * WU_TILE_CPLX + BMI_AT_WORDS + W_ZO_WORDS;
static_assert(WU_LDS_WORDS <= BMI_LDS_WORDS_MAX, "WU_LDS_WORDS exceeds the 160 KB of LDS");
static_assert(2 * 2 * 4 * WQ <= WU_TILE_CPLX, "the sums S of both limbs and outputs fit over the tiles");

// STATS (the test hook bmi_fft_margin_host): also records the largest distance of a limb sum from the integer it is rounded to
// GLWE: the kernel returns the accumulator itself, out = [count][2N], instead of the extracted sample, out = [count][N + 1]
template <int L, int BG, int PREC, bool STATS, bool GLWE>
__global__ void __launch_bounds__(W_THREADS)
    k_blind_rotate_wu_t64f(const u64 *__restrict__ small_cts, const uint32_t *__restrict__ lut_ids, const u64 *__restrict__ luts,
                           const double *__restrict__ bsk3_w, const double *__restrict__ g_tw, const double *__restrict__ g_zeta_oct,
                           u64 *__restrict__ out, uint32_t count, uint32_t n, unsigned long long *__restrict__ stat) {
    constexpr int LIMBS = Scheme<PREC>::LIMBS, LB = Scheme<PREC>::BITS, PRE = Scheme<PREC>::PRE, AB = 64 - PRE;
    // three keys, each scaled by |X^c - 1| <= 2: the limb sums are six times the plain step's
    static_assert(6.0 * 2.0 * L * WN * (double)(1ull << (BG - 1)) * (double)(1ull << (LB - 1)) <= 0x1p45, "limb sums must stay below 2^45");
    static_assert(LIMBS == 2 && L <= W_MAX_L && L * BG < AB, "two limbs, at most three levels");
    constexpr int ROWS = 3 * 2 * L;   // key rows of a step: [key 3][row 2L], contiguous in the key copy
    constexpr int KD = BMI_T64WU_KEY_ROWS_AHEAD < ROWS ? BMI_T64WU_KEY_ROWS_AHEAD : ROWS;
    extern __shared__ double lds[];
    double *acc = lds + fftq::QT_WORDS;                                     // [2 components][4 residues][512]: word / 2^PRE, exact, |.| < 2^51
    double2 *tiles = reinterpret_cast<double2 *>(acc + 2 * WN);             // [2L rows][4 quarters][256 slots] complex
    double2 *SD = tiles;                                                    // [limb][output][4 quarters][256 slots], once the tiles are read
    uint16_t *at = reinterpret_cast<uint16_t *>(tiles + WU_TILE_CPLX);
    double *zo_w = reinterpret_cast<double *>(tiles + WU_TILE_CPLX) + BMI_AT_WORDS;
    const double2 *ZO = reinterpret_cast<const double2 *>(zo_w);            // zeta^x, x in [0, 512]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < fftq::QT_WORDS; i += W_THREADS) lds[i] = g_tw[i];
    for (int i = tid; i < W_ZO_WORDS; i += W_THREADS) zo_w[i] = g_zeta_oct[i];
    const uint32_t ct = blockIdx.x;
    t64::stage_lwe<WLOG + 1>(at, small_cts + (size_t)ct * (n + 1), n, tid, W_THREADS);
    __syncthreads();
    load_start_acc<PRE>(acc, luts, lut_ids, ct, at, n, tid);
    __syncthreads();
    // phase B: output polynomial, slot, and which half of the radix-4 butterfly this lane starts from
    const int mo = wave >> 3, w8 = wave & 7, tp = lane >> 5, mq = w8 * 32 + (lane & 31);
    // X^c at this thread's first frequency k0 = kappa + 256 tp is zeta^((4 k0 + 1) c); at k0 + 512 it is that times (-1)^c
    const uint32_t root_e = 4 * ((uint32_t)fftq::slot_freq(mq >> 6, mq & 63) + 256 * (uint32_t)tp) + 1;
    const uint32_t pairs = (n + 1) >> 1;
    uint32_t since_centred = 0;   // steps taken since the accumulator was last reduced mod 2^AB
    double dev = 0.0;             // STATS: largest |value - nearest integer| this lane has rounded away

    auto a_first = [&](uint32_t ip) -> uint32_t { return at[2 * ip]; };
    auto a_second = [&](uint32_t ip) -> uint32_t { return 2 * ip + 1 < n ? at[2 * ip + 1] : 0u; };   // (at[n] is the body)
    // steps are the pairs with a non-zero coefficient (every factor X^0 - 1 vanishes: the oracle skips those too)
    auto next_step = [&](uint32_t ip) {   // uniform over the workgroup
        while (ip < pairs && (a_first(ip) | a_second(ip)) == 0) ip++;
        return ip;
    };
    // key words of this thread at pair ip: the step's rows [key 3][row 2L]
    auto step_key = [&](uint32_t ip) { return key_ptr<ROWS, LIMBS>(bsk3_w, ip, mo, w8, lane); };
    double2 kk[KD][LIMBS][2];
    auto request_first_rows = [&](const double2 *kth) { static_for<0, KD>([&](auto R) { request_row(kk[R], kth, R); }); };
    uint32_t ip = next_step(0);
    if (ip < pairs) request_first_rows(step_key(ip));
    while (ip < pairs) {
        const uint32_t a1 = a_first(ip), a2 = a_second(ip);
        const uint32_t cj[3] = {(a1 + a2) & (2 * WN - 1), a1, a2};
        const double2 *kth = step_key(ip);
        const uint32_t ip_next = next_step(ip + 1);
        auto forward_task = [&](const int T) {
            const int R = T >> 2, h = T & 3, c = R / L, lev = R % L;
            const double *ac = acc + c * WN + h * W_RES + lane;
            double x[8];   // re[r] = x[r], im[r] = x[r + 4]
            static_for<0, 8>([&](auto J) {
                const double dd = mod_ab<AB>(ac[64 * (J & 3) + 256 * (J >> 2)]);   // coefficient 4 (lane + 64 (J & 3)) + h + 1024 (J >> 2)
                x[J] = t64::digit<L, BG, AB>(dd, lev);
            });
            const double re[4] = {x[0], x[1], x[2], x[3]}, im[4] = {x[4], x[5], x[6], x[7]};
            C v[4];
            fftq::forward_quarter(h, re, im, v, lane, lds);
            double2 *tile = tiles + (size_t)T * WQ;
            static_for<0, 4>([&](auto R4) { tile[R4 * 64 + lane] = double2{v[R4].r, v[R4].i}; });
        };
        if (wave < 8 * L) forward_task(wave);
        if constexpr (8 * L > 16) {
            pin();
            if (wave < 8 * L - 16) forward_task(16 + wave);
        }
        __syncthreads();
        C s_lo[LIMBS], s_hi[LIMBS];
        {
            C s[LIMBS][2], y[LIMBS][2];   // sums over the three keys, scaled; one key's sums over its 2L rows
            static_for<0, LIMBS>([&](auto J) { s[J][0] = s[J][1] = y[J][0] = y[J][1] = C{0.0, 0.0}; });
            static_for<0, ROWS>([&](auto T) {
                constexpr int key = T / (2 * L), R = T % (2 * L);
                const double2 lo = tiles[(size_t)(R * 4 + tp) * WQ + mq], hi = tiles[(size_t)(R * 4 + tp + 2) * WQ + mq];
                C a0, a1f;   // the row at frequencies kappa + 256 tp and kappa + 256 (tp + 2)
                forward_half_butterfly(lo, hi, tp, lane, a0, a1f);
                static_for<0, LIMBS>([&](auto J) { cmac2(y[J], a0, a1f, kk[T % KD][J]); });
                if constexpr (T + KD < ROWS) request_row(kk[T % KD], kth, T + KD);
                if constexpr (R == 2 * L - 1) {   // the key is complete: scale by X^c - 1 at the thread's two frequencies, add
                    const uint32_t cc = cj[key];
                    const double2 z = zeta_pow(ZO, (root_e * cc) & (2 * WN - 1));
                    const double w0r = z.x - 1.0, w0i = z.y;
                    const double w1r = ((cc & 1) ? -z.x : z.x) - 1.0, w1i = (cc & 1) ? -z.y : z.y;
                    static_for<0, LIMBS>([&](auto J) {
                        s[J][0].r += __builtin_fma(y[J][0].r, w0r, -(y[J][0].i * w0i));
                        s[J][0].i += __builtin_fma(y[J][0].r, w0i, y[J][0].i * w0r);
                        s[J][1].r += __builtin_fma(y[J][1].r, w1r, -(y[J][1].i * w1i));
                        s[J][1].i += __builtin_fma(y[J][1].r, w1i, y[J][1].i * w1r);
                        y[J][0] = y[J][1] = C{0.0, 0.0};
                    });
                }
                pin();   // one row at a time: neither the next rows' tile reads nor their key requests move up (registers)
            });
            const double2 wl = reinterpret_cast<const double2 *>(lds)[conj_w_lo_index(tp, mq)];
            const double2 wh = reinterpret_cast<const double2 *>(lds)[conj_w_hi_index(tp, mq)];
            static_for<0, LIMBS>([&](auto J) { inverse_half_butterfly(s[J][0], s[J][1], tp, lane, wl, wh, s_lo[J], s_hi[J]); });
        }
        if (ip_next < pairs) request_first_rows(step_key(ip_next));   // (uniform) the next step's first rows
        pin();
        __syncthreads();   // every thread has read the tiles: the sums may overwrite them
        static_for<0, LIMBS>([&](auto J) { store_sums(SD + (size_t)((J * 2 + mo) * 4) * WQ + mq, tp, s_lo[J], s_hi[J]); });
        __syncthreads();
        if (wave >= 8) {   // (wavefronts 0 .. 7 ran two forward tasks where L = 3)
            const int o = (wave >> 2) & 1, h = wave & 3;
            double re[LIMBS][4], im[LIMBS][4];
            static_for<0, LIMBS>([&](auto J) {
                const double2 *sd = SD + (size_t)((J * 2 + o) * 4 + h) * WQ;
                C v[4];
                static_for<0, 4>([&](auto R) {
                    const double2 t = sd[R * 64 + lane];
                    v[R] = C{t.x, t.y};
                });
                fftq::inverse_quarter(v, re[J], im[J], lane, lds);
            });
            double *ao = acc + o * WN + h * W_RES + lane;
            static_for<0, 4>([&](auto R) {
                ao[64 * R] += t64::place_limbs<AB, LB, STATS>(re[0][R], re[1][R], dev);              // coefficient 4 (lane + 64 R) + h
                ao[64 * R + 256] += t64::place_limbs<AB, LB, STATS>(im[0][R], im[1][R], dev);        // ... + 1024
            });
        }
        __syncthreads();
        if (++since_centred == W_RECENTRE) {   // (uniform: counts the steps actually taken)
            since_centred = 0;
            recentre<AB, 4>(acc, tid);
            __syncthreads();
        }
        ip = ip_next;
    }
    if constexpr (STATS) atomicMax(stat, (unsigned long long)__double_as_longlong(dev));   // non-negative doubles order like their bit patterns
    if constexpr (GLWE) {   // the accumulator itself, out = [count][2N]
        u64 *g = out + (size_t)ct * (2 * WN);
        static_for<0, 2>([&](auto Q) { t64::store_glwe<WN, PRE, AB>(g, acc, acc_slot, tid + W_THREADS * Q); });
        return;
    }
    u64 *o = out + (size_t)ct * (WN + 1);
    static_for<0, 2>([&](auto Q) { t64::extract_sample<WN, PRE, AB>(o, acc, acc_slot, tid + W_THREADS * Q); });
}

}  // namespace

namespace bmit {

int launch_blind_rotate_wide_u(const RotBatch &b) {
    if (b.count == 0) return 0;
    if (!shape_supported_wide_unrolled(b.prec, b.levels, b.base_log)) return (int)hipErrorInvalidValue;
    return with_levels_stats_glwe(b.levels, b.stat != nullptr, b.glwe, [&](auto L, auto STATS, auto GLWE) {
        return launch_with_lds<k_blind_rotate_wu_t64f<L, 10, 40, STATS, GLWE>>(dim3(b.count), dim3(W_THREADS), (size_t)WU_LDS_WORDS * sizeof(double), b.s,
                                                                               b.cts, b.ids, b.luts.u(), b.key.d(), b.tab[0].d(), b.tab[1].d(), b.out, b.count, b.n, b.stat);
    });
}

}  // namespace bmit
