// 2^64 TORUS at N = 2048 (the secure128_torus set: n 742, k 1, l 3, Bg 2^10): blind rotation with the exact limb products
// carried by the floating-point transform of fft_quarter_f64.hpp (gfx950).
//
// Same scheme as bmi_kernels_t64f.hip one size up: bootstrap key stored at 46 bits of precision (words rounded to multiples of
// 2^18; the rounded key IS the key: exported, given to the oracle) as two balanced 23-bit limbs, digits in base 2^10,
// accumulator the exact integer word / 2^18 in a double.  Per limb the sum over the 2 l digit x limb polynomial products is an
// integer below 2^45; it is computed through the folded 1,024-point complex FFT and ROUNDED TO THE NEAREST INTEGER, which
// returns it exactly (a-priori bound 0.41 < 1/2 in the header; measured distance ~2^-12, bmi_fft_margin_host) - so the kernel's
// words equal the oracle's integer arithmetic bit for bit (tests/test_gpu_torus_wide.py).
//
// One workgroup of 16 wavefronts per ciphertext (what auto dispatch runs up to 256 ciphertexts; beyond: bmi_kernels_t64w2.hip); a transform is split over FOUR wavefronts by the folded index
// mod 4 (quarters of 256 points, 4 complex points per lane, no LDS inside a quarter).  Per CMUX:
//   A  8 l forward tasks (input polynomial c, level, quarter h) over the 16 wavefronts: rotate / decompose 512 coefficients of the
//      accumulator (the oracle's integer rule), forward quarter -> tile (slot order, times W_h)
//   B  all 1,024 threads = (output polynomial o, slot, tp): a pair of lanes 32 apart shares a slot - lane tp reads quarters tp and
//      tp + 2 of each row, half a radix-4 butterfly each, ONE 2 x 2 transpose on lane bit 5 (v_permlane32_swap) completes it: two
//      frequencies A_{kappa + 256 tp}, A_{kappa + 256 (tp + 2)} per thread and row, multiplied with both limbs' key words (32
//      KiB per wavefront, row and limb; the first rows of a step are requested during the step before, row r + KD when row r is done);
//      the inverse butterfly the same way back, times conj W_h -> the sums S_h (over the tiles, after a barrier)
//   C  8 inverse tasks (o, quarter) on wavefronts 8 .. 15: the inverse quarters of BOTH limbs (two independent transforms in one
//      wavefront), nearest integers, limb 1 shifted into place, one plain read-modify-write per coefficient of the accumulator
//      (an LDS f64 atomic costs ~32 cycles per wavefront instruction: 128 of them per CMUX were 4.4 k cycles); re-centred mod 2^46
//      every 8 steps
#include <hip/hip_runtime.h>

#include "bmi_internal.hpp"
#include "fft_quarter_f64.hpp"
#include "pair_sync.hpp"
#include "phase_prof.hpp"
#include "t64_common.hpp"
#include "t64_wide_steps.hpp"

using t64::i64;
using t64::u64;

namespace {

using namespace t64w;   // the N = 2048 family's constants (WN, WQ, W_*) and shared steps: t64_wide_steps.hpp
using t64::Scheme;

#ifndef BMI_T64W_KEY_ROWS_AHEAD
#define BMI_T64W_KEY_ROWS_AHEAD 2   // key rows (of 2 l) a thread holds in registers: requested before phase A, then row r + this many when row r is done
#endif
PH_ARRAY(g_phase_w)   // make -C csrc prof; tools/phase_prof_t64w.py
constexpr int WF_TILE_CPLX = 2 * W_MAX_L * 4 * WQ;            // complex words of the forward tiles (the sums S overlay them)
// LDS (doubles): tables | accumulator [2 components][4 residues][512] | tiles | mod-switched LWE words
constexpr int WF_LDS_WORDS = fftq::QT_WORDS + 2 * WN + 2 * WF_TILE_CPLX + BMI_AT_WORDS;
static_assert(WF_LDS_WORDS <= BMI_LDS_WORDS_MAX, "WF_LDS_WORDS exceeds the 160 KB of LDS");
static_assert(2 * 2 * 4 * WQ <= WF_TILE_CPLX, "the sums S of both limbs and outputs fit over the tiles");

// standard-domain GGSW polynomials (u64 torus words, already rounded to the key precision) -> per (polynomial, limb) 1,024
// complex words A_k / 2 in the order the multiplying threads read them: thread (w8 = slot / 32, lane) of phase B owns slot
// p = 32 w8 + (lane & 31) and, with tp = lane >> 5, the frequencies kappa(p) + 256 (tp + 2 f), f = 0, 1 - complex word
// 512 f + 64 w8 + lane (a wavefront's request is 1 KiB contiguous).  One workgroup of four wavefronts (the four quarters) per item.
__global__ void __launch_bounds__(256) k_bsk_to_w_t64(const u64 *__restrict__ std_polys, double *__restrict__ w_polys,
                                                      const double *__restrict__ g_tw, uint32_t n_polys, int prec) {
    const int limbs = t64::limbs_of(prec);
    __shared__ double lds[fftq::QT_WORDS + 4 * WQ * 2];
    for (int i = threadIdx.x; i < fftq::QT_WORDS; i += blockDim.x) lds[i] = g_tw[i];
    __syncthreads();
    const int h = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t item = blockIdx.x;   // (polynomial, limb)
    const uint32_t poly = item / limbs;
    const int j = (int)(item % limbs);
    double2 *tile = reinterpret_cast<double2 *>(lds + fftq::QT_WORDS);
    key_limb_to_tile(tile, std_polys, poly, j, prec, h, lane, lds);
    __syncthreads();
    {
        const int p = threadIdx.x;
        const double2 q0 = tile[p], q1 = tile[WQ + p], q2 = tile[2 * WQ + p], q3 = tile[3 * WQ + p];
        const C a{q0.x + q2.x, q0.y + q2.y}, b{q0.x - q2.x, q0.y - q2.y};
        const C cc{q1.x + q3.x, q1.y + q3.y}, d{-(q1.y - q3.y), q1.x - q3.x};   // i (q1 - q3)
        const C A[4] = {a + cc, b + d, a - cc, b - d};
        double2 *o = reinterpret_cast<double2 *>(w_polys + (size_t)item * WN);
        const int w8 = p >> 5, l5 = p & 31;
        static_for<0, 4>([&](auto T) {
            constexpr int tp = T & 1, f = T >> 1;
            o[f * (WN / 4) + w8 * 64 + tp * 32 + l5] = double2{0.5 * A[T].r, 0.5 * A[T].i};
        });
    }
}

// STATS (the test hook bmi_fft_margin_host): also records the largest distance of a limb sum from the integer it is rounded to
// GLWE: the kernel returns the accumulator itself, out = [count][2N], instead of the extracted sample, out = [count][N + 1]
template <int L, int BG, int PREC, bool STATS, bool GLWE>
__global__ void __launch_bounds__(W_THREADS)
    k_blind_rotate_w_t64f(const u64 *__restrict__ small_cts, const uint32_t *__restrict__ lut_ids, const u64 *__restrict__ luts,
                          const double *__restrict__ bsk_w, const double *__restrict__ g_tw, u64 *__restrict__ out, uint32_t count,
                          uint32_t n, unsigned long long *__restrict__ stat) {
    constexpr int LIMBS = Scheme<PREC>::LIMBS, LB = Scheme<PREC>::BITS, PRE = Scheme<PREC>::PRE, AB = 64 - PRE;
    // a limb's sum: 2 L N terms of |digit| <= 2^(BG-1) times |limb| <= 2^(LB-1) - the transform's error bound is stated for this size
    static_assert(2.0 * L * WN * (double)(1ull << (BG - 1)) * (double)(1ull << (LB - 1)) <= 0x1p45, "limb sums must stay below 2^45");
    static_assert(LIMBS == 2 && L <= W_MAX_L && L * BG < AB, "two limbs, at most three levels");
    constexpr int KD = BMI_T64W_KEY_ROWS_AHEAD < 2 * L ? BMI_T64W_KEY_ROWS_AHEAD : 2 * L;
    extern __shared__ double lds[];
    double *acc = lds + fftq::QT_WORDS;                                     // [2 components][4 residues][512]: word / 2^PRE, exact, |.| < 2^51
    double2 *tiles = reinterpret_cast<double2 *>(acc + 2 * WN);             // [2L rows][4 quarters][256 slots] complex
    double2 *SD = tiles;                                                    // [limb][output][4 quarters][256 slots], once the tiles are read
    uint16_t *at = reinterpret_cast<uint16_t *>(tiles + WF_TILE_CPLX);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < fftq::QT_WORDS; i += W_THREADS) lds[i] = g_tw[i];
    const uint32_t ct = blockIdx.x;
    t64::stage_lwe<WLOG + 1>(at, small_cts + (size_t)ct * (n + 1), n, tid, W_THREADS);
    __syncthreads();
    load_start_acc<PRE>(acc, luts, lut_ids, ct, at, n, tid);
    __syncthreads();
    // phase B: output polynomial, slot, and which half of the radix-4 butterfly this lane starts from
    const int mo = wave >> 3, w8 = wave & 7, tp = lane >> 5, mq = w8 * 32 + (lane & 31);
    uint32_t since_centred = 0;   // steps taken since the accumulator was last reduced mod 2^AB
    double dev = 0.0;             // STATS: largest |value - nearest integer| this lane has rounded away
    PH_DECL();

    // steps are the LWE coefficients that switch to a non-zero rotation (X^0 ACC - ACC = 0: the oracle skips those too)
    auto next_step = [&](uint32_t i) {   // uniform over the workgroup
        while (i < n && at[i] == 0) i++;
        return i;
    };
    // key words of this thread at step i: rows [2L] of the per-polynomial key copy
    auto step_key = [&](uint32_t i) { return key_ptr<2 * L, LIMBS>(bsk_w, i, mo, w8, lane); };
    // rows 0 .. KD-1 of a step are requested during the step BEFORE (after its products: they land under its inverse quarters and
    // the next forward tasks), row r + KD when row r has been multiplied
    double2 kk[KD][LIMBS][2];
    auto request_first_rows = [&](const double2 *kth) { static_for<0, KD>([&](auto R) { request_row(kk[R], kth, R); }); };
    uint32_t i = next_step(0);
    if (i < n) request_first_rows(step_key(i));
    while (i < n) {
        const uint32_t a_t = at[i];
        const double2 *kth = step_key(i);
        const uint32_t i_next = next_step(i + 1);
        PH_MARK(0);   // loop head, key requests
        auto forward_task = [&](const int T) {
            const int R = T >> 2, h = T & 3, c = R / L, lev = R % L;
            const double *ac = acc + c * WN;
            double x[8];   // re[r] = x[r], im[r] = x[r + 4]
            // (four coefficients at a time, fenced: the 32 key registers in flight leave this task ~90)
            static_for<0, 2>([&](auto G) {
                rotated_diff_digits<L, BG, AB, G>(x, ac, h, lane, a_t, lev);
                pin();
            });
            // (written out in all four kernels: inlined through a helper, the transform's own instructions come in another order)
            const double re[4] = {x[0], x[1], x[2], x[3]}, im[4] = {x[4], x[5], x[6], x[7]};
            C v[4];
            fftq::forward_quarter(h, re, im, v, lane, lds);
            double2 *tile = tiles + (size_t)T * WQ;
            static_for<0, 4>([&](auto R4) { tile[R4 * 64 + lane] = double2{v[R4].r, v[R4].i}; });
        };
        // (issue priorities in this phase, stepping down per task or held by the wavefronts with two tasks, measured no effect)
        forward_task(wave);
        PH_MARK(1);   // first forward task
        if constexpr (8 * L > 16) {
            pin();
            if (wave < 8 * L - 16) forward_task(16 + wave);
        }
        PH_MARK(2);   // second forward task (wavefronts 0 .. 8 L - 17)
        __syncthreads();
        PH_MARK(3);   // barrier A -> B
        C s_lo[LIMBS], s_hi[LIMBS];
        {
            C y[LIMBS][2];
            static_for<0, LIMBS>([&](auto J) { y[J][0] = y[J][1] = C{0.0, 0.0}; });
            static_for<0, 2 * L>([&](auto R) {
                const double2 lo = tiles[(size_t)(R * 4 + tp) * WQ + mq], hi = tiles[(size_t)(R * 4 + tp + 2) * WQ + mq];
                C a0, a1;   // the row at frequencies kappa + 256 tp and kappa + 256 (tp + 2)
                forward_half_butterfly(lo, hi, tp, lane, a0, a1);
                static_for<0, LIMBS>([&](auto J) { cmac2(y[J], a0, a1, kk[R % KD][J]); });
                if constexpr (R + KD < 2 * L) request_row(kk[R % KD], kth, R + KD);
                pin();   // one row at a time: neither the next rows' tile reads nor their key requests move up (registers)
            });
            const double2 wl = reinterpret_cast<const double2 *>(lds)[conj_w_lo_index(tp, mq)];
            const double2 wh = reinterpret_cast<const double2 *>(lds)[conj_w_hi_index(tp, mq)];
            static_for<0, LIMBS>([&](auto J) { inverse_half_butterfly(y[J][0], y[J][1], tp, lane, wl, wh, s_lo[J], s_hi[J]); });
        }
        if (i_next < n) request_first_rows(step_key(i_next));   // (uniform) the next step's first rows
        pin();
        PH_MARK(4);   // products of 2 L rows, inverse butterfly, next key requests
        __syncthreads();   // every thread has read the tiles: the sums may overwrite them
        static_for<0, LIMBS>([&](auto J) { store_sums(SD + (size_t)((J * 2 + mo) * 4) * WQ + mq, tp, s_lo[J], s_hi[J]); });
        __syncthreads();
        PH_MARK(5);   // barrier, the sums to LDS, barrier
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
        PH_MARK(6);   // inverse quarters of both limbs, rounding, accumulation
        __syncthreads();
        if (++since_centred == W_RECENTRE) {   // (uniform: counts the steps actually taken)
            since_centred = 0;
            recentre<AB, 4>(acc, tid);
            __syncthreads();
        }
        PH_MARK(7);   // closing barrier (+ re-centring every eighth step)
        i = i_next;
    }
    PH_STORE(g_phase_w, wave, lane);
    if constexpr (STATS) atomicMax(stat, (unsigned long long)__double_as_longlong(dev));   // non-negative doubles order like their bit patterns
    // (the epilogue through a helper: the step loop's registers are numbered differently, 126 VGPRs for 127)
    if constexpr (GLWE) {   // the accumulator itself, out = [count][2N]
        u64 *g = out + (size_t)ct * (2 * WN);
        static_for<0, 2>([&](auto Q) { t64::store_glwe<WN, PRE, AB>(g, acc, acc_slot, tid + W_THREADS * Q); });
        return;
    }
    u64 *o = out + (size_t)ct * (WN + 1);
    static_for<0, 2>([&](auto Q) { t64::extract_sample<WN, PRE, AB>(o, acc, acc_slot, tid + W_THREADS * Q); });
}

}  // namespace

PH_EXPORT(bmi_debug_phase_prof_t64w, g_phase_w)

namespace bmit {

int launch_bsk_to_wide(const KeyConv &k) {
    if (k.prec != 46 && k.prec != 40) return (int)hipErrorInvalidValue;   // 40: the unrolled key (bmi_kernels_t64wu.hip)
    const uint32_t items = k.n_polys * (uint32_t)t64::limbs_of(k.prec);
    hipLaunchKernelGGL(k_bsk_to_w_t64, dim3(items), dim3(256), 0, k.s, k.std_polys, (double *)k.dst, k.tab[0].d(), k.n_polys, k.prec);
    BMI_LAUNCH_CHECK();
    return 0;
}

int launch_blind_rotate_wide(const RotBatch &b) {
    if (b.count == 0) return 0;
    if (!shape_supported_wide(b.prec, b.levels, b.base_log)) return (int)hipErrorInvalidValue;
    return with_levels_stats_glwe(b.levels, b.stat != nullptr, b.glwe, [&](auto L, auto STATS, auto GLWE) {
        return launch_with_lds<k_blind_rotate_w_t64f<L, 10, 46, STATS, GLWE>>(dim3(b.count), dim3(W_THREADS), (size_t)WF_LDS_WORDS * sizeof(double), b.s,
                                                                              b.cts, b.ids, b.luts.u(), b.key.d(), b.tab[0].d(), b.out, b.count, b.n, b.stat);
    });
}

}  // namespace bmit
