// 2^64 TORUS at N = 2048, UNROLLED blind rotation, THROUGHPUT form: two ciphertexts per workgroup sharing every key word a thread
// loads (gfx950).
//
// Same function and the same words as k_blind_rotate_wu_t64f (bmi_kernels_t64wu.hip: the step of oracle/tfhe_oracle.c
// ora_blind_rotate_extract_unrolled, key at 40 bits of precision = two balanced 20-bit limbs, digits in base 2^10, accumulator the
// exact integer word / 2^24 in a double, limb sums through the folded 1,024-point complex FFT of fft_quarter_f64.hpp and ROUNDED TO
// THE NEAREST INTEGER), on the SAME key copy (bsk3.wide, the per-polynomial layout of launch_bsk_to_wide: no second copy of the
// unrolled key exists).  What changes is the arrangement.  That kernel keeps all 2 l digit transforms of a step in LDS (96 KB of
// tiles: one ciphertext per compute unit) and a step takes in 18 key rows, 1.18 MB, for ONE ciphertext.  Here a step walks the
// decomposition levels as k_blind_rotate_w2_t64f and k_blind_rotate_q_t64f do - one level's tiles of both ciphertexts in LDS
// (64 KB), the running sums in registers across the levels - and every key word is multiplied with both ciphertexts.
//
// Where the factor X^c - 1 goes.  With the levels outermost, sums per key (wu's `y`) would be 3 keys x 4 complex x 2 ciphertexts
// = 96 registers.  Instead each key's factor zeta^((4k+1) c_j) - 1 is applied to the DIGIT TRANSFORM before the product with that
// key's row, so that all three keys and all levels accumulate into one set of 4 complex sums per ciphertext (32 registers for
// both): two more complex multiplications per (row, ciphertext).  The three c_j differ per ciphertext: the six factors of a
// thread are re-read from the octant at every use, 36 LDS reads per step; a thread keeps their six exponents (the factors
// themselves would be 24 registers beside the 32 of the sums, the 32 of two key rows and the 16 of a row's butterflies of both
// ciphertexts: not tried in that form since `keep` below was added).
//
// Exactness.  The limb sums are the same integers as wu's, below 2^44.2.  tools/fft_bound.py unrolled_limb_sum_bound counts the
// scaling as one more multiplication stage on every product with beta = 1.5 e for a table entry minus one; that holds wherever in
// the chain of multiplications the factor is applied, so the a-priori bound is wu's 0.38 < 1/2.  The octant of zeta is folded by
// its exact symmetries as there: no factor is a product of two table entries.
//
// Two ciphertexts with different steps.  A pair is skipped only when BOTH ciphertexts have a = a' = 0 (uniform over the
// workgroup).  A ciphertext whose pair is zero beside one whose pair is not runs the step with the factors zeta^0 - 1 = 0
// exactly (the table's first entry is (1, 0)): its sums are exact zeros, its accumulator is unchanged.  The re-centring counts the
// steps the WORKGROUP takes, at least those either ciphertext takes, so |acc| stays below 2^51.  An odd batch: the last workgroup
// runs its one ciphertext twice and writes it once.
//
// Per step, for each level:
//   A  16 forward tasks (ciphertext, input polynomial c, quarter h), one per wavefront: decompose 512 coefficients of the
//      accumulator itself (no rotation), digit `level`, forward quarter -> tile (slot order, times W_h)
//   B  all 1,024 threads = (output polynomial o, slot, tp), lanes 32 apart sharing a slot as in wu: per input polynomial and
//      ciphertext the radix-4 butterfly (one 2 x 2 transpose on lane bit 5, v_permlane32_swap) ONCE for the three keys; per key the
//      two frequencies' values times that ciphertext's factor, then multiply-accumulates with both limbs' key words; the key
//      rows of a level are requested BMI_T64WU2_KEY_ROWS_AHEAD rows ahead in the order they are used (polynomial, key), the
//      first ones before the barrier that ends phase A
// then per ciphertext the inverse butterfly times conj W_h, and per limb: the sums to LDS (over the tiles), 16 inverse tasks
// (ciphertext, output, quarter): inverse quarter, nearest integer, shift into place, plain read-modify-write of the accumulator.
//
// Resources (make resource-usage): 123 VGPRs (125 with STATS, 128 with GLWE), 161,168 B of LDS (static_assert below), no scratch in
// the sample and STATS forms; the GLWE form spills one register, 8 B per lane, stored before the step loop and reloaded after it:
// the loop itself has no scratch access in any form.  That takes `keep` below: without it the compiler sinks the multiply-adds of
// all levels below the last level's forward task and parks their operands in scratch (1.4 - 1.6 KB per lane).
//
// Measured (tools/unrolled_wide2_ab.py, profiles/unrolled_wide2_ab.txt; n = 742, alternating with wu in one process): 11.35 ms for
// 512 ciphertexts (one round of 256 workgroups) against wu's 15.25 ms (two rounds), 45.0 against 61.0 ms for 2,048, 180.6 against
// 244.0 ms for 8,192: 45.4 k PBS/s against 33.6 k, 73 k cycles per step of a workgroup's two ciphertexts against 49 k for one.
// Largest distance of a limb sum from the integer it is rounded to, 258 rows of uniformly random words at n = 16: 2^-14.0 (wu:
// 2^-14.0), against the a-priori 0.38 (tests/test_gpu_torus_wide_unrolled2.py).
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

#ifndef BMI_T64WU2_KEY_ROWS_AHEAD
#define BMI_T64WU2_KEY_ROWS_AHEAD 2   // key rows (of the 6 of a level) a thread holds in registers (3: 32 - 40 B of scratch per lane)
#endif
constexpr int WU2_TILE_CPLX = 2 * 2 * 4 * WQ;                  // one level's tiles [ciphertext 2][component 2][quarter 4][256]; one limb's sums overlay them
// LDS (doubles): tables | accumulators [ciphertext 2][component 2][residue 4][512] | tiles | mod-switched LWE words of both | octant
constexpr int WU2_LDS_WORDS = fftq::QT_WORDS + 2 * 2 * WN + 2 * WU2_TILE_CPLX + 2 * BMI_AT_WORDS + W_ZO_WORDS;
static_assert(WU2_LDS_WORDS <= BMI_LDS_WORDS_MAX, "WU2_LDS_WORDS exceeds the 160 KB of LDS");

// STATS (the test hook bmi_fft_margin_host): also records the largest distance of a limb sum from the integer it is rounded to
// GLWE: the kernel returns the accumulator itself, out = [count][2N], instead of the extracted sample, out = [count][N + 1]
template <int L, int BG, int PREC, bool STATS, bool GLWE>
__global__ void __launch_bounds__(W_THREADS)
    k_blind_rotate_wu2_t64f(const u64 *__restrict__ small_cts, const uint32_t *__restrict__ lut_ids, const u64 *__restrict__ luts,
                            const double *__restrict__ bsk3_w, const double *__restrict__ g_tw, const double *__restrict__ g_zeta_oct,
                            u64 *__restrict__ out, uint32_t count, uint32_t n, unsigned long long *__restrict__ stat) {
    constexpr int LIMBS = Scheme<PREC>::LIMBS, LB = Scheme<PREC>::BITS, PRE = Scheme<PREC>::PRE, AB = 64 - PRE;
    // three keys, each scaled by |X^c - 1| <= 2: the limb sums are six times the plain step's
    static_assert(6.0 * 2.0 * L * WN * (double)(1ull << (BG - 1)) * (double)(1ull << (LB - 1)) <= 0x1p45, "limb sums must stay below 2^45");
    static_assert(LIMBS == 2 && L <= W_MAX_L && L * BG < AB, "two limbs, at most three levels");
    constexpr int LROWS = 3 * 2;   // key rows of a level: of the step's [key 3][row 2L] in the key copy, in the order (component, key)
    constexpr int KD = BMI_T64WU2_KEY_ROWS_AHEAD < LROWS ? BMI_T64WU2_KEY_ROWS_AHEAD : LROWS;
    extern __shared__ double lds[];
    double *accs = lds + fftq::QT_WORDS;                                    // [ciphertext][2 components][4 residues][512]: word / 2^PRE, exact, |.| < 2^51
    double2 *tiles = reinterpret_cast<double2 *>(accs + 2 * 2 * WN);        // [ciphertext 2][component 2][quarter 4][256 slots] of the current level
    double2 *SD = tiles;                                                    // one limb's sums [ciphertext 2][output 2][quarter 4][256 slots]
    uint16_t *at = reinterpret_cast<uint16_t *>(tiles + WU2_TILE_CPLX);     // [ciphertext 2][BMI_AT_WORDS * 4]
    constexpr int AT_STRIDE = BMI_AT_WORDS * 4;
    double *zo_w = reinterpret_cast<double *>(tiles + WU2_TILE_CPLX) + 2 * BMI_AT_WORDS;
    const double2 *ZO = reinterpret_cast<const double2 *>(zo_w);            // zeta^x, x in [0, 512]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < fftq::QT_WORDS; i += W_THREADS) lds[i] = g_tw[i];
    for (int i = tid; i < W_ZO_WORDS; i += W_THREADS) zo_w[i] = g_zeta_oct[i];
    // the two ciphertexts of this workgroup (an odd batch: the last workgroup runs its one ciphertext twice and writes it once)
    uint32_t cts[2];
    const bool live1 = ciphertext_pair(cts, blockIdx.x, count);
    for (int b = 0; b < 2; b++) {   // (written out, as is the loop below: see bmi_kernels_t64w2.hip)
        const u64 *lwe = small_cts + (size_t)cts[b] * (n + 1);
        for (uint32_t i = tid; i <= n; i += W_THREADS) at[b * AT_STRIDE + i] = (uint16_t)t64::modswitch<WLOG + 1>(lwe[i]);
    }
    __syncthreads();
    for (int b = 0; b < 2; b++) {
        const u64 *tv = luts + (size_t)(lut_ids[cts[b]] & (BMI_LUT_CAP - 1)) * WN;
        const uint32_t bt = at[b * AT_STRIDE + n];
        double *acc = accs + b * 2 * WN;
        static_for<0, 2>([&](auto Q) { t64::load_test_poly<WN, PRE>(acc, acc_slot, tv, bt, tid + W_THREADS * Q); });
    }
    __syncthreads();
    // phase B: output polynomial, slot, and which half of the radix-4 butterfly this lane starts from
    const int mo = wave >> 3, w8 = wave & 7, tp = lane >> 5, mq = w8 * 32 + (lane & 31);
    // phases A and C: wavefront = (ciphertext, component / output, quarter)
    const int wb = wave >> 3, wc = (wave >> 2) & 1, wh = wave & 3;
    // X^c at this thread's first frequency k0 = kappa + 256 tp is zeta^((4 k0 + 1) c); at k0 + 512 it is that times (-1)^c
    const uint32_t root_e = 4 * ((uint32_t)fftq::slot_freq(mq >> 6, mq & 63) + 256 * (uint32_t)tp) + 1;
    const uint32_t pairs = (n + 1) >> 1;
    uint32_t since_centred = 0;   // steps taken by the workgroup since the accumulators were last reduced mod 2^AB
    double dev = 0.0;             // STATS: largest |value - nearest integer| this lane has rounded away

    auto a_first = [&](int b, uint32_t ip) -> uint32_t { return at[b * AT_STRIDE + 2 * ip]; };
    auto a_second = [&](int b, uint32_t ip) -> uint32_t { return 2 * ip + 1 < n ? at[b * AT_STRIDE + 2 * ip + 1] : 0u; };   // (at[n] is the body)
    // steps are the pairs where either ciphertext has a non-zero coefficient
    auto next_step = [&](uint32_t ip) {   // uniform over the workgroup
        while (ip < pairs && (a_first(0, ip) | a_second(0, ip) | a_first(1, ip) | a_second(1, ip)) == 0) ip++;
        return ip;
    };
    // key words of this thread at pair ip: [key 3][row 2L][output 2][limb][f][64 w8 + lane] complex
    // (t64w::key_ptr called here: one vector instruction fewer)
    auto key_ptr = [&](uint32_t ip) {
        return reinterpret_cast<const double2 *>(bsk3_w + (size_t)ip * 3 * 4 * L * LIMBS * WN) + (size_t)mo * LIMBS * (WN / 2) + (w8 * 64 + lane);
    };
    double2 kk[KD][LIMBS][2];
    // the T-th row a level uses, T = component * 3 + key, in the key copy's order [key][component][level]
    auto row_of = [](const int lev, const int T) constexpr { return (T % 3) * 2 * L + (T / 3) * L + lev; };
    uint32_t ip = next_step(0);
    while (ip < pairs) {
        const double2 *kth = key_ptr(ip);
        const uint32_t ip_next = next_step(ip + 1);
        // the exponents of this thread's six factors zeta^((4 k0 + 1) c), c = (a + a', a, a') of either ciphertext (4 k0 + 1 is odd:
        // an exponent has the parity of its c)
        uint32_t fx[2][3];
        static_for<0, 2>([&](auto B) {
            const uint32_t a1 = a_first(B, ip), a2 = a_second(B, ip);
            fx[B][0] = (root_e * (a1 + a2)) & (2 * WN - 1);
            fx[B][1] = (root_e * a1) & (2 * WN - 1);
            fx[B][2] = (root_e * a2) & (2 * WN - 1);
        });
        C s[2][LIMBS][2];   // [ciphertext][limb][frequency]: sums over the three keys and all levels
        static_for<0, 2>([&](auto B) { static_for<0, LIMBS>([&](auto J) { s[B][J][0] = s[B][J][1] = C{0.0, 0.0}; }); });
        static_for<0, L>([&](auto LEV) {
            constexpr int lev = LEV;
            {   // phase A
                const double *ac = accs + wb * 2 * WN + wc * WN + wh * W_RES + lane;
                double x[8];   // re[r] = x[r], im[r] = x[r + 4]
                static_for<0, 8>([&](auto J) {
                    const double dd = mod_ab<AB>(ac[64 * (J & 3) + 256 * (J >> 2)]);   // coefficient 4 (lane + 64 (J & 3)) + h + 1024 (J >> 2)
                    x[J] = t64::digit<L, BG, AB>(dd, lev);
                });
                const double re[4] = {x[0], x[1], x[2], x[3]}, im[4] = {x[4], x[5], x[6], x[7]};
                C v[4];
                fftq::forward_quarter(wh, re, im, v, lane, lds);
                double2 *tile = tiles + (size_t)wave * WQ;     // wave = (ciphertext 2, component 2, quarter 4)
                static_for<0, 4>([&](auto R4) { tile[R4 * 64 + lane] = double2{v[R4].r, v[R4].i}; });
            }
            // the level's first key rows land under the barrier (held across phase A instead, they and the factors spill)
            static_for<0, KD>([&](auto R) { request_row(kk[R], kth, row_of(lev, R)); });
            pin();
            __syncthreads();
            static_for<0, 2>([&](auto CC) {   // rows (component CC, this level) of the three keys
                C a[2][2];   // [ciphertext][frequency kappa + 256 tp, kappa + 256 (tp + 2)]
                static_for<0, 2>([&](auto B) {
                    const double2 lo = tiles[(size_t)((B * 2 + CC) * 4 + tp) * WQ + mq], hi = tiles[(size_t)((B * 2 + CC) * 4 + tp + 2) * WQ + mq];
                    // t64w::forward_half_butterfly written out (through the helper the selects come in another order: 7 - 11 s_nop fewer)
                    C u{lo.x + hi.x, lo.y + hi.y};
                    const C dl{lo.x - hi.x, lo.y - hi.y};
                    C w = tp ? C{-dl.i, dl.r} : dl;
                    lanetr::tr_double<5>(u.r, w.r, lane);
                    lanetr::tr_double<5>(u.i, w.i, lane);
                    a[B][0] = u + w;
                    a[B][1] = u - w;
                });
                static_for<0, 3>([&](auto KEY) {
                    constexpr int T = CC * 3 + KEY;
                    static_for<0, 2>([&](auto B) {
                        // X^c - 1 at the thread's two frequencies (the second root is the first times (-1)^c), applied to the digits
                        const double2 z = zeta_pow(ZO, fx[B][KEY]);
                        const bool neg = fx[B][KEY] & 1;
                        const double w0r = z.x - 1.0, w0i = z.y;
                        const double w1r = (neg ? -z.x : z.x) - 1.0, w1i = neg ? -z.y : z.y;
                        const C p0{__builtin_fma(a[B][0].r, w0r, -(a[B][0].i * w0i)), __builtin_fma(a[B][0].r, w0i, a[B][0].i * w0r)};
                        const C p1{__builtin_fma(a[B][1].r, w1r, -(a[B][1].i * w1i)), __builtin_fma(a[B][1].r, w1i, a[B][1].i * w1r)};
                        static_for<0, LIMBS>([&](auto J) { cmac2(s[B][J], p0, p1, kk[T % KD][J]); });
                    });
                    if constexpr (T + KD < LROWS) request_row(kk[T % KD], kth, row_of(lev, T + KD));
                    keep(s);
                    pin();   // one row at a time: neither the next rows' work nor their key requests move up (registers)
                });
            });
            __syncthreads();   // every thread has read this level's tiles: the next level (or the sums) may overwrite them
        });
        {   // inverse butterfly times conj W_h: s[b][j] = (S_tp, S_{tp+2}) afterwards
            const double2 wl = reinterpret_cast<const double2 *>(lds)[conj_w_lo_index(tp, mq)];
            const double2 wh2 = reinterpret_cast<const double2 *>(lds)[conj_w_hi_index(tp, mq)];
            static_for<0, 2>([&](auto B) {
                static_for<0, LIMBS>([&](auto J) { inverse_half_butterfly(s[B][J][0], s[B][J][1], tp, lane, wl, wh2, s[B][J][0], s[B][J][1]); });
            });
        }
        static_for<0, LIMBS>([&](auto J) {
            static_for<0, 2>([&](auto B) { store_sums(SD + (size_t)((B * 2 + mo) * 4) * WQ + mq, tp, s[B][J][0], s[B][J][1]); });
            __syncthreads();
            {
                const double2 *sd = SD + (size_t)wave * WQ;     // wave = (ciphertext, output, quarter)
                C v[4];
                static_for<0, 4>([&](auto R) {
                    const double2 t = sd[R * 64 + lane];
                    v[R] = C{t.x, t.y};
                });
                inverse_task_limb<AB, LB, STATS>(accs + wb * 2 * WN + wc * WN, wh, v, J, lane, lds, dev);
            }
            __syncthreads();
        });
        if (++since_centred == W_RECENTRE) {   // (uniform: counts the steps the workgroup takes)
            since_centred = 0;
            recentre<AB, 8>(accs, tid);
            __syncthreads();
        }
        ip = ip_next;
    }
    if constexpr (STATS) atomicMax(stat, (unsigned long long)__double_as_longlong(dev));   // non-negative doubles order like their bit patterns
    for (int b = 0; b < (live1 ? 2 : 1); b++) {
        const double *acc = accs + b * 2 * WN;
        if constexpr (GLWE) {   // the accumulator itself, out = [count][2N]
            u64 *g = out + (size_t)cts[b] * (2 * WN);
            static_for<0, 2>([&](auto Q) { t64::store_glwe<WN, PRE, AB>(g, acc, acc_slot, tid + W_THREADS * Q); });
            continue;
        }
        u64 *o = out + (size_t)cts[b] * (WN + 1);
        static_for<0, 2>([&](auto Q) { t64::extract_sample<WN, PRE, AB>(o, acc, acc_slot, tid + W_THREADS * Q); });
    }
}

}  // namespace

namespace bmit {

int launch_blind_rotate_wide_u2(const RotBatch &b) {
    if (b.count == 0) return 0;
    if (!shape_supported_wide_unrolled(b.prec, b.levels, b.base_log)) return (int)hipErrorInvalidValue;
    return with_levels_stats_glwe(b.levels, b.stat != nullptr, b.glwe, [&](auto L, auto STATS, auto GLWE) {
        return launch_with_lds<k_blind_rotate_wu2_t64f<L, 10, 40, STATS, GLWE>>(dim3((b.count + 1) / 2), dim3(W_THREADS), (size_t)WU2_LDS_WORDS * sizeof(double), b.s,
                                                                                b.cts, b.ids, b.luts.u(), b.key.d(), b.tab[0].d(), b.tab[1].d(), b.out, b.count, b.n, b.stat);
    });
}

}  // namespace bmit
