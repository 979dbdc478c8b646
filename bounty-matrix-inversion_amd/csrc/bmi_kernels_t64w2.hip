// 2^64 TORUS at N = 2048, THROUGHPUT form: two ciphertexts per workgroup sharing every key word a thread loads (gfx950).
//
// Same function and the same words as k_blind_rotate_w_t64f (bmi_kernels_t64w.hip: key at 46 bits of precision = two balanced
// 23-bit limbs, digits in base 2^10, accumulator the exact integer word / 2^18 in a double, limb sums through the folded
// 1,024-point complex FFT of fft_quarter_f64.hpp and ROUNDED TO THE NEAREST INTEGER).  What changes is the arrangement: that kernel
// keeps all 2 l digit transforms of a CMUX in LDS (96 KB of tiles: one ciphertext per compute unit) and a CMUX takes in 393 KB of
// key for ONE ciphertext.  Here a CMUX walks the decomposition levels as the N = 4096 kernel does (bmi_kernels_t64q.hip) - one
// level's tiles in LDS, the running sums in registers across the levels - which leaves room for a SECOND ciphertext, and every
// key word is multiplied with both (half the key bytes per bootstrap: the batches a server runs, bmi dispatch for count > 256).
//   for each level:  A  16 forward tasks (ciphertext, component c, quarter h): rotate / decompose 512 coefficients, digit `level`,
//                       forward quarter -> tile (slot order, times W_h)
//                    B  all 1,024 threads = (slot, output polynomial, limb): per row and ciphertext the radix-4 butterfly over the
//                       four tiles and four complex multiply-accumulates with this thread's key words (loaded once)
//   then per ciphertext the inverse butterfly, and per limb: the sums to LDS (over the tiles), 16 inverse tasks (ciphertext, output,
//   quarter): conj W_h, inverse quarter, nearest integer, shift into place, plain read-modify-write of the accumulator.
#include <hip/hip_runtime.h>

#include <atomic>

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

constexpr int W2_TILE_CPLX = 2 * 2 * 4 * WQ;     // one level's tiles [ciphertext 2][component 2][quarter 4][256]; one limb's sums overlay them
// LDS (doubles): tables | accumulators [ciphertext 2][component 2][residue 4][512] | tiles | mod-switched LWE words of both
constexpr int W2_LDS_WORDS = fftq::QT_WORDS + 2 * 2 * WN + 2 * W2_TILE_CPLX + 2 * BMI_AT_WORDS;
static_assert(W2_LDS_WORDS <= BMI_LDS_WORDS_MAX, "W2_LDS_WORDS exceeds the 160 KB of LDS");

// sum_h i^(h t) q_h in q[t]  (INV: i^(-h t))
template <bool INV>
__device__ __forceinline__ void dft4(C (&q)[4]) {
    const C a0{q[0].r + q[2].r, q[0].i + q[2].i}, a1{q[0].r - q[2].r, q[0].i - q[2].i};
    const C b0{q[1].r + q[3].r, q[1].i + q[3].i}, b1{q[1].r - q[3].r, q[1].i - q[3].i};
    q[0] = C{a0.r + b0.r, a0.i + b0.i};
    q[2] = C{a0.r - b0.r, a0.i - b0.i};
    // i b1 = (-b1.i, b1.r)
    const C p{a1.r - b1.i, a1.i + b1.r}, m{a1.r + b1.i, a1.i - b1.r};
    q[1] = INV ? m : p;
    q[3] = INV ? p : m;
}

// standard-domain GGSW polynomials (u64 torus words, already rounded to the key precision) -> per (polynomial, limb) 1,024 complex
// words A_k / 2 as [t 4][slot 256]: frequency kappa(slot) + 256 t.  One workgroup of four wavefronts (the quarters) per item.
__global__ void __launch_bounds__(256) k_bsk_to_w2_t64(const u64 *__restrict__ std_polys, double *__restrict__ w2_polys,
                                                       const double *__restrict__ g_tw, uint32_t n_polys, int prec) {
    const int limbs = t64::limbs_of(prec);
    __shared__ double lds[fftq::QT_WORDS + 4 * WQ * 2];
    for (int i = threadIdx.x; i < fftq::QT_WORDS; i += blockDim.x) lds[i] = g_tw[i];
    __syncthreads();
    const int h = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t item = blockIdx.x;
    const uint32_t poly = item / limbs;
    const int j = (int)(item % limbs);
    double2 *tile = reinterpret_cast<double2 *>(lds + fftq::QT_WORDS);
    key_limb_to_tile(tile, std_polys, poly, j, prec, h, lane, lds);
    __syncthreads();
    {
        const int p = threadIdx.x;
        C q[4];
        static_for<0, 4>([&](auto H) {
            const double2 t = tile[H * WQ + p];
            q[H] = C{t.x, t.y};
        });
        dft4<false>(q);
        double2 *o = reinterpret_cast<double2 *>(w2_polys + (size_t)item * WN);
        static_for<0, 4>([&](auto T) { o[T * WQ + p] = double2{0.5 * q[T].r, 0.5 * q[T].i}; });
    }
}

// GLWE: the kernel returns the accumulator itself, out = [count][2N], instead of the extracted sample, out = [count][N + 1]
template <int L, int BG, int PREC, bool GLWE>
__global__ void __launch_bounds__(W_THREADS)
    k_blind_rotate_w2_t64f(const u64 *__restrict__ small_cts, const uint32_t *__restrict__ lut_ids, const u64 *__restrict__ luts,
                           const double *__restrict__ bsk_w2, const double *__restrict__ g_tw, u64 *__restrict__ out, uint32_t count,
                           uint32_t n) {
    constexpr int LIMBS = Scheme<PREC>::LIMBS, LB = Scheme<PREC>::BITS, PRE = Scheme<PREC>::PRE, AB = 64 - PRE;
    static_assert(2.0 * L * WN * (double)(1ull << (BG - 1)) * (double)(1ull << (LB - 1)) <= 0x1p45, "limb sums must stay below 2^45");
    static_assert(LIMBS == 2 && L <= W_MAX_L && L * BG < AB, "two limbs, at most three levels");
    extern __shared__ double lds[];
    double *accs = lds + fftq::QT_WORDS;                                    // [ciphertext][2 components][4 residues][512]: word / 2^PRE, exact
    double2 *tiles = reinterpret_cast<double2 *>(accs + 2 * 2 * WN);        // [ciphertext 2][component 2][quarter 4][256 slots] of the current level
    double2 *SD = tiles;                                                    // one limb's sums [ciphertext 2][output 2][quarter 4][256 slots]
    uint16_t *at = reinterpret_cast<uint16_t *>(tiles + W2_TILE_CPLX);      // [ciphertext 2][BMI_AT_WORDS * 4]
    constexpr int AT_STRIDE = BMI_AT_WORDS * 4;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < fftq::QT_WORDS; i += W_THREADS) lds[i] = g_tw[i];
    // the two ciphertexts of this workgroup (an odd batch: the last workgroup runs its one ciphertext twice and writes it once)
    uint32_t cts[2];
    const bool live1 = ciphertext_pair(cts, blockIdx.x, count);
    for (int b = 0; b < 2; b++) {
        const u64 *lwe = small_cts + (size_t)cts[b] * (n + 1);
        // (t64::stage_lwe written out: handing it at + b * AT_STRIDE turns the guard of the step loop around in the generated code)
        for (uint32_t i = tid; i <= n; i += W_THREADS) at[b * AT_STRIDE + i] = (uint16_t)t64::modswitch<WLOG + 1>(lwe[i]);
    }
    __syncthreads();
    for (int b = 0; b < 2; b++) {   // (t64w::load_start_acc per ciphertext: 12 B of scratch per lane)
        const u64 *tv = luts + (size_t)(lut_ids[cts[b]] & (BMI_LUT_CAP - 1)) * WN;
        const uint32_t bt = at[b * AT_STRIDE + n];
        double *acc = accs + b * 2 * WN;
        static_for<0, 2>([&](auto Q) { t64::load_test_poly<WN, PRE>(acc, acc_slot, tv, bt, tid + W_THREADS * Q); });
    }
    __syncthreads();
    // phase B: slot, output polynomial, limb (the four combinations of a slot sit 16 lanes apart: their tile reads coincide)
    const int slot = wave * 16 + (lane & 15), mo = lane >> 5, mj = (lane >> 4) & 1;
    // phases A and C: wavefront = (ciphertext, component / output, quarter)
    const int wb = wave >> 3, wc = (wave >> 2) & 1, wh = wave & 3;
    uint32_t since_centred = 0;

    for (uint32_t i = 0; i < n; i++) {
        const uint32_t a_own = at[wb * AT_STRIDE + i];                       // this wavefront's ciphertext (phase A)
        if ((at[i] | at[AT_STRIDE + i]) == 0) continue;                      // uniform over the workgroup: neither ciphertext rotates
        // key words of this thread: [row 2L][output 2][limb][t 4][256 slots] complex
        const double2 *kth = reinterpret_cast<const double2 *>(bsk_w2 + (size_t)i * 4 * L * LIMBS * WN) + ((size_t)mo * LIMBS + mj) * (WN / 2) + slot;
        auto row_ptr = [&](int R) { return kth + (size_t)R * 2 * LIMBS * (WN / 2); };
        C y[2][4];
        static_for<0, 2>([&](auto B) { static_for<0, 4>([&](auto T) { y[B][T] = C{0.0, 0.0}; }); });
        double2 kw[2][4];
        static_for<0, L>([&](auto LEV) {
            constexpr int lev = LEV;
            {   // phase A
                const double *ac = accs + wb * 2 * WN + wc * WN;
                double x[8];   // re[r] = x[r], im[r] = x[r + 4]
                static_for<0, 2>([&](auto G) {   // four coefficients at a time, fenced
                    rotated_diff_digits<L, BG, AB, G>(x, ac, wh, lane, a_own, lev);
                    pin();
                });
                // (written out in all four kernels: inlined through a helper, the transform's own instructions come in another order)
                const double re[4] = {x[0], x[1], x[2], x[3]}, im[4] = {x[4], x[5], x[6], x[7]};
                C v[4];
                fftq::forward_quarter(wh, re, im, v, lane, lds);
                double2 *tile = tiles + (size_t)wave * WQ;     // wave = (ciphertext 2, component 2, quarter 4)
                static_for<0, 4>([&](auto R4) { tile[R4 * 64 + lane] = double2{v[R4].r, v[R4].i}; });
            }
            // this thread's key words of the level's two rows (component 0 / 1): they land under the barrier (requested during
            // the level before instead: 48 B of scratch per lane, 14.77 against 13.45 ms per 512)
            static_for<0, 2>([&](auto CC) { static_for<0, 4>([&](auto T) { kw[CC][T] = row_ptr(CC * L + lev)[T * WQ]; }); });
            pin();
            __syncthreads();
            static_for<0, 2>([&](auto CC) {   // rows (component CC, this level)
                static_for<0, 2>([&](auto B) {
                    C q[4];
                    static_for<0, 4>([&](auto H) {
                        const double2 t = tiles[(size_t)((B * 2 + CC) * 4 + H) * WQ + slot];
                        q[H] = C{t.x, t.y};
                    });
                    dft4<false>(q);   // frequency kappa + 256 t in q[t]
                    static_for<0, 4>([&](auto T) {
                        y[B][T].r = __builtin_fma(q[T].r, kw[CC][T].x, __builtin_fma(-q[T].i, kw[CC][T].y, y[B][T].r));
                        y[B][T].i = __builtin_fma(q[T].r, kw[CC][T].y, __builtin_fma(q[T].i, kw[CC][T].x, y[B][T].i));
                    });
                });
                keep(y);
                pin();
            });
            __syncthreads();   // every thread has read this level's tiles: the next level (or the sums) may overwrite them
        });
        static_for<0, 2>([&](auto B) { dft4<true>(y[B]); });   // sum_t i^(-h t) Y_t in y[b][h]; conj W_h is applied by the inverse task
        static_for<0, LIMBS>([&](auto J) {
            if (mj == J) {
                static_for<0, 2>([&](auto B) {
                    static_for<0, 4>([&](auto H) { SD[(size_t)((B * 2 + mo) * 4 + H) * WQ + slot] = double2{y[B][H].r, y[B][H].i}; });
                });
            }
            __syncthreads();
            {
                const double2 *sd = SD + (size_t)wave * WQ;     // wave = (ciphertext, output, quarter)
                C v[4];
                static_for<0, 4>([&](auto R) {
                    const double2 t = sd[R * 64 + lane];
                    v[R] = C{t.x, t.y};
                });
                if (wh != 0) {   // (uniform over the wavefront) conj W_h
                    const double2 *w = reinterpret_cast<const double2 *>(lds + fftq::w_offset(wh));
                    static_for<0, 4>([&](auto R) {
                        const double2 t = w[R * 64 + lane];
                        v[R] = fftq::cmul<true>(v[R], t.x, t.y);
                    });
                }
                double dev = 0.0;   // (no statistics in this kernel)
                inverse_task_limb<AB, LB, false>(accs + wb * 2 * WN + wc * WN, wh, v, J, lane, lds, dev);
            }
            __syncthreads();
        });
        if (++since_centred == W_RECENTRE) {   // (uniform: counts the steps actually taken)
            since_centred = 0;
            recentre<AB, 8>(accs, tid);
            __syncthreads();
        }
    }
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

int launch_bsk_to_wide2(const KeyConv &k) {
    if (k.prec != 46) return (int)hipErrorInvalidValue;
    const uint32_t items = k.n_polys * (uint32_t)t64::limbs_of(k.prec);
    hipLaunchKernelGGL(k_bsk_to_w2_t64, dim3(items), dim3(256), 0, k.s, k.std_polys, (double *)k.dst, k.tab[0].d(), k.n_polys, k.prec);
    BMI_LAUNCH_CHECK();
    return 0;
}

int launch_blind_rotate_wide2(const RotBatch &b) {
    if (b.count == 0) return 0;
    if (!shape_supported_wide(b.prec, b.levels, b.base_log)) return (int)hipErrorInvalidValue;
    return with_levels_glwe(b.levels, b.glwe, [&](auto L, auto GLWE) {
        return launch_with_lds<k_blind_rotate_w2_t64f<L, 10, 46, GLWE>>(dim3((b.count + 1) / 2), dim3(W_THREADS), (size_t)W2_LDS_WORDS * sizeof(double), b.s,
                                                                        b.cts, b.ids, b.luts.u(), b.key.d(), b.tab[0].d(), b.out, b.count, b.n);
    });
}

}  // namespace bmit
