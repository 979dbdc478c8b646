// Shared by all 2^64-torus kernel files (bmi_kernels_t64.hip, _t64u, _t64f, _t64fu, _t64w, _t64wu, _t64wu2, _t64w2, _t64q) and the host
// (bmi_host.cpp): the limb schemes of the bootstrap key and, for the kernels (__HIPCC__ part), the steps every blind rotation
// states the same way - the word <-> exact-double conversions, the centred residue mod 2^AB, the oracle's rounding and digit
// rule, the placement of a limb's integer, and the prologue (mod-switch, test polynomial) and epilogue (sample extraction).
// All of them are force-inlined templates on the compile-time constants of the calling kernel.  What the four N = 2048 kernels
// (_t64w, _t64w2, _t64wu, _t64wu2) share beyond that, at the level of a transform - constants and accumulator layout, half
// butterflies, multiply-accumulate, key rows, powers of zeta, inverse task, `keep` - is in t64_wide_steps.hpp, built on this file;
// the N = 1024 half-transform kernels (lat_t64f, lat2u_t64f, tp2u_t64f) have t64_half_steps.hpp the same way.
//
// No transform exists mod 2^64, so a torus external product is computed EXACTLY over the integers: the digit polynomials
// (|d| <= 2^(Bg-1)) are transformed mod p = 2^49 - 720895 and multiplied with LIMBS balanced limb polynomials of every
// key word (read as a signed integer),  k = 2^PRE sum_j k_j 2^(BITS j);  per limb the sum over the 2 l N digit x limb terms
// is an integer below p / 2, so its centred residue mod p IS that integer; the limb results are recombined with shifts
// mod 2^64.  The scheme follows from the PRECISION the key is stored at (bmi_set_bsk_precision):
//
//   64 bits  3 limbs of 22 bits            the exact key; digits up to 2^14 (Bg <= 2^15): 2 l N 2^14 2^21 = 2^47.6 < p/2
//   48 bits  2 limbs of 24 bits, PRE = 16  key words rounded (half up, as signed integers) to multiples of 2^16; digits up
//                                          to 2^9 (Bg <= 2^10) leave room for the factor 6 of the UNROLLED step (three keys,
//                                          each product scaled by X^c - 1): 6 * 2 l N 2^9 2^23 = 2^47.2 < p/2.  The default
//                                          of the torus set (Bg = 2^10): 2/3 of the work of the exact key, and the rounding
//                                          error (2^15.x per word, summed over the GLWE key's set bits: 2^18.7 per row) stays
//                                          under the key noise 2^20 - output noise 2^-22.6 against 2^-19.85 of (Bg 2^15, exact)
//   42 bits  2 limbs of 21 bits, PRE = 22  round 2's throughput option at Bg = 2^15 (effective key noise 2^-39.3)
//   44 bits  2 limbs of 22 bits, PRE = 20  N = 4096 (Bg = 2^10, l = 3) through the floating-point transform only (bmi_kernels_t64q.hip,
//                                          fft_eighth_f64.hpp): the a-priori error bound of the 2,048-point transform is 0.45 at this width
//   46 bits  2 limbs of 23 bits, PRE = 18  N = 2048 (the secure128_torus set, Bg = 2^10, l = 3) through the floating-point
//                                          transform only (bmi_kernels_t64w.hip): a limb sum 2 l N 2^9 2^22 = 2^44.6 keeps the
//                                          a-priori error bound of the 1,024-point transform below 1/2 (fft_quarter_f64.hpp)
//   40 bits  2 limbs of 20 bits, PRE = 24  N = 2048 with the UNROLLED key only (bmi_kernels_t64wu.hip, _t64wu2.hip): the six-times larger limb
//                                          sums, 6 * 2 l N 2^9 2^19 = 2^44.2, keep that bound at 0.31 (21-bit limbs: 0.62)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define T64_HD __host__ __device__ __forceinline__
#else
#define T64_HD inline
#endif

namespace t64 {

typedef uint64_t u64;
typedef int64_t i64;

template <int PREC> struct Scheme;
template <> struct Scheme<64> { static constexpr int LIMBS = 3, BITS = 22, PRE = 0; };
template <> struct Scheme<48> { static constexpr int LIMBS = 2, BITS = 24, PRE = 16; };
template <> struct Scheme<42> { static constexpr int LIMBS = 2, BITS = 21, PRE = 22; };
template <> struct Scheme<46> { static constexpr int LIMBS = 2, BITS = 23, PRE = 18; };
template <> struct Scheme<44> { static constexpr int LIMBS = 2, BITS = 22, PRE = 20; };
template <> struct Scheme<40> { static constexpr int LIMBS = 2, BITS = 20, PRE = 24; };

T64_HD bool precision_ok(int prec) { return prec == 64 || prec == 48 || prec == 46 || prec == 44 || prec == 42 || prec == 40; }
T64_HD int limbs_of(int prec) { return prec == 64 ? 3 : 2; }
T64_HD int limb_bits(int prec) { return prec == 64 ? 22 : prec / 2; }
T64_HD int limb_pre(int prec) { return 64 - prec; }
// largest bootstrap base log a precision admits: 2 l N 2^(b-1) 2^(BITS-1) < p/2 at l = 3, N = 1024 means b + BITS <= 37;
// the unrolled step needs b + BITS <= 34
T64_HD int max_base_log(int prec, bool unrolled) { return (unrolled ? 34 : 37) - limb_bits(prec); }

// (The key word stored at `prec` bits of precision - rounded half up, as a signed integer, to a multiple of 2^(64 - prec) - is
// hc::round_key_word, key_set.hpp: the host rounds the key, in both libraries, and the kernels receive it rounded.)

// balanced limb j of a signed 64-bit word at precision `prec`: limb_j in [-2^(BITS-1), 2^(BITS-1)), the last one takes the rest
T64_HD i64 limb_of(i64 k, int j, int prec) {
    const int bits = limb_bits(prec), limbs = limbs_of(prec);
    const i64 B = (i64)1 << bits, H = B >> 1;
    k >>= limb_pre(prec);
    for (int t = 0; t < j; t++) {
        const i64 d = ((k + H) & (B - 1)) - H;
        k = (k - d) >> bits;
    }
    if (j == limbs - 1) return k;
    return ((k + H) & (B - 1)) - H;
}

#if defined(__HIPCC__)
// round(a * 2N / 2^64) mod 2N, ties up
template <int LOG_2N>
__device__ __forceinline__ uint32_t modswitch(u64 a) {
    return (uint32_t)(((a >> (63 - LOG_2N)) + 1) >> 1) & ((1u << LOG_2N) - 1);
}
// exact integer |v| < 2^52 held in a double -> two's complement 64-bit word
__device__ __forceinline__ u64 f64_to_word(double v) {
    const double hi = __builtin_floor(v * 0x1p-32);
    const double lo = __builtin_fma(-0x1p32, hi, v);          // in [0, 2^32)
    return ((u64)(uint32_t)(int32_t)hi << 32) | (u64)(uint32_t)lo;
}
// signed integer |t| < 2^52 held in an int64 -> double (exact)
__device__ __forceinline__ double word_to_f64(i64 t) {
    return __builtin_fma((double)(int32_t)(t >> 32), 0x1p32, (double)(uint32_t)t);
}
// The oracle's decomposition rule on a torus word (oracle/tfhe_oracle.c ora_decompose): the word as a signed integer, rounded
// half up to its top L * BG bits -> that rounded value as an exact double (the balanced digits are peeled off it in f64).
template <int L, int BG>
__device__ __forceinline__ double rounded_top(u64 v) {
    const i64 t = (i64)v >> (64 - L * BG - 1);                                   // L BG + 1 signed bits
    if constexpr (L * BG + 1 <= 32) return __builtin_floor(__builtin_fma((double)(int32_t)t, 0.5, 0.5));
    else return __builtin_floor(__builtin_fma(word_to_f64(t), 0.5, 0.5));
}

// ---- the accumulator as exact doubles: word / 2^PRE, an integer held mod 2^AB (AB = 64 - PRE <= 52) ----

// centred residue mod 2^AB of an exact integer |t| < 2^53
// (ties go to the negative end, like the two's complement reading of the u64 word: + 2^(AB-1) is - 2^(AB-1))
template <int AB>
__device__ __forceinline__ double mod_ab(double t) {
    return __builtin_fma(-(double)(1ull << AB), __builtin_floor(__builtin_fma(t, 1.0 / (double)(1ull << AB), 0.5)), t);
}
// the oracle's decomposition rule on such a value (the centred lift of a u64 difference, / 2^PRE, already reduced with mod_ab):
// rounded half up to its top L BG bits; rounded_top above is the same rule on a u64 word
template <int L, int BG, int AB>
__device__ __forceinline__ double rounded_top_f64(double dd) {
    return __builtin_floor(__builtin_fma(dd, 1.0 / (double)(1ull << (AB - L * BG)), 0.5));
}
// balanced digit `lev` (0 = most significant) of a value r rounded to L BG bits: the digits are peeled off from the least
// significant end in f64, each in [-2^(BG-1), 2^(BG-1)) (a half goes up: + 2^(BG-1) becomes - 2^(BG-1) with a carry), the
// top digit absorbing the last carry.  Operation order and unrolling are part of the contract: no reassociation.
template <int L, int BG>
__device__ __forceinline__ double peel_digit(double r, int lev) {
    double d = r;
#pragma unroll
    for (int s = L - 1; s > 0; s--) {
        const double rn = __builtin_floor(__builtin_fma(r, 1.0 / (double)(1ull << BG), 0.5));
        if (s == lev) d = __builtin_fma(-(double)(1ull << BG), rn, r);
        r = rn;
    }
    return lev == 0 ? r : d;
}
template <int L, int BG, int AB>
__device__ __forceinline__ double digit(double dd, int lev) {
    return peel_digit<L, BG>(rounded_top_f64<L, BG, AB>(dd), lev);
}

// A limb's sum comes out of the floating-point inverse transform within < 1/2 of the exact integer (|.| < 2^45; the kernels'
// static_asserts bound 2 L N terms of |digit| <= 2^(BG-1) times |limb| <= 2^(LB-1), the size the transforms' a-priori error
// bounds are stated for): its nearest integer IS that integer.  Limb 1 is then shifted into place, x 2^LB mod 2^AB, of which
// only the low AB - LB bits of the integer survive.  STATS (the test hook bmi_fft_margin_host) also records in `dev` the
// largest distance of a sum from the integer it was rounded to.
// One limb per thread, selected by j (0 or 1): that limb's contribution to the accumulator word.
template <int AB, int LB, bool STATS>
__device__ __forceinline__ double place_limb(double v, int j, double &dev) {
    double xr = __builtin_rint(v);
    if constexpr (STATS) dev = __builtin_fmax(dev, __builtin_fabs(v - xr));
    if (j == 0) return xr;
    constexpr double W = (double)(1ull << (AB - LB));
    xr = __builtin_fma(-W, __builtin_rint(xr * (1.0 / W)), xr);
    return xr * (double)(1ull << LB);
}
template <int AB, int LB>
__device__ __forceinline__ double place_limb(double v, int j) {
    double dev = 0.0;
    return place_limb<AB, LB, false>(v, j, dev);
}
// Both limbs of a coefficient in one thread: their sum.
template <int AB, int LB, bool STATS>
__device__ __forceinline__ double place_limbs(double v0, double v1, double &dev) {
    const double x0 = __builtin_rint(v0);
    double x1 = __builtin_rint(v1);
    if constexpr (STATS) dev = __builtin_fmax(dev, __builtin_fmax(__builtin_fabs(v0 - x0), __builtin_fabs(v1 - x1)));
    constexpr double W = (double)(1ull << (AB - LB));
    x1 = __builtin_fma(-W, __builtin_rint(x1 * (1.0 / W)), x1);
    return __builtin_fma(x1, (double)(1ull << LB), x0);
}

// ---- prologue and epilogue of a blind rotation ----

// Where coefficient n of an accumulator polynomial of N words sits when the words are kept split by residue mod 2^LOG_R
// (the points a lane holds of a transform split over 2^LOG_R wavefronts are of one residue); LOG_R = 0: natural order.
template <int N, int LOG_R>
struct ResidueSlot {
    __device__ __forceinline__ uint32_t operator()(uint32_t n) const { return (n & ((1u << LOG_R) - 1)) * (N >> LOG_R) + (n >> LOG_R); }
};
// an accumulator element <-> the torus word it stands for: u64 words as they are (the exact-transform kernels), doubles as
// word / 2^PRE (test polynomials are multiples of 2^PRE, host-checked; the way back reduces mod 2^AB first)
template <int PRE> __device__ __forceinline__ void set_acc(u64 &a, u64 w) { a = w; }
template <int PRE> __device__ __forceinline__ void set_acc(double &a, u64 w) { a = (double)((i64)w >> PRE); }
template <int PRE, int AB> __device__ __forceinline__ u64 acc_word(u64 a) { return a; }
template <int PRE, int AB> __device__ __forceinline__ u64 acc_word(double a) { return f64_to_word(mod_ab<AB>(a)) << PRE; }

// the n + 1 words of an LWE ciphertext, mod-switched to 2N = 2^LOG_2N, into at[] (LDS, uint16); thread tid of `threads`
template <int LOG_2N>
__device__ __forceinline__ void stage_lwe(uint16_t *at, const u64 *lwe, uint32_t n, uint32_t tid, uint32_t threads) {
    for (uint32_t i = tid; i <= n; i += threads) at[i] = (uint16_t)modswitch<LOG_2N>(lwe[i]);
}
// coefficient nn of the start accumulator (0, X^bt tv): the mask zero, the body the test polynomial tv rotated by the
// mod-switched body bt = at[n] (negacyclic: X^N = -1); acc = [mask N][body N], each in the order of `slot`
template <int N, int PRE, typename T, typename Slot>
__device__ __forceinline__ void load_test_poly(T *acc, Slot slot, const u64 *tv, uint32_t bt, uint32_t nn) {
    const uint32_t e = (nn + bt) & (2 * N - 1);
    const u64 v = tv[e & (N - 1)];
    acc[slot(nn)] = 0;
    set_acc<PRE>(acc[N + slot(nn)], (e & N) ? (u64)0 - v : v);
}
// sample extraction by thread nn < N: the LWE ciphertext of the body's constant coefficient, o[0 .. N-1] the mask read
// backwards with the negacyclic signs, o[N] the body
template <int N, int PRE, int AB, typename T, typename Slot>
__device__ __forceinline__ void extract_sample(u64 *o, const T *acc, Slot slot, uint32_t nn) {
    const u64 a0 = acc_word<PRE, AB>(acc[slot(nn)]);
    if (nn == 0) {
        o[0] = a0;
        o[N] = acc_word<PRE, AB>(acc[N + slot(0)]);
    } else {
        o[N - nn] = (u64)0 - a0;
    }
}
// The accumulator itself (the rotation kernels instantiated with GLWE = true return it): g = [mask N][body N] words in natural order,
// through the same conversion and slot map as the extraction.  One word of one polynomial (poly = its N elements) ...
template <int PRE, int AB, typename T, typename Slot>
__device__ __forceinline__ void store_glwe_word(u64 *g, const T *poly, Slot slot, uint32_t nn) {
    g[nn] = acc_word<PRE, AB>(poly[slot(nn)]);
}
// ... and coefficient nn < N of both, by one thread
template <int N, int PRE, int AB, typename T, typename Slot>
__device__ __forceinline__ void store_glwe(u64 *g, const T *acc, Slot slot, uint32_t nn) {
    store_glwe_word<PRE, AB>(g, acc, slot, nn);
    store_glwe_word<PRE, AB>(g + N, acc + N, slot, nn);
}
#endif

}  // namespace t64
