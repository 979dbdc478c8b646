// Internal declarations shared by every kernel TU (bmi_kernels*.hip) and the host TU (bmi_host.cpp): tunables and LDS limits,
// the launch scaffolding of the kernel TUs, and the launchers the host calls (one namespace per modulus).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "goldilocks.hpp"
#include "rotation_plan.hpp"

#ifndef BMI_TPX49_PF
#define BMI_TPX49_PF 13  // exchange-once kernel: where the two GGSW rows of a level are requested (see the kernel)
#endif

#ifndef BMI_TPX49_RESYNC
#define BMI_TPX49_RESYNC 4  // workgroup barrier every so many CMUX iterations (0: never): keeps the four pairs on the same key rows, which they share through L1 (83.5 -> 80.6 ms)
#endif

// Capacity of a context's look-up table buffer (tables of N words, allocated at creation).  A power of two: the kernels
// mask the ids they are handed with it, so that a wrong id in a device-resident id array reads a wrong (possibly
// unregistered) table instead of faulting; the host-buffer entry points refuse unknown ids outright.
#define BMI_LUT_CAP 1024
// Largest small-LWE dimension n the blind-rotation kernels take: every kernel stages the n + 1 mod-switched words of a
// ciphertext in LDS as uint16 (BMI_AT_WORDS 8-byte words per ciphertext).
#define BMI_MAX_LWE_N 1024
constexpr int BMI_AT_WORDS = 264;   // 1,056 uint16 slots >= BMI_MAX_LWE_N + 1
constexpr int BMI_LDS_WORDS_MAX = 160 * 1024 / 8;   // 160 KB of LDS per workgroup on gfx950
#ifndef BMI_KS_MFMA_MIN
#define BMI_KS_MFMA_MIN 1  // smallest batch that takes the matrix-core keyswitch (0.05 ms against 0.14 ms scalar even at one ciphertext)
#endif

// Scalar keyswitch (ks_lincomb.hpp): a workgroup stages one byte per (ciphertext of its tile of 8, coefficient of its slice, level)
// in dynamic LDS.  The kernel is launched without raising its dynamic-LDS limit, so a request stays within the 64 KiB every kernel
// has by default: bmi_keyswitch_batch picks `slices` accordingly and the launcher refuses anything larger before launching.
constexpr int BMI_KS_TILE = 8;
constexpr size_t BMI_KS_LDS_MAX = 64 * 1024;
inline size_t ks_scalar_lds_bytes(uint32_t big_n, uint32_t levels, uint32_t slices) {
    const uint32_t per = slices > 1 ? (big_n + slices - 1) / slices : big_n;
    return (size_t)BMI_KS_TILE * per * levels;
}

#ifndef BMI_TP_CTS
#define BMI_TP_CTS 2  // ciphertexts (= wavefront pairs) per workgroup in the throughput blind rotation
#endif

// hipFuncSetAttribute acts on the current device only: remember per kernel which devices have been configured
// (several contexts on several GPUs may live in one process).
#include <atomic>
#include <type_traits>
inline int set_max_dynamic_lds(const void *kernel, size_t bytes, std::atomic<uint64_t> &done_devices) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (dev < 64 && ((done_devices.load() >> dev) & 1)) return 0;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
    if (dev < 64) done_devices.fetch_or((uint64_t)1 << dev);
    return 0;
}

// after a kernel launch, inside a launcher returning int: the launch error, if any, is the launcher's result
#define BMI_LAUNCH_CHECK()                      \
    do {                                        \
        hipError_t e__ = hipGetLastError();     \
        if (e__ != hipSuccess) return (int)e__; \
    } while (0)

// Launch of a kernel that takes more dynamic LDS than the default limit.  KERN is a template parameter so that every kernel
// instantiation has its own "configured on these devices" flag.
template <auto KERN>
inline std::atomic<uint64_t> &lds_configured() {
    static std::atomic<uint64_t> configured{0};
    return configured;
}
template <auto KERN, typename... Args>
inline int launch_with_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, Args... args) {
    if (int rc = set_max_dynamic_lds(reinterpret_cast<const void *>(KERN), lds_bytes, lds_configured<KERN>())) return rc;
    hipLaunchKernelGGL(KERN, grid, block, lds_bytes, s, args...);
    BMI_LAUNCH_CHECK();
    return 0;
}

// The runtime (levels, statistics wanted) of the floating-point-transform families -> their instantiations: calls
// f(L, STATS) with L = std::integral_constant<int, 3 or 2> (the callers have checked the shape) and STATS = std::true_type
// or std::false_type, usable as template arguments.  The kernels without a STATS form take with_levels alone, or
// with_levels_glwe: f(L, GLWE), GLWE the epilogue flag described below.
template <typename F>
inline int with_levels(uint32_t levels, F f) {
    if (levels == 3) return f(std::integral_constant<int, 3>{});
    return f(std::integral_constant<int, 2>{});
}
template <typename F>
inline int with_levels_stats(uint32_t levels, bool stats, F f) {
    return with_levels(levels, [&](auto L) { return stats ? f(L, std::true_type{}) : f(L, std::false_type{}); });
}
template <typename F>
inline int with_levels_glwe(uint32_t levels, bool glwe, F f) {
    return with_levels(levels, [&](auto L) { return glwe ? f(L, std::true_type{}) : f(L, std::false_type{}); });
}

// The (levels, base log) of the 49-bit field's templated kernels -> their instantiations: calls f(L, BG) with
// std::integral_constant<int, .> for (3, 15), (2, 15) and (1, 23); any other shape is refused.
template <typename F>
inline int with_shape49(uint32_t levels, uint32_t base_log, F f) {
    if (levels == 3 && base_log == 15) return f(std::integral_constant<int, 3>{}, std::integral_constant<int, 15>{});
    if (levels == 2 && base_log == 15) return f(std::integral_constant<int, 2>{}, std::integral_constant<int, 15>{});
    if (levels == 1 && base_log == 23) return f(std::integral_constant<int, 1>{}, std::integral_constant<int, 23>{});
    return (int)hipErrorInvalidValue;
}

// ... and the epilogue of the torus FFT rotations (bmi_kernels_t64{f,fu,w,wu,wu2,w2,q}.hip), whose trailing template flag GLWE makes
// them return the accumulator itself (t64::store_glwe, out = [count][2N]) instead of the extracted sample (t64::extract_sample,
// out = [count][N + 1]); everything up to the end of the CMUX loop is the same text.  Calls f(L, STATS, GLWE).  The accumulator
// form is instantiated without statistics only: asked for both, the launcher returns hipErrorInvalidValue.  (Two families share
// their steps through a header - the four N = 2048 kernels through t64_wide_steps.hpp, the three N = 1024 half-transform kernels
// of bmi_kernels_t64{f,fu}.hip through t64_half_steps.hpp - but each kernel keeps this epilogue written out: behind a helper it
// renumbers the step loop's registers of the N = 2048 kernels, profiles/wide_steps_ab.txt; at N = 1024 a helper was not tried.)
template <typename F>
inline int with_levels_stats_glwe(uint32_t levels, bool stats, bool glwe, F f) {
    if (!glwe) return with_levels_stats(levels, stats, [&](auto L, auto STATS) { return f(L, STATS, std::false_type{}); });
    if (stats) return (int)hipErrorInvalidValue;
    return with_levels(levels, [&](auto L) { return f(L, std::false_type{}, std::true_type{}); });
}

// ------------------------------------------------------------------------------------------ what the host hands the launchers
// Device words are u64 on Goldilocks (and the test polynomials of the torus) and doubles elsewhere, 8 bytes either way.  The host
// carries test polynomials, key copies and tables untyped, as DevWords; a launcher names the type its kernel declares, .u() or
// .d().  This is the one place where the two element types meet.
struct DevWords {
    const void *p = nullptr;
    const gl::u64 *u() const { return static_cast<const gl::u64 *>(p); }
    const double *d() const { return static_cast<const double *>(p); }
};

// A batch to rotate: the one argument of every launch_blind_rotate_*.  launch_rotation (bmi_host.cpp) fills key and tab from the
// kernel's row (rotplan::row(rot): its key copy, its tables in the order the kernel takes them).
struct RotBatch {
    const gl::u64 *cts;         // [count][n + 1] small ciphertexts
    const uint32_t *ids;        // [count] ids of the test polynomials
    DevWords luts;              // BMI_LUT_CAP test polynomials of N words (49-bit field: centred doubles)
    DevWords key, tab[3];
    gl::u64 *out;               // [count][N + 1] extracted samples
    uint32_t count, n;
    int prec;                   // torus: the precision the key is stored at
    uint32_t levels, base_log;  // of the bootstrap decomposition
    // stat (may be null; the kernels of a row with the stat flag): receives, as the bit pattern of a double, the largest distance of
    // a limb sum from the integer it was rounded to
    unsigned long long *stat;
    // glwe (the kernels of a row with the accumulator flag): out receives the ACCUMULATOR, [count][mask N][body N] words in natural
    // order, instead of the extracted samples [count][N + 1]; stat must be null
    bool glwe;
    hipStream_t s;
};

// A key to convert: the one argument of every launch_bsk_to_*.  dst = one key copy (rotplan::Copy) of the n_polys standard-domain
// polynomials std_polys; tab = the tables of the copy's row; prec: the torus; paired: the 49-bit launch_bsk_to_lat.
struct KeyConv {
    const gl::u64 *std_polys;
    void *dst;
    DevWords tab[2];
    uint32_t n_polys;
    int prec;
    bool paired;
    hipStream_t s;
};

// The launchers that differ by modulus only, instantiated once per field policy (field_ops.hpp): each of bmi_kernels.hip,
// bmi_kernels_f64.hip and bmi_kernels_t64.hip exports one table, bmi_ctx_create picks one per context.
struct FieldOps {
    // slices > 1 (with a partial buffer of slices * count * ks_stride 16-byte words): latency form for small batches
    // ks_bias[col] = (B/2) * sum over all rows of ksk[row][col] mod q (the digits are staged unsigned, d + B/2)
    int (*keyswitch)(const gl::u64 *in, const gl::u64 *ksk, const gl::u64 *ks_bias, gl::u64 *out, void *partial, uint32_t slices,
                     uint32_t count, uint32_t n, uint32_t big_n, uint32_t levels, uint32_t base_log, uint32_t ks_stride, hipStream_t s);
    // Keyswitch on the matrix cores (ks_mfma.hpp): the key as ks_limbs balanced base-256 limbs in MFMA operand order,
    // digits = count * big_n * levels bytes, sums = slices * count * ks_limbs * ceil((n+1)/32)*32 int32 words.
    int (*ksk_to_limbs)(const gl::u64 *ksk, signed char *limbs, uint32_t rows, uint32_t n, uint32_t ks_stride, uint32_t ks_limbs, hipStream_t s);
    int (*keyswitch_mfma)(const gl::u64 *in, const signed char *limbs, signed char *digits, int *sums, gl::u64 *out, uint32_t slices,
                          uint32_t count, uint32_t n, uint32_t big_n, uint32_t levels, uint32_t base_log, hipStream_t s);
    int (*lincomb)(const gl::u64 *store, const uint32_t *row_ptr, const uint32_t *idx, const gl::i64 *coef, const gl::u64 *const_body,
                   gl::u64 *out, uint32_t count, uint32_t width, hipStream_t s);
    // lwe_phase.hpp: phase (and, with msgs, the decoded message and the signed error) of big-key ciphertexts; key_mask = the big
    // secret key as big_n / 64 words of bits
    int (*lwe_phase)(const gl::u64 *ct, const gl::u64 *key_mask, gl::u64 *phase, const gl::i64 *expected, gl::i64 *msgs, gl::i64 *err,
                     uint32_t count, uint32_t big_n, uint32_t delta_log, hipStream_t s);
    // the NTT test hook: on the prime fields only (null on the torus); g_tw = the field's own twiddle table (tw_gl / tw_wave)
    int (*negacyclic_mul)(const gl::u64 *a, const gl::u64 *b, gl::u64 *c, DevWords g_tw, uint32_t count, hipStream_t s);
    uint32_t ks_limbs;   // limbs per keyswitch-key word of the matrix-core keyswitch (9; the 49-bit field: 7)
};

// Goldilocks (bmi_kernels.hip): key copy, twiddles and test polynomials are u64
namespace bmi {
using gl::i64;
using gl::u64;

extern const FieldOps OPS;
int launch_bsk_to_ntt(const KeyConv &k);
int launch_blind_rotate_tp(const RotBatch &b);
int launch_blind_rotate_lat(const RotBatch &b);
// store[rows[i]] = src[i] (rows of `width` words); field independent
int launch_scatter_rows(const u64 *src, u64 *store, const uint32_t *rows, uint32_t count, uint32_t width, hipStream_t s);
// modswitch_centre.hip: out = the `count` small ciphertexts in ([count][n + 1], may be the same buffer) with the body minus half the
// sum of the mask words' rounding errors to the 2N positions; torus: q = 2^64, else the 49-bit field (Goldilocks has no such kernel)
int launch_modswitch_centre(const u64 *in, u64 *out, uint32_t count, uint32_t n, uint32_t log_N, bool torus, hipStream_t s);
// chacha_expand.hip (2^64 torus: seeded keys and ciphertexts): row r < rows receives, at base + r * pitch, the first words_per_row
// words of the ChaCha20 stream (key, nonce (domain << 56) | (first_row + r)) - what bmi_seeded_mask_words returns for that nonce;
// pitch >= words_per_row, domain < 256, rows of any 8-byte alignment; rows == 0 launches nothing
int launch_chacha_expand(u64 *base, u64 pitch, uint32_t words_per_row, u64 rows, const uint32_t key[8], u64 domain, u64 first_row,
                         hipStream_t s);
// ... and base[r * pitch + j] = bodies[r * w + j] for j < w: the compact body words into their slots behind the masks
int launch_place_bodies(const u64 *bodies, u64 *base, u64 pitch, uint32_t w, u64 rows, hipStream_t s);
}  // namespace bmi

// The same launchers for the 49-bit field (bmi_kernels_f64.hip): NTT-domain key, twiddles and test polynomials are f64.
namespace bmi49 {
using gl::i64;
using gl::u64;
extern const FieldOps OPS;
// (levels, base log) of the bootstrap decomposition: (3, 15), (2, 15) and (1, 23) are instantiated in the kernels of N <= 2048;
// the 49-bit N = 4096 kernel and the Goldilocks ones take (3, 15) only
int launch_bsk_to_ntt(const KeyConv &k);          // tab = tw_wave
int launch_blind_rotate_tpx(const RotBatch &b);   // key ntt49; tab = tw_wave
// third parameter set N = 4096: key copy in slot order (scaled by 1/4); tab = tw_wave, then T_1, T_2, T_3 and their inverses ([6][1024])
int launch_bsk_to_quad(const KeyConv &k);
int launch_blind_rotate_quad(const RotBatch &b);
// second parameter set N = 2048: key copy in slot order (scaled by 1/2); tab = tw_wave, then T / T^-1 of the even/odd combination
int launch_bsk_to_wide(const KeyConv &k);
int launch_blind_rotate_wide(const RotBatch &b);
// N = 2048 with the unrolled key: key = launch_bsk_to_wide of the unrolled key, tab[2] = psi_4096^x for x in [0, 2048)
int launch_blind_rotate_wide_u(const RotBatch &b);
// latency kernel, two wavefronts per transform (ntt_half_f64.hpp): own key copy in slot order, own twiddle tables (tab = tw_half)
// paired: A_lo[p], A_hi[p] side by side (one 16-byte request per slot; the unrolled kernel's layout), else [A_lo 512][A_hi 512]
int launch_bsk_to_lat(const KeyConv &k);
int launch_blind_rotate_lat2(const RotBatch &b);
// the same with the unrolled key (two LWE coefficients per step): key = [ceil(n/2)][3 keys] GGSW copies in the PAIRED slot
// order of launch_bsk_to_lat, tab[1] = psi^x for x in [0, 2N) as centred doubles
int launch_blind_rotate_lat2u(const RotBatch &b);
}  // namespace bmi49

// The 2^64 torus (bmi_kernels_t64*.hip): ciphertexts, test polynomials and keyswitch key are plain u64
// words; the bootstrap key is LIMBS transform-domain f64 limb polynomials per key polynomial ([poly][limb][N]); the limb
// scheme follows from the precision `prec` (64, 48, 46, 44, 42 or 40 bits) the key is stored at (t64_common.hpp).
namespace bmit {
using gl::i64;
using gl::u64;
extern const FieldOps OPS;
// (the (precision, levels, base log) combinations with instantiated kernels: bmit::shape_supported*, rotation_plan.hpp)
// exact transform mod 2^49 - 720895, wave pairs (bmi_kernels_t64.hip): tab = tw_wave
int launch_bsk_to_limbs(const KeyConv &k);
int launch_blind_rotate(const RotBatch &b);
// latency form (one workgroup of 16 wavefronts per ciphertext): own key copy, per limb in the slot order of the two-wave
// half transform ([poly][limb][512 slots][A_lo, A_hi]); tables of ntt_half_f64.hpp
int launch_bsk_to_lat(const KeyConv &k);
int launch_blind_rotate_lat(const RotBatch &b);
// the same with the unrolled key (two LWE coefficients per step; bmi_kernels_t64u.hip): key = launch_bsk_to_lat of the
// unrolled key [ceil(n/2)][3 keys] GGSW copies, tab[1] = psi^x (mod 2^49 - 720895) for x in [0, 2N) as centred doubles
int launch_blind_rotate_lat2u(const RotBatch &b);
// wave pairs with the exact limb products carried by the folded complex FFT (bmi_kernels_t64f.hip, fft_wave_f64.hpp): key copy
// [poly][limb][8 registers][64 lanes] complex words; tables fftw::TW_WORDS doubles; same results as launch_blind_rotate
int launch_bsk_to_fft(const KeyConv &k);
int launch_blind_rotate_fft(const RotBatch &b);
// latency form (one workgroup of 16 wavefronts per ciphertext, half transforms: fft_half_f64.hpp): own key copy, per (polynomial,
// limb) 256 slots of [F_k, F_{k+256}]; tables ffth::HT_WORDS doubles
int launch_bsk_to_latf(const KeyConv &k);
int launch_blind_rotate_lat_fft(const RotBatch &b);
// the unrolled step (two LWE coefficients) through the floating-point transform (bmi_kernels_t64fu.hip): key at 42 bits of precision
// (two 21-bit limbs: the six-times larger limb sums stay inside the transform's certified range); key = launch_bsk_to_latf of
// the unrolled key, tab[1] = exp(i pi x / 1024) for x in [0, 1024) as (re, im)
int launch_blind_rotate_lat2u_fft(const RotBatch &b);
// ... and its throughput form: two ciphertexts per workgroup, every key word a thread loads multiplied with both (same words)
int launch_blind_rotate_tp2u_fft(const RotBatch &b);
// N = 4096 (bmi_kernels_t64q.hip, fft_eighth_f64.hpp): key at 44 bits of precision (two 22-bit limbs), one workgroup per ciphertext,
// one decomposition level of tiles in LDS at a time; key copy per (polynomial, limb) [t 8][256 slots] complex words A_k / 4; tables
// ffte::ET_WORDS doubles
int launch_bsk_to_quad(const KeyConv &k);
int launch_blind_rotate_quad(const RotBatch &b);
// N = 2048, throughput form (bmi_kernels_t64w2.hip): two ciphertexts per workgroup, every key word multiplied with both; its own key copy,
// per (polynomial, limb) [t 4][256 slots] complex words A_k / 2; tables and results as launch_blind_rotate_wide
int launch_bsk_to_wide2(const KeyConv &k);
int launch_blind_rotate_wide2(const RotBatch &b);
// N = 2048 (bmi_kernels_t64w.hip, fft_quarter_f64.hpp): key at 46 bits of precision (two 23-bit limbs), one workgroup of 16
// wavefronts per ciphertext (auto dispatch: up to 256 ciphertexts; launch_blind_rotate_wide2 beyond); key copy per (polynomial, limb)
// 1,024 complex words A_k / 2 in the order of the multiplying threads; tables fftq::QT_WORDS doubles
int launch_bsk_to_wide(const KeyConv &k);
int launch_blind_rotate_wide(const RotBatch &b);
// N = 2048 with the unrolled key (bmi_kernels_t64wu.hip): key at 40 bits of precision (two 20-bit limbs: the six-times larger limb sums
// stay inside the transform's certified range), one workgroup per ciphertext (auto dispatch: up to 256 ciphertexts;
// launch_blind_rotate_wide_u2 beyond); key = launch_bsk_to_wide of the unrolled key [ceil(n/2)][3 keys][2 l rows][2] polynomials at
// prec = 40, tab[1] = exp(i pi x / 2048) for x in [0, 512] as (re, im)
int launch_blind_rotate_wide_u(const RotBatch &b);
// ... and its throughput form (bmi_kernels_t64wu2.hip): two ciphertexts per workgroup, every key word a thread loads multiplied with
// both, one decomposition level of tiles in LDS at a time; the SAME key copy and tables, the same words
int launch_blind_rotate_wide_u2(const RotBatch &b);
// glwe_lookup.hip: the look-ups of groups that share one rotation.  glwe = [groups][2N] accumulators of a rotation of the groups'
// base polynomials; group g serves the tables lut_ids[group_ptr[g] .. group_ptr[g+1]) and writes their LWE rows out[t] (N + 1
// words) = SampleExtract_0(ACC_g * P_t), P_t the table's sparse factor scaled by 2^(its scale - the scale of base_ids[g]).
// sparse_head = [BMI_LUT_CAP] {entries, scale}, sparse = [BMI_LUT_CAP][BMI_SPARSE_CAP] {position, coefficient} (bmi_lut_register).
constexpr uint32_t BMI_SPARSE_CAP = 64;   // entries of a table's sparse factor: 2^msg_bits, so msg_bits <= 6 share a rotation
int launch_glwe_lookup(const u64 *glwe, const uint32_t *group_ptr, const uint32_t *base_ids, const uint32_t *lut_ids,
                       const uint2 *sparse_head, const int2 *sparse, u64 *out, uint32_t groups, uint32_t total, uint32_t N,
                       hipStream_t s);
// lwe_pack.hip: compression of output ciphertexts (LWE-to-GLWE packing keyswitch, then a centred modulus switch).
// pack_slice = the most ciphertexts one launch_pack_slice takes (its T scratch is then 16 MB).  launch_pack_slice: the m
// ciphertexts cts [m][N + 1], numbers first .. first + m of their block, are decomposed (digits = m * N * levels uint32 words),
// multiplied with the compression key (key = [N * levels][2N] words, standard layout; bias[col] = 2^(base_log - 1) * the sum of the
// key's column col; T = m * 2N words) and their rotations X^i T_i are added to acc = [A: N][B: N] (first == 0 initialises it).
// launch_pack_switch: acc -> out = N mask values then m body values of log_modulus bits, by the centred switch.
uint32_t pack_slice(uint32_t N);
int launch_pack_slice(const u64 *cts, const u64 *key, const u64 *bias, uint32_t *digits, u64 *T, u64 *acc, uint32_t m, uint32_t first,
                      uint32_t N, uint32_t levels, uint32_t base_log, hipStream_t s);
int launch_pack_switch(const u64 *acc, uint32_t *out, uint32_t m, uint32_t N, uint32_t log_modulus, hipStream_t s);
// lwe_unpack.hip: decompression back to big-key LWE ciphertexts.  in = the compressed form of `count` ciphertexts (per block N mask
// values, then its body values); out[r] (N + 1 words) = the sample extraction of position index[r] (index == nullptr: position r),
// shifted up to 2^64; every index[r] < count is the caller's contract; rows == 0 launches nothing
int launch_unpack(const uint32_t *in, const uint32_t *index, u64 *out, uint32_t count, uint32_t rows, uint32_t N, uint32_t log_modulus,
                  hipStream_t s);
}  // namespace bmit
