// The support matrix of the blind rotation and the rule that selects a kernel, stated once: which (modulus, N, l, Bg, key precision)
// combinations have kernels, which device copies of a bootstrap key a context builds, which kernel runs a batch, and what the
// setters accept.  Plain structs and inline host functions - no context, no HIP, no device pointer - so that bmi_host.cpp, the
// launchers' own guards (bmi_kernels_t64*.hip) and a program without a GPU (tests/c_abi/rotation_plan_table.cpp) read the same
// text.  bmi_host.cpp describes a context to these functions (shape, settings, what it holds) and acts on the answer: a refusal is
// the text of bmi_last_error.  A new kernel family is added in two places: HERE (its predicate, its row in ROT_ROWS - and in
// COPY_ROWS / Table where it brings a key layout or a table of its own -, its place in choose_rotation) and as one launcher in the
// tables LAUNCHERS / CONVERTERS of bmi_host.cpp, in the order of the enumerations.
#pragma once
#include <stdint.h>

#include <string>

#include "t64_common.hpp"

// ------------------------------------------------------------------- (precision, levels, base log) with instantiated torus kernels
namespace bmit {

// the instantiated combinations of the exact-transform kernels (bmi_kernels_t64.hip: the predicate and both launchers expand this
// list) and of their unrolled form (bmi_kernels_t64u.hip)
#define BMIT_FOR_EACH_SHAPE(X) X(64, 3, 15) X(64, 2, 15) X(42, 3, 15) X(42, 2, 15) X(48, 3, 10) X(48, 2, 10) X(64, 3, 10)
#define BMIT_FOR_EACH_SHAPE_U(X) X(48, 3, 10) X(48, 2, 10)
#define BMIT_SHAPE_OK(P, L, B) if (prec == P && levels == L && base_log == B) return true;

inline bool shape_supported(int prec, uint32_t levels, uint32_t base_log) {
    BMIT_FOR_EACH_SHAPE(BMIT_SHAPE_OK)
    return false;
}
inline bool shape_supported_unrolled(int prec, uint32_t levels, uint32_t base_log) {
    BMIT_FOR_EACH_SHAPE_U(BMIT_SHAPE_OK)
    return false;
}
#undef BMIT_SHAPE_OK
// the combinations the N = 1024 floating-point transform's error bound was established for (bmi_kernels_t64f.hip)
inline bool shape_supported_fft(int prec, uint32_t levels, uint32_t base_log) {
    return prec == 48 && base_log == 10 && (levels == 3 || levels == 2);
}
// the unrolled floating-point-transform kernels (bmi_kernels_t64fu.hip): the 42-bit key (two 21-bit limbs) in base 2^10
inline bool shape_supported_unrolled_fft(int prec, uint32_t levels, uint32_t base_log) {
    return prec == 42 && base_log == 10 && (levels == 3 || levels == 2);
}
// the combinations the N = 2048 transform's error bound was established for (bmi_kernels_t64w.hip, _t64w2.hip)
inline bool shape_supported_wide(int prec, uint32_t levels, uint32_t base_log) {
    return prec == 46 && base_log == 10 && (levels == 3 || levels == 2);
}
// the N = 2048 unrolled kernels (bmi_kernels_t64wu.hip, _t64wu2.hip): the 40-bit key (two 20-bit limbs) in base 2^10
inline bool shape_supported_wide_unrolled(int prec, uint32_t levels, uint32_t base_log) {
    return prec == 40 && base_log == 10 && (levels == 3 || levels == 2);
}
// the combinations the N = 4096 transform's error bound was established for (bmi_kernels_t64q.hip)
inline bool shape_supported_quad(int prec, uint32_t levels, uint32_t base_log) {
    return prec == 44 && base_log == 10 && (levels == 3 || levels == 2);
}

}  // namespace bmit

namespace rotplan {

// ---------------------------------------------------------------------------------------------------- what a context is described by
enum class Modulus { goldilocks, field49, torus64 };

struct Shape {
    Modulus modulus;
    uint32_t log_N, bs_levels, bs_base_log;
    bool t64() const { return modulus == Modulus::torus64; }
    bool f64() const { return modulus == Modulus::field49; }
    bool wide() const { return log_N == 11; }
    bool quad() const { return log_N == 12; }
};

struct Settings {
    int bsk_prec;             // torus: bits of precision the bootstrap key is stored at (64 on the prime fields)
    bool bsk_prec_explicit;   // set by bmi_set_bsk_precision: bmi_set_bsk_unroll then leaves the precision alone
    uint32_t unroll;          // 1, or 2 = the unrolled key
    int variant;              // bmi_set_kernel_variant, 0 = auto
    uint32_t lat_threshold;   // auto: the latency kernels up to this batch size
};

// The tables a context uploads at creation (bmi_ctx::tables, built by bmi_ctx_create), with the kernels that read them.  A context
// holds those its modulus and N have a kernel for: context_tables.
enum class Table {
    tw_gl,         // Goldilocks: wave-NTT twiddles (ntt_wave.hpp) - bsk_to_ntt, negacyclic_mul, blind_rotate_lat / _tp
    tw_wave,       // 49-bit field and torus: the same mod 2^49 - 720895, centred doubles - 49-bit bsk_to_ntt, blind_rotate_tpx
                   // and their N = 2048 / 4096 forms, negacyclic_mul; torus bsk_to_limbs, blind_rotate
    tw_half,       // 49-bit field and torus: half transform (ntt_half_f64.hpp) - bsk_to_lat, blind_rotate_lat2 / _lat / _lat2u
    root_pow,      // 49-bit N <= 2048 and torus: psi^x, x < 2048 (psi_2048; N = 2048: psi_4096) - blind_rotate_lat2u, 49-bit _wide_u
    tw_wide49,     // 49-bit N = 2048: T / T^-1 of the even/odd combination - bsk_to_wide, blind_rotate_wide / _wide_u
    tw_quad49,     // 49-bit N = 4096: T_1..T_3, then their inverses - bsk_to_quad, blind_rotate_quad
    tw_fft,        // torus N = 1024: folded complex FFT (fft_wave_f64.hpp) - bsk_to_fft, blind_rotate_fft
    tw_fft_half,   // torus N = 1024: half FFT (fft_half_f64.hpp) - bsk_to_latf, blind_rotate_lat_fft / _lat2u_fft / _tp2u_fft
    zeta_pow,      // torus N = 1024: exp(i pi x / 1024), x in [0, 1024) as (re, im) - blind_rotate_lat2u_fft / _tp2u_fft
    zeta_oct,      // torus N = 2048: exp(i pi x / 2048), x in [0, 512] as (re, im), one octant - blind_rotate_wide_u
    tw_quarter,    // torus N = 2048: quarter transforms (fft_quarter_f64.hpp) - bsk_to_wide / _wide2, blind_rotate_wide / _wide2
    tw_eighth,     // torus N = 4096: eighth transforms (fft_eighth_f64.hpp) - bsk_to_quad, blind_rotate_quad
    COUNT,
    none = COUNT   // an unused table slot of a row
};
constexpr uint32_t bit(Table t) { return t == Table::none ? 0 : 1u << (int)t; }
inline uint32_t context_tables(const Shape &s) {
    if (!s.f64() && !s.t64()) return bit(Table::tw_gl);
    uint32_t t = bit(Table::tw_wave) | bit(Table::tw_half);   // (the torus kernels transform mod the 49-bit prime as well)
    if (s.t64() || !s.quad()) t |= bit(Table::root_pow);
    if (s.t64()) return t | (s.wide() ? bit(Table::tw_quarter) | bit(Table::zeta_oct) : s.quad() ? bit(Table::tw_eighth)
                                      : bit(Table::tw_fft) | bit(Table::tw_fft_half) | bit(Table::zeta_pow));
    return t | (s.wide() ? bit(Table::tw_wide49) : s.quad() ? bit(Table::tw_quad49) : 0);
}

// The device copies of a bootstrap key, one per layout (bmi_ctx::copies), in the order they are built: the layout, the conversion
// that makes it and the kernels that read it
enum class Copy {
    // the plain key
    ntt_gl,        // Goldilocks, NTT domain (bsk_to_ntt): blind_rotate_lat / _tp
    ntt49,         // 49-bit N = 1024, NTT domain (bsk_to_ntt): blind_rotate_tpx
    lat49,         // 49-bit N = 1024, split-transform slot order (bsk_to_lat): blind_rotate_lat2
    wide49,        // 49-bit N = 2048 (bsk_to_wide): blind_rotate_wide
    quad49,        // 49-bit N = 4096 (bsk_to_quad): blind_rotate_quad
    exact,         // torus N = 1024, limb polynomials of the exact transform (bsk_to_limbs): blind_rotate
    exact_lat,     // ... in the slot order of its latency form (bsk_to_lat): blind_rotate_lat
    fft,           // torus N = 1024, floating-point transform (bsk_to_fft): blind_rotate_fft
    fft_lat,       // ... in half-transform slot pairs (bsk_to_latf): blind_rotate_lat_fft
    wide,          // torus N = 2048 (bsk_to_wide): blind_rotate_wide
    wide2,         // torus N = 2048, two ciphertexts per workgroup (bsk_to_wide2): blind_rotate_wide2
    quad,          // torus N = 4096 (bsk_to_quad): blind_rotate_quad
    // the unrolled key
    u_lat49,       // 49-bit N = 1024, paired slot order (bsk_to_lat): blind_rotate_lat2u
    u_wide49,      // 49-bit N = 2048 (bsk_to_wide): blind_rotate_wide_u
    u_exact_lat,   // torus, exact transform (bsk_to_lat): blind_rotate_lat2u
    u_fft_lat,     // torus, key at 42 bits: floating-point transform (bsk_to_latf): blind_rotate_lat2u_fft / _tp2u_fft
    u_wide,        // torus N = 2048, key at 40 bits (bsk_to_wide): blind_rotate_wide_u / _wide_u2
    COUNT
};
constexpr uint32_t bit(Copy k) { return 1u << (int)k; }
struct CopyRow {
    const char *name;
    bool unrolled;    // a copy of the unrolled key
    Table tab[2];     // what its converter reads, in the order it takes them
};
constexpr Table NO_TABLE = Table::none;
constexpr CopyRow COPY_ROWS[] = {
    {"ntt_gl", false, {Table::tw_gl, NO_TABLE}},
    {"ntt49", false, {Table::tw_wave, NO_TABLE}},
    {"lat49", false, {Table::tw_half, NO_TABLE}},
    {"wide49", false, {Table::tw_wave, Table::tw_wide49}},
    {"quad49", false, {Table::tw_wave, Table::tw_quad49}},
    {"exact", false, {Table::tw_wave, NO_TABLE}},
    {"exact_lat", false, {Table::tw_half, NO_TABLE}},
    {"fft", false, {Table::tw_fft, NO_TABLE}},
    {"fft_lat", false, {Table::tw_fft_half, NO_TABLE}},
    {"wide", false, {Table::tw_quarter, NO_TABLE}},
    {"wide2", false, {Table::tw_quarter, NO_TABLE}},
    {"quad", false, {Table::tw_eighth, NO_TABLE}},
    {"u_lat49", true, {Table::tw_half, NO_TABLE}},
    {"u_wide49", true, {Table::tw_wave, Table::tw_wide49}},
    {"u_exact_lat", true, {Table::tw_half, NO_TABLE}},
    {"u_fft_lat", true, {Table::tw_fft_half, NO_TABLE}},
    {"u_wide", true, {Table::tw_quarter, NO_TABLE}},
};
static_assert(sizeof(COPY_ROWS) / sizeof(COPY_ROWS[0]) == (size_t)Copy::COUNT, "one row per key copy");
constexpr const CopyRow &row(Copy k) { return COPY_ROWS[(int)k]; }
inline const char *copy_name(Copy k) { return row(k).name; }

struct Held {
    uint32_t copies;   // bit(Copy) of every copy on the device
    bool have_keys, have_bsk3;
    bool has(Copy k) const { return (copies & bit(k)) != 0; }
};

// precision a torus context stores its bootstrap key at unless bmi_set_bsk_precision says otherwise: 48 bits (two 24-bit limbs)
// where the decomposition base leaves room for it (Bg <= 2^10: the default torus set), else the exact key (three 22-bit limbs)
// (N = 2048: 46 bits, two 23-bit limbs; N = 4096: 44 bits, two 22-bit limbs - the lengths at which the floating-point transform's error
// bound still certifies the rounding)
inline int default_bsk_precision(const Shape &s) { return s.log_N == 12 ? 44 : s.log_N == 11 ? 46 : (s.bs_base_log <= 10 ? 48 : 64); }

// a context as bmi_ctx_create leaves it (the lat_threshold: 2 rounds of 256 one-workgroup PBS, 11.2 ms, tie with one round of the
// wave-pair kernel, 11.3 ms)
inline Settings initial_settings(const Shape &s) { return Settings{s.t64() ? default_bsk_precision(s) : 64, false, 1, 0, 512}; }

// ------------------------------------------------------------------------------------------------- the shapes bmi_ctx_create admits
// (two questions, asked in this order with the check of k between them; empty = admitted)
inline std::string ring_refusal(const Shape &s) {
    if (s.log_N < 10 || s.log_N > 12 || (s.log_N != 10 && !s.f64() && !s.t64()))
        return "log_N must be 10 (N = 1024), 11 (N = 2048: 49-bit field or 2^64 torus) or 12 (N = 4096: 49-bit field or 2^64 torus)";
    return "";
}
inline std::string decomposition_refusal(const Shape &s) {
    const uint32_t l = s.bs_levels, b = s.bs_base_log;
    const bool lb_default = l == 3 && b == 15;
    const bool lb_f64 = lb_default || (l == 2 && b == 15) || (l == 1 && b == 23);
    const int prec = default_bsk_precision(s);
    // (2, 2^15) and (1, 2^23): the templated 49-bit kernels (N = 1024 wave-pair / latency kernels, N = 2048), and (2, 2^15) on the torus
    const bool ok_lb = (lb_default && !s.t64()) || (s.f64() && s.log_N <= 11 && lb_f64) ||
                       (s.t64() && s.log_N == 10 && bmit::shape_supported(prec, l, b)) ||
                       (s.t64() && s.log_N == 11 && bmit::shape_supported_wide(prec, l, b)) ||
                       (s.t64() && s.log_N == 12 && bmit::shape_supported_quad(prec, l, b));
    if (!ok_lb)
        return "(l, Bg) must be (3, 2^15); the 49-bit field at N <= 2048 also takes (2, 2^15) and (1, 2^23), the 2^64 torus (3 or 2, 2^10) "
               "and, at N = 1024, (3 or 2, 2^15)";
    return "";
}

// ------------------------------------------------------------------------------------------------------- the blind-rotation kernels
// The launchers (bmi_internal.hpp), one member each: choose_rotation picks one, launch_rotation (bmi_host.cpp) runs it.
enum class Rot {
    t64_wide_u, t64_wide_u2, t64_wide2, t64_wide, t64_quad, t64_tp2u_fft, t64_lat2u_fft, t64_lat2u, t64_lat_fft, t64_lat, t64_fft, t64_exact,   // 2^64 torus
    f49_wide_u, f49_wide, f49_quad, f49_lat2u, f49_lat2, f49_tpx,                                                   // 49-bit field
    gl_lat, gl_tp,                                                                                                  // Goldilocks
    COUNT
};

// What launch_rotation needs to know of a member, one row each in the order of the enumeration:
//   name         the __global__ function it launches: bmi_rotation_kernel answers with it
//   key          the key copy it reads
//   tab          the tables it reads, in the order the kernel takes them
//   accumulator  it has an accumulator form (bmi_blind_rotate_glwe_batch): the nine floating-point-transform kernels of the torus.
//                Not the exact-transform ones (the pair a pinned variant 1 / 3 / 4 selects, the unrolled key pinned at 48 bits), not
//                the prime fields.
//   stat         it takes the statistics pointer of bmi_fft_margin_host (the two-ciphertext forms w2 and tp2u have none)
struct RotRow {
    const char *name;
    Copy key;
    Table tab[3];
    bool accumulator, stat;
};
constexpr RotRow ROT_ROWS[] = {
    {"k_blind_rotate_wu_t64f", Copy::u_wide, {Table::tw_quarter, Table::zeta_oct, NO_TABLE}, true, true},
    {"k_blind_rotate_wu2_t64f", Copy::u_wide, {Table::tw_quarter, Table::zeta_oct, NO_TABLE}, true, true},   // one key copy serves both
    {"k_blind_rotate_w2_t64f", Copy::wide2, {Table::tw_quarter, NO_TABLE, NO_TABLE}, true, false},
    {"k_blind_rotate_w_t64f", Copy::wide, {Table::tw_quarter, NO_TABLE, NO_TABLE}, true, true},
    {"k_blind_rotate_q_t64f", Copy::quad, {Table::tw_eighth, NO_TABLE, NO_TABLE}, true, true},
    {"k_blind_rotate_tp2u_t64f", Copy::u_fft_lat, {Table::tw_fft_half, Table::zeta_pow, NO_TABLE}, true, false},
    {"k_blind_rotate_lat2u_t64f", Copy::u_fft_lat, {Table::tw_fft_half, Table::zeta_pow, NO_TABLE}, true, true},
    {"k_blind_rotate_lat2u_t64", Copy::u_exact_lat, {Table::tw_half, Table::root_pow, NO_TABLE}, false, false},
    {"k_blind_rotate_lat_t64f", Copy::fft_lat, {Table::tw_fft_half, NO_TABLE, NO_TABLE}, true, true},
    {"k_blind_rotate_lat_t64", Copy::exact_lat, {Table::tw_half, NO_TABLE, NO_TABLE}, false, false},
    {"k_blind_rotate_t64f", Copy::fft, {Table::tw_fft, NO_TABLE, NO_TABLE}, true, true},
    {"k_blind_rotate_t64", Copy::exact, {Table::tw_wave, NO_TABLE, NO_TABLE}, false, false},
    {"k_blind_rotate_wide49u", Copy::u_wide49, {Table::tw_wave, Table::tw_wide49, Table::root_pow}, false, false},
    {"k_blind_rotate_wide49", Copy::wide49, {Table::tw_wave, Table::tw_wide49, NO_TABLE}, false, false},
    {"k_blind_rotate_quad49", Copy::quad49, {Table::tw_wave, Table::tw_quad49, NO_TABLE}, false, false},
    {"k_blind_rotate_lat2u_49", Copy::u_lat49, {Table::tw_half, Table::root_pow, NO_TABLE}, false, false},
    {"k_blind_rotate_lat2_49", Copy::lat49, {Table::tw_half, NO_TABLE, NO_TABLE}, false, false},
    {"k_blind_rotate_tpx49", Copy::ntt49, {Table::tw_wave, NO_TABLE, NO_TABLE}, false, false},
    {"k_blind_rotate_lat", Copy::ntt_gl, {Table::tw_gl, NO_TABLE, NO_TABLE}, false, false},
    {"k_blind_rotate_tp", Copy::ntt_gl, {Table::tw_gl, NO_TABLE, NO_TABLE}, false, false},
};
static_assert(sizeof(ROT_ROWS) / sizeof(ROT_ROWS[0]) == (size_t)Rot::COUNT, "one row per kernel");
constexpr const RotRow &row(Rot rot) { return ROT_ROWS[(int)rot]; }
inline const char *rotation_name(Rot rot) { return row(rot).name; }
inline bool has_accumulator_form(Rot rot) { return row(rot).accumulator; }

// ------------------------------------------------------------------------------------------------ which copies a key set gets
// The plain key, in the layout of every kernel selectable on the context.
inline uint32_t plain_copies(const Shape &s, int prec) {
    const uint32_t l = s.bs_levels, b = s.bs_base_log;
    if (s.t64() && s.wide())   // N = 2048: one ciphertext per workgroup, and two (batches beyond 256)
        // (40 bits, the precision of the unrolled kernel only: no plain key copy)
        return bmit::shape_supported_wide(prec, l, b) ? bit(Copy::wide) | bit(Copy::wide2) : 0;
    if (s.t64() && s.quad()) return bit(Copy::quad);
    if (s.t64() && bmit::shape_supported_fft(prec, l, b))
        // the kernels auto dispatch runs on this key (48 bits, base 2^10): the wave-pair and the latency form of
        // bmi_kernels_t64f.hip, exact limb products through the floating-point transform.  The two copies of the
        // exact-transform kernels (variants 1 / 3 / 4: A/B only) are built when such a variant is first pinned: on_demand_copies.
        return bit(Copy::fft) | bit(Copy::fft_lat);
    if (s.t64())   // (a precision that only the unrolled kernel takes - 42 bits at base 2^10: no plain key copy)
        return bmit::shape_supported(prec, l, b) ? bit(Copy::exact) | bit(Copy::exact_lat) : 0;
    if (s.f64() && s.wide()) return bit(Copy::wide49);
    if (s.f64() && s.quad()) return bit(Copy::quad49);
    if (s.f64()) return bit(Copy::ntt49) | bit(Copy::lat49);   // (lat49: the slot order of the split-transform latency kernel)
    return bit(Copy::ntt_gl);
}
// ... and the copies a kernel needs that plain_copies may have left out: built before its first launch
inline uint32_t on_demand_copies(Rot rot) { return rot == Rot::t64_lat || rot == Rot::t64_exact ? bit(Copy::exact) | bit(Copy::exact_lat) : 0; }
// The unrolled key, in the layout of the context's unrolled kernel.
inline uint32_t unrolled_copies(const Shape &s, int prec) {
    if (s.t64() && s.wide()) return bit(Copy::u_wide);   // N = 2048: the per-polynomial layout of the plain kernel, over [pairs][3][2 l rows][2] polynomials
    if (s.t64() && bmit::shape_supported_unrolled_fft(prec, s.bs_levels, s.bs_base_log)) return bit(Copy::u_fft_lat);   // slot-pair order of the half FFT
    if (s.t64()) return bit(Copy::u_exact_lat);
    if (s.wide()) return bit(Copy::u_wide49);
    return bit(Copy::u_lat49);
}

// ----------------------------------------------------------------------------------------------------- the kernel of a batch
struct Choice {
    Rot rot;
    std::string refusal;   // empty: rot is the kernel
};
inline Choice refuse(const std::string &why) { return Choice{Rot::gl_tp, why}; }

// The kernel of bmi_blind_rotate_batch for a batch of `count`.  What the context holds is an argument, not recomputed from its
// shape: a context without keys is answered from the empty set.
inline Choice choose_rotation(const Shape &s, const Settings &set, const Held &h, uint32_t count) {
    // unrolled key (49-bit field and 2^64 torus at N = 1024 / 2048: bmi_set_bsk_unroll refuses the rest): kernels that give the same
    // words, so that a ciphertext's bits never depend on the batch it travelled in
    if (set.unroll == 2 && !h.have_bsk3)
        return refuse("unrolling selected but the context holds no unrolled key: generate keys after bmi_set_bsk_unroll, or bmi_import_bsk_unrolled");
    const int v = set.variant;
    // variant 0 = auto: the latency kernel (one workgroup per ciphertext) while the batch cannot fill the chip
    // with wave-pair work, the throughput kernel beyond that (49-bit field: the exchange-once form).
    const bool latency = v == 2 || (v == 0 && count <= set.lat_threshold);
    // torus, batches beyond one round of 256: two ciphertexts per workgroup sharing the key words (variants 1 / 3 pin it, 2 pins
    // the one-ciphertext form); the same words either way.  The unrolled N = 2048 pair (wu / wu2) follows the plain pair's rule:
    // one round of wu2 (up to 512 ciphertexts on 256 compute units) measures 11.35 ms against 7.6 ms for one round of wu (up to
    // 256) and 15.25 ms for two (257 .. 512), so wu2 wins from 257 on and wu up to 256; at 1,024 / 2,048 / 8,192 wu2 takes 0.74 of
    // wu's time (profiles/unrolled_wide2_ab.txt; 512 is the smallest batch measured - between 257 and 512 both kernels run the
    // round counts they run at 512).
    const bool two_per_wg = v == 1 || v == 3 || (v == 0 && count > 256);
    const int prec = set.bsk_prec;
    const uint32_t lv = s.bs_levels, bl = s.bs_base_log;
    const char *const unrolled_only = "this bootstrap-key precision exists for the unrolled kernel only: bmi_set_bsk_unroll(ctx, 2) before keygen";
    if (s.t64()) {
        if (s.wide() && set.unroll == 2) return {two_per_wg ? Rot::t64_wide_u2 : Rot::t64_wide_u, ""};   // one key copy serves both
        if (s.wide() && !h.has(Copy::wide)) return refuse(unrolled_only);
        if (s.wide() && h.has(Copy::wide2) && two_per_wg) return {Rot::t64_wide2, ""};
        if (s.wide()) return {Rot::t64_wide, ""};   // N = 2048 / 4096: one workgroup per ciphertext
        if (s.quad()) return {Rot::t64_quad, ""};
        if (set.unroll == 2)   // the floating-point-transform route where the key is at 42 bits, else the exact transform
            return {!bmit::shape_supported_unrolled_fft(prec, lv, bl) ? Rot::t64_lat2u : two_per_wg ? Rot::t64_tp2u_fft : Rot::t64_lat2u_fft, ""};
        // N = 1024: latency kernel (one workgroup per ciphertext) for small batches, wave pairs beyond
        const bool fft_key = h.has(Copy::fft);
        if (!fft_key && !bmit::shape_supported(prec, lv, bl)) return refuse(unrolled_only);
        if ((v == 5 || v == 6) && !fft_key)
            return refuse("kernel variant " + std::to_string(v) + " needs the bootstrap key at 48 bits of precision in base 2^10 (the torus default)");
        // (floating-point-transform kernels: two rounds of 256 one-workgroup bootstraps, 7.7 ms, still beat the wave-pair kernel's
        // 8.4 ms up to 1,024 ciphertexts; three rounds do not)
        const bool lat_t = v == 2 || v == 4 || v == 6 || (v == 0 && count <= set.lat_threshold);
        // through the floating-point transform where its key copy exists (48-bit key, base 2^10): variants 4 (latency) and
        // 1 / 3 (wave pairs) pin the exact transform mod 2^49 - 720895, 5 and 6 the floating-point one
        const bool fft = fft_key && (lat_t ? v != 4 : v == 0 || v == 5);
        return {lat_t ? (fft ? Rot::t64_lat_fft : Rot::t64_lat) : (fft ? Rot::t64_fft : Rot::t64_exact), ""};
    }
    if (s.f64()) {
        if (s.wide()) return {set.unroll == 2 ? Rot::f49_wide_u : Rot::f49_wide, ""};   // N = 2048 / 4096: one kernel for every batch size
        if (s.quad()) return {Rot::f49_quad, ""};
        return {set.unroll == 2 ? Rot::f49_lat2u : latency ? Rot::f49_lat2 : Rot::f49_tpx, ""};
    }
    return {latency ? Rot::gl_lat : Rot::gl_tp, ""};
}

// The kernel of bmi_fft_margin_host, the statistics hook of the floating-point-transform kernels.  Its own rule (batch size plays a
// part for the unrolled 40-bit key at N = 2048 only, where choose_rotation decides: the kernel that would run that batch): the
// unrolled kernel where the unrolled 42-bit key is in use, else at N = 1024 the latency form when kernel variant 6 / 2 is
// selected, else the N = 2048 / 4096 kernel, else the wave-pair kernel
inline Choice margin_rotation(const Shape &s, const Settings &set, const Held &h, uint32_t count) {
    const bool unrolled = s.t64() && set.unroll == 2 && h.have_bsk3;
    const bool ufft = unrolled && bmit::shape_supported_unrolled_fft(set.bsk_prec, s.bs_levels, s.bs_base_log);
    const bool uwide = unrolled && h.has(Copy::u_wide);   // N = 2048, the unrolled 40-bit key
    const bool wide_key = h.has(Copy::wide) || h.has(Copy::quad);
    if (!h.has(Copy::fft) && !wide_key && !ufft && !uwide)
        return refuse("the floating-point-transform kernels exist on the 2^64 torus with the bootstrap key at 48 bits (N = 1024), 46 bits "
                      "(N = 2048) or 44 bits (N = 4096) in base 2^10");
    if (uwide) return choose_rotation(s, set, h, count);
    if (ufft) return {Rot::t64_lat2u_fft, ""};
    if (!wide_key) return {set.variant == 6 || set.variant == 2 ? Rot::t64_lat_fft : Rot::t64_fft, ""};
    return {s.quad() ? Rot::t64_quad : Rot::t64_wide, ""};
}

// ------------------------------------------------------------------------------------------------------ what the setters accept
// bmi_set_bsk_precision(bits): empty = accepted (the key is then stored at `bits`, explicitly chosen)
inline std::string set_precision_refusal(const Shape &s, const Settings &set, const Held &h, uint32_t bits) {
    const uint32_t l = s.bs_levels, b = s.bs_base_log;
    if (!s.t64()) return "the bootstrap-key precision option exists on the 2^64 torus only";
    if (!t64::precision_ok((int)bits)) return "bootstrap-key precision must be 64 (exact), 48, 46, 44, 42 or 40 bits";
    if (h.have_keys) return "set the bootstrap-key precision before generating or importing keys";
    if (s.wide() || s.quad()) {
        // N = 2048 in unrolled mode (bmi_set_bsk_unroll first - which selects it by itself when no precision was set): 40 bits only
        if (s.wide() && set.unroll == 2) {
            if (!bmit::shape_supported_wide_unrolled((int)bits, l, b))
                return "at N = 2048 the unrolled torus kernel takes the key at 40 bits of precision (two 20-bit limbs) only: the six-times "
                       "larger limb sums of the unrolled step must stay inside the transform's certified range (bmi_kernels_t64wu.hip)";
        } else if (!(s.quad() ? bmit::shape_supported_quad : bmit::shape_supported_wide)((int)bits, l, b))
            return "at N = 2048 the torus kernel takes the key at 46 bits of precision (two 23-bit limbs) only - and at 40 bits (two 20-bit "
                   "limbs) for the unrolled kernel (bmi_set_bsk_unroll) -, at N = 4096 at 44 bits (two "
                   "22-bit limbs): the lengths at which the floating-point transform's error bound certifies the rounding "
                   "(fft_quarter_f64.hpp, fft_eighth_f64.hpp)";
        return "";
    }
    // 42 bits at base 2^10: in unrolled mode only (bmi_set_bsk_unroll first - which selects it by itself when no precision was set)
    const bool unrolled_fft = set.unroll == 2 && bmit::shape_supported_unrolled_fft((int)bits, l, b);
    if (!bmit::shape_supported((int)bits, l, b) && !unrolled_fft)
        return "no kernel for this precision at this decomposition: base 2^10 takes 48 (default) or 64 bits - and 42 bits for the "
               "unrolled floating-point-transform kernel (bmi_set_bsk_unroll) -, base 2^15 takes 64 (default) or 42 bits (a limb sum "
               "must stay below p/2: t64_common.hpp)";
    if (set.unroll == 2 && !unrolled_fft && !bmit::shape_supported_unrolled((int)bits, l, b))
        return "the unrolled torus kernels take the key at 48 bits (exact transform) or 42 bits (floating-point transform) at base 2^10";
    return "";
}

// bmi_set_bsk_unroll(factor): a refusal, or the precision the key is stored at from then on
struct UnrollChoice {
    int bsk_prec;
    std::string refusal;
};
inline UnrollChoice set_unroll(const Shape &s, const Settings &set, const Held &h, uint32_t factor) {
    const uint32_t l = s.bs_levels, b = s.bs_base_log;
    int prec = set.bsk_prec;
    if (factor != 1 && factor != 2) return {prec, "the unrolling factor is 1 or 2"};
    if (factor == 2 && !((s.f64() && !s.quad()) || s.t64()))
        return {prec, "bootstrap-key unrolling has HIP kernels for the 49-bit field and the 2^64 torus at N = 1024 and N = 2048 only"};
    if (factor == 2 && s.t64() && s.quad()) return {prec, "bootstrap-key unrolling has no HIP kernel on the 2^64 torus at N = 4096"};
    if (factor == 2 && s.t64() && s.wide() && !bmit::shape_supported_wide_unrolled(40, l, b))
        return {prec, "on the 2^64 torus at N = 2048 the unrolled kernel exists for l = 2 or 3 levels in base 2^10"};
    if (s.t64() && !set.bsk_prec_explicit && !h.have_keys) {
        // the precision nobody chose follows the mode: the unrolled step runs through the floating-point transform on a key stored
        // at 42 bits (k_blind_rotate_lat2u_t64f: 2.9 ms per bootstrap against 3.3 of the exact-transform kernel on the 48-bit key,
        // which bmi_set_bsk_precision(ctx, 48) still selects); back to the set's default when unrolling is switched off
        // (N = 2048: 40 bits, the only precision of k_blind_rotate_wu_t64f).  No refusal below follows a change made here.
        if (factor == 2 && s.wide()) prec = 40;
        else if (factor == 2 && bmit::shape_supported_unrolled_fft(42, l, b)) prec = 42;
        if (factor == 1) prec = default_bsk_precision(s);
    }
    if (factor == 2 && s.t64() && s.wide() && prec != 40)
        return {prec, "on the 2^64 torus at N = 2048 the unrolled kernel takes the key at 40 bits of precision only (chosen by itself when no "
                      "precision was set, before keygen): the limb sums of its three scaled products must stay inside the transform's "
                      "certified range"};
    if (factor == 2 && s.t64() && !s.wide() && !bmit::shape_supported_unrolled(prec, l, b) && !bmit::shape_supported_unrolled_fft(prec, l, b))
        return {prec, "on the 2^64 torus the unrolled kernels take the key at 48 or 42 bits at base 2^10 (the default torus set): the limb sums of "
                      "its three scaled products must stay below p/2"};
    if (factor == 2 && s.wide() && !s.t64() && l > 2)
        return {prec, "at N = 2048 the unrolled kernel exists for l <= 2 (at l = 3 it would not fit the registers: the plain kernel is faster)"};
    return {prec, ""};
}

// bmi_set_kernel_variant(variant)
inline std::string set_variant_refusal(const Shape &s, int variant) {
    if (variant < 0 || variant > 6) return "variant must be 0..6";
    if (variant >= 5 && !s.t64()) return "kernel variants 5 and 6 (floating-point transform) exist on the 2^64 torus only";
    if (s.f64() && !s.wide() && !s.quad() && (variant == 1 || variant == 4))
        return "kernel variants 1 and 4 are refused on the 49-bit field at N = 1024: 3 and 2 replaced their kernels there";
    return "";
}

// bmi_import_bsk_unrolled, and bmi_import_bsk_unrolled_seeded (which has established before that the context holds a key set
// expanded from a public key: on the 2^64 torus)
inline std::string import_unrolled_refusal(const Shape &s, const Settings &set, const Held &h) {
    if (!((s.f64() || s.t64()) && !s.quad()))
        return "bootstrap-key unrolling has HIP kernels for the 49-bit field and the 2^64 torus at N = 1024 and N = 2048 only";
    if (s.t64() && s.wide() && !bmit::shape_supported_wide_unrolled(set.bsk_prec, s.bs_levels, s.bs_base_log))
        return "on the 2^64 torus at N = 2048 the unrolled key is stored at 40 bits of precision: bmi_set_bsk_unroll(ctx, 2) before the key set";
    if (!h.have_keys) return "no keys: import or generate the key set first";
    return "";
}
inline std::string import_unrolled_seeded_refusal(const Shape &s, const Settings &set) {
    if (s.quad()) return "bootstrap-key unrolling has no HIP kernel on the 2^64 torus at N = 4096";
    if (s.wide() && !bmit::shape_supported_wide_unrolled(set.bsk_prec, s.bs_levels, s.bs_base_log))
        return "on the 2^64 torus at N = 2048 the unrolled key is stored at 40 bits of precision: bmi_set_bsk_unroll(ctx, 2) before the key set";
    return "";
}

}  // namespace rotplan
