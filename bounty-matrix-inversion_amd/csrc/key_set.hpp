// A key set on the host, free of HIP: the parameter tables, the state of a context that decides a generated word (which generator,
// which streams, the encryption counter, the precision the bootstrap key is rounded to, the compression shape remembered), the order
// in which a key set is drawn from the streams of host_crypto.hpp, and the host half of the C ABI of include/bmi_tfhe.h with its
// refusal texts.  libbmi_tfhe.so (bmi_host.cpp: bmi_ctx is a KeySet plus the device) and libbmi_client.so (bmi_client.cpp: a KeySet
// alone) are both built on this file, so a parameter set, the settings and a seed give the same words in either.  A plain C++17
// compiler takes it.
#pragma once

#include <cmath>
#include <string>
#include <vector>

#include "host_crypto.hpp"
#include "rotation_plan.hpp"

namespace hc {

constexpr uint32_t MAX_LWE_N = 1024;   // largest small-LWE dimension a blind-rotation kernel takes (BMI_MAX_LWE_N)

// The key word stored at `prec` bits of precision: rounded half up (as a signed integer) to a multiple of 2^(64 - prec);
// unsigned arithmetic, the wrap at the top of the range is the torus's own (the limb schemes: t64_common.hpp).
inline u64 round_key_word(u64 w, int prec) {
    const int drop = 64 - prec;
    if (drop == 0) return w;
    return ((w + ((u64)1 << (drop - 1))) >> drop) << drop;
}

// --------------------------------------------------------------------------- parameter sets
#ifndef BMI_DEFAULT_Q_BITS
#define BMI_DEFAULT_Q_BITS 65  // modulus of bmi_default_params(): 65 = BMI_Q_TORUS64 (q = 2^64, Concrete's own: the default since round 4), 49 (f64 kernels mod 2^49 - 720895) or 64 (Goldilocks)
#endif
inline int default_params_for(uint32_t q_bits, bmi_params *out) {
    if (!out || (q_bits != 64 && q_bits != 49 && q_bits != BMI_Q_TORUS64)) return -1;
    // same shape for every modulus; the 49-bit modulus keeps the absolute bootstrap-key noise above the integer grid
    // the torus set decomposes in base 2^10: the limb sums of its exact products then leave room for a two-limb key (48 bits of
    // precision) in the plain AND the unrolled blind rotation, and the output noise is lower than at 2^15 (t64_common.hpp)
    *out = bmi_params{630, 10, 1, 3, q_bits == BMI_Q_TORUS64 ? 10u : 15u, 8, 4, q_bits, std::ldexp(1.0, -25),
                      std::ldexp(1.0, q_bits == 49 ? -40 : -44)};
    return 0;
}

inline int default_params(bmi_params *out) { return default_params_for(BMI_DEFAULT_Q_BITS, out); }

inline int preset_params(const char *name, bmi_params *out) {
    if (!name || !out) return -1;
    const std::string s(name);
    if (s == "north_star") return default_params_for(49, out);
    if (s == "north_star_torus64") return default_params_for(BMI_Q_TORUS64, out);
    if (s == "north_star_goldilocks") return default_params_for(64, out);
    if (s == "secure128") {
        // n = 742 with LWE noise 7.07e-6 (2^-17.11) and a GLWE of size k N = 2048: the two security-relevant pairs of
        // TFHE-rs' published 128-bit set PARAM_MESSAGE_2_CARRY_2_KS_PBS (see bmi_tfhe.h); the GLWE noise is kept at
        // 2^-44 >= that set's 2.94e-16, so the GLWE side is at least as hard.  Decompositions are this build's: bootstrap 2 x 15
        // bits (output noise 2^-19.5: the circuits' linear combinations amplify it up to 75x), keyswitch 8 x 2 bits (its noise,
        // set by the LWE noise that security dictates, is what bounds the look-up margin: finer digits = less of it).
        *out = bmi_params{742, 11, 1, 2, 15, 8, 2, 49, 7.069849454709433e-6, std::ldexp(1.0, -44)};
        return 0;
    }
    if (s == "secure128_torus") {
        // the same two security-relevant pairs (n = 742 at LWE noise 2^-17.11; GLWE of size 2048 at noise 2^-44 >= 2.94e-16) on
        // Concrete's own modulus q = 2^64.  Decompositions: bootstrap 3 x 10 bits against a key stored at 46 bits of precision
        // (two 23-bit limbs: exact limb sums through the floating-point transform, fft_quarter_f64.hpp) - output noise 2^-22.9,
        // below the 49-bit preset's 2^-19.5; keyswitch 8 x 2 bits as there.
        *out = bmi_params{742, 11, 1, 3, 10, 8, 2, BMI_Q_TORUS64, 7.069849454709433e-6, std::ldexp(1.0, -44)};
        return 0;
    }
    if (s == "secure128_torus_wide") {
        // the same LWE pair under a GLWE of size 4096 (harder than the 2048 the noise 2^-44 is rated for) on q = 2^64, for the 5-bit
        // look-ups of the reference's unmodified circuits and of bases other than 2: key at 44 bits of precision (two 22-bit limbs,
        // fft_eighth_f64.hpp), bootstrap 3 x 10 bits.  The keyswitch noise (4,096 x levels rows at the LWE noise security dictates)
        // is what bounds the margin: 16 levels of 1 bit (mean-square digit 1/2) put a 5-bit look-up at 5.4 sigma, against 4.6 with
        // 8 x 2 bits and 4.4 at N = 2048 - whether that carries a circuit is error_budget's call (p_error), look-up count by count.
        *out = bmi_params{742, 12, 1, 3, 10, 16, 1, BMI_Q_TORUS64, 7.069849454709433e-6, std::ldexp(1.0, -44)};
        return 0;
    }
    return -1;
}

// A parameter set as rotation_plan.hpp takes it
inline rotplan::Shape shape_of(const bmi_params &P) {
    return {P.q_bits == BMI_Q_TORUS64 ? rotplan::Modulus::torus64 : P.q_bits == 49 ? rotplan::Modulus::field49 : rotplan::Modulus::goldilocks,
            P.log_N, P.bs_levels, P.bs_base_log};
}

// (ring size and bootstrap decomposition: the plan's lists; a q_bits not refused yet counts as Goldilocks there, as before)
inline bool params_supported(const bmi_params &P, std::string &why) {
    const rotplan::Shape shape = shape_of(P);
    if (!(why = rotplan::ring_refusal(shape)).empty()) return false;
    if (P.k != 1) { why = "only k = 1 has a HIP kernel in this build"; return false; }
    if (!(why = rotplan::decomposition_refusal(shape)).empty()) return false;
    if (P.n == 0 || P.n > MAX_LWE_N) { why = "n must be in [1, 1024]"; return false; }
    if (P.q_bits != 0 && P.q_bits != 64 && P.q_bits != 49 && P.q_bits != BMI_Q_TORUS64) {
        why = "q_bits must be 64 (2^64-2^32+1), 49 (2^49-720895) or BMI_Q_TORUS64 (2^64)";
        return false;
    }
    const uint32_t qb = P.q_bits == 49 ? 49 : 64;
    if (P.ks_levels * P.ks_base_log >= qb || P.ks_base_log > 7 || P.ks_levels == 0) { why = "unsupported keyswitch decomposition"; return false; }
    return true;
}

// --------------------------------------------------------------------------- the state
struct KeySet {
    bmi_params P{};
    Fq f;
    uint32_t N = 0, big_n = 0, rows = 0;
    bool have_keys = false;
    bool have_secret = false;  // false for a context that imported evaluation keys only (no encrypt / decrypt)
    u64 seed = 0, enc_counter = 0;
    int bsk_prec = 64;   // torus: bits of precision the bootstrap key is stored at (64 = exact, 48, 46, 44, 42, 40: t64_common.hpp; bmi_set_bsk_precision)
    bool bsk_prec_explicit = false;   // set by bmi_set_bsk_precision: bmi_set_bsk_unroll then leaves the precision alone
    bool secure_rng = false;       // true: keys / encryptions drawn from the CSPRNG below; false: test-only seeded streams
    ChaKey rng_secret, rng_public; // independent ChaCha20 keys from getrandom(): secrets + noise / public masks
    Sampler sampler(u64 of_seed) const { return {of_seed, f, secure_rng, rng_secret, rng_public}; }   // what the generators draw from
    // Where the mask words of the evaluation keys held came from (beside have_keys; the seeded forms of chacha_expand.hip):
    // OWN_STREAM = drawn by this context from rng_public (CSPRNG key generation), SEEDED_IMPORT = expanded from the public key of
    // bmi_import_keys_seeded, which rng_public then holds; OTHER = anything else (bmi_import_keys, the deterministic test streams):
    // such masks are no function of a public key that may be told.
    enum class MaskSource { OTHER, OWN_STREAM, SEEDED_IMPORT } mask_src = MaskSource::OTHER;
    bool bsk3_from_stream = false; // ... and the same for the unrolled key held: its masks are words of rng_public's S_BSK3_MASK streams
    std::vector<u64> sk_small, sk_big, bsk_std, ksk;
    // bootstrap-key unrolling (49-bit field at N = 1024 / 2048, 2^64 torus; bmi_set_bsk_unroll): per pair of LWE coefficients the GGSW encryptions of
    // s s', s (1 - s'), (1 - s) s'; host copy in the standard domain
    uint32_t unroll = 1;
    std::vector<u64> bsk3_std;
    bool have_bsk3 = false;
    uint32_t pairs() const { return (P.n + 1) / 2; }
    size_t bsk3_words() const { return (size_t)pairs() * 3 * rows * (P.k + 1) * N; }
    // compression of output ciphertexts (2^64 torus): the packing keyswitch key [N][pk_levels][2][N] of the key set held
    // (pk_levels == 0: none; dropped with the key set)
    uint32_t pk_levels = 0, pk_base_log = 0;
    // the (levels, base log) bmi_compression_keygen first used on the key set held (0: not yet): a row's masks and noise are the streams
    // (key, domain, row number) read from their start, so a second key of ANOTHER shape would reuse them under other messages - refused
    uint32_t pk_gen_levels = 0, pk_gen_base_log = 0;
    bool pksk_from_stream = false;     // its masks are words of rng_public's S_PKSK_MASK streams (as bsk3_from_stream)
    std::vector<u64> pksk;
    mutable std::string err;
    bool f64() const { return f.bits == 49; }
    bool t64() const { return f.torus; }

    // the state bmi_ctx_create leaves behind for the (admitted) parameter set `params`
    void init(const bmi_params &params) {
        P = params;
        if (P.q_bits == 0) P.q_bits = 64;
        if (P.q_bits == 49) f = Fq{FIELD49_Q, 49};
        if (P.q_bits == BMI_Q_TORUS64) f = Fq{0, 64, true};
        bsk_prec = rotplan::initial_settings(shape_of(P)).bsk_prec;
        N = 1u << params.log_N;
        big_n = params.k * N;
        rows = (params.k + 1) * params.bs_levels;
    }
};

inline thread_local std::string g_create_error;   // what bmi_last_error(NULL) returns: the refusal of the last bmi_ctx_create

inline int fail(const KeySet *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

// --------------------------------------------------------------------------- key generation
// fresh CSPRNG keys for this context (secret-class and public-class streams, never shared between them)
inline int rekey_csprng(KeySet *c) {
    if (!c->rng_secret.fill_from_os() || !c->rng_public.fill_from_os())
        return fail(c, -2, "getrandom() failed: no entropy source for key generation");
    c->secure_rng = true;
    c->enc_counter = 0;   // a new key: the (key, nonce) pairs of the new streams have never been used
    return 0;
}
inline void gen_secret_keys(KeySet *c, uint64_t seed) {
    c->sk_small.assign(c->P.n, 0);
    c->sk_big.assign(c->big_n, 0);
    secret_key_bits(c->sampler(seed), S_SK_SMALL, c->P.n, c->sk_small.data());
    secret_key_bits(c->sampler(seed), S_SK_BIG, c->big_n, c->sk_big.data());
}

// GGSW encryptions of the bits msg under the context's GLWE key, drawn from the streams (mask_stream, noise_stream) of `seed`
inline void gen_ggsw_rows(KeySet *c, uint64_t seed, u64 mask_stream, u64 noise_stream, const std::vector<u64> &msg, u64 *out) {
    const bmi_params &P = c->P;
    ggsw_rows(c->sampler(seed), mask_stream, noise_stream, c->sk_big.data(), c->N, P.k, P.bs_levels, P.bs_base_log, P.glwe_noise, msg.data(),
              msg.size(), out);
}

// the unrolled bootstrap key of the secret keys held, at full precision (hold_bsk3 rounds it)
inline void gen_bsk3(KeySet *c, uint64_t seed) {
    c->bsk3_std.assign(c->bsk3_words(), 0);
    gen_ggsw_rows(c, seed, S_BSK3_MASK, S_BSK3_NOISE, unrolled_messages(c->sk_small.data(), c->P.n), c->bsk3_std.data());
    c->bsk3_from_stream = c->secure_rng && c->mask_src == KeySet::MaskSource::OWN_STREAM;
}

// the compression key's host state goes with the key set it was made for
// new_key_set: the streams are new as well (or will never be read again): the shape bmi_compression_keygen is held to is forgotten
inline void forget_compression_key(KeySet *c, bool new_key_set) {
    if (new_key_set) c->pk_gen_levels = c->pk_gen_base_log = 0;
    c->pk_levels = c->pk_base_log = 0;
    c->pksk_from_stream = false;
    c->pksk.clear();
    c->pksk.shrink_to_fit();
}

// evaluation keys, at full precision, for the secret keys held in c->sk_small / c->sk_big, deterministic in `seed` (hold_eval_keys
// rounds the bootstrap key; in unrolled mode hold_bsk3 follows)
inline void gen_eval_key_words(KeySet *c, uint64_t seed) {
    forget_compression_key(c, true);
    const bmi_params &P = c->P;
    const uint32_t n = P.n, N = c->N, k = P.k, lk = P.ks_levels, rows = c->rows;
    c->seed = seed;
    if (!c->secure_rng) c->enc_counter = 0;   // deterministic test keys: encryption i of a key set is reproducible
    // --- bootstrap key: GGSW(s_i) rows, standard domain
    c->bsk_std.assign((size_t)n * rows * (k + 1) * N, 0);
    // (A torus key at 42 bits of precision is ROUNDED from this full-precision key when it is held.  Drawing the masks on the
    // 2^22 grid instead would keep the rounding error away from the secret key - measured: output noise 2^-20 - but the
    // body's noise, std 2^20, is then rounded to the grid too and vanishes in 95 % of the words: not an LWE sample any more.)
    gen_ggsw_rows(c, seed, S_BSK_MASK, S_BSK_NOISE, c->sk_small, c->bsk_std.data());
    c->have_bsk3 = false;
    c->mask_src = c->secure_rng ? KeySet::MaskSource::OWN_STREAM : KeySet::MaskSource::OTHER;
    if (c->unroll == 2) gen_bsk3(c, seed);
    // --- keyswitch key
    c->ksk.assign((size_t)k * N * lk * (n + 1), 0);
    ksk_rows(c->sampler(seed), c->sk_small.data(), n, c->sk_big.data(), c->big_n, lk, P.ks_base_log, P.lwe_noise, c->ksk.data());
    c->have_secret = true;
}

// The evaluation keys in c->bsk_std / c->ksk become the keys held.  Torus key stored at 48 / 42 bits of precision: every word
// rounded (half up, as a signed integer) to a multiple of 2^16 / 2^22.  The rounded key IS the key from here on (bmi_export_keys
// returns it), so every consumer agrees on it.  The caller sets have_keys once whatever it builds from them exists.
inline void round_eval_keys(KeySet *c) {
    if (c->t64() && c->bsk_prec != 64)
        for (u64 &w : c->bsk_std) w = round_key_word(w, c->bsk_prec);
    c->have_keys = false;
}
// ... and the unrolled key in c->bsk3_std (torus: the key stored at bsk_prec bits IS the key from here on, what
// bmi_export_bsk_unrolled returns); the caller sets have_bsk3
inline int round_bsk3(KeySet *c) {
    if (c->bsk3_std.size() != c->bsk3_words()) return fail(c, -1, "no unrolled bootstrap key to upload");
    if (c->t64() && c->bsk_prec != 64)
        for (u64 &w : c->bsk3_std) w = round_key_word(w, c->bsk_prec);
    c->have_bsk3 = false;
    return 0;
}

// bmi_keygen_from_secret up to the generation of the evaluation keys
inline int take_secret_keys(KeySet *c, const uint64_t *sk_small, const uint64_t *sk_big, uint64_t seed) {
    const uint32_t n = c->P.n, kN = c->P.k * c->N;
    if (!is_binary(sk_small, n) || !is_binary(sk_big, kN)) return fail(c, -1, "secret keys are binary");
    c->sk_small.assign(sk_small, sk_small + n);
    c->sk_big.assign(sk_big, sk_big + kN);
    if (seed == 0) {            // production: masks and noise from the CSPRNG
        if (int rc = rekey_csprng(c)) return rc;
    } else {
        c->secure_rng = false;  // test vectors: deterministic in seed
    }
    return 0;
}

// bmi_import_keys: what is refused before anything changes ...
inline int import_keys_pairing(const KeySet *c, const uint64_t *sk_small, const uint64_t *sk_big) {
    if ((sk_small == nullptr) != (sk_big == nullptr)) return fail(c, -1, "pass both secret keys or neither");
    return 0;
}
inline int import_keys_canonical(const KeySet *c, const uint64_t *bsk, const uint64_t *ksk) {
    const bmi_params &P = c->P;
    const size_t bsk_words = (size_t)P.n * c->rows * (P.k + 1) * c->N, ksk_words = (size_t)c->big_n * P.ks_levels * (P.n + 1);
    for (size_t i = 0; i < bsk_words; i++)
        if (!c->f.canonical(bsk[i])) return fail(c, -1, "bootstrap key word not reduced mod q");
    for (size_t i = 0; i < ksk_words; i++)
        if (!c->f.canonical(ksk[i])) return fail(c, -1, "keyswitch key word not reduced mod q");
    return 0;
}
// ... and the new key set's host state (the previous one's device state is the caller's to drop first)
inline int import_keys_store(KeySet *c, const uint64_t *sk_small, const uint64_t *sk_big, const uint64_t *bsk, const uint64_t *ksk) {
    const bmi_params &P = c->P;
    const size_t bsk_words = (size_t)P.n * c->rows * (P.k + 1) * c->N, ksk_words = (size_t)c->big_n * P.ks_levels * (P.n + 1);
    c->have_keys = false;
    forget_compression_key(c, true);
    c->have_bsk3 = false;   // an unrolled key belongs to the key set it was generated with: import it again (bmi_import_bsk_unrolled)
    c->mask_src = KeySet::MaskSource::OTHER;
    c->bsk_std.assign(bsk, bsk + bsk_words);
    c->ksk.assign(ksk, ksk + ksk_words);
    c->have_secret = sk_small != nullptr;
    if (c->have_secret) {
        if (!is_binary(sk_small, P.n) || !is_binary(sk_big, c->big_n)) return fail(c, -1, "secret keys are binary");
        c->sk_small.assign(sk_small, sk_small + P.n);
        c->sk_big.assign(sk_big, sk_big + c->big_n);
    } else {
        c->sk_small.clear();
        c->sk_big.clear();
    }
    return rekey_csprng(c);   // encryptions under an imported key set draw fresh CSPRNG randomness
}

inline int export_keys(const KeySet *c, uint64_t *sk_small, uint64_t *sk_big, uint64_t *bsk, uint64_t *ksk) {
    if (!c) return -1;
    if (!c->have_keys) return fail(c, -1, "no keys: call bmi_keygen first");
    if ((sk_small || sk_big) && !c->have_secret) return fail(c, -1, "evaluation-only context: it holds no secret key");
    if (sk_small) std::memcpy(sk_small, c->sk_small.data(), c->sk_small.size() * 8);
    if (sk_big) std::memcpy(sk_big, c->sk_big.data(), c->sk_big.size() * 8);
    if (bsk) std::memcpy(bsk, c->bsk_std.data(), c->bsk_std.size() * 8);
    if (ksk) std::memcpy(ksk, c->ksk.data(), c->ksk.size() * 8);
    return 0;
}

// --------------------------------------------------------------------------- settings that decide what a key is
// (held: what the context holds, as rotation_plan.hpp asks; settings: the KeySet's own plus the caller's kernel choices)
inline int set_bsk_precision(KeySet *c, const rotplan::Settings &set, const rotplan::Held &held, uint32_t bits) {
    const std::string refusal = rotplan::set_precision_refusal(shape_of(c->P), set, held, bits);
    if (!refusal.empty()) return fail(c, -1, refusal);
    c->bsk_prec = (int)bits;
    c->bsk_prec_explicit = true;
    return 0;
}
inline int get_bsk_precision(const KeySet *c, uint32_t *bits) {
    if (!c || !bits) return -1;
    *bits = c->t64() ? (uint32_t)c->bsk_prec : 64u;
    return 0;
}
// *generated: the unrolled key of the secret keys already held was drawn (fresh masks and noise: CSPRNG, or the seeded test
// streams) and waits in c->bsk3_std for round_bsk3
inline int set_bsk_unroll(KeySet *c, const rotplan::Settings &set, const rotplan::Held &held, uint32_t factor, bool *generated) {
    *generated = false;
    const rotplan::UnrollChoice ch = rotplan::set_unroll(shape_of(c->P), set, held, factor);
    if (!ch.refusal.empty()) return fail(c, -1, ch.refusal);
    c->bsk_prec = ch.bsk_prec;   // (the precision nobody chose follows the mode)
    c->unroll = factor;
    if (factor == 2 && c->have_keys && !c->have_bsk3) {
        if (!c->have_secret) return 0;   // evaluation-only context: the key arrives through bmi_import_bsk_unrolled
        gen_bsk3(c, c->seed);
        *generated = true;
    }
    return 0;
}
inline int import_bsk_unrolled_store(KeySet *c, const rotplan::Settings &set, const rotplan::Held &held, const uint64_t *bsk3) {
    const std::string refusal = rotplan::import_unrolled_refusal(shape_of(c->P), set, held);
    if (!refusal.empty()) return fail(c, -1, refusal);
    const size_t words = c->bsk3_words();
    for (size_t i = 0; i < words; i++)
        if (!c->f.canonical(bsk3[i])) return fail(c, -1, "unrolled bootstrap key word not reduced mod q");
    c->bsk3_std.assign(bsk3, bsk3 + words);
    c->bsk3_from_stream = false;
    return 0;
}
inline int export_bsk_unrolled(const KeySet *c, uint64_t *bsk3) {
    if (!c || !bsk3) return -1;
    if (!c->have_bsk3) return fail(c, -1, "no unrolled bootstrap key: bmi_set_bsk_unroll(ctx, 2) before keygen, or import one");
    std::memcpy(bsk3, c->bsk3_std.data(), c->bsk3_std.size() * 8);
    return 0;
}

// --------------------------------------------------------------------------- encryption, phase, decryption
// bmi_encrypt (ct_out: [count][k N + 1] words) and bmi_encrypt_seeded (bodies_out: [count] body words; the masks are not kept) are
// this one routine: ciphertext i takes the encryption counter first + i, its masks from the public stream, its noise from the secret one
inline int encrypt_rows(KeySet *c, const int64_t *msgs, uint32_t count, uint32_t delta_log, uint64_t *ct_out, uint64_t *bodies_out) {
    if (!c->have_keys) return fail(c, -1, "no keys: call bmi_keygen first");
    if (!c->have_secret) return fail(c, -1, "evaluation-only context: it holds no secret key");
    if (delta_log >= c->f.bits - 1) return fail(c, -1, "delta_log out of range");
    // (secure contexts: the counter is never reset while the CSPRNG keys live - one nonce per ciphertext)
    lwe_encrypt(c->sampler(c->seed), c->sk_big.data(), c->big_n, c->P.glwe_noise, c->enc_counter, msgs, count, delta_log, ct_out, bodies_out);
    c->enc_counter += count;
    return 0;
}
inline int encrypt(KeySet *c, const int64_t *msgs, uint32_t count, uint32_t delta_log, uint64_t *ct_out) {
    if (!c || !msgs || !ct_out) return -1;
    return encrypt_rows(c, msgs, count, delta_log, ct_out, nullptr);
}
inline int phase(const KeySet *c, const uint64_t *ct_in, uint32_t count, uint64_t *phase_out) {
    if (!c || !ct_in || !phase_out) return -1;
    if (!c->have_keys) return fail(c, -1, "no keys: call bmi_keygen first");
    if (!c->have_secret) return fail(c, -1, "evaluation-only context: it holds no secret key");
    lwe_phase(c->f, c->sk_big.data(), c->big_n, ct_in, count, phase_out);
    return 0;
}
inline int decrypt(const KeySet *c, const uint64_t *ct_in, uint32_t count, uint32_t delta_log, int64_t *msgs) {
    if (!c || !ct_in || !msgs) return -1;
    if (delta_log == 0 || delta_log >= c->f.bits - 1) return fail(c, -1, "delta_log out of range");
    std::vector<u64> ph(count);
    int rc = phase(c, ct_in, count, ph.data());
    if (rc) return rc;
    for (uint32_t i = 0; i < count; i++) msgs[i] = decode(c->f, ph[i], delta_log);
    return 0;
}
// ct words on the 2^64 torus <-> words mod q: the modulus switch round(x * q / 2^64) and back.  Context-free.
inline int torus64_to_field_words(uint32_t q_bits, const uint64_t *in, uint64_t words, uint64_t *out) {
    if (!in || !out || (q_bits != 64 && q_bits != 49)) return -1;
    torus64_to_field(q_bits == 49 ? FIELD49_Q : GOLDILOCKS_P, in, words, out);
    return 0;
}
inline int field_to_torus64_words(uint32_t q_bits, const uint64_t *in, uint64_t words, uint64_t *out) {
    if (!in || !out || (q_bits != 64 && q_bits != 49)) return -1;
    return field_to_torus64(q_bits == 49 ? FIELD49_Q : GOLDILOCKS_P, in, words, out) ? 0 : -1;
}

// --------------------------------------------------------------------------- seeded keys and ciphertexts
// The specification of the seeded forms (seeded_mask_words).  Context-free.
inline int seeded_mask_words_checked(const uint32_t pub_key[8], uint64_t nonce, uint64_t first_word, uint64_t count, uint64_t *out) {
    if (!pub_key || (count && !out)) return -1;
    seeded_mask_words(pub_key, nonce, first_word, count, out);
    return 0;
}
// What the seeded forms need of a context: masks that are words of a public stream whose key may be told.  `what` names the caller.
inline int seeded_ok(const KeySet *c, const char *what) {
    if (!c->t64())
        return fail(c, -1, std::string(what) + ": seeded forms exist on the 2^64 torus only - on the 49-bit field and Goldilocks the masks are "
                           "rejection-sampled, so a mask word's position in the stream depends on the words before it");
    if (!c->have_keys) return fail(c, -1, std::string(what) + ": no keys: call bmi_keygen first");
    if (c->mask_src == KeySet::MaskSource::OTHER)
        return fail(c, -1, std::string(what) + ": the masks of this key set did not come from the context's own public stream (keys loaded by "
                           "bmi_import_keys, or deterministic test keys, whose stream key is an invertible function of the seed and would "
                           "reveal the secrets): no seeded form");
    return 0;
}
inline int export_keys_seeded(const KeySet *c, uint32_t pub_key[8], uint64_t *bsk_bodies, uint64_t *ksk_bodies) {
    if (!c || !pub_key || !bsk_bodies || !ksk_bodies) return -1;
    if (int rc = seeded_ok(c, "bmi_export_keys_seeded")) return rc;
    std::memcpy(pub_key, c->rng_public.k, sizeof(c->rng_public.k));
    copy_bodies(c->bsk_std, (size_t)c->P.n * c->rows, c->big_n, c->N, bsk_bodies);
    copy_bodies(c->ksk, (size_t)c->big_n * c->P.ks_levels, c->P.n, 1, ksk_bodies);
    return 0;
}
inline int export_bsk_unrolled_seeded(const KeySet *c, uint64_t *bsk3_bodies) {
    if (!c || !bsk3_bodies) return -1;
    if (int rc = seeded_ok(c, "bmi_export_bsk_unrolled_seeded")) return rc;
    if (!c->have_bsk3) return fail(c, -1, "no unrolled bootstrap key: bmi_set_bsk_unroll(ctx, 2) before keygen, or import one");
    if (!c->bsk3_from_stream)
        return fail(c, -1, "bmi_export_bsk_unrolled_seeded: the masks of this unrolled key did not come from the context's own public stream "
                           "(a key loaded by bmi_import_bsk_unrolled): no seeded form");
    copy_bodies(c->bsk3_std, (size_t)c->pairs() * 3 * c->rows, c->big_n, c->N, bsk3_bodies);
    return 0;
}
inline int encrypt_seeded(KeySet *c, const int64_t *msgs, uint32_t count, uint32_t delta_log, uint64_t *first_counter, uint64_t *bodies) {
    if (!c || !first_counter || (count && (!msgs || !bodies))) return -1;
    if (int rc = seeded_ok(c, "bmi_encrypt_seeded")) return rc;
    const u64 first = c->enc_counter;
    if (int rc = encrypt_rows(c, msgs, count, delta_log, nullptr, bodies)) return rc;
    *first_counter = first;
    return 0;
}

// --------------------------------------------------------------------------- compression of output ciphertexts
// What every compression entry point needs of a context, and of a (levels, base log) pair.  `what` names the caller.
inline int compression_ok(const KeySet *c, const char *what) {
    if (!c->t64())
        return fail(c, -1, std::string(what) + ": compression of output ciphertexts exists on the 2^64 torus only (not on the 49-bit field or "
                           "Goldilocks)");
    if (!c->have_keys) return fail(c, -1, std::string(what) + ": no keys: call bmi_keygen first");
    return 0;
}
inline int compression_shape_ok(const KeySet *c, const char *what, uint32_t levels, uint32_t base_log) {
    if (levels < 1 || levels > 4 || base_log < 1 || base_log > 16 || levels * base_log > 63)
        return fail(c, -1, std::string(what) + ": the compression key's decomposition needs 1 <= levels <= 4, 1 <= base_log <= 16 and "
                           "levels * base_log <= 63");
    return 0;
}
inline int compression_key_held(const KeySet *c, const char *what) {
    if (int rc = compression_ok(c, what)) return rc;
    if (!c->pk_levels)
        return fail(c, -1, std::string(what) + ": no compression key: call bmi_compression_keygen or import one (a new key set drops it)");
    return 0;
}
inline int log_modulus_ok(const KeySet *c, const char *what, uint32_t log_modulus) {
    if (log_modulus < 2 || log_modulus > 32) return fail(c, -1, std::string(what) + ": log_modulus must be in [2, 32]");
    return 0;
}
// bmi_compression_keygen: what it refuses ...
inline int compression_keygen_refusal(const KeySet *c, uint32_t levels, uint32_t base_log) {
    if (int rc = compression_ok(c, "bmi_compression_keygen")) return rc;
    if (!c->have_secret) return fail(c, -1, "bmi_compression_keygen: evaluation-only context: it holds no secret key");
    if (int rc = compression_shape_ok(c, "bmi_compression_keygen", levels, base_log)) return rc;
    // One shape per key set.  Row jr takes its masks from the public stream (S_PKSK_MASK, jr) and its noise from the secret stream
    // (S_PKSK_NOISE, jr), both from their first word: a key of another shape would give row jr the same A and e under another
    // message, and the difference of the two bodies is an exact combination of secret-key bits.  The same shape again gives the
    // same key.
    if (c->pk_gen_levels && (c->pk_gen_levels != levels || c->pk_gen_base_log != base_log))
        return fail(c, -1, "bmi_compression_keygen: this key set already has a compression key of shape (" + std::to_string(c->pk_gen_levels) +
                           ", " + std::to_string(c->pk_gen_base_log) + "); a second one of another shape would reuse the rows' mask and noise "
                           "streams under other messages and reveal the secret key: generate a new key set first");
    return 0;
}
// ... and the key's words in c->pksk (the previous key's device state is the caller's to drop first; it sets pk_levels / pk_base_log
// once whatever it builds from the words exists, then pksk_from_stream = compression_key_from_stream(c))
inline void gen_compression_key(KeySet *c, uint32_t levels, uint32_t base_log) {
    forget_compression_key(c, false);
    c->pk_gen_levels = levels;
    c->pk_gen_base_log = base_log;
    c->pksk.assign((size_t)c->N * levels * 2 * c->N, 0);
    compression_key_rows(c->sampler(c->seed), c->sk_big.data(), c->N, levels, base_log, c->P.glwe_noise, c->pksk.data());
}
inline bool compression_key_from_stream(const KeySet *c) { return c->secure_rng && c->mask_src == KeySet::MaskSource::OWN_STREAM; }
inline int import_compression_key_refusal(const KeySet *c, uint32_t levels, uint32_t base_log) {
    if (int rc = compression_ok(c, "bmi_import_compression_key")) return rc;
    return compression_shape_ok(c, "bmi_import_compression_key", levels, base_log);
}
inline void import_compression_key_store(KeySet *c, uint32_t levels, const uint64_t *key) {
    forget_compression_key(c, false);
    c->pksk.assign(key, key + (size_t)c->N * levels * 2 * c->N);
}
inline int export_compression_key(const KeySet *c, uint64_t *key) {
    if (!c || !key) return -1;
    if (int rc = compression_key_held(c, "bmi_export_compression_key")) return rc;
    std::memcpy(key, c->pksk.data(), c->pksk.size() * 8);
    return 0;
}
inline int export_compression_key_seeded(const KeySet *c, uint64_t *bodies) {
    if (!c || !bodies) return -1;
    if (int rc = seeded_ok(c, "bmi_export_compression_key_seeded")) return rc;
    if (int rc = compression_key_held(c, "bmi_export_compression_key_seeded")) return rc;
    if (!c->pksk_from_stream)
        return fail(c, -1, "bmi_export_compression_key_seeded: the masks of this compression key did not come from the context's own public "
                           "stream (a key loaded by bmi_import_compression_key): no seeded form");
    copy_bodies(c->pksk, (size_t)c->N * c->pk_levels, c->N, c->N, bodies);
    return 0;
}
inline int compressed_words(const KeySet *c, uint32_t count, uint64_t *words) {
    if (!c || !words) return -1;
    if (!c->t64()) return fail(c, -1, "bmi_compressed_words: compression of output ciphertexts exists on the 2^64 torus only");
    *words = ((u64)count + c->N - 1) / c->N * c->N + count;
    return 0;
}
inline int phase_compressed(const KeySet *c, const uint32_t *data, uint32_t count, uint32_t log_modulus, uint64_t *phase_out) {
    if (!c || (count && (!data || !phase_out))) return -1;
    if (int rc = compression_ok(c, "bmi_phase_compressed")) return rc;
    if (!c->have_secret) return fail(c, -1, "bmi_phase_compressed: evaluation-only context: it holds no secret key");
    if (int rc = log_modulus_ok(c, "bmi_phase_compressed", log_modulus)) return rc;
    if (!compressed_phase(c->f, c->sk_big.data(), c->N, data, count, log_modulus, phase_out))
        return fail(c, -1, "bmi_phase_compressed: a value does not fit log_modulus bits");
    return 0;
}
inline int decrypt_compressed(const KeySet *c, const uint32_t *data, uint32_t count, uint32_t log_modulus, uint32_t delta_log, int64_t *msgs) {
    if (!c || (count && (!data || !msgs))) return -1;
    if (int rc = compression_ok(c, "bmi_decrypt_compressed")) return rc;
    if (delta_log == 0 || delta_log >= c->f.bits - 1) return fail(c, -1, "delta_log out of range");
    std::vector<u64> ph(count);
    if (int rc = phase_compressed(c, data, count, log_modulus, ph.data())) return rc;
    for (uint32_t i = 0; i < count; i++) msgs[i] = decode(c->f, ph[i], delta_log);
    return 0;
}

}  // namespace hc
