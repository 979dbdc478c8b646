// libbmi_client.so: the host half of the C ABI of include/bmi_tfhe.h - parameter sets, key generation, the key exports and imports a
// client needs, encryption, decryption, the seeded and compressed forms' host side - for a machine without a GPU (include/bmi_client.h).
// A context here is the key set of key_set.hpp and nothing else: every word it exports or encrypts is the word libbmi_tfhe.so
// exports or encrypts for the same parameter set, settings and seed, because both libraries call the same functions in the same
// order; where bmi_host.cpp uploads, this file only marks the keys as held.  Nothing here evaluates: the PBS path has no CPU form.
// Plain C++17, no HIP.
#include <cstring>
#include <string>

#include "../../include/bmi_client.h"
#include "key_set.hpp"

using namespace hc;

struct bmi_ctx : hc::KeySet {};

namespace {

// what rotation_plan.hpp asks of a context: this one has no kernel choices and no device copies
rotplan::Settings settings_of(const bmi_ctx *c) {
    return {c->bsk_prec, c->bsk_prec_explicit, c->unroll, 0, rotplan::initial_settings(shape_of(c->P)).lat_threshold};
}
rotplan::Held held_of(const bmi_ctx *c) { return {0, c->have_keys, c->have_bsk3}; }

// overwrites memory that held secrets in a way the compiler may not drop before a free
void wipe(void *p, size_t bytes) {
    volatile unsigned char *v = static_cast<volatile unsigned char *>(p);
    for (size_t i = 0; i < bytes; i++) v[i] = 0;
}
void wipe(std::vector<u64> &v) { wipe(v.data(), v.capacity() * sizeof(u64)); }

// the evaluation keys generated or imported into c->bsk_std / c->ksk become the keys held (bmi_host.cpp: upload_eval_keys)
int hold_eval_keys(bmi_ctx *c) {
    round_eval_keys(c);
    c->have_keys = true;
    return 0;
}
// ... and the unrolled key in c->bsk3_std (bmi_host.cpp: upload_bsk3)
int hold_bsk3(bmi_ctx *c) {
    if (int rc = round_bsk3(c)) return rc;
    c->have_bsk3 = true;
    return 0;
}
int gen_eval_keys(bmi_ctx *c, uint64_t seed) {
    gen_eval_key_words(c, seed);
    if (int rc = hold_eval_keys(c)) return rc;
    return c->unroll == 2 ? hold_bsk3(c) : 0;
}

}  // namespace

extern "C" {

int bmi_default_params_for(uint32_t q_bits, bmi_params *out) { return default_params_for(q_bits, out); }

int bmi_default_params(bmi_params *out) { return default_params(out); }

int bmi_preset_params(const char *name, bmi_params *out) { return preset_params(name, out); }

const char *bmi_last_error(const bmi_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int bmi_ctx_create(const bmi_params *params, int device, bmi_ctx **out) {
    if (!params || !out) return fail(nullptr, -1, "null argument");
    std::string why;
    if (!params_supported(*params, why)) return fail(nullptr, -1, why);
    if (device != BMI_CLIENT_NO_DEVICE)
        return fail(nullptr, -1, "libbmi_client.so holds keys and encrypts on the host only: pass BMI_CLIENT_NO_DEVICE (-1); a context on "
                                 "a device is libbmi_tfhe.so's");
    bmi_ctx *c = new bmi_ctx();
    c->init(*params);
    *out = c;
    return 0;
}

void bmi_ctx_destroy(bmi_ctx *c) {
    if (!c) return;
    // the secret keys and the secret ChaCha20 key (key bits and noise come from it) are overwritten before their memory goes back
    // to the allocator
    wipe(c->sk_small);
    wipe(c->sk_big);
    wipe(c->rng_secret.k, sizeof(c->rng_secret.k));
    c->seed = 0;
    delete c;
}

int bmi_get_params(const bmi_ctx *c, bmi_params *out) {
    if (!c || !out) return -1;
    *out = c->P;
    return 0;
}

int bmi_keygen(bmi_ctx *c) {
    if (!c) return -1;
    if (int rc = rekey_csprng(c)) return rc;
    gen_secret_keys(c, 0);
    return gen_eval_keys(c, 0);
}

int bmi_keygen_insecure_deterministic(bmi_ctx *c, uint64_t seed) {
    if (!c) return -1;
    c->secure_rng = false;
    gen_secret_keys(c, seed);
    return gen_eval_keys(c, seed);
}

int bmi_keygen_from_secret(bmi_ctx *c, const uint64_t *sk_small, const uint64_t *sk_big, uint64_t seed) {
    if (!c || !sk_small || !sk_big) return -1;
    if (int rc = take_secret_keys(c, sk_small, sk_big, seed)) return rc;
    return gen_eval_keys(c, seed);
}

int bmi_torus64_to_field(uint32_t q_bits, const uint64_t *in, uint64_t words, uint64_t *out) {
    return torus64_to_field_words(q_bits, in, words, out);
}

int bmi_field_to_torus64(uint32_t q_bits, const uint64_t *in, uint64_t words, uint64_t *out) {
    return field_to_torus64_words(q_bits, in, words, out);
}

int bmi_import_keys(bmi_ctx *c, const uint64_t *sk_small, const uint64_t *sk_big, const uint64_t *bsk, const uint64_t *ksk) {
    if (!c || !bsk || !ksk) return -1;
    if (int rc = import_keys_pairing(c, sk_small, sk_big)) return rc;
    if (!sk_small)
        return fail(c, -1, "libbmi_client.so imports a key set with both secret keys (a client reloading its own file): an "
                           "evaluation-only context is libbmi_tfhe.so's");
    if (int rc = import_keys_canonical(c, bsk, ksk)) return rc;
    if (int rc = import_keys_store(c, sk_small, sk_big, bsk, ksk)) return rc;
    return hold_eval_keys(c);
}

int bmi_export_keys(const bmi_ctx *c, uint64_t *sk_small, uint64_t *sk_big, uint64_t *bsk, uint64_t *ksk) {
    return hc::export_keys(c, sk_small, sk_big, bsk, ksk);
}

int bmi_encrypt(bmi_ctx *c, const int64_t *msgs, uint32_t count, uint32_t delta_log, uint64_t *ct_out) {
    return hc::encrypt(c, msgs, count, delta_log, ct_out);
}

int bmi_phase(const bmi_ctx *c, const uint64_t *ct_in, uint32_t count, uint64_t *phase) { return hc::phase(c, ct_in, count, phase); }

int bmi_decrypt(const bmi_ctx *c, const uint64_t *ct_in, uint32_t count, uint32_t delta_log, int64_t *msgs) {
    return hc::decrypt(c, ct_in, count, delta_log, msgs);
}

int bmi_set_bsk_precision(bmi_ctx *c, uint32_t bits) {
    if (!c) return -1;
    return hc::set_bsk_precision(c, settings_of(c), held_of(c), bits);
}

int bmi_get_bsk_precision(const bmi_ctx *c, uint32_t *bits) { return hc::get_bsk_precision(c, bits); }

int bmi_set_bsk_unroll(bmi_ctx *c, uint32_t factor) {
    if (!c) return -1;
    bool generated = false;
    if (int rc = hc::set_bsk_unroll(c, settings_of(c), held_of(c), factor, &generated)) return rc;
    return generated ? hold_bsk3(c) : 0;
}

int bmi_import_bsk_unrolled(bmi_ctx *c, const uint64_t *bsk3) {
    if (!c || !bsk3) return -1;
    if (int rc = import_bsk_unrolled_store(c, settings_of(c), held_of(c), bsk3)) return rc;
    return hold_bsk3(c);
}

int bmi_export_bsk_unrolled(const bmi_ctx *c, uint64_t *bsk3) { return hc::export_bsk_unrolled(c, bsk3); }

int bmi_seeded_mask_words(const uint32_t pub_key[8], uint64_t nonce, uint64_t first_word, uint64_t count, uint64_t *out) {
    return seeded_mask_words_checked(pub_key, nonce, first_word, count, out);
}

int bmi_export_keys_seeded(const bmi_ctx *c, uint32_t pub_key[8], uint64_t *bsk_bodies, uint64_t *ksk_bodies) {
    return hc::export_keys_seeded(c, pub_key, bsk_bodies, ksk_bodies);
}

int bmi_export_bsk_unrolled_seeded(const bmi_ctx *c, uint64_t *bsk3_bodies) { return hc::export_bsk_unrolled_seeded(c, bsk3_bodies); }

int bmi_encrypt_seeded(bmi_ctx *c, const int64_t *msgs, uint32_t count, uint32_t delta_log, uint64_t *first_counter, uint64_t *bodies) {
    return hc::encrypt_seeded(c, msgs, count, delta_log, first_counter, bodies);
}

int bmi_compression_keygen(bmi_ctx *c, uint32_t levels, uint32_t base_log) {
    if (!c) return -1;
    if (int rc = compression_keygen_refusal(c, levels, base_log)) return rc;
    gen_compression_key(c, levels, base_log);
    c->pk_levels = levels;
    c->pk_base_log = base_log;
    c->pksk_from_stream = compression_key_from_stream(c);
    return 0;
}

int bmi_compression_key_info(const bmi_ctx *c, uint32_t *levels, uint32_t *base_log, uint64_t *device_bytes) {
    if (!c) return -1;
    if (levels) *levels = c->pk_levels;
    if (base_log) *base_log = c->pk_base_log;
    if (device_bytes) *device_bytes = 0;   // no device
    return 0;
}

int bmi_export_compression_key(const bmi_ctx *c, uint64_t *key) { return hc::export_compression_key(c, key); }

int bmi_import_compression_key(bmi_ctx *c, uint32_t levels, uint32_t base_log, const uint64_t *key) {
    if (!c || !key) return -1;
    if (int rc = import_compression_key_refusal(c, levels, base_log)) return rc;
    import_compression_key_store(c, levels, key);
    c->pk_levels = levels;
    c->pk_base_log = base_log;
    return 0;
}

int bmi_export_compression_key_seeded(const bmi_ctx *c, uint64_t *bodies) { return hc::export_compression_key_seeded(c, bodies); }

int bmi_compressed_words(const bmi_ctx *c, uint32_t count, uint64_t *words) { return hc::compressed_words(c, count, words); }

int bmi_phase_compressed(const bmi_ctx *c, const uint32_t *data, uint32_t count, uint32_t log_modulus, uint64_t *phase) {
    return hc::phase_compressed(c, data, count, log_modulus, phase);
}

int bmi_decrypt_compressed(const bmi_ctx *c, const uint32_t *data, uint32_t count, uint32_t log_modulus, uint32_t delta_log, int64_t *msgs) {
    return hc::decrypt_compressed(c, data, count, log_modulus, delta_log, msgs);
}

}  // extern "C"
