// Calls the C functions libbmi_client.so exports (include/bmi_client.h), compiled together with csrc/bmi_client.cpp into one program
// of its own: no GPU, no Python.  tests/test_client_library.py builds it once with the address and undefined-behaviour sanitizers and
// once with the thread sanitizer, and runs it.
//
// On each modulus (q_bits 65 = the 2^64 torus, 49, 64), at the smallest shapes the library admits that still start threads in every
// generator (N = 1024, l = 3, n = 23 - odd: the unrolled key's s_n = 0 completion; bsk 138 rows, ksk 8,192, compression key 1,024;
// parallel_for is serial below 4 x threads rows and runs at most 32 threads): deterministic keygen twice into two contexts - the same
// words; the exports; 130 encryptions, their phases and decryption; import of the exported set with its secret keys - the same
// exports again; the unrolled key after the key set; CSPRNG keygen with the seeded exports and seeded encryptions (torus) or their
// refusal (prime fields); the compression key (torus), decrypt_compressed on a block whose mask values are zero (its phases are the
// body values shifted up, whatever the key), and every refusal on the way, with the text libbmi_tfhe.so gives.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bmi_client.h"

typedef uint64_t u64;

static int g_failed = 0, g_checked = 0;
static std::string g_case;
static void check(bool ok, const char *what) {
    g_checked++;
    if (ok) return;
    g_failed++;
    std::printf("FAIL %s: %s\n", g_case.c_str(), what);
}
// rc != 0 and the context's (or, with a null context, the creation's) error text contains `text`
static void refused(int rc, const bmi_ctx *c, const char *text, const char *what) {
    const std::string err = bmi_last_error(c);
    check(rc != 0 && err.find(text) != std::string::npos, (std::string(what) + " is refused with its text (got: " + err + ")").c_str());
}

struct Keys {
    std::vector<u64> sk_small, sk_big, bsk, ksk;
    bool operator==(const Keys &o) const { return sk_small == o.sk_small && sk_big == o.sk_big && bsk == o.bsk && ksk == o.ksk; }
};
static Keys exported(const bmi_ctx *c, const bmi_params &P) {
    const size_t N = (size_t)1 << P.log_N;
    Keys k{std::vector<u64>(P.n), std::vector<u64>(N), std::vector<u64>((size_t)P.n * 2 * P.bs_levels * 2 * N),
           std::vector<u64>(N * P.ks_levels * (P.n + 1))};
    check(bmi_export_keys(c, k.sk_small.data(), k.sk_big.data(), k.bsk.data(), k.ksk.data()) == 0, "bmi_export_keys");
    return k;
}

static void run_modulus(uint32_t q_bits) {
    g_case = "q_bits " + std::to_string(q_bits);
    const bool torus = q_bits == BMI_Q_TORUS64;
    bmi_params P;
    check(bmi_default_params_for(q_bits, &P) == 0 && P.q_bits == q_bits, "bmi_default_params_for");
    P.n = 23;
    const uint32_t N = 1u << P.log_N, delta_log = (q_bits == 49 ? 49 : 64) - 5, count = 130;

    // ---- creation and its refusals
    bmi_ctx *c = nullptr, *d = nullptr;
    refused(bmi_ctx_create(&P, 0, &c), nullptr, "libbmi_tfhe.so", "a device index");
    bmi_params bad = P;
    bad.log_N = 9;
    refused(bmi_ctx_create(&bad, BMI_CLIENT_NO_DEVICE, &c), nullptr, "log_N must be 10", "N = 512");
    bad = P;
    bad.k = 2;
    refused(bmi_ctx_create(&bad, BMI_CLIENT_NO_DEVICE, &c), nullptr, "only k = 1", "k = 2");
    bad = P;
    bad.bs_base_log = 12;
    refused(bmi_ctx_create(&bad, BMI_CLIENT_NO_DEVICE, &c), nullptr, "(l, Bg) must be", "base 2^12");
    bad = P;
    bad.n = 1025;
    refused(bmi_ctx_create(&bad, BMI_CLIENT_NO_DEVICE, &c), nullptr, "n must be in [1, 1024]", "n = 1025");
    refused(bmi_ctx_create(nullptr, BMI_CLIENT_NO_DEVICE, &c), nullptr, "null argument", "null parameters");
    check(bmi_ctx_create(&P, BMI_CLIENT_NO_DEVICE, &c) == 0 && c, "bmi_ctx_create");
    check(bmi_ctx_create(&P, BMI_CLIENT_NO_DEVICE, &d) == 0 && d, "bmi_ctx_create (second context)");
    if (!c || !d) return;
    bmi_params got;
    check(bmi_get_params(c, &got) == 0 && std::memcmp(&got, &P, sizeof(P)) == 0, "bmi_get_params");

    // ---- before any key
    std::vector<int64_t> msgs(count), back(count);
    for (uint32_t i = 0; i < count; i++) msgs[i] = (int64_t)(i % 16) - 8;
    std::vector<u64> ct((size_t)count * (N + 1)), ct2(ct.size()), ph(count);
    refused(bmi_export_keys(c, nullptr, nullptr, nullptr, nullptr), c, "no keys: call bmi_keygen first", "an export before keygen");
    refused(bmi_encrypt(c, msgs.data(), count, delta_log, ct.data()), c, "no keys: call bmi_keygen first", "an encryption before keygen");
    uint32_t prec = 0;
    check(bmi_get_bsk_precision(c, &prec) == 0 && prec == (torus ? 48u : 64u), "bmi_get_bsk_precision of a new context");
    if (torus) {
        refused(bmi_set_bsk_precision(c, 47), c, "must be 64 (exact), 48, 46, 44, 42 or 40", "a precision of 47 bits");
        check(bmi_set_bsk_precision(c, 64) == 0 && bmi_get_bsk_precision(c, &prec) == 0 && prec == 64, "bmi_set_bsk_precision(64)");
        check(bmi_set_bsk_precision(c, 48) == 0, "bmi_set_bsk_precision(48)");
    } else {
        refused(bmi_set_bsk_precision(c, 48), c, "2^64 torus only", "a key precision on a prime field");
    }
    refused(bmi_set_bsk_unroll(c, 3), c, "the unrolling factor is 1 or 2", "an unrolling factor of 3");

    // ---- deterministic keys: two contexts, the same words
    check(bmi_keygen_insecure_deterministic(c, 0x5EED) == 0, "bmi_keygen_insecure_deterministic");
    check(bmi_keygen_insecure_deterministic(d, 0x5EED) == 0, "bmi_keygen_insecure_deterministic (second context)");
    const Keys kc = exported(c, P), kd = exported(d, P);
    check(kc == kd, "two contexts generate the same keys from one seed");
    bool binary = true, rounded = true;
    for (u64 w : kc.sk_small) binary = binary && w <= 1;
    for (u64 w : kc.sk_big) binary = binary && w <= 1;
    check(binary, "secret keys are binary");
    if (torus)
        for (u64 w : kc.bsk) rounded = rounded && (w & 0xFFFF) == 0;
    check(rounded, "torus bootstrap key words are multiples of 2^16 at 48 bits of precision");
    if (torus) refused(bmi_set_bsk_precision(c, 64), c, "before generating or importing keys", "a precision after keygen");

    // ---- encryption, phase, decryption
    check(bmi_encrypt(c, msgs.data(), count, delta_log, ct.data()) == 0, "bmi_encrypt");
    check(bmi_encrypt(d, msgs.data(), count, delta_log, ct2.data()) == 0 && ct == ct2, "encryption i of a key set is reproducible");
    check(bmi_decrypt(c, ct.data(), count, delta_log, back.data()) == 0 && back == msgs, "bmi_decrypt returns the messages");
    check(bmi_phase(c, ct.data(), count, ph.data()) == 0, "bmi_phase");
    refused(bmi_decrypt(c, ct.data(), count, 0, back.data()), c, "delta_log out of range", "delta_log 0");
    refused(bmi_encrypt(c, msgs.data(), count, 63, ct.data()), c, "delta_log out of range", "delta_log 63");
    check(bmi_encrypt(c, nullptr, count, delta_log, ct.data()) == -1, "null messages");

    // ---- import: with the secret keys the same exports, without them refused
    refused(bmi_import_keys(d, nullptr, nullptr, kc.bsk.data(), kc.ksk.data()), d, "libbmi_tfhe.so", "an import without secret keys");
    refused(bmi_import_keys(d, kc.sk_small.data(), nullptr, kc.bsk.data(), kc.ksk.data()), d, "pass both secret keys or neither", "one secret key");
    check(bmi_import_keys(d, kc.sk_small.data(), kc.sk_big.data(), kc.bsk.data(), kc.ksk.data()) == 0, "bmi_import_keys");
    check(exported(d, P) == kc, "an imported key set is exported word for word");
    check(bmi_decrypt(d, ct.data(), count, delta_log, back.data()) == 0 && back == msgs, "the importing context decrypts");
    if (q_bits != BMI_Q_TORUS64) {
        std::vector<u64> big = kc.bsk;
        big[5] = ~(u64)0;
        refused(bmi_import_keys(d, kc.sk_small.data(), kc.sk_big.data(), big.data(), kc.ksk.data()), d, "not reduced mod q", "a word not below q");
    }
    std::vector<u64> two = kc.sk_small;
    two[0] = 2;
    refused(bmi_keygen_from_secret(d, two.data(), kc.sk_big.data(), 7), d, "secret keys are binary", "a key bit of 2");
    check(bmi_keygen_from_secret(d, kc.sk_small.data(), kc.sk_big.data(), 0x5EED) == 0 && exported(d, P) == kc,
          "bmi_keygen_from_secret with the seed's own secret keys gives the seed's evaluation keys");

    // ---- the unrolled key
    const size_t words3 = (size_t)((P.n + 1) / 2) * 3 * 2 * P.bs_levels * 2 * N;
    std::vector<u64> bsk3(words3), bsk3d(words3);
    refused(bmi_export_bsk_unrolled(c, bsk3.data()), c, "no unrolled bootstrap key", "an unrolled export before the mode is set");
    if (q_bits == 64) {
        refused(bmi_set_bsk_unroll(c, 2), c, "49-bit field and the 2^64 torus", "unrolling on Goldilocks");
        refused(bmi_import_bsk_unrolled(c, bsk3.data()), c, "49-bit field and the 2^64 torus", "an unrolled import on Goldilocks");
    } else {
        check(bmi_set_bsk_unroll(c, 2) == 0 && bmi_export_bsk_unrolled(c, bsk3.data()) == 0, "bmi_set_bsk_unroll(2) on a key set, and its export");
        check(bmi_import_bsk_unrolled(d, bsk3.data()) == 0 && bmi_export_bsk_unrolled(d, bsk3d.data()) == 0 && bsk3 == bsk3d,
              "an imported unrolled key is exported word for word");
        check(bmi_set_bsk_unroll(c, 1) == 0, "bmi_set_bsk_unroll(1)");
    }

    // ---- the seeded forms and the compression key: the deterministic key set
    uint32_t pub[8];
    std::vector<u64> bsk_body((size_t)P.n * 2 * P.bs_levels * N), ksk_body((size_t)N * P.ks_levels), bodies(count);
    u64 first = 99;
    const char *const no_seeded = torus ? "deterministic test keys" : "seeded forms exist on the 2^64 torus only";
    refused(bmi_export_keys_seeded(c, pub, bsk_body.data(), ksk_body.data()), c, no_seeded, "a seeded export of deterministic keys");
    refused(bmi_encrypt_seeded(c, msgs.data(), count, delta_log, &first, bodies.data()), c, no_seeded, "a seeded encryption under deterministic keys");
    u64 words = 0;
    uint32_t lv = 9, bl = 9;
    u64 dev_bytes = 9;
    std::vector<u64> pksk((size_t)N * 2 * N);
    if (!torus) {
        refused(bmi_compression_keygen(c, 1, 16), c, "2^64 torus only", "a compression key on a prime field");
        refused(bmi_compressed_words(c, 5, &words), c, "2^64 torus only", "bmi_compressed_words on a prime field");
        refused(bmi_decrypt_compressed(c, nullptr, 0, 16, delta_log, nullptr), c, "2^64 torus only", "bmi_decrypt_compressed on a prime field");
    } else {
        check(bmi_compression_key_info(c, &lv, &bl, &dev_bytes) == 0 && lv == 0 && bl == 0 && dev_bytes == 0, "no compression key yet");
        refused(bmi_export_compression_key(c, pksk.data()), c, "no compression key", "an export without a compression key");
        refused(bmi_compression_keygen(c, 5, 16), c, "1 <= levels <= 4", "a compression key of 5 levels");
        check(bmi_compression_keygen(c, 1, 16) == 0, "bmi_compression_keygen(1, 16)");
        check(bmi_compression_key_info(c, &lv, &bl, &dev_bytes) == 0 && lv == 1 && bl == 16 && dev_bytes == 0, "bmi_compression_key_info");
        refused(bmi_compression_keygen(c, 2, 16), c, "already has a compression key of shape (1, 16)", "a second compression key of another shape");
        check(bmi_compression_keygen(c, 1, 16) == 0 && bmi_export_compression_key(c, pksk.data()) == 0, "the same shape again, and its export");
        refused(bmi_export_compression_key_seeded(c, bsk_body.data()), c, "deterministic test keys", "a seeded compression key of deterministic keys");
        std::vector<u64> pksk2(pksk.size());
        check(bmi_import_compression_key(d, 1, 16, pksk.data()) == 0 && bmi_export_compression_key(d, pksk2.data()) == 0 && pksk == pksk2,
              "an imported compression key is exported word for word");
        // one partial block of 5 whose mask values are zero: phase i = body value i shifted up, under any key
        const uint32_t m = 5, log_modulus = 16;
        check(bmi_compressed_words(c, m, &words) == 0 && words == N + m, "bmi_compressed_words");
        std::vector<uint32_t> data(N + m, 0);
        for (uint32_t i = 0; i < m; i++) data[N + i] = (uint32_t)(((u64)msgs[i] << (delta_log - (64 - log_modulus))) & 0xFFFF);
        std::vector<int64_t> got5(m);
        std::vector<u64> ph5(m);
        check(bmi_decrypt_compressed(c, data.data(), m, log_modulus, delta_log, got5.data()) == 0 &&
                  std::equal(got5.begin(), got5.end(), msgs.begin()), "bmi_decrypt_compressed returns the messages");
        check(bmi_phase_compressed(c, data.data(), m, log_modulus, ph5.data()) == 0 && ph5[1] == (u64)msgs[1] << delta_log, "bmi_phase_compressed");
        data[3] = 1u << 16;
        refused(bmi_decrypt_compressed(c, data.data(), m, log_modulus, delta_log, got5.data()), c, "does not fit log_modulus bits", "a 17-bit value");
        refused(bmi_phase_compressed(c, data.data(), m, 33, ph5.data()), c, "log_modulus must be in [2, 32]", "log_modulus 33");
    }

    // ---- CSPRNG keys: a new key set drops the compression key; the seeded forms on the torus
    check(bmi_keygen(c) == 0, "bmi_keygen");
    const Keys ks = exported(c, P);
    check(!(ks == kc), "CSPRNG keys differ from the seeded ones");
    check(bmi_encrypt(c, msgs.data(), count, delta_log, ct.data()) == 0 && bmi_decrypt(c, ct.data(), count, delta_log, back.data()) == 0 &&
              back == msgs, "encryption and decryption under CSPRNG keys");
    if (torus) {
        check(bmi_compression_key_info(c, &lv, &bl, &dev_bytes) == 0 && lv == 0, "a new key set drops the compression key");
        check(bmi_export_keys_seeded(c, pub, bsk_body.data(), ksk_body.data()) == 0, "bmi_export_keys_seeded");
        bool bodies_ok = true;
        for (size_t r = 0; r < (size_t)N * P.ks_levels; r++) bodies_ok = bodies_ok && ksk_body[r] == ks.ksk[r * (P.n + 1) + P.n];
        check(bodies_ok, "the seeded keyswitch bodies are the key's body words");
        std::vector<u64> mask(P.n);
        check(bmi_seeded_mask_words(pub, ((u64)BMI_SEED_DOMAIN_KSK_MASK << 56) | 77, 0, P.n, mask.data()) == 0 &&
                  std::equal(mask.begin(), mask.end(), ks.ksk.begin() + (size_t)77 * (P.n + 1)),
              "row 77 of the keyswitch key takes its masks from the public stream at its nonce");
        check(bmi_encrypt_seeded(c, msgs.data(), count, delta_log, &first, bodies.data()) == 0 && first == count,
              "bmi_encrypt_seeded continues the encryption counter");
        check(bmi_compression_keygen(c, 2, 16) == 0, "another compression shape on the new key set");
        std::vector<u64> pk_body((size_t)N * 2 * N);
        check(bmi_export_compression_key_seeded(c, pk_body.data()) == 0, "bmi_export_compression_key_seeded");
        std::vector<u64> bsk3_body(words3 / 2);
        check(bmi_set_bsk_unroll(c, 2) == 0 && bmi_export_bsk_unrolled_seeded(c, bsk3_body.data()) == 0, "bmi_export_bsk_unrolled_seeded");
    } else {
        refused(bmi_export_keys_seeded(c, pub, bsk_body.data(), ksk_body.data()), c, "2^64 torus only", "a seeded export on a prime field");
    }
    bmi_ctx_destroy(c);
    bmi_ctx_destroy(d);
    bmi_ctx_destroy(nullptr);
}

int main() {
    bmi_params P;
    check(bmi_default_params(&P) == 0 && P.q_bits == BMI_Q_TORUS64 && P.n == 630, "bmi_default_params");
    check(bmi_preset_params("secure128_torus", &P) == 0 && P.n == 742 && P.log_N == 11, "bmi_preset_params");
    check(bmi_preset_params("no_such_set", &P) != 0, "an unknown preset");
    check(bmi_default_params_for(63, &P) != 0, "an unknown modulus");
    const u64 x[2] = {0, (u64)1 << 63};
    u64 y[2], z[2];
    check(bmi_torus64_to_field(49, x, 2, y) == 0 && y[0] == 0 && bmi_field_to_torus64(49, y, 2, z) == 0 && z[0] == 0, "the modulus switches");
    check(bmi_torus64_to_field(65, x, 2, y) != 0, "a modulus switch to the torus itself");
    const uint32_t torus = BMI_Q_TORUS64;
    for (uint32_t q_bits : {torus, 49u, 64u}) run_modulus(q_bits);
    std::printf("%d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
