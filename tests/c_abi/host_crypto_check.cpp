// Holds csrc/host_crypto.hpp - the library's host cryptography - to oracle/tfhe_oracle.c on the CPU: no GPU, no library, the header
// alone, linked with the oracle compiled as plain C (no OpenMP).  tests/test_host_crypto.py builds this once with the address and
// undefined-behaviour sanitizers and once with the thread sanitizer, and runs it.
//
// k = 1 on each modulus (q_bits 64, 49, 65 = the 2^64 torus), two shapes:
//   tiny      n = 5 (odd: the unrolled key's s_n = 0 completion), N = 8, l = 3, 3 keyswitch levels, compression key (1, 16), 9 encryptions
//   threaded  n = 23, N = 64, l = 3, 3 keyswitch levels, compression key (2, 16), 130 encryptions: every generator has at least 128
//             rows (bsk 138, bsk3 216, ksk 192, pksk 128), so parallel_for (serial below 4 x threads rows, at most 32 threads) runs threads
// Deterministic keys: sk_small, sk_big, bsk, ksk, bsk3, encryptions (first = 0 and 7), phases and decode word for word against the oracle.
// CSPRNG keys (fixed ChaCha20 keys, written below): the RFC 7539 block; on the torus every mask word of every row is the seeded
// format's word (seeded_mask_words of (domain << 56) | row from word 0), on every modulus it is the row's public stream; the
// bodies-only encryption is the last word of the full one.
// Both: every row's phase - computed with this file's own schoolbook product - is its message term plus noise, |noise| <= 8.6 sigma q + 1:
// Box-Muller on a 53-bit uniform cannot exceed sqrt(2 * 53 * ln 2) = 8.57 standard deviations, and the rounding adds at most 1/2.
// A GGSW row of component comp < k has the phase -g S_comp whether the message went into the mask (deterministic keys) or the body
// (CSPRNG keys); the mask checks above tell the two apart.  The compression key has no oracle twin: the phase check is its test.
#include <cstdio>
#include <string>

#include "../../bounty-matrix-inversion_amd/csrc/host_crypto.hpp"

using namespace hc;

extern "C" {
struct ora_params {   // = bmi_params (oracle/tfhe_oracle.c)
    uint32_t n, log_N, k, bs_levels, bs_base_log, ks_levels, ks_base_log, q_bits;
    double lwe_noise, glwe_noise;
};
int ora_set_field(uint32_t q_bits);
void ora_keygen(const ora_params *P, u64 seed, u64 *sk_small, u64 *sk_big, u64 *bsk, u64 *ksk);
void ora_keygen_bsk_unrolled(const ora_params *P, u64 seed, const u64 *sk_small, const u64 *sk_big, u64 *bsk3);
void ora_lwe_encrypt(const u64 *key, uint32_t dim, double noise, u64 seed, u64 first, const u64 *torus, uint32_t count, u64 *out);
void ora_lwe_phase(const u64 *key, uint32_t dim, const u64 *cts, uint32_t count, u64 *phase);
void ora_decode(const u64 *phase, uint32_t count, uint32_t delta_log, i64 *msg);
}

static int g_failed = 0, g_checked = 0;
static std::string g_case;
static void check(bool ok, const char *what) {
    g_checked++;
    if (ok) return;
    g_failed++;
    std::printf("FAIL %s: %s\n", g_case.c_str(), what);
}

struct Shape {
    const char *name;
    uint32_t n, log_N, l, bs_base_log, ks_levels, ks_base_log, pk_levels, pk_base_log, encryptions;
};
static const Shape SHAPES[] = {{"tiny", 5, 3, 3, 10, 3, 4, 1, 16, 9}, {"threaded", 23, 6, 3, 10, 3, 4, 2, 16, 130}};
static const u64 SEED = 0x5EED;
// the CSPRNG path's keys: fixed, so that a failure reproduces (the library fills them from getrandom)
static const ChaKey SECRET_KEY = {{0x243F6A88u, 0x85A308D3u, 0x13198A2Eu, 0x03707344u, 0xA4093822u, 0x299F31D0u, 0x082EFA98u, 0xEC4E6C89u}};
static const ChaKey PUBLIC_KEY = {{0x452821E6u, 0x38D01377u, 0xBE5466CFu, 0x34E90C6Cu, 0xC0AC29B7u, 0xC97C50DDu, 0x3F84D5B5u, 0xB5470917u}};

// out = a * s in Z_q[X] / (X^N + 1), schoolbook: this file's own product, which the header's shifted adds are held to
static std::vector<u64> negacyclic(const Fq &f, const u64 *a, const u64 *s, uint32_t N) {
    std::vector<u64> out(N, 0);
    for (uint32_t i = 0; i < N; i++)
        for (uint32_t j = 0; j < N; j++) {
            const u64 p = f.mul(a[i], s[j]);
            if (i + j < N) out[i + j] = f.add(out[i + j], p);
            else out[i + j - N] = f.sub(out[i + j - N], p);
        }
    return out;
}
// |centred(x)| <= 8.6 sigma q + 1
static bool is_noise(const Fq &f, u64 x, double sigma) {
    const double bound = 8.6 * sigma * (f.bits == 64 ? 18446744073709551616.0 : (double)f.q) + 1.0;
    return std::fabs((double)f.centered(x)) <= bound;
}
// the first `count` mask words of (domain, row): the row's public stream on every modulus, and on the torus the seeded format's words
static bool masks_are_the_stream(const Sampler &s, u64 domain, u64 row, const u64 *masks, uint32_t count) {
    RowRng r = s.mask(domain, row);
    std::vector<u64> words(count);
    seeded_mask_words(s.pub.k, (domain << 56) | row, 0, count, words.data());
    for (uint32_t x = 0; x < count; x++)
        if (masks[x] != r.uniform(0) || (s.f.torus && masks[x] != words[x])) return false;
    return true;
}

// GLWE rows [A | B] (k = 1) under S: B - A S = message polynomial + noise
static bool glwe_phase_is(const Fq &f, const u64 *row, const u64 *S, uint32_t N, const std::vector<u64> &message, double sigma) {
    const std::vector<u64> AS = negacyclic(f, row, S, N);
    for (uint32_t x = 0; x < N; x++)
        if (!is_noise(f, f.sub(f.sub(row[N + x], AS[x]), message[x]), sigma)) return false;
    return true;
}
// GGSW rows of the bits msg (k = 1): the row of component comp, level lev of bit b has the phase b g (-S, or 1 for comp = k), g = 2^(bits - Bg (lev + 1))
static void check_ggsw(const Sampler &s, u64 mask_domain, const u64 *sk_big, uint32_t N, uint32_t l, uint32_t base_log, double sigma,
                       const std::vector<u64> &msg, const std::vector<u64> &key, const char *what) {
    bool phases = true, masks = true;
    for (size_t ir = 0; ir < msg.size() * 2 * l; ir++) {
        const uint32_t comp = (uint32_t)(ir % (2 * l)) / l, lev = (uint32_t)(ir % l);
        const u64 g = s.f.mul(msg[ir / (2 * l)], (u64)1 << (s.f.bits - base_log * (lev + 1)));
        std::vector<u64> message(N, 0);
        if (comp == 1) message[0] = g;
        else
            for (uint32_t x = 0; x < N; x++) message[x] = s.f.neg(s.f.mul(g, sk_big[x]));
        const u64 *row = key.data() + ir * 2 * N;
        phases = phases && glwe_phase_is(s.f, row, sk_big, N, message, sigma);
        if (s.secure) masks = masks && masks_are_the_stream(s, mask_domain, ir, row, N);
    }
    check(phases, (std::string(what) + ": a row's phase is not its message plus noise").c_str());
    check(masks, (std::string(what) + ": a mask word is not the public stream's (a message in the mask tells the key bit)").c_str());
}

static void run(uint32_t q_bits, const Shape &sh, bool secure) {
    const Fq f = q_bits == 49 ? Fq{FIELD49_Q, 49, false} : q_bits == 65 ? Fq{0, 64, true} : Fq{};
    g_case = std::string(sh.name) + " q_bits " + std::to_string(q_bits) + (secure ? " csprng" : " deterministic");
    const uint32_t n = sh.n, N = 1u << sh.log_N, l = sh.l, rows = 2 * l, pairs = (n + 1) / 2;
    const ora_params P = {n, sh.log_N, 1, l, sh.bs_base_log, sh.ks_levels, sh.ks_base_log, q_bits, std::ldexp(1.0, -25),
                          std::ldexp(1.0, q_bits == 49 ? -40 : -44)};
    const Sampler s = {SEED, f, secure, SECRET_KEY, PUBLIC_KEY};
    const uint32_t delta_log = f.bits - 1 - 4;

    // ---- the header's keys
    std::vector<u64> sk_small(n), sk_big(N), bsk((size_t)n * rows * 2 * N), ksk((size_t)N * sh.ks_levels * (n + 1)),
        bsk3((size_t)pairs * 3 * rows * 2 * N);
    secret_key_bits(s, S_SK_SMALL, n, sk_small.data());
    secret_key_bits(s, S_SK_BIG, N, sk_big.data());
    check(is_binary(sk_small.data(), n) && is_binary(sk_big.data(), N), "secret keys are not binary");
    ggsw_rows(s, S_BSK_MASK, S_BSK_NOISE, sk_big.data(), N, 1, l, sh.bs_base_log, P.glwe_noise, sk_small.data(), n, bsk.data());
    const std::vector<u64> msg3 = unrolled_messages(sk_small.data(), n);
    check(msg3.size() == (size_t)pairs * 3, "the unrolled key has three messages per pair");
    ggsw_rows(s, S_BSK3_MASK, S_BSK3_NOISE, sk_big.data(), N, 1, l, sh.bs_base_log, P.glwe_noise, msg3.data(), msg3.size(), bsk3.data());
    ksk_rows(s, sk_small.data(), n, sk_big.data(), N, sh.ks_levels, sh.ks_base_log, P.lwe_noise, ksk.data());

    // ---- phases: message plus noise, on this file's own products and messages
    check_ggsw(s, S_BSK_MASK, sk_big.data(), N, l, sh.bs_base_log, P.glwe_noise, sk_small, bsk, "bsk");
    std::vector<u64> own3((size_t)pairs * 3);   // s s', s (1 - s'), (1 - s) s' with s_n = 0, in integers
    for (uint32_t i = 0; i < pairs; i++) {
        const u64 a = sk_small[2 * i], b = 2 * i + 1 < n ? sk_small[2 * i + 1] : 0;
        own3[3 * i] = a * b, own3[3 * i + 1] = a * (1 - b), own3[3 * i + 2] = (1 - a) * b;
    }
    check(own3 == msg3, "the unrolled key's messages are not s s', s (1 - s'), (1 - s) s'");
    check_ggsw(s, S_BSK3_MASK, sk_big.data(), N, l, sh.bs_base_log, P.glwe_noise, own3, bsk3, "bsk3");
    {
        bool phases = true, masks = true;
        for (size_t jr = 0; jr < (size_t)N * sh.ks_levels; jr++) {
            const u64 *row = ksk.data() + jr * (n + 1);
            u64 p = row[n];
            for (uint32_t x = 0; x < n; x++) p = f.sub(p, f.mul(row[x], sk_small[x]));
            const u64 m = f.mul(sk_big[jr / sh.ks_levels], (u64)1 << (f.bits - sh.ks_base_log * (jr % sh.ks_levels + 1)));
            phases = phases && is_noise(f, f.sub(p, m), P.lwe_noise);
            if (secure) masks = masks && masks_are_the_stream(s, S_KSK_MASK, jr, row, n);
        }
        check(phases, "ksk: a row's phase is not its message plus noise");
        check(masks, "ksk: a mask word is not the public stream's");
    }
    if (f.torus) {   // the compression key exists on the torus only
        std::vector<u64> pksk((size_t)N * sh.pk_levels * 2 * N);
        compression_key_rows(s, sk_big.data(), N, sh.pk_levels, sh.pk_base_log, P.glwe_noise, pksk.data());
        bool phases = true, masks = true;
        for (size_t jr = 0; jr < (size_t)N * sh.pk_levels; jr++) {
            std::vector<u64> message(N, 0);   // S_j 2^(64 - base_log (lev + 1)) at coefficient 0, zero elsewhere
            message[0] = sk_big[jr / sh.pk_levels] << (64 - sh.pk_base_log * (jr % sh.pk_levels + 1));
            phases = phases && glwe_phase_is(f, pksk.data() + jr * 2 * N, sk_big.data(), N, message, P.glwe_noise);
            if (secure) masks = masks && masks_are_the_stream(s, S_PKSK_MASK, jr, pksk.data() + jr * 2 * N, N);
        }
        check(phases, "compression key: a row's phase is not S_j 2^(64 - base_log (lev + 1)) at coefficient 0 plus noise");
        check(masks, "compression key: a mask word is not the public stream's");
        // column_bias on it: 2^(base_log - 1) times the column sums
        std::vector<u64> bias(2 * N), want(2 * N, 0);
        column_bias(f, pksk.data(), (size_t)N * sh.pk_levels, 2 * N, sh.pk_base_log, bias.data());
        for (size_t i = 0; i < pksk.size(); i++) want[i % (2 * N)] += pksk[i] << (sh.pk_base_log - 1);
        check(bias == want, "column_bias is not half the base times the column sums");
        // the phase of a compressed block: body 2^(64 - log_modulus) - (A S)_i
        std::vector<uint32_t> data(2 * N);
        for (uint32_t x = 0; x < 2 * N; x++) data[x] = (uint32_t)(mix64(x) & 0xFFFF);
        std::vector<u64> A(N), got(N - 1);
        for (uint32_t x = 0; x < N; x++) A[x] = (u64)data[x] << 48;
        const std::vector<u64> AS = negacyclic(f, A.data(), sk_big.data(), N);
        bool same = compressed_phase(f, sk_big.data(), N, data.data(), N - 1, 16, got.data());
        for (uint32_t i = 0; i + 1 < N; i++) same = same && got[i] == ((u64)data[N + i] << 48) - AS[i];
        check(same, "compressed_phase is not body - (A S)_i");
        data[3] = 1u << 16;
        check(!compressed_phase(f, sk_big.data(), N, data.data(), N - 1, 16, got.data()), "compressed_phase took a value of 17 bits");
    }

    // ---- encryptions at the counters 0 and 7, phases, bodies-only form
    std::vector<int64_t> msgs(sh.encryptions);
    for (uint32_t i = 0; i < sh.encryptions; i++) msgs[i] = (int64_t)(i % 16) - 8;
    for (const u64 first : {(u64)0, (u64)7}) {
        std::vector<u64> ct((size_t)sh.encryptions * (N + 1)), bodies(sh.encryptions), ph(sh.encryptions), torus(sh.encryptions);
        lwe_encrypt(s, sk_big.data(), N, P.glwe_noise, first, msgs.data(), sh.encryptions, delta_log, ct.data(), nullptr);
        lwe_encrypt(s, sk_big.data(), N, P.glwe_noise, first, msgs.data(), sh.encryptions, delta_log, nullptr, bodies.data());
        lwe_phase(f, sk_big.data(), N, ct.data(), sh.encryptions, ph.data());
        bool body_ok = true, phases = true, masks = true, decoded = true;
        for (uint32_t i = 0; i < sh.encryptions; i++) {
            torus[i] = f.mul(f.from_i64(msgs[i]), (u64)1 << delta_log);
            body_ok = body_ok && bodies[i] == ct[(size_t)i * (N + 1) + N];
            phases = phases && is_noise(f, f.sub(ph[i], torus[i]), P.glwe_noise);
            decoded = decoded && decode(f, ph[i], delta_log) == msgs[i];
            if (secure) masks = masks && masks_are_the_stream(s, S_ENC_MASK, first + i, ct.data() + (size_t)i * (N + 1), N);
        }
        check(body_ok, "the bodies-only encryption is not the last word of the full one");
        check(phases, "encryption: a phase is not its message plus noise");
        check(decoded, "encryption: a phase does not decode to its message");
        check(masks, "encryption: a mask word is not the public stream's");
        if (secure) continue;
        std::vector<u64> o_ct(ct.size()), o_ph(sh.encryptions);
        ora_lwe_encrypt(sk_big.data(), N, P.glwe_noise, SEED, first, torus.data(), sh.encryptions, o_ct.data());
        check(ct == o_ct, first ? "encryptions at first = 7 differ from ora_lwe_encrypt" : "encryptions at first = 0 differ from ora_lwe_encrypt");
        ora_lwe_phase(sk_big.data(), N, ct.data(), sh.encryptions, o_ph.data());
        check(ph == o_ph, "phases differ from ora_lwe_phase");
    }
    if (secure) return;

    // ---- deterministic keys: word for word the oracle's
    std::vector<u64> o_small(n), o_big(N), o_bsk(bsk.size()), o_ksk(ksk.size()), o_bsk3(bsk3.size());
    ora_keygen(&P, SEED, o_small.data(), o_big.data(), o_bsk.data(), o_ksk.data());
    ora_keygen_bsk_unrolled(&P, SEED, o_small.data(), o_big.data(), o_bsk3.data());
    check(sk_small == o_small, "sk_small differs from ora_keygen");
    check(sk_big == o_big, "sk_big differs from ora_keygen");
    check(bsk == o_bsk, "bsk differs from ora_keygen");
    check(ksk == o_ksk, "ksk differs from ora_keygen");
    check(bsk3 == o_bsk3, "bsk3 differs from ora_keygen_bsk_unrolled");

    // ---- decode on every residue of a 4-bit message, exactly and at both rounding ties (and one word inside each)
    std::vector<u64> ph;
    const u64 half = (u64)1 << (delta_log - 1);
    for (int64_t m = -8; m < 8; m++) {
        const u64 centre = f.mul(f.from_i64(m), (u64)1 << delta_log);
        for (const u64 p : {centre, f.add(centre, half), f.sub(centre, half), f.add(centre, half - 1), f.sub(centre, half - 1)}) ph.push_back(p);
    }
    std::vector<i64> want(ph.size());
    ora_decode(ph.data(), (uint32_t)ph.size(), delta_log, want.data());
    bool same = true;
    for (size_t i = 0; i < ph.size(); i++) same = same && decode(f, ph[i], delta_log) == want[i];
    check(same, "decode differs from ora_decode");
}

int main() {
    // RFC 7539 section 2.3.2 (key bytes 00 .. 1f, block counter 1, nonce 00:00:00:09 00:00:00:4a 00:00:00:00) in the 64-bit-counter
    // variant: state words 12 .. 15 are (counter64 low, high, nonce64 low, high) - as tests/test_seeded_stream.py
    g_case = "chacha20";
    ChaKey rfc;
    for (uint32_t i = 0; i < 8; i++) rfc.k[i] = (4 * i) | ((4 * i + 1) << 8) | ((4 * i + 2) << 16) | ((4 * i + 3) << 24);
    const uint32_t want[16] = {0xe4e7f110, 0x15593bd1, 0x1fdd0f50, 0xc47120a3, 0xc7f4d1c7, 0x0368c033, 0x9aaa2204, 0x4e6cd4c3,
                               0x466482d2, 0x09aa9f07, 0x05d7c214, 0xa2028bd9, 0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2};
    uint32_t block[16];
    chacha_block(rfc, 0x4A000000ULL, 1ULL | (0x09000000ULL << 32), block);
    check(std::memcmp(block, want, sizeof(want)) == 0, "the block of RFC 7539 section 2.3.2");

    for (const uint32_t q_bits : {64u, 49u, 65u}) {
        ora_set_field(q_bits);
        for (const Shape &sh : SHAPES)
            for (const bool secure : {false, true}) run(q_bits, sh, secure);
    }
    std::printf("%d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
