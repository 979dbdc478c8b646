// The library's cryptography on the host, free of HIP and of the context: the two random generators, key generation, encryption,
// phase and decoding, as functions over plain arrays and sizes.  bmi_host.cpp's entry points check their arguments and the
// context's state and call these; tests/c_abi/host_crypto_check.cpp holds them to oracle/tfhe_oracle.c without a device, under the
// address, undefined-behaviour and thread sanitizers (tests/test_host_crypto.py).  A plain C++17 compiler takes this file.
#pragma once

#include <errno.h>
#include <sys/random.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/bmi_tfhe.h"

namespace hc {

using u64 = uint64_t;
using i64 = int64_t;

// the two prime moduli (bmi_host.cpp asserts them against gl::P and f49::Q)
constexpr u64 GOLDILOCKS_P = 0xFFFFFFFF00000001ULL;   // 2^64 - 2^32 + 1
constexpr u64 FIELD49_Q = 562949952700417ULL;         // 2^49 - 720895

// --------------------------------------------------------------------------- deterministic RNG
// Counter-based splitmix64 (same specification as the oracle so that key generation can be
// cross-checked bit for bit): value(stream, idx) = mix(stream_key + (idx + 1) * GOLDEN).
inline u64 mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// Arithmetic mod the context's ciphertext modulus on the host (keygen, encryption, LUT construction): plain
// 128-bit remainders - none of this is on the hot path.
struct Fq {
    u64 q = GOLDILOCKS_P;
    uint32_t bits = 64;
    bool torus = false;   // q = 2^64 exactly (q field unused): plain wrap-around arithmetic
    u64 add(u64 a, u64 b) const { return torus ? a + b : (u64)(((unsigned __int128)a + b) % q); }
    u64 sub(u64 a, u64 b) const { return torus ? a - b : (a >= b ? a - b : (u64)((unsigned __int128)a + q - b)); }
    u64 neg(u64 a) const { return torus ? (u64)0 - a : (a ? q - a : 0); }
    u64 mul(u64 a, u64 b) const { return torus ? a * b : (u64)(((unsigned __int128)a * b) % q); }
    u64 from_i64(long long v) const {  // as f49::from_i64: |v| in unsigned arithmetic, canonical for -(multiple of q)
        if (torus) return (u64)v;
        if (v >= 0) return (u64)v % q;
        const u64 m = ((u64)0 - (u64)v) % q;
        return m ? q - m : 0;
    }
    long long centered(u64 a) const { return torus ? (long long)a : (a > (q >> 1) ? (long long)(a - q) : (long long)a); }
    bool canonical(u64 a) const { return torus || a < q; }
    u64 pow(u64 b, u64 e) const {
        u64 r = 1;
        while (e) {
            if (e & 1) r = mul(r, b);
            b = mul(b, b);
            e >>= 1;
        }
        return r;
    }
};

struct Stream {
    u64 key;
    Fq f;
    Stream(u64 seed, u64 id, const Fq &fq) : key(mix64(seed ^ (id * 0xD6E8FEB86659FD93ULL))), f(fq) {}
    u64 raw(u64 idx) const { return mix64(key + (idx + 1) * 0x9E3779B97F4A7C15ULL); }
    u64 bit(u64 idx) const { return raw(idx) & 1; }
    u64 uniform(u64 idx) const {
        u64 u = raw(idx);
        if (f.torus) return u;
        return f.bits == 64 ? (u >= f.q ? u - f.q : u) : u % f.q;
    }
    u64 gauss(u64 idx, double sigma) const {  // Box-Muller, rounded to an element of Z_q
        const double u1 = (double)((raw(2 * idx) >> 11) + 1) * (1.0 / 9007199254740992.0);
        const double u2 = (double)(raw(2 * idx + 1) >> 11) * (1.0 / 9007199254740992.0);
        const double g = std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586476925286766559 * u2);
        const long long e = std::llround(g * sigma * (f.bits == 64 ? 18446744073709551616.0 : (double)f.q));
        return f.from_i64(e);
    }
};
enum : u64 { S_SK_SMALL = 1, S_SK_BIG, S_BSK_MASK, S_BSK_NOISE, S_KSK_MASK, S_KSK_NOISE, S_ENC_MASK, S_ENC_NOISE, S_BSK3_MASK, S_BSK3_NOISE, S_PKSK_MASK, S_PKSK_NOISE };
// the mask domains are part of the seeded key / ciphertext format (include/bmi_tfhe.h)
static_assert(S_BSK_MASK == BMI_SEED_DOMAIN_BSK_MASK && S_KSK_MASK == BMI_SEED_DOMAIN_KSK_MASK && S_ENC_MASK == BMI_SEED_DOMAIN_ENC_MASK &&
                  S_BSK3_MASK == BMI_SEED_DOMAIN_BSK3_MASK && S_PKSK_MASK == BMI_SEED_DOMAIN_PKSK_MASK,
              "the published stream domains are the ones key generation uses");

// --------------------------------------------------------------------------- CSPRNG (production keys and encryptions)
// ChaCha20 (D. J. Bernstein's original variant: 256-bit key, 64-bit nonce, 64-bit block counter) keyed from the
// operating system (getrandom).  Secret material (key bits, noise) and public material (masks) use two independent keys,
// so that the public evaluation-key words say nothing about the stream the secrets came from.  Every (domain, row) pair
// is its own nonce: rows are sampled in parallel and sequentially within a row.
struct ChaKey {
    uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool fill_from_os() {
        size_t got = 0;
        unsigned char *p = reinterpret_cast<unsigned char *>(k);
        while (got < sizeof(k)) {
            const ssize_t r = getrandom(p + got, sizeof(k) - got, 0);
            if (r < 0) {
                if (errno == EINTR) continue;
                return false;
            }
            got += (size_t)r;
        }
        return true;
    }
};
inline uint32_t rotl32(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }
inline void chacha_block(const ChaKey &key, u64 nonce, u64 counter, uint32_t out[16]) {
    uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key.k[0], key.k[1], key.k[2], key.k[3],
                       key.k[4], key.k[5], key.k[6], key.k[7], (uint32_t)counter, (uint32_t)(counter >> 32),
                       (uint32_t)nonce, (uint32_t)(nonce >> 32)};
    uint32_t x[16];
    for (int i = 0; i < 16; i++) x[i] = in[i];
#define BMI_QR(a, b, c, d)                  \
    x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 16); \
    x[c] += x[d]; x[b] = rotl32(x[b] ^ x[c], 12); \
    x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 8);  \
    x[c] += x[d]; x[b] = rotl32(x[b] ^ x[c], 7)
    for (int r = 0; r < 10; r++) {
        BMI_QR(0, 4, 8, 12); BMI_QR(1, 5, 9, 13); BMI_QR(2, 6, 10, 14); BMI_QR(3, 7, 11, 15);
        BMI_QR(0, 5, 10, 15); BMI_QR(1, 6, 11, 12); BMI_QR(2, 7, 8, 13); BMI_QR(3, 4, 9, 14);
    }
#undef BMI_QR
    for (int i = 0; i < 16; i++) out[i] = x[i] + in[i];
}
struct ChaStream {
    const ChaKey *key;
    u64 nonce, counter = 0;
    uint32_t buf[16];
    int pos = 16;
    ChaStream(const ChaKey &k, u64 domain, u64 row) : key(&k), nonce((domain << 56) | (row & ((1ULL << 56) - 1))) {}
    // the stream of a whole nonce, positioned at its 64-bit word `first_word` (seeded_mask_words)
    ChaStream(const ChaKey &k, u64 whole_nonce, u64 first_word, int) : key(&k), nonce(whole_nonce), counter(first_word / 8) {
        for (u64 skip = first_word % 8; skip; skip--) (void)next64();
    }
    u64 next64() {
        if (pos > 14) {
            chacha_block(*key, nonce, counter++, buf);
            pos = 0;
        }
        const u64 v = (u64)buf[pos] | ((u64)buf[pos + 1] << 32);
        pos += 2;
        return v;
    }
    u64 bit() { return next64() & 1; }
    u64 uniform(const Fq &f) {   // rejection sampling: exactly uniform on [0, q)
        for (;;) {
            const u64 u = f.bits == 64 ? next64() : next64() >> (64 - f.bits);
            if (f.torus || u < f.q) return u;
        }
    }
    u64 gauss(const Fq &f, double sigma) {
        const double u1 = (double)((next64() >> 11) + 1) * (1.0 / 9007199254740992.0);
        const double u2 = (double)(next64() >> 11) * (1.0 / 9007199254740992.0);
        const double g = std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586476925286766559 * u2);
        return f.from_i64(std::llround(g * sigma * (f.bits == 64 ? 18446744073709551616.0 : (double)f.q)));
    }
};
// One row's source of masks / noise: the CSPRNG (sequential within the row) or, for the test-only deterministic key
// generation, the counter-indexed splitmix streams the oracle reproduces bit for bit.
struct RowRng {
    Stream det;   // (its own copy: a Sampler hands these out by value)
    ChaStream cha;
    bool secure;
    RowRng(const Stream &d, const ChaKey &k, u64 domain, u64 row, bool sec) : det(d), cha(k, domain, row), secure(sec) {}
    u64 uniform(u64 idx) { return secure ? cha.uniform(det.f) : det.uniform(idx); }
    u64 gauss(u64 idx, double sigma) { return secure ? cha.gauss(det.f, sigma) : det.gauss(idx, sigma); }
    u64 bit(u64 idx) { return secure ? cha.bit() : det.bit(idx); }
};
// Where every generator below takes its randomness from: the seed of the deterministic streams, the modulus, and - when `secure` -
// the two ChaCha20 keys.  Masks are public material (key `pub`), key bits and noise secret material (key `secret`).  Copied by
// value into the rows' threads (parallel_for); a RowRng points into the copy it came from and must not outlive it.
struct Sampler {
    u64 seed = 0;
    Fq f;
    bool secure = false;
    ChaKey secret, pub;
    RowRng mask(u64 domain, u64 row) const { return RowRng(Stream(seed, domain, f), pub, domain, row, secure); }
    RowRng noise(u64 domain, u64 row) const { return RowRng(Stream(seed, domain, f), secret, domain, row, secure); }
};

template <class F>
void parallel_for(size_t n, F f) {
    unsigned nt = std::max(1u, std::min(std::thread::hardware_concurrency(), 32u));
    if (n < 4 * nt) nt = 1;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([=]() {
            for (size_t i = t; i < n; i += nt) f(i);
        });
    for (auto &x : th) x.join();
}

// --------------------------------------------------------------------------- polynomials and small helpers
// out += X^t * a  (negacyclic), coefficient-wise in Z_q
inline void add_shifted(const Fq &f, u64 *out, const u64 *a, uint32_t t, uint32_t N) {
    for (uint32_t j = 0; j + t < N; j++) out[j + t] = f.add(out[j + t], a[j]);
    for (uint32_t j = N - t; j < N; j++) out[j + t - N] = f.sub(out[j + t - N], a[j]);
}
// acc += A * S in Z_q[X] / (X^N + 1) for a binary S: one shifted add per set key bit.  The one product of a mask polynomial with a
// GLWE key polynomial (GGSW rows, compression-key rows, the phase of a compressed ciphertext).
inline void mask_times_binary_key(const Fq &f, const u64 *A, const u64 *S, uint32_t N, u64 *acc) {
    for (uint32_t t = 0; t < N; t++)
        if (S[t]) add_shifted(f, acc, A, t, N);
}
inline bool is_binary(const u64 *v, size_t count) {
    for (size_t i = 0; i < count; i++)
        if (v[i] > 1) return false;
    return true;
}
// bias[x] = 2^(base_log - 1) * sum over the `rows` rows of key[row][x], x < width: what an unsigned-digit product with the key adds
// to its signed-digit form (keyswitch key, compression key)
inline void column_bias(const Fq &f, const u64 *key, size_t rows, size_t width, uint32_t base_log, u64 *bias) {
    std::fill(bias, bias + width, (u64)0);
    for (size_t r = 0; r < rows; r++)
        for (size_t x = 0; x < width; x++) bias[x] = f.add(bias[x], key[r * width + x]);
    for (size_t x = 0; x < width; x++) bias[x] = f.mul(bias[x], (u64)1 << (base_log - 1));
}
// the body words ([rows][body_w]) of a standard-domain array [rows][mask_w + body_w]
inline void copy_bodies(const std::vector<u64> &full, size_t rows, uint32_t mask_w, uint32_t body_w, u64 *bodies) {
    const size_t pitch = (size_t)mask_w + body_w;
    for (size_t r = 0; r < rows; r++) std::memcpy(bodies + r * body_w, full.data() + r * pitch + mask_w, (size_t)body_w * 8);
}
// The specification of the seeded forms: words first_word .. first_word + count of the ChaCha20 stream (pub_key, nonce), drawn the
// way key generation draws a row's masks on the 2^64 torus (ChaStream::next64).
inline void seeded_mask_words(const uint32_t pub_key[8], u64 nonce, u64 first_word, u64 count, u64 *out) {
    ChaKey key;
    std::memcpy(key.k, pub_key, sizeof(key.k));
    ChaStream s(key, nonce, first_word, 0);
    for (u64 i = 0; i < count; i++) out[i] = s.next64();
}
// ct words on the 2^64 torus <-> words mod the prime q: the modulus switch round(x * q / 2^64) and back (false: a word not below q)
inline void torus64_to_field(u64 q, const u64 *in, u64 words, u64 *out) {
    for (u64 i = 0; i < words; i++) {
        const unsigned __int128 t = (unsigned __int128)in[i] * q + ((unsigned __int128)1 << 63);
        const u64 r = (u64)(t >> 64);
        out[i] = r >= q ? r - q : r;
    }
}
inline bool field_to_torus64(u64 q, const u64 *in, u64 words, u64 *out) {
    for (u64 i = 0; i < words; i++) {
        if (in[i] >= q) return false;
        const unsigned __int128 t = ((unsigned __int128)in[i] << 64) + (q >> 1);   // round(in * 2^64 / q) mod 2^64
        out[i] = (u64)(t / q);
    }
    return true;
}

// --------------------------------------------------------------------------- keys
// `count` key bits of the secret stream `domain` (S_SK_SMALL, S_SK_BIG)
inline void secret_key_bits(const Sampler &s, u64 domain, uint32_t count, u64 *out) {
    RowRng r = s.noise(domain, 0);
    for (uint32_t i = 0; i < count; i++) out[i] = r.bit(i);
}

// GGSW encryptions (standard domain) of the bits msg[0 .. count) under the GLWE key sk_big ([k][N] bits), l levels in base
// 2^base_log, rows numbered g * (k + 1) l + comp * l + lev, each [k + 1][N]: B = sum_j A_j * S_j + E by shifted adds (S binary);
// mask / noise streams as in oracle/tfhe_oracle.c ggsw_rows.
inline void ggsw_rows(const Sampler &s, u64 mask_stream, u64 noise_stream, const u64 *sk_big, uint32_t N, uint32_t k, uint32_t l,
                      uint32_t base_log, double sigma, const u64 *msg, size_t count, u64 *out) {
    const uint32_t rows = (k + 1) * l;
    parallel_for(count * rows, [=](size_t ir) {
        RowRng sm = s.mask(mask_stream, ir), se = s.noise(noise_stream, ir);
        const Fq &f = s.f;
        const uint32_t i = (uint32_t)(ir / rows), r = (uint32_t)(ir % rows), comp = r / l, lev = r % l;
        u64 *row = out + ir * (k + 1) * N;
        u64 *B = row + (size_t)k * N;
        for (uint32_t x = 0; x < N; x++) B[x] = se.gauss((u64)ir * N + x, sigma);
        for (uint32_t j = 0; j < k; j++) {
            u64 *A = row + (size_t)j * N;
            for (uint32_t x = 0; x < N; x++) A[x] = sm.uniform(((u64)ir * (k + 1) + j) * N + x);
            mask_times_binary_key(f, A, sk_big + (size_t)j * N, N, B);
        }
        if (!msg[i]) return;
        const u64 g = (u64)1 << (f.bits - base_log * (lev + 1));
        if (s.secure && comp < k) {
            // CSPRNG keys: a row of component comp < k encrypts -g S_comp in its BODY (the form of TFHE-rs and Concrete; the same
            // phase, the same noise), so that every mask word stays a word of the public stream - what the seeded form of the key
            // rests on.  Adding g to the mask polynomial instead, as below, would make that word tell the key bit to whoever
            // knows the stream.
            for (uint32_t x = 0; x < N; x++)
                if (sk_big[(size_t)comp * N + x]) B[x] = f.sub(B[x], g);
        } else {
            row[(size_t)comp * N] = f.add(row[(size_t)comp * N], g);   // deterministic test keys: as oracle/tfhe_oracle.c ggsw_rows
        }
    });
}

// the messages of the unrolled bootstrap key: per pair (s, s') = (s_2i, s_2i+1) of the n small-key bits the three bits s s',
// s (1 - s'), (1 - s) s'; an odd n is completed by s_n = 0
inline std::vector<u64> unrolled_messages(const u64 *sk_small, uint32_t n) {
    const uint32_t pairs = (n + 1) / 2;
    std::vector<u64> msg((size_t)pairs * 3);
    for (uint32_t i = 0; i < pairs; i++) {
        const u64 s1 = sk_small[2 * i], s2 = 2 * i + 1 < n ? sk_small[2 * i + 1] : 0;
        msg[3 * i] = s1 & s2;
        msg[3 * i + 1] = s1 & (s2 ^ 1);
        msg[3 * i + 2] = (s1 ^ 1) & s2;
    }
    return msg;
}

// the keyswitch key: row j * levels + lev = an LWE encryption [n masks | body] under sk_small of sk_big[j] 2^(bits - base_log (lev + 1))
inline void ksk_rows(const Sampler &s, const u64 *sk_small, uint32_t n, const u64 *sk_big, uint32_t big_n, uint32_t levels,
                     uint32_t base_log, double sigma, u64 *ksk) {
    parallel_for((size_t)big_n * levels, [=](size_t jr) {
        RowRng sm = s.mask(S_KSK_MASK, jr), se = s.noise(S_KSK_NOISE, jr);
        const Fq &f = s.f;
        const uint32_t j = (uint32_t)(jr / levels), lev = (uint32_t)(jr % levels);
        u64 *row = ksk + jr * (n + 1);
        u64 b = se.gauss(jr, sigma);
        for (uint32_t x = 0; x < n; x++) {
            row[x] = sm.uniform((u64)jr * (n + 1) + x);
            if (sk_small[x]) b = f.add(b, row[x]);
        }
        if (sk_big[j]) b = f.add(b, (u64)1 << (f.bits - base_log * (lev + 1)));
        row[n] = b;
    });
}

// the compression key (2^64 torus, k = 1): row j * levels + lev = [A | B], B = A S + e + S_j 2^(64 - base_log (lev + 1)) X^0: masks
// from the public stream (CSPRNG keys: the first N words of the row's stream), noise from the secret one
inline void compression_key_rows(const Sampler &s, const u64 *sk_big, uint32_t N, uint32_t levels, uint32_t base_log, double sigma,
                                 u64 *key) {
    parallel_for((size_t)N * levels, [=](size_t jr) {
        RowRng sm = s.mask(S_PKSK_MASK, jr), se = s.noise(S_PKSK_NOISE, jr);
        const uint32_t j = (uint32_t)(jr / levels), lev = (uint32_t)(jr % levels);
        u64 *A = key + jr * 2 * N, *B = A + N;
        for (uint32_t x = 0; x < N; x++) A[x] = sm.uniform((u64)jr * N + x);
        for (uint32_t x = 0; x < N; x++) B[x] = se.gauss((u64)jr * N + x, sigma);
        mask_times_binary_key(s.f, A, sk_big, N, B);
        if (sk_big[j]) B[0] = s.f.add(B[0], (u64)1 << (64 - base_log * (lev + 1)));
    });
}

// --------------------------------------------------------------------------- encryption, phase, decoding
// LWE encryptions of msgs[i] 2^delta_log under the binary key `key` of dimension dim: ciphertext i takes the encryption counter
// first + i, its masks from the public stream, its noise from the secret one.  ct_out: [count][dim + 1] words; null: the masks are
// not kept and bodies_out [count] receives the body words (the seeded form).
inline void lwe_encrypt(const Sampler &s, const u64 *key, uint32_t dim, double sigma, u64 first, const int64_t *msgs, uint32_t count,
                        uint32_t delta_log, u64 *ct_out, u64 *bodies_out) {
    parallel_for(count, [=](size_t i) {
        RowRng sm = s.mask(S_ENC_MASK, first + i), se = s.noise(S_ENC_NOISE, first + i);
        const Fq &f = s.f;
        u64 *ct = ct_out ? ct_out + i * (dim + 1) : nullptr;
        const u64 torus = f.mul(f.from_i64(msgs[i]), (u64)1 << delta_log);
        u64 b = f.add(torus, se.gauss(first + i, sigma));
        for (uint32_t x = 0; x < dim; x++) {
            const u64 a = sm.uniform((first + i) * (u64)(dim + 1) + x);
            if (ct) ct[x] = a;
            if (key[x]) b = f.add(b, a);
        }
        if (ct) ct[dim] = b;
        else bodies_out[i] = b;
    });
}

// phase[i] = body - <mask, key> of the ciphertexts ct_in [count][dim + 1]
inline void lwe_phase(const Fq &f, const u64 *key, uint32_t dim, const u64 *ct_in, uint32_t count, u64 *phase) {
    for (uint32_t i = 0; i < count; i++) {
        const u64 *ct = ct_in + (size_t)i * (dim + 1);
        u64 p = ct[dim];
        for (uint32_t x = 0; x < dim; x++)
            if (key[x]) p = f.sub(p, ct[x]);
        phase[i] = p;
    }
}

// The phases of `count` compressed ciphertexts (2^64 torus): blocks of up to N, each [N mask values | N body values] of log_modulus
// bits; phase = body 2^(64 - log_modulus) - (A S)_i.  False: a value does not fit log_modulus bits.
inline bool compressed_phase(const Fq &f, const u64 *key, uint32_t N, const uint32_t *data, uint32_t count, uint32_t log_modulus,
                             u64 *phase) {
    const uint32_t up = 64 - log_modulus;
    std::vector<u64> A(N), AS(N);
    for (uint32_t t0 = 0; t0 < count; t0 += N) {
        const uint32_t m = std::min(N, count - t0);
        const uint32_t *blk = data + (size_t)(t0 / N) * 2 * N;
        for (uint32_t x = 0; x < N; x++) {
            if (log_modulus < 32 && (blk[x] >> log_modulus)) return false;
            A[x] = (u64)blk[x] << up;
        }
        std::fill(AS.begin(), AS.end(), 0);
        mask_times_binary_key(f, A.data(), key, N, AS.data());
        for (uint32_t i = 0; i < m; i++) {
            if (log_modulus < 32 && (blk[N + i] >> log_modulus)) return false;
            phase[t0 + i] = ((u64)blk[N + i] << up) - AS[i];
        }
    }
    return true;
}

// the signed message of a phase: round(centred(phase) / 2^delta_log), ties up (delta_log >= 1)
inline i64 decode(const Fq &f, u64 phase, uint32_t delta_log) {
    const i64 v = f.centered(phase);
    return (v >> delta_log) + ((v >> (delta_log - 1)) & 1);
}

}  // namespace hc
