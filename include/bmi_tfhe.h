/*
 * bmi_tfhe.h — C ABI of the MI355X-native TFHE programmable-bootstrap engine
 * (libbmi_tfhe.so) that sits behind the QFloat / qfloat_matrix_inverse API of
 * zama-ai/bounty-matrix-inversion.
 *
 * The reference reaches its FHE runtime only through concrete-python's Circuit object
 * (file:line relative to /root/reference):
 *      fhe.Compiler(...).compile(inputset)   matrix_inversion/main.py:53-66
 *      circuit.keygen()                      matrix_inversion/main.py:177
 *      circuit.encrypt(arrays, signs)        matrix_inversion/main.py:73-76
 *      circuit.run(args)                     matrix_inversion/main.py:78-81   <- every PBS executes here
 *      circuit.decrypt(result)               matrix_inversion/main.py:83-86
 * and, inside the traced circuit body, through table look-ups on encrypted scalars
 * (every non-linear operator on a Tracer; the one explicit LUT is
 * matrix_inversion/base_p_arrays.py:359-365).  Each entry point below names the call it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; bmi_last_error() gives the text.
 *   - plain pointers and sizes only.  Pointers named d_* are DEVICE pointers (HIP), all
 *     others are host pointers.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - ciphertext modulus q (bmi_params.q_bits): 2^64 - 2^32 + 1, 2^49 - 720895 or 2^64; words are canonical (< q)
 *     64-bit integers at this boundary for all three.
 *   - a "big" LWE ciphertext has k*N+1 words (mask, then body); a "small" one n+1 words.
 *   - messages are signed integers m encoded as m * 2^delta_log (mod q); a p-bit signed message space uses
 *     delta_log = q_bits - 1 - p (59 resp. 44 for p = 4).
 *   - a context is single-caller (no internal locking); work on a stream is asynchronous
 *     until bmi_sync() or a call that returns data to the host.
 */
#ifndef BMI_TFHE_H
#define BMI_TFHE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmi_ctx bmi_ctx;

/* bmi_params.q_bits value selecting q = 2^64 EXACTLY - the torus concrete-python computes on: ciphertext and key words
 * are Concrete's own u64 representation (no modulus-switch hop), the external product is the exact negacyclic product
 * mod 2^64.  Message scaling as for q_bits = 64 (delta_log = 63 - msg_bits). */
#define BMI_Q_TORUS64 65u

typedef struct {
    uint32_t n;           /* small LWE dimension (630; up to 1024) */
    uint32_t log_N;       /* log2 polynomial size (10; 11 and 12 on the 2^64 torus and the 49-bit field) */
    uint32_t k;           /* GLWE dimension (1) */
    uint32_t bs_levels;   /* l: bootstrap decomposition levels (3; (2, 15) and (1, 23) on the 49-bit field at N <= 2048, */
    uint32_t bs_base_log; /* bootstrap decomposition base log (15; 10 on the 2^64 torus)   (3 | 2, 10 | 15) on the torus) */
    uint32_t ks_levels;   /* keyswitch levels (8; up to 16 through the matrix-core kernel) */
    uint32_t ks_base_log; /* keyswitch base log (4) */
    uint32_t q_bits;      /* ciphertext modulus: 64 -> q = 2^64 - 2^32 + 1 (Goldilocks, integer kernels);
                             49 -> q = 2^49 - 720895 (exact integers carried in f64: the fastest kernels);
                             BMI_Q_TORUS64 -> q = 2^64 (Concrete's torus; exact products through limb-split f64
                             transforms); 0 = 64 */
    double lwe_noise;     /* std-dev / q of keyswitch-key encryptions */
    double glwe_noise;    /* std-dev / q of bootstrap-key rows and fresh big-key encryptions */
} bmi_params;

/* The north-star parameter set of BASELINE.json (n=630, N=1024, k=1, l=3) with the build's default modulus: q = 2^64
 * (BMI_Q_TORUS64, the modulus concrete-python computes on; Bg = 2^10, bootstrap key at 48 bits of precision).  One default across
 * the library, EncryptedMatrixInversion, smoke() and bench.py. */
int bmi_default_params(bmi_params *out);
/* ... and with an explicit choice of the ciphertext modulus (q_bits = BMI_Q_TORUS64, 49 or 64). */
int bmi_default_params_for(uint32_t q_bits, bmi_params *out);

/* Named parameter sets:
 *   "north_star_torus64"    BASELINE.json's shape (n 630, N 1024, k 1, l 3) on the 2^64 torus, Concrete's own modulus, with
 *                           Bg = 2^10 (two-limb key at 48 bits of precision, see bmi_set_bsk_precision) - bmi_default_params
 *   "north_star"            the same shape on the 49-bit field q = 2^49 - 720895, Bg = 2^15 (rounds 1-2's default);  "north_star_goldilocks": (l 3, Bg 2^15) on 2^64 - 2^32 + 1
 *   "secure128"             n 742, N 2048, k 1, l 2 x 15 bits, keyswitch 8 x 2 bits, 49-bit field, LWE noise 7.07e-6
 *                           (2^-17.1), GLWE noise 2^-44.  Security: the (dimension, noise / q) pairs are those of TFHE-rs'
 *                           published 128-bit set PARAM_MESSAGE_2_CARRY_2_KS_PBS (lwe_dimension 742, lwe std 7.07e-6;
 *                           glwe k N = 2048 with std 2.94e-16: here the GLWE noise is LARGER, 5.7e-14, hence at least as
 *                           hard), binary keys as there; the hardness of LWE depends on (n, sigma / q), not on q itself.
 *                           The decompositions are this build's (security does not depend on them).  4-bit look-ups
 *                           sit at ~8.7 sigma of keyswitch + mod-switch noise (measured, tests/test_gpu_parity.py: a
 *                           failure probability of ~2^-58 each; that set's own target is 2^-40).  What compiler.compile's parameter
 *                           optimiser guarantees for the reference (main.py:66) - here a fixed, documented set.
 *   "secure128_torus"       the same security-relevant pairs (n 742 at 2^-17.1; GLWE 2048 at 2^-44) on Concrete's own modulus
 *                           q = 2^64: N 2048, k 1, l 3 x 10 bits, keyswitch 8 x 2 bits, bootstrap key stored at 46 bits of
 *                           precision (two 23-bit limbs; exact limb sums through the floating-point transform,
 *                           k_blind_rotate_w_t64f).  Output noise 2^-22.9 (the 49-bit preset: 2^-19.5).
 *   "secure128_torus_wide"  the same LWE pair under N 4096 on q = 2^64, for 5-bit look-ups (the reference's unmodified circuits,
 *                           bases other than 2): l 3 x 10 bits, bootstrap key at 44 bits of precision (two 22-bit limbs,
 *                           k_blind_rotate_q_t64f), keyswitch 16 x 1 bit - the keyswitch noise bounds the margin: a 5-bit look-up
 *                           sits at 5.4 sigma (4.6 with 8 x 2 bits; 4.4 at N 2048).  error_budget.choose_params decides per circuit.
 * The north-star sets keep n = 630 as BASELINE.json prescribes; their noise is sized for correctness, NOT for 128-bit
 * security. */
int bmi_preset_params(const char *name, bmi_params *out);

/* replaces fhe.Compiler(...).compile(...) (main.py:53-66): fixes the crypto parameters, binds a GPU. */
int bmi_ctx_create(const bmi_params *params, int device, bmi_ctx **out);
void bmi_ctx_destroy(bmi_ctx *ctx);
/* ctx may be NULL: returns the last error of a failed bmi_ctx_create on this thread. */
const char *bmi_last_error(const bmi_ctx *ctx);
int bmi_get_params(const bmi_ctx *ctx, bmi_params *out);

/* replaces circuit.keygen() (main.py:177).  Generates both secret keys, the bootstrap key (uploaded and transformed
 * to the NTT domain on the GPU) and the keyswitch key.  All randomness comes from a CSPRNG: ChaCha20 keyed from the
 * operating system (getrandom), with one key for secret material (key bits, noise) and an independent one for the
 * public masks, so the evaluation keys reveal nothing about the secret streams.  bmi_encrypt then draws fresh
 * mask + noise for every ciphertext from the same generators (one nonce per ciphertext, never reused). */
int bmi_keygen(bmi_ctx *ctx);
/* TEST ONLY - NOT CRYPTOGRAPHIC.  The same key set, deterministic in `seed`: every word is a counter-indexed
 * splitmix64 output (an invertible map: public key words reveal the seed and with it the secret keys), and
 * bmi_encrypt under such a key set is deterministic too (ciphertext i of a key set repeats its mask and noise).  It
 * exists so that oracle/tfhe_oracle.c can reproduce keys and ciphertexts bit for bit in the parity tests and so that
 * every rank of a benchmark holds the same keys without an exchange (the reference's analogue: Concrete's
 * use_insecure_key_cache, qfloat_matrix_inversion.py:997-998).  Never use it for data that matters. */
int bmi_keygen_insecure_deterministic(bmi_ctx *ctx, uint64_t seed);
/* Test hook: copies out the secret keys and the standard-domain evaluation keys.
 * Sizes: sk_small[n], sk_big[k*N], bsk[n*(k+1)*l*(k+1)*N], ksk[k*N*ks_levels*(n+1)]; any may be NULL. */
int bmi_export_keys(const bmi_ctx *ctx, uint64_t *sk_small, uint64_t *sk_big, uint64_t *bsk, uint64_t *ksk);
/* Loads a key set generated elsewhere (same sizes and standard-domain layout as bmi_export_keys; words reduced mod q)
 * and uploads the evaluation keys.  sk_small and sk_big may both be NULL: the context is then evaluation-only (PBS,
 * keyswitch, linear combinations work; bmi_encrypt / bmi_decrypt / bmi_phase fail) - the server half of the
 * client/server split the reference reaches through Concrete's key objects (circuit.keys, the ".keys" cache of
 * qfloat_matrix_inversion.py:997-998). */
int bmi_import_keys(bmi_ctx *ctx, const uint64_t *sk_small, const uint64_t *sk_big, const uint64_t *bsk, const uint64_t *ksk);

/* Evaluation keys for secret keys made elsewhere (binary, sizes as in bmi_export_keys): the trusted-benchmark half of
 * interoperating with a Concrete client, whose LWE secret keys are binary vectors too.
 * seed = 0: masks and noise from the CSPRNG (production).  seed != 0: deterministic test vectors, NOT cryptographic
 * (same caveats as bmi_keygen_insecure_deterministic). */
int bmi_keygen_from_secret(bmi_ctx *ctx, const uint64_t *sk_small, const uint64_t *sk_big, uint64_t seed);
/* 2^64-torus interop (context-free, host): ciphertext words as Concrete stores them (u64, the torus scaled by 2^64)
 * to words mod q and back, by the modulus switch round(x * q / 2^64) resp. round(x * 2^64 / q).  A message m * 2^(63-p)
 * on the torus becomes m * 2^(q_bits-1-p) up to a relative 2^-30; the rounding adds < sqrt(kN/12) units of 1/q to
 * the phase.  `words` counts u64 words (count * (k*N+1) for a batch of big-key ciphertexts). */
int bmi_torus64_to_field(uint32_t q_bits, const uint64_t *in, uint64_t words, uint64_t *out);
int bmi_field_to_torus64(uint32_t q_bits, const uint64_t *in, uint64_t words, uint64_t *out);

/* replaces circuit.encrypt (main.py:76): big-key LWE encryptions of msgs[i] * 2^delta_log.  Fresh CSPRNG mask and noise
 * per ciphertext, except under bmi_keygen_insecure_deterministic keys (deterministic, test only).  Key sets loaded
 * with bmi_import_keys always encrypt from the CSPRNG. */
int bmi_encrypt(bmi_ctx *ctx, const int64_t *msgs, uint32_t count, uint32_t delta_log, uint64_t *ct_out);
/* replaces circuit.decrypt (main.py:86): msgs[i] = round(phase / 2^delta_log), signed. */
int bmi_decrypt(const bmi_ctx *ctx, const uint64_t *ct_in, uint32_t count, uint32_t delta_log, int64_t *msgs);
/* raw phases (for noise measurements) */
int bmi_phase(const bmi_ctx *ctx, const uint64_t *ct_in, uint32_t count, uint64_t *phase);

/* replaces a table look-up definition (fhe.univariate, base_p_arrays.py:365, and every non-linear
 * Tracer operator).  table[m + 2^(msg_bits-1)] = f(m) for signed m in [-2^(msg_bits-1), 2^(msg_bits-1));
 * the looked-up value is returned encoded as f(m) * 2^out_delta_log.  The input ciphertext of a PBS
 * using this LUT must encode m * 2^(q_bits-1-msg_bits).  Returns the id used by the batch calls.
 * On the 2^64 torus out_delta_log >= 22 (the kernels on a rounded bootstrap key keep accumulators as multiples of 2^16 / 2^22). */
int bmi_lut_register(bmi_ctx *ctx, const int64_t *table, uint32_t msg_bits, uint32_t out_delta_log, uint32_t *lut_id);
/* the N-coefficient test polynomial built for a LUT (host copy; test hook) */
int bmi_lut_get(const bmi_ctx *ctx, uint32_t lut_id, uint64_t *test_vector);

/* ---- the hot path: replaces circuit.run (main.py:81) -------------------------------------------- */
/* Programmable bootstrap of `count` big-key ciphertexts, Concrete order:
 *   keyswitch (big -> small) -> modulus switch to 2N -> blind rotation -> sample extraction.
 * d_in/d_out: [count][k*N+1] device words (may alias); d_lut_ids: [count] device uint32, every id one returned by
 * bmi_lut_register (the device-pointer entry points cannot inspect their ids; the *_host forms refuse unknown ones). */
int bmi_pbs_batch(bmi_ctx *ctx, const uint64_t *d_in, const uint32_t *d_lut_ids, uint32_t count, uint64_t *d_out,
                  void *stream);
/* the two stages, separately (d_small: [count][n+1]) */
int bmi_keyswitch_batch(bmi_ctx *ctx, const uint64_t *d_in, uint32_t count, uint64_t *d_small, void *stream);
int bmi_blind_rotate_batch(bmi_ctx *ctx, const uint64_t *d_small, const uint32_t *d_lut_ids, uint32_t count,
                           uint64_t *d_out, void *stream);
/* ---- centred modulus switch (2^64 torus and 49-bit field; csrc/modswitch_centre.hip; TFHE-rs' "centred mean" variant) ----
 * The rotation rounds the n mask words and the body of a small ciphertext to the 2N positions of the circle.  For a BINARY key s -
 * which every key path of this library presumes - the rounding error of the switched phase is
 *      sum_i s_i e_i - e_b  =  sum_i e_i / 2  +  sum_i (s_i - 1/2) e_i  -  e_b,
 * e_i the rounding error of mask word i and e_b the body's.  The first sum is public: subtracted from the body BEFORE the body is
 * rounded, it leaves sum (s_i - 1/2) e_i - e_b, of variance (1 + n/4) / 12 positions^2 whatever the key's weight, against
 * (1 + hw(s)) / 12 ~ (1 + n/2) / 12 of the standard switch.  No key material, no change to a rotation kernel: the rotation's own
 * rounding of the new body yields the compensated switch.  Under the unrolled key (bmi_set_bsk_unroll) the exponents
 * (a^ + a^', a^, a^') of a step are sums of the same rounded words, so the same compensation applies.
 * Exactly:  torus, S = 64 - log2(2N):  e_i = ((a_i + 2^(S-1)) mod 2^S) - 2^(S-1),  b' = b - (sum_i e_i >> 1) mod 2^64 (arithmetic shift);
 *           field, q = 2^49 - 720895:  A_i = floor((a_i 2N + (q >> 1)) / q),  E_i = a_i 2N - A_i q,  b' = b - floor(sum_i E_i / 4N) mod q.
 *
 * bmi_set_modswitch: mode 0 (default) = the standard switch, every word as before; mode 1 = centred: bmi_pbs_batch,
 * bmi_pbs_shared_batch and their *_host forms rewrite the bodies of their scratch small ciphertexts between the keyswitch and the
 * rotation, on the caller's stream.  Other values are refused, and mode 1 on Goldilocks (a cross-check engine).  Independent of the
 * key set, the unrolling, the kernel variant and the ring size; may be switched at any time.
 * bmi_keyswitch_batch, bmi_blind_rotate_batch and bmi_blind_rotate_glwe_batch (and their *_host forms) are UNCHANGED IN BOTH
 * MODES: they return, resp. rotate, exactly the words they are given.  A caller of the split stages applies
 * bmi_modswitch_centre_batch between them itself: d_small_in / d_small_out [count][n+1] (may alias; mask words are copied
 * unchanged, the body is replaced by b').  It needs no keys, works whatever the mode, and count == 0 launches nothing. */
int bmi_set_modswitch(bmi_ctx *ctx, uint32_t mode);
int bmi_get_modswitch(const bmi_ctx *ctx, uint32_t *mode);
int bmi_modswitch_centre_batch(bmi_ctx *ctx, const uint64_t *d_small_in, uint32_t count, uint64_t *d_small_out, void *stream);
int bmi_modswitch_centre_batch_host(bmi_ctx *ctx, const uint64_t *small_in, uint32_t count, uint64_t *small_out);
/* ---- one blind rotation shared by the look-ups of the same ciphertext (2^64 torus; csrc/glwe_lookup.hip) ----
 * A test polynomial of bmi_lut_register is a step function, so TV_f = TV_0 * P_f with TV_0 = 2^(unit_log - 1) * sum_x X^x and
 * P_f = (1 - X) TV_f / 2^unit_log a sparse polynomial of at most 2^msg_bits small integers (the differences of neighbouring table
 * values, times 2^(out_delta_log - unit_log)).  One rotation of TV_0 serves every table of a GROUP - tables that are looked up at
 * the same input and whose out_delta_log is >= the group's unit_log: output t is SampleExtract_0(ACC * P_t), at most 2^msg_bits
 * rotated additions per word instead of a keyswitch and a rotation.  The output's bootstrap noise variance grows by |P_t|^2 (the
 * sum of squares of its coefficients).  Tables of msg_bits <= 6 whose neighbouring entries differ by an int32 at most can share
 * (their sparse form is built at registration; the others are refused as members of a base's group, each with its own text).
 * Served by every floating-point-transform rotation of the torus: N = 1024 (key at 48 bits), N = 2048 (46 bits), N = 4096 (44 bits)
 * and the unrolled key of bmi_set_bsk_unroll at its own 42 bits (N = 1024) or 40 bits (N = 2048).  Refused with a bmi_last_error text: the 49-bit field and
 * Goldilocks; a pinned exact-transform kernel variant (1 / 3 / 4 at N = 1024); the unrolled key pinned at 48 bits of precision
 * (bmi_set_bsk_precision(ctx, 48) before bmi_set_bsk_unroll: the exact-transform unrolled kernel).
 *
 * bmi_lut_register_base: the id of TV_0 = + 2^(unit_log - 1) (every coefficient, PLUS sign; the existing table of -+1 at half
 * scale yields the negative) as an ordinary table id; one per unit_log however often it is asked for.  unit_log - 1 >= 64 -
 * (bootstrap-key precision), the grid bmi_lut_register holds its tables to: unit_log >= 17 at 48 bits, 19 at 46, 21 at 44
 * (N = 4096) and 23 at 42 (the unrolled key). */
int bmi_lut_register_base(bmi_ctx *ctx, uint32_t unit_log, uint32_t *lut_id);
/* bmi_blind_rotate_batch returning the rotated ACCUMULATOR instead of its extracted sample: d_glwe [count][2N] words, the mask
 * polynomial, then the body, coefficients in natural order (k = 1).  Any registered table; the same kernel choice by batch size
 * (at N = 4096 the one kernel of that ring; with the unrolled key one ciphertext per workgroup up to 256, two beyond), and
 * o[0] = A[0], o[x] = -A[N - x], o[N] = B[0] are the words bmi_blind_rotate_batch writes. */
int bmi_blind_rotate_glwe_batch(bmi_ctx *ctx, const uint64_t *d_small, const uint32_t *d_lut_ids, uint32_t count,
                                uint64_t *d_glwe, void *stream);
/* The look-ups of `groups` accumulators: group g is the rotation of the base polynomial d_base_ids[g] and serves the tables
 * d_lut_ids[d_group_ptr[g] .. d_group_ptr[g+1]) (CSR, d_group_ptr[groups] = total); d_out [total][N+1].  A table that IS its
 * group's base (lut id = base id, any registered table: what a group of one is given) is the plain extraction, the words of
 * bmi_blind_rotate_batch and no noise growth.  Preconditions (the *_host forms refuse a violation, the device forms stay inside
 * their buffers but compute something else): registered ids; for every table other than its group's base, a base id from
 * bmi_lut_register_base, msg_bits <= 6, int32 differences and out_delta_log >= the base's unit_log; non-decreasing group ranges
 * from 0 to total.  Independent of the ring size and of the key that rotated: N = 1024 / 2048 / 4096, plain or unrolled. */
int bmi_glwe_lookup_batch(bmi_ctx *ctx, const uint64_t *d_glwe, const uint32_t *d_group_ptr, const uint32_t *d_base_ids,
                          const uint32_t *d_lut_ids, uint32_t groups, uint32_t total, uint64_t *d_out, void *stream);
/* bmi_pbs_batch for grouped look-ups: keyswitch of the `groups` rows of d_in ([groups][N+1]), ONE rotation per group with its base
 * polynomial, then the look-ups of bmi_glwe_lookup_batch into d_out [total][N+1] (d_in is consumed by the keyswitch before d_out is
 * written).  The accumulators ([groups][2N] words: 64 KB each at N = 4096) live in context scratch that bmi_reserve pre-sizes.
 * On every engine bmi_blind_rotate_glwe_batch serves. */
int bmi_pbs_shared_batch(bmi_ctx *ctx, const uint64_t *d_in, const uint32_t *d_group_ptr, const uint32_t *d_base_ids,
                         const uint32_t *d_lut_ids, uint32_t groups, uint32_t total, uint64_t *d_out, void *stream);
/* Leveled (PBS-free) linear ops on big-key ciphertexts, CSR form:
 *   out[i] = const_body[i] + sum_{e in [row_ptr[i], row_ptr[i+1])} coef[e] * store[idx[e]]
 * replaces + - and constant * on Tracers and np.sum / slicing (qfloat.py:811-826, 901, 1015). */
int bmi_lincomb_batch(bmi_ctx *ctx, const uint64_t *d_store, const uint32_t *d_row_ptr, const uint32_t *d_idx,
                      const int64_t *d_coef, const uint64_t *d_const_body, uint32_t count, uint64_t *d_out,
                      void *stream);
/* d_store[d_rows[i]] = d_src[i] for i < count (big-key ciphertext rows).  Lets a scheduler keep a level's outputs
 * contiguous for the batch call and still place them in recycled rows of its ciphertext store (the reference leaves
 * value lifetimes to Concrete's runtime inside circuit.run, main.py:81). */
int bmi_scatter_rows(bmi_ctx *ctx, const uint64_t *d_src, uint32_t count, uint64_t *d_store, const uint32_t *d_rows,
                     void *stream);
/* Device-pointer forms of bmi_phase and bmi_decrypt (results read where they were computed: noise statistics, failure counts,
 * an executor's outputs): d_ct [count][k*N+1] device words, d_phase / d_msgs / d_err [count] device words.  The decoding rule and
 * the refusals are the host forms'; count == 0 launches nothing.  d_err[i] (may be NULL) is the centred residue of
 * phase - e * 2^delta_log mod q as a signed value, with e = d_expected[i], or the decoded message where d_expected is NULL: with
 * the expected result given it is the noise of a look-up, and a wrong result shows as |err| >= 2^delta_log / 2.
 * These calls keep A COPY OF THE BIG SECRET KEY ON THE DEVICE (a bit mask of k*N/64 words, owned by the context): it is built by
 * the first call, and overwritten with zeros and freed when the context generates or imports another key set or is destroyed. */
int bmi_phase_batch(bmi_ctx *ctx, const uint64_t *d_ct, uint32_t count, uint64_t *d_phase, void *stream);
int bmi_decrypt_batch(bmi_ctx *ctx, const uint64_t *d_ct, uint32_t count, uint32_t delta_log, const int64_t *d_expected,
                      int64_t *d_msgs, int64_t *d_err, void *stream);
/* Host-buffer convenience forms (what a ctypes/cgo binding over numpy buffers would call; every entry point named *_host, here
 * and below): copy in, run the device-pointer form on the context's own stream, copy out, synchronise.  They share ONE SCRATCH
 * ARENA OWNED BY THE CONTEXT, which grows to the largest call made so far and is never shrunk.  Argument and state refusals are
 * made before anything is queued; a call that is refused or fails later RETURNS ONLY AFTER THE CONTEXT'S STREAM HAS DRAINED, like a
 * call that succeeds: the caller's arrays may be freed or reused as soon as a host form has returned, whatever it returned. */
int bmi_pbs_batch_host(bmi_ctx *ctx, const uint64_t *in, const uint32_t *lut_ids, uint32_t count, uint64_t *out);
int bmi_keyswitch_batch_host(bmi_ctx *ctx, const uint64_t *in, uint32_t count, uint64_t *small_out);
int bmi_blind_rotate_batch_host(bmi_ctx *ctx, const uint64_t *small_in, const uint32_t *lut_ids, uint32_t count,
                                uint64_t *out);
/* ... and of the shared look-ups (glwe_out / glwe_in: [count resp. groups][2N] words).  They refuse what the device forms state
 * as preconditions: unknown ids, a base id that serves other tables and is no base polynomial, a table without a sparse form or encoded below its group's
 * unit, group ranges that do not run from 0 to total without decreasing; and, like the device forms, the engines without an
 * accumulator form (above). */
int bmi_blind_rotate_glwe_batch_host(bmi_ctx *ctx, const uint64_t *small_in, const uint32_t *lut_ids, uint32_t count,
                                     uint64_t *glwe_out);
int bmi_glwe_lookup_batch_host(bmi_ctx *ctx, const uint64_t *glwe_in, const uint32_t *group_ptr, const uint32_t *base_ids,
                               const uint32_t *lut_ids, uint32_t groups, uint32_t total, uint64_t *out);
int bmi_pbs_shared_batch_host(bmi_ctx *ctx, const uint64_t *in, const uint32_t *group_ptr, const uint32_t *base_ids,
                              const uint32_t *lut_ids, uint32_t groups, uint32_t total, uint64_t *out);
/* Test hook of the floating-point-transform kernels (2^64 torus; N = 1024: key at 48 bits, kernel variants 5 / 6; N = 2048: key at
 * 46 bits; N = 4096: key at 44 bits, k_blind_rotate_q_t64f): blind rotation of `count` small-key ciphertexts by the wave-pair kernel - by the latency form when kernel variant 6 or 2
 * is selected, by k_blind_rotate_w_t64f at N = 2048, with the unrolled key there by the kernel that runs a batch of `count`
 * (k_blind_rotate_wu_t64f or _wu2_t64f) -, which here also records how far every limb sum was from the integer it was
 * rounded to.  *max_distance must stay far below 1/2 (measured: below 2^-11) - that is what makes the
 * rounded results the exact integer sums, whatever the order of the floating-point operations. */
int bmi_fft_margin_host(bmi_ctx *ctx, const uint64_t *small_in, const uint32_t *lut_ids, uint32_t count, uint64_t *out,
                        double *max_distance);
/* negacyclic product of two polynomials through the GPU NTT (test hook for the transform) */
int bmi_negacyclic_mul_host(bmi_ctx *ctx, const uint64_t *a, const uint64_t *b, uint32_t count, uint64_t *c);

/* Pre-sizes the context's internal scratch (small-key ciphertexts of bmi_pbs_batch, digit matrix and limb sums of the
 * matrix-core keyswitch, on the torus the accumulators of bmi_pbs_shared_batch) for batches up to max_count, so that no allocation happens on the hot path afterwards. */
int bmi_reserve(bmi_ctx *ctx, uint32_t max_count);

int bmi_sync(bmi_ctx *ctx, void *stream);

/* Selects the blind-rotation kernel: 0 = auto (by batch size), 1 = throughput, a pair of wavefronts per
 * ciphertext exchanging every level, 2 = latency (one workgroup of 8 wavefronts per ciphertext), 3 = throughput,
 * a pair of wavefronts per ciphertext exchanging once per CMUX (49-bit field; what auto picks for large batches),
 * 4 = the one-wavefront-per-transform latency kernel (the 49-bit field at N = 1024 refuses 1 and 4: its wave-pair kernel 3 and
 *     its two-wavefronts-per-transform latency kernel 2 replaced them),
 * 5 = 2^64 torus only, bootstrap key at 48 bits in base 2^10 (the torus default): the wave-pair kernel whose exact limb
 *     products are carried by a folded 512-point complex FFT in f64 and rounded to the nearest integer (same words as 1 / 3,
 *     which pin the exact transform mod 2^49 - 720895; what auto picks for large batches on that key),
 * 6 = the same for the latency form (one workgroup per ciphertext; what auto and 2 pick on that key; 4 pins the exact transform).
 * 2^64 torus at N = 2048: auto = one workgroup per ciphertext up to 256 ciphertexts (2 pins it), two ciphertexts per workgroup sharing
 *     the key words beyond (1 / 3 pin it); the same words - on the plain key (k_blind_rotate_w_t64f / _w2_t64f) and on the unrolled
 *     key (k_blind_rotate_wu_t64f / _wu2_t64f, which share one key copy) alike.  N = 4096: one kernel. */
int bmi_set_kernel_variant(bmi_ctx *ctx, int variant);
/* *name = the name of the blind-rotation kernel (the __global__ function, a static string) that the context's current modulus,
 * key mode, precision and kernel variant run for a batch of `count` ciphertexts: answered by the function that dispatches
 * bmi_blind_rotate_batch, for every engine, so that tools can label timings and tests can tell kernels apart that give the same
 * words by construction.  Fails where a rotation would be refused (e.g. unrolling selected without an unrolled key). */
int bmi_rotation_kernel(const bmi_ctx *ctx, uint32_t count, const char **name);

/* 2^64 torus only, before keygen / import: precision the bootstrap key is stored at.  No transform exists mod 2^64, so the
 * external product is computed exactly over the integers from limbs of every key word (csrc/t64_common.hpp); the number of
 * limbs follows from the precision:
 *   64  exact key, three 22-bit limbs.  Default at Bg = 2^15 (51 k PBS/s, 5.5 ms per bootstrap).
 *   48  every key word (generated here or imported) rounded to a multiple of 2^16, two 24-bit limbs: 2/3 of the
 *       multiply-accumulates and inverse transforms.  Needs Bg <= 2^10 (a limb's sum must stay below p/2).  DEFAULT of the
 *       torus parameter set ("north_star_torus64": l = 3, Bg = 2^10): the rounding errors of a row (2^15 / sqrt 3 per word,
 *       summed over the ~N/2 set bits of the GLWE key: 2^18.7) stay under the key noise 2^20, and the finer base more than
 *       pays for them - bootstrap output noise 2^-22.6 against 2^-19.85 of (Bg = 2^15, exact key), measured on the formula
 *       (tests/test_gpu_parity.py).  With bmi_set_bsk_unroll: the exact-transform unrolled kernel (k_blind_rotate_lat2u_t64).
 *   46  N = 2048 only (its default and only precision; "secure128_torus"): multiples of 2^18, two 23-bit limbs - the limb width at
 *       which the a-priori error bound of the 1,024-point floating-point transform still certifies the rounding of a limb sum
 *       (0.41 < 1/2, csrc/fft_quarter_f64.hpp; 24-bit limbs: 0.83).
 *   44  N = 4096 only (its default and only precision; 6-bit look-ups, "secure128_torus_wide"): multiples of 2^20, two 22-bit limbs
 *       (2,048-point transform: bound 0.45, csrc/fft_eighth_f64.hpp; 23-bit limbs: 0.90).
 *   42  multiples of 2^22, two 21-bit limbs.  At Bg = 2^10 in UNROLLED mode only - the precision bmi_set_bsk_unroll(ctx, 2) selects
 *       by itself when none was set: the three scaled products of an unrolled step make the limb sums six times larger, and 21-bit
 *       limbs keep them inside the range the floating-point transform is certified for (k_blind_rotate_lat2u_t64f; output noise
 *       2^-19.3).  At Bg = 2^15: round 2's throughput option for flat PBS batches (output noise 2^-15.15: too noisy for the
 *       encrypted inverse).
 *   40  N = 2048 in UNROLLED mode only (Bg = 2^10, l = 3 or 2) - the precision bmi_set_bsk_unroll(ctx, 2) selects by itself there
 *       when none was set, and the only one it takes: multiples of 2^24, two 20-bit limbs.  The six-times larger limb sums of the
 *       unrolled step stay below 2^45 and the a-priori bound of the 1,024-point transform, with the scaling by zeta^(..c) - 1
 *       counted as a stage, is 0.38 < 1/2 (tools/fft_bound.py; 21-bit limbs: 0.76) - k_blind_rotate_wu_t64f (one workgroup per ciphertext: up to 256
 *       ciphertexts, kernel variant 2) and k_blind_rotate_wu2_t64f (two per workgroup sharing every key word: beyond 256, variants
 *       1 / 3), the same words from one key copy; output noise 2^-16.2
 *       (std) against 2^-22.2 of the plain 46-bit key, far below the keyswitch noise it feeds (std 2^-9.8): DESIGN section 2.
 *       Refused in plain mode; switching back to factor 1 restores 46.
 * The rounded key is the context's key from then on (bmi_export_keys / bmi_export_bsk_unrolled return it; results are
 * bit-exact against an oracle given that key; oracle/tfhe_oracle.c ora_round_key states the rule).  The rounding only ever
 * adds noise to valid LWE samples; generating the key on the grid directly would instead round its own noise away. */
int bmi_set_bsk_precision(bmi_ctx *ctx, uint32_t bits);
/* the precision in force (64 on the prime fields) */
int bmi_get_bsk_precision(const bmi_ctx *ctx, uint32_t *bits);

/* 49-bit field at N = 1024, and at N = 2048 with l <= 2 (the secure128 shape), and the 2^64 torus at its default set (Bg = 2^10;
 * key at 42 bits: k_blind_rotate_lat2u_t64f, the floating-point-transform route, 2.9 ms per bootstrap - what this call selects when
 * no precision was set -, or pinned at 48 bits: k_blind_rotate_lat2u_t64, the exact transform, 3.3 ms), and the 2^64 torus at N = 2048
 * (l = 3 or 2, Bg = 2^10, e.g. "secure128_torus"; key at 40 bits - selected by this call when no precision was set, any other explicit
 * precision is refused -: k_blind_rotate_wu_t64f, one workgroup per ciphertext, up to 256 ciphertexts and k_blind_rotate_wu2_t64f, two
 * ciphertexts per workgroup sharing every key word, beyond, as bmi_set_kernel_variant states; N = 4096 is
 * refused): bootstrap-key unrolling (Zhou et al. 2018, Bourse et al. 2018; unrolling factor 2).
 * factor 1 (default): the blind rotation of CGGI, one LWE coefficient per step.  factor 2: a step absorbs two coefficients,
 *   ACC <- ACC + sum_{j<3} (X^(c_j) - 1) (K_j [.] ACC),  c = (a + a', a, a'),  K = GGSW(s s'), GGSW(s (1 - s')), GGSW((1 - s) s'),
 * with one decomposition and one set of forward transforms per step (half as many as the plain rotation; the factors X^c - 1
 * are applied in the transform domain).  Every batch size then runs k_blind_rotate_lat2u_49 (49-bit field, N = 1024),
 * k_blind_rotate_wide49u (N = 2048) or the torus kernel above, one workgroup per ciphertext; on the torus's floating-point routes,
 * batches beyond 256 ciphertexts run k_blind_rotate_tp2u_t64f (N = 1024) or k_blind_rotate_wu2_t64f (N = 2048): two ciphertexts
 * per workgroup sharing every key word in registers (half the key bytes per bootstrap; the same words).
 * The unrolled key (1.5 x the plain key's size) is generated by the next keygen call, or at once when the context already
 * holds secret keys; an evaluation-only context receives it through bmi_import_bsk_unrolled.  Layout:
 * [ceil(n/2)][3][(k+1) l][(k+1)][N] words, standard domain (an odd n is completed by a zero key bit).  Price: the key-noise
 * term of the output variance triples (three products per pair of coefficients, each scaled by X^c - 1) - size the GLWE noise
 * for it: 2^-41 keeps the margin of the default (3, 2^15) set; a one-level (1, 2^23) decomposition needs about 2^-42 or less for
 * 4-bit look-ups.  Results are
 * bit-exact against oracle/tfhe_oracle.c ora_blind_rotate_extract_unrolled on the same keys. */
int bmi_set_bsk_unroll(bmi_ctx *ctx, uint32_t factor);
int bmi_import_bsk_unrolled(bmi_ctx *ctx, const uint64_t *bsk3);
int bmi_export_bsk_unrolled(const bmi_ctx *ctx, uint64_t *bsk3);

/* Selects the keyswitch kernel: 0 = auto (int8 matrix-core product when the parameter set allows it),
 * 1 = scalar 96-bit multiply-accumulate kernel.  The matrix-core form takes at most 16 levels, the scalar kernel n <= 767
 * (it splits the coefficients over workgroups until a workgroup's digits fit its 64 KiB of LDS); bmi_keyswitch_batch refuses,
 * before any launch, a parameter set that the selected kernel - or, with more than 16 levels and n > 767, either - cannot take. */
int bmi_set_keyswitch_variant(bmi_ctx *ctx, int variant);

/* ---- compiler passes on a traced circuit in flat (CSR) form; context-free, CPU only -----------------------------
 * What fhe.Compiler(...).compile does inside Concrete (main.py:53-66) for this path.  A circuit has n_in input leaves
 * and n_nodes look-ups in creation (= topological) order; look-up i reads the leaves term_leaf[node_ptr[i] ..
 * node_ptr[i+1]) and produces leaf n_in + i.
 * bmi_circuit_prune: live_node[i] = 1 iff an output (out_leaf[0 .. n_out_terms)) depends on look-up i.
 * bmi_circuit_schedule: level (1 .. depth) of every look-up; same depth as the ASAP schedule, but nodes with slack
 * are moved out of levels that would otherwise need one more kernel round (`round_` ciphertexts per latency-kernel
 * round up to two rounds, `wide_round` per throughput-kernel round beyond). */
int bmi_circuit_prune(uint32_t n_in, uint32_t n_nodes, const int64_t *node_ptr, const int32_t *term_leaf,
                      const int32_t *out_leaf, uint64_t n_out_terms, uint8_t *live_node);
int bmi_circuit_schedule(uint32_t n_in, uint32_t n_nodes, const int64_t *node_ptr, const int32_t *term_leaf,
                         uint32_t round_, uint32_t wide_round, int32_t *level_out, int32_t *depth_out);

/* ---- seeded evaluation keys and ciphertexts (2^64 torus; csrc/chacha_expand.hip) ---------------------------------------------
 * More than two thirds of the words of an evaluation key, and all but one word of a fresh ciphertext, are public masks drawn from
 * the ChaCha20 stream of the context's PUBLIC key (bmi_keygen: one key for secrets and noise, an independent one for the masks).
 * The seeded forms carry that 32-byte key and the body words only; the receiver regenerates the masks on its GPU.
 *
 * The format.  Every row has its own nonce (domain << 56) | row (56 bits of row), domain one of the four below, and its masks
 * are the first words of the stream (pub_key, nonce): ChaCha20 in D. J. Bernstein's variant (256-bit key, 64-bit block counter
 * starting at 0, 64-bit nonce), word j = output words (2 (j mod 8), 2 (j mod 8) + 1) of block j / 8, low word first.
 *   BSK_MASK   row = (i * (k+1) l + r) of GGSW(s_i) row r: k N mask words, then N body words
 *   BSK3_MASK  the same numbering over the rows of the unrolled key [ceil(n/2)][3][(k+1) l]
 *   KSK_MASK   row = j * ks_levels + level: n mask words, then one body word
 *   ENC_MASK   row = the encryption counter of the ciphertext: k N mask words, then the body
 * (So that every mask word of a bootstrap key IS a stream word, CSPRNG key generation puts the message of a GGSW row of component
 * < k, -g S, into the row's body - the form of TFHE-rs and Concrete; the deterministic test keys add g to the mask polynomial, as
 * oracle/tfhe_oracle.c does.  Same phase, same noise; every consumer takes either.)
 * Bodies are the words bmi_export_keys returns, i.e. rounded to the precision the key is stored at (bmi_set_bsk_precision); the
 * masks are rounded by the importer the same way, so AN IMPORTER AT THE EXPORTER'S PRECISION holds, in every device-resident copy,
 * byte for byte the key that bmi_import_keys of the full export gives.  Sizes against the full forms: 0.300 for the default and
 * the secure128_torus sets, 0.215 for secure128_torus_wide, 0.5 for an unrolled key, 8 bytes instead of (k N + 1) * 8 per ciphertext.
 *
 * Refused, with a bmi_last_error text that says why: contexts on the 49-bit field or Goldilocks (their masks are rejection-sampled:
 * a word's position in the stream depends on the words before it); contexts without keys; and contexts whose masks did not come from
 * their own public stream - keys loaded by bmi_import_keys, and the deterministic test keys (bmi_keygen_insecure_deterministic,
 * bmi_keygen_from_secret with seed != 0), whose stream key is an invertible function of the seed and would reveal the secrets. */
#define BMI_SEED_DOMAIN_BSK_MASK 3u
#define BMI_SEED_DOMAIN_KSK_MASK 5u
#define BMI_SEED_DOMAIN_ENC_MASK 7u
#define BMI_SEED_DOMAIN_BSK3_MASK 9u
/* out[i] = word first_word + i of the stream (pub_key, nonce), i < count: the specification the device kernel is held to.
 * Context-free, host only (like bmi_torus64_to_field). */
int bmi_seeded_mask_words(const uint32_t pub_key[8], uint64_t nonce, uint64_t first_word, uint64_t count, uint64_t *out);
/* The key set as (public key, bodies): bsk_bodies[n * (k+1) l * N], ksk_bodies[k N * ks_levels]. */
int bmi_export_keys_seeded(const bmi_ctx *ctx, uint32_t pub_key[8], uint64_t *bsk_bodies, uint64_t *ksk_bodies);
/* Makes the context evaluation-only with the key set of a bmi_export_keys_seeded: the bodies are uploaded, the masks expanded on
 * the device, then the path of every key set (rounding, key conversions, keyswitch bias and limb form).  bmi_export_keys then
 * returns the full key.  The context keeps pub_key: bmi_import_bsk_unrolled_seeded and bmi_expand_seeded_batch use it. */
int bmi_import_keys_seeded(bmi_ctx *ctx, const uint32_t pub_key[8], const uint64_t *bsk_bodies, const uint64_t *ksk_bodies);
/* The same for the unrolled key (bmi_set_bsk_unroll; N = 1024 at 42 bits, N = 2048 at 40 bits): bsk3_bodies[ceil(n/2) * 3 *
 * (k+1) l * N].  The import is refused unless a bmi_import_keys_seeded came before it (whose public key it uses); select the
 * unrolled mode before that call, as the exporter did before its keygen, so that both store the keys at the same precision. */
int bmi_export_bsk_unrolled_seeded(const bmi_ctx *ctx, uint64_t *bsk3_bodies);
int bmi_import_bsk_unrolled_seeded(bmi_ctx *ctx, const uint64_t *bsk3_bodies);
/* bmi_encrypt in seeded form: the ciphertexts bmi_encrypt would have produced at the context's encryption counter, as
 * (*first_counter, bodies[count]); the counter advances by count.  One routine serves both entry points. */
int bmi_encrypt_seeded(bmi_ctx *ctx, const int64_t *msgs, uint32_t count, uint32_t delta_log, uint64_t *first_counter,
                       uint64_t *bodies);
/* d_out [count][k N + 1] = the ciphertexts (first_counter + i, d_bodies[i]) in full, on the caller's stream: masks from the
 * context's own public key, or from the one imported by bmi_import_keys_seeded on a server.  count == 0 launches nothing. */
int bmi_expand_seeded_batch(bmi_ctx *ctx, uint64_t first_counter, const uint64_t *d_bodies, uint32_t count, uint64_t *d_out,
                            void *stream);
int bmi_expand_seeded_batch_host(bmi_ctx *ctx, uint64_t first_counter, const uint64_t *bodies, uint32_t count, uint64_t *out);

/* ---- compression of output ciphertexts (2^64 torus, k = 1, every N; csrc/lwe_pack.hip) ------------------------------------------
 * Every output of a circuit is a big-key LWE ciphertext of (N + 1) * 8 bytes.  Up to N of them are packed into the N coefficients of
 * ONE GLWE ciphertext by a packing keyswitch, and the 2N GLWE words are modulus-switched to log_modulus bits each (TFHE-rs'
 * compressed ciphertext list): a full block costs 2N values for N results - 4 bytes per result at 16 bits instead of 8,200.
 * Integer arithmetic mod 2^64 is the specification (restated in numpy in tests/compress_cases.py).
 *
 * Compression key (levels L, base_log b; 1 <= L <= 4, 1 <= b <= 16, L b <= 63): row j L + l, for every big-key coefficient j < N
 *   and level l < L, is a GLWE encryption [A: N words][B: N words], B = A S + e + S_j 2^(64 - b (l + 1)) X^0, under the context's own
 *   GLWE key S (whose coefficient vector is sk_big), e Gaussian with glwe_noise.  Layout [N][L][2][N] words, standard domain.  Under
 *   CSPRNG keys the masks A are the first N words of the public stream (domain PKSK_MASK below, row j L + l), the noise comes from
 *   the secret stream; the seeded form is the bodies B alone, [N][L][N].  Under the deterministic test keys the key is a
 *   deterministic function of the seed.  A compression key belongs to its key set: keygen or an import of a key set drops it.
 *   ONE SHAPE PER KEY SET: row j L + l reads its masks and its noise from the start of the streams (key, domain, j L + l), so two
 *   keys of different (L, b) made for one key set would share A and e in every common row under different messages, and the
 *   difference of two such bodies is an exact combination of bits of the secret key.  bmi_compression_keygen therefore remembers
 *   the first shape it used and refuses any other, with a text, until the next keygen or import of a key set (the same shape
 *   again gives the same key).  A client never publishes two compression keys of different shape for one key set.
 * Compression of `count` ciphertexts (a_i, b_i), in blocks of N (ciphertext i of a block lands in coefficient i):
 *   1. d[i][j][l] = the digits of a_i[j] at (L, b): centred lift, round half up to the top L b bits, balanced digits from the least
 *      significant one, the top digit absorbs the carry (oracle/tfhe_oracle.c ora_decompose);
 *   2. T_i = (0, b_i X^0) - sum_{j,l} d[i][j][l] row(j, l);
 *   3. (A, B) = sum_i X^i T_i (negacyclic);
 *   4. centred modulus switch to c = log_modulus bits (2 <= c <= 32; the rule of bmi_set_modswitch carried over to a polynomial):
 *      Sh = 64 - c, e_j = ((A_j + 2^(Sh-1)) mod 2^Sh) - 2^(Sh-1), P_x = sum_{j<=x} e_j (int64), E = P_{N-1},
 *      B'_x = B_x - ((2 P_x - E) >> 1) (arithmetic shift), out A^_j = ((A_j + 2^(Sh-1)) >> Sh) mod 2^c, B^_x likewise from B'_x.
 *      (No int64 overflow for c > log2 N; below that the sums wrap.)  The switch error is white, of variance (1 + N/4)/12 4^-c.
 * Compressed form: uint32 values below 2^c; per block N mask values, then its m body values; blocks concatenated:
 *   bmi_compressed_words = ceil(count / N) * N + count values.
 * Decryption (host, secret key): phase_i = B^_i 2^(64-c) - ((A^ 2^(64-c)) S)_i, message = round(phase / 2^delta_log) as bmi_decrypt.
 * The 49-bit field and Goldilocks refuse every entry point with a bmi_last_error text; so do out-of-range arguments and
 * bmi_compress_batch without a key.  Noise: error_budget.compression_variance.
 * Decompression back to big-key LWE ciphertexts (csrc/lwe_unpack.hip; no key of any kind, so a context that has run no keygen and
 *   an evaluation-only context serve it): the negacyclic sample extraction of coefficient i of its block, shifted back up to 2^64.
 *   With i = idx mod N and A^ / B^ the mask and body values of block idx / N, taken mod 2^c, row r of the output is
 *     out[r][j] = A^[i - j] 2^(64-c)          for j <= i
 *     out[r][j] = 0 - A^[N + i - j] 2^(64-c)  for i < j < N
 *     out[r][N] = B^[i] 2^(64-c)
 *   an ordinary ciphertext of N + 1 words whose phase under sk_big is, bit for bit, the phase_i above of position idx: it goes
 *   through the keyswitch and the blind rotation as any other.  An optional index list picks positions in any order, with repeats.
 *   Noise: decompression itself adds none.  A decompressed ciphertext carries the error of the ciphertext that was compressed plus
 *   the compression's own (error_budget.decompressed_variance = the source's variance + compression_variance); it is NOT a fresh
 *   encryption, and a circuit that takes such inputs is budgeted with failure_probability(..., input_variance=...). */
#define BMI_SEED_DOMAIN_PKSK_MASK 11u
int bmi_compression_keygen(bmi_ctx *ctx, uint32_t levels, uint32_t base_log);   /* needs the secret keys; one shape per key set */
/* *levels = 0 where the context holds no compression key; device_bytes = the key's device copy and the product's bias vector */
int bmi_compression_key_info(const bmi_ctx *ctx, uint32_t *levels, uint32_t *base_log, uint64_t *device_bytes);
int bmi_export_compression_key(const bmi_ctx *ctx, uint64_t *key);              /* [N][L][2][N] */
int bmi_import_compression_key(bmi_ctx *ctx, uint32_t levels, uint32_t base_log, const uint64_t *key);   /* evaluation-only contexts too */
/* bodies [N][L][N]; refused as bmi_export_keys_seeded is, and for a key loaded by bmi_import_compression_key */
int bmi_export_compression_key_seeded(const bmi_ctx *ctx, uint64_t *bodies);
/* after bmi_import_keys_seeded, whose public key expands the masks on the device: the device then holds word for word the key of the
 * full import */
int bmi_import_compression_key_seeded(bmi_ctx *ctx, uint32_t levels, uint32_t base_log, const uint64_t *bodies);
int bmi_compressed_words(const bmi_ctx *ctx, uint32_t count, uint64_t *words);
/* d_in [count][N + 1] device words -> d_out [bmi_compressed_words] device uint32 values, on the caller's stream; count == 0
 * launches nothing.  The context's scratch grows on demand (a block is processed in slices of at most 16 MB of products). */
int bmi_compress_batch(bmi_ctx *ctx, const uint64_t *d_in, uint32_t count, uint32_t log_modulus, uint32_t *d_out, void *stream);
int bmi_compress_batch_host(bmi_ctx *ctx, const uint64_t *in, uint32_t count, uint32_t log_modulus, uint32_t *out);
int bmi_phase_compressed(const bmi_ctx *ctx, const uint32_t *data, uint32_t count, uint32_t log_modulus, uint64_t *phase);
int bmi_decrypt_compressed(const bmi_ctx *ctx, const uint32_t *data, uint32_t count, uint32_t log_modulus, uint32_t delta_log,
                           int64_t *msgs);
/* d_in = the compressed form of `count` ciphertexts (device uint32 values) -> d_out [rows][N + 1] device words, on the caller's
 * stream: row r = position d_index[r] (device uint32 values), or position r where d_index is NULL, which needs rows == count.
 * rows == 0 launches nothing.  THE INDEX IS THE CALLER'S CONTRACT: every d_index[r] < count; the device form cannot refuse a larger
 * one, which reads values that are not there.  Values are taken mod 2^log_modulus. */
int bmi_decompress_batch(bmi_ctx *ctx, const uint32_t *d_in, uint32_t count, uint32_t log_modulus, const uint32_t *d_index,
                         uint32_t rows, uint64_t *d_out, void *stream);
/* the same from and to host memory; refuses an index >= count and a value that does not fit log_modulus bits */
int bmi_decompress_batch_host(bmi_ctx *ctx, const uint32_t *in, uint32_t count, uint32_t log_modulus, const uint32_t *index,
                              uint32_t rows, uint64_t *out);

/* bytes of device memory held by the keys: every resident transform-domain copy of the bootstrap key (one per selectable kernel
 * family, plus the unrolled key when present), and the keyswitch key in word form */
int bmi_key_bytes(const bmi_ctx *ctx, uint64_t *bsk_bytes, uint64_t *ksk_bytes);

#ifdef __cplusplus
}
#endif
#endif /* BMI_TFHE_H */
