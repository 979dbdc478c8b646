/* libbmi_client.so: the client half of include/bmi_tfhe.h, for a machine without a GPU and without ROCm.
 *
 * The library exports a subset of the functions bmi_tfhe.h declares, with the same signatures, the same results and the same
 * refusal texts; this header declares nothing new.  For one parameter set, one set of settings and one deterministic seed, every
 * word it exports or encrypts is the word libbmi_tfhe.so exports or encrypts; on the CSPRNG path it uses the same streams, nonces
 * and counters, so a seeded key file written here expands on a server to the keys held here, and the counters of
 * bmi_encrypt_seeded are the ones bmi_expand_seeded_batch expects.
 *
 * The subset:
 *   parameters   bmi_default_params, bmi_default_params_for, bmi_preset_params, bmi_get_params
 *   context      bmi_ctx_create (device = BMI_CLIENT_NO_DEVICE only; the shapes libbmi_tfhe.so refuses are refused here),
 *                bmi_ctx_destroy (overwrites the secret keys and the secret ChaCha20 key before it frees them), bmi_last_error
 *   settings     bmi_set_bsk_precision, bmi_get_bsk_precision, bmi_set_bsk_unroll  - they decide how a key is rounded
 *   keys         bmi_keygen, bmi_keygen_insecure_deterministic, bmi_keygen_from_secret, bmi_export_keys,
 *                bmi_import_keys (with both secret keys: a client reloading its own file; without them it is refused),
 *                bmi_export_bsk_unrolled, bmi_import_bsk_unrolled, bmi_export_keys_seeded, bmi_export_bsk_unrolled_seeded,
 *                bmi_compression_keygen, bmi_compression_key_info (device_bytes is 0), bmi_export_compression_key,
 *                bmi_import_compression_key, bmi_export_compression_key_seeded
 *   data         bmi_encrypt, bmi_encrypt_seeded, bmi_decrypt, bmi_phase, bmi_phase_compressed, bmi_decrypt_compressed,
 *                bmi_compressed_words, bmi_seeded_mask_words, bmi_torus64_to_field, bmi_field_to_torus64
 *   circuits     bmi_circuit_prune, bmi_circuit_schedule
 *
 * Nothing that touches a device is exported: no PBS, keyswitch, look-up table, expansion, compression, decompression, no *_batch
 * or *_host form, no bmi_reserve.  Link with -lbmi_client alone; do not load both libraries into one program through the linker
 * (they define the same names) - a process that needs both opens them with dlopen, as bmi_amd does. */
#ifndef BMI_CLIENT_H
#define BMI_CLIENT_H

#include "bmi_tfhe.h"

/* the `device` of bmi_ctx_create in libbmi_client.so: no device */
#define BMI_CLIENT_NO_DEVICE (-1)

#endif
