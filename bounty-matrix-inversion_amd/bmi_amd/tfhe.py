"""ctypes binding of the C ABI in include/bmi_tfhe.h (libbmi_tfhe.so).

This is the binding a maintainer of the reference would add in place of concrete-python's Circuit
object (reference call sites: matrix_inversion/main.py:53-86,177).  It fails loudly when the HIP
library is missing: the PBS path has no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libbmi_tfhe.so")
Q = 0xFFFFFFFF00000001  # Goldilocks modulus (q_bits = 64)
TORUS64 = 65                      # bmi_params.q_bits value for q = 2^64 exactly (BMI_Q_TORUS64, Concrete's torus)
MODULUS = {64: 0xFFFFFFFF00000001, 49: 562949952700417, TORUS64: 1 << 64}


class Params(C.Structure):
    _fields_ = [("n", C.c_uint32), ("log_N", C.c_uint32), ("k", C.c_uint32), ("bs_levels", C.c_uint32),
                ("bs_base_log", C.c_uint32), ("ks_levels", C.c_uint32), ("ks_base_log", C.c_uint32),
                ("q_bits", C.c_uint32), ("lwe_noise", C.c_double), ("glwe_noise", C.c_double)]

    @property
    def N(self):
        return 1 << self.log_N

    @property
    def big(self):
        return self.k * self.N + 1

    @property
    def small(self):
        return self.n + 1


class BmiError(RuntimeError):
    pass


_lib = None

_U64P = C.POINTER(C.c_uint64)
_SIGS = {
    "bmi_default_params": [C.POINTER(Params)],
    "bmi_default_params_for": [C.c_uint32, C.POINTER(Params)],
    "bmi_preset_params": [C.c_char_p, C.POINTER(Params)],
    "bmi_ctx_create": [C.POINTER(Params), C.c_int, C.POINTER(C.c_void_p)],
    "bmi_get_params": [C.c_void_p, C.POINTER(Params)],
    "bmi_keygen": [C.c_void_p],
    "bmi_keygen_insecure_deterministic": [C.c_void_p, C.c_uint64],
    "bmi_export_keys": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bmi_encrypt": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "bmi_decrypt": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "bmi_phase": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
    "bmi_lut_register": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)],
    "bmi_lut_get": [C.c_void_p, C.c_uint32, C.c_void_p],
    "bmi_lut_register_base": [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)],
    "bmi_blind_rotate_glwe_batch": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "bmi_glwe_lookup_batch": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                              C.c_void_p],
    "bmi_pbs_shared_batch": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                             C.c_void_p],
    "bmi_blind_rotate_glwe_batch_host": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
    "bmi_glwe_lookup_batch_host": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "bmi_pbs_shared_batch_host": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "bmi_pbs_batch": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "bmi_keyswitch_batch": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "bmi_blind_rotate_batch": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "bmi_lincomb_batch": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                          C.c_void_p, C.c_void_p],
    "bmi_scatter_rows": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p],
    "bmi_phase_batch": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "bmi_decrypt_batch": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bmi_pbs_batch_host": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
    "bmi_keyswitch_batch_host": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
    "bmi_blind_rotate_batch_host": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
    "bmi_negacyclic_mul_host": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
    "bmi_fft_margin_host": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_double)],
    "bmi_sync": [C.c_void_p, C.c_void_p],
    "bmi_reserve": [C.c_void_p, C.c_uint32],
    "bmi_import_keys": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bmi_keygen_from_secret": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64],
    "bmi_torus64_to_field": [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p],
    "bmi_field_to_torus64": [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p],
    "bmi_set_kernel_variant": [C.c_void_p, C.c_int],
    "bmi_rotation_kernel": [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p)],
    "bmi_set_keyswitch_variant": [C.c_void_p, C.c_int],
    "bmi_set_modswitch": [C.c_void_p, C.c_uint32],
    "bmi_get_modswitch": [C.c_void_p, C.POINTER(C.c_uint32)],
    "bmi_modswitch_centre_batch": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "bmi_modswitch_centre_batch_host": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
    "bmi_set_bsk_precision": [C.c_void_p, C.c_uint32],
    "bmi_get_bsk_precision": [C.c_void_p, C.POINTER(C.c_uint32)],
    "bmi_set_bsk_unroll": [C.c_void_p, C.c_uint32],
    "bmi_import_bsk_unrolled": [C.c_void_p, C.c_void_p],
    "bmi_export_bsk_unrolled": [C.c_void_p, C.c_void_p],
    "bmi_circuit_prune": [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p],
    "bmi_circuit_schedule": [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                             C.POINTER(C.c_int32)],
    "bmi_key_bytes": [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "bmi_seeded_mask_words": [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p],
    "bmi_export_keys_seeded": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bmi_import_keys_seeded": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "bmi_export_bsk_unrolled_seeded": [C.c_void_p, C.c_void_p],
    "bmi_import_bsk_unrolled_seeded": [C.c_void_p, C.c_void_p],
    "bmi_encrypt_seeded": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_void_p],
    "bmi_expand_seeded_batch": [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "bmi_expand_seeded_batch_host": [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p],
    "bmi_compression_keygen": [C.c_void_p, C.c_uint32, C.c_uint32],
    "bmi_compression_key_info": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)],
    "bmi_export_compression_key": [C.c_void_p, C.c_void_p],
    "bmi_import_compression_key": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "bmi_export_compression_key_seeded": [C.c_void_p, C.c_void_p],
    "bmi_import_compression_key_seeded": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "bmi_compressed_words": [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)],
    "bmi_compress_batch": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p],
    "bmi_compress_batch_host": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "bmi_phase_compressed": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "bmi_decrypt_compressed": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p],
    "bmi_decompress_batch": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
    "bmi_decompress_batch_host": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p],
}

# domains of the public mask streams (include/bmi_tfhe.h BMI_SEED_DOMAIN_*): part of the seeded key / ciphertext format
SEED_DOMAIN_BSK_MASK, SEED_DOMAIN_KSK_MASK, SEED_DOMAIN_ENC_MASK, SEED_DOMAIN_BSK3_MASK = 3, 5, 7, 9
SEED_DOMAIN_PKSK_MASK = 11      # the compression key's masks


def seeded_mask_words(pub_key, nonce, first_word, count):
    """words first_word .. first_word + count of the ChaCha20 stream (pub_key, nonce) that seeded keys and ciphertexts take their
    masks from (bmi_seeded_mask_words; context-free, CPU)"""
    key = np.ascontiguousarray(pub_key, dtype=np.uint32).reshape(-1)
    if key.size != 8:
        raise ValueError("the public key has 8 32-bit words")
    out = np.zeros(int(count), np.uint64)
    if load_library().bmi_seeded_mask_words(_ptr(key), C.c_uint64(int(nonce)), C.c_uint64(int(first_word)), C.c_uint64(int(count)),
                                            _ptr(out)):
        raise BmiError("bmi_seeded_mask_words failed")
    return out


class SeededCiphertexts:
    """Fresh big-key ciphertexts in seeded form: ciphertext i is (encryption counter first_counter + i, body word bodies[i]); its
    masks are words of the encrypting context's public stream, which Engine.expand_seeded regenerates on the GPU."""

    def __init__(self, first_counter, bodies):
        self.first_counter = int(first_counter)
        # host words, or (for the device form of expand_seeded) a device tensor of int64 words, kept as it is
        self.bodies = bodies if hasattr(bodies, "data_ptr") else np.ascontiguousarray(bodies, dtype=np.uint64).reshape(-1)

    def __len__(self):
        return int(self.bodies.numel()) if hasattr(self.bodies, "numel") else self.bodies.size


def compressed_words(count, N):
    """values of the compressed form of `count` ciphertexts: per block of N its N mask values, then its body values"""
    return -(-int(count) // int(N)) * int(N) + int(count)


class CompressedCiphertexts:
    """`count` big-key ciphertexts in compressed form (Engine.compress_host; include/bmi_tfhe.h): per block of N ciphertexts one
    GLWE ciphertext whose 2N words are cut to log_modulus bits - words = uint32 values below 2^log_modulus, per block N mask values
    then the block's body values.  The wire form (tobytes / frombytes) is a 16-byte header - the magic b"BMIC", count, N and
    log_modulus as little-endian uint32 - then the values as uint16 for log_modulus <= 16 and uint32 otherwise."""
    MAGIC = b"BMIC"
    HEADER_BYTES = 16

    def __init__(self, count, N, log_modulus, words):
        self.count, self.N, self.log_modulus = int(count), int(N), int(log_modulus)
        self.words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        if not 2 <= self.log_modulus <= 32:
            raise ValueError("log_modulus must be in [2, 32]")
        if self.words.size != compressed_words(self.count, self.N):
            raise ValueError(f"{self.count} ciphertexts at N = {self.N} compress to {compressed_words(self.count, self.N)} values, "
                             f"not {self.words.size}")

    def __len__(self):
        return self.count

    @property
    def nbytes(self):
        """bytes of the wire form"""
        return self.HEADER_BYTES + self.words.size * (2 if self.log_modulus <= 16 else 4)

    def tobytes(self):
        head = self.MAGIC + np.array([self.count, self.N, self.log_modulus], "<u4").tobytes()
        return head + self.words.astype("<u2" if self.log_modulus <= 16 else "<u4").tobytes()

    @classmethod
    def frombytes(cls, data):
        data = bytes(data)
        if len(data) < cls.HEADER_BYTES or data[:4] != cls.MAGIC:
            raise ValueError("not a compressed ciphertext list")
        count, N, log_modulus = (int(v) for v in np.frombuffer(data, "<u4", 3, 4))
        if N not in (1024, 2048, 4096) or not 2 <= log_modulus <= 32:
            raise ValueError("compressed ciphertext list with an impossible header")
        dt = "<u2" if log_modulus <= 16 else "<u4"
        want = compressed_words(count, N)
        if len(data) != cls.HEADER_BYTES + want * np.dtype(dt).itemsize:
            raise ValueError("compressed ciphertext list of the wrong length")
        return cls(count, N, log_modulus, np.frombuffer(data, dt, want, cls.HEADER_BYTES).astype(np.uint32))


def circuit_prune(n_in, node_ptr, term_leaf, out_leaf):
    """live mask of the look-ups an output depends on (bmi_circuit_prune; context-free, CPU)"""
    node_ptr = np.ascontiguousarray(node_ptr, np.int64)
    term_leaf = np.ascontiguousarray(term_leaf, np.int32)
    out_leaf = np.ascontiguousarray(out_leaf, np.int32)
    live = np.zeros(max(node_ptr.size - 1, 0), np.uint8)
    rc = _host_library().bmi_circuit_prune(int(n_in), live.size, _ptr(node_ptr), _ptr(term_leaf), _ptr(out_leaf),
                                          out_leaf.size, _ptr(live))
    if rc != 0:
        raise BmiError(f"bmi_circuit_prune failed ({rc}): malformed circuit arrays")
    return live.astype(bool)


def circuit_schedule(n_in, node_ptr, term_leaf, round_, wide_round):
    """width-aware level (1-based) of every look-up (bmi_circuit_schedule; context-free, CPU)"""
    node_ptr = np.ascontiguousarray(node_ptr, np.int64)
    term_leaf = np.ascontiguousarray(term_leaf, np.int32)
    level = np.zeros(max(node_ptr.size - 1, 0), np.int32)
    depth = C.c_int32(0)
    rc = _host_library().bmi_circuit_schedule(int(n_in), level.size, _ptr(node_ptr), _ptr(term_leaf), int(round_),
                                             int(wide_round), _ptr(level), C.byref(depth))
    if rc != 0:
        raise BmiError(f"bmi_circuit_schedule failed ({rc}): malformed circuit arrays")
    return level


def torus64_to_field(ct, q_bits):
    """modulus switch round(x * q / 2^64) of u64 torus words; context-free (bmi_torus64_to_field)"""
    a = np.ascontiguousarray(ct, dtype=np.uint64)
    out = np.empty_like(a)
    if load_library().bmi_torus64_to_field(int(q_bits), _ptr(a), a.size, _ptr(out)):
        raise BmiError("bmi_torus64_to_field failed")
    return out


def field_to_torus64(ct, q_bits):
    """round(x * 2^64 / q) mod 2^64 of words mod q; context-free (bmi_field_to_torus64)"""
    a = np.ascontiguousarray(ct, dtype=np.uint64)
    out = np.empty_like(a)
    if load_library().bmi_field_to_torus64(int(q_bits), _ptr(a), a.size, _ptr(out)):
        raise BmiError("bmi_field_to_torus64 failed (words must be reduced mod q)")
    return out


def _load_hip_runtime():
    """libbmi_tfhe.so is linked without a HIP runtime of its own (-no-hip-rt): it binds to the one already
    in the process.  PyTorch-ROCm bundles its own libamdhip64.so, and two HIP runtimes in one process cannot
    both own the GPU, so prefer torch's copy when torch is installed; otherwise use the system ROCm."""
    cands = []
    try:
        import torch  # noqa: F401  (plumbing only: device memory / streams / torch.distributed)
        cands.append(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    except Exception:
        pass
    cands += ["/opt/rocm/lib/libamdhip64.so", "libamdhip64.so"]
    errs = []
    for c in cands:
        try:
            return C.CDLL(c, mode=C.RTLD_GLOBAL)
        except OSError as e:
            errs.append(f"{c}: {e}")
    raise BmiError("no HIP runtime (libamdhip64.so) could be loaded: " + "; ".join(errs))


def load_library():
    """Loads libbmi_tfhe.so; raises BmiError (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BmiError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(make -C bounty-matrix-inversion_amd/csrc). There is no CPU fallback for the PBS path.")
        _load_hip_runtime()
        lib = C.CDLL(LIB_PATH)
        for name, argtypes in _SIGS.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = C.c_int
        lib.bmi_ctx_destroy.argtypes = [C.c_void_p]
        lib.bmi_ctx_destroy.restype = None
        lib.bmi_last_error.argtypes = [C.c_void_p]
        lib.bmi_last_error.restype = C.c_char_p
        _lib = lib
    return _lib


def _host_library():
    """the library behind the context-free host functions that both libraries export (the circuit passes, the parameter tables):
    libbmi_tfhe.so where it loads, else libbmi_client.so (client.py), which needs neither ROCm nor a GPU"""
    try:
        return load_library()
    except BmiError:
        from . import client
        return client.load_client_library()


def default_params(q_bits=None, **kw):
    """North-star parameter set; q_bits = 64 (Goldilocks) or 49 (f64 kernels), None = the library's default."""
    return _default_params(_host_library(), q_bits, kw)


def _default_params(lib, q_bits, kw):
    P = Params()
    rc = lib.bmi_default_params(C.byref(P)) if q_bits is None else lib.bmi_default_params_for(int(q_bits), C.byref(P))
    if rc != 0:
        raise BmiError("unsupported q_bits (64, 49 or TORUS64 = 65)")
    for k, v in kw.items():
        setattr(P, k, v)
    return P


def preset_params(name, **kw):
    """named parameter set of the library: "north_star", "north_star_torus64", "north_star_goldilocks", "secure128"
    (n 742, N 2048: the 128-bit-secure set on the 49-bit field) and "secure128_torus" (the same on q = 2^64, Concrete's
    modulus, l = 3 x 10 bits); include/bmi_tfhe.h"""
    return _preset_params(_host_library(), name, kw)


def _preset_params(lib, name, kw):
    P = Params()
    if lib.bmi_preset_params(name.encode(), C.byref(P)) != 0:
        raise BmiError(f"unknown parameter preset {name!r}")
    for k, v in kw.items():
        setattr(P, k, v)
    return P


def _ptr(a):
    """host numpy array / torch tensor (host or device) / int -> raw address"""
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return C.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):
        assert a.is_contiguous()
        return C.c_void_p(a.data_ptr())
    raise TypeError(type(a))


class Engine:
    """One context = crypto parameters + keys + one GPU (reference analogue: a compiled fhe.Circuit)."""

    def __init__(self, params=None, device=0):
        self.lib = load_library()
        self.P = params if params is not None else default_params()
        h = C.c_void_p()
        rc = self.lib.bmi_ctx_create(C.byref(self.P), int(device), C.byref(h))
        if rc != 0:
            raise BmiError(f"bmi_ctx_create failed ({rc}): {self.lib.bmi_last_error(None).decode()}")
        self.h = h
        self.device = device
        self._luts = {}
        self.q_bits = self.P.q_bits or 64
        self.modulus = MODULUS[self.q_bits]
        self.log_q = 49 if self.q_bits == 49 else 64     # bits of the torus messages are scaled on

    def delta_log(self, msg_bits=4):
        """scaling exponent of a signed msg_bits-bit message space: log_q - 1 - msg_bits (59 / 44 for 4 bits)"""
        return self.log_q - 1 - msg_bits

    def close(self):
        if getattr(self, "h", None):
            self.lib.bmi_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise BmiError(f"{what} failed ({rc}): {self.lib.bmi_last_error(self.h).decode()}")

    # ---- keys
    def keygen(self, seed=None):
        """seed=None: production key generation, all randomness from the library's CSPRNG (ChaCha20 keyed by getrandom).
        An integer seed selects bmi_keygen_insecure_deterministic: reproducible keys AND reproducible encryptions for
        the oracle parity tests and for replicating one key set on every rank of a benchmark - not cryptographic."""
        if seed is None:
            self._ck(self.lib.bmi_keygen(self.h), "bmi_keygen")
        else:
            self._ck(self.lib.bmi_keygen_insecure_deterministic(self.h, C.c_uint64(seed)), "bmi_keygen_insecure_deterministic")

    def keygen_shared(self, seed=None, group=None, src=0, share_secret=False, seeded=False):
        """One set of EVALUATION keys on every rank of a torch.distributed group WITHOUT the seeded (test-only) generator: rank
        `src` generates the key set (CSPRNG when seed is None) and broadcasts the bootstrap and keyswitch keys (about 100 MB at
        the north-star set; the unrolled key too in unrolled mode); the other ranks import them as evaluation-only contexts -
        the secret keys stay on `src`, the only rank that can encrypt / decrypt (share_secret=True replicates them as well, over
        whatever transport the group uses: only for tests and trusted single-node groups).  With a single process this is
        keygen(seed).  The sharded executor needs the same evaluation keys on every GPU and checks it (executor.py).
        seeded=True (opt-in): the public key and the body words travel (0.3 of the bytes at the default set) and every rank expands
        the masks on its own GPU; where the seeded export is refused (a deterministic seed, a prime field, share_secret) the full
        form travels as before."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self.keygen(seed)
        rank = dist.get_rank(group)
        unrolled = getattr(self, "unroll", 1) == 2     # the unrolled bootstrap key travels with the set
        P, rows = self.P, (self.P.k + 1) * self.P.bs_levels
        if seeded and seed is None and not share_secret and self.q_bits == TORUS64:   # what the seeded export takes, known on every rank
            if rank == src:
                self.keygen()
                pub, bsk_body, ksk_body = self.export_keys_seeded()
                parts = [pub.astype(np.uint64), bsk_body, ksk_body] + ([self.export_bsk_unrolled_seeded()] if unrolled else [])
            else:
                parts = [np.zeros(8, np.uint64), np.zeros((P.n, rows, P.N), np.uint64), np.zeros((P.k * P.N, P.ks_levels), np.uint64)]
                if unrolled:
                    parts.append(np.zeros(self.unrolled_key_shape()[:3] + (P.N,), np.uint64))
            self._broadcast_parts(parts, group, src)
            if rank != src:
                self.import_keys_seeded(parts[0].astype(np.uint32), parts[1], parts[2])
                if unrolled:
                    self.import_bsk_unrolled_seeded(parts[3])
            return
        if rank == src:
            self.keygen(seed)
            sk_small, sk_big, bsk, ksk = self.export_keys()
            parts = ([sk_small, sk_big] if share_secret else []) + [bsk, ksk] + ([self.export_bsk_unrolled()] if unrolled else [])
        else:
            parts = ([np.zeros(P.n, np.uint64), np.zeros(P.k * P.N, np.uint64)] if share_secret else []) + \
                    [np.zeros((P.n, rows, P.k + 1, P.N), np.uint64), np.zeros((P.k * P.N, P.ks_levels, P.n + 1), np.uint64)]
            if unrolled:
                parts.append(np.zeros(self.unrolled_key_shape(), np.uint64))
        self._broadcast_parts(parts, group, src)
        if rank != src:
            sec = parts[:2] if share_secret else [None, None]
            ev = parts[2:] if share_secret else parts
            self.import_keys(sec[0], sec[1], ev[0], ev[1])
            if unrolled:
                self.import_bsk_unrolled(ev[2])

    def _broadcast_parts(self, parts, group, src):
        """the uint64 arrays `parts` from rank `src` into the same arrays on every rank (through the GPU when the backend is RCCL)"""
        import torch
        import torch.distributed as dist
        on_gpu = dist.get_backend(group) == "nccl"
        for a in parts:
            t = torch.from_numpy(a.view(np.int64))
            if on_gpu:
                t = t.to(torch.device("cuda", self.device))
            dist.broadcast(t, src=src, group=group)
            if on_gpu:
                a.view(np.int64)[...] = t.cpu().numpy()

    def eval_key_fingerprint(self):
        """64-bit fingerprint of the evaluation keys this context holds (bootstrap, keyswitch and, in unrolled mode, the unrolled
        key): equal on two contexts iff they bootstrap alike.  Used by the sharded executor to refuse ranks with different keys."""
        import hashlib
        _, _, bsk, ksk = self.export_keys(secret=False)
        h = hashlib.blake2b(digest_size=8)
        for a in (bsk, ksk) + ((self.export_bsk_unrolled(),) if getattr(self, "unroll", 1) == 2 else ()):
            h.update(np.ascontiguousarray(a).view(np.uint8).data)
        return int.from_bytes(h.digest(), "little") >> 1      # fits a signed 64-bit tensor element

    def export_keys(self, secret=True):
        """(sk_small, sk_big, bsk, ksk), standard domain; secret=False returns (None, None, bsk, ksk) and also works on
        an evaluation-only context"""
        P = self.P
        rows = (P.k + 1) * P.bs_levels
        sk_small = np.zeros(P.n, np.uint64) if secret else None
        sk_big = np.zeros(P.k * P.N, np.uint64) if secret else None
        bsk = np.zeros((P.n, rows, P.k + 1, P.N), np.uint64)
        ksk = np.zeros((P.k * P.N, P.ks_levels, P.n + 1), np.uint64)
        self._ck(self.lib.bmi_export_keys(self.h, _ptr(sk_small), _ptr(sk_big), _ptr(bsk), _ptr(ksk)), "bmi_export_keys")
        return sk_small, sk_big, bsk, ksk

    def import_keys(self, sk_small, sk_big, bsk, ksk):
        """loads a key set (layout of export_keys); sk_small = sk_big = None makes this context evaluation-only"""
        P = self.P
        rows = (P.k + 1) * P.bs_levels
        bsk = np.ascontiguousarray(bsk, dtype=np.uint64)
        ksk = np.ascontiguousarray(ksk, dtype=np.uint64)
        if bsk.size != P.n * rows * (P.k + 1) * P.N or ksk.size != P.k * P.N * P.ks_levels * (P.n + 1):
            raise BmiError("key arrays do not match this context's parameters")
        if (sk_small is None) != (sk_big is None):
            raise BmiError("pass both secret keys or neither")
        if sk_small is not None:
            sk_small = np.ascontiguousarray(sk_small, dtype=np.uint64)
            sk_big = np.ascontiguousarray(sk_big, dtype=np.uint64)
            if sk_small.size != P.n or sk_big.size != P.k * P.N:
                raise BmiError("secret key arrays do not match this context's parameters")
        self._ck(self.lib.bmi_import_keys(self.h, _ptr(sk_small), _ptr(sk_big), _ptr(bsk), _ptr(ksk)), "bmi_import_keys")

    def export_keys_seeded(self):
        """(pub_key[8] uint32, bsk_body (n, rows, N), ksk_body (k N, ks_levels)): the evaluation keys without their masks, which
        are words of the ChaCha20 stream of pub_key (include/bmi_tfhe.h).  2^64 torus, CSPRNG keys generated by this context."""
        P = self.P
        pub = np.zeros(8, np.uint32)
        bsk_body = np.zeros((P.n, (P.k + 1) * P.bs_levels, P.N), np.uint64)
        ksk_body = np.zeros((P.k * P.N, P.ks_levels), np.uint64)
        self._ck(self.lib.bmi_export_keys_seeded(self.h, _ptr(pub), _ptr(bsk_body), _ptr(ksk_body)), "bmi_export_keys_seeded")
        return pub, bsk_body, ksk_body

    def import_keys_seeded(self, pub_key, bsk_body, ksk_body):
        """loads the key set of export_keys_seeded: the masks are expanded on the GPU; this context becomes evaluation-only.  For
        the exporter's key word for word, store the key at the exporter's precision (in unrolled mode: set_bsk_unroll(2) first)."""
        P = self.P
        pub = np.ascontiguousarray(pub_key, dtype=np.uint32).reshape(-1)
        bsk_body = np.ascontiguousarray(bsk_body, dtype=np.uint64)
        ksk_body = np.ascontiguousarray(ksk_body, dtype=np.uint64)
        if pub.size != 8 or bsk_body.size != P.n * (P.k + 1) * P.bs_levels * P.N or ksk_body.size != P.k * P.N * P.ks_levels:
            raise BmiError("seeded key arrays do not match this context's parameters")
        self._ck(self.lib.bmi_import_keys_seeded(self.h, _ptr(pub), _ptr(bsk_body), _ptr(ksk_body)), "bmi_import_keys_seeded")

    def export_bsk_unrolled_seeded(self):
        """the body polynomials (pairs, 3, rows, N) of the unrolled bootstrap key; its masks come from export_keys_seeded's pub_key"""
        body = np.zeros(self.unrolled_key_shape()[:3] + (self.P.N,), np.uint64)
        self._ck(self.lib.bmi_export_bsk_unrolled_seeded(self.h, _ptr(body)), "bmi_export_bsk_unrolled_seeded")
        return body

    def import_bsk_unrolled_seeded(self, bsk3_body):
        """the unrolled key of export_bsk_unrolled_seeded, after import_keys_seeded (whose public key expands its masks)"""
        body = np.ascontiguousarray(bsk3_body, dtype=np.uint64)
        if body.size != int(np.prod(self.unrolled_key_shape()[:3])) * self.P.N:
            raise BmiError("unrolled key bodies do not match this context's parameters")
        self._ck(self.lib.bmi_import_bsk_unrolled_seeded(self.h, _ptr(body)), "bmi_import_bsk_unrolled_seeded")

    # ---- compression of output ciphertexts (2^64 torus; include/bmi_tfhe.h, csrc/lwe_pack.hip)
    def compression_keygen(self, levels=1, base_log=16):
        """the packing keyswitch key of the key set held (needs the secret keys): N * levels GLWE rows under the context's own GLWE
        key; 16.8 MB at the defaults and N = 1024.  A new key set (keygen, import_keys, load_keys) drops it.  One shape per key
        set: a second call with another (levels, base_log) is refused until the next key set (it would reuse the rows' mask and
        noise streams under other messages, which reveals the secret key; include/bmi_tfhe.h)."""
        self._ck(self.lib.bmi_compression_keygen(self.h, int(levels), int(base_log)), "bmi_compression_keygen")

    def compression_key_info(self):
        """(levels, base_log, bytes on the device); levels == 0: no compression key"""
        lv, bl, by = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._ck(self.lib.bmi_compression_key_info(self.h, C.byref(lv), C.byref(bl), C.byref(by)), "bmi_compression_key_info")
        return lv.value, bl.value, by.value

    def export_compression_key(self):
        """(N, levels, 2, N) uint64, standard domain: row (j, l) = [mask polynomial, body polynomial]"""
        levels = self.compression_key_info()[0]
        key = np.zeros((self.P.N, max(levels, 1), 2, self.P.N), np.uint64)
        self._ck(self.lib.bmi_export_compression_key(self.h, _ptr(key)), "bmi_export_compression_key")
        return key

    def import_compression_key(self, key, levels, base_log):
        key = np.ascontiguousarray(key, dtype=np.uint64)
        if key.size != self.P.N * int(levels) * 2 * self.P.N:
            raise BmiError("compression key array does not match this context's parameters and levels")
        self._ck(self.lib.bmi_import_compression_key(self.h, int(levels), int(base_log), _ptr(key)), "bmi_import_compression_key")

    def export_compression_key_seeded(self):
        """the body polynomials (N, levels, N); the masks are words of export_keys_seeded's pub_key (domain SEED_DOMAIN_PKSK_MASK)"""
        levels = self.compression_key_info()[0]
        body = np.zeros((self.P.N, max(levels, 1), self.P.N), np.uint64)
        self._ck(self.lib.bmi_export_compression_key_seeded(self.h, _ptr(body)), "bmi_export_compression_key_seeded")
        return body

    def import_compression_key_seeded(self, bodies, levels, base_log):
        """the compression key of export_compression_key_seeded, after import_keys_seeded (whose public key expands its masks)"""
        bodies = np.ascontiguousarray(bodies, dtype=np.uint64)
        if bodies.size != self.P.N * int(levels) * self.P.N:
            raise BmiError("compression key bodies do not match this context's parameters and levels")
        self._ck(self.lib.bmi_import_compression_key_seeded(self.h, int(levels), int(base_log), _ptr(bodies)),
                 "bmi_import_compression_key_seeded")

    def compressed_words(self, count):
        w = C.c_uint64()
        self._ck(self.lib.bmi_compressed_words(self.h, int(count), C.byref(w)), "bmi_compressed_words")
        return w.value

    def compress(self, d_in, count, d_out, log_modulus=16, stream=0):
        """d_out (device tensor of compressed_words(count) 32-bit values) = the compressed form of the `count` big-key ciphertexts
        d_in [count][N + 1] (device words), on `stream` (bmi_compress_batch)"""
        self._ck(self.lib.bmi_compress_batch(self.h, _ptr(d_in), int(count), int(log_modulus), _ptr(d_out), C.c_void_p(stream)),
                 "bmi_compress_batch")

    def compress_host(self, cts, log_modulus=16):
        """numpy ciphertexts (count, N + 1) -> CompressedCiphertexts"""
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, self.P.big)
        out = np.zeros(compressed_words(cts.shape[0], self.P.N), np.uint32)
        self._ck(self.lib.bmi_compress_batch_host(self.h, _ptr(cts), cts.shape[0], int(log_modulus), _ptr(out)),
                 "bmi_compress_batch_host")
        return CompressedCiphertexts(cts.shape[0], self.P.N, log_modulus, out)

    def _compressed(self, cc):
        if cc.N != self.P.N:
            raise BmiError(f"ciphertexts compressed at N = {cc.N} on a context with N = {self.P.N}")
        return cc

    def phase_compressed(self, cc):
        """phases (uint64) of a CompressedCiphertexts under this context's secret key (host)"""
        out = np.zeros(self._compressed(cc).count, np.uint64)
        self._ck(self.lib.bmi_phase_compressed(self.h, _ptr(cc.words), cc.count, cc.log_modulus, _ptr(out)), "bmi_phase_compressed")
        return out

    def decrypt_compressed(self, cc, delta_log):
        out = np.zeros(self._compressed(cc).count, np.int64)
        self._ck(self.lib.bmi_decrypt_compressed(self.h, _ptr(cc.words), cc.count, cc.log_modulus, int(delta_log), _ptr(out)),
                 "bmi_decrypt_compressed")
        return out

    # ---- ... and back (csrc/lwe_unpack.hip): no key of any kind, so a context without keys or an evaluation-only one serves
    def decompress(self, words, count, log_modulus, d_out, index=None, stream=0):
        """d_out (device tensor, rows x (N + 1) words) = big-key LWE ciphertexts of the positions index[r] (None: all `count`, in
        order) of the compressed form `words`, on `stream` (bmi_decompress_batch): the sample extraction of coefficient index[r]
        mod N of its block, shifted back up to 2^64 - the phase under sk_big is bit for bit phase_compressed's.  words and index
        are device tensors of 32-bit values (which the caller keeps alive until the stream has run), or numpy arrays, which are
        uploaded beside d_out and kept alive here until the next call.  The sizes of words and d_out are checked; every
        index < count is the caller's contract here; decompress_host checks it."""
        uploads = []

        def dev(a):
            if a is None or hasattr(a, "data_ptr"):
                return a
            import torch
            uploads.append(torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32)).to(d_out.device))
            return uploads[-1]
        d_words, d_index = dev(words), dev(index)
        rows = int(count) if index is None else int(d_index.numel())
        if int(d_words.numel()) != compressed_words(count, self.P.N) or d_words.element_size() != 4:
            raise BmiError(f"{count} ciphertexts at N = {self.P.N} compress to {compressed_words(count, self.P.N)} 32-bit values, not "
                           f"{int(d_words.numel())} of {d_words.element_size()} bytes")
        if d_index is not None and d_index.element_size() != 4:
            raise BmiError("decompress: the index is a tensor of 32-bit values")
        if int(d_out.numel()) * d_out.element_size() < rows * self.P.big * 8:
            raise BmiError(f"decompress: d_out holds {int(d_out.numel()) * d_out.element_size()} bytes, {rows} rows of {self.P.big} words "
                           f"need {rows * self.P.big * 8}")
        if index is not None and rows == 0:
            return d_out          # (an empty index has no address to tell it from an absent one)
        if uploads:
            self._decompress_uploads = uploads
        self._ck(self.lib.bmi_decompress_batch(self.h, _ptr(d_words), int(count), int(log_modulus), _ptr(d_index), rows, _ptr(d_out),
                                               C.c_void_p(stream)), "bmi_decompress_batch")
        return d_out

    def decompress_host(self, cc, index=None):
        """CompressedCiphertexts -> (rows, N + 1) uint64 ciphertexts of its positions index (None: all, in order); refuses an
        index >= len(cc) and a value that does not fit log_modulus bits (bmi_decompress_batch_host)"""
        self._compressed(cc)
        if index is not None:
            index = np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
            if index.size and (index.min() < 0 or index.max() > 0xFFFFFFFF):
                raise BmiError("decompress_host: an index is negative or does not fit 32 bits")
            index = index.astype(np.uint32)
        rows = cc.count if index is None else index.size
        out = np.zeros((rows, self.P.big), np.uint64)
        if index is not None and rows == 0:
            return out
        self._ck(self.lib.bmi_decompress_batch_host(self.h, _ptr(cc.words), cc.count, cc.log_modulus, _ptr(index), rows, _ptr(out)),
                 "bmi_decompress_batch_host")
        return out

    def keygen_from_secret(self, sk_small, sk_big, seed=0):
        """evaluation keys for binary secret keys made elsewhere (e.g. by a Concrete client); seed=0: CSPRNG masks and
        noise, seed != 0: deterministic test vectors (not cryptographic)"""
        sk_small = np.ascontiguousarray(sk_small, dtype=np.uint64)
        sk_big = np.ascontiguousarray(sk_big, dtype=np.uint64)
        if sk_small.size != self.P.n or sk_big.size != self.P.k * self.P.N:
            raise BmiError("secret key arrays do not match this context's parameters")
        self._ck(self.lib.bmi_keygen_from_secret(self.h, _ptr(sk_small), _ptr(sk_big), int(seed)), "bmi_keygen_from_secret")

    def from_torus64(self, ct):
        """ciphertext words on the 2^64 torus (Concrete's representation) -> words mod q (same shape)"""
        return torus64_to_field(ct, self.q_bits)

    def to_torus64(self, ct):
        """ciphertext words mod q -> words on the 2^64 torus (same shape)"""
        return field_to_torus64(ct, self.q_bits)

    _PARAM_FIELDS = ("n", "log_N", "k", "bs_levels", "bs_base_log", "ks_levels", "ks_base_log", "q_bits", "lwe_noise", "glwe_noise")

    def save_keys(self, path, secret=True, seeded=False):
        """Key file (numpy .npz): the parameter set and the standard-domain keys.  secret=False writes the evaluation
        keys only - what a server needs (the reference's analogue: Concrete's key cache, qfloat_matrix_inversion.py:997).
        seeded=True (evaluation keys only: refused with secret=True): the seeded form - pub_key, bsk_body, ksk_body, in unrolled
        mode bsk_unrolled_body, params, and bsk_precision (the precision the bodies were rounded at, which the loading context
        must store the key at) - 0.3 of the full file at the default set; load_keys expands the masks on the GPU.
        Either form carries the compression key, if the engine holds one, and its (levels, base_log): in full, or in a seeded file
        as its bodies (a compression key that was loaded by import_compression_key has no seeded form and travels in full there)."""
        if seeded:
            if secret:
                raise BmiError("a seeded key file holds evaluation keys only: save_keys(path, secret=False, seeded=True)")
            pub, bsk_body, ksk_body = self.export_keys_seeded()
            arrays = {"pub_key": pub, "bsk_body": bsk_body, "ksk_body": ksk_body, "bsk_precision": np.array([self.bsk_precision]),
                      "params": np.array([float(getattr(self.P, f)) for f in self._PARAM_FIELDS])}
            if getattr(self, "unroll", 1) == 2:
                arrays["bsk_unrolled_body"] = self.export_bsk_unrolled_seeded()
            if self.compression_key_info()[0]:       # the compression key travels with the set: its bodies and (levels, base_log)
                try:
                    arrays["compression_key_body"] = self.export_compression_key_seeded()
                except BmiError:                     # a key loaded by import_compression_key has no seeded form: it travels in full
                    arrays["compression_key"] = self.export_compression_key()
                arrays["compression_shape"] = np.array(self.compression_key_info()[:2])
            with open(path, "wb") as f:
                np.savez(f, **arrays)
            return
        sk_small, sk_big, bsk, ksk = self.export_keys(secret=secret)
        arrays = {"bsk": bsk, "ksk": ksk, "params": np.array([float(getattr(self.P, f)) for f in self._PARAM_FIELDS])}
        if secret:
            arrays.update(sk_small=sk_small, sk_big=sk_big)
        if getattr(self, "unroll", 1) == 2:          # the unrolled bootstrap key travels with the set
            arrays["bsk_unrolled"] = self.export_bsk_unrolled()
        if self.q_bits == TORUS64 and self.compression_key_info()[0]:
            arrays["compression_key"] = self.export_compression_key()
            arrays["compression_shape"] = np.array(self.compression_key_info()[:2])
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    def load_keys(self, path):
        """loads a key file written by save_keys; the file's parameter set must equal this context's"""
        with np.load(path) as z:
            mine = [float(getattr(self.P, f)) for f in self._PARAM_FIELDS]
            mine[7] = float(self.q_bits)
            theirs = list(z["params"])
            if theirs[7] == 0:
                theirs[7] = 64.0
            if mine != theirs:
                raise BmiError(f"key file parameters {theirs} differ from this context's {mine}")
            if "pub_key" in z.files:                 # the seeded form (save_keys(..., seeded=True)): evaluation keys only
                unrolled = "bsk_unrolled_body" in z.files
                if unrolled:                         # before the keys: the mode decides the precision they are stored at
                    self.set_bsk_unroll(2)
                prec = int(z["bsk_precision"][0])
                if self.bsk_precision != prec:       # the masks must be rounded the way the writer's were
                    self.set_bsk_precision(prec)
                self.import_keys_seeded(z["pub_key"], z["bsk_body"], z["ksk_body"])
                if unrolled:
                    self.import_bsk_unrolled_seeded(z["bsk_unrolled_body"])
                if "compression_key_body" in z.files:
                    self.import_compression_key_seeded(z["compression_key_body"], *(int(v) for v in z["compression_shape"]))
                elif "compression_key" in z.files:
                    self.import_compression_key(z["compression_key"], *(int(v) for v in z["compression_shape"]))
                return False
            has_secret = "sk_small" in z.files
            self.import_keys(z["sk_small"] if has_secret else None, z["sk_big"] if has_secret else None, z["bsk"], z["ksk"])
            if "bsk_unrolled" in z.files:            # written by a context in unrolled mode: this one switches to it too
                self.set_bsk_unroll(2)
                self.import_bsk_unrolled(z["bsk_unrolled"])
            elif getattr(self, "unroll", 1) == 2 and has_secret:
                self.set_bsk_unroll(2)               # no unrolled key in the file: derived from the secret keys just loaded
            if "compression_key" in z.files:
                self.import_compression_key(z["compression_key"], *(int(v) for v in z["compression_shape"]))
        return has_secret

    def key_bytes(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._ck(self.lib.bmi_key_bytes(self.h, C.byref(a), C.byref(b)), "bmi_key_bytes")
        return a.value, b.value

    # ---- encrypt / decrypt (host buffers)
    def encrypt(self, msgs, delta_log):
        msgs = np.ascontiguousarray(msgs, dtype=np.int64).reshape(-1)
        out = np.zeros((msgs.size, self.P.big), np.uint64)
        self._ck(self.lib.bmi_encrypt(self.h, _ptr(msgs), msgs.size, delta_log, _ptr(out)), "bmi_encrypt")
        return out

    def encrypt_seeded(self, msgs, delta_log):
        """encrypt() in seeded form: SeededCiphertexts(first_counter, bodies), 8 bytes per ciphertext - the ciphertexts encrypt()
        would have returned at this context's encryption counter, without their masks (bmi_encrypt_seeded)"""
        msgs = np.ascontiguousarray(msgs, dtype=np.int64).reshape(-1)
        bodies = np.zeros(msgs.size, np.uint64)
        first = C.c_uint64(0)
        self._ck(self.lib.bmi_encrypt_seeded(self.h, _ptr(msgs), msgs.size, delta_log, C.byref(first), _ptr(bodies)),
                 "bmi_encrypt_seeded")
        return SeededCiphertexts(first.value, bodies)

    def expand_seeded(self, seeded, d_out=None, stream=0):
        """SeededCiphertexts -> the full ciphertexts (count, k N + 1), masks regenerated on the GPU from this context's public key
        (a server: the one of import_keys_seeded).  Host form (d_out None): numpy in, numpy out.  Device form: seeded.bodies may
        be a device tensor of int64 words, d_out is a device tensor of count x (k N + 1) words, filled on `stream`."""
        if d_out is not None:
            bodies = seeded.bodies
            count = int(bodies.numel()) if hasattr(bodies, "numel") else int(bodies.size)
            if isinstance(bodies, np.ndarray):       # host bodies into a device tensor beside d_out
                import torch
                bodies = torch.from_numpy(bodies.view(np.int64)).to(d_out.device)
            self._ck(self.lib.bmi_expand_seeded_batch(self.h, C.c_uint64(seeded.first_counter), _ptr(bodies), count, _ptr(d_out),
                                                      C.c_void_p(stream)), "bmi_expand_seeded_batch")
            return d_out
        return self.expand_seeded_host(seeded.first_counter, seeded.bodies)

    def expand_seeded_host(self, first_counter, bodies):
        """the ciphertexts (first_counter + i, bodies[i]) in full: (count, k N + 1) uint64 (bmi_expand_seeded_batch_host)"""
        bodies = np.ascontiguousarray(bodies, dtype=np.uint64).reshape(-1)
        out = np.zeros((bodies.size, self.P.big), np.uint64)
        self._ck(self.lib.bmi_expand_seeded_batch_host(self.h, C.c_uint64(int(first_counter)), _ptr(bodies), bodies.size, _ptr(out)),
                 "bmi_expand_seeded_batch_host")
        return out

    def decrypt(self, cts, delta_log):
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, self.P.big)
        out = np.zeros(cts.shape[0], np.int64)
        self._ck(self.lib.bmi_decrypt(self.h, _ptr(cts), cts.shape[0], delta_log, _ptr(out)), "bmi_decrypt")
        return out

    def phase(self, cts):
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, self.P.big)
        out = np.zeros(cts.shape[0], np.uint64)
        self._ck(self.lib.bmi_phase(self.h, _ptr(cts), cts.shape[0], _ptr(out)), "bmi_phase")
        return out

    # ---- LUTs
    def lut_register(self, table, msg_bits, out_delta_log):
        table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1)
        if table.size != 1 << msg_bits:
            raise ValueError("table must have 2^msg_bits entries")
        key = (table.tobytes(), msg_bits, out_delta_log)
        if key in self._luts:
            return self._luts[key]
        lid = C.c_uint32()
        self._ck(self.lib.bmi_lut_register(self.h, _ptr(table), msg_bits, out_delta_log, C.byref(lid)), "bmi_lut_register")
        self._luts[key] = lid.value
        return lid.value

    def lut_register_base(self, unit_log):
        """2^64 torus: the id of the base polynomial + 2^(unit_log - 1) sum_x X^x that the tables of a shared rotation with this
        unit are factors of (one id per unit)"""
        lid = C.c_uint32()
        self._ck(self.lib.bmi_lut_register_base(self.h, int(unit_log), C.byref(lid)), "bmi_lut_register_base")
        return lid.value

    def lut_get(self, lut_id):
        tv = np.zeros(self.P.N, np.uint64)
        self._ck(self.lib.bmi_lut_get(self.h, lut_id, _ptr(tv)), "bmi_lut_get")
        return tv

    def set_kernel_variant(self, v):
        """blind rotation: 0 auto, 1 pair kernel exchanging per level, 2 latency kernel (two wavefronts per transform on
        the 49-bit field), 3 pair kernel exchanging per CMUX, 4 latency kernel with one wavefront per transform, 5 (2^64 torus,
        48-bit key in base 2^10) pair kernel with the exact limb products carried by the f64 complex FFT, 6 its latency form"""
        self._ck(self.lib.bmi_set_kernel_variant(self.h, int(v)), "bmi_set_kernel_variant")

    def rotation_kernel(self, count):
        """name of the blind-rotation kernel the engine's current mode and kernel variant run for a batch of `count` ciphertexts
        (answered by the library's dispatch itself: include/bmi_tfhe.h bmi_rotation_kernel)"""
        name = C.c_char_p()
        self._ck(self.lib.bmi_rotation_kernel(self.h, int(count), C.byref(name)), "bmi_rotation_kernel")
        return name.value.decode()

    def set_bsk_precision(self, bits):
        """2^64 torus, before keygen: 64 = exact key (three limbs); 48 = key rounded to 48 bits (two limbs, 2/3 of the work; the
        default at Bg = 2^10, the torus parameter set); 42 = rounded to 42 bits (two limbs at Bg = 2^15, noisier); N = 2048 / 4096 take 46 / 44 only, and N = 2048 in unrolled mode 40
        (include/bmi_tfhe.h)"""
        self._ck(self.lib.bmi_set_bsk_precision(self.h, int(bits)), "bmi_set_bsk_precision")

    @property
    def bsk_precision(self):
        """bits of precision the bootstrap key is stored at (64 = exact; the prime fields always)"""
        v = C.c_uint32()
        self._ck(self.lib.bmi_get_bsk_precision(self.h, C.byref(v)), "bmi_get_bsk_precision")
        return v.value

    def set_bsk_unroll(self, factor):
        """49-bit field, N = 1024 (or N = 2048 with l <= 2), or the 2^64 torus at its default set and at N = 2048 (secure128_torus: the key
        is then stored at 40 bits): 1 = CGGI's blind rotation (default), 2 = two LWE coefficients per step with an unrolled
        bootstrap key (generated by the next keygen, or at once from the secret keys already held); include/bmi_tfhe.h"""
        self._ck(self.lib.bmi_set_bsk_unroll(self.h, int(factor)), "bmi_set_bsk_unroll")
        self.unroll = int(factor)

    def unrolled_key_shape(self):
        P = self.P
        return ((P.n + 1) // 2, 3, (P.k + 1) * P.bs_levels, P.k + 1, P.N)

    def export_bsk_unrolled(self):
        bsk3 = np.zeros(self.unrolled_key_shape(), np.uint64)
        self._ck(self.lib.bmi_export_bsk_unrolled(self.h, _ptr(bsk3)), "bmi_export_bsk_unrolled")
        return bsk3

    def import_bsk_unrolled(self, bsk3):
        """the unrolled bootstrap key of the key set this context holds (layout of export_bsk_unrolled)"""
        bsk3 = np.ascontiguousarray(bsk3, dtype=np.uint64)
        if bsk3.size != int(np.prod(self.unrolled_key_shape())):
            raise BmiError("unrolled key array does not match this context's parameters")
        self._ck(self.lib.bmi_import_bsk_unrolled(self.h, _ptr(bsk3)), "bmi_import_bsk_unrolled")

    def set_keyswitch_variant(self, v):
        """keyswitch: 0 auto (int8 matrix-core product), 1 scalar kernel"""
        self._ck(self.lib.bmi_set_keyswitch_variant(self.h, int(v)), "bmi_set_keyswitch_variant")

    def set_modswitch(self, mode):
        """modulus switch of pbs / pbs_shared and their host forms: 0 = standard (default), 1 = centred - the bodies of the
        keyswitched ciphertexts minus half the sum of the mask words' rounding errors, which takes the rounding variance from
        (1 + hw(s)) / 12 to (1 + n/4) / 12 positions^2 (2^64 torus and 49-bit field; include/bmi_tfhe.h).  keyswitch and
        blind_rotate are the same in both modes."""
        self._ck(self.lib.bmi_set_modswitch(self.h, int(mode)), "bmi_set_modswitch")

    @property
    def modswitch(self):
        """the modulus-switch mode in force (0 standard, 1 centred)"""
        v = C.c_uint32()
        self._ck(self.lib.bmi_get_modswitch(self.h, C.byref(v)), "bmi_get_modswitch")
        return v.value

    def modswitch_centre_host(self, small):
        """the centred bodies of small-key ciphertexts [count][n + 1] (mask words unchanged); whatever the mode"""
        small = np.ascontiguousarray(small, dtype=np.uint64).reshape(-1, self.P.small)
        out = np.zeros_like(small)
        self._ck(self.lib.bmi_modswitch_centre_batch_host(self.h, _ptr(small), small.shape[0], _ptr(out)),
                 "bmi_modswitch_centre_batch_host")
        return out

    # ---- hot path, host buffers (numpy in / numpy out)
    def pbs_host(self, cts, lut_ids):
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, self.P.big)
        ids = np.ascontiguousarray(lut_ids, dtype=np.uint32).reshape(-1)
        assert ids.size == cts.shape[0]
        out = np.zeros_like(cts)
        self._ck(self.lib.bmi_pbs_batch_host(self.h, _ptr(cts), _ptr(ids), cts.shape[0], _ptr(out)), "bmi_pbs_batch_host")
        return out

    def keyswitch_host(self, cts):
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, self.P.big)
        out = np.zeros((cts.shape[0], self.P.small), np.uint64)
        self._ck(self.lib.bmi_keyswitch_batch_host(self.h, _ptr(cts), cts.shape[0], _ptr(out)), "bmi_keyswitch_batch_host")
        return out

    def blind_rotate_host(self, small, lut_ids):
        small = np.ascontiguousarray(small, dtype=np.uint64).reshape(-1, self.P.small)
        ids = np.ascontiguousarray(lut_ids, dtype=np.uint32).reshape(-1)
        out = np.zeros((small.shape[0], self.P.big), np.uint64)
        self._ck(self.lib.bmi_blind_rotate_batch_host(self.h, _ptr(small), _ptr(ids), small.shape[0], _ptr(out)),
                 "bmi_blind_rotate_batch_host")
        return out

    def blind_rotate_glwe_host(self, small, lut_ids):
        """blind_rotate_host returning the accumulators [count][2N] (mask polynomial, then body) instead of the extracted samples"""
        small = np.ascontiguousarray(small, dtype=np.uint64).reshape(-1, self.P.small)
        ids = np.ascontiguousarray(lut_ids, dtype=np.uint32).reshape(-1)
        out = np.zeros((small.shape[0], 2 * self.P.N), np.uint64)
        self._ck(self.lib.bmi_blind_rotate_glwe_batch_host(self.h, _ptr(small), _ptr(ids), small.shape[0], _ptr(out)),
                 "bmi_blind_rotate_glwe_batch_host")
        return out

    def _groups(self, group_ptr, base_ids, lut_ids):
        gp = np.ascontiguousarray(group_ptr, dtype=np.uint32).reshape(-1)
        base = np.ascontiguousarray(base_ids, dtype=np.uint32).reshape(-1)
        ids = np.ascontiguousarray(lut_ids, dtype=np.uint32).reshape(-1)
        if gp.size != base.size + 1:
            raise ValueError("group_ptr must have one entry more than there are groups")
        return gp, base, ids

    def glwe_lookup_host(self, glwe, group_ptr, base_ids, lut_ids):
        """the look-ups lut_ids[group_ptr[g] : group_ptr[g+1]] of accumulator g (a rotation of the base polynomial base_ids[g])
        -> [len(lut_ids)][N + 1] ciphertexts"""
        gp, base, ids = self._groups(group_ptr, base_ids, lut_ids)
        glwe = np.ascontiguousarray(glwe, dtype=np.uint64).reshape(base.size, 2 * self.P.N)
        out = np.zeros((ids.size, self.P.big), np.uint64)
        self._ck(self.lib.bmi_glwe_lookup_batch_host(self.h, _ptr(glwe), _ptr(gp), _ptr(base), _ptr(ids), base.size, ids.size,
                                                     _ptr(out)), "bmi_glwe_lookup_batch_host")
        return out

    def pbs_shared_host(self, cts, group_ptr, base_ids, lut_ids):
        """pbs_host with one keyswitch and one rotation per GROUP: ciphertext g is looked up in the tables
        lut_ids[group_ptr[g] : group_ptr[g+1]] -> [len(lut_ids)][N + 1] ciphertexts"""
        gp, base, ids = self._groups(group_ptr, base_ids, lut_ids)
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(base.size, self.P.big)
        out = np.zeros((ids.size, self.P.big), np.uint64)
        self._ck(self.lib.bmi_pbs_shared_batch_host(self.h, _ptr(cts), _ptr(gp), _ptr(base), _ptr(ids), base.size, ids.size, _ptr(out)),
                 "bmi_pbs_shared_batch_host")
        return out

    def fft_margin_host(self, small, lut_ids):
        """test hook (2^64 torus, 48-bit key in base 2^10): blind rotation by the floating-point-transform wave-pair kernel ->
        (outputs, largest distance of a limb sum from the integer it was rounded to)"""
        small = np.ascontiguousarray(small, dtype=np.uint64).reshape(-1, self.P.small)
        ids = np.ascontiguousarray(lut_ids, dtype=np.uint32).reshape(-1)
        out = np.zeros((small.shape[0], self.P.big), np.uint64)
        dist = C.c_double(0.0)
        self._ck(self.lib.bmi_fft_margin_host(self.h, _ptr(small), _ptr(ids), small.shape[0], _ptr(out), C.byref(dist)),
                 "bmi_fft_margin_host")
        return out, float(dist.value)

    def negacyclic_mul_host(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, self.P.N)
        b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, self.P.N)
        c = np.zeros_like(a)
        self._ck(self.lib.bmi_negacyclic_mul_host(self.h, _ptr(a), _ptr(b), a.shape[0], _ptr(c)), "bmi_negacyclic_mul_host")
        return c

    # ---- hot path, device buffers (torch int64 tensors viewed as uint64 words; `stream` = raw hipStream_t)
    def pbs(self, d_in, d_lut_ids, count, d_out, stream=0):
        self._ck(self.lib.bmi_pbs_batch(self.h, _ptr(d_in), _ptr(d_lut_ids), count, _ptr(d_out), C.c_void_p(stream)),
                 "bmi_pbs_batch")

    def keyswitch(self, d_in, count, d_small, stream=0):
        self._ck(self.lib.bmi_keyswitch_batch(self.h, _ptr(d_in), count, _ptr(d_small), C.c_void_p(stream)),
                 "bmi_keyswitch_batch")

    def modswitch_centre(self, d_in, count, d_out, stream=0):
        """d_out = the small ciphertexts d_in [count][n + 1] with centred bodies (bmi_modswitch_centre_batch; d_out may be d_in)"""
        self._ck(self.lib.bmi_modswitch_centre_batch(self.h, _ptr(d_in), count, _ptr(d_out), C.c_void_p(stream)),
                 "bmi_modswitch_centre_batch")

    def blind_rotate(self, d_small, d_lut_ids, count, d_out, stream=0):
        self._ck(self.lib.bmi_blind_rotate_batch(self.h, _ptr(d_small), _ptr(d_lut_ids), count, _ptr(d_out),
                                                 C.c_void_p(stream)), "bmi_blind_rotate_batch")

    def blind_rotate_glwe(self, d_small, d_lut_ids, count, d_glwe, stream=0):
        self._ck(self.lib.bmi_blind_rotate_glwe_batch(self.h, _ptr(d_small), _ptr(d_lut_ids), count, _ptr(d_glwe),
                                                      C.c_void_p(stream)), "bmi_blind_rotate_glwe_batch")

    def glwe_lookup(self, d_glwe, d_group_ptr, d_base_ids, d_lut_ids, groups, total, d_out, stream=0):
        self._ck(self.lib.bmi_glwe_lookup_batch(self.h, _ptr(d_glwe), _ptr(d_group_ptr), _ptr(d_base_ids), _ptr(d_lut_ids), groups,
                                                total, _ptr(d_out), C.c_void_p(stream)), "bmi_glwe_lookup_batch")

    def pbs_shared(self, d_in, d_group_ptr, d_base_ids, d_lut_ids, groups, total, d_out, stream=0):
        """keyswitch + one rotation per group + the groups' look-ups (bmi_pbs_shared_batch)"""
        self._ck(self.lib.bmi_pbs_shared_batch(self.h, _ptr(d_in), _ptr(d_group_ptr), _ptr(d_base_ids), _ptr(d_lut_ids), groups,
                                               total, _ptr(d_out), C.c_void_p(stream)), "bmi_pbs_shared_batch")

    def lincomb(self, d_store, d_row_ptr, d_idx, d_coef, d_const, count, d_out, stream=0):
        self._ck(self.lib.bmi_lincomb_batch(self.h, _ptr(d_store), _ptr(d_row_ptr), _ptr(d_idx), _ptr(d_coef),
                                            _ptr(d_const), count, _ptr(d_out), C.c_void_p(stream)), "bmi_lincomb_batch")

    def scatter_rows(self, d_src, count, d_store, d_rows, stream=0):
        self._ck(self.lib.bmi_scatter_rows(self.h, _ptr(d_src), count, _ptr(d_store), _ptr(d_rows), C.c_void_p(stream)),
                 "bmi_scatter_rows")

    def phase_device(self, d_ct, count, d_phase, stream=0):
        """d_phase[i] = phase of the big-key ciphertext d_ct[i] (bmi_phase_batch); the context keeps a copy of the big secret key
        on the device from the first call on (include/bmi_tfhe.h)"""
        self._ck(self.lib.bmi_phase_batch(self.h, _ptr(d_ct), count, _ptr(d_phase), C.c_void_p(stream)), "bmi_phase_batch")

    def decrypt_device(self, d_ct, count, delta_log, d_msgs, d_expected=None, d_err=None, stream=0):
        """d_msgs[i] = the message of d_ct[i] at delta_log, by decrypt()'s rule (bmi_decrypt_batch); d_err (optional) = the signed
        centred residue phase - e 2^delta_log, e = d_expected[i] if given, else the decoded message"""
        self._ck(self.lib.bmi_decrypt_batch(self.h, _ptr(d_ct), count, delta_log, _ptr(d_expected), _ptr(d_msgs), _ptr(d_err),
                                            C.c_void_p(stream)), "bmi_decrypt_batch")

    def noise_stats(self, d_ct, count, delta_log, d_expected):
        """Decrypts `count` device ciphertexts against the int64 device tensor d_expected and reduces on the device; only the
        scalars come home: {count, wrong (messages != expected), mean, std (of the error about the expected value, as a
        fraction of q), max_abs (of that error, in units of the modulus' words)}"""
        import torch
        with torch.cuda.device(d_ct.device):
            msgs = torch.empty(count, dtype=torch.int64, device=d_ct.device)
            err = torch.empty(count, dtype=torch.int64, device=d_ct.device)
            self.decrypt_device(d_ct, count, delta_log, msgs, d_expected, err, torch.cuda.current_stream().cuda_stream)
            e = err.double() / float(self.modulus)
            return {"count": int(count), "wrong": int((msgs != d_expected[:count]).sum().item()),
                    "mean": float(e.mean().item()) if count else 0.0,
                    "std": float(e.std(unbiased=False).item()) if count else 0.0,
                    "max_abs": int(err.abs().max().item()) if count else 0}

    def reserve(self, max_count):
        self._ck(self.lib.bmi_reserve(self.h, int(max_count)), "bmi_reserve")

    def sync(self, stream=0):
        self._ck(self.lib.bmi_sync(self.h, C.c_void_p(stream)), "bmi_sync")
