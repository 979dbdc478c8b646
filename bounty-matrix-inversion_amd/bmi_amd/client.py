"""The client half without a GPU: ctypes binding of libbmi_client.so (include/bmi_client.h).

`ClientEngine` draws keys, writes and reloads key files, encrypts and decrypts on the host; it offers these methods under the
names, and with the code, of `tfhe.Engine`, so a file one of them writes the other reads, and for one parameter set, settings and
seed they hold the same words.  It evaluates nothing: look-ups, keyswitch, expansion and compression are a server's
(`tfhe.Engine`, after `load_keys` of the file a client wrote).  Importing this module and running a whole keygen / encrypt /
decrypt cycle loads neither torch nor a HIP runtime nor libbmi_tfhe.so."""
from __future__ import annotations

import ctypes as C
import os

from . import tfhe
from .tfhe import BmiError, CompressedCiphertexts, Engine, Params, SeededCiphertexts   # noqa: F401  (the classes of tfhe.py)

CLIENT_LIB_PATH = os.path.join(os.path.dirname(tfhe.LIB_PATH), "libbmi_client.so")
NO_DEVICE = -1          # BMI_CLIENT_NO_DEVICE: the only `device` bmi_ctx_create of the client library takes

# the subset of include/bmi_tfhe.h the client library exports (csrc/bmi_client.map), signatures as in tfhe._SIGS
EXPORTS = (
    "bmi_default_params", "bmi_default_params_for", "bmi_preset_params", "bmi_get_params", "bmi_ctx_create",
    "bmi_set_bsk_precision", "bmi_get_bsk_precision", "bmi_set_bsk_unroll",
    "bmi_keygen", "bmi_keygen_insecure_deterministic", "bmi_keygen_from_secret", "bmi_export_keys", "bmi_import_keys",
    "bmi_export_bsk_unrolled", "bmi_import_bsk_unrolled", "bmi_export_keys_seeded", "bmi_export_bsk_unrolled_seeded",
    "bmi_compression_keygen", "bmi_compression_key_info", "bmi_export_compression_key", "bmi_import_compression_key",
    "bmi_export_compression_key_seeded",
    "bmi_encrypt", "bmi_encrypt_seeded", "bmi_decrypt", "bmi_phase", "bmi_phase_compressed", "bmi_decrypt_compressed",
    "bmi_compressed_words", "bmi_seeded_mask_words", "bmi_torus64_to_field", "bmi_field_to_torus64",
    "bmi_circuit_prune", "bmi_circuit_schedule",
)

_lib = None


def load_client_library():
    """Loads libbmi_client.so (no HIP runtime, no GPU); raises BmiError when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(CLIENT_LIB_PATH):
            raise BmiError(f"{CLIENT_LIB_PATH} not found: build it with `make -C bounty-matrix-inversion_amd/csrc` "
                           "(a C++17 compiler is all it needs)")
        lib = C.CDLL(CLIENT_LIB_PATH)
        for name in EXPORTS:
            fn = getattr(lib, name)
            fn.argtypes = tfhe._SIGS[name]
            fn.restype = C.c_int
        lib.bmi_ctx_destroy.argtypes = [C.c_void_p]
        lib.bmi_ctx_destroy.restype = None
        lib.bmi_last_error.argtypes = [C.c_void_p]
        lib.bmi_last_error.restype = C.c_char_p
        _lib = lib
    return _lib


def default_params(q_bits=None, **kw):
    """tfhe.default_params from the client library's own table (the same table: csrc/key_set.hpp)"""
    return tfhe._default_params(load_client_library(), q_bits, kw)


def preset_params(name, **kw):
    """tfhe.preset_params from the client library's own table"""
    return tfhe._preset_params(load_client_library(), name, kw)


def _server_only(name):
    def refuse(self, *args, **kwargs):
        raise BmiError(f"{name} is a server's: a ClientEngine holds keys and encrypts / decrypts on the host only - use a "
                       "tfhe.Engine (on a GPU) after Engine.load_keys of the evaluation-key file this client wrote")
    refuse.__name__ = name
    return refuse


class ClientEngine:
    """One context = crypto parameters + keys, no GPU (the client of INTEGRATION section 5).  The methods below are tfhe.Engine's
    own functions, run against libbmi_client.so."""

    def __init__(self, params=None):
        self.lib = load_client_library()
        self.P = params if params is not None else default_params()
        h = C.c_void_p()
        rc = self.lib.bmi_ctx_create(C.byref(self.P), NO_DEVICE, C.byref(h))
        if rc != 0:
            raise BmiError(f"bmi_ctx_create failed ({rc}): {self.lib.bmi_last_error(None).decode()}")
        self.h = h
        self.device = None
        self.q_bits = self.P.q_bits or 64
        self.modulus = tfhe.MODULUS[self.q_bits]
        self.log_q = 49 if self.q_bits == 49 else 64     # bits of the torus messages are scaled on
        # the modulus-switch mode of the server this client's error budget is priced for (error_budget.py reads it; a client
        # switches nothing itself)
        self.modswitch = 0

    def set_modswitch(self, mode):
        if int(mode) not in (0, 1):
            raise BmiError("modulus-switch mode must be 0 (standard) or 1 (centred)")
        self.modswitch = int(mode)

    delta_log = Engine.delta_log
    close = Engine.close
    __del__ = Engine.__del__
    _ck = Engine._ck
    _PARAM_FIELDS = Engine._PARAM_FIELDS
    # ---- keys
    keygen = Engine.keygen
    keygen_from_secret = Engine.keygen_from_secret
    export_keys = Engine.export_keys
    import_keys = Engine.import_keys
    export_keys_seeded = Engine.export_keys_seeded
    export_bsk_unrolled_seeded = Engine.export_bsk_unrolled_seeded
    set_bsk_precision = Engine.set_bsk_precision
    bsk_precision = Engine.bsk_precision
    set_bsk_unroll = Engine.set_bsk_unroll
    unrolled_key_shape = Engine.unrolled_key_shape
    export_bsk_unrolled = Engine.export_bsk_unrolled
    import_bsk_unrolled = Engine.import_bsk_unrolled
    compression_keygen = Engine.compression_keygen
    compression_key_info = Engine.compression_key_info
    export_compression_key = Engine.export_compression_key
    import_compression_key = Engine.import_compression_key
    export_compression_key_seeded = Engine.export_compression_key_seeded
    save_keys = Engine.save_keys
    load_keys = Engine.load_keys      # of a file with both secret keys; a seeded or evaluation-only file is a server's
    # ---- data
    encrypt = Engine.encrypt
    encrypt_seeded = Engine.encrypt_seeded
    decrypt = Engine.decrypt
    phase = Engine.phase
    compressed_words = Engine.compressed_words
    _compressed = Engine._compressed
    phase_compressed = Engine.phase_compressed
    decrypt_compressed = Engine.decrypt_compressed
    # ---- what load_keys of a server's file, or a caller that took this for an Engine, would reach
    import_keys_seeded = _server_only("import_keys_seeded")
    import_bsk_unrolled_seeded = _server_only("import_bsk_unrolled_seeded")
    import_compression_key_seeded = _server_only("import_compression_key_seeded")
    expand_seeded = _server_only("expand_seeded")
    pbs_host = _server_only("pbs_host")
    compress_host = _server_only("compress_host")
    decompress_host = _server_only("decompress_host")
    lut_register = _server_only("lut_register")
