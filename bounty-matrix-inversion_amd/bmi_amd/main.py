"""EncryptedMatrixInversion — the drop-in counterpart of the reference's API wrapper
(matrix_inversion/main.py:17-116): same constructor arguments and the same
quantize / encrypt / evaluate / decrypt / dequantize / run methods (+ keygen, which the reference reaches
as `circuit.keygen()`, main.py:177).  `evaluate` runs every PBS on the MI355X through libbmi_tfhe.so and
raises if the library or the GPU is missing; `run(..., simulate=True)` evaluates the traced circuit in
plaintext, exactly like the reference's `circuit.simulate` branch (main.py:106-109)."""
from __future__ import annotations

import time
from typing import Tuple

import numpy as np

from .circuit import Circuit, MSG_BITS   # noqa: F401
from .program import Program, compile_cached   # noqa: F401
from .qfloat import QFloat   # noqa: F401
from .qfloat_matrix_inversion import float_matrix_to_qfloat_arrays, qfloat_and_signs_arrays_to_float_matrix
# the circuit of a configuration (tracing, division radix, compiled + cached program) lives in inverse_circuit.py - the module the
# tracer fingerprint covers; re-exported here under the names importers use
from .inverse_circuit import (estimated_evaluate_ms, message_bits_for, trace_inverse, _trace_inverse,   # noqa: F401
                              compile_inverse)


class EncryptedMatrixInversion:
    shape: Tuple[int, int]

    def __init__(self, n, sampler=None, qfloat_base=2, qfloat_len=32, qfloat_ints=16, true_division=False,
                 tensorize=False, engine=None, device=0, shard_threshold=None, cache=True, unroll=False, q_bits=None,
                 params=None, p_error=None, share_rotations=False, centred_modswitch=False, compress_outputs=False, client=False):
        """The reference's seven arguments (main.py:17-36), then: engine / device (the GPU context to use) and
        shard_threshold (with torch.distributed initialised on several ranks, levels at least this wide are split
        across the ranks' GPUs; None = every level wider than one kernel round, levels re-packed for the rank count,
        see executor.py); unroll (when this object creates the engine, 4-bit look-ups): bootstrap-key unrolling, two LWE
        coefficients per blind-rotation step (bmi_set_bsk_unroll; key noise 2^-41 so that the look-up margin of the default set
        is kept) - 2.6 ms per level instead of 3.6; q_bits (when this object creates the engine): the ciphertext modulus, None =
        the library's default = tfhe.TORUS64 = 2^64, the torus concrete-python computes on (its default set: Bg = 2^10,
        bootstrap key at 48 bits of precision; with unroll=True the unrolled torus kernel, key noise unchanged), 49 = the prime field
        2^49 - 720895 (with unroll=True the engine with the shortest single bootstrap: 0.83 s for the 3x3 against 1.26 s); params (when
        this object creates the engine): a named parameter set of the library ("secure128_torus", "secure128": the 128-bit-secure
        sets, include/bmi_tfhe.h) or a tfhe.Params - what `fhe.Compiler.compile`'s parameter optimiser chooses for the reference
        (main.py:53-66); it overrides q_bits; p_error (when this object creates the engine and params is not given): the bound on
        the probability that noise makes the whole evaluation wrong (Concrete's `global_p_error`, 1e-5 there) - the first
        parameter set of the chosen modulus whose error budget for THIS circuit meets it is taken (error_budget.choose_params:
        N = 1024 for small circuits, N = 2048 where the look-up count needs the wider margin, e.g. the 8x8 inverse); None keeps
        the north-star set and reports its budget in `self.error_budget`; share_rotations (2^64 torus, one rank): look-ups of a
        level that read the same input share one keyswitch and blind rotation (executor.py, shared_rotation.py) - evaluate and
        evaluate_many alike; the error budget and the p_error selection then count the larger noise of such look-ups;
        centred_modswitch (2^64 torus and 49-bit field): the centred modulus switch (bmi_set_modswitch(ctx, 1): the rounding
        variance of a look-up (1 + n/4) / 12 instead of (1 + hw(s)) / 12 positions^2; 6.2 -> 8.8 sigma for a 4-bit look-up of the
        default set) - set on the engine this object creates AND on an engine passed in (whose mode this changes); the p_error
        selection and `self.error_budget` price it.  Works with unroll, share_rotations, evaluate_many and several ranks (every
        rank's engine must be in the same mode: executor.py); compress_outputs (2^64 torus, one rank; True = 16 bits, or a
        log_modulus in [2, 32]): keygen also makes the compression key (levels 1, base 2^16), evaluate / evaluate_many return
        tfhe.CompressedCiphertexts - the outputs packed into GLWE ciphertexts and cut to log_modulus bits per word, about 4 bytes
        per output instead of (N + 1) * 8 - and decrypt takes either form; the error budget and the p_error selection add
        error_budget.compression_variance to every output.  Under torch.distributed: NotImplementedError; client=True: the
        client's role on a machine without a GPU - this object creates a client.ClientEngine (libbmi_client.so) with the parameter
        choice above (params, q_bits, p_error, unroll, centred_modswitch - recorded for the error budget, the server switches -,
        compress_outputs) and the same error budget; keygen, save_keys (the seeded evaluation keys a server loads), quantize,
        encrypt, decrypt, dequantize, simulate and failure_budget work; evaluate, evaluate_many, run(simulate=False) and run_many
        raise: they are a server-side object's, built with engine= a tfhe.Engine after Engine.load_keys of the client's file."""
        self.shape = (n, n)
        self.qfloat_base, self.qfloat_len, self.qfloat_ints = qfloat_base, qfloat_len, qfloat_ints
        self.true_division, self.tensorize = true_division, tensorize
        # The reference calls sampler() 100 times to let Concrete measure value ranges (main.py:41-47);
        # here ranges are derived by interval analysis, so the sampler is only validated.
        if sampler is not None:
            s = sampler()
            assert isinstance(s, np.ndarray) and np.issubdtype(s.dtype, np.floating) and s.shape == self.shape
        t0 = time.time()
        self.program, self.compile_info = compile_inverse(n, qfloat_len, qfloat_ints, qfloat_base, true_division,
                                                          tensorize, cache=cache)
        self.circuit = self.program      # what the reference calls the compiled circuit
        self.msg_bits = self.program.msg_bits
        self.trace_seconds = time.time() - t0
        self.engine = engine
        self.device = device
        self.shard_threshold = shard_threshold
        self.unroll = bool(unroll)
        self.q_bits = q_bits
        self.params = params
        self.p_error = p_error
        self.share_rotations = bool(share_rotations)
        self.centred_modswitch = bool(centred_modswitch)
        # 0 = outputs come home as full ciphertexts, else the log_modulus they are compressed to
        self.compress_log_modulus = 16 if compress_outputs is True else int(compress_outputs or 0)
        if self.compress_log_modulus and not 2 <= self.compress_log_modulus <= 32:
            raise ValueError("compress_outputs: True (16 bits) or a log_modulus in [2, 32]")
        if self.compress_log_modulus and self._dist() is not None:
            raise NotImplementedError("compress_outputs is a one-rank option: under torch.distributed the outputs come home as full "
                                      "ciphertexts")
        self.error_budget = None      # filled when the engine exists: Program.failure_probability under its parameters
        if engine is not None and params is not None:
            raise ValueError("pass an engine or a parameter set, not both (the engine already has its parameters)")
        if engine is not None and q_bits is not None and engine.q_bits != q_bits:
            raise ValueError(f"q_bits={q_bits} but the engine passed in computes on q_bits={engine.q_bits}")
        if self.unroll and engine is not None and getattr(engine, "unroll", 1) != 2:
            raise ValueError("unroll=True with an engine that is not in unrolled mode: call engine.set_bsk_unroll(2) before its "
                             "keygen, or let this object create the engine")
        self.client = bool(client)
        if self.client and engine is not None:
            raise ValueError("client=True creates its own ClientEngine: pass client=True or an engine, not both")
        self._exec = None

    def _server_only(self, what):
        if self.client:
            raise RuntimeError(f"{what} needs a GPU: this object was built with client=True (keys, encryption and decryption on "
                               "the host).  Evaluate on a server-side EncryptedMatrixInversion built with engine= a tfhe.Engine "
                               "after Engine.load_keys of the file this client's save_keys wrote")

    # ---- key generation / engine -------------------------------------------------------------------
    def _engine(self):
        if self.engine is None:
            from . import tfhe  # tfhe.Engine raises BmiError when libbmi_tfhe.so or the GPU is missing: no CPU fallback (client=True: client.py)
            # 4-bit look-ups: the north-star set (N = 1024); 5-bit ones (bases other than 2): N = 2048, same margin
            qb = self.q_bits
            if self.params is not None:    # a named set of the library, or a tfhe.Params
                params = tfhe.preset_params(self.params) if isinstance(self.params, str) else self.params
            elif self.p_error is not None:  # the first set of this modulus whose error budget for this circuit meets p_error
                from . import error_budget
                params, self.error_budget = error_budget.choose_params(self.program, self.p_error, q_bits=qb, unroll=self.unroll,
                                                                           share_rotations=self.share_rotations,
                                                                           centred_modswitch=self.centred_modswitch,
                                                                           compressed_outputs=self._compressed_outputs())
            elif self.msg_bits <= 4:
                params = tfhe.default_params(q_bits=qb)
            elif self.msg_bits <= 6 and qb in (None, tfhe.TORUS64, 49):
                # 5-bit look-ups: N = 2048, 6-bit ones: N = 4096 - one more message bit per doubling of N at the same margin; on the
                # library's default modulus (the 2^64 torus: k_blind_rotate_w_t64f / k_blind_rotate_q_t64f) unless q_bits says 49
                params = tfhe.default_params(log_N=self.msg_bits + 6, **({} if qb is None else dict(q_bits=qb)))
            else:
                raise ValueError("look-ups wider than 4 bits need N >= 2048, which exists on the 2^64 torus and the 49-bit field; "
                                 "wider than 6 bits: no parameter set")
            if self.unroll:
                # (the 2^64 torus also at N = 2048, e.g. secure128_torus: k_blind_rotate_wu_t64f on the key at 40 bits)
                wide_torus = params.log_N == 11 and params.q_bits == tfhe.TORUS64
                if self.msg_bits > 4 or (params.log_N != 10 and not wide_torus):
                    raise ValueError("bootstrap-key unrolling exists at N = 1024 and, on the 2^64 torus, at N = 2048 (4-bit look-ups) only")
                if params.q_bits == 49 and self.params is None:     # three products per step: key noise 2^-41 keeps the default set's output noise
                    params = tfhe.default_params(q_bits=49, glwe_noise=2.0 ** -41)
                elif params.q_bits != tfhe.TORUS64:
                    raise ValueError("bootstrap-key unrolling exists on the 49-bit field and on the 2^64 torus")
            if self.client:
                from .client import ClientEngine
                self.engine = ClientEngine(params)
            else:
                self.engine = tfhe.Engine(params, device=self.device)
            if self.unroll:
                self.engine.set_bsk_unroll(2)
        if self.centred_modswitch and self.engine.modswitch != 1:
            self.engine.set_modswitch(1)
        if self.engine.P.N < (1 << (self.msg_bits + 6)):
            raise ValueError(f"{self.msg_bits}-bit look-ups need a parameter set with N >= {1 << (self.msg_bits + 6)} "
                             f"(this engine has N = {self.engine.P.N})")
        if self.error_budget is None:
            from . import error_budget
            self.error_budget = error_budget.engine_failure_probability(self.program, self.engine, share_rotations=self.share_rotations,
                                                                        compressed_outputs=self._compressed_outputs())
            if self.p_error is not None and self.error_budget["p_fail"] > self.p_error:
                raise ValueError(f"this circuit's failure probability under the engine's parameters is {self.error_budget['p_fail']:.2e} "
                                 f"> p_error = {self.p_error:g}: pass a wider parameter set (e.g. log_N=11) or let this object choose")
        return self.engine

    COMPRESSION_SHAPE = (1, 16)      # (levels, base_log) of the compression key keygen makes

    def _compressed_outputs(self):
        """the error budget's `compressed_outputs` argument: (levels, base_log, log_modulus), or None"""
        return self.COMPRESSION_SHAPE + (self.compress_log_modulus,) if self.compress_log_modulus else None

    def keygen(self, seed=None):
        """circuit.keygen() (main.py:177).  seed=None: CSPRNG keys; an integer: the test-only deterministic key set.
        With torch.distributed initialised on several ranks (the sharded executor) rank 0 generates the set and the others
        receive its evaluation keys (Engine.keygen_shared): independent CSPRNG keys per rank would make the ranks' parts of a
        level undecryptable garbage to each other.  Only rank 0 can then encrypt / decrypt."""
        eng = self._engine()
        try:
            import torch.distributed as dist
            shared = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        except Exception:
            shared = False
        if shared:
            if self.compress_log_modulus:
                raise NotImplementedError("compress_outputs is a one-rank option: under torch.distributed the outputs come home as "
                                          "full ciphertexts")
            eng.keygen_shared(seed)
        else:
            eng.keygen(seed)
            if self.compress_log_modulus:
                eng.compression_keygen(*self.COMPRESSION_SHAPE)

    def save_keys(self, path):
        """the evaluation keys a server needs, in seeded form (Engine.save_keys(path, secret=False, seeded=True): 0.3 of the full
        file), with the compression key when compress_outputs is set; CSPRNG keys on the 2^64 torus (keygen() without a seed)"""
        self._engine().save_keys(path, secret=False, seeded=True)

    def failure_budget(self, input_variance=None):
        """this instance's error budget (error_budget.engine_failure_probability under its engine, rotation sharing and output
        compression) for inputs of the given variance in torus^2 - a scalar or one value per input; None: fresh encryptions, the
        dict `error_budget` holds.  For compressed inputs pass error_budget.decompressed_variance(...)."""
        from . import error_budget
        return error_budget.engine_failure_probability(self.program, self._engine(), share_rotations=self.share_rotations,
                                                       compressed_outputs=self._compressed_outputs(), input_variance=input_variance)

    def _executor(self, batch=1):
        """the executor of this circuit for `batch` input matrices per run (one per batch size, built on first use)"""
        self._server_only("evaluation")
        if self._exec is None:
            self._exec = {}
        if batch not in self._exec:
            from .executor import Executor
            self._exec[batch] = Executor(self.circuit, self._engine(), shard_threshold=self.shard_threshold, batch=batch,
                                         share_rotations=self.share_rotations)
        return self._exec[batch]

    # ---- the reference's six methods -----------------------------------------------------------------
    def quantize(self, matrix: np.ndarray):
        return float_matrix_to_qfloat_arrays(matrix, self.qfloat_len, self.qfloat_ints, self.qfloat_base)

    def _flat_inputs(self, quantized_matrix, qfloats_signs):
        q = np.asarray(quantized_matrix, dtype=np.int64)
        s = np.asarray(qfloats_signs, dtype=np.int64)
        n2 = self.shape[0] * self.shape[1]
        if q.shape != (n2, self.qfloat_len) or s.shape != (n2,):
            raise ValueError("quantized matrix / signs have the wrong shape")
        flat = np.concatenate([q.reshape(-1), s])
        c = self.circuit
        for i, v in enumerate(flat):
            if not (c.leaf_lo[i] <= v <= c.leaf_hi[i]):
                raise ValueError(f"input {i} = {v} outside the interval [{c.leaf_lo[i]}, {c.leaf_hi[i]}] the circuit "
                                 "was traced for (matrix entry too large for qfloat_ints?)")
        return flat

    def encrypt(self, quantized_matrix: np.ndarray, qfloats_signs: np.ndarray, seeded=False):
        """seeded=True (2^64 torus, CSPRNG keys): tfhe.SeededCiphertexts - 8 bytes per input instead of (N + 1) * 8; evaluate and
        evaluate_many of a server that loaded this client's seeded keys (Engine.import_keys_seeded / load_keys) take them"""
        flat = self._flat_inputs(quantized_matrix, qfloats_signs)
        eng = self._engine()
        return (eng.encrypt_seeded if seeded else eng.encrypt)(flat, eng.delta_log(self.msg_bits))

    def _expanded(self, enc):
        """an input of evaluate: seeded ciphertexts are expanded on the GPU, full ones pass as they are"""
        from .tfhe import SeededCiphertexts
        self._server_only("evaluation")
        return self._engine().expand_seeded(enc) if isinstance(enc, SeededCiphertexts) else enc

    def evaluate(self, encrypted_quantized_matrix) -> np.ndarray:
        """the encrypted inverse: (outputs, words) ciphertexts, or with compress_outputs a tfhe.CompressedCiphertexts.  The input
        is what encrypt() returned (full or seeded), or a tfhe.CompressedCiphertexts of the circuit's inputs in order
        (Engine.compress_host of them, or an earlier circuit's compressed result): its values alone go to the GPU, which
        decompresses them into the executor's input rows.  Such inputs are no fresh encryptions: failure_budget() prices them."""
        self._server_only("evaluate")
        if self.compress_log_modulus:
            return self._executor().run_compressed(self._expanded(encrypted_quantized_matrix), self.compress_log_modulus)
        return self._executor().run(self._expanded(encrypted_quantized_matrix))

    def evaluate_many(self, encrypted_quantized_matrices) -> np.ndarray:
        """B encrypted matrices (a sequence of encrypt() results, or one (B, inputs, words) array) through the circuit in ONE walk of
        its levels: every level is B times wider, so the look-ups run on the throughput kernel instead of B x depth rounds of the
        latency kernel (executor.py, `batch`) - the serving form.  Returns (B, outputs, words); decrypt() each.  With
        compress_outputs: a list of B tfhe.CompressedCiphertexts, every matrix in blocks of its own.  B tfhe.CompressedCiphertexts
        (a list or tuple of them) are decompressed on the GPU as in evaluate(); mixed with other forms they are refused."""
        from .tfhe import CompressedCiphertexts
        self._server_only("evaluate_many")
        seq = encrypted_quantized_matrices
        if isinstance(seq, (list, tuple)) and any(isinstance(e, CompressedCiphertexts) for e in seq):
            if not all(isinstance(e, CompressedCiphertexts) for e in seq):
                raise ValueError("evaluate_many: compressed inputs mixed with full or seeded ones: pass one form (Engine.decompress_host "
                                 "turns a CompressedCiphertexts into full ciphertexts)")
            ex = self._executor(len(seq))
            if self.compress_log_modulus:
                res = ex.run_compressed(list(seq), self.compress_log_modulus)
                return res if isinstance(res, list) else [res]
            return ex.run(list(seq)).reshape(len(seq), -1, self._engine().P.big)
        enc = np.ascontiguousarray(np.stack([np.asarray(self._expanded(e)) for e in encrypted_quantized_matrices]), dtype=np.uint64)
        if enc.ndim != 3:
            raise ValueError("expected B encrypted matrices of shape (inputs, words)")
        if self.compress_log_modulus:
            res = self._executor(enc.shape[0]).run_compressed(enc, self.compress_log_modulus)
            return res if isinstance(res, list) else [res]
        return self._executor(enc.shape[0]).run(enc).reshape(enc.shape[0], -1, enc.shape[2])

    def run_many(self, matrices, validate=True):
        """run() for a batch of matrices on one GPU: quantize, encrypt, ONE batched encrypted evaluation (evaluate_many), decrypt,
        dequantize - the same inverses as run() matrix by matrix"""
        self._server_only("run_many")
        if self._dist() is not None:
            raise NotImplementedError("run_many is the one-GPU serving form; under torch.distributed call run() per matrix")
        qs = []
        for m in matrices:
            assert np.issubdtype(m.dtype, np.floating) and m.shape == self.shape
            q = self.quantize(m)
            if validate:
                self.simulate(*q)
            qs.append(q)
        res = self.evaluate_many([self.encrypt(q, s_) for q, s_ in qs])
        return [self.dequantize(self.decrypt(r)) for r in res]

    def decrypt(self, encrypted_quantized_inverted_matrix: np.ndarray) -> np.ndarray:
        n2 = self.shape[0] * self.shape[1]
        eng = self._engine()
        from .tfhe import CompressedCiphertexts
        if isinstance(encrypted_quantized_inverted_matrix, CompressedCiphertexts):
            m = eng.decrypt_compressed(encrypted_quantized_inverted_matrix, eng.delta_log(self.msg_bits))
        else:
            m = eng.decrypt(encrypted_quantized_inverted_matrix, eng.delta_log(self.msg_bits))
        return m.reshape(n2, self.qfloat_len + 1)

    def dequantize(self, quantized_inverted_matrix: np.ndarray) -> np.ndarray:
        return qfloat_and_signs_arrays_to_float_matrix(quantized_inverted_matrix, self.qfloat_ints, self.qfloat_base)

    def simulate(self, quantized_matrix, qfloats_signs) -> np.ndarray:
        n2 = self.shape[0] * self.shape[1]
        flat = self._flat_inputs(quantized_matrix, qfloats_signs)
        return np.array(self.circuit.simulate(flat), dtype=np.int64).reshape(n2, self.qfloat_len + 1)

    @staticmethod
    def _dist():
        """torch.distributed when it is initialised on more than one rank, else None"""
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                return dist
        except Exception:
            pass
        return None

    def _broadcast(self, dist, arr, src=0):
        """a numpy array from rank `src` to every rank (through the GPU when the backend is RCCL)"""
        import torch
        a = np.ascontiguousarray(arr)
        t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a)
        on_gpu = dist.get_backend() == "nccl"
        if on_gpu:
            t = t.to(torch.device("cuda", self._engine().device))
        dist.broadcast(t, src=src)
        out = t.cpu().numpy() if on_gpu else t.numpy()
        return out.view(a.dtype)

    def run(self, matrix: np.ndarray, simulate=False, validate=True) -> np.ndarray:
        """The reference's one-call form (main.py:93-116).  validate (encrypted runs): the caller of run() holds the
        plaintext, so the compiled program is first evaluated in plaintext with every interval claim checked
        (program.Program.simulate: 0.07 s for 3x3, 2 s for 8x8) - an input the circuit was not traced for (a singular
        matrix whose reciprocal overflows its format, an entry beyond the leading-digit range) raises RangeError here
        instead of decrypting to garbage silently, which is what an encrypted evaluation outside its ranges does (on
        Concrete as well: its circuits are only defined on the ranges their inputset showed).  With torch.distributed
        initialised on several ranks every rank calls run() with the same matrix: rank 0 (the holder of the secret keys after
        keygen()) encrypts and decrypts, ciphertexts and result are broadcast, every rank returns the same inverse."""
        assert np.issubdtype(matrix.dtype, np.floating)
        assert matrix.shape == self.shape
        quantized_matrix, qfloats_signs = self.quantize(matrix)
        if not simulate:
            self._server_only("run(simulate=False)")
            if validate:
                self.simulate(quantized_matrix, qfloats_signs)
            dist = self._dist()
            if dist is None:
                enc = self.encrypt(quantized_matrix, qfloats_signs)
                enc_inv = self.evaluate(enc)
                quantized_inverted_matrix = self.decrypt(enc_inv)
            else:
                # several ranks (the sharded executor): keygen() left the secret keys on rank 0 only, so rank 0 encrypts and
                # decrypts and the ciphertexts / the result travel by broadcast; every rank walks the levels and returns the
                # same matrix
                eng = self._engine()
                n_ct = self.circuit.n_inputs
                enc = (self.encrypt(quantized_matrix, qfloats_signs) if dist.get_rank() == 0
                       else np.zeros((n_ct, eng.P.big), np.uint64))
                enc = self._broadcast(dist, enc)
                enc_inv = self.evaluate(enc)
                n2 = self.shape[0] * self.shape[1]
                quantized_inverted_matrix = (self.decrypt(enc_inv) if dist.get_rank() == 0
                                             else np.zeros((n2, self.qfloat_len + 1), np.int64))
                quantized_inverted_matrix = self._broadcast(dist, quantized_inverted_matrix)
        else:
            quantized_inverted_matrix = self.simulate(quantized_matrix, qfloats_signs)
        inverted_matrix = self.dequantize(quantized_inverted_matrix)
        assert np.issubdtype(inverted_matrix.dtype, np.floating)
        assert inverted_matrix.shape == self.shape
        return inverted_matrix
