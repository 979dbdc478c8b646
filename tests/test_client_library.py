"""libbmi_client.so and bmi_amd.client.ClientEngine: the client half without a GPU (include/bmi_client.h).  Nothing here needs a
device.  Every comparison is word for word: against the oracle, against the digests recorded from libbmi_tfhe.so on an MI355X
(tests/golden/host_crypto_digests.json), against the seeded format's stream, and against the numpy statement of the compression
(tests/compress_cases.py).  The only bound is the noise bound tests/c_abi/host_crypto_check.cpp derives: Box-Muller on a 53-bit uniform
cannot exceed 8.57 standard deviations and the rounding adds at most 1/2, so |noise| <= 8.6 sigma q + 1."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import compress_cases as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "bounty-matrix-inversion_amd")
LIB = os.path.join(PKG, "lib", "libbmi_client.so")
SEED = 0x5EED
U = np.uint64

# what include/bmi_client.h lists
EXPORTS = """bmi_default_params bmi_default_params_for bmi_preset_params bmi_get_params
bmi_ctx_create bmi_ctx_destroy bmi_last_error
bmi_set_bsk_precision bmi_get_bsk_precision bmi_set_bsk_unroll
bmi_keygen bmi_keygen_insecure_deterministic bmi_keygen_from_secret bmi_export_keys bmi_import_keys bmi_export_bsk_unrolled
bmi_import_bsk_unrolled bmi_export_keys_seeded bmi_export_bsk_unrolled_seeded bmi_compression_keygen bmi_compression_key_info
bmi_export_compression_key bmi_import_compression_key bmi_export_compression_key_seeded
bmi_encrypt bmi_encrypt_seeded bmi_decrypt bmi_phase bmi_phase_compressed bmi_decrypt_compressed bmi_compressed_words
bmi_seeded_mask_words bmi_torus64_to_field bmi_field_to_torus64
bmi_circuit_prune bmi_circuit_schedule""".split()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).data).hexdigest()


def params_of(name):
    from bmi_amd import client
    if name == "secure128_torus":
        return client.preset_params(name)
    return client.default_params(q_bits={"torus64": 65, "field49": 49, "goldilocks": 64}[name])


# ------------------------------------------------------------------------------------------------ 1. the library file
def test_dynamic_section_and_exports():
    needed = subprocess.run(["readelf", "-d", LIB], check=True, capture_output=True, text=True).stdout
    assert "NEEDED" in needed
    for word in ("amdhip", "hsa", "bmi_tfhe"):
        assert word not in needed, needed
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    got = sorted(line.split()[-1] for line in nm.splitlines() if line.strip())
    assert got == sorted(EXPORTS)


# ------------------------------------------------------------------------------------------------ 2. a clean process
CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
from bmi_amd.client import ClientEngine
e = ClientEngine()
e.keygen(0x5EED)
m = np.arange(-4, 4)
ct = e.encrypt(m, e.delta_log())
assert ct.shape == (8, e.P.big) and list(e.decrypt(ct, e.delta_log())) == list(m)
e.close()
assert "torch" not in sys.modules, "torch was imported"
maps = open("/proc/self/maps").read()
assert "libbmi_client" in maps
for word in ("libamdhip64", "libbmi_tfhe"):
    assert word not in maps, word + " is mapped"
print("clean")
"""


def test_a_whole_cycle_loads_no_torch_and_no_hip():
    out = subprocess.run([sys.executable, "-c", CHILD % (REPO, PKG)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "clean", out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------ 3. the oracle
@pytest.mark.parametrize("name", ["torus64", "field49", "goldilocks", "secure128_torus"])
def test_deterministic_words_are_the_oracles(name):
    from bmi_amd import client, tfhe
    from oracle import tfhe_oracle as to
    P = params_of(name)
    to.set_field(P.q_bits)
    oP = to.Params(**{f: getattr(P, f) for f, _ in tfhe.Params._fields_})
    ora = to.keygen(oP, SEED)
    e = client.ClientEngine(P)
    try:
        prec = e.bsk_precision
        assert prec == to.default_bsk_precision(oP)
        e.keygen(SEED)
        sk_small, sk_big, bsk, ksk = e.export_keys()
        assert np.array_equal(sk_small, ora.sk_small) and np.array_equal(sk_big, ora.sk_big)
        assert np.array_equal(ksk, ora.ksk)
        assert np.array_equal(bsk, to.round_key(ora.bsk, prec) if P.q_bits == tfhe.TORUS64 else ora.bsk)
        dl = e.delta_log()
        msgs = np.arange(-4, 4)
        ct = e.encrypt(msgs, dl)
        assert np.array_equal(ct, to.lwe_encrypt(ora.sk_big, P.glwe_noise, SEED, 0, to.encode(msgs, dl)))
        ct2 = e.encrypt(msgs[::-1], dl)     # encryption i of a key set: the counter goes on
        assert np.array_equal(ct2, to.lwe_encrypt(ora.sk_big, P.glwe_noise, SEED, 8, to.encode(msgs[::-1], dl)))
        assert np.array_equal(e.phase(ct), to.lwe_phase(ora.sk_big, ct))
        assert np.array_equal(e.decrypt(ct, dl), to.decode(to.lwe_phase(ora.sk_big, ct), dl))
        assert list(e.decrypt(ct2, dl)) == list(msgs[::-1])
    finally:
        e.close()
    # the unrolled key: the mode set before keygen decides the precision both keys are rounded to
    u = client.ClientEngine(P)
    try:
        if P.q_bits == 64:
            with pytest.raises(tfhe.BmiError, match="49-bit field and the 2\\^64 torus"):
                u.set_bsk_unroll(2)
            return
        u.set_bsk_unroll(2)
        prec = u.bsk_precision
        assert prec == ({10: 42, 11: 40}[P.log_N] if P.q_bits == tfhe.TORUS64 else 64)
        u.keygen(SEED)
        rounded = (lambda k: to.round_key(k, prec)) if P.q_bits == tfhe.TORUS64 else (lambda k: k)
        assert np.array_equal(u.export_keys()[2], rounded(ora.bsk))
        assert np.array_equal(u.export_bsk_unrolled(), rounded(to.keygen_bsk_unrolled(oP, SEED, ora.sk_small, ora.sk_big)))
    finally:
        u.close()


# ------------------------------------------------------------------------------------------------ 4. the device library's digests
def client_digests(q_bits):
    """tests/test_gpu_host_crypto_digests.py::digests on a ClientEngine, without the two entries that need a server import"""
    from bmi_amd import client, tfhe
    e = client.ClientEngine(client.default_params(q_bits=q_bits))
    try:
        e.keygen(SEED)
        sk_small, sk_big, bsk, ksk = e.export_keys()
        d = {"sk_small": sha(sk_small), "sk_big": sha(sk_big), "bsk": sha(bsk), "ksk": sha(ksk)}
        d["encryptions"] = sha(e.encrypt(np.arange(-4, 4), e.delta_log()))
        if q_bits == tfhe.TORUS64:
            e.compression_keygen(1, 16)
            d["compression_key"] = sha(e.export_compression_key())
        if q_bits != 64:
            e.set_bsk_unroll(2)
            d["bsk3"] = sha(e.export_bsk_unrolled())
        return d
    finally:
        e.close()


@pytest.mark.parametrize("modulus", ["field49", "goldilocks", "torus64"])
def test_words_are_the_ones_recorded_from_the_device_library(modulus):
    want = json.load(open(os.path.join(REPO, "tests", "golden", "host_crypto_digests.json")))[modulus]
    want = {k: v for k, v in want.items() if not k.startswith("seeded_")}     # (a server's import: tests/test_gpu_client_library.py)
    got = client_digests({"torus64": 65, "field49": 49, "goldilocks": 64}[modulus])
    assert sorted(got) == sorted(want)
    assert got == want, [k for k in want if got[k] != want[k]]


# ------------------------------------------------------------------------------------------------ 5. the seeded forms
@pytest.fixture(scope="module")
def csprng_client():
    """a torus client in unrolled mode with CSPRNG keys and the (1, 16) compression key, and its exports (read only)"""
    from bmi_amd import client
    e = client.ClientEngine()
    e.set_bsk_unroll(2)
    e.keygen()
    e.compression_keygen(1, 16)
    keys = e.export_keys()
    yield e, keys
    e.close()


def stream_rows(lib_words, pub, domain, rows, width):
    return np.stack([lib_words(pub, (domain << 56) | r, 0, width) for r in range(rows)])


def within_noise(err_words, sigma):
    """|centred error| <= 8.6 sigma 2^64 + 1 (tests/c_abi/host_crypto_check.cpp is_noise)"""
    return bool(np.all(np.abs(np.asarray(err_words, dtype=U).view(np.int64).astype(np.float64)) <= 8.6 * sigma * 2.0 ** 64 + 1.0))


def ggsw_errors(full, msg_bits, S, levels, base_log):
    """the errors of GGSW rows [count][2 l][2][N] (k = 1) of the bits msg_bits under the GLWE key S: phase B - A S minus the message -
    component 0: -bit g S(X), component 1: bit g X^0, g = 2^(64 - base_log (level + 1))"""
    count, N = full.shape[0], S.size
    flat = full.reshape(count * 2 * levels, 2, N)
    with np.errstate(over="ignore"):
        ph = flat[:, 1] - cc.rows_by_binary(flat[:, 0], S)
        ph = ph.reshape(count, 2, levels, N)
        for lev in range(levels):
            g = U(1 << (64 - base_log * (lev + 1)))
            ph[:, 0, lev, :] += (np.asarray(msg_bits, dtype=U)[:, None] * g) * S.astype(U)[None, :]
            ph[:, 1, lev, 0] -= np.asarray(msg_bits, dtype=U) * g
    return ph


def test_seeded_exports_are_stream_masks_plus_bodies(csprng_client):
    from bmi_amd import tfhe
    from bmi_amd.client import load_client_library
    import ctypes as C
    e, (sk_small, sk_big, bsk, ksk) = csprng_client
    P, lib = e.P, load_client_library()
    N, n, l, b = P.N, P.n, P.bs_levels, P.bs_base_log

    def words(pub, nonce, first, count):
        out = np.zeros(count, U)
        assert lib.bmi_seeded_mask_words(tfhe._ptr(pub), C.c_uint64(nonce), C.c_uint64(first), C.c_uint64(count), tfhe._ptr(out)) == 0
        return out
    pub, bsk_body, ksk_body = e.export_keys_seeded()
    # masks at the nonces of include/bmi_tfhe.h, bodies behind them
    full_bsk = np.concatenate([stream_rows(words, pub, tfhe.SEED_DOMAIN_BSK_MASK, n * 2 * l, N).reshape(n, 2 * l, 1, N),
                               bsk_body[:, :, None, :]], axis=2)
    full_ksk = np.concatenate([stream_rows(words, pub, tfhe.SEED_DOMAIN_KSK_MASK, N * P.ks_levels, n).reshape(N, P.ks_levels, n),
                               ksk_body[:, :, None]], axis=2)
    prec = e.bsk_precision
    assert prec == 42
    from oracle import tfhe_oracle as to
    assert np.array_equal(to.round_key(full_bsk, prec), bsk)        # the server rounds the expanded key as the client did
    assert np.array_equal(full_ksk, ksk)
    # ... and they decrypt to the messages: the bits of sk_small (GGSW), sk_big[j] 2^(64 - b (lev + 1)) (keyswitch key)
    assert within_noise(ggsw_errors(full_bsk, sk_small, sk_big, l, b), P.glwe_noise)
    with np.errstate(over="ignore"):
        ph = full_ksk[:, :, n] - (full_ksk[:, :, :n] * sk_small.astype(U)[None, None, :]).sum(axis=2, dtype=U)
        for lev in range(P.ks_levels):
            ph[:, lev] -= sk_big.astype(U) << U(64 - P.ks_base_log * (lev + 1))
    assert within_noise(ph, P.lwe_noise)
    # the unrolled key and the compression key the same way
    body3 = e.export_bsk_unrolled_seeded()
    pairs = (n + 1) // 2
    full3 = np.concatenate([stream_rows(words, pub, tfhe.SEED_DOMAIN_BSK3_MASK, pairs * 3 * 2 * l, N).reshape(pairs, 3, 2 * l, 1, N),
                            body3[:, :, :, None, :]], axis=3)
    assert np.array_equal(to.round_key(full3, prec), e.export_bsk_unrolled())
    s1, s2 = sk_small[0::2], np.append(sk_small[1::2], np.zeros(pairs - n // 2, U))
    msg3 = np.stack([s1 & s2, s1 & (s2 ^ U(1)), (s1 ^ U(1)) & s2], axis=1).reshape(-1)
    assert within_noise(ggsw_errors(full3.reshape(pairs * 3, 2 * l, 2, N), msg3, sk_big, l, b), P.glwe_noise)
    pk_body = e.export_compression_key_seeded()
    full_pk = np.concatenate([stream_rows(words, pub, tfhe.SEED_DOMAIN_PKSK_MASK, N, N).reshape(N, 1, 1, N), pk_body[:, :, None, :]], axis=2)
    assert np.array_equal(full_pk, e.export_compression_key())
    assert within_noise(cc.key_row_errors(full_pk, sk_big, 16), P.glwe_noise)
    # seeded encryptions: bodies plus the stream masks are encrypt() at the same counter
    msgs = np.arange(-8, 8)
    dl = e.delta_log()
    seeded = e.encrypt_seeded(msgs, dl)
    assert isinstance(seeded, tfhe.SeededCiphertexts) and len(seeded) == 16
    full = np.concatenate([np.stack([words(pub, (tfhe.SEED_DOMAIN_ENC_MASK << 56) | (seeded.first_counter + i), 0, N) for i in range(16)]),
                           seeded.bodies[:, None]], axis=1)
    assert list(e.decrypt(full, dl)) == list(msgs)
    again = e.encrypt(msgs, dl)                       # counters first + 16 ..: other masks, the same rule
    assert np.array_equal(again[:, :N], np.stack([words(pub, (tfhe.SEED_DOMAIN_ENC_MASK << 56) | (seeded.first_counter + 16 + i), 0, N)
                                                  for i in range(16)]))
    err = (e.phase(full) - (msgs.astype(np.int64).view(U) << U(dl)))
    assert within_noise(err, P.glwe_noise)


def test_seeded_forms_stay_refused_where_the_device_library_refuses():
    from bmi_amd import client, tfhe
    for q_bits in (49, 64):
        e = client.ClientEngine(client.default_params(q_bits=q_bits, n=16))
        try:
            e.keygen()
            with pytest.raises(tfhe.BmiError, match="seeded forms exist on the 2\\^64 torus only"):
                e.export_keys_seeded()
            with pytest.raises(tfhe.BmiError, match="seeded forms exist on the 2\\^64 torus only"):
                e.encrypt_seeded([1], e.delta_log())
        finally:
            e.close()
    e = client.ClientEngine(client.default_params(n=16))
    try:
        e.keygen(SEED)
        with pytest.raises(tfhe.BmiError, match="deterministic test keys"):
            e.export_keys_seeded()
        with pytest.raises(tfhe.BmiError, match="libbmi_tfhe.so"):
            e.import_keys(None, None, *e.export_keys()[2:])
        with pytest.raises(tfhe.BmiError, match="a server's"):
            e.pbs_host(None, None)
    finally:
        e.close()
    with pytest.raises(tfhe.BmiError, match="log_N must be 10"):
        client.ClientEngine(client.default_params(log_N=9))


# ------------------------------------------------------------------------------------------------ 6. compressed results
@pytest.mark.parametrize("count, log_modulus", [(5, 16), (5, 32), (1024, 16), (1024, 32)])
def test_compressed_results_decrypt(csprng_client, count, log_modulus):
    from bmi_amd import tfhe
    e, (_, sk_big, _, _) = csprng_client
    N, dl = e.P.N, e.delta_log()
    msgs = np.random.default_rng(count + log_modulus).integers(-8, 8, count)
    cts = e.encrypt(msgs, dl)
    words = cc.compress(cts, e.export_compression_key(), 1, 16, log_modulus)
    packed = tfhe.CompressedCiphertexts(count, N, log_modulus, words)
    assert e.compressed_words(count) == words.size
    assert np.array_equal(e.phase_compressed(packed), cc.phase(words, count, N, log_modulus, sk_big))
    assert list(e.decrypt_compressed(packed, dl)) == list(msgs)
    assert list(e.decrypt_compressed(tfhe.CompressedCiphertexts.frombytes(packed.tobytes()), dl)) == list(msgs)


def test_a_second_compression_shape_is_refused(csprng_client):
    from bmi_amd import tfhe
    e, _ = csprng_client
    with pytest.raises(tfhe.BmiError, match=r"already has a compression key of shape \(1, 16\); a second one of another shape would "
                                            "reuse the rows' mask and noise streams"):
        e.compression_keygen(2, 16)
    assert e.compression_key_info() == (1, 16, 0)


# ------------------------------------------------------------------------------------------------ 7. key files
def file_layout(P, secret, seeded, unrolled, compression):
    """what Engine.save_keys writes: name -> (shape, dtype)"""
    n, N, rows, kl = P.n, P.N, 2 * P.bs_levels, P.ks_levels
    pairs = (n + 1) // 2
    u64, i64, f64 = np.dtype(np.uint64), np.dtype(np.int64), np.dtype(np.float64)
    if seeded:
        out = {"pub_key": ((8,), np.dtype(np.uint32)), "bsk_body": ((n, rows, N), u64), "ksk_body": ((N, kl), u64),
               "bsk_precision": ((1,), i64), "params": ((10,), f64)}
        if unrolled:
            out["bsk_unrolled_body"] = ((pairs, 3, rows, N), u64)
        if compression:
            out["compression_key_body"] = ((N, 1, N), u64)
    else:
        out = {"bsk": ((n, rows, 2, N), u64), "ksk": ((N, kl, n + 1), u64), "params": ((10,), f64)}
        if secret:
            out.update(sk_small=((n,), u64), sk_big=((N,), u64))
        if unrolled:
            out["bsk_unrolled"] = ((pairs, 3, rows, 2, N), u64)
        if compression:
            out["compression_key"] = ((N, 1, 2, N), u64)
    if compression:
        out["compression_shape"] = ((2,), i64)
    return out


@pytest.mark.parametrize("unrolled", [False, True])
def test_key_files_have_the_engines_layout_and_reload(tmp_path, unrolled):
    from bmi_amd import client, tfhe
    P = client.default_params(n=24)
    e = client.ClientEngine(P)
    try:
        if unrolled:
            e.set_bsk_unroll(2)
        e.keygen()
        e.compression_keygen(1, 16)
        for secret, seeded in ((True, False), (False, False), (False, True)):
            path = str(tmp_path / f"keys_{secret}_{seeded}.npz")
            e.save_keys(path, secret=secret, seeded=seeded)
            with np.load(path) as z:
                got = {k: (z[k].shape, z[k].dtype) for k in z.files}
                assert got == file_layout(P, secret, seeded, unrolled, True)
                assert list(z["params"]) == [float(getattr(P, f)) for f in tfhe.Engine._PARAM_FIELDS]
                if seeded:
                    assert int(z["bsk_precision"][0]) == e.bsk_precision == (42 if unrolled else 48)
                assert list(z["compression_shape"]) == [1, 16]
        with pytest.raises(tfhe.BmiError, match="evaluation keys only"):
            e.save_keys(str(tmp_path / "no.npz"), secret=True, seeded=True)
        # its own secret file restores a context whose exports are the same words
        r = client.ClientEngine(client.default_params(n=24))
        try:
            assert r.load_keys(str(tmp_path / "keys_True_False.npz")) is True
            for a, b in zip(r.export_keys(), e.export_keys()):
                assert np.array_equal(a, b)
            assert np.array_equal(r.export_compression_key(), e.export_compression_key())
            if unrolled:
                assert np.array_equal(r.export_bsk_unrolled(), e.export_bsk_unrolled())
            dl = e.delta_log()
            assert list(r.decrypt(e.encrypt(np.arange(-8, 8), dl), dl)) == list(range(-8, 8))
        finally:
            r.close()
        # a server's files are a server's
        for name, text in (("keys_False_True.npz", "a server's"), ("keys_False_False.npz", "libbmi_tfhe.so")):
            r = client.ClientEngine(client.default_params(n=24))
            try:
                with pytest.raises(tfhe.BmiError, match=text):
                    r.load_keys(str(tmp_path / name))
            finally:
                r.close()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 8. the circuit passes
def csr_of(circ):
    """the flat form Program.from_circuit hands the two passes"""
    def flatten(rows):
        ptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)
        leaf = np.array([t[0] for r in rows for t in r[0]], np.int32)
        return ptr, leaf
    node_ptr, term_leaf = flatten(circ.nodes)
    _, out_leaf = flatten(circ.outputs)
    return circ.n_inputs, node_ptr, term_leaf, out_leaf


@pytest.mark.parametrize("fmt", [(8, 4), (20, 8)])
def test_circuit_passes_are_the_device_librarys(fmt):
    import ctypes as C
    from bmi_amd import client, tfhe
    from bmi_amd.main import trace_inverse
    from bmi_amd.program import ROUND, WIDE_ROUND
    n_in, node_ptr, term_leaf, out_leaf = csr_of(trace_inverse(2, fmt[0], fmt[1], 2, False, False))

    def passes(lib):
        live = np.zeros(node_ptr.size - 1, np.uint8)
        assert lib.bmi_circuit_prune(n_in, live.size, tfhe._ptr(node_ptr), tfhe._ptr(term_leaf), tfhe._ptr(out_leaf), out_leaf.size,
                                     tfhe._ptr(live)) == 0
        level, depth = np.zeros(live.size, np.int32), C.c_int32(0)
        assert lib.bmi_circuit_schedule(n_in, level.size, tfhe._ptr(node_ptr), tfhe._ptr(term_leaf), ROUND, WIDE_ROUND, tfhe._ptr(level),
                                        C.byref(depth)) == 0
        return live, level, depth.value
    mine, theirs = passes(client.load_client_library()), passes(tfhe.load_library())
    assert mine[0].any() and mine[1].max() == mine[2] > 1
    assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1]) and mine[2] == theirs[2]
    bad = out_leaf.copy()
    bad[0] = n_in + node_ptr.size           # a leaf that does not exist
    assert client.load_client_library().bmi_circuit_prune(n_in, node_ptr.size - 1, tfhe._ptr(node_ptr), tfhe._ptr(term_leaf),
                                                          tfhe._ptr(bad), bad.size, tfhe._ptr(np.zeros(node_ptr.size - 1, np.uint8))) == -1


# ------------------------------------------------------------------------------------------------ 9. the client role
def test_client_role_of_the_application():
    from bmi_amd import client, tfhe
    from bmi_amd.main import EncryptedMatrixInversion
    app = EncryptedMatrixInversion(2, qfloat_len=20, qfloat_ints=8, client=True)
    app.keygen()
    assert isinstance(app.engine, client.ClientEngine) and 0.0 <= app.error_budget["p_fail"] < 1.0
    m = np.array([[1.5, -2.25], [0.75, 3.0]])
    q, s = app.quantize(m)
    flat = np.concatenate([q.reshape(-1), s])
    seeded = app.encrypt(q, s, seeded=True)
    assert isinstance(seeded, tfhe.SeededCiphertexts) and len(seeded) == flat.size
    full = app.encrypt(q, s)
    eng = app.engine
    assert list(eng.decrypt(full, eng.delta_log(app.msg_bits))) == list(flat)
    sim = app.simulate(q, s)
    assert np.allclose(app.dequantize(sim), np.linalg.inv(m), atol=1e-2)
    assert np.allclose(app.run(m, simulate=True), np.linalg.inv(m), atol=1e-2)
    assert app.failure_budget()["p_fail"] == app.error_budget["p_fail"]
    for call in (lambda: app.evaluate(full), lambda: app.evaluate(seeded), lambda: app.evaluate_many([full]), lambda: app.run(m),
                 lambda: app.run_many([m])):
        with pytest.raises(RuntimeError, match="client=True.*server-side EncryptedMatrixInversion built with engine= a tfhe.Engine "
                                               "after Engine.load_keys"):
            call()
    with pytest.raises(ValueError, match="client=True or an engine"):
        EncryptedMatrixInversion(2, qfloat_len=20, qfloat_ints=8, client=True, engine=eng)


def test_client_role_decrypts_full_outputs_and_writes_the_servers_file(tmp_path):
    from bmi_amd.main import EncryptedMatrixInversion
    app = EncryptedMatrixInversion(2, qfloat_len=20, qfloat_ints=8, client=True, compress_outputs=True)
    app.keygen()
    eng, n_out = app.engine, 4 * 21
    dl = eng.delta_log(app.msg_bits)
    digits = np.random.default_rng(5).integers(0, 2, n_out)
    assert np.array_equal(app.decrypt(eng.encrypt(digits, dl)), digits.reshape(4, 21))         # the full form of a result
    from bmi_amd import tfhe
    packed = tfhe.CompressedCiphertexts(n_out, eng.P.N, 16, cc.compress(eng.encrypt(digits, dl), eng.export_compression_key(), 1, 16, 16))
    assert np.array_equal(app.decrypt(packed), digits.reshape(4, 21))                          # ... and the compressed one
    path = str(tmp_path / "server.npz")
    app.save_keys(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(file_layout(eng.P, False, True, False, True))


# ------------------------------------------------------------------------------------------------ the sanitizers
@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_the_c_functions_under_the_sanitizers(tmp_path, sanitizer):
    """tests/c_abi/client_check.cpp with csrc/bmi_client.cpp, one program, run as a process of its own (nothing is loaded into Python)"""
    exe = str(tmp_path / "client_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-pthread", "-o", exe, os.path.join(REPO, "tests", "c_abi", "client_check.cpp"),
                           os.path.join(PKG, "csrc", "bmi_client.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert out.stdout.splitlines()[-1].endswith(" checks, 0 failed"), out.stdout[-4000:]
