"""Compression of output ciphertexts (include/bmi_tfhe.h, csrc/lwe_pack.hip) on the GPU: every compressed value equals the numpy
restatement's (tests/compress_cases.py) on uniformly random ciphertext and key words, compressed encryptions decrypt, the phase
error sits on error_budget.compression_variance, a server built from the seeded form holds the client's compression key word for
word, what cannot be served is refused with a text, and the encrypted inverse returns the same digits through compressed outputs.
Contexts are cut to n = 16 wherever the small key plays no part."""
import numpy as np
import pytest

import compress_cases as cc
import pbs_cases as pc
import seeded_cases as sc

pytestmark = pytest.mark.gpu

PKSK_DOMAIN = 11       # include/bmi_tfhe.h BMI_SEED_DOMAIN_PKSK_MASK (tests/seeded_cases.py's table predates it: the nonce is restated here)
SETS = {"default": lambda tfhe: tfhe.default_params(n=16),
        "secure128_torus": lambda tfhe: tfhe.preset_params("secure128_torus", n=16),
        "secure128_torus_wide": lambda tfhe: tfhe.preset_params("secure128_torus_wide", n=16)}
SPARSE_FROM = 1000     # counts from here on: rows zero outside 32 fixed mask positions (keeps the reference short)


def make_engine(name="default", seed=0x5EED):
    from bmi_amd import tfhe
    e = tfhe.Engine(SETS[name](tfhe))
    e.keygen(seed)
    return e


@pytest.fixture(scope="module")
def random_key_engines():
    """(set, levels, base_log) -> (engine, key): one context per parameter set, holding a compression key of uniformly random words
    of the shape asked for (exactness needs no valid key); shared by the cases that only compress"""
    engines, keys, held = {}, {}, {}

    def get(name, levels, base_log):
        if name not in engines:
            engines[name] = make_engine(name)
        e, shape = engines[name], (name, levels, base_log)
        if shape not in keys:
            keys[shape] = pc.uniform_words(np.random.default_rng(levels * 100 + base_log), (e.P.N, levels, 2, e.P.N))
        if held.get(name) != shape:
            e.import_compression_key(keys[shape], levels, base_log)
            held[name] = shape
        return e, keys[shape]
    yield get
    for e in engines.values():
        e.close()


def edge_rows(rng, count, N, levels, base_log):
    """`count` rows of uniformly random words, the first ones carrying the adversarial words and the ties of the decomposition"""
    cts = pc.uniform_words(rng, (count, N + 1))
    if count >= SPARSE_FROM:
        keep = np.zeros(N + 1, bool)
        keep[np.r_[0:8, 500:508, N - 16:N + 1]] = True
        cts[:, ~keep] = 0
    edge = np.concatenate([np.array(cc.ADVERSARIAL_WORDS, dtype=np.uint64), cc.tie_words(levels, base_log)])
    if count:
        w = min(edge.size, 8)
        cts[0, :w] = edge[:w]
        cts[-1, N - 8:N] = np.resize(edge[::-1], 8)
        cts[count // 2, N] = np.uint64(1 << 63)
    return cts


def check_bit_exact(eng, key, count, levels, base_log, c, seed):
    import torch
    N = eng.P.N
    cts = edge_rows(np.random.default_rng(seed), count, N, levels, base_log)
    got = eng.compress_host(cts, c)
    assert len(got) == count and got.words.dtype == np.uint32 and got.words.size == eng.compressed_words(count) == cc.compressed_words(count, N)
    want = cc.compress(cts, key, levels, base_log, c)
    assert np.array_equal(got.words, want), f"{int((got.words != want).sum())} of {want.size} compressed values differ"
    # the device-pointer form on torch's stream
    d_in = torch.from_numpy(cts.view(np.int64)).cuda()
    d_out = torch.full((max(want.size, 1),), -1, dtype=torch.int32, device="cuda")
    eng.compress(d_in, count, d_out, c, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32)[:want.size], want)
    if count == 0:
        assert int(d_out[0]) == -1     # nothing was launched


@pytest.mark.parametrize("count", [0, 1, 5, 65, 1023, 1024, 1025])
def test_compressed_values_equal_the_reference_at_the_defaults(random_key_engines, count):
    """N = 1024, (1, 16, 16): no ciphertext, one, a partial tile, two tiles with one ciphertext in the second, a block short of
    one, a full block, and a second block with a single ciphertext"""
    eng, key = random_key_engines("default", 1, 16)
    check_bit_exact(eng, key, count, 1, 16, 16, count + 1)


@pytest.mark.parametrize("levels,base_log,c", [(2, 12, 12), (3, 8, 32)])
def test_compressed_values_equal_the_reference_at_other_shapes(random_key_engines, levels, base_log, c):
    """129 dense rows (three tiles, one ciphertext in the last) with several levels, at the narrowest useful and the widest modulus"""
    eng, key = random_key_engines("default", levels, base_log)
    check_bit_exact(eng, key, 129, levels, base_log, c, 7)


@pytest.mark.parametrize("name", ["secure128_torus", "secure128_torus_wide"])
def test_compressed_values_equal_the_reference_on_the_wider_rings(random_key_engines, name):
    """N = 2048 and N = 4096 (two and four coefficients per thread of the switch), three dense rows at (1, 16, 16)"""
    eng, key = random_key_engines(name, 1, 16)
    check_bit_exact(eng, key, 3, 1, 16, 16, 9)


def test_a_block_in_several_slices_equals_the_reference(random_key_engines):
    """N = 2048 takes a block in slices of 512 ciphertexts: 600 sparse rows cross the first slice boundary (the accumulator is
    initialised by the first slice and added to by the second)"""
    eng, key = random_key_engines("secure128_torus", 1, 16)
    cts = edge_rows(np.random.default_rng(3), 1100, eng.P.N, 1, 16)[:600]
    got = eng.compress_host(cts, 16)
    assert np.array_equal(got.words, cc.compress(cts, key, 1, 16, 16))


# ---- valid keys: round trip, key rows, noise

@pytest.fixture(scope="module")
def det_engine():
    e = make_engine("default", 0x5EED)
    yield e
    e.close()


@pytest.mark.parametrize("csprng,levels,base_log", [(True, 1, 16), (False, 1, 16), (False, 2, 16)])
def test_compressed_encryptions_decrypt_and_key_rows_encrypt_their_messages(csprng, levels, base_log):
    """keygen + compression_keygen, from the CSPRNG and from the deterministic test streams: every 4-bit message comes back at
    counts 16 and 1,040, and EVERY row of the exported key - both levels of a two-level one - decrypts under the exported sk_big to
    S_j 2^(64 - base_log (l + 1)) within 6 sigma of glwe_noise"""
    eng = make_engine("default", None if csprng else 0x5EED)
    try:
        N = eng.P.N
        eng.compression_keygen(levels, base_log)
        assert eng.compression_key_info() == (levels, base_log, N * levels * 2 * N * 8 + 2 * N * 8)
        dl = eng.delta_log()
        for count in (16, 1040):
            msgs = np.arange(count) % 16 - 8
            packed = eng.compress_host(eng.encrypt(msgs, dl), 32 if levels == 2 else 16)
            assert eng.decrypt_compressed(packed, dl).tolist() == msgs.tolist()
            assert cc.decode(eng.phase_compressed(packed), dl).tolist() == msgs.tolist()
        _, sk_big, _, _ = eng.export_keys()
        key = eng.export_compression_key()
        assert key.shape == (N, levels, 2, N)
        err = cc.key_row_errors(key, sk_big, base_log)
        assert err.shape == (N * levels, N)
        sigma = eng.P.glwe_noise * 2.0 ** 64
        print(f"compression key rows ({levels}, {base_log}): largest |error| = {np.abs(err).max() / sigma:.2f} sigma, "
              f"std = {err.std() / sigma:.4f} sigma")
        assert np.abs(err).max() <= 6 * sigma + 1
        assert 0.99 < err.std() / sigma < 1.01      # 10^6 samples: the standard deviation itself to 0.07 %; (1 sigma of rounding: 1/12 word^2)
    finally:
        eng.close()


def mse_ratio(eng, levels, base_log, c, per_call, calls, hw):
    from bmi_amd import error_budget
    dl = eng.delta_log()
    rng = np.random.default_rng(per_call + calls)
    sq = []
    for _ in range(calls):
        msgs = rng.integers(-8, 8, per_call)
        packed = eng.compress_host(eng.encrypt(msgs, dl), c)
        sq.append(cc.mean_square_error(eng.phase_compressed(packed), msgs, dl))
    return float(np.mean(sq)) / error_budget.compression_variance(eng.P, levels, base_log, c, min(per_call, eng.P.N), hw_big=hw)


def test_phase_error_sits_on_the_formula(det_engine):
    """the mean-square phase error of compressed fresh encryptions over compression_variance (with the key's own weight), within
    +-15 %: 4 blocks at (1, 16, 16), where the rounding and the switch carry it, and at (2, 16, 32), where the key's noise does,
    2 full blocks and 2 blocks of 256 ciphertexts (a quarter of the key term)"""
    eng = det_engine
    hw = int(eng.export_keys()[1].sum())
    eng.compression_keygen(1, 16)
    ratios = {"(1,16,16) 4 x 1024": mse_ratio(eng, 1, 16, 16, 4096, 1, hw)}
    eng.keygen(0x5EED)      # a key set takes one shape of compression key: the same keys again, for the second shape
    assert int(eng.export_keys()[1].sum()) == hw
    eng.compression_keygen(2, 16)
    ratios["(2,16,32) 2 x 1024"] = mse_ratio(eng, 2, 16, 32, 2048, 1, hw)
    ratios["(2,16,32) 2 x 256"] = mse_ratio(eng, 2, 16, 32, 256, 2, hw)
    for k, v in ratios.items():
        print(f"compression noise {k}: mean-square error / formula = {v:.3f}")
    assert all(0.85 < v < 1.15 for v in ratios.values()), ratios


# ---- seeded form and key files

@pytest.fixture(scope="module")
def client():
    e = make_engine("default", None)
    e.compression_keygen(2, 12)
    yield e
    e.close()


def test_seeded_import_holds_the_clients_compression_key(client):
    """import_keys_seeded + import_compression_key_seeded: the server's exported key equals the client's word for word, its masks
    are the words of the public stream at the new domain, and both compress alike"""
    from bmi_amd import tfhe
    N = client.P.N
    pub, bsk_body, ksk_body = client.export_keys_seeded()
    body = client.export_compression_key_seeded()
    full = client.export_compression_key()
    assert body.shape == (N, 2, N) and np.array_equal(body, full[:, :, 1])
    flat = full.reshape(2 * N, 2, N)
    for row in (0, 1, 2, 777, 2 * N - 1):
        assert np.array_equal(flat[row, 0], sc.stream_words(pub, (PKSK_DOMAIN << 56) | row, 0, N)), row
    server = tfhe.Engine(SETS["default"](tfhe))
    try:
        server.import_keys(None, None, *client.export_keys(secret=False)[2:])
        with pytest.raises(tfhe.BmiError, match="bmi_import_keys_seeded"):
            server.import_compression_key_seeded(body, 2, 12)
        server.import_keys_seeded(pub, bsk_body, ksk_body)
        assert server.compression_key_info()[0] == 0
        server.import_compression_key_seeded(body, 2, 12)
        assert server.compression_key_info() == client.compression_key_info()
        assert np.array_equal(server.export_compression_key(), full)
        cts = client.encrypt(np.arange(40) % 16 - 8, client.delta_log())
        assert np.array_equal(server.compress_host(cts, 14).words, client.compress_host(cts, 14).words)
        # a key loaded in full has no seeded form
        server.import_compression_key(full, 2, 12)
        with pytest.raises(tfhe.BmiError, match="no seeded form"):
            server.export_compression_key_seeded()
    finally:
        server.close()


@pytest.mark.parametrize("seeded", [False, True])
def test_key_files_carry_the_compression_key(client, tmp_path, seeded):
    from bmi_amd import tfhe
    path = str(tmp_path / "keys.npz")
    client.save_keys(path, secret=False, seeded=seeded)
    server = tfhe.Engine(SETS["default"](tfhe))
    try:
        server.load_keys(path)
        assert server.compression_key_info() == client.compression_key_info()
        assert np.array_equal(server.export_compression_key(), client.export_compression_key())
        dl = client.delta_log()
        msgs = np.arange(20) % 16 - 8
        packed = server.compress_host(client.encrypt(msgs, dl))
        wire = tfhe.CompressedCiphertexts.frombytes(packed.tobytes())
        assert client.decrypt_compressed(wire, dl).tolist() == msgs.tolist()
    finally:
        server.close()
    if seeded:
        # a compression key that was loaded in full has no seeded form: it travels in full inside the seeded file
        full = client.export_compression_key()
        other = tfhe.Engine(SETS["default"](tfhe))
        try:
            client.import_compression_key(full, 2, 12)
            client.save_keys(path, secret=False, seeded=True)
            other.load_keys(path)
            assert np.array_equal(other.export_compression_key(), full) and other.compression_key_info()[:2] == (2, 12)
        finally:
            other.close()
            client.compression_keygen(2, 12)     # the same shape again: the same key, with its seeded form
        assert np.array_equal(client.export_compression_key(), full)
        assert np.array_equal(client.export_compression_key_seeded(), full[:, :, 1])
    # a file without a compression key loads as before, and leaves none
    plain = make_engine("default", 3)
    other = tfhe.Engine(SETS["default"](tfhe))
    try:
        plain.save_keys(path)
        assert other.load_keys(path) is True and other.compression_key_info()[0] == 0
    finally:
        plain.close()
        other.close()


# ---- refusals

def test_refusals_say_why():
    from bmi_amd import tfhe
    eng = make_engine("default", 5)
    field = tfhe.Engine(tfhe.default_params(q_bits=49, n=16))
    try:
        cts = eng.encrypt(np.zeros(3, np.int64), eng.delta_log())
        with pytest.raises(tfhe.BmiError, match="no compression key"):
            eng.compress_host(cts)
        with pytest.raises(tfhe.BmiError, match="levels \\* base_log <= 63"):
            eng.compression_keygen(4, 16)
        for bad in ((0, 16), (5, 8), (1, 17), (1, 0)):
            with pytest.raises(tfhe.BmiError, match="decomposition"):
                eng.compression_keygen(*bad)
        eng.compression_keygen()
        for bad in (1, 33):
            with pytest.raises(tfhe.BmiError, match="log_modulus must be in \\[2, 32\\]"):
                eng.compress_host(cts, bad)
        assert len(eng.compress_host(cts, 2)) == len(eng.compress_host(cts, 32)) == 3
        eng.keygen(6)              # a new key set drops the compression key
        assert eng.compression_key_info()[0] == 0
        with pytest.raises(tfhe.BmiError, match="a new key set drops it"):
            eng.compress_host(cts)
        field.keygen(5)
        with pytest.raises(tfhe.BmiError, match="2\\^64 torus only"):
            field.compression_keygen()
        with pytest.raises(tfhe.BmiError, match="2\\^64 torus only"):
            field.compress_host(field.encrypt(np.zeros(1, np.int64), field.delta_log()))
        with pytest.raises(tfhe.BmiError, match="2\\^64 torus only"):
            field.compressed_words(3)
        with pytest.raises(tfhe.BmiError, match="2\\^64 torus only"):     # whatever the other arguments
            field.decrypt_compressed(tfhe.CompressedCiphertexts(1, 1024, 16, np.zeros(1025, np.uint32)), 0)
    finally:
        eng.close()
        field.close()


@pytest.mark.parametrize("csprng", [True, False])
def test_a_key_set_takes_one_shape_of_compression_key(csprng):
    """a second compression_keygen of another (levels, base_log) on the same key set would reuse every common row's mask and noise
    streams under another message (the difference of the two bodies tells secret-key bits): refused with a text, the key held stays
    as it is, the same shape again gives the same key, and a new key set takes any shape"""
    from bmi_amd import tfhe
    eng = make_engine("default", None if csprng else 7)
    try:
        eng.compression_keygen(1, 16)
        first = eng.export_compression_key()
        for other in ((2, 16), (1, 12), (2, 8)):
            with pytest.raises(tfhe.BmiError, match="already has a compression key of shape \\(1, 16\\)"):
                eng.compression_keygen(*other)
        assert eng.compression_key_info()[:2] == (1, 16) and np.array_equal(eng.export_compression_key(), first)
        # an imported key does not lift the rule either
        eng.import_compression_key(pc.uniform_words(np.random.default_rng(1), (eng.P.N, 2, 2, eng.P.N)), 2, 16)
        with pytest.raises(tfhe.BmiError, match="already has a compression key"):
            eng.compression_keygen(2, 16)
        eng.compression_keygen(1, 16)
        assert np.array_equal(eng.export_compression_key(), first)
        eng.keygen(None if csprng else 8)
        eng.compression_keygen(2, 16)
        assert eng.compression_key_info()[:2] == (2, 16)
    finally:
        eng.close()


# ---- the application

def test_encrypted_inverse_through_compressed_outputs():
    """the golden 2x2 inverse with compress_outputs=True: the digits of the plain form, the stated number of bytes on the wire,
    two matrices per walk in blocks of their own, and an error budget between the plain one and ten times it"""
    from bmi_amd import error_budget, tfhe
    from bmi_amd.main import EncryptedMatrixInversion
    c = pc.golden_inverse("survey_2x2")
    eng = tfhe.Engine()
    try:
        emi = EncryptedMatrixInversion(2, None, 2, c["len"], c["ints"], False, False, engine=eng, compress_outputs=True)
        emi.keygen(0x5EED)
        assert eng.compression_key_info()[:2] == (1, 16)
        plain = EncryptedMatrixInversion(2, None, 2, c["len"], c["ints"], False, False, engine=eng)
        M = np.array(c["M"]).reshape(2, 2)
        enc = emi.encrypt(*emi.quantize(M))
        packed = emi.evaluate(enc)
        n_out = 4 * (c["len"] + 1)
        assert isinstance(packed, tfhe.CompressedCiphertexts) and len(packed) == n_out and packed.log_modulus == 16
        assert len(packed.tobytes()) == packed.nbytes == 16 + 2 * (eng.P.N + n_out)
        full = plain.evaluate(enc)
        assert full.shape == (n_out, eng.P.N + 1)
        assert emi.decrypt(packed).tolist() == plain.decrypt(full).tolist() == c["out"]
        assert emi.decrypt(tfhe.CompressedCiphertexts.frombytes(packed.tobytes())).tolist() == c["out"]
        M2 = M.T.copy()
        want2 = plain.simulate(*plain.quantize(M2)).tolist()
        many = emi.evaluate_many([enc, emi.encrypt(*emi.quantize(M2))])
        assert isinstance(many, list) and len(many) == 2 and all(len(p) == n_out for p in many)
        assert emi.decrypt(many[0]).tolist() == c["out"] and emi.decrypt(many[1]).tolist() == want2
        p_plain = error_budget.failure_probability(emi.program, eng.P, eng.bsk_precision)["p_fail"]
        p_packed = error_budget.failure_probability(emi.program, eng.P, eng.bsk_precision, compressed_outputs=(1, 16, 16))["p_fail"]
        print(f"failure probability: plain {p_plain:.3e}, compressed outputs {p_packed:.3e}")
        assert p_plain <= p_packed < 10 * p_plain
        assert emi.error_budget["p_fail"] == pytest.approx(p_packed)
    finally:
        eng.close()
