"""Decompression of compressed ciphertexts back to big-key LWE ciphertexts (include/bmi_tfhe.h, csrc/lwe_unpack.hip) on the GPU: every
word equals the numpy restatement's (tests/decompress_cases.py) on uniformly random compressed values - no key is involved, so the
contexts of those cases hold none; under valid keys the decompressed phase is the compressed phase word for word; decompressed
ciphertexts bootstrap; the encrypted inverse takes its inputs compressed (and returns its outputs compressed); what cannot be served
is refused with a text.  Contexts are cut to n = 16 wherever no bootstrap runs."""
import numpy as np
import pytest

import compress_cases as cc
import decompress_cases as dc
import pbs_cases as pc

pytestmark = pytest.mark.gpu

SETS = {"default": lambda tfhe: tfhe.default_params(n=16),
        "secure128_torus": lambda tfhe: tfhe.preset_params("secure128_torus", n=16),
        "secure128_torus_wide": lambda tfhe: tfhe.preset_params("secure128_torus_wide", n=16)}
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def keyless():
    """one context per parameter set that has run no keygen at all"""
    from bmi_amd import tfhe
    engines = {}

    def get(name):
        if name not in engines:
            engines[name] = tfhe.Engine(SETS[name](tfhe))
        return engines[name]
    yield get
    for e in engines.values():
        e.close()


def check_bit_exact(eng, count, c, index, seed):
    """host form (an aligned device buffer of the context's) at each of the three plantings of the edge words, then the
    device-pointer form on torch's stream into rows that start on an odd 8-byte boundary, between two spare rows"""
    import torch
    from bmi_amd import tfhe
    N = eng.P.N
    rng = np.random.default_rng(seed)
    index = None if index is None else np.asarray(index, dtype=np.int64)
    rows = count if index is None else index.size
    for shift in range(3):
        words = dc.random_compressed(rng, count, N, c, shift)
        want = dc.decompress(words, count, N, c, index)
        got = eng.decompress_host(tfhe.CompressedCiphertexts(count, N, c, words), index)
        assert got.shape == (rows, N + 1) and got.dtype == np.uint64
        assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} words differ (host form, planting {shift})"
    stream = torch.cuda.current_stream().cuda_stream
    # values are taken mod 2^c on the device: the bits above c are garbage here
    dirty = words if c == 32 else words | (rng.integers(0, 1 << (32 - c), words.size, dtype=np.uint64).astype(np.uint32) << np.uint32(c))
    for on_device in (False, True):
        d_out = torch.full((rows + 2, N + 1), SENTINEL, dtype=torch.int64, device="cuda")
        assert (d_out[1:].data_ptr() & 15) == 8
        w = torch.from_numpy(dirty.view(np.int32)).cuda() if on_device else dirty
        ix = index if index is None or not on_device else torch.from_numpy(index.astype(np.int32)).cuda()
        eng.decompress(w, count, c, d_out[1:], index=ix, stream=stream)
        torch.cuda.synchronize()
        host = d_out.cpu().numpy().view(np.uint64)
        assert np.all(host[0] == SENTINEL) and np.all(host[-1] == SENTINEL), "a spare row was written"
        assert np.array_equal(host[1:-1], want), f"{int((host[1:-1] != want).sum())} of {want.size} words differ (device form)"
    # ... and on an aligned base
    d_out = torch.full((rows + 1, N + 1), SENTINEL, dtype=torch.int64, device="cuda")
    assert (d_out.data_ptr() & 15) == 0
    eng.decompress(words, count, c, d_out, index=index, stream=stream)
    torch.cuda.synchronize()
    host = d_out.cpu().numpy().view(np.uint64)
    assert np.array_equal(host[:-1], want) and np.all(host[-1] == SENTINEL)


@pytest.mark.parametrize("count", [0, 1, 5, 1023, 1024, 1025])
def test_decompressed_words_equal_the_reference_at_the_defaults(keyless, count):
    """N = 1024 at 16 bits, every position in order: nothing (no launch: the sentinel stays), one row, a few, a block short of
    one, a full block, and a second block that holds a single body value"""
    check_bit_exact(keyless("default"), count, 16, None, count + 1)


@pytest.mark.parametrize("c", [2, 32])
def test_decompressed_words_equal_the_reference_at_the_narrowest_and_widest_modulus(keyless, c):
    check_bit_exact(keyless("default"), 129, c, None, c)


INDEX_FORMS = {"reversed": np.arange(1030)[::-1], "second_block_only": np.array([1029, 1024, 1027]),
               "repeats": np.array([5, 5, 1024, 0, 1029, 5, 1023, 1024]), "no_rows": np.zeros(0, np.int64)}


@pytest.mark.parametrize("form", sorted(INDEX_FORMS))
def test_an_index_picks_positions_in_any_order(keyless, form):
    """1,030 compressed ciphertexts (a full block and one of 6): all of them backwards, three of the second block alone, repeats
    across both blocks, and an empty index, which launches nothing"""
    check_bit_exact(keyless("default"), 1030, 16, INDEX_FORMS[form], 40 + len(form))


@pytest.mark.parametrize("name", ["secure128_torus", "secure128_torus_wide"])
def test_decompressed_words_equal_the_reference_on_the_wider_rings(keyless, name):
    """N = 2048 and N = 4096 at 16 bits: three rows in order, and of N + 1 compressed ciphertexts the single one of the second
    block, then the first and the last of the first"""
    eng = keyless(name)
    N = eng.P.N
    check_bit_exact(eng, 3, 16, None, 9)
    check_bit_exact(eng, N + 1, 16, [N, 0, N - 1], 10)


# ---- valid keys

@pytest.fixture(scope="module")
def cut_engine():
    from bmi_amd import tfhe
    e = tfhe.Engine(SETS["default"](tfhe))
    e.keygen(0x5EED)
    e.compression_keygen(1, 16)
    yield e
    e.close()


def test_decompressed_phase_is_the_compressed_phase(cut_engine, keyless):
    """1,040 encryptions of i mod 16 - 8 (a full block and one of 16): the phase kernel on the decompressed rows gives
    phase_compressed word for word, decrypt returns the messages, and a context without any key decompresses to the same rows"""
    import torch
    eng = cut_engine
    dl = eng.delta_log()
    msgs = np.arange(1040) % 16 - 8
    packed = eng.compress_host(eng.encrypt(msgs, dl), 16)
    stream = torch.cuda.current_stream().cuda_stream
    d_ct = torch.empty((1040, eng.P.big), dtype=torch.int64, device="cuda")
    d_ph = torch.empty(1040, dtype=torch.int64, device="cuda")
    eng.decompress(packed.words, 1040, 16, d_ct, stream=stream)
    eng.phase_device(d_ct, 1040, d_ph, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_ph.cpu().numpy().view(np.uint64), eng.phase_compressed(packed))
    rows = d_ct.cpu().numpy().view(np.uint64)
    assert eng.decrypt(rows, dl).tolist() == msgs.tolist()
    assert np.array_equal(eng.decompress_host(packed), rows)
    assert np.array_equal(keyless("default").decompress_host(packed), rows)
    _, sk_big, _, _ = eng.export_keys()
    assert np.array_equal(dc.lwe_phase(rows, sk_big), cc.phase(packed.words, 1040, eng.P.N, 16, sk_big))


# ---- full parameters: a bootstrap, and the application

@pytest.fixture(scope="module")
def full_engine():
    from bmi_amd import tfhe
    e = tfhe.Engine()
    e.keygen(0x5EED)
    e.compression_keygen(1, 16)
    yield e
    e.close()


def test_decompressed_ciphertexts_bootstrap(full_engine):
    """n = 630: every 4-bit message four times, compressed at (1, 16, 16), decompressed under a permutation straight into the
    input of one pbs through a random 4-bit table: every output decrypts to the table's entry"""
    import torch
    eng = full_engine
    rng = np.random.default_rng(33)
    dl = eng.delta_log()
    msgs = np.repeat(np.arange(-8, 8), 4)
    table = rng.integers(-8, 8, 16)
    lid = eng.lut_register(table, 4, dl)
    packed = eng.compress_host(eng.encrypt(msgs, dl), 16)
    perm = rng.permutation(64)
    stream = torch.cuda.current_stream().cuda_stream
    d_ct = torch.empty((64, eng.P.big), dtype=torch.int64, device="cuda")
    d_out = torch.empty_like(d_ct)
    d_ids = torch.full((64,), lid, dtype=torch.int32, device="cuda")
    eng.decompress(packed.words, 64, 16, d_ct, index=perm, stream=stream)
    eng.pbs(d_ct, d_ids, 64, d_out, stream)
    torch.cuda.synchronize()
    assert eng.decrypt(d_ct.cpu().numpy().view(np.uint64), dl).tolist() == msgs[perm].tolist()
    assert eng.decrypt(d_out.cpu().numpy().view(np.uint64), dl).tolist() == table[msgs[perm] + 8].tolist()


@pytest.fixture(scope="module")
def survey(full_engine):
    """the golden 2x2 case on the shared engine (which already holds its keys and the compression key of the shape keygen makes):
    the plain instance, the one with compressed outputs, the matrix's full and compressed encryptions"""
    from types import SimpleNamespace
    from bmi_amd.main import EncryptedMatrixInversion
    c = pc.golden_inverse("survey_2x2")
    plain = EncryptedMatrixInversion(2, None, 2, c["len"], c["ints"], False, False, engine=full_engine)
    packing = EncryptedMatrixInversion(2, None, 2, c["len"], c["ints"], False, False, engine=full_engine, compress_outputs=True)
    assert full_engine.compression_key_info()[:2] == packing.COMPRESSION_SHAPE
    M = np.array(c["M"]).reshape(2, 2)
    enc = plain.encrypt(*plain.quantize(M))
    return SimpleNamespace(c=c, plain=plain, packing=packing, M=M, enc=enc, cin=full_engine.compress_host(enc, 16))


def test_encrypted_inverse_from_compressed_inputs(full_engine, survey):
    """compressed in, full out and compressed out: the golden digits and the stated wire bytes; the compressed outputs decompress,
    under the permutation into (digits ..., signs) order, to the messages of the full outputs' rows - what a second circuit would
    take as its inputs; the instance's budget for such inputs is failure_probability's"""
    from bmi_amd import error_budget, tfhe
    eng, s = full_engine, survey
    ln, n_out = s.c["len"], 4 * (s.c["len"] + 1)
    assert isinstance(s.cin, tfhe.CompressedCiphertexts) and len(s.cin) == s.plain.program.n_inputs == 84
    assert s.cin.nbytes == 16 + 2 * (eng.P.N + 84)
    full = s.plain.evaluate(s.cin)
    assert full.shape == (n_out, eng.P.N + 1)
    assert s.plain.decrypt(full).tolist() == s.c["out"]
    packed = s.packing.evaluate(s.cin)
    assert isinstance(packed, tfhe.CompressedCiphertexts) and len(packed) == n_out and packed.log_modulus == 16
    assert len(packed.tobytes()) == packed.nbytes == 16 + 2 * (eng.P.N + n_out)
    assert s.packing.decrypt(packed).tolist() == s.c["out"]
    # outputs come (digits, sign) entry by entry; inputs go all digits, then all signs
    perm = np.concatenate([(np.arange(4)[:, None] * (ln + 1) + np.arange(ln)[None, :]).reshape(-1), np.arange(4) * (ln + 1) + ln])
    rows = eng.decompress_host(packed, perm)
    dl = eng.delta_log(s.plain.msg_bits)
    out = np.array(s.c["out"])
    want = np.concatenate([out[:, :ln].reshape(-1), out[:, ln]])
    assert cc.decode(eng.phase(rows), dl).tolist() == cc.decode(eng.phase(full[perm]), dl).tolist() == want.tolist()
    assert np.array_equal(eng.phase(rows), eng.phase_compressed(packed)[perm])
    v = error_budget.decompressed_variance(eng.P, 1, 16, 16, 84, eng.P.glwe_noise ** 2)
    assert s.plain.failure_budget(v) == error_budget.failure_probability(s.plain.program, eng.P, eng.bsk_precision, input_variance=v)
    assert s.packing.failure_budget(v) == error_budget.failure_probability(s.plain.program, eng.P, eng.bsk_precision, input_variance=v,
                                                                         compressed_outputs=(1, 16, 16))
    assert s.plain.failure_budget() == s.plain.error_budget
    assert s.plain.error_budget["p_fail"] < s.plain.failure_budget(v)["p_fail"] < 10 * s.plain.error_budget["p_fail"]


def test_evaluate_many_and_an_input_index_from_compressed_inputs(full_engine, survey):
    """two compressed matrices in one walk return both matrices' digits; one walk reads its inputs through an index out of a longer,
    shuffled compressed list"""
    eng, s = full_engine, survey
    M2 = s.M.T.copy()
    want2 = s.plain.simulate(*s.plain.quantize(M2)).tolist()
    cin2 = eng.compress_host(s.plain.encrypt(*s.plain.quantize(M2)), 16)
    many = s.plain.evaluate_many([s.cin, cin2])
    assert many.shape == (2, 4 * (s.c["len"] + 1), eng.P.N + 1)
    assert s.plain.decrypt(many[0]).tolist() == s.c["out"] and s.plain.decrypt(many[1]).tolist() == want2
    rng = np.random.default_rng(4)
    filler = eng.encrypt(rng.integers(-8, 8, 1000), eng.delta_log(s.plain.msg_bits))
    place = rng.permutation(1084)                       # input j sits at position place[j] of 1,084: both blocks hold inputs
    mixed = np.concatenate([s.enc, filler])
    shuffled = np.empty_like(mixed)
    shuffled[place] = mixed
    assert place[:84].max() >= 1024 > place[:84].min()
    got = s.plain._executor().run_decrypted(eng.compress_host(shuffled, 16), input_index=place[:84])
    assert got.reshape(4, -1).tolist() == s.c["out"]


# ---- refusals

def test_refusals_say_why(cut_engine):
    import torch
    from bmi_amd import tfhe
    eng = cut_engine
    N = eng.P.N
    words = dc.random_compressed(np.random.default_rng(1), 5, N, 16)
    packed = tfhe.CompressedCiphertexts(5, N, 16, words)
    field = tfhe.Engine(tfhe.default_params(q_bits=49, n=16))
    try:
        d_out = torch.full((6, N + 1), SENTINEL, dtype=torch.int64, device="cuda")
        with pytest.raises(tfhe.BmiError, match="2\\^64 torus only"):
            field.decompress_host(packed)
        with pytest.raises(tfhe.BmiError, match="2\\^64 torus only"):
            field.decompress(words, 5, 16, d_out)
        for bad in (1, 33):
            with pytest.raises(tfhe.BmiError, match="log_modulus must be in \\[2, 32\\]"):
                eng.decompress(words, 5, bad, d_out)
            odd = tfhe.CompressedCiphertexts(5, N, 16, words)
            odd.log_modulus = bad
            with pytest.raises(tfhe.BmiError, match="log_modulus must be in \\[2, 32\\]"):
                eng.decompress_host(odd)
        with pytest.raises(tfhe.BmiError, match="compressed at N = 2048 on a context with N = 1024"):
            eng.decompress_host(tfhe.CompressedCiphertexts(1, 2048, 16, np.zeros(2049, np.uint32)))
        for bad in ([0, 5], [4, 1 << 31]):
            with pytest.raises(tfhe.BmiError, match="is not below the count of 5"):
                eng.decompress_host(packed, bad)
        # the device form checks what it can see: the sizes of the buffers it is handed
        with pytest.raises(tfhe.BmiError, match="d_out holds"):
            eng.decompress(words, 5, 16, d_out[2:])
        with pytest.raises(tfhe.BmiError, match="compress to 1029 32-bit values, not 1028"):
            eng.decompress(torch.from_numpy(words[:-1].view(np.int32)).cuda(), 5, 16, d_out)
        with pytest.raises(tfhe.BmiError, match="compress to 1029 32-bit values, not 1030"):
            eng.decompress(np.append(words, np.uint32(0)), 5, 16, d_out)
        with pytest.raises(tfhe.BmiError, match="negative"):
            eng.decompress_host(packed, [-1])
        wide = words.copy()
        wide[N + 4] = 1 << 16
        with pytest.raises(tfhe.BmiError, match="a value does not fit log_modulus bits"):
            eng.decompress_host(tfhe.CompressedCiphertexts(5, N, 16, wide))
        # no index and rows != count: only the C interface can ask for that
        out = np.zeros((4, N + 1), np.uint64)
        assert eng.lib.bmi_decompress_batch_host(eng.h, tfhe._ptr(words), 5, 16, None, 4, tfhe._ptr(out)) != 0
        assert "rows must equal count" in eng.lib.bmi_last_error(eng.h).decode()
        d_words = torch.from_numpy(words.view(np.int32)).cuda()
        assert eng.lib.bmi_decompress_batch(eng.h, tfhe._ptr(d_words), 5, 16, None, 4, tfhe._ptr(d_out), None) != 0
        assert "rows must equal count" in eng.lib.bmi_last_error(eng.h).decode()
        torch.cuda.synchronize()
        assert bool((d_out == SENTINEL).all()) and not out.any()        # no refusal wrote anything
    finally:
        field.close()


def test_the_executor_refuses_inputs_that_do_not_fit(full_engine, survey):
    from bmi_amd import tfhe
    eng, s = full_engine, survey
    ex = s.plain._executor()
    short = eng.compress_host(s.enc[:83], 16)
    with pytest.raises(ValueError, match="83 compressed ciphertexts for a program of 84 inputs"):
        ex.run(short)
    with pytest.raises(ValueError, match="input_index has 83 positions, the program has 84 inputs"):
        ex.run(s.cin, input_index=np.arange(83))
    with pytest.raises(ValueError, match="input_index reaches position 84"):
        ex.run(s.cin, input_index=np.arange(1, 85))
    with pytest.raises(ValueError, match="1 compressed input lists for an executor of batch 2"):
        s.plain._executor(2).run([s.cin])
    with pytest.raises(tfhe.BmiError, match="compressed at N = 2048"):
        ex.run(tfhe.CompressedCiphertexts(84, 2048, 16, np.zeros(2048 + 84, np.uint32)))
    with pytest.raises(ValueError, match="not a CompressedCiphertexts"):
        ex.run(s.enc, input_index=np.arange(84))
    with pytest.raises(ValueError, match="compressed inputs mixed with full or seeded ones"):
        s.plain.evaluate_many([s.cin, s.enc])
