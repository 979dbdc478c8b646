"""Decompression of compressed ciphertexts on the CPU: the numpy restatement of the rule (tests/decompress_cases.py) against the
compressed phase of tests/compress_cases.py word for word, messages, the mean-square error against
error_budget.compression_variance (+-15 %, the project's noise tolerance), and the error budget's input_variance argument on the
2x2 inverse.  The GPU is held to the same restatement bit for bit in tests/test_gpu_decompress.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import compress_cases as cc
import decompress_cases as dc

N, COUNT, DL = 64, 70, 59       # one full block and one of 6 ciphertexts
# (levels, base_log, log_modulus) -> noise of the fresh encryptions, chosen next to the compression's own so that both terms of
# decompressed_variance count: (1, 16, 16) adds about (hw + 1 + N / 4) / 12 4^-16 = 2^-30, (2, 12, 32) about hw / 12 4^-24 = 2^-46.6
SHAPES = {(1, 16, 16): 2.0 ** -15, (2, 12, 32): 2.0 ** -24}
KEY_NOISE = 2.0 ** -50          # the key's own noise: below a millionth of either total


@pytest.fixture(scope="module", params=sorted(SHAPES))
def packed(request):
    levels, base_log, c = request.param
    rng = np.random.default_rng(levels * 1000 + base_log * 10 + c)
    S = rng.integers(0, 2, N).astype(np.uint64)
    key = cc.make_key(rng, S, levels, base_log, KEY_NOISE)
    msgs = np.arange(COUNT) % 16 - 8
    cts = cc.encrypt(rng, S, msgs, DL, SHAPES[request.param])
    words = cc.compress(cts, key, levels, base_log, c)
    return SimpleNamespace(shape=request.param, rng=rng, S=S, key=key, msgs=msgs, words=words, c=c,
                           phase=cc.phase(words, COUNT, N, c, S))


def test_decompressed_phase_is_the_compressed_phase_word_for_word(packed):
    """every position in order, reversed, and under an index with repeats that takes from both blocks: the LWE phase of the
    decompressed row under S equals the compressed phase of its position, and the messages decode"""
    p = packed
    assert p.words.size == cc.compressed_words(COUNT, N) == 2 * N + COUNT
    rows = dc.decompress(p.words, COUNT, N, p.c)
    assert rows.shape == (COUNT, N + 1) and rows.dtype == np.uint64
    assert np.array_equal(dc.lwe_phase(rows, p.S), p.phase)
    assert cc.decode(dc.lwe_phase(rows, p.S), DL).tolist() == p.msgs.tolist()
    for index in (np.arange(COUNT)[::-1], np.array([69, 0, 63, 64, 0, 69, 69, 5, 64])):
        got = dc.decompress(p.words, COUNT, N, p.c, index)
        assert np.array_equal(got, rows[index])
        assert np.array_equal(dc.lwe_phase(got, p.S), p.phase[index])
        assert cc.decode(dc.lwe_phase(got, p.S), DL).tolist() == p.msgs[index].tolist()
    assert dc.decompress(p.words, COUNT, N, p.c, np.zeros(0, np.int64)).shape == (0, N + 1)
    # the low bits of a row are empty: the words are the values shifted up
    assert not np.any(rows & np.uint64((1 << (64 - p.c)) - 1))


def test_values_are_taken_mod_the_modulus():
    rng = np.random.default_rng(2)
    words = dc.random_compressed(rng, 5, N, 12)
    dirty = words | np.uint32(0xF000)
    assert np.array_equal(dc.decompress(dirty, 5, N, 12), dc.decompress(words, 5, N, 12))


def decompressed_mse(p, sigma, seed):
    """mean-square phase error of the decompressed rows over 30 compressions of 70 encryptions of noise sigma each (2,100 phases:
    the estimate itself is +-3 %, 1 sigma) under the fixture's key"""
    levels, base_log, c = p.shape
    rng = np.random.default_rng(seed)
    sq = []
    for _ in range(30):
        msgs = rng.integers(-8, 8, COUNT)
        words = cc.compress(cc.encrypt(rng, p.S, msgs, DL, sigma), p.key, levels, base_log, c)
        sq.append(cc.mean_square_error(dc.lwe_phase(dc.decompress(words, COUNT, N, c), p.S), msgs, DL))
    return float(np.mean(sq))


def test_mean_square_error_sits_on_compression_variance(packed):
    """noise-free encryptions, so that the compression's own error stands alone (as tests/test_compress_model.py measures it): the
    mean-square error of the decompressed rows over compression_variance, with the key's own weight, within +-15 %.  Then
    encryptions whose own noise is of the compression's size: what they carry beyond their own variance sits on
    compression_variance within the same +-15 %, and decompressed_variance is the sum of the two"""
    from bmi_amd import error_budget
    p = packed
    levels, base_log, c = p.shape
    sigma = SHAPES[p.shape]
    P = SimpleNamespace(log_N=N.bit_length() - 1, k=1, glwe_noise=KEY_NOISE)
    hw = int(p.S.sum())
    added = error_budget.compression_variance(P, levels, base_log, c, COUNT, hw_big=hw)
    alone = decompressed_mse(p, 0.0, 16) / added
    print(f"{p.shape}: noise-free encryptions, mean-square error / compression_variance = {alone:.3f}")
    assert 0.85 < alone < 1.15
    assert error_budget.decompressed_variance(P, levels, base_log, c, COUNT, sigma ** 2, hw_big=hw) == pytest.approx(sigma ** 2 + added, rel=1e-12)
    assert error_budget.decompressed_variance(P, levels, base_log, c, COUNT, 0.0, hw_big=hw) == added
    beyond = (decompressed_mse(p, sigma, 17) - sigma ** 2) / added
    print(f"{p.shape}: encryptions of variance {sigma ** 2 / added:.2f} x compression_variance, (mean-square error - their variance) / "
          f"compression_variance = {beyond:.3f}")
    assert 0.85 < beyond < 1.15


# ---- the error budget's input term

@pytest.fixture(scope="module")
def inverse_2x2():
    from bmi_amd import tfhe
    from bmi_amd.main import compile_inverse
    prog, _ = compile_inverse(2, 20, 8)
    return prog, tfhe.default_params(q_bits=tfhe.TORUS64)


def test_no_input_variance_and_the_fresh_one_give_the_unchanged_budget(inverse_2x2):
    from bmi_amd import error_budget
    prog, P = inverse_2x2
    fresh = error_budget.failure_probability(prog, P)
    assert fresh == prog.failure_probability(P)                      # the path that takes no such argument
    assert fresh["log10_p_fail"] == pytest.approx(-5.77, abs=0.01) and fresh["worst_margin_sigma"] == pytest.approx(6.24, abs=0.01)
    assert error_budget.failure_probability(prog, P, input_variance=None) == fresh
    assert error_budget.failure_probability(prog, P, input_variance=P.glwe_noise ** 2) == fresh
    assert error_budget.failure_probability(prog, P, input_variance=np.full(prog.n_inputs, P.glwe_noise ** 2)) == fresh
    eng = SimpleNamespace(P=P, q_bits=P.q_bits, bsk_precision=error_budget.default_bsk_precision(P))
    assert error_budget.engine_failure_probability(prog, eng) == fresh
    assert error_budget.engine_failure_probability(prog, eng, input_variance=P.glwe_noise ** 2) == fresh
    with pytest.raises(ValueError, match="one per input"):
        error_budget.failure_probability(prog, P, input_variance=np.zeros(prog.n_inputs + 1))
    with pytest.raises(ValueError, match="not negative"):
        error_budget.failure_probability(prog, P, input_variance=-1.0)


def test_failure_probability_grows_with_the_input_variance(inverse_2x2):
    """non-decreasing over seven decades; the inputs decompressed from (1, 16, 16) in one block of the program's 84 inputs cost
    between one and ten times the fresh budget (10^-5.26 against 10^-5.77), and 12 bits leave nothing"""
    from bmi_amd import error_budget
    prog, P = inverse_2x2
    assert prog.n_inputs == 84
    fresh = error_budget.failure_probability(prog, P)["p_fail"]
    v0 = P.glwe_noise ** 2
    ps = [error_budget.failure_probability(prog, P, input_variance=v0 * 10.0 ** e)["p_fail"] for e in np.arange(0, 36, 0.5)]
    assert ps[0] == fresh and all(a <= b for a, b in zip(ps, ps[1:])) and ps[-1] == 1.0
    v16 = error_budget.decompressed_variance(P, 1, 16, 16, 84, v0)
    assert v16 == v0 + error_budget.compression_variance(P, 1, 16, 16, 84)
    r16 = error_budget.failure_probability(prog, P, input_variance=v16)
    print(f"2x2 inverse: fresh 10^{np.log10(fresh):.2f}, inputs decompressed from (1, 16, 16) 10^{r16['log10_p_fail']:.2f}, "
          f"worst margin {r16['worst_margin_sigma']:.2f} sigma")
    assert fresh < r16["p_fail"] < 10 * fresh
    assert r16["log10_p_fail"] == pytest.approx(-5.26, abs=0.01) and r16["worst_margin_sigma"] == pytest.approx(5.69, abs=0.01)
    # one input alone at that variance costs less than all of them
    one = np.full(84, v0)
    one[0] = v16
    assert fresh <= error_budget.failure_probability(prog, P, input_variance=one)["p_fail"] < r16["p_fail"]
    v12 = error_budget.decompressed_variance(P, 1, 16, 12, 84, v0)
    assert error_budget.failure_probability(prog, P, input_variance=v12)["p_fail"] == 1.0
