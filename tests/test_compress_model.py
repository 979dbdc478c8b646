"""The compression of output ciphertexts on the CPU: the numpy restatement of the scheme (tests/compress_cases.py) against
Python-integer arithmetic and the oracle's digit rule, a compress-then-decrypt round trip, and the three terms of
error_budget.compression_variance each held alone to the mean-square error of the restatement (+-15 %, the project's noise
tolerance).  The GPU is held to the same restatement bit for bit in tests/test_gpu_compress.py."""
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import compress_cases as cc

M64 = (1 << 64) - 1


def py_digits(a, levels, base_log):
    """the rule written out in Python integers"""
    c = a - (1 << 64) if a >> 63 else a
    shift = 64 - levels * base_log
    r = (c >> shift) + ((c >> (shift - 1)) & 1)
    B = 1 << base_log
    out = [0] * levels
    for lev in range(levels - 1, 0, -1):
        d = r % B
        r //= B
        if d >= B // 2:
            d -= B
            r += 1
        out[lev] = d
    out[0] = r
    return out


SHAPES = [(1, 16), (2, 12), (3, 8), (4, 15), (1, 1), (4, 1), (3, 16), (2, 16)]


@pytest.mark.parametrize("levels,base_log", SHAPES)
def test_digits_follow_the_rule_on_adversarial_words(levels, base_log):
    """0, 2^63, 2^63 - 1, 2^64 - 1, ties at every level and random words: the helper's digits are the written-out rule's, they
    rebuild the word rounded to its top levels * base_log bits, the lower digits stay in [-B/2, B/2) and the top one in
    [-B/2, B/2] - and, where the oracle is built, they are ora_decompose's"""
    rng = np.random.default_rng(levels * 100 + base_log)
    words = np.concatenate([np.array(cc.ADVERSARIAL_WORDS, dtype=np.uint64), cc.tie_words(levels, base_log), cc.uniform_words(rng, 200)])
    got = cc.digits(words, levels, base_log)
    half = 1 << (base_log - 1)
    assert got.shape == (words.size, levels)
    assert got[:, 0].min() >= -half and got[:, 0].max() <= half
    if levels > 1:
        assert got[:, 1:].min() >= -half and got[:, 1:].max() < half
    shift = 64 - levels * base_log
    for w, d in zip(words.tolist(), got.tolist()):
        assert d == py_digits(w, levels, base_log), hex(w)
        c = w - (1 << 64) if w >> 63 else w
        rounded = ((c >> shift) + ((c >> (shift - 1)) & 1)) << shift
        assert sum(dl << (64 - base_log * (lev + 1)) for lev, dl in enumerate(d)) == rounded, hex(w)
    # the top digit reaches + B/2: 2^63 - 1 rounds up to + 2^63
    assert cc.digits(np.array([(1 << 63) - 1], dtype=np.uint64), levels, base_log)[0, 0] == half
    try:
        from oracle import tfhe_oracle as to
        to.lib()
    except (ImportError, OSError, subprocess.CalledProcessError):
        return          # no oracle library and no compiler to build it: the written-out rule above stands alone
    before = {0: 65, 562949952700417: 49}.get(int(to.lib().ora_modulus()), 64)      # the oracle's field is a global
    to.set_field(65)
    try:
        for w, d in zip(words.tolist(), got.tolist()):
            assert list(to.decompose(w, levels, base_log)) == d, hex(w)
    finally:
        to.set_field(before)


def test_exact_product_and_packing_equal_python_integers():
    """N = 16, 5 ciphertexts, (2, 12): the float64-limb product, the rows T_i, their rotated sum and the centred switch against the
    same definitions in Python integers"""
    N, count, levels, base_log, c = 16, 5, 2, 12, 16
    rng = np.random.default_rng(5)
    key = cc.uniform_words(rng, (N, levels, 2, N))
    cts = cc.uniform_words(rng, (count, N + 1))
    cts[0, :4] = np.array(cc.ADVERSARIAL_WORDS, dtype=np.uint64)
    D = cc.digits(cts[:, :N], levels, base_log).reshape(count, N * levels)
    K = key.reshape(N * levels, 2 * N)
    prod = cc.exact_product(D, K)
    Dl, Kl = D.tolist(), K.tolist()
    want = [[sum(Dl[i][k] * Kl[k][col] for k in range(N * levels)) & M64 for col in range(2 * N)] for i in range(count)]
    assert prod.tolist() == want
    # every digit at its extreme against all-ones words: the largest limb sums
    De = np.full((3, N * levels), 1 << 15, np.int64)
    De[1] = -(1 << 15)
    Ke = np.full((N * levels, 4), M64, np.uint64)
    assert cc.exact_product(De, Ke).tolist() == [[(int(De[i, 0]) * N * levels * M64) & M64] * 4 for i in range(3)]
    T = [[(-want[i][col] + (int(cts[i, N]) if col == N else 0)) & M64 for col in range(2 * N)] for i in range(count)]
    assert cc.lwe_to_glwe_rows(cts, key, levels, base_log).tolist() == T
    acc = [0] * (2 * N)
    for i in range(count):
        for comp in range(2):
            for x in range(N):
                src = T[i][comp * N + (x - i) % N]
                acc[comp * N + x] = (acc[comp * N + x] + (src if i <= x else -src)) & M64
    assert cc.rotate_sum(np.array(T, dtype=np.uint64), N).tolist() == acc
    sh = 64 - c
    cen = lambda v: ((v + (1 << (sh - 1))) % (1 << sh)) - (1 << (sh - 1))   # noqa: E731
    e = [cen(a) for a in acc[:N]]
    P = [sum(e[:x + 1]) for x in range(N)]
    words = [((a + (1 << (sh - 1))) >> sh) % (1 << c) for a in acc[:N]]
    for x in range(count):
        b = (acc[N + x] - ((2 * P[x] - P[-1]) >> 1)) & M64
        words.append(((b + (1 << (sh - 1))) >> sh) % (1 << c))
    assert cc.compress(cts, key, levels, base_log, c).tolist() == words


def test_compress_then_decrypt_returns_every_message():
    """N = 256, a random binary key, one full block and one of 44 ciphertexts at the defaults (1, 16, 16): every 4-bit message"""
    N, levels, base_log, c, dl = 256, 1, 16, 16, 59
    rng = np.random.default_rng(11)
    S = rng.integers(0, 2, N).astype(np.uint64)
    key = cc.make_key(rng, S, levels, base_log, 2.0 ** -50)
    msgs = np.arange(300) % 16 - 8
    cts = cc.encrypt(rng, S, msgs, dl, 2.0 ** -50)
    words = cc.compress(cts, key, levels, base_log, c)
    assert words.size == cc.compressed_words(300, N) == 2 * N + 300 and words.max() < 1 << c
    assert cc.decode(cc.phase(words, 300, N, c, S), dl).tolist() == msgs.tolist()


def compression_variance(N, glwe_noise, levels, base_log, log_modulus, count, hw_big):
    from bmi_amd import error_budget
    P = SimpleNamespace(log_N=N.bit_length() - 1, k=1, glwe_noise=glwe_noise)
    return error_budget.compression_variance(P, levels, base_log, log_modulus, count, hw_big=hw_big)


# term -> (levels, base_log, log_modulus, noise of the key rows): the shape at which the term stands alone
TERMS = {"switch": (2, 12, 16, 0.0), "key": (2, 16, 32, 2.0 ** -40), "rounding": (1, 16, 32, 0.0)}


@pytest.mark.parametrize("term", sorted(TERMS))
def test_each_variance_term_alone_matches_the_mean_square_error(term):
    """16 full blocks at N = 256 (4,096 coefficients) of noise-free encryptions: the mean-square phase error over
    compression_variance within +-15 %, at a shape where the other two terms are below a thousandth of the one measured (noiseless
    key rows for the switch and the rounding)"""
    levels, base_log, c, sigma = TERMS[term]
    N, blocks, dl = 256, 16, 59
    rng = np.random.default_rng(sorted(TERMS).index(term) + 1)
    S = rng.integers(0, 2, N).astype(np.uint64)
    hw = int(S.sum())
    key = cc.make_key(rng, S, levels, base_log, sigma)
    msgs = rng.integers(-8, 8, blocks * N)
    cts = cc.encrypt(rng, S, msgs, dl, 0.0)
    words = cc.compress(cts, key, levels, base_log, c)
    mse = cc.mean_square_error(cc.phase(words, msgs.size, N, c, S), msgs, dl)
    model = compression_variance(N, sigma, levels, base_log, c, N, hw)
    parts = {"key": N * N * levels * (4.0 ** base_log + 2) / 12 * sigma ** 2, "rounding": hw * 4.0 ** (-levels * base_log) / 12,
             "switch": (1 + N / 4) / 12 * 4.0 ** -c}
    assert model == pytest.approx(sum(parts.values()), rel=1e-12)
    assert parts[term] > 1000 * (model - parts[term])
    print(f"{term}: mean-square error / formula = {mse / model:.3f}")
    assert 0.85 < mse / model < 1.15


def test_compression_variance_counts_a_partial_block_and_caps_at_a_full_one():
    from bmi_amd import error_budget
    P = SimpleNamespace(log_N=10, k=1, glwe_noise=2.0 ** -51)
    v = lambda count: error_budget.compression_variance(P, 1, 16, 32, count) - error_budget.compression_variance(P, 1, 16, 32, 0)   # noqa: E731
    assert v(512) == pytest.approx(v(1024) / 2) and v(5000) == v(1024)
