"""The case table of tests/keyswitch_cases.py on the CPU: the crafted ciphertext words decompose to the digit vectors they were
built from, the Python-integer decomposition agrees with the oracle's ora_decompose, and the Python-integer keyswitch agrees with
the oracle's on every key family - which is what licenses the GPU test (tests/test_gpu_keyswitch.py) to hold its bulk rows to
the oracle alone.  Also pins the coverage the GPU file claims: which ring remainders and slice counts its cases reach."""
import numpy as np
import pytest

import keyswitch_cases as kc
from oracle import tfhe_oracle as to

SMALL_N = {64: 5, 49: 4, kc.TORUS64: 6}       # one small n per modulus: the keyswitch against the oracle


@pytest.fixture(params=[64, 49, kc.TORUS64], ids=["goldilocks64", "p49", "torus64"])
def field(request):
    to.set_field(request.param)
    yield request.param
    to.set_field(64)


def test_crafted_words_decompose_as_written_out(field):
    q = field
    seen = set()
    for levels, base_log in kc.shapes(q):
        B, h = 1 << base_log, 1 << (base_log - 1)
        words = kc.crafted_words(levels, base_log, q)
        got = kc.digits([a for _, a, _ in words], levels, base_log, q)
        for (name, a, want), d in zip(words, got):
            d = [int(x) for x in d]
            assert 0 <= a < kc.MODULUS[q]
            assert all(-h <= x < h for x in d[1:]) and -h <= d[0] <= h, (name, levels, base_log, d)
            # the vector spells, in base B, the centred lift rounded half up (exact rationals)
            assert sum(x * B ** (levels - 1 - l) for l, x in enumerate(d)) == kc.rounded(a, levels, base_log, q), (name, levels, base_log)
            if want is not None:
                assert d == want, (name, levels, base_log, d, want)
            seen.update(d)
            if d[0] == h:
                seen.add("top +B/2")
        names = [name for name, _, _ in words]
        assert any(n.startswith("tie alone") for n in names) and any(n.startswith("every digit -B/2") for n in names)
        # both extremes of a lower digit and the top digit's +B/2 occur on every shape (one level has no lower digit; +B/2 needs
        # a rounding carry into the top, or a value the lift holds)
        flat = got[:, 1:].reshape(-1)
        if levels > 1:
            assert flat.min() == -h and flat.max() == h - 1, (levels, base_log)
        assert got[:, 0].min() == -h or q != kc.TORUS64
        assert got[:, 0].max() == h, (levels, base_log)
    assert "top +B/2" in seen


def test_digits_match_the_oracle(field):
    q = field
    Q = kc.MODULUS[q]
    rng = np.random.default_rng(11)
    for levels, base_log in kc.shapes(q):
        words = [a for _, a, _ in kc.crafted_words(levels, base_log, q)] + [int(a) for a in kc.rand_words(rng, 300, Q)]
        got = kc.digits(words, levels, base_log, q)
        want = np.stack([to.decompose(a, levels, base_log) for a in words])
        assert np.array_equal(got, want), (levels, base_log)


def test_keyswitch_matches_the_oracle_on_every_key_family(field):
    q = field
    n = SMALL_N[q]
    for levels, base_log in kc.shapes(q):
        names, cts = kc.rows(levels, base_log, q)
        P = to.default_params(n=n, q_bits=q, ks_levels=levels, ks_base_log=base_log)
        bsk = np.zeros(to.key_shapes(P)[2], np.uint64)
        for family in kc.key_families(q):
            ksk = kc.make_key(family, kc.BIG_N, levels, n, q)
            ctx = to.Ctx(P, bsk, ksk)
            try:
                want = ctx.keyswitch(cts)
            finally:
                ctx.close()
            got = kc.want_crafted(ksk, n, levels, base_log, q)
            assert np.array_equal(got, want), f"{(levels, base_log)} {family}\n" + kc.describe_mismatch(got, want, names)
            if q != kc.TORUS64:
                assert (got < np.uint64(kc.MODULUS[q])).all()


def test_key_families_are_what_they_claim():
    for q in (64, 49, kc.TORUS64):
        Q = kc.MODULUS[q]
        fam = kc.key_families(q)
        assert len(set(fam)) == len(fam) and {"uniform", "q-1", "half", "half+1", "one-row-one-column"} <= set(fam)
        assert ("2^63" in fam) == (q == kc.TORUS64)
        words = {f: kc.key_word(f, q) for f in fam if f not in ("uniform", "one-row-one-column")}
        assert all(0 <= w < Q for w in words.values()) and len(set(words.values())) >= len(words) - 3     # 2^63 is the torus' half
        # the balanced limbs of the lift families, by the school method on the centred value: a run of -128 with carries, of -1 and
        # then zeros, of 127 without a carry
        def limbs(a):
            c, out = kc.centred(a, q), []
            for _ in range(9):
                d = (c + 128) % 256 - 128
                c = (c - d) // 256
                out.append(d)
            assert c == 0
            return out
        assert limbs(words["lift+7f"])[:6] == [127] * 6
        assert limbs(words["lift+80"])[:6] == [-128] + [-127] * 5
        assert limbs(words["lift+ff"])[:5] == [-1] + [0] * 4 and 1 in limbs(words["lift+ff"])
        assert limbs(words["lift-80"])[:6] == [-128] * 6 and limbs(words["lift-7f"])[:6] == [-127] * 6
        key = kc.make_key("one-row-one-column", 64, 3, 9, q)
        assert np.count_nonzero(key) <= 10 + 64 * 3 and np.count_nonzero(key[:, :, 4]) > 180 and np.count_nonzero(key[61, 2]) >= 9


def test_coverage_of_the_gpu_cases():
    """what tests/test_gpu_keyswitch.py states in its docstring, derived from the slice rules restated in keyswitch_cases"""
    for q in (64, 49, kc.TORUS64):
        cov = kc.coverage(q)
        depth = kc.ring_depth(q)
        mfma = [c for c in cov if c[3] == "mfma"]
        assert {c[6] for c in mfma} == set(range(depth)), q
        assert any(c[5] < depth for c in mfma) and any(c[0][0] == 1 and c[5] < depth for c in mfma)
        assert {c[1] for c in cov} == {1, 31, 32, 255, 256, 511, 512, 767, 768, 1024}
        assert {c[1] for c in cov if c[3] == "scalar"} == {1, 31, 32, 255, 256, 511, 512, 767}
        assert {c[2] for c in mfma} == set(kc.COUNTS) == {c[2] for c in cov if c[3] == "scalar"}
        want_shapes = {(1, 1), (1, 7), (3, 5), (5, 6), (6, 7), (8, 4), (16, 3), (17, 2)} | ({(9, 7), (21, 3)} if q != 49 else set())
        assert want_shapes <= {c[0] for c in cov}
        assert want_shapes - {(17, 2), (21, 3)} <= {c[0] for c in mfma}
        assert want_shapes <= {c[0] for c in cov if c[3] == "scalar"}
        # shift 1: 63 of 64 bits, 48 of 49
        assert any(l * b == kc.width(q) - 1 for (l, b) in kc.shapes(q))
    assert kc.scalar_slices(kc.BIG_COUNT, 8) == 1 and kc.scalar_slices(kc.BIG_COUNT, 21) == 4 and kc.scalar_slices(33, 8, pinned=True) == 1
    assert kc.scalar_slices(33, 9, pinned=True) == 2 and kc.scalar_slices(33, 16, pinned=True, big_n=4096) == 8
