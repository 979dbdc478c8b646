"""tests/pbs_cases.py on the CPU: every helper against its expression written out - the same arrays from the same draws in the
same order (the generator ends in the same state: the GPU tests' inputs are a function of their seeds and of that order) -, the
centred error against its definition in Python integers on all three moduli, and the oracle's parameter sets against the library's."""
import numpy as np
import pytest

import pbs_cases as pc

GOLD = (1 << 64) - (1 << 32) + 1
P49 = (1 << 49) - 720895
SEEDS = [0, 1, 1000 + 257]


def two_draws(rng, shape):
    return rng.integers(0, 1 << 63, shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, shape, dtype=np.uint64)


def same_stream(a, b):
    """the two generators give the same next draw: they consumed the same stream"""
    return a.integers(0, 1 << 62) == b.integers(0, 1 << 62)


@pytest.mark.parametrize("Q", [1 << 64, GOLD, P49], ids=["torus64", "goldilocks64", "p49"])
def test_centred_error_is_the_integer_definition(Q):
    phases = [0, 1, Q // 2 - 1, Q // 2, Q // 2 + 1, Q - 1]
    for dl in (58, 59):
        bits = 63 - dl
        for m in (-(1 << (bits - 1)), (1 << (bits - 1)) - 1):
            want = np.array([((int(x) - (int(m) << dl)) + Q // 2) % Q - Q // 2 for x in phases], dtype=np.float64) / Q
            got = pc.centred_error(np.array(phases, dtype=np.uint64), [m] * len(phases), dl, Q)
            assert got.dtype == np.float64 and np.array_equal(got, want), (dl, m)
            assert np.array_equal(pc.centred_words(np.array(phases, dtype=np.uint64), [m] * len(phases), dl, Q) / Q, want)
            assert np.all(np.abs(got) <= 0.5)


@pytest.mark.parametrize("seed", SEEDS)
def test_uniform_words_and_sample_rows_consume_the_stream_as_written_out(seed):
    a, b = np.random.default_rng(seed), np.random.default_rng(seed)
    for shape in (7, (3, 5)):
        assert np.array_equal(pc.uniform_words(a, shape), two_draws(b, shape))
    for count, fixed, extra in ((5, [0, 4, 255, 256, 511, 512], 10), (8, [0, 1, 2, 3, 4, 7, 255, 256], 4), (9, [0, 8, 255, 256, 511, 512], 6),
                                (300, [0, 299, 255, 256, 511, 512], 10), (600, [0, 1, 2, 3, 4, 599, 255, 256], 2), (520, [0, 1, 2, 3, 4, 519, 255, 256], 1)):
        want = np.arange(count) if count <= 8 else np.unique(np.concatenate([fixed, b.integers(0, count, extra)]) % count)
        assert np.array_equal(pc.sample_rows(count, fixed, a, extra), want)
    assert same_stream(a, b)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("count", [1, 2, 3, 4, 5])
def test_adversarial_rows_as_written_out(seed, count):
    a, b = np.random.default_rng(seed), np.random.default_rng(seed)
    got, small = np.full((count, 21), 7, np.uint64), np.full((count, 21), 7, np.uint64)
    pc.adversarial_rows(got, a, count)
    small[0] = two_draws(b, small.shape[1])
    if count > 2:
        small[1] = 0
        small[2] = np.uint64(0xFFFFFFFFFFFFFFFF)
    if count > 4:
        small[3] = b.integers(0, 1 << 63, small.shape[1], dtype=np.uint64) * np.uint64(2)
        small[3, 7::8] = 0
    assert np.array_equal(got, small) and same_stream(a, b)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("Q,rows,skipped", [(1 << 64, 10, False), (1 << 64, 10, True), (P49, 12, False)], ids=["torus", "torus_fft", "p49"])
def test_extreme_rows_unrolled_as_written_out(seed, Q, rows, skipped):
    a, b = np.random.default_rng(seed), np.random.default_rng(seed)
    got = pc.extreme_rows_unrolled(a, rows, 35, skipped_pairs=skipped, Q=Q)
    if Q == 1 << 64:
        small = b.integers(0, 2 ** 63, (rows, 35), dtype=np.uint64) * np.uint64(2) + b.integers(0, 2, (rows, 35), dtype=np.uint64)
        top, half, one = 2 ** 64 - 1, 2 ** 63, 2 ** 53
    else:
        small = b.integers(0, Q, (rows, 35), dtype=np.uint64)
        top, half, one = Q - 1, Q // 2, (Q + 2047) // 2048
    small[0] = 0
    small[1] = np.uint64(top)
    small[2] = np.uint64(half)
    small[3, ::2] = 0
    small[4, 1::2] = 0
    small[5, :-1] = np.uint64(one)
    if skipped:
        small[6, 14::16] = 0
        small[6, 15::16] = 0
    assert np.array_equal(got, small) and same_stream(a, b)


def test_keyswitch_variance_and_lookup_margin_on_the_secure128_torus_numbers():
    from collections import namedtuple
    P = namedtuple("P", "n N k ks_levels ks_base_log lwe_noise")(742, 2048, 1, 8, 2, 2.0 ** -17.11)
    B = 2.0 ** 2
    analytic = 2048 * 8 * (B * B + 2) / 12.0 * (2.0 ** -17.11) ** 2 + 2048 / 2.0 / (12.0 * B ** 16)
    assert pc.keyswitch_variance(P) == analytic
    for power, bits, half_box in ((analytic, 4, 2048 / 32.0), (1.3 * analytic, 5, 2048 / 64.0)):
        sigma_pos = np.sqrt(power * (2 * 2048) ** 2 + (742 / 2.0 + 1) / 12.0)
        assert pc.lookup_margin(P, power, bits) == (sigma_pos, half_box / sigma_pos)
    assert 8.0 < pc.lookup_margin(P, analytic, 4)[1] < 9.0      # the margin the GPU tests measure on this set


# every parameter set a caller of oracle_for builds its engine from: the library's set, copied field by field, is the oracle's own
# default_params of the same arguments.  (An engine keeps the Params it was made from: set_bsk_unroll and set_bsk_precision change
# the context, not eng.P.  Like tests/test_abi.py this needs the built library; loading it is most of the test's time.)
PARAMETER_SETS = [(qb, kw) for qb in (49, 64, 65) for kw in (dict(), dict(n=629), dict(n=1024), dict(n=1), dict(bs_levels=2), dict(bs_levels=1, bs_base_log=23))]
PARAMETER_SETS += [(64, dict(n=97, ks_levels=5, ks_base_log=6)), (49, dict(n=97, ks_levels=5, ks_base_log=6)), (49, dict(n=639, ks_levels=4, ks_base_log=7)),
                   (49, dict(n=1024, ks_levels=8, ks_base_log=4)), (49, dict(n=211, bs_levels=2, bs_base_log=15)), (49, dict(n=211, bs_levels=1, bs_base_log=23)),
                   (65, dict(n=211, bs_levels=2, bs_base_log=15)), (65, dict(n=211, bs_base_log=15)), (65, dict(n=211, bs_levels=2)), (65, dict(n=211)),
                   (65, dict(bs_base_log=15)), (49, dict(log_N=11)), (49, dict(log_N=12)), (49, dict(n=3, log_N=11, bs_levels=1, bs_base_log=23))]


def test_field_copy_of_the_library_parameters_equals_the_oracle_defaults():
    from bmi_amd import tfhe
    from oracle import tfhe_oracle as to
    fields = [f for f, _ in tfhe.Params._fields_]
    assert fields == [f for f, _ in to.Params._fields_]
    for q_bits, kw in PARAMETER_SETS:
        lib, ora = tfhe.default_params(q_bits=q_bits, **kw), to.default_params(q_bits=q_bits, **kw)
        assert [getattr(lib, f) for f in fields] == [getattr(ora, f) for f in fields], (q_bits, kw)
    # the one set where they differ: the unrolled (l, Bg) = (1, 2^23) cases lower the engine's key noise and build the oracle's set
    # without it - that caller (tests/test_gpu_unrolled.py) passes its own Params
    lib = tfhe.default_params(q_bits=49, bs_levels=1, bs_base_log=23, glwe_noise=2.0 ** -46)
    ora = to.default_params(q_bits=49, n=lib.n, log_N=lib.log_N, bs_levels=lib.bs_levels, bs_base_log=lib.bs_base_log)
    assert [f for f in fields if getattr(lib, f) != getattr(ora, f)] == ["glwe_noise"]
