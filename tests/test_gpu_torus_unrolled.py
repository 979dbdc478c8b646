"""GPU parity tests of the UNROLLED blind rotation on the 2^64 TORUS (Concrete's ciphertext modulus; bmi_set_bsk_unroll(ctx, 2)
on a torus context with the key pinned at 48 bits, k_blind_rotate_lat2u_t64 - the exact-transform predecessor of the unrolled FFT
kernel of tests/test_gpu_torus_unrolled_fft.py): two LWE coefficients per step, exact limb-split products against a bootstrap key
stored at 48 bits of precision.  Bit for bit against oracle/tfhe_oracle.c ora_blind_rotate_extract_unrolled (which rotates in
the coefficient domain and multiplies through Goldilocks transforms of the key's 32-bit halves - a different route to the same
integers) on the same keys; output noise on the formula; the encrypted inverses against the reference's golden digits."""
import numpy as np
import pytest

import pbs_cases as pc

pytestmark = pytest.mark.gpu

SEED = 0x5EED
QB = 65
# the key pinned at 48 bits: every key and accumulator word on the 2^16 grid; 6 random rows to the oracle beside the fixed ones
CFG = pc.UnrolledConfig(q_bits=QB, precision=48, grid_mask=0xFFFF, oracle_rows=6, margin_hook=False)


def _engine(seed=SEED, **kw):
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=QB, **kw))
    e.set_bsk_precision(48)       # the exact-transform unrolled kernel (without this, unrolling picks the 42-bit key and the FFT route:
    e.set_bsk_unroll(2)           # tests/test_gpu_torus_unrolled_fft.py)
    e.keygen(seed)
    return e


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


def test_default_torus_set_and_seeded_keys_match_the_oracle(eng):
    """the torus set: (l, Bg) = (3, 2^10), bootstrap key at 48 bits; the library's keys = the oracle's keys rounded by the
    oracle's own statement of the rule, for the plain and for the unrolled key"""
    from oracle import tfhe_oracle as to
    P = pc.check_unrolled_seeded_keys(eng, CFG, SEED)
    assert (eng.P.n, eng.P.N, eng.P.k, eng.P.bs_levels, eng.P.bs_base_log) == (630, 1024, 1, 3, 10) == (P.n, P.N, P.k, P.bs_levels, P.bs_base_log)
    assert eng.bsk_precision == 48 == to.default_bsk_precision(P)


@pytest.mark.parametrize("count", [1, 5, 300, 700])
def test_unrolled_torus_pbs_bit_exact_every_batch_size(eng, count):
    pc.check_unrolled_pbs_every_batch_size(eng, CFG, count)


def test_unrolled_torus_blind_rotation_extreme_inputs(eng):
    pc.check_unrolled_extreme_inputs(eng, CFG, rows=10)


@pytest.mark.parametrize("kw", [dict(n=629), dict(n=1024), dict(bs_levels=2), dict(n=1)], ids=["odd_n", "n1024", "l2", "n1"])
def test_unrolled_torus_other_shapes_bit_exact(kw):
    e = _engine(seed=77, **kw)
    try:
        pc.check_unrolled_other_shape(e, decrypts=kw.get("n") != 1)   # (one coefficient cannot hold a message's phase)
    finally:
        e.close()


def test_unrolling_on_the_torus_is_refused_where_the_limb_sums_would_not_fit():
    """the three scaled products of an unrolled step must keep every limb sum below p/2: base 2^10 with the 48-bit key only"""
    from bmi_amd import tfhe
    for kw, prec in ((dict(bs_base_log=15), None), (dict(), 64)):
        e = tfhe.Engine(tfhe.default_params(q_bits=QB, **kw))
        try:
            if prec:
                e.set_bsk_precision(prec)
            with pytest.raises(tfhe.BmiError):
                e.set_bsk_unroll(2)
        finally:
            e.close()
    e = tfhe.Engine(tfhe.default_params(q_bits=QB))
    try:
        e.set_bsk_unroll(2)
        assert e.bsk_precision == 42         # the precision nobody chose follows the mode: the unrolled step takes the FFT route
        with pytest.raises(tfhe.BmiError):
            e.set_bsk_precision(64)          # would leave the unrolled mode without a kernel
        e.set_bsk_precision(48)              # the exact-transform unrolled kernel stays selectable
        e.set_bsk_unroll(1)
        assert e.bsk_precision == 48         # (an explicit choice is kept)
    finally:
        e.close()


def test_unrolled_torus_key_under_csprng_and_on_an_evaluation_only_context():
    """(the evaluation keys the second context imports are already on the 2^16 grid)"""
    pc.check_unrolled_csprng_key_and_evaluation_only_context(QB, count=7)


def test_unrolled_torus_output_noise_on_the_formula_and_timing(eng, capsys):
    """4,096 bootstraps: output variance = 3 x the key-noise term (the key noise a bootstrap sees includes the rounding of the
    48-bit key: body + the mask words the GLWE key selects) + the decomposition term of the pairs whose key bits are not both
    zero, doubled by the factor X^c - 1 (at Bg = 2^10 this term is the larger one); prints the latency of the unrolled kernel
    beside the plain torus latency kernel's (same set, same precision)"""
    rng = np.random.default_rng(21)
    B = 4096
    dl = eng.delta_log()
    ident = np.arange(-8, 8)
    msgs = rng.integers(-8, 8, B)
    lid = eng.lut_register(ident, 4, dl)
    ct = eng.encrypt(msgs, dl)
    out = eng.pbs_host(ct, np.full(B, lid, np.uint32))
    assert list(eng.decrypt(out, dl)) == list(msgs)
    err = pc.centred_error(eng.phase(out), msgs, dl, 1 << 64)
    want = pc.unrolled_torus_variance(eng)
    ratio = float(np.mean(err ** 2)) / want
    timing = pc.time_blind_rotation_beside_plain(eng, SEED, ident, msgs, dl)
    with capsys.disabled():
        print(f"\nunrolled torus PBS: output log2 std {0.5 * np.log2(np.mean(err ** 2)):.2f} (3 x key term + rounding term: {0.5 * np.log2(want):.2f}, "
              f"variance ratio {ratio:.3f}, worst 2^{np.log2(np.abs(err).max()):.2f}); blind rotation ms (host-buffer calls, copies included): " + timing)
    assert 0.88 < ratio < 1.12


@pytest.mark.parametrize("tag", ["baseline_n2_len20_ints8", "baseline_n3_len30_ints12", "baseline_n4_len40_ints16", "baseline_n8_len48_ints16",
                                 "overflow_digit_2x2", "overflow_digit_3x3", "uniform_3x3_small_truediv", "uniform_2x2_tensorize"])
def test_encrypted_inverse_on_the_torus_with_the_unrolled_key_matches_reference_golden(tag, capsys):
    """BASELINE configs 2-5, the overflow-digit cases and the true-division / tensorize modes on 2^64-torus ciphertexts with
    EncryptedMatrixInversion(q_bits=65, unroll=True) - the wrapper's unrolled torus engine: 42-bit key, k_blind_rotate_lat2u_t64f: decrypted digits == the reference's plaintext QFloat output
    (tests/golden/inverse.json, generated from the reference)."""
    from bmi_amd.main import EncryptedMatrixInversion
    c = pc.golden_inverse(tag)
    emi = EncryptedMatrixInversion(c["n"], None, 2, c["len"], c["ints"], c["true_division"], c["tensorize"], unroll=True, q_bits=QB)
    try:
        emi.keygen()                                # CSPRNG keys
        assert emi.engine.q_bits == QB and emi.engine.bsk_precision == 42 and emi.engine.P.glwe_noise == 2.0 ** -44   # the FFT-route unrolled kernel
        out, wall, depth = pc.timed_inverse(emi, c, warm_up=c["n"] < 8)   # (no warm-up for the long 8x8 run)
        assert out == c["out"], f"circuit failure probability by noise under these parameters: {emi.error_budget['p_fail']:.1e}"
        with capsys.disabled():
            print(f"\ntorus, unrolled key, {tag}: evaluate {wall:.2f} s, {depth} levels, {wall / depth * 1e3:.2f} ms per level")
    finally:
        emi.engine.close()
