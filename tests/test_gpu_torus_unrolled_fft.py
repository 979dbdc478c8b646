"""GPU parity tests of the UNROLLED blind rotation on the 2^64 torus through the FLOATING-POINT transform
(k_blind_rotate_lat2u_t64f, csrc/bmi_kernels_t64fu.hip): bmi_set_bsk_precision(ctx, 42) + bmi_set_bsk_unroll(ctx, 2) - two LWE
coefficients per step, the three scaled GGSW products of a step summed per limb as exact integers (below 2^45: the key is stored
at 42 bits = two 21-bit limbs so that the six-times larger sums stay inside the transform's certified range).  Bit for bit against
oracle/tfhe_oracle.c ora_blind_rotate_extract_unrolled (integer arithmetic: coefficient-domain rotation, Goldilocks transforms of
the key's 32-bit halves) on the same rounded keys; the rounding distance of the limb sums; output noise on the formula; BASELINE
configs 2-4 through EncryptedMatrixInversion(q_bits=65, unroll=True) against the reference's golden digits."""
import numpy as np
import pytest

import pbs_cases as pc

pytestmark = pytest.mark.gpu

SEED = 0x5EED
QB = 65
PREC = 42
# the 42-bit key: every key and accumulator word on the 2^22 grid; 6 random rows to the oracle beside the fixed ones; f64 accumulator
CFG = pc.UnrolledConfig(q_bits=QB, precision=PREC, grid_mask=(1 << 22) - 1, oracle_rows=6, margin_hook=True)


def _engine(seed=SEED, **kw):
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=QB, **kw))
    e.set_bsk_unroll(2)           # selects the 42-bit key and the FFT route by itself ...
    assert e.bsk_precision == PREC
    e.set_bsk_precision(PREC)     # ... and the explicit choice is accepted in unrolled mode
    e.keygen(seed)
    return e


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


def test_keys_are_the_oracles_rounded_to_42_bits_and_plain_pbs_is_refused(eng):
    from bmi_amd import tfhe
    pc.check_unrolled_seeded_keys(eng, CFG, SEED)
    # the 42-bit key at base 2^10 exists for the unrolled kernel only: a context in plain mode refuses the precision, and one that
    # leaves the unrolled mode with the precision pinned refuses to bootstrap
    e = tfhe.Engine(tfhe.default_params(q_bits=QB))
    try:
        with pytest.raises(tfhe.BmiError):
            e.set_bsk_precision(PREC)
        e.set_bsk_unroll(2)
        e.set_bsk_precision(PREC)
        e.set_bsk_unroll(1)
        e.keygen(SEED)
        lid = e.lut_register(np.arange(-8, 8), 4, e.delta_log())
        with pytest.raises(tfhe.BmiError):
            e.blind_rotate_host(np.zeros((1, e.P.small), np.uint64), np.full(1, lid, np.uint32))
    finally:
        e.close()


@pytest.mark.parametrize("count", [1, 2, 5, 256, 257, 300, 701])
def test_two_ciphertexts_per_workgroup_give_the_same_words(eng, count):
    """the throughput form (k_blind_rotate_tp2u_t64f: two ciphertexts per workgroup sharing every key word in registers; what auto
    runs beyond 256 ciphertexts) against the one-ciphertext form, word for word, for even and odd batches and adversarial rows"""
    rng = np.random.default_rng(1000 + count)
    lid = eng.lut_register(rng.integers(-8, 8, 16), 4, eng.delta_log())
    ids = np.full(count, lid, np.uint32)
    small = pc.uniform_words(rng, (count, eng.P.small))
    small[0] = 0                                   # a ciphertext whose every step is skipped beside one that takes them all
    if count > 2:
        small[2, ::2] = 0
        small[count - 1, 14::16] = 0
        small[count - 1, 15::16] = 0
    with pc.pinned_variant(eng, 2):
        one = eng.blind_rotate_host(small, ids)
    with pc.pinned_variant(eng, 1):
        two = eng.blind_rotate_host(small, ids)
    assert np.array_equal(one, two)
    assert np.array_equal(eng.blind_rotate_host(small, ids), one)     # auto: whichever it picked


@pytest.mark.parametrize("count", [1, 5, 300, 700])
def test_unrolled_fft_pbs_bit_exact_every_batch_size(eng, count):
    pc.check_unrolled_pbs_every_batch_size(eng, CFG, count)


def test_unrolled_fft_blind_rotation_extreme_inputs_and_rounding_margin(eng):
    """arbitrary small-key words (zeros, maxima, pair sums that wrap 2N, skipped steps) straight into the blind rotation; and the
    largest distance of a limb sum from the integer it is rounded to over 512 bootstraps of uniformly random words (digits at
    their full range): far below 1/2 (a-priori bound 0.29)"""
    rng, lid = pc.check_unrolled_extreme_inputs(eng, CFG, rows=10)
    count = 512
    rnd = pc.uniform_words(rng, (count, eng.P.n + 1))
    out, dist = eng.fft_margin_host(rnd, np.full(count, lid, np.uint32))
    print(f"\nunrolled FFT kernel: largest distance from an integer before rounding 2^{np.log2(max(dist, 1e-300)):.1f}")
    assert 0.0 < dist < 2.0 ** -7, dist
    assert np.array_equal(out, eng.blind_rotate_host(rnd, np.full(count, lid, np.uint32)))


@pytest.mark.parametrize("kw", [dict(n=629), dict(n=1024), dict(bs_levels=2), dict(n=1)], ids=["odd_n", "n1024", "l2", "n1"])
def test_unrolled_fft_other_shapes_bit_exact(kw):
    e = _engine(seed=77, **kw)
    try:
        pc.check_unrolled_other_shape(e, decrypts=kw.get("n") != 1)   # (one coefficient cannot hold a message's phase)
    finally:
        e.close()


def test_two_level_forms_bit_exact_at_an_odd_n_and_batch():
    """(l, Bg) = (2, 2^10) is otherwise bootstrapped by k_blind_rotate_lat2u_t64f in the extracted form only: here the other two-level
    instantiations - tp2u plain and GLWE, lat2u STATS and GLWE - each named by the library's dispatch.  n = 3 (an odd n: the last
    pair is half empty), a batch of 3 (an odd batch: tp2u's last workgroup runs the padding copy), uniformly random words, variant
    1 (tp2u) and variant 2 (lat2u) pinned.  The extracted words against the oracle's unrolled mode; all 2N words of the accumulator
    against the exact numpy rotation of tests/test_gpu_shared_rotation_wide_unrolled.py, itself pinned to the oracle through the
    extraction; the rounding distance under the 2^-7 the l = 3 kernel is held to (its sums are larger)."""
    from test_gpu_shared_rotation import extract
    from test_gpu_shared_rotation_wide_unrolled import numpy_unrolled_blind_rotation
    e = _engine(seed=78, n=3, bs_levels=2)
    try:
        rng = np.random.default_rng(19)
        lid = e.lut_register(rng.integers(-8, 8, 16), 4, e.delta_log())
        tv = e.lut_get(lid)
        small = pc.uniform_words(rng, (3, e.P.small))
        ids = np.full(3, lid, np.uint32)
        with pc.oracle_for(e, unrolled=True) as o:
            want = o.ctx.blind_rotate(small, tv[None, :], np.zeros(3, np.uint32), unrolled=True)
        bsk3 = e.export_bsk_unrolled()
        ref = np.stack([numpy_unrolled_blind_rotation(e.P, bsk3, row, tv) for row in small])
        assert np.array_equal(extract(ref, e.P.N), want)
        for variant, name in ((1, "k_blind_rotate_tp2u_t64f"), (2, "k_blind_rotate_lat2u_t64f")):
            with pc.pinned_variant(e, variant):
                assert e.rotation_kernel(3) == name
                assert np.array_equal(e.blind_rotate_host(small, ids), want)
                assert np.array_equal(e.blind_rotate_glwe_host(small, ids), ref)
        out, dist = e.fft_margin_host(small, ids)      # the STATS form of lat2u, whatever the batch
        assert np.array_equal(out, want) and 0.0 < dist < 2.0 ** -7, dist
    finally:
        e.close()


def test_unrolled_fft_output_noise_on_the_formula_and_timing(eng, capsys):
    """2,048 bootstraps: the output variance against the unrolled CGGI formula with the 42-bit key's effective noise
    (bmi_amd/error_budget.pbs_output_variance with the exact key weights); latency of 1 and of a full round of 256"""
    import torch
    from bmi_amd import error_budget
    rng = np.random.default_rng(5)
    dl = eng.delta_log()
    table = rng.integers(-8, 8, 16)
    lid = eng.lut_register(table, 4, dl)
    count = 2048
    msgs = rng.integers(-8, 8, count)
    ct = eng.encrypt(msgs, dl)
    out = eng.pbs_host(ct, np.full(count, lid, np.uint32))
    want = table[msgs + 8]
    assert np.array_equal(eng.decrypt(out, dl), want)
    err = pc.centred_error(eng.phase(out), want, dl, 1 << 64)
    P = eng.P
    analytic = pc.unrolled_torus_variance(eng)
    ratio = float(np.var(err)) / analytic
    model = error_budget.pbs_output_variance(P, PREC, unroll=True)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    small = eng.keyswitch_host(ct[:256])
    d_small = torch.from_numpy(small.view(np.int64)).to(dev)
    d_ids = torch.full((256,), lid, dtype=torch.int32, device=dev)
    d_out = torch.empty((256, P.N + 1), dtype=torch.int64, device=dev)
    t = {}
    for cnt in (1, 256):
        eng.blind_rotate(d_small, d_ids, cnt, d_out, s)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(5):
            eng.blind_rotate(d_small, d_ids, cnt, d_out, s)
        b.record()
        torch.cuda.synchronize()
        t[cnt] = a.elapsed_time(b) / 5
    with capsys.disabled():
        print(f"\nunrolled FFT kernel (42-bit key): output log2 std {0.5 * np.log2(np.var(err)):.2f} (formula {0.5 * np.log2(analytic):.2f}, variance "
              f"ratio {ratio:.3f}; error-budget model {0.5 * np.log2(model):.2f}); blind rotation {t[1]:.2f} ms for 1, {t[256]:.2f} ms for 256")
    assert 0.88 < ratio < 1.12 and abs(0.5 * np.log2(model / analytic)) < 0.2


@pytest.mark.parametrize("tag", ["baseline_n2_len20_ints8", "baseline_n3_len30_ints12", "baseline_n4_len40_ints16"])
def test_encrypted_inverse_with_the_unrolled_fft_kernel_matches_reference_golden(eng, tag, capsys):
    from bmi_amd.main import EncryptedMatrixInversion
    c = pc.golden_inverse(tag)
    emi = EncryptedMatrixInversion(c["n"], None, 2, c["len"], c["ints"], False, False, engine=eng, unroll=True)
    out, wall, depth = pc.timed_inverse(emi, c, warm_up=True)
    assert out == c["out"], f"circuit failure probability by noise under these parameters: {emi.error_budget['p_fail']:.1e}"
    with capsys.disabled():
        print(f"\ntorus, unrolled FFT kernel, {tag}: evaluate {wall:.2f} s, {depth} levels, {wall / depth * 1e3:.2f} ms per level, "
              f"p_fail {emi.error_budget['p_fail']:.1e}")
