"""GPU tests of the two-ciphertexts-per-workgroup UNROLLED blind rotation on the 2^64 torus at N = 2048 (k_blind_rotate_wu2_t64f,
csrc/bmi_kernels_t64wu2.hip): preset_params("secure128_torus") + bmi_set_bsk_unroll(ctx, 2), batches beyond 256 under auto dispatch
and every batch with kernel variant 1 / 3 pinned.  The kernel gives the words of k_blind_rotate_wu_t64f by construction, so the
tests name the kernel they ran through bmi_rotation_kernel (the library's own dispatch) and hold every word to
oracle/tfhe_oracle.c ora_blind_rotate_extract_unrolled on the exported keys: rows paired so that the two ciphertexts of a workgroup
take different steps (wide_unrolled2_cases.paired_rows), an odd batch, both level counts, an even and an odd n; the accumulator form
and shared rotations; the rounding distance of the limb sums; whole bootstraps and the golden 2x2 inverse served by evaluate_many at
the real n = 742."""
import os
import sys

import numpy as np
import pytest

import pbs_cases as pc
import wide_unrolled_cases as wu
import wide_unrolled2_cases as w2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import fft_bound  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x5EED + 260
CFG = pc.UnrolledConfig(q_bits=65, precision=wu.PREC, grid_mask=wu.GRID_MASK, oracle_rows=6, margin_hook=True)
# (n, l): 16 = 8 pairs; 17: odd, the last pair is completed by a' = 0 (nine steps: one past the re-centring); l = 2: the other
# instantiation; 24 = 12 pairs: two ciphertexts of one workgroup past eight steps with different counts
SHAPES = [(16, 3), (17, 3), (16, 2), (17, 2), (24, 3)]
COUNT = 259      # 129 full workgroups and one with a single live ciphertext


@pytest.fixture(scope="module", params=SHAPES, ids=[f"n{n}_l{l}" for n, l in SHAPES])
def short(request):
    n, l = request.param
    e = wu.engine(SEED + n + 100 * l, n=n, bs_levels=l)
    yield e
    e.close()


@pytest.fixture(scope="module")
def short16():
    e = wu.engine(SEED + 5, n=16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def real():
    """the preset at its real n = 742"""
    e = wu.engine(SEED)
    yield e
    e.close()


def test_dispatch_names_the_kernel_that_runs(short16):
    """bmi_rotation_kernel answers from the function that dispatches: unrolled secure128_torus switches to two ciphertexts per
    workgroup beyond 256 as the plain key does; 2 pins the one-ciphertext kernels, 1 and 3 the two-ciphertext ones; the default set
    names its latency and wave-pair kernels"""
    from bmi_amd import tfhe
    eng = short16
    assert CFG.q_bits == eng.q_bits
    assert eng.rotation_kernel(1) == eng.rotation_kernel(256) == w2.WU and eng.rotation_kernel(257) == eng.rotation_kernel(8192) == w2.WU2
    with pc.pinned_variant(eng, 2):
        assert eng.rotation_kernel(1000) == w2.WU
    for v in (1, 3):
        with pc.pinned_variant(eng, v):
            assert eng.rotation_kernel(1) == w2.WU2
    assert eng.key_bytes()[0] == eng.export_bsk_unrolled().size * 16      # one copy of the unrolled key serves both kernels
    plain = tfhe.Engine(tfhe.preset_params(wu.PRESET, n=16))
    try:
        plain.keygen(SEED)
        assert plain.rotation_kernel(256) == "k_blind_rotate_w_t64f" and plain.rotation_kernel(257) == "k_blind_rotate_w2_t64f"
        with pc.pinned_variant(plain, 2):
            assert plain.rotation_kernel(1000) == "k_blind_rotate_w_t64f"
        for v in (1, 3):
            with pc.pinned_variant(plain, v):
                assert plain.rotation_kernel(1) == "k_blind_rotate_w2_t64f"
    finally:
        plain.close()
    ev = tfhe.Engine(tfhe.preset_params(wu.PRESET, n=16))
    try:
        ev.set_bsk_unroll(2)             # the mode without its key: no kernel would run
        with pytest.raises(tfhe.BmiError):
            ev.rotation_kernel(1)
    finally:
        ev.close()
    dflt = tfhe.Engine(tfhe.default_params(n=16))
    try:
        dflt.keygen(SEED)
        assert dflt.rotation_kernel(1) == "k_blind_rotate_lat_t64f" and dflt.rotation_kernel(8192) == "k_blind_rotate_t64f"
    finally:
        dflt.close()


def test_every_word_against_the_oracle(short):
    """259 rows under auto dispatch, every one against the oracle; the same rows on the one-ciphertext kernel; 2 and 5 rows (and a
    window that pairs the rows the other way round) with variant 1 pinned"""
    eng = short
    rng = np.random.default_rng(1000 * eng.P.n + 10 * eng.P.bs_levels)
    small, ids, sel = w2.batch(eng, rng, COUNT)
    if eng.P.n == 24:      # both past the re-centring after eight steps, by different counts
        live = [int(w2.pair_is_live(small[r]).sum()) for r in (14, 15)]
        assert live == [12, 10]
    assert eng.rotation_kernel(COUNT) == w2.WU2
    got = eng.blind_rotate_host(small, ids[sel])
    assert got.shape == (COUNT, 2049) and not (got & np.uint64(wu.GRID_MASK)).any()    # the accumulator lives on the key's grid
    with pc.oracle_for(eng, unrolled=True) as o:
        want = wu.oracle_rotation(eng, o, small, ids, sel, np.arange(COUNT))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"rows {bad[:20].tolist()} of {COUNT} differ from the oracle"
    # rows 0 and 9 take no step: the extraction of the test polynomial, beside partners that rotate
    for r in (0, 9):
        tv = eng.lut_get(ids[sel[r]])
        assert got[r, 2048] == tv[0] and not got[r, :2048].any()
    with pc.pinned_variant(eng, 2):
        assert eng.rotation_kernel(COUNT) == w2.WU
        assert np.array_equal(eng.blind_rotate_host(small, ids[sel]), want)
    with pc.pinned_variant(eng, 1):
        for lo, cnt in ((0, 5), (0, 2), (8, 2), (10, 2), (12, 2), (14, 2), (9, 5), (11, 5)):
            assert eng.rotation_kernel(cnt) == w2.WU2
            assert np.array_equal(eng.blind_rotate_host(small[lo:lo + cnt], ids[sel[lo:lo + cnt]]), want[lo:lo + cnt]), (lo, cnt)


def test_whole_pbs_at_the_real_n(real):
    """258 encryptions at n = 742 through keyswitch and the two-ciphertext kernel: every output decrypts, sampled rows equal the
    oracle's bootstrap"""
    assert real.rotation_kernel(258) == w2.WU2
    pc.check_unrolled_pbs_every_batch_size(real, CFG, 258)


def test_accumulator_form(short16):
    """blind_rotate_glwe_host of 259 rows: its extraction is blind_rotate_host, its 2N words those of the one-ciphertext kernel"""
    eng = short16
    rng = np.random.default_rng(401)
    small, ids, sel = w2.batch(eng, rng, COUNT)
    glwe = eng.blind_rotate_glwe_host(small, ids[sel])
    assert glwe.shape == (COUNT, 2 * 2048)
    got = eng.blind_rotate_host(small, ids[sel])
    assert np.array_equal(glwe[:, 0], got[:, 0]) and np.array_equal(glwe[:, 2048], got[:, 2048])
    assert np.array_equal(np.uint64(0) - glwe[:, 2047:0:-1], got[:, 1:2048])
    with pc.pinned_variant(eng, 2):
        assert np.array_equal(eng.blind_rotate_glwe_host(small, ids[sel]), glwe)
    with pc.pinned_variant(eng, 1):      # a batch of one: the padding copy writes nothing
        assert np.array_equal(eng.blind_rotate_glwe_host(small[14:15], ids[sel[14:15]]), glwe[14:15])


def test_shared_rotations_of_257_groups_at_the_real_n(real):
    """257 groups of three tables on one rotation each (the accumulator form of the two-ciphertext kernel): every output decrypts,
    word for word the chain of host forms"""
    eng = real
    rng = np.random.default_rng(34)
    dl = eng.delta_log()
    groups = 257
    assert eng.rotation_kernel(groups) == w2.WU2
    msgs = rng.integers(-8, 8, groups)
    ts = [(rng.integers(-8, 8, 16), dl), (np.array([1] * 8 + [-1] * 8), dl - 1), (np.arange(-8, 8), dl)]
    ids = np.array([eng.lut_register(t, 4, s) for t, s in ts], np.uint32)
    base = eng.lut_register_base(dl - 1)
    ct = eng.encrypt(msgs, dl)
    gp = np.arange(groups + 1) * 3
    gbase, lut_ids = np.full(groups, base, np.uint32), np.tile(ids, groups)
    out = eng.pbs_shared_host(ct, gp, gbase, lut_ids)
    glwe = eng.blind_rotate_glwe_host(eng.keyswitch_host(ct), gbase)
    assert np.array_equal(out, eng.glwe_lookup_host(glwe, gp, gbase, lut_ids))
    out = out.reshape(groups, 3, -1)
    for j, (t, s) in enumerate(ts):
        assert np.array_equal(eng.decrypt(np.ascontiguousarray(out[:, j]), s), t[msgs + 8]), j


def test_rounding_margin_of_the_limb_sums(short16):
    """bmi_fft_margin_host measures the kernel that runs the batch: 258 rows of uniformly random words (digits at their full range)
    at n = 16 stay below the a-priori bound that certifies the rounding (tools/fft_bound.py: 0.38 < 1/2)"""
    eng = short16
    bound = fft_bound.unrolled_limb_sum_bound(11, 3, 10, 20)
    assert bound < 0.5
    rng = np.random.default_rng(12)
    lid = eng.lut_register(rng.integers(-8, 8, 16), 4, eng.delta_log())
    ids = np.full(258, lid, np.uint32)
    rnd = pc.uniform_words(rng, (258, eng.P.small))
    assert eng.rotation_kernel(258) == w2.WU2
    out, dist = eng.fft_margin_host(rnd, ids)
    print(f"\nN = 2048 unrolled two-ciphertext kernel: largest distance from an integer before rounding 2^{np.log2(max(dist, 1e-300)):.1f}")
    assert 0.0 < dist < bound, dist
    assert np.array_equal(out, eng.blind_rotate_host(rnd, ids))
    with pc.pinned_variant(eng, 2):
        assert np.array_equal(out, eng.blind_rotate_host(rnd, ids))


def test_evaluate_many_serves_the_golden_2x2_on_the_two_ciphertext_kernel():
    """EncryptedMatrixInversion(params="secure128_torus", unroll=True).evaluate_many of three encryptions of the golden 2x2: every
    replica decrypts to the reference's digits, and the widest level runs on k_blind_rotate_wu2_t64f"""
    from bmi_amd.main import EncryptedMatrixInversion
    c = pc.golden_inverse("baseline_n2_len20_ints8")
    emi = EncryptedMatrixInversion(c["n"], None, 2, c["len"], c["ints"], False, False, params=wu.PRESET, unroll=True)
    emi.keygen(SEED + 1)
    try:
        eng = emi.engine
        assert eng.unroll == 2 and eng.bsk_precision == wu.PREC and eng.P.n == 742
        M = np.array(c["M"]).reshape(c["n"], c["n"])
        q, s = emi.quantize(M)
        res = emi.evaluate_many([emi.encrypt(q, s) for _ in range(3)])
        assert res.shape[0] == 3
        for b in range(3):
            assert emi.decrypt(res[b]).tolist() == c["out"], b
        widest = max(width for width, *_ in emi._executor(3).levels)
        assert eng.rotation_kernel(widest) == w2.WU2, widest
    finally:
        emi.engine.close()
