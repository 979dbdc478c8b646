"""GPU parity tests of the UNROLLED blind rotation on the 2^64 torus at N = 2048 (k_blind_rotate_wu_t64f,
csrc/bmi_kernels_t64wu.hip): preset_params("secure128_torus") + bmi_set_bsk_unroll(ctx, 2) - two LWE coefficients per step, the
three scaled GGSW products of a step summed per limb as exact integers (below 2^45: the key is stored at 40 bits = two 20-bit
limbs so that the six-times larger sums stay inside the transform's certified range, tools/fft_bound.py).  Bit for bit against
oracle/tfhe_oracle.c ora_blind_rotate_extract_unrolled on the same rounded keys, on short LWE sides; the accumulator form and a
group of tables sharing one rotation; the rounding distance of the limb sums; at the real n = 742 the output noise on the formula
and the golden 2x2 inverse through EncryptedMatrixInversion(params="secure128_torus", unroll=True)."""
import numpy as np
import pytest

import pbs_cases as pc
import wide_unrolled_cases as wu

pytestmark = pytest.mark.gpu

SEED = 0x5EED + 240
# (n, l): 16 = 8 pairs, the words are stored right after the re-centre of the 8th step taken; 24: four steps after one; 15: odd,
# the last pair is half empty; 1: one half-empty pair; l = 2: the other instantiation
SHAPES = [(16, 3), (24, 3), (15, 3), (1, 3), (16, 2)]


@pytest.fixture(scope="module", params=SHAPES, ids=[f"n{n}_l{l}" for n, l in SHAPES])
def short(request):
    n, l = request.param
    e = wu.engine(SEED + n + 100 * l, n=n, bs_levels=l)
    yield e
    e.close()


@pytest.fixture(scope="module", params=[16, 15], ids=["n16", "n15"])
def short3(request):
    e = wu.engine(SEED + 7 + request.param, n=request.param)
    yield e
    e.close()


@pytest.fixture(scope="module")
def real():
    """the preset at its real n = 742"""
    e = wu.engine(SEED)
    yield e
    e.close()


def test_unrolling_selects_the_40_bit_key_and_what_stays_refused():
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.preset_params(wu.PRESET, n=16))
    try:
        assert e.bsk_precision == 46
        with pytest.raises(tfhe.BmiError):
            e.set_bsk_precision(40)          # plain mode: no kernel at 40 bits
        e.set_bsk_unroll(2)
        assert e.bsk_precision == 40         # the precision nobody chose follows the mode
        e.set_bsk_precision(40)              # ... and the explicit choice is accepted in unrolled mode
        for bits in (64, 48, 46, 44, 42):
            with pytest.raises(tfhe.BmiError, match="40"):
                e.set_bsk_precision(bits)
    finally:
        e.close()
    e = tfhe.Engine(tfhe.preset_params(wu.PRESET, n=16))
    try:
        e.set_bsk_unroll(2)
        e.set_bsk_unroll(1)
        assert e.bsk_precision == 46         # back to the set's default
    finally:
        e.close()
    e = tfhe.Engine(tfhe.preset_params("secure128_torus_wide", n=16))
    try:
        with pytest.raises(tfhe.BmiError, match="4096"):
            e.set_bsk_unroll(2)
    finally:
        e.close()


def test_seeded_keys_are_the_oracles_rounded_to_the_2_24_grid(short3):
    from bmi_amd import tfhe
    from oracle import tfhe_oracle as to
    eng = short3
    to.set_field(eng.q_bits)
    P = to.Params(**{f: getattr(eng.P, f) for f, _ in tfhe.Params._fields_})
    seed = SEED + 7 + eng.P.n
    K = to.keygen(P, seed)
    sk_small, sk_big, bsk, ksk = eng.export_keys()
    assert np.array_equal(K.sk_small, sk_small) and np.array_equal(K.sk_big, sk_big) and np.array_equal(K.ksk, ksk)
    assert np.array_equal(to.round_key(K.bsk, wu.PREC), bsk) and not np.array_equal(K.bsk, bsk)
    bsk3 = eng.export_bsk_unrolled()
    assert bsk3.shape == ((eng.P.n + 1) // 2, 3, 2 * eng.P.bs_levels, 2, 2048)
    assert np.array_equal(to.round_key(to.keygen_bsk_unrolled(P, seed, K.sk_small, K.sk_big), wu.PREC), bsk3)
    assert not (bsk3 & np.uint64(wu.GRID_MASK)).any() and not (bsk & np.uint64(wu.GRID_MASK)).any()


def test_an_evaluation_only_context_imports_both_keys_and_gives_the_same_words(short3):
    from bmi_amd import tfhe
    eng = short3
    rng = np.random.default_rng(5)
    dl = eng.delta_log()
    table = rng.integers(-8, 8, 16)
    small = wu.edge_rows(rng, eng.P.small)
    got = eng.blind_rotate_host(small, np.full(9, eng.lut_register(table, 4, dl), np.uint32))
    ev = tfhe.Engine(tfhe.preset_params(wu.PRESET, n=eng.P.n))
    try:
        ev.set_bsk_unroll(2)
        _, _, bsk, ksk = eng.export_keys(secret=False)
        ev.import_keys(None, None, bsk, ksk)
        ids = np.full(9, ev.lut_register(table, 4, dl), np.uint32)
        with pytest.raises(tfhe.BmiError):      # unrolling selected, no unrolled key yet
            ev.blind_rotate_host(small, ids)
        ev.import_bsk_unrolled(eng.export_bsk_unrolled())
        assert np.array_equal(ev.blind_rotate_host(small, ids), got)
        assert np.array_equal(ev.export_bsk_unrolled(), eng.export_bsk_unrolled())
        # the device copy of the unrolled key: two limbs of doubles per word (no plain key copy at 40 bits)
        assert ev.key_bytes()[0] == eng.key_bytes()[0] == eng.export_bsk_unrolled().size * 16
    finally:
        ev.close()


@pytest.mark.parametrize("count", [1, 5, 257])
def test_blind_rotation_bit_exact_against_the_oracle(short, count):
    """word for word against ora_blind_rotate_extract_unrolled on the exported keys: every row of the small batches, the edge
    rows, the last row and six random ones of 257 (more workgroups than compute units)"""
    eng = short
    rng = np.random.default_rng(1000 * eng.P.n + 10 * eng.P.bs_levels + count)
    small, ids, sel = wu.batch(eng, rng, count)
    got = eng.blind_rotate_host(small, ids[sel])
    assert got.shape == (count, 2049) and not (got & np.uint64(wu.GRID_MASK)).any()    # the accumulator lives on the key's grid
    pick = pc.sample_rows(count, [0, 1, 2, 3, 4, 5, 6, 7, 8, 255, 256], rng, 6)
    with pc.oracle_for(eng, unrolled=True) as o:
        assert np.array_equal(got[pick], wu.oracle_rotation(eng, o, small, ids, sel, pick))
    if count > 2:      # rows 1 and 2 take no step: the extraction of the test polynomial
        tv = eng.lut_get(ids[sel[1]])
        assert got[1, 2048] == tv[0] and not got[1, :2048].any()


def test_edge_rows_one_by_one_against_the_oracle(short3):
    """every edge row alone in its batch (a ciphertext's words never depend on the batch it travelled in)"""
    eng = short3
    rng = np.random.default_rng(77)
    small, ids, sel = wu.batch(eng, rng, 9)
    batch = eng.blind_rotate_host(small, ids[sel])
    with pc.oracle_for(eng, unrolled=True) as o:
        assert np.array_equal(batch, wu.oracle_rotation(eng, o, small, ids, sel, np.arange(9)))
    for r in range(9):
        assert np.array_equal(eng.blind_rotate_host(small[r:r + 1], ids[sel[r:r + 1]]), batch[r:r + 1]), r


def test_kernel_variants_0_1_2_give_the_same_words(short3):
    eng = short3
    rng = np.random.default_rng(31)
    small, ids, sel = wu.batch(eng, rng, 300)
    auto = eng.blind_rotate_host(small, ids[sel])
    for v in (1, 2):
        with pc.pinned_variant(eng, v):
            assert np.array_equal(eng.blind_rotate_host(small, ids[sel]), auto), v


def test_rounding_margin_of_the_limb_sums():
    """the largest distance of a limb sum from the integer it is rounded to over 512 bootstraps of uniformly random words (digits
    at their full range) at n = 16: a tripwire far below 1/2 (the certificate is the a-priori bound 0.38, tools/fft_bound.py)"""
    eng = wu.engine(SEED + 9, n=16)
    try:
        rng = np.random.default_rng(12)
        lid = eng.lut_register(rng.integers(-8, 8, 16), 4, eng.delta_log())
        ids = np.full(512, lid, np.uint32)
        rnd = pc.uniform_words(rng, (512, eng.P.small))
        out, dist = eng.fft_margin_host(rnd, ids)
        print(f"\nN = 2048 unrolled kernel: largest distance from an integer before rounding 2^{np.log2(max(dist, 1e-300)):.1f}")
        assert 0.0 < dist < 2.0 ** -7, dist
        assert np.array_equal(out, eng.blind_rotate_host(rnd, ids))
    finally:
        eng.close()


@pytest.mark.parametrize("count", [1, 5, 257])
def test_accumulator_form_extracts_to_the_plain_rotation(short3, count):
    eng = short3
    rng = np.random.default_rng(400 + count)
    small, ids, sel = wu.batch(eng, rng, count)
    glwe = eng.blind_rotate_glwe_host(small, ids[sel])
    assert glwe.shape == (count, 2 * 2048)
    got = eng.blind_rotate_host(small, ids[sel])
    assert np.array_equal(glwe[:, 0], got[:, 0]) and np.array_equal(glwe[:, 2048], got[:, 2048])
    assert np.array_equal(np.uint64(0) - glwe[:, 2047:0:-1], got[:, 1:2048])


def test_base_polynomials_follow_the_40_bit_grid(short3):
    from bmi_amd import tfhe
    with pytest.raises(tfhe.BmiError, match="grid"):
        short3.lut_register_base(24)
    short3.lut_register_base(25)


def test_a_group_of_four_tables_shares_one_rotation_for_every_message(real):
    """four 4-bit tables, one of them at half scale, on the base polynomial of the finer unit, through pbs_shared_host: every
    message four times, every output decrypts, word for word the chain of host forms"""
    eng = real
    rng = np.random.default_rng(33)
    dl = eng.delta_log()
    msgs = np.tile(np.arange(-8, 8), 4)
    half = np.array([1] * 8 + [-1] * 8)
    edge = rng.integers(-8, 8, 16)
    edge[0] = edge[15] = -8
    ts = [(rng.integers(-8, 8, 16), dl), (half, dl - 1), (np.arange(-8, 8), dl), (edge, dl)]
    ids = np.array([eng.lut_register(t, 4, s) for t, s in ts], np.uint32)
    base = eng.lut_register_base(dl - 1)
    ct = eng.encrypt(msgs, dl)
    gp = np.arange(msgs.size + 1) * 4
    gbase, lut_ids = np.full(msgs.size, base, np.uint32), np.tile(ids, msgs.size)
    out = eng.pbs_shared_host(ct, gp, gbase, lut_ids)
    glwe = eng.blind_rotate_glwe_host(eng.keyswitch_host(ct), gbase)
    assert np.array_equal(out, eng.glwe_lookup_host(glwe, gp, gbase, lut_ids))
    out = out.reshape(msgs.size, 4, -1)
    for j, (t, s) in enumerate(ts):
        assert np.array_equal(eng.decrypt(np.ascontiguousarray(out[:, j]), s), t[msgs + 8]), j


def test_output_noise_on_the_formula_and_timing(real, capsys):
    """2,048 bootstraps of a random 4-bit table at n = 742: all decrypt; the output variance against the unrolled CGGI formula
    with the 40-bit key's effective noise and this key's exact weights (pbs_cases.unrolled_torus_variance) in the band the N = 1024
    test holds; the error budget's model (average weights) within 0.2 bits of it; blind-rotation time of 1 and of 256 by events"""
    import torch
    from bmi_amd import error_budget
    eng = real
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
    model = error_budget.pbs_output_variance(P, wu.PREC, unroll=True)
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
        print(f"\nN = 2048 unrolled kernel (40-bit key): output log2 std {0.5 * np.log2(np.var(err)):.2f} (formula {0.5 * np.log2(analytic):.2f}, "
              f"variance ratio {ratio:.3f}; error-budget model {0.5 * np.log2(model):.2f}); blind rotation {t[1]:.2f} ms for 1, "
              f"{t[256]:.2f} ms for 256")
    assert 0.88 < ratio < 1.12 and abs(0.5 * np.log2(model / analytic)) < 0.2


def test_encrypted_inverse_on_secure128_torus_with_the_unrolled_key_matches_reference_golden(capsys):
    """EncryptedMatrixInversion(params="secure128_torus", unroll=True) builds the engine itself (the 40-bit key); the golden 2x2:
    decrypted digits == the reference's plaintext QFloat output; the same with shared rotations on that engine"""
    from bmi_amd.main import EncryptedMatrixInversion
    c = pc.golden_inverse("baseline_n2_len20_ints8")
    emi = EncryptedMatrixInversion(c["n"], None, 2, c["len"], c["ints"], False, False, params=wu.PRESET, unroll=True)
    emi.keygen(SEED + 1)
    try:
        eng = emi.engine
        assert eng.unroll == 2 and eng.bsk_precision == wu.PREC and eng.P.N == 2048 and eng.P.n == 742
        out, wall, depth = pc.timed_inverse(emi, c, warm_up=False)
        assert out == c["out"], f"circuit failure probability by noise under these parameters: {emi.error_budget['p_fail']:.1e}"
        sh = EncryptedMatrixInversion(c["n"], None, 2, c["len"], c["ints"], False, False, engine=eng, unroll=True, share_rotations=True)
        out2, wall2, _ = pc.timed_inverse(sh, c, warm_up=False)
        ex = sh._executor()
        assert out2 == c["out"] and ex.rotations < ex.lookups
        with capsys.disabled():
            print(f"\nsecure128_torus, unrolled key, 2x2: evaluate {wall:.2f} s, {depth} levels, p_fail {emi.error_budget['p_fail']:.1e}; "
                  f"with shared rotations {wall2:.2f} s, {ex.rotations} rotations for {ex.lookups} look-ups")
    finally:
        emi.engine.close()
