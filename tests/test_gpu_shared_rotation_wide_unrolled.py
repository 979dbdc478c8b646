"""Shared rotations on the two engines that could not hand over their accumulator (tests/test_gpu_shared_rotation.py holds the
other four kernels): N = 4096 (k_blind_rotate_q_t64f, csrc/bmi_kernels_t64q.hip; preset secure128_torus_wide) and the unrolled key
through the floating-point transform (k_blind_rotate_lat2u_t64f and the two-per-workgroup k_blind_rotate_tp2u_t64f,
csrc/bmi_kernels_t64fu.hip; key at 42 bits).

As there: the accumulator entries are held to the oracle-pinned extraction path word for word and, on the words the extraction
does not read, to an exact numpy rotation that is first pinned to the oracle itself - for the unrolled key a numpy statement of
oracle/tfhe_oracle.c ora_blind_rotate_extract_unrolled on the exported unrolled key; then a group of tables end to end and against
the chain of host forms, the noise against the budget's model (error_budget.pbs_output_variance_parts, for the unrolled key its
unroll=True split), and the application: the reference's own 5-bit circuits at N = 4096, the golden inverses on the unrolled key."""
import gzip
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pbs_cases as pc
from test_gpu_shared_rotation import (check_accumulator_extracts_to_the_plain_rotation, check_shared_lookup_noise, extract, negacyclic_dense,
                                      numpy_blind_rotation)

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 0x5EED + 177
WIDE = "secure128_torus_wide"


# ---- engines ---------------------------------------------------------------------------------------------------------------------
def _wide(seed, **kw):
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.preset_params(WIDE, **kw))
    e.keygen(seed)
    return e


def _unrolled(seed, **kw):
    """the default torus set in unrolled mode: the 42-bit key, the floating-point-transform route"""
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=tfhe.TORUS64, **kw))
    e.set_bsk_unroll(2)
    assert e.bsk_precision == 42
    e.keygen(seed)
    return e


@pytest.fixture(scope="module")
def wide():
    e = _wide(SEED)
    yield e
    e.close()


@pytest.fixture(scope="module", params=[3, 2], ids=["l3", "l2"])
def wide16(request):
    """the N = 4096 kernel on a short LWE side (n = 16), both instantiations"""
    e = _wide(SEED + 1, n=16, bs_levels=request.param)
    yield e
    e.close()


@pytest.fixture(scope="module")
def unr():
    e = _unrolled(SEED + 2)
    yield e
    e.close()


@pytest.fixture(scope="module", params=[16, 15])
def unr_short(request):
    """the unrolled kernels on a short LWE side; n = 15: the last pair is completed by a zero"""
    e = _unrolled(SEED + 3, n=request.param)
    yield e
    e.close()


def group_run(eng, msgs, bits, tables_scales, unit):
    """every ciphertext (encrypted at the full scale of `bits`-bit messages) through ONE group of the given (table, scale) list on
    the base polynomial of `unit`: the outputs [len(msgs)][tables][N + 1]; word for word the chain keyswitch_host ->
    blind_rotate_glwe_host -> glwe_lookup_host; every output decrypts to its table's value"""
    h = 1 << (bits - 1)
    ids = np.array([eng.lut_register(t, bits, s) for t, s in tables_scales], np.uint32)
    base = eng.lut_register_base(unit)
    ct = eng.encrypt(msgs, eng.delta_log(bits))
    k = len(tables_scales)
    gp = np.arange(msgs.size + 1) * k
    gbase, lut_ids = np.full(msgs.size, base, np.uint32), np.tile(ids, msgs.size)
    out = eng.pbs_shared_host(ct, gp, gbase, lut_ids)
    glwe = eng.blind_rotate_glwe_host(eng.keyswitch_host(ct), gbase)
    assert np.array_equal(out, eng.glwe_lookup_host(glwe, gp, gbase, lut_ids))
    out = out.reshape(msgs.size, k, -1)
    for j, (t, s) in enumerate(tables_scales):
        assert np.array_equal(eng.decrypt(np.ascontiguousarray(out[:, j]), s), t[msgs + h]), j
    return out


def tables_of(bits, rng):
    """random, identity, sign-like, and the edge table whose neighbouring boxes -2^(p-1) | +2^(p-1) differ by 2^p"""
    h = 1 << (bits - 1)
    edge = rng.integers(-h, h, 2 * h)
    edge[0] = edge[2 * h - 1] = -h
    return [rng.integers(-h, h, 2 * h), np.arange(-h, h), np.array([-3] * h + [3] * h), edge]


# ================================================================ N = 4096 ==========================================================
@pytest.mark.parametrize("count", [1, 5, 300])
def test_accumulator_form_extracts_to_the_plain_rotation_n4096(wide16, count):
    """uniformly random small-key words under pbs_cases.adversarial_rows; 300: more workgroups than compute units"""
    glwe = check_accumulator_extracts_to_the_plain_rotation(wide16, count, 400 + count, keyswitched=False)
    assert glwe.shape == (count, 2 * 4096)


def test_every_word_of_the_accumulator_equals_an_exact_numpy_rotation_n4096():
    """n = 12, a 5-bit table.  Row 0 dense (12 steps: stored after a re-centre and four more steps); row 1 all ones (every exponent
    0, no step: the test polynomial in the body, zero in the mask); row 2 skips steps 1, 4, 7, 10 (8 steps: stored right after a
    re-centre).  The numpy rotation is pinned to the oracle through the extraction, then all 2N words must equal it."""
    e = _wide(SEED + 4, n=12)
    try:
        rng = np.random.default_rng(19)
        N = e.P.N
        lid = e.lut_register(rng.integers(-16, 16, 32), 5, e.delta_log(5))
        tv = e.lut_get(lid)
        small = pc.uniform_words(rng, (3, e.P.small))
        small[1] = np.uint64(0xFFFFFFFFFFFFFFFF)
        small[2, 1::3] = 0
        ids = np.full(3, lid, np.uint32)
        bsk = e.export_keys()[2]
        with ThreadPoolExecutor(3) as pool:      # (numpy's convolution releases the interpreter lock)
            ref = np.stack(list(pool.map(lambda row: numpy_blind_rotation(e.P, bsk, row, tv), small)))
        assert np.array_equal(ref[1, N:], tv) and not ref[1, :N].any()
        with pc.oracle_for(e) as o:
            assert np.array_equal(extract(ref, N), o.ctx.blind_rotate(small, tv[None, :], np.zeros(3, np.uint32)))
        assert np.array_equal(e.blind_rotate_glwe_host(small, ids), ref)
    finally:
        e.close()


def test_every_five_bit_message_through_groups_of_tables_n4096(wide):
    """the full preset: every 5-bit message 8 times through one group of four full-scale tables on the unit 2^dl, and through a
    group with the half-scale -+1 table on the unit 2^(dl - 1)"""
    rng = np.random.default_rng(33)
    dl = wide.delta_log(5)
    msgs = np.tile(np.arange(-16, 16), 8)
    T = tables_of(5, rng)
    group_run(wide, msgs, 5, [(t, dl) for t in T], dl)
    half = np.array([1] * 16 + [-1] * 16)
    group_run(wide, msgs[:64], 5, [(T[1], dl), (half, dl - 1), (T[0], dl), (T[3], dl - 1)], dl - 1)
    floor = 64 - wide.bsk_precision + 1
    assert floor == pc.FLOOR_UNIT[4096] == 21


def test_shared_lookup_noise_against_the_budgets_model_n4096(wide):
    """4,096 shared rotations on the full preset (16 rounds): the measured output variance over |P_f|^2 v_white + |S P_f|^2
    v_carried with this key's exact weights, in the +-15 % band; every output decrypts (check_shared_lookup_noise, unchanged)"""
    ratios = check_shared_lookup_noise(wide)
    print(f"\nsecure128_torus_wide: shared look-up noise over the budget's model {ratios[0]:.3f} (identity), {ratios[1]:.3f} (random)")


@pytest.mark.parametrize("which", ["mul_qfloats", "inverse_2x2_fused"])
def test_reference_five_bit_circuits_with_shared_rotations_n4096(wide, which):
    """the reference's own mul_qfloats 5-bit circuit (88 levels) and its traced, lazily fused 2x2 inverse (303 levels of one 17 ms
    round each: the application is rotation-bound) through Executor(share_rotations=True): the golden vector, one rotation per
    group, and the shared budget below 1e-5"""
    from bmi_amd import error_budget
    from bmi_amd.circuit import Circuit
    from bmi_amd.executor import Executor
    from bmi_amd.shared_rotation import rotation_groups
    dl = wide.delta_log(5)
    if which == "mul_qfloats":
        with gzip.open(os.path.join(G, "ref_own_fhe_tests.json.gz"), "rt") as f:
            case = next(c for c in json.load(f)["cases"] if c["msg_bits"] == 5 and c["function"] == "mul_qfloats")
        vectors = [(r["inputs"], r["outputs"]) for r in case["runs"]]
    else:
        with gzip.open(os.path.join(G, "ref_traced_inverse.json.gz"), "rt") as f:
            case = json.load(f)["cases"][2]
        assert case["name"] == "qfloat_matrix_inverse_2x2_fused"
        vectors = [(v["inputs"], v["expected"]) for v in case["vectors"][:1]]
    c = Circuit.from_dict(case["circuit"])
    assert c.msg_bits == 5
    ex = Executor(c, wide, share_rotations=True)
    for inputs, want in vectors:
        assert list(wide.decrypt(ex.run(wide.encrypt(inputs, dl)), dl)) == want
    assert ex.rotations == rotation_groups(ex.prog).groups < ex.lookups == ex.prog.n_nodes
    rep = error_budget.failure_probability(ex.prog, wide.P, wide.bsk_precision, share_rotations=True)
    print(f"\n{which} on {WIDE} with shared rotations: {ex.lookups} look-ups, {ex.rotations} rotations, p_fail {rep['p_fail']:.1e}")
    assert rep["p_fail"] < 1e-5 and rep["rotations"] == ex.rotations


# ====================================================== the unrolled key, FFT route ==================================================
def unrolled_rows(rng, count, width):
    """the last `count` of pbs_cases.extreme_rows_unrolled's rows with skipped_pairs (seven fixed rows - zeros, maxima, pair sums
    that wrap 2N, pairs that are both zero - then random ones)"""
    return pc.extreme_rows_unrolled(rng, max(count, 7), width, skipped_pairs=True)[-count:] if count < 7 else \
        pc.extreme_rows_unrolled(rng, count, width, skipped_pairs=True)


@pytest.mark.parametrize("count,variant", [(1, 0), (5, 0), (5, 1), (257, 0), (300, 0)])
def test_accumulator_form_extracts_to_the_plain_unrolled_rotation(unr_short, count, variant):
    """1 and 5 under auto dispatch: k_blind_rotate_lat2u_t64f; 257 (the padding copy of an odd batch) and 300 under auto, and 5
    with variant 1 pinned: k_blind_rotate_tp2u_t64f, whose two ciphertexts take different numbers of steps (rows 0 / 1: none
    beside all)"""
    eng = unr_short
    rng = np.random.default_rng(600 + count + variant)
    dl = eng.delta_log()
    ids = np.array([eng.lut_register(rng.integers(-8, 8, 16), 4, dl) for _ in range(3)], np.uint32)
    small = unrolled_rows(rng, count, eng.P.small)
    sel = ids[rng.integers(0, 3, count)]
    with pc.pinned_variant(eng, variant):
        glwe = eng.blind_rotate_glwe_host(small, sel)
        assert glwe.shape == (count, 2 * eng.P.N)
        assert np.array_equal(extract(glwe, eng.P.N), eng.blind_rotate_host(small, sel))


def numpy_unrolled_blind_rotation(P, bsk3, lwe, tv):
    """The unrolled blind rotation of one small ciphertext in u64 wrap-around arithmetic (oracle/tfhe_oracle.c
    ora_blind_rotate_extract_unrolled), returning the whole accumulator [mask N][body N]: per pair (a, a') ONE decomposition of ACC,
    then ACC += sum_j (X^(c_j) - 1) (K3[i][j] [.] ACC) with c = (a + a' mod 2N, a, a'); pairs and keys with c = 0 skipped.
    bsk3: the exported (rounded) unrolled key [pairs][3 keys][2 l rows][2 columns][N], row = component * l + level."""
    N, n, L, BG = P.N, P.n, P.bs_levels, P.bs_base_log
    log2N = P.log_N + 1
    ms = lambda w: int((((int(w) >> (63 - log2N)) + 1) >> 1) & (2 * N - 1))   # noqa: E731  round(w 2N / 2^64), ties up

    def rot(poly, t):
        """X^t poly, t in [0, 2N)"""
        j = (np.arange(N) - t) % (2 * N)
        v = poly[j & (N - 1)]
        return np.where(j & N, np.uint64(0) - v, v)

    with np.errstate(over="ignore"):
        acc = np.zeros((2, N), np.uint64)
        acc[1] = rot(tv, (2 * N - ms(lwe[n])) % (2 * N))
        shift = 64 - L * BG
        for i in range((n + 1) // 2):
            a1, a2 = ms(lwe[2 * i]), (ms(lwe[2 * i + 1]) if 2 * i + 1 < n else 0)
            if (a1 | a2) == 0:
                continue
            digits = []                                                 # [component * L + level]
            for comp in range(2):
                c = acc[comp].view(np.int64)
                r = (c >> shift) + ((c >> (shift - 1)) & 1)             # round half up to the top L BG bits
                d_of = [None] * L
                for lev in range(L - 1, 0, -1):
                    d = r & ((1 << BG) - 1)
                    r = r >> BG
                    up = d >= (1 << (BG - 1))
                    d_of[lev] = np.where(up, d - (1 << BG), d)
                    r = r + up
                d_of[0] = r
                digits += [d.astype(np.int64).view(np.uint64) for d in d_of]
            for j, cj in enumerate(((a1 + a2) % (2 * N), a1, a2)):
                if cj == 0:
                    continue
                for col in range(2):
                    res = np.zeros(N, np.uint64)
                    for row in range(2 * L):
                        res += negacyclic_dense(digits[row], bsk3[i, j, row, col])
                    acc[col] += rot(res, cj) - res
    return acc.reshape(2 * N)


def test_every_word_of_the_unrolled_accumulator_equals_an_exact_numpy_rotation():
    """n = 24: 12 steps, so the dense rows (0 and 4) are stored after a re-centre and four more steps; row 1 all ones (no step: the
    test polynomial itself); row 2 skips every third pair (8 steps: stored right after a re-centre); row 3 has a + a' = 0 mod 2N
    in its second pair (the key of s s' is skipped, the other two are not).  Five rows: the two-per-workgroup kernel runs (0, 1),
    (2, 3) - ciphertexts that take different numbers of steps - and a last workgroup with the padding copy.  The numpy rotation is
    pinned to the oracle's unrolled mode through the extraction; then both kernels' 2N words must equal it."""
    e = _unrolled(SEED + 5, n=24)
    try:
        rng = np.random.default_rng(29)
        N = e.P.N
        lid = e.lut_register(rng.integers(-8, 8, 16), 4, e.delta_log())
        tv = e.lut_get(lid)
        small = pc.uniform_words(rng, (5, e.P.small))
        small[1] = np.uint64(0xFFFFFFFFFFFFFFFF)
        small[2, 4::6] = 0
        small[2, 5:24:6] = 0
        small[3, 2] = np.uint64(5 << 53)                       # a = 5, a' = 2N - 5
        small[3, 3] = np.uint64((2 * N - 5) << 53)
        ids = np.full(5, lid, np.uint32)
        bsk3 = e.export_bsk_unrolled()
        with ThreadPoolExecutor(4) as pool:
            ref = np.stack(list(pool.map(lambda row: numpy_unrolled_blind_rotation(e.P, bsk3, row, tv), small)))
        assert np.array_equal(ref[1, N:], tv) and not ref[1, :N].any()
        with pc.oracle_for(e, unrolled=True) as o:
            assert np.array_equal(extract(ref, N), o.ctx.blind_rotate(small, tv[None, :], np.zeros(5, np.uint32), unrolled=True))
        assert np.array_equal(e.blind_rotate_glwe_host(small, ids), ref)          # auto: k_blind_rotate_lat2u_t64f
        with pc.pinned_variant(e, 1):                                             # k_blind_rotate_tp2u_t64f
            assert np.array_equal(e.blind_rotate_glwe_host(small, ids), ref)
    finally:
        e.close()


def test_every_message_through_groups_of_tables_on_the_unrolled_key(unr):
    """the full set: every 4-bit message 16 times through a group of four full-scale tables on the unit 2^dl and through a group
    with the half-scale -+1 table on the unit 2^(dl - 1); base polynomials exist down to the 42-bit key's grid floor, 2^23"""
    from bmi_amd import tfhe
    rng = np.random.default_rng(35)
    dl = unr.delta_log()
    msgs = np.tile(np.arange(-8, 8), 16)
    T = tables_of(4, rng)
    group_run(unr, msgs, 4, [(t, dl) for t in T], dl)
    group_run(unr, msgs, 4, [(T[1], dl), (T[0], dl), (T[3], dl), (np.array([1] * 8 + [-1] * 8), dl - 1)], dl - 1)
    with pytest.raises(tfhe.BmiError, match="grid"):
        unr.lut_register_base(22)
    assert unr.lut_register_base(23) == unr.lut_register_base(23)


def test_shared_lookup_noise_against_the_unrolled_budgets_model(unr):
    """4,096 rotations shared by the identity table and a random one: the variance of the outputs' centred error over |P_f|^2
    v_white + |S P_f|^2 v_carried of error_budget.pbs_output_variance_parts(unroll=True) with this key's exact pair count and
    weights, in the +-15 % band of the project's noise tests; the parts ARE the unrolled variance the unshared noise test uses
    (pbs_cases.unrolled_torus_variance); every output decrypts"""
    from bmi_amd import error_budget
    from bmi_amd.shared_rotation import key_carried_norm2, sparse_table
    eng = unr
    rng = np.random.default_rng(43)
    dl = eng.delta_log()
    tables = [(np.arange(-8, 8), dl), (rng.integers(-8, 8, 16), dl)]
    msgs = rng.integers(-8, 8, 4096)
    ids = np.array([eng.lut_register(t, 4, s) for t, s in tables], np.uint32)
    base = eng.lut_register_base(dl)
    out = eng.pbs_shared_host(eng.encrypt(msgs, dl), np.arange(msgs.size + 1) * 2, np.full(msgs.size, base, np.uint32), np.tile(ids, msgs.size))
    out = out.reshape(msgs.size, 2, -1)
    sk_small, sk_big = eng.export_keys()[:2]
    hs, hb = int(sk_small.sum()), int(sk_big.sum())
    pairs = sk_small[0::2].copy()
    pairs[:sk_small[1::2].size] |= sk_small[1::2]
    v_rot = pc.unrolled_torus_variance(eng)
    v_white, v_carried = error_budget.pbs_output_variance_parts(eng.P, eng.bsk_precision, hs, hb, unroll=True, live_pairs=int(pairs.sum()))
    assert abs((v_white + hb * v_carried) / v_rot - 1.0) < 1e-6
    ratios = []
    for j, (t, s) in enumerate(tables):
        rows = np.ascontiguousarray(out[:, j])
        assert np.array_equal(eng.decrypt(rows, s), t[msgs + 8])
        pos, coef = sparse_table(t, 4, s, dl, eng.P.N)
        n2 = float((coef.astype(np.float64) ** 2).sum())
        model = n2 * v_white + key_carried_norm2(pos, coef, sk_big) * v_carried
        measured = float(np.var(pc.centred_error(eng.phase(rows), t[msgs + 8], s, eng.modulus)))
        ratios.append(measured / model)
        print(f"\nshared look-up on the unrolled key, table {j}: |P|^2 {n2:.0f}, log2 std measured {0.5 * np.log2(measured):.2f}; variance over "
              f"|P|^2 x one rotation's (white model) {measured / (n2 * v_rot):.3f}, over the budget's model {ratios[-1]:.3f}")
        assert measured < float(np.abs(coef).sum()) ** 2 * v_rot        # the worst case, fully correlated coefficients
    assert all(0.85 < r < 1.15 for r in ratios), ratios


@pytest.mark.parametrize("tag", ["baseline_n2_len20_ints8", "baseline_n3_len30_ints12"])
def test_inverse_with_shared_rotations_on_the_unrolled_key_matches_reference_golden(unr, tag):
    from bmi_amd.main import EncryptedMatrixInversion
    from bmi_amd.shared_rotation import rotation_groups
    c = pc.golden_inverse(tag)
    emi = EncryptedMatrixInversion(c["n"], None, 2, c["len"], c["ints"], False, False, engine=unr, unroll=True, share_rotations=True)
    digits, wall, _ = pc.timed_inverse(emi, c, warm_up=False)
    ex = emi._executor()
    print(f"\n{tag} on the unrolled key with shared rotations: {wall:.2f} s, {ex.lookups} look-ups, {ex.rotations} rotations, "
          f"p_fail {emi.error_budget['p_fail']:.1e}")
    assert digits == c["out"]
    assert ex.rotations == rotation_groups(ex.prog).groups < ex.lookups == ex.prog.n_nodes
    assert emi.error_budget["shared_lookups"] > 0 and emi.error_budget["rotations"] == ex.rotations


def test_batched_inverses_with_shared_rotations_on_the_unrolled_key(unr):
    """evaluate_many of two encryptions of the 2x2 golden input: its widest level has 2 x 223 groups, past the 256 rotations beyond
    which auto dispatch takes the two-per-workgroup kernel - which therefore serves groups; each replica decrypts to the golden
    digits"""
    from bmi_amd.main import EncryptedMatrixInversion
    from bmi_amd.shared_rotation import rotation_groups
    c = pc.golden_inverse("baseline_n2_len20_ints8")
    emi = EncryptedMatrixInversion(c["n"], None, 2, c["len"], c["ints"], False, False, engine=unr, unroll=True, share_rotations=True)
    q, s = emi.quantize(np.array(c["M"]).reshape(c["n"], c["n"]))
    res = emi.evaluate_many([emi.encrypt(q, s) for _ in range(2)])
    assert res.shape[0] == 2
    for r in res:
        assert emi.decrypt(r).tolist() == c["out"]
    ex = emi._executor(2)
    assert ex.share_rotations and ex.rotations == 2 * rotation_groups(ex.prog).groups < ex.lookups == 2 * ex.prog.n_nodes
    assert max(ng for ng, _, _ in ex.glevels) > 256 > min(ng for ng, _, _ in ex.glevels)


# ---- what stays refused ----------------------------------------------------------------------------------------------------------
def test_the_unrolled_key_pinned_at_48_bits_has_no_accumulator_form():
    """bmi_set_bsk_precision(48) before bmi_set_bsk_unroll(2): the exact-transform unrolled kernel (k_blind_rotate_lat2u_t64); it
    bootstraps, and refuses the accumulator form and the shared look-up by name"""
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=tfhe.TORUS64, n=16))
    try:
        e.set_bsk_precision(48)
        e.set_bsk_unroll(2)
        assert e.bsk_precision == 48
        e.keygen(SEED + 6)
        dl = e.delta_log()
        lid, base = e.lut_register(np.arange(-8, 8), 4, dl), e.lut_register_base(dl)
        small = pc.uniform_words(np.random.default_rng(1), (2, e.P.small))
        assert e.blind_rotate_host(small, [lid, lid]).shape == (2, e.P.N + 1)
        with pytest.raises(tfhe.BmiError, match="unrolled key pinned at 48 bits"):
            e.blind_rotate_glwe_host(small, [base, base])
        with pytest.raises(tfhe.BmiError, match="unrolled key pinned at 48 bits"):
            e.pbs_shared_host(np.zeros((1, e.P.big), np.uint64), np.array([0, 1]), [base], [lid])
    finally:
        e.close()
