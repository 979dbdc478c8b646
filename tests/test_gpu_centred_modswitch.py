"""The centred modulus switch on the GPU (include/bmi_tfhe.h: bmi_set_modswitch, bmi_modswitch_centre_batch;
csrc/modswitch_centre.hip): the kernel bit for bit against the integer restatement of tests/test_centred_modswitch_model.py on
every ring, n, batch shape and edge content; the pipeline in mode 1 word for word against oracle.blind_rotate(centre(
oracle.keyswitch(ct))); the refusals; the failure counts of look-ups too wide for the default set against the centred prediction
of bmi_amd/failure_rate.py; and the encrypted inverse with centred_modswitch=True against the reference's golden digits.

Figures of a run of this file with -s are kept in profiles/centred_modswitch_ab.txt."""
import numpy as np
import pytest

import pbs_cases as pc
from test_centred_modswitch_model import Q49, centre, edge_rows

pytestmark = pytest.mark.gpu

KEY_SEED = 0x5EED
SENTINEL = 0x5A5A5A5AC3C3C3C3
PAD = 5                                  # sentinel words before and after a buffer's rows (odd: the rows start 8-byte aligned only)
COUNTS = (1, 3, 5, 257)                  # one live wavefront in the last workgroup; an odd tail; more than one round of workgroups
FIRST_EDGE = {1: 2, 3: 3, 5: 0, 257: 0}  # which edge row a batch starts with: over the four counts every one is used

# (q_bits, log_N, n): torus N = 1024 around the 64-lane stride and at both ends; the N = 2048 / 4096 presets; the 49-bit field
SHAPES = [(65, 10, n) for n in (16, 17, 63, 64, 65, 630, 1024)] + [(65, 11, 16), (65, 11, 742), (65, 12, 16), (65, 12, 742)] + \
         [(49, 10, 17), (49, 10, 630)]


def params_of(tfhe, q_bits, log_N, n):
    if q_bits == 49:
        return tfhe.default_params(q_bits=49, n=n)
    return tfhe.preset_params({10: "north_star_torus64", 11: "secure128_torus", 12: "secure128_torus_wide"}[log_N], n=n)


@pytest.fixture(scope="module")
def bare():
    """contexts without keys (the kernel needs none), by shape; closed with the module"""
    from bmi_amd import tfhe
    made = {}

    def get(q_bits, log_N, n):
        if (q_bits, log_N, n) not in made:
            made[q_bits, log_N, n] = tfhe.Engine(params_of(tfhe, q_bits, log_N, n))
        return made[q_bits, log_N, n]
    yield get
    for e in made.values():
        e.close()


def keyed(make):
    from bmi_amd import tfhe
    e = make(tfhe)
    e.keygen(KEY_SEED)
    return e


@pytest.fixture(scope="module")
def dflt():
    e = keyed(lambda t: t.Engine())
    yield e
    e.close()


@pytest.fixture(scope="module")
def unrolled():
    def make(t):
        e = t.Engine(t.default_params(q_bits=t.TORUS64))
        e.set_bsk_unroll(2)
        return e
    e = keyed(make)
    yield e
    e.close()


def contents(q_bits, log_N, n, count, seed):
    """`count` rows of random canonical words, the first ones the edge rows (zeros, the largest word, every mask word at the tie,
    one below it, a leading q - 1, random) starting at FIRST_EDGE[count]"""
    rng = np.random.default_rng(seed)
    rows = pc.rand_q(rng, (count, n + 1), Q49 if q_bits == 49 else 1 << 64)
    edge = np.roll(edge_rows(n, q_bits, log_N, rng), -FIRST_EDGE[count], axis=0)
    k = min(count, len(edge))
    rows[:k] = edge[:k]
    return rows


def padded(rows, fill_rows):
    """a device tensor of PAD sentinels, the rows' words (or as many sentinels), PAD sentinels; and the view of the rows"""
    import torch
    flat = np.full(2 * PAD + rows.size, SENTINEL, np.uint64)
    if fill_rows:
        flat[PAD:PAD + rows.size] = rows.reshape(-1)
    d = torch.from_numpy(flat.view(np.int64)).to("cuda:0")
    return d, d[PAD:PAD + rows.size]


def unpad(d, shape):
    h = d.cpu().numpy().view(np.uint64)
    assert (h[:PAD] == SENTINEL).all() and (h[-PAD:] == SENTINEL).all()
    return h[PAD:-PAD].reshape(shape)


# ------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("q_bits,log_N,n", SHAPES, ids=[f"q{q}-N{1 << l}-n{n}" for q, l, n in SHAPES])
def test_kernel_equals_the_restatement(bare, q_bits, log_N, n):
    import torch
    eng = bare(q_bits, log_N, n)
    assert eng.P.n == n and eng.P.log_N == log_N and eng.modswitch == 0
    s = torch.cuda.current_stream().cuda_stream
    for count in COUNTS:
        rows = contents(q_bits, log_N, n, count, 1000 * n + count)
        want = centre(rows, q_bits, log_N)
        assert np.array_equal(want[:, :-1], rows[:, :-1])
        # in place, rows at an odd word offset
        d_all, d_rows = padded(rows, True)
        assert d_rows.data_ptr() % 16 == 8
        eng.modswitch_centre(d_rows, count, d_rows, s)
        # into another buffer, which starts as sentinels: every word of the rows is written, nothing beyond them
        d_src_all, d_src = padded(rows, True)
        d_dst_all, d_dst = padded(rows, False)
        eng.modswitch_centre(d_src, count, d_dst, s)
        torch.cuda.synchronize()
        assert np.array_equal(unpad(d_all, rows.shape), want), count
        assert np.array_equal(unpad(d_dst_all, rows.shape), want), count
        assert np.array_equal(unpad(d_src_all, rows.shape), rows), count
    # 16-byte aligned rows give the same words; count == 0 launches nothing; the host form
    rows = contents(q_bits, log_N, n, 5, n)
    d = torch.from_numpy(np.concatenate([rows.reshape(-1), np.full(2, SENTINEL, np.uint64)]).view(np.int64)).to("cuda:0")
    assert d.data_ptr() % 16 == 0
    eng.modswitch_centre(d, 5, d, s)
    eng.modswitch_centre(d[rows.size:], 0, d[rows.size:], s)
    torch.cuda.synchronize()
    h = d.cpu().numpy().view(np.uint64)
    assert np.array_equal(h[:rows.size].reshape(rows.shape), centre(rows, q_bits, log_N)) and (h[rows.size:] == SENTINEL).all()
    assert np.array_equal(eng.modswitch_centre_host(rows), centre(rows, q_bits, log_N))


# ------------------------------------------------------------------------------------------ 2. the pipeline
def check_pipeline(eng, count, unrolled=False, extra=4):
    """mode 1: pbs_host == oracle.blind_rotate(centre(oracle.keyswitch)); keyswitch_host and blind_rotate_host as in mode 0; mode 0
    afterwards: the oracle's plain pbs again"""
    rng = np.random.default_rng(count)
    dl = eng.delta_log()
    table = rng.integers(-8, 8, 16)
    lid = eng.lut_register(table, 4, dl)
    tv = eng.lut_get(lid)[None, :]
    ids = np.full(count, lid, np.uint32)
    ct = eng.encrypt(rng.integers(-8, 8, count), dl)
    small0 = eng.keyswitch_host(ct)
    rot0 = eng.blind_rotate_host(small0, ids)
    pick = pc.sample_rows(count, [0, count - 1, 255, 256], rng, extra)
    zeros = np.zeros(pick.size, np.uint32)
    assert eng.modswitch == 0
    eng.set_modswitch(1)
    try:
        assert eng.modswitch == 1
        got = eng.pbs_host(ct, ids)
        assert np.array_equal(eng.keyswitch_host(ct), small0) and np.array_equal(eng.blind_rotate_host(small0, ids), rot0)
        centred = centre(small0, eng.q_bits, eng.P.log_N)
        assert np.array_equal(eng.modswitch_centre_host(small0), centred)
        assert np.array_equal(got, eng.blind_rotate_host(centred, ids))            # every row: the library's own stages
        with pc.oracle_for(eng, unrolled=unrolled) as o:
            ks = o.ctx.keyswitch(ct[pick])
            assert np.array_equal(ks, small0[pick])
            want = o.ctx.blind_rotate(centre(ks, eng.q_bits, eng.P.log_N), tv, zeros, unrolled=unrolled)
            assert np.array_equal(got[pick], want)
            eng.set_modswitch(0)
            back = eng.pbs_host(ct, ids)
            assert np.array_equal(back, rot0) and np.array_equal(back[pick], o.ctx.pbs(ct[pick], tv, zeros, unrolled=unrolled))
        # at the sets' own n the bodies move by several positions (at n = 16 by less than one: the words may well be the same), and
        # both modes decrypt alike (short-n engines carry no message)
        if eng.P.n >= 630:
            assert not np.array_equal(got, back)
            assert list(eng.decrypt(got, dl)) == list(eng.decrypt(back, dl))
    finally:
        eng.set_modswitch(0)


@pytest.mark.parametrize("count,variant,kernel", [(5, 0, "k_blind_rotate_lat_t64f"), (300, 0, "k_blind_rotate_lat_t64f"),
                                                  (300, 5, "k_blind_rotate_t64f")], ids=["5", "300", "300-throughput-kernel"])
def test_pipeline_default_torus(dflt, count, variant, kernel):
    """5 and 300 ciphertexts on the kernel auto dispatch takes (the latency form up to 512), and 300 on the pinned throughput kernel"""
    with pc.pinned_variant(dflt, variant):
        assert dflt.rotation_kernel(count).startswith(kernel), dflt.rotation_kernel(count)
        check_pipeline(dflt, count)


@pytest.mark.parametrize("which", ["secure128_torus", "secure128_torus_wide", "p49"])
def test_pipeline_other_engines(which):
    from bmi_amd import tfhe
    eng = keyed((lambda t: t.Engine(t.default_params(q_bits=49))) if which == "p49" else
                (lambda t: t.Engine(t.preset_params(which, n=16))))
    try:
        check_pipeline(eng, 5)
    finally:
        eng.close()


def test_pipeline_unrolled_key(unrolled):
    assert "2u" in unrolled.rotation_kernel(5)
    check_pipeline(unrolled, 5, unrolled=True)


def test_shared_rotation_pipeline(dflt):
    """pbs_shared_host in mode 1 == glwe_lookup_host(blind_rotate_glwe_host(centre(keyswitch_host))); mode 0 afterwards: uncentred"""
    eng = dflt
    rng = np.random.default_rng(77)
    dl = eng.delta_log()
    ids = np.array([eng.lut_register(t, 4, dl) for t in (np.arange(-8, 8), rng.integers(-8, 8, 16), rng.integers(-8, 8, 16))], np.uint32)
    base = eng.lut_register_base(dl)
    msgs = np.arange(-8, 8)[:7]
    ct = eng.encrypt(msgs, dl)
    gp = np.arange(msgs.size + 1) * 3
    bases, lut_ids = np.full(msgs.size, base, np.uint32), np.tile(ids, msgs.size)
    small = eng.keyswitch_host(ct)

    def chain(sm):
        return eng.glwe_lookup_host(eng.blind_rotate_glwe_host(sm, bases), gp, bases, lut_ids)
    plain = eng.pbs_shared_host(ct, gp, bases, lut_ids)
    glwe0 = eng.blind_rotate_glwe_host(small, bases)
    assert np.array_equal(plain, chain(small))
    eng.set_modswitch(1)
    try:
        got = eng.pbs_shared_host(ct, gp, bases, lut_ids)
        assert np.array_equal(eng.blind_rotate_glwe_host(small, bases), glwe0) and np.array_equal(eng.keyswitch_host(ct), small)
        assert np.array_equal(got, chain(centre(small, eng.q_bits, eng.P.log_N))) and not np.array_equal(got, plain)
    finally:
        eng.set_modswitch(0)
    assert np.array_equal(eng.pbs_shared_host(ct, gp, bases, lut_ids), plain)


# ------------------------------------------------------------------------------------------ 3. refusals
def test_refusals(dflt):
    import ctypes as C
    import torch
    from bmi_amd import tfhe
    ptr = tfhe._ptr

    def last(e):
        return e.lib.bmi_last_error(e.h).decode()

    with pytest.raises(tfhe.BmiError, match="must be 0 .standard. or 1 .centred."):
        dflt.set_modswitch(2)
    assert dflt.modswitch == 0
    gold = tfhe.Engine(tfhe.default_params(q_bits=64))
    try:
        gold.set_modswitch(0)
        with pytest.raises(tfhe.BmiError, match="2\\^64 torus and the 49-bit field only"):
            gold.set_modswitch(1)
        assert gold.modswitch == 0
        with pytest.raises(tfhe.BmiError, match="2\\^64 torus and the 49-bit field only"):
            gold.modswitch_centre_host(np.zeros((1, gold.P.small), np.uint64))
    finally:
        gold.close()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d = torch.full((dflt.P.small,), 7, dtype=torch.int64, device="cuda:0")
    host = np.zeros((1, dflt.P.small), np.uint64)
    lib, h = dflt.lib, dflt.h
    assert lib.bmi_modswitch_centre_batch(h, None, 1, ptr(d), s) < 0 and last(dflt) == "bmi_modswitch_centre_batch: null ciphertext pointer"
    assert lib.bmi_modswitch_centre_batch(h, ptr(d), 1, None, s) < 0 and last(dflt) == "bmi_modswitch_centre_batch: null ciphertext pointer"
    assert lib.bmi_modswitch_centre_batch(h, None, 0, None, s) == 0
    assert lib.bmi_modswitch_centre_batch_host(h, None, 1, ptr(host)) < 0 and last(dflt) == "bmi_modswitch_centre_batch_host: null ciphertext pointer"
    assert lib.bmi_modswitch_centre_batch_host(h, ptr(host), 1, None) < 0
    assert lib.bmi_get_modswitch(h, None) < 0 and last(dflt) == "bmi_get_modswitch: null result pointer"
    assert lib.bmi_set_modswitch(None, 1) < 0 and lib.bmi_modswitch_centre_batch(None, ptr(d), 1, ptr(d), s) < 0
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 7).all()


# ------------------------------------------------------------------------------------------ 4. failure counts
def report(tag, res, standard):
    print(f"\n{tag}: centred: observed {res['wrong']} wrong of {res['n']}, predicted {res['expected']:.1f}, band {res['band'][0]:.1f} .. "
          f"{res['band'][1]:.1f}; standard switch at the same key weights (hw(s) {res['hw_small']}, hw(S) {res['hw_big']}): predicted "
          f"{standard['expected']:.1f}, band {standard['band'][0]:.1f} .. {standard['band'][1]:.1f}; off by one: {res['off_by_one']}")


@pytest.fixture(scope="module")
def fresh():
    """a context of its own for the counts: the seeded encryption stream starts at its beginning"""
    e = keyed(lambda t: t.Engine())
    e.set_modswitch(1)
    yield e
    e.close()


def test_six_bit_failure_count(fresh):
    """6-bit identity table on the default set, 2^16 look-ups, half a box = 8 positions.  Centred model: 2.2 sigma, about 1.8 k
    wrong; standard model: 1.56 sigma, about 7.8 k.  The count lies in the harness's own band of the centred prediction (+-15 % on
    the variance, 3 sqrt(count)) and below the lower edge of the standard prediction at the same key weights."""
    from bmi_amd import failure_rate
    res = failure_rate.measure(fresh, 6, 8)
    standard = failure_rate.prediction(fresh.P, 6, res["n"], res["hw_small"], res["hw_big"])
    report("north_star_torus64 6-bit", res, standard)
    assert res["n"] == 1 << 16 and res["modswitch"] == 1
    assert 900 < res["expected"] < 3600 and 3900 < standard["expected"] < 15600          # the figures above, for hw(s) = n / 2
    lo, hi = res["band"]
    assert lo <= res["wrong"] <= hi, (res["wrong"], lo, hi)
    assert res["wrong"] < standard["band"][0], (res["wrong"], standard["band"])
    assert res["off_by_one"]


def test_five_bit_failure_count(fresh):
    """5-bit identity table, 2^18 look-ups: the standard switch counted 566 wrong (band 187 .. 1,217; tests/test_gpu_decrypt_device.py);
    centred predicts about 3, band up to about 20"""
    from bmi_amd import failure_rate
    res = failure_rate.measure(fresh, 5, 32)
    standard = failure_rate.prediction(fresh.P, 5, res["n"], res["hw_small"], res["hw_big"])
    report("north_star_torus64 5-bit", res, standard)
    assert res["n"] == 1 << 18 and res["modswitch"] == 1
    lo, hi = res["band"]
    assert hi < 187 and 0.5 < res["expected"] < 12
    assert lo <= res["wrong"] <= hi, (res["wrong"], lo, hi)
    assert res["wrong"] < standard["band"][0]
    assert res["off_by_one"]


# ------------------------------------------------------------------------------------------ 5. the application
@pytest.mark.parametrize("tag,options", [("baseline_n2_len20_ints8", {}), ("baseline_n3_len30_ints12", {}),
                                         ("baseline_n2_len20_ints8", {"unroll": True}), ("baseline_n2_len20_ints8", {"share_rotations": True})],
                         ids=["2x2", "3x3", "2x2-unrolled", "2x2-shared-rotations"])
def test_encrypted_inverse_with_the_centred_switch(request, tag, options):
    from bmi_amd.main import EncryptedMatrixInversion
    eng = request.getfixturevalue("unrolled" if options.get("unroll") else "dflt")
    c = pc.golden_inverse(tag)
    try:
        emi = EncryptedMatrixInversion(c["n"], None, 2, c["len"], c["ints"], False, False, engine=eng, centred_modswitch=True, **options)
        digits, wall, depth = pc.timed_inverse(emi, c, warm_up=False)
        assert eng.modswitch == 1                                    # set on the engine passed in
        assert digits == c["out"]
        budget = emi.error_budget
        print(f"\n{tag} {options or ''} centred: {wall:.2f} s, {depth} levels, worst margin {budget['worst_margin_sigma']:.3f} sigma, "
              f"p_fail {budget['p_fail']:.2e}")
        if not options.get("unroll"):
            assert budget["worst_margin_sigma"] > 8.5
            eng.set_modswitch(0)
            plain = EncryptedMatrixInversion(c["n"], None, 2, c["len"], c["ints"], False, False, engine=eng, **options)
            plain._engine()
            assert plain.error_budget["worst_margin_sigma"] < budget["worst_margin_sigma"] and eng.modswitch == 0
            if not options:
                assert plain.error_budget["worst_margin_sigma"] == pytest.approx(6.236, abs=0.01)
    finally:
        eng.set_modswitch(0)
