"""GPU parity tests (run on the MI355X box with `-m gpu`): every stage of the HIP PBS path must match
the exact CPU oracle BIT FOR BIT on identical keys, inputs and LUTs (integer arithmetic: no tolerance).
All calls go through the C ABI (include/bmi_tfhe.h) via bmi_amd.tfhe."""
import numpy as np
import pytest

import pbs_cases as pc

pytestmark = pytest.mark.gpu

SEED = 0x5EED


def words(values, Q):
    """python ints mod Q -> uint64 array (Q may be 2^64)"""
    return np.array([int(v) % Q for v in np.asarray(values, dtype=object).reshape(-1)], dtype=np.uint64).reshape(np.shape(values))


@pytest.fixture(scope="module", params=[64, 49, 65], ids=["goldilocks64", "p49_f64", "torus64"])
def eng(request):
    """the three ciphertext moduli: q = 2^64 - 2^32 + 1 (integer kernels), q = 2^49 - 720895 (f64 kernels) and
    q = 2^64 exactly (Concrete's torus; limb-split f64 kernels)"""
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=request.param))
    e.keygen(SEED)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ora(eng):
    with pc.oracle_for(eng) as o:
        yield o


@pytest.fixture(autouse=True)
def _select_oracle_field(request):
    """tests that take the engine fixture run the oracle on its modulus (the others select their own)"""
    if "eng" in request.fixturenames:
        from oracle import tfhe_oracle as to
        to.set_field(request.getfixturevalue("eng").q_bits)
    yield


def test_negacyclic_product_matches_oracle(eng, ora):
    if eng.q_bits == 65:
        pytest.skip("no transform exists mod 2^64 (the torus product is covered by the blind-rotation tests)")
    to = ora.to
    rng = np.random.default_rng(1)
    Q = eng.modulus
    a, b = pc.rand_q(rng, (9, 1024), Q), pc.rand_q(rng, (9, 1024), Q)
    # edge rows: zeros, ones, X^(N-1) * X = -1, max values
    a[0] = 0
    a[1] = 1
    a[2] = 0; a[2, 1023] = 1
    b[2] = 0; b[2, 1] = 1
    a[3] = Q - 1; b[3] = Q - 1
    got = eng.negacyclic_mul_host(a, b)
    for i in range(a.shape[0]):
        assert np.array_equal(got[i], to.negacyclic(10, a[i], b[i])), i
    assert np.array_equal(got[4], to.negacyclic(10, a[4], b[4], schoolbook=True))
    assert int(got[2, 0]) == Q - 1 and not got[2, 1:].any()


def test_keygen_matches_oracle_keygen(eng, ora):
    """Same seed, same RNG specification -> identical keys (covers the host keygen's negacyclic A*S)."""
    to, P, sk_small, sk_big = ora.to, ora.P, ora.sk_small, ora.sk_big
    _, _, bsk, ksk = eng.export_keys()
    K = to.keygen(P, SEED)
    assert np.array_equal(K.sk_small, sk_small) and np.array_equal(K.sk_big, sk_big)
    assert np.array_equal(K.ksk, ksk)
    # the default torus set stores its bootstrap key at 48 bits of precision: the library's key is the oracle's, rounded by the
    # oracle's own statement of the rule (ora_round_key); 64 bits (every other set) is the identity
    assert eng.bsk_precision == to.default_bsk_precision(P) == (48 if eng.q_bits == 65 else 64)
    assert np.array_equal(to.round_key(K.bsk, eng.bsk_precision), bsk)
    if eng.bsk_precision != 64:
        assert not np.array_equal(K.bsk, bsk) and not (bsk & np.uint64((1 << (64 - eng.bsk_precision)) - 1)).any()


def test_encrypt_decrypt_roundtrip_and_oracle_phase(eng, ora):
    to, P, sk_big = ora.to, ora.P, ora.sk_big
    msgs = np.arange(-8, 8)
    ct = eng.encrypt(msgs, eng.delta_log())
    assert list(eng.decrypt(ct, eng.delta_log())) == list(msgs)
    assert np.array_equal(eng.phase(ct), to.lwe_phase(sk_big, ct))
    assert list(to.decode(to.lwe_phase(sk_big, ct), eng.delta_log())) == list(msgs)


def test_lut_test_vector_matches_oracle(eng, ora):
    to = ora.to
    rng = np.random.default_rng(3)
    for p in (1, 2, 3, 4, 6):  # 6 bits: only the test-polynomial construction is compared
        table = rng.integers(-(1 << (p - 1)), 1 << (p - 1), 1 << p)
        lid = eng.lut_register(table, p, eng.delta_log(p))
        assert np.array_equal(eng.lut_get(lid), to.make_test_vector(10, p, table, eng.delta_log(p)))


def test_keyswitch_bit_exact(eng, ora):
    to, ctx, sk_small = ora.to, ora.ctx, ora.sk_small
    rng = np.random.default_rng(4)
    msgs = rng.integers(-8, 8, 19)  # not a multiple of the kernel tile: exercises the ragged tail
    ct = eng.encrypt(msgs, eng.delta_log())
    Q = eng.modulus
    ct[3, :1024] = pc.rand_q(rng, 1024, Q)     # arbitrary masks are valid inputs too
    ct[4, :1024] = np.uint64(Q - 1)          # extreme words
    ct[5, :1024] = np.uint64(Q // 2)
    ct[6, :1024] = np.uint64((Q // 2 + 1) % Q)
    ct[7, :] = 0
    got = eng.keyswitch_host(ct)
    want = ctx.keyswitch(ct)
    assert np.array_equal(got, want)
    eng.set_keyswitch_variant(1)          # the scalar kernel (K-split form at this batch size)
    try:
        assert np.array_equal(eng.keyswitch_host(ct), want)
    finally:
        eng.set_keyswitch_variant(0)
    ok = [0, 1, 2] + list(range(8, 19))
    assert list(to.decode(to.lwe_phase(sk_small, got[ok]), eng.delta_log())) == list(msgs[ok])


def test_keyswitch_matrix_core_path_bit_exact(eng, ora):
    """Every batch from one ciphertext up takes the int8 matrix-core keyswitch (ks_mfma.hpp; BMI_KS_MFMA_MIN = 1): ragged tile
    counts, extreme words, and the scalar kernel on the same inputs must all agree with the oracle bit for bit."""
    to, ctx, sk_small = ora.to, ora.ctx, ora.sk_small
    rng = np.random.default_rng(14)
    Q = eng.modulus
    for count in (64, 97):   # 97 = 3 full tiles of 32 + 1
        msgs = rng.integers(-8, 8, count)
        ct = eng.encrypt(msgs, eng.delta_log())
        ct[3, :1024] = pc.rand_q(rng, 1024, Q)
        ct[4, :1024] = np.uint64(Q - 1)
        ct[5, :1024] = np.uint64(Q // 2)
        ct[6, :1024] = np.uint64((Q // 2 + 1) % Q)
        ct[7, :] = 0
        ct[count - 1, :1024] = pc.rand_q(rng, 1024, Q)   # the ragged last row
        want = ctx.keyswitch(ct)
        got = eng.keyswitch_host(ct)
        assert np.array_equal(got, want), count
        eng.set_keyswitch_variant(1)
        try:
            assert np.array_equal(eng.keyswitch_host(ct), want), count
        finally:
            eng.set_keyswitch_variant(0)
        ok = [0, 1, 2] + list(range(8, count - 1))
        assert list(to.decode(to.lwe_phase(sk_small, got[ok]), eng.delta_log())) == list(msgs[ok])


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6],
                         ids=["pair_per_level", "latency", "pair_per_cmux", "latency_one_wave_transform", "pair_float_transform",
                              "latency_float_transform"])
def test_blind_rotate_every_kernel_variant(eng, ora, variant):
    """7 ciphertexts: ragged against the 2 (variant 1) and 4 (variant 3) ciphertexts per workgroup.  Variant 5 (2^64 torus: the
    wave-pair kernel whose exact limb products go through the folded complex FFT, bmi_kernels_t64f.hip) must return the same
    words as the integer arithmetic of the oracle."""
    to, ctx, sk_big = ora.to, ora.ctx, ora.sk_big
    rng = np.random.default_rng(15)
    tables = [np.arange(-8, 8), rng.integers(-8, 8, 16)]
    ids = [eng.lut_register(t, 4, eng.delta_log()) for t in tables]
    tvs = np.stack([eng.lut_get(i) for i in ids])
    msgs = rng.integers(-8, 8, 6)
    small = ctx.keyswitch(eng.encrypt(msgs, eng.delta_log()))
    small = np.concatenate([small, pc.rand_q(rng, (1, 631), eng.modulus)])
    sel = np.array([0, 1, 0, 1, 0, 1, 1], np.uint32)
    if variant in (5, 6) and eng.q_bits != 65:
        from bmi_amd import tfhe
        with pytest.raises(tfhe.BmiError):
            eng.set_kernel_variant(variant)
        return
    if eng.q_bits == 49 and variant in (1, 4):
        # the predecessors of the 49-bit kernels are retired (variants 3 and 2 replaced them): refused, not run
        from bmi_amd import tfhe
        with pytest.raises(tfhe.BmiError):
            eng.set_kernel_variant(variant)
        return
    with pc.pinned_variant(eng, variant):
        got = eng.blind_rotate_host(small, np.array(ids, np.uint32)[sel])
    assert np.array_equal(got, ctx.blind_rotate(small, tvs, sel))


def test_blind_rotate_bit_exact(eng, ora):
    to, ctx, sk_big = ora.to, ora.ctx, ora.sk_big
    rng = np.random.default_rng(5)
    tables = [np.arange(-8, 8), rng.integers(-8, 8, 16)]
    ids = [eng.lut_register(t, 4, eng.delta_log()) for t in tables]
    tvs = np.stack([eng.lut_get(i) for i in ids])
    msgs = rng.integers(-8, 8, 6)
    small = ctx.keyswitch(eng.encrypt(msgs, eng.delta_log()))
    small = np.concatenate([small, pc.rand_q(rng, (1, 631), eng.modulus), np.zeros((1, 631), np.uint64)])  # random + all-zero ciphertexts
    sel = np.array([0, 1, 0, 1, 0, 1, 1, 0], np.uint32)
    got = eng.blind_rotate_host(small, np.array(ids, np.uint32)[sel])
    want = ctx.blind_rotate(small, tvs, sel)
    assert np.array_equal(got, want)
    dec = to.decode(to.lwe_phase(sk_big, got[:6]), eng.delta_log())
    assert list(dec) == [int(tables[s][m + 8]) for s, m in zip(sel[:6], msgs)]


def test_pbs_bit_exact_and_evaluates_every_entry(eng, ora):
    to, ctx, sk_big = ora.to, ora.ctx, ora.sk_big
    rng = np.random.default_rng(6)
    table = rng.integers(-8, 8, 16)
    sq = np.array([(m * m) // 4 % 8 for m in range(-8, 8)])
    ids = [eng.lut_register(table, 4, eng.delta_log()), eng.lut_register(sq, 4, eng.delta_log())]
    tvs = np.stack([eng.lut_get(i) for i in ids])
    msgs = np.concatenate([np.arange(-8, 8), np.arange(-8, 8)])
    sel = np.array([0] * 16 + [1] * 16, np.uint32)
    ct = eng.encrypt(msgs, eng.delta_log())
    got = eng.pbs_host(ct, np.array(ids, np.uint32)[sel])
    want = ctx.pbs(ct, tvs, sel)
    assert np.array_equal(got, want)
    dec = eng.decrypt(got, eng.delta_log())
    assert list(dec[:16]) == list(table) and list(dec[16:]) == list(sq)
    # a second bootstrap of the outputs (noise stays bounded; still bit-exact)
    got2 = eng.pbs_host(got, np.array([ids[1]] * 32, np.uint32))
    assert np.array_equal(got2, ctx.pbs(got, tvs, np.ones(32, np.uint32)))
    assert list(eng.decrypt(got2, eng.delta_log())) == [int(sq[m + 8]) for m in dec]


def test_small_message_space_luts(eng):
    # p = 1..3 use wider boxes (input scaled by 2^(4-p) by the caller)
    for p in (1, 2, 3):
        M = 1 << p
        msgs = np.arange(-M // 2, M // 2)
        table = (msgs * 3 + 1) % M - M // 2
        lid = eng.lut_register(table, p, eng.delta_log())
        ct = eng.encrypt(msgs, eng.delta_log(p))
        out = eng.pbs_host(ct, np.full(M, lid, np.uint32))
        assert list(eng.decrypt(out, eng.delta_log())) == list(table)


def test_lincomb_device_matches_oracle(eng, ora):
    import torch
    to, P, sk_big = ora.to, ora.P, ora.sk_big
    msgs = np.array([1, -2, 3, 0, 2])
    ct = eng.encrypt(msgs, eng.delta_log())
    row_ptr = np.array([0, 2, 5, 5, 8], np.uint32)
    idx = np.array([0, 1, 2, 3, 0, 4, 4, 1], np.uint32)
    coef = np.array([2, -1, 1, 1, -1, 3, -7, 1], np.int64)
    consts = to.encode([1, 0, -4, 0], eng.delta_log())
    want = to.lincomb(P.big, ct, row_ptr, idx, coef, consts)
    dev = torch.device("cuda:0")
    d = lambda a, dt: torch.from_numpy(a.view(dt) if a.dtype != dt else a).to(dev)
    d_ct = d(ct.view(np.int64), np.int64)
    d_rp = d(row_ptr.view(np.int32), np.int32)
    d_ix = d(idx.view(np.int32), np.int32)
    d_cf = d(coef, np.int64)
    d_cs = d(consts.view(np.int64), np.int64)
    d_out = torch.zeros((4, P.big), dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    eng.lincomb(d_ct, d_rp, d_ix, d_cf, d_cs, 4, d_out, s)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want)
    assert list(eng.decrypt(got, eng.delta_log())) == [5, 2, -4, -10]


def test_pbs_device_pointers_and_noise_budget(eng, ora):
    """Device-resident call (torch tensors as plain device memory) + output noise inside the budget."""
    import torch
    to, ctx, sk_big = ora.to, ora.ctx, ora.sk_big
    rng = np.random.default_rng(8)
    B = 300  # spans several workgroups, ragged last group
    msgs = rng.integers(-8, 8, B)
    ident = eng.lut_register(np.arange(-8, 8), 4, eng.delta_log())
    ct = eng.encrypt(msgs, eng.delta_log())
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(ct.view(np.int64)).to(dev)
    d_ids = torch.full((B,), ident, dtype=torch.int32, device=dev)
    d_out = torch.empty_like(d_in)
    s = torch.cuda.current_stream().cuda_stream
    eng.pbs(d_in, d_ids, B, d_out, s)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint64)
    assert list(eng.decrypt(out, eng.delta_log())) == list(msgs)
    # spot-check bit-exactness on a sample (oracle is ~30 ms per PBS per core)
    pick = rng.choice(B, 12, replace=False)
    tv = eng.lut_get(ident)[None, :]
    assert np.array_equal(out[pick], ctx.pbs(ct[pick], tv, np.zeros(12, np.uint32)))
    ph = eng.phase(out)
    Q, dl = eng.modulus, eng.delta_log()
    err = pc.centred_words(ph, msgs, dl, Q)
    assert np.max(np.abs(err)) < 2.0 ** (dl - 9)  # half a box is 2^(dl-1)


def test_pbs_output_noise_matches_the_cggi_formula(eng):
    """the output noise of one PBS, measured over 4,096 bootstraps per modulus, against the analytic
    CGGI variance for (n 630, N 1024, k 1, l 3, Bg 2^15; the torus set: Bg 2^10 and a key stored at 48 bits, whose rounding error
    enters the formula as key noise - effective_params).  Exact arithmetic adds no error of its own, so the measured
    variance must sit AT the formula (within sampling + the formula's uniform-digit idealisation) on all three
    moduli - in particular the 49-bit field is not noisier than its parameters say (its key noise is 2^-40 by choice,
    the 64-bit moduli use 2^-44).  Also: mean error ~ 0, worst sample far inside half a box (2^-5 of the torus)."""
    import torch
    rng = np.random.default_rng(33)
    B = 4096
    dl = eng.delta_log()
    msgs = rng.integers(-8, 8, B)
    table = rng.integers(-8, 8, 16)
    lid = eng.lut_register(table, 4, dl)
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(eng.encrypt(msgs, dl).view(np.int64)).to(dev)
    d_ids = torch.full((B,), lid, dtype=torch.int32, device=dev)
    d_out = torch.empty_like(d_in)
    eng.pbs(d_in, d_ids, B, d_out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint64)
    want = table[msgs + 8]
    assert np.array_equal(eng.decrypt(out, dl), want)
    err = pc.centred_error(eng.phase(out), want, dl, eng.modulus)
    sk_small, sk_big = eng.export_keys()[:2]
    measured, analytic = float(np.var(err)), pc.cggi_output_variance(pc.effective_params(eng), eng.log_q, int(sk_small.sum()), int(sk_big.sum()))
    ratio = measured / analytic
    print(f"q_bits {eng.q_bits}: log2 std measured {0.5 * np.log2(measured):.2f}, CGGI {0.5 * np.log2(analytic):.2f}, "
          f"variance ratio {ratio:.3f}, max |err| 2^{np.log2(np.abs(err).max()):.2f}")
    assert 0.85 < ratio < 1.15, ratio                     # 4,096 samples: the variance estimate itself is +-2.2 % (1 sigma)
    assert abs(err.mean()) < 4 * np.sqrt(measured / B)
    assert np.abs(err).max() < 2.0 ** -9                  # half a box is 2^-6


def test_torus_key_at_42_bits_of_precision_bit_exact_and_noise():
    """bmi_set_bsk_precision(42) on the 2^64 torus: bootstrap-key words are multiples of 2^22 (two 21-bit limbs, 2/3 of the
    work).  The context's key is what export_keys returns, so the oracle bootstraps with the same key: both torus kernels stay
    bit-exact.  Noise, measured against the CGGI formula for a generated and for an imported key alike: the rounding errors
    of a row's mask words are summed over the ~N/2 set bits of the GLWE key, so the effective key noise is 2^-39.3 and the
    output noise 2^-15.15.  (Drawing the masks on the grid would avoid that - and round the key's own noise away: measured
    2^-20.05, i.e. LESS noise than the exact key, which is how the idea was caught and dropped.)"""
    from bmi_amd import tfhe
    from oracle import tfhe_oracle as to
    to.set_field(65)
    P = to.default_params(q_bits=65, bs_base_log=15)
    exact = to.keygen(P, SEED + 9)
    rng = np.random.default_rng(43)
    table = rng.integers(-8, 8, 16)
    B = 4096
    msgs = rng.integers(-8, 8, B)
    for mode in ("generated", "imported"):
        e = tfhe.Engine(tfhe.default_params(q_bits=65, bs_base_log=15))
        try:
            assert e.bsk_precision == 64                         # the default at base 2^15 is the exact key
            with pytest.raises(tfhe.BmiError):
                e.set_bsk_precision(48)                          # two 24-bit limbs need Bg <= 2^10
            e.set_bsk_precision(42)
            if mode == "generated":
                e.keygen(SEED + 9)
                with pytest.raises(tfhe.BmiError):
                    e.set_bsk_precision(64)                      # only before keys exist
            else:
                e.import_keys(exact.sk_small, exact.sk_big, exact.bsk, exact.ksk)
            bsk = e.export_keys()[2]
            assert not (bsk & np.uint64((1 << 22) - 1)).any()    # the context's key lives on the 2^22 grid
            if mode == "imported":
                d = (bsk.astype(np.int64) - exact.bsk.astype(np.int64))   # wrap-around difference = the rounding error
                assert np.abs(d).max() <= 1 << 21 and abs(float(np.var(d.astype(np.float64))) / (2.0 ** 44 / 12) - 1) < 0.02
            dl = e.delta_log()
            lid = e.lut_register(table, 4, dl)
            ct = e.encrypt(msgs, dl)
            ids = np.full(B, lid, np.uint32)
            out = e.pbs_host(ct, ids)                                  # wave-pair kernel
            pick = rng.choice(B, 6, replace=False)
            with pc.oracle_for(e) as o:
                want = o.ctx.pbs(ct[pick], e.lut_get(lid)[None, :], np.zeros(6, np.uint32))
            assert np.array_equal(out[pick], want)
            assert np.array_equal(e.pbs_host(ct[pick], ids[:6]), want)  # latency kernel
            assert np.array_equal(e.decrypt(out, dl), table[msgs + 8])
            err = pc.centred_error(e.phase(out), table[msgs + 8], dl, 1 << 64)
            # effective key noise: the body's rounding error + those of the k N / 2 key-selected mask words
            Pe = tfhe.default_params(q_bits=65, bs_base_log=15)
            words = 1 + Pe.k * Pe.N / 2.0
            Pe.glwe_noise = float(np.sqrt(Pe.glwe_noise ** 2 + words * 2.0 ** 44 / 12 / 2.0 ** 128))
            ratio = float(np.var(err)) / pc.cggi_output_variance(Pe, 64)
            print(f"torus, 42-bit key ({mode}): output log2 std {0.5 * np.log2(np.var(err)):.2f}, effective key noise 2^{np.log2(Pe.glwe_noise):.2f}, "
                  f"ratio to the CGGI formula {ratio:.3f}")
            assert 0.85 < ratio < 1.15
        finally:
            e.close()


def test_secure128_preset_bit_exact_noise_and_margin():
    """The 128-bit-secure preset (n 742, N 2048, LWE noise 2^-17.1; include/bmi_tfhe.h): keys, keyswitch, blind
    rotation and PBS bit-exact against the oracle at these parameters; every 4-bit message through a random table;
    keyswitch noise at its analytic value; the look-up margin it leaves (mod-switch + keyswitch noise vs half a box)."""
    from bmi_amd import tfhe
    P = tfhe.preset_params("secure128")
    assert (P.n, P.N, P.k, P.bs_levels, P.bs_base_log, P.q_bits, P.ks_levels, P.ks_base_log) == (742, 2048, 1, 2, 15, 49, 8, 2) and abs(np.log2(P.lwe_noise) + 17.11) < 0.01
    e = tfhe.Engine(P)
    try:
        e.keygen(SEED + 5)
        with pc.oracle_for(e) as o:
            to, ctx, sk_small = o.to, o.ctx, o.sk_small
            _, _, bsk, ksk = e.export_keys()
            K = to.keygen(o.P, SEED + 5)
            assert np.array_equal(K.bsk, bsk) and np.array_equal(K.ksk, ksk) and np.array_equal(K.sk_small, sk_small)
            rng = np.random.default_rng(41)
            dl = e.delta_log()
            table = rng.integers(-8, 8, 16)
            lid = e.lut_register(table, 4, dl)
            msgs = np.concatenate([np.arange(-8, 8)] * 32)                    # 512 ciphertexts, every message 32 times
            ct = e.encrypt(msgs, dl)
            small = e.keyswitch_host(ct)
            assert np.array_equal(small[:40], ctx.keyswitch(ct[:40]))
            out = e.pbs_host(ct, np.full(msgs.size, lid, np.uint32))
            pick = rng.choice(msgs.size, 6, replace=False)
            assert np.array_equal(out[pick], ctx.pbs(ct[pick], e.lut_get(lid)[None, :], np.zeros(6, np.uint32)))
            assert np.array_equal(e.decrypt(out, dl), table[msgs + 8])
            # keyswitch noise: phase error of the small ciphertexts, relative to q
            err = pc.centred_error(to.lwe_phase(sk_small, small), msgs, dl, e.modulus)
        analytic = pc.keyswitch_variance(P)
        ratio = float(np.var(err)) / analytic
        # what reaches the blind rotation, in units of the 2N positions of the circle: keyswitch noise + mod-switch rounding
        sigma_pos, margin = pc.lookup_margin(P, np.var(err), 4)
        print(f"secure128: keyswitch log2 std {0.5 * np.log2(np.var(err)):.2f} (analytic {0.5 * np.log2(analytic):.2f}, ratio "
              f"{ratio:.3f}); positions sigma {sigma_pos:.2f} of {2 * P.N}; 4-bit look-up margin {margin:.1f} sigma")
        assert 0.75 < ratio < 1.3 and margin > 8.0
        # bootstrap output noise at (l, Bg) = (2, 2^15): at the CGGI value, far below the keyswitch noise it feeds
        oerr = pc.centred_error(e.phase(out), table[msgs + 8], dl, e.modulus)
        oratio = float(np.var(oerr)) / pc.cggi_output_variance(P, 49)
        print(f"secure128: PBS output log2 std {0.5 * np.log2(np.var(oerr)):.2f} (CGGI ratio {oratio:.3f})")
        assert 0.7 < oratio < 1.4 and np.var(oerr) * 75 ** 2 < np.var(err) / 4     # x75: the widest linear combination of the circuits
        pc.time_pbs(e, ct, lid, "secure128")
    finally:
        e.close()


@pytest.mark.parametrize("q_bits,kw", [(64, dict(n=97, ks_levels=5, ks_base_log=6)), (49, dict(n=97, ks_levels=5, ks_base_log=6)),
                                       (49, dict(n=639, ks_levels=4, ks_base_log=7)),
                                       (49, dict(n=1024, ks_levels=8, ks_base_log=4)),
                                       (49, dict(n=211, bs_levels=2, bs_base_log=15)),
                                       (49, dict(n=211, bs_levels=1, bs_base_log=23)),
                                       (65, dict(n=211, bs_levels=2, bs_base_log=15)),
                                       (65, dict(n=1024)),
                                       (65, dict(n=211, bs_base_log=15)),
                                       (65, dict(n=211, bs_levels=2)),
                                       (65, dict(n=211, _precision=64)),
                                       (65, dict(n=211, bs_base_log=15, _precision=42)),
                                       (65, dict(n=211, bs_levels=2, bs_base_log=15, _precision=42))],
                         ids=["goldilocks64-n97", "p49-n97", "p49-n639", "p49-n1024-max", "p49-l2", "p49-l1-Bg23", "torus64-l2-Bg15",
                              "torus64-n1024-max", "torus64-Bg15-exact-key", "torus64-l2", "torus64-Bg10-exact-key", "torus64-Bg15-key42",
                              "torus64-l2-Bg15-key42"])
def test_other_parameter_shape_bit_exact(q_bits, kw):
    """n = 97 (98 output columns: a ragged column block in the matrix-core keyswitch) with a 5 x 6-bit keyswitch
    decomposition, n = 639 (640 columns exactly) with 4 x 7-bit digits (|d| <= 64, the int8 limit of the matrix-core
    form), the largest n = 1024, and the other bootstrap decompositions (l, Bg) = (2, 2^15) and (1, 2^23) on the 49-bit
    field and (2, 2^15) on the 2^64 torus: keyswitch (both kernels), every blind-rotation kernel and the fused PBS
    against the oracle, every 4-bit message through a random table; an empty batch is a no-op on every entry point."""
    from bmi_amd import tfhe
    kw = dict(kw)
    precision = kw.pop("_precision", None)     # torus: a non-default precision of the stored bootstrap key
    e = tfhe.Engine(tfhe.default_params(q_bits=q_bits, **kw))
    try:
        if precision:
            e.set_bsk_precision(precision)
        e.keygen(SEED + 1)
        with pc.oracle_for(e) as o:
            rng = np.random.default_rng(16)
            dl = e.delta_log()
            msgs = rng.integers(-8, 8, 70)
            ct = e.encrypt(msgs, dl)
            ct[1, :1024] = pc.rand_q(rng, 1024, e.modulus)
            want_small = o.ctx.keyswitch(ct)
            assert np.array_equal(e.keyswitch_host(ct), want_small)
            e.set_keyswitch_variant(1)
            if e.P.n + 1 > 768:     # the scalar keyswitch kernel stops at n = 767: refused, not wrong
                with pytest.raises(tfhe.BmiError):
                    e.keyswitch_host(ct)
            else:
                assert np.array_equal(e.keyswitch_host(ct), want_small)
            e.set_keyswitch_variant(0)
            table = rng.integers(-8, 8, 16)
            every = np.arange(-8, 8)
            assert np.array_equal(e.decrypt(e.pbs_host(e.encrypt(every, dl), np.full(16, e.lut_register(table, 4, dl), np.uint32)), dl),
                                  table[every + 8])
            lid = e.lut_register(rng.integers(-8, 8, 16), 4, dl)
            tv = e.lut_get(lid)[None, :]
            ids = np.full(5, lid, np.uint32)
            want = o.ctx.blind_rotate(want_small[:5], tv, np.zeros(5, np.uint32))
        for variant in (0, 1, 2, 3, 4):
            if variant in (1, 4) and q_bits == 49:       # the predecessors of the 49-bit kernels are retired: refused
                with pytest.raises(tfhe.BmiError):
                    e.set_kernel_variant(variant)
                continue
            with pc.pinned_variant(e, variant):
                assert np.array_equal(e.blind_rotate_host(want_small[:5], ids), want), variant
        assert np.array_equal(e.pbs_host(ct[:5], ids), want)
        empty = np.zeros((0, e.P.big), np.uint64)
        assert e.pbs_host(empty, np.zeros(0, np.uint32)).shape == (0, e.P.big)
        assert e.keyswitch_host(empty).shape == (0, e.P.small)
        assert e.blind_rotate_host(np.zeros((0, e.P.small), np.uint64), np.zeros(0, np.uint32)).shape == (0, e.P.big)
    finally:
        e.close()


def test_one_level_decomposition_at_N2048_with_the_plain_key_bit_exact_at_an_odd_n_and_batch():
    """k_blind_rotate_wide49<1, 23>: (l, Bg) = (1, 2^23) on the 49-bit field at N = 2048 is otherwise bootstrapped with the unrolled
    key only (tests/test_gpu_unrolled.py).  The blind rotation alone: n = 3, a batch of 3, uniformly random words of Z_q, every word
    against the oracle."""
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=49, n=3, log_N=11, bs_levels=1, bs_base_log=23))
    try:
        e.keygen(SEED + 2)
        rng = np.random.default_rng(23)
        lid = e.lut_register(rng.integers(-8, 8, 16), 4, e.delta_log())
        small = pc.rand_q(rng, (3, e.P.small), e.modulus)
        with pc.oracle_for(e) as o:
            want = o.ctx.blind_rotate(small, e.lut_get(lid)[None, :], np.zeros(3, np.uint32))
        assert e.rotation_kernel(3) == "k_blind_rotate_wide49"
        assert np.array_equal(e.blind_rotate_host(small, np.full(3, lid, np.uint32)), want)
    finally:
        e.close()


def test_full_batch_properties(eng, ora):
    """The bench batch size (8,192 ciphertexts, throughput kernels) through size-independent properties: every
    output decrypts to LUT[m]; a random sample is bit-exact against the oracle; the keyswitch is additive
    (KS(c1 + c2) and KS(c1) + KS(c2) decrypt alike although their digits differ); identical inputs at different
    batch positions give identical outputs (no dependence on the workgroup / wavefront a ciphertext lands in)."""
    to, ctx, sk_small, sk_big = ora.to, ora.ctx, ora.sk_small, ora.sk_big
    rng = np.random.default_rng(17)
    B = 8192
    dl = eng.delta_log()
    table = rng.integers(-8, 8, 16)
    lid = eng.lut_register(table, 4, dl)
    msgs = rng.integers(-8, 8, B)
    ct = eng.encrypt(msgs, dl)
    ct[4097] = ct[5]                      # duplicates far apart in the batch
    ct[8191] = ct[5]
    msgs[4097] = msgs[8191] = msgs[5]
    ids = np.full(B, lid, np.uint32)
    out = eng.pbs_host(ct, ids)
    assert np.array_equal(eng.decrypt(out, dl), table[msgs + 8])
    assert np.array_equal(out[4097], out[5]) and np.array_equal(out[8191], out[5])
    sample = np.sort(rng.choice(B, 12, replace=False))
    want = ctx.pbs(ct[sample], eng.lut_get(lid)[None, :], np.zeros(sample.size, np.uint32))
    assert np.array_equal(out[sample], want)
    # additivity of the keyswitch on small messages (|m1 + m2| < 8)
    m1, m2 = rng.integers(-3, 4, 256), rng.integers(-3, 4, 256)
    c1, c2 = eng.encrypt(m1, dl), eng.encrypt(m2, dl)
    Q = eng.modulus
    csum = ((c1.astype(object) + c2.astype(object)) % Q).astype(np.uint64)
    ks_sum = eng.keyswitch_host(csum)
    k1, k2 = eng.keyswitch_host(c1), eng.keyswitch_host(c2)
    sum_ks = ((k1.astype(object) + k2.astype(object)) % Q).astype(np.uint64)
    d1 = to.decode(to.lwe_phase(sk_small, ks_sum), dl)
    d2 = to.decode(to.lwe_phase(sk_small, sum_ks), dl)
    assert list(d1) == list(m1 + m2) and list(d2) == list(m1 + m2)


def test_context_lifecycle_rekey_growth_and_two_contexts():
    """One context re-keyed with a second seed (device keys, limb-form keyswitch key and latency-kernel key copy must
    all follow), scratch growth past bmi_reserve, and two contexts (one per field) alive on the same GPU."""
    from bmi_amd import tfhe
    e49 = tfhe.Engine(tfhe.default_params(q_bits=49))
    e64 = tfhe.Engine(tfhe.default_params(q_bits=64))
    try:
        rng = np.random.default_rng(18)
        table = rng.integers(-8, 8, 16)
        for seed in (11, 12):
            e49.keygen(seed)
            dl = e49.delta_log()
            lid = e49.lut_register(table, 4, dl)
            msgs = rng.integers(-8, 8, 6)
            ct = e49.encrypt(msgs, dl)
            ids = np.full(6, lid, np.uint32)
            with pc.oracle_for(e49) as o:
                want = o.ctx.pbs(ct, e49.lut_get(lid)[None, :], np.zeros(6, np.uint32))
            assert np.array_equal(e49.pbs_host(ct, ids), want), seed                     # latency kernel + its key copy
            with pc.pinned_variant(e49, 3):
                assert np.array_equal(e49.pbs_host(ct, ids), want), seed                 # throughput kernel
        # growth: reserve small, then run a batch 40x larger (scratch buffers reallocate under queued work)
        e49.reserve(32)
        big = rng.integers(-8, 8, 1300)
        out = e49.pbs_host(e49.encrypt(big, dl), np.full(big.size, lid, np.uint32))
        assert np.array_equal(e49.decrypt(out, dl), table[big + 8])
        # the other field's context was created before and is still usable after all of the above
        e64.keygen(13)
        dl64 = e64.delta_log()
        l64 = e64.lut_register(table, 4, dl64)
        m = rng.integers(-8, 8, 70)
        o64 = e64.pbs_host(e64.encrypt(m, dl64), np.full(m.size, l64, np.uint32))
        assert np.array_equal(e64.decrypt(o64, dl64), table[m + 8])
        o49 = e49.pbs_host(e49.encrypt(m, dl), np.full(m.size, lid, np.uint32))
        assert np.array_equal(e49.decrypt(o49, dl), table[m + 8])
    finally:
        e49.close()
        e64.close()


def test_key_import_and_evaluation_only_context(tmp_path):
    """Keys exported from one context and imported into another give identical ciphertexts; a context that imported
    the evaluation keys only bootstraps but refuses to encrypt / decrypt; the key file round-trips."""
    from bmi_amd import tfhe
    a = tfhe.Engine(tfhe.default_params(q_bits=49))
    b = tfhe.Engine(tfhe.default_params(q_bits=49))
    c = tfhe.Engine(tfhe.default_params(q_bits=49))
    try:
        a.keygen(21)
        dl = a.delta_log()
        rng = np.random.default_rng(19)
        table = rng.integers(-8, 8, 16)
        msgs = rng.integers(-8, 8, 9)
        ct = a.encrypt(msgs, dl)
        la = a.lut_register(table, 4, dl)
        want = a.pbs_host(ct, np.full(9, la, np.uint32))
        sk_small, sk_big, bsk, ksk = a.export_keys()
        b.import_keys(None, None, bsk, ksk)                       # server: evaluation keys only
        lb = b.lut_register(table, 4, dl)
        assert np.array_equal(b.pbs_host(ct, np.full(9, lb, np.uint32)), want)
        for call in (lambda: b.encrypt(msgs, dl), lambda: b.decrypt(want, dl), lambda: b.phase(want), lambda: b.export_keys()):
            with pytest.raises(tfhe.BmiError):
                call()
        assert b.export_keys(secret=False)[0] is None
        assert list(a.decrypt(want, dl)) == list(table[msgs + 8])  # the client decrypts the server's output
        a.save_keys(tmp_path / "full.npz")
        a.save_keys(tmp_path / "eval.npz", secret=False)
        assert c.load_keys(tmp_path / "full.npz") is True
        assert list(c.decrypt(c.pbs_host(ct, np.full(9, c.lut_register(table, 4, dl), np.uint32)), dl)) == list(table[msgs + 8])
        assert c.load_keys(tmp_path / "eval.npz") is False
        with pytest.raises(tfhe.BmiError):
            c.decrypt(want, dl)
        bad = bsk.copy()
        bad[0, 0, 0, 0] = np.uint64(a.modulus)                     # not reduced
        with pytest.raises(tfhe.BmiError):
            c.import_keys(None, None, bad, ksk)
        e64 = tfhe.Engine(tfhe.default_params(q_bits=64))
        try:
            with pytest.raises(tfhe.BmiError):
                e64.load_keys(tmp_path / "eval.npz")                # other field: parameter mismatch
        finally:
            e64.close()
    finally:
        a.close(); b.close(); c.close()


@pytest.mark.parametrize("log_N", [11, 12], ids=["N2048", "N4096"])
def test_wider_parameter_sets_bit_exact(log_N):
    """N = 2048 and N = 4096 (k = 1, l = 3, n = 630) on the 49-bit field: the transform as two / four 1024-point wave
    transforms (coefficients by index mod 2 / mod 4) combined on the fly.  Keygen, keyswitch (16,384 / 32,768-row
    matrix-core product), blind rotation and the fused PBS against the oracle; every 4-bit message through a random
    table; ragged batch; one more message bit per doubling of N at the same margin (5-bit / 6-bit look-ups)."""
    from bmi_amd import tfhe
    N = 1 << log_N
    e = tfhe.Engine(tfhe.default_params(q_bits=49, log_N=log_N))
    try:
        e.keygen(SEED + 2)
        _, _, bsk, ksk = e.export_keys()
        with pc.oracle_for(e) as o:
            to = o.to
            K = to.keygen(o.P, SEED + 2)
            assert np.array_equal(K.bsk, bsk) and np.array_equal(K.ksk, ksk) and np.array_equal(K.sk_big, o.sk_big)
            rng = np.random.default_rng(20)
            dl = e.delta_log()
            table = rng.integers(-8, 8, 16)
            lid = e.lut_register(table, 4, dl)
            assert np.array_equal(e.lut_get(lid), to.make_test_vector(log_N, 4, table, dl))
            msgs = np.concatenate([np.arange(-8, 8), rng.integers(-8, 8, 5)])   # 21: ragged against every tile size
            ct = e.encrypt(msgs, dl)
            assert ct.shape == (21, N + 1)
            small = e.keyswitch_host(ct)
            assert np.array_equal(small, o.ctx.keyswitch(ct))
            ids = np.full(msgs.size, lid, np.uint32)
            out = e.pbs_host(ct, ids)
            assert list(e.decrypt(out, dl)) == list(table[msgs + 8])
            pick = np.array([0, 7, 15, 20])
            want = o.ctx.pbs(ct[pick], e.lut_get(lid)[None, :], np.zeros(pick.size, np.uint32))
            assert np.array_equal(out[pick], want)
            assert np.array_equal(e.blind_rotate_host(small[pick], ids[pick]), want)
            with pytest.raises(tfhe.BmiError):
                e.negacyclic_mul_host(np.zeros((1, N), np.uint64), np.zeros((1, N), np.uint64))
            # 5-bit (N = 2048) / 6-bit (N = 4096) messages fit these rings at the margin 4-bit ones have at N = 1024
            pw = log_N - 6
            tw = rng.integers(-(1 << (pw - 1)), 1 << (pw - 1), 1 << pw)
            lw = e.lut_register(tw, pw, e.q_bits - 1 - pw)
            mw = np.concatenate([rng.integers(-(1 << (pw - 1)), 1 << (pw - 1), 10), [-(1 << (pw - 1)), (1 << (pw - 1)) - 1]])
            ow = e.pbs_host(e.encrypt(mw, e.q_bits - 1 - pw), np.full(mw.size, lw, np.uint32))
            assert list(e.decrypt(ow, e.q_bits - 1 - pw)) == list(tw[mw + (1 << (pw - 1))])
    finally:
        e.close()
    with pytest.raises(tfhe.BmiError):
        tfhe.Engine(tfhe.default_params(q_bits=64, log_N=log_N))    # the wider rings exist on the 49-bit field and the 2^64 torus


def test_pbs_known_answer_digests_on_gpu():
    """The committed known-answer digests (tests/golden/pbs_kat.json, produced by the oracle): the library's keys,
    ciphertexts, keyswitch and PBS outputs hash to the same values on every supported (field, N) - no oracle needed
    at run time."""
    import hashlib
    import json
    import os
    from bmi_amd import tfhe
    kat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "pbs_kat.json")))
    h = lambda a: hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()  # noqa: E731
    for case in kat["cases"]:
        e = tfhe.Engine(tfhe.default_params(q_bits=case["q_bits"], log_N=case["log_N"], **case["params"]))
        try:
            assert e.bsk_precision == case["bsk_precision"]
            e.keygen(kat["seed"])
            sk_small, sk_big, bsk, ksk = e.export_keys()
            assert (h(sk_big), h(bsk), h(ksk)) == (case["sk_big"], case["bsk"], case["ksk"]), case
            dl = e.delta_log()
            lid = e.lut_register(np.array(kat["table"]), 4, dl)
            assert h(e.lut_get(lid)) == case["test_vector"]
            ct = e.encrypt(np.array(kat["msgs"]), dl)
            assert h(ct) == case["ciphertexts"]
            assert h(e.keyswitch_host(ct)) == case["keyswitched"]
            out = e.pbs_host(ct, np.full(len(kat["msgs"]), lid, np.uint32))
            assert h(out) == case["bootstrapped"]
            for variant in (() if case["log_N"] != 10 else (2, 3) if case["q_bits"] == 49 else (1, 2, 3, 4)):
                with pc.pinned_variant(e, variant):
                    assert h(e.pbs_host(ct, np.full(len(kat["msgs"]), lid, np.uint32))) == case["bootstrapped"], variant
            if "bootstrapped_unrolled" in case:      # the unrolled key of the same secrets, made at once (bmi_set_bsk_unroll)
                e.set_bsk_unroll(2)
                assert h(e.export_bsk_unrolled()) == case["bsk_unrolled"]
                assert h(e.pbs_host(ct, np.full(len(kat["msgs"]), lid, np.uint32))) == case["bootstrapped_unrolled"]
        finally:
            e.close()


@pytest.mark.parametrize("q_bits", [49, 64], ids=["p49_f64", "goldilocks64"])
def test_torus64_client_interop(q_bits):
    """a client that works on the 2^64 torus the way Concrete does (binary LWE secret keys,
    u64 ciphertext words, message m * 2^(63 - p)) - here a numpy stand-in - encrypts under its own keys; the server
    derives evaluation keys for those secrets (bmi_keygen_from_secret), switches the ciphertexts to its field
    (bmi_torus64_to_field), bootstraps on the GPU and switches back; the client decrypts LUT[m] on the torus."""
    from bmi_amd import tfhe
    rng = np.random.default_rng(2064)
    e = tfhe.Engine(tfhe.default_params(q_bits=q_bits))
    try:
        P = e.P
        kN = P.k * P.N
        sk_small = rng.integers(0, 2, P.n, dtype=np.uint64)
        sk_big = rng.integers(0, 2, kN, dtype=np.uint64)
        e.keygen_from_secret(sk_small, sk_big, seed=77)
        got_small, got_big, _, _ = e.export_keys()
        assert np.array_equal(got_small, sk_small) and np.array_equal(got_big, sk_big)
        p = 4
        table = rng.integers(-8, 8, 16)
        lid = e.lut_register(table, p, e.delta_log(p))
        msgs = np.concatenate([np.arange(-8, 8), rng.integers(-8, 8, 112)])
        # client-side encryption on the 2^64 torus (uint64 arithmetic wraps mod 2^64)
        a = pc.uniform_words(rng, (msgs.size, kN))
        noise = np.rint(rng.normal(0.0, P.glwe_noise * 2.0**64, msgs.size)).astype(np.int64).astype(np.uint64)
        body = (a * sk_big[None, :]).sum(axis=1, dtype=np.uint64) + (msgs.astype(np.int64) << (63 - p)).astype(np.uint64) + noise
        ct_torus = np.concatenate([a, body[:, None]], axis=1)
        out_field = e.pbs_host(e.from_torus64(ct_torus), np.full(msgs.size, lid, dtype=np.uint32))
        out_torus = e.to_torus64(out_field)
        # client-side decryption on the torus
        phase = (out_torus[:, kN] - (out_torus[:, :kN] * sk_big[None, :]).sum(axis=1, dtype=np.uint64)).astype(np.int64)
        dec = (phase + (1 << (62 - p))) >> (63 - p)
        want = table[msgs + 8]
        assert np.array_equal(dec, want)
        assert np.array_equal(e.decrypt(out_field, e.delta_log(p)), want)      # and the field-side view agrees
        # distance of the torus phase from the exact encoding: well inside half a box (2^(62-p))
        err = np.abs(phase - (want.astype(np.int64) << (63 - p)))
        assert err.max() < (1 << (62 - p)) // 4
    finally:
        e.close()
