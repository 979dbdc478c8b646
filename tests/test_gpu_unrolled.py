"""GPU parity tests of the UNROLLED blind rotation (bmi_set_bsk_unroll(ctx, 2); k_blind_rotate_lat2u_49): two LWE
coefficients per step.  Bit for bit against oracle/tfhe_oracle.c ora_blind_rotate_extract_unrolled on the same keys (seeded
key generation reproduces the oracle's keys word for word; CSPRNG keys are exported), output noise on the formula."""
import time

import numpy as np
import pytest

import pbs_cases as pc

pytestmark = pytest.mark.gpu

SEED = 0x5EED
# the exact key of the 49-bit field: no grid; 10 random rows to the oracle beside the fixed ones
CFG = pc.UnrolledConfig(q_bits=49, precision=64, grid_mask=0, oracle_rows=10, margin_hook=False)


def _engine(seed=SEED, **kw):
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=49, **kw))
    e.set_bsk_unroll(2)
    e.keygen(seed)
    return e


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


def test_seeded_unrolled_keygen_matches_the_oracle_keygen(eng):
    pc.check_unrolled_seeded_keys(eng, CFG, SEED)


@pytest.mark.parametrize("count", [1, 5, 300, 700])
def test_unrolled_pbs_bit_exact_every_batch_size(eng, count):
    pc.check_unrolled_pbs_every_batch_size(eng, CFG, count)


def test_unrolled_blind_rotation_extreme_inputs(eng):
    pc.check_unrolled_extreme_inputs(eng, CFG, rows=12)


# (l, Bg) = (1, 2^23): a 23-bit digit multiplies the key noise by 2^22 / sqrt(12); with three products per step the default
# 2^-40 would leave 4-bit look-ups at 2.6 - 3.6 sigma, so those cases run at key noise 2^-46 (the bits are compared either way)
@pytest.mark.parametrize("kw", [dict(n=629), dict(n=1024), dict(bs_levels=2), dict(bs_levels=1, bs_base_log=23, glwe_noise=2.0 ** -46), dict(n=1),
                                dict(log_N=11, bs_levels=2), dict(log_N=11, bs_levels=2, n=741),
                                dict(log_N=11, bs_levels=1, bs_base_log=23, glwe_noise=2.0 ** -46)],
                         ids=["odd_n", "n1024", "l2", "l1", "n1", "N2048_l2", "N2048_l2_odd_n", "N2048_l1"])
def test_unrolled_other_shapes_bit_exact(kw):
    from oracle import tfhe_oracle as to
    e = _engine(seed=77, **kw)
    try:
        # the oracle's own parameter set (its key noise is the default where the engine's is lowered: evaluation does not read it)
        P = to.default_params(q_bits=49, n=e.P.n, log_N=e.P.log_N, bs_levels=e.P.bs_levels, bs_base_log=e.P.bs_base_log)
        pc.check_unrolled_other_shape(e, decrypts=kw.get("n") != 1, params=P)   # (one coefficient cannot hold a message's phase)
    finally:
        e.close()


def test_unrolling_is_refused_where_no_kernel_exists():
    from bmi_amd import tfhe
    for kw in (dict(q_bits=49, log_N=11), dict(q_bits=49, log_N=12), dict(q_bits=65, bs_base_log=15), dict(q_bits=64)):
        e = tfhe.Engine(tfhe.default_params(**kw))
        try:
            with pytest.raises(tfhe.BmiError):
                e.set_bsk_unroll(2)
        finally:
            e.close()


def test_unrolled_key_under_csprng_and_on_an_evaluation_only_context():
    pc.check_unrolled_csprng_key_and_evaluation_only_context(49, count=9)


def test_key_files_carry_the_unrolled_key(eng, tmp_path):
    """Engine.save_keys / load_keys: an evaluation-only key file written in unrolled mode makes the loading (server) context
    reproduce the writer's ciphertexts; a full key file without the unrolled key lets an unrolled-mode context derive its own"""
    from bmi_amd import tfhe
    rng = np.random.default_rng(17)
    dl = eng.delta_log()
    table = rng.integers(-8, 8, 16)
    msgs = rng.integers(-8, 8, 7)
    ct = eng.encrypt(msgs, dl)
    got = eng.pbs_host(ct, np.full(7, eng.lut_register(table, 4, dl), np.uint32))
    eng.save_keys(tmp_path / "eval_unrolled.npz", secret=False)
    server = tfhe.Engine(tfhe.default_params(q_bits=49))
    plain = tfhe.Engine(tfhe.default_params(q_bits=49))
    client2 = tfhe.Engine(tfhe.default_params(q_bits=49))
    try:
        assert server.load_keys(tmp_path / "eval_unrolled.npz") is False
        assert np.array_equal(server.pbs_host(ct, np.full(7, server.lut_register(table, 4, dl), np.uint32)), got)
        plain.keygen(SEED)                                  # the same secret keys, plain mode: its key file has no unrolled key
        plain.save_keys(tmp_path / "full_plain.npz")
        client2.set_bsk_unroll(2)
        assert client2.load_keys(tmp_path / "full_plain.npz") is True
        out = client2.pbs_host(ct, np.full(7, client2.lut_register(table, 4, dl), np.uint32))
        assert list(client2.decrypt(out, dl)) == [int(table[m + 8]) for m in msgs]
    finally:
        server.close()
        plain.close()
        client2.close()


def test_unrolled_output_noise_on_the_formula_and_timing(eng, capsys):
    """4,096 bootstraps: output variance = 3 x the key-noise term of the CGGI value (+ the unchanged decomposition term);
    prints the per-bootstrap latency of the unrolled kernel next to the plain latency kernel's"""
    rng = np.random.default_rng(21)
    B = 4096
    dl = eng.delta_log()
    ident = np.arange(-8, 8)
    msgs = rng.integers(-8, 8, B)
    lid = eng.lut_register(ident, 4, dl)
    ct = eng.encrypt(msgs, dl)
    out = eng.pbs_host(ct, np.full(B, lid, np.uint32))
    assert list(eng.decrypt(out, dl)) == list(msgs)
    err = pc.centred_error(eng.phase(out), msgs, dl, eng.modulus)
    want = pc.unrolled_field_variance(eng.P)
    ratio = float(np.mean(err ** 2)) / want
    timing = pc.time_blind_rotation_beside_plain(eng, SEED, ident, msgs, dl)
    with capsys.disabled():
        print(f"\nunrolled PBS: output log2 std {0.5 * np.log2(np.mean(err ** 2)):.2f} (3 x key term + dec/2: {0.5 * np.log2(want):.2f}, "
              f"variance ratio {ratio:.3f}); blind rotation ms (host-buffer calls, copies included): " + timing)
    assert 0.9 < ratio < 1.1


@pytest.mark.parametrize("tag", ["baseline_n2_len20_ints8", "baseline_n3_len30_ints12", "baseline_n4_len40_ints16", "baseline_n8_len48_ints16",
                                 "overflow_digit_2x2", "overflow_digit_3x3", "uniform_3x3_small_truediv", "uniform_2x2_tensorize"])
def test_encrypted_inverse_with_the_unrolled_key_matches_reference_golden(tag, capsys):
    """BASELINE configs 2-5, the overflow-digit cases and the true-division / tensorize modes on ciphertexts with
    EncryptedMatrixInversion(unroll=True): decrypted digits == the reference's plaintext QFloat output
    (tests/golden/inverse.json, generated from the reference)."""
    from bmi_amd.main import EncryptedMatrixInversion
    c = pc.golden_inverse(tag)
    emi = EncryptedMatrixInversion(c["n"], None, 2, c["len"], c["ints"], c["true_division"], c["tensorize"], unroll=True, q_bits=49)
    try:
        emi.keygen()                                # CSPRNG keys
        assert emi.engine.P.glwe_noise == 2.0 ** -41
        out, wall, depth = pc.timed_inverse(emi, c, warm_up=c["n"] < 8)
        assert out == c["out"], ("digits differ" + ("; the 8x8 runs 2.1 M look-ups at the 6.2 sigma decision margin the north star's (n 630, "
                                 "N 1024, 4-bit messages) leave: about 1 run in 1,000 fails by noise alone - rerun once before "
                                 "suspecting the kernels" if c["n"] == 8 else ""))
        with capsys.disabled():
            print(f"\nunrolled key, {tag}: evaluate {wall:.2f} s, {depth} levels, {wall / depth * 1e3:.2f} ms per level")
    finally:
        emi.engine.close()


def test_secure128_preset_with_the_unrolled_key(capsys):
    """The 128-bit-secure preset (n 742, N 2048, l = 2) on the unrolled key: bit-exact against the oracle's unrolled mode under
    CSPRNG keys, output noise on the 3 x formula and still far below the keyswitch noise it feeds (the look-up margin is set by
    the latter), latency beside the plain kernel's, and the encrypted 2x2 inverse decrypting to the reference's digits."""
    from bmi_amd import tfhe
    from bmi_amd.main import EncryptedMatrixInversion
    P = tfhe.preset_params("secure128")
    e = tfhe.Engine(P)
    plain = tfhe.Engine(P)
    try:
        e.set_bsk_unroll(2)
        e.keygen()
        plain.keygen()
        rng = np.random.default_rng(43)
        dl = e.delta_log()
        table = rng.integers(-8, 8, 16)
        lid = e.lut_register(table, 4, dl)
        msgs = np.concatenate([np.arange(-8, 8)] * 64)                    # 1,024 ciphertexts
        ct = e.encrypt(msgs, dl)
        out = e.pbs_host(ct, np.full(msgs.size, lid, np.uint32))
        assert np.array_equal(e.decrypt(out, dl), table[msgs + 8])
        pick = rng.choice(msgs.size, 5, replace=False)
        with pc.oracle_for(e, unrolled=True) as o:
            assert np.array_equal(out[pick], o.ctx.pbs(ct[pick], e.lut_get(lid)[None, :], np.zeros(5, np.uint32), unrolled=True))
        oerr = pc.centred_error(e.phase(out), table[msgs + 8], dl, e.modulus)
        ratio = float(np.var(oerr)) / pc.unrolled_field_variance(P)
        B = 2.0 ** P.ks_base_log
        ks_var = P.N * P.ks_levels * (B * B + 2) / 12.0 * P.lwe_noise ** 2      # keyswitch noise (measured at this value in test_gpu_parity)
        assert 0.8 < ratio < 1.25 and np.var(oerr) * 75 ** 2 < ks_var / 4        # x75: the widest linear combination of the circuits
        t = {}
        for name, en in (("unrolled", e), ("plain", plain)):
            l2 = en.lut_register(table, 4, dl)
            c2 = en.encrypt(msgs[:256], dl)
            small = en.keyswitch_host(c2)
            for cnt in (1, 256):
                ids = np.full(cnt, l2, np.uint32)
                en.blind_rotate_host(small[:cnt], ids)
                t0 = time.perf_counter()
                for _ in range(3):
                    en.blind_rotate_host(small[:cnt], ids)
                t[(name, cnt)] = (time.perf_counter() - t0) / 3 * 1e3
        c = pc.golden_inverse("baseline_n2_len20_ints8")
        emi = EncryptedMatrixInversion(2, None, 2, c["len"], c["ints"], False, False, engine=e)
        q, s = emi.quantize(np.array(c["M"]).reshape(2, 2))
        enc = emi.encrypt(q, s)
        emi.evaluate(enc)
        t0 = time.time()
        res = emi.evaluate(enc)
        wall = time.time() - t0
        assert emi.decrypt(res).tolist() == c["out"]
        with capsys.disabled():
            print(f"\nsecure128 + unrolled key: output log2 std {0.5 * np.log2(np.var(oerr)):.2f} (variance / formula {ratio:.3f}); blind rotation ms "
                  + ", ".join(f"{k[0]} x{k[1]}: {v:.2f}" for k, v in t.items()) + f"; encrypted 2x2 inverse {wall:.2f} s")
    finally:
        e.close()
        plain.close()
