"""The shared scaffolding of the GPU parity tests (tests/test_gpu_*.py): the oracle on an engine's exported keys, pinned kernel
variants, the random and adversarial input rows, the centred phase error, the analytic noise expressions, and the test bodies
that several files run at their own configuration (check_*).  Every numeric bound of an assertion stays in the test file that
owns it and arrives here as an argument or in that file's configuration record.  A plain helper module: no fixtures, no pytest
hooks.  tests/test_pbs_cases.py holds the helpers to their written-out expressions, on the CPU."""
import contextlib
import json
import os
import time
from collections import namedtuple

import numpy as np
import pytest

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

Oracle = namedtuple("Oracle", "to ctx P sk_small sk_big")


@contextlib.contextmanager
def oracle_for(eng, unrolled=False, bsk3=None, params=None):
    """the oracle context on the engine's exported keys, its field selected and its Params a copy of every field of eng.P
    (tests/test_pbs_cases.py: equal to the oracle's own default_params on every set the callers use; `params`: a caller whose
    set differs passes its own); closed on every exit path"""
    from bmi_amd import tfhe
    from oracle import tfhe_oracle as to
    to.set_field(eng.q_bits)
    sk_small, sk_big, bsk, ksk = eng.export_keys()
    P = params if params is not None else to.Params(**{f: getattr(eng.P, f) for f, _ in tfhe.Params._fields_})
    ctx = to.Ctx(P, bsk, ksk)
    try:
        if unrolled:
            ctx.set_bsk_unrolled(eng.export_bsk_unrolled() if bsk3 is None else bsk3)
        yield Oracle(to, ctx, P, sk_small, sk_big)
    finally:
        ctx.close()


@contextlib.contextmanager
def pinned_variant(eng, v):
    """kernel variant v for the block, auto dispatch (0) again on every exit path"""
    eng.set_kernel_variant(v)
    try:
        yield
    finally:
        eng.set_kernel_variant(0)


def uniform_words(rng, shape):
    """uniformly random 64-bit words (as ciphertext rows not valid encryptions: they drive the digits to their full range)"""
    return rng.integers(0, 1 << 63, shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, shape, dtype=np.uint64)


def rand_q(rng, shape, Q):
    """uniform canonical words of Z_q (top values included)"""
    if Q >> 64:      # the 2^64 torus: every word is canonical
        return uniform_words(rng, shape)
    if Q >> 63:
        v = uniform_words(rng, shape)
        return np.where(v >= np.uint64(Q), v - np.uint64(Q), v)
    return rng.integers(0, Q, shape, dtype=np.uint64)


def adversarial_rows(small, rng, count):
    """overwrites the first rows of a batch of `count` small ciphertexts: uniformly random words, zeros, all ones, and random
    words whose every eighth coefficient is 0 (a skipped step: the f64 accumulator is re-centred every eight steps TAKEN,
    whichever steps a ciphertext skips)"""
    small[0] = uniform_words(rng, small.shape[1])
    if count > 2:
        small[1] = 0
        small[2] = np.uint64(0xFFFFFFFFFFFFFFFF)
    if count > 4:
        small[3] = rng.integers(0, 1 << 63, small.shape[1], dtype=np.uint64) * np.uint64(2)
        small[3, 7::8] = 0


def extreme_rows_unrolled(rng, rows, width, skipped_pairs=False, Q=1 << 64):
    """arbitrary small-key words for the unrolled blind rotation: zeros, maxima, the pair sums that wrap 2N"""
    small = rand_q(rng, (rows, width), Q)
    small[0] = 0                                # every exponent zero: the accumulator is the test polynomial
    small[1] = np.uint64(Q - 1)
    small[2] = np.uint64(Q // 2)                # every a = N: the pair sums wrap to 0
    small[3, ::2] = 0                           # first coefficient of every pair zero
    small[4, 1::2] = 0
    small[5, :-1] = np.uint64((Q + 2047) // 2048)   # a = 1 everywhere
    if skipped_pairs:
        small[6, 14::16] = 0                    # a whole pair zero every eighth step: the f64 accumulator is re-centred every
        small[6, 15::16] = 0                    # eight steps TAKEN
    return small


def sample_rows(count, fixed, rng, extra):
    """the rows of a batch the oracle checks: all of a batch up to 8, else the fixed rows and `extra` random ones"""
    if count <= 8:
        return np.arange(count)
    return np.unique(np.concatenate([fixed, rng.integers(0, count, extra)]) % count)


def centred_words(phases, expected_msgs, delta_log, Q):
    """phase - m * 2^delta_log, centred on 0, in words of Z_Q (float64).  Python integers: exact on 2^64 too, where int64 wraps"""
    return np.array([((int(x) - (int(m) << delta_log)) + Q // 2) % Q - Q // 2 for x, m in zip(phases, expected_msgs)], dtype=np.float64)


def centred_error(phases, expected_msgs, delta_log, Q):
    """centred_words relative to Q"""
    return centred_words(phases, expected_msgs, delta_log, Q) / float(Q)


def cggi_output_variance(P, log_q, hw_small=None, hw_big=None):
    """Analytic variance (relative to q^2) of the phase error after one blind rotation, binary keys (CGGI):
    n CMUXes, each adding  l (k+1) N (Bg^2 + 2) / 12 * sigma_bsk^2  (digits uniform in [-Bg/2, Bg/2) against fresh key noise)
    +  (1 + k N / 2) / (12 Bg^(2l))  (the rounding of the decomposition, carried by the binary GLWE key).
    The rounding term as printed in the literature is a worst case: the rounding error of a CMUX is multiplied by the key bit
    its GGSW encrypts, so only the hw_small SET bits of the LWE key contribute, and it is carried by the hw_big set bits of the
    GLWE key.  With the weights given, the exact expectation is returned (it matters where the rounding term is not
    negligible: the torus set, Bg = 2^10); without them, the textbook worst case."""
    N, k, l, Bg = P.N, P.k, P.bs_levels, 2.0 ** P.bs_base_log
    key = l * (k + 1) * N * (Bg * Bg + 2) / 12.0 * P.glwe_noise ** 2
    rnd = (1 + (k * N / 2.0 if hw_big is None else hw_big)) * (1.0 / (12.0 * Bg ** (2 * l)) - 1.0 / (12.0 * 4.0 ** log_q))
    return P.n * key + (P.n if hw_small is None else hw_small) * rnd


def effective_params(eng):
    """the engine's parameters with the key noise a bootstrap actually sees: a torus key stored at p < 64 bits carries, per row,
    the rounding error of the body and of the mask words the GLWE key selects (uniform on 2^(64 - p): variance 2^(2 (64 - p)) / 12
    each), on top of its Gaussian noise"""
    from bmi_amd import tfhe
    P = tfhe.Params(**{f: getattr(eng.P, f) for f, _ in tfhe.Params._fields_})
    prec = eng.bsk_precision
    if prec != 64:
        hw = int(eng.export_keys()[1].sum())
        P.glwe_noise = float(np.sqrt(P.glwe_noise ** 2 + (1 + hw) * 4.0 ** (64 - prec) / 12 / 2.0 ** 128))
    return P


def unrolled_field_variance(P):
    """output variance of the unrolled blind rotation with an exact key: 3 x the key-noise term of the CGGI value + half its
    decomposition term"""
    Bg = 2.0 ** P.bs_base_log
    key_term = P.n * P.bs_levels * 2 * P.N * (Bg * Bg + 2) / 12 * P.glwe_noise ** 2
    dec_term = P.n * (1 + P.N / 2) / (12 * Bg ** (2 * P.bs_levels))
    return 3 * key_term + dec_term / 2


def unrolled_torus_variance(eng):
    """output variance of the unrolled blind rotation on the torus: 3 x the key-noise term (the key noise a bootstrap sees
    includes the rounding of the stored key: body + the mask words the GLWE key selects) + the decomposition rounding: a step's
    rounding error is multiplied by the bit its GGSW encrypts - exactly one of the three keys of a pair encrypts 1 unless both key
    bits are 0 - then scaled by X^c - 1 (x 2) and carried by the GLWE key's set bits"""
    P = eng.P
    Bg = 2.0 ** P.bs_base_log
    sk_small, sk_big = eng.export_keys()[:2]
    hw = int(sk_big.sum())
    sigma2 = P.glwe_noise ** 2 + (1 + hw) * 4.0 ** (64 - eng.bsk_precision) / 12 / 2.0 ** 128
    pairs = sk_small[0::2].copy()
    pairs[:sk_small[1::2].size] |= sk_small[1::2]
    key_term = P.n * P.bs_levels * 2 * P.N * (Bg * Bg + 2) / 12 * sigma2
    return 3 * key_term + 2 * int(pairs.sum()) * (1 + hw) / (12 * Bg ** (2 * P.bs_levels))


def keyswitch_variance(P):
    """analytic variance (relative to q^2) of the keyswitch's phase error: digits uniform in [-B/2, B/2) against the key's noise
    + the rounding of the decomposition carried by the binary key"""
    B = 2.0 ** P.ks_base_log
    kN = P.k * P.N
    return kN * P.ks_levels * (B * B + 2) / 12.0 * P.lwe_noise ** 2 + kN / 2.0 / (12.0 * B ** (2 * P.ks_levels))


def lookup_margin(P, ks_error_power, box_bits):
    """(sigma_pos, margin): what reaches the blind rotation in units of the 2N positions of the circle - keyswitch error of the
    given power (variance or mean square, relative to q^2) + mod-switch rounding - and half a box of a box_bits-bit look-up
    (boxes are N / 2^box_bits positions wide) in those sigmas"""
    sigma_pos = np.sqrt(ks_error_power * (2 * P.N) ** 2 + (P.n / 2.0 + 1) / 12.0)
    return sigma_pos, (P.N / float(2 << box_bits)) / sigma_pos


def time_pbs(eng, ct, lid, tag):
    """prints the latency of one bootstrap and of a full round (256 ciphertexts: one workgroup per CU)"""
    ids256 = np.full(256, lid, np.uint32)
    eng.pbs_host(ct[:256], ids256)
    t0 = time.perf_counter(); eng.pbs_host(ct[:256], ids256); t256 = time.perf_counter() - t0
    t0 = time.perf_counter(); eng.pbs_host(ct[:1], ids256[:1]); t1 = time.perf_counter() - t0
    print(f"{tag}: 1 PBS {t1 * 1e3:.2f} ms, 256 PBS {t256 * 1e3:.2f} ms (host-buffer calls, copies included)")


def time_blind_rotation_beside_plain(eng, seed, table, msgs, dl):
    """ms per blind rotation of 1 and of 256 ciphertexts (host-buffer calls, copies included) on `eng` and on a plain engine of
    the same modulus and keys, as the text the noise tests print"""
    from bmi_amd import tfhe
    plain = tfhe.Engine(tfhe.default_params(q_bits=eng.q_bits))
    plain.keygen(seed)
    t = {}
    for name, e in (("unrolled", eng), ("plain latency kernel", plain)):
        l2 = e.lut_register(table, 4, dl)
        for cnt in (1, 256):
            c = e.encrypt(msgs[:cnt], dl)
            ids = np.full(cnt, l2, np.uint32)
            small = e.keyswitch_host(c)
            e.blind_rotate_host(small, ids)
            t0 = time.perf_counter()
            for _ in range(3):
                e.blind_rotate_host(small, ids)
            t[(name, cnt)] = (time.perf_counter() - t0) / 3 * 1e3
    plain.close()
    return ", ".join(f"{k[0]} x{k[1]}: {v:.2f}" for k, v in t.items())


def golden_inverse(tag):
    """one case of tests/golden/inverse.json (generated from the reference)"""
    with open(os.path.join(GOLDEN_DIR, "inverse.json")) as f:
        return next(x for x in json.load(f) if x["tag"] == tag)


def timed_inverse(emi, c, warm_up):
    """the golden case's matrix through the encrypted inverse; returns (decrypted digits, seconds of one evaluation, levels)"""
    M = np.array(c["M"]).reshape(c["n"], c["n"])
    q, s = emi.quantize(M)
    enc = emi.encrypt(q, s)
    emi._executor()
    if warm_up:
        emi.evaluate(enc)
    t0 = time.time()
    res = emi.evaluate(enc)
    wall = time.time() - t0
    return emi.decrypt(res).tolist(), wall, emi.circuit.summary()["depth"]


# ---- shared rotations: the look-up kernel's edge tables and groups, one statement for the GPU test that runs them
# ---- (tests/test_gpu_shared_rotation.py) and the CPU test that pins their reference to the oracle (tests/test_shared_rotation_model.py)

# the finest unit a base polynomial can have, by ring size: 64 - (bits the default bootstrap key of that ring is stored at) + 1
FLOOR_UNIT = {1024: 17, 2048: 19, 4096: 21}


def edge_lookup_tables(rng):
    """name -> (table, bits, scale): a 6-bit table whose 64 neighbouring differences are all non-zero (BMI_SPARSE_CAP entries;
    (-1)^i (i mod 7 + 1) has 63: f(0) = -f(31), so f(-32) is changed), random 6-bit tables at their full scale and one above, 1-
    and 2-bit tables of one to four entries, the all-zero table (no entry), a constant table (one entry, at N/2 - N/32), and
    4-bit tables at full scale and at 2^22"""
    six = np.array([(-1) ** i * (i % 7 + 1) for i in range(64)])
    six[0] = 2
    return {"six64": (six, 6, 57), "six_random": (rng.integers(-32, 32, 64), 6, 57), "six_at58": (rng.integers(-16, 16, 64), 6, 58),
            "one": (np.array([-1, 0]), 1, 62), "one_const": (np.array([-1, -1]), 1, 62),
            "two": (np.array([-2, 1, 0, 0]), 2, 61), "two_edge": (np.array([-2, 1, 0, -2]), 2, 61),
            "zero": (np.zeros(16, np.int64), 4, 59), "const": (np.full(16, 5), 4, 59),
            "four": (rng.integers(-8, 8, 16), 4, 59), "four_low": (rng.integers(-8, 8, 16), 4, 22)}


def edge_lookup_groups(floor_unit):
    """(unit of the group's base polynomial, members) of one block of four groups: the key's grid floor serving tables 2^42 / 2^40
    / 2^38 and a few bits above it; the base polynomial of a coarser unit ("base59": P = 2) next to a 6-bit table; an empty
    group; the narrow, empty and constant tables"""
    return [(floor_unit, ["four", "six64", "six_random", "four_low"]),
            (58, ["base59", "six_at58"]),
            (59, []),
            (59, ["zero", "const", "one", "one_const", "two", "two_edge"])]


# ---- the unrolled blind rotation at three configurations: the 49-bit field, the torus with the 48-bit key (exact transform) and
# ---- with the 42-bit key (floating-point transform)

# precision: bits the bootstrap key is stored at; grid_mask: the bits of every key and accumulator word that are then zero;
# oracle_rows: random rows the oracle checks beside the fixed ones; margin_hook: the kernel accumulates in f64 (bmi_fft_margin_host
# exists, and rows that skip whole pairs are an edge)
UnrolledConfig = namedtuple("UnrolledConfig", "q_bits precision grid_mask oracle_rows margin_hook")


def check_unrolled_seeded_keys(eng, cfg, seed):
    """seeded key generation reproduces the oracle's keys, plain and unrolled, rounded by the oracle's own statement of the rule"""
    from oracle import tfhe_oracle as to
    to.set_field(cfg.q_bits)
    P = to.default_params(q_bits=cfg.q_bits)
    assert eng.bsk_precision == cfg.precision
    K = to.keygen(P, seed)
    sk_small, sk_big, bsk, ksk = eng.export_keys()
    assert np.array_equal(K.sk_small, sk_small) and np.array_equal(K.ksk, ksk)
    assert np.array_equal(to.round_key(K.bsk, cfg.precision), bsk)
    bsk3 = eng.export_bsk_unrolled()
    assert np.array_equal(to.round_key(to.keygen_bsk_unrolled(P, seed, K.sk_small, K.sk_big), cfg.precision), bsk3)
    assert not (bsk3 & np.uint64(cfg.grid_mask)).any() and not (bsk & np.uint64(cfg.grid_mask)).any()
    return P


def check_unrolled_pbs_every_batch_size(eng, cfg, count):
    """one kernel for every batch size: the ciphertext bits do not depend on the batch a ciphertext travelled in"""
    with oracle_for(eng, unrolled=True) as o:
        rng = np.random.default_rng(count)
        dl = eng.delta_log()
        tables = [np.arange(-8, 8), rng.integers(-8, 8, 16)]
        lids = [eng.lut_register(t, 4, dl) for t in tables]
        tvs = np.stack([eng.lut_get(l) for l in lids])
        msgs = rng.integers(-8, 8, count)
        sel = rng.integers(0, 2, count).astype(np.uint32)
        ct = eng.encrypt(msgs, dl)
        got = eng.pbs_host(ct, np.array(lids, np.uint32)[sel])
        assert list(eng.decrypt(got, dl)) == [int(tables[s][m + 8]) for s, m in zip(sel, msgs)]
        assert not (got & np.uint64(cfg.grid_mask)).any()      # the accumulator lives on the key's grid
        pick = sample_rows(count, [0, count - 1, 255, 256, 511, 512], rng, cfg.oracle_rows)
        assert np.array_equal(got[pick], o.ctx.pbs(ct[pick], tvs, sel[pick], unrolled=True))


def check_unrolled_extreme_inputs(eng, cfg, rows):
    """arbitrary small-key words (extreme_rows_unrolled) straight into the blind rotation; returns the generator and the table's
    id for the caller that goes on"""
    with oracle_for(eng, unrolled=True) as o:
        rng = np.random.default_rng(11)
        small = extreme_rows_unrolled(rng, rows, o.P.n + 1, skipped_pairs=cfg.margin_hook, Q=eng.modulus)
        lid = eng.lut_register(rng.integers(-8, 8, 16), 4, eng.delta_log())
        got = eng.blind_rotate_host(small, np.full(rows, lid, np.uint32))
        assert np.array_equal(got, o.ctx.blind_rotate(small, eng.lut_get(lid)[None, :], np.zeros(rows, np.uint32), unrolled=True))
    return rng, lid


def check_unrolled_other_shape(e, decrypts, params=None):
    """six bootstraps on an engine of another shape against the oracle's unrolled mode; `decrypts`: the shape can hold a message"""
    with oracle_for(e, unrolled=True, params=params) as o:
        rng = np.random.default_rng(3)
        dl = e.delta_log()
        table = rng.integers(-8, 8, 16)
        lid = e.lut_register(table, 4, dl)
        msgs = rng.integers(-8, 8, 6)
        ct = e.encrypt(msgs, dl)
        got = e.pbs_host(ct, np.full(6, lid, np.uint32))
        if decrypts:
            assert list(e.decrypt(got, dl)) == [int(table[m + 8]) for m in msgs]
        assert np.array_equal(got, o.ctx.pbs(ct, e.lut_get(lid)[None, :], np.zeros(6, np.uint32), unrolled=True))


def check_unrolled_csprng_key_and_evaluation_only_context(q_bits, count):
    """production key generation (no seed): plain keys first, the unrolled key derived from the secrets held and exported to the
    oracle; a second, evaluation-only context imports both evaluation keys and reproduces the same ciphertexts"""
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=q_bits))
    e.keygen()
    e.set_bsk_unroll(2)
    ev = tfhe.Engine(tfhe.default_params(q_bits=q_bits))
    try:
        with oracle_for(e, unrolled=True) as o:
            rng = np.random.default_rng(8)
            dl = e.delta_log()
            table = rng.integers(-8, 8, 16)
            msgs = rng.integers(-8, 8, count)
            ct = e.encrypt(msgs, dl)
            lid = e.lut_register(table, 4, dl)
            got = e.pbs_host(ct, np.full(count, lid, np.uint32))
            assert list(e.decrypt(got, dl)) == [int(table[m + 8]) for m in msgs]
            assert np.array_equal(got, o.ctx.pbs(ct, e.lut_get(lid)[None, :], np.zeros(count, np.uint32), unrolled=True))
            _, _, bsk, ksk = e.export_keys(secret=False)
            ev.import_keys(None, None, bsk, ksk)
            ev.set_bsk_unroll(2)
            with pytest.raises(tfhe.BmiError):      # unrolling selected, no unrolled key yet
                ev.pbs_host(ct, np.full(count, ev.lut_register(table, 4, dl), np.uint32))
            ev.import_bsk_unrolled(e.export_bsk_unrolled())
            assert np.array_equal(ev.pbs_host(ct, np.full(count, ev.lut_register(table, 4, dl), np.uint32)), got)
    finally:
        e.close()
        ev.close()


# ---- the 128-bit-secure torus presets: N = 2048 (secure128_torus) and N = 4096 (secure128_torus_wide)

# seed_offset: added to the tests' base seed for the module's keys; bits: message width of the tables; shape: the preset's (n, N, k,
# bs_levels, bs_base_log, q_bits, ks_levels, ks_base_log); precision / grid_bits: bits the bootstrap key is stored at and the zero low
# bits that leaves; refused: precisions this shape refuses; batch_seed / counts / oracle_rows: of the batch-shape test, the offset of
# its seeds, its batch sizes and the random rows the oracle checks beside the fixed ones; ks_power: how the keyswitch error is
# measured against the analytic value (its variance, or its mean square where the digits' mean leaves a constant offset per key)
TorusPreset = namedtuple("TorusPreset", "name seed_offset bits shape precision grid_bits refused batch_seed counts oracle_rows ks_power")


def check_preset_shape_keys_and_refusals(eng, ora, cfg, seed):
    """the preset's numbers; the key generator reproduces the oracle's word for word up to the rounding of the stored key; what
    the shape refuses (other precisions, unrolling, tables below the key's grid, other decomposition bases)"""
    from bmi_amd import tfhe
    to, P = ora.to, eng.P
    assert (P.n, P.N, P.k, P.bs_levels, P.bs_base_log, P.q_bits, P.ks_levels, P.ks_base_log) == cfg.shape
    assert abs(np.log2(P.lwe_noise) + 17.11) < 0.01 and eng.bsk_precision == cfg.precision == to.default_bsk_precision(ora.P)
    K = to.keygen(ora.P, seed)
    _, _, bsk, ksk = eng.export_keys()
    assert np.array_equal(to.round_key(K.bsk, cfg.precision), bsk) and np.array_equal(K.ksk, ksk) and np.array_equal(K.sk_small, ora.sk_small)
    assert not np.array_equal(K.bsk, bsk) and np.all(bsk & np.uint64((1 << cfg.grid_bits) - 1) == 0)
    e2 = tfhe.Engine(tfhe.preset_params(cfg.name))
    try:
        for bits in cfg.refused:
            with pytest.raises(tfhe.BmiError):
                e2.set_bsk_precision(bits)
        e2.set_bsk_precision(cfg.precision)
        with pytest.raises(tfhe.BmiError):
            e2.set_bsk_unroll(2)
    finally:
        e2.close()
    with pytest.raises(tfhe.BmiError):   # accumulators on the rounded key are multiples of 2^grid_bits: no table below that scale
        eng.lut_register(np.arange(-8, 8), 4, cfg.grid_bits - 1)
    with pytest.raises(tfhe.BmiError):   # the wider rings on the torus: (l, Bg) = (3 or 2, 2^10) only
        tfhe.Engine(tfhe.preset_params(cfg.name, bs_base_log=15))


def torus_batch(eng, count, seed, bits):
    """identity and random tables of `bits` bits, `count` keyswitched encryptions with the adversarial rows written over the first"""
    rng = np.random.default_rng(seed)
    h = 1 << (bits - 1)
    tables = [np.arange(-h, h), rng.integers(-h, h, 2 * h)]
    dl = 64 - 1 - bits
    ids = np.array([eng.lut_register(t, bits, dl) for t in tables], np.uint32)
    tvs = np.stack([eng.lut_get(i) for i in ids])
    msgs = rng.integers(-h, h, count)
    sel = rng.integers(0, 2, count).astype(np.uint32)
    small = eng.keyswitch_host(eng.encrypt(msgs, dl))
    adversarial_rows(small, rng, count)
    return tables, ids, tvs, msgs, sel, small, dl


def check_blind_rotation_every_batch_shape(eng, ora, cfg, count):
    """messages of the preset's width through identity / random tables; adversarial rows; the oracle on a sample"""
    tables, ids, tvs, msgs, sel, small, dl = torus_batch(eng, count, cfg.batch_seed + count, cfg.bits)
    got = eng.blind_rotate_host(small, ids[sel])
    pick = sample_rows(count, [0, 1, 2, 3, 4, count - 1, 255, 256], np.random.default_rng(count), cfg.oracle_rows)
    assert np.array_equal(got[pick], ora.ctx.blind_rotate(small[pick], tvs, sel[pick]))
    ok = np.arange(4, count)
    if ok.size:
        dec = ora.to.decode(ora.to.lwe_phase(ora.sk_big, got[ok]), dl)
        assert list(dec) == [int(tables[s][m + (1 << (cfg.bits - 1))]) for s, m in zip(sel[ok], msgs[ok])]


def check_keyswitch_and_whole_pbs_bit_exact(eng, ora, cfg, seed, repeats, ks_rows, pbs_rows):
    """every message of the preset's width `repeats` times through a random table: keyswitch (the first ks_rows) and the whole PBS
    (pbs_rows random ones) against the oracle, every output decrypted; returns the relative errors of the keyswitched and of the
    bootstrapped ciphertexts, and (ct, lid) for the timing"""
    rng = np.random.default_rng(seed)
    h, dl = 1 << (cfg.bits - 1), 64 - 1 - cfg.bits
    table = rng.integers(-h, h, 2 * h)
    lid = eng.lut_register(table, cfg.bits, dl)
    msgs = np.concatenate([np.arange(-h, h)] * repeats)
    ct = eng.encrypt(msgs, dl)
    small = eng.keyswitch_host(ct)
    assert np.array_equal(small[:ks_rows], ora.ctx.keyswitch(ct[:ks_rows]))
    out = eng.pbs_host(ct, np.full(msgs.size, lid, np.uint32))
    pick = rng.choice(msgs.size, pbs_rows, replace=False)
    assert np.array_equal(out[pick], ora.ctx.pbs(ct[pick], eng.lut_get(lid)[None, :], np.zeros(pbs_rows, np.uint32)))
    assert np.array_equal(eng.decrypt(out, dl), table[msgs + h])
    err = centred_error(ora.to.lwe_phase(ora.sk_small, small), msgs, dl, 1 << 64)
    oerr = centred_error(eng.phase(out), table[msgs + h], dl, 1 << 64)
    return err, oerr, ct, lid


def check_rounding_margin(eng, cfg, count, random_rows, bound):
    """bmi_fft_margin_host: over `count` bootstraps (the first random_rows uniformly random words, which drive the digits to their
    full range) the limb sums stay within `bound` of the integers they are rounded to, and the words equal the product kernel's"""
    rng = np.random.default_rng(12)
    h, dl = 1 << (cfg.bits - 1), 64 - 1 - cfg.bits
    lid = eng.lut_register(rng.integers(-h, h, 2 * h), cfg.bits, dl)
    small = eng.keyswitch_host(eng.encrypt(rng.integers(-h, h, count), dl))
    small[:random_rows] = uniform_words(rng, (random_rows, small.shape[1]))
    ids = np.full(count, lid, np.uint32)
    out, dist = eng.fft_margin_host(small, ids)
    print(f"\n{cfg.name}: largest distance from an integer before rounding 2^{np.log2(max(dist, 1e-300)):.1f}")
    assert 0.0 < dist < bound, dist
    assert np.array_equal(out, eng.blind_rotate_host(small, ids))


def check_l2_shape(cfg, seed, n, bits):
    """(l, Bg) = (2, 2^10), the other instantiated shape of the preset's ring, on nine rows of random words under `bits`-bit tables"""
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.preset_params(cfg.name, bs_levels=2, n=n))
    try:
        e.keygen(seed)
        with oracle_for(e) as o:
            rng = np.random.default_rng(3)
            h = 1 << (bits - 1)
            lid = e.lut_register(rng.integers(-h, h, 2 * h), bits, 64 - 1 - bits)
            small = uniform_words(rng, (9, e.P.small))
            got = e.blind_rotate_host(small, np.full(9, lid, np.uint32))
            assert np.array_equal(got, o.ctx.blind_rotate(small, e.lut_get(lid)[None, :], np.zeros(9, np.uint32)))
    finally:
        e.close()
