"""Helpers of tests/test_gpu_torus_wide_unrolled.py: the secure128_torus engine in unrolled
mode (N = 2048, bootstrap key at 40 bits: k_blind_rotate_wu_t64f, csrc/bmi_kernels_t64wu.hip), the rows that drive its edges and
the oracle on its exported keys.  A plain helper module: no fixtures, no pytest hooks."""
import numpy as np

import pbs_cases as pc

PRESET = "secure128_torus"
PREC = 40
GRID_MASK = (1 << 24) - 1      # the 40-bit key: every key and accumulator word on the 2^24 grid


def engine(seed, **kw):
    """preset_params("secure128_torus", ...) + set_bsk_unroll(2): the call selects the 40-bit key by itself"""
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.preset_params(PRESET, **kw))
    e.set_bsk_unroll(2)
    assert e.bsk_precision == PREC
    e.keygen(seed)
    return e


def edge_rows(rng, width):
    """nine rows of small-key words: uniformly random, all zero (no step), all ones (every exponent 0), every a = N (the pair
    sums wrap to 0 mod 4096 while a, a' != 0), the first / the second coefficient of every pair zero, a whole pair zero every
    eighth step (the accumulator is re-centred every eight steps TAKEN), a = 1 everywhere, uniformly random again"""
    small = pc.uniform_words(rng, (9, width))
    small[1] = 0
    small[2] = np.uint64(0xFFFFFFFFFFFFFFFF)
    small[3] = np.uint64(1 << 63)
    small[4, ::2] = 0
    small[5, 1::2] = 0
    small[6, 14::16] = 0
    small[6, 15::16] = 0
    small[7, :-1] = np.uint64(1 << 52)      # 2^64 / 4096: a = 1
    return small


def batch(eng, rng, count):
    """`count` rows: the edge rows first (as many as fit), uniformly random words behind them; two tables picked at random"""
    dl = eng.delta_log()
    ids = np.array([eng.lut_register(rng.integers(-8, 8, 16), 4, dl) for _ in range(2)], np.uint32)
    small = pc.uniform_words(rng, (count, eng.P.small))
    edges = edge_rows(rng, eng.P.small)
    if count > 1:                           # (a batch of one stays uniformly random)
        small[:min(count, 9)] = edges[:min(count, 9)]
    sel = rng.integers(0, 2, count).astype(np.uint32)
    return small, ids, sel


def oracle_rotation(eng, o, small, ids, sel, pick):
    """the oracle's unrolled blind rotation of the rows `pick` on the engine's exported keys"""
    tvs = np.stack([eng.lut_get(i) for i in ids])
    return o.ctx.blind_rotate(small[pick], tvs, sel[pick], unrolled=True)
