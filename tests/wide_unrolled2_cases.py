"""Helpers of tests/test_gpu_torus_wide_unrolled2.py: the rows that put two ciphertexts with DIFFERENT steps into one workgroup of
k_blind_rotate_wu2_t64f (csrc/bmi_kernels_t64wu2.hip: workgroup w holds rows 2w and 2w + 1), beside the engine and the oracle of
wide_unrolled_cases.py.  A plain helper module: no fixtures, no pytest hooks."""
import numpy as np

import pbs_cases as pc

WU = "k_blind_rotate_wu_t64f"
WU2 = "k_blind_rotate_wu2_t64f"
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
PAIRED_FROM, PAIRED_TO = 8, 16      # the rows paired_rows places, after the seven of pbs_cases.extreme_rows_unrolled


def exponents(row):
    """the mod-switched mask words of a small-key row at N = 2048: round(a 4096 / 2^64) mod 4096, ties up"""
    a = np.asarray(row[:-1], dtype=np.uint64)
    return (((a >> np.uint64(51)) + np.uint64(1)) >> np.uint64(1)) & np.uint64(4095)


def pair_is_live(row):
    """per pair of mask words (an odd n is completed by a' = 0): does the row take that step?"""
    e = exponents(row)
    if e.size % 2:
        e = np.concatenate([e, np.zeros(1, np.uint64)])
    return (e.reshape(-1, 2) != 0).any(axis=1)


def zero_pairs(row, pairs):
    n = row.size - 1
    for p in pairs:
        row[2 * p:min(2 * p + 2, n)] = 0


def paired_rows(rng, count, width):
    """`count` >= 16 rows of small-key words: pbs_cases.extreme_rows_unrolled (rows 0 .. 6, random ones behind them) and four
    workgroups built on purpose -
      (8, 9)    a dense row beside a row of all-ones words (every exponent 0: no step, the extraction of the test polynomial)
      (10, 11)  a dense row beside a row whose every second pair is zero (steps of one ciphertext only: its partner's factors are 0)
      (12, 13)  two rows that are zero on the same pairs (1 and 5: the workgroup skips the step)
      (14, 15)  a row that takes every step beside one that skips pair 2 (and pair 9 where n > 18): different counts, and beyond
                eight pairs the re-centring falls at different steps of the two"""
    n = width - 1
    pairs = (n + 1) // 2
    small = pc.extreme_rows_unrolled(rng, count, width, skipped_pairs=True)
    small[9] = ONES
    zero_pairs(small[11], range(0, pairs, 2))
    for r in (12, 13):
        zero_pairs(small[r], [p for p in (1, 5) if p < pairs])
    zero_pairs(small[15], [p for p in (2, 9) if p < pairs])
    # what the rows were built for holds on these very words
    live = np.stack([pair_is_live(small[r]) for r in range(PAIRED_FROM, PAIRED_TO)])
    assert live[0].all() and not live[1].any() and not exponents(small[9]).any()
    assert live[2].all() and not live[3][0::2].any() and live[3][1::2].all()
    assert np.array_equal(live[4], live[5]) and not live[4].all() and live[4].any()
    assert live[6].all() and live[6].sum() > live[7].sum() and (pairs < 11 or live[7].sum() > 8)
    return small


def batch(eng, rng, count):
    """paired_rows and two tables picked at random per row"""
    dl = eng.delta_log()
    ids = np.array([eng.lut_register(rng.integers(-8, 8, 16), 4, dl) for _ in range(2)], np.uint32)
    sel = rng.integers(0, 2, count).astype(np.uint32)
    return paired_rows(rng, count, eng.P.small), ids, sel
