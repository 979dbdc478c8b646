"""The case table of the leveled-kernel tests (k_lincomb, k_scatter_rows): a store of edge and random rows, CSR output rows
on either side of every branch of the kernel, and the expected words computed with Python integers only - neither the
oracle nor the library takes part in `want`, so both are tested against it (tests/test_lincomb_reference.py on the CPU,
tests/test_gpu_lincomb.py on the GPU).  A plain helper module: no fixtures, no pytest hooks."""
import functools

import numpy as np

INT64_MAX = (1 << 63) - 1
INT64_MIN = -(1 << 63)
T = 1 << 31                     # k_lincomb sums |coef| < 2^31 in 128 bits; anything larger goes through F::mul_small
GOLDEN = 0x9E3779B97F4A7C15
P49 = 562949952700417
STORE_ROWS = 12
# either side of the branch threshold and the ends of int64
BRANCH_COEFS = (T - 1, T, T + 1, -(T - 1), -T, -(T + 1), INT64_MAX, INT64_MIN, INT64_MIN + 1)


def rand_words(rng, shape, Q):
    """uniform canonical words of Z_Q as Python integers: 128 random bits reduced mod Q (bias < 2^-64 on every modulus)"""
    hi = rng.integers(0, 1 << 63, shape, dtype=np.uint64).astype(object) * 2 + rng.integers(0, 2, shape, dtype=np.uint64).astype(object)
    lo = rng.integers(0, 1 << 63, shape, dtype=np.uint64).astype(object) * 2 + rng.integers(0, 2, shape, dtype=np.uint64).astype(object)
    return ((hi << 64) + lo) % Q


def store_rows(Q, width, seed):
    """the 12 store rows as an object array of Python integers (canonical words)"""
    rng = np.random.default_rng([seed, width, Q % (1 << 32)])
    x = np.arange(width, dtype=np.uint64).astype(object)
    s = np.empty((STORE_ROWS, width), dtype=object)
    s[0] = 0
    s[1] = Q - 1
    s[2] = 1
    s[3] = Q // 2
    s[4] = (Q // 2 + 1) % Q
    s[5] = x % Q                     # rows 5 and 6: a column that lands in the wrong block shows
    s[6] = (x * GOLDEN) % Q
    s[7:] = rand_words(rng, (STORE_ROWS - 7, width), Q)
    return s


def output_rows(Q, seed):
    """[(name, [(store row, coefficient), ...], constant or None = random)] - the same list for every width"""
    rng = np.random.default_rng([seed, 0xC5])
    rows = [("empty row, constant Q-1", [], Q - 1),
            ("identity 1*row5, constant 0", [(5, 1)], 0),
            ("-1*row1, constant Q-1 (the body wraps to 0)", [(1, -1)], Q - 1),
            ("0*row7", [(7, 0)], None)]
    for c in BRANCH_COEFS:
        rows.append((f"{c}*row1 (all Q-1)", [(1, c)], None))
        rows.append((f"{c}*row8 (random)", [(8, c)], None))
    if Q == P49:                     # multiples of Q and their neighbours: the results are canonical (-Q*v is 0, not Q)
        for c in (Q, -Q, 2 * Q, -2 * Q, Q - 1, -(Q - 1), Q + 1):
            rows.append((f"{c}*row9 (coefficient near a multiple of Q)", [(9, c)], None))
    rows.append(("7 terms, both branches interleaved",
                 list(zip((7, 8, 9, 1, 3, 4, 6), (3, INT64_MIN, -5, T, -T + 1, INT64_MAX, -7))), None))
    rows.append(("257 x -(2^31-1)*row1 (128-bit total about -2^103)", [(1, -(T - 1))] * 257, None))
    rows.append(("257 x +(2^31-1)*row1 (128-bit total about +2^103)", [(1, T - 1)] * 257, None))
    rows.append(("64 random rows, coefficients in [-75, 75]",
                 [(int(i), int(c)) for i, c in zip(rng.integers(0, STORE_ROWS, 64), rng.integers(-75, 76, 64))], None))
    return rows


def case_names(Q, seed=0):
    return [name for name, _, _ in output_rows(Q, seed)]


def to_u64(a):
    """object array of Python integers in [0, 2^64) -> uint64 array"""
    return np.array([int(v) for v in a.reshape(-1)], dtype=np.uint64).reshape(a.shape)


@functools.lru_cache(maxsize=None)
def build(Q, width, seed):
    """(store, row_ptr, idx, coef, consts, want): read-only arrays, computed once per (Q, width, seed).
    want[i] = (sum_e coef[e] * store[idx[e]] + consts[i] * [x == width - 1]) mod Q, in Python integers."""
    s = store_rows(Q, width, seed)
    rows = output_rows(Q, seed)
    rng = np.random.default_rng([seed, width, 0xC0])
    random_consts = rand_words(rng, len(rows), Q)
    row_ptr, idx, coef, consts = [0], [], [], []
    want = np.empty((len(rows), width), dtype=object)
    for i, (_, terms, const) in enumerate(rows):
        acc = np.zeros(width, dtype=object)
        for r, c in terms:
            assert INT64_MIN <= c <= INT64_MAX and 0 <= r < STORE_ROWS
            idx.append(r)
            coef.append(c)
            acc = acc + c * s[r]
        const = int(random_consts[i]) if const is None else const
        acc[width - 1] += const
        want[i] = acc % Q
        consts.append(const)
        row_ptr.append(len(idx))
    out = (to_u64(s), np.array(row_ptr, np.uint32), np.array(idx, np.uint32), np.array(coef, np.int64),
           np.array(consts, np.uint64), to_u64(want))
    for a in out:
        a.setflags(write=False)
    return out


def describe_mismatch(got, want, names):
    """names of the output rows whose words differ, with the first differing column of each (assertion message)"""
    bad = [i for i in range(want.shape[0]) if not np.array_equal(got[i], want[i])]
    lines = []
    for i in bad:
        x = int(np.flatnonzero(got[i] != want[i])[0])
        lines.append(f"row {i} [{names[i]}]: {int((got[i] != want[i]).sum())} of {want.shape[1]} words, first at column {x}: "
                     f"got {int(got[i, x])}, want {int(want[i, x])}")
    return "\n".join(lines)
