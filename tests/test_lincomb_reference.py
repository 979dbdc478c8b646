"""The case table of tests/lincomb_cases.py against the oracle's ora_lincomb, without a GPU: the expected words of the table are
plain Python-integer arithmetic, so this pins the oracle on every modulus at the widths the GPU test uses - coefficients at
both ends of int64 (INT64_MIN is negated in unsigned arithmetic), multiples of Q on the 49-bit field (canonical results),
128-bit totals of either sign - and keeps the table itself honest."""
import numpy as np
import pytest

import lincomb_cases as lc
from oracle import tfhe_oracle as to

SEED = 20
WIDTHS = [1025, 2049, 4097]


@pytest.fixture(params=[64, 49, to.TORUS64], ids=["goldilocks64", "p49", "torus64"])
def field(request):
    q = to.set_field(request.param)
    yield q
    to.set_field(64)


@pytest.mark.parametrize("width", WIDTHS)
def test_oracle_lincomb_matches_integer_reference(field, width):
    Q = field
    store, row_ptr, idx, coef, consts, want = lc.build(Q, width, SEED)
    names = lc.case_names(Q, SEED)
    assert want.shape == (len(names), width) == (row_ptr.size - 1, width)
    got = to.lincomb(width, store, row_ptr, idx, coef, consts)
    assert np.array_equal(got, want), lc.describe_mismatch(got, want, names)
    if Q < 1 << 64:
        assert (got < np.uint64(Q)).all() and (store < np.uint64(Q)).all() and (consts < np.uint64(Q)).all()


def test_case_table_reaches_what_it_claims():
    """the properties the GPU tests rely on, stated on the table itself"""
    for Q in (to.GOLD, to.P49, 1 << 64):
        store, row_ptr, idx, coef, consts, want = lc.build(Q, 1025, SEED)
        names = lc.case_names(Q, SEED)
        count = len(names)
        assert count == (33 if Q == to.P49 else 26) and store.shape == (12, 1025)
        assert row_ptr[0] == 0 and row_ptr[count] == idx.size == coef.size and row_ptr[count // 2] != 0
        lens = np.diff(row_ptr.astype(np.int64))
        assert lens[0] == 0 and 7 in lens and 257 in lens and 64 in lens          # empty, odd, long, circuit-like
        assert {lc.INT64_MIN, lc.INT64_MAX, lc.T, -lc.T, lc.T - 1, -(lc.T - 1)} <= set(int(c) for c in coef)
        # the two long rows drive the signed 128-bit accumulator to a high word far from 0 (2^103 in all on the 64-bit moduli,
        # 2^88 on the 49-bit field), one of each sign
        assert (257 * (lc.T - 1) * (Q - 1)) >> 64 > 1 << 20
        # the identity row reproduces the column pattern; -Q * v and the empty row are 0 away from the body
        assert np.array_equal(want[1, :-1], np.arange(1024, dtype=np.uint64)) and not want[0, :-1].any() and int(want[0, -1]) == Q - 1
        assert int(want[2, -1]) == 0 and (want[2, :-1] == 1).all()
        if Q == to.P49:
            i = names.index(f"{-Q}*row9 (coefficient near a multiple of Q)")
            assert not want[i, :-1].any()
