"""Host-side scheduler (bmi_amd.qfloat / base_p_arrays / qfloat_matrix_inversion / circuit) on CPU:
  * plaintext mode (digits are ints) against the reference-generated goldens, incl. the reference's own
    tests/test_qfloat.py cases (with two-sided tolerances);
  * encrypted mode traced into the PBS circuit and evaluated with Circuit.simulate (the analogue of
    circuit.simulate) against the same goldens — bit-exact digits and signs, every interval claim checked."""
import json
import os

import numpy as np
import pytest

from bmi_amd import qfloat_matrix_inversion as qmi
from bmi_amd.circuit import Circuit, Lin, RangeError
from bmi_amd.main import EncryptedMatrixInversion, trace_inverse
from bmi_amd.qfloat import QFloat, SignedBinary, Zero

G = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    with open(os.path.join(G, name)) as f:
        return json.load(f)


def same_plain(q, g):
    assert [int(x) for x in q.array] == g["array"]
    assert int(q.sign) == g["sign"] and q.ints == g["ints"] and q.base == g["base"]


# ------------------------------------------------------------------------------ plaintext mode
def test_plaintext_kats_and_str():
    k = load("kats.json")
    assert str(QFloat.from_float(103.785, 24, 8, 2)) == "01100111.1100100011110101"
    assert str(QFloat.from_float(13.75, 10, 5, 2)) == "01101.11000"      # reference tests/test_qfloat.py:40-55
    assert str(QFloat.from_float(-13.75, 10, 5, 2)) == "-01101.11000"
    assert str(QFloat.from_float(0, 10, 5, 2)) == "00000.00000"
    q = QFloat.from_float(1, 10, 5, 2)
    q._sign = 0
    assert str(q) == "00000.00000"
    same_plain(QFloat(np.array([0, 3, -5, 7, -2, 1]), 3, 2, False), k["base_tidy_0_3_-5_7_-2_1"])
    same_plain(QFloat(np.array([5, 0, 0, 0]), 2, 2, False), k["base_tidy_5_0_0_0"])
    same_plain(QFloat.from_float(2.5, 10, 5, 2) + QFloat.from_float(-2.5, 10, 5, 2), k["add_2.5_-2.5"])
    same_plain(QFloat.from_float(1.75, 8, 4, 2) * QFloat.from_float(0.0625, 8, 4, 2), k["mul_1.75_0.0625_8_4"])
    same_plain(QFloat.from_float(5, 10, 5, 2) / QFloat.from_float(3, 10, 5, 2), k["div_5_3_10_5"])
    same_plain(QFloat.from_float(3, 10, 5, 2).invert(1, 10, 0), k["invert_3_10_0"])
    same_plain(QFloat.from_float(5, 10, 5, 2) / SignedBinary(0), k["div_5_by_sb0"])
    assert QFloat.from_float(0, 10, 5, 2).sign == 1


def test_plaintext_ops_match_goldens():
    g = load("qfloat_ops.json")
    for c in g["pairs"]:
        q1 = QFloat.from_float(c["f1"], c["len"], c["ints"], c["base"])
        q2 = QFloat.from_float(c["f2"], c["len"], c["ints"], c["base"])
        same_plain(q1 + q2, c["add"])
        same_plain(q1 - q2, c["sub"])
        same_plain(q1 + 2, c["add_int2"])
        same_plain(2 - q1, c["rsub_int2"])
        same_plain(SignedBinary(1) + q1, c["add_sb1"])
        same_plain(SignedBinary(1) - q1, c["rsub_sb1"])
        same_plain(q1 * q2, c["mul"])
        same_plain(q1 * 2, c["mul_int"])
        same_plain(-3 * q1, c["mul_intm3"])
        same_plain(q1 * SignedBinary(-1), c["mul_sbm1"])
        same_plain(QFloat.from_mul(q1, q2), c["from_mul"])
        f = c["from_mul_fmt"]
        same_plain(QFloat.from_mul(q1, q2, f["newlen"], f["newints"]), f)
        same_plain(abs(q1), c["abs"])
        assert int(q1 > q2) == c["gt"] and int(q1 >= q2) == c["ge"] and int(q1 < q2) == c["lt"]
        assert int(q1 <= q2) == c["le"] and int(q1 == q2) == c["eq"]
        if "div" in c:
            same_plain(q1 / q2, c["div"])
            f = c["invert_fmt"]
            same_plain(q2.invert(1, f["newlen"], f["newints"]), f)
            same_plain(SignedBinary(-1) / q2, c["invert_m1"])
    for c in g["tidy"]:
        q = QFloat(np.array(c["in"]), c["ints"], c["base"], False)
        same_plain(q, c["base_tidy"])
        q.tidy()
        same_plain(q, c["tidy"])


def test_reference_unit_test_patterns_two_sided():
    """The reference's randomized checks (tests/test_qfloat.py:22-224) with abs() tolerances."""
    rng = np.random.default_rng(5)
    for _ in range(25):
        ints = int(rng.integers(8, 12))
        f1 = (int(rng.integers(0, 20000)) - 10000) / 100
        f2 = (int(rng.integers(0, 20000)) - 10000) / 100
        q1, q2 = QFloat.from_float(f1, 32, ints, 2), QFloat.from_float(f2, 32, ints, 2)
        assert abs(q1.to_float() - f1) < 0.1 and q1.sign == (np.sign(f1) or 1)
        assert abs((q1 + q2).to_float() - (f1 + f2)) < 0.1 and abs((q1 - q2).to_float() - (f1 - f2)) < 0.1
        assert abs((2 + q1).to_float() - (2 + f1)) < 0.1 and abs((SignedBinary(1) - q1).to_float() - (1 - f1)) < 0.1
        z = q1.copy()
        z._sign = 0
        assert abs((z + q2).to_float() - f2) < 0.1 and (z * q2).to_float() == 0
        g1, g2 = (int(rng.integers(0, 200)) - 100) / 10 or 1.0, (int(rng.integers(0, 200)) - 100) / 10 or 1.0
        p1, p2 = QFloat.from_float(g1, 32, 11, 2), QFloat.from_float(g2, 32, 11, 2)
        assert abs((p1 * p2).to_float() - g1 * g2) < 0.1 and abs((p1 / p2).to_float() - g1 / g2) < 0.1
        assert abs((SignedBinary(-1) / p1).to_float() + 1.0 / g1) < 0.1
        assert abs((p1 / SignedBinary(0)).to_float()) > 1000  # overflow on division by zero
        assert int(p1 >= p2) == int(g1 >= g2)
    assert (QFloat.from_float(1.0, 10, 5, 2) + Zero()) is None  # reference quirk qfloat.py:803-804
    with pytest.raises(ValueError):
        QFloat(np.zeros((2, 2)))
    with pytest.raises(ValueError):
        QFloat(np.zeros(4), 9)
    with pytest.raises(ValueError):
        QFloat.from_float(1.0, 8, 4, 2).check_compatibility(QFloat.from_float(1.0, 8, 3, 2))
    with pytest.raises(ValueError):
        Zero() / Zero()


# ------------------------------------------------------------------------------ encrypted mode (traced)
def enc_q(c, g, top=3):
    """declare circuit inputs for a QFloat fixture; returns (QFloat over Lin, flat input values)"""
    base = g["base"]
    digits = [c.input(0, max(base - 1, top if i == 0 else base - 1)) for i in range(len(g["array"]))]
    sign = c.input(-1, 1)
    return QFloat(digits, g["ints"], base, True, sign), list(g["array"]) + [g["sign"]]


def run_traced(build, fixtures):
    """build(c, *encrypted QFloats) -> QFloat or scalar; returns simulated (digits, sign) or scalar"""
    c = Circuit()
    qs, vals = [], []
    for g in fixtures:
        q, v = enc_q(c, g)
        qs.append(q)
        vals += v
    res = build(c, *qs)
    if isinstance(res, QFloat):
        outs = list(res.array) + [res.sign]
    else:
        outs = [res]
    c.set_outputs(outs)
    out = c.simulate(vals)
    return out, c


def same_traced(out, g):
    assert out[:-1] == g["array"], (out[:-1], g["array"])
    assert out[-1] == g["sign"]


def test_traced_ops_match_goldens():
    g = load("qfloat_ops.json")
    n_checked = 0
    for c in g["pairs"]:
        if c["base"] != 2:
            continue
        a, b = c["q1"], c["q2"]
        same_traced(run_traced(lambda cc, x, y: x + y, [a, b])[0], c["add"])
        same_traced(run_traced(lambda cc, x, y: x - y, [a, b])[0], c["sub"])
        same_traced(run_traced(lambda cc, x: x + 2, [a])[0], c["add_int2"])
        same_traced(run_traced(lambda cc, x: 2 - x, [a])[0], c["rsub_int2"])
        same_traced(run_traced(lambda cc, x: SignedBinary(1) - x, [a])[0], c["rsub_sb1"])
        same_traced(run_traced(lambda cc, x, y: x * y, [a, b])[0], c["mul"])
        same_traced(run_traced(lambda cc, x: x * SignedBinary(-1), [a])[0], c["mul_sbm1"])
        f = c["from_mul_fmt"]
        same_traced(run_traced(lambda cc, x, y: QFloat.from_mul(x, y, f["newlen"], f["newints"]), [a, b])[0], f)
        same_traced(run_traced(lambda cc, x: abs(x), [a])[0], c["abs"])
        assert run_traced(lambda cc, x, y: x > y, [a, b])[0] == [c["gt"]]
        assert run_traced(lambda cc, x, y: x >= y, [a, b])[0] == [c["ge"]]
        assert run_traced(lambda cc, x, y: x <= y, [a, b])[0] == [c["le"]]
        assert run_traced(lambda cc, x, y: x == y, [a, b])[0] == [c["eq"]]
        if "div" in c:
            same_traced(run_traced(lambda cc, x, y: x / y, [a, b])[0], c["div"])
            fi = c["invert_fmt"]
            same_traced(run_traced(lambda cc, y: y.invert(1, fi["newlen"], fi["newints"]), [b])[0], fi)
            same_traced(run_traced(lambda cc, y: SignedBinary(-1) / y, [b])[0], c["invert_m1"])
        n_checked += 1
        if n_checked >= 12:
            break
    assert n_checked >= 8
    for c in g["from_mul_mixed"][:4]:
        same_traced(run_traced(lambda cc, x, y: QFloat.from_mul(x, y, 18, 1), [c["q1"], c["q2"]])[0], c["out"])


@pytest.mark.parametrize("bits", [1, 2, 3])
def test_traced_division_every_radix(bits):
    """x / y, y.invert and -1 / y with 1, 2 and 3 quotient bits per step (radix 2, 4, 8, odd and even dividend
    lengths): every radix must return the reference's restoring-division digits."""
    from bmi_amd import base_p_arrays as bpa
    g = load("qfloat_ops.json")
    saved = bpa.DIVISION_BITS
    bpa.DIVISION_BITS = bits
    try:
        n_checked = 0
        for c in g["pairs"]:
            if c["base"] != 2 or "div" not in c:
                continue
            a, b = c["q1"], c["q2"]
            same_traced(run_traced(lambda cc, x, y: x / y, [a, b])[0], c["div"])
            fi = c["invert_fmt"]
            same_traced(run_traced(lambda cc, y: y.invert(1, fi["newlen"], fi["newints"]), [b])[0], fi)
            same_traced(run_traced(lambda cc, y: SignedBinary(-1) / y, [b])[0], c["invert_m1"])
            n_checked += 1
            if n_checked >= 6:
                break
        assert n_checked >= 4
    finally:
        bpa.DIVISION_BITS = saved


def test_wide_odd_lookup_and_lookahead_networks():
    """Circuit.lut_odd (5-bit inputs for functions with f(v - 16) = -f(v)) and the look-ahead networks built on it:
    window-4 signals and the three-way combine on every input; subtraction with borrow-out against integer
    arithmetic for widths on both sides of every depth step, wide and 4-bit-only forms giving the same digits with
    the wide one never deeper."""
    import itertools
    import random
    from bmi_amd import base_p_arrays as bpa
    from bmi_amd.circuit import RangeError
    sgn = lambda v: (v > 0) - (v < 0)  # noqa: E731
    c = Circuit()
    d = [c.input(-1, 1) for _ in range(4)]
    s3 = [c.input(-1, 1) for _ in range(3)]
    c.set_outputs([c.lut_odd(d[3] * 8 + d[2] * 4 + d[1] * 2 + d[0], sgn), c.lut_odd(s3[2] * 9 + s3[1] * 3 + s3[0], bpa._comb3)])
    assert len(c.wide_leaves) == 2
    for vals in itertools.product((-1, 0, 1), repeat=7):
        w = 8 * vals[3] + 4 * vals[2] + 2 * vals[1] + vals[0]
        t = vals[6] if vals[6] else (vals[5] if vals[5] else vals[4])
        assert c.simulate(list(vals)) == [sgn(w), t]
    c2 = Circuit()
    x = c2.input(-15, 15)
    with pytest.raises(RangeError):
        c2.lut_odd(x, lambda v: int(v < 0))          # a bit is not an odd function
    with pytest.raises(RangeError):
        c2.lut_odd(c2.input(-16, 15) if False else x + x, sgn)   # interval beyond the torus
    saved = bpa.WIDE_LOOKAHEAD
    try:
        for m in (1, 3, 4, 12, 13, 24, 25, 33, 37):
            depth = {}
            for wide in (True, False):
                bpa.WIDE_LOOKAHEAD = wide
                cc = Circuit()
                a = [cc.input(0, 1) for _ in range(m)]
                b = [cc.input(0, 1) for _ in range(m)]
                out, lt = bpa.base_p_subtraction(cc, a, b, 2, True)
                ge = bpa.is_greater_or_equal(cc, a, b)
                cc.set_outputs(out + [lt, ge])
                depth[wide] = len(cc.asap_levels())
                rng = random.Random(m)
                for k in range(40):
                    av = [rng.randint(0, 1) for _ in range(m)]
                    bv = list(av) if k % 4 == 0 else [rng.randint(0, 1) for _ in range(m)]
                    if k % 5 == 1:
                        bv = list(av)
                        bv[rng.randrange(m)] ^= 1
                    A, B = int("".join(map(str, av)), 2), int("".join(map(str, bv)), 2)
                    want = [int(ch) for ch in bin((A - B) % (1 << m))[2:].zfill(m)] + [int(A < B), int(A >= B)]
                    assert cc.simulate(av + bv) == want, (m, wide)
            assert depth[True] <= depth[False]
        assert depth[True] < depth[False]                # at 37 digits: 4 levels against 5
    finally:
        bpa.WIDE_LOOKAHEAD = saved


def test_circuit_message_width_is_configurable():
    """Circuit(msg_bits=6): 64-value look-ups, 8 x 8 packed bivariate ones and 7-bit odd ones (what the N = 4096
    parameter set carries); the default stays 4 bits and rejects the same look-ups."""
    import random
    c = Circuit(msg_bits=6)
    x, a, b, w = c.input(-32, 31), c.input(0, 7), c.input(0, 7), c.input(-63, 63)
    f = lambda v: (v * v) % 64 - 32  # noqa: E731
    g = lambda u, v: (u * v) % 61 - 30  # noqa: E731
    sgn = lambda v: (v > 0) - (v < 0)  # noqa: E731
    c.set_outputs([c.lut(x, f), c.lut2(a, b, g), c.lut_odd(w, sgn)])
    assert c.luts[0][0] == 6 and len(c.luts[0][1]) == 64
    rng = random.Random(1)
    for _ in range(200):
        xv, av, bv, wv = rng.randint(-32, 31), rng.randint(0, 7), rng.randint(0, 7), rng.randint(-63, 63)
        assert c.simulate([xv, av, bv, wv]) == [f(xv), g(av, bv), sgn(wv)]
    c4 = Circuit()
    with pytest.raises(RangeError):
        c4.lut(c4.input(-32, 31), f)


def test_width_aware_level_schedule_properties():
    """Circuit.levels(): same depth as ASAP, every node after its producers, all nodes scheduled exactly once, and no
    level wider than the rounds its critical nodes need (random layered circuits + the traced 2x2 inverse)."""
    import random

    def check(c):
        asap = c.asap_levels()
        lv = c.levels()
        assert len(lv) == len(asap)
        pos = {}
        for li, level in enumerate(lv):
            for i in level:
                assert i not in pos
                pos[i] = li
        assert len(pos) == len(c.nodes)
        producer = {leaf: i for i, (_, _, _, leaf) in enumerate(c.nodes)}
        for i, (terms, _, _, _) in enumerate(c.nodes):
            for t, _ in terms:
                if t in producer:
                    assert pos[producer[t]] < pos[i]
        cost = lambda w: -(-w // 256) if w <= 512 else 2.45 * -(-w // 1024)  # noqa: E731  (rounds, in latency-round units)
        assert sum(cost(len(x)) for x in lv) <= sum(cost(len(x)) for x in asap) + 1e-9
        return lv

    rng = random.Random(3)
    for trial in range(3):
        c = Circuit()
        pool = [c.input(0, 1) for _ in range(40)]
        for depth in range(12):
            width = rng.choice([30, 200, 300, 600])
            new = []
            for _ in range(width):
                a, b = rng.sample(pool[-400:], 2)
                new.append(c.lut(a + b, lambda v: int(v == 1)))
            pool += new
        c.set_outputs(pool[-5:])
        check(c)
    lv = check(trace_inverse(2, 20, 8, 2, False, False))
    assert max(len(x) for x in lv) <= 512


def test_traced_tidy_on_mixed_sign_digits():
    """Pattern of the reference's test_tidy_np (tests/test_qfloat.py:191-213) on encrypted digits.  The
    reference draws untidy digits in [-4b, 4b), which only its plaintext mode can hold; on ciphertexts a
    digit plus carry must fit one 4-bit look-up, so digits are drawn in [-3, 3]; expected values come from
    the (golden-pinned) oracle."""
    from oracle import qfloat_oracle as qo
    rng = np.random.default_rng(11)
    for _ in range(20):
        size = int(rng.integers(8, 20))
        ints = int(rng.integers(size // 2 - 2, size // 2 + 2))
        arr = rng.integers(-3, 4, size)
        want = qo.Q(arr.copy(), ints, 2, False)
        want.tidy()
        circ = Circuit()
        ins = [circ.input(-3, 3) for _ in range(size)]
        q = QFloat(ins, ints, 2, False)   # base_tidy in the constructor (signed carry chain)
        q.tidy()
        circ.set_outputs(list(q.array) + [q.sign])
        out = circ.simulate([int(x) for x in arr])
        assert out[:-1] == [int(x) for x in want.d] and out[-1] == int(want.sign)


def _plain_add(d1, s1, d2, s2, ints):
    """the reference's steps in plaintext mode (digits are ints: QFloat.__iadd__ runs digit-times-sign, the carry chain and
    tidy - pinned to the reference's goldens above)"""
    a = QFloat(np.array(d1), ints, 2, True, s1)
    b = QFloat(np.array(d2), ints, 2, True, s2)
    a += b
    return [int(x) for x in a.array], int(a.sign)


@pytest.mark.parametrize("size", [1, 2, 3, 4, 5, 9, 13, 30, 37])
def test_fused_signed_addition_equals_the_reference_steps(size):
    """QFloat += QFloat on encrypted base-2 digits takes base_p_arrays.signed_add_binary (three look-aheads in parallel and a
    packed selection: four levels) instead of the reference's digit-times-sign sum, truncating carry chain and tidy.  Same
    integers on random operands - leading digits up to 3 (from_float does not reduce them), signs -1 / 0 / +1 (a zero sign
    makes the digits irrelevant), results that overflow the format, equal magnitudes, zeros - and every interval claim holds."""
    rng = np.random.default_rng(100 + size)
    ints = size // 2
    circ = Circuit()
    da = [circ.input(0, 3 if i == 0 else 1) for i in range(size)]
    db = [circ.input(0, 3 if i == 0 else 1) for i in range(size)]
    sa, sb = circ.input(-1, 1), circ.input(-1, 1)
    q = QFloat(list(da), ints, 2, True, sa)
    q += QFloat(list(db), ints, 2, True, sb)
    assert q._neg is not None                         # went through the fused path
    circ.set_outputs(list(q.array) + [q.sign])
    depth = max(circ.leaf_level)
    assert depth <= (9 if size > 36 else 8)           # operands with signs that may be zero and wide leading digits: 1 + 1 + 4 (+ sign 2)
    cases = []
    for t in range(300):
        x = rng.integers(0, 2, size)
        y = rng.integers(0, 2, size)
        if t % 3 == 0:
            x[0], y[0] = rng.integers(0, 4), rng.integers(0, 4)
        if t % 7 == 0:
            y = x.copy()                              # equal magnitudes: opposite signs cancel to +0
        if t % 11 == 0:
            x[:] = 0
        if t % 13 == 0:
            y[:] = 0
        if t % 17 == 0:
            x[:], y[:] = 1, 1                         # overflows when the signs agree
        s1, s2 = (int(rng.choice([-1, 1])), int(rng.choice([-1, 1]))) if t % 5 else (int(rng.integers(-1, 2)), int(rng.integers(-1, 2)))
        cases.append((x, s1, y, s2))
    for x, s1, y, s2 in cases:
        want_d, want_s = _plain_add(x, s1, y, s2, ints)
        out = circ.simulate([int(v) for v in x] + [int(v) for v in y] + [s1, s2])
        assert out[:-1] == want_d and out[-1] == want_s, (list(x), s1, list(y), s2, out, want_d, want_s)


def test_fused_addition_chain_scalars_and_depth():
    """A chain of additions costs four levels each once the operands carry their sign as a bit; scalars in {-1, 0, 1} (plain,
    SignedBinary, encrypted) enter at digit ints - 1 like in the reference; operands the fused form does not cover (a scalar
    beyond [-1, 1], another base) still take the reference's steps.  All against the plaintext mode."""
    rng = np.random.default_rng(5)
    size, ints = 12, 5
    circ = Circuit()
    ops = [([circ.input(0, 1) for _ in range(size)], circ.input(-1, 1)) for _ in range(4)]
    v_enc = circ.input(-1, 1)
    q = QFloat(list(ops[0][0]), ints, 2, True, ops[0][1])
    levels = []
    for d, sg in ops[1:]:
        q += QFloat(list(d), ints, 2, True, sg)
        levels.append(max(circ.leaf_level[t] for x in q.array if isinstance(x, Lin) for t in x.terms))
    assert levels[1] - levels[0] <= 4 and levels[2] - levels[1] <= 4      # digits: at most four levels per chained addition (12 digits: 2 + 1, the sign path may add one)
    q = q - SignedBinary(v_enc)          # r = -other; r += self with an encrypted ternary scalar
    q = 1 - q
    q += SignedBinary(-1)
    q += 0
    wide = q + 2                          # beyond [-1, 1]: the reference's steps
    circ.set_outputs(list(q.array) + [q.sign] + list(wide.array) + [wide.sign])
    for _ in range(200):
        vals, plain = [], []
        for _k in range(4):
            d = rng.integers(0, 2, size)
            sg = int(rng.choice([-1, 1]))
            vals += [int(x) for x in d] + [sg]
            plain.append(QFloat(np.array(d), ints, 2, True, sg))
        v = int(rng.integers(-1, 2))
        p = plain[0]
        for o in plain[1:]:
            p += o
        p = p - SignedBinary(v)
        p = 1 - p
        p += SignedBinary(-1)
        p += 0
        pw = p + 2
        out = circ.simulate(vals + [v])
        assert out == [int(x) for x in p.array] + [int(p.sign)] + [int(x) for x in pw.array] + [int(pw.sign)]


def test_sign_to_bit_lookup_on_the_whole_torus():
    """Circuit.lut_neg: [v < 0] for v in [-15, 15] as ONE look-up (the constant test polynomial at half the output scale; the
    consumers' constants absorb Delta / 2 - program.half_unit_consts).  Every value, through Circuit.simulate, through the frozen
    Program and through a serialisation round trip; narrow inputs fall back to ordinary look-ups; out-of-range inputs raise."""
    from bmi_amd.program import Program
    c = Circuit()
    a = [c.input(0, 1) for _ in range(4)]
    b = [c.input(0, 1) for _ in range(4)]
    w = sum((a[i] - b[i]) * (1 << i) for i in range(4))          # a window of four digit differences: [-15, 15]
    bit = c.lut_neg(w)
    assert isinstance(bit, Lin) and (bit.lo, bit.hi) == (0, 1) and len(c.nodes) == 1
    assert c.lut_neg(w) is not bit and len(c.nodes) == 1           # shared (CSE)
    narrow = c.lut_neg(a[0] - b[0])                                # fits the ordinary message space: an ordinary look-up
    total = bit * 3 + narrow - 1                                   # a consumer with a coefficient: owes 3 Delta / 2
    c.set_outputs([bit, total])
    assert c.lut_neg(5) .const == 0 and c.lut_neg(-5).const == 1
    with pytest.raises(RangeError):
        c.lut_neg(w * 2)
    prog = Program.from_circuit(c)
    assert prog.node_half.sum() == 1 and prog.lut_half.sum() == 1
    consts = prog.half_unit_consts(prog.out_ptr, prog.out_leaf, prog.out_coef, prog.out_const)
    assert consts.tolist() == [1, 2 * (-1) + 3]                    # units of Delta / 2
    back = Circuit.from_dict(json.loads(json.dumps(c.to_dict())))
    for x in range(16):
        for y in range(16):
            vals = [(x >> i) & 1 for i in range(4)] + [(y >> i) & 1 for i in range(4)]
            want = [int(x < y), 3 * int(x < y) + int((x & 1) < (y & 1)) - 1]
            assert c.simulate(vals) == want and prog.simulate(vals) == want and back.simulate(vals) == want


def test_circuit_guards():
    c = Circuit()
    x = c.input(0, 40)
    with pytest.raises(RangeError):
        c.lut(x, lambda v: v)              # wider than the 4-bit message space
    y = c.input(0, 1)
    with pytest.raises(ValueError):
        c.input(0, 1) if c.lut(y, lambda v: 1 - v) is None else (_ for _ in ()).throw(ValueError())
    c2 = Circuit()
    a = c2.input(0, 1)
    bad = (a + 5).assume(5, 5)             # a claim that is false when a = 1
    c2.set_outputs([bad])
    with pytest.raises(RangeError):
        c2.simulate([1])
    with pytest.raises(RangeError):
        c2.simulate([2])                   # input outside its declared interval
    # CSE: identical look-ups are shared
    c3 = Circuit()
    u = c3.input(-2, 2)
    p, q = u.lt0(), u.lt0()
    assert c3.stats["pbs"] == 1 and c3.stats["cse_hits"] == 1 and isinstance(p, Lin) and q.terms == p.terms


CASES = load("inverse.json")     # every golden: all BASELINE configs incl. 8x8 (len 48, ints 16), base 3 (5-bit look-ups)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["tag"])
def test_traced_inverse_matches_reference_golden(case):
    c = case
    emi = EncryptedMatrixInversion(c["n"], None, c["base"], c["len"], c["ints"], c["true_division"], c["tensorize"])
    M = np.array(c["M"]).reshape(c["n"], c["n"])
    q, s = emi.quantize(M)
    assert q.tolist() == c["in_arrays"] and s.tolist() == c["in_signs"]
    out = emi.simulate(q, s)
    assert out.tolist() == c["out"]
    assert QFloat.ADDITIONS >= 0  # stats exist (trace-time counts)
    got = emi.run(M, simulate=True)
    assert got.flatten().tolist() == c["float"]
    summ = emi.circuit.summary()
    assert summ["pbs"] > 0 and summ["depth"] > 0
    assert [summ["additions"], summ["multiplications"], summ["divisions"]] == c["stats"]   # the reference's op counters


def test_trace_stats_match_reference_counts():
    trace_inverse(2, 20, 8)
    assert [QFloat.ADDITIONS, QFloat.MULTIPLICATION, QFloat.DIVISION] == [1, 6, 1]
    trace_inverse(3, 18, 8)
    assert [QFloat.ADDITIONS, QFloat.MULTIPLICATION, QFloat.DIVISION] == [41, 29, 6]


def test_encrypt_rejects_out_of_range_inputs():
    emi = EncryptedMatrixInversion(2, None, 2, 16, 7)
    q, s = emi.quantize(np.array([[5000.0, 1.0], [2.0, 3.0]]))  # leading digit far above 3
    with pytest.raises(ValueError):
        emi.simulate(q, s)


def test_evaluate_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bmi_amd import tfhe
    emi = EncryptedMatrixInversion(2, None, 2, 16, 7)
    with pytest.raises(tfhe.BmiError):
        emi.keygen()


def test_reference_functions_traced_unmodified_simulate():
    """tests/golden/ref_traced.json (tools/gen_ref_traced.py): the reference's UNMODIFIED base_p_arrays / QFloat functions,
    traced in the build container through the Concrete-compatible front end (bmi_amd/compat) into this IR and stored as data.
    The deserialised circuits must reproduce the reference's own plaintext outputs recorded beside them."""
    data = load("ref_traced.json")
    assert len(data["cases"]) >= 9
    for case in data["cases"]:
        c = Circuit.from_dict(case["circuit"])
        assert len(c.nodes) == case["pbs"] and len(c.levels()) == case["depth"]
        assert Circuit.from_dict(c.to_dict()).to_dict() == c.to_dict()
        for v in case["vectors"]:
            assert c.simulate(v["inputs"]) == v["expected"], case["name"]


def load_gz(name):
    import gzip
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name), "rt") as f:
        return json.load(f)


def test_reference_whole_inverse_traced_unmodified_simulate():
    """tests/golden/ref_traced_inverse.json.gz: the reference's UNMODIFIED `qfloat_matrix_inverse`
    (qfloat_matrix_inversion.py:672-720, with everything it calls in qfloat.py / base_p_arrays.py) traced through
    bmi_amd/compat at BASELINE.json's sizes (2x2 len 20 ints 8; 3x3 len 30 ints 12), ranges measured on a 2,000-matrix
    inputset as Concrete's compiler does; the third case is the 2x2 again with the shim's lazy look-up fusion (values
    that are univariate in one linear combination stay tables until they meet another one: 374 -> 306 levels).  The
    stored circuits reproduce the reference's own plaintext outputs, and our
    restated, fused circuits give the same digits on the same matrices at a fraction of the depth."""
    data = load_gz("ref_traced_inverse.json.gz")
    assert [(c["n"], c["lazy_lookup_fusion"]) for c in data["cases"]] == [(2, False), (3, False), (2, True)]
    for case in data["cases"]:
        c = Circuit.from_dict(case["circuit"])
        assert c.msg_bits == 5 and case["widest_lookup_bits"] <= 5
        assert len(c.nodes) == case["pbs"] and len(c.levels()) == case["depth"]
        n, ln, ints = case["n"], case["len"], case["ints"]
        ours = trace_inverse(n, ln, ints, 2, False, False)
        assert len(ours.levels()) * 4 < case["depth"]
        for v in case["vectors"]:
            assert c.simulate(v["inputs"]) == v["expected"]
            assert ours.simulate(v["inputs"]) == v["expected"]


REF_MODULES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "matrix_inversion")


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF_MODULES, "qfloat_matrix_inversion.pyc")),
                    reason="needs the reference's modules, which build() compiles into oracle/_ref only where a reference checkout is readable")
def test_shim_retraces_the_reference_to_the_committed_fixture():
    """Generator guard, build container only: the Concrete-compatible front end (bmi_amd/compat) run again on the reference's
    unmodified `base_p_subtraction` and `QFloat.__mul__` gives circuits that agree with the committed fixture on its
    vectors (the trace is deterministic up to the random inputset, so outputs are compared, not node lists); the whole
    inverse in the reference's other modes (tensorize=True: its multi_* functions; true_division=True), with and without
    the shim's lazy fusion, reproduces the reference's plaintext results."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import json, os, random, sys
repo = sys.argv[1]
sys.path[:0] = [os.path.join(repo, "bounty-matrix-inversion_amd", "bmi_amd", "compat"), sys.argv[2], os.path.join(repo, "bounty-matrix-inversion_amd")]
import numpy as np
from concrete import fhe
import base_p_arrays as ref
import qfloat as rq
data = {c["name"]: c for c in json.load(open(os.path.join(repo, "tests", "golden", "ref_traced.json")))["cases"]}
rng = random.Random(5)
bits = lambda k: [rng.randint(0, 1) for _ in range(k)]
sub = lambda a, b: ref.base_p_subtraction(a, b, 2, True)
inputset = [(bits(10), bits(10)) for _ in range(400)] + [([0] * 10, [1] * 10), ([1] * 10, [0] * 10)]
c, _ = fhe.trace(sub, [[(0, 1)] * 10] * 2, inputset, msg_bits=4)
for v in data["base_p_subtraction_overflow"]["vectors"]:
    assert c.simulate(v["inputs"]) == v["expected"]
def mul(a, sa, b, sb):
    r = rq.QFloat(a, 4, 2, True, sa[0]) * rq.QFloat(b, 4, 2, True, sb[0])
    return (r._array, r._sign)
inputset = [(bits(8), [rng.choice((-1, 1))], bits(8), [rng.choice((-1, 1))]) for _ in range(1500)]
inputset += [([1] * 8, [s], [1] * 8, [t]) for s in (-1, 1) for t in (-1, 1)] + [([0] * 8, [1], bits(8), [-1])]
c, _ = fhe.trace(mul, [[(0, 1)] * 8, [(-1, 1)], [(0, 1)] * 8, [(-1, 1)]], inputset, msg_bits=4)
ok = 0
from bmi_amd.circuit import RangeError
for v in data["QFloat.__mul__"]["vectors"]:
    try:
        assert c.simulate(v["inputs"]) == v["expected"]
        ok += 1
    except RangeError:
        pass
assert ok >= 12, ok
# the reference's other modes (its multi_* "tensorized" functions, true divisions) and the shim's lazy fusion, against
# the reference's own plaintext results on fresh matrices
import qfloat_matrix_inversion as rmi
def whole(n, L, I, td, tz, fuse):
    nr = np.random.RandomState(11)
    def sample():
        a, sg = rmi.float_matrix_to_qfloat_arrays(nr.randn(n, n) * 100, L, I, 2)
        return ([int(v) for v in np.asarray(a).reshape(-1)], [int(v) for v in np.asarray(sg).reshape(-1)])
    fn = lambda a, sg: rmi.qfloat_matrix_inverse(a.reshape(n * n, L), sg, n, L, I, 2, td, tz)
    c, _ = fhe.trace(fn, [[(0, 1)] * (n * n * L), [(-1, 1)] * (n * n)], [sample() for _ in range(800)], msg_bits=6, fuse=fuse)
    good = 0
    for _ in range(5):
        a, sg = sample()
        want = [int(v) for v in np.asarray(fn(np.array(a), np.array(sg))).reshape(-1)]
        try:
            assert c.simulate(a + sg) == want
            good += 1
        except RangeError:
            pass
    assert good >= 2, (n, td, tz, fuse, good)   # the rest left the ranges measured on the inputset: undefined, never wrong
whole(2, 20, 8, False, True, False)
whole(3, 16, 8, True, True, True)
print("ok")
'''
    out = subprocess.run([sys.executable, "-c", code, repo, REF_MODULES], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_reference_own_fhe_tests_replayed_in_simulation():
    """tests/golden/ref_own_fhe_tests.json.gz (tools/gen_ref_fhe_tests.py): the reference's own FHE test file
    (tests/test_qfloat_fhe.py, unmodified, 7 tests: add/sub, mul, mul by SignedBinary, from_mul, neg, div, multi) was run
    against the Compiler-compatible shim and passed its own assertions; the circuits it compiled and the inputs it ran are
    kept as data.  Every kept circuit reproduces the recorded outputs, and its look-ups fit the parameter set it names."""
    data = load_gz("ref_own_fhe_tests.json.gz")
    assert data["unittest_summary"].startswith("Ran 7 tests") and data["unittest_summary"].endswith("OK")
    names = {c["function"] for c in data["cases"]}
    assert {"add_qfloats", "mul_qfloats", "mul_sb_qfloat", "from_mul_qfloats", "neg_qfloats", "div_qfloats", "multi_qfloats"} <= names
    for case in data["cases"]:
        c = Circuit.from_dict(case["circuit"])
        assert c.msg_bits == case["msg_bits"] <= 5 and len(c.nodes) == case["pbs"]
        assert all(p <= c.msg_bits + 1 for p, _ in c.luts)
        for r in case["runs"]:
            assert c.simulate(r["inputs"]) == r["outputs"], case["function"]


# ----------------------------------------------------------------------------------------------------------------
# program.Program: the frozen array form of a traced circuit (pruned, scheduled, cached on disk) and its vectorised
# plaintext evaluator; executor.assign_rows: store rows recycled after a leaf's last consumer.
def _small_program_and_circuit():
    from bmi_amd.program import Program
    circ = trace_inverse(2, 10, 5, 2, False, False, 2)
    return Program.from_circuit(circ), circ


def test_program_matches_circuit_simulation_and_prunes_dead_lookups():
    prog, circ = _small_program_and_circuit()
    assert prog.n_nodes + prog.meta["pruned_pbs"] == len(circ.nodes) and prog.depth == len(circ.levels())
    rng = np.random.default_rng(3)
    for _ in range(20):
        x = [int(rng.integers(lo, hi + 1)) for lo, hi in zip(circ.leaf_lo[:circ.n_inputs], circ.leaf_hi[:circ.n_inputs])]
        try:
            want = circ.simulate(x)
        except RangeError:          # e.g. a determinant whose reciprocal overflows the claimed range: both must refuse
            with pytest.raises(RangeError):
                prog.simulate(x)
            continue
        assert prog.simulate(x) == want
    with pytest.raises(RangeError):
        prog.simulate([99] + [0] * (prog.n_inputs - 1))
    with pytest.raises(ValueError):
        prog.simulate([0])
    # schedule: every look-up after its producers, level widths sum to the node count
    lvl = prog.node_level
    for i in range(prog.n_nodes):
        for t in prog.term_leaf[prog.node_ptr[i]: prog.node_ptr[i + 1]]:
            if t >= prog.n_inputs:
                assert lvl[t - prog.n_inputs] < lvl[i]
    assert int(prog.level_widths().sum()) == prog.n_nodes


def test_program_cache_round_trip(tmp_path, monkeypatch):
    from bmi_amd.main import compile_inverse
    from bmi_amd.program import Program
    monkeypatch.setenv("BMI_CACHE_DIR", str(tmp_path))
    p1, i1 = compile_inverse(2, 10, 5, division_bits=2)
    p2, i2 = compile_inverse(2, 10, 5, division_bits=2)
    assert not i1["cached"] and i2["cached"] and os.path.dirname(i2["path"]) == str(tmp_path)
    assert all(np.array_equal(getattr(p1, k), getattr(p2, k)) for k in Program.ARRAYS) and p1.meta == p2.meta
    p3, i3 = compile_inverse(2, 10, 5, division_bits=2, cache=False)
    assert not i3["cached"] and i3["path"] is None and np.array_equal(p3.node_level, p1.node_level)
    open(i2["path"], "wb").write(b"not an npz")          # a damaged cache file is rebuilt, not trusted
    p4, i4 = compile_inverse(2, 10, 5, division_bits=2)
    assert not i4["cached"] and np.array_equal(p4.term_leaf, p1.term_leaf)


def test_shipped_programs_are_current_and_round_trip(tmp_path, monkeypatch):
    """bmi_amd/programs/ carries the compiled programs of the configurations whose trace takes minutes (8 x 8, 10 x 10) in the
    compact form (index arrays as differences + LZMA).  Their file names carry the tracer fingerprint: a change to the tracer's
    sources makes them stale, and this test says so (regenerate with tools/ship_programs.py).  The compact form is lossless."""
    import hashlib
    from bmi_amd import program as pg
    from bmi_amd.main import message_bits_for
    for n, ln, ints in ((8, 48, 16), (10, 23, 9)):
        key = dict(kind="inverse", n=n, len=ln, ints=ints, base=2, truediv=False, tensorize=False, divbits=0, msg=message_bits_for(2))
        h = hashlib.sha256(repr((pg.FORMAT, pg._tracer_fingerprint(), sorted(key.items()))).encode()).hexdigest()[:24]
        name = "_".join(f"{k}{v}" for k, v in sorted(key.items()) if not isinstance(v, bool) or v)
        path = os.path.join(pg.shipped_dir(), f"{name}_{h}.prog.xz")
        assert os.path.exists(path), f"shipped program for {n}x{n} is stale or missing: run tools/ship_programs.py ({os.path.basename(path)})"
    # an empty cache directory: the configuration is served from the shipped file, not traced
    monkeypatch.setenv("BMI_CACHE_DIR", str(tmp_path))
    from bmi_amd.main import compile_inverse
    prog, info = compile_inverse(10, 23, 9)
    assert info["cached"] and info.get("shipped") and prog.n_nodes > 1_000_000
    c = next(x for x in load("inverse.json") if x["tag"] == "main_n10_len23_ints9")
    q, sg = qmi.float_matrix_to_qfloat_arrays(np.array(c["M"]).reshape(10, 10), 23, 9, 2)
    out = np.array(prog.simulate(np.concatenate([np.asarray(q).reshape(-1), np.asarray(sg)]))).reshape(100, 24)
    assert out.tolist() == c["out"]
    # round trip of the compact form on a small program
    small, _ = _small_program_and_circuit()
    small.save_compact(str(tmp_path / "s.prog.xz"))
    back = pg.Program.load_compact(str(tmp_path / "s.prog.xz"))
    assert all(np.array_equal(getattr(back, k), getattr(small, k)) for k in pg.Program.ARRAYS) and back.meta == small.meta


def test_store_rows_are_recycled_only_after_the_last_consumer():
    from bmi_amd.executor import assign_rows
    prog, _ = _small_program_and_circuit()
    row, n_rows = assign_rows(prog)
    flat, n_all = assign_rows(prog, recycle=False)
    assert n_all == prog.n_inputs + prog.n_nodes and len(set(flat.tolist())) == n_all
    assert n_rows < n_all // 4
    # replay the level walk: a row may be overwritten only when no later level (nor an output) reads its old leaf
    order, counts = prog.level_order()
    n_in = prog.n_inputs
    owner = {int(row[i]): i for i in range(n_in)}
    readers = {}
    for i in range(prog.n_nodes):
        for t in prog.term_leaf[prog.node_ptr[i]: prog.node_ptr[i + 1]]:
            readers.setdefault(int(t), []).append(int(prog.node_level[i]))
    outs = set(prog.out_leaf.tolist())
    pos = 0
    for t, w in enumerate(counts.tolist(), start=1):
        for i in order[pos: pos + w]:
            r = int(row[n_in + i])
            old = owner.get(r)
            if old is not None:
                assert old not in outs and max(readers.get(old, [0])) <= t, (old, t)
            owner[r] = n_in + int(i)
        pos += w
    assert len({int(row[o]) for o in outs}) == len(outs)


def test_imul_by_an_integer_plain_and_encrypted_matches_reference_golden():
    """QFloat *= k (reference qfloat.py:858-865): k a plain int, and k an ENCRYPTED integer in [-7, 7] (a Tracer there);
    digits and sign equal the reference's on every golden case."""
    cases = load("qfloat_ops.json")["imul_int"]
    assert len(cases) == 40
    # one circuit per format: the QFloat and the integer are both encrypted inputs
    circuits = {}
    for g in cases:
        q = QFloat.from_float(g["f"], g["len"], g["ints"], 2)
        assert [int(x) for x in q.array] == g["q"]["array"]
        q *= g["k"]
        assert [int(x) for x in q.array] == g["out"]["array"] and int(q.sign) == g["out"]["sign"], g
        key = (g["len"], g["ints"])
        if key not in circuits:
            c = Circuit()
            eq, _ = enc_q(c, g["q"], top=1)
            k = c.input(-7, 7)
            eq *= k
            c.set_outputs(list(eq.array) + [eq.sign])
            circuits[key] = c
        c = circuits[key]
        out = c.simulate(g["q"]["array"] + [g["q"]["sign"], g["k"]])
        assert out[:-1] == g["out"]["array"], g
        if any(g["out"]["array"]):                     # the reference leaves the sign of a zero product as it falls
            assert out[-1] == g["out"]["sign"], g
    assert all(c.stats["pbs"] > 0 for c in circuits.values())


def test_digit_array_primitives_take_the_reference_signatures():
    """base_p_arrays called exactly like the reference's (operands first, no circuit argument), plain and encrypted, and
    the tensorised twins multi_* / insert_array_at_index (reference base_p_arrays.py:108-280, 326-354) on the goldens."""
    from bmi_amd import base_p_arrays as bpa
    g = load("base_p_arrays.json")
    subs = [c for c in g if c["op"] == "sub" and c["p"] == 2]
    assert subs
    for c in subs:
        a, b = np.array(c["a"]), np.array(c["b"])
        d, lt = bpa.base_p_subtraction(a, b, 2, True)                       # reference call form, numpy operands
        assert [int(x) for x in d] == c["diff"] and int(lt) == c["lt"]
        assert [int(x) for x in bpa.base_p_subtraction(None, list(a), list(b), 2)] == c["diff_noov"]
    same = [c for c in subs if len(c["a"]) == len(c["b"])]
    same = [c for c in same if len(c["a"]) == len(same[0]["a"])]
    assert same
    D, LT = bpa.multi_base_p_subtraction(np.array([c["a"] for c in same]), np.array([c["b"] for c in same]), 2, True)
    assert [[int(x) for x in r] for r in D] == [c["diff"] for c in same] and [int(x) for x in LT] == [c["lt"] for c in same]
    assert [int(x) for x in bpa.multi_is_greater_or_equal([c["a"] for c in same], [c["b"] for c in same])] == [1 - c["lt"] for c in same]
    # encrypted operands, reference call form: the circuit is found from the operands
    c0 = same[0]
    circ = Circuit()
    ea = [circ.input(0, 1) for _ in c0["a"]]
    eb = [circ.input(0, 1) for _ in c0["b"]]
    d, lt = bpa.base_p_subtraction(ea, eb, 2, True)
    ge = bpa.is_greater_or_equal(ea, eb)
    circ.set_outputs(list(d) + [lt, ge])
    out = circ.simulate(c0["a"] + c0["b"])
    assert out[:-2] == c0["diff"] and out[-2] == c0["lt"]
    # division twin
    divs = [c for c in g if c["op"] == "div" and c["p"] == 2][:3]
    for c in divs:
        assert [int(x) for x in bpa.base_p_division(np.array(c["a"]), np.array(c["b"]), 2)] == c["q"]
    if divs:
        same_d = [c for c in divs if len(c["a"]) == len(divs[0]["a"]) and len(c["b"]) == len(divs[0]["b"])]
        Q = bpa.multi_base_p_division([c["a"] for c in same_d], [c["b"] for c in same_d], 2)
        assert [[int(x) for x in r] for r in Q] == [c["q"] for c in same_d]
    # insertion helpers: clipping on both sides
    B = [[0] * 5 for _ in range(2)]
    bpa.insert_array_at_index([1, 2, 3], B, 0, 3)
    bpa.insert_array_at_index([1, 2, 3], B, 1, -1)
    assert B == [[0, 0, 0, 1, 2], [2, 3, 0, 0, 0]]
    S = [[[0] * 4 for _ in range(2)] for _ in range(2)]
    bpa.insert_array_at_index_3D([[7, 8], [9, 1]], S, 1, 3)
    assert S[0][1] == [0, 0, 0, 7] and S[1][1] == [0, 0, 0, 9] and S[0][0] == [0] * 4


def test_run_validates_the_plaintext_against_the_traced_ranges_before_encrypting(monkeypatch):
    """EncryptedMatrixInversion.run(validate=True) evaluates the compiled program in plaintext, every interval claim
    checked, BEFORE any encryption: a violated claim or an entry beyond the traced leading-digit range is refused while
    no engine exists yet.  (A singular matrix is not such a case: like the reference it yields the all-ones quotient.)"""
    emi = EncryptedMatrixInversion(2, None, 2, 16, 7)
    with pytest.raises(ValueError):
        emi.run(np.array([[5000.0, 1.0], [2.0, 3.0]]))
    assert emi.engine is None
    calls = []
    real = emi.program.simulate
    monkeypatch.setattr(emi.program, "simulate", lambda flat, check=True: (calls.append(check), real(flat, check))[1])

    def no_gpu(*a, **k):
        raise RuntimeError("encrypt reached")
    monkeypatch.setattr(emi, "encrypt", no_gpu)
    with pytest.raises(RuntimeError, match="encrypt reached"):
        emi.run(np.array([[10.0, -3.5], [4.25, 20.0]]))
    assert calls == [True]                                   # validated with the claim checks on, then went on to encrypt
    singular = emi.run(np.array([[2.0, 4.0], [1.0, 2.0]]), simulate=True)
    assert np.isfinite(singular).all()


def test_program_rescheduled_for_more_round_capacity_keeps_depth_and_dependencies():
    """Program.rescheduled (levels re-packed for G x 256 ciphertexts per round: what the executor does on G ranks): same
    depth, every look-up after its producers, and fewer levels that need more than one round."""
    from bmi_amd.main import compile_inverse
    from bmi_amd.program import ROUND, WIDE_ROUND, estimated_evaluate_ms
    prog, _ = compile_inverse(3, 18, 8)
    p4 = prog.rescheduled(4 * ROUND, 4 * WIDE_ROUND)
    assert p4.depth == prog.depth and p4.n_nodes == prog.n_nodes
    lvl = p4.node_level
    prod = np.repeat(np.arange(p4.n_nodes), np.diff(p4.node_ptr))
    inner = p4.term_leaf >= p4.n_inputs
    assert (lvl[p4.term_leaf[inner] - p4.n_inputs] < lvl[prod[inner]]).all()
    flat = [int(v) for v in np.concatenate([np.array(c) for c in ([],)])] if False else None
    g = next(x for x in load("inverse.json") if x["tag"] == "uniform_3x3_small")
    vals = np.concatenate([np.array(g["in_arrays"]).reshape(-1), np.array(g["in_signs"])])
    assert p4.simulate(vals) == prog.simulate(vals)
    assert estimated_evaluate_ms(p4.level_widths(), 4) <= estimated_evaluate_ms(prog.level_widths(), 1)
