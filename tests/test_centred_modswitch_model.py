"""The centred modulus switch (bmi_set_modswitch(ctx, 1); csrc/modswitch_centre.hip) on the CPU: the two definitions of
include/bmi_tfhe.h restated in exact integer arithmetic (tests/test_gpu_centred_modswitch.py holds the kernel to these functions
bit for bit), the identity and the variances they are built on, and the error budget's pricing of the mode.

The restatements use numpy's 64-bit integers where no step can overflow (the bounds are in the comments) and are held to plain
Python integers below."""
import numpy as np
import pytest

Q49 = (1 << 49) - 720895


def switch_torus(words, log_N):
    """t64::modswitch<L> before its mask with 2N - 1: round(a 2N / 2^64), ties up (0 .. 2N)"""
    L = log_N + 1
    return ((np.asarray(words, np.uint64) >> np.uint64(63 - L)) + np.uint64(1)) >> np.uint64(1)


def errors_torus(words, log_N):
    """e = ((a + 2^(S-1)) mod 2^S) - 2^(S-1) in [-2^(S-1), 2^(S-1)), S = 64 - log2(2N): a = switch(a) 2^S + e"""
    S = 64 - (log_N + 1)
    half, mask = np.uint64(1 << (S - 1)), np.uint64((1 << S) - 1)
    return ((np.asarray(words, np.uint64) + half) & mask).astype(np.int64) - np.int64(1 << (S - 1))   # the sum wraps mod 2^64, a multiple of 2^S


def centre_torus(small, log_N):
    """[count][n + 1] words on the 2^64 torus -> the same with b' = b - (T >> 1) mod 2^64, T = sum_{i<n} e_i as int64
    (|T| <= n 2^(S-1) <= 2^62 for n <= 1024, N >= 1024), arithmetic shift"""
    small = np.ascontiguousarray(small, np.uint64)
    out = small.copy()
    T = errors_torus(small[:, :-1], log_N).sum(axis=1, dtype=np.int64)
    out[:, -1] = small[:, -1] - (T >> np.int64(1)).astype(np.uint64)          # uint64 arithmetic wraps mod 2^64
    return out


def switch_f49(words, log_N):
    """f49::modswitch before its mask with 2N - 1: floor((a 2N + (q >> 1)) / q) (a < q < 2^49, 2N <= 2^13: below 2^62)"""
    return ((np.asarray(words, np.uint64) << np.uint64(log_N + 1)) + np.uint64(Q49 >> 1)) // np.uint64(Q49)


def errors_f49(words, log_N):
    """E = a 2N - switch(a) q in [-q/2, q/2]"""
    w = np.asarray(words, np.uint64)
    return (w << np.uint64(log_N + 1)).astype(np.int64) - (switch_f49(w, log_N) * np.uint64(Q49)).astype(np.int64)


def centre_f49(small, log_N):
    """[count][n + 1] canonical words mod q = 2^49 - 720895 -> the same with b' = (b - floor(T / 4N)) mod q, T = sum E_i (|T| < 2^59)"""
    small = np.ascontiguousarray(small, np.uint64)
    out = small.copy()
    T = errors_f49(small[:, :-1], log_N).sum(axis=1, dtype=np.int64)
    d = T >> np.int64(log_N + 2)                                              # floor division by 4N
    out[:, -1] = ((small[:, -1].astype(np.int64) - d) % np.int64(Q49)).astype(np.uint64)
    return out


def centre(small, q_bits, log_N):
    return centre_f49(small, log_N) if q_bits == 49 else centre_torus(small, log_N)


# ---- the same two definitions in Python integers, word by word as the header states them
def centre_row_by_integers(row, q_bits, log_N):
    row = [int(w) for w in row]
    two_N = 2 << log_N
    if q_bits == 49:
        T = 0
        for a in row[:-1]:
            T += a * two_N - ((a * two_N + (Q49 >> 1)) // Q49) * Q49
        return row[:-1] + [(row[-1] - T // (2 * two_N)) % Q49]
    S = 64 - (log_N + 1)
    T = sum(((a + (1 << (S - 1))) % (1 << S)) - (1 << (S - 1)) for a in row[:-1])
    return row[:-1] + [(row[-1] - (T >> 1)) % (1 << 64)]


def edge_rows(n, q_bits, log_N, rng):
    """zeros; the largest word; every mask word at the tie (the most negative sum: -n 2^(S-1) on the torus; on the field the
    smallest word that switches to 1); one below it (the most positive sum); a row that starts with q - 1 (on the field its
    unmasked switch is 2N); random words"""
    Q = Q49 if q_bits == 49 else 1 << 64
    if q_bits == 49:
        two_N = 2 << log_N
        tie = -(-(Q49 - (Q49 >> 1)) // two_N)
        draw = lambda size: rng.integers(0, Q49, size, dtype=np.uint64)
    else:
        tie = 1 << (64 - (log_N + 1) - 1)
        draw = lambda size: rng.integers(0, 1 << 63, size, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size, dtype=np.uint64)
    rows = np.zeros((6, n + 1), np.uint64)
    rows[1] = np.uint64(Q - 1)
    rows[2, :-1], rows[2, -1] = np.uint64(tie), np.uint64(5)
    rows[3, :-1], rows[3, -1] = np.uint64(tie - 1), np.uint64(Q - 3)
    rows[4] = draw(n + 1)
    rows[4, 0] = np.uint64(Q - 1)
    rows[5] = draw(n + 1)
    return rows


@pytest.mark.parametrize("q_bits,log_N,n", [(65, 10, 1024), (65, 10, 17), (65, 11, 742), (65, 12, 16), (49, 10, 630), (49, 10, 17)])
def test_numpy_restatement_equals_python_integers(q_bits, log_N, n):
    rng = np.random.default_rng(n)
    rows = edge_rows(n, q_bits, log_N, rng)
    got = centre(rows, q_bits, log_N)
    assert np.array_equal(got[:, :-1], rows[:, :-1])
    for r, g in zip(rows, got):
        assert [int(w) for w in g] == centre_row_by_integers(r, q_bits, log_N)
    if q_bits == 65:
        S = 64 - (log_N + 1)
        assert int(errors_torus(rows[2, :-1], log_N).sum()) == -n << (S - 1)        # -2^62 at n = 1024, N = 1024
        assert int(errors_torus(rows[3, :-1], log_N).sum()) == n * ((1 << (S - 1)) - 1)
        assert int(got[2, -1]) == (5 + (n << (S - 2))) % (1 << 64)
    else:
        assert int(switch_f49(rows[4, :1], log_N)[0]) == 2 << log_N and int(errors_f49(rows[4, :1], log_N)[0]) == -(2 << log_N)
        assert int(switch_f49(rows[2, :1], log_N)[0]) == 1 and int(switch_f49(rows[3, :1], log_N)[0]) == 0
        assert int(errors_f49(rows[2, :1], log_N)[0]) < -(Q49 // 2) + (2 << log_N) and int(errors_f49(rows[3, :1], log_N)[0]) > Q49 // 2 - (2 << log_N)


# ---- the identity and the variances
def switched_phase_errors(q_bits, log_N, n, count, seed):
    """`count` small ciphertexts of known phase under a random binary key -> (2 x the switched-phase error of the standard switch,
    2 x that of the centred switch, 2 x what the identity says the latter is, without its floor term; floor term), in units of
    1 / 2^S positions (torus) resp. 1 / q positions (field), as Python integers; and the key"""
    rng = np.random.default_rng(seed)
    Q = Q49 if q_bits == 49 else 1 << 64
    two_N = 2 << log_N
    unit = Q49 if q_bits == 49 else 1 << (64 - (log_N + 1))        # one position in these units; the circle is 2N * unit = Q * (2N or 1)
    circle = two_N * unit
    scale = two_N if q_bits == 49 else 1                           # phase in words -> these units
    s = rng.integers(0, 2, n).astype(np.int64)
    draw = (lambda shape: rng.integers(0, Q49, shape, dtype=np.uint64)) if q_bits == 49 else \
        (lambda shape: rng.integers(0, 1 << 63, shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, shape, dtype=np.uint64))
    a = draw((count, n))
    phase = draw(count)
    small = np.empty((count, n + 1), np.uint64)
    small[:, :-1] = a
    masked_sum = a @ s.astype(np.uint64)                            # wraps mod 2^64 on the torus; below 2^59 on the field
    small[:, -1] = phase + masked_sum if q_bits != 49 else (phase + masked_sum) % np.uint64(Q49)
    switch, errors = (switch_f49, errors_f49) if q_bits == 49 else (switch_torus, errors_torus)
    e = errors(a, log_N)
    a_hat = switch(a, log_N).astype(np.int64)
    masked = (a_hat @ s)                                            # sum s_i a^_i (below 2^23)
    signed = e @ (2 * s - 1)                                        # sum (2 s_i - 1) e_i (|.| < 2^59 + ...: int64)
    T = e.sum(axis=1)

    def centred_lift(x):
        x %= circle
        return x - circle if x >= circle // 2 else x

    out = []
    for ct, with_T in ((small, False), (centre(small, q_bits, log_N), True)):
        b_hat = switch(ct[:, -1], log_N).astype(np.int64)
        e_b = errors(ct[:, -1], log_N)
        got = [2 * centred_lift((int(bh) - int(m)) * unit - int(p) * scale) for bh, m, p in zip(b_hat, masked, phase)]
        out.append((got, e_b))
    floor_term = [int(t) % (2 * scale) for t in T]                 # T & 1 on the torus, T mod 4N on the field
    want_centred = [int(sg) - 2 * int(eb) for sg, eb in zip(signed, out[1][1])]
    want_standard = [2 * (int(x) - int(eb)) for x, eb in zip(e @ s, out[0][1])]
    return out[0][0], want_standard, out[1][0], want_centred, floor_term, s, unit


@pytest.mark.parametrize("n", [16, 630])
@pytest.mark.parametrize("q_bits", [65, 49])
def test_identity_and_variances(q_bits, n):
    """N = 1024, 4,096 ciphertexts.  Exactly: the standard switch is off by sum s_i e_i - e_b, the centred one by
    sum (s_i - 1/2) e_i - e_b' plus the floor's remainder (T mod 2) / 2 resp. (T mod 4N) / 2 - less than one unit of the body.
    Sample variances within 10 % of (1 + hw(s)) / 12 and (1 + n / 4) / 12 positions^2: 4.5 standard errors of a variance estimated
    from 4,096 samples, sqrt(2 / 4096) = 2.2 %."""
    count = 4096
    std, want_std, cen, want_cen, floor_term, s, unit = switched_phase_errors(q_bits, 10, n, count, seed=100 * q_bits + n)
    assert std == want_std
    assert cen == [w + f for w, f in zip(want_cen, floor_term)]
    assert max(floor_term) < (2 * 2048 if q_bits == 49 else 2)
    hw = int(s.sum())
    var_std = np.var(np.array(std, np.float64) / (2.0 * unit))
    var_cen = np.var(np.array(cen, np.float64) / (2.0 * unit))
    print(f"\nq_bits {q_bits}, n {n}, hw(s) {hw}: standard {var_std:.3f} positions^2 (model {(1 + hw) / 12:.3f}), "
          f"centred {var_cen:.3f} (model {(1 + n / 4) / 12:.3f})")
    assert abs(var_std / ((1 + hw) / 12.0) - 1) < 0.10
    assert abs(var_cen / ((1 + n / 4.0) / 12.0) - 1) < 0.10


# ---- the error budget
def chain(bits, n):
    from bmi_amd.circuit import Circuit
    from bmi_amd.program import Program
    c = Circuit(msg_bits=bits)
    h = 1 << (bits - 1)
    xs = [c.input(-h, h - 1) for _ in range(n)]
    c.set_outputs([c.lut(x, lambda v: -v - 1) for x in xs])
    return Program.from_circuit(c)


def test_the_keyword_changes_the_rounding_term_alone():
    from bmi_amd import error_budget as eb, tfhe
    P = tfhe.preset_params("north_star_torus64")
    v_ks = eb.keyswitch_variance(P)
    v_in = eb.pbs_output_variance(P)
    for hs in (1.0, 315.0, 630.0):
        s0, m0 = eb._lookup_margin(P, 4, v_in, v_ks, hs)
        s1, m1 = eb._lookup_margin(P, 4, v_in, v_ks, hs, centred_modswitch=True)
        assert s0 ** 2 - s1 ** 2 == pytest.approx((1 + hs) / 12.0 - (1 + 630 / 4.0) / 12.0, abs=1e-9)
        assert m1 == pytest.approx(32.0 / np.sqrt((1 + 630 / 4.0) / 12.0 + (v_in + v_ks) * 2048.0 ** 2), rel=1e-12)
        assert m1 == pytest.approx(8.8, abs=0.05) and m1 * s1 == pytest.approx(32.0)
    assert m0 != m1
    p = [eb.lookup_failure_probability(P, 4, v_in, hw_small=h, centred_modswitch=True) for h in (1, 315, 630)]
    assert p[0] == p[1] == p[2] and 1e-19 < p[0] < 1e-17
    assert eb.lookup_failure_probability(P, 4, v_in, hw_small=1) < eb.lookup_failure_probability(P, 4, v_in, hw_small=630)
    assert 3e-10 < eb.lookup_failure_probability(P, 4, v_in) < 6e-10                              # 6.24 sigma: the standard switch
    # a whole program: everything but the margins and what follows from them is the same report
    prog = chain(4, 5)
    off, on = eb.failure_probability(prog, P), eb.failure_probability(prog, P, centred_modswitch=True)
    assert off == eb.failure_probability(prog, P, centred_modswitch=False)
    for k in ("lookups", "params", "log2_std_pbs_output", "log2_std_keyswitch", "widest_amplification", "output_margin_sigma"):
        assert off[k] == on[k]
    assert off["worst_margin_sigma"] == pytest.approx(6.24, abs=0.05) and on["worst_margin_sigma"] == pytest.approx(8.8, abs=0.05)


def test_the_shipped_8x8_meets_concretes_default_on_the_default_set_when_centred():
    from bmi_amd import error_budget as eb, tfhe
    from bmi_amd.main import compile_inverse
    prog, _ = compile_inverse(8, 48, 16)
    P = tfhe.preset_params("north_star_torus64")
    off, on = eb.failure_probability(prog, P), eb.failure_probability(prog, P, centred_modswitch=True)
    print(f"\n8x8 inverse, {off['lookups']} look-ups, default set: p_fail {off['p_fail']:.2e} -> centred {on['p_fail']:.2e}")
    assert off["p_fail"] > 1e-5 and on["p_fail"] <= 1e-5
    chosen, rep = eb.choose_params(prog, 1e-5, centred_modswitch=True)
    assert (chosen.N, chosen.n, chosen.q_bits) == (1024, 630, tfhe.TORUS64) and rep["p_fail"] == on["p_fail"] and len(rep["tried"]) == 1
    chosen, rep = eb.choose_params(prog, 1e-5)
    assert (chosen.N, chosen.n) == (2048, 630) and rep["tried"][0][1] == off["p_fail"]


def test_five_bit_look_ups_on_the_wide_secure_set():
    """secure128_torus_wide: 141.1 -> 125.6 positions^2 (the keyswitch term does not move), so the margin grows by their root"""
    from bmi_amd import error_budget as eb, tfhe
    P = tfhe.preset_params("secure128_torus_wide")
    prog = chain(5, 60)
    off, on = eb.failure_probability(prog, P), eb.failure_probability(prog, P, centred_modswitch=True)
    assert on["worst_margin_sigma"] / off["worst_margin_sigma"] == pytest.approx(np.sqrt(141.1 / 125.6), rel=0.01)
    assert 5.2 < off["worst_margin_sigma"] < 5.5 < on["worst_margin_sigma"] < 5.9


def test_engines_and_wrappers_carry_the_mode():
    """error_budget.engine_failure_probability reads engine.modswitch; EncryptedMatrixInversion and the compat Configuration forward
    the flag (no GPU here: a stand-in with the engine's fields, as in tests/test_error_budget.py)"""
    from bmi_amd import error_budget as eb, tfhe
    from bmi_amd.compat.concrete import fhe
    from bmi_amd.main import EncryptedMatrixInversion

    class FakeEngine:
        def __init__(self, P, mode=0):
            self.P, self.q_bits, self.bsk_precision, self.unroll, self.device, self.modswitch = P, P.q_bits, 48, 1, 0, mode

        def set_modswitch(self, mode):
            self.modswitch = mode

    P = tfhe.default_params(q_bits=tfhe.TORUS64)
    prog = chain(4, 5)
    assert eb.engine_failure_probability(prog, FakeEngine(P, 1)) == eb.failure_probability(prog, P, 48, centred_modswitch=True)
    assert eb.engine_failure_probability(prog, FakeEngine(P, 0)) == eb.failure_probability(prog, P, 48) == prog.failure_probability(FakeEngine(P, 0))
    eng = FakeEngine(P)
    emi = EncryptedMatrixInversion(2, None, 2, 20, 8, engine=eng, centred_modswitch=True)
    emi._engine()
    assert eng.modswitch == 1 and emi.error_budget["worst_margin_sigma"] > 8.5
    eng = FakeEngine(P)
    emi = EncryptedMatrixInversion(2, None, 2, 20, 8, engine=eng)
    emi._engine()
    assert eng.modswitch == 0 and emi.error_budget["worst_margin_sigma"] == pytest.approx(6.236, abs=0.01)
    assert fhe.Configuration().centred_modswitch is False and fhe.Configuration(centred_modswitch=True).centred_modswitch is True
