"""The error budget of shared rotations on the unrolled bootstrap key (error_budget.pbs_output_variance_parts(unroll=True),
failure_probability(unroll=True, share_rotations=True)): the split of the unrolled key's output variance into the white and the
key-carried part, the plain split unchanged, and the budget of hand-built programs against the formula written out (the manner
of tests/test_shared_rotation_model.py; the GPU holds the model to the measured noise in
tests/test_gpu_shared_rotation_wide_unrolled.py)."""
import math

import numpy as np
import pytest

from bmi_amd import error_budget, tfhe
from bmi_amd.circuit import Circuit
from bmi_amd.program import Program
from bmi_amd.shared_rotation import rotation_groups, sparse_table

PREC = 42       # what the unrolled floating-point-transform engine of the torus stores its key at


def torus():
    return tfhe.default_params(q_bits=tfhe.TORUS64)


@pytest.mark.parametrize("weights", [{}, {"hw_small": 301, "hw_big": 530}, {"hw_small": 301, "hw_big": 530, "live_pairs": 233},
                                     {"live_pairs": 240}])
def test_unrolled_parts_add_up_to_the_unrolled_variance(weights):
    """v_white + hw(S) v_carried == pbs_output_variance(unroll=True) on the north-star torus set at 42 bits: at the average
    weights, at explicit ones, and with the exact count of live pairs (then against the formula written out, the total taking
    no such argument)"""
    P = torus()
    N, n, l, Bg = 1 << P.log_N, P.n, P.bs_levels, 2.0 ** P.bs_base_log
    kw = {k: v for k, v in weights.items() if k != "live_pairs"}
    hb = weights.get("hw_big", P.k * N / 2.0)
    v_white, v_carried = error_budget.pbs_output_variance_parts(P, PREC, unroll=True, **weights)
    assert v_white > v_carried > 0
    if "live_pairs" not in weights:
        assert math.isclose(v_white + hb * v_carried, error_budget.pbs_output_variance(P, PREC, unroll=True, **kw), rel_tol=1e-12)
    pairs = weights.get("live_pairs", (n + 1) // 2 * 0.75 if "hw_small" not in weights else min((n + 1) // 2, weights["hw_small"]))
    rho = 4.0 ** (64 - PREC) / 12.0 / 2.0 ** 128
    K = n * l * (P.k + 1) * N * (Bg * Bg + 2) / 12.0
    rnd = 2 * pairs / (12.0 * Bg ** (2 * l))
    assert math.isclose(v_white, 3 * K * (P.glwe_noise ** 2 + rho) + rnd, rel_tol=1e-12)
    assert math.isclose(v_carried, 3 * K * rho + rnd, rel_tol=1e-12)
    # 3 K sigma_eff^2 + 2 pairs (1 + hw(S)) / (12 Bg^(2l)), sigma_eff^2 = sigma^2 + (1 + hw(S)) rho
    total = 3 * K * (P.glwe_noise ** 2 + (1 + hb) * rho) + rnd * (1 + hb)
    assert math.isclose(v_white + hb * v_carried, total, rel_tol=1e-12)


def test_parts_and_total_price_the_same_precision_when_none_is_given():
    """no bsk_precision: both functions price default_bsk_precision(P) - 48 bits on this set, NOT the 42 the unrolled
    floating-point-transform engine stores, which a budget for a live engine passes (main.py: engine.bsk_precision)"""
    P = torus()
    assert error_budget.default_bsk_precision(P) == 48
    hb = P.k * (1 << P.log_N) / 2.0
    w, c = error_budget.pbs_output_variance_parts(P, unroll=True)
    assert math.isclose(w + hb * c, error_budget.pbs_output_variance(P, unroll=True), rel_tol=1e-12)
    assert (w, c) == error_budget.pbs_output_variance_parts(P, 48, unroll=True)
    assert error_budget.pbs_output_variance(P, PREC, unroll=True) > 10 * error_budget.pbs_output_variance(P, unroll=True)


@pytest.mark.parametrize("params", [None, "secure128_torus", "secure128_torus_wide", 49])
def test_plain_parts_are_what_they_were(params):
    """every existing call shape of the plain function against its formula written out"""
    P = tfhe.default_params(q_bits=49) if params == 49 else tfhe.default_params() if params is None else tfhe.preset_params(params)
    N, n, l, Bg = 1 << P.log_N, P.n, P.bs_levels, 2.0 ** P.bs_base_log
    K = n * l * (P.k + 1) * N * (Bg * Bg + 2) / 12.0
    for args, kw in (((), {}), ((None, 300, 500), {}), ((error_budget.default_bsk_precision(P),), {"hw_small": 17}), ((64,), {}),
                     ((), {"bsk_precision": 64, "hw_big": 99})):
        prec = args[0] if args and args[0] is not None else kw.get("bsk_precision") or error_budget.default_bsk_precision(P)
        hs = args[1] if len(args) > 1 else kw.get("hw_small", n / 2.0)
        rho = 4.0 ** (64 - prec) / 12.0 / 2.0 ** 128 if (P.q_bits == tfhe.TORUS64 and prec < 64) else 0.0
        rnd = hs / (12.0 * Bg ** (2 * l))
        assert error_budget.pbs_output_variance_parts(P, *args, **kw) == (K * (P.glwe_noise ** 2 + rho) + rnd, K * rho + rnd)
        assert error_budget.pbs_output_variance_parts(P, *args, **kw) == error_budget.pbs_output_variance_parts(P, *args, unroll=False, **kw)
        hb = args[2] if len(args) > 2 else kw.get("hw_big", P.k * N / 2.0)
        w, c = error_budget.pbs_output_variance_parts(P, *args, **kw)
        assert math.isclose(w + hb * c, error_budget.pbs_output_variance(P, prec, hw_small=hs, hw_big=hb), rel_tol=1e-12)


def chain_program():
    """no two look-ups read the same ciphertext: every group is of one"""
    c = Circuit()
    x = c.input(-8, 7)
    a = c.lut(x, lambda v: v // 2)
    c.set_outputs([c.lut(a, lambda v: -v)])
    return Program.from_circuit(c, native=False)


def three_node_program():
    c = Circuit()
    x = c.input(-8, 7)
    a = c.lut(x, lambda v: v // 2)            # two tables of the same input: one group
    b = c.lut(x, lambda v: (v * v) % 5 - 2)
    c.set_outputs([c.lut(a + b, lambda v: -v)])
    return Program.from_circuit(c, native=False)


def test_without_a_group_the_shared_unrolled_budget_is_the_unshared_one():
    prog = chain_program()
    assert rotation_groups(prog).sizes.tolist() == [1, 1]
    P = torus()
    plain = error_budget.failure_probability(prog, P, PREC, unroll=True)
    shared = error_budget.failure_probability(prog, P, PREC, unroll=True, share_rotations=True)
    assert shared["shared_lookups"] == 0 and shared["rotations"] == 2
    assert {k: v for k, v in shared.items() if k not in ("shared_lookups", "rotations")} == plain


@pytest.mark.parametrize("weights", [{}, {"hw_small": 301, "hw_big": 530}])
def test_budget_of_a_group_on_the_unrolled_key_is_the_written_out_formula(weights):
    """the members of the one group of two carry norm2 v_white + E |S P_f|^2 v_carried of the UNROLLED parts; the third look-up,
    a group of one, the unrolled variance itself"""
    prog = three_node_program()
    rg = rotation_groups(prog)
    assert rg.sizes.tolist() == [2, 1]
    P = torus()
    N = 1 << P.log_N
    hs = weights.get("hw_small", P.n / 2.0)
    dens = weights.get("hw_big", N / 2.0) / N
    v_pbs = error_budget.pbs_output_variance(P, PREC, True, **weights)
    v_ks = error_budget.keyswitch_variance(P, weights.get("hw_big"))
    v_white, v_carried = error_budget.pbs_output_variance_parts(P, PREC, unroll=True, **weights)
    plain_parts = error_budget.pbs_output_variance_parts(P, PREC, **weights)
    assert v_white > 2.9 * plain_parts[0] and v_carried > 2.9 * plain_parts[1]        # not the plain key's parts
    shared_var = []
    for node in (0, 1):
        j = int(prog.node_lut[node])
        p = int(prog.lut_p[j])
        pos, cf = sparse_table(prog.lut_tab[j, : 1 << p], p, 59, 59, N)
        n2 = float((cf.astype(np.float64) ** 2).sum())
        m = np.array([sum(c if x >= q else -c for q, c in zip(pos.tolist(), cf.tolist())) for x in range(N)], np.float64)
        # E |S P|^2 over keys of density d: N d (1 - d) |P|^2 + d^2 sum_j m_j^2
        shared_var.append(n2 * v_white + (N * dens * (1 - dens) * n2 + dens * dens * float((m ** 2).sum())) * v_carried)

    def tail(v_in, p):
        sigma = math.sqrt((v_in + v_ks) * (2.0 * N) ** 2 + (1 + hs) / 12.0)
        return math.erfc(N / 2.0 ** (p + 1) / sigma / math.sqrt(2.0))

    def total(va, vb, vc):
        c0, c1 = [float(v) for v in prog.term_coef[prog.node_ptr[2]: prog.node_ptr[3]]]
        p_of = lambda i: int(prog.lut_p[prog.node_lut[i]])   # noqa: E731
        x_coef = float(prog.term_coef[0])
        lookups = 2 * tail(x_coef ** 2 * P.glwe_noise ** 2, p_of(0)) + tail(c0 * c0 * va + c1 * c1 * vb, p_of(2))
        return lookups + math.erfc(2.0 ** -(prog.msg_bits + 2) / math.sqrt(vc) / math.sqrt(2.0))

    plain = error_budget.failure_probability(prog, P, PREC, True, **weights)
    shared = error_budget.failure_probability(prog, P, PREC, True, share_rotations=True, **weights)
    assert shared["shared_lookups"] == 2 and shared["rotations"] == 2 and shared["lookups"] == 3
    assert math.isclose(plain["p_fail"], total(v_pbs, v_pbs, v_pbs), rel_tol=1e-9)
    assert math.isclose(shared["p_fail"], total(shared_var[0], shared_var[1], v_pbs), rel_tol=1e-9)
    assert min(shared_var) > v_pbs and shared["p_fail"] >= plain["p_fail"]
