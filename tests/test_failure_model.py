"""error_budget.lookup_failure_probability: the per-look-up term of failure_probability as a function of its own (the quantity
tests/test_gpu_decrypt_device.py holds measured failure counts to).  No GPU."""
import math

import pytest

from bmi_amd import error_budget, failure_rate, tfhe


def one_lookup(bits):
    from bmi_amd.circuit import Circuit
    from bmi_amd.program import Program
    c = Circuit(msg_bits=bits)
    h = 1 << (bits - 1)
    c.set_outputs([c.lut(c.input(-h, h - 1), lambda v: -v - 1)])
    return Program.from_circuit(c)


@pytest.mark.parametrize("preset,bits", [("north_star_torus64", 4), ("north_star_torus64", 5), ("secure128_torus", 5), ("secure128_torus", 6),
                                         ("north_star", 5)])
def test_one_lookup_program_is_the_lookup_term_plus_the_output_term(preset, bits):
    P = tfhe.preset_params(preset)
    prog = one_lookup(bits)
    assert (prog.n_nodes, prog.n_outputs, prog.msg_bits) == (1, 1, bits)
    for kw in ({}, {"hw_small": P.n // 2 - 20, "hw_big": P.N // 2 + 31}):
        rep = error_budget.failure_probability(prog, P, **kw)
        look = error_budget.lookup_failure_probability(P, bits, input_variance=P.glwe_noise ** 2, **kw)
        out_margin = 2.0 ** -(bits + 2) / math.sqrt(error_budget.pbs_output_variance(P, **kw))
        assert rep["output_margin_sigma"] == pytest.approx(out_margin, rel=1e-12)
        assert rep["p_fail"] == pytest.approx(look + math.erfc(out_margin / math.sqrt(2.0)), rel=1e-9)
        assert look > 0 and look == pytest.approx(math.erfc(rep["worst_margin_sigma"] / math.sqrt(2.0)), rel=1e-9)


def test_monotone_in_table_width_and_variance_scale():
    for preset in ("north_star_torus64", "secure128_torus", "north_star"):
        P = tfhe.preset_params(preset)
        v = 2 * P.glwe_noise ** 2
        by_bits = [error_budget.lookup_failure_probability(P, b, v) for b in range(2, 8)]
        assert all(a < b for a, b in zip(by_bits, by_bits[1:])), by_bits
        by_scale = [error_budget.lookup_failure_probability(P, 5, v, variance_scale=s) for s in (0.5, 0.85, 1.0, 1.15, 2.0)]
        assert all(a < b for a, b in zip(by_scale, by_scale[1:])), by_scale
        assert error_budget.lookup_failure_probability(P, 5, v) < error_budget.lookup_failure_probability(P, 5, 1e6 * v + 2.0 ** -24)
    with pytest.raises(ValueError):
        error_budget.lookup_failure_probability(tfhe.preset_params("north_star_torus64"), 10)


def margin_of(p):
    """sigma of margin for a two-sided Gaussian tail p (bisection on erfc)"""
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if math.erfc(mid / math.sqrt(2.0)) > p else (lo, mid)
    return lo


def test_the_three_calibration_figures():
    """the figures quoted for the GPU calibration, at the expected key weights hw(s) = n / 2, hw(S) = k N / 2"""
    ns, sec = tfhe.preset_params("north_star_torus64"), tfhe.preset_params("secure128_torus")
    # 1. 5-bit identity on north_star_torus64: rounding term 26.33 of 26.33 positions^2, 3.12 sigma, p = 1.8e-3, ~480 of 2^18
    assert (1 + ns.n / 2) / 12 == pytest.approx(26.33, abs=0.01)
    pred = failure_rate.prediction(ns, 5, 1 << 18, ns.n / 2, ns.N / 2)
    p = pred["p"]["1.0"]
    assert p == pytest.approx(1.8e-3, rel=0.03) and margin_of(p) == pytest.approx(3.12, abs=0.01)
    assert pred["expected"] == pytest.approx(480, rel=0.02)
    assert pred["band"][0] == pytest.approx(150, abs=5) and pred["band"][1] == pytest.approx(1050, abs=5)
    var = (ns.N / 2 ** 6 / margin_of(p)) ** 2          # half a 5-bit box is N / 2^6 = 16 positions
    assert (1 + ns.n / 2) / 12 / var > 0.9999
    # the exact integer-box reading of the same variance, P(e >= 15.5) + P(e <= -16.5), lies inside the band
    boxed = 0.5 * math.erfc(15.5 / math.sqrt(2 * var)) + 0.5 * math.erfc(16.5 / math.sqrt(2 * var))
    assert boxed == pytest.approx(1.9e-3, rel=0.03) and pred["band"][0] < boxed * (1 << 18) < pred["band"][1]
    # 2. 6-bit identity on secure128_torus: keyswitch noise 20.9 of 51.9 positions^2, 2.22 sigma, p = 2.6e-2, ~1,730 of 2^16
    ks = error_budget.keyswitch_variance(sec) * (2.0 * sec.N) ** 2
    assert ks == pytest.approx(20.9, abs=0.05) and ks + (1 + sec.n / 2) / 12 == pytest.approx(51.9, abs=0.05)
    pred = failure_rate.prediction(sec, 6, 1 << 16, sec.n / 2, sec.N / 2)
    p = pred["p"]["1.0"]
    assert p == pytest.approx(2.6e-2, rel=0.03) and margin_of(p) == pytest.approx(2.22, abs=0.01)
    assert pred["expected"] == pytest.approx(1730, rel=0.01)
    assert pred["band"][0] == pytest.approx(950, abs=10) and pred["band"][1] == pytest.approx(2670, abs=10)
    # 3. control: the 4-bit table of the set's own width, 4e-6 wrong look-ups expected in 8,192
    pred = failure_rate.prediction(ns, 4, 8192, ns.n / 2, ns.N / 2)
    assert pred["expected"] == pytest.approx(4e-6, rel=0.1)
