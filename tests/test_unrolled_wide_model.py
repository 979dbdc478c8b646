"""The unrolled bootstrap key on the 2^64 torus at N = 2048 (secure128_torus; k_blind_rotate_wu_t64f), on the CPU: the a-priori
bound that certifies the rounding of its limb sums at 40 bits of key precision (tools/fft_bound.py), and what the error budget
prices for it (error_budget.choose_params keeps `unroll` for torus sets with log_N == 11, at 40 bits; N = 1024 unchanged)."""
import math
import os
import sys

import pytest

from bmi_amd import error_budget, tfhe
from bmi_amd.main import compile_inverse

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import fft_bound  # noqa: E402


def test_the_bound_certifies_20_bit_limbs_and_not_21():
    """six times the plain limb sum (three keys, each scaled by |X^c - 1| <= 2), the scaling counted as a multiplication stage
    of its own and its factor's error (a table entry minus one) in beta: below 1/2 with 20-bit limbs, not with 21"""
    b20 = fft_bound.unrolled_limb_sum_bound(11, 3, 10, 20)
    b21 = fft_bound.unrolled_limb_sum_bound(11, 3, 10, 21)
    # never below six times the plain bound the quarter transform is certified with (0.052 x 6 = 0.31)
    plain20 = 6 * fft_bound.limb_sum_bound(11, 3, 10, 20)[0]
    assert plain20 == pytest.approx(0.312, abs=0.001) and plain20 < b20 < 0.5 <= b21
    assert 6 * fft_bound.limb_sum_bound(11, 3, 10, 21)[0] >= 0.5          # 21 bits fail before the scaling stage is counted
    assert b20 == pytest.approx(0.38, abs=0.005)                           # the value in the kernel's header and DESIGN section 2
    assert fft_bound.unrolled_limb_sum_bound(11, 2, 10, 20) < b20          # l = 2, the other instantiation
    # the limb sums stay below 2^45, the size the bound is stated for
    assert 6 * 2 * 3 * 2048 * 2.0 ** 9 * 2.0 ** 19 < 2.0 ** 45


def test_choose_params_prices_the_unrolled_key_at_40_bits_on_secure128_torus():
    prog, _ = compile_inverse(2, 20, 8)
    P, plain = error_budget.choose_params(prog, 1e-5, secure=True)
    Pu, unr = error_budget.choose_params(prog, 1e-5, secure=True, unroll=True)
    assert plain["chosen"] == unr["chosen"] == "secure128_torus" and (Pu.N, Pu.n, Pu.q_bits) == (2048, 742, tfhe.TORUS64)
    want = error_budget.failure_probability(prog, Pu, 40, unroll=True)
    assert unr["p_fail"] == want["p_fail"] and unr["log10_p_fail"] == want["log10_p_fail"]
    assert unr["p_fail"] != plain["p_fail"]                                # (the flag used to be dropped at N = 2048)
    assert unr["p_fail"] > plain["p_fail"]                                 # three products per pair on a coarser key: more noise
    # the bootstrap's output std: 2^-22.2 plain at 46 bits, 2^-16.2 unrolled at 40 bits (3 x 742 x 3 x 2 x 2048 x 2^20 / 12 x
    # (1 + 1024) 4^24 / 12 / 2^128 = 2^-32.5 in variance) - still far below the keyswitch's 2^-9.8
    assert 0.5 * math.log2(error_budget.pbs_output_variance(Pu)) == pytest.approx(-22.2, abs=0.15)
    v40 = error_budget.pbs_output_variance(Pu, 40, unroll=True)
    assert 0.5 * math.log2(v40) == pytest.approx(-16.23, abs=0.1)
    assert v40 < error_budget.keyswitch_variance(Pu) / 1000
    with_shared = error_budget.choose_params(prog, 1e-5, secure=True, unroll=True, share_rotations=True)[1]
    assert with_shared["p_fail"] == error_budget.failure_probability(prog, Pu, 40, unroll=True, share_rotations=True)["p_fail"]


def test_the_3x3_still_lands_on_secure128_torus_with_the_unrolled_key():
    prog, _ = compile_inverse(3, 30, 12)
    P, rep = error_budget.choose_params(prog, p_error=1e-5, secure=True, unroll=True)
    assert rep["chosen"] == "secure128_torus" and len(rep["tried"]) == 1 and rep["p_fail"] <= 1e-5


def test_the_n1024_unrolled_report_is_unchanged():
    prog, _ = compile_inverse(2, 20, 8)
    for qb in (tfhe.TORUS64, 49):
        P, rep = error_budget.choose_params(prog, 1e-3, q_bits=qb, unroll=True)
        assert P.log_N == 10
        want = error_budget.failure_probability(prog, P, unroll=True)
        assert all(rep[k] == want[k] for k in want)
    # the secure N = 4096 set and the 49-bit N = 2048 set have no unrolled price: the flag is dropped there as before
    big, _ = compile_inverse(4, 40, 16)
    P, rep = error_budget.choose_params(big, 1e-5, q_bits=49, unroll=True)
    assert P.log_N == 11 and rep["p_fail"] == error_budget.failure_probability(big, P)["p_fail"]
