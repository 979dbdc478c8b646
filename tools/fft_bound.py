#!/usr/bin/env python3
"""A-priori bound on the rounding error of the limb sums the 2^64-torus kernels compute through a floating-point transform
(csrc/fft_wave_f64.hpp / fft_half_f64.hpp at N = 1024, csrc/fft_quarter_f64.hpp at N = 2048), to be compared with 1/2: below
it, rounding the inverse transform to the nearest integer returns the exact integer sum whatever the order of the
floating-point operations.

Percival (2003), error of a weighted (right-angle) FFT product z = x * y of length 2^n computed in floating point:

    |z' - z|_inf  <  ||x|| ||y|| ((1 + e)^(3n) (1 + e sqrt 5)^(3n + 1) (1 + b)^(3n) - 1)

e = 2^-53 (f64 unit round-off), b = largest error of a table entry (tables are rounded from long double: b <= e).  n is the
number of butterfly stages of the COMPLEX transform (the real polynomial of N coefficients is folded into N / 2 complex
points: n = log2 N - 1); `extra` counts additional full multiplication stages a particular split adds (the separate twist
of the folded form; the W_h twiddle of the quarter split is the twiddle of its radix-4 stage and is NOT extra).

A limb sum is 2 l products of a digit polynomial (|d| <= Bg / 2) with a balanced limb polynomial (|k| <= 2^(bits - 1)):
||d|| <= sqrt(N) Bg / 2, ||k|| <= sqrt(N) 2^(bits - 1); the errors of the 2 l products add."""
import math
import sys

E = 2.0 ** -53


def percival_factor(n, beta=E):
    # (1 + 2^-53 is not representable: evaluate through log1p / expm1)
    return math.expm1(3 * n * math.log1p(E) + (3 * n + 1) * math.log1p(E * math.sqrt(5)) + 3 * n * math.log1p(beta))


def limb_sum_bound(log_n_poly, levels, base_log, limb_bits, extra=1, beta=E):
    """bound on |computed - exact| of one limb sum; extra = multiplication stages counted on top of the log2(N) - 1 butterflies"""
    n_poly = 1 << log_n_poly
    norm = n_poly * 2.0 ** (base_log - 1) * 2.0 ** (limb_bits - 1)      # ||d|| ||k||, both at their largest in every coefficient
    per_product = norm * percival_factor(log_n_poly - 1 + extra, beta)
    return 2 * levels * per_product, per_product


# The UNROLLED step (csrc/bmi_kernels_t64fu.hip at N = 1024, csrc/bmi_kernels_t64wu.hip at N = 2048): a limb's inverse transform
# returns sum_{j<3} (X^(c_j) - 1) sum_rows digit x limb - three keys, each scaled in the transform domain by a factor of
# magnitude <= 2: six times the plain limb sum.  The scaling is one more multiplication stage (extra = 2).  Its factor
# zeta^x - 1 is a table entry (rounded once from long double: the N = 2048 kernel folds one octant of the powers by exact
# symmetries, never multiplying two entries) minus one: absolute error <= e (the entry) + 2 e (the subtraction's rounding, on a
# result of magnitude <= 2) = 3 e on a factor bounded by 2, i.e. beta = 1.5 e, which the formula then charges to every stage.
# The bound does not depend on WHERE in a product's chain of multiplications the factor is applied: k_blind_rotate_wu_t64f scales
# a key's sums after the products with its rows, k_blind_rotate_wu2_t64f (csrc/bmi_kernels_t64wu2.hip: two ciphertexts per
# workgroup) scales the digit transform before them - the same stages on every product, one table entry per factor in both,
# hence the same bound for both kernels.
UNROLLED_BETA = 1.5 * E


def unrolled_limb_sum_bound(log_n_poly, levels, base_log, limb_bits):
    """bound on |computed - exact| of one limb sum of the unrolled step"""
    return 6 * limb_sum_bound(log_n_poly, levels, base_log, limb_bits, extra=2, beta=UNROLLED_BETA)[0]


SETS = {
    "north_star_torus64 (N 1024, l 3, Bg 2^10, 24-bit limbs)": (10, 3, 10, 24),
    "secure128_torus   (N 2048, l 3, Bg 2^10, 23-bit limbs)": (11, 3, 10, 23),
    "N 2048 with 24-bit limbs (NOT used: bound fails)": (11, 3, 10, 24),
    "N 4096 torus sets (l 3, Bg 2^10, 22-bit limbs)": (12, 3, 10, 22),
    "N 4096 with 23-bit limbs (NOT used: bound fails)": (12, 3, 10, 23),
}

UNROLLED_SETS = {
    "secure128_torus unrolled (N 2048, l 3, Bg 2^10, 20-bit limbs: key at 40 bits)": (11, 3, 10, 20),
    "N 2048 unrolled with 21-bit limbs (NOT used: bound fails)": (11, 3, 10, 21),
}

if __name__ == "__main__":
    for name, (lg, l, bg, lb) in SETS.items():
        total, per = limb_sum_bound(lg, l, bg, lb)
        total0, _ = limb_sum_bound(lg, l, bg, lb, extra=0)
        print(f"{name}: per product {per:.4f}, limb sum {total:.3f} (twist counted as a stage; {total0:.3f} without)  "
              f"{'< 1/2 ok' if total < 0.5 else '>= 1/2 NOT certified'}")
    for name, (lg, l, bg, lb) in UNROLLED_SETS.items():
        total = unrolled_limb_sum_bound(lg, l, bg, lb)
        plain = 6 * limb_sum_bound(lg, l, bg, lb)[0]
        print(f"{name}: limb sum {total:.3f} (scaling by zeta^x - 1 counted as a stage, beta 1.5 e; {plain:.3f} = 6 x the plain bound without)  "
              f"{'< 1/2 ok' if total < 0.5 else '>= 1/2 NOT certified'}")
    sys.exit(0)
