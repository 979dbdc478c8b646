"""Circuit-level error budget: the probability that an encrypted evaluation of a compiled program returns a wrong integer
because of NOISE (as opposed to an input outside the traced ranges, which `Program.simulate` catches).

Concrete sizes its parameters for a global `p_error` (the reference relies on it: `fhe.Compiler(...).compile(inputset)` at its
defaults, matrix_inversion/main.py:53-66; `fhe.Configuration(...)` in qfloat_matrix_inversion.py:995-1002).  This module is the
counterpart for the fixed, documented parameter sets of this library: for every look-up of a program it computes the standard
deviation of what reaches the blind rotation and the distance to the nearest decision boundary, and sums the Gaussian tails.

Noise model (variances relative to q^2; the formulas the GPU tests hold the measured noise to within +-15 %,
tests/test_gpu_parity.py, tests/test_gpu_torus_wide.py):

  PBS output      v_pbs = n l (k+1) N (Bg^2 + 2) / 12 * s_eff^2  +  hw(s) (1 + hw(S)) / (12 Bg^(2l)),
                  s_eff^2 = glwe_noise^2 + (1 + hw(S)) 4^(64 - prec) / 12 / 2^128   (torus key stored at prec < 64 bits);
                  unrolled key: 3 x the key term, rounding term 2 x (pairs of key bits not both zero)
  fresh input     v_enc = glwe_noise^2                                                       (bmi_encrypt)
  a look-up's input is a linear combination sum_t c_t leaf_t: v_in = sum_t c_t^2 v(leaf_t)   (independent leaves)
  keyswitch       v_ks = kN l_ks (B^2 + 2) / 12 * lwe_noise^2 + hw(S) / (12 B^(2 l_ks))
  mod-switch      (v_in + v_ks) (2N)^2 + (1 + hw(s)) / 12    positions^2 on the circle of 2N positions
  ... centred     (v_in + v_ks) (2N)^2 + (1 + n / 4) / 12    (centred_modswitch=True: bmi_set_modswitch(ctx, 1) subtracts the public
                  mean sum e_i / 2 of the mask words' rounding errors from the body; what is left, sum (s_i - 1/2) e_i - e_b, does
                  not depend on the key's weight)

Decision boundary: a table over p bits has boxes of 2N / 2^(p+1) positions (narrower tables than the circuit's message space are
scaled up by the tracer: wider boxes, and their coefficients carry the scale); a value fails when the noise exceeds half a box on
either side: P = erfc(half_box / (sigma sqrt 2)).  Outputs fail at decryption when their noise exceeds Delta / 2.

Shared rotations (share_rotations=True; shared_rotation.py): a look-up served from a rotation it shares with others is
SampleExtract(ACC P_f), P_f its table's sparse factor (from the same shared_rotation.rotation_groups the executor runs).  v_pbs
splits into a part that is white across the accumulator's coefficients and a part carried by the GLWE key, whose coefficients are
correlated (pbs_output_variance_parts: v_pbs = v_white + hw(S) v_carried); the output carries

    |P_f|^2 v_white  +  N (p (1 - p) |P_f|^2 + p^2 mean_j m_j^2) v_carried,        p = hw(S) / N

(the expectation of |S P_f|^2 over keys of that weight; shared_rotation's docstring).  |P_f|^2 v_pbs, the white-noise model, was
measured 3.1 x too low for the identity table and 1.7 x too high for a random one on the default set; this one within 3 %
(tests/test_gpu_shared_rotation.py, EXPERIMENTS A21).  A group of one is an ordinary look-up.  On the unrolled key the parts
are the same split of its own variance (3 x the key terms; rounding 2 x per pair of key bits not both zero, once white and once per
set bit of S): measured within 2 % (tests/test_gpu_shared_rotation_wide_unrolled.py, EXPERIMENTS A23).

Compressed outputs (compressed_outputs=(levels L, base_log b, log_modulus c); include/bmi_tfhe.h, csrc/lwe_pack.hip): an output packed
with `count` others into a GLWE ciphertext and cut to c bits per word carries, on top of its own variance, compression_variance =

    min(count, N) N L (4^b + 2) / 12 glwe_noise^2   (the key's noise: N L digits of each of the block's ciphertexts)
  + hw(S) 4^(-L b) / 12                              (the rounding of the mask words to the top L b bits)
  + (1 + N / 4) / 12 4^(-c)                          (the centred switch of the 2N GLWE words to c bits)

each term held alone to +-15 % (tests/test_compress_model.py, tests/test_gpu_compress.py).

Decompressed inputs (input_variance=...; csrc/lwe_unpack.hip): decompression back to an LWE ciphertext adds no noise of its own - the
phase of the decompressed ciphertext is bit for bit the compressed one - but what a circuit then reads is no fresh encryption: it
carries decompressed_variance = source_variance + compression_variance.  The caller says what was compressed: source_variance =
glwe_noise^2 for fresh encryptions compressed by the client's side, and for chained results the output variance of the circuit that
produced them (a bootstrapped leaf: pbs_output_variance times its squared coefficients).  failure_probability(..., input_variance=v)
then uses v (a scalar, or one value per input) for the input leaves in place of glwe_noise^2.  At the key shape (1, 16) the
rounding term alone is a standard deviation of 2^-13.3 of the torus whatever log_modulus is; it is not negligible against a look-up's
margin (2x2 inverse on the default set: 10^-5.77 fresh, 10^-5.26 from (1, 16, 16), useless at 12 bits).

Key weights are random: hw(s) = n / 2, hw(S) = kN / 2 (their expectations) unless given."""
from __future__ import annotations

import math

import numpy as np

TORUS64 = 65


def default_bsk_precision(P):
    """bits of precision the library stores a bootstrap key at by default (csrc/bmi_host.cpp default_bsk_precision)"""
    if P.q_bits != TORUS64:
        return 64
    if P.log_N == 11:
        return 46
    if P.log_N == 12:
        return 44
    return 48 if P.bs_base_log <= 10 else 64


def pbs_output_variance(P, bsk_precision=None, unroll=False, hw_small=None, hw_big=None):
    N, k, l, n = 1 << P.log_N, P.k, P.bs_levels, P.n
    Bg = 2.0 ** P.bs_base_log
    hs = n / 2.0 if hw_small is None else float(hw_small)
    hb = k * N / 2.0 if hw_big is None else float(hw_big)
    prec = default_bsk_precision(P) if bsk_precision is None else int(bsk_precision)
    s2 = P.glwe_noise ** 2
    if P.q_bits == TORUS64 and prec < 64:
        s2 += (1 + hb) * 4.0 ** (64 - prec) / 12.0 / 2.0 ** 128
    key = n * l * (k + 1) * N * (Bg * Bg + 2) / 12.0 * s2
    rnd = (1 + hb) / (12.0 * Bg ** (2 * l))
    if unroll:
        return 3 * key + 2 * _live_pairs(n, hw_small) * rnd
    return key + hs * rnd


def _live_pairs(n, hw_small):
    """pairs of LWE key bits not both zero (the steps of an unrolled rotation whose rounding reaches the output): 3/4 of the
    pairs at the average weight, else the upper bound the weight alone gives"""
    return (n + 1) // 2 * 0.75 if hw_small is None else min((n + 1) // 2, float(hw_small))


def pbs_output_variance_parts(P, bsk_precision=None, hw_small=None, hw_big=None, unroll=False, live_pairs=None):
    """(v_white, v_carried) with pbs_output_variance = v_white + hw(S) v_carried: the noise that is white across the
    accumulator's coefficients - the key's Gaussian noise, the rounding of the stored body words, the decomposition's rounding of
    the body - and, per set bit of the GLWE key, the noise that key carries (the roundings of the mask words).
    unroll: the same split of the unrolled key's variance (3 x the key term; the rounding term 2 x per pair of LWE key bits not
    both zero: `live_pairs`, else the count pbs_output_variance(unroll=True) assumes for the same hw_small).  Without a
    bsk_precision both functions price default_bsk_precision(P); the unrolled floating-point-transform engine of the torus stores
    its key at 42 bits, so a budget for a live engine passes engine.bsk_precision."""
    N, k, l, n = 1 << P.log_N, P.k, P.bs_levels, P.n
    Bg = 2.0 ** P.bs_base_log
    hs = n / 2.0 if hw_small is None else float(hw_small)
    prec = default_bsk_precision(P) if bsk_precision is None else int(bsk_precision)
    rho = 4.0 ** (64 - prec) / 12.0 / 2.0 ** 128 if (P.q_bits == TORUS64 and prec < 64) else 0.0
    K = n * l * (k + 1) * N * (Bg * Bg + 2) / 12.0
    if unroll:
        rnd = 2 * (_live_pairs(n, hw_small) if live_pairs is None else float(live_pairs)) / (12.0 * Bg ** (2 * l))
        return 3 * K * (P.glwe_noise ** 2 + rho) + rnd, 3 * K * rho + rnd
    rnd = hs / (12.0 * Bg ** (2 * l))
    return K * (P.glwe_noise ** 2 + rho) + rnd, K * rho + rnd


def keyswitch_variance(P, hw_big=None):
    N, k = 1 << P.log_N, P.k
    B = 2.0 ** P.ks_base_log
    hb = k * N / 2.0 if hw_big is None else float(hw_big)
    return k * N * P.ks_levels * (B * B + 2) / 12.0 * P.lwe_noise ** 2 + hb / (12.0 * B ** (2 * P.ks_levels))


def compression_variance(P, levels, base_log, log_modulus, count, hw_big=None):
    """variance (torus^2, the units of pbs_output_variance) that compression adds to each of `count` ciphertexts packed together
    (per block of N) at the key shape (levels, base_log) and cut to log_modulus bits: key noise + decomposition rounding + centred
    modulus switch (module docstring)"""
    N = 1 << P.log_N
    hb = P.k * N / 2.0 if hw_big is None else float(hw_big)
    key = min(int(count), N) * N * levels * (4.0 ** base_log + 2) / 12.0 * P.glwe_noise ** 2
    rounding = hb * 4.0 ** (-levels * base_log) / 12.0
    switch = (1 + N / 4.0) / 12.0 * 4.0 ** (-log_modulus)
    return key + rounding + switch


def decompressed_variance(P, levels, base_log, log_modulus, count, source_variance, hw_big=None):
    """variance (torus^2) of a ciphertext decompressed from `count` packed together at the key shape (levels, base_log) and
    log_modulus bits: what the compressed ciphertext carried (source_variance: glwe_noise^2 for a fresh encryption, the producing
    circuit's output variance for a chained result) plus compression_variance; the decompression adds nothing (module docstring)"""
    return float(source_variance) + compression_variance(P, levels, base_log, log_modulus, count, hw_big)


def _log_erfc(x):
    """log10 of erfc(x), finite for large x (erfc underflows beyond x ~ 26)"""
    x = np.asarray(x, np.float64)
    out = np.empty_like(x)
    small = x < 25.0
    with np.errstate(divide="ignore"):
        out[small] = np.log10(np.maximum(np.vectorize(math.erfc)(x[small]), 1e-320)) if small.any() else 0
    big = ~small
    # erfc(x) ~ exp(-x^2) / (x sqrt(pi))
    out[big] = (-x[big] ** 2 - np.log(x[big] * math.sqrt(math.pi))) / math.log(10.0)
    return out


def _lookup_margin(P, lut_bits, input_variance, v_ks, hs, variance_scale=1.0, centred_modswitch=False):
    """(sigma in positions of the 2N circle, half box / sigma) of look-ups through tables of `lut_bits` bits (scalars or arrays)"""
    N = 1 << P.log_N
    rounding = (1 + P.n / 4.0) / 12.0 if centred_modswitch else (1 + hs) / 12.0
    sigma_pos = np.sqrt(((input_variance + v_ks) * (2.0 * N) ** 2 + rounding) * variance_scale)
    return sigma_pos, N / (2.0 ** (lut_bits + 1)) / sigma_pos


def failure_probability(prog, P, bsk_precision=None, unroll=False, hw_small=None, hw_big=None, share_rotations=False,
                        centred_modswitch=False, compressed_outputs=None, input_variance=None):
    """Error budget of `prog` (a program.Program) under the parameter set `P` (tfhe.Params or anything with its fields).
    input_variance: None (fresh encryptions: glwe_noise^2), or the variance in torus^2 of the inputs as they arrive - a scalar, or
    an array of n_inputs values - e.g. decompressed_variance(...) for inputs that arrive compressed (module docstring).
    centred_modswitch: the budget of an engine in modulus-switch mode 1 (only the rounding term of the mod-switch changes).
    compressed_outputs: None, or (levels, base_log, log_modulus) of outputs that come home compressed (Executor.run_compressed):
    compression_variance of the program's outputs packed together is added to every output's own variance.

    Returns a dict: p_fail (probability that at least one look-up or output decodes wrong, union bound), log10_p_fail,
    lookups, worst_margin_sigma (smallest half-box / sigma over the look-ups), p_fail_worst_lookup, widest_amplification
    (largest sum of squared coefficients feeding a look-up), output_margin_sigma, sigma_positions_typical."""
    N = 1 << P.log_N
    n_in, nn = prog.n_inputs, prog.n_nodes
    v_pbs = pbs_output_variance(P, bsk_precision, unroll, hw_small, hw_big)
    v_enc = P.glwe_noise ** 2
    v_ks = keyswitch_variance(P, hw_big)
    hs = P.n / 2.0 if hw_small is None else float(hw_small)
    leaf_var = np.full(n_in + nn, v_pbs)
    if input_variance is None:
        leaf_var[:n_in] = v_enc
    else:
        v_inp = np.asarray(input_variance, np.float64)
        if v_inp.ndim > 1 or (v_inp.ndim == 1 and v_inp.size != n_in):
            raise ValueError(f"input_variance: a scalar or {n_in} values, one per input (got shape {v_inp.shape})")
        if v_inp.size and (not np.all(np.isfinite(v_inp)) or v_inp.min() < 0):
            raise ValueError("input_variance: variances are finite and not negative")
        leaf_var[:n_in] = v_inp
    shared = 0
    if share_rotations and nn:
        from .shared_rotation import rotation_groups
        rg = rotation_groups(prog)
        in_shared = np.repeat(rg.sizes, rg.sizes) > 1
        v_white, v_carried = pbs_output_variance_parts(P, bsk_precision, hw_small, hw_big, unroll=unroll)
        dens = 0.5 if hw_big is None else float(hw_big) / (P.k * N)
        carried2 = N * (dens * (1 - dens) * rg.norm2[in_shared] + dens * dens * rg.mean2[in_shared])      # E |S P_f|^2
        leaf_var[n_in + rg.members[in_shared]] = rg.norm2[in_shared] * v_white + carried2 * v_carried
        shared = int(in_shared.sum())

    def lincomb_var(ptr, leaf, coef):
        ln = np.diff(ptr)
        seg = np.repeat(np.arange(ln.size), ln)
        c2 = np.asarray(coef, np.float64) ** 2
        return (np.bincount(seg, weights=c2 * leaf_var[leaf], minlength=ln.size),
                np.bincount(seg, weights=c2, minlength=ln.size))

    res = {"lookups": int(nn), "params": {"n": int(P.n), "N": int(N), "l": int(P.bs_levels), "log2_Bg": int(P.bs_base_log),
                                          "q_bits": int(P.q_bits), "log2_lwe_noise": round(math.log2(P.lwe_noise), 2)},
           "log2_std_pbs_output": 0.5 * math.log2(v_pbs), "log2_std_keyswitch": 0.5 * math.log2(v_ks)}
    if share_rotations:
        res.update(shared_lookups=shared, rotations=int(rg.groups) if nn else 0)
    log_terms = []
    if nn:
        v_in, amp = lincomb_var(prog.node_ptr, prog.term_leaf, prog.term_coef)
        p_node = prog.lut_p[prog.node_lut].astype(np.int64)
        if (1 << (int(p_node.max()) + 1)) > N:
            raise ValueError(f"a {int(p_node.max())}-bit look-up does not fit N = {N}")
        sigma_pos, margin = _lookup_margin(P, p_node, v_in, v_ks, hs, centred_modswitch=centred_modswitch)
        lp = _log_erfc(margin / math.sqrt(2.0))
        log_terms.append(lp)
        res.update(worst_margin_sigma=float(margin.min()), log10_p_fail_worst_lookup=float(lp.max()),
                   widest_amplification=float(amp.max()), sigma_positions_typical=float(np.median(sigma_pos)))
    if prog.n_outputs:
        v_out, _ = lincomb_var(prog.out_ptr, prog.out_leaf, prog.out_coef)
        if compressed_outputs is not None:
            v_out = v_out + compression_variance(P, *compressed_outputs, count=prog.n_outputs, hw_big=hw_big)
        m_out = 2.0 ** -(prog.msg_bits + 2) / np.sqrt(np.maximum(v_out, 1e-300))     # Delta / 2 over sigma, Delta = q / 2^(msg_bits + 1)
        log_terms.append(_log_erfc(m_out / math.sqrt(2.0)))
        res["output_margin_sigma"] = float(m_out.min())
    if log_terms:
        lt = np.concatenate(log_terms)
        mx = float(lt.max())
        log10_sum = mx + math.log10(float(np.sum(10.0 ** (lt - mx))))       # union bound, summed in log space
        res["log10_p_fail"] = min(log10_sum, 0.0)
        res["p_fail"] = min(1.0, 10.0 ** log10_sum) if log10_sum > -300 else 0.0
    else:
        res.update(log10_p_fail=-math.inf, p_fail=0.0)
    return res


def engine_failure_probability(prog, eng, hw_small=None, hw_big=None, share_rotations=False, compressed_outputs=None,
                               input_variance=None):
    """failure_probability of `prog` on a live tfhe.Engine as it is configured: its parameters, the precision its bootstrap key is
    stored at, its unrolling and its modulus-switch mode (Engine.modswitch; a stand-in without that attribute counts as mode 0).
    Program.failure_probability(engine) prices the standard switch whatever the engine's mode: program.py is part of the tracer
    fingerprint that names the shipped programs, so the mode is read here instead."""
    return failure_probability(prog, eng.P, eng.bsk_precision if eng.q_bits == TORUS64 else None, getattr(eng, "unroll", 1) == 2,
                               hw_small, hw_big, share_rotations=share_rotations,
                               centred_modswitch=getattr(eng, "modswitch", 0) == 1, compressed_outputs=compressed_outputs,
                               input_variance=input_variance)


def lookup_failure_probability(P, lut_bits, input_variance=0.0, bsk_precision=None, unroll=False, hw_small=None, hw_big=None,
                               variance_scale=1.0, centred_modswitch=False):
    """The per-look-up term of failure_probability on its own: the probability that one look-up through a table of `lut_bits`
    bits decodes a neighbouring box, for an input of variance `input_variance` (relative to q^2: 2 glwe_noise^2 for the sum of
    two fresh encryptions, pbs_output_variance(P, bsk_precision, unroll, ...) times the squared coefficients for bootstrapped
    leaves - the only place the key's precision and unrolling enter, so those two arguments are accepted and unused here).
    `variance_scale` multiplies the variance in positions^2 (the +-15 % the variance terms are held to give the band a measured
    failure count is accepted in: tests/test_gpu_decrypt_device.py).  centred_modswitch: as in failure_probability."""
    N = 1 << P.log_N
    if (1 << (int(lut_bits) + 1)) > N:
        raise ValueError(f"a {int(lut_bits)}-bit look-up does not fit N = {N}")
    hs = P.n / 2.0 if hw_small is None else float(hw_small)
    _, margin = _lookup_margin(P, int(lut_bits), float(input_variance), keyswitch_variance(P, hw_big), hs, float(variance_scale),
                               centred_modswitch)
    return float(10.0 ** _log_erfc(np.array([margin / math.sqrt(2.0)]))[0])


def candidate_sets(msg_bits, q_bits=None, secure=False):
    """Parameter sets to try in order (cheapest first) for a circuit of `msg_bits`-bit look-ups: (label, kwargs of
    tfhe.default_params) or (label, preset name)."""
    from . import tfhe
    torus = q_bits in (None, tfhe.TORUS64)       # None: the library's default modulus
    if secure:
        # the secure LWE noise leaves a 4-bit look-up 9 sigma at N = 2048; a 5-bit one sits at 4.4 sigma there and at 4.9 sigma at
        # N = 4096 (torus only) - whether that meets p_error is the budget's call, circuit by circuit
        if msg_bits > 5 or (msg_bits > 4 and not torus):
            raise ValueError("the 128-bit-secure sets carry 4-bit look-ups (5-bit ones on the 2^64 torus, at 4.4 - 4.9 sigma)")
        return [("secure128_torus", "secure128_torus"), ("secure128_torus_wide", "secure128_torus_wide")] if torus else [("secure128", "secure128")]
    out = []
    for log_n in (10, 11, 12):
        if (1 << (msg_bits + 6)) > (1 << log_n):
            continue                                  # N >= 2^(msg_bits + 6): the box structure of the tracer's message space
        qb = tfhe.TORUS64 if torus else 49
        out.append((f"q_bits={qb}, N={1 << log_n}", dict(q_bits=qb, log_N=log_n) if log_n != 10 else dict(q_bits=qb)))
    if not out:
        raise ValueError(f"no parameter set carries {msg_bits}-bit look-ups on this modulus")
    return out


def choose_params(prog, p_error=1e-5, q_bits=None, secure=False, unroll=False, share_rotations=False, centred_modswitch=False,
                  compressed_outputs=None):
    """The first candidate set whose failure probability for `prog` is at most p_error (Concrete's `global_p_error`); the report of
    every set tried.  Raises when none qualifies.  centred_modswitch and compressed_outputs are passed through to
    failure_probability."""
    from . import tfhe
    tried = []
    for label, spec in candidate_sets(prog.msg_bits, q_bits, secure):
        P = tfhe.preset_params(spec) if isinstance(spec, str) else tfhe.default_params(**spec)
        # unrolled kernels: N = 1024, and the 2^64 torus at N = 2048, whose unrolled key is stored at 40 bits (bmi_set_bsk_unroll)
        if unroll and P.log_N == 11 and P.q_bits == TORUS64:
            rep = failure_probability(prog, P, 40, unroll=True, share_rotations=share_rotations, centred_modswitch=centred_modswitch,
                                      compressed_outputs=compressed_outputs)
        else:
            rep = failure_probability(prog, P, unroll=unroll and P.log_N == 10, share_rotations=share_rotations,
                                      centred_modswitch=centred_modswitch, compressed_outputs=compressed_outputs)
        tried.append((label, rep["p_fail"]))
        if rep["p_fail"] <= p_error:
            return P, dict(rep, chosen=label, tried=tried, p_error=p_error)
    raise ValueError(f"no parameter set reaches p_error = {p_error:g} for this circuit: tried {tried}")
