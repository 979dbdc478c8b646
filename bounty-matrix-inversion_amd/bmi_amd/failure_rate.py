"""Measured failure rate of a look-up against error_budget.lookup_failure_probability, where failures can be seen: a table one
or two bits wider than the parameter set carries comfortably, so that the Gaussian tail the budget sums is thousands of wrong
look-ups in 2^16 .. 2^18 instead of none in any soak run.

The harness stays on the device.  A pool of B encryptions of 0 is uploaded once; round r forms
in[i] = pool[i] + pool[(i + r + 1) mod B] + m_r[i] Delta with bmi_lincomb_batch (pairs of distinct pool rows have pairwise-independent
masks - all the variance of a count needs), bootstraps through the IDENTITY table of the width (every box boundary, the wrap
included, separates different outputs) and decrypts against the known messages with bmi_decrypt_batch; counts and noise
statistics are reduced with torch and only scalars come home."""
from __future__ import annotations

import math

import numpy as np

from . import error_budget as eb

SCALES = (0.85, 1.0, 1.15)     # the tolerance the variance terms of error_budget are held to (tests/test_gpu_parity.py)


def key_weights(eng):
    """(hw(s), hw(S)) of the secret keys the context holds (bmi_export_keys without the evaluation keys)"""
    from .tfhe import _ptr
    sk_small, sk_big = np.zeros(eng.P.n, np.uint64), np.zeros(eng.P.k * eng.P.N, np.uint64)
    eng._ck(eng.lib.bmi_export_keys(eng.h, _ptr(sk_small), _ptr(sk_big), None, None), "bmi_export_keys")
    return int(sk_small.sum()), int(sk_big.sum())


def prediction(P, lut_bits, n, hw_small, hw_big, modswitch=0):
    """per-look-up probabilities at variance_scale 0.85 / 1 / 1.15 for the sum of two fresh encryptions, the expected count and
    the accepted band [n p(0.85) - 3 sqrt(n p(0.85)), n p(1.15) + 3 sqrt(n p(1.15))] (model tolerance + Poisson sampling noise);
    modswitch: the engine's modulus-switch mode (Engine.modswitch: 1 = centred)"""
    p = [eb.lookup_failure_probability(P, lut_bits, input_variance=2.0 * P.glwe_noise ** 2, hw_small=hw_small, hw_big=hw_big,
                                       variance_scale=s, centred_modswitch=modswitch == 1) for s in SCALES]
    return {"p": dict(zip(("0.85", "1.0", "1.15"), p)), "expected": n * p[1],
            "band": [n * p[0] - 3.0 * math.sqrt(n * p[0]), n * p[2] + 3.0 * math.sqrt(n * p[2])]}


def _pool_stats(parts):
    """noise_stats dicts of disjoint samples -> the dict of their union"""
    n = sum(s["count"] for s in parts)
    if n == 0:
        return {"count": 0, "wrong": 0, "mean": 0.0, "std": 0.0, "max_abs": 0}
    mean = sum(s["count"] * s["mean"] for s in parts) / n
    second = sum(s["count"] * (s["std"] ** 2 + s["mean"] ** 2) for s in parts) / n
    return {"count": n, "wrong": sum(s["wrong"] for s in parts), "mean": mean, "std": math.sqrt(max(second - mean * mean, 0.0)),
            "max_abs": max(s["max_abs"] for s in parts)}


def measure(eng, lut_bits, rounds, pool=8192, seed=2024):
    """`rounds` x `pool` look-ups of uniform messages through the `lut_bits`-bit identity table on `eng` (keys generated), in the
    modulus-switch mode the engine is in (the prediction follows it).
    Returns {n, wrong, off_by_one (every wrong result is expected +-1 modulo 2^lut_bits), right / wrong_stats (Engine.noise_stats of
    the look-ups that decoded right / wrong, pooled over the rounds), hw_small, hw_big, delta_log} and the prediction()."""
    import torch
    P, B, big = eng.P, int(pool), eng.P.big
    dl = eng.delta_log(lut_bits)
    half, M = 1 << (lut_bits - 1), 1 << lut_bits
    dev = torch.device("cuda", eng.device)
    rng = np.random.default_rng(seed)
    lid = eng.lut_register(np.arange(-half, half), lut_bits, dl)
    q_word = eng.modulus & ((1 << 64) - 1)                      # q as a 64-bit word (0 on the torus) ...
    q_i64 = q_word - (1 << 64) if q_word >= 1 << 63 else q_word  # ... and its int64 bit pattern
    right, wrong_stats, wrong, off_by_one = [], [], 0, True
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream().cuda_stream
        d_pool = torch.from_numpy(eng.encrypt(np.zeros(B, np.int64), dl).view(np.int64)).to(dev)
        d_rp = torch.arange(0, 2 * B + 1, 2, dtype=torch.int32, device=dev)
        d_coef = torch.ones(2 * B, dtype=torch.int64, device=dev)
        d_ids = torch.full((B,), lid, dtype=torch.int32, device=dev)
        d_in = torch.empty((B, big), dtype=torch.int64, device=dev)
        d_out = torch.empty_like(d_in)
        d_msgs = torch.empty(B, dtype=torch.int64, device=dev)
        first = torch.arange(B, dtype=torch.int64, device=dev)
        for r in range(rounds):
            d_m = torch.from_numpy(rng.integers(-half, half, B)).to(dev)
            d_idx = torch.stack([first, (first + r + 1) % B], dim=1).reshape(-1).to(torch.int32)
            d_const = (d_m << dl) + (d_m < 0) * q_i64               # m 2^dl mod q as a word (int64 arithmetic wraps)
            eng.lincomb(d_pool, d_rp, d_idx, d_coef, d_const, B, d_in, s)
            eng.pbs(d_in, d_ids, B, d_out, s)
            eng.decrypt_device(d_out, B, dl, d_msgs, d_m, None, s)
            bad = d_msgs != d_m
            n_bad = int(bad.sum().item())
            wrong += n_bad
            if n_bad:
                diff = (d_msgs[bad] - d_m[bad]) % M
                off_by_one = off_by_one and bool(((diff == 1) | (diff == M - 1)).all().item())
                rows = bad.nonzero().reshape(-1)
                wrong_stats.append(eng.noise_stats(d_out[rows].contiguous(), n_bad, dl, d_m[rows].contiguous()))
            rows = (~bad).nonzero().reshape(-1)
            right.append(eng.noise_stats(d_out[rows].contiguous(), B - n_bad, dl, d_m[rows].contiguous()))
    hs, hb = key_weights(eng)
    n = rounds * B
    res = {"n": n, "lut_bits": lut_bits, "delta_log": dl, "rounds": rounds, "pool": B, "wrong": wrong, "off_by_one": off_by_one,
           "right": _pool_stats(right), "wrong_stats": _pool_stats(wrong_stats), "hw_small": hs, "hw_big": hb}
    res["modswitch"] = eng.modswitch
    res.update(prediction(P, lut_bits, n, hs, hb, res["modswitch"]))
    res["ratio"] = wrong / res["expected"] if res["expected"] > 0 else None
    res["pbs_output_std_model"] = math.sqrt(eb.pbs_output_variance(P, bsk_precision=eng.bsk_precision, hw_small=hs, hw_big=hb))
    return res
