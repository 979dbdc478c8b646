#!/usr/bin/env python3
"""Failure-rate calibration of the error budget on the GPU box (bmi_amd/failure_rate.py): observed wrong look-ups through an
identity table too wide for the parameter set against error_budget.lookup_failure_probability, plus the time of the device
phase kernel beside a one-term bmi_lincomb_batch over the same rows (same bytes read).
usage: gpu_failure_rate.py [PRESET:LUT_BITS:ROUNDS ...] [--out FILE] [--commit ID] [--centred]
  --centred: the engines in modulus-switch mode 1 (bmi_set_modswitch; measure() and its prediction follow the engine's mode)
  default cases: north_star_torus64:5:32 secure128_torus:6:8 north_star_torus64:4:1 ; default FILE profiles/failure_rate_calibration.json"""
import json, os, subprocess, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "bounty-matrix-inversion_amd"))
import numpy as np, torch
from bmi_amd import tfhe, failure_rate

DEFAULT_CASES = ["north_star_torus64:5:32", "secure128_torus:6:8", "north_star_torus64:4:1"]


def head_commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    except Exception:
        return "unknown"


def kernel_times(eng, B=8192, reps=20):
    """ms per call (HIP events, mean of `reps` after a warm-up): k_lwe_phase on B ciphertexts, bmi_lincomb_batch on B one-term rows"""
    dev = torch.device("cuda", eng.device)
    s = torch.cuda.current_stream().cuda_stream
    d_ct = torch.from_numpy(eng.encrypt(np.zeros(B, np.int64), eng.delta_log()).view(np.int64)).to(dev)
    d_phase = torch.empty(B, dtype=torch.int64, device=dev)
    d_out = torch.empty_like(d_ct)
    d_rp = torch.arange(B + 1, dtype=torch.int32, device=dev)
    d_idx = torch.arange(B, dtype=torch.int32, device=dev)
    d_coef = torch.ones(B, dtype=torch.int64, device=dev)
    d_const = torch.zeros(B, dtype=torch.int64, device=dev)
    calls = {"lwe_phase_ms": lambda: eng.phase_device(d_ct, B, d_phase, s),
             "lincomb_one_term_ms": lambda: eng.lincomb(d_ct, d_rp, d_idx, d_coef, d_const, B, d_out, s)}
    out = {"ciphertexts": B, "width": eng.P.big}
    for name, call in calls.items():
        call(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): call()
        e1.record(); torch.cuda.synchronize()
        out[name] = e0.elapsed_time(e1) / reps
    out["read_GBps_lwe_phase"] = B * eng.P.big * 8 / out["lwe_phase_ms"] / 1e6
    return out


def main():
    args = sys.argv[1:]
    centred = "--centred" in args
    if centred:
        args.remove("--centred")
    opt = {"--out": os.path.join(REPO, "profiles", "failure_rate_calibration.json"), "--commit": None}
    for k in list(opt):
        if k in args:
            i = args.index(k); opt[k] = args[i + 1]; del args[i: i + 2]
    cases = args or DEFAULT_CASES
    engines, report = {}, {"head_commit": opt["--commit"] or head_commit(), "key_seed": "0x5EED", "modswitch": int(centred), "cases": [], "kernel_times": []}
    for case in cases:
        preset, bits, rounds = case.split(":")
        if preset not in engines:
            engines[preset] = tfhe.Engine(tfhe.preset_params(preset))
            engines[preset].keygen(0x5EED)
            if centred:
                engines[preset].set_modswitch(1)
            report["kernel_times"].append(dict(preset=preset, **kernel_times(engines[preset])))
        res = failure_rate.measure(engines[preset], int(bits), int(rounds))
        report["cases"].append(dict(preset=preset, **res))
        print(f"{case}: observed {res['wrong']} of {res['n']}, predicted {res['expected']:.1f} (band {res['band'][0]:.0f} .. {res['band'][1]:.0f}), "
              f"ratio {res['ratio']:.3f}, hw {res['hw_small']}/{res['hw_big']}, right-look-up output std 2^{np.log2(res['right']['std']):.2f} "
              f"(model 2^{np.log2(res['pbs_output_std_model']):.2f}), off by one: {res['off_by_one']}", flush=True)
    for t in report["kernel_times"]:
        print(f"{t['preset']}: k_lwe_phase {t['lwe_phase_ms']:.4f} ms, one-term lincomb {t['lincomb_one_term_ms']:.4f} ms on {t['ciphertexts']} x {t['width']} words")
    for e in engines.values():
        e.close()
    with open(opt["--out"], "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
