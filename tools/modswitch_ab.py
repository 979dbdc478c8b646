#!/usr/bin/env python3
"""Cost of the centred modulus switch (bmi_set_modswitch(ctx, 1); record: profiles/centred_modswitch_ab.txt).  ONE process, one
engine per parameter set, the two modes alternating `rounds` times each (0 1 0 1 ...):
  (a) bmi_pbs_batch on device buffers between two events, at 256 and at 8,192 ciphertexts on the default set: one warm call, then
      the mean of `reps` calls per sample;
  (b) the wall-clock of one evaluation of the encrypted 3x3 inverse (len 30, ints 12) on the default set and on secure128_torus,
      decrypted against the golden digits of tests/golden/inverse.json in both modes.
Rule, per line: every mode 1 sample lies inside the min .. max spread of the mode 0 samples of the same process.  A line that
does not is reported with the measured cost (median mode 1 - median mode 0); the mode stays opt-in either way.
Also timed: bmi_modswitch_centre_batch alone at both batch sizes.
usage: modswitch_ab.py [--rounds 3] [--reps 5] [--out FILE]"""
import json, os, statistics, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "bounty-matrix-inversion_amd"))
import numpy as np, torch
from bmi_amd import error_budget, tfhe
from bmi_amd.main import EncryptedMatrixInversion

BATCHES = (256, 8192)


def option(args, name, default):
    if name in args:
        i = args.index(name)
        v = args[i + 1]
        del args[i:i + 2]
        return v
    return default


def events(call, reps):
    call(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): call()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def verdict(label, unit, samples, lines):
    lo, hi = min(samples[0]), max(samples[0])
    inside = all(lo <= x <= hi for x in samples[1])
    cost = statistics.median(samples[1]) - statistics.median(samples[0])
    lines.append(f"{label:44} mode 0: " + " ".join(f"{x:.4f}" for x in samples[0]) + "   mode 1: " + " ".join(f"{x:.4f}" for x in samples[1]) +
                 f"   {unit}; mode 0 spread {lo:.4f} .. {hi:.4f}: mode 1 {'INSIDE' if inside else 'OUTSIDE'}, median cost {cost:+.4f} {unit} "
                 f"({100 * cost / statistics.median(samples[0]):+.2f} %)")
    print(lines[-1], flush=True)
    return inside


def main():
    args = sys.argv[1:]
    rounds, reps = int(option(args, "--rounds", 3)), int(option(args, "--reps", 5))
    out = option(args, "--out", None)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    lines, outside = [], 0
    with open(os.path.join(REPO, "tests", "golden", "inverse.json")) as f:
        golden = next(x for x in json.load(f) if x["tag"] == "baseline_n3_len30_ints12")
    M = np.array(golden["M"]).reshape(3, 3)
    for preset in ("north_star_torus64", "secure128_torus"):
        eng = tfhe.Engine(tfhe.preset_params(preset))
        eng.keygen(0x5EED)
        dl = eng.delta_log()
        if preset == "north_star_torus64":
            # (a) the flat batch
            eng.reserve(max(BATCHES))
            lid = eng.lut_register(np.random.default_rng(9).integers(-8, 8, 16), 4, dl)
            for B in BATCHES:
                d_in = torch.from_numpy(eng.encrypt(np.random.default_rng(B).integers(-8, 8, B), dl).view(np.int64)).to(dev)
                d_ids = torch.full((B,), lid, dtype=torch.int32, device=dev)
                d_out = torch.empty_like(d_in)
                d_small = torch.empty((B, eng.P.small), dtype=torch.int64, device=dev)
                eng.keyswitch(d_in, B, d_small, s)
                samples = {0: [], 1: []}
                for r in range(2 * rounds):
                    eng.set_modswitch(r % 2)
                    samples[r % 2].append(events(lambda: eng.pbs(d_in, d_ids, B, d_out, s), reps))
                eng.set_modswitch(0)
                outside += not verdict(f"(a) bmi_pbs_batch, {B} ciphertexts, {eng.rotation_kernel(B)}", "ms", samples, lines)
                alone = events(lambda: eng.modswitch_centre(d_small, B, d_small, s), 20)
                lines.append(f"    bmi_modswitch_centre_batch alone, {B} x {eng.P.small} words in place: {alone * 1e3:.1f} us")
                print(lines[-1], flush=True)
        # (b) the 3x3 inverse
        emi = EncryptedMatrixInversion(3, None, 2, 30, 12, False, False, engine=eng)
        q, sg = emi.quantize(M)
        enc = emi.encrypt(q, sg)
        emi._executor()
        emi.evaluate(enc)
        samples, right = {0: [], 1: []}, True
        for r in range(2 * rounds):
            eng.set_modswitch(r % 2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = emi.evaluate(enc)
            samples[r % 2].append(time.perf_counter() - t0)
            right = right and emi.decrypt(res).tolist() == golden["out"]
        budgets = []
        for mode in (0, 1):
            eng.set_modswitch(mode)
            b = error_budget.engine_failure_probability(emi.program, eng)
            budgets.append(f"mode {mode}: worst margin {b['worst_margin_sigma']:.2f} sigma, p_fail {b['p_fail']:.1e}")
        eng.set_modswitch(0)
        outside += not verdict(f"(b) 3x3 inverse, {preset}", "s", samples, lines)
        lines.append(f"    golden digits in every run: {right}; " + "; ".join(budgets))
        print(lines[-1], flush=True)
        eng.close()
    lines.append(f"{outside} line(s) with a mode 1 sample outside the mode 0 spread")
    print(lines[-1])
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


main()
