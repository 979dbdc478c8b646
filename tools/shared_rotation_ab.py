#!/usr/bin/env python3
"""A/B of shared blind rotations (Executor(share_rotations=True): one keyswitch and one rotation per group of look-ups with the same
input) on the default torus engine (--engine unrolled: the same set with the unrolled key, 42 bits), in ONE process, the two forms
alternating:
    the 3x3 inverse in its serving form (evaluate_many, 8 matrices per walk)   and   the 8x8 inverse,
each `--reps` times with and without the flag, every result checked against the plaintext evaluation of the program.
With --traced B1,B2 it runs instead the reference's traced, lazily fused 2x2 inverse (tests/golden/ref_traced_inverse.json.gz, 5-bit
look-ups) on secure128_torus_wide (N = 4096), B inputs per walk (Executor(batch=B)), against the golden vector.
With --parent-tree DIR (a built checkout of the parent commit) it then runs `bench.py --gpus 1 --steps 5 --warmup 1` of that tree and
of this one alternating, `--bench-reps` times each, every run a fresh process: the headline must stay inside the parent's spread.
usage: shared_rotation_ab.py [--reps 3] [--cases 3x8,8x1] [--engine default|unrolled] [--traced 1,32] [--parent-tree DIR] [--bench-reps 3]
                             [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "bounty-matrix-inversion_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="3x8,8x1", help="n x matrices per walk, comma separated")
    ap.add_argument("--engine", default="default", choices=["default", "unrolled"])
    ap.add_argument("--traced", default=None, help="inputs per walk of the reference's fused 2x2 on secure128_torus_wide, comma separated")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--bench-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import numpy as np
    from bmi_amd import tfhe
    from bmi_amd.inverse_bench import CONFIGS
    from bmi_amd.main import EncryptedMatrixInversion

    def summary(label, times, counts):
        for flag in (False, True):
            t = times[flag]
            say(f"{label}, share_rotations={flag}: {counts[flag][0]} look-ups, {counts[flag][1]} rotations, "
                f"min / median / max {min(t):.3f} / {sorted(t)[len(t) // 2]:.3f} / {max(t):.3f} s (spread {max(t) - min(t):.3f}); executor build {counts[flag][2]:.1f} s")
        a, b = sorted(times[False])[len(times[False]) // 2], sorted(times[True])[len(times[True]) // 2]
        say(f"{label}: shared / unshared median {b / a:.3f}; rotations / look-ups {counts[True][1] / counts[True][0]:.3f}")

    if args.traced:
        import gzip
        from bmi_amd.circuit import Circuit
        from bmi_amd.executor import Executor
        say("shared rotations A/B (tools/shared_rotation_ab.py): the reference's fused 2x2 inverse on secure128_torus_wide, seeded keys; seconds per walk")
        with gzip.open(os.path.join(REPO, "tests", "golden", "ref_traced_inverse.json.gz"), "rt") as f:
            case = json.load(f)["cases"][2]
        circ, vec = Circuit.from_dict(case["circuit"]), case["vectors"][0]
        eng = tfhe.Engine(tfhe.preset_params("secure128_torus_wide"))
        eng.keygen(0x5EED)
        dl = eng.delta_log(circ.msg_bits)
        for batch in (int(v) for v in args.traced.split(",")):
            exs, counts, times = {}, {}, {False: [], True: []}
            for flag in (False, True):
                t0 = time.time()
                exs[flag] = Executor(circ, eng, batch=batch, share_rotations=flag)
                counts[flag] = (exs[flag].lookups, exs[flag].rotations, time.time() - t0)
            ct = np.stack([eng.encrypt(vec["inputs"], dl) for _ in range(batch)])
            for rep in range(args.reps):
                for flag in (False, True):
                    t0 = time.time()
                    res = exs[flag].run(ct if batch > 1 else ct[0])
                    times[flag].append(time.time() - t0)
                    ok = all(list(eng.decrypt(r, dl)) == vec["expected"] for r in res.reshape(batch, -1, res.shape[-1]))
                    say(f"  {case['name']} x {batch}  share_rotations={flag!s:5}  run {rep + 1}: {times[flag][-1]:8.3f} s  matches the golden vector: {ok}")
                    if not ok:
                        raise SystemExit("a decrypted output differs from the golden vector")
            summary(f"{case['name']}, {batch} per walk", times, counts)
            del exs
        eng.close()
        return

    say(f"shared rotations A/B (tools/shared_rotation_ab.py): {args.engine} torus engine, seeded keys; seconds per walk of the levels")
    eng = tfhe.Engine()
    if args.engine == "unrolled":
        eng.set_bsk_unroll(2)
    eng.keygen(0x5EED)
    for case in args.cases.split(","):
        n, batch = (int(v) for v in case.split("x"))
        ln, ints = CONFIGS[n]
        rng = np.random.default_rng(4321 + n)
        Ms = [rng.standard_normal((n, n)) * 100 for _ in range(batch)]
        emis = {flag: EncryptedMatrixInversion(n, None, 2, ln, ints, False, False, engine=eng, unroll=args.engine == "unrolled", share_rotations=flag)
                for flag in (False, True)}
        qs = [emis[False].quantize(M) for M in Ms]
        encs = [emis[False].encrypt(q, s) for q, s in qs]
        want = [emis[False].simulate(q, s) for q, s in qs]
        times = {False: [], True: []}
        counts = {}
        for flag in (False, True):
            t0 = time.time()
            ex = emis[flag]._executor(batch)
            counts[flag] = (ex.lookups, ex.rotations, time.time() - t0)
            if n <= 4:
                emis[flag].evaluate_many(encs)      # warm-up (first launches); skipped for the long 8x8 walk
        for rep in range(args.reps):
            for flag in (False, True):
                t0 = time.time()
                res = emis[flag].evaluate_many(encs)
                times[flag].append(time.time() - t0)
                ok = all(np.array_equal(emis[flag].decrypt(r), w) for r, w in zip(res, want))
                say(f"  {n}x{n} x {batch}  share_rotations={flag!s:5}  run {rep + 1}: {times[flag][-1]:8.3f} s  matches the plaintext circuit: {ok}")
                if not ok:
                    raise SystemExit("a decrypted inverse differs from the plaintext evaluation")
        summary(f"{n}x{n} (len {ln}, ints {ints}), {batch} per walk", times, counts)
        for e in emis.values():
            e._exec = None
    eng.close()
    del eng

    if args.parent_tree:
        import torch
        torch.cuda.empty_cache()
        vals = {"parent": [], "branch": []}
        for rep in range(args.bench_reps):
            for name, tree in (("parent", args.parent_tree), ("branch", REPO)):
                p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1"], cwd=tree, capture_output=True, text=True,
                                   timeout=600)
                if p.returncode != 0:
                    say(f"bench.py of the {name} tree failed (exit {p.returncode}): {p.stderr[-400:]}")
                    raise SystemExit(1)
                res = json.loads([ln_ for ln_ in p.stdout.splitlines() if ln_.startswith("{")][-1])
                vals[name].append(float(res["value"]))
                say(f"  bench.py --gpus 1 --steps 5 --warmup 1, {name}, run {rep + 1}: {res['value']} {res.get('unit', '')}")
        for name, v in vals.items():
            say(f"bench.py {name}: min / max {min(v):.0f} / {max(v):.0f} (spread {max(v) - min(v):.0f})")
        lo, hi = min(vals["parent"]), max(vals["parent"])
        say(f"branch within the parent's spread: {all(lo <= x <= hi for x in vals['branch'])}; branch median / parent median "
            f"{sorted(vals['branch'])[len(vals['branch']) // 2] / sorted(vals['parent'])[len(vals['parent']) // 2]:.4f}")


if __name__ == "__main__":
    main()
