#!/usr/bin/env python3
"""A/B of the unrolled bootstrap key on secure128_torus (N = 2048; k_blind_rotate_wu_t64f, key at 40 bits) against the plain
kernel of the same set (k_blind_rotate_w_t64f, key at 46 bits: the yardstick), in ONE process on the same seeded secret keys:
    blind_rotate of 1 and of 256 resident ciphertexts, between two HIP events around `--calls` back-to-back calls, the two engines
    alternating `--reps` times (medians and spreads);
    then the golden 3x3 inverse (tests/golden/inverse.json baseline_n3_len30_ints12), evaluate wall-clock on both, alternating,
    every result checked against the reference's digits.
usage: unrolled_wide_ab.py [--reps 5] [--calls 10] [--inverse-reps 3] [--out profiles/unrolled_wide_ab.txt]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "bounty-matrix-inversion_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--inverse-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 4:
        raise SystemExit("--reps: the engines alternate at least four times")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import numpy as np
    import torch
    from bmi_amd import tfhe
    from bmi_amd.main import EncryptedMatrixInversion

    say("unrolled key A/B on secure128_torus (tools/unrolled_wide_ab.py): seeded keys 0x5EED, one process, engines alternating")
    engines = {}
    for name in ("plain", "unrolled"):
        e = tfhe.Engine(tfhe.preset_params("secure128_torus"))
        if name == "unrolled":
            e.set_bsk_unroll(2)
        e.keygen(0x5EED)
        engines[name] = e
        say(f"  {name}: bootstrap key at {e.bsk_precision} bits, {e.key_bytes()[0] / 2 ** 20:.0f} MiB of bootstrap-key copies on the device")

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(5)
    table = rng.integers(-8, 8, 16)
    msgs = rng.integers(-8, 8, 256)
    state = {}
    for name, e in engines.items():
        dl = e.delta_log()
        lid = e.lut_register(table, 4, dl)
        small = e.keyswitch_host(e.encrypt(msgs, dl))
        d_small = torch.from_numpy(small.view(np.int64)).to(dev)
        d_ids = torch.full((256,), lid, dtype=torch.int32, device=dev)
        d_out = torch.empty((256, e.P.N + 1), dtype=torch.int64, device=dev)
        e.blind_rotate(d_small, d_ids, 256, d_out, stream)      # first launch
        torch.cuda.synchronize()
        ok = list(e.decrypt(d_out.cpu().numpy().view(np.uint64), dl)) == [int(table[m + 8]) for m in msgs]
        say(f"  {name}: 256 blind rotations decrypt to the table's values: {ok}")
        if not ok:
            raise SystemExit("a blind rotation decrypts wrong")
        state[name] = (d_small, d_ids, d_out)

    ms = {(name, cnt): [] for name in engines for cnt in (1, 256)}
    for rep in range(args.reps):
        for cnt in (1, 256):
            for name, e in engines.items():
                d_small, d_ids, d_out = state[name]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.calls):
                    e.blind_rotate(d_small, d_ids, cnt, d_out, stream)
                b.record()
                torch.cuda.synchronize()
                ms[(name, cnt)].append(a.elapsed_time(b) / args.calls)
                say(f"  blind_rotate x {cnt:3}  {name:8}  pass {rep + 1}: {ms[(name, cnt)][-1]:7.3f} ms")
    med = {}
    for (name, cnt), t in ms.items():
        med[(name, cnt)] = sorted(t)[len(t) // 2]
        say(f"blind_rotate x {cnt}, {name}: min / median / max {min(t):.3f} / {med[(name, cnt)]:.3f} / {max(t):.3f} ms (spread {max(t) - min(t):.3f})")
    for cnt in (1, 256):
        spread = max(max(ms[(n_, cnt)]) - min(ms[(n_, cnt)]) for n_ in engines)
        diff = med[("plain", cnt)] - med[("unrolled", cnt)]
        say(f"blind_rotate x {cnt}: unrolled / plain median {med[('unrolled', cnt)] / med[('plain', cnt)]:.3f}; plain - unrolled "
            f"{diff:+.3f} ms against an alternation spread of {spread:.3f} ms: "
            f"{'shorter by more than the spread' if diff > spread else 'longer by more than the spread' if -diff > spread else 'inside the spread'}")

    with open(os.path.join(REPO, "tests", "golden", "inverse.json")) as f:
        c = next(x for x in json.load(f) if x["tag"] == "baseline_n3_len30_ints12")
    emis = {name: EncryptedMatrixInversion(c["n"], None, 2, c["len"], c["ints"], False, False, engine=e, unroll=name == "unrolled")
            for name, e in engines.items()}
    M = np.array(c["M"]).reshape(c["n"], c["n"])
    encs, walls = {}, {name: [] for name in engines}
    for name, emi in emis.items():
        q, s = emi.quantize(M)
        encs[name] = emi.encrypt(q, s)
        emi._executor()
        emi.evaluate(encs[name])      # warm-up
    for rep in range(args.inverse_reps):
        for name, emi in emis.items():
            t0 = time.time()
            res = emi.evaluate(encs[name])
            walls[name].append(time.time() - t0)
            ok = emi.decrypt(res).tolist() == c["out"]
            say(f"  golden 3x3 inverse  {name:8}  run {rep + 1}: {walls[name][-1]:7.3f} s  matches the reference's digits: {ok}")
            if not ok:
                raise SystemExit("a decrypted inverse differs from the golden digits")
    wm = {name: sorted(t)[len(t) // 2] for name, t in walls.items()}
    depth = emis["plain"].circuit.summary()["depth"]
    for name, t in walls.items():
        say(f"golden 3x3 inverse ({depth} levels), {name}: min / median / max {min(t):.3f} / {wm[name]:.3f} / {max(t):.3f} s; "
            f"p_fail {emis[name].error_budget['p_fail']:.1e}")
    say(f"golden 3x3 inverse: unrolled / plain median {wm['unrolled'] / wm['plain']:.3f}")
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
