#!/usr/bin/env python3
"""A/B of the two unrolled blind-rotation kernels of secure128_torus (n 742, N 2048, key at 40 bits) in ONE process on ONE engine:
    kernel variant 2 = k_blind_rotate_wu_t64f   (one workgroup per ciphertext: the yardstick)
    kernel variant 1 = k_blind_rotate_wu2_t64f  (two ciphertexts per workgroup sharing every key word)
alternating `--reps` times each at every batch size, inputs resident on the device, every run timed by device events around `--iters`
launches (after a warm-up of both at that size); the words of the two are compared at every size.  Prints every run, the spread of the
alternation, PBS/s, and cycles per step (a pair of LWE coefficients) of a workgroup's two ciphertexts at the clock read from the
device.  Then the 3x3 inverse in its serving form (evaluate_many, 8 matrices per walk) both ways, against the plaintext circuit.
usage: unrolled_wide2_ab.py [--batches 512,1024,2048,8192] [--reps 4] [--iters 3] [--inverse-reps 2] [--out FILE]"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "bounty-matrix-inversion_amd"))

VARIANTS = ((2, "wu "), (1, "wu2"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="512,1024,2048,8192")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--inverse-reps", type=int, default=2, help="walks of the 3x3 inverse each way (0: none)")
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
    import torch
    from bmi_amd import tfhe
    from bmi_amd.inverse_bench import CONFIGS
    from bmi_amd.main import EncryptedMatrixInversion

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, it does not fall back")
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    cus = props.multi_processor_count
    mhz = getattr(props, "clock_rate", 2400000) / 1000.0      # the device's peak engine clock: cycles below are at that clock
    say(f"unrolled N = 2048 A/B (tools/unrolled_wide2_ab.py): secure128_torus, unrolled key at 40 bits, n 742, seeded keys; {props.name}, "
        f"{cus} CUs, {mhz:.0f} MHz; {args.iters} launches per run, ms per launch by device events")
    eng = tfhe.Engine(tfhe.preset_params("secure128_torus"))
    eng.set_bsk_unroll(2)
    eng.keygen(0x5EED)
    P = eng.P
    steps = (P.n + 1) // 2
    dl = eng.delta_log()
    rng = np.random.default_rng(7)
    table = rng.integers(-8, 8, 16)
    lid = eng.lut_register(table, 4, dl)
    batches = [int(b) for b in args.batches.split(",")]
    top = max(batches)
    msgs = rng.integers(-8, 8, top)
    small = np.concatenate([eng.keyswitch_host(eng.encrypt(msgs[i:i + 2048], dl)) for i in range(0, top, 2048)])
    d_small = torch.from_numpy(small.view(np.int64)).to(dev)
    d_ids = torch.full((top,), lid, dtype=torch.int32, device=dev)
    d_out = {v: torch.empty((top, P.N + 1), dtype=torch.int64, device=dev) for v, _ in VARIANTS}
    eng.reserve(top)
    s = torch.cuda.current_stream().cuda_stream
    wins = {}
    for B in batches:
        names = {}
        for v, _ in VARIANTS:      # warm-up of both at this size, and their words
            eng.set_kernel_variant(v)
            names[v] = eng.rotation_kernel(B)
            eng.blind_rotate(d_small, d_ids, B, d_out[v], s)
        torch.cuda.synchronize()
        same = bool(torch.equal(d_out[2][:B], d_out[1][:B]))
        ok = list(eng.decrypt(d_out[1][:min(B, 64)].cpu().numpy().view(np.uint64), dl)) == [int(table[m + 8]) for m in msgs[:min(B, 64)]]
        say(f"B = {B}: variant 2 -> {names[2]}, variant 1 -> {names[1]}; same words: {same}; first rows decrypt to the table: {ok}")
        if not (same and ok):
            raise SystemExit("the two kernels differ")
        t = {v: [] for v, _ in VARIANTS}
        for rep in range(args.reps):
            for v, tag in VARIANTS:
                eng.set_kernel_variant(v)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters):
                    eng.blind_rotate(d_small, d_ids, B, d_out[v], s)
                b.record()
                torch.cuda.synchronize()
                t[v].append(a.elapsed_time(b) / args.iters)
                say(f"  B = {B:5d}  {tag}  run {rep + 1}: {t[v][-1]:9.3f} ms")
        med = {v: sorted(x)[len(x) // 2] for v, x in t.items()}
        spread = max(max(x) - min(x) for x in t.values())
        for v, tag in VARIANTS:
            per_wg = 1 if v == 2 else 2
            workgroups = (B + per_wg - 1) // per_wg
            rounds = (workgroups + cus - 1) // cus      # one workgroup per compute unit at a time (LDS)
            cyc = med[v] * 1e-3 * mhz * 1e6 / (rounds * steps)
            say(f"B = {B}: {tag} min / median / max {min(t[v]):.3f} / {med[v]:.3f} / {max(t[v]):.3f} ms; {B / med[v]:.1f} k PBS/s; {rounds} rounds of "
                f"workgroups, {cyc / 1e3:.1f} k cycles per step of a workgroup ({per_wg} ciphertext{'s' if per_wg > 1 else ''})")
        wins[B] = med[2] - med[1] > spread
        say(f"B = {B}: wu2 / wu median {med[1] / med[2]:.3f}; difference {med[2] - med[1]:+.3f} ms against the alternation's spread {spread:.3f} ms: "
            f"{'wu2 wins' if wins[B] else 'no win beyond the spread'}")
    eng.set_kernel_variant(0)
    if args.inverse_reps > 0:
        n, batch = 3, 8
        ln, ints = CONFIGS[n]
        rng = np.random.default_rng(4321 + n)
        Ms = [rng.standard_normal((n, n)) * 100 for _ in range(batch)]
        emi = EncryptedMatrixInversion(n, None, 2, ln, ints, False, False, engine=eng, unroll=True)
        qs = [emi.quantize(M) for M in Ms]
        encs = [emi.encrypt(q, sg) for q, sg in qs]
        want = [emi.simulate(q, sg) for q, sg in qs]
        ex = emi._executor(batch)
        widths = sorted(w for w, *_ in ex.levels)
        say(f"3x3 inverse (len {ln}, ints {ints}), evaluate_many of {batch}: {len(widths)} levels, widths min / median / max "
            f"{widths[0]} / {widths[len(widths) // 2]} / {widths[-1]}, {sum(w > 256 for w in widths)} levels beyond 256")
        tt = {2: [], 0: []}
        emi.evaluate_many(encs)
        for rep in range(args.inverse_reps):
            for v, tag in ((2, "variant 2 (wu at every width)"), (0, "auto (wu2 beyond 256)")):
                eng.set_kernel_variant(v)
                t0 = time.time()
                res = emi.evaluate_many(encs)
                tt[v].append(time.time() - t0)
                good = all(np.array_equal(emi.decrypt(r), w) for r, w in zip(res, want))
                say(f"  3x3 x {batch}  {tag}  run {rep + 1}: {tt[v][-1]:8.3f} s  matches the plaintext circuit: {good}")
                if not good:
                    raise SystemExit("a decrypted inverse differs from the plaintext evaluation")
        eng.set_kernel_variant(0)
        say(f"3x3 x {batch}: auto / variant 2 (best run) {min(tt[0]) / min(tt[2]):.3f}")
    eng.close()


if __name__ == "__main__":
    main()
