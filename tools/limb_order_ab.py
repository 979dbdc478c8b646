#!/usr/bin/env python3
"""A/B of the torus throughput kernel (k_blind_rotate_t64f) between builds of the library (record: profiles/limb_order_ab.txt).
ONE process, one engine per library (the same seeded keys), the libraries alternating `rounds` times (A B C A B C ...):
  time    the blind rotation of `batch` resident ciphertexts (kernel variant 5) between two events, one launch per sample after one
          warm launch per library and `warm` untimed alternations (the first timed launches of a call run up to 1 ms faster than the steady state); min / median / max per library; the outputs of every library must equal the first one's.
          Rule against the first library (the parent): median lower by at least 3 x the parent's spread (max - min) of this
          call AND the slowest sample below the parent's fastest.
  record  (--record FILE, first library only) the rounding distances of tests/test_gpu_t64f_limb_order.py::margin_inputs at every
          (levels, n, batch) of that test, as float.hex(): the golden file of the test when the first library is the parent's.
usage: limb_order_ab.py [--rounds 7] [--warm 3] [--batch 8192] [--levels 3] [--record FILE] NAME=path/to/lib.so [NAME=path ...]"""
import json, os, statistics, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "bounty-matrix-inversion_amd")); sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np, torch
from bmi_amd import tfhe


def option(args, name, default):
    if name in args:
        i = args.index(name)
        v = args[i + 1]
        del args[i:i + 2]
        return v
    return default


def engine_on(path, **kw):
    """an engine bound to the library at `path` (the module keeps one library at a time: engines keep their own)"""
    tfhe._lib, tfhe.LIB_PATH = None, os.path.abspath(path)
    e = tfhe.Engine(tfhe.default_params(q_bits=65, **kw))
    e.keygen(0x5EED)
    return e


def record(path, out):
    import test_gpu_t64f_limb_order as t
    res = {}
    for levels in t.LEVELS:
        for n in t.STEPS:
            e = engine_on(path, bs_levels=levels, n=n)
            for count in t.COUNTS:
                small, ids = t.margin_inputs(e, count)
                e.set_kernel_variant(5)
                res[t.margin_key(levels, n, count)] = e.fft_margin_host(small, ids)[1].hex()
            e.close()
    with open(out, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
    print(f"recorded {len(res)} rounding distances from {path} -> {out}: {sorted(set(res.values()))}")


def main():
    args = sys.argv[1:]
    rounds, B, levels = int(option(args, "--rounds", 7)), int(option(args, "--batch", 8192)), int(option(args, "--levels", 3))
    rec, warm = option(args, "--record", None), int(option(args, "--warm", 3))
    libs = [a.split("=", 1) for a in args]
    if rec:
        record(libs[0][1], rec)
        return
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    engines, bufs = {}, {}
    for name, path in libs:
        e = engines[name] = engine_on(path, bs_levels=levels)
        e.set_kernel_variant(5)
        dl = e.delta_log()
        lid = e.lut_register(np.arange(-8, 8), 4, dl)
        if not bufs:
            small = e.keyswitch_host(e.encrypt(np.random.default_rng(1).integers(-8, 8, B), dl))
            d_small = torch.from_numpy(small.view(np.int64)).to(dev)
        bufs[name] = (torch.full((B,), lid, dtype=torch.int32, device=dev), torch.empty((B, e.P.N + 1), dtype=torch.int64, device=dev))
        e.blind_rotate(d_small, bufs[name][0], B, bufs[name][1], s)
        torch.cuda.synchronize()
    first = libs[0][0]
    same = {name: bool(torch.equal(bufs[name][1], bufs[first][1])) for name, _ in libs}
    ms = {name: [] for name, _ in libs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(-warm, rounds):   # (r < 0: untimed alternations, every engine exists by then)
        for name, _ in libs:
            e0.record()
            engines[name].blind_rotate(d_small, bufs[name][0], B, bufs[name][1], s)
            e1.record(); torch.cuda.synchronize()
            if r >= 0:
                ms[name].append(e0.elapsed_time(e1))
    p = ms[first]
    spread = max(p) - min(p)
    print(f"blind rotation of {B} ciphertexts, l = {levels}, variant 5, {rounds} alternations after {warm} untimed ones; ms per launch")
    for name, _ in libs:
        v = ms[name]
        line = f"  {name:10s} min {min(v):7.3f}  median {statistics.median(v):7.3f}  max {max(v):7.3f}   outputs equal to {first}'s: {same[name]}"
        if name != first:
            gain = statistics.median(p) - statistics.median(v)
            ok = gain >= 3 * spread and max(v) < min(p)
            line += f"   median gain {gain:+.3f} ms ({100 * gain / statistics.median(p):+.2f} %) against 3 x spread {3 * spread:.3f}; slowest below {first}'s fastest: {max(v) < min(p)} -> {'PASSES' if ok else 'misses'} the rule"
        print(line)
        print(f"  {'':10s} samples " + " ".join(f"{x:.3f}" for x in v))
    for e in engines.values():
        e.close()


main()
