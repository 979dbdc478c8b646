#!/usr/bin/env python3
"""Timing rule of the exact-transform latency kernels' shared steps (csrc/exact_half_steps.hpp; record: profiles/exact_steps_ab.txt).
Three builds of the library are loaded into ONE process: the parent's under two file names (P1, P2: a copy of the same file) and
the branch's (B).  Per kernel an engine on each, the same seeded keys and inputs; per batch (1 and 256: the batches these kernels
serve) `rounds` rounds in which the three rotate through the positions of a round.  A sample is the one of tools/preset_timing.py:
one warm call, then the mean of five blind rotations between two events.  Per kernel and batch the margin is
|median(P1) - median(P2)| - what the procedure cannot resolve, measured in the same call - and the branch passes if
median(B) <= max(median(P1), median(P2)) + margin.  The three engines' outputs are compared word for word as well.
With the label host_forms the rule times the host-buffer forms instead (record: profiles/host_forms_ab.txt): on the default torus
set pbs_host at 5 and 600 ciphertexts, keyswitch_host at 600, compress_host and decompress_host at 1,024; a sample is one warm call,
then the mean of five calls on the host's clock (each form ends in a stream synchronise).
usage: exact_steps_ab.py <parent .so> <copy of the parent .so> <branch .so> [rounds = 3] [kernel labels, comma separated | host_forms]"""
import os, statistics, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "bounty-matrix-inversion_amd"))
import numpy as np, torch
from bmi_amd import tfhe

# label: (parameter set, key precision or None, unroll, kernel variant pinned, the kernel the dispatch must answer with)
CONFIGS = {
    "lat2_49": (lambda: tfhe.default_params(q_bits=49), None, 1, 2, "k_blind_rotate_lat2_49"),
    "lat2u_49": (lambda: tfhe.default_params(q_bits=49), None, 2, 0, "k_blind_rotate_lat2u_49"),
    "lat_t64": (lambda: tfhe.default_params(q_bits=tfhe.TORUS64), None, 1, 4, "k_blind_rotate_lat_t64"),
    "lat2u_t64": (lambda: tfhe.default_params(q_bits=tfhe.TORUS64), 48, 2, 0, "k_blind_rotate_lat2u_t64"),
    "wide49": (lambda: tfhe.preset_params("secure128"), None, 1, 0, "k_blind_rotate_wide49"),
    "wide49u": (lambda: tfhe.preset_params("secure128"), None, 2, 0, "k_blind_rotate_wide49u"),
    # the default torus set under auto dispatch: what a change to the host's launch path costs per call (profiles/launch_rows_ab.txt)
    "default_t64": (lambda: tfhe.default_params(q_bits=tfhe.TORUS64), None, 1, 0, "k_blind_rotate_lat_t64f"),
}
BATCHES = (1, 256)


def engine_on(lib_path, params, precision, unroll, variant):
    tfhe._lib, tfhe.LIB_PATH = None, lib_path      # the next Engine binds to this build
    eng = tfhe.Engine(params())
    if precision:
        eng.set_bsk_precision(precision)
    if unroll == 2:
        eng.set_bsk_unroll(2)
    eng.keygen(0x5EED)
    eng.set_kernel_variant(variant)
    return eng


def verdict(ms, unit):
    """(the medians, margin and verdict of one case as text, whether the branch passes)"""
    med = {k: statistics.median(v) for k, v in ms.items()}
    margin = abs(med["P1"] - med["P2"])
    passes = med["B"] <= max(med["P1"], med["P2"]) + margin
    return (f"medians {med['P1']:.4f} {med['P2']:.4f} {med['B']:.4f} {unit}  margin {margin:.4f}  {'passes' if passes else 'MISSES'}", passes)


def host_forms(libs, rounds):
    """the host-buffer forms on the default torus set; returns the number of cases outside the margin"""
    engs = {k: engine_on(p, lambda: tfhe.default_params(q_bits=tfhe.TORUS64), None, 1, 0) for k, p in libs.items()}
    e0 = engs["P1"]
    DL = e0.delta_log()
    table = np.random.default_rng(9).integers(-8, 8, 16)
    lids = {k: e.lut_register(table, 4, DL) for k, e in engs.items()}
    for e in engs.values():
        e.compression_keygen()
    ct = {B: e0.encrypt(np.random.default_rng(B).integers(-8, 8, B), DL) for B in (5, 600, 1024)}
    cc = e0.compress_host(ct[1024])
    words = lambda r: r.words if hasattr(r, "words") else r
    cases = [("pbs_host", 5, lambda k: engs[k].pbs_host(ct[5], np.full(5, lids[k], np.uint32))),
             ("pbs_host", 600, lambda k: engs[k].pbs_host(ct[600], np.full(600, lids[k], np.uint32))),
             ("keyswitch_host", 600, lambda k: engs[k].keyswitch_host(ct[600])),
             ("compress_host", 1024, lambda k: engs[k].compress_host(ct[1024])),
             ("decompress_host", 1024, lambda k: engs[k].decompress_host(cc))]
    misses = 0
    for name, B, call in cases:
        ms, outs = {k: [] for k in engs}, {}
        for r in range(rounds):
            order = list(engs)[r % 3:] + list(engs)[:r % 3]
            for k in order:
                outs[k] = words(call(k))
                t0 = time.perf_counter()
                for _ in range(5): call(k)
                ms[k].append((time.perf_counter() - t0) * 1e3 / 5)
        same = np.array_equal(outs["P1"], outs["B"]) and np.array_equal(outs["P1"], outs["P2"])
        text, passes = verdict(ms, "ms")
        misses += not passes
        print(f"{name:15} B = {B:4d}  " + "  ".join(f"{k} " + " ".join(f"{x:.3f}" for x in ms[k]) for k in ms) +
              f"  | {text}  same words {same}", flush=True)
    for e in engs.values():
        e.close()
    return misses


def main():
    libs = dict(zip(("P1", "P2", "B"), (os.path.abspath(p) for p in sys.argv[1:4])))
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    labels = sys.argv[5].split(",") if len(sys.argv) > 5 else list(CONFIGS)
    if labels == ["host_forms"]:
        print(f"{host_forms(libs, rounds)} (form, batch) outside the margin")
        return
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    misses = 0
    for label in labels:
        params, precision, unroll, variant, kernel = CONFIGS[label]
        engs = {k: engine_on(p, params, precision, unroll, variant) for k, p in libs.items()}
        e0 = engs["P1"]
        DL = e0.delta_log()
        table = np.random.default_rng(9).integers(-8, 8, 16)
        lids = {k: e.lut_register(table, 4, DL) for k, e in engs.items()}
        for B in BATCHES:
            assert all(e.rotation_kernel(B) == kernel for e in engs.values()), (label, B, [e.rotation_kernel(B) for e in engs.values()])
            msgs = np.random.default_rng(B).integers(-8, 8, B)
            small = e0.keyswitch_host(e0.encrypt(msgs, DL))
            d_small = torch.from_numpy(small.view(np.int64)).to(dev)
            d_ids = {k: torch.full((B,), lids[k], dtype=torch.int32, device=dev) for k in engs}
            d_out = torch.empty((B, e0.P.N + 1), dtype=torch.int64, device=dev)
            ms = {k: [] for k in engs}
            outs = {}
            for r in range(rounds):
                order = list(engs)[r % 3:] + list(engs)[:r % 3]
                for k in order:
                    eng = engs[k]
                    eng.blind_rotate(d_small, d_ids[k], B, d_out, s); torch.cuda.synchronize()
                    outs[k] = d_out.cpu().numpy().view(np.uint64).copy()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(5): eng.blind_rotate(d_small, d_ids[k], B, d_out, s)
                    t1.record(); torch.cuda.synchronize()
                    ms[k].append(t0.elapsed_time(t1) / 5)
            same = np.array_equal(outs["P1"], outs["B"]) and np.array_equal(outs["P1"], outs["P2"])
            ok = list(e0.decrypt(outs["B"], DL)) == [int(table[m + 8]) for m in msgs]
            text, passes = verdict(ms, "ms")
            misses += not passes
            print(f"{label:10} B = {B:3d}  " + "  ".join(f"{k} " + " ".join(f"{x:.3f}" for x in ms[k]) for k in ms) +
                  f"  | {text}  same words {same}  decrypts_to_lut {ok}", flush=True)
        for e in engs.values():
            e.close()
    print(f"{misses} (kernel, batch) outside the margin")


main()
