#!/usr/bin/env python3
"""Cost of decompressing compressed ciphertexts back to LWE ciphertexts (bmi_decompress_batch, csrc/lwe_unpack.hip; record:
profiles/decompress_ab.txt).  ONE process, one context per ring size (no keys: decompression takes none):
  (a) Engine.decompress of one full block (N ciphertexts, and of 16 blocks) on device buffers between two events, alternating with
      a device-to-device copy of the same rows x (N + 1) x 8 output bytes: one warm call, then `reps` calls per sample - reps chosen so
      that a sample fills about 0.2 s - and `rounds` samples of each, taken in turn (kernel, copy, kernel, copy ...).  The copy is the
      yardstick: it reads what it writes, the kernel reads a few KB per block.  Beside each time the bytes per second computed from the
      shapes (the output bytes; for the copy read + written), and the host time spent issuing one call: where that is the event
      time, the sample measured the host's call rate and not the GPU.
  (b) the bytes that go to the device for the inputs of the 2x2 and the 3x3 inverse, full against compressed (computed, not timed).
No threshold is attached: the lines say whether the kernel's median lies at or below the copy's, within the spread of the copy's samples.
usage: decompress_ab.py [--rounds 5] [--out FILE]"""
import os, statistics, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "bounty-matrix-inversion_amd"))
import numpy as np, torch
from bmi_amd import tfhe

PRESETS = ("north_star_torus64", "secure128_torus", "secure128_torus_wide")
LOG_MODULUS = 16


def option(args, name, default):
    if name in args:
        i = args.index(name)
        v = args[i + 1]
        del args[i:i + 2]
        return v
    return default


HOST = {}       # name -> host seconds per call spent ISSUING the last sample's calls (before any synchronisation)


def events(call, reps, name=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(reps): call()
    HOST[name] = (time.perf_counter() - t0) / reps
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    args = sys.argv[1:]
    rounds = int(option(args, "--rounds", 5))
    out = option(args, "--out", None)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    for preset in PRESETS:
        eng = tfhe.Engine(tfhe.preset_params(preset, n=16))
        N = eng.P.N
        for blocks in (1, 16):
            count = blocks * N
            words = np.random.default_rng(N + blocks).integers(0, 1 << LOG_MODULUS, tfhe.compressed_words(count, N), dtype=np.uint64)
            d_words = torch.from_numpy(words.astype(np.uint32).view(np.int32)).to(dev)
            d_out = torch.empty((count, N + 1), dtype=torch.int64, device=dev)
            d_src = torch.randint(0, 1 << 62, (count, N + 1), dtype=torch.int64, device=dev)
            d_dst = torch.empty_like(d_src)
            calls = {"kernel": lambda: eng.decompress(d_words, count, LOG_MODULUS, d_out, stream=s), "copy": lambda: d_dst.copy_(d_src)}
            reps = {}
            for k, call in calls.items():
                call(); torch.cuda.synchronize()
                reps[k] = max(20, int(200.0 / max(events(call, 20), 1e-4)))
            t, host = {"kernel": [], "copy": []}, {"kernel": [], "copy": []}
            for _ in range(rounds):
                for k, call in calls.items():
                    t[k].append(events(call, reps[k], k))
                    host[k].append(HOST[k])
            out_bytes = count * (N + 1) * 8
            med = {k: statistics.median(v) for k, v in t.items()}
            lo, hi = min(t["copy"]), max(t["copy"])
            verdict = "AT OR BELOW the copy's median" if med["kernel"] <= med["copy"] else \
                ("above the copy's median, INSIDE its spread" if med["kernel"] <= hi else "ABOVE the copy's spread")
            say(f"{preset}: N = {N}, {blocks:2} block(s) = {count} ciphertexts to {out_bytes} output bytes, {LOG_MODULUS} bits")
            say(f"    bmi_decompress_batch ({reps['kernel']} calls per sample): " + " ".join(f"{1e3 * x:.2f}" for x in t["kernel"]) +
                f" us; median {1e3 * med['kernel']:.2f} us = {out_bytes / med['kernel'] / 1e9:.3f} TB/s written")
            say(f"    device-to-device copy ({reps['copy']} calls per sample):  " + " ".join(f"{1e3 * x:.2f}" for x in t["copy"]) +
                f" us; median {1e3 * med['copy']:.2f} us = {2 * out_bytes / med['copy'] / 1e9:.3f} TB/s read + written; spread "
                f"{1e3 * lo:.2f} .. {1e3 * hi:.2f}")
            say(f"    kernel / copy = {med['kernel'] / med['copy']:.3f}: the kernel is {verdict}")
            # a sample whose calls take the host as long to issue as the events say they took to run was paced by the host: the queue
            # never held more than the call being issued, and the event time is the host's call rate, not the kernel's duration
            hk, hc = 1e3 * statistics.median(host["kernel"]), 1e3 * statistics.median(host["copy"])
            paced = [k for k, h in (("kernel", hk), ("copy", hc)) if h >= 0.9 * med[k]]
            say(f"    host time to issue one call: kernel {1e3 * hk:.2f} us, copy {1e3 * hc:.2f} us" +
                (f"; PACED BY THE HOST (issue time >= 0.9 of the event time): {', '.join(paced)}" if paced else "; neither is paced by the host"))
        eng.close()
    N = 1024
    for label, n_in in (("2x2 inverse (len 20, ints 8)", 4 * 21), ("3x3 inverse (len 30, ints 12)", 9 * 31)):
        full = n_in * (N + 1) * 8
        packed = tfhe.compressed_words(n_in, N)
        say(f"(b) {label}: {n_in} inputs at N = {N}: {full} bytes to the device as full ciphertexts, {4 * packed} as compressed values "
            f"(uint32 each; {16 + 2 * packed} on the wire at 16 bits): {full / (4 * packed):.0f} x fewer")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


main()
