#!/usr/bin/env python3
"""Cost of compressing output ciphertexts (bmi_compress_batch, csrc/lwe_pack.hip; record: profiles/compress_outputs_ab.txt).  ONE
process, one engine per parameter set:
  (a) Engine.compress on device buffers between two events - 279, 1,024 and 3,136 ciphertexts on the default set, 1,024 on
      secure128_torus - one warm call, then the mean of `reps` calls per sample, `rounds` samples; beside it, in the same process,
      one round of 256 bootstraps (bmi_pbs_batch), and the bytes that go home per form;
  (b) the wall-clock of one evaluation of the encrypted 3x3 inverse (len 30, ints 12) on the default set by Executor.run against
      Executor.run_compressed, alternating `rounds` times each (run, run_compressed, run, ...), both decrypted against the golden
      digits of tests/golden/inverse.json.
No threshold is attached: the lines say whether a full block costs less than a round of 256 bootstraps and whether the
run_compressed samples lie inside the spread of the run samples.
usage: compress_ab.py [--rounds 3] [--reps 10] [--out FILE]"""
import json, os, statistics, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "bounty-matrix-inversion_amd"))
import numpy as np, torch
from bmi_amd import error_budget, tfhe
from bmi_amd.main import EncryptedMatrixInversion

COUNTS = {"north_star_torus64": (279, 1024, 3136), "secure128_torus": (1024,)}
LOG_MODULUS = 16


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


def main():
    args = sys.argv[1:]
    rounds, reps = int(option(args, "--rounds", 3)), int(option(args, "--reps", 10))
    out = option(args, "--out", None)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    with open(os.path.join(REPO, "tests", "golden", "inverse.json")) as f:
        golden = next(x for x in json.load(f) if x["tag"] == "baseline_n3_len30_ints12")
    M = np.array(golden["M"]).reshape(3, 3)
    for preset, counts in COUNTS.items():
        eng = tfhe.Engine(tfhe.preset_params(preset))
        eng.keygen(0x5EED)
        t0 = time.perf_counter()
        eng.compression_keygen()
        levels, base_log, key_bytes = eng.compression_key_info()
        say(f"{preset}: N = {eng.P.N}, compression key ({levels}, 2^{base_log}) generated in {time.perf_counter() - t0:.2f} s, "
            f"{key_bytes / 1e6:.1f} MB on the device")
        dl = eng.delta_log()
        # one round of 256 bootstraps in the same process
        lid = eng.lut_register(np.random.default_rng(9).integers(-8, 8, 16), 4, dl)
        eng.reserve(256)
        d256 = torch.from_numpy(eng.encrypt(np.random.default_rng(1).integers(-8, 8, 256), dl).view(np.int64)).to(dev)
        d_ids = torch.full((256,), lid, dtype=torch.int32, device=dev)
        d_pbs = torch.empty_like(d256)
        pbs = [events(lambda: eng.pbs(d256, d_ids, 256, d_pbs, s), reps) for _ in range(rounds)]
        say(f"(a) bmi_pbs_batch, 256 ciphertexts, {eng.rotation_kernel(256)}: " + " ".join(f"{x:.4f}" for x in pbs) + " ms")
        for count in counts:
            msgs = np.random.default_rng(count).integers(-8, 8, count)
            d_in = torch.from_numpy(eng.encrypt(msgs, dl).view(np.int64)).to(dev)
            words = eng.compressed_words(count)
            d_out = torch.empty(words, dtype=torch.int32, device=dev)
            t = [events(lambda: eng.compress(d_in, count, d_out, LOG_MODULUS, s), reps) for _ in range(rounds)]
            packed = tfhe.CompressedCiphertexts(count, eng.P.N, LOG_MODULUS, d_out.cpu().numpy().view(np.uint32))
            right = eng.decrypt_compressed(packed, dl).tolist() == msgs.tolist()
            full = count * eng.P.big * 8
            med = statistics.median(t)
            say(f"(a) bmi_compress_batch, {count:5} ciphertexts to {LOG_MODULUS} bits: " + " ".join(f"{x:.4f}" for x in t) +
                f" ms (median {med / count * 1e3:.2f} us per ciphertext; {med / statistics.median(pbs):.2f} of a round of 256 bootstraps); "
                f"bytes home {full} full -> {packed.nbytes} compressed ({full / packed.nbytes:.0f} x); decrypts right: {right}")
        if preset == "north_star_torus64":
            d_in = torch.from_numpy(eng.encrypt(np.zeros(1024, np.int64), dl).view(np.int64)).to(dev)
            d_out = torch.empty(eng.compressed_words(1024), dtype=torch.int32, device=dev)
            med_block = statistics.median(events(lambda: eng.compress(d_in, 1024, d_out, LOG_MODULUS, s), reps) for _ in range(rounds))
            full_block = med_block < statistics.median(pbs)
            say(f"    a full block ({med_block:.4f} ms) costs {'LESS' if full_block else 'MORE'} than one round of 256 bootstraps "
                f"({statistics.median(pbs):.4f} ms) timed in this process")
            # (b) the 3x3 inverse: run against run_compressed
            emi = EncryptedMatrixInversion(3, None, 2, 30, 12, False, False, engine=eng)
            enc = emi.encrypt(*emi.quantize(M))
            ex = emi._executor()
            ex.run(enc); ex.run_compressed(enc, LOG_MODULUS)
            samples, right = {0: [], 1: []}, True
            for r in range(2 * rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = ex.run_compressed(enc, LOG_MODULUS) if r % 2 else ex.run(enc)
                samples[r % 2].append(time.perf_counter() - t0)
                right = right and emi.decrypt(res).tolist() == golden["out"]
            lo, hi = min(samples[0]), max(samples[0])
            inside = all(lo <= x <= hi for x in samples[1])
            cost = statistics.median(samples[1]) - statistics.median(samples[0])
            say("(b) 3x3 inverse, run: " + " ".join(f"{x:.4f}" for x in samples[0]) + "   run_compressed: " +
                " ".join(f"{x:.4f}" for x in samples[1]) + f"   s; run spread {lo:.4f} .. {hi:.4f}: run_compressed "
                f"{'INSIDE' if inside else 'OUTSIDE'}, median cost {cost * 1e3:+.2f} ms ({100 * cost / statistics.median(samples[0]):+.2f} %)")
            n_out = emi.program.n_outputs
            b0 = error_budget.engine_failure_probability(emi.program, eng)
            b1 = error_budget.engine_failure_probability(emi.program, eng, compressed_outputs=(levels, base_log, LOG_MODULUS))
            v = error_budget.compression_variance(eng.P, levels, base_log, LOG_MODULUS, n_out)
            say(f"    golden digits in every run: {right}; {n_out} outputs: {n_out * eng.P.big * 8} bytes home by run, "
                f"{res.nbytes} by run_compressed; compression_variance {v:.3e} (std 2^{0.5 * np.log2(v):.2f}); output margin "
                f"{b0['output_margin_sigma']:.1f} -> {b1['output_margin_sigma']:.1f} sigma, p_fail {b0['p_fail']:.2e} -> {b1['p_fail']:.2e}")
        eng.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


main()
