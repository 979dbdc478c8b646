#!/usr/bin/env python3
"""What the seeded key / ciphertext forms save and cost (record: profiles/seeded_keys_ab.txt, EXPERIMENTS A30).  ONE process:
  (a) sizes of the full and the seeded evaluation-key file (Engine.save_keys, uncompressed .npz) for the three torus sets and the
      two unrolled keys, CSPRNG keys;
  (b) wall-clock of Engine.load_keys on a fresh evaluation-only engine, seeded and full file of the same key alternating `rounds`
      times (file read + upload / expansion + key conversions; the files sit in the page cache after the first read), and of
      import_keys_seeded / import_keys alone on arrays already in memory;
  (c) k_place_bodies + k_chacha_expand between two events through Engine.expand_seeded (device form): 8,192 ciphertexts of the default
      set, and 3,780 rows of 1,024 words - the mask words of the default bootstrap key.
Nothing is asserted beyond the keys' equality: the figures are recorded as measured.
usage: seeded_keys_ab.py [--rounds 3] [--reps 20] [--sets default,secure128_torus,...] [--out FILE]"""
import os, statistics, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "bounty-matrix-inversion_amd"))
import numpy as np, torch
from bmi_amd import tfhe

SETS = {"default": (lambda: tfhe.default_params(), False), "secure128_torus": (lambda: tfhe.preset_params("secure128_torus"), False),
        "secure128_torus_wide": (lambda: tfhe.preset_params("secure128_torus_wide"), False),
        "default_unrolled": (lambda: tfhe.default_params(), True), "secure128_torus_unrolled": (lambda: tfhe.preset_params("secure128_torus"), True)}


def option(args, name, default):
    if name in args:
        i = args.index(name)
        v = args[i + 1]
        del args[i:i + 2]
        return v
    return default


def engine(name):
    params, unroll = SETS[name]
    e = tfhe.Engine(params())
    if unroll:
        e.set_bsk_unroll(2)
    return e


def main():
    args = sys.argv[1:]
    rounds, reps = int(option(args, "--rounds", 3)), int(option(args, "--reps", 20))
    names = option(args, "--sets", ",".join(SETS)).split(",")
    out = option(args, "--out", None)
    lines = []

    if out:
        open(out, "w").close()

    def say(s):      # (written line by line: a run cut short keeps what it measured)
        lines.append(s)
        print(s, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(s + "\n")

    with tempfile.TemporaryDirectory() as tmp:
        for name in names:
            client = engine(name)
            t0 = time.time()
            client.keygen()
            t_gen = time.time() - t0
            full, seeded = os.path.join(tmp, name + "_full.npz"), os.path.join(tmp, name + "_seeded.npz")
            client.save_keys(full, secret=False)
            client.save_keys(seeded, secret=False, seeded=True)
            sf, ss = os.path.getsize(full), os.path.getsize(seeded)
            say(f"(a) {name:26} key file: full {sf:>11,} B   seeded {ss:>11,} B   ratio {ss / sf:.4f}   (keygen {t_gen:.2f} s)")
            fp = client.eval_key_fingerprint()
            walls = {"seeded": [], "full": []}
            for r in range(rounds):
                for kind, path in (("seeded", seeded), ("full", full)):
                    server = engine(name) if kind == "full" else tfhe.Engine(SETS[name][0]())   # (the seeded file selects the mode itself)
                    t0 = time.time()
                    server.load_keys(path)
                    server.sync()
                    walls[kind].append(time.time() - t0)
                    if r == 0:
                        assert server.eval_key_fingerprint() == fp, (name, kind)
                    server.close()
            say(f"(b) {name:26} load_keys  seeded: " + " ".join(f"{x:.3f}" for x in walls["seeded"]) + "   full: " +
                " ".join(f"{x:.3f}" for x in walls["full"]) + f"   s; medians {statistics.median(walls['seeded']):.3f} / {statistics.median(walls['full']):.3f}")
            if not SETS[name][1]:
                pub, bsk_body, ksk_body = client.export_keys_seeded()
                _, _, bsk, ksk = client.export_keys(secret=False)
                imports = {"seeded": [], "full": []}
                for r in range(rounds):
                    for kind in ("seeded", "full"):
                        server = engine(name)
                        t0 = time.time()
                        if kind == "seeded":
                            server.import_keys_seeded(pub, bsk_body, ksk_body)
                        else:
                            server.import_keys(None, None, bsk, ksk)
                        server.sync()
                        imports[kind].append(time.time() - t0)
                        server.close()
                say(f"(b) {name:26} import     seeded: " + " ".join(f"{x:.3f}" for x in imports["seeded"]) + "   full: " +
                    " ".join(f"{x:.3f}" for x in imports["full"]) + f"   s; medians {statistics.median(imports['seeded']):.3f} / {statistics.median(imports['full']):.3f}")
            if name == "default":
                dev = torch.device("cuda", client.device)
                with torch.cuda.device(dev):
                    s = torch.cuda.current_stream().cuda_stream
                    for count, what in ((8192, "8,192 ciphertexts"), (3780, "3,780 rows of 1,024 words (the default bootstrap key's masks)")):
                        d_bodies = torch.zeros(count, dtype=torch.int64, device=dev)
                        d_out = torch.zeros((count, client.P.big), dtype=torch.int64, device=dev)
                        sc = tfhe.SeededCiphertexts(0, d_bodies)
                        client.expand_seeded(sc, d_out, s)
                        torch.cuda.synchronize()
                        samples = []
                        for _ in range(3):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(reps):
                                client.expand_seeded(sc, d_out, s)
                            e1.record()
                            torch.cuda.synchronize()
                            samples.append(e0.elapsed_time(e1) / reps)
                        mb = count * client.P.big * 8 / 1e6
                        say(f"(c) expansion of {what}: " + " ".join(f"{x:.4f}" for x in samples) +
                            f"   ms per call by events ({mb:.1f} MB written: {mb / 1e3 / (min(samples) / 1e3):.0f} GB/s at the fastest)")
            client.close()


if __name__ == "__main__":
    main()
