#!/usr/bin/env python3
"""bench.py - PBS throughput of the MI355X-native TFHE engine (BASELINE.json metric "PBS/sec per GPU + encrypted n x n inverse
wall-clock").

`value` = whole-job PBS/s on the 2^64 TORUS (the ciphertext modulus Concrete, the reference's back end, computes on) at the
north-star set (n=630, N=1024, k=1, l=3).  One "step" = one pass of the hot path (keyswitch -> mod-switch -> blind rotation ->
sample extraction) over one batch of B synthetic ciphertexts per GPU, inputs already resident in HBM.  The batch shards over GPUs
with no data-path collective (independent ciphertexts; keys replicated) -> "scaling": "weak".

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Started without a launcher (`WORLD_SIZE` unset) and with --gpus N > 1, it starts the N ranks itself (a torch.distributed.run child
process, one rank per GPU, before this process touches a GPU) and exits with the child's code; it never prints a line for fewer
GPUs than were asked for.  Rank 0 prints ONE JSON line.

A plain run does only what the headline needs: set-up, W warm-up steps, K timed steps, the decrypt check of the timed outputs,
and a line with the contract's fields (`ms_per_step` = wall-clock of one timed step) and the run's configuration.
--dump-outputs DIR writes rank 0's outputs of the last timed step as float64 .npy files (see dump_outputs); the inputs are
seeded, so two builds given the same arguments can be compared output for output.  --full adds everything below:

* top level: the contract's fields, then the scalars to quote - inverse_{2x2,3x3,4x4}_s (headline engine, evaluate wall-clock),
  inverse_3x3_batched_{s_per_matrix, pbs_per_s} (16 matrices in one walk of the levels: the serving form, evaluate_many),
  secure128_torus_{pbs_per_s, latency_ms_1, latency_ms_256, inverse_*_s} (the 128-bit-secure set on q = 2^64), value_p49 /
  value_torus64_unrolled / inverse_3x3_s_{torus64_unrolled, p49_unrolled} (the other engines);
* `roofline`: the PHYSICAL bound of the dominant kernel (f64 vector issue: static instruction counts x live launch rate against
  1,024 SIMDs x the sampled shader clock), kernel_ms by events on the launch stream, kernel_cycles_per_cmux, `traffic` (HBM bytes
  per launch, profiled); the north star's HBM-read convention (bootstrap-key bytes per PBS, no reuse, vs 8 TB/s) is
  `roofline.north_star` / `roofline.north_star_frac`;
* `cpu_baseline`: the oracle's fast path (exact f64 arithmetic, OpenMP over the batch; bit-identical to the generic oracle and to
  the GPU, re-checked inside the run) on this box's host cores, on a bounded sample of the same ciphertexts (N=1, rank 0 only);
* legs (N=1, rank 0; objects `secure128_torus`, `secure128_torus_wide`, `p49_field`, `torus64_unrolled_key`, `unrolled_key_49`; `--goldilocks-leg` adds the
  Goldilocks kernels): PBS/s, kernel time, output noise against the CGGI formula, latency of 1 and 256, inverse wall-clocks.
The --no-* options, --goldilocks-leg and --inverse-sharded trim or extend what --full does.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
for p in (REPO, os.path.join(REPO, "bounty-matrix-inversion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

BSK_BYTES_PER_PBS = 630 * 4 * 3 * 1024 * 8  # 61,931,520 (SURVEY.md §8d / BASELINE.md §3)
MODMUL_PER_PBS = 33_546_240                # SURVEY.md §8d (radix-2 count, the reference figure)
HBM_PEAK_GBS = 8000.0                      # MI355X_MICROARCH.md: 8 TB/s spec


class SclkSampler:
    """Samples the shader clock from sysfs (pp_dpm_sclk: the line marked '*') while the timed kernels run; median of the samples.
    Falls back to the spec maximum (2,400 MHz) when the file cannot be read - the fraction printed is then a lower bound."""

    def __init__(self):
        import glob
        import threading
        self.files = sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"))
        self.samples, self._stop = [], threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)

    def _read(self):
        best = 0.0
        for f in self.files:
            try:
                for line in open(f).read().splitlines():
                    if line.rstrip().endswith("*"):
                        best = max(best, float(line.split(":")[1].lower().replace("mhz", "").replace("*", "").strip()))
            except Exception:
                pass
        return best

    def _run(self):
        while not self._stop.is_set():
            v = self._read()
            if v > 0:
                self.samples.append(v)
            self._stop.wait(0.01)

    def start(self):
        self._t.start()

    def stop(self):
        self._stop.set()
        self._t.join()

    def result(self):
        if self.samples:
            return float(np.median(self.samples)), (f"sysfs pp_dpm_sclk (the selected DPM level), median of {len(self.samples)} samples during the timed "
                                                    "steps; near the power limit the average clock is lower (rocm-smi: ~2.25 GHz under this "
                                                    "kernel), so the fraction is a lower bound - the PMC view is valu_busy_frac_profiled")
        return 2400.0, "spec maximum (pp_dpm_sclk not readable here): the fraction is a lower bound"


def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n_gpus, argv):
    """--gpus N > 1 without a launcher: run the same command under torch.distributed.run with N ranks (child process;
    this parent has made no GPU call).  Returns the child's exit code; a failed start is an error, never an N = 1 line."""
    import subprocess
    import torch
    share = os.environ.get("BMI_BENCH_SHARE_DEVICE") == "1" or os.environ.get("BMI_BENCH_REHEARSE") == "plumbing"
    have = torch.cuda.device_count()      # counts devices without initialising the GPU
    if not share and have < n_gpus:
        print(f"bench.py: --gpus {n_gpus} requested but {have} GPU(s) are visible", file=sys.stderr)
        return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def rehearse_plumbing(args, rank, world):
    """BMI_BENCH_REHEARSE=plumbing (tests only, never the driver): the rank start-up, rendezvous, barrier and MAX-over-ranks
    timing of an N-rank run on a box without GPUs (gloo).  No PBS is executed and the line says so: value is null."""
    import torch
    import torch.distributed as dist
    dist.init_process_group(backend="gloo")
    assert dist.get_world_size() == world == args.gpus
    dist.barrier()
    t = torch.tensor([1.0 + rank], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    # the ranks' parts of the whole-job batch, as main() cuts them (weak scaling: B * world ciphertexts, contiguous ranges)
    from bmi_amd.shard import shard_range
    ranges = [None] * world
    dist.all_gather_object(ranges, list(shard_range(args.batch * world, rank, world)))
    if rank == 0:
        print(json.dumps({"metric": "PBS/sec per GPU + encrypted n x n inverse wall-clock (n=2,3,4)", "value": None,
                          "unit": "PBS/s", "n_gpus": world, "world_size_seen": dist.get_world_size(), "steps": args.steps,
                          "warmup": args.warmup, "rehearsal": "plumbing only: no PBS executed, nothing measured",
                          "max_over_ranks_check": float(t.item()), "batch_per_gpu": args.batch, "shard_ranges": ranges}))
    dist.barrier()
    dist.destroy_process_group()


INV_COMPACT = ("evaluate_s", "ms_per_level", "pbs", "depth", "matches_plaintext_circuit", "sharded_levels", "ranks")


def compact(res):
    """the printed line: long explanatory strings and the per-stage timings of the inverse legs stay in bench_details.json"""
    def inv(d):
        if not isinstance(d, dict):
            return d
        return {k: ({f: v[f] for f in INV_COMPACT if f in v} if isinstance(v, dict) and "evaluate_s" in v else v) for k, v in d.items()}

    def leg(d):
        if not isinstance(d, dict):
            return d
        out = {k: v for k, v in d.items() if k not in ("key", "arithmetic", "reference_readme_64core_cpu_run_s")}
        if "encrypted_inverse_wall_clock" in out:
            out["encrypted_inverse_wall_clock"] = inv(out["encrypted_inverse_wall_clock"])
        if isinstance(out.get("alu"), dict):
            out["alu"] = {k: v for k, v in out["alu"].items() if k in ("bound", "frac", "achieved", "peak", "unit", "sclk_mhz")}
        return out

    r = dict(res)
    cfg = dict(res.get("config", {}))
    for k in list(cfg):
        if k.startswith("encrypted_inverse_wall_clock_") and k != "encrypted_inverse_wall_clock_sharded":
            del cfg[k]                       # copies of the legs' reports
    for k in ("encrypted_inverse_wall_clock", "encrypted_inverse_wall_clock_sharded"):
        if k in cfg:
            cfg[k] = inv(cfg[k])
    rb = cfg.get("reference_readme_benchmark")
    if isinstance(rb, dict) and "error" not in rb:
        cfg["reference_readme_benchmark"] = {k: {f: v.get(f) for f in ("encrypt_run_decrypt_s", "total_cold_s", "speedup_run", "speedup_total_cold",
                                                                      "matches_plaintext_circuit")} | {"reference_run_s": v["reference_readme"]["run_s"]}
                                             for k, v in rb.items()}
    cfg.pop("arithmetic", None)
    cfg.pop("keys", None)
    cfg.pop("multi_gpu_placement", None) if res.get("n_gpus", 1) == 1 else None
    r["config"] = cfg
    rl = dict(res.get("roofline", {}))
    if isinstance(rl.get("alu"), dict):
        rl["alu"] = {k: v for k, v in rl["alu"].items() if k not in ("sclk_source", "source", "valu_busy_source")}
    rl.pop("traffic_source", None)
    if isinstance(rl.get("north_star"), dict):
        rl["north_star"] = {k: v for k, v in rl["north_star"].items() if k != "convention"}
    r["roofline"] = rl
    cb = res.get("cpu_baseline")
    if isinstance(cb, dict):
        r["cpu_baseline"] = {k: v for k, v in cb.items() if k not in ("host", "concrete")}
    for k in ("secure128_torus", "secure128_torus_wide", "torus64", "p49_field", "torus64_unrolled_key", "unrolled_key_49", "roofline_q64_goldilocks"):
        if k in r:
            r[k] = leg(r[k])
    r["details"] = "gpurun_out/bench_details.json (every leg in full)"

    def sig(o, top=True):   # nested floats to 5 significant digits (the top-level scalars stay as measured)
        if isinstance(o, dict):
            return {k: (v if (top and isinstance(v, float)) else sig(v, False)) for k, v in o.items()}
        if isinstance(o, list):
            return [sig(v, False) for v in o]
        if isinstance(o, float) and o == o and abs(o) not in (0.0, float("inf")):
            return float(f"{o:.5g}")
        return o
    return sig(r)


DUMP_ROWS = 1024      # ciphertexts kept whole in the dump: 2 x 1,024 x 1,025 x 8 B = 16.8 MB at N = 1024, far below 64 MB


def dump_outputs(path, eng, out, dec):
    """What a caller of the timed path receives, as float64 (exact): `messages` (every output decrypted), `phase` (every
    output's phase as a signed fraction of the modulus: message plus noise) and a fixed sample of DUMP_ROWS whole output
    ciphertexts (rows drawn with seed 2024, ascending) split into `ciphertexts_sample_hi32` / `_lo32`, the high and low 32 bits
    of every word.  The full batch (B x (N + 1) words, 67 MB at the default) is larger than a dump should be."""
    os.makedirs(path, exist_ok=True)
    Qm = eng.modulus
    rows = np.sort(np.random.default_rng(2024).choice(out.shape[0], min(out.shape[0], DUMP_ROWS), replace=False))
    arrays = {"messages": dec.astype(np.float64),
              "phase": np.array([((int(x) + Qm // 2) % Qm - Qm // 2) / Qm for x in eng.phase(out)], dtype=np.float64),
              "ciphertexts_sample_hi32": (out[rows] >> np.uint64(32)).astype(np.float64),
              "ciphertexts_sample_lo32": (out[rows] & np.uint64(0xFFFFFFFF)).astype(np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(path, f"{name}.npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=int(os.environ.get("BMI_BENCH_BATCH", "8192")),
                    help="ciphertexts per GPU per step")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="target wall time of the CPU baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--q-bits", type=int, default=None, choices=[64, 49, 65],
                    help="ciphertext modulus of the headline: 65 = 2^64 exactly (Concrete's torus; exact limb products through an f64 "
                         "FFT; the default), 49 = 2^49-720895 (exact f64 transform mod p), 64 = 2^64-2^32+1 (integer kernels); "
                         "given explicitly, the extra legs on the other moduli are skipped")
    ap.add_argument("--no-inverse", action="store_true", help="skip the encrypted-inverse wall-clock leg")
    ap.add_argument("--no-readme-benchmark", action="store_true",
                    help="skip the reference's README benchmark configurations (2x2 / 3x3 low precision, ~20 s with cold compiles)")
    ap.add_argument("--no-second-field", action="store_true",
                    help="skip the extra legs (N=1, rank 0): the 128-bit-secure torus set, the 49-bit field, the unrolled keys")
    ap.add_argument("--goldilocks-leg", action="store_true",
                    help="also time the Goldilocks-field kernels (an independent implementation, 4x slower; never the product path)")
    ap.add_argument("--inverse-batch", type=int, default=16, help="matrices per batched 3x3 evaluation (EncryptedMatrixInversion.evaluate_many)")
    ap.add_argument("--no-secure-leg", action="store_true", help="skip the secure128_torus leg (n 742, N 2048 on q = 2^64)")
    ap.add_argument("--inverse-sizes", default=None, help="matrix sizes of the encrypted-inverse legs: default 2,3,4 at N=1 (BASELINE "
                    "configs 2, 3, 4 on rank 0; 8 takes ~2 min more) and 8 for --inverse-sharded (config 5: the one whose levels are wide "
                    "enough to split)")
    ap.add_argument("--inverse-sharded", action="store_true",
                    help="N > 1 only (opt-in): also run the encrypted-inverse leg with its wide levels split across the "
                         "ranks (executor.py; one RCCL all-gather per split level)")
    ap.add_argument("--shard-threshold", type=int, default=None,
                    help="narrowest level that is split across ranks (default: every level wider than one kernel round)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write rank 0's outputs of the last timed step to DIR/<name>.npy (float64)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: roofline, output noise, latencies, CPU baseline, "
                         "the other engines and parameter sets, encrypted-inverse wall-clocks, the complete report")
    args = ap.parse_args()
    sharded_sizes = args.inverse_sizes or "8"
    args.inverse_sizes = args.inverse_sizes or "2,3,4"
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    if (args.goldilocks_leg or args.inverse_sharded) and not args.full:
        raise SystemExit("--goldilocks-leg and --inverse-sharded are parts of --full")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a line for another GPU count")
    if os.environ.get("BMI_BENCH_REHEARSE") == "plumbing":
        return rehearse_plumbing(args, rank, world)

    import torch
    from bmi_amd import tfhe

    dist = None
    # Rehearsal knobs (not used by the driver): BMI_BENCH_SHARE_DEVICE=1 puts every rank on cuda:0 and
    # BMI_BENCH_BACKEND=gloo replaces RCCL, so that the N > 1 code path can be exercised on a one-GPU box.
    dev_index = 0 if os.environ.get("BMI_BENCH_SHARE_DEVICE") == "1" else local_rank
    backend = os.environ.get("BMI_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=backend)

    headline_q = tfhe.TORUS64 if args.q_bits is None else args.q_bits
    eng = tfhe.Engine(tfhe.default_params(q_bits=headline_q), device=dev_index)
    eng.keygen(0x5EED)  # keys replicated on every GPU (same seed)
    P = eng.P
    DL = eng.delta_log()
    B = args.batch
    from bmi_amd.shard import shard_range
    # the whole job's batch is B * world ciphertexts (weak scaling); rank r owns a contiguous range of it
    lo, hi = shard_range(B * world, rank, world)
    msgs = np.random.default_rng(1234).integers(-8, 8, B * world)[lo:hi]
    ident = eng.lut_register(np.arange(-8, 8), 4, DL)
    rnd_table = np.random.default_rng(99).integers(-8, 8, 16)
    rlut = eng.lut_register(rnd_table, 4, DL)
    ct = eng.encrypt(msgs, DL)
    lut_sel = (np.arange(B) & 1).astype(np.int32)
    d_in = torch.from_numpy(ct.view(np.int64)).to(dev)
    d_ids = torch.from_numpy(np.where(lut_sel == 0, ident, rlut).astype(np.int32)).to(dev)
    d_small = torch.empty((B, P.small), dtype=torch.int64, device=dev)
    d_out = torch.empty_like(d_in)
    stream = torch.cuda.current_stream().cuda_stream

    def step(events=None):
        eng.keyswitch(d_in, B, d_small, stream)
        if events is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        eng.blind_rotate(d_small, d_ids, B, d_out, stream)
        if events is not None:
            e1.record()
            events.append((e0, e1))

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    # --full: kernel time by events and the shader clock during the timed steps, for the roofline
    events = [] if args.full else None
    clock = SclkSampler() if args.full else None
    if clock:
        clock.start()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(events)
    barrier()
    elapsed = time.perf_counter() - t0
    if clock:
        clock.stop()
    per_rank_s = [elapsed]
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        per_rank_s = [float(x.item()) for x in allt]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # correctness of what was timed: every output decrypts to LUT[m]
    out = d_out.cpu().numpy().view(np.uint64)
    dec = eng.decrypt(out, DL)
    want = np.where(lut_sel == 0, msgs, rnd_table[msgs + 8])
    verified = bool(np.array_equal(dec, want))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, eng, out, dec)

    KERNEL = {64: "k_blind_rotate_tp<2>", 49: "k_blind_rotate_tpx49<13, 3, 15>", 65: "k_blind_rotate_t64f<3, 10, false>"}
    ARITH = {64: "integers mod 2^64-2^32+1 in u64 (64-bit integer VALU)",
             49: "exact integers mod 2^49-720895 carried in f64 (FMA pairs); keyswitch: int8 matrix cores, int32 sums",
             65: "ciphertexts mod 2^64 (Concrete's torus), Bg 2^10; exact external products: digit polynomials against two 24-bit limbs "
                 "of every key word (key stored at 48 bits of precision) through a folded 512-point complex FFT in f64, every limb sum "
                 "(an integer below 2^45, transform error below 2^-11) rounded to the nearest integer and recombined mod 2^64 - the same "
                 "words as the oracle's integer arithmetic; keyswitch: int8 matrix cores"}
    DTYPE = {64: "u64", 49: "f64", 65: "u64/f64"}
    CTS_PER_WG = {64: 2, 49: 4, 65: 4}       # ciphertexts per workgroup of the wave-pair kernels (one workgroup per compute unit)

    total_pbs = B * world * args.steps
    value = total_pbs / elapsed
    res = {
        "metric": "PBS/sec per GPU + encrypted n x n inverse wall-clock (n=2,3,4)", "value": value, "unit": "PBS/s",
        "n_gpus": world, "world_size_seen": (dist.get_world_size() if dist is not None else 1),
        "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": DTYPE[eng.q_bits], "data": "synthetic",
        "config": {"workload": f"pbs_batch: B={B} LWE ciphertexts per GPU per step, TFHE n=630 N=1024 k=1 l=3 "
                               f"(Bg=2^{P.bs_base_log}, ks 8x4 bits), q_bits={eng.q_bits}, 4-bit signed messages, 2 LUTs (identity, random)",
                   "arithmetic": ARITH[eng.q_bits],
                   "keys": "bmi_keygen_insecure_deterministic(0x5EED): one key set replicated on every rank without an exchange",
                   "batch_per_gpu": B, "pbs_per_gpu_per_s": value / world,
                   "per_rank_pbs_per_s": [B * args.steps / t for t in per_rank_s],
                   "verified_decrypt": verified,
                   "multi_gpu_placement": "PBS batches shard over the ranks (contiguous ranges, no data-path collective); the encrypted "
                                          "inverses of configs 2-4 are placed on ONE GPU by design (their levels are at most 256-1,024 wide: "
                                          "one kernel round); --inverse-sharded splits the wide levels of the 8x8 across the ranks",
                   "derived_reference_pbs_per_s_64core_cpu": "35-69 (derived, BASELINE.md section 1)"},
    }

    def close():
        """ends the run on every rank; exits non-zero when the timed outputs failed the decrypt check"""
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        eng.close()
        if not verified:
            raise SystemExit("bench outputs failed decrypt verification")

    if not args.full:
        if rank == 0:
            print(json.dumps(res))
        return close()

    def key_weights(e):
        sk_small, sk_big = e.export_keys()[:2]
        pairs = sk_small[0::2].copy()
        pairs[:sk_small[1::2].size] |= sk_small[1::2]
        return int(sk_small.sum()), int(sk_big.sum()), int(pairs.sum())

    # output noise of the timed batch against the analytic CGGI variance (tests/test_gpu_parity.py holds it to +-15 %).  The
    # rounding term of a step is multiplied by the key bit its GGSW encrypts, so it is counted for the SET bits of the LWE key
    # (unrolled: the pairs whose bits are not both zero, doubled by the factor X^c - 1); a torus key stored at p < 64 bits adds
    # the rounding error of a row's body and key-selected mask words to the key noise
    def output_noise(e, outputs, expected, unrolled=False):
        Pp, Qm, dlx = e.P, e.modulus, e.delta_log()
        err = np.array([((int(x) - (int(m) << dlx)) + Qm // 2) % Qm - Qm // 2 for x, m in zip(e.phase(outputs), expected)],
                       dtype=np.float64) / float(Qm)
        hw_small, hw_big, live_pairs = key_weights(e)
        Bg = 2.0 ** Pp.bs_base_log
        prec = e.bsk_precision
        sigma2 = Pp.glwe_noise ** 2 + ((1 + hw_big) * 4.0 ** (64 - prec) / 12 / 2.0 ** 128 if prec != 64 else 0.0)
        key_term = Pp.n * Pp.bs_levels * (Pp.k + 1) * Pp.N * (Bg * Bg + 2) / 12.0 * sigma2
        rnd = (1 + hw_big) / (12.0 * Bg ** (2 * Pp.bs_levels))
        analytic = 3 * key_term + 2 * live_pairs * rnd if unrolled else key_term + hw_small * rnd
        return {"samples": int(err.size), "log2_std_measured": float(0.5 * np.log2(np.var(err))),
                "log2_std_cggi_formula": float(0.5 * np.log2(analytic)), "variance_ratio": float(np.var(err) / analytic),
                "log2_max_abs": float(np.log2(np.abs(err).max())), "log2_half_box": -6.0,
                "bsk_precision_bits": int(prec)}

    br_ms = float(np.mean([a.elapsed_time(b) for a, b in events]))
    # shader clock while the timed kernels ran (sysfs, sampled by a thread during the timed region); the spec maximum if unreadable
    sclk_mhz, sclk_src = clock.result()

    # the vector-ALU roof (what the blind rotation is bound by): issue cycles of the kernel's vector instructions per second
    # against 1,024 SIMDs x shader clock.  Issue cost per wave64 instruction on a SIMD-32: 2 cycles, f64 and 64-bit integer
    # instructions 4 (MI355X_MICROARCH.md: `v_fma_f32` 2 cycles; f64 runs at half the f32 rate).  Instruction counts: static, one
    # step of the kernel's main loop (tools/isa_count.py -> profiles/r04_isa_counts.json)
    isa = {}
    try:
        isa = json.load(open(os.path.join(REPO, "profiles", "r04_isa_counts.json")))["kernels"]
    except Exception:
        pass

    def alu_roof(kernel, kernel_ms, count, n_lwe, waves_per_ct=2, steps_per_ct=None):
        c = isa.get(kernel)
        if not c:
            return {"bound": "valu issue", "error": f"no static instruction count for {kernel} in profiles/r04_isa_counts.json"}
        steps = n_lwe if steps_per_ct is None else steps_per_ct
        cyc_per_ct = float(c["valu_issue_cycles"]) * waves_per_ct * steps
        achieved = cyc_per_ct * count / (kernel_ms * 1e-3)
        peak = 1024 * sclk_mhz * 1e6
        return {"bound": "valu issue (f64)", "achieved": achieved, "peak": peak, "unit": "SIMD issue cycles/s", "frac": achieved / peak,
                "valu_instructions_per_step_per_wavefront": c["valu"], "of_them_f64": c["valu_f64"],
                "valu_issue_cycles_per_step_per_wavefront": c["valu_issue_cycles"], "wavefronts_per_ciphertext": waves_per_ct,
                "steps_per_ciphertext": steps, "sclk_mhz": sclk_mhz, "sclk_source": sclk_src,
                "source": "static ISA count (profiles/r04_isa_counts.json) x live launch rate; peak = 256 CUs x 4 SIMDs x sclk",
                "modmul_per_s": MODMUL_PER_PBS * count / (kernel_ms * 1e-3), "modmul_per_pbs": MODMUL_PER_PBS}

    achieved_gbs = BSK_BYTES_PER_PBS * B / (br_ms * 1e-3) / 1e9
    traffic = valu_busy = None
    tpath = os.path.join(REPO, "profiles", "hbm_traffic.json")
    if os.path.exists(tpath):
        try:
            for tj in json.load(open(tpath)).get("entries", []):
                if tj.get("kernel") == KERNEL[eng.q_bits] and tj.get("batch") == B:
                    traffic = tj.get("bytes_per_launch")
                    valu_busy = tj.get("valu_busy_frac")
        except Exception:
            traffic = valu_busy = None
    alu = alu_roof(KERNEL[eng.q_bits], br_ms, B, P.n)
    alu["valu_busy_frac_profiled"] = valu_busy
    alu["valu_busy_source"] = "profiled-static (waves per SIMD x SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES, profiles/hbm_traffic.json)"

    def cycles_per_cmux(kernel_ms, count, n_lwe, cts_per_wg, clock_mhz):
        """shader-clock cycles one workgroup spends per blind-rotation step: launch time x clock / (steps x workgroup rounds per CU)"""
        rounds = -(-count // (cts_per_wg * 256))
        return kernel_ms * 1e-3 * clock_mhz * 1e6 / (n_lwe * rounds)

    north_star = {"bound": "hbm", "achieved": achieved_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved_gbs / HBM_PEAK_GBS,
                  "algorithmic_bytes_per_pbs": BSK_BYTES_PER_PBS,
                  "convention": "bootstrap-key bytes per PBS (no reuse) x PBS per launch / launch time vs peak HBM: BASELINE.json's figure "
                                "(1e5 PBS/s = 0.774); not a physical roof - the key is shared by the batch and stays in L2 / MALL"}
    # `roofline` is the PHYSICAL bound of the dominant kernel (vector issue: static instruction counts x live launch rate against
    # 1,024 SIMDs x the sampled shader clock); the north star's HBM-read convention sits beside it as `north_star` / `north_star_frac`
    roofline = {"bound": "valu_issue_f64", "achieved": alu.get("achieved"), "peak": alu.get("peak"), "unit": alu.get("unit", "SIMD issue cycles/s"),
                "frac": alu.get("frac"), "traffic": traffic,
                "traffic_vs_algorithmic": (None if traffic is None else traffic / (BSK_BYTES_PER_PBS * B)),
                "traffic_source": "profiled-static: rocprofv3 --pmc pass of this command, profiles/hbm_traffic.json",
                "kernel": KERNEL[eng.q_bits], "kernel_ms": br_ms,
                "kernel_cycles_per_cmux": cycles_per_cmux(br_ms, B, P.n, CTS_PER_WG[eng.q_bits], sclk_mhz),
                "sclk_mhz": sclk_mhz,
                "north_star_frac": achieved_gbs / HBM_PEAK_GBS, "north_star": north_star, "alu": alu}
    res["config"]["output_noise"] = output_noise(eng, out, want) if rank == 0 else None
    res["roofline"] = roofline

    def latency_ms(e, d_small_x, d_ids_x, d_out_x, cnt):
        e.blind_rotate(d_small_x, d_ids_x, cnt, d_out_x, stream)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(5):
            e.blind_rotate(d_small_x, d_ids_x, cnt, d_out_x, stream)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / 5

    if rank == 0 and world == 1:
        d_lat = torch.empty_like(d_out)   # (the timed outputs stay untouched: they are checked against the oracle below)
        res["latency_ms_1"], res["latency_ms_256"] = (latency_ms(eng, d_small, d_ids, d_lat, c) for c in (1, 256))
        del d_lat
        if eng.q_bits == 65:   # the reference's own modulus is the headline: the fields rounds 2-3 asked for repeat it
            res.update(value_torus64=value, frac_torus64=achieved_gbs / HBM_PEAK_GBS, alu_frac_torus64=alu.get("frac"),
                       latency_ms_torus64=res["latency_ms_1"])

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        # threads of the CPU baseline = the host cores this process may actually use (affinity mask, cgroup CPU quota),
        # not the machine's core count: an over-subscribed OpenMP team would make the baseline look worse than it is
        def host_cores():
            cores = len(os.sched_getaffinity(0))
            quota = None
            for qf, pf in (("/sys/fs/cgroup/cpu.max", None), ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "/sys/fs/cgroup/cpu/cpu.cfs_period_us")):
                try:
                    if pf is None:
                        q, per = open(qf).read().split()
                        quota = None if q == "max" else float(q) / float(per)
                    else:
                        q, per = float(open(qf).read()), float(open(pf).read())
                        quota = None if q <= 0 else q / per
                    break
                except Exception:
                    continue
            usable = cores if quota is None else max(1, min(cores, int(quota + 0.999)))
            return usable, {"cpu_count": os.cpu_count(), "affinity": cores, "cgroup_quota_cores": quota}
        usable, host_info = host_cores()
        from oracle import tfhe_oracle as to
        if "OMP_NUM_THREADS" not in os.environ:
            to.set_num_threads(usable)
        sk_small, sk_big, bsk, ksk = eng.export_keys()
        tvs = np.stack([eng.lut_get(ident), eng.lut_get(rlut)])
        threads = to.num_threads()
        # the vectorised exact-f64 path exists for the 49-bit field and for the torus at its default set (48-bit key, two 24-bit limbs);
        # Goldilocks times the generic path
        fast = eng.q_bits == 49 or (eng.q_bits == 65 and eng.bsk_precision == 48 and P.bs_base_log <= 10)
        octx = (to.FastCtx if fast else to.Ctx)(to.default_params(q_bits=eng.q_bits), bsk, ksk)
        probe = octx.pbs(ct[:threads], tvs, lut_sel[:threads].astype(np.uint32))   # (first call: thread start-up, tables)
        n_probe = min(B, 8 * threads)                                                # several ciphertexts per thread: the per-call cost is amortised
        t1 = time.perf_counter()
        octx.pbs(ct[:n_probe], tvs, lut_sel[:n_probe].astype(np.uint32))
        rate = n_probe / max(time.perf_counter() - t1, 1e-3)
        sample = int(max(threads, min(B, round(rate * args.cpu_seconds / threads) * threads)))
        t1 = time.perf_counter()
        ref = octx.pbs(ct[:sample], tvs, lut_sel[:sample].astype(np.uint32))
        cpu_s = time.perf_counter() - t1
        bit_exact = bool(np.array_equal(ref, out[:sample]) and np.array_equal(probe, out[:threads]))
        self_check = None
        if fast:   # the slow generic path (the definition) on a few ciphertexts of the sample
            slow = to.Ctx(to.default_params(q_bits=eng.q_bits), bsk, ksk)
            pick = np.linspace(0, sample - 1, min(sample, max(4, threads // 8))).astype(int)
            self_check = bool(np.array_equal(slow.pbs(ct[pick], tvs, lut_sel[pick].astype(np.uint32)), ref[pick]))
            slow.close()
        res["cpu_baseline"] = {"value": sample / cpu_s, "unit": "PBS/s", "cores": threads, "host": host_info, "kind": "port",
                               "ms_per_pbs_per_thread": cpu_s / sample * threads * 1e3,
                               "sample": f"first {sample} ciphertexts of the same batch, same keys / LUTs; oracle/tfhe_oracle.c "
                                         + ("fast path (exact f64 arithmetic mod 2^49-720895; the torus as two 24-bit limbs; AVX-512 clones)" if fast
                                            else "generic exact path") + f", OpenMP over the batch, {cpu_s:.1f} s",
                               "fast_path_matches_generic_path": self_check,
                               "gpu_matches_bit_for_bit": bit_exact,
                               "concrete": "Concrete not present (import concrete fails: not installed, no network)"}
        res["config"]["verified_bit_exact_vs_oracle"] = bit_exact
        octx.close()

    if rank == 0 and world == 1 and args.q_bits is None and not args.no_second_field:
        # the same batch on the 2^64 torus (Concrete's own ciphertext modulus: a first-class result, also printed at the top level as
        # value_torus64 / frac_torus64), with the unrolled keys, and on the Goldilocks field: 1 warm-up + 3 timed steps each, kernel
        # time by events; reported beside the headline, never `value`
        def leg(qb, unroll=False, inverses=False, preset=None, batch=None):
            kw = {"glwe_noise": 2.0 ** -41} if (unroll and qb == 49) else {}
            e2 = tfhe.Engine(tfhe.preset_params(preset) if preset else tfhe.default_params(q_bits=qb, **kw), device=dev_index)
            B = batch or args.batch          # (shadows the headline's batch inside this leg)
            msgs_l, lut_sel_l, want_l = msgs[:B], lut_sel[:B], want[:B]
            try:
                if unroll:
                    e2.set_bsk_unroll(2)
                e2.keygen(0x5EED)
                dl2 = e2.delta_log()
                i2 = e2.lut_register(np.arange(-8, 8), 4, dl2)
                r2 = e2.lut_register(rnd_table, 4, dl2)
                ct2 = e2.encrypt(msgs_l, dl2)
                d_in2 = torch.from_numpy(ct2.view(np.int64)).to(dev)
                d_ids2 = torch.from_numpy(np.where(lut_sel_l == 0, i2, r2).astype(np.int32)).to(dev)
                d_small2 = torch.empty((B, e2.P.small), dtype=torch.int64, device=dev)
                d_out2 = torch.empty_like(d_in2)
                e2.pbs(d_in2, d_ids2, B, d_out2, stream)
                torch.cuda.synchronize()
                ev = []
                ck = SclkSampler()
                ck.start()
                t1 = time.perf_counter()
                for _ in range(3):
                    e2.keyswitch(d_in2, B, d_small2, stream)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    e2.blind_rotate(d_small2, d_ids2, B, d_out2, stream)
                    b.record()
                    ev.append((a, b))
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t1) / 3
                ck.stop()
                kms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
                out2 = d_out2.cpu().numpy().view(np.uint64)
                ok2 = bool(np.array_equal(e2.decrypt(out2, dl2), want_l))
                Pe = e2.P
                plain_key_bytes = Pe.n * 4 * Pe.bs_levels * Pe.N * 8
                gbs = plain_key_bytes * B / (kms * 1e-3) / 1e9
                kname = (("k_blind_rotate_w2_t64f<3, 10, 46>" if B > 256 else "k_blind_rotate_w_t64f<3, 10, 46, false>") if (qb == 65 and Pe.N == 2048) else
                         "k_blind_rotate_q_t64f<3, 10, 44, false>" if (qb == 65 and Pe.N == 4096) else
                         {49: "k_blind_rotate_lat2u_49<3, 15>", 65: ("k_blind_rotate_tp2u_t64f<3, 10, 42>" if B > 256 else "k_blind_rotate_lat2u_t64f<3, 10, 42, false>")}[qb] if unroll else KERNEL[qb])
                one_wg_per_ct = unroll or Pe.N > 1024
                sm, ss = ck.result()
                rep = {"q_bits": qb, "params": {"n": int(Pe.n), "N": int(Pe.N), "k": int(Pe.k), "l": int(Pe.bs_levels), "log2_Bg": int(Pe.bs_base_log),
                                                "ks": f"{Pe.ks_levels}x{Pe.ks_base_log} bits", "log2_lwe_noise": round(float(np.log2(Pe.lwe_noise)), 2),
                                                "log2_glwe_noise": round(float(np.log2(Pe.glwe_noise)), 2)},
                       "batch": B, "pbs_per_s": B / dt, "ms_per_step": dt * 1e3, "verified_decrypt": ok2,
                       "bsk_precision_bits": int(e2.bsk_precision),
                       "output_noise": output_noise(e2, out2, want_l, unrolled=unroll),
                       "kernel": kname, "kernel_ms": kms,
                       "kernel_cycles_per_cmux": cycles_per_cmux(kms, B, (Pe.n + 1) // 2 if unroll else Pe.n, (2 if ("tp2u" in kname or "w2_t64f" in kname) else 1) if one_wg_per_ct else CTS_PER_WG[qb], sm),
                       "sclk_mhz": sm,
                       "north_star": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                                      "algorithmic_bytes_per_pbs": plain_key_bytes},
                       "frac": gbs / HBM_PEAK_GBS}
                if unroll:
                    own = (Pe.n + 1) // 2 * 3 * 4 * Pe.bs_levels * Pe.N * 8
                    rep["frac_own_key_bytes"] = own * B / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS
                    rep["own_key_bytes_per_pbs"] = own
                elif not one_wg_per_ct:   # wave-pair kernels: static instruction count x live rate against the issue roof at the clock sampled here
                    c = isa.get(kname)
                    if c:
                        cyc = float(c["valu_issue_cycles"]) * 2 * Pe.n * B / (kms * 1e-3)
                        rep["alu"] = {"bound": "valu issue (f64)", "achieved": cyc, "peak": 1024 * sm * 1e6, "frac": cyc / (1024 * sm * 1e6),
                                      "unit": "SIMD issue cycles/s", "sclk_mhz": sm, "sclk_source": ss,
                                      "valu_instructions_per_step_per_wavefront": c["valu"]}
                # latency of one bootstrap and of one full round of 256 (events around the kernel)
                d_lat2 = torch.empty_like(d_out2)
                for cnt in (1, 256):
                    rep[f"latency_ms_{cnt}"] = latency_ms(e2, d_small2, d_ids2, d_lat2, cnt)
                del d_lat2
                if not args.no_cpu_baseline and (unroll or qb == 65):
                    # the oracle's blind rotation (plain or unrolled mode) on a few ciphertexts of the batch: bit for bit
                    from oracle import tfhe_oracle as to
                    _, _, bsk_u, ksk_u = e2.export_keys()
                    to.set_field(qb)
                    oc = to.Ctx(to.Params(**{f: getattr(Pe, f) for f, _ in tfhe.Params._fields_}), bsk_u, ksk_u)
                    if unroll:
                        oc.set_bsk_unrolled(e2.export_bsk_unrolled())
                    tv2 = np.stack([e2.lut_get(i2), e2.lut_get(r2)])
                    pick = np.arange(0, B, max(1, B // 6))[:(2 if Pe.N > 1024 else 6)]
                    wantu = oc.pbs(ct2[pick], tv2, lut_sel_l[pick].astype(np.uint32), unrolled=unroll)
                    rep["bit_exact_vs_oracle"] = bool(np.array_equal(wantu, out2[pick]))
                    oc.close()
                    to.set_field(eng.q_bits)
                if inverses and not args.no_inverse:
                    from bmi_amd import inverse_bench
                    sizes = tuple(int(x) for x in args.inverse_sizes.split(",") if x)
                    rep["encrypted_inverse_wall_clock"] = inverse_bench.run(e2, sizes)
                return rep
            finally:
                e2.close()

        INV_FIELDS = ("len", "ints", "evaluate_s", "end_to_end_s", "ms_per_level", "pbs", "depth", "matches_plaintext_circuit")
        # (name, q_bits, unrolled key, inverse wall-clocks, preset, batch)
        legs = [("torus64", 65, False, False, None, None), ("p49_field", 49, False, True, None, None),
                ("torus64_unrolled_key", 65, True, True, None, None), ("unrolled_key_49", 49, True, True, None, None)]
        if not args.no_secure_leg:
            legs.insert(0, ("secure128_torus", 65, False, True, "secure128_torus", min(B, 2048)))
            legs.insert(1, ("secure128_torus_wide", 65, False, False, "secure128_torus_wide", min(B, 1024)))
        if args.goldilocks_leg:
            legs.append(("roofline_q64_goldilocks", 64, False, False, None, None))
        for name, qb, un, inv, preset, bt in legs:
            if qb == eng.q_bits and not un and preset is None:
                continue
            try:
                res[name] = leg(qb, un, inv, preset, bt)
            except Exception as e:  # reported, never hidden
                res[name] = {"q_bits": qb, "error": repr(e)}

        def inv_scalars(prefix, inv):
            if isinstance(inv, dict):
                for k, v in inv.items():
                    if isinstance(v, dict) and "evaluate_s" in v:
                        res[f"{prefix}inverse_{k}_s"] = v["evaluate_s"]

        if "kernel_ms" in res.get("secure128_torus", {}):
            st = res["secure128_torus"]
            st["key"] = ("preset secure128_torus: n 742 at LWE noise 2^-17.1, N 2048 at GLWE noise 2^-44 (the 128-bit-secure pairs of TFHE-rs' "
                         "PARAM_MESSAGE_2_CARRY_2_KS_PBS) on q = 2^64; (l, Bg) = (3, 2^10), key stored at 46 bits (two 23-bit limbs), exact limb "
                         "sums through the folded 1,024-point f64 FFT; one workgroup of 16 wavefronts per ciphertext up to 256 ciphertexts, two ciphertexts "
                         "per workgroup sharing the key words beyond (k_blind_rotate_w2_t64f)")
            res["secure128_torus_pbs_per_s"] = st["pbs_per_s"]
            res["secure128_torus_latency_ms_1"] = st.get("latency_ms_1")
            res["secure128_torus_latency_ms_256"] = st.get("latency_ms_256")
            inv = st.get("encrypted_inverse_wall_clock")
            inv_scalars("secure128_torus_", inv)
            if isinstance(inv, dict):
                st["reference_readme_64core_cpu_run_s"] = {"2x2_len23_ints9": 85.0, "3x3_len23_ints9": "1349-1768",
                                                           "note": "README.md:129-141: concrete-python 2.1.0 at its 128-bit defaults, `low` "
                                                                   "precision (len 23, ints 9); the sizes here are BASELINE's (20, 8) / (30, 12) / (40, 16)"}
        if "kernel_ms" in res.get("secure128_torus_wide", {}):
            sw = res["secure128_torus_wide"]
            sw["key"] = ("preset secure128_torus_wide: the same LWE pair under N 4096 on q = 2^64 (5-bit look-ups: the reference's unmodified "
                         "circuits); (l, Bg) = (3, 2^10), key at 44 bits (two 22-bit limbs), folded 2,048-point f64 FFT split over eight "
                         "wavefronts, keyswitch 16 x 1 bit on the matrix cores; measured here on 4-bit tables")
            res["secure128_torus_wide_pbs_per_s"] = sw["pbs_per_s"]
            res["secure128_torus_wide_latency_ms_256"] = sw.get("latency_ms_256")
        if "kernel_ms" in res.get("torus64", {}):
            res["value_torus64"] = res["torus64"]["pbs_per_s"]
            res["frac_torus64"] = res["torus64"]["frac"]
            res["alu_frac_torus64"] = res["torus64"].get("alu", {}).get("frac")
            res["latency_ms_torus64"] = res["torus64"]["latency_ms_1"]
        if "kernel_ms" in res.get("p49_field", {}):
            res["value_p49"] = res["p49_field"]["pbs_per_s"]
            res["frac_p49"] = res["p49_field"]["frac"]
            res["alu_frac_p49"] = res["p49_field"].get("alu", {}).get("frac")
            res["latency_ms_p49"] = res["p49_field"]["latency_ms_1"]
            inv = res["p49_field"].get("encrypted_inverse_wall_clock")
            if isinstance(inv, dict):
                res["config"]["encrypted_inverse_wall_clock_p49"] = {k: {f: v.get(f) for f in INV_FIELDS} for k, v in inv.items()}
        if "kernel_ms" in res.get("torus64_unrolled_key", {}):
            res["value_torus64_unrolled"] = res["torus64_unrolled_key"]["pbs_per_s"]
            res["frac_torus64_unrolled"] = res["torus64_unrolled_key"]["frac"]
            res["latency_ms_torus64_unrolled"] = res["torus64_unrolled_key"]["latency_ms_1"]
            inv = res["torus64_unrolled_key"].get("encrypted_inverse_wall_clock")
            if isinstance(inv, dict):
                res["config"]["encrypted_inverse_wall_clock_torus64_unrolled_key"] = {k: {f: v.get(f) for f in INV_FIELDS} for k, v in inv.items()}
                res["inverse_3x3_s_torus64_unrolled"] = inv.get("3x3", {}).get("evaluate_s")
        if "kernel_ms" in res.get("unrolled_key_49", {}):
            inv = res["unrolled_key_49"].get("encrypted_inverse_wall_clock")
            if isinstance(inv, dict):   # the wall-clocks to quote for EncryptedMatrixInversion(unroll=True)
                res["config"]["encrypted_inverse_wall_clock_unrolled_key"] = {k: {f: v.get(f) for f in INV_FIELDS} for k, v in inv.items()}
                res["inverse_3x3_s_p49_unrolled"] = inv.get("3x3", {}).get("evaluate_s")

    if not args.no_inverse and rank == 0 and world == 1:
        try:
            from bmi_amd import inverse_bench
            sizes = tuple(int(x) for x in args.inverse_sizes.split(",") if x)
            res["config"]["encrypted_inverse_wall_clock"] = inverse_bench.run(eng, sizes)
            for k, v in res["config"]["encrypted_inverse_wall_clock"].items():   # the headline engine's wall-clocks, first class
                res[f"inverse_{k}_s"] = v["evaluate_s"]
        except Exception as e:  # reported, never hidden
            res["config"]["encrypted_inverse_wall_clock"] = {"error": repr(e)}
        try:   # the serving form: 16 matrices through one walk of the 3x3 circuit's levels (throughput kernel instead of 319 latency rounds each)
            bt = inverse_bench.run_batched(eng, 3, args.inverse_batch)
            res["config"]["encrypted_inverse_batched"] = bt
            res["inverse_3x3_batched_s_per_matrix"] = bt["per_matrix_s"]
            res["inverse_3x3_batched_pbs_per_s"] = bt["pbs_per_s"]
        except Exception as e:
            res["config"]["encrypted_inverse_batched"] = {"error": repr(e)}
        if not args.no_readme_benchmark:
            try:   # the reference's own published benchmark configurations (README.md:129-142), beside its figures
                res["config"]["reference_readme_benchmark"] = inverse_bench.run_readme_low(eng)
            except Exception as e:
                res["config"]["reference_readme_benchmark"] = {"error": repr(e)}

    if args.inverse_sharded and world > 1:
        from bmi_amd import inverse_bench
        sizes = tuple(int(x) for x in sharded_sizes.split(",") if x)
        rep = inverse_bench.run(eng, sizes, shard_threshold=args.shard_threshold)   # collective: every rank calls it
        res["config"]["encrypted_inverse_wall_clock_sharded"] = rep
        for k, v in rep.items():
            res[f"inverse_{k}_s_sharded_{world}gpu"] = v["evaluate_s"]
            res[f"inverse_{k}_sharded_levels"] = v.get("sharded_levels")

    if rank == 0:
        # the complete report goes to gpurun_out/bench_details.json (scratch; merged back by gpurun); the printed line keeps the
        # contract's fields, the scalars to quote and a compact form of every leg, so that a tail of stdout still holds all of it
        try:
            os.makedirs(os.path.join(REPO, "gpurun_out"), exist_ok=True)
            json.dump(res, open(os.path.join(REPO, "gpurun_out", "bench_details.json"), "w"), indent=1)
        except Exception:
            pass
        print(json.dumps(compact(res)))
    close()


if __name__ == "__main__":
    main()
