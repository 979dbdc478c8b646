#!/usr/bin/env python3
"""Per-phase cycles (s_memtime) of wavefronts 0..7 of workgroup 0 of k_blind_rotate_t64f (debug build: make -C csrc prof).
The marks wait for the wavefront's outstanding LDS / scalar-memory operations, so a phase's figure includes its own waits."""
import os, sys, ctypes as C
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "bounty-matrix-inversion_amd"))
import numpy as np, torch
from bmi_amd import tfhe
tfhe.LIB_PATH = os.environ.get("BMI_TFHE_LIB") or tfhe.LIB_PATH.replace("libbmi_tfhe.so", "libbmi_tfhe_prof.so")   # (BMI_TFHE_LIB: an A/B profiling build)
# (rows 3-5 are summed over the CMUX's two hand-offs; row 4 includes the wait for the partner's acknowledgement of limb 0's partial;
#  the wait for its acknowledgement of limb 1's is inside row 6, under the first DFT8)
NAMES = ["resync barrier", "accumulator reads + rounding", "digits + 3 forward transforms", "products (12 rows, both limbs) + publishing (2)",
         "waiting for the partner's partials (2) + its first acknowledgement", "adding them + posting the acknowledgements (2)",
         "inverse transforms (2) + limb 0's rounding + acknowledgement wait", "recombination (1) + loop head"]
for B in [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "8192").split(",")]:
    eng = tfhe.Engine(tfhe.default_params(q_bits=65)); eng.keygen(0x5EED)
    DL = eng.delta_log(); lid = eng.lut_register(np.arange(-8, 8), 4, DL)
    ct = eng.encrypt(np.random.default_rng(1).integers(-8, 8, B), DL)
    dev = torch.device("cuda:0"); s = torch.cuda.current_stream().cuda_stream
    d_in = torch.from_numpy(ct.view(np.int64)).to(dev)
    d_small = torch.empty((B, eng.P.n + 1), dtype=torch.int64, device=dev)
    d_ids = torch.full((B,), lid, dtype=torch.int32, device=dev)
    d_out = torch.empty((B, 1025), dtype=torch.int64, device=dev)
    eng.set_kernel_variant(5); eng.keyswitch(d_in, B, d_small, s)
    for _ in range(2): eng.blind_rotate(d_small, d_ids, B, d_out, s)
    torch.cuda.synchronize()
    buf = (C.c_ulonglong * 128)(); assert tfhe.load_library().bmi_debug_phase_prof_t64f(buf) == 0
    a = np.array(buf[:64], dtype=np.float64).reshape(8, 8) / eng.P.n
    print(f"B = {B}: shader-clock cycles (s_memtime) per CMUX, wavefronts 0-7 of workgroup 0 (partners w and w ^ 1; w and w + 4 share a SIMD and, with w + 2 and w + 6, a key row; 4-7 set the pace)")
    for k, nm in enumerate(NAMES):
        print(f"  {nm:66s} " + " ".join(f"{a[w, k]:8.1f}" for w in range(8)))
    print(f"  {'total':66s} " + " ".join(f"{a[w].sum():8.1f}" for w in range(8)))
    eng.close()
