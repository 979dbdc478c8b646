#!/usr/bin/env python3
"""The keyswitch noise of ONE key set has a mean: the signed digits lie in [-B/2, B/2) below the top level (mean -1/2; the top
level, which absorbs the carry, has a small positive mean: +1/6 at B = 4), and the noises e_r of the key's rows are fixed numbers,
so a keyswitched phase carries -sum_r d_r e_r = -sum_lev mean(d_lev) sum_j e_(j,lev) + a zero-mean part.
error_budget.keyswitch_variance is the second moment averaged over keys (offset^2 included); a measured failure count belongs to
one key.  This prints, for the seeded key set of a preset (the CPU oracle reproduces it bit for bit: no GPU needed), the row
noises' sums, the mean / variance of the keyswitched phase of encryptions of 0 in positions of the 2N circle, and the failure
probability of a look-up of LUT_BITS bits with and without the offset (profiles/keyswitch_key_offset.txt).
usage: ks_key_offset.py [PRESET:LUT_BITS ...]   (torus presets; default secure128_torus:6 north_star_torus64:5)"""
import math, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "bounty-matrix-inversion_amd"))
import numpy as np
from oracle import tfhe_oracle as to
from bmi_amd import tfhe, error_budget as eb

SEED, B = 0x5EED, 8192


def tail(x):
    return 0.5 * math.erfc(x / math.sqrt(2.0))


def digit_means(words, levels, base_log):
    """mean of every level's digit over `words`, by the library's torus rule (FieldT::digits, csrc/bmi_kernels_t64.hip): round to
    the top levels * base_log bits, digits in [-B/2, B/2) from the bottom up, the top level absorbs the carry"""
    shift, B = 64 - levels * base_log, 1 << base_log
    c = words.view(np.int64)
    r = (c >> shift) + ((c >> (shift - 1)) & 1)
    means = np.zeros(levels)
    for lev in range(levels - 1, 0, -1):
        v = r & (B - 1)
        r = r >> base_log
        carry = v >= B // 2
        means[lev] = (v - B * carry).mean()
        r = r + carry
    means[0] = r.mean()
    return means


for case in sys.argv[1:] or ["secure128_torus:6", "north_star_torus64:5"]:
    preset, bits = case.split(":")
    Pt = tfhe.preset_params(preset)
    assert Pt.q_bits == tfhe.TORUS64, "wrapping 64-bit arithmetic below: torus presets only"
    to.set_field(Pt.q_bits)
    P = to.Params(**{f: getattr(Pt, f) for f, _ in tfhe.Params._fields_})
    K = to.keygen(P, SEED)
    sk_small, sk_big = np.asarray(K.sk_small), np.asarray(K.sk_big)
    n, N, l, b = P.n, P.N, P.ks_levels, P.ks_base_log
    ksk = np.asarray(K.ksk).reshape(P.k * N, l, n + 1)
    body = ksk[..., n] - (ksk[..., :n] * sk_small[None, None, :]).sum(-1, dtype=np.uint64)
    msg = np.array([[(int(sk_big[j]) << (64 - b * (lev + 1))) & ((1 << 64) - 1) for lev in range(l)] for j in range(P.k * N)], dtype=np.uint64)
    e = (body - msg).view(np.int64).astype(np.float64) / 2.0 ** 64 * 2 * N          # row noises, in positions
    cts = to.lwe_encrypt(sk_big, P.glwe_noise, SEED, 0, np.zeros(B, np.uint64))
    ctx = to.Ctx(P, K.bsk, K.ksk)
    small = np.asarray(ctx.keyswitch(cts)).reshape(B, n + 1)
    ctx.close()
    pos = (small[:, n] - (small[:, :n] * sk_small[None, :]).sum(-1, dtype=np.uint64)).view(np.int64).astype(np.float64) / 2.0 ** 64 * 2 * N
    hs, hb = int(sk_small.sum()), int(sk_big.sum())
    model = eb.keyswitch_variance(Pt, hw_big=hb) * (2.0 * N) ** 2
    rnd = (1 + hs) / 12.0
    half = N / 2.0 ** (int(bits) + 1)
    s = math.sqrt(pos.var() + rnd)
    print(f"{preset} (seed {SEED:#x}, hw(s) {hs}, hw(S) {hb}; keyswitch {l} x {b} bits, {P.k * N * l} rows of noise 2^{math.log2(e.std() / (2 * N)):.2f})")
    mu = digit_means(np.ascontiguousarray(cts[:, :P.k * N]).reshape(-1), l, b)
    print(f"  sum of the row noises per level (top first) {np.round(e.sum(0), 3).tolist()} positions; mean digit per level {np.round(mu, 3).tolist()}; "
          f"expected offset of this key, -sum_lev mean(d_lev) sum_j e_(j,lev): {-(mu * e.sum(0)).sum():.3f}")
    print(f"  keyswitched phase of {B} encryptions of 0: mean {pos.mean():.3f} +- {pos.std() / math.sqrt(B):.3f}, variance {pos.var():.3f}, "
          f"second moment {(pos ** 2).mean():.3f} positions^2; keyswitch_variance (average over keys) {model:.3f}")
    print(f"  {bits}-bit look-up, half box {half:g}, rounding term {rnd:.2f}: p = {2 * tail(half / math.sqrt(model + rnd)):.5f} (budget: zero mean, second moment "
          f"{model + rnd:.2f}); {tail((half - 0.5 - pos.mean()) / s) + tail((half + 0.5 + pos.mean()) / s):.5f} (this key: mean {pos.mean():.2f}, variance {pos.var() + rnd:.2f}, "
          f"integer boxes [-{half + 0.5:g}, {half - 0.5:g}])", flush=True)
