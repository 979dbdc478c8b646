"""The case table of the keyswitch tests (csrc/ks_mfma.hpp, csrc/ks_lincomb.hpp): the decomposition rule and the keyswitch itself
in Python integers, crafted keyswitch keys, and ciphertext rows built from the digit vectors they must decompose to.  Neither the
oracle nor the library takes part in anything computed here, so both are tested against it (tests/test_keyswitch_reference.py on
the CPU, tests/test_gpu_keyswitch.py on the GPU).  A plain helper module: no fixtures, no pytest hooks.

Conventions: q_bits = 64 (Goldilocks), 49 (the 49-bit field), 65 (the 2^64 torus); w = 49 or 64 is the width the gadget lives
on, g_l = 2^(w - base_log (l + 1)) the gadget element of level l (level 0 the most significant), B = 2^base_log,
shift = w - levels base_log >= 1 the number of bits rounded away."""
import functools
from fractions import Fraction
import math

import numpy as np

GOLD = 0xFFFFFFFF00000001
P49 = 562949952700417
TORUS64 = 65
MODULUS = {64: GOLD, 49: P49, TORUS64: 1 << 64}
NAMES = {64: "goldilocks64", 49: "p49", TORUS64: "torus64"}


def width(q_bits):
    return 49 if q_bits == 49 else 64


def lift_range(q_bits):
    """(lowest, highest) centred lift: [-2^63, 2^63) on the torus, (-q/2, q/2] on a prime"""
    Q = MODULUS[q_bits]
    return (-(1 << 63), (1 << 63) - 1) if q_bits == TORUS64 else (-((Q - 1) // 2), (Q - 1) // 2)


def centred(a, q_bits):
    Q = MODULUS[q_bits]
    assert 0 <= a < Q
    return a - Q if a > lift_range(q_bits)[1] else a


def rounded(a, levels, base_log, q_bits):
    """floor(centred(a) / 2^shift + 1/2) in exact rationals: the integer the digit vector of `a` spells in base B"""
    return math.floor(Fraction(centred(int(a), q_bits), 1 << (width(q_bits) - levels * base_log)) + Fraction(1, 2))


def digits(words, levels, base_log, q_bits):
    """[len(words)][levels] int64, level 0 the most significant: centred lift, rounded half up to its top levels * base_log
    bits, balanced digits in [-B/2, B/2) from the least significant one, the top digit absorbing the last carry (so it lies
    in [-B/2, B/2])."""
    B = 1 << base_log
    shift = width(q_bits) - levels * base_log
    assert levels >= 1 and base_log >= 1 and shift >= 1
    out = np.zeros((len(words), levels), np.int64)
    for i, a in enumerate(words):
        c = centred(int(a), q_bits)
        r = (2 * c + (1 << shift)) // (1 << (shift + 1))          # floor(c / 2^shift + 1/2), Python's floor division
        for lev in range(levels - 1, 0, -1):
            d = (r + B // 2) % B - B // 2
            r = (r - d) // B
            out[i, lev] = d
        out[i, 0] = r
    return out


def keyswitch(cts, ksk, n, levels, base_log, q_bits, D=None):
    """out[i][col] = ((col == n ? b_i : 0) - sum_j sum_lev d[i][j][lev] * ksk[j][lev][col]) mod q, exact.
    D: mask_digits(cts, ...) if the caller holds it already (crafted_digits below), else computed here.
    cts [rows][big_n + 1], ksk [big_n][levels][n + 1] (uint64 words below q).  The key is cut into four 16-bit quarters and each
    quarter's sums are one float64 matrix product: |d| <= 64, a quarter < 2^16 and at most 2^17 terms keep every partial sum an
    integer below 2^39, which float64 holds exactly in any order of summation; the quarters are recombined, and everything else
    is done, in Python integers."""
    Q = MODULUS[q_bits]
    cts = np.ascontiguousarray(cts, dtype=np.uint64)
    big_n = cts.shape[1] - 1
    K = big_n * levels
    ksk = np.ascontiguousarray(ksk, dtype=np.uint64).reshape(K, n + 1)
    D = mask_digits(cts, levels, base_log, q_bits) if D is None else D[:cts.shape[0]]
    assert D.shape == (cts.shape[0], K)
    assert base_log <= 7 and K <= 1 << 17 and np.abs(D).max(initial=0) <= 64
    Df = D.astype(np.float64)
    total = np.zeros((cts.shape[0], n + 1), dtype=object)
    for quarter in range(4):
        part = ((ksk >> np.uint64(16 * quarter)) & np.uint64(0xFFFF)).astype(np.float64)
        s = Df @ part
        assert np.abs(s).max(initial=0) < 2.0 ** 53
        total = total + s.astype(np.int64).astype(object) * (1 << (16 * quarter))
    out = -total
    out[:, n] = out[:, n] + cts[:, big_n].astype(object)
    return to_u64(out % Q)


def mask_digits(cts, levels, base_log, q_bits):
    """[rows][big_n * levels] int64: digits() of every mask word, row by row (index j * levels + lev)"""
    cts = np.asarray(cts)
    return np.stack([digits(row[:-1], levels, base_log, q_bits).reshape(-1) for row in cts]) if len(cts) else \
        np.zeros((0, (cts.shape[1] - 1) * levels), np.int64)


def to_u64(a):
    """object array of Python integers in [0, 2^64) -> uint64 array"""
    return np.array([int(v) for v in a.reshape(-1)], dtype=np.uint64).reshape(a.shape)


def rand_words(rng, shape, Q):
    """uniform canonical words of Z_Q as uint64: uniform words of Q's bit length, the few that reach Q drawn again"""
    bits = (Q - 1).bit_length()
    draw = lambda size: rng.integers(0, 1 << 32, size, dtype=np.uint64) << np.uint64(32) | rng.integers(0, 1 << 32, size, dtype=np.uint64)
    a = (draw(shape) >> np.uint64(64 - bits)).reshape(-1)
    while Q < 1 << 64:
        bad = np.flatnonzero(a >= np.uint64(Q))
        if bad.size == 0:
            break
        a[bad] = draw(bad.size) >> np.uint64(64 - bits)
    return a.reshape(shape)


# ------------------------------------------------------------------------------------------------ keyswitch keys
BYTE_PATTERNS = {"7f": 0x7F7F7F7F7F7F7F7F, "80": 0x8080808080808080, "ff": 0xFFFFFFFFFFFFFFFF, "7f80": 0x7F807F807F807F80,
                 "807f": 0x807F807F807F807F}


def key_families(q_bits):
    """names of the key families of this modulus.  "bytes-*": the 64-bit word of that byte pattern reduced below q.  "lift+*" /
    "lift-*": the word whose CENTRED lift is plus / minus that byte pattern, cut to the widest whole number of bytes that stays
    inside the lift's range - the balanced base-256 limbs are taken of the centred lift, so these are the carry chains
    themselves (0x80 -> limb -128 and a carry into every next byte; 0xFF -> limb -1 and a carry that runs to the top)."""
    fam = ["uniform", "q-1", "half", "half+1"]
    if q_bits == TORUS64:
        fam += ["2^63", "2^63-1"]
    fam += [f"bytes-{p}" for p in ("7f", "80", "ff", "7f80")]
    fam += [f"lift{s}{p}" for p in ("7f", "80", "ff", "807f") for s in "+-"]
    fam += ["one-row-one-column"]
    return fam


def key_word(family, q_bits):
    """the word of a constant-word family"""
    Q = MODULUS[q_bits]
    if family == "q-1":
        return Q - 1
    if family == "half":
        return Q // 2
    if family == "half+1":
        return (Q // 2 + 1) % Q
    if family == "2^63":
        return 1 << 63
    if family == "2^63-1":
        return (1 << 63) - 1
    if family.startswith("bytes-"):
        return BYTE_PATTERNS[family[6:]] % Q
    if family.startswith("lift"):
        sign, pat = (1 if family[4] == "+" else -1), BYTE_PATTERNS[family[5:]]
        lo, hi = lift_range(q_bits)
        nbytes = 8
        while not lo <= sign * (pat & ((1 << (8 * nbytes)) - 1)) <= hi:
            nbytes -= 1
        return (sign * (pat & ((1 << (8 * nbytes)) - 1))) % Q
    raise KeyError(family)


def make_key(family, big_n, levels, n, q_bits, seed=0):
    """[big_n][levels][n + 1] uint64, every word below q"""
    Q = MODULUS[q_bits]
    rng = np.random.default_rng([seed, big_n, levels, n, q_bits, 0x4B])
    shape = (big_n, levels, n + 1)
    if family == "uniform":
        key = rand_words(rng, shape, Q)
    elif family == "one-row-one-column":
        key = np.zeros(shape, np.uint64)
        j, lev, col = big_n - 3 if big_n > 3 else 0, levels - 1, n // 2
        key[j, lev, :] = rand_words(rng, n + 1, Q)
        key[:, :, col] = rand_words(rng, (big_n, levels), Q)
    else:
        key = np.full(shape, key_word(family, q_bits), np.uint64)
    assert Q == 1 << 64 or (key < np.uint64(Q)).all()
    key.setflags(write=False)
    return key


# ------------------------------------------------------------------------------------------------ ciphertext words and rows
def carry_one(d, B):
    """the digit vector d (level 0 first) plus one unit of its last digit, carries rippled by hand: a lower digit that reaches
    B/2 becomes -B/2 and hands one on; the top digit keeps what it gets"""
    d = list(d)
    d[-1] += 1
    for lev in range(len(d) - 1, 0, -1):
        if d[lev] == B // 2:
            d[lev] = -(B // 2)
            d[lev - 1] += 1
    return d


def crafted_words(levels, base_log, q_bits):
    """[(name, word, digit vector or None)]: words built as sum_l d_l g_l (+ a part below the last kept bit) mod q, with the digit
    vector they must decompose to written out beside them; None where only rounded() states the expectation (0, q - 1 and the
    two middles of the modulus).  A pattern whose value falls outside the centred lift's range has its top digit moved towards
    0 until it fits ("fitted"); one that cannot exist on this modulus and shape is left out."""
    Q, w = MODULUS[q_bits], width(q_bits)
    B, h, L = 1 << base_log, 1 << (base_log - 1), levels
    shift = w - L * base_log
    g = [1 << (w - base_log * (l + 1)) for l in range(L)]
    lo, hi = lift_range(q_bits)
    out = []

    def value(d, extra=0):
        return sum(dl * gl for dl, gl in zip(d, g)) + extra

    def add(name, d, extra=0, want=None, fit=True):
        d = list(d)
        assert all(-h <= x < h for x in d[1:]) and -h <= d[0] <= h
        while fit and not lo <= value(d, extra) <= hi and d[0] != 0:
            d[0] -= 1 if d[0] > 0 else -1
        if not lo <= value(d, extra) <= hi:
            return
        want = d if want is None else want(d)
        assert all(-h <= x < h for x in want[1:]) and -h <= want[0] <= h
        out.append((name, value(d, extra) % Q, [int(x) for x in want]))

    tie = 1 << (shift - 1)
    add("every digit -B/2 (top fitted)", [-h] * L)
    add("every digit B/2-1 (top fitted)", [h - 1] * L)
    add("top +B/2 over lower digits -B/2", [h] + [-h] * (L - 1), fit=False)
    add("top +B/2 alone, under a negative tie: 2^(w-1) - 2^(shift-1)", [h] + [0] * (L - 1), extra=-tie, fit=False)
    add("tie below every digit at B/2-1: the carry runs into the top digit (+B/2)", [h - 1] * L, extra=tie,
        want=lambda d: carry_one(d, B), fit=False)
    add("alternating -B/2, B/2-1 (top fitted)", [(-h, h - 1)[l & 1] for l in range(L)])
    add("alternating B/2-1, -B/2 (top fitted)", [(h - 1, -h)[l & 1] for l in range(L)])
    add("tie alone: half of the last kept bit rounds up", [0] * L, extra=tie, want=lambda d: carry_one(d, B))
    add("negative tie alone: -half of the last kept bit rounds up to 0", [0] * L, extra=-tie)
    add("tie below a last digit at B/2-1: the carry moves on", [1 if L > 1 else 0] + [0] * (L - 2) + [h - 1] * (L > 1), extra=tie,
        want=lambda d: carry_one(d, B))
    add("tie below every lower digit at B/2-1 (top fitted): the carry runs to the top", [0] + [h - 1] * (L - 1), extra=tie,
        want=lambda d: carry_one(d, B))
    add("tie below every digit -B/2 (top fitted)", [-h] * L, extra=tie, want=lambda d: carry_one(d, B))
    if shift >= 2:
        add("one below the tie stays", [0] * (L - 1) + [h - 1], extra=tie - 1)
        add("one below the negative tie rounds down to -1", [0] * L, extra=-tie - 1, want=lambda d: d[:-1] + [-1])
    for name, a in (("0", 0), ("q-1", Q - 1), ("floor(q/2)", Q // 2), ("floor(q/2)+1", (Q // 2 + 1) % Q)):
        out.append((name, a, None))
    return out


SEED = 7
UNIFORM_ROWS = 3          # behind the crafted rows


@functools.lru_cache(maxsize=None)
def rows(levels, base_log, q_bits, big_n=1024, seed=SEED):
    """(names, cts): the crafted ciphertext rows [rows][big_n + 1] of a shape, read-only, the same for every n and key.
    One row per crafted word with that word in EVERY mask coefficient (the all-extreme rows), one row cycling through the
    crafted words, a zero row, a row with only a body, then UNIFORM_ROWS uniform rows.  Bodies: the extremes 0, q - 1,
    floor(q/2) in turn, then uniform."""
    Q = MODULUS[q_bits]
    rng = np.random.default_rng([seed, levels, base_log, q_bits, big_n])
    words = crafted_words(levels, base_log, q_bits)
    names, cts = [], []
    bodies = [0, Q - 1, Q // 2]
    for i, (name, a, _) in enumerate(words):
        names.append("all " + name)
        cts.append([a] * big_n + [bodies[i] if i < 3 else int(rand_words(rng, 1, Q)[0])])
    names.append("crafted words in turn")
    cts.append([words[j % len(words)][1] for j in range(big_n)] + [int(rand_words(rng, 1, Q)[0])])
    names.append("zero row")
    cts.append([0] * (big_n + 1))
    names.append("body only")
    cts.append([0] * big_n + [int(rand_words(rng, 1, Q)[0])])
    cts = np.array(cts, dtype=np.uint64)
    uni = rand_words(rng, (UNIFORM_ROWS, big_n + 1), Q)
    names += [f"uniform {i}" for i in range(UNIFORM_ROWS)]
    cts = np.concatenate([cts, uni])
    cts.setflags(write=False)
    return tuple(names), cts


@functools.lru_cache(maxsize=None)
def crafted_digits(levels, base_log, q_bits, big_n=1024, seed=SEED):
    """mask_digits of rows(): computed once per shape and modulus, read-only"""
    D = mask_digits(rows(levels, base_log, q_bits, big_n, seed)[1], levels, base_log, q_bits)
    D.setflags(write=False)
    return D


def want_crafted(ksk, n, levels, base_log, q_bits, count=None, big_n=1024, seed=SEED):
    """the integer reference on the first `count` (default: all) rows of rows()"""
    cts = rows(levels, base_log, q_bits, big_n, seed)[1]
    cts = cts if count is None else cts[:count]
    return keyswitch(cts, ksk, n, levels, base_log, q_bits, D=crafted_digits(levels, base_log, q_bits, big_n, seed))


@functools.lru_cache(maxsize=None)
def batch(levels, base_log, q_bits, count, big_n=1024, seed=SEED):
    """`count` ciphertext rows, read-only: the crafted rows of rows() first (cut if count is smaller), uniform rows behind them"""
    _, head = rows(levels, base_log, q_bits, big_n, seed)
    if count <= head.shape[0]:
        cts = head[:count].copy()
    else:
        rng = np.random.default_rng([seed, levels, base_log, q_bits, big_n, count])
        cts = np.concatenate([head, rand_words(rng, (count - head.shape[0], big_n + 1), MODULUS[q_bits])])
    cts.setflags(write=False)
    return cts


def describe_mismatch(got, want, names=()):
    """rows whose words differ, with the first differing column of each (assertion message)"""
    bad = [i for i in range(want.shape[0]) if not np.array_equal(got[i], want[i])]
    lines = []
    for i in bad[:12]:
        x = int(np.flatnonzero(got[i] != want[i])[0])
        name = names[i] if i < len(names) else "uniform"
        lines.append(f"row {i} [{name}]: {int((got[i] != want[i]).sum())} of {want.shape[1]} words, first at column {x}: "
                     f"got {int(got[i, x])}, want {int(want[i, x])}")
    return f"{len(bad)} of {want.shape[0]} rows differ\n" + "\n".join(lines)


# ------------------------------------------------------------------------------------------------ the cases of the GPU file
BIG_N = 1024
COUNTS = (1, 7, 8, 9, 31, 32, 33, 97, 127, 128, 129)
BIG_COUNT = 4097              # one scalar tile row beyond 4,096: the unsplit scalar form by batch size
# ((levels, base_log), n) per modulus, one context each: big decompositions ride on small n (the oracle's work is
# rows x 1024 x levels x (n + 1)).  n = 1 carries (8, 4): 8 levels are the most the unsplit scalar form stages at N = 1024
# (exactly 64 KiB), and the 4,097-row batch reaches that form at the smallest n.  Every shape sits on some n <= 767, so the
# scalar kernel sees it; n = 768 and 1024 (matrix cores only) repeat the one-level shapes.
PAIRING = {
    64: (((8, 4), 1), ((21, 3), 31), ((17, 2), 32), ((16, 3), 255), ((9, 7), 256), ((6, 7), 511), ((5, 6), 512), ((3, 5), 767),
         ((1, 7), 31), ((1, 1), 32), ((1, 7), 768), ((1, 1), 1024)),
    49: (((8, 4), 1), ((17, 2), 31), ((16, 3), 32), ((3, 5), 255), ((5, 6), 256), ((6, 7), 511), ((1, 7), 512), ((1, 1), 767),
         ((1, 1), 31), ((1, 7), 768), ((1, 1), 1024)),          # (17, 2) has no matrix-core form: n = 31 once more for it
}
PAIRING[TORUS64] = PAIRING[64]


def shapes(q_bits):
    """the (levels, base_log) of a modulus, each once"""
    return sorted({shape for shape, _ in PAIRING[q_bits]})
MFMA_MAX_LEVELS = 16          # ks_mfma_ok: the digit kernel holds 16 digits
SCALAR_MAX_N = 767            # 3 x 256 output columns per workgroup
SCALAR_LDS_MAX = 64 * 1024    # bytes of staged digits per workgroup: 8 ciphertexts x coefficients of the slice x levels


def ring_depth(q_bits):
    """k-steps the matrix-core kernel keeps in flight: 4 with 7 key limbs (49-bit field), 3 with 9 (the 64-bit moduli)"""
    return 4 if q_bits == 49 else 3


def mfma_slices(count, n, levels, big_n=BIG_N):
    """ks_mfma_slices of csrc/bmi_host.cpp"""
    tiles, cbs, ksteps = (count + 31) // 32, (n + 1 + 31) // 32, big_n * levels // 32
    slices = 1
    while slices < 64 and slices * 2 <= ksteps and ksteps % (slices * 2) == 0 and tiles * cbs * slices < 2048:
        slices *= 2
    return slices


def scalar_slices(count, levels, pinned=False, big_n=BIG_N):
    """the slices of the scalar form in bmi_keyswitch_batch: by batch size (none under a pinned rotation variant other than 0 / 2),
    then doubled until the staged digits fit"""
    tiles, slices = (count + 7) // 8, 1
    if not pinned:
        while slices < 64 and tiles * slices * 2 <= 1024:
            slices *= 2
    while slices < 64 and 8 * -(-big_n // slices) * levels > SCALAR_LDS_MAX:
        slices *= 2
    return slices


def coverage(q_bits):
    """[(shape, n, count, path, slices, steps per slice, steps per slice mod ring depth or None)] of the dense cases: every
    context of PAIRING at every count of COUNTS on every path that takes it"""
    out = []
    for (levels, base_log), n in PAIRING[q_bits]:
        for count in COUNTS:
            if levels <= MFMA_MAX_LEVELS:
                s = mfma_slices(count, n, levels)
                steps = BIG_N * levels // 32 // s
                out.append(((levels, base_log), n, count, "mfma", s, steps, steps % ring_depth(q_bits)))
            if n <= SCALAR_MAX_N:
                out.append(((levels, base_log), n, count, "scalar", scalar_slices(count, levels), None, None))
    return out
