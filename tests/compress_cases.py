"""The independent reference of the compression of output ciphertexts (include/bmi_tfhe.h, csrc/lwe_pack.hip): a numpy restatement
of the scheme in integer arithmetic mod 2^64 - digits, exact product, rotation, centred modulus switch, phase - and the key and
encryption routines the CPU model test needs.  Shared by tests/test_compress_model.py (CPU) and tests/test_gpu_compress.py;
nothing here calls the library.

All words are numpy uint64 (wrap-around arithmetic); signed quantities are int64, whose sums wrap the same way."""
import numpy as np

U = np.uint64
ADVERSARIAL_WORDS = (0, 1 << 63, (1 << 63) - 1, (1 << 64) - 1)


def tie_words(levels, base_log):
    """words that sit exactly on a rounding tie of every level of the (levels, base_log) decomposition, on both sides of zero:
    the half of the last kept bit alone, and the same below a digit that is itself at its extreme"""
    out = []
    for lev in range(1, levels + 1):
        half_ulp = 1 << (64 - lev * base_log - 1) if lev * base_log < 64 else 0
        top = 1 << (64 - lev * base_log)
        for w in (half_ulp, (1 << 64) - half_ulp, top * ((1 << (base_log - 1)) - 1) + half_ulp, top * (1 << (base_log - 1)) + half_ulp,
                  top * (1 << (base_log - 1)), (1 << 64) - top * (1 << (base_log - 1))):
            out.append(w % (1 << 64))
    return np.array(out, dtype=U)


def digits(a, levels, base_log):
    """the digits of the words `a` by the oracle's rule (oracle/tfhe_oracle.c ora_decompose): centred lift, round half up to the
    top levels * base_log bits, balanced digits from the least significant one, the top digit absorbs the carry (so it ranges over
    [-2^(b-1), 2^(b-1)], both ends included).  Returns int64, shape a.shape + (levels,)."""
    c = np.asarray(a, dtype=U).view(np.int64)
    shift = 64 - levels * base_log
    r = (c >> np.int64(shift)) + ((c >> np.int64(shift - 1)) & np.int64(1))
    B, half = np.int64(1 << base_log), np.int64(1 << (base_log - 1))
    out = np.zeros(c.shape + (levels,), np.int64)
    for lev in range(levels - 1, 0, -1):
        d = r & (B - np.int64(1))
        r = r >> np.int64(base_log)
        carry = d >= half
        out[..., lev] = np.where(carry, d - B, d)
        r = r + carry.astype(np.int64)
    out[..., 0] = r
    return out


def exact_product(D, key):
    """D @ key mod 2^64 for small integers D [m][K] (|d| <= 2^15) and words key [K][W]: four float64 matrix products of D with
    the key's 16-bit limbs - every limb sum is below K * 2^15 * 2^16 <= 2^45 < 2^53, so float64 carries it exactly - recombined
    mod 2^64.  Rows of the key that meet only zero digits are left out."""
    D = np.asarray(D, dtype=np.int64)
    key = np.asarray(key, dtype=U)
    assert D.ndim == 2 and key.ndim == 2 and D.shape[1] == key.shape[0]
    assert np.abs(D).max(initial=0) <= 1 << 15 and key.shape[0] <= 1 << 14
    live = np.flatnonzero(np.any(D != 0, axis=0))
    Df = D[:, live].astype(np.float64)
    kl = key[live]
    out = np.zeros((D.shape[0], key.shape[1]), U)
    for p in range(4):
        limb = ((kl >> U(16 * p)) & U(0xFFFF)).astype(np.float64)
        s = Df @ limb
        out += s.astype(np.int64).view(U) << U(16 * p)
    return out


def lwe_to_glwe_rows(cts, key, levels, base_log):
    """T_i = (0, b_i X^0) - sum_{j,l} d[i][j][l] row(j, l) for the ciphertexts cts [m][N + 1]; key [N][levels][2][N] -> [m][2N]"""
    cts = np.asarray(cts, dtype=U)
    N = cts.shape[1] - 1
    D = digits(cts[:, :N], levels, base_log).reshape(cts.shape[0], N * levels)
    T = U(0) - exact_product(D, np.asarray(key, dtype=U).reshape(N * levels, 2 * N))
    T[:, N] += cts[:, N]
    return T


def rotate_sum(T, N):
    """(A, B) = sum_i X^i T_i, negacyclic, per component: coefficient c receives +T_i[c - i] for i <= c and -T_i[N + c - i] for
    i > c.  T [m][2N] -> [2N]"""
    acc = np.zeros(2 * N, U)
    for i in range(T.shape[0]):
        for comp in range(2):
            t = T[i, comp * N:(comp + 1) * N]
            seg = acc[comp * N:(comp + 1) * N]
            seg[i:] += t[:N - i]
            seg[:i] -= t[N - i:]
    return acc


def centred_switch(acc, N, m, log_modulus):
    """the centred modulus switch of one block (A | B) to log_modulus bits -> uint32 [N + m]: N mask values, m body values"""
    sh = 64 - log_modulus
    half, mask = U(1 << (sh - 1)), U((1 << sh) - 1)
    A, B = acc[:N], acc[N:]
    e = ((A + half) & mask).view(np.int64) - np.int64(1 << (sh - 1))
    P = np.cumsum(e, dtype=np.int64)
    corr = (np.int64(2) * P - P[-1]) >> np.int64(1)
    Bc = B - corr.view(U)
    omask = U((1 << log_modulus) - 1)
    a_hat = ((A + half) >> U(sh)) & omask
    b_hat = ((Bc + half) >> U(sh)) & omask
    return np.concatenate([a_hat, b_hat[:m]]).astype(np.uint32)


def compressed_words(count, N):
    return -(-count // N) * N + count


def compress(cts, key, levels, base_log, log_modulus):
    """the compressed form of the ciphertexts cts [count][N + 1]: blocks of N, each N mask values then its body values"""
    cts = np.asarray(cts, dtype=U)
    N = cts.shape[1] - 1
    out = []
    with np.errstate(over="ignore"):
        for t0 in range(0, cts.shape[0], N):
            blk = cts[t0:t0 + N]
            out.append(centred_switch(rotate_sum(lwe_to_glwe_rows(blk, key, levels, base_log), N), N, blk.shape[0], log_modulus))
    return np.concatenate(out) if out else np.zeros(0, np.uint32)


def negacyclic_by_binary(A, S):
    """A S mod X^N + 1 for a binary polynomial S (words mod 2^64)"""
    N = A.size
    out = np.zeros(N, U)
    with np.errstate(over="ignore"):
        for t in np.flatnonzero(S):
            out[t:] += A[:N - t]
            out[:t] -= A[N - t:]
    return out


def phase(words, count, N, log_modulus, S):
    """phase_i = B^_i 2^(64-c) - ((A^ 2^(64-c)) S)_i mod 2^64 of a compressed form under the binary GLWE key S"""
    words = np.asarray(words, dtype=np.uint32)
    up = U(64 - log_modulus)
    out = np.zeros(count, U)
    with np.errstate(over="ignore"):
        for t0 in range(0, count, N):
            m = min(N, count - t0)
            blk = words[(t0 // N) * 2 * N:][:N + m].astype(U)
            out[t0:t0 + m] = (blk[N:] << up) - negacyclic_by_binary(blk[:N] << up, S)[:m]
    return out


def decode(phases, delta_log):
    """round(phase / 2^delta_log) of centred phases, as bmi_decrypt"""
    v = np.asarray(phases, dtype=U).view(np.int64)
    return (v >> np.int64(delta_log)) + ((v >> np.int64(delta_log - 1)) & np.int64(1))


def uniform_words(rng, shape):
    return rng.integers(0, 1 << 63, shape, dtype=U) * U(2) + rng.integers(0, 2, shape, dtype=U)


def gaussian_words(rng, shape, sigma):
    """rounded Gaussian noise of standard deviation sigma (a fraction of the torus) as words mod 2^64"""
    if sigma == 0:
        return np.zeros(shape, U)
    return np.rint(rng.normal(0.0, sigma * 2.0 ** 64, shape)).astype(np.int64).view(U)


def rows_by_binary(A, S):
    """A_r S mod X^N + 1 for every row of A [rows][N] at once: (A S)_x = sum_j A_j C[j][x], C[j][x] = S[x - j] for x >= j and
    -S[N + x - j] otherwise, through exact_product"""
    N = S.size
    idx = (np.arange(N)[None, :] - np.arange(N)[:, None]) % N
    C = np.where(np.arange(N)[None, :] >= np.arange(N)[:, None], 1, -1) * np.asarray(S).astype(np.int64)[idx]
    return np.ascontiguousarray(exact_product(C.T, np.ascontiguousarray(np.asarray(A, dtype=U).T)).T)


def key_row_errors(key, S, base_log):
    """the signed errors (int64 words) of every row of a compression key [N][levels][2][N] under the binary GLWE key S: the row's
    phase B - A S minus its message S_j 2^(64 - base_log (l + 1)) X^0"""
    N, levels = key.shape[0], key.shape[1]
    flat = np.asarray(key, dtype=U).reshape(N * levels, 2, N)
    with np.errstate(over="ignore"):
        ph = flat[:, 1] - rows_by_binary(flat[:, 0], S)
        for lev in range(levels):
            ph[lev::levels, 0] -= np.asarray(S, dtype=U) << U(64 - base_log * (lev + 1))
    return ph.view(np.int64)


def make_key(rng, S, levels, base_log, sigma):
    """a compression key [N][levels][2][N] under the binary GLWE key S: row (j, l) = [A, A S + e + S_j 2^(64 - b (l + 1)) X^0]"""
    N = S.size
    A = uniform_words(rng, (N * levels, N))
    with np.errstate(over="ignore"):
        B = rows_by_binary(A, S) + gaussian_words(rng, (N * levels, N), sigma)
        for j in np.flatnonzero(S):
            for lev in range(levels):
                B[j * levels + lev, 0] += U(1 << (64 - base_log * (lev + 1)))
    return np.stack([A, B], axis=1).reshape(N, levels, 2, N)


def encrypt(rng, S, msgs, delta_log, sigma):
    """fresh LWE encryptions [count][N + 1] of the messages under the coefficient vector of S"""
    msgs = np.asarray(msgs, dtype=np.int64)
    a = uniform_words(rng, (msgs.size, S.size))
    with np.errstate(over="ignore"):
        b = (a * S.astype(U)[None, :]).sum(axis=1, dtype=U) + (msgs.view(U) << U(delta_log)) + gaussian_words(rng, msgs.size, sigma)
    return np.concatenate([a, b[:, None]], axis=1)


def mean_square_error(phases, msgs, delta_log):
    """mean square of (phase - message 2^delta_log), centred, as a fraction of the torus squared"""
    with np.errstate(over="ignore"):
        err = (np.asarray(phases, dtype=U) - (np.asarray(msgs, dtype=np.int64).view(U) << U(delta_log))).view(np.int64)
    return float(np.mean((err.astype(np.float64) / 2.0 ** 64) ** 2))
