"""The independent reference of the decompression of compressed ciphertexts back to big-key LWE ciphertexts (include/bmi_tfhe.h,
csrc/lwe_unpack.hip): a numpy restatement of the rule in integer arithmetic mod 2^64.  Shared by tests/test_decompress_model.py (CPU)
and tests/test_gpu_decompress.py; nothing here calls the library, the rest (keys, encryption, compression, phase) is
tests/compress_cases.py.

With Sh = 64 - log_modulus, i = idx[r] mod N and A^ / B^ the N mask values and the body values of block idx[r] / N:
    out[r][j] = (A^[i - j] << Sh)            for j <= i
    out[r][j] = 0 - (A^[N + i - j] << Sh)    for i < j < N
    out[r][N] = B^[i] << Sh
the negacyclic sample extraction of coefficient i, whose LWE phase out[r][N] - sum_j out[r][j] S_j is compress_cases.phase of
position idx[r] bit for bit."""
import numpy as np

import compress_cases as cc

U = cc.U


def decompress(words, count, N, log_modulus, index=None):
    """the compressed form `words` of `count` ciphertexts -> [rows][N + 1] uint64: row r = position index[r] (None: all, in order);
    values are taken mod 2^log_modulus"""
    words = np.asarray(words, dtype=np.uint32).reshape(-1)
    assert words.size == cc.compressed_words(count, N)
    index = np.arange(count, dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64).reshape(-1)
    assert index.size == 0 or (index.min() >= 0 and index.max() < count)
    sh = U(64 - log_modulus)
    vals = (words.astype(U) & U((1 << log_modulus) - 1)) << sh
    out = np.zeros((index.size, N + 1), U)
    j = np.arange(N)
    with np.errstate(over="ignore"):
        for r, idx in enumerate(index.tolist()):
            blk = vals[(idx // N) * 2 * N:]
            i = idx % N
            a = blk[(i - j) % N]
            out[r, :N] = np.where(j <= i, a, U(0) - a)
            out[r, N] = blk[N + i]
    return out


def lwe_phase(cts, S):
    """b - <a, S> mod 2^64 of ciphertexts [rows][N + 1] under the binary key S"""
    cts = np.asarray(cts, dtype=U)
    with np.errstate(over="ignore"):
        return cts[:, -1] - (cts[:, :-1] * np.asarray(S, dtype=U)[None, :]).sum(axis=1, dtype=U)


def random_compressed(rng, count, N, log_modulus, shift=0):
    """uniformly random compressed values, with the words 0, 2^c - 1 and 2^(c-1) planted at mask positions 0 and N - 1 of the first
    and the last block and in the first and the last body; shift = 0, 1, 2 puts each of the three words at each place once"""
    words = rng.integers(0, 1 << log_modulus, cc.compressed_words(count, N), dtype=np.uint64).astype(np.uint32)
    if count == 0:
        return words
    edge = [0, (1 << log_modulus) - 1, 1 << (log_modulus - 1)]
    last = ((count - 1) // N) * 2 * N
    for k, at in enumerate((0, N - 1, N, last, last + N - 1, words.size - 1)):
        words[at] = edge[(k + shift) % 3]
    return words
