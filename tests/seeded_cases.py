"""The independent reference of the seeded forms: ChaCha20 (D. J. Bernstein's variant: 64-bit block counter in state words 12 / 13,
64-bit nonce in 14 / 15) in numpy, vectorised over blocks, and the stream words / row nonces built on it.  Shared by
tests/test_seeded_stream.py (CPU) and tests/test_gpu_seeded_keys.py; nothing here calls the library."""
import numpy as np

DOMAINS = {"bsk": 3, "ksk": 5, "enc": 7, "bsk3": 9}      # include/bmi_tfhe.h BMI_SEED_DOMAIN_*
_CONSTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)


def chacha_blocks(key, nonce, counters):
    """key: 8 uint32 words, nonce: 64-bit int, counters: 64-bit block counters -> (blocks, 16) uint32 output words"""
    c = np.atleast_1d(np.asarray(counters, dtype=np.uint64))
    full = lambda v: np.full(c.shape, v, np.uint32)   # noqa: E731
    st = [full(v) for v in _CONSTS] + [full(int(v)) for v in key] + \
         [(c & np.uint64(0xFFFFFFFF)).astype(np.uint32), (c >> np.uint64(32)).astype(np.uint32),
          full(nonce & 0xFFFFFFFF), full(nonce >> 32)]
    x = [s.copy() for s in st]
    rotl = lambda v, n: (v << np.uint32(n)) | (v >> np.uint32(32 - n))   # noqa: E731

    def qr(a, b, cc, d):
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16)   # noqa: E702
        x[cc] += x[d]; x[b] = rotl(x[b] ^ x[cc], 12)   # noqa: E702
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8)   # noqa: E702
        x[cc] += x[d]; x[b] = rotl(x[b] ^ x[cc], 7)   # noqa: E702
    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)   # noqa: E702
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)   # noqa: E702
    return np.stack([x[i] + st[i] for i in range(16)], axis=-1)


def stream_words(key, nonce, first_word, count):
    """64-bit words first_word .. first_word + count of the stream (key, nonce): word j = output words (2 (j % 8), 2 (j % 8) + 1)
    of block j // 8, low word first"""
    if count == 0:
        return np.zeros(0, np.uint64)
    b0, b1 = first_word // 8, (first_word + count - 1) // 8
    blocks = chacha_blocks(key, nonce, np.arange(b0, b1 + 1, dtype=np.uint64)).astype(np.uint64)
    words = (blocks[:, 0::2] | (blocks[:, 1::2] << np.uint64(32))).reshape(-1)
    return words[first_word - 8 * b0: first_word - 8 * b0 + count]


def row_nonce(domain, row):
    return (DOMAINS[domain] << 56) | (row & ((1 << 56) - 1))


def row_masks(key, domain, row, count):
    """the first `count` mask words of row `row` of a key or ciphertext array"""
    return stream_words(key, row_nonce(domain, row), 0, count)
