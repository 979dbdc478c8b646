"""The stream of the seeded forms, on the CPU: bmi_seeded_mask_words (the specification the device kernel of csrc/chacha_expand.hip is
held to) against an independent numpy ChaCha20 (tests/seeded_cases.py), which is itself pinned to the test vector of RFC 7539."""
import numpy as np
import pytest

import seeded_cases as sc

# RFC 7539 section 2.3.2: key bytes 00 .. 1f, block counter 1, nonce 00:00:00:09 00:00:00:4a 00:00:00:00.  The RFC's state words
# 12 .. 15 are (counter, nonce words); in the 64-bit-counter variant used here they are (counter64 low, high, nonce64 low, high):
RFC_KEY = np.frombuffer(bytes(range(32)), dtype="<u4")
RFC_COUNTER64 = 1 | (0x09000000 << 32)
RFC_NONCE64 = 0x4A000000
RFC_BLOCK = [int(w, 16) for w in ("e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
                                  "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2").split()]


def test_numpy_reference_reproduces_rfc7539():
    got = sc.chacha_blocks(RFC_KEY, RFC_NONCE64, [RFC_COUNTER64])[0]
    assert [int(v) for v in got] == RFC_BLOCK
    words = sc.stream_words(RFC_KEY, RFC_NONCE64, 8 * RFC_COUNTER64, 8)
    assert [int(v) for v in words] == [RFC_BLOCK[2 * j] | (RFC_BLOCK[2 * j + 1] << 32) for j in range(8)]


def test_library_stream_reproduces_rfc7539():
    from bmi_amd import tfhe
    words = tfhe.seeded_mask_words(RFC_KEY, RFC_NONCE64, 8 * RFC_COUNTER64, 8)
    assert [int(v) for v in words] == [RFC_BLOCK[2 * j] | (RFC_BLOCK[2 * j + 1] << 32) for j in range(8)]


def test_published_domains():
    from bmi_amd import tfhe
    assert (tfhe.SEED_DOMAIN_BSK_MASK, tfhe.SEED_DOMAIN_KSK_MASK, tfhe.SEED_DOMAIN_ENC_MASK, tfhe.SEED_DOMAIN_BSK3_MASK) == \
        (sc.DOMAINS["bsk"], sc.DOMAINS["ksk"], sc.DOMAINS["enc"], sc.DOMAINS["bsk3"])
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bmi_tfhe.h")).read()
    for name, dom in (("BSK", "bsk"), ("KSK", "ksk"), ("ENC", "enc"), ("BSK3", "bsk3")):
        assert re.search(rf"#define BMI_SEED_DOMAIN_{name}_MASK {sc.DOMAINS[dom]}u\b", header), name


@pytest.mark.parametrize("domain", sorted(sc.DOMAINS))
@pytest.mark.parametrize("row", [0, 5, (1 << 32) - 1, 1 << 32, (1 << 56) - 1])
def test_library_stream_equals_reference(domain, row):
    """random keys; a nonce of every domain; rows whose low 32 bits wrap; starts that are no multiple of 8; counts around a block
    and the default n = 630 = 78 * 8 + 6"""
    from bmi_amd import tfhe
    rng = np.random.default_rng(sc.DOMAINS[domain] * 1000003 + row % 1000003)
    key = rng.integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32)
    nonce = sc.row_nonce(domain, row)
    for first in (0, 3, 8, 13, 1024 * 8 + 5):
        for count in (0, 1, 7, 8, 9, 630):
            got = tfhe.seeded_mask_words(key, nonce, first, count)
            assert got.dtype == np.uint64 and got.size == count
            assert np.array_equal(got, sc.stream_words(key, nonce, first, count)), (domain, row, first, count)


def test_prefix_property():
    """word j of a row does not depend on where the request started: any window is a slice of the row"""
    from bmi_amd import tfhe
    key = np.arange(8, dtype=np.uint32) * np.uint32(0x9E3779B9)
    whole = tfhe.seeded_mask_words(key, sc.row_nonce("ksk", 77), 0, 700)
    for first, count in ((1, 699), (629, 1), (624, 6), (7, 9)):
        assert np.array_equal(tfhe.seeded_mask_words(key, sc.row_nonce("ksk", 77), first, count), whole[first:first + count])
