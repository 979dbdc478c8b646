"""The library still makes the same words: SHA-256 digests of what the host cryptography (csrc/host_crypto.hpp, called from
csrc/bmi_host.cpp) generates on the default set of each modulus from a deterministic seed, against
tests/golden/host_crypto_digests.json - recorded from the commit BEFORE the cryptography moved into that header, with

    python tests/test_gpu_host_crypto_digests.py record [FILE]

(which writes the fixture, or FILE, from the library in the tree; the fixture holds digests only)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_crypto_digests.json")
SEED = 0x5EED
MODULI = {"torus64": 65, "field49": 49, "goldilocks": 64}
PUB_KEY = np.arange(1, 9, dtype=np.uint32) * np.uint32(0x9E3779B9)   # the public key of the CSPRNG-free seeded import


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).data).hexdigest()


def digests(q_bits):
    """every deterministic product of one context: the keys of keygen(SEED), eight encryptions, then (where the modulus has them) the
    unrolled key, the compression key of shape (1, 16) and the bodies of a seeded export that involves no CSPRNG - a server that
    imported these keys' own bodies under PUB_KEY"""
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=q_bits))
    try:
        e.keygen(SEED)
        sk_small, sk_big, bsk, ksk = e.export_keys()
        d = {"sk_small": sha(sk_small), "sk_big": sha(sk_big), "bsk": sha(bsk), "ksk": sha(ksk)}
        d["encryptions"] = sha(e.encrypt(np.arange(-4, 4), e.delta_log()))
        if q_bits == tfhe.TORUS64:
            e.compression_keygen(1, 16)
            d["compression_key"] = sha(e.export_compression_key())
            srv = tfhe.Engine(tfhe.default_params(q_bits=q_bits))
            try:
                srv.import_keys_seeded(PUB_KEY, bsk[:, :, -1, :], ksk[:, :, -1])
                _, bsk_body, ksk_body = srv.export_keys_seeded()
                d["seeded_bsk_bodies"], d["seeded_ksk_bodies"] = sha(bsk_body), sha(ksk_body)
            finally:
                srv.close()
        if q_bits != 64:   # (Goldilocks has no unrolled kernel: bmi_set_bsk_unroll refuses)
            e.set_bsk_unroll(2)   # keys held: the unrolled key of the same secret keys, from the seed's own streams
            d["bsk3"] = sha(e.export_bsk_unrolled())
        return d
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("modulus", sorted(MODULI))
def test_generated_words_are_the_recorded_ones(modulus):
    want = json.load(open(FIXTURE))[modulus]
    got = digests(MODULI[modulus])
    assert sorted(got) == sorted(want)
    assert got == want, [name for name in want if got[name] != want[name]]


if __name__ == "__main__" and sys.argv[1:2] == ["record"]:
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [here, os.path.join(here, "bounty-matrix-inversion_amd")]
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    json.dump({name: digests(q) for name, q in sorted(MODULI.items())}, open(out, "w"), indent=1, sort_keys=True)
    print("recorded", out)
