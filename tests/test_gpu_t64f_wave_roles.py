"""The wavefront roles of the torus throughput kernel (k_blind_rotate_t64f): which wavefront serves which ciphertext slot of a
workgroup, which input polynomial it owns, who its partner is, which 64 of the pair's 128 staging threads it is, and which
wavefront writes the mask and which the body of the output.

A wrong role assignment swaps or mixes ciphertext slots, or the two polynomials of one ciphertext.  The batches here are the
residues against four ciphertexts per workgroup with more than one workgroup that tests/test_gpu_pair_handoff.py leaves out
(2 and 6: two live pairs and two dead ones in the last workgroup; 7: three; 8: none; 9: one), at three and at two
decomposition levels and the default n = 630 (631 words to stage: ragged against the pair's 128 staging threads).  Consecutive
ciphertexts take alternating look-up tables (the identity and a seeded random one) and distinct messages, so every slot of a
workgroup holds different words and any swap changes the output.  From four ciphertexts on, the first workgroup also holds an
all-zero ciphertext (every exponent 0: no rotation at all), an all-ones ciphertext and one of uniformly random words beside an
encryption.

Every word of the throughput kernel (variant 5) must equal the latency kernel's (variant 6: one workgroup per ciphertext, no
roles to get wrong) and the oracle's integer arithmetic on every ciphertext, and every ciphertext that went in as an
encryption must decrypt to its table applied to its message."""
import numpy as np
import pytest

import pbs_cases as pc

pytestmark = pytest.mark.gpu

SEED = 0x5EED
QB = 65
LEVELS = [3, 2]
COUNTS = [2, 6, 7, 8, 9]
ZERO_ROW, ONES_ROW, RANDOM_ROW = 1, 2, 3     # slots of the first workgroup, batches of at least 4 (slot 0 stays an encryption)


@pytest.fixture(scope="module", params=LEVELS, ids=[f"l{l}" for l in LEVELS])
def ctx(request):
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=QB, bs_levels=request.param))
    e.keygen(SEED)
    try:
        with pc.oracle_for(e) as o:
            yield e, o.ctx
    finally:
        e.close()


@pytest.mark.parametrize("count", COUNTS)
def test_every_slot_keeps_its_own_ciphertext(ctx, count):
    eng, octx = ctx
    assert eng.P.n == 630 and eng.P.N == 1024
    rng = np.random.default_rng(7000 * eng.P.bs_levels + count)
    dl = eng.delta_log()
    tables = [np.arange(-8, 8), rng.integers(-8, 8, 16)]
    ids = np.array([eng.lut_register(t, 4, dl) for t in tables], np.uint32)
    tvs = np.stack([eng.lut_get(i) for i in ids])
    sel = (np.arange(count) & 1).astype(np.uint32)          # consecutive ciphertexts: alternating tables ...
    msgs = rng.permutation(np.arange(-8, 8))[:count]        # ... and distinct messages
    small = eng.keyswitch_host(eng.encrypt(msgs, dl))
    encrypted = np.ones(count, bool)
    if count >= 4:
        small[ZERO_ROW] = 0
        small[ONES_ROW] = np.uint64(0xFFFFFFFFFFFFFFFF)
        small[RANDOM_ROW] = pc.uniform_words(rng, small.shape[1])
        encrypted[[ZERO_ROW, ONES_ROW, RANDOM_ROW]] = False
    with pc.pinned_variant(eng, 5):
        got = eng.blind_rotate_host(small, ids[sel])
    with pc.pinned_variant(eng, 6):
        lat = eng.blind_rotate_host(small, ids[sel])
    assert np.array_equal(got, lat), "throughput kernel differs from the latency kernel"
    want = octx.blind_rotate(small, tvs, sel)
    assert np.array_equal(got, want), "throughput kernel differs from the oracle"
    dec = np.asarray(eng.decrypt(got, dl))
    expect = np.array([int(tables[s][m + 8]) for s, m in zip(sel, msgs)])
    assert np.array_equal(dec[encrypted], expect[encrypted]), "a ciphertext does not decrypt to its table applied to its message"
