"""The pair hand-off of the torus throughput kernel (k_blind_rotate_t64f: pair_sync.hpp, the hook of fftw::inverse).

The two wavefronts of a ciphertext exchange their partial sums through LDS tiles guarded by flags; the protocol decides WHEN a
tile may be overwritten, never what is computed.  So every output word must stay what it was - equal to the latency kernel's
(no hand-off at all: workgroup barriers) and to the oracle's integer arithmetic - at the batch shapes that stress the protocol:
dead pairs in the last workgroup (1, 3, 5, 255, 257, 1,023 are ragged against four ciphertexts per workgroup), one round per
compute unit and several (1,023 = 256 workgroups), at three and at two decomposition levels.  The latency kernel is compared on
every word of every ciphertext; the oracle (0.1 s per ciphertext on the CPU) on every ciphertext of the batches up to 5 and, beyond,
on the first workgroup, the whole of the last two workgroups and four random ciphertexts.

The rounding distance reported by bmi_fft_margin_host depends on every floating-point operation of the kernel and on their
order: it is compared to the last bit with the value recorded from the kernel before the hand-off was changed
(tests/golden/pair_handoff_margin.json, on inputs that are a pure function of the seeds below).  How it was recorded: the
library built from commit 89b29d3 (the parent of the hand-off change) was loaded in place of the product's, and
fft_margin_host run on margin_inputs() at both level counts; float.hex() of the two distances is the file
(profiles/pair_handoff_ab.txt, section 5)."""
import json
import os

import numpy as np
import pytest

import pbs_cases as pc

pytestmark = pytest.mark.gpu

SEED = 0x5EED
QB = 65
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_handoff_margin.json")
LEVELS = [3, 2]
MARGIN_COUNT = 257


def _engine(levels):
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=QB, bs_levels=levels))
    e.keygen(SEED)
    return e


def margin_inputs(eng):
    """the inputs of the recorded rounding distance: a pure function of the seeds (no encryption randomness)"""
    rng = np.random.default_rng(23)
    lid = eng.lut_register(rng.integers(-8, 8, 16), 4, eng.delta_log())
    small = pc.uniform_words(rng, (MARGIN_COUNT, eng.P.n + 1))
    small[1] = 0
    small[2] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return small, np.full(MARGIN_COUNT, lid, np.uint32)


@pytest.fixture(scope="module", params=LEVELS, ids=[f"l{l}" for l in LEVELS])
def ctx(request):
    e = _engine(request.param)   # (the two level counts the floating-point transform is certified for: shape_supported_fft)
    try:
        with pc.oracle_for(e) as o:
            yield e, o.ctx
    finally:
        e.close()


@pytest.mark.parametrize("count", [1, 3, 4, 5, 255, 257, 1023])
def test_throughput_kernel_equals_latency_kernel_and_oracle(ctx, count):
    eng, octx = ctx
    rng = np.random.default_rng(1000 * eng.P.bs_levels + count)
    tables = [np.arange(-8, 8), rng.integers(-8, 8, 16)]
    ids = np.array([eng.lut_register(t, 4, eng.delta_log()) for t in tables], np.uint32)
    tvs = np.stack([eng.lut_get(i) for i in ids])
    sel = rng.integers(0, 2, count).astype(np.uint32)
    msgs = rng.integers(-8, 8, count)
    small = eng.keyswitch_host(eng.encrypt(msgs, eng.delta_log()))
    # every other ciphertext of the first and of the last workgroup is random words: the partners of a pair then differ most
    for k in list(range(0, min(count, 4), 2)) + list(range(max(count - 4, 0), count, 2)):
        small[k] = pc.uniform_words(rng, (1, small.shape[1]))[0]
    with pc.pinned_variant(eng, 5):
        got = eng.blind_rotate_host(small, ids[sel])
    with pc.pinned_variant(eng, 6):
        lat = eng.blind_rotate_host(small, ids[sel])
    assert np.array_equal(got, lat), "throughput kernel differs from the latency kernel"
    if count <= 5:
        pick = np.arange(count)
    else:
        pick = np.unique(np.concatenate([np.arange(4), np.arange(count - 8, count), rng.integers(0, count, 4)]))
    want = octx.blind_rotate(small[pick], tvs, sel[pick])
    assert np.array_equal(got[pick], want), "throughput kernel differs from the oracle"


@pytest.mark.parametrize("levels", LEVELS, ids=[f"l{l}" for l in LEVELS])
def test_rounding_distance_unchanged_to_the_last_bit(levels):
    with open(GOLDEN) as f:
        recorded = json.load(f)[f"l{levels}"]
    e = _engine(levels)
    try:
        small, ids = margin_inputs(e)
        out, dist = e.fft_margin_host(small, ids)
        print(f"\nl = {levels}: rounding distance {dist.hex()} (recorded {recorded['distance_hex']})")
        assert dist.hex() == recorded["distance_hex"]
        with pc.pinned_variant(e, 6):
            lat = e.blind_rotate_host(small, ids)
        assert np.array_equal(out, lat)
    finally:
        e.close()
