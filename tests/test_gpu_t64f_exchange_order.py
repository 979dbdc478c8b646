"""The order of LDS stores and reads inside the torus throughput kernel (k_blind_rotate_t64f): the exchanges of its transforms
(fft_wave_f64.hpp) and the publication of the partner's partial sum.

The inverse transforms issue each pair of stores of an exchange as soon as its values are finished, from inside the DFT8 that
produces them and around the wait for the partner's acknowledgement, instead of eight stores in a row after it (EXPERIMENTS A20;
the other exchanges were tried in the same form).  What can go wrong with that: a store to a tile is issued before an earlier read of the tile
has been served - a read by the wavefront itself, or by the partner before its acknowledgement - or the publication flag
overtakes the stores of the partial it announces.  Such faults are wrong words under uneven load, not crashes.  So the batches
here load the workgroups unevenly - 1 (one live pair beside three dead ones), 3 (three live, one dead), 4 (a full workgroup),
5 (a full workgroup and one live pair), 12 (three full workgroups) - at three and at two decomposition levels, the default
n = 630, N = 1024 and the seeded keys.  Consecutive ciphertexts take alternating look-up tables and distinct messages; from four
ciphertexts on, the first workgroup also holds an all-zero row (no rotation in any step), an all-ones row and a row of uniformly
random words beside an encryption, as in tests/test_gpu_t64f_wave_roles.py.

Every word of the throughput kernel (variant 5) must equal the latency kernel's (variant 6: workgroup barriers, no tiles shared
between wavefronts outside them) and the oracle's integer arithmetic; every encryption must decrypt to its table applied to its
message; and the same batch run three times in a row must give the same words each time (a hand-off race shows first as a
run-to-run difference).

The rounding distance reported by bmi_fft_margin_host (the STATS build of the same kernel) depends on every floating-point
operation and on their order, none of which moved: on margin_inputs() - 8 rows, a pure function of the seeds - it must equal, to
the last bit, the value recorded from the library built from the parent of this change (6e5f9e4), loaded in place of the
product's in the same GPU session (profiles/exchange_bubbles_ab.txt, section 0):
    l = 3: 0x1.4000000000000p-12      l = 2: 0x1.0000000000000p-12
(The 257-row values of tests/golden/pair_handoff_margin.json, which A19 found unchanged, are held by tests/test_gpu_pair_handoff.py.)"""
import numpy as np
import pytest

import pbs_cases as pc

pytestmark = pytest.mark.gpu

SEED = 0x5EED
QB = 65
LEVELS = [3, 2]
COUNTS = [1, 3, 4, 5, 12]
ZERO_ROW, ONES_ROW, RANDOM_ROW = 1, 2, 3     # slots of the first workgroup, batches of at least 4 (slot 0 stays an encryption)
MARGIN_COUNT = 8
PARENT_DISTANCE = {3: "0x1.4000000000000p-12", 2: "0x1.0000000000000p-12"}   # float.hex() of the parent's distances on margin_inputs()


def margin_inputs(eng):
    """the inputs of the recorded rounding distance: a pure function of the seeds (no encryption randomness)"""
    rng = np.random.default_rng(29)
    lid = eng.lut_register(rng.integers(-8, 8, 16), 4, eng.delta_log())
    small = pc.uniform_words(rng, (MARGIN_COUNT, eng.P.n + 1))
    small[ZERO_ROW] = 0
    small[ONES_ROW] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return small, np.full(MARGIN_COUNT, lid, np.uint32)


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
def test_words_under_uneven_load(ctx, count):
    eng, octx = ctx
    assert eng.P.n == 630 and eng.P.N == 1024
    rng = np.random.default_rng(9000 * eng.P.bs_levels + count)
    dl = eng.delta_log()
    tables = [np.arange(-8, 8), rng.integers(-8, 8, 16)]
    ids = np.array([eng.lut_register(t, 4, dl) for t in tables], np.uint32)
    tvs = np.stack([eng.lut_get(i) for i in ids])
    sel = (np.arange(count) & 1).astype(np.uint32)
    msgs = rng.permutation(np.arange(-8, 8))[:count]
    small = eng.keyswitch_host(eng.encrypt(msgs, dl))
    encrypted = np.ones(count, bool)
    if count >= 4:
        small[ZERO_ROW] = 0
        small[ONES_ROW] = np.uint64(0xFFFFFFFFFFFFFFFF)
        small[RANDOM_ROW] = pc.uniform_words(rng, small.shape[1])
        encrypted[[ZERO_ROW, ONES_ROW, RANDOM_ROW]] = False
    with pc.pinned_variant(eng, 5):
        runs = [eng.blind_rotate_host(small, ids[sel]) for _ in range(3)]
    got = runs[0]
    assert np.array_equal(runs[1], got) and np.array_equal(runs[2], got), "the same batch gives different words from run to run"
    with pc.pinned_variant(eng, 6):
        lat = eng.blind_rotate_host(small, ids[sel])
    assert np.array_equal(got, lat), "throughput kernel differs from the latency kernel"
    want = octx.blind_rotate(small, tvs, sel)
    assert np.array_equal(got, want), "throughput kernel differs from the oracle"
    dec = np.asarray(eng.decrypt(got, dl))
    expect = np.array([int(tables[s][m + 8]) for s, m in zip(sel, msgs)])
    assert np.array_equal(dec[encrypted], expect[encrypted]), "a ciphertext does not decrypt to its table applied to its message"


def test_rounding_distance_is_the_parents_to_the_last_bit(ctx):
    eng, _ = ctx
    small, ids = margin_inputs(eng)
    out, dist = eng.fft_margin_host(small, ids)
    recorded = PARENT_DISTANCE[eng.P.bs_levels]
    print(f"\nl = {eng.P.bs_levels}: rounding distance {dist.hex()} (parent {recorded})")
    assert dist.hex() == recorded
    with pc.pinned_variant(eng, 6):
        lat = eng.blind_rotate_host(small, ids)
    assert np.array_equal(out, lat)
