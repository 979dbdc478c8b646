"""The torus throughput kernel (k_blind_rotate_t64f) in the row order "both limbs' products before the inverses".

Per CMUX a wavefront multiplies all 4 L key rows - (limb 0, partner's column), (limb 0, own column), (limb 1, partner's), (limb 1,
own) - publishes two partial sums through its one tile and runs both inverse transforms afterwards; limb 0's result waits in
registers and the accumulator is recombined once.  The order decides WHEN a tile may be written and which registers hold what,
never what is computed: every floating-point operation of a limb sum and of a transform, and their order, are those of the kernel
before.  tests/test_pair_handoff_order_model.py holds the hand-off protocol; here the kernel itself runs where that protocol can
go wrong: one CMUX (n = 1: every flag value used once), two and three (the forward exchanges of step i + 1 write the tile whose
last acknowledgement belongs to step i) and five, at three and at two levels, on batches of 1 and 3 (dead pairs in the only
workgroup), 4 (a full workgroup), 5 and 9 (a last workgroup with one live pair beside three dead ones).  From four ciphertexts on
the first workgroup holds an all-zero row, an all-ones row and a row of uniformly random words beside an encryption.  n = 630
is left to tests/test_gpu_pair_handoff.py, tests/test_gpu_t64f_phase_offset.py and tests/test_gpu_t64f_exchange_order.py.

Every word of the throughput kernel (variant 5) must equal the latency kernel's (variant 6) and the oracle's; the same batch run
three times must give the same words; the accumulator-returning entry at batches 1, 5 and 9 must equal the latency kernel's on
all 2N words.

The rounding distance reported by bmi_fft_margin_host depends on every floating-point operation of the kernel and on their order:
at every (levels, n, batch) above it must equal, to the last bit, the value of the kernel BEFORE the row order changed.  How
tests/golden/limb_order_margin.json was recorded (as profiles/pair_handoff_ab.txt, section 5, describes for the hand-off change):
the library built from the parent commit of the change (6552fd5) was loaded in place of the product's and fft_margin_host run on
margin_inputs() - a pure function of the seeds below, no encryption randomness - for each key "l<levels>-n<n>-c<batch>";
float.hex() of the distance is the value (profiles/limb_order_ab.txt, section 6)."""
import json
import os

import numpy as np
import pytest

import pbs_cases as pc

pytestmark = pytest.mark.gpu

SEED = 0x5EED
QB = 65
LEVELS = [3, 2]
STEPS = [1, 2, 3, 5]
COUNTS = [1, 3, 4, 5, 9]
GLWE_COUNTS = [1, 5, 9]
ZERO_ROW, ONES_ROW, RANDOM_ROW = 1, 2, 3     # slots of the first workgroup, batches of at least 4 (slot 0 stays an encryption)
GOLDEN = os.path.join(pc.GOLDEN_DIR, "limb_order_margin.json")

_batches = {}    # (levels, n, count) -> the batch and the oracle's words, computed once and left unchanged


@pytest.fixture(scope="module", params=[(l, n) for l in LEVELS for n in STEPS], ids=lambda p: f"l{p[0]}-n{p[1]}")
def ctx(request):
    from bmi_amd import tfhe
    levels, n = request.param
    e = tfhe.Engine(tfhe.default_params(q_bits=QB, bs_levels=levels, n=n))
    e.keygen(SEED)
    try:
        with pc.oracle_for(e) as o:
            yield e, o.ctx
    finally:
        e.close()


def batch(eng, octx, count):
    key = (eng.P.bs_levels, eng.P.n, count)
    if key not in _batches:
        rng = np.random.default_rng(9000 * eng.P.bs_levels + 10 * eng.P.n + count)
        dl = eng.delta_log()
        tables = [np.arange(-8, 8), rng.integers(-8, 8, 16)]
        ids = np.array([eng.lut_register(t, 4, dl) for t in tables], np.uint32)
        tvs = np.stack([eng.lut_get(i) for i in ids])
        sel = (np.arange(count) & 1).astype(np.uint32)
        small = octx.keyswitch(eng.encrypt(rng.permutation(np.arange(-8, 8))[:count], dl))
        if count >= 4:
            small[ZERO_ROW] = 0
            small[ONES_ROW] = np.uint64(0xFFFFFFFFFFFFFFFF)
            small[RANDOM_ROW] = pc.uniform_words(rng, small.shape[1])
        want = octx.blind_rotate(small, tvs, sel)
        for a in (small, want):
            a.setflags(write=False)
        _batches[key] = (small, ids[sel], want)
    return _batches[key]


def margin_key(levels, n, count):
    return f"l{levels}-n{n}-c{count}"


def margin_inputs(eng, count):
    """the inputs of the recorded rounding distances: a pure function of the seeds (no encryption randomness) - uniformly random
    words, which drive the digits to their full range, with the zero and the all-ones row from four ciphertexts on"""
    rng = np.random.default_rng(31000 + 1000 * eng.P.bs_levels + 10 * eng.P.n + count)
    lid = eng.lut_register(rng.integers(-8, 8, 16), 4, eng.delta_log())
    small = pc.uniform_words(rng, (count, eng.P.n + 1))
    if count >= 4:
        small[ZERO_ROW] = 0
        small[ONES_ROW] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return small, np.full(count, lid, np.uint32)


@pytest.mark.parametrize("count", COUNTS)
def test_words_equal_latency_kernel_and_oracle(ctx, count):
    eng, octx = ctx
    assert eng.P.N == 1024
    small, ids, want = batch(eng, octx, count)
    assert small.shape == (count, eng.P.n + 1)
    with pc.pinned_variant(eng, 5):
        runs = [eng.blind_rotate_host(small, ids) for _ in range(3)]
    got = runs[0]
    assert np.array_equal(runs[1], got) and np.array_equal(runs[2], got), "the same batch gives different words from run to run"
    with pc.pinned_variant(eng, 6):
        lat = eng.blind_rotate_host(small, ids)
    assert np.array_equal(got, lat), "throughput kernel differs from the latency kernel"
    assert np.array_equal(got, want), "throughput kernel differs from the oracle"


@pytest.mark.parametrize("count", GLWE_COUNTS)
def test_accumulator_entry_equals_latency_kernel(ctx, count):
    eng, octx = ctx
    small, ids, _ = batch(eng, octx, count)
    with pc.pinned_variant(eng, 5):
        glwe = eng.blind_rotate_glwe_host(small, ids)
    assert glwe.shape == (count, 2 * eng.P.N)
    with pc.pinned_variant(eng, 6):
        lat = eng.blind_rotate_glwe_host(small, ids)
    assert np.array_equal(glwe, lat), "the accumulator differs from the latency kernel's"


@pytest.mark.parametrize("count", COUNTS)
def test_rounding_distance_unchanged_to_the_last_bit(ctx, count):
    eng, _ = ctx
    with open(GOLDEN) as f:
        recorded = json.load(f)[margin_key(eng.P.bs_levels, eng.P.n, count)]
    small, ids = margin_inputs(eng, count)
    with pc.pinned_variant(eng, 5):
        out, dist = eng.fft_margin_host(small, ids)
    print(f"\n{margin_key(eng.P.bs_levels, eng.P.n, count)}: rounding distance {dist.hex()} (recorded {recorded})")
    assert dist.hex() == recorded
    with pc.pinned_variant(eng, 6):
        lat = eng.blind_rotate_host(small, ids)
    assert np.array_equal(out, lat)
