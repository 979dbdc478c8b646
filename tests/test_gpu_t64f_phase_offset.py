"""The torus throughput kernel (k_blind_rotate_t64f) at the start-up of its CMUX loop and under every load of a workgroup.

The eight wavefronts of a workgroup execute their per-CMUX hardware barrier at two sites: wavefronts 4-7 (group B) at the loop
head, wavefronts 0-3 (group A) between their forward transforms and their first product row, so that group A runs one forward
phase ahead of its SIMD-mates (EXPERIMENTS A22; the kernel's header comment).  The barrier only paces - no wavefront reads
another's LDS words across it - so a wavefront out of step cannot show as a wrong word through the barrier itself, only through
the pair hand-offs around it, or as a hang: every wavefront must execute exactly one barrier per step whatever its group, for
live and for dead pairs, from the first step on.
So the kernel runs here at n = 1, 2 (start-up: the lead is established in the first step), 7, 8, 9, 17 and the default 630, at
three and at two decomposition levels, on batches of 1 and 3 (dead pairs in the only workgroup: in group B alone, or a whole
group), 4 and 8 (one and two full workgroups), 5 and 9 (a last workgroup with one live pair beside three dead ones).  The short
step counts are the default parameter set with `n` overridden, as tests/test_gpu_shared_rotation.py does for n = 12; their
small ciphertexts come from the oracle's keyswitch.  (7, 8, 9 and 17 lie around the eighth and sixteenth step, where the
latency kernel they are compared with re-centres its accumulator.)  From
four ciphertexts on the first workgroup also holds an all-zero row (no rotation in any step), an all-ones row and a row of
uniformly random words beside an encryption.

Every word of the throughput kernel (variant 5) must equal the latency kernel's (variant 6: workgroup barriers for all its
wavefronts) and the oracle's integer arithmetic; the same batch run three times must give the same words; every encryption must
decrypt to its table applied to its message.  The accumulator-returning entry (the same loop under another epilogue) is held to
the same oracle words through the sample extraction, and to the latency kernel on all 2N words, at batches 1, 5 and 9."""
import numpy as np
import pytest

import pbs_cases as pc

pytestmark = pytest.mark.gpu

SEED = 0x5EED
QB = 65
LEVELS = [3, 2]
STEPS = [1, 2, 7, 8, 9, 17, 630]
COUNTS = [1, 3, 4, 5, 8, 9]
GLWE_COUNTS = [1, 5, 9]
ZERO_ROW, ONES_ROW, RANDOM_ROW = 1, 2, 3     # slots of the first workgroup, batches of at least 4 (slot 0 stays an encryption)

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


def extract(glwe, N):
    """sample extraction of coefficient 0 from accumulators [count][2N] (mask polynomial, then body)"""
    out = np.zeros((glwe.shape[0], N + 1), np.uint64)
    out[:, 0] = glwe[:, 0]
    out[:, 1:N] = np.uint64(0) - glwe[:, N - 1:0:-1]
    out[:, N] = glwe[:, N]
    return out


def batch(eng, octx, count):
    key = (eng.P.bs_levels, eng.P.n, count)
    if key not in _batches:
        rng = np.random.default_rng(7000 * eng.P.bs_levels + 10 * eng.P.n + count)
        dl = eng.delta_log()
        tables = [np.arange(-8, 8), rng.integers(-8, 8, 16)]
        ids = np.array([eng.lut_register(t, 4, dl) for t in tables], np.uint32)
        tvs = np.stack([eng.lut_get(i) for i in ids])
        sel = (np.arange(count) & 1).astype(np.uint32)
        msgs = rng.permutation(np.arange(-8, 8))[:count]
        small = octx.keyswitch(eng.encrypt(msgs, dl))
        encrypted = np.ones(count, bool)
        if count >= 4:
            small[ZERO_ROW] = 0
            small[ONES_ROW] = np.uint64(0xFFFFFFFFFFFFFFFF)
            small[RANDOM_ROW] = pc.uniform_words(rng, small.shape[1])
            encrypted[[ZERO_ROW, ONES_ROW, RANDOM_ROW]] = False
        want = octx.blind_rotate(small, tvs, sel)
        expect = np.array([int(tables[s][m + 8]) for s, m in zip(sel, msgs)])
        for a in (small, want):
            a.setflags(write=False)
        _batches[key] = (small, ids[sel], want, expect, encrypted, dl)
    return _batches[key]


@pytest.mark.parametrize("count", COUNTS)
def test_words_at_every_step_count_and_load(ctx, count):
    eng, octx = ctx
    assert eng.P.N == 1024
    small, ids, want, expect, encrypted, dl = batch(eng, octx, count)
    assert small.shape == (count, eng.P.n + 1)
    with pc.pinned_variant(eng, 5):
        runs = [eng.blind_rotate_host(small, ids) for _ in range(3)]
    got = runs[0]
    assert np.array_equal(runs[1], got) and np.array_equal(runs[2], got), "the same batch gives different words from run to run"
    with pc.pinned_variant(eng, 6):
        lat = eng.blind_rotate_host(small, ids)
    assert np.array_equal(got, lat), "throughput kernel differs from the latency kernel"
    assert np.array_equal(got, want), "throughput kernel differs from the oracle"
    dec = np.asarray(eng.decrypt(got, dl))
    assert np.array_equal(dec[encrypted], expect[encrypted]), "a ciphertext does not decrypt to its table applied to its message"


@pytest.mark.parametrize("count", GLWE_COUNTS)
def test_accumulator_entry_at_every_step_count(ctx, count):
    eng, octx = ctx
    small, ids, want, _, _, _ = batch(eng, octx, count)
    with pc.pinned_variant(eng, 5):
        glwe = eng.blind_rotate_glwe_host(small, ids)
    assert glwe.shape == (count, 2 * eng.P.N)
    assert np.array_equal(extract(glwe, eng.P.N), want), "the accumulator's extracted sample differs from the oracle"
    with pc.pinned_variant(eng, 6):
        lat = eng.blind_rotate_glwe_host(small, ids)
    assert np.array_equal(glwe, lat), "the accumulator differs from the latency kernel's"
