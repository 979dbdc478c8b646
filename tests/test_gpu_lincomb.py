"""The two leveled kernels around the PBS of every level of the encrypted inverse, and the in-place form of the PBS itself:
k_lincomb (csrc/ks_lincomb.hpp) against the Python-integer reference of tests/lincomb_cases.py on every modulus and width
(column blocks beyond the first, the large-coefficient branch of each field policy, 128-bit totals of either sign, the
executor's pointer arithmetic), k_scatter_rows (csrc/bmi_kernels.hip) and bmi_pbs_batch with d_out == d_in.
Word for word: no tolerance.  The lincomb and scatter tests need a context only, no keys."""
import numpy as np
import pytest

import lincomb_cases as lc

pytestmark = pytest.mark.gpu

SEED = 20
KEY_SEED = 0x5EED
SENTINEL = 0xDEADBEEFCAFEF00D      # above the 49-bit modulus; no output word of the table equals it

# name -> (parameter set, ciphertext width k N + 1)
CONTEXTS = {
    "goldilocks64-N1024": (lambda t: t.default_params(q_bits=64), 1025),
    "p49-N1024": (lambda t: t.default_params(q_bits=49, log_N=10), 1025),
    "p49-N2048": (lambda t: t.default_params(q_bits=49, log_N=11), 2049),
    "p49-N4096": (lambda t: t.default_params(q_bits=49, log_N=12), 4097),
    "torus64-N1024": (lambda t: t.preset_params("north_star_torus64"), 1025),
    "secure128_torus-N2048": (lambda t: t.preset_params("secure128_torus"), 2049),
    "secure128_torus_wide-N4096": (lambda t: t.preset_params("secure128_torus_wide"), 4097),
}


@pytest.fixture(scope="module")
def engines():
    """key-less contexts by name, created on first use and closed with the module"""
    from bmi_amd import tfhe
    made = {}

    def get(name):
        if name not in made:
            params, width = CONTEXTS[name]
            made[name] = tfhe.Engine(params(tfhe))
            assert made[name].P.big == width
        return made[name]
    yield get
    for e in made.values():
        e.close()


def dev_i64(a):
    """uint64 / int64 host array -> int64 device tensor holding the same words"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to("cuda:0")


def dev_i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to("cuda:0")


def sentinel_rows(rows, width):
    import torch
    return torch.full((rows, width), int(np.uint64(SENTINEL).astype(np.int64)), dtype=torch.int64, device="cuda:0")


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_lincomb_matches_integer_reference(engines, name):
    import torch
    eng = engines(name)
    Q, width = eng.modulus, eng.P.big
    store, row_ptr, idx, coef, consts, want = lc.build(Q, width, SEED)
    names = lc.case_names(Q, SEED)
    count = want.shape[0]
    d_store, d_rp, d_ix, d_cf, d_cs = dev_i64(store), dev_i32(row_ptr), dev_i32(idx), dev_i64(coef), dev_i64(consts)
    d_out = sentinel_rows(count + 2, width)           # one guard row before and one after the rows written
    eng.lincomb(d_store, d_rp, d_ix, d_cf, d_cs, count, d_out[1:], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = host_u64(d_out)
    got = out[1:count + 1]
    assert np.array_equal(got, want), lc.describe_mismatch(got, want, names)
    assert (out[0] == np.uint64(SENTINEL)).all() and (out[count + 1] == np.uint64(SENTINEL)).all()
    assert np.array_equal(host_u64(d_store), store)
    if Q < 1 << 64:
        assert (got < np.uint64(Q)).all()


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_lincomb_sliced_like_the_executor(engines, name):
    """Executor.run calls a level in slices: row_ptr, const_body and out advanced by the slice's first row, idx and coef whole -
    so the second call's row_ptr[0] is not 0.  On a stream of its own; a second pass over the filled buffer gives the same
    words (the kernel overwrites, it does not accumulate); an empty batch with valid pointers writes nothing."""
    import torch
    eng = engines(name)
    Q, width = eng.modulus, eng.P.big
    store, row_ptr, idx, coef, consts, want = lc.build(Q, width, SEED)
    names = lc.case_names(Q, SEED)
    count = want.shape[0]
    r = count // 2
    assert 0 < r < count and row_ptr[r] != 0
    d_store, d_rp, d_ix, d_cf, d_cs = dev_i64(store), dev_i32(row_ptr), dev_i32(idx), dev_i64(coef), dev_i64(consts)
    d_out = sentinel_rows(count + 2, width)
    d_empty = sentinel_rows(3, width)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    assert s != torch.cuda.default_stream().cuda_stream
    for sync in (lambda: eng.sync(s), torch.cuda.synchronize):
        eng.lincomb(d_store, d_rp, d_ix, d_cf, d_cs, r, d_out[1:], s)
        eng.lincomb(d_store, d_rp[r:], d_ix, d_cf, d_cs[r:], count - r, d_out[1 + r:], s)
        sync()
        out = host_u64(d_out)
        got = out[1:count + 1]
        assert np.array_equal(got, want), lc.describe_mismatch(got, want, names)
        assert (out[0] == np.uint64(SENTINEL)).all() and (out[count + 1] == np.uint64(SENTINEL)).all()
    eng.lincomb(d_store, d_rp[r:], d_ix, d_cf, d_cs[r:], 0, d_empty[1:], s)
    eng.sync(s)
    assert (host_u64(d_empty) == np.uint64(SENTINEL)).all()
    assert np.array_equal(host_u64(d_store), store)


@pytest.mark.parametrize("name", ["goldilocks64-N1024", "secure128_torus-N2048", "p49-N4096"])
def test_scatter_rows(engines, name):
    """store[rows[i]] = src[i]: one kernel for every modulus, so one context per width.  Nine distinct source rows into a
    16-row store, first and last row among the targets; the row list both on its own and as a pointer into the middle of a
    longer array (the executor passes d_rows[pos:]), whose leading entries name rows that must stay untouched."""
    import torch
    eng = engines(name)
    Q, width = eng.modulus, eng.P.big
    src = np.concatenate([lc.to_u64(lc.store_rows(Q, width, SEED)[5:12]), lc.to_u64(lc.store_rows(Q, width, SEED + 1)[7:9])])
    assert src.shape == (9, width) and len({row.tobytes() for row in src}) == 9
    rows = np.array([15, 3, 0, 8, 12, 1, 7, 10, 5], np.uint32)
    untouched = sorted(set(range(16)) - set(int(x) for x in rows))
    assert len(untouched) == 7
    longer = np.concatenate([np.array(untouched[:4], np.uint32), rows, np.array(untouched[4:], np.uint32)])
    d_src, d_rows, d_longer = dev_i64(src), dev_i32(rows), dev_i32(longer)
    s = torch.cuda.current_stream().cuda_stream
    for d_list in (d_rows, d_longer[4:]):
        d_store = sentinel_rows(16, width)
        eng.scatter_rows(d_src, 0, d_store, d_list, s)
        torch.cuda.synchronize()
        assert (host_u64(d_store) == np.uint64(SENTINEL)).all()       # an empty batch writes nothing
        eng.scatter_rows(d_src, 9, d_store, d_list, s)
        torch.cuda.synchronize()
        store = host_u64(d_store)
        for i, target in enumerate(rows):
            assert np.array_equal(store[target], src[i]), (i, int(target))
        assert (store[untouched] == np.uint64(SENTINEL)).all()
        assert np.array_equal(host_u64(d_src), src)


@pytest.fixture(scope="module", params=[64, 49, 65], ids=["goldilocks64", "p49_f64", "torus64"])
def keyed(request):
    """the three moduli at the default set, with keys"""
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=request.param))
    e.keygen(KEY_SEED)
    yield e
    e.close()


# Both batch sizes take the latency blind-rotation kernel (count <= 512).  The keyswitch is the matrix-core form at every batch
# size unless the scalar kernel is selected (set_keyswitch_variant(1): K-split partial sums + the reduce kernel at B = 5).
@pytest.mark.parametrize("B,ks_variant", [(5, 1), (5, 0), (70, 0)],
                         ids=["B5-scalar-keyswitch", "B5-matrix-core-keyswitch", "B70-matrix-core-keyswitch-ragged-tile"])
def test_pbs_batch_in_place(keyed, B, ks_variant):
    """include/bmi_tfhe.h: "d_in/d_out ... may alias".  The in-place call returns the words of the out-of-place call on a copy
    of the same inputs, which it leaves unchanged - through the scalar keyswitch kernel and through the matrix-core one (one
    ragged tile of 32 at B = 5, two full tiles and a ragged one at B = 70)."""
    import torch
    eng = keyed
    rng = np.random.default_rng(21 + B)
    dl = eng.delta_log()
    table = rng.integers(-8, 8, 16)
    lid = eng.lut_register(table, 4, dl)
    msgs = rng.integers(-8, 8, B)
    ct = eng.encrypt(msgs, dl)
    d_x = dev_i64(ct)
    d_copy = d_x.clone()
    d_out = sentinel_rows(B, eng.P.big)
    d_ids = torch.full((B,), lid, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    eng.set_keyswitch_variant(ks_variant)
    try:
        eng.pbs(d_copy, d_ids, B, d_out, s)
        eng.pbs(d_x, d_ids, B, d_x, s)
        torch.cuda.synchronize()
    finally:
        eng.set_keyswitch_variant(0)
    want = host_u64(d_out)
    assert np.array_equal(host_u64(d_x), want)
    assert np.array_equal(host_u64(d_copy), ct)
    assert np.array_equal(eng.decrypt(want, dl), table[msgs + 8])
