"""The host-buffer forms of include/bmi_tfhe.h (the *_host entry points, which every parity test stands on) on the GPU: each
returns word for word what its device-pointer form computes on torch tensors holding the same inputs, while the context's one
scratch arena (csrc/bmi_host.cpp, Stage) is reused, outgrown and reused again; and a call that is refused leaves the context
usable.  One small engine: the default 2^64-torus set with n cut to 33, a second one keyed from the CSPRNG for the seeded form,
and a 49-bit-field one for the transform hook."""
import numpy as np
import pytest

import pbs_cases as pc

pytestmark = pytest.mark.gpu

SEED = 0x5EED
N_SMALL = 33      # the small dimension the l = 2 shape tests already use


def torus_engine(seed):
    """seed None: keys from the CSPRNG (the seeded forms are refused for anything else)"""
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=tfhe.TORUS64, n=N_SMALL))
    e.keygen(seed)
    return e


def to_device(eng, a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).to(torch.device("cuda", eng.device))


def device_result(eng, shape, dtype, call):
    """what `call` writes into a zeroed device tensor of `shape` words on the current stream, as numpy"""
    import torch
    d_out = torch.zeros(shape, dtype=torch.int64 if dtype == np.uint64 else torch.int32, device=torch.device("cuda", eng.device))
    call(d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(dtype)


def pbs_on_device(eng, ct, ids):
    d_ct, d_ids = to_device(eng, ct), to_device(eng, ids)
    return device_result(eng, ct.shape, np.uint64, lambda d_out: eng.pbs(d_ct, d_ids, ct.shape[0], d_out))


def walk_every_form(eng, sec, shared, count):
    """every host form at `count` ciphertexts (groups, rows), interleaved so that consecutive calls lay the arena out differently,
    each against its device-pointer form"""
    N, big, small_w = eng.P.N, eng.P.big, eng.P.small
    tables, ids, tvs, msgs, sel, small, dl = pc.torus_batch(eng, count, 100 + count, 4)
    lut = ids[sel]
    ct = eng.encrypt(msgs, dl)
    d_ct, d_lut, d_small = to_device(eng, ct), to_device(eng, lut), to_device(eng, small)

    out = eng.pbs_host(ct, lut)
    assert np.array_equal(out, pbs_on_device(eng, ct, lut)), "pbs"
    assert list(eng.decrypt(out, dl)) == [int(tables[s][m + 8]) for s, m in zip(sel, msgs)]      # (the equal words are the look-ups)
    switched = eng.keyswitch_host(ct)
    assert np.array_equal(switched, device_result(eng, (count, small_w), np.uint64, lambda d: eng.keyswitch(d_ct, count, d))), "keyswitch"
    cc = eng.compress_host(out)
    d_out = to_device(eng, out)
    assert np.array_equal(cc.words, device_result(eng, (cc.words.size,), np.uint32, lambda d: eng.compress(d_out, count, d))), "compress"
    d_switched = to_device(eng, switched)
    assert np.array_equal(eng.modswitch_centre_host(switched),
                          device_result(eng, (count, small_w), np.uint64, lambda d: eng.modswitch_centre(d_switched, count, d))), "modswitch_centre"
    rotated = eng.blind_rotate_host(small, lut)
    assert np.array_equal(rotated, device_result(eng, (count, big), np.uint64, lambda d: eng.blind_rotate(d_small, d_lut, count, d))), "blind_rotate"
    assert np.array_equal(eng.decompress_host(cc),
                          device_result(eng, (count, big), np.uint64, lambda d: eng.decompress(cc.words, count, cc.log_modulus, d))), "decompress"
    words, distance = eng.fft_margin_host(small, lut)
    assert np.array_equal(words, rotated) and distance < 0.5, ("fft_margin", distance)

    # the shared look-ups: pbs_cases' edge groups, repeated to `count` groups
    lid, bid, block = shared
    groups = (block * -(-count // len(block)))[:count]
    gp = np.concatenate([[0], np.cumsum([len(m) for _, m in groups])]).astype(np.uint32)
    gbase = np.array([bid[u] for u, _ in groups], np.uint32)
    members = np.array([lid[name] for _, m in groups for name in m], np.uint32)
    total = members.size
    d_gp, d_gbase, d_members = to_device(eng, gp), to_device(eng, gbase), to_device(eng, members)
    glwe = eng.blind_rotate_glwe_host(small, gbase)
    assert np.array_equal(glwe, device_result(eng, (count, 2 * N), np.uint64,
                                              lambda d: eng.blind_rotate_glwe(d_small, d_gbase, count, d))), "blind_rotate_glwe"
    index = np.random.default_rng(count).integers(0, count, 2 * count + 1).astype(np.uint32)      # repeats, and more rows than ciphertexts
    assert np.array_equal(eng.decompress_host(cc, index),
                          device_result(eng, (index.size, big), np.uint64,
                                        lambda d: eng.decompress(cc.words, count, cc.log_modulus, d, index=index))), "decompress (index)"
    d_glwe = to_device(eng, glwe)
    assert np.array_equal(eng.glwe_lookup_host(glwe, gp, gbase, members),
                          device_result(eng, (total, big), np.uint64,
                                        lambda d: eng.glwe_lookup(d_glwe, d_gp, d_gbase, d_members, count, total, d))), "glwe_lookup"
    assert np.array_equal(eng.pbs_shared_host(ct, gp, gbase, members),
                          device_result(eng, (total, big), np.uint64,
                                        lambda d: eng.pbs_shared(d_ct, d_gp, d_gbase, d_members, count, total, d))), "pbs_shared"

    from bmi_amd import tfhe
    bodies = pc.uniform_words(np.random.default_rng(7 * count), count)
    first = (1 << 32) - 2
    assert np.array_equal(sec.expand_seeded_host(first, bodies),
                          device_result(sec, (count, big), np.uint64,
                                        lambda d: sec.expand_seeded(tfhe.SeededCiphertexts(first, bodies), d_out=d))), "expand_seeded"


def test_host_forms_equal_device_forms_across_arena_growth_and_reuse():
    """3 ciphertexts, then 257 - one past the arena's floor (bmi_pbs_batch_host of 256), so the arena is reallocated in the middle
    of the walk - then 3 again, on one context; a region that one call downloads lies where the next one uploads"""
    eng, sec = torus_engine(SEED), torus_engine(None)
    try:
        eng.compression_keygen()
        floor = 64 - eng.bsk_precision + 1
        assert floor == pc.FLOOR_UNIT[eng.P.N]
        T = pc.edge_lookup_tables(np.random.default_rng(1))
        lid = {name: eng.lut_register(t, p, s) for name, (t, p, s) in T.items()}
        block = pc.edge_lookup_groups(floor)
        bid = {u: eng.lut_register_base(u) for u in sorted({u for u, _ in block} | {59})}
        lid["base59"] = bid[59]
        for count in (3, 257, 3):
            walk_every_form(eng, sec, (lid, bid, block), count)
    finally:
        eng.close()
        sec.close()


def negacyclic_mod_q(a, b, Q):
    """a b mod (X^N + 1, Q) for words below 2^50: 25-bit limbs, so that every integer convolution stays below 2^63"""
    N = a.size
    lo, hi = (lambda v: (v & np.uint64((1 << 25) - 1)).astype(np.int64)), (lambda v: (v >> np.uint64(25)).astype(np.int64))

    def wrapped(x, y):
        full = np.convolve(x, y)
        full[:N - 1] -= full[N:]
        return full[:N].astype(object)
    r = wrapped(lo(a), lo(b)) + ((wrapped(lo(a), hi(b)) + wrapped(hi(a), lo(b))) << 25) + (wrapped(hi(a), hi(b)) << 50)
    return np.array([int(x) % Q for x in r], np.uint64)


@pytest.mark.parametrize("count", [1, 5])
def test_negacyclic_mul_host_equals_the_numpy_product(count):
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=49, n=N_SMALL))
    try:
        Q = e.modulus
        rng = np.random.default_rng(count)
        a, b = pc.rand_q(rng, (count, e.P.N), Q), pc.rand_q(rng, (count, e.P.N), Q)
        a[0, :4] = Q - 1
        b[0, -4:] = Q - 1
        for _ in range(2):       # the second call runs in the arena the first one left
            got = e.negacyclic_mul_host(a, b)
            for i in range(count):
                assert np.array_equal(got[i], negacyclic_mod_q(a[i], b[i], Q)), i
    finally:
        e.close()


def test_a_refused_call_leaves_the_context_usable():
    """three refusals the library already makes - before anything is queued (no keys; an index that is no position) and after the
    uploads were queued (the accumulator form under a pinned exact-transform kernel) - each followed by an ordinary pbs_host on
    the same context: the device form's words, and the table's values"""
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=tfhe.TORUS64, n=N_SMALL))
    try:
        dl = e.delta_log()
        table = np.random.default_rng(5).integers(-8, 8, 16)
        lid = e.lut_register(table, 4, dl)
        msgs = np.arange(-8, 8)
        ids = np.full(msgs.size, lid, np.uint32)

        def pbs_still_works():
            ct = e.encrypt(msgs, dl)
            out = e.pbs_host(ct, ids)
            assert np.array_equal(out, pbs_on_device(e, ct, ids))
            assert np.array_equal(e.decrypt(out, dl), table[msgs + 8])

        with pytest.raises(tfhe.BmiError, match="no keys"):
            e.pbs_host(np.zeros((msgs.size, e.P.big), np.uint64), ids)
        e.keygen(SEED)
        pbs_still_works()
        small = e.keyswitch_host(e.encrypt(msgs, dl))
        with pc.pinned_variant(e, 1):
            with pytest.raises(tfhe.BmiError, match="the accumulator form exists for the floating-point-transform kernels only"):
                e.blind_rotate_glwe_host(small, ids)
        pbs_still_works()
        count = 3
        cc = tfhe.CompressedCiphertexts(count, e.P.N, 16, np.zeros(tfhe.compressed_words(count, e.P.N), np.uint32))
        with pytest.raises(tfhe.BmiError, match=f"index {count} .row 1. is not below the count of {count} ciphertexts"):
            e.decompress_host(cc, [0, count])
        pbs_still_works()
    finally:
        e.close()
