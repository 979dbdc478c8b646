"""The LWE keyswitch, kernel by kernel: the int8 matrix-core form (csrc/ks_mfma.hpp: k_ks_digits, k_ksk_to_limbs, k_ks_mfma,
k_ks_combine) and the scalar form (csrc/ks_lincomb.hpp: k_keyswitch split and unsplit, k_keyswitch_reduce) on Goldilocks, the
49-bit field and the 2^64 torus, against the Python-integer reference of tests/keyswitch_cases.py on the crafted rows and
against the oracle on every row.  Word for word: no tolerance anywhere.  Contexts are small (N = 1024 unless a test says
otherwise) and take an imported key - a zero bootstrap key and a crafted keyswitch key - so nothing is generated.

Paths: "mfma" = keyswitch variant 0 where the shape allows the matrix cores (levels <= 16); "scalar" = variant 1, and variant 0
where levels > 16.  The scalar kernel takes n <= 767 and stages 8 x (coefficients of its slice) x levels bytes of digits in
64 KiB of LDS: the host doubles the slices until that fits, and refuses what no kernel takes.

The dense cases (test_every_shape_n_and_count): each context below runs every count of 1, 7, 8, 9, 31, 32, 33, 97, 127, 128, 129
on every path that takes it; the key is uniform.  Columns: matrix-core K-slices and k-steps per slice at 1 / 2 / 4 / 5 tiles of
32 ciphertexts (counts 1..32 / 33 / 97..128 / 129), written slices:steps%depth -> remainder (ring depth 3 with the 9 limbs of
the 64-bit moduli, 4 with the 49-bit field's 7); scalar slices at 1 / 2 / 4..5 / 13..16 / 17 tiles of 8 (counts 1..8 / 9 /
31..33 / 97..128 / 129).  test_coverage_table_is_current regenerates the table from the slice rules and compares.

COVERAGE-TABLE-BEGIN
Goldilocks and the 2^64 torus (ring depth 3)
  shape    n     mfma 1 tile   2 tiles       4 tiles       5 tiles       scalar slices
  (8, 4)   1     64:4%3 -> 1   64:4%3 -> 1   64:4%3 -> 1   64:4%3 -> 1   64/64/64/64/32
  (21, 3)  31    -             -             -             -             64/64/64/64/32
  (17, 2)  32    -             -             -             -             64/64/64/64/32
  (16, 3)  255   64:8%3 -> 2   64:8%3 -> 2   64:8%3 -> 2   64:8%3 -> 2   64/64/64/64/32
  (9, 7)   256   32:9%3 -> 0   32:9%3 -> 0   32:9%3 -> 0   32:9%3 -> 0   64/64/64/64/32
  (6, 7)   511   64:3%3 -> 0   64:3%3 -> 0   32:6%3 -> 0   32:6%3 -> 0   64/64/64/64/32
  (5, 6)   512   32:5%3 -> 2   32:5%3 -> 2   32:5%3 -> 2   32:5%3 -> 2   64/64/64/64/32
  (3, 5)   767   32:3%3 -> 0   32:3%3 -> 0   32:3%3 -> 0   32:3%3 -> 0   64/64/64/64/32
  (1, 7)   31    32:1%3 -> 1   32:1%3 -> 1   32:1%3 -> 1   32:1%3 -> 1   64/64/64/64/32
  (1, 1)   32    32:1%3 -> 1   32:1%3 -> 1   32:1%3 -> 1   32:1%3 -> 1   64/64/64/64/32
  (1, 7)   768   32:1%3 -> 1   32:1%3 -> 1   32:1%3 -> 1   32:1%3 -> 1   refused (n > 767)
  (1, 1)   1024  32:1%3 -> 1   32:1%3 -> 1   16:2%3 -> 2   16:2%3 -> 2   refused (n > 767)
the 49-bit field (ring depth 4)
  shape    n     mfma 1 tile   2 tiles       4 tiles       5 tiles       scalar slices
  (8, 4)   1     64:4%4 -> 0   64:4%4 -> 0   64:4%4 -> 0   64:4%4 -> 0   64/64/64/64/32
  (17, 2)  31    -             -             -             -             64/64/64/64/32
  (16, 3)  32    64:8%4 -> 0   64:8%4 -> 0   64:8%4 -> 0   64:8%4 -> 0   64/64/64/64/32
  (3, 5)   255   32:3%4 -> 3   32:3%4 -> 3   32:3%4 -> 3   32:3%4 -> 3   64/64/64/64/32
  (5, 6)   256   32:5%4 -> 1   32:5%4 -> 1   32:5%4 -> 1   32:5%4 -> 1   64/64/64/64/32
  (6, 7)   511   64:3%4 -> 3   64:3%4 -> 3   32:6%4 -> 2   32:6%4 -> 2   64/64/64/64/32
  (1, 7)   512   32:1%4 -> 1   32:1%4 -> 1   32:1%4 -> 1   32:1%4 -> 1   64/64/64/64/32
  (1, 1)   767   32:1%4 -> 1   32:1%4 -> 1   32:1%4 -> 1   32:1%4 -> 1   64/64/64/64/32
  (1, 1)   31    32:1%4 -> 1   32:1%4 -> 1   32:1%4 -> 1   32:1%4 -> 1   64/64/64/64/32
  (1, 7)   768   32:1%4 -> 1   32:1%4 -> 1   32:1%4 -> 1   32:1%4 -> 1   refused (n > 767)
  (1, 1)   1024  32:1%4 -> 1   32:1%4 -> 1   16:2%4 -> 2   16:2%4 -> 2   refused (n > 767)
COVERAGE-TABLE-END

Beyond the table: every key family of keyswitch_cases.key_families against the all-extreme ciphertext rows, on (9, 7) (64-bit
moduli) and (6, 7) (49-bit field) at n = 31, both paths (test_key_families); 4,097 rows at n = 1 on (8, 4) - the unsplit scalar
form by batch size, at exactly 64 KiB of staged digits - and the unsplit form at 33 rows under a pinned rotation variant, where
(17, 2) / (21, 3) must be split after all (test_device_pointer_form..., test_every_shape...); the device-pointer entry point on a
non-default stream with a poisoned guard row, batch sizes 129, 1, 4097, 33, 8 before and after reserve(4097) (16 matrix-core
slices at 4,097 rows and n = 1); one matrix-core slice - 96 k-steps through the ring - and the unsplit scalar form over two column
blocks, 4,097 rows of (3, 5) at n = 511 (test_one_slice_at_4097_rows); N = 2048 and N = 4096 (test_wider_rings); and the
refusals, by their text."""
import contextlib
import functools

import numpy as np
import pytest

import keyswitch_cases as kc

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEFCAFEF00D      # fills the output buffers: the guard row must still hold it afterwards
MODULI = [64, 49, kc.TORUS64]
PINNED_ROTATION = 3                # a rotation variant other than 0 / 2 that every modulus has: the scalar keyswitch is then unsplit
REFUSED_SCALAR = "the scalar keyswitch kernel takes n <= 767; this parameter set needs the matrix-core form"
REFUSED_BOTH = "no keyswitch kernel takes this parameter set"


def ctx_id(q, shape, n):
    return f"{kc.NAMES[q]}-{shape[0]}x{shape[1]}-n{n}"


DENSE = [(q, shape, n) for q in MODULI for shape, n in kc.PAIRING[q]]


def coverage_table():
    """the table of the module docstring, from keyswitch_cases.coverage()"""
    lines = []
    for q, title in ((64, "Goldilocks and the 2^64 torus (ring depth 3)"), (49, "the 49-bit field (ring depth 4)")):
        cov = kc.coverage(q)
        lines.append(title)
        lines.append("  shape    n     mfma 1 tile   2 tiles       4 tiles       5 tiles       scalar slices")
        for shape, n in kc.PAIRING[q]:
            cells = []
            for count in (32, 33, 128, 129):
                c = [x for x in cov if x[:4] == (shape, n, count, "mfma")]
                cells.append(f"{c[0][4]}:{c[0][5]}%{kc.ring_depth(q)} -> {c[0][6]}" if c else "-")
            sc = [str(x[4]) for count in (8, 9, 33, 128, 129) for x in cov if x[:4] == (shape, n, count, "scalar")]
            lines.append(f"  {str(shape):<8} {n:<5} " + " ".join(f"{c:<13}" for c in cells) + " " + ("/".join(sc) if sc else "refused (n > 767)"))
    return "\n".join(line.rstrip() for line in lines)


def test_coverage_table_is_current():
    """the docstring's table is what the slice rules give, and it reaches what it must: every remainder of the per-slice step
    count modulo the ring depth, a per-slice count below the depth (levels = 1), every n, count and shape on every path"""
    doc = __doc__.split("COVERAGE-TABLE-BEGIN\n")[1].split("\nCOVERAGE-TABLE-END")[0]
    assert doc == coverage_table(), "\n" + coverage_table()
    assert kc.coverage(64) == kc.coverage(kc.TORUS64)
    for q in MODULI:
        cov = kc.coverage(q)
        depth = kc.ring_depth(q)
        mfma = [c for c in cov if c[3] == "mfma"]
        scalar = [c for c in cov if c[3] == "scalar"]
        assert {c[6] for c in mfma} == set(range(depth)), q
        assert any(c[0][0] == 1 and c[5] < depth for c in mfma)
        assert {c[1] for c in mfma} == {1, 31, 32, 255, 256, 511, 512, 767, 768, 1024}
        assert {c[1] for c in scalar} == {1, 31, 32, 255, 256, 511, 512, 767}
        assert {c[2] for c in mfma} == set(kc.COUNTS) == {c[2] for c in scalar}
        shapes = {(1, 1), (1, 7), (3, 5), (5, 6), (6, 7), (8, 4), (16, 3), (17, 2)} | ({(9, 7), (21, 3)} if q != 49 else set())
        assert shapes == set(kc.shapes(q)) == {c[0] for c in scalar}
        assert shapes - {(17, 2), (21, 3)} == {c[0] for c in mfma}
        assert any(c[5] > depth and c[6] for c in mfma)            # a ring that has refilled and still ends on a part round
        # small contexts split as far as they can; one slice is test_one_slice_at_4097_rows
        assert {c[4] for c in mfma} == {16, 32, 64} and {c[4] for c in scalar} == {32, 64}
        assert kc.mfma_slices(kc.BIG_COUNT, 511, 3) == 1 and kc.scalar_slices(kc.BIG_COUNT, 3) == 1
        assert kc.mfma_slices(kc.BIG_COUNT, 1, 8) == 16
    # the scalar form is unsplit at 4,097 rows with 8 levels and under a pinned rotation variant; more than 8 levels at N = 1024
    # do not fit unsplit and are split whatever the batch
    assert kc.scalar_slices(kc.BIG_COUNT, 8) == 1 and kc.scalar_slices(33, 8, pinned=True) == 1
    assert kc.scalar_slices(33, 17, pinned=True) == 4 and kc.scalar_slices(33, 21, pinned=True) == 4
    assert kc.scalar_slices(33, 8, pinned=True, big_n=2048) == 2 and kc.scalar_slices(33, 16, pinned=True, big_n=4096) == 8


# ------------------------------------------------------------------------------------------------ helpers
def dev_i64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to("cuda:0")


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


def sentinel_rows(rows, width):
    import torch
    return torch.full((rows, width), int(np.uint64(SENTINEL).astype(np.int64)), dtype=torch.int64, device="cuda:0")


def params_for(tfhe, q, shape, n, preset=None):
    if preset:
        P = tfhe.preset_params(preset, n=n)
        assert (P.ks_levels, P.ks_base_log) == shape and P.q_bits == q
        return P
    return tfhe.default_params(q_bits=q, n=n, ks_levels=shape[0], ks_base_log=shape[1])


@contextlib.contextmanager
def engine_for(q, shape, n, preset=None):
    from bmi_amd import tfhe
    e = tfhe.Engine(params_for(tfhe, q, shape, n, preset))
    try:
        assert e.P.big == e.P.N + 1
        yield e
    finally:
        e.close()


def import_ksk(eng, ksk):
    P = eng.P
    eng.import_keys(None, None, np.zeros((P.n, (P.k + 1) * P.bs_levels, P.k + 1, P.N), np.uint64), ksk)


def oracle_keyswitch(eng, ksk, cts):
    """the oracle's keyswitch of every row, on the same key (a zero bootstrap key: the keyswitch does not read it)"""
    from bmi_amd import tfhe
    from oracle import tfhe_oracle as to
    P = to.Params(**{f: getattr(eng.P, f) for f, _ in tfhe.Params._fields_})
    to.set_field(eng.q_bits)
    ctx = to.Ctx(P, np.zeros(to.key_shapes(P)[2], np.uint64), ksk)
    try:
        return ctx.keyswitch(cts)
    finally:
        ctx.close()
        to.set_field(64)


def run(eng, d_in, count, stream=None):
    """bmi_keyswitch_batch on the first `count` rows of d_in into a poisoned buffer of count + 1 rows; the rows written"""
    import torch
    n = eng.P.n
    d_out = sentinel_rows(count + 1, n + 1)
    if stream is None:
        eng.keyswitch(d_in, count, d_out, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            assert torch.cuda.current_stream().cuda_stream == stream.cuda_stream != torch.cuda.default_stream().cuda_stream
            eng.keyswitch(d_in, count, d_out, torch.cuda.current_stream().cuda_stream)
        eng.sync(stream.cuda_stream)
    out = host_u64(d_out)
    assert (out[count] == np.uint64(SENTINEL)).all(), f"the guard row behind {count} rows was written"
    return out[:count]


@contextlib.contextmanager
def path(eng, name, pinned_rotation=False):
    """name = "mfma" | "scalar"; everything back to auto on exit"""
    eng.set_keyswitch_variant(1 if name == "scalar" else 0)
    if pinned_rotation:
        eng.set_kernel_variant(PINNED_ROTATION)
    try:
        yield
    finally:
        eng.set_keyswitch_variant(0)
        eng.set_kernel_variant(0)


def paths_of(shape, n):
    """the paths a context has: (name, runs) - "mfma" runs where the matrix cores take the shape, "scalar" where n <= 767"""
    out = []
    if shape[0] <= kc.MFMA_MAX_LEVELS:
        out.append(("mfma", True))
    out.append(("scalar", n <= kc.SCALAR_MAX_N))
    return out


def check(got, want, names, what):
    assert np.array_equal(got, want), f"{what}\n" + kc.describe_mismatch(got, want, names)


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("q,shape,n", DENSE, ids=[ctx_id(*c) for c in DENSE])
def test_every_shape_n_and_count(q, shape, n):
    """One context of the table: a uniform key, 129 rows (the crafted rows first), the oracle on all of them and the integer
    reference on the crafted ones; then every count on every path.  A count's rows are the first rows of the same batch, so one
    reference serves them all.  Where the scalar kernel cannot take the context (n > 767) its refusal is asserted by text, and the
    unsplit scalar form runs at 33 rows under a pinned rotation variant (split after all where more than 8 levels do not fit)."""
    from bmi_amd import tfhe
    levels, base_log = shape
    names, crafted = kc.rows(levels, base_log, q)
    cts = kc.batch(levels, base_log, q, max(kc.COUNTS))
    ksk = kc.make_key("uniform", kc.BIG_N, levels, n, q)
    with engine_for(q, shape, n) as eng:
        import_ksk(eng, ksk)
        want = oracle_keyswitch(eng, ksk, cts)
        check(want[:len(names)], kc.want_crafted(ksk, n, levels, base_log, q), names, "the oracle against the integer reference")
        d_in = dev_i64(cts)
        for name, runs in paths_of(shape, n):
            with path(eng, name):
                if not runs:
                    with pytest.raises(tfhe.BmiError, match=REFUSED_SCALAR):
                        run(eng, d_in, 33)
                    continue
                for count in kc.COUNTS:
                    check(run(eng, d_in, count), want[:count], names, f"{name}, {count} rows")
        if n <= kc.SCALAR_MAX_N:
            with path(eng, "scalar", pinned_rotation=True):
                check(run(eng, d_in, 33), want[:33], names, "scalar under a pinned rotation variant, 33 rows")
            if shape[0] > kc.MFMA_MAX_LEVELS:    # no matrix-core form: variant 0 is the scalar kernel as well
                with path(eng, "mfma"):
                    check(run(eng, d_in, 129), want[:129], names, "variant 0 without a matrix-core form, 129 rows")
        assert np.array_equal(host_u64(d_in), cts)


@pytest.mark.parametrize("q", MODULI, ids=[kc.NAMES[q] for q in MODULI])
def test_key_families(q):
    """every key family against the all-extreme ciphertext rows, both paths: the balanced base-256 limbs and their carry chains
    (k_ksk_to_limbs), the signed recombination and reduce128 (k_ks_combine), reduce96 / reduce128 and the bias of the scalar
    path at the largest accumulators (every key word q - 1 against every digit at its extreme)"""
    shape, n = ((6, 7) if q == 49 else (9, 7)), 31
    levels, base_log = shape
    names, cts = kc.rows(levels, base_log, q)
    count = len(names)
    with engine_for(q, shape, n) as eng:
        d_in = dev_i64(cts)
        for family in kc.key_families(q):
            ksk = kc.make_key(family, kc.BIG_N, levels, n, q)
            import_ksk(eng, ksk)
            ref = kc.want_crafted(ksk, n, levels, base_log, q)
            check(oracle_keyswitch(eng, ksk, cts), ref, names, f"{family}: the oracle against the integer reference")
            for name in ("mfma", "scalar"):
                with path(eng, name):
                    check(run(eng, d_in, count), ref, names, f"{family}, {name}")
            if q != kc.TORUS64:
                assert (ref < np.uint64(kc.MODULUS[q])).all()


@functools.lru_cache(maxsize=None)
def big_batch(q):
    return kc.batch(8, 4, q, kc.BIG_COUNT)


@pytest.mark.parametrize("q", MODULI, ids=[kc.NAMES[q] for q in MODULI])
def test_device_pointer_form_any_order_of_batches(q):
    """bmi_keyswitch_batch on torch's current non-default stream, the output followed by a poisoned guard row, batch sizes in an
    order that makes the scratch buffers grow and shrink in need (129, 1, 4097, 33, 8: their sizing is not monotonic in the
    batch), before and after reserve(4097), on both paths.  At 4,097 rows the scalar kernel runs unsplit (8 levels at N = 1024
    stage exactly 64 KiB).  The integer reference covers the first 16 rows, the oracle all 4,097."""
    import torch
    shape, n = (8, 4), 1
    names, _ = kc.rows(8, 4, q)
    cts = big_batch(q)
    ksk = kc.make_key("uniform", kc.BIG_N, 8, n, q)
    with engine_for(q, shape, n) as eng:
        import_ksk(eng, ksk)
        want = oracle_keyswitch(eng, ksk, cts)
        check(want[:16], kc.want_crafted(ksk, n, 8, 4, q, count=16), names, "the oracle against the integer reference")
        d_in = dev_i64(cts)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        for reserved in (False, True):
            if reserved:
                eng.reserve(kc.BIG_COUNT)
            for name in ("mfma", "scalar"):
                with path(eng, name):
                    for count in (129, 1, kc.BIG_COUNT, 33, 8):
                        check(run(eng, d_in, count, stream), want[:count], names, f"{name}, {count} rows, reserved={reserved}")
        assert np.array_equal(host_u64(d_in), cts)


@pytest.mark.parametrize("q", MODULI, ids=[kc.NAMES[q] for q in MODULI])
def test_one_slice_at_4097_rows(q):
    """(3, 5) at n = 511: 129 tiles x 16 column blocks leave the matrix-core product unsplit (one slice of 96 k-steps, the
    whole ring many times round), and the scalar kernel unsplit over two column blocks.  The 4,097 rows repeat the 129 rows of
    the dense batch (a row's result does not depend on its place), so the references are those of 129 rows."""
    shape, n = (3, 5), 511
    names, _ = kc.rows(3, 5, q)
    base = kc.batch(3, 5, q, 129)
    index = np.arange(kc.BIG_COUNT) % 129
    ksk = kc.make_key("uniform", kc.BIG_N, 3, n, q)
    with engine_for(q, shape, n) as eng:
        import_ksk(eng, ksk)
        want = oracle_keyswitch(eng, ksk, base)
        check(want[:len(names)], kc.want_crafted(ksk, n, 3, 5, q), names, "the oracle against the integer reference")
        d_in = dev_i64(base[index])
        for name in ("mfma", "scalar"):
            with path(eng, name):
                check(run(eng, d_in, kc.BIG_COUNT), want[index], (), f"{name}, 4097 rows")


WIDE = [("secure128_torus", (8, 2), 2048), ("secure128_torus_wide", (16, 1), 4096)]


@pytest.mark.parametrize("preset,shape,big_n", WIDE, ids=[w[0] for w in WIDE])
def test_wider_rings(preset, shape, big_n):
    """N = 2048 and N = 4096 on the 2^64 torus with n shortened to 33: a uniform and an all-(q - 1) key, 33 and 129 rows, both
    paths.  The scalar kernel's digits do not fit unsplit at these sizes (128 KiB, 512 KiB): it runs split, also under a pinned
    rotation variant."""
    q, n = kc.TORUS64, 33
    levels, base_log = shape
    names, _ = kc.rows(levels, base_log, q, big_n)
    cts = kc.batch(levels, base_log, q, 129, big_n)
    with engine_for(q, shape, n, preset) as eng:
        assert eng.P.N == big_n
        d_in = dev_i64(cts)
        for family in ("uniform", "q-1"):
            ksk = kc.make_key(family, big_n, levels, n, q)
            import_ksk(eng, ksk)
            want = oracle_keyswitch(eng, ksk, cts)
            check(want[:len(names)], kc.want_crafted(ksk, n, levels, base_log, q, big_n=big_n), names,
                  f"{family}: the oracle against the integer reference")
            for name in ("mfma", "scalar"):
                with path(eng, name):
                    for count in (33, 129):
                        check(run(eng, d_in, count), want[:count], names, f"{family}, {name}, {count} rows")
            with path(eng, "scalar", pinned_rotation=True):
                check(run(eng, d_in, 33), want[:33], names, f"{family}, scalar under a pinned rotation variant")


@pytest.mark.parametrize("q", MODULI, ids=[kc.NAMES[q] for q in MODULI])
def test_refused_where_no_kernel_takes_the_set(q):
    """levels > 16 has no matrix-core form and n > 767 no scalar one: refused before any launch, whichever variant is asked for,
    with a text that does not send the caller to a form that does not exist"""
    from bmi_amd import tfhe
    shape, n = (17, 2), 768
    cts = kc.batch(17, 2, q, 8)
    with engine_for(q, shape, n) as eng:
        import_ksk(eng, kc.make_key("q-1", kc.BIG_N, 17, n, q))
        d_in = dev_i64(cts)
        for name in ("mfma", "scalar"):
            with path(eng, name):
                with pytest.raises(tfhe.BmiError, match=REFUSED_BOTH) as err:
                    run(eng, d_in, 8)
                assert "needs the matrix-core form" not in str(err.value)
