"""Shared blind rotations on the CPU (bmi_amd/shared_rotation.py, Executor(share_rotations=True),
error_budget.failure_probability(share_rotations=True)): the sparse factor of a test polynomial against the oracle's own formula,
the groups of the two shipped programs, the budget's formula, and the grouped level walk of the executor on a plaintext stand-in
engine (the manner of tests/test_shard_gloo.py; the same walk runs on the GPU in tests/test_gpu_shared_rotation.py)."""
import glob
import math
import os

import numpy as np
import pytest
import torch

from bmi_amd import error_budget, tfhe
from bmi_amd.circuit import Circuit
from bmi_amd.program import Program, shipped_dir
from bmi_amd.shared_rotation import base_polynomial, key_carried_norm2, rotation_groups, sparse_moments, sparse_table

MASK = (1 << 64) - 1


def negacyclic_sparse(dense, pos, coef):
    """dense (uint64 words) times the sparse polynomial sum_k coef_k X^pos_k mod (X^N + 1, 2^64)"""
    N = dense.size
    out = np.zeros(N, np.uint64)
    with np.errstate(over="ignore"):
        for c, v in zip(pos.tolist(), coef.tolist()):
            rot = np.concatenate([(np.uint64(0) - dense[N - c:]) if c else dense[:0], dense[: N - c]])
            out += rot * np.uint64(v & MASK)
    return out


def tables_of(p, rng):
    h = 1 << (p - 1)
    edge = rng.integers(-h, h, 2 * h)
    edge[2 * h - 1] = -h        # f(2^(p-1) - 1) = -2^(p-1) = f(-2^(p-1)): neighbouring boxes +-2^(p-1) apart by 2^p
    edge[0] = -h
    return {"random": rng.integers(-h, h, 2 * h), "identity": np.arange(-h, h), "half": np.array([1] * h + [-1] * h), "edge": edge}


@pytest.mark.parametrize("log_N", [10, 11, 12])
def test_sparse_factor_times_base_is_the_oracles_test_polynomial(log_N):
    from oracle import tfhe_oracle as to
    to.set_field(65)
    N = 1 << log_N
    rng = np.random.default_rng(log_N)
    for p in range(1, 7):
        for name, table in tables_of(p, rng).items():
            odl = 63 - p - (1 if name == "half" else 0)
            want = to.make_test_vector(log_N, p, table, odl)
            for unit in (odl, odl - 1):
                pos, coef = sparse_table(table, p, odl, unit, N)
                assert pos.size == coef.size <= (1 << p) and (pos > 0).all() and (pos < N).all() and (coef != 0).all(), (p, name)
                assert np.array_equal(negacyclic_sparse(base_polynomial(unit, N), pos, coef), want), (log_N, p, name, unit)
    # the edge table's largest difference keeps its sign: +2^p, not the torus word's -2^p
    h = 8
    pos, coef = sparse_table(tables_of(4, rng)["edge"], 4, 59, 59, N)
    assert coef[pos == 8 * (N >> 4) - (N >> 5)].tolist() == [2 * h]


@pytest.mark.parametrize("log_N", [10, 11, 12])
def test_sparse_factor_at_the_floor_units_and_edge_tables(log_N):
    """the (table, scale, unit) triples the GPU test of k_glwe_lookup's edges runs (pbs_cases.edge_lookup_tables / _groups: units
    down to the key's grid floor, 42 / 40 / 38 bits below the table's scale): sparse_table times the unit's base polynomial is the
    oracle's test polynomial there too, so the dense product that test compares the kernel with is pinned at the shapes it uses"""
    import pbs_cases as pc
    from oracle import tfhe_oracle as to
    to.set_field(65)
    N = 1 << log_N
    T = pc.edge_lookup_tables(np.random.default_rng(N + 1))
    floor = pc.FLOOR_UNIT[N]
    entries = {}
    for unit, members in pc.edge_lookup_groups(floor):
        for name in members:
            if name == "base59":        # a base polynomial as a member of a finer group: P = 2^(59 - unit)
                assert np.array_equal(base_polynomial(unit, N) * np.uint64(1 << (59 - unit)), base_polynomial(59, N))
                continue
            table, p, scale = T[name]
            pos, coef = sparse_table(table, p, scale, unit, N)
            entries[name] = pos.size
            assert (pos > 0).all() and (pos < N).all() and (np.diff(pos) > 0).all() and (coef != 0).all(), name
            assert np.array_equal(negacyclic_sparse(base_polynomial(unit, N), pos, coef), to.make_test_vector(log_N, p, table, scale)), (name, unit)
            if name == "const":
                assert pos.tolist() == [N // 2 - N // 32] and coef.tolist() == [-10]
    edge = {"six64": 64, "zero": 0, "const": 1, "one": 2, "one_const": 1, "two": 3, "two_edge": 4}     # entries of the sparse factors
    assert {k: entries[k] for k in edge} == edge and len(entries) == len(T)
    assert 59 - pc.FLOOR_UNIT[1024] == 42 and 59 - pc.FLOOR_UNIT[2048] == 40


def test_moments_of_a_sparse_factor():
    """sparse_moments against its definition, and E |S P|^2 = N (|P|^2 / 4 + mean m^2 / 4) against the exact |S P|^2 of random keys"""
    rng = np.random.default_rng(2)
    N = 1024
    assert sparse_moments([0], [1], N) == (1.0, 1.0)                # P = 1: an ordinary rotation
    for table in (np.arange(-8, 8), rng.integers(-8, 8, 16), np.array([1] * 8 + [-1] * 8)):
        pos, coef = sparse_table(table, 4, 59, 59, N)
        n2, m2 = sparse_moments(pos, coef, N)
        m = np.array([sum(c if x >= q else -c for q, c in zip(pos.tolist(), coef.tolist())) for x in range(N)], np.float64)
        assert n2 == float((coef ** 2).sum()) and math.isclose(m2, float((m ** 2).mean()), rel_tol=1e-12)
        assert sparse_moments(pos * 2, coef, 2 * N) == (n2, m2)    # the positions scale with N, the moments do not
        exact = np.mean([key_carried_norm2(pos, coef, rng.integers(0, 2, N)) for _ in range(200)])
        assert abs(exact / (N * (n2 + m2) / 4.0) - 1.0) < 0.05, (exact, n2, m2)
    assert sparse_moments(*sparse_table(np.arange(-8, 8), 4, 59, 59, N), N)[0] == 16.0


def test_sparse_table_refuses_what_cannot_share():
    with pytest.raises(ValueError):
        sparse_table(np.arange(-8, 8), 4, 58, 59, 1024)      # encoded below the unit
    with pytest.raises(ValueError):
        sparse_table(np.arange(-8, 8), 3, 59, 59, 1024)      # not 2^p entries


@pytest.fixture(scope="module")
def shipped():
    progs = {}
    for f in glob.glob(os.path.join(shipped_dir(), "*.prog.xz")):
        prog = Program.load_compact(f)
        progs[int(prog.meta.get("n", 0)) or os.path.basename(f)] = (prog, rotation_groups(prog))
    return progs


def _shipped_by_lookups(shipped, lookups):
    for prog, rg in shipped.values():
        if prog.n_nodes == lookups:
            return prog, rg
    pytest.fail(f"no shipped program with {lookups} look-ups")


@pytest.mark.parametrize("lookups,groups", [(1910110, 1532563), (1226555, 988023)])
def test_rotation_groups_of_the_shipped_programs(shipped, lookups, groups):
    prog, rg = _shipped_by_lookups(shipped, lookups)
    assert rg.groups == groups
    assert np.array_equal(np.sort(rg.members), np.arange(prog.n_nodes))           # a partition of the nodes
    assert int(rg.level_groups.sum()) == groups and rg.level_groups.size == prog.depth
    gid = np.repeat(np.arange(groups), rg.sizes)
    lead = rg.members[rg.group_ptr[:-1]][gid]
    assert np.array_equal(prog.node_level[rg.members], prog.node_level[lead])    # members share the level ...
    lens = np.diff(prog.node_ptr)
    assert np.array_equal(lens[rg.members], lens[lead]) and np.array_equal(prog.node_const[rg.members], prog.node_const[lead])
    big = np.flatnonzero(rg.sizes > 1)[:: max(1, int((rg.sizes > 1).sum()) // 2000)]   # ... and the input, term for term (a sample)
    for g in big.tolist():
        rows = [(prog.term_leaf[prog.node_ptr[i]: prog.node_ptr[i + 1]].tolist(), prog.term_coef[prog.node_ptr[i]: prog.node_ptr[i + 1]].tolist())
                for i in rg.members[rg.group_ptr[g]: rg.group_ptr[g + 1]].tolist()]
        assert all(r == rows[0] for r in rows)
    # levels in order, and inside a level the groups by their first member in level order
    assert (np.diff(prog.node_level[rg.members]) >= 0).all()
    shared = np.repeat(rg.sizes, rg.sizes) > 1
    assert 2.0 <= rg.norm2[shared].min() and rg.norm2[shared].max() <= 64.0


def three_node_program():
    c = Circuit()
    x = c.input(-8, 7)
    a = c.lut(x, lambda v: v // 2)            # two tables of the same input: one group
    b = c.lut(x, lambda v: (v * v) % 5 - 2)
    c.set_outputs([c.lut(a + b, lambda v: -v)])
    return Program.from_circuit(c, native=False)


def test_budget_of_a_hand_built_program_is_the_written_out_formula():
    prog = three_node_program()
    rg = rotation_groups(prog)
    assert rg.sizes.tolist() == [2, 1]
    P = tfhe.default_params()
    N, hs = 1 << P.log_N, P.n / 2.0
    v_pbs, v_ks = error_budget.pbs_output_variance(P), error_budget.keyswitch_variance(P)
    v_white, v_carried = error_budget.pbs_output_variance_parts(P)
    assert math.isclose(v_white + (N / 2.0) * v_carried, v_pbs, rel_tol=1e-12)
    n2, shared_var = [], []
    for node in (0, 1):
        j = int(prog.node_lut[node])
        p = int(prog.lut_p[j])
        pos, cf = sparse_table(prog.lut_tab[j, : 1 << p], p, 59, 59, N)
        n2.append(float((cf.astype(np.float64) ** 2).sum()))
        m = np.array([sum(c if x >= q else -c for q, c in zip(pos.tolist(), cf.tolist())) for x in range(N)], np.float64)
        # |P|^2 v_white + E |S P|^2 v_carried, keys of density 1/2: E |S P|^2 = N |P|^2 / 4 + sum_j m_j^2 / 4
        shared_var.append(n2[-1] * v_white + (N * n2[-1] / 4.0 + float((m ** 2).sum()) / 4.0) * v_carried)
    assert sorted(rg.norm2[:2].tolist()) == sorted(n2)

    def tail(v_in, p):
        sigma = math.sqrt((v_in + v_ks) * (2.0 * N) ** 2 + (1 + hs) / 12.0)
        return math.erfc(N / 2.0 ** (p + 1) / sigma / math.sqrt(2.0))

    def total(va, vb, vc):
        c0, c1 = [float(v) for v in prog.term_coef[prog.node_ptr[2]: prog.node_ptr[3]]]
        p_of = lambda i: int(prog.lut_p[prog.node_lut[i]])   # noqa: E731
        x_coef = float(prog.term_coef[0])
        lookups = 2 * tail(x_coef ** 2 * P.glwe_noise ** 2, p_of(0)) + tail(c0 * c0 * va + c1 * c1 * vb, p_of(2))
        return lookups + math.erfc(2.0 ** -(prog.msg_bits + 2) / math.sqrt(vc) / math.sqrt(2.0))

    plain = error_budget.failure_probability(prog, P)
    shared = error_budget.failure_probability(prog, P, share_rotations=True)
    assert shared["shared_lookups"] == 2 and shared["rotations"] == 2
    order = [int(prog.node_lut[i]) for i in (0, 1)]
    assert order[0] != order[1]
    assert math.isclose(plain["p_fail"], total(v_pbs, v_pbs, v_pbs), rel_tol=1e-9)
    assert math.isclose(shared["p_fail"], total(shared_var[0], shared_var[1], v_pbs), rel_tol=1e-9)
    assert min(shared_var) > v_pbs
    assert shared["p_fail"] >= plain["p_fail"]


@pytest.mark.parametrize("preset", [None, "secure128_torus"])
def test_sharing_never_lowers_the_budget_of_the_shipped_8x8(shipped, preset):
    prog, _ = _shipped_by_lookups(shipped, 1910110)
    P = tfhe.default_params() if preset is None else tfhe.preset_params(preset)
    plain = error_budget.failure_probability(prog, P)
    shared = error_budget.failure_probability(prog, P, share_rotations=True)
    print(f"\n8x8 under {preset or 'the default set'}: log10 p_fail {plain['log10_p_fail']:.3f} unshared, {shared['log10_p_fail']:.3f} shared "
          f"(ratio {10.0 ** (shared['log10_p_fail'] - plain['log10_p_fail']):.6f}); worst margin {plain['worst_margin_sigma']:.3f} -> "
          f"{shared['worst_margin_sigma']:.3f} sigma; {shared['shared_lookups']} shared look-ups, {shared['rotations']} rotations")
    assert shared["log10_p_fail"] >= plain["log10_p_fail"] and shared["worst_margin_sigma"] <= plain["worst_margin_sigma"]
    assert shared["rotations"] == 1532563 and shared["lookups"] == 1910110


# ---- the grouped level walk of the executor on plaintext rows (last word = 2 x message: delta_log 1, as tests/test_shard_gloo.py)
class _PlainParams:
    big = 3


class PlainSharedEngine:
    P = _PlainParams()
    modulus = 1 << 64
    device = "cpu"

    def __init__(self):
        self.tables = []        # (msg_bits, entries << out_delta_log, out_delta_log); a base polynomial: (None, None, unit_log)
        self.calls = {"pbs": 0, "pbs_shared": 0, "rotations": 0, "lookups": 0}

    def torch_device(self):
        return torch.device("cpu")

    def delta_log(self, msg_bits=4):
        return 1

    def lut_register(self, table, msg_bits, out_delta_log):
        self.tables.append((int(msg_bits), [int(v) << int(out_delta_log) for v in table], int(out_delta_log)))
        return len(self.tables) - 1

    def lut_register_base(self, unit_log):
        self.tables.append((None, None, int(unit_log)))
        return len(self.tables) - 1

    def reserve(self, n):
        pass

    def lincomb(self, store, rp, ix, cf, cs, count, out, stream=0):
        for r in range(count):
            acc = torch.zeros(self.P.big, dtype=torch.int64)
            for e in range(int(rp[r]), int(rp[r + 1])):
                acc += int(cf[e]) * store[int(ix[e])]
            acc[-1] += int(cs[r])
            out[r] = acc

    def scatter_rows(self, src, count, store, rows, stream=0):
        for r in range(count):
            store[int(rows[r])] = src[r]

    def _look_up(self, x, lut_id):
        p, table, _ = self.tables[lut_id]
        assert x % 2 == 0                     # whole multiples of Delta reach a look-up
        m = (x >> 1) >> (4 - p)
        half = 1 << (p - 1)
        if m >= half:                         # the other half of the torus: negacyclic wrap-around
            return -table[m - half]
        if m < -half:
            return -table[m + 3 * half]
        return table[m + half]

    def pbs(self, d_in, ids, count, d_out, stream=0):
        self.calls["pbs"] += 1
        self.calls["rotations"] += count
        self.calls["lookups"] += count
        for r in range(count):
            d_out[r] = 0
            d_out[r, -1] = self._look_up(int(d_in[r, -1]), int(ids[r]))

    def pbs_shared(self, d_in, gptr, gbase, ids, groups, total, d_out, stream=0):
        self.calls["pbs_shared"] += 1
        self.calls["rotations"] += groups
        self.calls["lookups"] += total
        assert int(gptr[0]) == 0 and int(gptr[groups]) == total
        for g in range(groups):
            kind, _, unit = self.tables[int(gbase[g])]
            for t in range(int(gptr[g]), int(gptr[g + 1])):
                if int(ids[t]) != int(gbase[g]):                 # (a table that is its group's own base is a plain bootstrap)
                    assert kind is None and self.tables[int(ids[t])][2] >= unit      # a base polynomial; no table below its unit
                else:
                    assert int(gptr[g + 1]) - int(gptr[g]) == 1
                d_out[t] = 0
                d_out[t, -1] = self._look_up(int(d_in[g, -1]), int(ids[t]))


def toy_circuit():
    """groups of 5, 2 and 1 in the first level (one of them with a half-scale table: the unit is then the half scale), then a
    level that reads them"""
    c = Circuit()
    x, y, z, u = c.input(-8, 7), c.input(-8, 7), c.input(-8, 7), c.input(-7, 7)
    fx = [c.lut(x, f) for f in (lambda v: v // 2, lambda v: (v * v) % 7 - 3, lambda v: -v - 1, lambda v: int(v > 2), lambda v: abs(v) - 4)]
    d = y - u                                           # [-15, 14]: the whole torus
    fy = [c.lut_neg(d), c.lut_odd(d, lambda v: 3 if v >= 0 else -3)]
    fz = c.lut(z, lambda v: 7 - abs(v))
    s = fx[0] + fx[3] + fy[0]
    outs = [c.lut(s, lambda v: 2 * v), c.lut(s, lambda v: (v * v) % 6 - 3), fz + fy[1], fx[1] - fx[2], fx[4]]
    c.set_outputs(outs)
    return c


def run_plain(circ, inputs, **kw):
    from bmi_amd.executor import Executor
    eng = PlainSharedEngine()
    ex = Executor(circ, eng, **kw)
    B = kw.get("batch", 1)
    inputs = np.asarray(inputs, np.int64).reshape(B, -1)
    cts = np.zeros((B, inputs.shape[1], 3), np.uint64)
    cts[:, :, -1] = (2 * inputs).view(np.uint64)
    out = ex.run(cts if B > 1 else cts[0])
    msgs = out[..., -1].view(np.int64)
    assert not (msgs % 2).any()
    return msgs // 2, ex, eng


def random_inputs(circ, rng, rows=None):
    one = lambda: [int(rng.integers(lo, hi + 1)) for lo, hi in zip(circ.leaf_lo[:circ.n_inputs], circ.leaf_hi[:circ.n_inputs])]   # noqa: E731
    return one() if rows is None else [one() for _ in range(rows)]


def test_shared_walk_of_a_toy_circuit_equals_the_unshared_walk():
    circ = toy_circuit()
    prog = Program.from_circuit(circ, native=False)
    rg = rotation_groups(prog)
    assert sorted(rg.sizes[: rg.level_groups[0]].tolist()) == [1, 2, 5] and rg.unit_half[: rg.level_groups[0]].sum() == 1
    rng = np.random.default_rng(4)
    for _ in range(6):
        x = random_inputs(circ, rng)
        want = circ.simulate(x)
        plain, ex0, e0 = run_plain(prog, x)
        shared, ex1, e1 = run_plain(prog, x, share_rotations=True)
        assert plain.tolist() == shared.tolist() == want
        assert ex0.rotations == ex0.lookups == prog.n_nodes == e0.calls["rotations"]
        assert ex1.lookups == prog.n_nodes == e1.calls["lookups"] and ex1.rotations == rg.groups == e1.calls["rotations"] < ex1.lookups
        assert e1.calls["pbs"] == 0 and e1.calls["pbs_shared"] == prog.depth


def test_shared_walk_of_a_batch_equals_the_unshared_walk():
    if not os.path.exists(tfhe.LIB_PATH):
        pytest.skip("a batch re-packs the levels in the library (bmi_circuit_schedule): build it first")
    circ = toy_circuit()
    rng = np.random.default_rng(5)
    xs = random_inputs(circ, rng, 3)
    want = [circ.simulate(x) for x in xs]
    plain, *_ = run_plain(circ, xs, batch=3)
    shared, ex, eng = run_plain(circ, xs, batch=3, share_rotations=True)
    assert plain.tolist() == shared.tolist() == want
    assert ex.rotations == 3 * rotation_groups(ex.prog).groups == eng.calls["rotations"] and ex.lookups == 3 * ex.prog.n_nodes


@pytest.mark.parametrize("batch", [1, 3])
def test_shared_walk_of_the_2x2_inverse(batch):
    if not os.path.exists(tfhe.LIB_PATH):
        pytest.skip("tracing the inverse runs the library's graph passes: build it first")
    from bmi_amd.main import trace_inverse
    circ = trace_inverse(2, 8, 4, 2, False, False)
    rng = np.random.default_rng(6)
    xs = random_inputs(circ, rng, batch)
    want = [circ.simulate(x) for x in xs]
    shared, ex, _ = run_plain(circ, xs if batch > 1 else xs[0], batch=batch, share_rotations=True)
    assert shared.reshape(batch, -1).tolist() == want
    assert ex.rotations == batch * rotation_groups(ex.prog).groups < ex.lookups


def _two_rank_worker(rank, world, port):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from bmi_amd.executor import Executor
    prog = Program.from_circuit(toy_circuit(), native=False)
    try:
        with pytest.raises(ValueError):
            Executor(prog, PlainSharedEngine(), share_rotations=True)
        Executor(prog, PlainSharedEngine(), shard_threshold=1)      # (the unshared walk still builds on two ranks)
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_sharing_with_more_than_one_rank_raises():
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_two_rank_worker, args=(2, port), nprocs=2, join=True)
