"""GPU executor: runs a compiled `program.Program` level by level through the C ABI.

Per level:  bmi_lincomb_batch (forms the level's PBS inputs from the device-resident leaf store) ->
bmi_pbs_batch (keyswitch -> blind rotation -> extraction, into a contiguous level buffer) -> bmi_scatter_rows (level
buffer -> the store rows assigned to the outputs).  All index arrays are built once, vectorised, from the program's CSR
arrays and stay on the device; a run is 3 launches per level plus the keyswitch's on one stream, with no host
synchronisation until the outputs are read back.  PyTorch is used only as the device allocator.

Store rows are recycled: a leaf's row returns to the free list at the level of its last consumer (liveness is known
at compile time), so the store holds the live set, not every look-up ever made (8x8 inverse: 2.6 M look-ups, a few
hundred thousand rows).

Several GPUs: every rank holds the same evaluation keys (Engine.keygen_shared, or seeded test keys; checked at construction) and the whole store and walks the same level
list.  A level at least `shard_threshold` wide is split into contiguous row ranges (shard.shard_range on a padded
width): each rank forms and bootstraps ITS rows only, one all-gather (RCCL) on the level buffer completes it
everywhere, then every rank scatters the whole level into its store; this is the path's only exchange step.  Narrower
levels are computed redundantly by every rank - cheaper than any transfer, since a level below ~256 ciphertexts
costs one latency-kernel round whatever its width.

Several INPUTS at once (`batch`): the same program evaluated on `batch` independent input vectors in one walk of the level list -
every level is `batch` times wider (replica b of a node reads replica b's rows: the store is `batch` stacked copies of the
one-input store), so the levels of one latency-kernel round become throughput-kernel launches: the serving form (a 3x3 inverse
is 319 rounds of <= 256 look-ups alone, 69 k look-ups at the throughput kernel's rate in a batch).

Shared rotations (`share_rotations=True`, 2^64 torus): the look-ups of a level that read the same linear combination
(shared_rotation.rotation_groups: carry and digit of one column sum, the comparison bits of one division step ...) cost ONE
keyswitch and ONE blind rotation together.  Per level: one linear combination per GROUP -> bmi_pbs_shared_batch (keyswitch and
rotation of the groups' base polynomials, then every member's table from its group's accumulator) -> the same scatter of every
member's row.  Under `batch` every replica groups alike.  Not combined with several ranks.
"""
from __future__ import annotations

import numpy as np

from .circuit import Circuit
from .program import Program
from .program import ROUND as Program_ROUND, WIDE_ROUND as Program_WIDE_ROUND


def _torus(v, delta_log, q):
    """signed integers -> v * 2^delta_log mod q, as int64 bit patterns"""
    out = np.empty(len(v), np.int64)
    for i, x in enumerate(v):
        t = (int(x) << delta_log) % q
        out[i] = t - (1 << 64) if t >= (1 << 63) else t
    return out


def assign_rows(prog: Program, recycle=True):
    """Store row of every leaf (inputs first).  With recycling, the rows of leaves whose last consumer is level t are
    handed to the outputs of level t (the level's inputs are copied out by its lincomb before its PBS writes).
    Returns (row per leaf, number of rows)."""
    n_in, nn = prog.n_inputs, prog.n_nodes
    n_leaves = n_in + nn
    row = np.empty(n_leaves, np.int64)
    row[:n_in] = np.arange(n_in)
    order, counts = prog.level_order()
    if not recycle:
        row[n_in + order] = n_in + np.arange(nn)
        return row, n_leaves
    depth = prog.depth
    # last level that reads each leaf: terms visited in level order, so the last write per leaf is the latest level
    lens = np.diff(prog.node_ptr)
    term_level = np.repeat(prog.node_level, lens)
    by_level = np.argsort(term_level, kind="stable")
    last_use = np.zeros(n_leaves, np.int64)
    last_use[prog.term_leaf[by_level]] = term_level[by_level]
    last_use[prog.out_leaf] = depth + 1          # outputs stay until the end
    dying = np.argsort(last_use, kind="stable")  # leaves grouped by the level that frees them
    dead_counts = np.bincount(last_use, minlength=depth + 2)
    dead_start = np.concatenate([[0], np.cumsum(dead_counts)])
    free = np.empty(n_leaves, np.int64)
    nfree, top, pos = 0, n_in, 0
    for t in range(1, depth + 1):
        d = dying[dead_start[t]: dead_start[t + 1]]
        if d.size:
            free[nfree: nfree + d.size] = row[d]
            nfree += d.size
        k = int(counts[t - 1])
        take = min(k, nfree)
        nodes = order[pos: pos + k]
        pos += k
        if take:
            row[n_in + nodes[:take]] = free[nfree - take: nfree]
            nfree -= take
        if k > take:
            row[n_in + nodes[take:]] = top + np.arange(k - take)
            top += k - take
    return row, top


class Executor:
    def __init__(self, circuit, engine, group=None, shard_threshold=None, recycle=True, batch=1, share_rotations=False):
        """circuit: a program.Program (or a circuit.Circuit, frozen here); group: a torch.distributed process group (None:
        the default group when initialised with more than one rank, otherwise single-GPU execution); shard_threshold:
        narrowest level that is split across the ranks - None (default) = every level wider than one latency-kernel
        round (257 ciphertexts), and the program's levels are then re-packed for `world` x 256 ciphertexts per round
        (Program.rescheduled): G GPUs working on one level are one machine with G x 256 workgroup slots; recycle: reuse
        store rows after a leaf's last consumer; batch: number of independent input vectors one run() evaluates (module docstring);
        share_rotations: one keyswitch and blind rotation per group of look-ups with the same input (module docstring; single rank).
        After construction `lookups` is the number of table look-ups of one run() and `rotations` the number of blind rotations."""
        import torch
        self.torch = torch
        prog = Program.from_circuit(circuit) if isinstance(circuit, Circuit) else circuit
        self.c = self.prog = prog
        self.eng = engine
        self.dev = engine.torch_device() if hasattr(engine, "torch_device") else torch.device("cuda", engine.device)
        self.on_gpu = self.dev.type == "cuda"
        self.dist, self.group, self.rank, self.world = None, group, 0, 1
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            self.dist, self.rank, self.world = dist, dist.get_rank(group), dist.get_world_size(group)
            # every rank bootstraps its part of a split level with ITS evaluation keys: they must be one key set (seeded keygen on
            # every rank, or Engine.keygen_shared / EncryptedMatrixInversion.keygen).  Independent keys would gather ciphertexts
            # under different keys and decrypt to garbage without any error - refused here instead.
            if hasattr(engine, "eval_key_fingerprint"):
                fp = engine.eval_key_fingerprint()
                on_gpu = dist.get_backend(group) == "nccl"
                lo = torch.tensor([fp], dtype=torch.int64, device=self.dev if on_gpu else "cpu")
                hi = lo.clone()
                dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
                dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
                if int(lo.item()) != int(hi.item()):
                    raise RuntimeError("the ranks of this group hold different evaluation keys: generate one key set and share it "
                                       "(Engine.keygen_shared, or EncryptedMatrixInversion.keygen under torch.distributed)")
            # ... and with one modulus switch (Engine.set_modswitch): a level split between a rank that centres and one that does not
            # would decrypt, at two different noise levels that no error budget describes
            mode = int(getattr(engine, "modswitch", 0))
            modes = torch.tensor([mode, -mode], dtype=torch.int64, device=self.dev if dist.get_backend(group) == "nccl" else "cpu")
            dist.all_reduce(modes, op=dist.ReduceOp.MIN, group=group)
            if int(modes[0].item()) != -int(modes[1].item()):
                raise RuntimeError("the ranks of this group report different modulus-switch modes: call set_modswitch with the same "
                                   "mode on every rank's engine (EncryptedMatrixInversion(centred_modswitch=...) does)")
        self.share_rotations = bool(share_rotations)
        if self.share_rotations and self.world > 1:
            raise ValueError("share_rotations is not combined with several ranks: a sharded level is split by look-ups, not by groups")
        if shard_threshold is None:
            shard_threshold = Program_ROUND + 1
            if self.world > 1:
                prog = prog.rescheduled(Program_ROUND * self.world, Program_WIDE_ROUND * self.world)
                self.c = self.prog = prog
        self.shard_threshold = max(int(shard_threshold), 1)
        if int(batch) > 1:
            # `batch` replicas of every level run side by side: a level is cheapest when replicas x width fills whole rounds of the
            # throughput kernel (1,024 ciphertexts per round and GPU), so the program's levels are re-packed for that width per
            # replica (same depth; 3x3 at 8 matrices per walk: 7 % fewer rounds, 2x2: 17 %)
            per = max(Program_WIDE_ROUND * self.world // int(batch), 1)
            prog = prog.rescheduled(per, per)
            self.c = self.prog = prog
        self.big = engine.P.big
        self.batch = B = int(batch)
        if B < 1:
            raise ValueError("batch must be at least 1")
        n_in = prog.n_inputs
        order, counts = prog.level_order()
        self.row_of, self.n_rows1 = assign_rows(prog, recycle)
        self.n_rows = self.n_rows1 * B
        self.delta_log = engine.delta_log(prog.msg_bits)
        q, dl = engine.modulus, self.delta_log
        # a lut_neg table (-+1) is registered at half the output scale: its ciphertexts carry (bit - 1/2) Delta, and every
        # consumer's constant below makes up for the missing Delta / 2 (Circuit.lut_neg, Program.half_unit_consts)
        lut_ids = np.asarray([engine.lut_register(prog.lut_tab[j, : 1 << int(prog.lut_p[j])].astype(np.int64),
                                                  int(prog.lut_p[j]), dl - 1 if prog.lut_half[j] else dl)
                              for j in range(prog.lut_p.size)], np.int32)
        to_dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.dev)  # noqa: E731
        rg = None
        if self.share_rotations:
            # a level's nodes group by group (same widths, so the rows assigned above stand); the groups' first members carry
            # the linear combinations
            from .shared_rotation import rotation_groups
            rg = rotation_groups(prog)
            order = rg.members

        # every level's rows in level order: one set of flat arrays for the whole program, sliced per level
        consts = prog.half_unit_consts(prog.node_ptr, prog.term_leaf, prog.term_coef, prog.node_const)   # units of Delta / 2
        shift = np.zeros(order.size, np.int64)      # store-row offset of a node's replica
        if B > 1:
            # replica b of every node right after replica b - 1 of its level: per level the node list tiled B times
            lvl_start = np.concatenate([[0], np.cumsum(counts)])
            tiled = [np.tile(order[lvl_start[t]: lvl_start[t + 1]], B) for t in range(len(counts))]
            shift = np.concatenate([np.repeat(np.arange(B, dtype=np.int64) * self.n_rows1, int(counts[t])) for t in range(len(counts))]) \
                if len(counts) else shift
            order = np.concatenate(tiled) if tiled else order
            counts = counts * B
        self.d_ids = to_dev(lut_ids[prog.node_lut[order]] if order.size else [0], np.int32)
        self.d_rows = to_dev(self.row_of[n_in + order] + shift if order.size else [0], np.int32)
        self.lookups = int(order.size)
        lin_order, lin_shift = order, shift         # the nodes whose linear combinations are formed: all of them ...
        self.glevels = None
        if rg is not None:
            # ... or the first member of every group.  Per level: (groups, position of its first group, offset of its group_ptr
            # segment); a segment starts at 0 and has groups + 1 entries (the B replicas' groups one after the other)
            sizes = rg.sizes
            first = np.concatenate([[0], np.cumsum(rg.level_groups)])
            # a group's base: the base polynomial of its unit - or, for a group of one, the table itself (a plain bootstrap)
            base_ids = np.asarray([engine.lut_register_base(dl - 1 if h else dl) for h in (False, True)], np.int32)
            group_base = np.where(sizes == 1, lut_ids[prog.node_lut[rg.members[rg.group_ptr[:-1]]]], base_ids[rg.unit_half.astype(np.int64)])
            leaders, lshift, gbase, gptr, self.glevels = [], [], [], [], []
            gpos = poff = 0
            for t in range(len(rg.level_groups)):
                g0, g1 = int(first[t]), int(first[t + 1])
                ng = (g1 - g0) * B
                leaders.append(np.tile(rg.members[rg.group_ptr[g0:g1]], B))
                lshift.append(np.repeat(np.arange(B, dtype=np.int64) * self.n_rows1, g1 - g0))
                gbase.append(np.tile(group_base[g0:g1], B))
                gptr.append(np.concatenate([[0], np.cumsum(np.tile(sizes[g0:g1], B))]))
                self.glevels.append((ng, gpos, poff))
                gpos += ng
                poff += ng + 1
            lin_order = np.concatenate(leaders) if leaders else order
            lin_shift = np.concatenate(lshift) if lshift else shift
            self.d_gbase = to_dev(np.concatenate(gbase) if gpos else [0], np.int32)
            self.d_gptr = to_dev(np.concatenate(gptr) if gptr else [0], np.int32)
        self.rotations = int(lin_order.size)
        lens = np.diff(prog.node_ptr)[lin_order]
        starts = prog.node_ptr[:-1][lin_order]
        tot = int(lens.sum())
        off = np.arange(tot) - np.repeat(np.cumsum(lens) - lens, lens) + np.repeat(starts, lens)
        self.d_idx = to_dev(self.row_of[prog.term_leaf[off]] + np.repeat(lin_shift, lens) if tot else [0], np.int32)
        self.d_coef = to_dev(prog.term_coef[off] if tot else [0], np.int64)
        consts = consts[lin_order]
        uniq, inv = np.unique(consts, return_inverse=True)
        self.d_const = to_dev(_torus(uniq, dl - 1, q)[inv] if consts.size else [0], np.int64)
        # row_ptr of all linear combinations in level order, absolute term offsets: a level (or a rank's part of it) is a slice
        self.d_rp = to_dev(np.concatenate([[0], np.cumsum(lens)]), np.int32)
        self.levels = []          # (width, position of the level's first node, padded width)
        pos = 0
        for w in counts.tolist():
            padded = -(-w // self.world) * self.world if (self.world > 1 and w >= self.shard_threshold) else w
            self.levels.append((w, pos, padded))
            pos += w
        o_len = np.diff(prog.out_ptr)
        o_rows = self.row_of[prog.out_leaf] if prog.out_leaf.size else np.zeros(0, np.int64)
        o_const = _torus(prog.half_unit_consts(prog.out_ptr, prog.out_leaf, prog.out_coef, prog.out_const), dl - 1, q)
        self.out_csr = (to_dev(np.concatenate([[0], np.cumsum(np.tile(o_len, B))]), np.int32),
                        to_dev(np.concatenate([o_rows + b * self.n_rows1 for b in range(B)]) if o_rows.size else [0], np.int32),
                        to_dev(np.tile(prog.out_coef, B) if prog.out_coef.size else [0], np.int64),
                        to_dev(np.tile(o_const, B), np.int64))
        self.n_out = prog.n_outputs * B
        self.max_width = max((p for *_, p in self.levels), default=1)
        self.sharded_levels = sum(1 for w, *_ in self.levels if self.world > 1 and w >= self.shard_threshold)
        self.store = torch.zeros((max(self.n_rows, 1), self.big), dtype=torch.int64, device=self.dev)
        self.tmp = torch.zeros((max(self.max_width, 1), self.big), dtype=torch.int64, device=self.dev)
        self.lvl = torch.zeros((max(self.max_width, 1), self.big), dtype=torch.int64, device=self.dev)
        self.out = torch.zeros((max(self.n_out, 1), self.big), dtype=torch.int64, device=self.dev)
        engine.reserve(self.max_width)

    def store_bytes(self):
        return int(self.store.numel() + self.tmp.numel() + self.lvl.numel()) * 8

    def run(self, ct_inputs, input_index=None):
        """ct_inputs: (n_inputs, k*N+1) uint64 ciphertexts (host) -> (n_outputs, k*N+1) uint64 (host); with batch > 1:
        (batch, n_inputs, k*N+1) -> (batch, n_outputs, k*N+1).
        Compressed inputs (2^64 torus, one rank): ct_inputs may be a tfhe.CompressedCiphertexts (with batch > 1 a sequence of `batch`
        of them); only its values and the index go to the device, where Engine.decompress writes the input rows of the store on
        the walk's stream.  input_index: n_inputs positions of the compressed form, input j = position input_index[j] (any order,
        repeats allowed; the same for every replica); None = the identity, which needs len(cc) == n_inputs.  Such inputs are not
        fresh encryptions: error_budget.failure_probability(..., input_variance=decompressed_variance(...)) prices them."""
        self._walk(ct_inputs, input_index)
        if self.on_gpu:
            self.torch.cuda.synchronize(self.dev)
        res = self.out[: self.n_out].cpu().numpy().view(np.uint64)
        return res if self.batch == 1 else res.reshape(self.batch, -1, self.big)

    def run_decrypted(self, ct_inputs, input_index=None):
        """run() with the outputs decrypted where they are (Engine.decrypt_device on the output rows: the context must hold the
        secret key): int64 messages (n_outputs,), with batch > 1 (batch, n_outputs) - 8 bytes per output come home instead of a
        ciphertext.  ct_inputs / input_index as in run()."""
        torch = self.torch
        stream = self._walk(ct_inputs, input_index)
        with torch.cuda.device(self.dev):
            msgs = torch.empty(max(self.n_out, 1), dtype=torch.int64, device=self.dev)
            self.eng.decrypt_device(self.out, self.n_out, self.delta_log, msgs, stream=stream)
            torch.cuda.synchronize(self.dev)
        res = msgs[: self.n_out].cpu().numpy()
        return res if self.batch == 1 else res.reshape(self.batch, -1)

    def run_compressed(self, ct_inputs, log_modulus=16, input_index=None):
        """run() with the outputs compressed where they are (Engine.compress on the output rows, on the walk's stream: the context
        must hold a compression key): a tfhe.CompressedCiphertexts - about 4 bytes per output of a full block at 16 bits come home
        instead of a ciphertext.  With batch > 1 every matrix is compressed separately and a list is returned, so that every client
        receives its own blocks.  ct_inputs / input_index as in run(): compressed in, compressed out."""
        from .tfhe import CompressedCiphertexts, compressed_words
        torch = self.torch
        if self.world > 1:
            raise NotImplementedError("run_compressed is a one-rank form: under torch.distributed call run()")
        stream = self._walk(ct_inputs, input_index)
        per, N = self.n_out // self.batch, self.eng.P.N
        words = compressed_words(per, N)
        with torch.cuda.device(self.dev):
            packed = torch.empty((self.batch, max(words, 1)), dtype=torch.int32, device=self.dev)
            for b in range(self.batch):
                self.eng.compress(self.out[b * per:], per, packed[b], log_modulus, stream=stream)
            torch.cuda.synchronize(self.dev)
        host = packed.cpu().numpy().view(np.uint32)
        res = [CompressedCiphertexts(per, N, log_modulus, host[b, :words]) for b in range(self.batch)]
        return res[0] if self.batch == 1 else res

    def _compressed_inputs(self, ct_inputs, input_index):
        """ct_inputs of run() in compressed form -> (list of `batch` CompressedCiphertexts, index as uint32 array or None), or None
        where ct_inputs is a full array; every mismatch raises with a text"""
        from .tfhe import CompressedCiphertexts
        if isinstance(ct_inputs, CompressedCiphertexts):
            ccs = [ct_inputs]
        elif isinstance(ct_inputs, (list, tuple)) and ct_inputs and all(isinstance(c, CompressedCiphertexts) for c in ct_inputs):
            ccs = list(ct_inputs)
        else:
            if input_index is not None:
                raise ValueError("input_index selects positions of compressed inputs: ct_inputs is not a CompressedCiphertexts")
            return None
        if self.world > 1:
            raise NotImplementedError("compressed inputs are a one-rank form: under torch.distributed decompress them first "
                                      "(Engine.decompress_host) and pass the full ciphertexts")
        n_in = self.prog.n_inputs
        if len(ccs) != self.batch:
            raise ValueError(f"{len(ccs)} compressed input lists for an executor of batch {self.batch}")
        index = None
        if input_index is not None:
            index = np.ascontiguousarray(input_index, dtype=np.int64).reshape(-1)
            if index.size != n_in:
                raise ValueError(f"input_index has {index.size} positions, the program has {n_in} inputs")
        for cc in ccs:
            self.eng._compressed(cc)
            if index is None and len(cc) != n_in:
                raise ValueError(f"{len(cc)} compressed ciphertexts for a program of {n_in} inputs (pass input_index to select)")
            if index is not None and index.size and (index.min() < 0 or index.max() >= len(cc)):
                raise ValueError(f"input_index reaches position {int(index.max())} (lowest {int(index.min())}) of {len(cc)} compressed ciphertexts")
        return ccs, None if index is None else index.astype(np.uint32)

    def _walk(self, ct_inputs, input_index=None):
        """the level walk of run(): leaves the output ciphertexts in self.out, queued on the stream it returns"""
        torch = self.torch
        n_in = self.prog.n_inputs
        packed = self._compressed_inputs(ct_inputs, input_index)
        if packed is None:
            ct = np.ascontiguousarray(ct_inputs, dtype=np.uint64).reshape(self.batch, n_in, self.big)
        import contextlib
        with (torch.cuda.device(self.dev) if self.on_gpu else contextlib.nullcontext()):
            stream = torch.cuda.current_stream().cuda_stream if self.on_gpu else 0
            if packed is None:
                self.store.view(self.batch, -1, self.big)[:, :n_in].copy_(torch.from_numpy(ct.view(np.int64)), non_blocking=False)
            elif n_in:
                # the compressed values and the index alone cross to the device; the input rows are written there, before level 1
                ccs, index = packed
                d_index = None if index is None else torch.from_numpy(index.view(np.int32)).to(self.dev)
                self._packed_inputs = [d_index]       # alive until the next walk: the kernels below are only queued
                for b, cc in enumerate(ccs):
                    d_words = torch.from_numpy(cc.words.view(np.int32)).to(self.dev)
                    self._packed_inputs.append(d_words)
                    self.eng.decompress(d_words, cc.count, cc.log_modulus, self.store[b * self.n_rows1:], index=d_index, stream=stream)
            eng, tmp, lvl = self.eng, self.tmp, self.lvl
            for t, (width, pos, padded) in enumerate(self.levels):
                if self.glevels is not None:     # one linear combination, keyswitch and rotation per group; every member's row as usual
                    ng, gpos, poff = self.glevels[t]
                    if width:
                        eng.lincomb(self.store, self.d_rp[gpos:], self.d_idx, self.d_coef, self.d_const[gpos:], ng, tmp, stream)
                        eng.pbs_shared(tmp, self.d_gptr[poff:], self.d_gbase[gpos:], self.d_ids[pos:], ng, width, lvl, stream)
                        eng.scatter_rows(lvl, width, self.store, self.d_rows[pos:], stream)
                    continue
                lo, hi = 0, width
                sharded = self.world > 1 and width >= self.shard_threshold
                if sharded:
                    per = padded // self.world
                    lo = min(self.rank * per, width)
                    hi = min(lo + per, width)
                if hi > lo:
                    eng.lincomb(self.store, self.d_rp[pos + lo:], self.d_idx, self.d_coef, self.d_const[pos + lo:], hi - lo, tmp[lo:], stream)
                    eng.pbs(tmp[lo:], self.d_ids[pos + lo:], hi - lo, lvl[lo:], stream)
                if sharded:
                    per = padded // self.world
                    pad_from = max(hi, self.rank * per)       # this rank's gather region is [rank * per, (rank + 1) * per)
                    if pad_from < (self.rank + 1) * per:      # rows past the level's width: they travel as zeros, never scattered
                        lvl[pad_from: (self.rank + 1) * per].zero_()
                    self._all_gather_rows(lvl[:padded], padded // self.world)
                eng.scatter_rows(lvl, width, self.store, self.d_rows[pos:], stream)
            rp, ix, cf, cs = self.out_csr
            eng.lincomb(self.store, rp, ix, cf, cs, self.n_out, self.out, stream)
            return stream

    def _all_gather_rows(self, region, per):
        """in-place all-gather of a level buffer: rank r contributed rows [r*per, (r+1)*per) (rows of the last rank past
        the level's width are padding: gathered, never scattered)"""
        dist, torch = self.dist, self.torch
        mine = region[self.rank * per: (self.rank + 1) * per]
        if dist.get_backend(self.group) == "nccl":
            # RCCL, in place (rank r's part already sits at its offset), ordered after this level's kernels: they were
            # launched on torch's current stream, which the collective synchronises with.  Exercised by
            # tests/test_gpu_inverse.py::test_two_gpu_rccl_sharded_inverse, which needs two GPUs (the build's test boxes
            # have one: there the gloo branch below runs).
            dist.all_gather_into_tensor(region, mine, group=self.group)
            return
        # other backends (gloo rehearsal): stage through the host
        if self.on_gpu:
            torch.cuda.synchronize(self.dev)
        parts = [torch.empty((per, self.big), dtype=torch.int64) for _ in range(self.world)]
        dist.all_gather(parts, mine.cpu().contiguous(), group=self.group)
        for r, part in enumerate(parts):
            if r != self.rank:
                region[r * per: (r + 1) * per].copy_(part)
