"""One blind rotation for the look-ups of the same ciphertext (multi-value bootstrap of Carpov, Izabachene and Mollimard, fitted
to this library's test polynomials; device side: csrc/glwe_lookup.hip, include/bmi_tfhe.h bmi_pbs_shared_batch).

A test polynomial TV_f of a p-bit table is a step function: M = 2^p boxes of N / M coefficients, shifted by half a box, with the
values s_0 .. s_M = f(0 .. M/2-1), -f(-M/2 .. -1), -f(0) (the last on half a box), times 2^out_delta_log.  So (1 - X) TV_f has at
most M non-zero coefficients - the differences s_b - s_(b-1) at the box boundaries b N/M - N/(2M); coefficient 0 is
TV_f(0) + TV_f(N-1) = 0 - and with TV_0 = 2^(unit_log - 1) sum_x X^x, for which (1 - X) TV_0 = 2^unit_log mod X^N + 1,

    TV_f = TV_0 P_f,        P_f = (1 - X) TV_f / 2^unit_log.

Noise.  The accumulator's phase error is E(X) = E_w(X) + W(X) S(X): a part that is white across coefficients (the key's Gaussian
noise, the body words' rounding) and a part CARRIED BY THE GLWE KEY S - the decomposition's rounding and the stored key's rounding
of the mask words, white polynomials W multiplied by the binary key - whose coefficients are therefore correlated (covariance
v_w sum_i S_i S_(i+d), with the negacyclic signs).  The look-up's error is coefficient 0 of E P_f:

    variance = |P_f|^2 v_e + |S P_f|^2 v_w          (|.|^2: sum of squared coefficients; one rotation: v_e + hw(S) v_w)

and over random keys of density p:  E |S P_f|^2 = N (p (1 - p) |P_f|^2 + p^2 mean_j m_j^2),  m_j = sum_k (+-) P_k with the minus
where j < c_k.  On the default set 92 % of a rotation's variance is key-carried, and |P_f|^2 v_rot alone (the white model) is off
by 3.1 x for the identity table and 0.59 x for a random one (measured: tests/test_gpu_shared_rotation.py, EXPERIMENTS A21).
`sparse_moments` returns (|P_f|^2, mean m^2), `key_carried_norm2` the exact |S P_f|^2 of a given key.

`sparse_table` returns P_f; `rotation_groups` finds the look-ups of a program that can share a rotation: nodes of one level whose
input is the same linear combination.  The executor (Executor(share_rotations=True)) and the error budget
(error_budget.failure_probability(share_rotations=True)) both read the groups from here.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


def sparse_table(table, p, out_delta_log, unit_log, N):
    """(positions, coefficients) of P_f = (1 - X) TV_f / 2^unit_log for the table f over p bits (table[m + 2^(p-1)] = f(m)) encoded
    at out_delta_log >= unit_log: int64 arrays of at most 2^p entries, positions ascending in [1, N), zero differences left out.
    Computed from the table's integers: a difference of 2^p at full scale has no sign once it is a 2^64 word."""
    M, Mh = 1 << int(p), 1 << (int(p) - 1)
    t = [int(v) for v in np.asarray(table).reshape(-1)]
    if len(t) != M:
        raise ValueError("table must have 2^p entries")
    if 2 * M > N:
        raise ValueError("a table over p bits needs N >= 2^(p + 1)")
    if out_delta_log < unit_log:
        raise ValueError("a table cannot be encoded below its group's unit")
    w = N >> int(p)
    s = t[Mh:] + [-v for v in t[:Mh]] + [-t[Mh]]            # s_0 .. s_M
    pos, coef = [], []
    for b in range(1, M + 1):
        d = s[b] - s[b - 1]
        if d:
            pos.append(b * w - w // 2)
            coef.append(d << (int(out_delta_log) - int(unit_log)))
    return np.asarray(pos, np.int64), np.asarray(coef, np.int64)


def sparse_moments(pos, coef, N):
    """(|P|^2, mean over j < N of m_j^2) of the sparse polynomial sum_k coef_k X^pos_k, m_j = sum_k coef_k (+1 if j >= pos_k else -1):
    what the noise of SampleExtract(ACC P) needs (module docstring).  P = 1: (1, 1)."""
    pos, coef = np.asarray(pos, np.int64), np.asarray(coef, np.float64)
    step = np.zeros(int(N) + 1, np.float64)
    np.add.at(step, pos, 2.0 * coef)
    m = np.cumsum(step[:-1]) - coef.sum()
    return float((coef ** 2).sum()), float((m ** 2).mean())


def key_carried_norm2(pos, coef, sk_big):
    """|S P|^2 for the binary GLWE key S (N bits): the sum of the squared coefficients of the negacyclic product"""
    S = np.asarray(sk_big, np.int64).reshape(-1)
    N = S.size
    dense = np.zeros(N, np.int64)
    dense[np.asarray(pos, np.int64)] = np.asarray(coef, np.int64)
    full = np.convolve(S, dense)
    sp = full[:N].copy()
    sp[: N - 1] -= full[N:]
    return float((sp.astype(np.float64) ** 2).sum())


def base_polynomial(unit_log, N):
    """TV_0 = + 2^(unit_log - 1) on every coefficient, as uint64 words (what Engine.lut_register_base registers)"""
    return np.full(N, 1 << (int(unit_log) - 1), np.uint64)


@dataclass
class RotationGroups:
    group_ptr: np.ndarray      # [groups + 1] into members
    members: np.ndarray        # node indices: level by level, inside a level group by group (groups in the order of their first
                               # member in Program.level_order, members in that order too)
    level_groups: np.ndarray   # [depth] number of groups of every level
    unit_half: np.ndarray      # [groups] bool: the group's unit is the half scale (a member is a lut_neg table): unit = min of the scales
    norm2: np.ndarray          # [len(members)] |P_f|^2 of every member relative to its group's unit (aligned with members): the
                               # factor on its bootstrap noise when its group has two members or more (a group of one is a plain
                               # bootstrap of the table itself: factor 1 whatever this says)
    mean2: np.ndarray          # [len(members)] mean_j m_j^2 of the same P_f (sparse_moments): the key-carried part of the noise

    @property
    def groups(self):
        return int(self.group_ptr.size - 1)

    @property
    def sizes(self):
        return np.diff(self.group_ptr)


def _row_hashes(prog):
    """two independent order-sensitive 64-bit hashes of every node's (leaf, coefficient) row"""
    lens = np.diff(prog.node_ptr)
    nn = lens.size
    tot = int(lens.sum())
    posn = (np.arange(tot) - np.repeat(prog.node_ptr[:-1], lens)).astype(np.uint64)
    leaf = prog.term_leaf.astype(np.int64).view(np.uint64)
    coef = prog.term_coef.astype(np.int64).view(np.uint64)
    out = []
    with np.errstate(over="ignore"):
        for c1, c2, c3 in ((0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9), (0xD6E8FEB86659FD93, 0xA0761D6478BD642F, 0xE7037ED1A0B428DB)):
            x = (leaf + np.uint64(1)) * np.uint64(c1) ^ (coef * np.uint64(c2)) ^ ((posn + np.uint64(1)) * np.uint64(c3))
            x ^= x >> np.uint64(29)
            x *= np.uint64(0xBF58476D1CE4E5B9)
            x ^= x >> np.uint64(32)
            h = np.zeros(nn, np.uint64)
            if tot:
                nz = np.flatnonzero(lens)
                h[nz] = np.add.reduceat(x, prog.node_ptr[:-1][nz].astype(np.int64))
            out.append(h)
    return out


def rotation_groups(prog):
    """Groups the look-ups of `prog` (a program.Program) that read the same input in the same level: equal terms (leaves and
    coefficients, in the row's order) and equal constant.  Every node is in exactly one group; a group of one is an ordinary
    look-up.  Returns a RotationGroups."""
    nn = prog.n_nodes
    order, counts = prog.level_order()
    if nn == 0:
        z = np.zeros(0, np.int64)
        return RotationGroups(np.zeros(1, np.int64), z, np.zeros(len(counts), np.int64), np.zeros(0, bool), np.zeros(0, np.float64),
                              np.zeros(0, np.float64))
    lens = np.diff(prog.node_ptr)
    h1, h2 = _row_hashes(prog)
    # nodes in level order; rows that agree in (level, length, constant, both hashes) are candidates for one group
    keys = (h2[order], h1[order], np.asarray(prog.node_const, np.int64)[order], lens[order], np.asarray(prog.node_level, np.int64)[order])
    srt = np.lexsort(keys)                       # stable: inside a run the positions ascend
    new = np.ones(nn, bool)
    new[1:] = np.zeros(nn - 1, bool)
    for k in keys:
        ks = k[srt]
        new[1:] |= ks[1:] != ks[:-1]
    run = np.cumsum(new) - 1                     # run id of every sorted entry
    leader_pos = srt[new]                        # first (smallest) position of every run
    # exactness: every member's row equals its leader's, term for term (a hash collision would show here)
    lead_of_pos = np.empty(nn, np.int64)
    lead_of_pos[srt] = leader_pos[run]
    a, b = order, order[lead_of_pos]
    ln = lens[a]
    tot = int(ln.sum())
    if tot:
        within = np.arange(tot) - np.repeat(np.cumsum(ln) - ln, ln)
        oa = np.repeat(prog.node_ptr[:-1][a], ln) + within
        ob = np.repeat(prog.node_ptr[:-1][b], ln) + within
        if not (np.array_equal(prog.term_leaf[oa], prog.term_leaf[ob]) and np.array_equal(prog.term_coef[oa], prog.term_coef[ob])):
            raise RuntimeError("row hashes collided: two different look-up inputs were grouped")   # (2^-128 per pair)
    # groups in the order of their leaders; members by position
    group_rank = np.empty(leader_pos.size, np.int64)
    group_rank[np.argsort(leader_pos, kind="stable")] = np.arange(leader_pos.size)
    gid_of_pos = np.empty(nn, np.int64)
    gid_of_pos[srt] = group_rank[run]
    by_group = np.argsort(gid_of_pos, kind="stable")
    members = order[by_group]
    sizes = np.bincount(gid_of_pos, minlength=leader_pos.size)
    group_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    level_of_group = np.asarray(prog.node_level, np.int64)[members[group_ptr[:-1]]]
    level_groups = np.bincount(level_of_group, minlength=prog.depth + 1)[1:]
    # units and |P|^2: a table's own |P|^2 at its scale, times 4 where it is a full-scale table in a half-scale group
    lut_half = np.asarray(prog.lut_half, bool)
    n2_lut = np.zeros(max(int(prog.lut_p.size), 1), np.float64)
    m2_lut = np.zeros_like(n2_lut)
    for j in range(int(prog.lut_p.size)):
        p = int(prog.lut_p[j])
        ps, cf = sparse_table(prog.lut_tab[j, : 1 << p].astype(np.int64), p, 0, 0, 1 << (p + 1))
        n2_lut[j], m2_lut[j] = sparse_moments(ps, cf, 1 << (p + 1))       # (neither depends on N: the positions scale with it)
    m_lut = np.asarray(prog.node_lut, np.int64)[members]
    m_half = lut_half[m_lut]
    gid_sorted = gid_of_pos[by_group]
    unit_half = np.bincount(gid_sorted, weights=m_half, minlength=sizes.size) > 0
    scale2 = np.where(unit_half[gid_sorted] & ~m_half, 4.0, 1.0)
    return RotationGroups(group_ptr, members, level_groups.astype(np.int64), unit_half, n2_lut[m_lut] * scale2, m2_lut[m_lut] * scale2)
