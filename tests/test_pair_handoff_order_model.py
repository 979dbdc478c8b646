"""A model of the pair hand-off of the torus throughput kernel (k_blind_rotate_t64f) in its row order "both limbs' products
before the inverses" (the kernel's header comment; the diagram of pair_sync.hpp).

The two wavefronts of a ciphertext each own one LDS tile.  A wavefront alone WRITES its tile - the exchanges of its forward
transforms, the two partial sums it publishes per CMUX, the exchanges of its inverse transforms - and its partner READS it, only
between seeing pub = h and storing ack = h.  The flags are counters: each value is stored once by its only writer and compared
for equality.  A protocol error in the kernel shows as a hang or as a wrong word on the GPU; here the protocol is stated as
the program-order event list of one wavefront per CMUX, and EVERY interleaving of the two wavefronts over three consecutive
CMUXes is explored (a depth-first search over the two program counters: the flags and the tiles' contents are functions of
them).  Three properties:

  1. no tile write happens between the partner's wait(pub = h) and its ack(h)  (the partner may be reading the tile),
  2. no read of a partial happens before its post, and the tile still holds that partial when it is read,
  3. no reachable state exists in which both wavefronts wait.

The same model with the wait for the partner's acknowledgement of limb 0's partial removed (the one in front of the store of
limb 1's partial) must fail property 1: the model can see a violation."""
CMUXES = 3


def program(ack_wait_before_second_partial=True):
    """one wavefront's events over CMUXES steps, in program order; hand-off h = 2 i + 1 (limb 0) and 2 i + 2 (limb 1) of step i"""
    ev = []
    for i in range(CMUXES):
        h0, h1 = 2 * i + 1, 2 * i + 2
        ev.append(("write", f"forward {i}"))        # exchanges of the forward transforms
        ev.append(("write", f"partial {h0}"))       # rows P0: partner's column, limb 0
        ev.append(("post", h0))
        ev.append(("wait_pub", h0))                 # after rows O0
        ev.append(("read", h0))
        ev.append(("ack", h0))
        if ack_wait_before_second_partial:
            ev.append(("wait_ack", h0))             # after rows P1, in front of the store of their sum
        ev.append(("write", f"partial {h1}"))
        ev.append(("post", h1))
        ev.append(("wait_pub", h1))                 # after rows O1
        ev.append(("read", h1))
        ev.append(("ack", h1))
        ev.append(("wait_ack", h1))                 # the hook of the first inverse transform, before its first store
        ev.append(("write", f"inverse {i}"))        # exchanges of both inverse transforms
    return ev


def flag(prog, pc, kind):
    """value of a wavefront's pub / ack counter when it stands at pc: the last one it stored"""
    v = 0
    for k, a in prog[:pc]:
        if k == kind:
            v = a
    return v


def tile(prog, pc):
    """what a wavefront's tile holds when it stands at pc: its last write"""
    c = None
    for k, a in prog[:pc]:
        if k == "write":
            c = a
    return c


def reading(prog, pc):
    """a wavefront at pc has seen pub = h and not yet stored ack = h: it may be reading the partner's tile"""
    return pc < len(prog) and prog[pc][0] in ("read", "ack")


def blocked(prog, pc, other_pc):
    k, a = prog[pc]
    if k == "wait_pub":
        return flag(prog, other_pc, "post") != a
    if k == "wait_ack":
        return flag(prog, other_pc, "ack") != a
    return False


def explore(prog):
    """every interleaving of two wavefronts running `prog` -> (the states seen, the violations found as (property, text)); a
    step that violates a property is recorded and not taken"""
    end = len(prog)
    seen, stack, bad = set(), [(0, 0)], []
    while stack:
        st = stack.pop()
        if st in seen:
            continue
        seen.add(st)
        can_move = False
        for w in (0, 1):
            pc, opc = st[w], st[1 - w]
            if pc == end or blocked(prog, pc, opc):
                continue
            can_move = True
            k, a = prog[pc]
            if k == "write" and reading(prog, opc):
                bad.append((1, f"wavefront {w} writes '{a}' into its tile while its partner stands at {prog[opc]}"))
                continue
            if k == "read" and flag(prog, opc, "post") < a:
                bad.append((2, f"wavefront {w} reads partial {a} before its post"))
                continue
            if k == "read" and tile(prog, opc) != f"partial {a}":
                bad.append((2, f"wavefront {w} reads partial {a} but the tile holds '{tile(prog, opc)}'"))
                continue
            nxt = list(st)
            nxt[w] = pc + 1
            stack.append(tuple(nxt))
        if not can_move and st != (end, end):
            bad.append((3, f"both wavefronts wait: {[prog[p] if p < end else 'done' for p in st]}"))
    return seen, bad


def test_every_interleaving_of_three_cmuxes_is_safe_and_live():
    prog = program()
    seen, bad = explore(prog)
    assert not bad, bad[:3]
    assert (len(prog), len(prog)) in seen, "the end of the third CMUX is not reachable"
    # the search is not vacuous: somewhere a wavefront is ahead of its partner by more than a hand-off's worth of events
    assert max(abs(a - b) for a, b in seen) >= 4


def test_model_sees_a_missing_acknowledgement_wait():
    """without it limb 1's partial overwrites limb 0's while the partner may still be reading (and, the flags being compared for
    equality, a partner that has not yet looked for pub = h0 never sees it)"""
    _, bad = explore(program(ack_wait_before_second_partial=False))
    assert 1 in {p for p, _ in bad}, bad[:3]


def test_model_sees_a_read_before_its_post_and_a_deadlock():
    """the other two properties can fail too: a read moved in front of its wait; a post moved behind the wait for the partner's"""
    prog = program()
    i = prog.index(("wait_pub", 1))
    _, bad = explore(prog[:i] + [prog[i + 1], prog[i]] + prog[i + 2:])
    assert 2 in {p for p, _ in bad}, bad[:3]
    j = prog.index(("post", 1))
    _, bad = explore(prog[:j] + [prog[j + 1], prog[j]] + prog[j + 2:])
    assert 3 in {p for p, _ in bad}, bad[:3]
