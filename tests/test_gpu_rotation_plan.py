"""The library's dispatch against tests/rotation_plan_cases.txt, line by line (the table tests/test_rotation_plan.py derives from
csrc/rotation_plan.hpp alone; its format is described in tests/c_abi/rotation_plan_table.cpp): every context shape, and under it
every sequence on a fresh Engine - set_bsk_unroll / set_bsk_precision with the precision they leave, keygen with the bytes of the
key copies built (key_bytes), set_kernel_variant and rotation_kernel for every variant and batch size, the refusal of
fft_margin_host, import_bsk_unrolled - with every BmiError text.  All parameter sets have n = 8: dispatch does not look at n, and a
key set is then small.  These two tests launch no blind rotation: the accepted lines of the margin hook (it would launch its
kernel) and the import_unrolled_seeded lines (they need a seeded key set first) are checked by the host-only test alone.

test_every_kernel_rotates_on_the_key_copy_and_tables_of_its_row then launches each of the 20 kernels once on such a context: a row
of the plan that named the wrong key copy or table would produce wrong words, not an error."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rotation_plan_cases.txt")
Q_BITS = {"goldilocks": 64, "field49": 49, "torus64": 65}
COUNTS = (1, 256, 257, 512, 513, 1025)
N_LWE = 8


def parse():
    """[(modulus, log_N, l, Bg, verdict, [(sequence name, [step lines, `same as` expanded])])]"""
    ctxs, blocks = [], {}
    for line in open(TABLE).read().splitlines():
        if line.startswith("ctx "):
            m = re.match(r"ctx (\w+) logN=(\d+) l=(\d+) Bg=(\d+) -> (.*)$", line)
            ctxs.append((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5), []))
            blocks = {}
        elif line.startswith(" seq "):
            name, n_blocks = line[5:], 0
            ctxs[-1][5].append((name, []))
        else:
            steps, step = ctxs[-1][5][-1][1], line.strip()
            if step.startswith("same as "):
                n_blocks += 1
                steps.extend(blocks[step[8:]])
                continue
            if step.startswith("variant ") and not (steps and steps[-1].startswith("variant ")):   # a block begins
                n_blocks += 1
                blocks[f"{name} #{n_blocks}"] = []
            if step.split(" ", 1)[0] in ("variant", "margin", "import_unrolled_seeded", "import_unrolled"):
                blocks[f"{name} #{n_blocks}"].append(step)
            steps.append(step)
    return ctxs


CTXS = parse()


def answer(call):
    """what the table would say of a call: `REFUSED: <text>` or None"""
    from bmi_amd import tfhe
    try:
        call()
    except tfhe.BmiError as e:
        return "REFUSED: " + re.match(r"\w+ failed \(-?\d+\): (.*)$", str(e), re.S).group(1)
    return None


def run_sequence(P, name, steps):
    from bmi_amd import tfhe
    e = tfhe.Engine(P)
    try:
        for step in steps:
            call, want = step.split(" -> ", 1)
            op, _, arg = call.partition(" ")
            where = f"{name}: {step}"
            if op in ("unroll", "precision"):
                got = answer(lambda: (e.set_bsk_unroll if op == "unroll" else e.set_bsk_precision)(int(arg)))
                assert (got or f"ok prec={e.bsk_precision}") == want, where
            elif op in ("keygen", "keys"):
                if op == "keygen":
                    e.keygen(0x5EED)
                assert e.key_bytes()[0] == int(want.rsplit("bytes=", 1)[1]), where
            elif op == "variant":
                for v in map(int, arg.split(",")):
                    got = answer(lambda: e.set_kernel_variant(v))
                    if want.startswith("REFUSED: "):
                        assert got == want, where
                        continue
                    assert got is None, where
                    per_count = dict.fromkeys(COUNTS, want[4:]) if want.startswith("* = ") else \
                        {int(c): k for c, k in (x.split(" = ", 1) for x in want.split(" ; "))}
                    assert tuple(per_count) == COUNTS, where
                    for count, kernel in per_count.items():
                        holder = []
                        got = answer(lambda: holder.append(e.rotation_kernel(count)))
                        assert (got or holder[0]) == kernel, f"{where} (variant {v}, {count} ciphertexts)"
                e.set_kernel_variant(0)
            elif op == "margin":
                if not want.startswith("* = REFUSED: "):
                    continue   # an accepted call launches the kernel
                for v in map(int, arg.split(",")):
                    e.set_kernel_variant(v)
                    assert answer(lambda: e.fft_margin_host(np.zeros((1, N_LWE + 1), np.uint64), np.zeros(1, np.uint32))) == want[4:], where
                e.set_kernel_variant(0)
            elif op == "import_unrolled":
                assert (answer(lambda: e.import_bsk_unrolled(np.zeros(e.unrolled_key_shape(), np.uint64))) or "ok") == want, where
            else:
                assert op == "import_unrolled_seeded", where
    finally:
        e.close()


@pytest.mark.parametrize("modulus,log_N", sorted({(c[0], c[1]) for c in CTXS if c[4] == "ok"}))
def test_admitted_contexts_follow_the_table(modulus, log_N):
    from bmi_amd import tfhe
    shapes = [c for c in CTXS if (c[0], c[1]) == (modulus, log_N) and c[4] == "ok"]
    assert shapes
    for _, _, l, bg, _, sequences in shapes:
        # torus: 2 factors x (precision unset + 6 values before and after); prime fields, which refuse every precision: 2 factors with
        # the 12 calls in one sequence; and the 2 late changes of factor
        assert len(sequences) == (28 if modulus == "torus64" else 4)
        P = tfhe.default_params(q_bits=Q_BITS[modulus], n=N_LWE, log_N=log_N, bs_levels=l, bs_base_log=bg)
        for name, steps in sequences:
            run_sequence(P, f"{modulus} logN={log_N} l={l} Bg={bg} / {name}", steps)


def test_refused_contexts_say_what_the_table_says():
    from bmi_amd import tfhe
    refused = [c for c in CTXS if c[4] != "ok"]
    assert len(refused) == 10 and all(not c[5] for c in refused)
    for modulus, log_N, l, bg, want, _ in refused:
        P = tfhe.default_params(q_bits=Q_BITS[modulus], n=N_LWE, log_N=log_N, bs_levels=l, bs_base_log=bg)
        assert answer(lambda: tfhe.Engine(P)) == want, (modulus, log_N, l, bg)


# One line per kernel (rotplan::Rot): a context on which the dispatch answers with it for batches of 1 and 3 -
# (kernel, modulus, log_N, l, Bg, key precision to set or None, unrolling factor, kernel variant to pin, accumulator form, variant
# under which fft_margin_host runs it or None)
KERNELS = [
    ("k_blind_rotate_wu_t64f", "torus64", 11, 3, 10, None, 2, 0, True, 0),
    ("k_blind_rotate_wu2_t64f", "torus64", 11, 3, 10, None, 2, 1, True, 1),
    ("k_blind_rotate_w2_t64f", "torus64", 11, 3, 10, None, 1, 1, True, None),
    ("k_blind_rotate_w_t64f", "torus64", 11, 3, 10, None, 1, 0, True, 0),
    ("k_blind_rotate_q_t64f", "torus64", 12, 3, 10, None, 1, 0, True, 0),
    ("k_blind_rotate_tp2u_t64f", "torus64", 10, 3, 10, None, 2, 1, True, None),
    ("k_blind_rotate_lat2u_t64f", "torus64", 10, 3, 10, None, 2, 0, True, 0),
    ("k_blind_rotate_lat2u_t64", "torus64", 10, 3, 10, 48, 2, 0, False, None),
    ("k_blind_rotate_lat_t64f", "torus64", 10, 3, 10, None, 1, 0, True, 6),
    ("k_blind_rotate_lat_t64", "torus64", 10, 3, 10, None, 1, 4, False, None),
    ("k_blind_rotate_t64f", "torus64", 10, 3, 10, None, 1, 5, True, 0),
    ("k_blind_rotate_t64", "torus64", 10, 3, 10, None, 1, 1, False, None),
    ("k_blind_rotate_wide49u", "field49", 11, 2, 15, None, 2, 0, False, None),
    ("k_blind_rotate_wide49", "field49", 11, 3, 15, None, 1, 0, False, None),
    ("k_blind_rotate_quad49", "field49", 12, 3, 15, None, 1, 0, False, None),
    ("k_blind_rotate_lat2u_49", "field49", 10, 3, 15, None, 2, 0, False, None),
    ("k_blind_rotate_lat2_49", "field49", 10, 3, 15, None, 1, 2, False, None),
    ("k_blind_rotate_tpx49", "field49", 10, 3, 15, None, 1, 3, False, None),
    ("k_blind_rotate_lat", "goldilocks", 10, 3, 15, None, 1, 2, False, None),
    ("k_blind_rotate_tp", "goldilocks", 10, 3, 15, None, 1, 1, False, None),
]


def extract(glwe, N):
    """SampleExtract_0 of accumulators [rows][2N]: o[0] = A[0], o[x] = -A[N - x], o[N] = B[0]"""
    out = np.zeros((glwe.shape[0], N + 1), np.uint64)
    out[:, 0] = glwe[:, 0]
    out[:, 1:N] = np.uint64(0) - glwe[:, N - 1:0:-1]
    out[:, N] = glwe[:, N]
    return out


@pytest.mark.parametrize("kernel,modulus,log_N,l,bg,precision,unroll,variant,accumulator,margin_variant", KERNELS, ids=[k[0] for k in KERNELS])
def test_every_kernel_rotates_on_the_key_copy_and_tables_of_its_row(kernel, modulus, log_N, l, bg, precision, unroll, variant, accumulator,
                                                                    margin_variant):
    """Batches of 1 and 3 (odd: the two-ciphertexts-per-workgroup kernels run their padding slot) through the kernel, confirmed by
    rotation_kernel: every output decrypts to the registered 4-bit table's value.  The nine kernels with an accumulator form: its
    sample extraction is the plain rotation, word for word; the seven that fft_margin_host can run: the same words again, and a
    largest rounding distance below 1/2."""
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.default_params(q_bits=Q_BITS[modulus], n=N_LWE, log_N=log_N, bs_levels=l, bs_base_log=bg))
    try:
        if precision:
            e.set_bsk_precision(precision)
        if unroll == 2:
            e.set_bsk_unroll(2)
        e.keygen(0x5EED)
        dl = e.delta_log()
        table = np.array([(5 * m + 3) % 16 - 8 for m in range(-8, 8)])
        lid = e.lut_register(table, 4, dl)
        for count in (1, 3):
            msgs = np.array([-8, 7, 2])[:count]
            ids = np.full(count, lid, np.uint32)
            small = e.keyswitch_host(e.encrypt(msgs, dl))
            e.set_kernel_variant(variant)
            assert e.rotation_kernel(count) == kernel
            out = e.blind_rotate_host(small, ids)
            assert list(e.decrypt(out, dl)) == [int(table[m + 8]) for m in msgs], count
            if accumulator:
                assert np.array_equal(extract(e.blind_rotate_glwe_host(small, ids), e.P.N), out), count
            if margin_variant is not None:
                e.set_kernel_variant(margin_variant)
                words, distance = e.fft_margin_host(small, ids)
                assert np.array_equal(words, out) and 0 <= distance < 0.5, (count, distance)
    finally:
        e.close()
