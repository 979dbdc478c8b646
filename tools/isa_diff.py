#!/usr/bin/env python3
"""Compares the gfx950 machine code of two source trees, kernel by kernel (CPU only: it compiles, it runs nothing).
Every .hip translation unit of csrc/ is compiled to a listing with the product flags of that tree's csrc/Makefile (the per-TU
scheduler choice included); a listing is split per kernel, and comments, directives, the per-compilation __hip_cuid symbol and the
function index inside local labels (.LBB<n>_) are stripped.  Per kernel: "identical"; "registers only (k lines)" when the k
differing lines all vanish once register numbers are erased (the same instruction sequence, numbered differently); else "DIFFERENT
(k lines, m after erasing register numbers)" and the per-class instruction counts of both sides (classes of isa_count.py; whole
kernel and main loop); VGPR / AGPR / SGPR / scratch / LDS / occupancy of both sides.
usage: isa_diff.py <tree A> <tree B> [--only SUBSTR] [--defs "-DX -DY"] [--jobs N]
       --only: translation units whose file name contains SUBSTR;  --defs: extra defines (-DBMI_PHASE_PROF: the `make prof` build)
exit status 1 when any kernel differs (or exists on one side only)"""
import argparse, difflib, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_count import classify, demangle, main_loop

CSRC = os.path.join("bounty-matrix-inversion_amd", "csrc")
CLASSES = ("f64", "int64", "other", "lds", "vmem", "scratch", "barrier", "waitcnt", "scalar")
RESOURCES = (("VGPR", "NumVgprs"), ("AGPR", "NumAgprs"), ("SGPR", "TotalNumSgprs"), ("scratch", "ScratchSize"), ("LDS", "LDSByteSize"), ("occ", "Occupancy"))


def sched_flags(csrc):
    """(default scheduler flags, {TU base name: its own flags}) as csrc/Makefile states them"""
    mk = open(os.path.join(csrc, "Makefile")).read()
    default = re.search(r"^SCHED \?=(.*)$", mk, re.M).group(1).split()
    return default, {m.group(1): m.group(2).split() for m in re.finditer(r"^SCHED_(\w+) :=(.*)$", mk, re.M)}


def listing(csrc, src, defs, out):
    default, own = sched_flags(csrc)
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950"] + own.get(os.path.splitext(src)[0], default) + defs + \
          ["-ffp-contract=off", "--offload-device-only", "-S", "-o", out, "-x", "hip", src]
    subprocess.run(cmd, check=True, cwd=csrc, stderr=subprocess.DEVNULL)
    return out


def kernels_of(path):
    """{mangled name: (stripped instruction stream, resources)}; a kernel's text runs to the next kernel's label, which takes in the
    resource comments the assembler printer puts behind s_endpgm"""
    L = open(path).read().split("\n")
    starts = [i for i, l in enumerate(L) if l.startswith("_Z") and ":" in l and "@" in l]
    out = {}
    for i, end in zip(starts, starts[1:] + [len(L)]):
        stream, res = [], {}
        for l in L[i + 1:end]:
            m = re.match(r"^; (\w+): (\d+)", l)
            if m and m.group(1) not in res:
                res[m.group(1)] = int(m.group(2))
            s = l.split(";")[0].strip()
            if not s or "__hip_cuid" in s or s == "s_code_end" or (s.startswith(".") and not re.match(r"^\.LBB[0-9_]+:", s)):
                continue
            stream.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
        out[L[i].split(":")[0]] = (stream, {k: res.get(v) for k, v in RESOURCES})
    return out


def counts(stream):
    """per-class counts of the whole kernel and of its main loop (isa_count.main_loop: the widest backward branch)"""
    ins, span = main_loop(["\t" + s if not s.endswith(":") else s for s in stream])
    def tally(xs):
        c = dict.fromkeys(CLASSES, 0)
        for s in xs:
            c[classify(s.split()[0])] += 1
        c["s_nop"] = sum(s.startswith("s_nop") for s in xs)
        return c
    return len(ins), tally(ins), (tally(ins[span[0]:span[1] + 1]) if span else None)


def erased(stream):
    """the stream with register NUMBERS erased: v12 -> v, s[4:5] -> s[2], a3 -> a (one token per register class and width); opcodes,
    modifiers, immediates, labels and order are kept"""
    def one(s):
        s = re.sub(r"\b([vsa]|ttmp)\[(\d+):(\d+)\]", lambda m: f"{m.group(1)}[{int(m.group(3)) - int(m.group(2)) + 1}]", s)
        return re.sub(r"\b([vsa]|ttmp)\d+\b", r"\1", s)
    return [one(s) for s in stream]


def differing_lines(a, b):
    """lines outside the longest matching blocks of the two streams (per differing block the longer side counts)"""
    ops = difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes()
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal")


def fmt(c):
    return "-" if c is None else " ".join(f"{k} {v}" for k, v in c.items())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--only", default="")
    ap.add_argument("--defs", default="")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    trees = [os.path.join(os.path.abspath(t), CSRC) for t in (a.tree_a, a.tree_b)]
    tus = sorted({f for t in trees for f in os.listdir(t) if f.endswith(".hip") and a.only in f})
    differing = 0
    with tempfile.TemporaryDirectory() as td, ThreadPoolExecutor(a.jobs) as pool:
        jobs = {(s, f): pool.submit(listing, t, f, a.defs.split(), os.path.join(td, f"{s}_{f}.s"))
                for s, t in enumerate(trees) for f in tus if os.path.exists(os.path.join(t, f))}
        for f in tus:
            A, B = (kernels_of(jobs[s, f].result()) if (s, f) in jobs else {} for s in (0, 1))
            names = list(A) + [n for n in B if n not in A]
            for n, d in zip(names, demangle(names)):
                if n not in A or n not in B:
                    differing += 1
                    print(f"{f[len('bmi_kernels_'):-4] if f.startswith('bmi_kernels_') else f[:-4]:6} {d:50} only in {'A' if n in A else 'B'}")
                    continue
                (sa, ra), (sb, rb) = A[n], B[n]
                na, ca, la = counts(sa)
                nb, cb, lb = counts(sb)
                same = sa == sb
                differing += not same
                verdict = "identical"
                if not same:
                    k, m = differing_lines(sa, sb), differing_lines(erased(sa), erased(sb))
                    verdict = f"registers only ({k} lines)" if m == 0 else f"DIFFERENT ({k} lines, {m} after erasing register numbers)"
                res = " ".join(f"{k} {ra[k]}" for k in ra) + ("  resources equal" if ra == rb else "  |  " + " ".join(f"{k} {rb[k]}" for k in rb) + "  RESOURCES DIFFER")
                print(f"{f[len('bmi_kernels_'):-4] if f.startswith('bmi_kernels_') else f[:-4]:6} {d:50} {na:6d} {nb:6d}  {verdict}  {res}")
                if verdict.startswith("DIFFERENT"):
                    print(f"         kernel    A: {fmt(ca)}\n         kernel    B: {fmt(cb)}\n         main loop A: {fmt(la)}\n         main loop B: {fmt(lb)}")
    print(f"{differing} kernel(s) differ")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
