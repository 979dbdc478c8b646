"""The dispatch table of the library without a GPU: tests/c_abi/rotation_plan_table.cpp, a program of its own that includes
csrc/rotation_plan.hpp and nothing of the library, prints every admitted context shape x unrolling factor x key precision
(unset, set before or after the factor) x keys (absent, generated, generated before the factor changed) with what the setters
answer, the key copies built, and the kernel per variant and batch size; the output must be tests/rotation_plan_cases.txt, the
file tests/test_gpu_rotation_plan.py holds the real library to.  Built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "tests", "rotation_plan_cases.txt")


def test_the_plan_prints_the_committed_table(tmp_path):
    exe = str(tmp_path / "rotation_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(REPO, "tests", "c_abi", "rotation_plan_table.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-4000:]
    got, want = out.stdout.splitlines(), open(TABLE).read().splitlines()
    first = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    assert got == want, f"line {first + 1}: the plan says {got[first:first + 1]}, the table {want[first:first + 1]}"
    assert sum(l.startswith("ctx ") and l.endswith("-> ok") for l in want) == 16   # 1 Goldilocks, 7 on the 49-bit field, 8 on the torus
