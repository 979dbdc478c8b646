"""The library's host cryptography without a GPU: tests/c_abi/host_crypto_check.cpp, a program of its own that includes
csrc/host_crypto.hpp and nothing else of the library and links oracle/tfhe_oracle.c compiled as plain C (no OpenMP: its pragmas are
ignored).  Deterministic keys, encryptions, phases and decoding word for word against the oracle; CSPRNG keys against the seeded
format's stream; every row's phase against its message within the noise bound that Box-Muller cannot exceed.  Built and run once
with the address and undefined-behaviour sanitizers and once with the thread sanitizer (the threaded shape gives every generator
at least 128 rows, so parallel_for really starts threads)."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_host_crypto_against_the_oracle(tmp_path, sanitizer):
    exe, oracle = str(tmp_path / "host_crypto_check"), str(tmp_path / "tfhe_oracle.o")
    flags = ["-O1", "-g", f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all"]
    # the oracle runs on the main thread only and picks its transforms' clones at load time, before the thread sanitizer's runtime is
    # up: instrumented for addresses and undefined behaviour, plain under the thread sanitizer
    ora_flags = flags if sanitizer != "thread" else ["-O1", "-g"]
    subprocess.check_call(["gcc", "-std=gnu11", *ora_flags, "-c", "-o", oracle, os.path.join(REPO, "oracle", "tfhe_oracle.c")])
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(REPO, "tests", "c_abi", "host_crypto_check.cpp"), oracle, "-lpthread", "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert out.stdout.splitlines()[-1].endswith(" checks, 0 failed"), out.stdout[-4000:]
