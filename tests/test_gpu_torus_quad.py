"""GPU parity tests of the 2^64 torus at N = 4096 (preset "secure128_torus_wide": n 742, k 1, l 3 x 10 bits, bootstrap key at 44
bits of precision = two 22-bit limbs; csrc/bmi_kernels_t64q.hip, fft_eighth_f64.hpp).  The specification is the oracle's INTEGER
arithmetic on the same (rounded, exported) key - the generic path of oracle/tfhe_oracle.c - : every output word must be identical
for every batch shape, and the limb sums must sit far from the half-integers when they are rounded."""
import gzip
import json
import os

import numpy as np
import pytest

import pbs_cases as pc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SEED = 0x5EED
QB = 65
CFG = pc.TorusPreset(name="secure128_torus_wide", seed_offset=11, bits=5, shape=(742, 4096, 1, 3, 10, QB, 16, 1), precision=44, grid_bits=20,
                     refused=(64, 48, 46, 42), batch_seed=700, counts=[1, 5, 257, 520], oracle_rows=1,
                     ks_power=lambda err: np.mean(err ** 2))   # (the mean square: test_keyswitch_and_whole_pbs_... says why)


@pytest.fixture(scope="module")
def eng():
    from bmi_amd import tfhe
    e = tfhe.Engine(tfhe.preset_params(CFG.name))
    e.keygen(SEED + CFG.seed_offset)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ora(eng):
    with pc.oracle_for(eng) as o:
        yield o


def test_preset_shape_keys_and_refusals(eng, ora):
    pc.check_preset_shape_keys_and_refusals(eng, ora, CFG, SEED + CFG.seed_offset)


@pytest.mark.parametrize("count", CFG.counts)
def test_blind_rotation_bit_exact_every_batch_shape(eng, ora, count):
    """5-bit messages (the width this set carries at the secure LWE noise) through identity / random tables; adversarial rows"""
    pc.check_blind_rotation_every_batch_shape(eng, ora, CFG, count)


def test_keyswitch_and_whole_pbs_bit_exact_noise_and_margin(eng, ora):
    """keyswitch (16 levels of 1 bit through the matrix-core kernel) and the whole PBS against the oracle; every 5-bit message through
    a random table; the look-up margin the keyswitch noise leaves - its MEAN SQUARE: the digits' mean of -1/2 makes a constant offset
    per key, which the analytic (B^2 + 2) / 12 counts and a variance over ciphertexts of one key would miss -; bootstrap output noise on
    the CGGI formula with the rounded key's effective noise"""
    P = eng.P
    err, oerr, ct, lid = pc.check_keyswitch_and_whole_pbs_bit_exact(eng, ora, CFG, seed=47, repeats=32, ks_rows=12, pbs_rows=3)
    analytic = pc.keyswitch_variance(P)
    ms = float(CFG.ks_power(err))
    ratio = ms / analytic
    sigma_pos, margin = pc.lookup_margin(P, ms, CFG.bits)
    margin_analytic = pc.lookup_margin(P, analytic, CFG.bits)[1]
    print(f"\nsecure128_torus_wide: keyswitch log2 rms {0.5 * np.log2(ms):.2f} (of which offset {np.mean(err):.2e}; analytic {0.5 * np.log2(analytic):.2f}, "
          f"ratio {ratio:.3f}); positions sigma {sigma_pos:.2f} of {2 * P.N}; 5-bit look-up margin {margin:.1f} sigma (analytic "
          f"{margin_analytic:.1f})")
    assert 0.45 < ratio < 2.0 and margin > 4.5 and margin_analytic > 5.3
    oratio = float(np.var(oerr)) / pc.cggi_output_variance(pc.effective_params(eng), 64, hw_small=int(ora.sk_small.sum()), hw_big=int(ora.sk_big.sum()))
    print(f"secure128_torus_wide: PBS output log2 std {0.5 * np.log2(np.var(oerr)):.2f} (variance / formula {oratio:.3f})")
    assert 0.85 < oratio < 1.15
    pc.time_pbs(eng, ct, lid, "secure128_torus_wide")


def test_rounding_margin_of_the_limb_sums(eng):
    """bmi_fft_margin_host on this shape: over 512 bootstraps (256 of them uniformly random words, which drive the digits to their
    full range) the limb sums stay within 2^-8 of the integers they are rounded to - against the 1/2 at which a result would
    change (a-priori bound 0.45: tools/fft_bound.py) - and the words equal the product kernel's"""
    pc.check_rounding_margin(eng, CFG, count=512, random_rows=256, bound=2.0 ** -8)


def test_l2_shape_and_six_bit_tables_bit_exact():
    """(l, Bg) = (2, 2^10) at N = 4096, the other instantiated shape, under 6-bit tables (the widest look-up the tracer emits)"""
    pc.check_l2_shape(CFG, SEED, n=35, bits=6)


def test_reference_five_bit_circuits_at_128_bit_security(eng):
    """What this set is for: the reference's UNMODIFIED qfloat_matrix_inverse (tests/golden/ref_traced_inverse.json.gz: 2x2 as
    written and lazily fused; 5-bit look-ups) and the 5-bit circuits of its own FHE test file (ref_own_fhe_tests.json.gz), on
    Concrete's modulus under the 128-bit-secure LWE pair; the error budget of each is what EncryptedMatrixInversion(p_error=...)
    would hold it to (reference: matrix_inversion/main.py:53-66, tests/test_qfloat_fhe.py:136-335)"""
    from bmi_amd.circuit import Circuit
    from bmi_amd.executor import Executor
    from bmi_amd.program import Program
    dl = eng.delta_log(5)
    with gzip.open(os.path.join(G, "ref_traced_inverse.json.gz"), "rt") as f:
        traced = json.load(f)["cases"]
    for case in (traced[0], traced[2]):
        c = Circuit.from_dict(case["circuit"])
        assert c.msg_bits == 5
        rep = Program.from_circuit(c).failure_probability(eng)
        print(f"\n{case['name']}: {rep['lookups']} look-ups, worst margin {rep['worst_margin_sigma']:.2f} sigma, p_fail {rep['p_fail']:.1e}")
        assert rep["p_fail"] < 1e-5 and 5.2 < rep["worst_margin_sigma"] < 5.5
        ex = Executor(c, eng)
        v = case["vectors"][0]
        assert list(eng.decrypt(ex.run(eng.encrypt(v["inputs"], dl)), dl)) == v["expected"], case["name"]
    with gzip.open(os.path.join(G, "ref_own_fhe_tests.json.gz"), "rt") as f:
        own = [c for c in json.load(f)["cases"] if c["msg_bits"] == 5 and c["function"] != "div_qfloats"]
    assert len(own) >= 2
    for case in own:
        ex = Executor(Circuit.from_dict(case["circuit"]), eng)
        for r in case["runs"]:
            assert list(eng.decrypt(ex.run(eng.encrypt(r["inputs"], dl)), dl)) == r["outputs"], case["function"]
