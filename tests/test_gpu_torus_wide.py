"""GPU parity tests of the 2^64 torus at N = 2048 (preset "secure128_torus": n 742, k 1, l 3 x 10 bits, bootstrap key at 46 bits
of precision = two 23-bit limbs; csrc/bmi_kernels_t64w.hip, fft_quarter_f64.hpp).  The specification is the oracle's INTEGER
arithmetic on the same (rounded, exported) key - the generic path of oracle/tfhe_oracle.c, whose torus product goes through
Goldilocks transforms of the key's 32-bit halves, a different route from the GPU's floating-point transform on purpose: every
output word must be identical for every batch shape, and the limb sums must sit far from the half-integers when they are rounded."""
import numpy as np
import pytest

import pbs_cases as pc

pytestmark = pytest.mark.gpu

SEED = 0x5EED
QB = 65
CFG = pc.TorusPreset(name="secure128_torus", seed_offset=9, bits=4, shape=(742, 2048, 1, 3, 10, QB, 8, 2), precision=46, grid_bits=18,
                     refused=(64, 48, 42), batch_seed=300, counts=[1, 5, 257, 600], oracle_rows=2, ks_power=np.var)


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
    pc.check_blind_rotation_every_batch_shape(eng, ora, CFG, count)


def test_keyswitch_and_whole_pbs_bit_exact_noise_and_margin(eng, ora):
    """keyswitch and the whole PBS against the oracle; every 4-bit message through a random table; keyswitch noise at its analytic
    value and the look-up margin it leaves; bootstrap output noise on the CGGI formula with the rounded key's effective noise"""
    P = eng.P
    err, oerr, ct, lid = pc.check_keyswitch_and_whole_pbs_bit_exact(eng, ora, CFG, seed=43, repeats=64, ks_rows=24, pbs_rows=4)
    analytic = pc.keyswitch_variance(P)
    power = CFG.ks_power(err)
    ratio = float(power) / analytic
    sigma_pos, margin = pc.lookup_margin(P, power, CFG.bits)
    print(f"\nsecure128_torus: keyswitch log2 std {0.5 * np.log2(power):.2f} (analytic {0.5 * np.log2(analytic):.2f}, ratio "
          f"{ratio:.3f}); positions sigma {sigma_pos:.2f} of {2 * P.N}; 4-bit look-up margin {margin:.1f} sigma")
    assert 0.75 < ratio < 1.3 and margin > 8.0
    oratio = float(np.var(oerr)) / pc.cggi_output_variance(pc.effective_params(eng), 64, hw_small=int(ora.sk_small.sum()), hw_big=int(ora.sk_big.sum()))
    print(f"secure128_torus: PBS output log2 std {0.5 * np.log2(np.var(oerr)):.2f} (variance / formula {oratio:.3f})")
    assert 0.85 < oratio < 1.15 and np.var(oerr) * 75 ** 2 < power / 4     # x75: the widest linear combination of the circuits
    pc.time_pbs(eng, ct, lid, "secure128_torus")


def test_rounding_margin_of_the_limb_sums(eng):
    """bmi_fft_margin_host on this shape: over 1,024 bootstraps (512 of them uniformly random words, which drive the digits to
    their full range) the limb sums stay within 2^-9 of the integers they are rounded to - against the 1/2 at which a result
    would change (a-priori bound 0.42: tools/fft_bound.py) - and the words equal the product kernel's"""
    pc.check_rounding_margin(eng, CFG, count=1024, random_rows=512, bound=2.0 ** -9)


def test_l2_shape_bit_exact():
    """(l, Bg) = (2, 2^10) at N = 2048: the other instantiated shape (16 forward tasks: one per wavefront)"""
    pc.check_l2_shape(CFG, SEED, n=33, bits=4)


@pytest.mark.parametrize("count", [257, 300, 601])
def test_two_ciphertexts_per_workgroup_form_same_words(eng, ora, count):
    """k_blind_rotate_w2_t64f (csrc/bmi_kernels_t64w2.hip: what auto dispatch runs beyond 256 ciphertexts; variants 1 / 3 pin it, 2 pins
    the one-ciphertext form): the same words as the one-ciphertext kernel on every batch shape - odd batches (the last workgroup runs
    one ciphertext twice), adversarial rows, skipped steps - and as the oracle"""
    tables, ids, tvs, msgs, sel, small, _ = pc.torus_batch(eng, count, 900 + count, CFG.bits)
    small[5] = small[4]
    small[5, ::2] = 0                      # a pair whose ciphertexts skip different steps
    with pc.pinned_variant(eng, 2):
        one = eng.blind_rotate_host(small, ids[sel])
    two = eng.blind_rotate_host(small, ids[sel])
    assert np.array_equal(one, two)
    for c in (1, 2, 3, 7):                 # pinned on small and odd batches as well
        with pc.pinned_variant(eng, 3):
            got = eng.blind_rotate_host(small[:c], ids[sel][:c])
        assert np.array_equal(got, one[:c]), c
    pick = np.array([0, 1, 2, 3, 4, 5, count - 1])
    assert np.array_equal(two[pick], ora.ctx.blind_rotate(small[pick], tvs, sel[pick]))
