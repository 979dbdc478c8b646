// The FieldOps table (bmi_internal.hpp) of one modulus: the keyswitch, linear-combination and phase launchers instantiated on the
// field policy F with LIMBS balanced base-256 limbs per keyswitch-key word, and the translation unit's NTT test hook (null on the
// torus).  Included by the three translation units that define a field policy.
#pragma once
#include "bmi_internal.hpp"
#include "ks_lincomb.hpp"
#include "ks_mfma.hpp"
#include "lwe_phase.hpp"

// (Not constexpr, on purpose: a table with a constant initialiser is promoted to device memory by the device pass, which then asks
// for device copies of the launchers it points to.  Filled when the library is loaded, it stays host data, while both passes still
// instantiate the launchers and through them the kernels.)
template <class F, int LIMBS>
FieldOps field_ops(decltype(FieldOps::negacyclic_mul) negacyclic_mul) {
    return {ksl::launch_keyswitch<F>,
            ksm::launch_ksk_to_limbs<F>,
            ksm::launch_keyswitch<F, LIMBS>,
            ksl::launch_lincomb<F>,
            lwp::launch_lwe_phase<F>,
            negacyclic_mul,
            LIMBS};
}
