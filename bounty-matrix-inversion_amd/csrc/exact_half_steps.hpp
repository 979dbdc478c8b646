// The steps the exact-transform latency blind rotations state the same way (gfx950): k_blind_rotate_lat2_49 (bmi_kernels_f64.hip),
// k_blind_rotate_lat2u_49 (bmi_kernels_f64u.hip), k_blind_rotate_lat_t64 (bmi_kernels_t64.hip), k_blind_rotate_lat2u_t64
// (bmi_kernels_t64u.hip) - one workgroup of 16 wavefronts per ciphertext, every transform split over two wavefronts by parity
// (ntt_half_f64.hpp) - their key conversions k_bsk_to_lat49 / k_bsk_to_lat_t64, and the start accumulator of every 49-bit kernel
// that keeps its accumulator de-interleaved (N = 2048 and 4096 included).  Built like t64_half_steps.hpp, by
// the same rules: force-inlined functions on the caller's compile-time constants, no state, no barrier, pin(), s_setprio or phase
// mark (where a step stands relative to those distinguishes the kernels and stays in their step loops); LDS words come in as values
// or as the caller's pointers.  A step is here if at least two kernels call it with their machine code unchanged or renumbered
// only (tools/isa_diff.py: "identical" / "registers only"; the record is profiles/exact_steps_ab.txt); a kernel whose instruction
// order a helper changes keeps the step written out and says so in one line.  Written out in every kernel, for that reason: the
// E +- O' pairs of the digit transforms, the pair exponents (a + a', a, a'), the read of the sums with the inverse half, and the
// (A_lo, A_hi) store of the key conversions.
#pragma once
#include <hip/hip_runtime.h>

#include "bmi_internal.hpp"
#include "ntt_half_f64.hpp"
#include "t64_common.hpp"

namespace exh {

using f49::u64;
using nttf::N;
using nttf::static_for;

// ---- the family's constants and LDS map ----
constexpr int L2_THREADS = 1024;   // 16 wavefronts
// twiddles, accumulator [2 components][2 parities][512], twelve tiles (4 x (L = 3)), sums / differences [limb][2 outputs][S, D][512],
// mod-switched ciphertext, and with the unrolled key the 2N root powers
constexpr int lds_words(int limbs, bool root_powers) {
    return ntth::HT_WORDS + 2 * N + 12 * ntth::HSCRATCH + limbs * 2 * N + BMI_AT_WORDS + (root_powers ? 2 * N : 0);
}

// ---- the 49-bit accumulator, de-interleaved mod 2^LOG_R: acc[component][nn mod 2^LOG_R][PN >> LOG_R] ----
// coefficient nn of the start accumulator (0, X^bt tv): the mask zero, the body the test polynomial rotated by the body's exponent
template <int PN, int LOG_R>
__device__ __forceinline__ void load_test_poly49(double *acc, const double *tv, uint32_t bt, uint32_t nn) {
    constexpr t64::ResidueSlot<PN, LOG_R> slot{};
    const uint32_t e = (nn + bt) & (2 * PN - 1);
    const double v = tv[e & (PN - 1)];
    acc[slot(nn)] = 0.0;
    acc[PN + slot(nn)] = (e & PN) ? -v : v;
}
// sample extraction at coefficient 0: word nn of the mask (negated and reversed) and, from thread 0, the body
template <int PN, int LOG_R>
__device__ __forceinline__ void extract_sample49(u64 *o, const double *acc, uint32_t nn) {
    constexpr t64::ResidueSlot<PN, LOG_R> slot{};
    const double a0 = acc[slot(nn)];
    if (nn == 0) {
        o[0] = f49::to_u(a0);
        o[PN] = f49::to_u(acc[PN]);
    } else {
        o[PN - nn] = f49::to_u(-a0);
    }
}

// ---- phase A ----
// the forward tail: half transform of the wavefront's parity h, then the finished half into its tile
__device__ __forceinline__ void forward_to_tile(double (&x)[8], int h, int lane, const double *lds, double *tile) {
    if (h) ntth::forward_half<true>(x, lane, lds, tile);
    else ntth::forward_half<false>(x, lane, lds, tile);
    nttf::wave_sync();
    static_for<0, 8>([&](auto R) { tile[R * 64 + lane] = x[R]; });
}

// ---- phase B: thread = (output polynomial mo, slot mp) ----
// this thread's 2 x R2 key words of limb j of one GGSW key at bj: [R2 rows][2 outputs][limb][512 slots][A_lo, A_hi], one 16-byte
// request per row
template <int LIMBS, int R2>
__device__ __forceinline__ void request_rows(double (&dst)[R2][2], const double *bj, int mo, int j, int mp) {
#pragma unroll
    for (int r = 0; r < R2; r++) {
        const double2 w = reinterpret_cast<const double2 *>(bj + ((size_t)(r * 2 + mo) * LIMBS + j) * N)[mp];
        dst[r][0] = w.x;
        dst[r][1] = w.y;
    }
}
// lazy multiply-accumulate over the R2 <= six rows: the sums are not reduced (the caller states its bound; exact in f64 below 2^53)
template <int R2>
__device__ __forceinline__ void mac_rows(double &ylo, double &yhi, const double (&alo)[R2], const double (&ahi)[R2], const double (&kw)[R2][2]) {
#pragma unroll
    for (int r = 0; r < R2; r++) {
        ylo += f49::mul(alo[r], kw[r][0]);
        yhi += f49::mul(ahi[r], kw[r][1]);
    }
}
// what the inverse halves start from: sum and difference of the (reduced) lo / hi results, into sd = [2 outputs][S, D][512]
__device__ __forceinline__ void sum_diff_store(double *sd, int mo, int mp, double lo, double hi) {
    sd[(mo * 2 + 0) * ntth::HALF + mp] = lo + hi;
    sd[(mo * 2 + 1) * ntth::HALF + mp] = lo - hi;
}

// ---- the unrolled key: X^c - 1 in the transform domain ----
// The table psi^x, x in [0, 2N), is stored at x ^ (bits 5..9 of x): the exponents of a wavefront, odd multiples of c, share their
// low bits when c is even - without the fold they would meet in a few LDS banks (SQ_LDS_BANK_CONFLICT: 30 % of the LDS cycles of
// k_blind_rotate_lat2u_49, rocprofv3 --pmc); each kernel stages it with its own loop.
// psi^(root_e c): the value of X^c at the slot's root psi^root_e; at the root -psi^root_e it is (-1)^c times that
__device__ __forceinline__ double root_pow(const double *RP, uint32_t root_e, uint32_t c) {
    const uint32_t xe = (root_e * c) & (2 * N - 1);
    return RP[xe ^ ((xe >> 5) & 31)];
}

// ---- phase C on the torus ----
// a limb's exact integers (|.| < p/2: the centred residue IS the integer) shifted into place; the limbs of a coefficient meet in a
// slot and add atomically
__device__ __forceinline__ void place_limb(u64 *ao, const double (&x)[8], int lane, int sh) {
    unsigned long long *a = reinterpret_cast<unsigned long long *>(ao);
    static_for<0, 8>([&](auto J) { atomicAdd(a + lane + 64 * J, (unsigned long long)(t64::f64_to_word(f49::red(x[J])) << sh)); });
}

}  // namespace exh
