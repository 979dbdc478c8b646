// HIP kernel (gfx950) of the UNROLLED blind rotation on the 49-bit field (bmi_set_bsk_unroll(ctx, 2)).  A translation unit
// of its own because it is compiled with the compiler's default instruction scheduler: the rest of the f64 kernels are built
// with -amdgpu-sched-strategy=max-ilp, which costs this kernel 3 % (2.28 against 2.23 ms per bootstrap, A/B in one call).
#include <hip/hip_runtime.h>

#include "bmi_internal.hpp"
#include "dec49.hpp"
#include "exact_half_steps.hpp"
#include "ntt_half_f64.hpp"
#include "ntt_wave_f64.hpp"
#include "phase_prof.hpp"

using f49::i64;
using f49::u64;
using namespace nttf;
using dec49::Dec;
using dec49::round_half_up;
using exh::L2_THREADS;

namespace {

// Phase timing (debug build only: make prof; tools/phase_prof.py with unroll = 2)
PH_ARRAY(g_phase_u)
#ifdef BMI_PHASE_PROF
__device__ unsigned long long g_wg_times_u[1024][2];   // [workgroup][start, end] in ticks of the 100 MHz real-time counter (tools/wg_times.py)
#endif

// ------------------------------------------------------------------------------------------------------------------
// LATENCY kernel with the UNROLLED bootstrap key (two LWE coefficients per step; oracle/tfhe_oracle.c
// ora_blind_rotate_extract_unrolled):   ACC <- ACC + sum_{j<3} (X^(c_j) - 1) (K3[i][j] [.] ACC),  c = (a + a', a, a').
// The structure of k_blind_rotate_lat2_49 with half the steps: phase A decomposes ACC itself (no rotation) and runs the
// twelve forward half transforms ONCE per pair of coefficients; phase B multiplies the six digit transforms with the three
// GGSW keys of the pair and scales each product by  psi^(e c_j) - 1,  the value of X^(c_j) - 1 at the slot's root psi^e
// (e = 2 kk + 1 for A_lo, e + N for A_hi: a look-up in a 2N-entry table of root powers), so the rotation never touches the
// coefficient domain; phase C is unchanged.  Per pair: 12 + 4 half transforms and 42 modular multiplications per thread,
// against 24 + 8 and 24 of two plain steps.  The price is noise: the key-noise term of the output variance triples.
constexpr int L2U_LDS_WORDS = exh::lds_words(1, true);   // the layout of k_blind_rotate_lat2_49, then the root powers
static_assert(L2U_LDS_WORDS <= BMI_LDS_WORDS_MAX, "L2U_LDS_WORDS exceeds the 160 KB of LDS");

template <int L = 3, int BG = 15>
__global__ void __launch_bounds__(L2_THREADS)
    k_blind_rotate_lat2u_49(const u64 *__restrict__ small_cts, const uint32_t *__restrict__ lut_ids,
                            const double *__restrict__ luts, const double *__restrict__ bsk3_lat,
                            const double *__restrict__ g_tw_h, const double *__restrict__ g_root_pow,
                            u64 *__restrict__ out, uint32_t count, uint32_t n) {
#ifdef BMI_PHASE_PROF
    if (threadIdx.x == 0 && blockIdx.x < 1024) g_wg_times_u[blockIdx.x][0] = wall_clock64();
#endif
    extern __shared__ double lds[];
    double *acc = lds + ntth::HT_WORDS;              // [2 components][2 parities][512], centred (<= q/2 + 2)
    double *tiles = acc + 2 * N;                     // [12][HSCRATCH]
    double *SD = tiles + 12 * ntth::HSCRATCH;        // [2 outputs][sum, difference][512]
    uint16_t *at = reinterpret_cast<uint16_t *>(SD + 2 * N);
    double *RP = SD + 2 * N + BMI_AT_WORDS;          // psi^x, x in [0, 2N)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < ntth::HT_WORDS; i += L2_THREADS) lds[i] = g_tw_h[i];
    for (int i = tid; i < 2 * N; i += L2_THREADS) RP[i ^ ((i >> 5) & 31)] = g_root_pow[i];   // folded: exh::root_pow
    const uint32_t ct = blockIdx.x;
    const u64 *lwe = small_cts + (size_t)ct * (n + 1);
    for (uint32_t i = tid; i <= n; i += L2_THREADS) at[i] = (uint16_t)f49::modswitch(lwe[i], LOG_N + 1);
    __syncthreads();
    {
        const double *tv = luts + (size_t)(lut_ids[ct] & (BMI_LUT_CAP - 1)) * N;
        const uint32_t bt = at[n];
        exh::load_test_poly49<N, 1>(acc, tv, bt, tid);
    }
    __syncthreads();
    const int mo = tid >> 9, mp = tid & 511;  // phase B: output polynomial, slot
    const uint32_t root_e = 2 * ntth::kk_of(mp & 63, mp >> 6) + 1;   // A_lo[mp] is the value at psi^root_e, A_hi[mp] at -psi^root_e
    const uint32_t pairs = (n + 1) >> 1;
    // this thread's 2 L x 2 words of GGSW key `key` (0..2) of pair `ip`: [2 L rows][2 outputs][512 slots][A_lo, A_hi], one
    // 16-byte request per row
    auto load_key = [&](double (&dst)[2 * L][2], uint32_t ip, int key) {
        exh::request_rows<1>(dst, bsk3_lat + ((size_t)ip * 3 + key) * 4 * L * N, mo, 0, mp);
    };
    double b[2 * L][2];

    PH_DECL();
    for (uint32_t ip = 0; ip < pairs; ip++) {
        const uint32_t a1 = at[2 * ip], a2 = (2 * ip + 1 < n) ? at[2 * ip + 1] : 0u;
        if ((a1 | a2) == 0) continue;  // uniform over the workgroup: every factor X^0 - 1 vanishes  (exponents written out: a helper adds a scalar instruction to the loop)
        const uint32_t cj[3] = {(a1 + a2) & (2 * N - 1), a1, a2};
        PH_MARK(7);
        load_key(b, ip, 0);
        if (wave < 4 * L) {
            const int c = wave / (2 * L), lev = (wave % (2 * L)) >> 1, h = wave & 1;
            const int pz = wave >> 1;
            const double *ac = acc + c * N + h * ntth::HALF;
            double x[8];
            __builtin_amdgcn_s_setprio(3);
            static_for<0, 8>([&](auto J) {
                x[J] = Dec<L, BG>::digit(round_half_up(ac[lane + 64 * J], Dec<L, BG>::SC), lev);
            });
            double *tile = tiles + (2 * pz + h) * ntth::HSCRATCH;
            // (written out: exh::forward_to_tile renumbers this kernel's registers, and at one bootstrap that build fell outside the
            // timing margin by less than a microsecond, twice: profiles/exact_steps_ab.txt)
            if (h) ntth::forward_half<true>(x, lane, lds, tile);
            else ntth::forward_half<false>(x, lane, lds, tile);
            wave_sync();
            static_for<0, 8>([&](auto R) { tile[R * 64 + lane] = x[R]; });
            __builtin_amdgcn_s_setprio(0);
        }
        PH_MARK(0);
        __syncthreads();
        PH_MARK(1);
        {
            double alo[2 * L], ahi[2 * L];   // (written out: behind a helper the multiply phase is scheduled in another order)
#pragma unroll
            for (int r = 0; r < 2 * L; r++) {
                const double e = tiles[(2 * r) * ntth::HSCRATCH + mp], od = tiles[(2 * r + 1) * ntth::HSCRATCH + mp];
                alo[r] = e + od;
                ahi[r] = e - od;
            }
            double slo = 0.0, shi = 0.0;   // sums of three reduced products (<= 1.6 q)
            auto one_key = [&](const double (&kw)[2 * L][2], uint32_t c) {
                double ylo = 0.0, yhi = 0.0;  // lazy sums of 2 L <= six reduced products (<= 3.1 q)
                exh::mac_rows(ylo, yhi, alo, ahi, kw);
                const double w = exh::root_pow(RP, root_e, c);   // psi^(e c); at the root -psi^e: (-1)^c times it
                const double wh = (c & 1) ? -w : w;
                slo += f49::mul(ylo, w - 1.0);   // the lazy sum goes into the product as it is (|.| <= 3.1 q: exact, like e + od above)
                shi += f49::mul(yhi, wh - 1.0);
            };
            // key 0 was requested before the forward phase; key 1 is requested now, key 2 as soon as key 0 has been consumed.
            // (Requesting more ahead was built and measured: the next pair's first key under the inverse phase or key 1 under
            // the forward phase need registers the forward tasks do not have - 76-80 bytes of spills per lane, 25 % slower;
            // key 1 right before the barrier, or keys 1 and 2 together: no gain / 5 % slower; a second copy of the step loop for
            // the four wavefronts without a forward task, which then hold all three keys from the start of a step - 124
            // registers, no spills, bit-exact: 1 % faster, not kept; those wavefronts touching every line of keys 1 and 2
            // under the forward phase so that the real requests hit the L2: 3 % SLOWER.)
            double bn[2 * L][2];
            load_key(bn, ip, 1);
            one_key(b, cj[0]);
            load_key(b, ip, 2);
            one_key(bn, cj[1]);
            one_key(b, cj[2]);
            slo = f49::red(slo);
            shi = f49::red(shi);
            exh::sum_diff_store(SD, mo, mp, slo, shi);
        }
        PH_MARK(2);
        __syncthreads();
        PH_MARK(3);
        if (wave < 4) {
            const int o = wave >> 1, h = wave & 1;
            double x[8];   // (read + inverse half written out: a helper reorders the task)
            static_for<0, 8>([&](auto R) { x[R] = SD[(o * 2 + h) * ntth::HALF + R * 64 + lane]; });
            double *tile = tiles + wave * ntth::HSCRATCH;
            if (h) ntth::inverse_half<true>(x, lane, lds, tile);
            else ntth::inverse_half<false>(x, lane, lds, tile);
            double *ao = acc + o * N + h * ntth::HALF;
            static_for<0, 8>([&](auto J) { ao[lane + 64 * J] = f49::red(ao[lane + 64 * J] + x[J]); });
        }
        PH_MARK(4);
        __syncthreads();
        PH_MARK(5);
    }
    PH_STORE(g_phase_u, wave, lane);
#ifdef BMI_PHASE_PROF
    if (threadIdx.x == 0 && blockIdx.x < 1024) g_wg_times_u[blockIdx.x][1] = wall_clock64();
#endif
    exh::extract_sample49<N, 1>(out + (size_t)ct * (N + 1), acc, tid);
}

}  // namespace

PH_EXPORT(bmi_debug_phase_prof_unrolled, g_phase_u)
#ifdef BMI_PHASE_PROF
extern "C" int bmi_debug_wg_times_unrolled(unsigned long long *out2048) {
    return (int)hipMemcpyFromSymbol(out2048, HIP_SYMBOL(g_wg_times_u), sizeof(unsigned long long) * 2048);
}
#endif

namespace bmi49 {

int launch_blind_rotate_lat2u(const RotBatch &b) {
    if (b.count == 0) return 0;
    return with_shape49(b.levels, b.base_log, [&](auto L, auto BG) {
        return launch_with_lds<k_blind_rotate_lat2u_49<L, BG>>(dim3(b.count), dim3(L2_THREADS), (size_t)L2U_LDS_WORDS * sizeof(double), b.s, b.cts,
                                                                b.ids, b.luts.d(), b.key.d(), b.tab[0].d(), b.tab[1].d(), b.out, b.count, b.n);
    });
}

}  // namespace bmi49
