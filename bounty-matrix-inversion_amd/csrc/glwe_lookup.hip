// 2^64 TORUS: the look-ups of ciphertexts that share one blind rotation (multi-value bootstrap of Carpov, Izabachene and Mollimard,
// fitted to the step-function test polynomials of bmi_lut_register).
//
// A test polynomial TV_f is a step function: M = 2^p boxes of N / M coefficients shifted by half a box, values f(0 .. M/2-1), then
// -f(-M/2 .. -1), then -f(0) on the last half box.  So (1 - X) TV_f has at most M non-zero coefficients - the differences of
// consecutive boxes, at the box boundaries; coefficient 0 is TV_f(0) + TV_f(N-1) = 0 - and, since (1 - X) sum_x X^x = 2 mod X^N + 1,
//      TV_f = TV_0 P_f,     TV_0 = 2^(u-1) sum_x X^x  (bmi_lut_register_base),     P_f = (1 - X) TV_f / 2^u,
// with small integer coefficients d_k 2^(scale_f - u), d_k the differences of the table's own integers.  ONE rotation of TV_0 gives
// ACC = (A, B); every table of the group then costs SampleExtract_0(ACC P_f): at most M rotated additions per output word, in u64
// wrap-around arithmetic.  With C_A = A P_f:   C_A[j] = sum_k P_k (+-) A[(j - c_k) mod N], minus where j < c_k (X^N = -1), and the
// extracted row is o[0] = C_A[0], o[x] = -C_A[N - x], o[N] = C_B[0].
//
// k_glwe_lookup<N>: one workgroup per group.  It stages the group's 2N accumulator words in LDS once (16 KB at N = 1024, 64 KB at
// N = 4096) and walks the group's tables; thread x computes output word x of the current table (a wavefront's 64 reads of one
// term are 64 consecutive LDS words), thread 0 also the body.  The (position, difference) pairs of a table are uniform over the
// workgroup.  A table that is its group's own base (lut id = base id: what a group of one is given, whatever the table) has
// P = 1: the plain extraction, word for word what bmi_blind_rotate_batch writes, and no noise growth.
// Nothing a device-resident id or pointer array can hold makes the kernel leave its buffers: ids are masked with the table
// capacity, entry counts clamped to BMI_SPARSE_CAP (a table without a sparse form counts as empty: a zero row), positions masked
// with N - 1, the group's range clamped to `total`, and a table below its group's unit is taken at the unit (the *_host entry
// points refuse all of these).
#include <hip/hip_runtime.h>

#include "bmi_internal.hpp"

namespace {

using bmit::BMI_SPARSE_CAP;
using bmit::i64;
using bmit::u64;

constexpr int GL_THREADS = 256;

template <int N>
__global__ void __launch_bounds__(GL_THREADS)
    k_glwe_lookup(const u64 *__restrict__ glwe, const uint32_t *__restrict__ group_ptr, const uint32_t *__restrict__ base_ids,
                  const uint32_t *__restrict__ lut_ids, const uint2 *__restrict__ sparse_head, const int2 *__restrict__ sparse,
                  u64 *__restrict__ out, uint32_t total) {
    extern __shared__ u64 acc[];   // [mask N][body N], natural order
    const uint32_t g = blockIdx.x, tid = threadIdx.x;
    const u64 *src = glwe + (size_t)g * (2 * N);
    for (uint32_t i = tid; i < 2 * N; i += GL_THREADS) acc[i] = src[i];
    __syncthreads();
    const uint32_t unit = sparse_head[base_ids[g] & (BMI_LUT_CAP - 1)].y;
    const uint32_t t0 = group_ptr[g], t1 = min(group_ptr[g + 1], total);
    for (uint32_t t = t0; t < t1; t++) {
        const uint32_t id = lut_ids[t] & (BMI_LUT_CAP - 1);
        const uint2 head = sparse_head[id];
        const bool own_base = lut_ids[t] == base_ids[g];                      // P = 1
        const uint32_t entries = own_base ? 1 : head.x <= BMI_SPARSE_CAP ? head.x : 0;
        const uint32_t shift = !own_base && head.y > unit ? min(head.y - unit, 63u) : 0;   // P_k = d_k 2^(table's scale - group's unit)
        const int2 *e = sparse + (size_t)id * BMI_SPARSE_CAP;
        u64 *o = out + (size_t)t * (N + 1);
        for (uint32_t x = tid; x < N; x += GL_THREADS) {
            const uint32_t j = (N - x) & (N - 1);   // o[0] = C_A[0], o[x] = -C_A[N - x]
            u64 s = 0;
            for (uint32_t k = 0; k < entries; k++) {
                const int2 pk = own_base ? int2{0, 1} : e[k];
                const uint32_t c = (uint32_t)pk.x & (N - 1);
                const u64 a = acc[(j - c) & (N - 1)];
                s += (u64)(i64)pk.y * (j < c ? (u64)0 - a : a);
            }
            s <<= shift;
            o[x] = x == 0 ? s : (u64)0 - s;
        }
        if (tid == 0) {   // o[N] = C_B[0]
            u64 s = 0;
            for (uint32_t k = 0; k < entries; k++) {
                const int2 pk = own_base ? int2{0, 1} : e[k];
                const uint32_t c = (uint32_t)pk.x & (N - 1);
                const u64 b = acc[N + ((N - c) & (N - 1))];
                s += (u64)(i64)pk.y * (c ? (u64)0 - b : b);
            }
            o[N] = s << shift;
        }
    }
}

}  // namespace

namespace bmit {

int launch_glwe_lookup(const u64 *glwe, const uint32_t *group_ptr, const uint32_t *base_ids, const uint32_t *lut_ids,
                       const uint2 *sparse_head, const int2 *sparse, u64 *out, uint32_t groups, uint32_t total, uint32_t N,
                       hipStream_t s) {
    if (groups == 0 || total == 0) return 0;
    auto launch = [&](auto NN) {
        constexpr int n = decltype(NN)::value;
        return launch_with_lds<k_glwe_lookup<n>>(dim3(groups), dim3(GL_THREADS), (size_t)2 * n * sizeof(u64), s, glwe, group_ptr, base_ids,
                                                 lut_ids, sparse_head, sparse, out, total);
    };
    if (N == 1024) return launch(std::integral_constant<int, 1024>{});
    if (N == 2048) return launch(std::integral_constant<int, 2048>{});
    if (N == 4096) return launch(std::integral_constant<int, 4096>{});
    return (int)hipErrorInvalidValue;
}

}  // namespace bmit
