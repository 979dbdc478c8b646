// 2^64 TORUS, throughput blind rotation with the exact products carried by a floating-point transform (gfx950).
//
// Same function as k_blind_rotate_t64<48, L, 10> (bmi_kernels_t64.hip) - bootstrap key stored at 48 bits of precision as two
// balanced 24-bit limbs, digits in base 2^10, accumulator as the exact integer word / 2^16 in a double - and the same results
// bit for bit: per limb the sum over the 2 L digit x limb polynomial products is an integer below 2^45, and it is computed here
// through the folded 512-point complex FFT of fft_wave_f64.hpp and ROUNDED TO THE NEAREST INTEGER, which returns that
// integer exactly (the transform's error on these operands stays below 2^-11, see the header; tests/test_gpu_parity.py and
// tests/test_gpu_torus_fft.py hold the kernel to the oracle's integer arithmetic).  What changes is the cost: a transform of
// 1,024 real coefficients is ~300 f64 instructions per lane instead of ~700 for the exact one mod 2^49 - 720895, and a
// multiply-accumulate is 4 fused multiply-adds per complex point (2 coefficients) instead of 6 instructions per coefficient.
//
// Structure = k_blind_rotate_t64: a pair of wavefronts per ciphertext, four ciphertexts per workgroup; wavefront c owns input
// polynomial c (decomposes it, transforms its L digit polynomials once, multiplies them with both key columns of both limbs),
// publishes the partner's partial sums through its LDS tile, adds the partner's, and runs the inverse transforms of output c.
// Order of a CMUX (EXPERIMENTS A31, profiles/limb_order_ab.txt): ALL 4 L product rows first - column, then limb, then level:
// (limb 0, partner's column) -> tile, (limb 0, own column), (limb 1, partner's column) -> tile, (limb 1, own column) - then both
// inverse transforms, then ONE recombination.  After the last row the digit transforms X (96 registers) are dead: limb 0's rounded
// result waits in registers across the second inverse transform instead of going through the accumulator in LDS, and both inverse
// transforms use one set of table twiddles.  The key stream has no gap: every row but the CMUX's first is requested one row ahead.
//
// Roles of the eight wavefronts of a workgroup: ciphertext slot ctl = wave >> 1, polynomial c = wave & 1, partner = wave ^ 1.
// Wavefronts w and w + 4 share a SIMD, so the two wavefronts of a ciphertext sit on different SIMDs and each SIMD holds one
// wavefront of slots 0-1 (group A, the older: it wins issue and leads by a forward phase, below) and one of slots 2-3 (group B).  The four
// wavefronts with the same c (0, 2, 4, 6 or 1, 3, 5, 7) read the same key rows (bsk_c depends on c only) and share them through
// L1 - in part.  With all eight wavefronts in phase (before the offset below) the trailing wavefronts asked for a row two to
// five rows after the leaders and a workgroup fetched 2.1 x one copy of the key from L2 per CMUX (4,207 M 128-byte read requests
// per launch of 8,192 against 1,982 M).  With the offset a row's four readers are two of each group, a forward phase apart by
// design, and it is 2.4 x (4,778 M, same call) - in the faster kernel; with all product rows in front of the inverse transforms
// it is 2.8 x (5,546 M against 4,779 M in one call, EXPERIMENTS A31) - again in the faster kernel.  That traffic is not what holds the kernel: making the two wavefronts of a ciphertext SIMD-mates (ctl = wave % 4, c = wave / 4), which keeps the
// four readers of a row together, brought it down to 1.3 x and was 1.2 - 1.7 ms per 8,192 SLOWER; a workgroup barrier at each limb's
// first row was 8 ms slower (profiles/key_row_sharing_ab.txt, EXPERIMENTS A19).  These roles stay.
// What a CMUX keeps in registers instead of re-reading from LDS: the forward transforms' table twiddles (ForwardTwiddles: loaded
// once, used by the L transforms), the inverse transforms' (InverseTwiddles: loaded after the last hand-off, used by both), limb 0's
// rounded result (x0) and the lane's own 16 accumulator words across the back edge (`keep`).
//
// Who may touch a tile when (pair_sync.hpp; a CMUX has two hand-offs, h0 = 2 i + 1 for limb 0 and h1 = 2 i + 2 for limb 1, strictly
// increasing; pub[w] / ack[w] are written by wavefront w only).  Tile T_w of wavefront w is WRITTEN by w alone - the exchanges of its
// forward transforms, the two partials it publishes, the exchanges of its inverse transforms - and READ by the partner w' = w ^ 1 only
// between w' seeing pub[w] = h and w' storing ack[w'] = h.  One CMUX of w, in program order:
//   L rows (limb 0, column c^1); stores partial h0 into T_w; pub[w] = h0 (release: the stores are visible before the flag)
//   L rows (limb 0, column c); sees pub[w'] = h0; reads T_w' (8 reads per lane) and adds; waits until they have returned; ack[w] = h0
//   L rows (limb 1, column c^1); sees ack[w'] = h0 (w' has read partial h0); stores partial h1 into T_w; pub[w] = h1
//   L rows (limb 1, column c); sees pub[w'] = h1; reads T_w' and adds; ack[w] = h1
//   first two butterfly stages of the first DFT8 of the first inverse transform (registers only); sees ack[w'] = h1; only then the
//   first store of that transform into T_w; the second inverse transform; the recombination
// Every wait but the last looks at a flag the partner stored L rows before it reached the same point of ITS program; the last one
// sits under the first DFT8.  Where the stores of an exchange sit: the forward transforms and the partials issue their eight
// ds_write_b128 back to back after the arithmetic; the two exchanges of an inverse transform issue them from inside the last
// butterfly stage of the DFT8 in front (fftw::dft8_emit: two stores, then the next pair's four f64 instructions), so the VGPR-to-LDS
// transfer of a pair runs under arithmetic of the same wavefront (profiles/exchange_bubbles_ab.txt, EXPERIMENTS A20).  The protocol
// does not see the difference: the wait for ack[w'] = h1 and the wavefront fence still precede the first store in program order,
// every store of an exchange still precedes the fence in front of its reads, and an earlier read of T_w by w itself has been
// consumed by the arithmetic the stores depend on.
// No write of T_w can overtake a read of it by w': partial h1 is stored after ack[w'] = h0 is seen; the first inverse transform's
// stores after ack[w'] = h1; everything later - the second inverse transform, the next CMUX's forward transforms and its partial
// h0 + 2 - follows that store in w's program order, and w' reads T_w again only after pub[w] = h0 + 2.  Reads by w' never see a stale
// partial: it reads only after pub[w] = h, which w stores after the partial.  The flags need no reset: each is compared for equality
// with a value its only writer stores exactly once - which is also why pub[w] = h1 must follow ack[w'] = h0: a partner that had not
// yet looked for pub[w] = h0 would never see it.
// No deadlock: the waits of w, in order, are for pub[w'] = h0, ack[w'] = h0, pub[w'] = h1, ack[w'] = h1.  w' stores pub[w'] = h0
// before any of its waits of this CMUX (its last wait before is for ack[w] = h0 - 1, stored by w before w began this CMUX); it stores
// ack[w'] = h0 after waiting for pub[w] = h0 only, which w stored before its first wait; pub[w'] = h1 after waiting for ack[w] = h0,
// which w stored before waiting for ack[w'] = h0; ack[w'] = h1 after waiting for pub[w] = h1, which w stored before waiting for
// pub[w'] = h1.  Each store a wait depends on precedes, in its writer's program, every wait of the writer that could depend on the
// waiting wavefront's later stores: the waits cannot form a cycle (tests/test_pair_handoff_order_model.py explores every interleaving
// of three CMUXes).  Dead pairs (beyond `count`) run the whole protocol on a copy of the last ciphertext.  The per-CMUX workgroup
// barrier is reached by every wavefront outside any hand-off, at either site.
// Registers: with X, two limb sums and two key rows live (224 of 256) the product phase has no room for the loop's invariant
// addresses, and hoisted they were spilled (212 B of scratch, 41 reloads per CMUX).  So the wavefront's number is a scalar, and the
// lane and wavefront numbers are taken from opaque per-CMUX copies (lane_a, lane_i, wave_i): the addresses are recomputed, about 80
// 32-bit vector and 40 scalar instructions per CMUX, and <3, 10> compiles to no scratch at all (the order before: 12 B).
//
// Who is in which phase when (EXPERIMENTS A22, profiles/phase_offset_ab.txt).  Wavefronts 0 .. CTS-1 are group A, CTS .. 2 CTS-1
// group B; each SIMD holds one wavefront of each group and both wavefronts of a pair are in the same group, so the pair protocol
// never crosses groups (CTS is even; at CTS = 2 a SIMD holds one wavefront and the offset has no mate to serve).  Every wavefront executes ONE hardware barrier per CMUX (n in all, after the one of the prologue), at one
// of two sites under a scalar branch (pair_sync.hpp: barrier_if): group B at the loop head, group A between its last forward
// transform and its first product row.  The hardware counts arrivals: barrier i releases when B stands at the head of step i and A
// has finished the forward transforms of step i.  From then on A leads its SIMD-mate by one forward phase - A multiplies key rows
// (the compute unit's intake is the limit there, the f64 pipe idles) while B transforms (f64 and LDS stores, one prefetched row
// on the memory path) - and eight wavefronts never enter the intake-bound product phase in step.  The lead cannot grow: A waits
// at its site of step i + 1 until B has reached the head of step i + 1.  The barrier only paces: no wavefront reads another's
// LDS words across it (tiles are guarded by the pair flags; at[] and the tables are read-only after the prologue), so it is bare
// - no fence, no wait for outstanding loads - and a step count of 1, dead pairs and both level counts need no special case.
// (One barrier per CMUX for all eight at the loop head, the form before: 1.3 ms per 8,192 slower; none at all: 83.2 ms against 68.9.)
// Issue priority follows from mates being in different phases: 0 through the forward transforms, 1 from the first product row to
// the end of the CMUX.  A product row is a few instructions whose loads should leave at once, the hand-offs and inverse transforms
// are what the partner waits on, and the mate's transforms fill the rest.  With the in-phase ladder (3, 2, 1 / 0) the transforming
// wavefront starves its mate's loads and the offset LOSES 1.5 - 4.4 ms; with no priorities it loses 3; the new priorities
// without the offset lose 5.
#include <hip/hip_runtime.h>

#include "bmi_internal.hpp"
#include "fft_half_f64.hpp"
#include "fft_wave_f64.hpp"
#include "pair_sync.hpp"
#include "phase_prof.hpp"
#include "t64_common.hpp"
#include "t64_half_steps.hpp"

using t64::i64;
using t64::u64;
using namespace fftw;

namespace {

PH_ARRAY(g_phase_f)   // make -C csrc prof; tools/phase_prof_t64f.py
using t64::f64_to_word;
using t64::mod_ab;
using t64::Scheme;
#ifndef BMI_T64F_CTS
#define BMI_T64F_CTS 4      // ciphertexts (wavefront pairs) per workgroup, even: 4 fill the CU's LDS; 3 (before the barrier groups) and 2 measured slower per ciphertext
#endif
constexpr int TF_CTS = BMI_T64F_CTS;
constexpr int TF_LDS_WORDS = TW_WORDS + 2 * TF_CTS * (SCRATCH_WORDS + N) + TF_CTS * BMI_AT_WORDS + 4 * TF_CTS;
static_assert(TF_LDS_WORDS <= BMI_LDS_WORDS_MAX, "TF_LDS_WORDS exceeds the 160 KB of LDS");
static_assert(SCRATCH_WORDS >= N, "a tile carries 512 complex partial sums to the partner");
// the two barrier groups are wavefronts 0 .. CTS-1 and CTS .. 2 CTS-1: with an odd CTS the pair (CTS-1, CTS) would straddle them
static_assert(TF_CTS % 2 == 0, "both wavefronts of a pair must be in the same barrier group");

// standard-domain GGSW polynomials (u64 torus words, already rounded to the key precision) -> per polynomial the two limb
// polynomials in the evaluation layout of fft_wave_f64.hpp ([poly][limb][register c][lane] complex words)
__global__ void __launch_bounds__(256) k_bsk_to_fft_t64(const u64 *__restrict__ std_polys, double *__restrict__ limb_polys,
                                                        const double *__restrict__ g_tw, uint32_t n_polys, int prec) {
    const int limbs = t64::limbs_of(prec);
    __shared__ double lds[TW_WORDS + 4 * SCRATCH_WORDS];
    for (int i = threadIdx.x; i < TW_WORDS; i += blockDim.x) lds[i] = g_tw[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t item = blockIdx.x * 4 + wave;            // (polynomial, limb)
    if (item >= n_polys * (uint32_t)limbs) return;
    const uint32_t poly = item / limbs;
    const int j = (int)(item % limbs);
    double *scratch = lds + TW_WORDS + wave * SCRATCH_WORDS;
    double x[16];
    static_for<0, 16>([&](auto J) { x[J] = (double)t64::limb_of((i64)std_polys[(size_t)poly * N + lane + 64 * J], j, prec); });
    forward(x, lane, lds, scratch);
    double2 *dst = reinterpret_cast<double2 *>(limb_polys + (size_t)item * N);
    static_for<0, 8>([&](auto Cc) { dst[Cc * 64 + lane] = double2{x[Cc], x[Cc + 8]}; });
}

// STATS (the test hook bmi_fft_margin_host): also records the largest distance of a limb sum from the integer it is rounded to
// GLWE: the kernel returns the accumulator itself, out = [count][2N], instead of the extracted sample, out = [count][N + 1]
template <int L, int BG, bool STATS, bool GLWE>
__global__ void __launch_bounds__(128 * TF_CTS)
    k_blind_rotate_t64f(const u64 *__restrict__ small_cts, const uint32_t *__restrict__ lut_ids, const u64 *__restrict__ luts,
                        const double *__restrict__ bsk, const double *__restrict__ g_tw, u64 *__restrict__ out,
                        uint32_t count, uint32_t n, unsigned long long *__restrict__ stat) {
    constexpr int CTS = TF_CTS;
    constexpr int LIMBS = Scheme<48>::LIMBS, LB = Scheme<48>::BITS, PRE = Scheme<48>::PRE, AB = 64 - PRE;
    // a limb's sum: 2 L N terms of |digit| <= 2^(BG-1) times |limb| <= 2^(LB-1) - the transform's error bound is stated for this size
    static_assert(2.0 * L * N * (double)(1ull << (BG - 1)) * (double)(1ull << (LB - 1)) <= 0x1p45, "limb sums must stay below 2^45");
    static_assert(LIMBS == 2 && L * BG < AB, "two limbs; the decomposed bits lie inside the key precision");
    extern __shared__ double lds[];
    double *tiles = lds + TW_WORDS;
    double *accs = tiles + 2 * CTS * SCRATCH_WORDS;          // accumulators: exact integers word / 2^PRE, centred mod 2^AB
    double *at_base = accs + 2 * CTS * N;
    uint32_t *flags = reinterpret_cast<uint32_t *>(at_base + CTS * BMI_AT_WORDS);  // [2 CTS] published, [2 CTS] consumed
    // the wavefront's number as a scalar: its roles, tiles, flags and key rows are then addressed from scalar registers (as vector
    // values they were loop invariants that the product phase - 224 registers of operands - had no room for)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ctl = wave >> 1, c = wave & 1;
    if (threadIdx.x < 4 * CTS) flags[threadIdx.x] = 0;
    for (int i = threadIdx.x; i < TW_WORDS; i += blockDim.x) lds[i] = g_tw[i];
    const uint32_t ct_raw = blockIdx.x * CTS + ctl;
    const bool live = ct_raw < count;
    const uint32_t ct = live ? ct_raw : count - 1;
    double *accf = accs + wave * N;
    uint16_t *at = reinterpret_cast<uint16_t *>(at_base + ctl * BMI_AT_WORDS);
    const u64 *lwe = small_cts + (size_t)ct * (n + 1);
    t64::stage_lwe<LOG_N + 1>(at, lwe, n, lane + 64 * c, 128);   // by the pair of wavefronts
    __syncthreads();
    {
        const u64 *tv = luts + (size_t)(lut_ids[ct] & (BMI_LUT_CAP - 1)) * N;
        const uint32_t bt = at[n];
        static_for<0, 16>([&](auto J) {
            const uint32_t e = (lane + 64 * J + bt) & (2 * N - 1);
            const u64 v = tv[e & (N - 1)];
            const u64 w0 = c ? ((e & N) ? (u64)0 - v : v) : (u64)0;
            t64::set_acc<PRE>(accf[lane + 64 * J], w0);
        });
    }

    uint32_t hand = 0;   // hand-off counter of the pair (two per CMUX: one per limb)
    double dev = 0.0;    // STATS: largest |value - nearest integer| this lane has rounded away
    PH_DECL();
    // this lane's own 16 accumulator words, carried across the back edge: the recombination below stores them and the next CMUX
    // would read the same words back (the rotated read still goes through LDS: those words are other lanes')
    double keep[16];
    static_for<0, 16>([&](auto J) { keep[J] = accf[lane + 64 * J]; });
    for (uint32_t i = 0; i < n; i++) {
        // the wavefront's group, its tile, its partner's and the four flags come from an opaque per-CMUX copy of the wavefront's number:
        // a few scalar instructions per CMUX instead of loop invariants in vector registers (the flag addresses and the barrier's
        // condition are vector operands: hoisted, they were spilled and reloaded inside the loop)
        int wave_i = wave;
        asm volatile("" : "+s"(wave_i));
        PH_MARK(7);
        barrier_if(wave_i >= CTS);   // barrier i of group B (the group flag is recomputed at each site, not carried)
        PH_MARK(0);   // resync barrier
        const uint32_t a_t = at[i];
        double *tile = tiles + wave_i * SCRATCH_WORDS;
        const double *ptile = tiles + (wave_i ^ 1) * SCRATCH_WORDS;
        uint32_t *f_pub = flags + wave_i, *f_pub_partner = flags + (wave_i ^ 1);
        uint32_t *f_ack = flags + 2 * CTS + wave_i, *f_ack_partner = flags + 2 * CTS + (wave_i ^ 1);
        int lane_a = lane;   // (opaque per-CMUX copy for the phases in front of the product rows: see lane_i below)
        asm volatile("" : "+v"(lane_a));
        // this wavefront's L GGSW rows: [row = L c + lev][column][limb][N]
        const double *bsk_c = bsk + ((size_t)i * 4 * L + c * 2 * L) * LIMBS * N;
        __builtin_amdgcn_s_setprio(0);   // issue priority: 0 through the forward transforms, 1 in the limb loop (header: SIMD-mates are in different phases)
        wave_sync();
        double r[16];
        {
            double vr[16], vs[16];  // all 16 reads in flight before the first use
            static_for<0, 16>([&](auto J) {
                vr[J] = accf[((lane_a + 2 * N - a_t) + 64 * J) & (N - 1)];   // (= lane + 64 J + 2 N - a_t)
                vs[J] = keep[J];
            });
            sched_fence();
            static_for<0, 16>([&](auto J) {
                const uint32_t e = ((lane_a + 2 * N - a_t) + 64 * J) & (2 * N - 1);
                const double d = mod_ab<AB>(((e & N) ? -vr[J] : vr[J]) - vs[J]);            // the centred lift of the u64 difference, / 2^PRE
                r[J] = t64::rounded_top_f64<L, BG, AB>(d);
            });
        }
        PH_MARK(1);   // accumulator reads, difference, rounding
        double X[L][16];   // the L digit polynomials, evaluation layout, live across the limb loop
        // key rows in the order they are multiplied: t = seg * L + lev, seg = 0 .. 3 = (limb 0, partner's column c^1), (limb 0, own
        // column c), (limb 1, c^1), (limb 1, c) - every product row of the CMUX before either inverse transform.  A partner's-column
        // sum is published while the own column of the same limb is still being multiplied.  A row is 8 complex words per lane; the
        // NEXT row is requested before the current one is multiplied (two register sets), across the column and limb boundaries too,
        // the first one before the last forward transform: a row's 32 multiply-adds are far shorter than the latency of its loads.
        auto row_ptr = [&](int t) {
            const int seg = t / L, lev = t % L, j = seg >> 1, col = (seg & 1) ? c : (c ^ 1);
            return reinterpret_cast<const double2 *>(bsk_c + ((size_t)(lev * 2 + col) * LIMBS + j) * N);
        };
        double2 kb[2][8];
        auto fetch = [&](double2 (&dst)[8], int t) { static_for<0, 8>([&](auto P) { dst[P] = row_ptr(t)[P * 64 + lane]; }); };
        // the forward transforms' 15 table twiddles per lane, read from LDS once per CMUX instead of once per transform (the
        // wavefront fences inside a transform keep the compiler from doing this itself): 30 ds_read_b128 fewer per CMUX
        ForwardTwiddles ftw;
        load_forward_twiddles(ftw, lane_a, lds);
        sched_fence();
        static_for<0, L>([&](auto LEV) {
            constexpr int lev = L - 1 - LEV;  // least significant digit first
            pin();
            static_for<0, 16>([&](auto J) {
                if constexpr (lev == 0) {
                    X[0][J] = r[J];
                } else {
                    const double rn = __builtin_floor(__builtin_fma(r[J], 1.0 / (double)(1ull << BG), 0.5));
                    X[lev][J] = __builtin_fma(-(double)(1ull << BG), rn, r[J]);          // digit in [-2^(BG-1), 2^(BG-1))
                    r[J] = rn;
                }
            });
            if constexpr (lev == 0) {
                fetch(kb[0], 0);
                pin();
            }
            forward(X[lev], lane_a, ftw, tile);
        });
        __builtin_amdgcn_s_setprio(1);
        PH_MARK(2);   // digits + L forward transforms
        barrier_if(wave_i < CTS);   // barrier i of group A
        PH_MARK(0);
        const uint32_t h0 = hand + 1, h1 = hand + 2;   // the CMUX's two hand-offs: limb 0's partial sums, limb 1's
        hand = h1;
        double acc[16], acc0[16];   // acc: segments 0, 2, 3 in turn (limb 1's sum at the end); acc0: segment 1, limb 0's sum
        // publishes the partner's-column sum of a limb through this wavefront's tile (free since the last transform, or since the
        // partner acknowledged the partial before)
        auto publish = [&](uint32_t h) {
            wave_sync();
            static_for<0, 8>([&](auto P) {
                reinterpret_cast<double2 *>(tile)[P * 64 + lane] = double2{acc[P], acc[P + 8]};
            });
            pair_post(f_pub, h);
        };
        // adds the partner's partial h to the own column's sum and acknowledges it: the partner posted it L rows ago
        auto take = [&](double (&a)[16], uint32_t h) {
            PH_MARK(3);   // 4L rows of products (+ publishing the partner's partials)
            pair_wait(f_pub_partner, h);
            PH_MARK(4);   // waiting for the partner's partials (and for its acknowledgement of limb 0's)
            static_for<0, 8>([&](auto P) {
                const double2 p = reinterpret_cast<const double2 *>(ptile)[P * 64 + lane];
                a[P] += p.x;
                a[P + 8] += p.y;
            });
            pin();
            pair_ack(f_ack, h);           // the eight reads above have landed: the partner may overwrite its tile
            pin();
            PH_MARK(5);   // adding the partner's partials, posting the acknowledgements
        };
        // The lane number as the inverse transforms and the recombination see it: an opaque copy made per CMUX.  The LDS addresses
        // derived from it (rotated exchange slots, the 16 accumulator words) are then computed after the last product row instead
        // of being hoisted out of the loop, where with X, two sums and two key rows live (224 registers) they were spilled: 212 B
        // of scratch and 41 reloads per CMUX at three levels without these copies (lane_a, lane_i, wave_i), none with them.
        int lane_i = lane;
        asm volatile("" : "+v"(lane_i));
        InverseTwiddles itw;
        static_for<0, 4 * L>([&](auto T) {
            constexpr int t = T, seg = t / L, lev = t % L, cur = t & 1;
            if constexpr (t + 1 < 4 * L) fetch(kb[cur ^ 1], t + 1);
            sched_fence();
            double (&a)[16] = seg == 1 ? acc0 : acc;
            static_for<0, 8>([&](auto P) {
                const double xr = X[lev][P], xi = X[lev][P + 8];
                if constexpr (lev == 0) {
                    a[P] = __builtin_fma(xr, kb[cur][P].x, -(xi * kb[cur][P].y));
                    a[P + 8] = __builtin_fma(xr, kb[cur][P].y, xi * kb[cur][P].x);
                } else {
                    a[P] = __builtin_fma(xr, kb[cur][P].x, __builtin_fma(-xi, kb[cur][P].y, a[P]));
                    a[P + 8] = __builtin_fma(xr, kb[cur][P].y, __builtin_fma(xi, kb[cur][P].x, a[P + 8]));
                }
            });
            if constexpr (lev == L - 1 && seg == 0) publish(h0);
            if constexpr (lev == L - 1 && seg == 2) {
                // limb 1's partial overwrites limb 0's: the partner has read that one once its acknowledgement - posted when it
                // finished ITS segment 1, L rows ago - is seen
                pin();
                PH_MARK(3);
                pair_wait(f_ack_partner, h0);
                PH_MARK(4);
                pin();
                publish(h1);
            }
            pin();
            if constexpr (lev == L - 1 && seg == 1) take(acc0, h0);
            if constexpr (lev == L - 1 && seg == 3) {
                take(acc, h1);
                // X is dead from here: the inverse transforms' 15 table twiddles per lane are read from LDS once for both transforms
                // (requested after the hand-off; requested in front of its wait the kernel measured 3.7 ms per 8,192 SLOWER)
                load_inverse_twiddles(itw, lane_i, lds);
                pin();
            }
        });
        // the partner has read this tile (limb 1's partial) once its acknowledgement is seen: the first inverse transform waits for
        // it just before its first store to the tile, between the second and the last butterfly stage of its first DFT8 (registers only)
        auto ack_hook = [&]() {
            pin();
            pair_wait(f_ack_partner, h1);
            pin();
        };
        inverse(acc0, lane_i, itw, tile, ack_hook);
        // limb 0's exact integer result (|.| < 2^45: nearest integer of the transform's output), held across the second transform
        double x0[16];
        static_for<0, 16>([&](auto J) {
            x0[J] = __builtin_rint(acc0[J]);
            if constexpr (STATS) dev = __builtin_fmax(dev, __builtin_fabs(acc0[J] - x0[J]));
        });
        pin();
        inverse(acc, lane_i, itw, tile);
        PH_MARK(6);   // both inverse transforms, including the wait for the partner's acknowledgement after the first DFT8
        // limb 1's result shifted into place, x 2^LB mod 2^AB: only the low AB - LB bits of the limb's integer survive the shift;
        // one pass over the lane's own accumulator words: old + limb 0 (2^47 + 2^45 stays exact), then the shifted limb 1, reduced
        static_for<0, 16>([&](auto J) {
            double x = __builtin_rint(acc[J]);
            if constexpr (STATS) dev = __builtin_fmax(dev, __builtin_fabs(acc[J] - x));
            constexpr double W = (double)(1ull << (AB - LB));
            x = __builtin_fma(-W, __builtin_rint(x * (1.0 / W)), x);
            keep[J] = mod_ab<AB>(__builtin_fma(x, (double)(1ull << LB), accf[lane_i + 64 * J] + x0[J]));
            accf[lane_i + 64 * J] = keep[J];
        });
        pin();
    }

    PH_MARK(7);
    PH_STORE(g_phase_f, wave, lane);
    if constexpr (STATS) atomicMax(stat, (unsigned long long)__double_as_longlong(dev));   // non-negative doubles order like their bit patterns
    if (!live) return;
    wave_sync();
    if constexpr (GLWE) {   // the accumulator itself, out = [count][2N]: this wavefront's polynomial (c = 0: mask, 1: body)
        u64 *g = out + (size_t)ct * (2 * N) + c * N;
        static_for<0, 16>([&](auto J) { t64::store_glwe_word<PRE, AB>(g, accf, t64::ResidueSlot<N, 0>{}, lane + 64 * J); });
        return;
    }
    u64 *o = out + (size_t)ct * (N + 1);
    if (c == 0) {
        static_for<0, 16>([&](auto J) {
            const uint32_t m = lane + 64 * J;
            const u64 v = f64_to_word(accf[m]) << PRE;
            if (m == 0) o[0] = v;
            else o[N - m] = (u64)0 - v;
        });
    } else if (lane == 0) {
        o[N] = f64_to_word(accf[0]) << PRE;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// LATENCY form: one workgroup of 16 wavefronts per ciphertext, every transform split over TWO wavefronts by parity
// (fft_half_f64.hpp: 256-point halves whose lane exchanges are register swaps and DPP moves - no LDS round trip inside a
// transform); three phases per CMUX separated by workgroup barriers
//   A  wavefronts 0 .. 4L-1 = (input polynomial c, level, parity h): rotate / decompose 512 coefficients of the u64 accumulator
//      (integer rule of the oracle), forward half -> tile (slot order)
//   B  all 1,024 threads = (limb j, output polynomial o, slot q): E + O' and E - O' of the 2L digit transforms, the two complex
//      multiply-accumulates per row against this thread's key words (own key copy: per slot the pair F_k, F_{k+256} side by
//      side; requested before phase A, landing under it), then the sum and the twisted difference for the inverse halves
//   C  wavefronts 0 .. 7 = (limb, o, parity): inverse half, nearest integer, shift into place and ONE LDS atomic add (f64) per
//      coefficient into the accumulator (the two limbs of a coefficient meet there)
// The accumulator is the exact integer word / 2^16 in a double, as in the wave-pair kernel, but only re-centred mod 2^48 every
// H_RECENTRE steps (the atomic adds cannot reduce): 2^47 + 8 (2^45 + 2^47) < 2^51 keeps every sum exact.
using namespace t64h;   // the family's constants (H_*), acc_slot and shared steps: t64_half_steps.hpp
constexpr int LF_LDS_WORDS = ffth::HT_WORDS + 2 * N + 2 * H_MAX_L * N + 2 * 2 * N + BMI_AT_WORDS;
static_assert(LF_LDS_WORDS <= BMI_LDS_WORDS_MAX, "LF_LDS_WORDS exceeds the 160 KB of LDS");

// standard-domain GGSW polynomials -> per (polynomial, limb) 256 slots of [F_k, F_{k+256}] (k = ffth::slot_freq of the slot)
__global__ void __launch_bounds__(256) k_bsk_to_latf_t64(const u64 *__restrict__ std_polys, double *__restrict__ lat_polys,
                                                         const double *__restrict__ g_tw_h, uint32_t n_polys, int prec) {
    const int limbs = t64::limbs_of(prec);
    __shared__ double lds[ffth::HT_WORDS + 4 * H_HALF];
    for (int i = threadIdx.x; i < ffth::HT_WORDS; i += blockDim.x) lds[i] = g_tw_h[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h = wave & 1;
    const uint32_t item = blockIdx.x * 2 + (wave >> 1);   // (polynomial, limb): two per workgroup, two wavefronts each
    const bool ok = item < n_polys * (uint32_t)limbs;
    const uint32_t poly = ok ? item / limbs : 0;
    const int j = ok ? (int)(item % limbs) : 0;
    double2 *tile = reinterpret_cast<double2 *>(lds + ffth::HT_WORDS + wave * H_HALF);   // 256 complex per wavefront
    if (ok) {
        double re[4], im[4];
        static_for<0, 4>([&](auto R) {
            const uint32_t m = 2 * (lane + 64 * R) + h;
            re[R] = (double)t64::limb_of((i64)std_polys[(size_t)poly * N + m], j, prec);
            im[R] = (double)t64::limb_of((i64)std_polys[(size_t)poly * N + m + 512], j, prec);
        });
        ffth::C v[4];
        forward_half_of(h, re, im, v, lane, lds);
        static_for<0, 4>([&](auto R) { tile[R * 64 + lane] = double2{v[R].r, v[R].i}; });   // (in the helper too: two s_nop fewer, not identical)
    }
    __syncthreads();
    if (ok) {
        const double2 *te = reinterpret_cast<const double2 *>(lds + ffth::HT_WORDS + (wave & ~1) * H_HALF), *to = te + H_HALF / 2;
        double2 *o = reinterpret_cast<double2 *>(lat_polys + (size_t)item * N);
        static_for<0, 2>([&](auto Q2) {
            const int q = (h * 2 + Q2) * 64 + lane;
            const double2 e = te[q], od = to[q];
            o[2 * q] = double2{e.x + od.x, e.y + od.y};
            o[2 * q + 1] = double2{e.x - od.x, e.y - od.y};
        });
    }
}

// STATS (the test hook bmi_fft_margin_host with the latency form selected): also records the largest distance of a limb sum from the
// integer it is rounded to
// GLWE: the kernel returns the accumulator itself, out = [count][2N], instead of the extracted sample, out = [count][N + 1]
template <int L, int BG, bool STATS, bool GLWE>
__global__ void __launch_bounds__(H_THREADS)
    k_blind_rotate_lat_t64f(const u64 *__restrict__ small_cts, const uint32_t *__restrict__ lut_ids, const u64 *__restrict__ luts,
                            const double *__restrict__ bsk_latf, const double *__restrict__ g_tw_h, u64 *__restrict__ out,
                            uint32_t count, uint32_t n, unsigned long long *__restrict__ stat) {
    constexpr int LIMBS = Scheme<48>::LIMBS, LB = Scheme<48>::BITS, PRE = Scheme<48>::PRE, AB = 64 - PRE;
    static_assert(2.0 * L * N * (double)(1ull << (BG - 1)) * (double)(1ull << (LB - 1)) <= 0x1p45, "limb sums must stay below 2^45");
    static_assert(LIMBS == 2 && L <= H_MAX_L && L * BG < AB, "two limbs, at most three levels");
    extern __shared__ double lds[];
    double *acc = lds + ffth::HT_WORDS;                                     // [2 components][2 parities][512]: word / 2^16, exact, |.| < 2^51
    double2 *tiles = reinterpret_cast<double2 *>(lds + ffth::HT_WORDS + 2 * N);   // [2L rows][2 halves][256 slots] complex
    double2 *SD = tiles + H_MAX_L * N;                                     // [limb][output][S, D][256 slots] complex
    uint16_t *at = reinterpret_cast<uint16_t *>(SD + 2 * N);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < ffth::HT_WORDS; i += H_THREADS) lds[i] = g_tw_h[i];
    const uint32_t ct = blockIdx.x;
    const u64 *lwe = small_cts + (size_t)ct * (n + 1);
    t64::stage_lwe<LOG_N + 1>(at, lwe, n, tid, H_THREADS);
    __syncthreads();
    {   // (written out in this family: a helper is identical here only, profiles/half_steps_ab.txt)
        const u64 *tv = luts + (size_t)(lut_ids[ct] & (BMI_LUT_CAP - 1)) * N;
        const uint32_t bt = at[n];
        t64::load_test_poly<N, PRE>(acc, acc_slot, tv, bt, tid);
    }
    __syncthreads();
    const int mj = tid >> 9, mo = (tid >> 8) & 1, mq = tid & 255;   // phase B: limb, output polynomial, slot
    uint32_t since_centred = 0;   // steps taken since the accumulator was last reduced mod 2^48
    double dev = 0.0;             // STATS: largest |value - nearest integer| this lane has rounded away

    for (uint32_t i = 0; i < n; i++) {
        const uint32_t a_t = at[i];
        if (a_t == 0) continue;  // uniform over the workgroup
        // key words of this thread: [row 2L][output 2][limb][256 slots][F_k, F_{k+256}]
        const double *bi = bsk_latf + (size_t)i * 4 * L * LIMBS * N;
        double2 klo[2 * L], khi[2 * L];
        static_for<0, 2 * L>([&](auto R) {
            const double2 *row = reinterpret_cast<const double2 *>(bi + ((size_t)(R * 2 + mo) * LIMBS + mj) * N);
            klo[R] = row[2 * mq];
            khi[R] = row[2 * mq + 1];
        });
        if (wave < 4 * L) {
            const int c = wave / (2 * L), lev = (wave % (2 * L)) >> 1, h = wave & 1;
            const double *ac = acc + c * N;
            double x[8];   // re[r] = x[r], im[r] = x[r + 4]
            double vr[8], vs[8];
            // coefficient m_J = 2 (lane + 64 (J & 3)) + h + 512 (J >> 2); its rotated source e_J = m_J - a_t mod 2N: half of it is
            // t0 + 64 (J & 3) + 256 (J >> 2) - the low 9 bits are the slot inside the parity block, bit 9 is the sign
            const uint32_t e0 = (2 * lane + h + 2 * N - a_t) & (2 * N - 1);
            const uint32_t t0 = e0 >> 1, pbase = (e0 & 1) * H_HALF;
            static_for<0, 8>([&](auto J) {
                const uint32_t t = t0 + 64 * (J & 3) + 256 * (J >> 2);
                vr[J] = ac[pbase + (t & (H_HALF - 1))];
                vs[J] = ac[h * H_HALF + lane + 64 * (J & 3) + 256 * (J >> 2)];
            });
            static_for<0, 8>([&](auto J) {
                const uint32_t t = t0 + 64 * (J & 3) + 256 * (J >> 2);
                const double dd = mod_ab<AB>(((t >> 9) & 1) ? -vr[J] - vs[J] : vr[J] - vs[J]);   // the centred lift of the u64 difference, / 2^PRE
                x[J] = t64::digit<L, BG, AB>(dd, lev);
            });
            const double re[4] = {x[0], x[1], x[2], x[3]}, im[4] = {x[4], x[5], x[6], x[7]};
            ffth::C v[4];
            forward_half_of(h, re, im, v, lane, lds);
            double2 *tile = tiles + (size_t)(wave >> 1) * H_HALF + h * (H_HALF / 2);   // (the store stays here: in the helper it renumbers registers)
            static_for<0, 4>([&](auto R) { tile[R * 64 + lane] = double2{v[R].r, v[R].i}; });
        }
        __syncthreads();
        {
            ffth::C ylo{0.0, 0.0}, yhi{0.0, 0.0};
            static_for<0, 2 * L>([&](auto R) {
                const double2 e = tiles[(size_t)R * H_HALF + mq], od = tiles[(size_t)R * H_HALF + H_HALF / 2 + mq];
                mac_pair(ylo, yhi, e, od, klo[R], khi[R]);
            });
            const double2 w = reinterpret_cast<const double2 *>(lds + ffth::HT_W)[mq];
            sum_diff_store(SD + (size_t)(mj * 2 + mo) * H_HALF, mq, ylo, yhi, w);
        }
        __syncthreads();
        // phase C: eight tasks (limb, output, parity) meeting by LDS f64 atomics; four tasks running both limbs' inverse halves
        // with plain read-modify-writes measured 3.80 / 4.01 ms for 1 / 256 against 3.60 / 3.95 (four wavefronts leave the SIMDs idle)
        if (wave < 4 * LIMBS) {
            const int j = wave >> 2, o = (wave >> 1) & 1, h = wave & 1;
            const double2 *sd = SD + (size_t)(j * 2 + o) * H_HALF + h * (H_HALF / 2);
            ffth::C v[4];
            read_sums(v, sd, lane);
            double re[4], im[4];   // (from here written out: a helper gives the same counts in another order and, timed, missed the rule at one bootstrap - profiles/half_steps_ab.txt)
            if (h) ffth::inverse_half<1>(v, re, im, lane, lds);
            else ffth::inverse_half<0>(v, re, im, lane, lds);
            double *ao = acc + o * N + h * H_HALF + lane;
            static_for<0, 4>([&](auto R) {
                atomicAdd(ao + 64 * R, t64::place_limb<AB, LB, STATS>(re[R], j, dev));          // coefficient 2 (lane + 64 R) + h
                atomicAdd(ao + 64 * R + 256, t64::place_limb<AB, LB, STATS>(im[R], j, dev));    // ... + 512
            });
        }
        __syncthreads();
        if (++since_centred == H_RECENTRE) {   // (uniform: counts the steps actually taken) keep the accumulator's magnitude below 2^51
            since_centred = 0;
            recentre<AB, 2>(acc, tid);
            __syncthreads();
        }
    }
    if constexpr (STATS) atomicMax(stat, (unsigned long long)__double_as_longlong(dev));   // non-negative doubles order like their bit patterns
    if constexpr (GLWE) t64::store_glwe<N, PRE, AB>(out + (size_t)ct * (2 * N), acc, acc_slot, tid);   // out = [count][2N]
    else t64::extract_sample<N, PRE, AB>(out + (size_t)ct * (N + 1), acc, acc_slot, tid);
}

}  // namespace

PH_EXPORT(bmi_debug_phase_prof_t64f, g_phase_f)

namespace bmit {

int launch_bsk_to_fft(const KeyConv &k) {
    if (k.prec != 48) return (int)hipErrorInvalidValue;
    const uint32_t items = k.n_polys * (uint32_t)t64::limbs_of(k.prec);
    hipLaunchKernelGGL(k_bsk_to_fft_t64, dim3((items + 3) / 4), dim3(256), 0, k.s, k.std_polys, (double *)k.dst, k.tab[0].d(), k.n_polys, k.prec);
    BMI_LAUNCH_CHECK();
    return 0;
}

int launch_bsk_to_latf(const KeyConv &k) {
    if (k.prec != 48 && k.prec != 42) return (int)hipErrorInvalidValue;   // (42: the unrolled key of bmi_kernels_t64fu.hip)
    const uint32_t items = k.n_polys * (uint32_t)t64::limbs_of(k.prec);
    hipLaunchKernelGGL(k_bsk_to_latf_t64, dim3((items + 1) / 2), dim3(256), 0, k.s, k.std_polys, (double *)k.dst, k.tab[0].d(), k.n_polys, k.prec);
    BMI_LAUNCH_CHECK();
    return 0;
}

int launch_blind_rotate_lat_fft(const RotBatch &b) {
    if (b.count == 0) return 0;
    if (!shape_supported_fft(b.prec, b.levels, b.base_log)) return (int)hipErrorInvalidValue;
    return with_levels_stats_glwe(b.levels, b.stat != nullptr, b.glwe, [&](auto L, auto STATS, auto GLWE) {
        return launch_with_lds<k_blind_rotate_lat_t64f<L, 10, STATS, GLWE>>(dim3(b.count), dim3(H_THREADS), (size_t)LF_LDS_WORDS * sizeof(double), b.s,
                                                                             b.cts, b.ids, b.luts.u(), b.key.d(), b.tab[0].d(), b.out, b.count, b.n, b.stat);
    });
}

int launch_blind_rotate_fft(const RotBatch &b) {
    if (b.count == 0) return 0;
    if (!shape_supported_fft(b.prec, b.levels, b.base_log)) return (int)hipErrorInvalidValue;
    return with_levels_stats_glwe(b.levels, b.stat != nullptr, b.glwe, [&](auto L, auto STATS, auto GLWE) {
        return launch_with_lds<k_blind_rotate_t64f<L, 10, STATS, GLWE>>(dim3((b.count + TF_CTS - 1) / TF_CTS), dim3(128 * TF_CTS),
                                                                         (size_t)TF_LDS_WORDS * sizeof(double), b.s, b.cts, b.ids, b.luts.u(), b.key.d(),
                                                                         b.tab[0].d(), b.out, b.count, b.n, b.stat);
    });
}

}  // namespace bmit
