// Synchronisation of the two wavefronts that share a ciphertext in the wave-pair kernels (bmi_kernels_t64.hip,
// bmi_kernels_t64f.hip, k_blind_rotate_tpx49 of bmi_kernels_f64.hip): LDS counters posted by one wavefront and polled by its partner.
//
// The hand-off of one partial sum (counter value h, strictly increasing; "tile" = the publisher's own transform scratch):
//   publisher P                                         consumer Q (the partner)
//   stores the partial into P's tile
//   pair_post(pub_P, h)      release: orders the stores
//                                                       pair_wait(pub_P, h)
//                                                       reads P's tile (eight ds_read_b128 per lane)
//                                                       pair_ack(ack_Q, h)   ordered after those reads only
//   pair_wait(ack_Q, h)
//   next write of P's tile
// Both wavefronts of a pair play both roles in every hand-off.  In bmi_kernels_t64f.hip a CMUX has two hand-offs through the one
// tile, h0 (limb 0) and h1 (limb 1), with L key rows between any two waits but the last:
//   rows (limb 0, partner's column); store partial; pair_post(pub, h0)
//   rows (limb 0, own column);       pair_wait(pub_partner, h0); add the partner's partial; pair_ack(ack, h0)
//   rows (limb 1, partner's column); pair_wait(ack_partner, h0); store partial; pair_post(pub, h1)
//   rows (limb 1, own column);       pair_wait(pub_partner, h1); add the partner's partial; pair_ack(ack, h1)
//   first two butterfly stages of the first register DFT8 of the first inverse transform;
//   pair_wait(ack_partner, h1)       (the hook of fftw::inverse); first store of the transform into the tile; second inverse transform
// (the other two kernels have one hand-off per inverse transform: post, wait + read + ack, the hook's wait.)
// No wait depends on anything the partner does after one of ITS waits for the same or a later flag value: pub(h) is posted after the
// wait for ack(h - 1), which the partner posted before it reached its wait for pub(h), and ack(h) is posted after the wait for pub(h)
// only - so the waits cannot form a cycle.  The flags are compared for EQUALITY: pub(h + 1) must not be posted before the partner's
// ack(h) is seen, or a partner that has not yet looked for pub(h) never finds it (tests/test_pair_handoff_order_model.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t pair_lds_addr(const uint32_t *flag) {
    return (uint32_t)(size_t)(__attribute__((address_space(3))) const uint32_t *)flag;
}
__device__ __forceinline__ void pair_post(uint32_t *flag, uint32_t v) {
    __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// Acknowledges that this wavefront has read the partner's tile.  The LDS serves a wavefront's operations in the order they were
// issued and lgkmcnt(0) waits until every one of them (the tile reads are the last) has returned its data; the flag store is
// issued after that.  Unlike a release store this does not wait for the wavefront's outstanding GLOBAL loads (vmcnt): key rows
// requested ahead stay in flight across the acknowledgement.  The tile reads must precede this call in program order; the
// "memory" clobber keeps the compiler from moving them below it.
__device__ __forceinline__ void pair_ack(uint32_t *flag, uint32_t v) {
    asm volatile(
        "s_waitcnt lgkmcnt(0)\n\t"
        "ds_write_b32 %0, %1"
        :
        : "v"(pair_lds_addr(flag)), "v"(v)
        : "memory");
}
// one opaque asm block (as C++ control flow the poll loop makes the register allocator spill: ~180 dwords per lane measured in
// k_blind_rotate_tpx49); all lanes read the same LDS word
__device__ __forceinline__ void pair_wait(uint32_t *flag, uint32_t v) {
    uint32_t tmp;
    asm volatile(
        "1:\n\t"
        "ds_read_b32 %0, %1\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_cmp_eq_u32 vcc, %2, %0\n\t"
        "s_cbranch_vccnz 2f\n\t"
        "s_sleep 1\n\t"
        "s_branch 1b\n"
        "2:"
        : "=&v"(tmp)
        : "v"(pair_lds_addr(flag)), "s"(v)
        : "vcc", "memory");
}
// The workgroup's hardware barrier for the wavefronts whose `here` (wave-uniform, read from the first lane) is non-zero; the others
// fall through.  Bare: no fence and no wait for outstanding memory operations in front of it - it paces wavefronts, it does not
// order their LDS words.  The hardware counts arrivals, not sites: two groups of wavefronts may execute their barrier k at
// different places of the same loop as long as every wavefront executes the same NUMBER of barriers.  One opaque block, as
// pair_wait (the condition is a scalar, the branch never reaches the register allocator).
__device__ __forceinline__ void barrier_if(bool here) {
    asm volatile(
        "s_cmp_eq_u32 %0, 0\n\t"
        "s_cbranch_scc1 .Lbarrier_if_%=\n\t"
        "s_barrier\n"
        ".Lbarrier_if_%=:"
        :
        : "s"(__builtin_amdgcn_readfirstlane((uint32_t)here))
        : "scc", "memory");
}
// nothing moves across this point (neither the compiler's memory operations nor the instruction scheduler's)
__device__ __forceinline__ void pin() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
