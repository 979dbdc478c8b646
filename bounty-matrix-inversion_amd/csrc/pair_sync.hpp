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
//   first two butterfly stages of the first register DFT8 of P's inverse transform
//   pair_wait(ack_Q, h)      (the hook of fftw::inverse)
//   first store of the inverse transform into P's tile
// Both wavefronts of a pair play both roles in every hand-off.  No wait of hand-off h depends on anything the partner does after
// one of ITS waits of hand-off h or later: pub(h) is posted after the wait for ack(h - 1), which the partner posted before it
// reached its wait for pub(h) - so the waits cannot form a cycle.
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
