// f8_chain_common.h — what the stage-chain kernels share (f8_chain.hip, f8_bchain.hip, f8_cchain.hip, f8_bcchain.hip; included by those four only):
// the protocol by which their workgroups hand data to each other through memory, and the tile helpers around it (gfx950).
//
// Exchange protocol, on the scratch of ChainSync (f8_internal.h):
//   * ticket: one lane per workgroup takes its place in the LOGICAL grid from an atomic counter (sync[0]).  The set of started workgroups is
//     then a prefix of the logical grid, whatever order the hardware starts them in: a workgroup only ever waits for one that has started.
//   * signal: the producer writes its data with write-through stores (sc0 sc1), every storing wave drains (vmcnt(0)), a barrier, then ONE relaxed
//     agent-scope flag store of the exchange number `seq` (sync[16 + workgroup]).
//   * wait: one lane per awaited flag polls it (agent scope), bounded by a wall-clock limit.  A workgroup that never arrives sets the sticky error
//     word (epoch << 8) | code | (seq & 0x3f) and its host mirror, and the launch RUNS ON without waiting any more — here and in every other
//     workgroup, which see the word of this run's epoch in their own polls.  (An early return from the middle of a block loop would give the loop a
//     second exit: in f8_chain.hip's opening-block instance that was a second copy of the 112 stream registers at the loop header and its spills.)
//   * re-arm: the last workgroup out zeroes the ticket, the counter (sync[1]) and the flags for the NEXT launch on this scratch (round 4: the
//     hipMemsetAsync node in front of every chain launch was 3 x 5 us per step on the critical path).  A workgroup counts itself out once ITS flag
//     stores have been performed (lane 0 issued them: its vmcnt(0)) and its last poll has returned; the last one out sees every other workgroup
//     past its last access of the words, and the kernel boundary orders the zeroes before the next launch.  Every workgroup gets there — a
//     timed-out wait runs on — and the words are zeroed once at allocation (f8_net.cpp), so the first launch starts clean.
// Every helper takes the ChainSync BY REFERENCE (a.cs): passing its fields as separate values changed the kernels' SGPR allocation.
#pragma once
#include "f8_device.h"

namespace f8 {

// ticket: this workgroup's place in the logical grid (one lane calls it)
__device__ __forceinline__ unsigned chain_ticket(const ChainSync& s) {
    return __hip_atomic_fetch_add(s.sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the flags, one per workgroup.  A kernel takes this pointer and its wait bound (timeout_ticks) ONCE at the top and hands them to the helpers
// below: read from the ChainSync inside them, they were loaded again late in the kernel, and that changed the register allocation.
__device__ __forceinline__ unsigned* chain_flags(const ChainSync& s) { return s.sync + 16; }

// the flag store alone: exchange `seq` of this workgroup is in memory (one lane, behind the drain and the barrier)
__device__ __forceinline__ void chain_flag(unsigned* flag, unsigned seq) {
    __hip_atomic_store(flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// signal: every storing wave drains, barrier, one flag store
__device__ __forceinline__ void chain_signal(unsigned* flag, unsigned seq) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) chain_flag(flag, seq);
}

// bounded wait of one lane for `flag` to reach `seq`; on a time-out: the sticky error word with CODE, and run on
template <unsigned CODE, int SLEEP>
__device__ __forceinline__ void chain_wait_flag(const ChainSync& s, const unsigned* flag, unsigned seq, unsigned long long t_limit) {
    const unsigned long long t0 = wall_clock64();
    bool ok = true;
    while ((int)(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - seq) < 0) {
        __builtin_amdgcn_s_sleep(SLEEP);
        if (wall_clock64() - t0 > t_limit) { ok = false; break; }
        if ((__hip_atomic_load(s.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 8) == s.epoch) break;   // another workgroup of THIS run gave up
    }
    if (!ok) {
        __hip_atomic_store(s.err, (s.epoch << 8) | CODE | (seq & 0x3fu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s.err_host) __hip_atomic_store(s.err_host, (s.epoch << 8) | CODE | (seq & 0x3fu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// re-arm (the whole workgroup of NT threads calls it, behind its last exchange): `last` is an LDS word
template <int NT>
__device__ __forceinline__ void chain_rearm(const ChainSync& s, unsigned* flags, int* last) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        *last = (__hip_atomic_fetch_add(s.sync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u) ? 1 : 0;
    }
    __syncthreads();
    if (*last) {
        for (int i = tid; i < (int)gridDim.x; i += NT) __hip_atomic_store(flags + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid == 0) { __hip_atomic_store(s.sync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __hip_atomic_store(s.sync + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    }
}

#define F8_LDS3(p) ((__attribute__((address_space(3))) void*)(p))

// a scalar the optimiser may not look through (keeps run-time rotated addresses from being precomputed for every unrolled step)
__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+s"(v)); return v; }

// 16 accumulator values of one 32x32 tile (this lane: one pixel, channels 8g + 4 lh + e) -> this lane's 16 bytes: channels [16 lh, 16 lh + 16) of the
// tile (two v_permlane32_swap put a lane's four dwords side by side) — a piece of an int8 row, and in the cluster kernels' fragment order the lane's
// 16 bytes of the consumer's B fragment.
// FAST: unsigned 8-bit behind a ReLU with a right shift; otherwise either direction, any clamp.  FAST == 1: through the float converter
// (requant_u8x4, 3 operations per value, f8_device.h) — planned only where every shift is 1 .. 16 and the planner has BOUNDED every value that is
// requantised: the conv accumulators (ChainArgs::acc_ok) and, since round 4, the int32 stream itself (ChainArgs::stream_ok: the stream of a chain
// that starts with a stage-opening block is a sum of bounded accumulators — the 4-operation wrap-exact float form round 3 used for it cost the
// 56x56 launch 6.5 %); FAST == 2: the INTEGER form (requant_u8x4_int: v_bfe_u32, v_add3_u32, v_ashr_pk_u8_i32 — no float instruction; exact for
// every int32, the reference's wrap included, and any shift): option requant_float = 0, or anything unbounded.
template <int FAST, bool ACC = false, class Y>
__device__ __forceinline__ v4i quant_tile16(const Y& y, int n, int lo, int hi, unsigned x_or) {
    unsigned d[4];
    const float sc = FAST == 1 ? requant_u8_scale(n) : 0.0f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if constexpr (FAST == 1) d[g] = requant_u8x4(y[4 * g], y[4 * g + 1], y[4 * g + 2], y[4 * g + 3], sc) ^ x_or;
        else if constexpr (FAST == 2) d[g] = requant_u8x4_int(y[4 * g], y[4 * g + 1], y[4 * g + 2], y[4 * g + 3], n) ^ x_or;
        else d[g] = pack4(requant1(y[4 * g], n, lo, hi), requant1(y[4 * g + 1], n, lo, hi), requant1(y[4 * g + 2], n, lo, hi), requant1(y[4 * g + 3], n, lo, hi)) ^ x_or;
    }
    auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
    auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
    const v4i o = {(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
    return o;
}

// barrier that leaves vector-memory operations (the LDS-DMA ring) in flight: __syncthreads() drains them (s_waitcnt vmcnt(0) in front of every s_barrier —
// each ring stage then exposes its whole latency); LDS accesses are complete, and no memory access moves across it
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// Found with f8_cchain.hip (round 6).  In the TAIL phase seven independent MFMAs (one per pixel tile) end a K step and the epilogue's vector code follows.
// Left to itself the scheduler moved that code up INTO the last step: the float-converter instance (FAST = 1) read the first tile's accumulators one MFMA
// + `s_nop 6` behind the MFMA that writes them, and wrote `v_cvt_f32_i32 v114, ...` in the slot after `v_mfma ..., v[114:117], ...` (a dying B operand, reused
// at once).  That build returned a few pixels of a tile DIFFERENT FROM RUN TO RUN (tests/test_gpu_chain.py, requant_float=1 on the 7x7 TAIL chain; the
// integer instance, scheduled differently, was exact); with the vector code kept behind the MFMAs it is bit-exact (every variant of this guard, 0 to 16
// wait states).  The mechanism is NOT isolated: tools/ubench/ubench_mfma_hazard.hip (profiles/ubench_mfma_hazard_r06.txt) shows the hardware interlocks a
// vector write to SrcA / SrcB right behind the MFMA (never a wrong result, with or without a backlog of MFMAs), and that a vector read of a result needs
// 9 .. 16 wait states directly behind its MFMA, 3 .. 4 with one independent MFMA in between, none with two — the compiler's `s_nop 6` satisfies that.  What
// is known is the cure: nothing is scheduled across the end of an MFMA group (an `asm volatile` alone does not stop the machine scheduler — the first
// version of this guard left the instructions where they were), plus wait states.  The cluster kernels (f8_cchain.hip, f8_bcchain.hip) use it behind
// every MFMA group, so the tuning switches below reach both.
#ifndef F8_CC_WAR_NOPS
#define F8_CC_WAR_NOPS 16
#endif
__device__ __forceinline__ void mfma_operands_read() {
#ifdef F8_CC_NO_GUARD       // (tuning / demonstration builds: the schedule the compiler picks by itself)
    return;
#endif
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (F8_CC_WAR_NOPS >= 16) asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
    else if constexpr (F8_CC_WAR_NOPS >= 8) asm volatile("s_nop 7" ::: "memory");
    else if constexpr (F8_CC_WAR_NOPS >= 4) asm volatile("s_nop 3" ::: "memory");
    else if constexpr (F8_CC_WAR_NOPS >= 2) asm volatile("s_nop 1" ::: "memory");
    else if constexpr (F8_CC_WAR_NOPS >= 1) asm volatile("s_nop 0" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

}  // namespace f8
