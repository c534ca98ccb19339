// f8_concat.hip — channel concatenation (f8_net_concat): out = concat(x_0 .. x_{K-1}) along C, K <= F8_MAX_CONCAT sources of one map.
//
// Memory-bound gathers, grid-stride, no LDS, plain vector loads / stores.  The planner (plan_tensor_forms, f8_net.cpp) picks the mode per node:
//   concat_i8   every source already exists in the OUTPUT's int8 format (its producer requantised it by n_i = n - (out.fl - fl_i)), so the launch
//               moves bytes: concat_i8_kernel<ALIGNED>.  Up to two output forms per launch, each with its own set of source pointers.
//   concat_i32  sources in their int32 form (I32T, i32t_index): shift left by out.fl - fl_i with the reference's wrap, clamp_sym31
//               (fix_resnet.py:40-54 with a zero residual), optional int32 output, up to two int8 forms through QuantOut: concat_i32_kernel.
// The source of a channel is found by an unrolled compare / select walk over the table in the kernel arguments: the table is never indexed with a
// lane's value, so it stays in scalar registers (a dynamically indexed by-value array would move to scratch).
// Pad channels [sum C_i, Cs) of the output are written as the format's zero — 0 in int32, 0 ^ bias_xor per byte in int8 (0x80 for unsigned forms) —
// because every int8 conv reads Cs channels; a source's own pad bytes are never copied.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "f8_device.h"

namespace f8 {

// ALIGNED (every channel offset and every C_i a multiple of 16): one lane owns one 16-byte vector of an output pixel — one 16 B load, one 16 B store
// per form.  General: a lane owns 4 output bytes and merges them from the dwords of every source that overlaps them (at most two aligned dwords per
// source and group: the source row starts 4-byte aligned, the group's first byte sits at byte `lc & 3` of the first).
template <bool ALIGNED>
__global__ void __launch_bounds__(256) concat_i8_kernel(const ConcatArgs a) {
    constexpr int V = ALIGNED ? 16 : 4;
    const unsigned vpp = (unsigned)a.Cs / V;                         // vectors per output pixel
    const size_t total = (size_t)a.M * vpp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const unsigned m = (unsigned)(idx / vpp);
        const int c = (int)(idx - (size_t)m * vpp) * V;
        if constexpr (ALIGNED) {
            int lc = 0, cs = 0;
            const int8_t* p0 = nullptr; const int8_t* p1 = nullptr;
#pragma unroll
            for (int i = 0; i < kMaxConcat; ++i)
                if (i < a.K && c >= a.off[i] && c < a.off[i] + a.C[i]) { lc = c - a.off[i]; cs = a.Cs_src[i]; p0 = (const int8_t*)a.src[0][i]; p1 = (const int8_t*)a.src[1][i]; }
            const size_t so = (size_t)m * cs + lc, dst = (size_t)m * a.Cs + c;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!a.q[k].ptr) continue;
                const int8_t* p = k ? p1 : p0;
                const unsigned z = a.q[k].bias_xor;
                uint4 v = {z, z, z, z};                              // c >= sum C_i: the format's zero
                if (p) v = *(const uint4*)(p + so);
                *(uint4*)(a.q[k].ptr + dst) = v;
            }
        } else {
            unsigned w[2] = {a.q[0].bias_xor, a.q[1].bias_xor};
#pragma unroll
            for (int i = 0; i < kMaxConcat; ++i) {
                if (i >= a.K) break;
                const int lc = c - a.off[i];                          // the group's first channel in source i's numbering
                if (lc <= -4 || lc >= a.C[i]) continue;
                const int base = lc & ~3, sh = (lc & 3) * 8;          // (lc in -3 .. -1: base = -4, only the second dword is read)
                unsigned mask = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) if (lc + e >= 0 && lc + e < a.C[i]) mask |= 0xffu << (8 * e);
                const size_t row = (size_t)m * a.Cs_src[i];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    if (!a.q[k].ptr) continue;
                    const int8_t* p = (const int8_t*)a.src[k][i] + row;
                    const unsigned lo = base >= 0 ? *(const unsigned*)(p + base) : 0u;
                    const unsigned hi = (sh && base + 4 < a.Cs_src[i]) ? *(const unsigned*)(p + base + 4) : 0u;
                    const unsigned v = (unsigned)((((unsigned long long)hi << 32) | lo) >> sh);
                    w[k] = (w[k] & ~mask) | (v & mask);
                }
            }
            const size_t dst = (size_t)m * a.Cs + c;
#pragma unroll
            for (int k = 0; k < 2; ++k) if (a.q[k].ptr) *(unsigned*)(a.q[k].ptr + dst) = w[k];
        }
    }
}

// One lane = one pixel x 4 output channels, as add_kernel.  The group may straddle sources at any offset: each overlapping source is read through
// i32t_index — one 16-byte load where the group starts on a 4-channel boundary of the source, single dwords otherwise.
__global__ void __launch_bounds__(256) concat_i32_kernel(const ConcatArgs a) {
    const int cgs = a.Cs >> 2;
    const size_t total = (size_t)a.M * cgs;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % cgs) << 2, m = (int)(idx / cgs);
        int y[4] = {0, 0, 0, 0};                                      // pad channels: 0
#pragma unroll
        for (int i = 0; i < kMaxConcat; ++i) {
            if (i >= a.K) break;
            const int lc = c - a.off[i];
            if (lc <= -4 || lc >= a.C[i]) continue;
            const int32_t* p = (const int32_t*)a.src[0][i];
            int v[4] = {0, 0, 0, 0};
            if (lc >= 0 && (lc & 3) == 0) {                           // (the source's channels are padded to 32: the four ints exist)
                const v4i t = *(const v4i*)(p + i32t_index(m, lc, a.Cs_src[i]));
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (lc + e >= 0 && lc + e < a.C[i]) v[e] = p[i32t_index(m, lc + e, a.Cs_src[i])];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (lc + e >= 0 && lc + e < a.C[i]) y[e] = clamp_sym31((int)((unsigned)v[e] << a.shl[i]));
        }
        if (a.out32) { v4i o = {y[0], y[1], y[2], y[3]}; *(v4i*)(a.out32 + i32t_index(m, c, a.Cs)) = o; }
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (a.q[k].ptr)
                *(unsigned*)(a.q[k].ptr + (size_t)m * a.Cs + c) =
                    requant_pack4(y[0], y[1], y[2], y[3], a.q[k]);
    }
}

// 0: concat_i32_kernel, 1: concat_i8_kernel<true>, 2: concat_i8_kernel<false>
int concat_inst(const ConcatArgs& a, bool i8) {
    if (!i8) return 0;
    for (int i = 0; i < a.K; ++i) if ((a.off[i] | a.C[i]) & 15) return 2;
    return 1;
}
const char* concat_kernel_name(int inst) {
    return inst == 0 ? "f8::concat_i32_kernel" : inst == 1 ? "f8::concat_i8_kernel<true>" : "f8::concat_i8_kernel<false>";
}
hipError_t launch_concat(const ConcatArgs& a, int inst, hipStream_t s) {
    if (a.K < 2 || a.K > kMaxConcat || a.M < 1 || (a.Cs & 31)) return hipErrorInvalidValue;
    const size_t work = (size_t)a.M * (a.Cs / (inst == 1 ? 16 : 4));
    const dim3 grid((unsigned)std::min<size_t>((work + 255) / 256, 8192));
    if (inst == 0) hipLaunchKernelGGL(concat_i32_kernel, grid, dim3(256), 0, s, a);
    else if (inst == 1) hipLaunchKernelGGL(concat_i8_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(concat_i8_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace f8
