// f8_chanmap.hip — channel slice (f8_net_slice) and channel shuffle (f8_net_channel_shuffle): out[c] = src[first + c] and
// out[c] = src[(c % groups) * Cg + c / groups], Cg = C / groups (torch.nn.functional.channel_shuffle).  No arithmetic: no shift, clamp or ReLU.
//
// Memory-bound gathers, grid-stride, 256 threads, no LDS, plain vector loads / stores, arguments by value, no communication between workgroups.
// The planner (plan_tensor_forms, f8_net.cpp) picks the mode per node, the nearest-upsample rule:
//   i8    the source's producer already wrote the OUTPUT's int8 formats (a channel gather commutes with every element-wise function), so the launch
//         moves bytes.  slice_i8_kernel<ALIGNED>; shuffle_i8_kernel<V> for two groups whose width and offsets are multiples of V; every other
//         shuffle shuffle_i8_general_kernel.  Up to two output forms per launch, each with its own source pointers.
//   i32   the source's int32 form (I32T, i32t_index) gathered into the output's int32 form and / or up to two int8 forms through QuantOut:
//         chanmap_i32_kernel, both ops.
// A shuffle reads a TABLE of `groups` entries (pointer per form, row stride, channel offset): stand-alone entry i is the source at offset i * Cg,
// fused with the concat in front of it (concat+shuffle{g}_i8:) entry i is concat operand i at offset 0 — the kernels see no other difference.  The
// table is walked with unrolled compare / select and never indexed with a lane's value, so it stays in scalar registers.
// Pad channels [C, Cs) of the output are written as the format's zero — 0 in int32, 0 ^ bias_xor per byte in int8 (0x80 for unsigned forms) —
// because every int8 conv reads Cs channels.  Source bytes past the slice's last channel, the source's own pad bytes among them, are masked.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "f8_device.h"

namespace f8 {

// the first `rem` bytes of a dword (rem <= 0: none, rem >= 4: all)
__device__ __forceinline__ unsigned head_mask(int rem) { return rem >= 4 ? 0xffffffffu : rem <= 0 ? 0u : (1u << (8 * rem)) - 1u; }

// ALIGNED (first % 16 == 0): a lane owns one 16-byte vector of an output pixel — one 16 B load, one 16 B store per form.  General: a lane owns 4
// output bytes and funnel-shifts them out of the two aligned source dwords that hold them (the source row starts 4-byte aligned, the group's first
// byte sits at byte `(first + c) & 3` of the first).  Loads stay inside the source row: first + c < first + C <= Cs_src.
template <bool ALIGNED>
__global__ void __launch_bounds__(256) slice_i8_kernel(const ChanMapArgs a) {
    constexpr int V = ALIGNED ? 16 : 4;
    const unsigned vpp = (unsigned)a.Cs / V;                         // vectors per output pixel
    const size_t total = (size_t)a.M * vpp;
    const int first = a.off[0], cs = a.Cs_src[0];
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const unsigned m = (unsigned)(idx / vpp);
        const int c = (int)(idx - (size_t)m * vpp) * V;
        const int rem = a.C - c;                                      // real channels from c on (<= 0: a pad vector)
        const size_t so = (size_t)m * cs + first + c, dst = (size_t)m * a.Cs + c;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!a.q[k].ptr) continue;
            const int8_t* p = (const int8_t*)a.src[k][0];
            const unsigned z = a.q[k].bias_xor;
            if constexpr (ALIGNED) {
                uint4 v = {z, z, z, z};
                if (rem > 0) {
                    const uint4 x = *(const uint4*)(p + so);
                    const unsigned m0 = head_mask(rem), m1 = head_mask(rem - 4), m2 = head_mask(rem - 8), m3 = head_mask(rem - 12);
                    v.x = (x.x & m0) | (z & ~m0); v.y = (x.y & m1) | (z & ~m1); v.z = (x.z & m2) | (z & ~m2); v.w = (x.w & m3) | (z & ~m3);
                }
                *(uint4*)(a.q[k].ptr + dst) = v;
            } else {
                unsigned w = z;
                if (rem > 0) {
                    const int lc = first + c, base = lc & ~3, sh = (lc & 3) * 8;
                    const int8_t* row = p + (size_t)m * cs;
                    const unsigned lo = *(const unsigned*)(row + base);
                    const unsigned hi = (sh && base + 4 < cs) ? *(const unsigned*)(row + base + 4) : 0u;
                    const unsigned x = (unsigned)((((unsigned long long)hi << 32) | lo) >> sh);
                    const unsigned mk = head_mask(rem);
                    w = (x & mk) | (z & ~mk);
                }
                *(unsigned*)(a.q[k].ptr + dst) = w;
            }
        }
    }
}

// Two groups, V in {16, 4, 2} dividing Cg and both entries' offsets: a lane reads V consecutive bytes of each group and writes the 2 V interleaved
// bytes contiguously — {a0, b0, a1, b1} and {a2, b2, a3, b3} of a dword pair by v_perm_b32 (the byte transpose of f8_dws7.hip).  A vector is all real
// (j V < Cg) or all pad.
template <int V>
__global__ void __launch_bounds__(256) shuffle_i8_kernel(const ChanMapArgs a) {
    const unsigned ipp = (unsigned)a.Cs / (2 * V);                   // items per output pixel
    const size_t total = (size_t)a.M * ipp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const unsigned m = (unsigned)(idx / ipp);
        const int gc = (int)(idx - (size_t)m * ipp) * V;              // first channel inside each group
        const bool real = gc < a.Cg;
        const size_t s0 = (size_t)m * a.Cs_src[0] + a.off[0] + gc, s1 = (size_t)m * a.Cs_src[1] + a.off[1] + gc;
        const size_t dst = (size_t)m * a.Cs + 2 * gc;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!a.q[k].ptr) continue;
            const int8_t* p0 = (const int8_t*)a.src[k][0]; const int8_t* p1 = (const int8_t*)a.src[k][1];
            const unsigned z = a.q[k].bias_xor;
            if constexpr (V == 16) {
                uint4 lo = {z, z, z, z}, hi = lo;
                if (real) {
                    const uint4 x = *(const uint4*)(p0 + s0), y = *(const uint4*)(p1 + s1);
                    lo.x = __builtin_amdgcn_perm(y.x, x.x, 0x05010400u); lo.y = __builtin_amdgcn_perm(y.x, x.x, 0x07030602u);
                    lo.z = __builtin_amdgcn_perm(y.y, x.y, 0x05010400u); lo.w = __builtin_amdgcn_perm(y.y, x.y, 0x07030602u);
                    hi.x = __builtin_amdgcn_perm(y.z, x.z, 0x05010400u); hi.y = __builtin_amdgcn_perm(y.z, x.z, 0x07030602u);
                    hi.z = __builtin_amdgcn_perm(y.w, x.w, 0x05010400u); hi.w = __builtin_amdgcn_perm(y.w, x.w, 0x07030602u);
                }
                *(uint4*)(a.q[k].ptr + dst) = lo;
                *(uint4*)(a.q[k].ptr + dst + 16) = hi;
            } else if constexpr (V == 4) {
                uint2 o = {z, z};
                if (real) {
                    const unsigned x = *(const unsigned*)(p0 + s0), y = *(const unsigned*)(p1 + s1);
                    o.x = __builtin_amdgcn_perm(y, x, 0x05010400u); o.y = __builtin_amdgcn_perm(y, x, 0x07030602u);
                }
                *(uint2*)(a.q[k].ptr + dst) = o;
            } else {
                unsigned o = z;
                if (real) {
                    const unsigned x = *(const unsigned short*)(p0 + s0), y = *(const unsigned short*)(p1 + s1);
                    o = __builtin_amdgcn_perm(y, x, 0x05010400u);
                }
                *(unsigned*)(a.q[k].ptr + dst) = o;
            }
        }
    }
}

// Any groups 2 .. 8, any C: a lane owns 4 output bytes c .. c + 3 and fetches each from its group — output channel oc is byte oc / groups of entry
// oc % groups.  (quotient, remainder) of c once by the magic divisor, then counted up.
__global__ void __launch_bounds__(256) shuffle_i8_general_kernel(const ChanMapArgs a) {
    const unsigned vpp = (unsigned)a.Cs >> 2;
    const size_t total = (size_t)a.M * vpp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const unsigned m = (unsigned)(idx / vpp);
        const int c = (int)(idx - (size_t)m * vpp) << 2;
        int qo = (int)fast_div((unsigned)c, a.dG), r = c - qo * a.groups;
        unsigned w[2] = {a.q[0].bias_xor, a.q[1].bias_xor};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (c + e < a.C) {
                const int8_t* p0 = nullptr; const int8_t* p1 = nullptr; int cs = 0, off = 0;
#pragma unroll
                for (int i = 0; i < kMaxConcat; ++i)
                    if (i == r) { p0 = (const int8_t*)a.src[0][i]; p1 = (const int8_t*)a.src[1][i]; cs = a.Cs_src[i]; off = a.off[i]; }
                const size_t so = (size_t)m * cs + off + qo;
                const unsigned mk = 0xffu << (8 * e);
                if (a.q[0].ptr) w[0] = (w[0] & ~mk) | ((unsigned)(uint8_t)p0[so] << (8 * e));
                if (a.q[1].ptr) w[1] = (w[1] & ~mk) | ((unsigned)(uint8_t)p1[so] << (8 * e));
            }
            if (++r == a.groups) { r = 0; ++qo; }
        }
        const size_t dst = (size_t)m * a.Cs + c;
#pragma unroll
        for (int k = 0; k < 2; ++k) if (a.q[k].ptr) *(unsigned*)(a.q[k].ptr + dst) = w[k];
    }
}

// The int32 mode of both ops.  Walks the OUTPUT's 4 KB I32T blocks (32 pixels x 32 channels), one wave per block as tap_kernel and
// upsample_i32_kernel do: lane = pixel pb * 32 + (lane & 31), channels cb * 32 + 8g + 4 (lane >> 5) + 0..3, g = 0..3 — the int32 stores of one g are
// one contiguous 1 KB transaction per wave.  Each output channel is read from the source (same pixel, its own Cs) through i32t_index at first + c
// (one 16-byte load where first is a multiple of 4) or (c % groups) * Cg + c / groups.  Guards: m < M (ragged last block: its int32 rows exist —
// Form::slack — but the int8 forms have none, and nothing is stored for them); channels >= C are written as 0 / the format's zero.
__global__ void __launch_bounds__(256) chanmap_i32_kernel(const ChanMapArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned M = (unsigned)a.M;
    const unsigned cbs = (unsigned)a.Cs >> 5;
    const unsigned nblk = ((M + 31u) >> 5) * cbs;
    const int32_t* x = (const int32_t*)a.src[0][0];
    const int first = a.off[0], cs = a.Cs_src[0];
    for (unsigned b = blockIdx.x * 4u + wave; b < nblk; b += gridDim.x * 4u) {
        const unsigned pb = b / cbs, cb = b - pb * cbs;
        const unsigned m = pb * 32u + (lane & 31u);
        if (m >= M) continue;
        const int c0 = (int)(cb * 32u + 4u * (lane >> 5));
        v4i* const o32 = a.out32 ? (v4i*)(a.out32 + (size_t)b * 1024u) + lane : nullptr;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = c0 + 8 * g;
            int y[4] = {0, 0, 0, 0};                                  // pad channels: 0
            if (a.groups == 0 && (first & 3) == 0) {
                if (c < a.C) {                                        // (first + c + 3 < Cs_src: the source's channels are padded to 32)
                    const v4i t = *(const v4i*)(x + i32t_index((int)m, first + c, cs));
                    y[0] = t.x; y[1] = t.y; y[2] = t.z; y[3] = t.w;
                }
            } else {
                int qo = (int)fast_div((unsigned)c, a.dG), r = c - qo * a.groups;      // (slice: unused)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int sc = a.groups ? r * a.Cg + qo : first + c + e;
                    if (c + e < a.C) y[e] = x[i32t_index((int)m, sc, cs)];
                    if (++r == a.groups) { r = 0; ++qo; }
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) if (c + e >= a.C) y[e] = 0;
            if (o32) { const v4i o = {y[0], y[1], y[2], y[3]}; o32[g * 64] = o; }
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (a.q[k].ptr)
                    *(unsigned*)(a.q[k].ptr + (size_t)m * a.Cs + c) =
                        requant_pack4(y[0], y[1], y[2], y[3], a.q[k]);
        }
    }
}

// 0: chanmap_i32_kernel, 1 / 2: slice_i8_kernel<true> / <false>, 3 / 4 / 5: shuffle_i8_kernel<16> / <4> / <2>, 6: shuffle_i8_general_kernel
int chanmap_inst(const ChanMapArgs& a, bool i8) {
    if (!i8) return 0;
    if (a.groups == 0) return (a.off[0] & 15) ? 2 : 1;
    if (a.groups != 2) return 6;
    const int bits = a.Cg | a.off[0] | a.off[1];
    return !(bits & 15) ? 3 : !(bits & 3) ? 4 : !(bits & 1) ? 5 : 6;
}
const char* chanmap_kernel_name(int inst) {
    static const char* const names[] = {"f8::chanmap_i32_kernel", "f8::slice_i8_kernel<true>", "f8::slice_i8_kernel<false>", "f8::shuffle_i8_kernel<16>",
                                        "f8::shuffle_i8_kernel<4>", "f8::shuffle_i8_kernel<2>", "f8::shuffle_i8_general_kernel"};
    return inst >= 0 && inst <= 6 ? names[inst] : "?";
}
hipError_t launch_chanmap(const ChanMapArgs& a, int inst, hipStream_t s) {
    if (a.M < 1 || (a.Cs & 31) || a.C < 1 || a.C > a.Cs || a.K < 1 || a.K > kMaxConcat || inst < 0 || inst > 6) return hipErrorInvalidValue;
    if (a.groups ? (a.groups < 2 || a.groups != a.K || a.Cg * a.groups != a.C) : (a.K != 1 || a.off[0] < 0)) return hipErrorInvalidValue;
    for (int i = 0; i < a.K; ++i)                                     // every entry's channels lie inside its row
        if ((a.Cs_src[i] & 31) || a.off[i] < 0 || a.off[i] + (a.groups ? a.Cg : a.C) > a.Cs_src[i]) return hipErrorInvalidValue;
    if (inst == 0 && a.K != (a.groups ? a.groups : 1)) return hipErrorInvalidValue;
    if (inst >= 3 && inst <= 5) {
        const int V = inst == 3 ? 16 : inst == 4 ? 4 : 2;
        if (a.groups != 2 || ((a.Cg | a.off[0] | a.off[1]) & (V - 1))) return hipErrorInvalidValue;
    }
    if (inst == 1 && (a.off[0] & 15)) return hipErrorInvalidValue;
    if (inst == 0) {
        const size_t nblk = (((size_t)a.M + 31) >> 5) * (size_t)(a.Cs >> 5);
        hipLaunchKernelGGL(chanmap_i32_kernel, dim3((unsigned)std::min<size_t>((nblk + 3) / 4, 2048)), dim3(256), 0, s, a);      // (as tap_kernel)
        return hipGetLastError();
    }
    const int bytes = inst == 1 ? 16 : inst == 3 ? 32 : inst == 4 ? 8 : 4;      // output bytes per lane
    const size_t work = (size_t)a.M * (a.Cs / bytes);
    const dim3 grid((unsigned)std::min<size_t>((work + 255) / 256, 8192));
    switch (inst) {
        case 1: hipLaunchKernelGGL(slice_i8_kernel<true>, grid, dim3(256), 0, s, a); break;
        case 2: hipLaunchKernelGGL(slice_i8_kernel<false>, grid, dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL(shuffle_i8_kernel<16>, grid, dim3(256), 0, s, a); break;
        case 4: hipLaunchKernelGGL(shuffle_i8_kernel<4>, grid, dim3(256), 0, s, a); break;
        case 5: hipLaunchKernelGGL(shuffle_i8_kernel<2>, grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL(shuffle_i8_general_kernel, grid, dim3(256), 0, s, a); break;
    }
    return hipGetLastError();
}

}  // namespace f8
