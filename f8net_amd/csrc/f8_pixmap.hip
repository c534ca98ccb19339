// f8_pixmap.hip — depth-to-space (f8_net_depth_to_space) and space-to-depth (f8_net_space_to_depth), r = block:
//   depth_to_space  [C r^2, H, W] -> [C, H r, W r]    CRD: out[c][h r + i][w r + j] = src[c r^2 + i r + j][h][w]      (torch pixel_shuffle)
//                                                     DCR: out[c][h r + i][w r + j] = src[(i r + j) C + c][h][w]      (ONNX DepthToSpace's default)
//   space_to_depth  [C, H r, W r] -> [C r^2, H, W]    the inverse of each (CRD: torch pixel_unshuffle; DCR: ONNX SpaceToDepth, TResNet's stem)
// No arithmetic: no shift, clamp or ReLU.
//
// Memory-bound gathers, grid-stride, 256 threads, no LDS, plain vector loads / stores, arguments by value, no communication between workgroups.
// The planner (plan_tensor_forms, f8_net.cpp) picks the mode per node by the rule of the other gathers:
//   i8    the source's producer already wrote the OUTPUT's int8 formats (a permutation commutes with every element-wise function), so the launch
//         moves bytes.  In NHWC the DCR orders move whole channel runs: a depth_to_space output pixel's row is bytes [(i r + j) C, + C) of its source
//         pixel, a space_to_depth output pixel's row is r^2 source rows of Csrc bytes side by side.  pixmap_run_i8_kernel where that run is a multiple
//         of 16 bytes: a lane owns one 16-byte vector of an output pixel — one 16 B load, one 16 B store per form.  The CRD orders are byte
//         transposes; pixmap_crd2_i8_kernel<S2D> for r = 2 and a multiple of 4 channels (EDSR's 4 C -> C and its inverse): a lane moves 4 channels x
//         4 sub-pixels, transposed with v_perm_b32.  Every other (op, order, r, C) pixmap_i8_general_kernel: a lane owns 4 output bytes and fetches
//         each one.  Up to two output forms per launch, each with its own source.
//   i32   the source's int32 form (I32T, i32t_index) gathered into the output's int32 form and / or up to two int8 forms through QuantOut:
//         pixmap_i32_kernel, both ops and orders.
// Pad channels [C, Cs) of the output are written as the format's zero — 0 in int32, 0 ^ bias_xor per byte in int8 — because every int8 conv reads Cs
// channels.  Only source channels below Csrc are ever read, so the source's own pad bytes reach no output.
// Indices: pixels (N P Q and N Hs Ws) are below 2^31 — launch_pixmap refuses anything else — and 32-bit; byte and int offsets are size_t.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "f8_device.h"

namespace f8 {

struct PixSrc { unsigned m; int c; };                                 // source pixel (linear, over the batch) and channel

// where channel oc of output pixel (n, oh, ow) comes from
__device__ __forceinline__ PixSrc pix_source(const PixMapArgs& a, unsigned n, unsigned oh, unsigned ow, int oc) {
    const unsigned r = (unsigned)a.r;
    unsigned h, w; int sc;
    if (!a.s2d) {
        h = fast_div(oh, a.dR); w = fast_div(ow, a.dR);
        const unsigned k = (oh - h * r) * r + (ow - w * r);           // i r + j
        sc = a.crd ? oc * (int)(r * r) + (int)k : (int)k * a.C + oc;
    } else {
        unsigned k;
        if (a.crd) { sc = (int)fast_div((unsigned)oc, a.dRR); k = (unsigned)oc - (unsigned)sc * r * r; }
        else { k = fast_div((unsigned)oc, a.dC); sc = oc - (int)k * a.Csrc; }
        const unsigned i = fast_div(k, a.dR);
        h = oh * r + i; w = ow * r + (k - i * r);
    }
    return {(n * (unsigned)a.Hs + h) * (unsigned)a.Ws + w, sc};
}

// output pixel m -> (image, row, column)
__device__ __forceinline__ void pix_split(const PixMapArgs& a, unsigned m, unsigned& n, unsigned& oh, unsigned& ow) {
    n = fast_div(m, a.dPQ);
    const unsigned pq = m - n * (unsigned)(a.P * a.Q);
    oh = fast_div(pq, a.dQ); ow = pq - oh * (unsigned)a.Q;
}

// DCR order, runs of a multiple of 16 channels (depth_to_space: C; space_to_depth: Csrc): the 16 channels from c on (c a multiple of 16) are 16
// consecutive source bytes at a 16-byte aligned address (rows are multiples of 32 bytes), all real (c < C) or all pad.
__global__ void __launch_bounds__(256) pixmap_run_i8_kernel(const PixMapArgs a) {
    const unsigned vpp = (unsigned)a.Cs >> 4;                         // vectors per output pixel
    const size_t total = (size_t)a.N * a.P * a.Q * vpp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const unsigned m = (unsigned)(idx / vpp);
        const int c = (int)(idx - (size_t)m * vpp) << 4;
        const bool real = c < a.C;
        unsigned n, oh, ow;
        pix_split(a, m, n, oh, ow);
        const PixSrc s = pix_source(a, n, oh, ow, real ? c : 0);
        const size_t so = (size_t)s.m * a.Cs_src + s.c, dst = (size_t)m * a.Cs + c;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!a.q[k].ptr) continue;
            const unsigned z = a.q[k].bias_xor;
            uint4 v = {z, z, z, z};
            if (real) v = *(const uint4*)((const int8_t*)a.src[k] + so);
            *(uint4*)(a.q[k].ptr + dst) = v;
        }
    }
}

// 4 x 4 byte transpose: t[k] byte e = d[e] byte k (v_perm_b32, as shuffle_i8_kernel interleaves)
__device__ __forceinline__ void transpose4x4(const unsigned d[4], unsigned t[4]) {
    const unsigned lo01 = __builtin_amdgcn_perm(d[1], d[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(d[1], d[0], 0x07030602u);      // {d0.b0, d1.b0, d0.b1, d1.b1}, {d0.b2, d1.b2, d0.b3, d1.b3}
    const unsigned lo23 = __builtin_amdgcn_perm(d[3], d[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(d[3], d[2], 0x07030602u);
    t[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u); t[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    t[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u); t[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
}

// CRD order, r = 2, a multiple of 4 channels (depth_to_space: C; space_to_depth: Csrc).  An item is 4 channels c .. c + 3 of the SMALL-channel side
// at one pixel (h, w) of the small map, i.e. 16 bytes 4 c .. 4 c + 15 of the deep side: byte 4 cc + k of the deep pixel is channel c + cc of
// sub-pixel k = 2 i + j.  depth_to_space: one 16 B load, transpose, one dword store to each of the four sub-pixels; space_to_depth: the other way
// round.  An item is all real (c < the small side's C) or all pad, and only the OUTPUT's pad is written (the format's zero).
template <bool S2D>
__global__ void __launch_bounds__(256) pixmap_crd2_i8_kernel(const PixMapArgs a) {
    const int Cq = S2D ? a.Cs >> 2 : a.Cs;                            // padded small-side channels the items of a pixel cover: the output's Cs / 4 or Cs
    const int Creal = S2D ? a.Csrc : a.C;
    const unsigned ipp = (unsigned)Cq >> 2;                           // items per small-map pixel
    const unsigned Hm = (unsigned)(S2D ? a.P : a.Hs), Wm = (unsigned)(S2D ? a.Q : a.Ws);      // the small map
    const size_t total = (size_t)a.N * Hm * Wm * ipp;
    const FastDiv dHW = S2D ? a.dPQ : a.dHsWs, dW = S2D ? a.dQ : a.dWs;      // / (Hm Wm), / Wm
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const unsigned m = (unsigned)(idx / ipp);                     // small-map pixel
        const int c = (int)(idx - (size_t)m * ipp) << 2;
        const bool real = c < Creal;
        const unsigned n = fast_div(m, dHW), hw = m - n * Hm * Wm, h = fast_div(hw, dW), w = hw - h * Wm;
        const unsigned big0 = (n * 2u * Hm + 2u * h) * 2u * Wm + 2u * w;      // sub-pixel (0, 0) on the big map; (i, j): + i * 2 Wm + j
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!a.q[k].ptr) continue;
            const int8_t* p = (const int8_t*)a.src[k];
            const unsigned z = a.q[k].bias_xor;
            unsigned d[4] = {z, z, z, z}, t[4] = {z, z, z, z};
            if constexpr (!S2D) {
                if (real) {
                    const uint4 x = *(const uint4*)(p + (size_t)m * a.Cs_src + 4 * c);
                    d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
                    transpose4x4(d, t);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    *(unsigned*)(a.q[k].ptr + (size_t)(big0 + (s >> 1) * 2u * Wm + (s & 1)) * a.Cs + c) = t[s];
            } else {
                if (real) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) d[s] = *(const unsigned*)(p + (size_t)(big0 + (s >> 1) * 2u * Wm + (s & 1)) * a.Cs_src + c);
                    transpose4x4(d, t);
                }
                const uint4 v = {t[0], t[1], t[2], t[3]};
                *(uint4*)(a.q[k].ptr + (size_t)m * a.Cs + 4 * c) = v;
            }
        }
    }
}

// Any op, order, block and C: a lane owns 4 output bytes c .. c + 3 of one output pixel and fetches each from its source pixel and channel.
__global__ void __launch_bounds__(256) pixmap_i8_general_kernel(const PixMapArgs a) {
    const unsigned vpp = (unsigned)a.Cs >> 2;
    const size_t total = (size_t)a.N * a.P * a.Q * vpp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const unsigned m = (unsigned)(idx / vpp);
        const int c = (int)(idx - (size_t)m * vpp) << 2;
        unsigned n, oh, ow;
        pix_split(a, m, n, oh, ow);
        unsigned w[2] = {a.q[0].bias_xor, a.q[1].bias_xor};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (c + e < a.C) {
                const PixSrc s = pix_source(a, n, oh, ow, c + e);
                const size_t so = (size_t)s.m * a.Cs_src + s.c;
                const unsigned mk = 0xffu << (8 * e);
                if (a.q[0].ptr) w[0] = (w[0] & ~mk) | ((unsigned)((const uint8_t*)a.src[0])[so] << (8 * e));
                if (a.q[1].ptr) w[1] = (w[1] & ~mk) | ((unsigned)((const uint8_t*)a.src[1])[so] << (8 * e));
            }
        }
        const size_t dst = (size_t)m * a.Cs + c;
#pragma unroll
        for (int k = 0; k < 2; ++k) if (a.q[k].ptr) *(unsigned*)(a.q[k].ptr + dst) = w[k];
    }
}

// The int32 mode of both ops and orders.  Walks the OUTPUT's 4 KB I32T blocks (32 pixels x 32 channels), one wave per block as chanmap_i32_kernel does:
// lane = pixel pb * 32 + (lane & 31), channels cb * 32 + 8g + 4 (lane >> 5) + 0..3, g = 0..3 — the int32 stores of one g are one contiguous 1 KB
// transaction per wave.  Each value is read through i32t_index at its source pixel and channel.  Guards: m < M (ragged last block: its int32 rows exist —
// Form::slack — but the int8 forms have none, and nothing is stored for them); channels >= C are written as 0 / the format's zero.
__global__ void __launch_bounds__(256) pixmap_i32_kernel(const PixMapArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned M = (unsigned)(a.N * a.P * a.Q);
    const unsigned cbs = (unsigned)a.Cs >> 5;
    const unsigned nblk = ((M + 31u) >> 5) * cbs;
    const int32_t* x = (const int32_t*)a.src[0];
    for (unsigned b = blockIdx.x * 4u + wave; b < nblk; b += gridDim.x * 4u) {
        const unsigned pb = b / cbs, cb = b - pb * cbs;
        const unsigned m = pb * 32u + (lane & 31u);
        if (m >= M) continue;
        unsigned n, oh, ow;
        pix_split(a, m, n, oh, ow);
        const int c0 = (int)(cb * 32u + 4u * (lane >> 5));
        v4i* const o32 = a.out32 ? (v4i*)(a.out32 + (size_t)b * 1024u) + lane : nullptr;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = c0 + 8 * g;
            int y[4] = {0, 0, 0, 0};                                  // pad channels: 0
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (c + e < a.C) {
                    const PixSrc s = pix_source(a, n, oh, ow, c + e);
                    y[e] = x[i32t_index((int)s.m, s.c, a.Cs_src)];
                }
            }
            if (o32) { const v4i o = {y[0], y[1], y[2], y[3]}; o32[g * 64] = o; }
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (a.q[k].ptr)
                    *(unsigned*)(a.q[k].ptr + (size_t)m * a.Cs + c) = requant_pack4(y[0], y[1], y[2], y[3], a.q[k]);
        }
    }
}

// 0: pixmap_i32_kernel, 1: pixmap_run_i8_kernel, 2: pixmap_i8_general_kernel, 3 / 4: pixmap_crd2_i8_kernel<false> / <true>.  The rule,
// on the SMALL side's channels — the output's C for depth_to_space, the source's for space_to_depth: DCR and a multiple of 16: the run mover; CRD,
// r = 2 and a multiple of 4: the transposer; everything else the general kernel.
int pixmap_inst(const PixMapArgs& a, bool i8) {
    if (!i8) return 0;
    const int c = a.s2d ? a.Csrc : a.C;
    if (!a.crd) return (c & 15) ? 2 : 1;
    return a.r == 2 && !(c & 3) ? (a.s2d ? 4 : 3) : 2;
}
const char* pixmap_kernel_name(int inst) {
    static const char* const names[] = {"f8::pixmap_i32_kernel", "f8::pixmap_run_i8_kernel", "f8::pixmap_i8_general_kernel", "f8::pixmap_crd2_i8_kernel<false>",
                                        "f8::pixmap_crd2_i8_kernel<true>"};
    return inst >= 0 && inst <= 4 ? names[inst] : "?";
}
hipError_t launch_pixmap(const PixMapArgs& a, int inst, hipStream_t s) {
    if (a.N < 1 || a.C < 1 || a.C > a.Cs || (a.Cs & 31) || a.Csrc < 1 || a.Csrc > a.Cs_src || (a.Cs_src & 31) || inst < 0 || inst > 4) return hipErrorInvalidValue;
    if (a.r < 2 || a.r > 16 || a.P < 1 || a.Q < 1 || a.Hs < 1 || a.Ws < 1 || (a.s2d & ~1) || (a.crd & ~1)) return hipErrorInvalidValue;
    const int64_t rr = (int64_t)a.r * a.r;
    // the two maps hold the same values: every source pixel and channel a lane computes then lies inside the source
    if (a.s2d ? ((int64_t)a.Csrc * rr != a.C || (int64_t)a.P * a.r != a.Hs || (int64_t)a.Q * a.r != a.Ws)
              : ((int64_t)a.C * rr != a.Csrc || (int64_t)a.Hs * a.r != a.P || (int64_t)a.Ws * a.r != a.Q)) return hipErrorInvalidValue;
    const int64_t M = (int64_t)a.N * a.P * a.Q, Ms = (int64_t)a.N * a.Hs * a.Ws;
    if (M >= (int64_t(1) << 31) || Ms >= (int64_t(1) << 31)) return hipErrorInvalidValue;      // 32-bit pixel indices
    if (inst == 1 && (a.crd || ((a.s2d ? a.Csrc : a.C) & 15))) return hipErrorInvalidValue;
    if (inst >= 3 && (!a.crd || a.r != 2 || a.s2d != (inst == 4) || ((a.s2d ? a.Csrc : a.C) & 3))) return hipErrorInvalidValue;
    for (int k = 0; inst != 0 && k < 2; ++k) if (a.q[k].ptr && !a.src[k]) return hipErrorInvalidValue;      // bytes mode: one source per output form
    if (inst == 0) {
        if (!a.src[0]) return hipErrorInvalidValue;
        const size_t nblk = (((size_t)M + 31) >> 5) * (size_t)(a.Cs >> 5);
        if (nblk >= (size_t(1) << 32)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(pixmap_i32_kernel, dim3((unsigned)std::min<size_t>((nblk + 3) / 4, 2048)), dim3(256), 0, s, a);      // (as chanmap_i32_kernel)
        return hipGetLastError();
    }
    // items: a 16-byte vector (1) or a dword (2) of an output pixel; 4 channels of a small-map pixel (3: the source's pixels, 4: the output's)
    const size_t work = inst == 1 ? (size_t)M * (a.Cs >> 4) : inst == 2 ? (size_t)M * (a.Cs >> 2) : inst == 3 ? (size_t)Ms * (a.Cs >> 2) : (size_t)M * (a.Cs >> 4);
    const dim3 grid((unsigned)std::min<size_t>((work + 255) / 256, 8192));
    switch (inst) {
        case 1: hipLaunchKernelGGL(pixmap_run_i8_kernel, grid, dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL(pixmap_crd2_i8_kernel<false>, grid, dim3(256), 0, s, a); break;
        case 4: hipLaunchKernelGGL(pixmap_crd2_i8_kernel<true>, grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL(pixmap_i8_general_kernel, grid, dim3(256), 0, s, a); break;
    }
    return hipGetLastError();
}

}  // namespace f8
