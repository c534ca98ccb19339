// f8_mul.hip — fixed-point multiply of two activations (f8_net_mul) and the hard gate relu6(x + 3) (f8_net_hard_gate), gfx950.
//
//   out[m][c] = A[m][c] * B[m][c]            element-wise ("mul"), or
//   out[m][c] = A[m][c] * B[m / HW][c]       b is [C, 1, 1]: a per-image channel gate ("chmul", the scale of a squeeze-and-excitation block)
// A and B are 8-bit fixed-point values (0 .. 255 or -127 .. 127), so |out| <= 255 * 255: nothing wraps, and the optional ReLU is a max.
//   gate(x)   = clamp(x, -lim, lim) + lim,  lim = 3 * 2^fl: the clamp first, so no int32 input overflows and the result lies in 0 .. 6 * 2^28.
//
// Bandwidth kernels: grid-stride, 256 threads, no LDS, plain vector loads / stores, arguments by value (MulArgs, f8_internal.h), no communication.
// The operands are read in their INT8 forms, which their producers wrote in the mul's formats (the planner registers the mul as an int8 reader, as a
// conv).  A stored byte s holds x ^ 0x80 for an unsigned format and x for a signed one; so with u = the byte of (s ^ 0x80): x = u (unsigned) or
// x = u - 128 (signed) — one v_xor_b32 per dword, one v_bfe_u32 and one subtraction of a wave-uniform 0 / 128 per value, no branch.
// With a hard gate FUSED in (MulArgs::gate) operand b is the gate's SOURCE in int32 (I32T): the launch clamps, offsets and requantises it to b's format
// (requant1: the integer round-half-even path of f8_device.h) and the gate tensor never exists.
//   mul_i8_kernel<BCAST, GATE, V>   int8 outputs only.  Lane = V channels of one pixel (NHWC): V = 16 where the real channel count is a multiple of 16
//                                   (a vector is all real or all pad), else V = 4 with an end mask.  GATE only with BCAST: the gate row is one I32T
//                                   pixel per image, N x C values.  A wave spans image boundaries (49 pixels an image against 64 lanes): the image index is
//                                   per lane, m / HW by FastDiv.
//   mul_i32_kernel<BCAST, GATE>     every launch that writes the int32 form, and the fused element-wise product (hard-swish), whose gate source is a full
//                                   I32T map: the I32T walker of tap_kernel / chanmap_i32_kernel — one wave per 4 KB block of the output (32 pixels x 32
//                                   channels), lane = pixel (lane & 31), channels 8g + 4 (lane >> 5) + 0..3, g = 0..3: the int32 loads / stores of one g
//                                   are one contiguous 1 KB transaction per wave.
//   hgate_kernel                    the stand-alone hard gate: the same walker over the source's blocks.
// Pad channels [C, Cs) of every output are written as the format's zero — 0 in int32, 0 ^ bias_xor per byte in int8 — whatever the
// operands' pad bytes hold: the product of a pad channel is replaced by 0 before the requantisation.  Ragged last block: lanes with m >= M do nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "f8_pointwise.h"      // ubyte, quant4, products

namespace f8 {

__device__ __forceinline__ int hard_gate(int x, int lim) { return med3i(x, -lim, lim) + lim; }

template <bool BCAST, bool GATE, int V>
__global__ void __launch_bounds__(256) mul_i8_kernel(const MulArgs a) {
    static_assert(!GATE || BCAST, "an element-wise fused gate runs on mul_i32_kernel");
    constexpr int D = V / 4;                                          // dwords per lane
    const unsigned vpp = (unsigned)a.Cs / V;                          // vectors per pixel
    const unsigned total = (unsigned)a.M * vpp;                       // (< 2^31: a form stays below 2 GiB)
    const int offa = a.ra.lo < 0 ? 128 : 0, offb = a.rb.lo < 0 ? 128 : 0;
    const int floor = a.relu ? 0 : INT32_MIN;
    const int8_t* const b8 = (const int8_t*)a.b; const int32_t* const xg = (const int32_t*)a.b;
    for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const unsigned m = fast_div(idx, a.dVpp);
        const int c = (int)(idx - m * vpp) * V;
        const size_t at = (size_t)m * a.Cs + c;
        unsigned o[2][D];
#pragma unroll
        for (int j = 0; j < D; ++j) { o[0][j] = a.q[0].bias_xor; o[1][j] = a.q[1].bias_xor; }
        if (c < a.C) {                                                // (V = 16: C is a multiple of 16, the vector is all real)
            const unsigned n = BCAST ? fast_div(m, a.dHW) : m;        // b's row: the image, or the pixel
            unsigned wa[D], wb[D];
            if constexpr (V == 16) { const uint4 t = *(const uint4*)(a.a + at); wa[0] = t.x; wa[1] = t.y; wa[2] = t.z; wa[3] = t.w; }
            else wa[0] = *(const unsigned*)(a.a + at);
            if constexpr (!GATE) {
                const int8_t* const pb = b8 + (size_t)n * a.Cs + c;
                if constexpr (V == 16) { const uint4 t = *(const uint4*)pb; wb[0] = t.x; wb[1] = t.y; wb[2] = t.z; wb[3] = t.w; }
                else wb[0] = *(const unsigned*)pb;
            }
#pragma unroll
            for (int j = 0; j < D; ++j) {
                int B[4], y[4];
                if constexpr (GATE) {
                    const v4i x = *(const v4i*)(xg + i32t_index((int)n, c + 4 * j, a.Cs));
#pragma unroll
                    for (int e = 0; e < 4; ++e) B[e] = requant1(hard_gate(x[e], a.lim), a.rb.n, a.rb.lo, a.rb.hi);
                } else {
                    const unsigned w = wb[j] ^ 0x80808080u;
#pragma unroll
                    for (int e = 0; e < 4; ++e) B[e] = ubyte(w, e) - offb;
                }
                products(y, wa[j] ^ 0x80808080u, offa, B, floor, a.C - (c + 4 * j));
#pragma unroll
                for (int k = 0; k < 2; ++k) if (a.q[k].ptr) o[k][j] = quant4(y, a.q[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!a.q[k].ptr) continue;
            if constexpr (V == 16) { const uint4 t = {o[k][0], o[k][1], o[k][2], o[k][3]}; *(uint4*)(a.q[k].ptr + at) = t; }
            else *(unsigned*)(a.q[k].ptr + at) = o[k][0];
        }
    }
}

template <bool BCAST, bool GATE>
__global__ void __launch_bounds__(256) mul_i32_kernel(const MulArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned M = (unsigned)a.M;
    const unsigned cbs = (unsigned)a.Cs >> 5;
    const unsigned nblk = ((M + 31u) >> 5) * cbs;
    const int offa = a.ra.lo < 0 ? 128 : 0, offb = a.rb.lo < 0 ? 128 : 0;
    const int floor = a.relu ? 0 : INT32_MIN;
    const int8_t* const b8 = (const int8_t*)a.b; const int32_t* const xg = (const int32_t*)a.b;
    for (unsigned b = blockIdx.x * 4u + wave; b < nblk; b += gridDim.x * 4u) {
        const unsigned pb = b / cbs, cb = b - pb * cbs;
        const unsigned m = pb * 32u + (lane & 31u);
        if (m >= M) continue;                                         // ragged last block
        const unsigned n = BCAST ? fast_div(m, a.dHW) : m;
        const int c0 = (int)(cb * 32u + 4u * (lane >> 5));
        v4i* const o32 = a.out32 ? (v4i*)(a.out32 + (size_t)b * 1024u) + lane : nullptr;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = c0 + 8 * g;
            int B[4], y[4];
            if constexpr (GATE) {
                // element-wise: the gate's source has the output's shape, so its block and this lane's place in it are the output's
                const v4i x = BCAST ? *(const v4i*)(xg + i32t_index((int)n, c, a.Cs)) : ((const v4i*)(xg + (size_t)b * 1024u))[g * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) B[e] = requant1(hard_gate(x[e], a.lim), a.rb.n, a.rb.lo, a.rb.hi);
            } else {
                const unsigned w = *(const unsigned*)(b8 + (size_t)n * a.Cs + c) ^ 0x80808080u;
#pragma unroll
                for (int e = 0; e < 4; ++e) B[e] = ubyte(w, e) - offb;
            }
            products(y, *(const unsigned*)(a.a + (size_t)m * a.Cs + c) ^ 0x80808080u, offa, B, floor, a.C - c);
            if (o32) { const v4i o = {y[0], y[1], y[2], y[3]}; o32[g * 64] = o; }
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (a.q[k].ptr) *(unsigned*)(a.q[k].ptr + (size_t)m * a.Cs + c) = quant4(y, a.q[k]);
        }
    }
}

__global__ void __launch_bounds__(256) hgate_kernel(const MulArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned M = (unsigned)a.M;
    const unsigned cbs = (unsigned)a.Cs >> 5;
    const unsigned nblk = ((M + 31u) >> 5) * cbs;
    const int32_t* const xg = (const int32_t*)a.b;
    for (unsigned b = blockIdx.x * 4u + wave; b < nblk; b += gridDim.x * 4u) {
        const unsigned pb = b / cbs, cb = b - pb * cbs;
        const unsigned m = pb * 32u + (lane & 31u);
        if (m >= M) continue;
        const int c0 = (int)(cb * 32u + 4u * (lane >> 5));
        const v4i* const in = (const v4i*)(xg + (size_t)b * 1024u) + lane;
        v4i* const o32 = a.out32 ? (v4i*)(a.out32 + (size_t)b * 1024u) + lane : nullptr;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = c0 + 8 * g;
            const v4i x = in[g * 64];
            int y[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = c + e < a.C ? hard_gate(x[e], a.lim) : 0;      // (a pad channel of the source holds 0, whose gate is lim)
            if (o32) { const v4i o = {y[0], y[1], y[2], y[3]}; o32[g * 64] = o; }
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (a.q[k].ptr) *(unsigned*)(a.q[k].ptr + (size_t)m * a.Cs + c) = quant4(y, a.q[k]);
        }
    }
}

// mode 0: the stand-alone hard gate; 1: a mul that writes the int32 form; 2: a mul with int8 outputs only
int mul_inst(const MulArgs& a, int mode) {
    if (mode == 0) return 0;
    if (mode == 1 || (a.gate && !a.bcast)) return 1 + 2 * (a.bcast != 0) + (a.gate != 0);
    return 5 + (a.bcast ? 2 + 2 * (a.gate != 0) : 0) + ((a.C & 15) ? 1 : 0);
}
int mul_vector_bytes(int inst) { return inst < 5 ? 4 : ((inst - 5) & 1) ? 4 : 16; }
const char* mul_kernel_name(int inst) {
    static const char* const names[] = {"f8::hgate_kernel", "f8::mul_i32_kernel<false, false>", "f8::mul_i32_kernel<false, true>", "f8::mul_i32_kernel<true, false>",
                                        "f8::mul_i32_kernel<true, true>", "f8::mul_i8_kernel<false, false, 16>", "f8::mul_i8_kernel<false, false, 4>",
                                        "f8::mul_i8_kernel<true, false, 16>", "f8::mul_i8_kernel<true, false, 4>", "f8::mul_i8_kernel<true, true, 16>",
                                        "f8::mul_i8_kernel<true, true, 4>"};
    return inst >= 0 && inst <= 10 ? names[inst] : "?";
}
hipError_t launch_mul(const MulArgs& a, int inst, hipStream_t s) {
    if (a.M < 1 || (a.Cs & 31) || a.C < 1 || a.C > a.Cs || inst < 0 || inst > 10 || !a.b) return hipErrorInvalidValue;
    if (inst == 0 || a.gate) { if (a.lim < 3 || a.lim > (3 << 28)) return hipErrorInvalidValue; }
    if (inst > 0) {
        if (!a.a || (a.bcast && (a.HW < 1 || a.M % a.HW))) return hipErrorInvalidValue;
        const int bc = inst < 5 ? (inst - 1) >> 1 : inst >= 7, gt = inst < 5 ? (inst - 1) & 1 : inst >= 9;      // what the instance was compiled for
        if (bc != (a.bcast != 0) || gt != (a.gate != 0)) return hipErrorInvalidValue;
        if (inst >= 5 && (a.out32 || (mul_vector_bytes(inst) == 16 && (a.C & 15)))) return hipErrorInvalidValue;
    }
    if (inst < 5) {
        const size_t nblk = (((size_t)a.M + 31) >> 5) * (size_t)(a.Cs >> 5);
        const dim3 grid((unsigned)std::min<size_t>((nblk + 3) / 4, 2048));                                           // (as tap_kernel)
        switch (inst) {
            case 0: hipLaunchKernelGGL(hgate_kernel, grid, dim3(256), 0, s, a); break;
            case 1: hipLaunchKernelGGL((mul_i32_kernel<false, false>), grid, dim3(256), 0, s, a); break;
            case 2: hipLaunchKernelGGL((mul_i32_kernel<false, true>), grid, dim3(256), 0, s, a); break;
            case 3: hipLaunchKernelGGL((mul_i32_kernel<true, false>), grid, dim3(256), 0, s, a); break;
            default: hipLaunchKernelGGL((mul_i32_kernel<true, true>), grid, dim3(256), 0, s, a); break;
        }
        return hipGetLastError();
    }
    const size_t work = (size_t)a.M * (a.Cs / mul_vector_bytes(inst));
    if (work >= (1ull << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::min<size_t>((work + 255) / 256, 8192));
    switch (inst) {
        case 5: hipLaunchKernelGGL((mul_i8_kernel<false, false, 16>), grid, dim3(256), 0, s, a); break;
        case 6: hipLaunchKernelGGL((mul_i8_kernel<false, false, 4>), grid, dim3(256), 0, s, a); break;
        case 7: hipLaunchKernelGGL((mul_i8_kernel<true, false, 16>), grid, dim3(256), 0, s, a); break;
        case 8: hipLaunchKernelGGL((mul_i8_kernel<true, false, 4>), grid, dim3(256), 0, s, a); break;
        case 9: hipLaunchKernelGGL((mul_i8_kernel<true, true, 16>), grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((mul_i8_kernel<true, true, 4>), grid, dim3(256), 0, s, a); break;
    }
    return hipGetLastError();
}

}  // namespace f8
