// f8_table.hip — the 256-entry table op (f8_net_table): any pointwise function of an 8-bit fixed-point activation — sigmoid, swish, tanh, ... — gfx950.
//
//   out[m][c] = table[u],  u = (stored byte of the source at [m][c]) ^ 0x80
// The source is read in its INT8 form, which its producer wrote in the table's index format (the planner registers the table as an int8 reader, as a
// conv).  A stored byte holds q ^ 0x80 for an unsigned format (q = 0 .. 255) and q for a signed one (-127 .. 127), so u = q or q + 128: the entries'
// own order for either sign, one v_xor_b32 per dword and no branch.
// Bandwidth kernels: 256 threads, the workgroup loads its table(s) into LDS once, one barrier, then grid-stride; arguments by value (TableArgs /
// TableMulArgs, f8_internal.h), no communication between workgroups.
//   table_i8_kernel<V, R>      int8 outputs only: a pure byte gather.  Per output form 256 BYTES composed on the host — the entry requantised to the form,
//                              storage bias folded in (compose_byte_table, f8_net.cpp) — so one ds_read_u8 per byte and no arithmetic.  Lane = V channels
//                              of one pixel (NHWC): V = 16 where the real channel count is a multiple of 16, else 4 with an end mask, as mul_i8_kernel.
//                              R copies of each table, copy r one dword further than 64 r (its banks rotate by r), lane l reads copy l % R.
//   table_i32_kernel           every launch that writes the int32 form: the 256 int32 entries in LDS (1 KB), the I32T walker of mul_i32_kernel — one wave
//                              per 4 KB block of the output — writes int32 and requantises to up to two int8 forms.
//   table_chmul_i8_kernel<V>   a table fused into the broadcast mul that reads it (the sigmoid SE gate): mul_i8_kernel<true, false, V> whose b dword is
//   table_chmul_i32_kernel     the table's SOURCE row (one per image), looked up in a byte table composed for the mul's format of b; mul_i32_kernel likewise.
// Pad channels [C, Cs) of every output are written as the format's zero — 0 in int32, 0 ^ bias_xor per byte in int8 — whatever the source's pad bytes
// hold: table[index of 0] is generally not 0 (sigmoid: 1/2).  Ragged last block: lanes with m >= M do nothing (after the barrier).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "f8_pointwise.h"      // ubyte, quant4, products

namespace f8 {

// the four bytes of w (already ^ 0x80808080) looked up in the byte table t (LDS) -> one dword
__device__ __forceinline__ unsigned lookup4(const uint8_t* t, unsigned w) {
    return (unsigned)t[ubyte(w, 0)] | ((unsigned)t[ubyte(w, 1)] << 8) | ((unsigned)t[ubyte(w, 2)] << 16) | ((unsigned)t[ubyte(w, 3)] << 24);
}
// 64 dwords of a byte table from global memory into R copies in LDS (the whole workgroup; the caller's barrier follows)
template <int R, int STRIDE>
__device__ __forceinline__ void load_byte_table(unsigned* lds, const uint8_t* bt) {
    for (unsigned i = threadIdx.x; i < (unsigned)R * 64u; i += 256u) lds[(i >> 6) * STRIDE + (i & 63u)] = ((const unsigned*)bt)[i & 63u];
}

template <int V, int R>
__global__ void __launch_bounds__(256) table_i8_kernel(const TableArgs a) {
    constexpr int D = V / 4;                                          // dwords per lane
    constexpr int STRIDE = R > 1 ? 65 : 64;                           // dwords from one copy to the next
    __shared__ unsigned lds[2][R * STRIDE];
#pragma unroll
    for (int k = 0; k < 2; ++k) if (a.q[k].ptr) load_byte_table<R, STRIDE>(lds[k], a.bt[k]);
    __syncthreads();
    const unsigned copy = (threadIdx.x % R) * STRIDE;
    const uint8_t* const t[2] = {(const uint8_t*)(lds[0] + copy), (const uint8_t*)(lds[1] + copy)};
    const unsigned vpp = (unsigned)a.Cs / V;                          // vectors per pixel
    const unsigned total = (unsigned)a.M * vpp;                       // (< 2^31: a form stays below 2 GiB)
    for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const unsigned m = fast_div(idx, a.dVpp);
        const int c = (int)(idx - m * vpp) * V;
        const size_t at = (size_t)m * a.Cs + c;
        unsigned o[2][D];
#pragma unroll
        for (int j = 0; j < D; ++j) { o[0][j] = a.q[0].bias_xor; o[1][j] = a.q[1].bias_xor; }
        if (c < a.C) {                                                // (V = 16: C is a multiple of 16, the vector is all real)
            unsigned w[D];
            if constexpr (V == 16) { const uint4 s = *(const uint4*)(a.src + at); w[0] = s.x; w[1] = s.y; w[2] = s.z; w[3] = s.w; }
            else w[0] = *(const unsigned*)(a.src + at);
            const int rem = a.C - c;                                  // V = 4: the bytes from rem on are pad
            const unsigned keep = (V == 16 || rem >= 4) ? 0xffffffffu : (1u << (8 * rem)) - 1u;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!a.q[k].ptr) continue;
#pragma unroll
                for (int j = 0; j < D; ++j) o[k][j] = (lookup4(t[k], w[j] ^ 0x80808080u) & keep) | (a.q[k].bias_xor & ~keep);
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!a.q[k].ptr) continue;
            if constexpr (V == 16) { const uint4 s = {o[k][0], o[k][1], o[k][2], o[k][3]}; *(uint4*)(a.q[k].ptr + at) = s; }
            else *(unsigned*)(a.q[k].ptr + at) = o[k][0];
        }
    }
}

__global__ void __launch_bounds__(256) table_i32_kernel(const TableArgs a) {
    __shared__ int tab[256];
    tab[threadIdx.x] = a.t32[threadIdx.x];
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned M = (unsigned)a.M;
    const unsigned cbs = (unsigned)a.Cs >> 5;
    const unsigned nblk = ((M + 31u) >> 5) * cbs;
    for (unsigned b = blockIdx.x * 4u + wave; b < nblk; b += gridDim.x * 4u) {
        const unsigned pb = b / cbs, cb = b - pb * cbs;
        const unsigned m = pb * 32u + (lane & 31u);
        if (m >= M) continue;                                         // ragged last block
        const int c0 = (int)(cb * 32u + 4u * (lane >> 5));
        v4i* const o32 = a.out32 ? (v4i*)(a.out32 + (size_t)b * 1024u) + lane : nullptr;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = c0 + 8 * g;
            const unsigned w = *(const unsigned*)(a.src + (size_t)m * a.Cs + c) ^ 0x80808080u;
            int y[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = c + e < a.C ? tab[ubyte(w, e)] : 0;
            if (o32) { const v4i o = {y[0], y[1], y[2], y[3]}; o32[g * 64] = o; }
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (a.q[k].ptr) *(unsigned*)(a.q[k].ptr + (size_t)m * a.Cs + c) = quant4(y, a.q[k]);
        }
    }
}

// operand b of four channels: the table's source dword (already ^ 0x80808080) -> the looked-up bytes in the mul's stored format of b -> values
__device__ __forceinline__ void gate4(int (&B)[4], const uint8_t* t, unsigned w, int offb) {
    const unsigned s = lookup4(t, w) ^ 0x80808080u;
#pragma unroll
    for (int e = 0; e < 4; ++e) B[e] = ubyte(s, e) - offb;
}

template <int V>
__global__ void __launch_bounds__(256) table_chmul_i8_kernel(const TableMulArgs ta) {
    const MulArgs& a = ta.m;
    constexpr int D = V / 4;
    __shared__ unsigned lds[64];
    load_byte_table<1, 64>(lds, ta.bt);
    __syncthreads();
    const uint8_t* const t = (const uint8_t*)lds;
    const unsigned vpp = (unsigned)a.Cs / V;
    const unsigned total = (unsigned)a.M * vpp;
    const int offa = a.ra.lo < 0 ? 128 : 0, offb = a.rb.lo < 0 ? 128 : 0;
    const int floor = a.relu ? 0 : INT32_MIN;
    const int8_t* const b8 = (const int8_t*)a.b;
    for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const unsigned m = fast_div(idx, a.dVpp);
        const int c = (int)(idx - m * vpp) * V;
        const size_t at = (size_t)m * a.Cs + c;
        unsigned o[2][D];
#pragma unroll
        for (int j = 0; j < D; ++j) { o[0][j] = a.q[0].bias_xor; o[1][j] = a.q[1].bias_xor; }
        if (c < a.C) {
            const unsigned n = fast_div(m, a.dHW);                    // b's row: the image
            const int8_t* const pb = b8 + (size_t)n * a.Cs + c;
            unsigned wa[D], wb[D];
            if constexpr (V == 16) {
                const uint4 x = *(const uint4*)(a.a + at); wa[0] = x.x; wa[1] = x.y; wa[2] = x.z; wa[3] = x.w;
                const uint4 g = *(const uint4*)pb; wb[0] = g.x; wb[1] = g.y; wb[2] = g.z; wb[3] = g.w;
            } else { wa[0] = *(const unsigned*)(a.a + at); wb[0] = *(const unsigned*)pb; }
#pragma unroll
            for (int j = 0; j < D; ++j) {
                int B[4], y[4];
                gate4(B, t, wb[j] ^ 0x80808080u, offb);
                products(y, wa[j] ^ 0x80808080u, offa, B, floor, a.C - (c + 4 * j));
#pragma unroll
                for (int k = 0; k < 2; ++k) if (a.q[k].ptr) o[k][j] = quant4(y, a.q[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!a.q[k].ptr) continue;
            if constexpr (V == 16) { const uint4 s = {o[k][0], o[k][1], o[k][2], o[k][3]}; *(uint4*)(a.q[k].ptr + at) = s; }
            else *(unsigned*)(a.q[k].ptr + at) = o[k][0];
        }
    }
}

__global__ void __launch_bounds__(256) table_chmul_i32_kernel(const TableMulArgs ta) {
    const MulArgs& a = ta.m;
    __shared__ unsigned lds[64];
    load_byte_table<1, 64>(lds, ta.bt);
    __syncthreads();
    const uint8_t* const t = (const uint8_t*)lds;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned M = (unsigned)a.M;
    const unsigned cbs = (unsigned)a.Cs >> 5;
    const unsigned nblk = ((M + 31u) >> 5) * cbs;
    const int offa = a.ra.lo < 0 ? 128 : 0, offb = a.rb.lo < 0 ? 128 : 0;
    const int floor = a.relu ? 0 : INT32_MIN;
    const int8_t* const b8 = (const int8_t*)a.b;
    for (unsigned b = blockIdx.x * 4u + wave; b < nblk; b += gridDim.x * 4u) {
        const unsigned pb = b / cbs, cb = b - pb * cbs;
        const unsigned m = pb * 32u + (lane & 31u);
        if (m >= M) continue;                                         // ragged last block
        const unsigned n = fast_div(m, a.dHW);
        const int c0 = (int)(cb * 32u + 4u * (lane >> 5));
        v4i* const o32 = a.out32 ? (v4i*)(a.out32 + (size_t)b * 1024u) + lane : nullptr;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = c0 + 8 * g;
            int B[4], y[4];
            gate4(B, t, *(const unsigned*)(b8 + (size_t)n * a.Cs + c) ^ 0x80808080u, offb);
            products(y, *(const unsigned*)(a.a + (size_t)m * a.Cs + c) ^ 0x80808080u, offa, B, floor, a.C - c);
            if (o32) { const v4i o = {y[0], y[1], y[2], y[3]}; o32[g * 64] = o; }
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (a.q[k].ptr) *(unsigned*)(a.q[k].ptr + (size_t)m * a.Cs + c) = quant4(y, a.q[k]);
        }
    }
}

static dim3 walker_grid(int M, int Cs) {                              // one wave per I32T block, four per workgroup (as tap_kernel)
    const size_t nblk = (((size_t)M + 31) >> 5) * (size_t)(Cs >> 5);
    return dim3((unsigned)std::min<size_t>((nblk + 3) / 4, 2048));
}

int table_inst(const TableArgs& a, bool i8) { return !i8 ? 0 : (a.C & 15) ? 2 : 1; }
const char* table_kernel_name(int inst) {
    static_assert(kTableReplicas == 1, "the symbols below name R");
    static const char* const names[] = {"f8::table_i32_kernel", "f8::table_i8_kernel<16, 1>", "f8::table_i8_kernel<4, 1>"};
    return inst >= 0 && inst <= 2 ? names[inst] : "?";
}
hipError_t launch_table(const TableArgs& a, int inst, hipStream_t s) {
    if (a.M < 1 || (a.Cs & 31) || a.C < 1 || a.C > a.Cs || inst < 0 || inst > 2 || !a.src) return hipErrorInvalidValue;
    if (inst == 0) {
        if (!a.t32) return hipErrorInvalidValue;
        hipLaunchKernelGGL(table_i32_kernel, walker_grid(a.M, a.Cs), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    const int V = inst == 1 ? 16 : 4;
    if (a.out32 || (V == 16 && (a.C & 15))) return hipErrorInvalidValue;
    for (int k = 0; k < 2; ++k) if (a.q[k].ptr && !a.bt[k]) return hipErrorInvalidValue;
    const size_t work = (size_t)a.M * (a.Cs / V);
    if (work >= (1ull << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::min<size_t>((work + 255) / 256, 8192));
    if (inst == 1) hipLaunchKernelGGL((table_i8_kernel<16, kTableReplicas>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((table_i8_kernel<4, kTableReplicas>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

int table_mul_inst(const TableMulArgs& a, bool i8) { return !i8 ? 0 : (a.m.C & 15) ? 2 : 1; }
const char* table_mul_kernel_name(int inst) {
    static const char* const names[] = {"f8::table_chmul_i32_kernel", "f8::table_chmul_i8_kernel<16>", "f8::table_chmul_i8_kernel<4>"};
    return inst >= 0 && inst <= 2 ? names[inst] : "?";
}
hipError_t launch_table_mul(const TableMulArgs& ta, int inst, hipStream_t s) {
    const MulArgs& a = ta.m;
    if (a.M < 1 || (a.Cs & 31) || a.C < 1 || a.C > a.Cs || inst < 0 || inst > 2 || !a.a || !a.b || !ta.bt) return hipErrorInvalidValue;
    if (!a.bcast || a.gate || a.HW < 1 || a.M % a.HW) return hipErrorInvalidValue;
    if (inst == 0) {
        hipLaunchKernelGGL(table_chmul_i32_kernel, walker_grid(a.M, a.Cs), dim3(256), 0, s, ta);
        return hipGetLastError();
    }
    const int V = inst == 1 ? 16 : 4;
    if (a.out32 || (V == 16 && (a.C & 15))) return hipErrorInvalidValue;
    const size_t work = (size_t)a.M * (a.Cs / V);
    if (work >= (1ull << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::min<size_t>((work + 255) / 256, 8192));
    if (inst == 1) hipLaunchKernelGGL((table_chmul_i8_kernel<16>), grid, dim3(256), 0, s, ta);
    else hipLaunchKernelGGL((table_chmul_i8_kernel<4>), grid, dim3(256), 0, s, ta);
    return hipGetLastError();
}

}  // namespace f8
