// f8_se.hip — the squeeze path of a squeeze-and-excitation branch in ONE launch (option fuse_se, gfx950): fc2(fc1(avgpool_sum(x))).
//
// The three launches it replaces are latency-bound and ran on kernels written for other work: avgpool_kernel (eight lanes per (image, 4 channels)) and
// two 64 x 64 conv_igemm_kernel tile grids over "pixels" = images, two or three workgroups each at batch 128.  Here ONE workgroup of 512 threads owns
// ONE image (grid = the images of the launch's part) and walks three phases that share LDS; nothing but fc2's result goes to memory.
//
//   1. pool   the image's pixels are rows m in [n HW, (n + 1) HW) of the source's int32 form (I32T, i32t_index: blocks of 32 pixels x 32 channels,
//             4 KB; a wave instruction that loads 16 bytes per lane reads ONE contiguous KB = 32 pixels x 8 channels).  The blocks an image straddles
//             are shared with its neighbours: lanes are masked by m, not by block, and a masked lane loads nothing.  A wave owns a unit = (channel
//             block, slice of the image's pixel blocks), units round robin over the waves; it keeps 16 unsigned accumulators per lane (4 groups x 4
//             channels) over its pixel blocks, two blocks = eight 16-byte loads in flight, reduces ONCE over the 32 pixel lanes (DPP row reduction,
//             one cross-row step) and adds the 32 sums into psum[Cs] in LDS (ds_add_u32: the slices of one channel block meet there).  Adds
//             modulo 2^32 commute: any order gives f8_net_avgpool_sum's wrapping sum.
//   2. fc1    q1 = requant(psum -> fc1's input format), four channels per lane, as BYTES in the library's storage (unsigned formats biased by 0x80,
//             the bias table carries + 128 sum(w): pack_se_weights, f8_net.cpp); acc = sum w q1 + bias [ReLU], int32 in LDS.
//   3. fc2    q2 = requant(fc1 -> fc2's input format), the same multiply, and the epilogue of a conv launch: the int32 form at i32t_index(n, c, Cs)
//             and / or up to two int8 forms (requant_pack4), four channels per lane.  Pad channels [cout, Cs) are written as 0 / the format's zero.
//
// The two layers have opposite shapes — the squeeze has K large and few outputs, the excite K small and many — so the kernel carries TWO v_dot4
// mappings and the host picks one per layer (se_klanes: cout <= cin takes the first):
//   K over lanes        weights [coutP][Kp] int8 rows, Kp a multiple of 16.  Lane l owns bytes [16 l, 16 l + 16) of every 1024-byte pass of K and
//                       keeps its q fragments in registers for the whole layer; waves take output rows round robin, FOUR rows' weights requested
//                       before the first multiply (16-byte loads straight to registers, no LDS staging: fc_dense_kernel's approach); four v_dot4 per
//                       lane, row and pass, then one cross-lane reduction per output (DPP row reduction, two cross-row steps).
//   outputs over lanes  weights K-major [Kp / 4][coutP] dwords: consecutive lanes read consecutive dwords.  Lane = output channel (passes of 512), q is
//                       a broadcast LDS dword per step of 4 K, no cross-lane reduction.
// K and output padding is ZERO WEIGHTS in both images, so a pad byte of q never matters; it is the format's zero all the same.
//
// No matrix instructions: a workgroup has ONE image, so a 32 x 32 x 32 MFMA step would be 31 / 32 = 97 % padding, and the arithmetic of both layers
// (at most 0.5 M multiply-adds per image at 960 / 240) is far below what the launch spends fetching the map.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "f8_device.h"

namespace f8 {

// sum over the 16 lanes of each DPP row: two quad permutes, row_half_mirror, row_mirror (every lane of the row ends with the row's sum)
__device__ __forceinline__ unsigned se_row_sum(unsigned v) {
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1 /* quad_perm [1, 0, 3, 2] */, 0xf, 0xf, true);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E /* quad_perm [2, 3, 0, 1] */, 0xf, 0xf, true);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141 /* row_half_mirror */, 0xf, 0xf, true);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140 /* row_mirror */, 0xf, 0xf, true);
    return v;
}
__device__ __forceinline__ unsigned se_half_sum(unsigned v) {      // over the 32 lanes of each half of the wave
    v = se_row_sum(v);
    return v + (unsigned)__shfl_xor((int)v, 16);
}
__device__ __forceinline__ unsigned se_wave_sum(unsigned v) {      // over all 64 lanes
    v = se_half_sum(v);
    return v + (unsigned)__shfl_xor((int)v, 32);
}

// q[i] = four values of src (int32 in LDS; beyond `real`: 0) in the format r, i < kp4: the int8 operand of a layer, its K padding the format's zero
__device__ __forceinline__ void se_quantize(const int* src, int real, int kp4, const Requant& r, unsigned* q, int tid) {
    for (int i = tid; i < kp4; i += 512) {
        int v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = 4 * i + e < real ? src[4 * i + e] : 0;
        q[i] = requant_pack4(v[0], v[1], v[2], v[3], r);
    }
}

__device__ __forceinline__ int se_finish(const SELayer& L, int acc, int o) {
    const int v = (int)((unsigned)acc + (unsigned)L.bias[o]);
    return L.relu ? max(v, 0) : v;
}

// K over lanes; MAXP: the passes of 1024 K bytes the layer can have (fc1: 4, fc2: 1)
template <int MAXP>
__device__ __forceinline__ void se_fc_klanes(const SELayer& L, const unsigned* q, int* dst, int wave, int lane) {
    v4i qf[MAXP];
    const v4i zero = {0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
        const int off = 1024 * p + 16 * lane;
        qf[p] = off < L.Kp ? *(const v4i*)((const char*)q + off) : zero;
    }
    for (int r0 = wave; r0 < L.cout; r0 += 32) {              // rows r0, r0 + 8, r0 + 16, r0 + 24: all their weights requested first
        v4i wf[4][MAXP];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int p = 0; p < MAXP; ++p) {
                const int r = r0 + 8 * u, off = 1024 * p + 16 * lane;
                wf[u][p] = (r < L.cout && off < L.Kp) ? *(const v4i*)(L.w + (size_t)r * L.Kp + off) : zero;
            }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int acc = 0;
#pragma unroll
            for (int p = 0; p < MAXP; ++p)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_sdot4(wf[u][p][e], qf[p][e], acc, false);
            acc = (int)se_wave_sum((unsigned)acc);
            const int r = r0 + 8 * u;
            if (lane == 0 && r < L.cout) dst[r] = se_finish(L, acc, r);
        }
    }
}

// outputs over lanes
__device__ __forceinline__ void se_fc_olanes(const SELayer& L, const unsigned* q, int* dst, int tid) {
    const int k4n = L.Kp >> 2;                                 // a multiple of 4
    for (int o = tid; o < L.coutP; o += 512) {
        const int* const wp = (const int*)L.w + o;
        int acc = 0;
        for (int k = 0; k < k4n; k += 4) {
            int w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = wp[(size_t)(k + j) * L.coutP];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_sdot4(w[j], (int)q[k + j], acc, false);
        }
        if (o < L.cout) dst[o] = se_finish(L, acc, o);
    }
}

template <bool K1, bool K2>
__global__ void __launch_bounds__(512) se_kernel(const SEArgs a) {
    __shared__ unsigned psum[kSeMaxC];                         // the pooled sums
    __shared__ int h[kSeMaxMid];                               // fc1's result
    __shared__ int y[kSeMaxC];                                 // fc2's result
    __shared__ __attribute__((aligned(16))) unsigned q1[kSeMaxC / 4];
    __shared__ __attribute__((aligned(16))) unsigned q2[kSeMaxMid / 4];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.x;
    const int Cs = a.Cs, ncb = Cs >> 5;
    for (int i = tid; i < Cs; i += 512) psum[i] = 0u;
    __syncthreads();
    // ---- 1. pool
    {
        const int m0 = n * a.HW, m1 = m0 + a.HW;                // this image's pixels
        const int pb0 = m0 >> 5, pbe = ((m1 - 1) >> 5) + 1;     // ... and the pixel blocks they lie in
        const int S = min(pbe - pb0, max(1, (8 + ncb - 1) / ncb));      // slices of the pixel blocks: at least eight units where the image has the blocks
        for (int u = wave; u < ncb * S; u += 8) {
            const int cb = u % ncb, s = u / ncb;
            const int32_t* const base = a.x + (size_t)cb * 1024u + (size_t)(lane << 2);      // i32t_index: + block row * ncb * 1024 + g * 256
            unsigned acc[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g][0] = acc[g][1] = acc[g][2] = acc[g][3] = 0u;
            for (int pb = pb0 + s; pb < pbe; pb += 2 * S) {
                const int pb2 = pb + S;
                const int ma = pb * 32 + l31, mb = pb2 * 32 + l31;
                const bool oka = ma >= m0 && ma < m1, okb = pb2 < pbe && mb >= m0 && mb < m1;
                const v4i zero = {0, 0, 0, 0};
                v4i va[4], vb[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) va[g] = oka ? *(const v4i*)(base + (size_t)pb * ncb * 1024u + g * 256) : zero;
#pragma unroll
                for (int g = 0; g < 4; ++g) vb[g] = okb ? *(const v4i*)(base + (size_t)pb2 * ncb * 1024u + g * 256) : zero;
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[g][e] += (unsigned)va[g][e] + (unsigned)vb[g][e];
            }
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned t = se_half_sum(acc[g][e]);
                    if (l31 == 0) atomicAdd(&psum[cb * 32 + 8 * g + 4 * lh + e], t);
                }
        }
    }
    __syncthreads();
    // ---- 2. fc1
    se_quantize((const int*)psum, a.C, a.l1.Kp >> 2, a.l1.rq, q1, tid);
    __syncthreads();
    if constexpr (K1) se_fc_klanes<kSeMaxC / 1024>(a.l1, q1, h, wave, lane);
    else se_fc_olanes(a.l1, q1, h, tid);
    __syncthreads();
    // ---- 3. fc2
    se_quantize(h, a.l1.cout, a.l2.Kp >> 2, a.l2.rq, q2, tid);
    __syncthreads();
    if constexpr (K2) se_fc_klanes<kSeMaxMid / 1024>(a.l2, q2, y, wave, lane);
    else se_fc_olanes(a.l2, q2, y, tid);
    __syncthreads();
    const int Co = a.l2.coutP;                                 // the result's padded channels (a multiple of 32)
    for (int c = 4 * tid; c < Co; c += 2048) {
        int v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c + e < a.l2.cout ? y[c + e] : 0;
        if (a.out32) { const v4i o = {v[0], v[1], v[2], v[3]}; *(v4i*)(a.out32 + i32t_index(n, c, Co)) = o; }
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (a.q[k].ptr) *(unsigned*)(a.q[k].ptr + (size_t)n * Co + c) = requant_pack4(v[0], v[1], v[2], v[3], a.q[k]);
    }
}

// THE mapping rule: a layer with no more outputs than inputs reduces K over the lanes, any other spreads its outputs over them
bool se_klanes(int cin, int cout) { return cout <= cin; }
int se_inst(const SEArgs& a) { return 2 * (a.l1.klanes != 0) + (a.l2.klanes != 0); }
const char* se_kernel_name(int inst) {
    static const char* const names[] = {"f8::se_kernel<false, false>", "f8::se_kernel<false, true>", "f8::se_kernel<true, false>", "f8::se_kernel<true, true>"};
    return inst >= 0 && inst <= 3 ? names[inst] : "?";
}

static bool se_layer_ok(const SELayer& L, int K, int max_out) {
    return L.w && L.bias && L.K == K && L.Kp == (K + 15) / 16 * 16 && L.cout >= 1 && L.cout <= max_out && L.coutP == (L.cout + 31) / 32 * 32;
}

hipError_t launch_se(const SEArgs& a, int inst, hipStream_t s) {
    if (!a.x || a.N < 1 || a.HW < 1 || a.C < 1 || a.C > a.Cs || (a.Cs & 31) || a.Cs > kSeMaxC || inst != se_inst(a)) return hipErrorInvalidValue;
    if (!se_layer_ok(a.l1, a.C, kSeMaxMid) || !se_layer_ok(a.l2, a.l1.cout, kSeMaxC)) return hipErrorInvalidValue;
    if ((long long)a.N * a.HW >= (1ll << 26)) return hipErrorInvalidValue;      // pixel indices stay far inside 32 bits
    const dim3 grid((unsigned)a.N), block(512);
    switch (inst) {
        case 0: hipLaunchKernelGGL((se_kernel<false, false>), grid, block, 0, s, a); break;
        case 1: hipLaunchKernelGGL((se_kernel<false, true>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((se_kernel<true, false>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((se_kernel<true, true>), grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}

}  // namespace f8
