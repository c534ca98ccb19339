// f8_upsample.hip — upsampling (f8_net_upsample): [C, Hs, Ws] -> [C, Hs * sh, Ws * sw], nearest neighbour or bilinear (half-pixel centres).
//
// Memory-bound: the output is sh * sw times the input.  Grid-stride, no LDS, plain vector loads / stores.  The planner (plan_tensor_forms, f8_net.cpp)
// picks the mode per node:
//   upsample_nearest_i8    the source already exists in the OUTPUT's int8 format (same fraclen, same shift), so the launch replicates bytes:
//                          upsample_i8_kernel.  Up to two output forms per launch, each with its own source pointer.
//   upsample_nearest_i32   the source's int32 form (I32T, i32t_index) replicated into the output's int32 form and / or up to two int8 forms.
//   upsample_bilinear_i32  out = (wlH x[i0] + wuH x[i1]) over H of the same over W, the integer weights of include/f8net.h: for output index
//                          o = s i + j, j < s / 2: (s - 2j - 1) x[max(i - 1, 0)] + (s + 2j + 1) x[i]; else (3s - 2j - 1) x[i] + (2j + 1 - s) x[min(i + 1, n - 1)].
//                          Both axes: the exact interpolated value times 4 s^2, in wrapping 32-bit arithmetic, no rounding, no clamp.
// Pad channels [C, Cs): the i8 mode copies the source's (its producer wrote the format's zero); the i32 mode writes 0 / the format's zero.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "f8_device.h"

namespace f8 {

// A work item is (image, output row, source column, 16-byte channel vector): one 16-byte load of the source vector per form, sw 16-byte stores to
// consecutive output pixels.  One item -> coordinates decomposition per item (three magic divisions), none per store.  Source rows are re-read sh
// times, from cache.  A [C, 1, 1] source (the ASPP broadcast) still has N * P * Cs / 16 items.
__global__ void __launch_bounds__(256) upsample_i8_kernel(const UpsampleArgs a) {
    const unsigned vpp = (unsigned)a.Cs >> 4;                        // vectors per pixel
    const unsigned total = (unsigned)a.N * (unsigned)a.P * (unsigned)a.Ws * vpp;      // <= output bytes / 16 < 2^27 (f8_net_finalize: a form stays below 2 GiB)
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const unsigned r = fast_div(idx, a.dVpp), v = idx - r * vpp;
        const unsigned row = fast_div(r, a.dWs), j = r - row * (unsigned)a.Ws;      // row = n * P + p
        const unsigned srow = fast_div(row, a.dSh);                                  // n * Hs + p / sh (P = Hs * sh)
        const size_t so = ((size_t)srow * a.Ws + j) * a.Cs + v * 16u;
        const size_t dst = ((size_t)row * a.Q + (size_t)j * a.sw) * a.Cs + v * 16u;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!a.q[k].ptr) continue;
            const uint4 x = *(const uint4*)((const int8_t*)a.src[k] + so);
            int8_t* o = a.q[k].ptr + dst;
            for (int e = 0; e < a.sw; ++e) *(uint4*)(o + (size_t)e * a.Cs) = x;
        }
    }
}

// Walks the OUTPUT's 4 KB I32T blocks (32 pixels x 32 channels), one wave per block as tap_kernel does: lane = output pixel pb * 32 + (lane & 31),
// channels cb * 32 + 8g + 4 (lane >> 5) + 0..3, g = 0..3 — the int32 stores of one g are one contiguous 1 KB transaction per wave.  m -> (n, p, q)
// once per lane and block; the source pixel (nearest) or the four clamped neighbours (bilinear) come through i32t_index, 16 bytes each, shared by
// neighbouring lanes through the cache.  Guards: m < M (ragged last block: its int32 rows exist — Form::slack — but the int8 forms have none, and
// nothing is stored for them), a block may straddle rows and images (n, p, q are per lane), channels >= C are written as 0 / the format's zero.
template <bool BILINEAR>
__global__ void __launch_bounds__(256) upsample_i32_kernel(const UpsampleArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned PQ = (unsigned)a.P * (unsigned)a.Q;
    const unsigned M = (unsigned)a.N * PQ;
    const unsigned cbs = (unsigned)a.Cs >> 5;
    const unsigned nblk = ((M + 31u) >> 5) * cbs;
    const int32_t* x = (const int32_t*)a.src[0];
    for (unsigned b = blockIdx.x * 4u + wave; b < nblk; b += gridDim.x * 4u) {
        const unsigned pb = b / cbs, cb = b - pb * cbs;
        const unsigned m = pb * 32u + (lane & 31u);
        if (m >= M) continue;
        const unsigned n = fast_div(m, a.dPQ), pq = m - n * PQ;
        const unsigned p = fast_div(pq, a.dQ), q = pq - p * (unsigned)a.Q;
        const int c0 = (int)(cb * 32u + 4u * (lane >> 5));
        const int base = (int)n * a.Hs;                               // first source row of the image
        int m00, m01 = 0, m10 = 0, m11 = 0;                           // source pixels (rows i0 / i1, columns j0 / j1)
        unsigned w00 = 1, w01 = 0, w10 = 0, w11 = 0;
        if constexpr (BILINEAR) {
            const int s = 1 << a.k, h = s >> 1;
            const int i = (int)(p >> a.k), jp = (int)(p & (unsigned)(s - 1)), ii = (int)(q >> a.k), jq = (int)(q & (unsigned)(s - 1));
            const bool up = jp < h, left = jq < h;
            const int i0 = up ? max(i - 1, 0) : i, i1 = up ? i : min(i + 1, a.Hs - 1);
            const int j0 = left ? max(ii - 1, 0) : ii, j1 = left ? ii : min(ii + 1, a.Ws - 1);
            const unsigned wl = (unsigned)(up ? s - 2 * jp - 1 : 3 * s - 2 * jp - 1), wu = (unsigned)(up ? s + 2 * jp + 1 : 2 * jp + 1 - s);
            const unsigned vl = (unsigned)(left ? s - 2 * jq - 1 : 3 * s - 2 * jq - 1), vu = (unsigned)(left ? s + 2 * jq + 1 : 2 * jq + 1 - s);
            m00 = (base + i0) * a.Ws + j0; m01 = (base + i0) * a.Ws + j1;
            m10 = (base + i1) * a.Ws + j0; m11 = (base + i1) * a.Ws + j1;
            w00 = wl * vl; w01 = wl * vu; w10 = wu * vl; w11 = wu * vu;
        } else {
            const unsigned i = fast_div(p, a.dSh), ii = fast_div(q, a.dSw);
            m00 = (base + (int)i) * a.Ws + (int)ii;
        }
        v4i* const o32 = a.out32 ? (v4i*)(a.out32 + (size_t)b * 1024u) + lane : nullptr;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = c0 + 8 * g;
            v4i t = *(const v4i*)(x + i32t_index(m00, c, a.Cs));
            unsigned y[4] = {(unsigned)t.x, (unsigned)t.y, (unsigned)t.z, (unsigned)t.w};
            if constexpr (BILINEAR) {
                const v4i t1 = *(const v4i*)(x + i32t_index(m01, c, a.Cs));
                const v4i t2 = *(const v4i*)(x + i32t_index(m10, c, a.Cs));
                const v4i t3 = *(const v4i*)(x + i32t_index(m11, c, a.Cs));
                y[0] = w00 * y[0] + w01 * (unsigned)t1.x + w10 * (unsigned)t2.x + w11 * (unsigned)t3.x;
                y[1] = w00 * y[1] + w01 * (unsigned)t1.y + w10 * (unsigned)t2.y + w11 * (unsigned)t3.y;
                y[2] = w00 * y[2] + w01 * (unsigned)t1.z + w10 * (unsigned)t2.z + w11 * (unsigned)t3.z;
                y[3] = w00 * y[3] + w01 * (unsigned)t1.w + w10 * (unsigned)t2.w + w11 * (unsigned)t3.w;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) if (c + e >= a.C) y[e] = 0u;  // pad channels
            if (o32) { const v4i o = {(int)y[0], (int)y[1], (int)y[2], (int)y[3]}; o32[g * 64] = o; }
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (a.q[k].ptr)
                    *(unsigned*)(a.q[k].ptr + (size_t)m * a.Cs + c) =
                        pack4(requant1((int)y[0], a.q[k].n, a.q[k].lo, a.q[k].hi), requant1((int)y[1], a.q[k].n, a.q[k].lo, a.q[k].hi),
                              requant1((int)y[2], a.q[k].n, a.q[k].lo, a.q[k].hi), requant1((int)y[3], a.q[k].n, a.q[k].lo, a.q[k].hi)) ^ a.q[k].bias_xor;
        }
    }
}

// 0: upsample_i8_kernel, 1: upsample_i32_kernel<false> (nearest), 2: upsample_i32_kernel<true> (bilinear)
int upsample_inst(bool bilinear, bool i8) { return i8 ? 0 : bilinear ? 2 : 1; }
const char* upsample_kernel_name(int inst) {
    return inst == 0 ? "f8::upsample_i8_kernel" : inst == 1 ? "f8::upsample_i32_kernel<false>" : "f8::upsample_i32_kernel<true>";
}
hipError_t launch_upsample(const UpsampleArgs& a, int inst, hipStream_t s) {
    if (a.N < 1 || a.Hs < 1 || a.Ws < 1 || a.sh < 1 || a.sw < 1 || a.P != a.Hs * a.sh || a.Q != a.Ws * a.sw || (a.Cs & 31) || a.C < 1 || a.C > a.Cs)
        return hipErrorInvalidValue;
    if (inst == 2 && (a.sh != a.sw || a.sh != (1 << a.k) || a.k < 1 || a.k > 4)) return hipErrorInvalidValue;
    if (inst == 0) {
        const size_t work = (size_t)a.N * a.P * a.Ws * (a.Cs >> 4);
        hipLaunchKernelGGL(upsample_i8_kernel, dim3((unsigned)std::min<size_t>((work + 255) / 256, 8192)), dim3(256), 0, s, a);
    } else {
        const size_t nblk = (((size_t)a.N * a.P * a.Q + 31) >> 5) * (size_t)(a.Cs >> 5);
        const dim3 grid((unsigned)std::min<size_t>((nblk + 3) / 4, 2048));      // 2048 workgroups x 4 waves = 8 waves per SIMD on 256 CUs (as tap_kernel)
        if (inst == 1) hipLaunchKernelGGL(upsample_i32_kernel<false>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(upsample_i32_kernel<true>, grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace f8
