// f8_sumpool.hip — windowed average pooling (f8_net_avgpool_window): [C, H, W] -> [C, P, Q], P = (H + 2 pad - k) / stride + 1.
//
// FXQAvgPool2d's int branch applied per window: out = the SUM of the window's in-image values in wrapping 32-bit arithmetic — no division, no
// rounding, no clamp; a tap outside the map contributes 0 (count_include_pad = True: the divisor k^2 is a constant, folded with 2^shift into the
// neighbouring conv's weights by the exporter).  Memory-bound: the source's int32 form (I32T, i32t_index) is read once through the cache, no LDS,
// plain 16-byte vector loads / stores.  Two kernels; the planner (plan_tensor_forms, f8_net.cpp; option sumpool_wide) picks one per node:
//   sumpool_i32_kernel<K>   walks the OUTPUT's I32T blocks, a lane is one output pixel and sums its own window: 2x2 / 2 and every overlapping window
//                           (neighbouring lanes share taps through the cache).
//   sumpool_wide_kernel     a group of lanes shares one output item and splits the window's taps: windows of 3 and more that do not overlap (PSPNet's
//                           bins), where the walker's lanes would sit `kernel` pixels apart.  The rule and what it was measured on: sumpool_wide_rule
//                           (f8_internal.h), profiles/sumpool_r12.md.
// Same values from both, bit for bit: 32-bit adds wrap and commute.  Pad channels [C, Cs) are written as 0 / the format's zero.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "f8_device.h"

namespace f8 {

__device__ __forceinline__ void sumpool_store8(const SumPoolArgs& a, size_t off, const unsigned (&y)[4]) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (a.q[k].ptr)
            *(unsigned*)(a.q[k].ptr + off) =
                requant_pack4((int)y[0], (int)y[1], (int)y[2], (int)y[3], a.q[k]);
}

// Walks the OUTPUT's 4 KB I32T blocks (32 pixels x 32 channels), one wave per block as upsample_i32_kernel / tap_kernel do: lane = output pixel
// pb * 32 + (lane & 31), channels cb * 32 + 8g + 4 (lane >> 5) + 0..3, g = 0..3 — the int32 stores of one g are one contiguous 1 KB transaction per
// wave.  m -> (n, p, q) once per lane and block; the window's taps come through i32t_index, 16 bytes each, neighbouring lanes share them through the
// cache (stride < k) or read neighbouring pieces (stride == k).  K = 2 / 3: the tap loops unrolled; K = 0: the kernel size at run time (a.k).
// Guards: a tap outside [0, H) x [0, W) is not loaded and adds nothing; m < M (ragged last block: its int32 rows exist — Form::slack — but the int8
// forms have none, and nothing is stored for them); a block may straddle rows and images (n, p, q are per lane); channels >= C are written as 0.
template <int K>
__global__ void __launch_bounds__(256) sumpool_i32_kernel(const SumPoolArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned PQ = (unsigned)a.P * (unsigned)a.Q;
    const unsigned M = (unsigned)a.N * PQ;
    const unsigned cbs = (unsigned)a.Cs >> 5;
    const unsigned nblk = ((M + 31u) >> 5) * cbs;
    const int k = K ? K : a.k;
    for (unsigned b = blockIdx.x * 4u + wave; b < nblk; b += gridDim.x * 4u) {
        const unsigned pb = b / cbs, cb = b - pb * cbs;
        const unsigned m = pb * 32u + (lane & 31u);
        if (m >= M) continue;
        const unsigned n = fast_div(m, a.dPQ), pq = m - n * PQ;
        const unsigned p = fast_div(pq, a.dQ), q = pq - p * (unsigned)a.Q;
        const int c0 = (int)(cb * 32u + 4u * (lane >> 5));
        const int h0 = (int)p * a.stride - a.pad, w0 = (int)q * a.stride - a.pad;
        const int row0 = (int)n * a.H;                                // first source row of the image
        unsigned y[4][4];
#pragma unroll
        for (int g = 0; g < 4; ++g) y[g][0] = y[g][1] = y[g][2] = y[g][3] = 0u;
        auto tap = [&](int r, int s) {
            const int h = h0 + r, w = w0 + s;
            if ((unsigned)h >= (unsigned)a.H || (unsigned)w >= (unsigned)a.W) return;      // outside the map: contributes 0
            const int ms = (row0 + h) * a.W + w;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const v4i t = *(const v4i*)(a.x + i32t_index(ms, c0 + 8 * g, a.Cs));
                y[g][0] += (unsigned)t.x; y[g][1] += (unsigned)t.y; y[g][2] += (unsigned)t.z; y[g][3] += (unsigned)t.w;
            }
        };
        if constexpr (K != 0) {
#pragma unroll
            for (int r = 0; r < K; ++r)
#pragma unroll
                for (int s = 0; s < K; ++s) tap(r, s);
        } else {
            for (int r = 0; r < k; ++r)
                for (int s = 0; s < k; ++s) tap(r, s);
        }
        v4i* const o32 = a.out32 ? (v4i*)(a.out32 + (size_t)b * 1024u) + lane : nullptr;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = c0 + 8 * g;
#pragma unroll
            for (int e = 0; e < 4; ++e) if (c + e >= a.C) y[g][e] = 0u;   // pad channels
            if (o32) { const v4i o = {(int)y[g][0], (int)y[g][1], (int)y[g][2], (int)y[g][3]}; o32[g * 64] = o; }
            sumpool_store8(a, (size_t)m * a.Cs + c, y[g]);
        }
    }
}

// avgpool_kernel's scheme widened from a map to a window: G = 1 << a.lg lanes (4 .. 64: sumpool_wide_lg, whole groups inside a wave) share one item = (output pixel m,
// 4 channels); lane j of the group sums the taps j, j + G, ... of the k x k window in row-major order — consecutive lanes read consecutive pixels of a
// source row, consecutive 16-byte pieces of an I32T tile — and lg xor-shuffles add the partial sums; lane 0 stores.  Items are walked grid-stride
// by GROUP: a group is live or not as a whole, so a shuffle (mask < G) never reads a lane that left the loop.
__global__ void __launch_bounds__(256) sumpool_wide_kernel(const SumPoolArgs a) {
    const unsigned G = 1u << a.lg;
    const unsigned j = threadIdx.x & (G - 1u);
    const unsigned PQ = (unsigned)a.P * (unsigned)a.Q;
    const unsigned cgs = (unsigned)a.Cs >> 2;
    const unsigned items = (unsigned)a.N * PQ * cgs;                  // < 2^27 (f8_net_finalize: a form stays below 2 GiB)
    const unsigned kk = (unsigned)(a.k * a.k);
    const unsigned step = (gridDim.x * 256u) >> a.lg;
    for (unsigned item = (blockIdx.x * 256u + threadIdx.x) >> a.lg; item < items; item += step) {
        const unsigned m = fast_div(item, a.dCg), cg = item - m * cgs;
        const unsigned n = fast_div(m, a.dPQ), pq = m - n * PQ;
        const unsigned p = fast_div(pq, a.dQ), q = pq - p * (unsigned)a.Q;
        const int c = (int)(cg << 2);
        const int h0 = (int)p * a.stride - a.pad, w0 = (int)q * a.stride - a.pad;
        const int row0 = (int)n * a.H;
        unsigned y[4] = {0u, 0u, 0u, 0u};
        for (unsigned t = j; t < kk; t += G) {
            const unsigned r = fast_div(t, a.dK), s = t - r * (unsigned)a.k;
            const int h = h0 + (int)r, w = w0 + (int)s;
            if ((unsigned)h >= (unsigned)a.H || (unsigned)w >= (unsigned)a.W) continue;    // outside the map: contributes 0
            const v4i v = *(const v4i*)(a.x + i32t_index((row0 + h) * a.W + w, c, a.Cs));
            y[0] += (unsigned)v.x; y[1] += (unsigned)v.y; y[2] += (unsigned)v.z; y[3] += (unsigned)v.w;
        }
        for (unsigned x = 1; x < G; x <<= 1)
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] += (unsigned)__shfl_xor((int)y[e], (int)x);
        if (j != 0) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (c + e >= a.C) y[e] = 0u;      // pad channels
        if (a.out32) { const v4i o = {(int)y[0], (int)y[1], (int)y[2], (int)y[3]}; *(v4i*)(a.out32 + i32t_index((int)m, c, a.Cs)) = o; }
        sumpool_store8(a, (size_t)m * a.Cs + c, y);
    }
}

// 0: sumpool_i32_kernel<0> (kernel size at run time), 2 / 3: sumpool_i32_kernel<2> / <3>, 4: sumpool_wide_kernel
int sumpool_inst(int k, bool wide) { return wide ? 4 : (k == 2 || k == 3) ? k : 0; }
const char* sumpool_kernel_name(int inst) {
    return inst == 4 ? "f8::sumpool_wide_kernel" : inst == 2 ? "f8::sumpool_i32_kernel<2>" : inst == 3 ? "f8::sumpool_i32_kernel<3>" : "f8::sumpool_i32_kernel<0>";
}
// lanes per item of the wide kernel: the power of two at or above k — a group covers a window ROW per step, the longest contiguous run a window has —,
// 4 .. 64.  (The power of two at or above k^2 left 28 of 64 lanes idle at 6 x 6 and ran 1.9 x the time of 4 x 4 per byte: profiles/sumpool_r12.md.)
int sumpool_wide_lg(int k) { int lg = 2; while (lg < 6 && (1 << lg) < k) ++lg; return lg; }

hipError_t launch_sumpool(const SumPoolArgs& a, int inst, hipStream_t s) {
    if (a.N < 1 || a.H < 1 || a.W < 1 || a.k < 1 || a.k > 64 || a.stride < 1 || a.stride > 64 || a.pad < 0 || 2 * a.pad > a.k || (a.Cs & 31) || a.C < 1 || a.C > a.Cs ||
        a.P != (a.H + 2 * a.pad - a.k) / a.stride + 1 || a.Q != (a.W + 2 * a.pad - a.k) / a.stride + 1 || a.P < 1 || a.Q < 1)
        return hipErrorInvalidValue;
    if ((inst == 2 || inst == 3) && a.k != inst) return hipErrorInvalidValue;
    if (inst == 4) {
        if (a.lg < 2 || a.lg > 6) return hipErrorInvalidValue;
        const size_t threads = ((size_t)a.N * a.P * a.Q * (a.Cs >> 2)) << a.lg;
        hipLaunchKernelGGL(sumpool_wide_kernel, dim3((unsigned)std::min<size_t>((threads + 255) / 256, 16384)), dim3(256), 0, s, a);
    } else {
        const size_t nblk = (((size_t)a.N * a.P * a.Q + 31) >> 5) * (size_t)(a.Cs >> 5);
        const dim3 grid((unsigned)std::min<size_t>((nblk + 3) / 4, 2048));      // 2048 workgroups x 4 waves = 8 waves per SIMD on 256 CUs (as tap_kernel)
        if (inst == 2) hipLaunchKernelGGL(sumpool_i32_kernel<2>, grid, dim3(256), 0, s, a);
        else if (inst == 3) hipLaunchKernelGGL(sumpool_i32_kernel<3>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(sumpool_i32_kernel<0>, grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace f8
