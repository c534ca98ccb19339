// f8_argmax.hip — channel argmax as a network output (f8_net_output_argmax): out[n, h, w] = the smallest c for which src[n, c, h, w] is maximal,
// over the int32 values the tensor holds (signed compare, no fraclen), written as uint8 or int32 [N, H, W] into the caller's buffer.
//
//   argmax_i32t_kernel<IDX>                 reads the source's int32 form (I32T, i32t_index in f8_device.h) as tap_kernel does: one wave per 32-pixel
//                                           block, looping over the block's channel blocks; four contiguous 16-byte loads per lane and step.  Value (g, j) of
//                                           lane l is channel cb * 32 + 8g + 4 (l >> 5) + j of pixel pb * 32 + (l & 31): a lane meets its channels in ascending
//                                           order (cb, then g, then j), so a strict `>` keeps the lowest index of its half; the two halves of a pixel (lanes l
//                                           and l ^ 32) meet once per pixel block: the other half wins on `>`, or on `==` with the smaller index.
//   upsample_argmax_kernel<BILINEAR, IDX>   the argmax of an upsampled tensor that nothing else reads (option fuse_argmax): a lane owns four consecutive
//                                           output pixels of one row, loops over the SOURCE's channels four at a time, interpolates in registers — the weights
//                                           and the wrapping uint32 arithmetic of upsample_i32_kernel (f8_upsample.hip), term by term — and keeps (max, index)
//                                           per pixel.  The upsampled logits never exist.  The source (25 - 100 KB an image) is served by the caches.
// Both: channels >= C are never compared (they hold 0 and would win on an all-negative pixel); the running maximum starts at (INT32_MIN, 0), so a pixel of
// all INT32_MIN yields 0.  IDX = 1: one byte per pixel (C <= 255), IDX = 4: int32.  A chain launch of THIS run that gave up a halo wait turns the map
// into 255 / INT32_MIN, as output_kernel and tap_kernel poison values.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <algorithm>
#include "f8_device.h"

namespace f8 {

// strict: an equal value later in channel order never replaces an earlier one
__device__ __forceinline__ void amax_step(int v, int c, int& best, int& bi) {
    const bool gt = v > best;
    best = gt ? v : best;
    bi = gt ? c : bi;
}

template <int IDX>
__global__ void __launch_bounds__(256) argmax_i32t_kernel(const ArgmaxArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned M = (unsigned)a.N * (unsigned)a.P * (unsigned)a.Q;      // pixels (an int32 form stays below 2 GiB: f8_net_finalize)
    const unsigned cbs = (unsigned)a.Cs >> 5;                      // channel blocks per pixel block
    const unsigned npb = (M + 31u) >> 5;
    const bool bad = a.err != nullptr && (*a.err >> 8) == a.epoch;         // a chain launch of this run gave up a halo wait
    const int half = (int)(4u * (lane >> 5));
    for (unsigned pb = blockIdx.x * 4u + wave; pb < npb; pb += gridDim.x * 4u) {
        int best = INT32_MIN, bi = 0;
        const int4* src = (const int4*)(a.x + (size_t)pb * cbs * 1024u) + lane;      // (the ragged last pixel block's rows exist in the arena: Form::slack)
        for (unsigned cb = 0; cb < cbs; ++cb, src += 256) {
            int4 v[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) v[g] = src[g * 64];
            const int c0 = (int)(cb * 32u) + half;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int q[4] = {v[g].x, v[g].y, v[g].z, v[g].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c0 + 8 * g + j;
                    if (c < a.C) amax_step(q[j], c, best, bi);      // pad channels hold 0: never compared
                }
            }
        }
        // the other half of the pixel's channels: lane ^ 32
        const int ov = __shfl_xor(best, 32), oi = __shfl_xor(bi, 32);
        if (ov > best || (ov == best && oi < bi)) bi = oi;
        if (bad) bi = IDX == 1 ? 255 : INT32_MIN;
        // lanes 0 - 31 hold 32 consecutive pixels of the NHW result
        const unsigned m = pb * 32u + (lane & 31u);
        if constexpr (IDX == 4) {
            if (lane < 32u && m < M) ((int*)a.out)[m] = bi;          // 128 contiguous bytes per wave
        } else {
            uint8_t* const o = (uint8_t*)a.out + m;
            // four pixels per dword where the caller's buffer allows it (a sub-batch starts at any byte: n0 * H * W) and the block is whole
            const unsigned b1 = (unsigned)__shfl_down(bi, 1), b2 = (unsigned)__shfl_down(bi, 2), b3 = (unsigned)__shfl_down(bi, 3);
            const bool wide = (((uintptr_t)a.out & 3u) == 0u) && pb * 32u + 32u <= M;      // wave-uniform
            if (wide) {
                if (lane < 32u && (lane & 3u) == 0u) *(unsigned*)o = ((unsigned)bi & 255u) | (b1 & 255u) << 8 | (b2 & 255u) << 16 | b3 << 24;
            } else if (lane < 32u && m < M) {
                *o = (uint8_t)bi;
            }
        }
    }
}

// The source pixels and integer weights of output pixel (p, q) of image n: upsample_i32_kernel's (f8_upsample.hip), the same expressions.  Nearest: m[0]
// alone.  Bilinear (scale s = 1 << k on both axes, half-pixel centres): the four clamped neighbours (rows i0 / i1, columns j0 / j1) and the products of
// the per-axis weights of include/f8net.h.  (Kept here and not in a shared header: moved into one, the upsample kernels' object code changed.)
template <bool BILINEAR>
__device__ __forceinline__ void upsample_taps(const ArgmaxArgs& a, unsigned n, unsigned p, unsigned q, int m[4], unsigned w[4]) {
    const int base = (int)n * a.Hs;                                // first source row of the image
    if constexpr (BILINEAR) {
        const int s = 1 << a.k, h = s >> 1;
        const int i = (int)(p >> a.k), jp = (int)(p & (unsigned)(s - 1)), ii = (int)(q >> a.k), jq = (int)(q & (unsigned)(s - 1));
        const bool up = jp < h, left = jq < h;
        const int i0 = up ? max(i - 1, 0) : i, i1 = up ? i : min(i + 1, a.Hs - 1);
        const int j0 = left ? max(ii - 1, 0) : ii, j1 = left ? ii : min(ii + 1, a.Ws - 1);
        const unsigned wl = (unsigned)(up ? s - 2 * jp - 1 : 3 * s - 2 * jp - 1), wu = (unsigned)(up ? s + 2 * jp + 1 : 2 * jp + 1 - s);
        const unsigned vl = (unsigned)(left ? s - 2 * jq - 1 : 3 * s - 2 * jq - 1), vu = (unsigned)(left ? s + 2 * jq + 1 : 2 * jq + 1 - s);
        m[0] = (base + i0) * a.Ws + j0; m[1] = (base + i0) * a.Ws + j1;
        m[2] = (base + i1) * a.Ws + j0; m[3] = (base + i1) * a.Ws + j1;
        w[0] = wl * vl; w[1] = wl * vu; w[2] = wu * vl; w[3] = wu * vu;
    } else {
        const unsigned i = fast_div(p, a.dSh), ii = fast_div(q, a.dSw);
        m[0] = (base + (int)i) * a.Ws + (int)ii;
    }
}

// A work item is (image, output row, four consecutive output columns q0 .. q0 + 3): item = (n * P + p) * Q4 + q0 / 4, Q4 = ceil(Q / 4).  Columns >= Q of a
// ragged last item are computed on column Q - 1 and not stored.  N * P * Q4 < 2^31 (the planner fuses below that).
template <bool BILINEAR, int IDX>
__global__ void __launch_bounds__(256) upsample_argmax_kernel(const ArgmaxArgs a) {
    const unsigned Q4 = ((unsigned)a.Q + 3u) >> 2;
    const unsigned total = (unsigned)a.N * (unsigned)a.P * Q4;
    const bool bad = a.err != nullptr && (*a.err >> 8) == a.epoch;
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const unsigned row = fast_div(idx, a.dQ4), q0 = (idx - row * Q4) * 4u;      // row = n * P + p
        const unsigned n = fast_div(row, a.dP), p = row - n * (unsigned)a.P;
        int m[4][4]; unsigned w[4][4];
        int best[4], bi[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            upsample_taps<BILINEAR>(a, n, p, min(q0 + (unsigned)e, (unsigned)a.Q - 1u), m[e], w[e]);
            best[e] = INT32_MIN; bi[e] = 0;
        }
        for (int c = 0; c < a.C; c += 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const v4i t = *(const v4i*)(a.x + i32t_index(m[e][0], c, a.Cs));
                unsigned y[4] = {(unsigned)t.x, (unsigned)t.y, (unsigned)t.z, (unsigned)t.w};
                if constexpr (BILINEAR) {
                    const v4i t1 = *(const v4i*)(a.x + i32t_index(m[e][1], c, a.Cs));
                    const v4i t2 = *(const v4i*)(a.x + i32t_index(m[e][2], c, a.Cs));
                    const v4i t3 = *(const v4i*)(a.x + i32t_index(m[e][3], c, a.Cs));
                    y[0] = w[e][0] * y[0] + w[e][1] * (unsigned)t1.x + w[e][2] * (unsigned)t2.x + w[e][3] * (unsigned)t3.x;
                    y[1] = w[e][0] * y[1] + w[e][1] * (unsigned)t1.y + w[e][2] * (unsigned)t2.y + w[e][3] * (unsigned)t3.y;
                    y[2] = w[e][0] * y[2] + w[e][1] * (unsigned)t1.z + w[e][2] * (unsigned)t2.z + w[e][3] * (unsigned)t3.z;
                    y[3] = w[e][0] * y[3] + w[e][1] * (unsigned)t1.w + w[e][2] * (unsigned)t2.w + w[e][3] * (unsigned)t3.w;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c + j < a.C) amax_step((int)y[j], c + j, best[e], bi[e]);      // the wrapped value, signed; pad channels never compared
            }
        }
        if (bad) { bi[0] = bi[1] = bi[2] = bi[3] = IDX == 1 ? 255 : INT32_MIN; }
        const size_t o = (size_t)row * (unsigned)a.Q + q0;
        const unsigned nv = min(4u, (unsigned)a.Q - q0);             // valid columns of this item
        if constexpr (IDX == 4) {
            int* const out = (int*)a.out + o;
            if (nv == 4u && (((uintptr_t)out & 15u) == 0u)) { const v4i v = {bi[0], bi[1], bi[2], bi[3]}; *(v4i*)out = v; }
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if ((unsigned)e < nv) out[e] = bi[e];
            }
        } else {
            uint8_t* const out = (uint8_t*)a.out + o;
            if (nv == 4u && (((uintptr_t)out & 3u) == 0u)) *(unsigned*)out = ((unsigned)bi[0] & 255u) | ((unsigned)bi[1] & 255u) << 8 | ((unsigned)bi[2] & 255u) << 16 | (unsigned)bi[3] << 24;
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if ((unsigned)e < nv) out[e] = (uint8_t)bi[e];
            }
        }
    }
}

// 0 / 1: argmax_i32t_kernel<1> / <4>; 2 / 3: upsample_argmax_kernel<false, 1> / <false, 4> (nearest); 4 / 5: upsample_argmax_kernel<true, 1> / <true, 4> (bilinear)
int argmax_inst(bool fused, bool bilinear, int index_bytes) { return (fused ? (bilinear ? 4 : 2) : 0) + (index_bytes == 4); }
const char* argmax_kernel_name(int inst) {
    static const char* const names[6] = {"f8::argmax_i32t_kernel<1>", "f8::argmax_i32t_kernel<4>", "f8::upsample_argmax_kernel<false, 1>",
                                         "f8::upsample_argmax_kernel<false, 4>", "f8::upsample_argmax_kernel<true, 1>", "f8::upsample_argmax_kernel<true, 4>"};
    return inst >= 0 && inst < 6 ? names[inst] : "?";
}
hipError_t launch_argmax(const ArgmaxArgs& a, int inst, hipStream_t s) {
    if (a.N < 1 || a.P < 1 || a.Q < 1 || a.C < 2 || a.C > a.Cs || (a.Cs & 31) || !a.x || !a.out || inst < 0 || inst > 5) return hipErrorInvalidValue;
    if (!(inst & 1) && a.C > 255) return hipErrorInvalidValue;
    if (inst < 2) {
        const size_t npb = ((size_t)a.N * a.P * a.Q + 31) >> 5;
        const dim3 grid((unsigned)std::min<size_t>((npb + 3) / 4, 2048));      // 2048 workgroups x 4 waves = 8 waves per SIMD on 256 CUs (as tap_kernel)
        if (inst == 0) hipLaunchKernelGGL(argmax_i32t_kernel<1>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(argmax_i32t_kernel<4>, grid, dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (a.Hs < 1 || a.Ws < 1 || a.sh < 1 || a.sw < 1 || a.P != a.Hs * a.sh || a.Q != a.Ws * a.sw) return hipErrorInvalidValue;
    if (inst >= 4 && (a.sh != a.sw || a.sh != (1 << a.k) || a.k < 1 || a.k > 4)) return hipErrorInvalidValue;
    const size_t work = (size_t)a.N * a.P * ((a.Q + 3) >> 2);
    if (work >= (1ull << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::min<size_t>((work + 255) / 256, 8192));
    switch (inst) {
        case 2: hipLaunchKernelGGL((upsample_argmax_kernel<false, 1>), grid, dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL((upsample_argmax_kernel<false, 4>), grid, dim3(256), 0, s, a); break;
        case 4: hipLaunchKernelGGL((upsample_argmax_kernel<true, 1>), grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((upsample_argmax_kernel<true, 4>), grid, dim3(256), 0, s, a); break;
    }
    return hipGetLastError();
}

}  // namespace f8
