// f8_tap.hip — copy-out of a network output beyond the first (f8_net_output called more than once; option tap_tiled): I32T -> NCHW int32 / float32.
//
// output_kernel (f8_kernels.hip) walks the DESTINATION's index space: a 64-bit divide per element, and a lane reads 4 bytes of every 16 of the
// I32T source, so a wave load touches 1 KB for 256 useful bytes.  Right for 1000 logits, wrong for a 128 x 256 x 56 x 56 map.  This kernel walks
// the SOURCE's 4 KB blocks (32 pixels x 32 channels, i32t_index in f8_device.h):
//   work unit  one wave per block, four waves per workgroup, grid-stride over ceil(N*HW / 32) * Cs/32 blocks
//   loads      four 16-byte loads per lane = 4 x 1 KB per wave, contiguous, every byte used
//   layout     value (g, j) of lane l is channel cb*32 + 8g + 4(l >> 5) + j of pixel m = pb*32 + (l & 31): for fixed (g, j) lanes 0-31 hold 32
//              consecutive pixels of ONE channel — 128 contiguous bytes of an NCHW row — and lanes 32-63 the same pixels of channel + 4.  No LDS.
//   stores     16 dwords per lane; one m / HW, m % HW per lane and block
//   guards     m < N*HW (ragged last pixel block: its rows exist in the arena — Form::slack — and are never written out), c < C (channels padded
//              to 32), and a pixel block may straddle images (49-pixel maps): n is per lane
// Conversion and poisoning are output_kernel's: (float)v rounds to nearest even; a chain launch of THIS run that gave up a halo wait turns the
// values into NaN / INT32_MIN.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <algorithm>
#include "f8_internal.h"

namespace f8 {

template <bool AS_FLOAT>
__global__ void __launch_bounds__(256) tap_kernel(const OutArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned M = (unsigned)a.N * (unsigned)a.HW;             // pixels (an int32 form stays below 2 GiB: f8_net_finalize)
    const unsigned cbs = (unsigned)a.Cs >> 5;                      // channel blocks per pixel block
    const unsigned nblk = ((M + 31u) >> 5) * cbs;
    const bool bad = a.err != nullptr && (*a.err >> 8) == a.epoch;     // f8_fc.hip: a chain launch of this run gave up a halo wait
    for (unsigned b = blockIdx.x * 4u + wave; b < nblk; b += gridDim.x * 4u) {
        const unsigned pb = b / cbs, cb = b - pb * cbs;
        const int4* src = (const int4*)(a.x + (size_t)b * 1024u) + lane;
        int4 v[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) v[g] = src[g * 64];
        const unsigned m = pb * 32u + (lane & 31u);
        if (m >= M) continue;
        const unsigned n = m / (unsigned)a.HW, i = m - n * (unsigned)a.HW;
        const int c0 = (int)(cb * 32u + 4u * (lane >> 5));
        const size_t o = ((size_t)n * a.C + c0) * a.HW + i;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int q[4] = {v[g].x, v[g].y, v[g].z, v[g].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int dc = 8 * g + j;
                if (c0 + dc >= a.C) continue;
                const size_t idx = o + (size_t)dc * a.HW;
                if constexpr (AS_FLOAT) ((float*)a.out)[idx] = bad ? __builtin_nanf("") : (float)q[j];
                else ((int*)a.out)[idx] = bad ? INT32_MIN : q[j];
            }
        }
    }
}

const char* tap_kernel_name(int as_float) { return as_float ? "f8::tap_kernel<true>" : "f8::tap_kernel<false>"; }
hipError_t launch_tap(const OutArgs& a, hipStream_t s) {
    const size_t nblk = (((size_t)a.N * a.HW + 31) >> 5) * (size_t)(a.Cs >> 5);
    const unsigned grid = (unsigned)std::min<size_t>((nblk + 3) / 4, 2048);      // 2048 workgroups x 4 waves = 8 waves per SIMD on 256 CUs
    if (a.as_float) hipLaunchKernelGGL(tap_kernel<true>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(tap_kernel<false>, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace f8
