// f8_maxpool.hip — stride-1 max pools on an LDS tile: maxpool_tile_kernel<LEVELS>, LEVELS = 1 .. 3 (options maxpool_tile and fuse_spp, f8_net.cpp).
//
// int8 forms only, stride 1, odd windows 3 .. 13 with pad = k / 2 (the output map is the input map).  LEVELS = 1 is a stand-alone pool (`maxpool_i8:`);
// LEVELS = 2 / 3 is the SPP / SPPF pyramid with its concat (`spp{k1}_{k2}_{k3}+concat_i8:`): level l + 1 is a window of k_{l+1} - k_l + 1 over level l,
// every level is stored to its own channel offset of one output row (pitch oCs), and x itself may be copied to a fourth offset.
//
// Work split.  A workgroup of 384 threads owns one image x 64 channels x one T x T tile of output pixels, T = 24 - 2 R, R = the last level's k / 2
// (T = 22 / 20 / 16 / 12 at k = 3 / 5 / 9 / 13).  It fetches the haloed 24 x 24 x 64-byte patch once — four consecutive lanes read the four 16-byte
// pieces of a pixel's 64 channels — xors it into the unsigned-comparable form (stored ^ 0x80 preserves the order of plain s8 and of biased u8 alike) and
// keeps it in LDS; positions outside the image, and channels past Cs, hold 0, the identity of max in that form.
// LDS: 24 rows x 1600 bytes = 38 400 bytes (a row is 24 x 64 bytes + 64 bytes of padding: 400 dwords = 16 mod 64 banks, so the four rows a wave
// touches in the row pass fall on distinct banks); four workgroups = 24 waves a CU.
//
// Passes.  Per level a row pass, then a column pass, in place.  A thread owns one line (row or column) of the patch x one dword of channels: it reads
// the line's 24 dwords into registers, splits each into even / odd bytes (16-bit lanes), and builds the running maximum of w = 2 r + 1 neighbours by
// doubling: a step s in {1, 2, 4} turns "max of w' from j on" into "max of w' + s" with one packed 16-bit max per half and element (s <= w', so no
// gap).  13 = 1 +1 +2 +4 +4 +1: five steps, 9 = four, 5 = three, 3 = two (maxpool_tile_steps; the steps are kernel arguments, so each is a uniform
// branch to fully unrolled code and the line stays in registers).  The line is merged back to bytes and written centred: position c gets the maximum
// from c - r on, for r <= c < 24 - r; what lies outside that range is never read again.  24 lines x 16 dwords = 384 items: one per thread and pass.
// The xor is applied once per byte on the way in and once per stored byte on the way out, never per tap.
//
// Exactness of the levels.  A level is computed over the whole patch, out-of-image positions included: such a position then holds the maximum of the
// IN-IMAGE values within r of it (or 0).  The next level's window at an in-image p therefore only ever sees in-image values within r1 + r2 of p — and it
// sees all of them: every clipped (r1 + r2)-window is the union of the clipped r1-windows of the in-image points q of its clipped r2-window (for an
// in-image x within r1 + r2 of p, clamp p's coordinates towards x by r2: the image is a box, so q is in it).  So window 5 over window 5 IS window 9,
// padding included, and three chained 5 x 5 pools are the 5 / 9 / 13 pyramid, bit for bit.
//
// Resources (gfx950, -O3): see the table in DESIGN.md 4.5x.  0 bytes of scratch in every instance.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "f8_device.h"

namespace f8 {

typedef unsigned short mpt_us2 __attribute__((ext_vector_type(2)));
constexpr int kMptP = kMaxpoolTilePatch;                     // patch side (pixels)
constexpr int kMptCB = 64;                                   // channels (bytes) a workgroup
constexpr int kMptRow = kMptP * kMptCB + 64;                 // LDS bytes a patch row
constexpr int kMptThreads = kMptP * (kMptCB / 4);            // one (line, dword) item per thread and pass

// one doubling step: v[j] = max(v[j], v[j + S]) where j + S is inside the line (the others are never written back)
template <int S>
__device__ __forceinline__ void mpt_step(mpt_us2 (&ev)[kMptP], mpt_us2 (&od)[kMptP]) {
#pragma unroll
    for (int j = 0; j + S < kMptP; ++j) {
        ev[j] = __builtin_elementwise_max(ev[j], ev[j + S]);
        od[j] = __builtin_elementwise_max(od[j], od[j + S]);
    }
}

// a row (stride = 64 bytes) or column (stride = one LDS row) pass of radius r over the line at `line`
__device__ __forceinline__ void mpt_pass(unsigned char* line, int stride, int r, unsigned steps) {
    mpt_us2 ev[kMptP], od[kMptP];
#pragma unroll
    for (int j = 0; j < kMptP; ++j) {
        const unsigned u = *(const unsigned*)(line + j * stride);
        ev[j] = __builtin_bit_cast(mpt_us2, u & 0x00ff00ffu);
        od[j] = __builtin_bit_cast(mpt_us2, (u >> 8) & 0x00ff00ffu);
    }
    for (; steps; steps >>= 4) {
        const unsigned s = steps & 15u;
        if (s == 1) mpt_step<1>(ev, od);
        else if (s == 2) mpt_step<2>(ev, od);
        else mpt_step<4>(ev, od);
    }
    const int n = kMptP - 2 * r;                               // positions r .. P - r - 1 get the maximum from j = 0 .. n - 1 on
    unsigned char* out = line + r * stride;
#pragma unroll
    for (int j = 0; j < kMptP - 2; ++j)                        // (r >= 1)
        if (j < n) *(unsigned*)(out + j * stride) = __builtin_bit_cast(unsigned, ev[j]) | (__builtin_bit_cast(unsigned, od[j]) << 8);
}

template <int LEVELS>
__global__ void __launch_bounds__(kMptThreads) maxpool_tile_kernel(const MaxPoolTileArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kMptP * kMptRow];
    const int tid = threadIdx.x;
    const int ty = (int)fast_div(blockIdx.x, a.dTW), tx = (int)blockIdx.x - ty * a.tiles_w;
    const int c0 = blockIdx.y * kMptCB, n = blockIdx.z;
    const int R = a.R, T = kMptP - 2 * R;
    const int h0 = ty * T - R, w0 = tx * T - R;               // image position of patch (0, 0)
    const int8_t* xn = a.x + (size_t)n * a.H * a.W * a.Cs;
    int8_t* on = a.q[0].ptr + (size_t)n * a.H * a.W * a.oCs;
    // ---- the patch: 24 x 24 pixels x four 16-byte pieces; x's own copy leaves from the registers
    for (int i = tid; i < kMptP * kMptP * 4; i += kMptThreads) {
        const int pc = i & 3, px = i >> 2;
        const int pr = px / kMptP, pq = px - pr * kMptP;
        const int h = h0 + pr, w = w0 + pq, c = c0 + pc * 16;
        uint4 v = {0u, 0u, 0u, 0u};
        if ((unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W && c < a.Cs) {
            const size_t m = (size_t)h * a.W + w;
            v = *(const uint4*)(xn + m * a.Cs + c);
            if (a.coff[3] >= 0 && pr >= R && pr < R + T && pq >= R && pq < R + T) *(uint4*)(on + m * a.oCs + a.coff[3] + c) = v;
            v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
        }
        *(uint4*)(lds + pr * kMptRow + pq * kMptCB + pc * 16) = v;
    }
    __syncthreads();
    const int ln = tid >> 4, dw = (tid & 15) * 4;              // this thread's line and dword of channels
#pragma unroll
    for (int l = 0; l < LEVELS; ++l) {
        mpt_pass(lds + ln * kMptRow + dw, kMptCB, a.r[l], a.steps[l]);
        __syncthreads();
        mpt_pass(lds + ln * kMptCB + dw, kMptRow, a.r[l], a.steps[l]);
        __syncthreads();
        // ---- the tile's in-image pixels of this level, 16 bytes a lane
        for (int i = tid; i < T * T * 4; i += kMptThreads) {
            const int pc = i & 3, px = i >> 2;
            const int pr = px / T, pq = px - pr * T;
            const int h = h0 + R + pr, w = w0 + R + pq, c = c0 + pc * 16;
            if (h >= a.H || w >= a.W || c >= a.Cs) continue;
            uint4 v = *(const uint4*)(lds + (R + pr) * kMptRow + (R + pq) * kMptCB + pc * 16);
            v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
            *(uint4*)(on + ((size_t)h * a.W + w) * a.oCs + a.coff[l] + c) = v;
        }
        if (l + 1 < LEVELS) __syncthreads();                  // the next level overwrites what the stores read
    }
}

// the doubling steps of a window w = 3 .. 13 (odd), low nibble first: each the largest s in {4, 2, 1} with s <= the window so far and no overshoot
uint32_t maxpool_tile_steps(int w) {
    uint32_t steps = 0;
    int have = 1, sh = 0;
    while (have < w) {
        int s = 4;
        while (s > have || have + s > w) s >>= 1;
        steps |= (uint32_t)s << sh; sh += 4; have += s;
    }
    return steps;
}
// Option maxpool_tile = 1: the shapes the tile kernel keeps, MEASURED at batch 128 against maxpool_i8x16_kernel (profiles/maxpool_tile_r26.md; the legs'
// repeats spread by about +-5 %).  A workgroup walks its whole 24 x 24 patch whatever the map fills of it, so what counts is the share of the tiles' area
// that is map: fill = H W / (tiles T^2).
//   k = 3: 1.19 x faster on the 80 x 80 map, inside the spread at 19 x 19 and 20 x 20 (0.99 - 1.23), 0.67 at 28 x 28 (fill 0.40): kept from 6400 pixels on at fill >= 0.8.
//   k >= 5: faster on every measured shape, 1.18 x (k = 5, 28 x 28, fill 0.49) to 3.84 x (k = 13, 80 x 80); the lowest measured fill is 0.35 (k = 9, 19 x 19:
//   1.42 x).  Kept at fill >= 0.35; below it NOT measured, so the old kernel stays.  k = 7 and 11 were NOT measured: they lie between measured neighbours.
bool maxpool_tile_rule(int k, int H, int W, int Cs) {
    (void)Cs;                                                       // (256 and 512 channels ranked alike)
    const int T = kMptP - 2 * (k / 2), th = (H + T - 1) / T, tw = (W + T - 1) / T;
    if (k == 3) return H * (long long)W >= 80 * 80 && 100ll * H * W >= 80ll * th * tw * T * T;      // (the 80 x 80 map fills 0.83 of its 16 tiles)
    return 100ll * H * W >= 35ll * th * tw * T * T;
}
int maxpool_tile_kernel_name(char* buf, size_t cap, int levels) { return snprintf(buf, cap, "f8::maxpool_tile_kernel<%d>", levels); }
hipError_t launch_maxpool_tile(const MaxPoolTileArgs& a, int levels, hipStream_t s) {
    const int T = kMptP - 2 * a.R;
    int rsum = 0;
    for (int l = 0; l < levels; ++l) rsum += a.r[l];
    if (levels < 1 || levels > 3 || a.R < 1 || a.R > 6 || rsum != a.R || (a.Cs & 31) || (a.oCs & 15) || a.N < 1 || a.N > 65535 ||
        a.tiles_w != (a.W + T - 1) / T || a.tiles_h != (a.H + T - 1) / T)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.tiles_w * a.tiles_h), (unsigned)((a.Cs + kMptCB - 1) / kMptCB), (unsigned)a.N);
    if (levels == 1) hipLaunchKernelGGL(maxpool_tile_kernel<1>, grid, dim3(kMptThreads), 0, s, a);
    else if (levels == 2) hipLaunchKernelGGL(maxpool_tile_kernel<2>, grid, dim3(kMptThreads), 0, s, a);
    else hipLaunchKernelGGL(maxpool_tile_kernel<3>, grid, dim3(kMptThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace f8
