// f8_dws7.hip — one launch for a depthwise-separable block whose OUTPUT map is 7 x 7 (MobileNet-V1's last blocks; gfx950; option fuse_dws7),
// with the average pool behind the block summed in its epilogue where the plan folds it in.
//
//   x (int8 NHWC, CIN ch; 7 x 7 at stride 1 or 14 x 14 at stride 2) --depthwise 3x3 / s, pad 1, ReLU--> mid --1x1 CIN->COUT [ReLU]--> y
//   y: int8 NHWC in up to two formats, or (POOL) only its per-image sums over the 49 pixels: int32 (I32T, one pixel per image) and / or int8.
//
// The function is dws_kernel's (f8_dws.hip), which has no form for these maps: its depthwise phase walks rows on the matrix cores and 7 of 32
// lanes would be live.  Here:
// Work unit: I images x a slice of the output-channel tiles.  The pixels of I consecutive images lie end to end — I * 49 <= 196 pixels = 7 MFMA
//   pixel tiles, and since the maps are whole, that is also their order in the NHWC output.  Workgroup (g, z) of ceil(N / I) * Z runs phase A
//   for image group g and phase B over output tiles [z * nco / Z, (z + 1) * nco / Z): phase A is recomputed Z times (9 multiply-adds per value
//   against COUT / Z in phase B) so that a few image groups still fill the chip.
//   A  depthwise 3x3 on v_dot4_i32_i8, the form the default plan runs on 7-wide maps (dwconv3x3_dot4_kernel, f8_kernels.hip; the matrix-core
//      form measured slower there): one thread = one pixel x 16 channels, the 9 taps read straight from HBM / L2 with the biased-zero border,
//      per 4-channel quad the tap dwords byte-transposed (8 v_perm_b32) and reduced by 4 v_dot4 against the tap-transposed weight image of
//      pack_dw_weights; ReLU + requantisation; the thread's 16 bytes are exactly one half-slot of the LDS mid tile [CIN/32][PX32][32 B]: one
//      16-byte ds_write, no lane swap.  One barrier.
//   B  1x1 GEMM over the mid tile, dws_kernel's phase B (a copy: that file is a measured kernel and stays as it is): a wave owns slices of
//      one 32-channel output tile x G pixel tiles, the weights stream from L2 into registers in fragment order, batches of four K steps.
//      Epilogue per slice: [ReLU +] requantisation into the consumers' int8 formats, 16-byte stores — or, POOL, the post-ReLU int32 values
//      summed per image: an image's 49 pixels straddle pixel tiles and a tile holds pixels of at most two images, so per accumulator row two
//      masked lane reductions (the second only where the tile has a seam), then one LDS add per (image, channel); after a barrier the
//      workgroup writes the pooled forms.  Wrapping int32 adds: exact in any order (FXQAvgPool2d's int branch is a wrapping sum).
// A ragged last group has fewer than I images: its missing pixels are neither read nor stored nor summed.
// 512 threads = 8 waves.  No exchange between workgroups.
#include "f8_device.h"
#include <algorithm>

namespace f8 {

namespace {
constexpr int D7_NW = 8;                            // waves per workgroup
constexpr int D7_PX = 49;                           // pixels of the output map (7 x 7)
constexpr int D7_MAX_I = 4;                         // images per group: 196 pixels = 7 pixel tiles
constexpr int D7_KB = 4;                            // K steps per weight batch (16 registers; two batches live)
constexpr size_t D7_LDS = 160u * 1024;
}

// S: stride.  FQ: the requantisations — depthwise -> mid and, without POOL, 1x1 -> every output format — are right shifts into unsigned 8-bit
// behind a ReLU: 1 = through the float converter (bounded accumulators, shifts <= 16), 2 = the integer form (v_ashr_pk_u8_i32); 0 = any format.
// POOL: only the per-image sums of the block output leave the chip (requantised in the general form: one value per image and channel).
template <int S, int FQ, bool POOL>
__global__ void __launch_bounds__(D7_NW * 64) dws7_kernel(const Dws7Args a) {
    if constexpr (FQ == 1) set_fp_round_nearest_even();
    extern __shared__ __attribute__((aligned(16))) char mid[];      // [CIN / 32][px32][32 B], then (POOL) sums [I][ncz * 32]
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & (D7_NW - 1);
    const int grp = blockIdx.x / a.Z, z = blockIdx.x - grp * a.Z;
    const int n0 = grp * a.I;
    const int imgs = (a.N - n0) < a.I ? (a.N - n0) : a.I;           // a ragged last group has fewer
    const int npx = imgs * D7_PX, npt = (npx + 31) >> 5;
    const int plane = a.px32 * 32;                                  // bytes of one 32-channel plane of mid
    const int nk = a.Cin >> 5, nco = a.Cout >> 5, ncz = nco / a.Z;  // K steps, output tiles, output tiles of this workgroup
    unsigned* const sums = (unsigned*)(mid + (size_t)nk * plane);
    if constexpr (POOL)
        for (int i = tid; i < imgs * ncz * 32; i += D7_NW * 64) sums[i] = 0u;

    // ================= A: depthwise 3x3 -> mid, one (pixel, 16 channels) per thread at a time; the 16-channel group runs fastest
    {
        const int cgs = a.Cin >> 4;
        const unsigned padv = a.in_signed ? 0u : 0x80808080u;
        const float sc1 = FQ == 1 ? requant_u8_scale(a.r1.n) : 0.0f;
        (void)sc1;
        for (int idx = tid; idx < npx * cgs; idx += D7_NW * 64) {
            const int px = idx / cgs, cg = idx - px * cgs, c = cg << 4;
            const int im = px / D7_PX, pp = px - im * D7_PX, p = pp / 7, q = pp - p * 7;
            const int h0 = p * S - 1, w0 = q * S - 1;
            const int8_t* const xi = a.x + (size_t)(n0 + im) * a.H * a.W * a.Cin + c;
            v4i x[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int h = h0 + r, w = w0 + s;
                    v4i v = {(int)padv, (int)padv, (int)padv, (int)padv};
                    if ((unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W) v = *(const v4i*)(xi + ((size_t)h * a.W + w) * a.Cin);
                    x[r * 3 + s] = v;
                }
            unsigned o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {                           // 4-channel quad inside the 16
                const unsigned* const wq = (const unsigned*)a.wd4 + (size_t)((c >> 2) + k) * 9;     // [wA0..3, wB0..3, wC]
                const v4i bv = *(const v4i*)(a.bd4 + c + 4 * k);
                int acc[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int g = 0; g < 2; ++g) {                       // taps 0-3, 4-7: byte-transpose 4 taps x 4 channels, one dot4 per channel
                    const unsigned t0 = (unsigned)x[g * 4][k], t1 = (unsigned)x[g * 4 + 1][k], t2 = (unsigned)x[g * 4 + 2][k], t3 = (unsigned)x[g * 4 + 3][k];
                    const unsigned lo01 = __builtin_amdgcn_perm(t1, t0, 0x05010400u), hi01 = __builtin_amdgcn_perm(t1, t0, 0x07030602u);
                    const unsigned lo23 = __builtin_amdgcn_perm(t3, t2, 0x05010400u), hi23 = __builtin_amdgcn_perm(t3, t2, 0x07030602u);
                    const unsigned c0 = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u), c1 = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
                    const unsigned c2 = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u), c3 = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
                    acc[0] = __builtin_amdgcn_sdot4((int)c0, (int)wq[g * 4 + 0], acc[0], false);
                    acc[1] = __builtin_amdgcn_sdot4((int)c1, (int)wq[g * 4 + 1], acc[1], false);
                    acc[2] = __builtin_amdgcn_sdot4((int)c2, (int)wq[g * 4 + 2], acc[2], false);
                    acc[3] = __builtin_amdgcn_sdot4((int)c3, (int)wq[g * 4 + 3], acc[3], false);
                }
                const unsigned t8 = (unsigned)x[8][k], wC = wq[8];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    acc[e] = (int)((unsigned)acc[e] + (unsigned)((int)(signed char)(t8 >> (8 * e)) * (int)(signed char)(wC >> (8 * e))));
                if constexpr (FQ) o[k] = requant_u8x4_sel<FQ == 2 ? 2 : 1>(acc[0], acc[1], acc[2], acc[3], a.r1.n, sc1) ^ 0x80808080u;
                else o[k] = requant_pack4(max(acc[0], 0), max(acc[1], 0), max(acc[2], 0), max(acc[3], 0), a.r1);
            }
            const v4i ov = {(int)o[0], (int)o[1], (int)o[2], (int)o[3]};
            *(v4i*)(mid + (cg >> 1) * plane + px * 32 + (cg & 1) * 16) = ov;
        }
    }
    __syncthreads();                                                // mid complete (and the sums zero)

    // ================= B: 1x1 GEMM over mid, one slice (output tile j, pixel tiles g0 .. g0 + G - 1) at a time
    const int floor0 = a.relu0 ? 0 : INT32_MIN;
    (void)floor0;
    auto slices = [&](auto gc) {
        constexpr int G = decltype(gc)::value;
        const int ngr = (npt + G - 1) / G;
        for (int it = wave; it < ncz * ngr; it += D7_NW) {
            const int jj = it % ncz, g0 = (it / ncz) * G;
            int jl = jj + (int)((unsigned)grp % (unsigned)ncz);     // rotated start: the workgroups spread over the weight stream
            if (jl >= ncz) jl -= ncz;
            const int j = z * ncz + jl;
            const v4i* const wp = (const v4i*)a.w1 + (size_t)j * nk * 64 + lane;      // fragment order: [tile][K32 step][lane][16 B]
            v16i acc[G];
            {
                v4i bq[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) bq[g] = *(const v4i*)(a.b1 + j * 32 + 8 * g + 4 * lh);
#pragma unroll
                for (int t = 0; t < G; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[t][r] = bq[r >> 2][r & 3];
            }
            v4i wc[D7_KB], wn[D7_KB];
            auto load_batch = [&](v4i (&dst)[D7_KB], int k0) {
#pragma unroll
                for (int s = 0; s < D7_KB; ++s) { const int k = (k0 + s) < nk ? (k0 + s) : (nk - 1); dst[s] = wp[(size_t)k * 64]; }
            };
            load_batch(wc, 0);
            for (int k0 = 0; k0 < nk; k0 += D7_KB) {
                if (k0 + D7_KB < nk) load_batch(wn, k0 + D7_KB);
#pragma unroll
                for (int s = 0; s < D7_KB; ++s) {
                    if (k0 + s >= nk) continue;                     // wave-uniform
                    const char* const mp = mid + (k0 + s) * plane + l31 * 32 + lh * 16;
#pragma unroll
                    for (int t = 0; t < G; ++t) {
                        if (g0 + t >= npt) continue;                // wave-uniform
                        const v4i xf = *(const v4i*)(mp + (g0 + t) * 1024);
                        acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wc[s], xf, acc[t], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int s = 0; s < D7_KB; ++s) wc[s] = wn[s];
            }
            // ---- epilogue of the slice
#pragma unroll
            for (int t = 0; t < G; ++t) {
                if (g0 + t >= npt) continue;                        // wave-uniform
                const int px = (g0 + t) * 32 + l31;
                const bool ok = px < npx;
                if constexpr (POOL) {
                    // the tile's pixels belong to image ia or ia + 1 (49 > 32); pixels past npx to none
                    const int first = (g0 + t) * 32, last = (first + 31 < npx ? first + 31 : npx - 1);
                    const int ia = first / D7_PX, ib = last / D7_PX;        // wave-uniform
                    const int seam = (ia + 1) * D7_PX;
                    const bool in_a = ok && px < seam, in_b = ok && px >= seam;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const unsigned v = (unsigned)max(acc[t][r], floor0);
                        unsigned sa = in_a ? v : 0u;
#pragma unroll
                        for (int m = 1; m < 32; m <<= 1) sa += (unsigned)__shfl_xor((int)sa, m);     // inside each 32-lane half: the halves hold different channels
                        const int ch = jl * 32 + 8 * (r >> 2) + 4 * lh + (r & 3);
                        if (l31 == 0) atomicAdd(&sums[ia * ncz * 32 + ch], sa);
                        if (ib != ia) {
                            unsigned sb = in_b ? v : 0u;
#pragma unroll
                            for (int m = 1; m < 32; m <<= 1) sb += (unsigned)__shfl_xor((int)sb, m);
                            if (l31 == 0) atomicAdd(&sums[ib * ncz * 32 + ch], sb);
                        }
                    }
                } else {
                    const size_t o = ((size_t)n0 * D7_PX + (ok ? px : 0)) * a.Cout + j * 32 + 16 * lh;
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        if (!a.q[k].ptr) continue;                  // wave-uniform
                        unsigned d[4];
                        if constexpr (FQ) {
                            const float sc = FQ == 1 ? requant_u8_scale(a.q[k].n) : 0.0f;
#pragma unroll
                            for (int g = 0; g < 4; ++g) d[g] = requant_u8x4_sel<FQ == 2 ? 2 : 1>(acc[t][4 * g], acc[t][4 * g + 1], acc[t][4 * g + 2], acc[t][4 * g + 3], a.q[k].n, sc) ^ 0x80808080u;
                        } else {
#pragma unroll
                            for (int g = 0; g < 4; ++g)
                                d[g] = requant_pack4(max(acc[t][4 * g], floor0), max(acc[t][4 * g + 1], floor0), max(acc[t][4 * g + 2], floor0), max(acc[t][4 * g + 3], floor0), a.q[k]);
                        }
                        auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
                        auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
                        if (ok) {
                            const v4i ov = {(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
                            *(v4i*)(a.q[k].ptr + o) = ov;
                        }
                    }
                }
            }
        }
    };
    if (ncz * ((npt + 3) >> 2) >= D7_NW) slices(std::integral_constant<int, 4>{});
    else slices(std::integral_constant<int, 2>{});

    if constexpr (POOL) {
        __syncthreads();                                            // every slice's sums are in
        // the pooled tensor's forms, four channels of one image per thread at a time
        for (int i = tid; i < imgs * ncz * 8; i += D7_NW * 64) {
            const int im = i / (ncz * 8), c4 = (i - im * ncz * 8) * 4;
            const v4i v = *(const v4i*)(sums + im * ncz * 32 + c4);
            const int n = n0 + im, c = z * ncz * 32 + c4;
            if (a.out32) *(v4i*)(a.out32 + i32t_index(n, c, a.Cout)) = v;
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (a.q[k].ptr)
                    *(unsigned*)(a.q[k].ptr + (size_t)n * a.Cout + c) =
                        requant_pack4(v.x, v.y, v.z, v.w, a.q[k]);
        }
    }
}

// LDS of a launch: the mid tile of I images and, with the pool, one int32 sum per image and output channel (sized for Z = 1)
static size_t dws7_lds(int cinS, int coutS, int I, bool pool) {
    return (size_t)((I * D7_PX + 31) / 32 * 32) * cinS + (pool ? (size_t)I * coutS * 4 : 0);
}

// The shapes the launch has: an OUTPUT map of exactly 7 x 7 (input 7 x 7 at stride 1, 14 x 14 at stride 2), pad 1, whole 32-channel tiles on
// both sides, 32-bit element indices for `imgs` images.  *I = images per workgroup: the most (<= 4) whose mid tile — and, with the pool, sums —
// fit the 160 KB of LDS (CIN <= 512: 4; CIN = 1024: 3, exactly 160 KB, without the pool, 2 with it).  H, W: the block INPUT map.
bool dws7_supported(int cinS, int coutS, int H, int W, int stride, int imgs, bool pool, int* I) {
    if ((stride != 1 && stride != 2) || cinS < 32 || coutS < 32 || (cinS & 31) || (coutS & 31) || imgs < 1) return false;
    if (H != 7 * stride || W != 7 * stride) return false;
    if ((size_t)imgs * H * W * cinS >= 0x7fffffffull || (size_t)imgs * D7_PX * coutS >= 0x7fffffffull) return false;
    int i = D7_MAX_I;
    while (i >= 1 && dws7_lds(cinS, coutS, i, pool) > D7_LDS) --i;
    if (i < 1) return false;
    if (I) *I = i;
    return true;
}

// Z, the slices of the output tiles: the smallest divisor of COUT / 32 that gives every compute unit a workgroup (groups * Z >= cus), all of
// them — one tile per workgroup — where none does.  (128 images x 1024 -> 1024 channels on 256 CUs: 43 groups of 3, Z = 8, 344 workgroups.)
int dws7_slices(int groups, int nco, int cus) {
    for (int zz = 1; zz < nco; ++zz) if (nco % zz == 0 && (long)groups * zz >= cus) return zz;
    return nco;
}

// FQ (see the kernel).  With the pool only the depthwise requantisation is in it: the pooled values take the general form.
int dws7_inst(const Dws7Args& a, int nq) {
    int fq = (a.relu0 && (a.pool || nq > 0) && a.r1.u8_shr()) ? ((a.acc_ok && !a.rq_int && a.r1.u8_float()) ? 1 : 2) : 0;
    for (int k = 0; k < nq && fq && !a.pool; ++k) {
        if (!a.q[k].u8_shr()) fq = 0;
        else if (fq == 1 && !a.q[k].u8_float()) fq = 2;
    }
    return fq;
}

int dws7_kernel_name(char* buf, size_t cap, const Dws7Args& a, int inst) {
    return snprintf(buf, cap, "f8::dws7_kernel<%d, %d, %s>", a.stride, inst & 3, a.pool ? "true" : "false");
}

template <int S, int FQ, bool POOL>
static hipError_t launch_dws7_t(const Dws7Args& a, int lds, hipStream_t s) {
    // dynamic LDS above 64 KB must be opted into per kernel AND per device (a process may drive several GPUs): keep the maximum per device
    static int attr_lds[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (lds > 64 * 1024 && (dev < 0 || lds > attr_lds[dev])) {
        hipError_t e = hipFuncSetAttribute((const void*)dws7_kernel<S, FQ, POOL>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        if (dev >= 0) attr_lds[dev] = lds;
    }
    const int groups = (a.N + a.I - 1) / a.I;
    hipLaunchKernelGGL((dws7_kernel<S, FQ, POOL>), dim3((unsigned)(groups * a.Z)), dim3(D7_NW * 64), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_dws7(const Dws7Args& a0, int inst, int num_cu, hipStream_t s) {
    Dws7Args a = a0;
    int I = 0;
    const bool pool = a.pool != 0;
    if (!a.x || !a.wd4 || !a.bd4 || !a.w1 || !a.b1 || a.N < 1 || !dws7_supported(a.Cin, a.Cout, a.H, a.W, a.stride, a.N, pool, &I) || I != a.I ||
        (pool && !a.out32 && !a.q[0].ptr) || (!pool && !a.q[0].ptr)) return hipErrorInvalidValue;
    a.px32 = (a.I * D7_PX + 31) / 32 * 32;
    a.Z = dws7_slices((a.N + a.I - 1) / a.I, a.Cout >> 5, num_cu > 0 ? num_cu : 256);
    const int lds = (int)dws7_lds(a.Cin, a.Cout, a.I, pool);
    const int fq = inst & 3;
#define F8_DWS7(S_, P_) (fq == 1 ? launch_dws7_t<S_, 1, P_>(a, lds, s) : fq == 2 ? launch_dws7_t<S_, 2, P_>(a, lds, s) : launch_dws7_t<S_, 0, P_>(a, lds, s))
    if (a.stride == 1) return pool ? F8_DWS7(1, true) : F8_DWS7(1, false);
    return pool ? F8_DWS7(2, true) : F8_DWS7(2, false);
#undef F8_DWS7
}

}  // namespace f8
