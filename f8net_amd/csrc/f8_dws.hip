// f8_dws.hip — one launch for a depthwise-separable block (MobileNet-V1; gfx950; option fuse_dws).
//
//   x (int8 NHWC, CIN ch) --depthwise 3x3 / s, pad 1, ReLU--> mid --1x1 CIN->COUT [ReLU]--> y (int8 NHWC, up to two formats)
//
// Unfused the block is two launches and the requantised depthwise result — as large as the block input — is written to HBM and read
// straight back.  Here it only ever exists in LDS.
//
// Work unit: R output rows x the full width of one image (R * Wo <= 224 pixels = 7 MFMA pixel tiles; a whole 14x14 map is one unit).
//   A  depthwise 3x3 on the matrix cores: the row walker of f8_dwmma_common.h, one (strip, 32-channel tile) per wave at a time, reading the
//      block input straight from HBM / L2; ReLU + requantisation into the LDS mid tile [CIN/32][PX32][32 B] — the order P3 of f8_ir.hip
//      reads its mid2 in: one wave-wide 1 KB B fragment per 32 channels x 32 pixels.  One barrier.
//   B  1x1 GEMM COUT x CIN over the mid tile: a wave owns SLICES of one 32-channel output tile x G pixel tiles (G = 4: 64 accumulator
//      registers; G = 2 where that leaves waves without a slice), the accumulators start at the bias, the weights stream from L2 straight
//      into registers in MFMA-fragment order (pack_frag_weights, as f8_wreg.hip: one coalesced 1 KB instruction per A operand, batches of
//      four K steps, the next batch in flight under this one's multiplies) and every weight fragment feeds G multiplies.  Workgroups start
//      their walk over the output tiles at different tiles, so that they do not all ask L2 for the same kilobyte at once.
//      Epilogue per slice: [ReLU +] requantisation into the consumers' int8 formats (up to two), 16-byte stores.
// 512 threads = 8 waves.  All shapes are run-time values; the instances differ in the walker's form (stride, sub-rows) and the requantisation.
#include "f8_dwmma_common.h"

namespace f8 {

namespace {
constexpr int DWS_NW = 8;                           // waves per workgroup
constexpr int DWS_MAX_PX = 224;                     // pixels of a tile (7 pixel tiles: 14 x 14 = 196 in one)
constexpr int DWS_KB = 4;                           // K steps per weight batch (16 registers; two batches live)
struct DwsSrc { const int8_t* x; const int8_t* w; const int32_t* bias; int32_t N, H, W, Cs, in_signed; };   // what dw_walk reads
}

// S: stride.  SUBS: the walker's sub-rows (2: 14-wide outputs).  FQ: BOTH requantisations — depthwise -> mid, 1x1 -> every output format — are
// right shifts into unsigned 8-bit behind a ReLU: 1 = through the float converter (bounded accumulators, shifts <= 16), 2 = the integer form
// (v_ashr_pk_u8_i32); 0 = any format (general epilogues).
template <int S, int FQ, int SUBS>
__global__ void __launch_bounds__(DWS_NW * 64) dws_kernel(const DwsArgs a) {
    constexpr int VW = SUBS == 2 ? 14 : DWS_SW;
    if constexpr (FQ == 1) set_fp_round_nearest_even();
    extern __shared__ __attribute__((aligned(16))) char mid[];      // [CIN / 32][px32][32 B]
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & (DWS_NW - 1);
    const int n = blockIdx.x / a.tiles_per_img, p0 = (blockIdx.x - n * a.tiles_per_img) * a.R;
    const int p1 = (p0 + a.R) < a.P ? (p0 + a.R) : a.P;
    const int npx = (p1 - p0) * a.Q, npt = (npx + 31) >> 5;         // output pixels of this tile (a ragged last tile has fewer), pixel tiles
    const int plane = a.px32 * 32;                                  // bytes of one 32-channel plane of mid

    // ================= A: depthwise 3x3 -> mid
    {
        const DwsSrc src{a.x, a.wd, a.bd, a.N, a.H, a.W, a.Cin, a.in_signed};
        const int cts = a.Cin >> 5, strips = (a.Q + VW - 1) / VW;
        const int u = SUBS == 2 ? l31 & 15 : l31;
        const float sc1 = FQ == 1 ? requant_u8_scale(a.r1.n) : 0.0f;
        (void)sc1;
        for (int it = wave; it < strips * cts; it += DWS_NW) {      // channel tile fastest: the waves read the same pixels' other channels
            const int ct = it % cts, q0 = (it / cts) * VW;
            const int col_out = q0 + u;
            const bool col_ok = u < VW && col_out < a.Q;
            dw_walk<S, SUBS>(src, n, ct, q0, p0, p1, [&](const v16i& acc, int p) {
                unsigned d[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if constexpr (FQ) d[g] = requant_u8x4_sel<FQ == 2 ? 2 : 1>(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3], a.r1.n, sc1) ^ 0x80808080u;
                    else d[g] = requant_pack4(max(acc[4 * g], 0), max(acc[4 * g + 1], 0), max(acc[4 * g + 2], 0), max(acc[4 * g + 3], 0), a.r1);
                }
                auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
                auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
                if (col_ok && p < p1) {
                    const v4i ov = {(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
                    *(v4i*)(mid + ct * plane + ((p - p0) * a.Q + col_out) * 32 + lh * 16) = ov;
                }
            });
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                   // mid complete

    // ================= B: 1x1 GEMM over mid, one slice (output tile j, pixel tiles g0 .. g0 + G - 1) at a time
    const int nk = a.Cin >> 5, nco = a.Cout >> 5;
    const int floor0 = a.relu0 ? 0 : INT32_MIN;
    (void)floor0;
    auto slices = [&](auto gc) {
        constexpr int G = decltype(gc)::value;
        const int ngr = (npt + G - 1) / G;
        for (int it = wave; it < nco * ngr; it += DWS_NW) {
            const int jj = it % nco, g0 = (it / nco) * G;
            int j = jj + (int)(blockIdx.x % (unsigned)nco);         // rotated start: the workgroups spread over the weight stream
            if (j >= nco) j -= nco;
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
            v4i wc[DWS_KB], wn[DWS_KB];
            auto load_batch = [&](v4i (&dst)[DWS_KB], int k0) {
#pragma unroll
                for (int s = 0; s < DWS_KB; ++s) { const int k = (k0 + s) < nk ? (k0 + s) : (nk - 1); dst[s] = wp[(size_t)k * 64]; }
            };
            load_batch(wc, 0);
            for (int k0 = 0; k0 < nk; k0 += DWS_KB) {
                if (k0 + DWS_KB < nk) load_batch(wn, k0 + DWS_KB);
#pragma unroll
                for (int s = 0; s < DWS_KB; ++s) {
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
                for (int s = 0; s < DWS_KB; ++s) wc[s] = wn[s];
            }
            // ---- epilogue of the slice
#pragma unroll
            for (int t = 0; t < G; ++t) {
                if (g0 + t >= npt) continue;                        // wave-uniform
                const int px = (g0 + t) * 32 + l31;
                const bool ok = px < npx;
                const size_t o = ((size_t)(n * a.P + p0) * a.Q + (ok ? px : 0)) * a.Cout + j * 32 + 16 * lh;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    if (!a.q[k].ptr) continue;                      // wave-uniform
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
    };
    if (nco * ((npt + 3) >> 2) >= DWS_NW) slices(std::integral_constant<int, 4>{});
    else slices(std::integral_constant<int, 2>{});
}

// Rows per tile: as many as fit 224 pixels and the LDS next to nothing else (the weights go to registers), a divisor of the map's height
// where one lies in the upper half of that range (no ragged last tile).
static int dws_rows(int cinS, int P, int Q) {
    if (Q < 1 || Q > DWS_MAX_PX) return 0;
    int rmax = DWS_MAX_PX / Q;
    if (rmax > P) rmax = P;
    while (rmax > 1 && (size_t)((rmax * Q + 31) / 32 * 32) * cinS > 160u * 1024) --rmax;
    if ((size_t)((rmax * Q + 31) / 32 * 32) * cinS > 160u * 1024) return 0;
    for (int r = rmax; 2 * r > rmax; --r) if (P % r == 0) return r;
    return rmax;
}

// The shapes the launch has: what the shared walker can do (output width >= 28, or exactly 14; stride 1 / 2 over an even map, pad 1),
// whole 32-channel tiles on both sides, a mid tile that fits LDS, 32-bit element indices for `imgs` images.  H, W: the block INPUT map.
bool dws_supported(int cinS, int coutS, int H, int W, int stride, int imgs, int* R) {
    if ((stride != 1 && stride != 2) || H < 1 || W < 1 || cinS < 32 || coutS < 32 || (cinS & 31) || (coutS & 31)) return false;
    if (stride == 2 && ((H | W) & 1)) return false;
    const int P = H / stride, Q = W / stride;
    if (!(Q >= DWS_SW || Q == 14)) return false;                     // (7-wide maps: no matrix-core walker form; they stay two launches)
    if ((size_t)imgs * H * W * cinS >= 0x7fffffffull || (size_t)imgs * P * Q * coutS >= 0x7fffffffull) return false;
    const int r = dws_rows(cinS, P, Q);
    if (r < 1) return false;
    if (R) *R = r;
    return true;
}

// FQ (see the kernel) | sub-rows << 2
int dws_inst(const DwsArgs& a, int nq) {
    int fq = (a.relu0 && nq > 0 && a.r1.u8_shr()) ? ((a.acc_ok && !a.rq_int && a.r1.u8_float()) ? 1 : 2) : 0;
    for (int k = 0; k < nq && fq; ++k) {
        if (!a.q[k].u8_shr()) fq = 0;
        else if (fq == 1 && !a.q[k].u8_float()) fq = 2;
    }
    return fq | (a.Q >= DWS_SW ? 1 : 2) << 2;
}

int dws_kernel_name(char* buf, size_t cap, const DwsArgs& a, int inst) {
    return snprintf(buf, cap, "f8::dws_kernel<%d, %d, %d>", a.stride, inst & 3, inst >> 2);
}

template <int S, int FQ, int SUBS>
static hipError_t launch_dws_t(const DwsArgs& a, int lds, hipStream_t s) {
    // dynamic LDS above 64 KB must be opted into per kernel AND per device (a process may drive several GPUs): keep the maximum per device
    static int attr_lds[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (lds > 64 * 1024 && (dev < 0 || lds > attr_lds[dev])) {
        hipError_t e = hipFuncSetAttribute((const void*)dws_kernel<S, FQ, SUBS>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        if (dev >= 0) attr_lds[dev] = lds;
    }
    hipLaunchKernelGGL((dws_kernel<S, FQ, SUBS>), dim3((unsigned)(a.N * a.tiles_per_img)), dim3(DWS_NW * 64), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_dws(const DwsArgs& a0, int inst, hipStream_t s) {
    DwsArgs a = a0;
    int R = 0;
    if (!a.x || !a.wd || !a.bd || !a.w1 || !a.b1 || a.N < 1 || !dws_supported(a.Cin, a.Cout, a.H, a.W, a.stride, a.N, &R) || R != a.R ||
        a.P != a.H / a.stride || a.Q != a.W / a.stride || (inst >> 2) != (a.Q >= DWS_SW ? 1 : 2)) return hipErrorInvalidValue;
    a.tiles_per_img = (a.P + a.R - 1) / a.R;
    a.px32 = (a.R * a.Q + 31) / 32 * 32;
    const int lds = a.px32 * a.Cin;
    const int fq = inst & 3, subs = inst >> 2;
#define F8_DWS(S_, SB_) (fq == 1 ? launch_dws_t<S_, 1, SB_>(a, lds, s) : fq == 2 ? launch_dws_t<S_, 2, SB_>(a, lds, s) : launch_dws_t<S_, 0, SB_>(a, lds, s))
    if (a.stride == 1) return subs == 1 ? F8_DWS(1, 1) : F8_DWS(1, 2);
    return subs == 1 ? F8_DWS(2, 1) : F8_DWS(2, 2);
#undef F8_DWS
}

}  // namespace f8
