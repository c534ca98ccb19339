// f8_gconvx.hip — grouped 3x3 convolution for group widths 72 .. 256, "weights streamed, accumulators stationary" on v_mfma_i32_32x32x32_i8 (gfx950 only).
//
// The shapes: kernel 3, stride 1 / 2, pad 0 / 1, cin == cout == C, cg = C / groups a multiple of 8 in 72 .. 256, groups >= 2; H, W, N at run time.
// At these widths a group is a GEMM of its own (N = cg, K = 9 cg): f8_gconvw.hip's resident weights (9 KS fragments a wave, KS = ceil(cg / 32)) would
// be 108 .. 288 VGPRs.  Here the roles are turned round: a wave keeps the ACCUMULATORS of up to NPG 32-pixel groups of its tile and streams the weights.
//
//   * UNITS are f8_gconvw.hip's, and so is their packed order (f8_net.cpp pack_gconvw_weights): unit g KS + j = group g x 32-output subtile j,
//     live = min(32, cg - 32 j) channels, K = the group's own cg input channels over KS K32 steps per tap, zero rows past `live` and zero K bytes past
//     the group; [group][subtile][tap][kstep][lane][16 B], so the fragment of one (tap, kstep) is one coalesced 1 KB load and a subtile's 9 KS fragments
//     are consecutive.  Where Cs > C one all-zero unit behind the last group writes the padded channels C .. Cs - 1 through the same epilogue.
//   * A WORKGROUP (4 waves) owns ONE group (or the pad unit) x one pixel tile of gconvx_tile: R rows x TW columns of one image or G whole small images,
//     at most 8 x 32 output pixels (stride 2: 4 x 32).  Workgroups of one group are consecutive (tile index fastest), so the groups in flight — and their weights, up to
//     9 x 8 x 8 KB — are few; the input is read once whatever the order.
//   * PATCH: the haloed input patch of the group's channel span, fetched once by LDS-direct DMA in 16-byte slots, zero fill by the buffer range check
//     (out-of-image pixels, images past N, channels past Cs), border-class bias for biased inputs.  The span starts AT the group's first byte g cg — a
//     multiple of 8, and 8 mod 16 for odd groups of cg = 8 mod 16 (72, 88, ..., 232): the 16-byte LDS-direct load takes a source that is only
//     8-byte aligned on gfx950 (bit-exact on the device: tests/test_gpu_gconv_xwide.py, every odd group), so every lane's 16 K bytes are ONE
//     ds_read_b128.  MEASURED ALTERNATIVE: the span rounded down to 16 and, for a group at offset 8, two ds_read_b64 (f8_gconvw.hip's wave-uniform
//     choice) was 1.3 .. 2.2x slower on every cg = 8 mod 16 shape (720 x 14 x 14, cg 120: 83.6 against 55.9 us; profiles/gconv_xwide_r20.md).
//     The pixel pitch is 32 KS + 16 bytes: an ODD number of 16-byte chunks, so that 16 consecutive patch pixels cover the 16 chunk columns of a
//     256-byte bank row once without a swizzle (a pitch that is not a power of two has no XOR swizzle).  Stride 2: a patch row holds its even
//     columns, then its odd ones (the permutation is applied on the DMA's source side), so consecutive output pixels read consecutive LDS pixels there
//     too.  Only the ceil(cg / 16) chunks that meet a non-zero weight are fetched; the rest of the pitch is written as zeros by the range check.  The
//     last chunk of a group may run up to 8 bytes past it — into the next group, the next pixel or (range check: zeros) past the tensor: those K bytes
//     meet zero weights.
//   * WORK ITEMS: subtile j x one of `psplit` parts of the tile's pixel groups, dealt round-robin to the waves.  psplit = 1 unless splitting shortens
//     the longest wave and still leaves four pixel groups an item (gconvx_tile).  An item: NPG x 16 accumulators (instances NPG = 4 and, stride 1 only, 8), loop (tap, kstep) outer and
//     pixel groups inner — every fetched fragment feeds all of the item's pixel groups before the next replaces it, and the next is loaded under the
//     MFMAs of the current one.
//
// Arithmetic and output forms are gconvw3x3_kernel's: wrapping int32 accumulation, class bias, optional ReLU floor, the tiled int32 form and / or up to
// two requantised int8 forms — integer requantisation (requant1) whatever Options::requant_float says.  No residual join.
#include "f8_device.h"
#include <algorithm>

namespace f8 {

typedef int v2i __attribute__((ext_vector_type(2)));

namespace {
constexpr int GX_LDS_BUDGET = 64 * 1024;            // patch bytes per workgroup: two workgroups (two waves per SIMD) per CU, which is what 128 accumulators a lane allow anyway
constexpr int GX_TW_MAX[3] = {0, 64, 32};           // widest tile by stride (gconv_tile's)
constexpr int GX_NPG_MAX[3] = {0, 8, 4};            // 32-pixel groups per tile by stride: 256 output pixels; stride 2: 128 (its patch is four times its outputs:
                                                    // more than 128 fit the budget only below cg 100, and then barely)
}

template <int S, int NPG>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NPG == 4 ? 3 : 2))) gconvx3x3_kernel(const GConvXArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;
    const int l31 = lane & 31, lh = lane >> 5;

    // ---- this workgroup's group and tile: tile fastest
    const int ntile = ((a.N + a.G - 1) / a.G) * a.tiles_r * a.tiles_c;
    const int gi = blockIdx.x / ntile;                          // the group; a.groups: the pad unit
    int t = blockIdx.x - gi * ntile;
    const int tc = t % a.tiles_c; t /= a.tiles_c;
    const int tr = t % a.tiles_r;
    const int n0 = (t / a.tiles_r) * a.G;
    const int p0 = tr * a.R, q0 = tc * a.TW;
    const int IMG_PP = a.PR * a.PW;                             // patch pixels per image
    const int CH = a.pitch >> 4;                                // 16-byte chunks of a patch pixel
    const int slots = a.G * IMG_PP * CH;
    const int h0 = p0 * S - a.pad, w0 = q0 * S - a.pad;         // image position of patch pixel (0, 0)
    const bool padu = gi == a.groups;
    const int c0 = gi * a.cg;                                   // the group's first channel (the pad unit: C)
    const int nch = padu ? 0 : (a.cg + 15) >> 4;                // chunks that meet a non-zero weight (the pad unit: none — its patch is zeros)
    constexpr int PWE_ON = S == 2;                              // stride 2: a patch row holds its even columns, then its odd ones
    const int PWe = (a.PW + 1) >> 1;

    // ---- patch: every 16-byte slot once, linear: slot s = chunk s % CH of patch pixel s / CH
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
    for (int i = 0; i * 256 + wave * 64 < slots; ++i) {         // wave-uniform bound
        const int s = i * 256 + tid;
        const int ppx = (int)fast_div((unsigned)s, a.dCH), chunk = s - ppx * CH;
        const int img = (int)fast_div((unsigned)ppx, a.dIPP), rem = ppx - img * IMG_PP;
        const int pr = (int)fast_div((unsigned)rem, a.dPW), px = rem - pr * a.PW;
        const int pc = !PWE_ON ? px : px < PWe ? 2 * px : 2 * (px - PWe) + 1;
        const int h = h0 + pr, w = w0 + pc, n = n0 + img, cb = c0 + chunk * 16;
        const bool ok = s < slots && (unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W && n < a.N && chunk < nch && cb < a.Cs;
        const unsigned off = ok ? (unsigned)(((n * a.H + h) * a.W + w) * a.Cs + cb) : kOOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(lds + i * 4096 + wave * 1024), 16, off, 0, 0, 0);
    }
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();

    const int KS = a.ks;
    const int nsub = padu ? 1 : KS;
    const int RTW = a.R * a.TW, out_px = a.G * RTW;
    const int npg = (out_px + 31) >> 5;
    const int floor0 = a.relu0 ? 0 : INT32_MIN;

    for (int it = wave; it < nsub * a.psplit; it += 4) {        // wave-uniform
        const int j = it / a.psplit, pg0 = (it - j * a.psplit) * a.ipg;
        const int pgn = min(a.ipg, npg - pg0);                  // live pixel groups of the item (<= 0: none)
        if (pgn <= 0) continue;
        const int co = c0 + 32 * j;                             // first output channel of the subtile
        const int live = padu ? a.Cs - co : min(32, a.cg - 32 * j);

        // the lane's LDS byte address of tap (0, 0), kstep 0, per pixel group (padding lanes and groups: the tile's last pixel, result unused)
        unsigned ad[NPG];
#pragma unroll
        for (int pg = 0; pg < NPG; ++pg) {
            const int oc = min((pg0 + pg) * 32 + l31, out_px - 1);
            const int img = (int)fast_div((unsigned)oc, a.dRTW), orem = oc - img * RTW;
            const int orow = (int)fast_div((unsigned)orem, a.dTW), ocol = orem - orow * a.TW;
            ad[pg] = (unsigned)((img * IMG_PP + orow * S * a.PW + ocol) * a.pitch + 16 * lh);
        }

        v16i acc[NPG];
#pragma unroll
        for (int pg = 0; pg < NPG; ++pg)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[pg][r] = 0;

        // ---- (tap, kstep) outer, pixel groups inner; the next fragment is in flight under the MFMAs of the current one
        const int nf = 9 * KS;
        const v4i* wp = (const v4i*)a.w + (size_t)(gi * KS + j) * (size_t)(nf * 64) + lane;
        v4i cur = wp[0];
        int f = 0;
        for (int kr = 0; kr < 3; ++kr)
            for (int kc = 0; kc < 3; ++kc) {
                const unsigned toff = (unsigned)((kr * a.PW + (PWE_ON ? (kc & 1) * PWe + (kc >> 1) : kc)) * a.pitch);
                for (int ks = 0; ks < KS; ++ks) {
                    f = min(f + 1, nf - 1);                     // (the last step loads its own fragment again)
                    const v4i nxt = wp[f * 64];
                    const unsigned o = toff + 32 * ks;
#pragma unroll
                    for (int pg = 0; pg < NPG; ++pg) {
                        if (pg >= 4 && pg >= pgn) continue;     // wave-uniform: the lower four run unguarded (padding groups cost MFMAs, not branches)
                        const v4i xb = *(const v4i*)(lds + ad[pg] + o);
                        acc[pg] = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur, xb, acc[pg], 0, 0, 0);
                    }
                    cur = nxt;
                }
            }

        // ---- epilogue per pixel group: D register r of lane l = channel (r & 3) + 8 (r >> 2) + 4 (l >> 5) of pixel l & 31; rows past `live` are zero and unused
        const bool st16 = (co & 15) == 0;                       // wave-uniform: 16-byte int8 stores
#pragma unroll
        for (int pg = 0; pg < NPG; ++pg) {
            if (pg >= pgn) continue;                            // wave-uniform
            const int op = (pg0 + pg) * 32 + l31;
            const int oc = min(op, out_px - 1);
            const int img = (int)fast_div((unsigned)oc, a.dRTW), orem = oc - img * RTW;
            const int orow = (int)fast_div((unsigned)orem, a.dTW), ocol = orem - orow * a.TW;
            const int n = n0 + img, p = p0 + orow, q = q0 + ocol;
            const bool ok = op < out_px && n < a.N && p < a.P && q < a.Q;       // (edge tiles: rows / columns / images past the map / batch)
            const int32_t* bias = a.bias;
            if (a.ncc > 0) bias += (size_t)(a.rowcls[ok ? p : 0] * a.ncc + a.colcls[ok ? q : 0]) * (size_t)a.Cs;
            int y[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                v4i b = {0, 0, 0, 0};
                if (8 * g < live) b = *(const v4i*)(bias + co + 8 * g + 4 * lh);
#pragma unroll
                for (int e = 0; e < 4; ++e) y[g][e] = max((int)((unsigned)acc[pg][4 * g + e] + (unsigned)b[e]), floor0);
            }
            const int m = (n * a.P + p) * a.Q + q;
            if (a.out32 && ok) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (8 * g >= live) continue;                // wave-uniform
                    v4i o = {y[g][0], y[g][1], y[g][2], y[g][3]};
                    *(v4i*)(a.out32 + i32t_index(m, co + 8 * g + 4 * lh, a.Cs)) = o;
                }
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!a.q[k].ptr) continue;                      // wave-uniform
                unsigned d[4];
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    d[g] = requant_pack4(y[g][0], y[g][1], y[g][2], y[g][3], a.q[k]);
                // lane half 0 collects channels 0 .. 15 of its pixel, half 1 channels 16 .. 31
                auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
                auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
                if (!ok) continue;
                int8_t* dst = a.q[k].ptr + (size_t)m * a.Cs + co + 16 * lh;
                if (st16 && 16 * lh + 16 <= live) {
                    v4i o = {(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
                    *(v4i*)dst = o;
                } else {
                    if (16 * lh < live) { v2i o = {(int)s0[0], (int)s0[1]}; *(v2i*)dst = o; }
                    if (16 * lh + 8 < live) { v2i o = {(int)s1[0], (int)s1[1]}; *(v2i*)(dst + 8) = o; }
                }
            }
        }
    }
}

int gconvx_pitch(int cg) { return 32 * ((cg + 31) / 32) + 16; }

// gconv_tile's pitch-aware sibling.  TW output columns (Q split evenly into pieces of at most GX_TW_MAX whose three patch rows fit), R output rows (the
// most whose patch fits the LDS budget and whose R x TW pixels fit GX_NPG_MAX pixel groups (8; stride 2: 4), P split evenly) and — where one tile is the whole map — G
// images per workgroup up to that many pixels.  psplit: a subtile's pixel groups are dealt to the waves in this many parts — 2 or 4 where that shortens
// the longest wave (ceil(KS psplit / 4) / psplit subtile-tiles) and a part keeps at least four pixel groups, i.e. four MFMAs per fetched fragment.
void gconvx_tile(int P, int Q, int stride, int cg, int* R, int* TW, int* G, int* psplit) {
    const int S = stride == 2 ? 2 : 1, KS = (cg + 31) / 32;
    const int maxpp = GX_LDS_BUDGET / gconvx_pitch(cg);         // patch pixels: 240 (cg 232 .. 256) .. 585 (cg 72 .. 96)
    const int tw_max = std::min(GX_TW_MAX[S], (maxpp / 3 - 3) / S + 1);
    const int tiles_c = (Q + tw_max - 1) / tw_max;
    *TW = (Q + tiles_c - 1) / tiles_c;
    const int PW = (*TW - 1) * S + 3;
    const int r_max = std::max(1, std::min((maxpp / PW - 3) / S + 1, GX_NPG_MAX[S] * 32 / *TW));
    const int tiles_r = (P + r_max - 1) / r_max;
    *R = (P + tiles_r - 1) / tiles_r;
    *G = 1;
    if (tiles_c == 1 && tiles_r == 1) {
        const int PR = (*R - 1) * S + 3;
        *G = std::max(1, std::min(maxpp / (PR * PW), GX_NPG_MAX[S] * 32 / (P * Q)));
    }
    const int npg = (*G * *R * *TW + 31) / 32;
    *psplit = 1;
    for (int ps = 2; ps <= 4; ps *= 2)
        if ((npg + ps - 1) / ps >= 4 && ((KS * ps + 3) / 4) * *psplit < ((KS * *psplit + 3) / 4) * ps) *psplit = ps;
}

static int gconvx_lds_bytes(const GConvXArgs& a) { return (a.G * a.PR * a.PW * a.pitch + 1023) / 1024 * 1024; }       // whole 1 KB wave pieces

int gconvx_kernel_name(char* buf, size_t cap, const GConvXArgs& a) { return snprintf(buf, cap, "f8::gconvx3x3_kernel<%d, %d>", a.stride, a.ipg <= 4 ? 4 : 8); }

hipError_t launch_gconvx(const GConvXArgs& a, hipStream_t s) {
    if ((a.stride != 1 && a.stride != 2) || a.pad < 0 || a.pad > 1 || a.Cs % 32 || a.R < 1 || a.TW < 1 || a.G < 1 || a.tiles_r * a.R < a.P ||
        a.tiles_c * a.TW < a.Q || a.PR != (a.R - 1) * a.stride + 3 || a.PW != (a.TW - 1) * a.stride + 3 || a.pitch < 16 || a.pitch % 16 ||
        gconvx_lds_bytes(a) > GX_LDS_BUDGET || a.N < 1)
        return hipErrorInvalidValue;
    // the set, and what the kernel's addressing rests on: whole groups plus at most one pad unit up to Cs; every K32 read of a group at offset 0 or 8
    // of its span ends inside the pixel's pitch; bytes past the group meet zero weights (the packer), bytes past Cs / the image / N are the range check's
    const int C = a.groups * a.cg, npg = (a.G * a.R * a.TW + 31) / 32;
    if (a.cg % 8 || a.cg < 72 || a.cg > 256 || a.groups < 2 || C > a.Cs || a.Cs - C >= 32 || a.ks != (a.cg + 31) / 32 ||
        32 * a.ks > a.pitch || a.units != a.groups * a.ks + (a.Cs > C ? 1 : 0) ||
        (a.psplit != 1 && a.psplit != 2 && a.psplit != 4) || a.ipg < 1 || a.ipg > GX_NPG_MAX[a.stride] || a.ipg * a.psplit < npg)
        return hipErrorInvalidValue;
    const long grid = (long)((a.N + a.G - 1) / a.G) * a.tiles_r * a.tiles_c * (a.groups + (a.Cs > C ? 1 : 0));
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    auto k = a.stride == 2 ? gconvx3x3_kernel<2, 4> : a.ipg <= 4 ? gconvx3x3_kernel<1, 4> : gconvx3x3_kernel<1, 8>;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(256), gconvx_lds_bytes(a), s, a);
    return hipGetLastError();
}

}  // namespace f8
