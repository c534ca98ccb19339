// f8_gconvw.hip — grouped 3x3 convolution for group widths 24 .. 64, "group-aligned" on v_mfma_i32_32x32x32_i8 (gfx950 only).
//
// The shapes: kernel 3, stride 1 / 2, pad 0 / 1, cin == cout == C, cg = C / groups in {24, 40, 48, 56, 64}; H, W, N at run time; C a multiple of 8.
// f8_gconv.hip's slice-diagonal tiling needs a group inside one 32-channel slice; here a 32-output tile aligned to 32 would straddle two groups and
// read up to 128 input channels per tap (cg 56: outputs 32 .. 63 read inputs 0 .. 111).  So the tiling is aligned to GROUPS:
//
//   * A UNIT = one group g x one output subtile j of it: output channels g cg + 32 j .. + live - 1, live = min(32, cg - 32 j) (a multiple of 8);
//     input channels g cg .. g cg + 32 KS - 1, KS = ceil(cg / 32) K32 steps per tap (1 for cg 24, 2 for cg 40 .. 64; a group has KS subtiles).  The packer
//     (f8_net.cpp pack_gconvw_weights) writes zero weights for rows past `live` and input channels past the group's end, in MFMA-fragment order
//     [unit][tap][kstep][lane][16 B] — the kernel has no notion of groups.  The padded channels C .. Cs - 1 of the outputs are one more unit behind the
//     last group (co = C, live = Cs - C, all weights zero): same epilogue, no second code path.
//   * A workgroup (4 waves) = 4 consecutive units = UG = 4 / KS whole groups (cg 24: four groups, 96 channels; cg 40 .. 64: two groups x two
//     subtiles, 80 .. 128 channels) x f8_gconv.hip's tile (gconv_tile: R rows x TW columns of one image, or G whole small images).  Its input span
//     starts at channel wg UG cg — a multiple of 16 bytes for every cg of the set — so the haloed patch is fetched as there: 16-byte LDS-direct slots
//     at a 128-byte pixel pitch, Swz<128> on the source side, zero fill through the buffer range check, the border-class bias table for biased inputs.
//     Only the ceil(UG cg / 16) chunks that meet a non-zero weight are fetched (cg 40: 5 of 8); the other slots are written as zeros by the range check
//     and cost no traffic.  Every K32 read of every unit ends at or before byte 128 of the span.
//   * Wave w owns unit 4 wg + w: its 9 KS weight fragments (36 / 72 VGPRs) stay in registers for the life of the workgroup.  A unit's byte offset
//     inside the span, (w / KS) cg, is a multiple of 8: where it is a multiple of 16 (cg 48 / 64 always, every second group of cg 24) a lane's 16 K
//     bytes are one ds_read_b128, else two ds_read_b64 from two swizzled chunks — a wave-uniform choice made once, outside the pixel loop.
//   * Stores: only the `live` channels of a subtile.  int32: the tiled form, 16 bytes per lane and 8-channel group.  int8: the lane halves swap as in
//     f8_gconv.hip (half h holds channels 16 h .. + 15); 16 bytes per lane where the unit's channel base is a multiple of 16, else 8 bytes per lane
//     and 8-channel group.
//
// Arithmetic is gconv3x3_kernel's: wrapping int32 accumulation, class bias, optional ReLU floor, the tiled int32 form and / or up to two
// requantised int8 forms — integer requantisation (requant1) whatever Options::requant_float says.  No residual join.
#include "f8_device.h"

namespace f8 {

typedef int v2i __attribute__((ext_vector_type(2)));

template <int S, int KS>
__global__ void __launch_bounds__(256) gconvw3x3_kernel(const GConvWArgs a) {
    using SW = Swz<128>;
    constexpr int UG = 4 / KS;                                  // groups per workgroup
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;
    const int l31 = lane & 31, lh = lane >> 5;

    // ---- this workgroup's tile: unit quad fastest (the quads of one tile read neighbouring spans of the same pixel rows)
    const int nwg = (a.units + 3) >> 2;
    const int wg = blockIdx.x % nwg;
    int t = blockIdx.x / nwg;
    const int tc = t % a.tiles_c; t /= a.tiles_c;
    const int tr = t % a.tiles_r;
    const int n0 = (t / a.tiles_r) * a.G;
    const int p0 = tr * a.R, q0 = tc * a.TW;
    const int IMG_PP = a.PR * a.PW;                             // patch pixels per image
    const int npp = a.G * IMG_PP;
    const int slots = npp * 8;                                  // 16-byte slots of the patch
    const int h0 = p0 * S - a.pad, w0 = q0 * S - a.pad;         // image position of patch pixel (0, 0)
    const int span = wg * UG * a.cg;                            // first input channel of the workgroup: a multiple of 16

    // ---- patch: every 16-byte slot once; chunk c of patch pixel r sits at chunk c ^ f(r) (SW), applied on the source side.  Chunks past nch meet
    //      zero weights only: not fetched (the range check writes zeros)
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
    for (int i = 0; i * 256 + wave * 64 < slots; ++i) {         // wave-uniform bound
        const int s = i * 256 + tid;
        const int ppx = s >> 3, chunk = (s & 7) ^ SW::f(ppx);
        const int img = (int)fast_div((unsigned)ppx, a.dIPP), rem = ppx - img * IMG_PP;
        const int pr = (int)fast_div((unsigned)rem, a.dPW), pc = rem - pr * a.PW;
        const int h = h0 + pr, w = w0 + pc, n = n0 + img, cb = span + chunk * 16;
        const bool ok = s < slots && (unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W && n < a.N && chunk < a.nch && cb < a.Cs;
        const unsigned off = ok ? (unsigned)(((n * a.H + h) * a.W + w) * a.Cs + cb) : kOOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(lds + i * 4096 + wave * 1024), 16, off, 0, 0, 0);
    }

    // ---- this wave's unit: 9 KS weight fragments, resident
    const int unit = wg * 4 + wave;
    const bool ulive = unit < a.units;                          // wave-uniform (the last quad may hold fewer than four units)
    const int gl = wave / KS, j = wave % KS;                    // group inside the workgroup, subtile inside the group
    const int uoff = gl * a.cg;                                 // the unit's first input byte inside the span: a multiple of 8
    const int co = (wg * UG + gl) * a.cg + 32 * j;              // its first output channel (the pad unit: C)
    const int live = min(min(32, a.cg - 32 * j), a.Cs - co);    // its output channels: 8 .. 32, a multiple of 8
    v4i wf[9 * KS];
    if (ulive) {
        const v4i* wp = (const v4i*)a.w + (size_t)unit * (9 * KS * 64) + lane;
#pragma unroll
        for (int k = 0; k < 9 * KS; ++k) wf[k] = wp[k * 64];
    }
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (!ulive) return;

    const int RTW = a.R * a.TW, out_px = a.G * RTW;
    const int floor0 = a.relu0 ? 0 : INT32_MIN;
    const bool st16 = (co & 15) == 0;                           // wave-uniform: 16-byte int8 stores
    // SPLIT: the unit's bytes start in the middle of a 16-byte chunk (wave-uniform, chosen once below)
    auto run = [&](auto split) {
        constexpr bool SPLIT = decltype(split)::value;
        for (int pt = 0; pt * 32 < out_px; ++pt) {
            // output pixel of this lane inside the tile (padding lanes: the tile's last pixel, result unused)
            const int op = pt * 32 + l31;
            const int oc = op < out_px ? op : out_px - 1;
            const int img = (int)fast_div((unsigned)oc, a.dRTW), orem = oc - img * RTW;
            const int orow = (int)fast_div((unsigned)orem, a.dTW), ocol = orem - orow * a.TW;
            const int bpx = img * IMG_PP + orow * S * a.PW + ocol * S;          // patch pixel of tap (0, 0)
            const int n = n0 + img, p = p0 + orow, q = q0 + ocol;
            const bool ok = op < out_px && n < a.N && p < a.P && q < a.Q;       // (edge tiles: rows / columns / images past the map / batch)

            v16i acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int ppx = bpx + (k / 3) * a.PW + (k % 3);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const int c = (uoff >> 4) + 2 * ks + lh;                    // the chunk of the lane's first K byte (SPLIT: its upper half)
                    v4i xb;
                    if constexpr (SPLIT) {
                        const v2i lo = *(const v2i*)(lds + SW::off(ppx, c) + 8);
                        const v2i hi = *(const v2i*)(lds + SW::off(ppx, c + 1));
                        xb = v4i{lo[0], lo[1], hi[0], hi[1]};
                    } else {
                        xb = *(const v4i*)(lds + SW::off(ppx, c));
                    }
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[k * KS + ks], xb, acc, 0, 0, 0);
                }
            }

            // ---- epilogue: D register r of lane l = channel (r & 3) + 8 (r >> 2) + 4 (l >> 5) of pixel l & 31; rows past `live` are zero and unused
            const int32_t* bias = a.bias;
            if (a.ncc > 0) bias += (size_t)(a.rowcls[ok ? p : 0] * a.ncc + a.colcls[ok ? q : 0]) * (size_t)a.Cs;
            int y[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                v4i b = {0, 0, 0, 0};
                if (8 * g < live) b = *(const v4i*)(bias + co + 8 * g + 4 * lh);
#pragma unroll
                for (int e = 0; e < 4; ++e) y[g][e] = max((int)((unsigned)acc[4 * g + e] + (unsigned)b[e]), floor0);
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
    };
    if (uoff & 8) run(std::true_type{}); else run(std::false_type{});
}

static int gconvw_lds_bytes(const GConvWArgs& a) { return (a.G * a.PR * a.PW * 128 + 1023) / 1024 * 1024; }    // whole 1 KB wave pieces

int gconvw_kernel_name(char* buf, size_t cap, const GConvWArgs& a) { return snprintf(buf, cap, "f8::gconvw3x3_kernel<%d, %d>", a.stride, (a.cg + 31) / 32); }

hipError_t launch_gconvw(const GConvWArgs& a, hipStream_t s) {
    const int KS = (a.cg + 31) / 32, UG = 4 / KS;
    if ((a.stride != 1 && a.stride != 2) || a.pad < 0 || a.pad > 1 || a.Cs % 32 || a.R < 1 || a.TW < 1 || a.G < 1 ||
        a.PR != (a.R - 1) * a.stride + 3 || a.PW != (a.TW - 1) * a.stride + 3 || gconvw_lds_bytes(a) > 64 * 1024 || a.N < 1)
        return hipErrorInvalidValue;
    // the set, and what the kernel's addressing rests on: whole groups plus at most one pad unit up to Cs; every unit's reads inside the 128-byte span
    const int C = a.groups * a.cg;
    if ((a.cg != 24 && a.cg != 40 && a.cg != 48 && a.cg != 56 && a.cg != 64) || a.groups < 1 || C > a.Cs || a.Cs - C >= 32 ||
        a.units != a.groups * KS + (a.Cs > C ? 1 : 0) || (UG - 1) * a.cg + 32 * KS > 128 || a.nch != (UG * a.cg + 15) / 16)
        return hipErrorInvalidValue;
    const long grid = (long)((a.N + a.G - 1) / a.G) * a.tiles_r * a.tiles_c * ((a.units + 3) / 4);
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    auto k = a.stride == 1 ? (KS == 1 ? gconvw3x3_kernel<1, 1> : gconvw3x3_kernel<1, 2>) : (KS == 1 ? gconvw3x3_kernel<2, 1> : gconvw3x3_kernel<2, 2>);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(256), gconvw_lds_bytes(a), s, a);
    return hipGetLastError();
}

}  // namespace f8
