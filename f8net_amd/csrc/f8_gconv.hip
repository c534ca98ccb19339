// f8_gconv.hip — grouped 3x3 convolution, "slice-diagonal" on v_mfma_i32_32x32x32_i8 (gfx950 only).
//
// The shapes: kernel 3, stride 1 / 2, pad 0 / 1, cin == cout == C, cg = C / groups in {2, 4, 8, 16, 32}; H, W, N at run time.  With NHWC int8 and the
// channels padded to 32, a group never straddles a 32-channel SLICE (cg divides 32), so output-channel tile t (32 channels) reads input slice t only:
// 32 bytes per pixel = ONE K32 step per tap.  The packer (f8_net.cpp pack_gconv_weights) writes every tap's 32 x 32 block block-diagonally, in
// MFMA-fragment order [slice][tap][lane][16 B] — the kernel has no notion of groups; padded channels carry zero weights.  9 MFMAs per (32 pixels x 32
// channels) output tile; the matrix cores run at cg / 32 of their rate (the zeros of the block diagonal), which at these shapes is beside the point:
// the launch moves its activations once.
//
//   * A workgroup (4 waves) owns a TILE — R output rows x TW output columns of one image, or G whole small images — x up to FOUR adjacent slices
//     (128 contiguous bytes per pixel).  Its haloed input patch, ((R - 1) S + 3) x ((TW - 1) S + 3) pixels x 128 B, is fetched ONCE by LDS-direct DMA;
//     out-of-image pixels, images past N and slices past Cs come back as zeros through the buffer range check (for unsigned — biased — inputs the
//     border-class bias table repairs them, as in conv_igemm_kernel).
//   * Wave w owns slice 4 * quad + w: its 9 weight fragments (36 VGPRs) stay in registers for the life of the workgroup; it walks the tile's
//     32-pixel groups, a tap is a constant LDS offset from the pixel's patch address, stride 2 reads every second patch pixel.
//   * Steady-state memory traffic: the patch in, the outputs out.
//
// Arithmetic is conv_igemm_kernel's: wrapping int32 accumulation, class bias, optional ReLU floor, the tiled int32 form and / or up to two
// requantised int8 forms — integer requantisation (requant1) whatever Options::requant_float says, as f8_dwk.hip / f8_irk.hip.  No residual join.
#include "f8_device.h"
#include <algorithm>

namespace f8 {

namespace {
constexpr int GC_LDS_BUDGET = 48 * 1024;            // patch bytes per workgroup: three workgroups (12 waves) per CU
constexpr int GC_TW_MAX[3] = {0, 64, 32};           // widest tile by stride: a one-row tile's patch (3 x 66 / 3 x 65 pixels) is 25 KB
constexpr int GC_PX_FILL = 256;                     // whole small images are gathered up to this many output pixels per workgroup
}

template <int S>
__global__ void __launch_bounds__(256) gconv3x3_kernel(const GConvArgs a) {
    using SW = Swz<128>;
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;
    const int l31 = lane & 31, lh = lane >> 5;

    // ---- this workgroup's tile: slice quad fastest (the quads of one tile read the same 128-byte-strided pixel rows)
    const int nquad = (a.Cs + 127) >> 7;
    const int quad = blockIdx.x % nquad;
    int t = blockIdx.x / nquad;
    const int tc = t % a.tiles_c; t /= a.tiles_c;
    const int tr = t % a.tiles_r;
    const int n0 = (t / a.tiles_r) * a.G;
    const int p0 = tr * a.R, q0 = tc * a.TW;
    const int IMG_PP = a.PR * a.PW;                             // patch pixels per image
    const int npp = a.G * IMG_PP;
    const int slots = npp * 8;                                  // 16-byte slots of the patch
    const int h0 = p0 * S - a.pad, w0 = q0 * S - a.pad;         // image position of patch pixel (0, 0)

    // ---- patch: every 16-byte slot once; chunk c of patch pixel r sits at chunk c ^ f(r) (SW), applied on the source side
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
    for (int i = 0; i * 256 + wave * 64 < slots; ++i) {         // wave-uniform bound
        const int s = i * 256 + tid;
        const int ppx = s >> 3, chunk = (s & 7) ^ SW::f(ppx);
        const int img = (int)fast_div((unsigned)ppx, a.dIPP), rem = ppx - img * IMG_PP;
        const int pr = (int)fast_div((unsigned)rem, a.dPW), pc = rem - pr * a.PW;
        const int h = h0 + pr, w = w0 + pc, n = n0 + img, cb = quad * 128 + chunk * 16;
        const bool ok = s < slots && (unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W && n < a.N && cb < a.Cs;
        const unsigned off = ok ? (unsigned)(((n * a.H + h) * a.W + w) * a.Cs + cb) : kOOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(lds + i * 4096 + wave * 1024), 16, off, 0, 0, 0);
    }

    // ---- this wave's slice: 9 weight fragments, resident
    const int slice = quad * 4 + wave;
    const bool live = slice * 32 < a.Cs;                        // wave-uniform (the last quad may hold fewer than four slices)
    v4i wf[9];
    if (live) {
        const v4i* wp = (const v4i*)a.w + (size_t)slice * (9 * 64) + lane;
#pragma unroll
        for (int k = 0; k < 9; ++k) wf[k] = wp[k * 64];
    }
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (!live) return;

    const int RTW = a.R * a.TW, out_px = a.G * RTW;
    const int floor0 = a.relu0 ? 0 : INT32_MIN;
    const int co = slice * 32;
    for (int pt = 0; pt * 32 < out_px; ++pt) {
        // output pixel of this lane inside the tile (padding lanes: the tile's last pixel, result unused)
        const int op = pt * 32 + l31;
        const int oc = op < out_px ? op : out_px - 1;
        const int img = (int)fast_div((unsigned)oc, a.dRTW), orem = oc - img * RTW;
        const int orow = (int)fast_div((unsigned)orem, a.dTW), ocol = orem - orow * a.TW;
        const int bpx = img * IMG_PP + orow * S * a.PW + ocol * S;              // patch pixel of tap (0, 0)
        const int n = n0 + img, p = p0 + orow, q = q0 + ocol;
        const bool ok = op < out_px && n < a.N && p < a.P && q < a.Q;           // (edge tiles: rows / columns / images past the map / batch)

        v16i acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int ppx = bpx + (k / 3) * a.PW + (k % 3);
            const v4i xb = *(const v4i*)(lds + SW::off(ppx, wave * 2 + lh));
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[k], xb, acc, 0, 0, 0);
        }

        // ---- epilogue: D register r of lane l = channel (r & 3) + 8 (r >> 2) + 4 (l >> 5) of pixel l & 31
        const int32_t* bias = a.bias;
        if (a.ncc > 0) bias += (size_t)(a.rowcls[ok ? p : 0] * a.ncc + a.colcls[ok ? q : 0]) * (size_t)a.Cs;
        int y[4][4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const v4i b = *(const v4i*)(bias + co + 8 * g + 4 * lh);
#pragma unroll
            for (int e = 0; e < 4; ++e) y[g][e] = max((int)((unsigned)acc[4 * g + e] + (unsigned)b[e]), floor0);
        }
        const int m = (n * a.P + p) * a.Q + q;
        if (a.out32 && ok) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                v4i o = {y[g][0], y[g][1], y[g][2], y[g][3]};
                *(v4i*)(a.out32 + i32t_index(m, co + 8 * g + 4 * lh, a.Cs)) = o;
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!a.q[k].ptr) continue;                          // wave-uniform
            unsigned d[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                d[g] = requant_pack4(y[g][0], y[g][1], y[g][2], y[g][3], a.q[k]);
            // lane half 0 collects channels 0 .. 15 of its pixel, half 1 channels 16 .. 31: one 16-byte store per lane
            auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
            auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
            if (ok) {
                v4i o = {(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
                *(v4i*)(a.q[k].ptr + (size_t)m * a.Cs + co + 16 * lh) = o;
            }
        }
    }
}

// The tile of a P x Q output map: TW output columns (Q split evenly into pieces of at most GC_TW_MAX), R output rows (the most whose patch fits the
// LDS budget, P split evenly), and — where one tile is the whole map — G images per workgroup, up to GC_PX_FILL output pixels.
void gconv_tile(int P, int Q, int stride, int* R, int* TW, int* G) {
    const int S = stride == 2 ? 2 : 1;
    const int tiles_c = (Q + GC_TW_MAX[S] - 1) / GC_TW_MAX[S];
    *TW = (Q + tiles_c - 1) / tiles_c;
    const int PW = (*TW - 1) * S + 3;
    const int pr_max = GC_LDS_BUDGET / (PW * 128);              // >= 3 by GC_TW_MAX
    const int r_max = std::max(1, (pr_max - 3) / S + 1);
    const int tiles_r = (P + r_max - 1) / r_max;
    *R = (P + tiles_r - 1) / tiles_r;
    *G = 1;
    if (tiles_c == 1 && tiles_r == 1) {
        const int PR = (*R - 1) * S + 3;
        const int fit = GC_LDS_BUDGET / (PR * PW * 128), want = (GC_PX_FILL + P * Q - 1) / (P * Q);
        *G = std::max(1, std::min(fit, want));
    }
}

static int gconv_lds_bytes(const GConvArgs& a) { return (a.G * a.PR * a.PW * 128 + 1023) / 1024 * 1024; }      // whole 1 KB wave pieces

int gconv_kernel_name(char* buf, size_t cap, const GConvArgs& a) { return snprintf(buf, cap, "f8::gconv3x3_kernel<%d>", a.stride); }

hipError_t launch_gconv(const GConvArgs& a, hipStream_t s) {
    if ((a.stride != 1 && a.stride != 2) || a.pad < 0 || a.pad > 1 || a.Cs % 32 || a.R < 1 || a.TW < 1 || a.G < 1 ||
        a.PR != (a.R - 1) * a.stride + 3 || a.PW != (a.TW - 1) * a.stride + 3 || gconv_lds_bytes(a) > 64 * 1024 || a.N < 1)
        return hipErrorInvalidValue;
    const long grid = (long)((a.N + a.G - 1) / a.G) * a.tiles_r * a.tiles_c * ((a.Cs + 127) / 128);
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    if (a.stride == 1) hipLaunchKernelGGL(gconv3x3_kernel<1>, dim3((unsigned)grid), dim3(256), gconv_lds_bytes(a), s, a);
    else hipLaunchKernelGGL(gconv3x3_kernel<2>, dim3((unsigned)grid), dim3(256), gconv_lds_bytes(a), s, a);
    return hipGetLastError();
}

}  // namespace f8
