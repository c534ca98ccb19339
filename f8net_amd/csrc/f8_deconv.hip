// f8_deconv.hip — transposed convolution, stride 2 .. 4, on v_mfma_i32_32x32x32_i8 (gfx950 only).
//
// out[n, co, oh, ow] = b[co] + sum x[n, ci, ih, iw] w[ci, co, kh, kw] over the taps with oh + pad - kh = s ih, ow + pad - kw = s iw (include/f8net.h).
// The output pixels of one PHASE (rh, rw) = ((oh + pad) % s, (ow + pad) % s) all see the same taps, kh = rh + s th (th < Th) at the input row ih = a - th
// with oh = s a + rh - pad: one phase is a plain implicit GEMM over its sub-grid of the output, K = Th * Tw * CK, and its weights are packed as one
// matrix [coutP][Th * Tw * CK] in MFMA-fragment order, a coalesced 1 KB per wave load (f8_net.cpp pack_deconv_weights).  No zero is ever multiplied: the launch does H W k^2 cin cout multiply-adds.
//
//   * Work item of a wave = (64 phase pixels, phase, CT cout tiles of 32): 2 x CT accumulator blocks, so that a weight fragment fetched feeds two MFMAs and
//     a pixel fragment CT of them.  The pixels of an MFMA tile belong to ONE phase, so the tap set — the K loop's trip
//     count — is wave-uniform.  A workgroup's four waves are neighbouring cout groups of one pixel tile (up to four), else neighbouring pixel tiles.
//     No LDS, no barrier: both operands are fetched as MFMA fragments straight into registers (16 B per lane, K-contiguous — whatever the hardware's
//     k order is, it is the same for A and B), one K32 step ahead of the multiply; the waves of a SIMD hide the rest of the latency.
//   * Out-of-image taps (ih or iw outside the map), pixels past the phase's last, cout tiles past coutP and the step fetched past the K loop's end come
//     back as zeros through the buffer range check.  Unsigned inputs are stored biased (x ^ 0x80) as everywhere: the border-class bias table, indexed
//     by the class of the OUTPUT row and column, adds 128 * sum(w) over exactly the taps that met an in-image pixel (classes exist at pad 0 too;
//     mask 0 = bias only).
//   * Logical work items are ordered cout group fastest, then phase, then pixel tile, and dealt to the XCDs in contiguous runs (the bijective remap of
//     f8_wreg.hip): the cout tiles of a pixel tile and the s^2 phases of one input region, which read the same input rows, share an L2.
//   * Epilogue as gconv3x3_kernel: class bias, ReLU floor, the tiled int32 form and / or up to two requantised int8 forms (integer requantisation,
//     requant1, whatever Options::requant_float says), 16-byte int8 rows per lane.  The output pixel of a lane is (n, s a + rh - pad, s c + rw - pad):
//     neighbouring lanes are s pixels apart, so the I32T stores are 16-byte pieces, not 1 KB runs.
#include "f8_device.h"
#include <algorithm>

namespace f8 {

namespace {
// waves of a workgroup along cout for ncg cout groups (a power of two; the other 4 / wct waves take neighbouring pixel tiles)
__host__ __device__ inline int deconv_wct(int ncg) { return ncg >= 4 ? 4 : ncg >= 2 ? 2 : 1; }
}

template <int CT>
__global__ void __launch_bounds__(256) deconv_kernel(const DeconvArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;
    const int l31 = lane & 31, lh = lane >> 5;

    int t;
    {   // XCD-aware order (bijective): consecutive logical items on one XCD
        const int nwg = gridDim.x, bid = blockIdx.x, xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
        t = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
    }
    const int nct = a.coutP >> 5;                                  // cout tiles
    const int ncg = (nct + CT - 1) / CT;                           // cout groups (a wave's CT tiles)
    const int wct = deconv_wct(ncg);
    const int nbg = (ncg + wct - 1) / wct;
    const int cgb = t % nbg; t /= nbg;
    const int pi = t % a.nph, tg = t / a.nph;
    const int cg = cgb * wct + (wave & (wct - 1));
    const int tile = tg * (4 / wct) + wave / wct;                  // 64 phase pixels
    if (cg >= ncg) return;                                          // (wave-uniform; no barrier below)
    const DeconvPhase& ph = a.ph[pi];
    const int AC = ph.A * ph.Cn, Mph = a.N * AC;
    if (tile * 64 >= Mph) return;

    // ---- this lane's two pixels of the phase
    bool live[2]; int n[2], pa[2], pc[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int mp = tile * 64 + p * 32 + l31;
        live[p] = mp < Mph;
        const int mc = live[p] ? mp : Mph - 1;
        n[p] = (int)fast_div((unsigned)mc, ph.dAC);
        const int rem = mc - n[p] * AC;
        const int ai = (int)fast_div((unsigned)rem, ph.dC);
        pa[p] = ph.a0 + ai; pc[p] = ph.c0 + (rem - ai * ph.Cn);
    }

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, a.w_bytes, 0x00020000);
    const int nch = a.CK >> 5;                                      // K32 steps per tap
    const int nk = ph.Th * ph.Tw * nch;
    unsigned wbase[CT];                                             // kOOB: a cout tile past coutP (the last group of an odd tile count)
#pragma unroll
    for (int c = 0; c < CT; ++c)
        wbase[c] = (cg * CT + c) < nct ? ph.w_off + (unsigned)((cg * CT + c) * nk) * 1024u + (unsigned)(lane * 16) : kOOB;      // fragment order: [tile][K32 step][lane][16 B]
    const unsigned xlane = (unsigned)(lh * 16);
    // byte offset of tap (th, tw) at this lane's pixel p, kOOB outside the image
    auto tap_off = [&](int p, int th, int tw) -> unsigned {
        const int ih = pa[p] - th, iw = pc[p] - tw;
        const bool ok = live[p] && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
        return ok ? (unsigned)(((n[p] * a.H + ih) * a.W + iw) * a.CK) + xlane : kOOB;
    };

    v16i acc[2][CT];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[p][c][r] = 0;
    int th = 0, tw = 0, ch = 0;
    unsigned xo[2];
    v4i xb[2], wb[CT];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        xo[p] = nk > 0 ? tap_off(p, 0, 0) : kOOB;
        xb[p] = __builtin_amdgcn_raw_buffer_load_b128(rx, xo[p], 0, 0);
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) wb[c] = __builtin_amdgcn_raw_buffer_load_b128(rw, nk > 0 ? wbase[c] : kOOB, 0, 0);
    for (int j = 0; j < nk; ++j) {
        // the next step's operands (past the end: zeros, never multiplied)
        if (++ch == nch) {
            ch = 0;
            if (++tw == ph.Tw) { tw = 0; ++th; }
#pragma unroll
            for (int p = 0; p < 2; ++p) xo[p] = tap_off(p, th, tw);
        }
        const bool more = j + 1 < nk;
        v4i xn[2], wn[CT];
#pragma unroll
        for (int p = 0; p < 2; ++p) xn[p] = __builtin_amdgcn_raw_buffer_load_b128(rx, (more && xo[p] != kOOB) ? xo[p] + (unsigned)(ch * 32) : kOOB, 0, 0);
#pragma unroll
        for (int c = 0; c < CT; ++c) wn[c] = __builtin_amdgcn_raw_buffer_load_b128(rw, (more && wbase[c] != kOOB) ? wbase[c] + (unsigned)(j + 1) * 1024u : kOOB, 0, 0);
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[p][c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wb[c], xb[p], acc[p][c], 0, 0, 0);
#pragma unroll
        for (int p = 0; p < 2; ++p) xb[p] = xn[p];
#pragma unroll
        for (int c = 0; c < CT; ++c) wb[c] = wn[c];
    }

    // ---- epilogue: D register r of lane l = channel (r & 3) + 8 (r >> 2) + 4 (l >> 5) of pixel l & 31
    const int floor0 = a.relu0 ? 0 : INT32_MIN;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (tile * 64 + p * 32 >= Mph) continue;                    // (wave-uniform: the second pixel tile lies past the phase's last pixel)
        const int oh = a.stride * pa[p] + ph.rh - a.pad, ow = a.stride * pc[p] + ph.rw - a.pad;      // inside [0, P) x [0, Q) by the sub-grid's construction
        const int32_t* bias = a.bias;
        if (a.ncc > 0) bias += (size_t)(a.rowcls[oh] * a.ncc + a.colcls[ow]) * (size_t)a.coutP;
        const int m = (n[p] * a.P + oh) * a.Q + ow;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if ((cg * CT + c) >= nct) continue;                     // (wave-uniform)
            const int co = (cg * CT + c) * 32;
            int y[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const v4i b = *(const v4i*)(bias + co + 8 * g + 4 * lh);
#pragma unroll
                for (int e = 0; e < 4; ++e) y[g][e] = max((int)((unsigned)acc[p][c][4 * g + e] + (unsigned)b[e]), floor0);
            }
            if (a.out32 && live[p]) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    v4i o = {y[g][0], y[g][1], y[g][2], y[g][3]};
                    *(v4i*)(a.out32 + i32t_index(m, co + 8 * g + 4 * lh, a.coutP)) = o;
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
                if (live[p]) {
                    v4i o = {(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
                    *(v4i*)(a.q[k].ptr + (size_t)m * a.coutP + co + 16 * lh) = o;
                }
            }
        }
    }
}

// The instance: CT = 2 cout tiles per wave where there are two (coutP >= 64), else 1
int deconv_inst(const DeconvArgs& a) { return a.coutP >= 64 ? 2 : 1; }
const char* deconv_kernel_name(int inst) { return inst == 2 ? "f8::deconv_kernel<2>" : "f8::deconv_kernel<1>"; }

hipError_t launch_deconv(const DeconvArgs& a0, int inst, hipStream_t s) {
    DeconvArgs a = a0;
    if (a.N < 1 || a.nph < 1 || a.nph > kMaxDeconvPhases || a.nph != a.stride * a.stride || a.CK % 32 || a.coutP % 32 || a.CK < 32 || a.coutP < 32 ||
        (inst != 1 && inst != 2)) return hipErrorInvalidValue;
    long px = 0;                                                    // pixels of the largest phase
    for (int i = 0; i < a.nph; ++i) {
        const DeconvPhase& p = a.ph[i];
        if (p.A < 0 || p.Cn < 0 || p.Th < 0 || p.Tw < 0) return hipErrorInvalidValue;
        // every pixel of the sub-grid is an output pixel: the epilogue indexes the class tables and the output forms with it unchecked
        if (p.A > 0 && p.Cn > 0 && (a.stride * p.a0 + p.rh - a.pad < 0 || a.stride * (p.a0 + p.A - 1) + p.rh - a.pad >= a.P ||
                                     a.stride * p.c0 + p.rw - a.pad < 0 || a.stride * (p.c0 + p.Cn - 1) + p.rw - a.pad >= a.Q)) return hipErrorInvalidValue;
        px = std::max(px, (long)a.N * p.A * p.Cn);
    }
    if (px < 1 || px > 0x7fffffffL) return hipErrorInvalidValue;
    const int nct = a.coutP / 32, ncg = (nct + inst - 1) / inst, wct = deconv_wct(ncg);
    a.tiles = (int)((px + 63) / 64);
    const long tgs = (a.tiles + 4 / wct - 1) / (4 / wct);
    const long grid = tgs * a.nph * ((ncg + wct - 1) / wct);
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    if (inst == 2) hipLaunchKernelGGL(deconv_kernel<2>, dim3((unsigned)grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(deconv_kernel<1>, dim3((unsigned)grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace f8
