// f8_dwdeconv.hip — depthwise transposed convolution (gfx950): f8_net_conv_transpose with groups == cin == cout under option dw_deconv, kernel 1 .. 16,
// stride 2 .. 8, pad 0 .. kernel - 1.  VALU (the arithmetic intensity is k^2 / s^2 multiply-adds per output byte: nothing for MFMA); a launch of its own
// (S_DWDECONV, f8_net.cpp).
//
//   out[n, c, oh, ow] = b[c] + sum x[n, c, ih, iw] w[c, 0, kh, kw] over the taps with oh + pad - kh = s ih, ow + pad - kw = s iw (include/f8net.h).
//
// With oh = s a + rh - pad (ANCHOR row a = (oh + pad) / s, PHASE row rh = (oh + pad) % s) the taps of an output row are kh = rh + s th at the input row
// ih = a - th, th < T = ceil(k / s); the same for the columns.  Both kernels work in the stored domain of f8_dwk.hip: NHWC int8 with channel stride Cs (a
// multiple of 32); unsigned tensors are stored biased (x ^ 0x80); wrapping int32 accumulation; optional ReLU floor; up to two int8 forms (QuantOut) and / or
// the tiled int32 form; integer requantisation (requant1) whatever Options::requant_float says.
//
//   dwdeconv_kernel<SIGNED_IN>   k, s, pad at run time; one thread = one OUTPUT pixel x 4 channels; tap loops over th, tw, bytes multiplied one by one
//                                (unsigned inputs as unsigned bytes: out-of-image taps are skipped, plain bias).  Writes any form.  The correctness anchor, and
//                                what runs when a launch writes the int32 form, when T > 4, under dwk_dot4 = 0 and under dw_deconv = 2.
//   dwdeconv_dot4_kernel<T>      int8 forms only, T <= 4, on v_dot4_i32_i8, INPUT-anchored.  All s^2 phases of anchor (a, c) read the same T x T input
//                                neighbourhood x[a - th][c - tw] against different weights w[rh + s th][rw + s tw]: a phase is a T x T depthwise correlation.
//                                One thread = 4 channels x DWD_PIX adjacent anchor columns c0 .. c0 + 3 of one anchor row a.  It walks its DWD_PIX + T - 1
//                                input columns c0 - (T - 1) .. c0 + 3 ONCE: per column T dwords (rows a .. a - T + 1, 4 channels each; outside the image —
//                                anchors at or past H included, k > s — the biased zero), byte-transposed with v_perm_b32 into one dword per channel, byte j =
//                                row a - j (the scheme of dwconvk_dot4_kernel; T = 1: three shifts, T = 2: two v_perm_b32 and two shifts, else eight).  The
//                                (DWD_PIX + T - 1) x 4 transposed dwords stay in registers across the loops over the phases (rh, rw): a phase loads its T x 4
//                                weight dwords, runs DWD_PIX x T x 4 dot4 into 16 accumulators that start at the phase's bias, requantises and stores its
//                                DWD_PIX pixels (oh, s (c0 + j) + rw - pad).  Per output value of 4 channels: 4 T dot4 for 4 T^2 multiply-add slots, and
//                                (T loads + the transposes) (DWD_PIX + T - 1) / (DWD_PIX s^2) of the input side — at 4x4 / 2: 0.6 loads per output pixel
//                                where the output-anchored kernel issues 4.  Output pixels outside [0, P) x [0, Q) are computed and not stored.  Lanes run
//                                fastest over the channel quads: a pixel's channel row is one contiguous store, and a phase's weight dwords one contiguous load.
//                                Weights: pack_dwdeconv_weights' image (f8_net.cpp) [s^2 phases][T columns][Cs / 4][4 channels] dwords, byte j of
//                                (rh s + rw, tw, quad, e) = w[4 quad + e][rh + s j][rw + s tw], 0 where that kernel row or column is >= k; read through L1
//                                (a workgroup's slice is at most 64 quads x 16 B per phase and column and every wave of the workgroup reads the same one).
//                                Bias: [s^2][Cs], b[c] + 128 x the sum of the phase's taps for unsigned inputs.  A phase without a tap (k <= rh or k <= rw)
//                                meets zero weights and stores its bias.
#include "f8_device.h"
#include <algorithm>

namespace f8 {

namespace {
constexpr int DWD_PIX = 4;                          // adjacent anchor columns per thread of the dot4 kernel
}

template <bool SIGNED_IN>
__global__ void __launch_bounds__(256) dwdeconv_kernel(const DwDeconvArgs a) {
    const int cgs = a.Cs >> 2;
    const size_t total = (size_t)a.N * a.P * a.Q * cgs;
    const int T = (a.k + a.stride - 1) / a.stride;
    const unsigned in_xor = SIGNED_IN ? 0u : 0x80808080u;   // unsigned tensors are stored biased
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int cg = (int)(idx % cgs);
        size_t m = idx / cgs;
        const int q = (int)(m % a.Q); m /= a.Q;
        const int p = (int)(m % a.P);
        const int n = (int)(m / a.P);
        const int c = cg << 2;
        int acc[4];
        {
            const v4i b = *(const v4i*)(a.bias + c);
            acc[0] = b.x; acc[1] = b.y; acc[2] = b.z; acc[3] = b.w;
        }
        const int ah = (p + a.pad) / a.stride, rh = (p + a.pad) - ah * a.stride;      // anchor and phase, per axis
        const int aw = (q + a.pad) / a.stride, rw = (q + a.pad) - aw * a.stride;
        for (int th = 0; th < T; ++th) {
            const int kh = rh + a.stride * th, h = ah - th;
            if (kh >= a.k || (unsigned)h >= (unsigned)a.H) continue;
            for (int tw = 0; tw < T; ++tw) {
                const int kw = rw + a.stride * tw, w = aw - tw;
                if (kw >= a.k || (unsigned)w >= (unsigned)a.W) continue;
                const unsigned xv = *(const unsigned*)(a.x + (((size_t)n * a.H + h) * a.W + w) * a.Cs + c) ^ in_xor;
                const unsigned wv = *(const unsigned*)(a.w + (size_t)(kh * a.k + kw) * a.Cs + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int xe = SIGNED_IN ? (int)(signed char)(xv >> (8 * e)) : (int)((xv >> (8 * e)) & 0xffu);
                    const int we = (int)(signed char)(wv >> (8 * e));
                    acc[e] = (int)((unsigned)acc[e] + (unsigned)(xe * we));
                }
            }
        }
        if (a.relu0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = max(acc[e], 0);
        }
        const int mo = (n * a.P + p) * a.Q + q;
        const size_t o = (size_t)mo * a.Cs + c;
        if (a.out32) { v4i v = {acc[0], acc[1], acc[2], acc[3]}; *(v4i*)(a.out32 + i32t_index(mo, c, a.Cs)) = v; }
#pragma unroll
        for (int f = 0; f < 2; ++f)
            if (a.q[f].ptr) *(unsigned*)(a.q[f].ptr + o) = requant_pack4(acc[0], acc[1], acc[2], acc[3], a.q[f]);
    }
}

template <int T>
__global__ void __launch_bounds__(256) dwdeconv_dot4_kernel(const DwDeconvArgs a) {
    constexpr int PIX = DWD_PIX, NCOL = PIX + T - 1;  // input columns c0 - (T - 1) .. c0 + PIX - 1
    static_assert(T >= 1 && T <= 4, "a dot4 reduces over the T <= 4 rows of a phase");
    const int s = a.stride;
    const int cgs = a.Cs >> 2;                        // 4-channel quads
    const int A = (a.P - 1 + a.pad) / s + 1;          // anchor rows / columns that own an output pixel
    const int NG = ((a.Q - 1 + a.pad) / s + PIX) / PIX;
    const size_t total = (size_t)a.N * A * NG * cgs;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int cg = (int)(idx % cgs);
    size_t st = idx / cgs;
    const int g = (int)(st % NG); st /= NG;
    const int ar = (int)(st % A);
    const int n = (int)(st / A);
    const int c = cg << 2, c0 = g * PIX;
    const unsigned padv = a.in_signed ? 0u : 0x80808080u;

    // ---- the thread's input columns, transposed: col[cc][e] = channel c + e of column c0 - (T - 1) + cc, byte j = row ar - j
    unsigned col[NCOL][4];
    const int8_t* const xn = a.x + (size_t)n * a.H * a.W * a.Cs + c;
#pragma unroll
    for (int cc = 0; cc < NCOL; ++cc) {
        const int w = c0 - (T - 1) + cc;
        const bool wok = (unsigned)w < (unsigned)a.W;
        unsigned t[T];
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int h = ar - j;
            unsigned v = padv;
            if (wok && (unsigned)h < (unsigned)a.H) v = *(const unsigned*)(xn + ((size_t)h * a.W + w) * a.Cs);
            t[j] = v;
        }
        if constexpr (T == 1) {                       // one row: byte 0; the other slots meet zero weights and may hold anything
            col[cc][0] = t[0]; col[cc][1] = t[0] >> 8; col[cc][2] = t[0] >> 16; col[cc][3] = t[0] >> 24;
        } else if constexpr (T == 2) {                // two rows: bytes 0, 1
            const unsigned lo01 = __builtin_amdgcn_perm(t[1], t[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(t[1], t[0], 0x07030602u);
            col[cc][0] = lo01; col[cc][1] = lo01 >> 16; col[cc][2] = hi01; col[cc][3] = hi01 >> 16;
        } else {
            const unsigned t3 = T == 4 ? t[T - 1] : t[2];                                    // (three rows: slot 3 meets a zero weight)
            const unsigned lo01 = __builtin_amdgcn_perm(t[1], t[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(t[1], t[0], 0x07030602u);
            const unsigned lo23 = __builtin_amdgcn_perm(t3, t[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(t3, t[2], 0x07030602u);
            col[cc][0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u); col[cc][1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
            col[cc][2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u); col[cc][3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
        }
    }

    // ---- the s^2 phases of the thread's anchors against those columns
    const int floor0 = a.relu0 ? 0 : INT32_MIN;
    const v4i* const wq = (const v4i*)a.w4 + cg;      // [phase][column tw][quad]
    int8_t* const q0 = a.q[0].ptr, * const q1 = a.q[1].ptr;
    for (int rh = 0; rh < s; ++rh) {
        const int oh = s * ar + rh - a.pad;
        if ((unsigned)oh >= (unsigned)a.P) continue;
        const size_t orow = ((size_t)n * a.P + oh) * a.Q;
        for (int rw = 0; rw < s; ++rw) {
            const int ph = rh * s + rw;
            v4i wv[T];
#pragma unroll
            for (int tw = 0; tw < T; ++tw) wv[tw] = wq[(size_t)(ph * T + tw) * cgs];
            const v4i bv = *(const v4i*)(a.bias4 + (size_t)ph * a.Cs + c);
#pragma unroll
            for (int j = 0; j < PIX; ++j) {
                int acc0 = bv.x, acc1 = bv.y, acc2 = bv.z, acc3 = bv.w;
#pragma unroll
                for (int tw = 0; tw < T; ++tw) {      // anchor column c0 + j meets kernel column rw + s tw at input column c0 + j - tw
                    const int cc = j - tw + T - 1;
                    acc0 = __builtin_amdgcn_sdot4((int)col[cc][0], wv[tw].x, acc0, false);
                    acc1 = __builtin_amdgcn_sdot4((int)col[cc][1], wv[tw].y, acc1, false);
                    acc2 = __builtin_amdgcn_sdot4((int)col[cc][2], wv[tw].z, acc2, false);
                    acc3 = __builtin_amdgcn_sdot4((int)col[cc][3], wv[tw].w, acc3, false);
                }
                const int ow = s * (c0 + j) + rw - a.pad;
                if ((unsigned)ow >= (unsigned)a.Q) continue;
                acc0 = max(acc0, floor0); acc1 = max(acc1, floor0); acc2 = max(acc2, floor0); acc3 = max(acc3, floor0);
                const size_t off = (orow + ow) * a.Cs + c;
                if (q0) *(unsigned*)(q0 + off) = requant_pack4(acc0, acc1, acc2, acc3, a.q[0]);
                if (q1) *(unsigned*)(q1 + off) = requant_pack4(acc0, acc1, acc2, acc3, a.q[1]);
            }
        }
    }
}

// Does dw_deconv = 1 plan the dot4 kernel for a launch it can serve?  Everywhere: on the five DLA-34 shapes of profiles/dwdeconv_r25.md (batch 128) it was
// 3.1 .. 3.9x faster than dwdeconv_kernel and 1.5 .. 7.5x faster than the dense deconv_kernel over diagonal-expanded weights, at 1.30 .. 1.51x the time of a
// device copy of the output's bytes; no shape lost, so no shape is kept off it.
static bool dwdeconv_rule(const DwDeconvArgs&, int /*nq*/) { return true; }

// The instance: 0 = dwdeconv_kernel<in_signed>; T = 1 .. 4 = dwdeconv_dot4_kernel<T> — int8 forms only, T = ceil(k / s) <= 4, Options::dwk_dot4, and
// Options::dw_deconv == 1 (`mode`; 2 plans the anchor everywhere).
int dwdeconv_inst(const DwDeconvArgs& a, bool out32, int nq, bool dot4, int mode) {
    const int T = (a.k + a.stride - 1) / a.stride;
    return dot4 && mode == 1 && !out32 && nq >= 1 && T <= 4 && dwdeconv_rule(a, nq) ? T : 0;
}

int dwdeconv_kernel_name(char* buf, size_t cap, const DwDeconvArgs& a, int inst) {
    if (inst) return snprintf(buf, cap, "f8::dwdeconv_dot4_kernel<%d>", inst);
    return snprintf(buf, cap, "f8::dwdeconv_kernel<%s>", a.in_signed ? "true" : "false");
}

hipError_t launch_dwdeconv(const DwDeconvArgs& a, int inst, hipStream_t s) {
    const int T = a.stride > 0 ? (a.k + a.stride - 1) / a.stride : 0;
    if (a.N < 1 || a.k < 1 || a.k > 16 || a.stride < 2 || a.stride > 8 || a.pad < 0 || a.pad >= a.k || a.Cs < 32 || a.Cs % 32 || a.H < 1 || a.W < 1 || a.P < 1 ||
        a.Q < 1 || a.P > (a.H - 1) * a.stride - 2 * a.pad + a.k + a.stride - 1 || a.Q > (a.W - 1) * a.stride - 2 * a.pad + a.k + a.stride - 1 ||
        (inst != 0 && inst != T) || inst > 4)
        return hipErrorInvalidValue;
    if (inst) {
        if (a.out32 || !a.w4 || !a.bias4) return hipErrorInvalidValue;
        const size_t A = (size_t)(a.P - 1 + a.pad) / a.stride + 1, NG = ((size_t)(a.Q - 1 + a.pad) / a.stride + DWD_PIX) / DWD_PIX;
        const size_t work = (size_t)a.N * A * NG * (a.Cs >> 2);
        if ((work + 255) / 256 > 0x7fffffffu) return hipErrorInvalidValue;
        const unsigned grid = (unsigned)((work + 255) / 256);
        switch (inst) {
#define F8_DWD(T_) case T_: hipLaunchKernelGGL((dwdeconv_dot4_kernel<T_>), dim3(grid), dim3(256), 0, s, a); return hipGetLastError();
            F8_DWD(1) F8_DWD(2) F8_DWD(3) F8_DWD(4)
#undef F8_DWD
        }
        return hipErrorInvalidValue;
    }
    const size_t work = (size_t)a.N * a.P * a.Q * (a.Cs >> 2);
    const unsigned grid = (unsigned)std::min<size_t>((work + 255) / 256, 256 * 8 * 4);      // (grid-stride loop)
    if (a.in_signed) hipLaunchKernelGGL(dwdeconv_kernel<true>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dwdeconv_kernel<false>, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace f8
