// f8_dwk.hip — general depthwise convolution (gfx950): square kernels 3 / 5 / 7, stride 1 / 2, any pad up to K / 2, and the 3x3 at dilation d > 1
// (pad up to d) — everything depthwise that is not the undilated 3x3 / pad 1 of f8_kernels.hip / f8_dwmma.hip, which keeps its own kernels.  VALU; a
// launch of its own (S_DW, f8_net.cpp).
//
// All kernels work in the stored domain of the 3x3 kernels: NHWC int8 with channel stride Cs (a multiple of 32); unsigned tensors are stored
// biased (x ^ 0x80); wrapping int32 accumulation; optional ReLU floor; up to two int8 forms (QuantOut) and / or the tiled int32 form.
//
//   dwconvk_kernel<SIGNED_IN>     K, stride, pad, dilation at run time; one thread = one output pixel x 4 channels; bytes extracted and multiplied one by
//                                 one (unsigned inputs as unsigned bytes: out-of-image taps are skipped, plain bias).  Writes any form.  The
//                                 correctness anchor, and what runs when a launch writes the int32 form or option dwk_dot4 is 0.
//   dwconvk_dot4_kernel<K, S>     int8 forms only, on v_dot4_i32_i8.  One thread = 4 channels (one dword per tap) x DWK_PIX adjacent output pixels
//                                 of one row.  A dot4 reduces over four ROWS of one input column: the thread walks the (DWK_PIX - 1) * S + K input
//                                 columns of its pixels once, loads the K dwords of a column, byte-transposes rows 4g .. 4g + 3 into one dword per
//                                 channel (8 v_perm_b32 per group of four rows; a last group of ONE row — K = 5 — is three shifts: its other three
//                                 byte slots meet zero weights and may hold anything) and feeds each transposed column to every pixel whose window
//                                 holds it — up to K of them at stride 1 —, 4 x ceil(K / 4) dot4 each.  Per output value of 4 channels at stride 1:
//                                 K = 5: 40 dot4 + 22 transposing operations for 100 multiply-adds; K = 7: 56 + 40 for 196 (the 3x3 tap-raster kernel:
//                                 8 + 8 + 4 for 36).  Out-of-image taps are the biased zero (a real 0 for signed inputs) and 128 * sum(w) sits in
//                                 the bias, as in dwconv3x3_dot4_kernel.  Weights: pack_dwk_weights' image (f8_net.cpp),
//                                 [Cs / 4][K columns][G = ceil(K / 4) row groups][4 channels] dwords, byte j of a dword = row 4g + j (0 beyond K).
//   dwconv3x3_dil_dot4_kernel     int8 forms only, 3x3 at run-time dilation d > 1, stride 1, on the same K = 3 weight image.  A dot4 reduces over the
//                                 three rows h0, h0 + d, h0 + 2d of one input column (the fourth byte meets a zero weight).  Adjacent output pixels share
//                                 no column under dilation, so a thread owns 4 channels x DWK_PIX output pixels q, q + d, q + 2d, q + 3d of one row — one
//                                 residue class mod d — and walks the six columns q - pad, q - pad + d, .. q - pad + 5d once; each transposed column feeds
//                                 up to three pixels: 18 loads, 48 v_perm_b32 and 48 dot4 for 4 x 4 output values (144 multiply-adds).  A row is cut into
//                                 min(d, Q) residues x ceil(ceil(Q / d) / DWK_PIX) groups; pixels at or beyond Q are computed and not stored.
//   dwstrip_dot4_kernel<NW>       int8 forms only, the strips 1 x k / k x 1 of f8_net_conv_rect (3 <= k <= 31) at stride 1, both orientations in one kernel:
//                                 see the comment in front of it.  Strips at stride 2, with an int32 form or under dwk_dot4 = 0 run dwconvk_kernel, whose
//                                 tap loops are per axis (DwArgs::k rows behind the top pad, DwArgs::kw columns behind pad_w).
#include "f8_device.h"
#include <algorithm>

namespace f8 {

namespace {
constexpr int DWK_PIX = 4;                          // adjacent output pixels per thread of the dot4 kernel
}

template <bool SIGNED_IN>
__global__ void __launch_bounds__(256) dwconvk_kernel(const DwArgs a) {
    const int cgs = a.Cs >> 2;
    const size_t total = (size_t)a.N * a.P * a.Q * cgs;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * blockDim.x) {
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
        const int h0 = p * a.stride - a.pad, w0 = q * a.stride - a.pad_w;      // (per axis: k rows behind the top pad, kw columns behind the left pad)
        const unsigned in_xor = SIGNED_IN ? 0u : 0x80808080u;   // unsigned tensors are stored biased
        for (int r = 0; r < a.k; ++r) {
            const int h = h0 + r * a.dil;
            if ((unsigned)h >= (unsigned)a.H) continue;
            for (int s = 0; s < a.kw; ++s) {
                const int w = w0 + s * a.dil;
                if ((unsigned)w >= (unsigned)a.W) continue;
                const unsigned xv = *(const unsigned*)(a.x + (((size_t)n * a.H + h) * a.W + w) * a.Cs + c) ^ in_xor;
                const unsigned wv = *(const unsigned*)(a.w + (size_t)(r * a.kw + s) * a.Cs + c);
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
        for (int k = 0; k < 2; ++k)
            if (a.q[k].ptr)
                *(unsigned*)(a.q[k].ptr + o) =
                    requant_pack4(acc[0], acc[1], acc[2], acc[3], a.q[k]);
    }
}

template <int K, int S>
__global__ void __launch_bounds__(256) dwconvk_dot4_kernel(const DwArgs a) {
    constexpr int PIX = DWK_PIX;
    constexpr int NCOL = (PIX - 1) * S + K;          // input columns the thread's pixels read
    constexpr int G = (K + 3) / 4;                   // groups of four rows
    constexpr int LAST = K - 4 * (G - 1);            // rows of the last group: 3 (K = 3, 7) or 1 (K = 5)
    static_assert(LAST == 1 || LAST == 3, "K is 3, 5 or 7");
    const int cgs = a.Cs >> 2;                       // 4-channel quads
    const int QS = (a.Q + PIX - 1) / PIX;
    const size_t total = (size_t)a.N * a.P * QS * cgs;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int cg = (int)(idx % cgs);
    size_t st = idx / cgs;
    const int qs = (int)(st % QS); st /= QS;
    const int p = (int)(st % a.P);
    const int n = (int)(st / a.P);
    const int c = cg << 2, q0 = qs * PIX;
    const unsigned padv = a.in_signed ? 0u : 0x80808080u;
    const int h0 = p * S - a.pad, w0 = q0 * S - a.pad;
    const unsigned* const wq = (const unsigned*)a.w + (size_t)cg * (K * G * 4);      // [column][group][channel]

    int acc[PIX][4];
    {
        const v4i bv = *(const v4i*)(a.bias + c);
#pragma unroll
        for (int j = 0; j < PIX; ++j) { acc[j][0] = bv.x; acc[j][1] = bv.y; acc[j][2] = bv.z; acc[j][3] = bv.w; }
    }
    const int8_t* const xn = a.x + (size_t)n * a.H * a.W * a.Cs + c;
#pragma unroll
    for (int cc = 0; cc < NCOL; ++cc) {
        const int w = w0 + cc;
        const bool wok = (unsigned)w < (unsigned)a.W;
        unsigned t[4 * G];                            // rows 0 .. K - 1 of this column, 4 channels each
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int h = h0 + r;
            unsigned v = padv;
            if (wok && (unsigned)h < (unsigned)a.H) v = *(const unsigned*)(xn + ((size_t)h * a.W + w) * a.Cs);
            t[r] = v;
        }
        unsigned col[G][4];                           // [row group][channel]: bytes = the group's four rows
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (g == G - 1 && LAST == 1) {            // one row: byte 0 is the row, the other slots meet zero weights
                col[g][0] = t[4 * g]; col[g][1] = t[4 * g] >> 8; col[g][2] = t[4 * g] >> 16; col[g][3] = t[4 * g] >> 24;
            } else {
                const unsigned t0 = t[4 * g], t1 = t[4 * g + 1], t2 = t[4 * g + 2];
                const unsigned t3 = (g == G - 1) ? t2 : t[4 * g + 3];                 // (three rows: slot 3 meets a zero weight)
                const unsigned lo01 = __builtin_amdgcn_perm(t1, t0, 0x05010400u), hi01 = __builtin_amdgcn_perm(t1, t0, 0x07030602u);
                const unsigned lo23 = __builtin_amdgcn_perm(t3, t2, 0x05010400u), hi23 = __builtin_amdgcn_perm(t3, t2, 0x07030602u);
                col[g][0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u); col[g][1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
                col[g][2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u); col[g][3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
            }
        }
        // every pixel j whose window [j * S, j * S + K) holds column cc: kernel column s = cc - j * S
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            const int s = cc - j * S;
            if (s < 0 || s >= K) continue;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const v4i wv = *(const v4i*)(wq + (s * G + g) * 4);
                acc[j][0] = __builtin_amdgcn_sdot4((int)col[g][0], wv.x, acc[j][0], false);
                acc[j][1] = __builtin_amdgcn_sdot4((int)col[g][1], wv.y, acc[j][1], false);
                acc[j][2] = __builtin_amdgcn_sdot4((int)col[g][2], wv.z, acc[j][2], false);
                acc[j][3] = __builtin_amdgcn_sdot4((int)col[g][3], wv.w, acc[j][3], false);
            }
        }
    }
    const int floor0 = a.relu0 ? 0 : INT32_MIN;
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        if (q0 + j >= a.Q) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j][e] = max(acc[j][e], floor0);
        const size_t o = ((((size_t)n * a.P + p) * a.Q + q0 + j)) * a.Cs + c;
#pragma unroll
        for (int f = 0; f < 2; ++f)
            if (a.q[f].ptr)
                *(unsigned*)(a.q[f].ptr + o) =
                    requant_pack4(acc[j][0], acc[j][1], acc[j][2], acc[j][3], a.q[f]);
    }
}

// One thread = 4 channels x DWK_PIX output pixels of one row and one residue class mod dil: q = (DWK_PIX * g + j) * dil + res, j = 0 .. DWK_PIX - 1.
__global__ void __launch_bounds__(256) dwconv3x3_dil_dot4_kernel(const DwArgs a) {
    constexpr int PIX = DWK_PIX, NCOL = PIX + 2;     // the pixels' columns: q0 - pad + cc * dil
    const int d = a.dil;
    const int cgs = a.Cs >> 2;                       // 4-channel quads
    const int DR = min(d, a.Q);                      // residue classes that hold a pixel
    const int NG = ((a.Q + d - 1) / d + PIX - 1) / PIX;
    const size_t total = (size_t)a.N * a.P * NG * DR * cgs;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int cg = (int)(idx % cgs);
    size_t st = idx / cgs;
    const int res = (int)(st % DR); st /= DR;
    const int g = (int)(st % NG); st /= NG;
    const int p = (int)(st % a.P);
    const int n = (int)(st / a.P);
    const int c = cg << 2, q0 = g * PIX * d + res;
    const unsigned padv = a.in_signed ? 0u : 0x80808080u;
    const int h0 = p - a.pad, w0 = q0 - a.pad;
    const unsigned* const wq = (const unsigned*)a.w + (size_t)cg * (3 * 4);          // [column][channel]: bytes = rows 0 .. 2, 0

    int acc[PIX][4];
    {
        const v4i bv = *(const v4i*)(a.bias + c);
#pragma unroll
        for (int j = 0; j < PIX; ++j) { acc[j][0] = bv.x; acc[j][1] = bv.y; acc[j][2] = bv.z; acc[j][3] = bv.w; }
    }
    v4i wv[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) wv[s] = *(const v4i*)(wq + s * 4);
    const int8_t* const xn = a.x + (size_t)n * a.H * a.W * a.Cs + c;
#pragma unroll
    for (int cc = 0; cc < NCOL; ++cc) {
        const int w = w0 + cc * d;
        const bool wok = (unsigned)w < (unsigned)a.W;
        unsigned t[3];                                // rows h0, h0 + d, h0 + 2d of this column, 4 channels each
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int h = h0 + r * d;
            unsigned v = padv;
            if (wok && (unsigned)h < (unsigned)a.H) v = *(const unsigned*)(xn + ((size_t)h * a.W + w) * a.Cs);
            t[r] = v;
        }
        // byte transpose: col[e] = rows 0, 1, 2 (and 2 again: slot 3 meets a zero weight) of channel e
        const unsigned lo01 = __builtin_amdgcn_perm(t[1], t[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(t[1], t[0], 0x07030602u);
        const unsigned lo23 = __builtin_amdgcn_perm(t[2], t[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(t[2], t[2], 0x07030602u);
        const unsigned col0 = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u), col1 = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
        const unsigned col2 = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u), col3 = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
        // every pixel j whose window holds column cc: kernel column s = cc - j
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            const int s = cc - j;
            if (s < 0 || s >= 3) continue;
            acc[j][0] = __builtin_amdgcn_sdot4((int)col0, wv[s].x, acc[j][0], false);
            acc[j][1] = __builtin_amdgcn_sdot4((int)col1, wv[s].y, acc[j][1], false);
            acc[j][2] = __builtin_amdgcn_sdot4((int)col2, wv[s].z, acc[j][2], false);
            acc[j][3] = __builtin_amdgcn_sdot4((int)col3, wv[s].w, acc[j][3], false);
        }
    }
    const int floor0 = a.relu0 ? 0 : INT32_MIN;
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const int q = q0 + j * d;
        if (q >= a.Q) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j][e] = max(acc[j][e], floor0);
        const size_t o = ((((size_t)n * a.P + p) * a.Q + q)) * a.Cs + c;
#pragma unroll
        for (int f = 0; f < 2; ++f)
            if (a.q[f].ptr)
                *(unsigned*)(a.q[f].ptr + o) =
                    requant_pack4(acc[j][0], acc[j][1], acc[j][2], acc[j][3], a.q[f]);
    }
}

// Depthwise strips 1 x k / k x 1 at stride 1 (f8_net_conv_rect), int8 forms only, on v_dot4_i32_i8: ONE kernel for both orientations — the strip axis is a
// run-time byte step between successive taps and successive outputs (Cs for 1 x k, W * Cs for k x 1).  One thread = 4 channels x DWS_RUN consecutive
// outputs o0 .. o0 + DWS_RUN - 1 along the strip.  It loads the DWS_RUN / 4 + NW - 1 groups of four input positions from i0 = o0 - pad on, once (a position
// outside the image: the biased zero), byte-transposes each group with the 8 v_perm_b32 of dwconvk_dot4_kernel — one dword per channel, byte b = position
// i0 + 4 g + b — and accumulates output j, whose window starts at byte j % 4 of group j / 4, against weight image j % 4 of pack_dwk_weights: the k taps
// shifted by that many bytes and zero-filled, NW = ceil((k + 3) / 4) dwords per channel.  The data is transposed once and never re-aligned; the phases are
// compile-time (o0 is a multiple of DWS_RUN).  Per output value of one channel: NW dot4 instead of k multiplies; per run (DWS_RUN + 4 NW - 4) / 4 group
// loads instead of k loads per output.  Lanes run over channel quads first, then over the other axis' pixels (k x 1) or the runs (1 x k): either
// orientation reads whole rows of Cs bytes.  NW is the only template parameter: one instance serves four kernel sizes (4 NW - 6 .. 4 NW - 3).
namespace {
constexpr int DWS_RUN = 8;                          // consecutive outputs along the strip per thread
}
template <int NW>
__global__ void __launch_bounds__(256) dwstrip_dot4_kernel(const DwArgs a) {
    constexpr int RUN = DWS_RUN, NG = RUN / 4 + NW - 1;      // groups of four input positions
    const bool vert = a.kw == 1;                     // k x 1: the strip runs down the rows
    const int cgs = a.Cs >> 2;                       // 4-channel quads
    const int LO = vert ? a.P : a.Q, LI = vert ? a.H : a.W;      // outputs / inputs along the strip
    const int B = vert ? a.Q : a.P;                  // pixels on the other axis (the same in and out: kernel 1, no pad)
    const int RUNS = (LO + RUN - 1) / RUN;
    const size_t total = (size_t)a.N * RUNS * B * cgs;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int cg = (int)(idx % cgs);
    size_t st = idx / cgs;
    int run, b;
    if (vert) { b = (int)(st % B); st /= B; run = (int)(st % RUNS); st /= RUNS; }
    else { run = (int)(st % RUNS); st /= RUNS; b = (int)(st % B); st /= B; }
    const int n = (int)st;
    const int c = cg << 2, o0 = run * RUN;
    const int i0 = o0 - (vert ? a.pad : a.pad_w);
    const size_t istep = vert ? (size_t)a.W * a.Cs : (size_t)a.Cs, ibstep = vert ? (size_t)a.Cs : (size_t)a.W * a.Cs;
    const size_t ostep = vert ? (size_t)a.Q * a.Cs : (size_t)a.Cs, obstep = vert ? (size_t)a.Cs : (size_t)a.Q * a.Cs;
    const unsigned padv = a.in_signed ? 0u : 0x80808080u;
    const int8_t* const xb = a.x + (size_t)n * a.H * a.W * a.Cs + (size_t)b * ibstep + c;

    unsigned col[NG][4];                             // [group][channel]: bytes = the group's four positions
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        unsigned t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + 4 * g + j;
            unsigned v = padv;
            if ((unsigned)i < (unsigned)LI) v = *(const unsigned*)(xb + (size_t)i * istep);
            t[j] = v;
        }
        const unsigned lo01 = __builtin_amdgcn_perm(t[1], t[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(t[1], t[0], 0x07030602u);
        const unsigned lo23 = __builtin_amdgcn_perm(t[3], t[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(t[3], t[2], 0x07030602u);
        col[g][0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u); col[g][1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
        col[g][2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u); col[g][3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
    }
    const v4i bv = *(const v4i*)(a.bias + c);
    const unsigned* const wq = (const unsigned*)a.w + (size_t)cg * (4 * NW * 4);      // [phase][dword][channel]
    const int floor0 = a.relu0 ? 0 : INT32_MIN;
    int8_t* const q0 = a.q[0].ptr, * const q1 = a.q[1].ptr;
    const size_t ob = ((size_t)n * a.P * a.Q) * a.Cs + (size_t)b * obstep + c;
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) {
        v4i wv[NW];
#pragma unroll
        for (int m = 0; m < NW; ++m) wv[m] = *(const v4i*)(wq + (ph * NW + m) * 4);
#pragma unroll
        for (int jj = 0; jj < RUN / 4; ++jj) {
            int acc0 = bv.x, acc1 = bv.y, acc2 = bv.z, acc3 = bv.w;
#pragma unroll
            for (int m = 0; m < NW; ++m) {
                acc0 = __builtin_amdgcn_sdot4((int)col[jj + m][0], wv[m].x, acc0, false);
                acc1 = __builtin_amdgcn_sdot4((int)col[jj + m][1], wv[m].y, acc1, false);
                acc2 = __builtin_amdgcn_sdot4((int)col[jj + m][2], wv[m].z, acc2, false);
                acc3 = __builtin_amdgcn_sdot4((int)col[jj + m][3], wv[m].w, acc3, false);
            }
            const int o = o0 + 4 * jj + ph;
            if (o >= LO) continue;
            acc0 = max(acc0, floor0); acc1 = max(acc1, floor0); acc2 = max(acc2, floor0); acc3 = max(acc3, floor0);
            const size_t off = ob + (size_t)o * ostep;
            if (q0) *(unsigned*)(q0 + off) = requant_pack4(acc0, acc1, acc2, acc3, a.q[0]);
            if (q1) *(unsigned*)(q1 + off) = requant_pack4(acc0, acc1, acc2, acc3, a.q[1]);
        }
    }
}

// General depthwise: the v_dot4 kernels for int8-only launches (Options::dwk_dot4), else the generic one.  A dilated conv (3x3 only) has its dot4
// kernel — instance 2 — at stride 1, exactly where dwconvk_dot4_kernel<3, 1> runs the undilated one.
int dwk_inst(const DwArgs& a, bool out32, bool dot4) {
    if (a.kw != a.k) return dot4 && !out32 && a.stride == 1 && a.dil == 1 && (a.k == 1 || a.kw == 1) ? 3 : 0;      // a strip: instance 3, dwstrip_dot4_kernel
    if (a.dil > 1) return dot4 && !out32 && a.k == 3 && a.stride == 1 ? 2 : 0;
    return dot4 && !out32 && (a.k == 3 || a.k == 5 || a.k == 7) && (a.stride == 1 || a.stride == 2) ? 1 : 0;
}

int dwk_kernel_name(char* buf, size_t cap, const DwArgs& a, int inst) {
    if (inst == 2) return snprintf(buf, cap, "f8::dwconv3x3_dil_dot4_kernel");
    if (inst == 3) return snprintf(buf, cap, "f8::dwstrip_dot4_kernel<%d>", (std::max(a.k, a.kw) + 6) / 4);
    if (inst) return snprintf(buf, cap, "f8::dwconvk_dot4_kernel<%d, %d>", a.k, a.stride);
    return snprintf(buf, cap, "f8::dwconvk_kernel<%s>", a.in_signed ? "true" : "false");
}

hipError_t launch_dwk(const DwArgs& a, int inst, hipStream_t s) {
    if (a.kw != a.k) {                                    // a strip 1 x k / k x 1: pads below k on its axis, none on the other; instance 3 or the generic kernel
        const int k = std::max(a.k, a.kw);
        if (std::min(a.k, a.kw) != 1 || k < 3 || k > 31 || a.dil != 1 || a.pad < 0 || a.pad >= a.k || a.pad_w < 0 || a.pad_w >= a.kw || (inst != 0 && inst != 3))
            return hipErrorInvalidValue;
        if (inst == 3) {
            const bool vert = a.kw == 1;
            if (a.out32 || !a.w4 || a.stride != 1 || (vert ? a.Q != a.W : a.P != a.H)) return hipErrorInvalidValue;      // (the other axis: the same pixels in and out)
            const size_t work = (size_t)a.N * (((vert ? a.P : a.Q) + DWS_RUN - 1) / DWS_RUN) * (vert ? a.Q : a.P) * (a.Cs >> 2);
            const unsigned grid = (unsigned)((work + 255) / 256);
            DwArgs b = a; b.w = a.w4; b.bias = a.bias4;
            switch ((k + 6) / 4) {
#define F8_DWS(NW_) case NW_: hipLaunchKernelGGL((dwstrip_dot4_kernel<NW_>), dim3(grid), dim3(256), 0, s, b); return hipGetLastError();
                F8_DWS(2) F8_DWS(3) F8_DWS(4) F8_DWS(5) F8_DWS(6) F8_DWS(7) F8_DWS(8) F8_DWS(9)
#undef F8_DWS
            }
            return hipErrorInvalidValue;
        }
    } else {
        if (a.k < 1 || a.dil < 1 || a.pad < 0 || a.pad > (a.dil > 1 ? a.dil : a.k / 2) || (a.dil > 1 && a.k != 3) || a.pad_w != a.pad) return hipErrorInvalidValue;
        if ((inst == 2) != (a.dil > 1 && inst != 0)) return hipErrorInvalidValue;      // a dot4 instance: 2 for a dilated conv and only for one
    }
    if (inst == 2) {
        if (a.out32 || !a.w4 || a.stride != 1) return hipErrorInvalidValue;
        const int DR = std::min(a.dil, a.Q), NG = ((a.Q + a.dil - 1) / a.dil + DWK_PIX - 1) / DWK_PIX;
        const size_t work = (size_t)a.N * a.P * NG * DR * (a.Cs >> 2);
        DwArgs b = a; b.w = a.w4; b.bias = a.bias4;
        hipLaunchKernelGGL(dwconv3x3_dil_dot4_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, b);
        return hipGetLastError();
    }
    if (inst) {
        if (a.out32 || !a.w4) return hipErrorInvalidValue;
        const size_t work = (size_t)a.N * a.P * ((a.Q + DWK_PIX - 1) / DWK_PIX) * (a.Cs >> 2);
        const unsigned grid = (unsigned)((work + 255) / 256);
        DwArgs b = a; b.w = a.w4; b.bias = a.bias4;
#define F8_DWK(K_, S_) if (a.k == K_ && a.stride == S_) { hipLaunchKernelGGL((dwconvk_dot4_kernel<K_, S_>), dim3(grid), dim3(256), 0, s, b); return hipGetLastError(); }
        F8_DWK(3, 1) F8_DWK(3, 2) F8_DWK(5, 1) F8_DWK(5, 2) F8_DWK(7, 1) F8_DWK(7, 2)
#undef F8_DWK
        return hipErrorInvalidValue;
    }
    const size_t work = (size_t)a.N * a.P * a.Q * (a.Cs >> 2);
    const unsigned grid = (unsigned)std::min<size_t>((work + 255) / 256, 256 * 8 * 4);      // (grid-stride loop)
    if (a.in_signed) hipLaunchKernelGGL(dwconvk_kernel<true>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dwconvk_kernel<false>, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace f8
