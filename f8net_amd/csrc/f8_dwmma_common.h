// f8_dwmma_common.h — the row-walking depthwise 3x3 (stride 1 / 2, pad 1) on the matrix cores as a device function: the walker of
// dwconv3x3_mma_kernel (f8_dwmma.hip; its header comment describes the method), with what is done with a finished row of accumulators
// left to the caller.  f8_dws.hip requantises the row into an LDS tile a 1x1 GEMM reads.  (f8_dwmma.hip itself keeps its own text:
// calling this function from it changed the register allocation of 4 of its 12 instances by one or two registers — DESIGN.md 4.5c.)
#pragma once
#include "f8_device.h"

namespace f8 {

constexpr int DWS_SW = 28;                          // output columns per strip (lanes 28 .. 31 only feed the shifts): DW_SW of f8_dwmma.hip

__device__ __forceinline__ v4i dws_next_lane(const v4i& v) {   // lane i <- lane i + 1, each dword (= 4 channels of one pixel) on its own
    v4i r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = __builtin_amdgcn_update_dpp(v[k], v[k], 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
    return r;
}

// One wave's walk: image n, channel tile ct, output columns q0 .. q0 + VW - 1, output rows p0 .. p1 - 1.
// S: stride.  SUBS: output rows per MFMA pixel tile: 1 = 32 lanes along one row (VW = 28 outputs), 2 = two rows of 16 lanes (VW = 14
// outputs each: 14-wide maps).  `a` carries x (int8 NHWC), w ([9][Cs] tap-major), bias ([Cs], + 128 * sum(w) for unsigned inputs), N, H, W,
// Cs, in_signed.  emit(acc, p), once per step: the accumulators (bias included) of output row p — lane l31 holds column
// q0 + (SUBS == 2 ? l31 & 15 : l31) of row p (= the step's first row + (SUBS == 2 ? l31 >> 4 : 0)), channels as the MFMA leaves them;
// rows p >= p1 and columns beyond VW / the map are the caller's to drop.
template <int S, int SUBS, class A, class Emit>
__device__ __forceinline__ void dw_walk(const A& a, int n, int ct, int q0, int p0, int p1, Emit&& emit) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
    const int sub = SUBS == 2 ? l31 >> 4 : 0, u = SUBS == 2 ? l31 & 15 : l31;      // sub-row of the tile, lane inside it
    const int ch = ct * 32 + 16 * lh;                               // first of this lane's 16 channels (B operand)

    // ---- the nine diagonal weight fragments of this channel tile, the bias in accumulator order
    v4i wa[9];
    {
        const bool mine = (l31 >> 4) == lh;                         // K index == row index: rows 0-15 sit in K half 0, 16-31 in half 1
        const int dsel = (l31 & 15) >> 2, bsh = 8 * (l31 & 3);
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) {
            const unsigned wv = (unsigned)(unsigned char)a.w[(size_t)tp * a.Cs + ct * 32 + l31];
            const int piece = mine ? (int)(wv << bsh) : 0;
            wa[tp] = v4i{dsel == 0 ? piece : 0, dsel == 1 ? piece : 0, dsel == 2 ? piece : 0, dsel == 3 ? piece : 0};
        }
    }
    v4i bq[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bq[g] = *(const v4i*)(a.bias + ct * 32 + 8 * g + 4 * lh);

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (unsigned)((size_t)a.N * a.H * a.W * a.Cs), 0x00020000);
    const int padv = a.in_signed ? 0 : (int)0x80808080u;
    // input column of this lane: stride 1: q0 - 1 + l (taps kx = 0, 1, 2 are this fragment shifted by 0, 1, 2 lanes);
    // stride 2: O = 2 (q0 + l) - 1 (kx = 0; kx = 2 is O of the next lane), E = 2 (q0 + l) (kx = 1)
    const int colA = S == 1 ? q0 - 1 + u : 2 * (q0 + u) - 1;
    const int colB = 2 * (q0 + u);
    const bool okA = colA >= 0 && colA < a.W, okB = colB < a.W;
    auto row_off = [&](int r, int col, bool ok) -> unsigned {
        return (ok && r >= 0 && r < a.H) ? (unsigned)((((size_t)n * a.H + r) * a.W + col) * a.Cs + ch) : kOOB;
    };
    auto fix = [&](v4i v, unsigned off) { if (off == kOOB) v = v4i{padv, padv, padv, padv}; return v; };

    // fragments of an input row: f[0..2] = taps kx = 0, 1, 2
    struct Row { v4i f[3]; };
    auto make_row = [&](const v4i& va, const v4i& vb) {
        Row R;
        if constexpr (S == 1) { R.f[0] = va; R.f[1] = dws_next_lane(va); R.f[2] = dws_next_lane(R.f[1]); }
        else { R.f[0] = va; R.f[1] = vb; R.f[2] = dws_next_lane(va); }
        return R;
    };
    auto load_row = [&](int r, v4i& va, v4i& vb, unsigned& oa, unsigned& ob) {
        oa = row_off(r, colA, okA);
        va = __builtin_amdgcn_raw_buffer_load_b128(rx, oa, 0, 0);
        if constexpr (S == 2) { ob = row_off(r, colB, okB); vb = __builtin_amdgcn_raw_buffer_load_b128(rx, ob, 0, 0); }
    };
    auto mac3 = [&](v16i acc, const Row& R, int ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wa[ky * 3 + kx], R.f[kx], acc, 0, 0, 0);
        return acc;
    };
    auto acc0 = [&]() {
        v16i acc;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[4 * g + e] = bq[g][e];
        return acc;
    };

    // Output row p + sub reads input rows S (p + sub) - 1 + k, k = 0 .. 2 (fragment k).  A step advances SUBS output rows: fragment k of
    // the next step is fragment k + NEW of this one where that exists (the rows slide in registers), NEW fragments are loaded — one
    // step ahead, under this step's multiplies.
    constexpr int NEW = S == 1 ? SUBS : (SUBS == 1 ? 2 : 3), KEEP = 3 - NEW;
    auto in_row = [&](int p, int k) { return S * (p + sub) - 1 + k; };
    Row R[3];
    {
        v4i va[3], vb[3]; unsigned oa[3], ob[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 3; ++k) load_row(in_row(p0, k), va[k], vb[k], oa[k], ob[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) R[k] = make_row(fix(va[k], oa[k]), S == 2 ? fix(vb[k], ob[k]) : vb[k]);
    }
    for (int p = p0; p < p1; p += SUBS) {
        v4i na[NEW], nb[NEW]; unsigned noa[NEW], nob[NEW];
        const bool more = p + SUBS < p1;
        if (more) {
#pragma unroll
            for (int j = 0; j < NEW; ++j) { nob[j] = 0; load_row(in_row(p + SUBS, KEEP + j), na[j], nb[j], noa[j], nob[j]); }
        }
        v16i acc = acc0();
#pragma unroll
        for (int k = 0; k < 3; ++k) acc = mac3(acc, R[k], k);
        emit(acc, p + sub);
        if (more) {
#pragma unroll
            for (int k = 0; k < KEEP; ++k) R[k] = R[k + NEW];
#pragma unroll
            for (int j = 0; j < NEW; ++j) R[KEEP + j] = make_row(fix(na[j], noa[j]), S == 2 ? fix(nb[j], nob[j]) : nb[j]);
        }
    }
}

}  // namespace f8
