// f8_irchain.hip — one launch for a run of consecutive stride-1 MobileNet-V2 inverted-residual blocks on one map (gfx950).
//
//   per block:  x8 --1x1 CIN->E, ReLU--> e1 --depthwise 3x3 / 1, pad 1, ReLU--> e2 --1x1 E->COUT--> [+ stream (int32)] -> y
//
// i.e. IntBlock.forward of ref:models/fix_mobilenet_v2.py:20-48 applied block after block, every int_op_only_fix_quant
// (fix_quant_ops.py:90-114) in place.  Work unit: ONE workgroup owns ONE image for the whole chain — no halo exchange, no ticket, no flag
// between workgroups, hence no co-residency requirement: the grid is N workgroups.  Between two blocks nothing goes to HBM:
//   X     the block input, int8 in its expand conv's input format            [CIN/32][xp][32 B]             (written by the previous epilogue)
//   strm  the int32 stream (the block output the NEXT block joins; the first block's int32 input), in the accumulator layout of v_mfma_i32_32x32x32_i8
//         [COUT/32][pixel tile][4][64 lanes][16 B]: a lane reads / writes the values it joins, 1 KB contiguous per wave and group
// Inside a block, the chunk scheme of fused_ir_kernel (f8_ir.hip): the expanded channels in chunks of 64, per chunk
//   P1  expand: e1[chunk] over the image (MFMA, K = CIN, input from X)       -> requant -> LDS patch (zero border = biased zero)
//   P2  depthwise 3x3 on the patch, on the matrix cores (diagonal fragments)  -> requant -> LDS mid2
//   P3  project: acc[px][COUT] += W4[:, chunk] . mid2 (MFMA, K = 64)          accumulators stay in registers across the chunks
// The chunk's weight slices are loaded into registers while the previous chunk computes (the chunk index runs on across blocks, so the next
// block's first slices are in flight during this block's last chunk); they are written to ONE LDS buffer after the chunk's P3 (one more
// barrier per chunk than fused_ir_kernel's two buffers: the 14x14 stream takes that LDS).  Epilogue of a block: bias, [ReLU], [join
// (acc << acc_shl) + (stream << res_shl), wrapping, clamp to +-(2^31 - 1), ReLU], then the stream (strm, when the next block joins it) and
// the next block's int8 input (X), or — last block — the int32 (I32T) and int8 forms in HBM.
//
// Waves: 8 (NW).  A wave owns pixel tile (wave % npw) and the output-channel tiles j == wave / npw (mod 8 / npw) in P3 and the epilogues, with
// npw = the pixel tiles of the map rounded up to a power of two: every shape is a run-time value (the 64x64 / 96x96 test nets run the same
// code at 2x2 .. 8x8).  Template parameters only size registers and the host's LDS check: the largest CIN / COUT of a block and NPW_MAX,
// the most pixel tiles (NPW_MAX x 32 pixels per image).
#include "f8_device.h"

namespace f8 {

// a wave-uniform value held in a VECTOR register: the block descriptors' clamp bounds, storage biases and join shifts are read once per
// block and live across its whole chunk loop — as scalars they pushed the 320-channel instances into SGPR spills through scratch
__device__ __forceinline__ int vgpr(int x) { int r; asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "s"(x)); return r; }

template <int CIN_MAX, int COUT_MAX, int NPW_MAX, int NW, int FQ>
__global__ void __launch_bounds__(NW * 64, 1) irchain_kernel(const IRChainArgs a) {
    constexpr int NT = NW * 64;
    constexpr int NJ = (COUT_MAX / 32 + NW / NPW_MAX - 1) / (NW / NPW_MAX);   // output-channel tiles per wave (fewest channel groups)
    constexpr int W0_L = (64 * CIN_MAX / 16 + NT - 1) / NT, W4_L = (COUT_MAX * 64 / 16 + NT - 1) / NT;
    if constexpr (FQ == 1) set_fp_round_nearest_even();
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* const X = lds;
    char* const strm = lds + a.off_strm;
    char* const patch = lds + a.off_patch;                 // [2][H + 2][W + 2][32 B]: channel-tile planes
    char* const mid2 = lds + a.off_mid2;                   // [2][xp][32 B]
    char* const wb = lds + a.off_w;                        // W0 [cin/32][64][32 B] | W4 [2][cout][32 B] | dw 576 B (+64) | dw bias 256 B | b0 256 B

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const int H = a.H, W = a.W, PW = W + 2, HW = H * W, xp = a.xp;
    const int npt = (HW + 31) >> 5;
    int npw = 1;
    while (npw < npt) npw <<= 1;                           // <= NPW_MAX <= NW (irchain_supported)
    const int nch = NW / npw, pw = wave & (npw - 1), ch = wave / npw;
    const int pct = (H + 2) * PW * 32;                     // bytes of one 32-channel plane of the patch
    const int mid_ct = xp * 32;                            // ... of mid2
    const int n0 = blockIdx.x;
    auto split_px = [&](int px, int& r, int& c) {
        r = (int)fast_div((unsigned)px, a.dW);
        c = px - r * W;
    };

    // ---- block 0 input -> X ([kk][px][32 B]; pixels beyond the map are zero)
    {
        const int cin = a.blk[0].cin, nslot = xp * (cin >> 5) * 2;
        for (int sl = tid; sl < nslot; sl += NT) {
            const int kk = sl / (xp * 2), rem = sl - kk * (xp * 2), px = rem >> 1, half = rem & 1;
            v4i v = {0, 0, 0, 0};
            if (px < HW) v = *(const v4i*)(a.x8 + ((size_t)n0 * HW + px) * cin + kk * 32 + half * 16);
            *(v4i*)(X + (size_t)sl * 16) = v;
        }
    }
    auto fill_border = [&](unsigned xor1) {                // patch <- biased zero (P1 only ever writes interior pixels)
        const v4i zv = {(int)xor1, (int)xor1, (int)xor1, (int)xor1};
        for (int o = tid * 16; o < 2 * pct; o += NT * 16) *(v4i*)(patch + o) = zv;
    };
    fill_border(a.blk[0].r1.bias_xor);
    if (a.blk[0].res) {                                    // ---- block 0 joins the int32 input: I32T -> strm (accumulator layout)
        const int n = (a.blk[0].cin >> 5) * npt * 256;
        for (int i = tid; i < n; i += NT) {
            const int ln = i & 63, gq = (i >> 6) & 3, rest = i >> 8, j = rest / npt, pt = rest - j * npt, px = pt * 32 + (ln & 31);
            v4i v = {0, 0, 0, 0};
            if (px < HW) v = *(const v4i*)(a.xr + i32t_index(n0 * HW + px, j * 32 + 8 * gq + 4 * (ln >> 5), a.blk[0].cin));
            *(v4i*)(strm + (size_t)i * 16) = v;
        }
    }

    // ---- weight slices of one chunk: global -> registers (early) -> LDS (late)
    v4i rw0[W0_L], rw4[W4_L], rsm;
    auto load_w = [&](const auto& B, int e) {
        const int rows_ok = B.E32 - 64 * e, cin = B.cin, cout = B.cout;
#pragma unroll
        for (int i = 0; i < W0_L; ++i) {                   // W0 rows 64e .. 64e+63 -> [kk][row][32 B]
            const int sl = tid + i * NT;
            const int kk = sl >> 7, row = (sl >> 1) & 63, half = sl & 1;
            v4i v = {0, 0, 0, 0};
            if (sl < 4 * cin && row < rows_ok) v = *(const v4i*)(B.w0 + (size_t)(64 * e + row) * cin + kk * 32 + half * 16);
            rw0[i] = v;
        }
#pragma unroll
        for (int i = 0; i < W4_L; ++i) {                   // W4 columns 64e .. 64e+63 of every row -> [kk][row][32 B]
            const int sl = tid + i * NT;
            v4i v = {0, 0, 0, 0};
            if (sl < 4 * cout) {
                const int kk = sl / (cout * 2), row = (sl >> 1) - kk * cout, half = sl & 1;
                if (kk * 32 < rows_ok) v = *(const v4i*)(B.w4 + (size_t)row * B.E32 + 64 * e + kk * 32 + half * 16);
            }
            rw4[i] = v;
        }
        {   // depthwise weights (dot4 image: 36 B per 4-channel quad), depthwise bias, expand bias: 64 channels each
            v4i v = {0, 0, 0, 0};
            if (tid < 36) { if (tid * 16 + 16 <= (rows_ok >= 64 ? 576 : 288)) v = *(const v4i*)(B.wd4 + (size_t)(16 * e) * 36 + tid * 16); }
            else if (tid < 52) { const int i = tid - 36; if (4 * i < rows_ok) v = *(const v4i*)(B.bd4 + 64 * e + 4 * i); }
            else if (tid < 68) { const int i = tid - 52; if (4 * i < rows_ok) v = *(const v4i*)(B.b0 + 64 * e + 4 * i); }
            rsm = v;
        }
    };
    auto store_w = [&](const auto& B) {
        const int off_w4 = 64 * B.cin, off_dw = off_w4 + 64 * B.cout;
#pragma unroll
        for (int i = 0; i < W0_L; ++i) { const int sl = tid + i * NT; if (sl < 4 * B.cin) *(v4i*)(wb + sl * 16) = rw0[i]; }
#pragma unroll
        for (int i = 0; i < W4_L; ++i) { const int sl = tid + i * NT; if (sl < 4 * B.cout) *(v4i*)(wb + off_w4 + sl * 16) = rw4[i]; }
        if (tid < 36) *(v4i*)(wb + off_dw + tid * 16) = rsm;
        else if (tid < 52) *(v4i*)(wb + off_dw + 640 + (tid - 36) * 16) = rsm;
        else if (tid < 68) *(v4i*)(wb + off_dw + 896 + (tid - 52) * 16) = rsm;
    };
    load_w(a.blk[0], 0);
    store_w(a.blk[0]);

    v16i acc3[NJ];
    // ================= epilogue of a block: bias, [ReLU], [join + clamp], then the stream / the next block's input (LAST: the HBM forms, after the
    //                   block loop, so that the output pointers and formats are not live across it)
    auto epilogue = [&](const IRChainBlk& B, auto last_c) {
        constexpr bool LAST = decltype(last_c)::value;
        const int cout = B.cout, nco = cout >> 5;
        if (pw < npt) {
            const int opx = pw * 32 + l31;
            const bool ok = opx < HW;
            const int m = n0 * HW + (ok ? opx : 0);
            const int floor0 = vgpr(B.relu0 ? 0 : INT32_MIN), floor1 = vgpr(B.relu1 ? 0 : -2147483647);
            const int acc_shl = vgpr(B.acc_shl), res_shl = vgpr(B.res_shl), loq = vgpr(B.rq.lo), hiq = vgpr(B.rq.hi);
            const unsigned xorq = (unsigned)vgpr((int)B.rq.bias_xor);
    #pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int j = ch + nch * jj;
                if (j >= nco) continue;
                const int cot = j * 32;
                int y[4][4];
    #pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const v4i bv = *(const v4i*)(B.b4 + cot + 8 * gq + 4 * lh);
                    char* const sp = strm + ((size_t)((j * npt + pw) * 4 + gq) * 64 + lane) * 16;
                    v4i rv = {0, 0, 0, 0};
                    if (B.res) rv = *(const v4i*)sp;
    #pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        int v = max((int)((unsigned)acc3[jj][4 * gq + q] + (unsigned)bv[q]), floor0);
                        if (B.res) {
                            const unsigned sres = ((unsigned)v << acc_shl) + ((unsigned)rv[q] << res_shl);
                            v = max((int)sres, floor1);
                        }
                        y[gq][q] = v;
                    }
                    if (B.keep) *(v4i*)sp = v4i{y[gq][0], y[gq][1], y[gq][2], y[gq][3]};
                }
                if constexpr (!LAST) {                               // the next block's expand input, int8 in its format -> X
                    unsigned d[4];
    #pragma unroll
                    for (int gq = 0; gq < 4; ++gq)
                        d[gq] = pack4(requant1(y[gq][0], B.rq.n, loq, hiq), requant1(y[gq][1], B.rq.n, loq, hiq),
                                      requant1(y[gq][2], B.rq.n, loq, hiq), requant1(y[gq][3], B.rq.n, loq, hiq)) ^ xorq;
                    auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
                    auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
                    if (ok) *(v4i*)(X + ((size_t)j * xp + opx) * 32 + lh * 16) = v4i{(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
                    continue;
                }
                if (a.out32 && ok) {
    #pragma unroll
                    for (int gq = 0; gq < 4; ++gq)
                        *(v4i*)(a.out32 + i32t_index(m, cot + 8 * gq + 4 * lh, cout)) = v4i{y[gq][0], y[gq][1], y[gq][2], y[gq][3]};
                }
    #pragma unroll
                for (int q8 = 0; q8 < 2; ++q8) {
                    if (!a.q[q8].ptr) continue;
                    const QuantOut& Q = a.q[q8];
                    unsigned d[4];
    #pragma unroll
                    for (int gq = 0; gq < 4; ++gq)
                        d[gq] = requant_pack4(y[gq][0], y[gq][1], y[gq][2], y[gq][3], Q);
                    auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
                    auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
                    if (ok) *(v4i*)(Q.ptr + (size_t)m * cout + cot + 16 * lh) = v4i{(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
                }
            }
        }
    };
    for (int k = 0; k < a.nblk; ++k) {
        const IRChainBlk& B = a.blk[k];
        const int cin = B.cin, cout = B.cout, nco = cout >> 5, KK1 = cin >> 5;
        const int off_w4 = 64 * cin, off_dw = off_w4 + 64 * cout, off_dwb = off_dw + 640, off_b0 = off_dwb + 256;
        const int nchunk = (B.E32 + 63) >> 6;
        // the generic instance's inner requantisations (FQ == 0) / the float converter's scales (FQ == 1)
        [[maybe_unused]] const int floor_a = vgpr(B.relu_a ? 0 : INT32_MIN), floor_b = vgpr(B.relu_b ? 0 : INT32_MIN);
        [[maybe_unused]] const int lo1 = vgpr(B.r1.lo), hi1 = vgpr(B.r1.hi), lo2 = vgpr(B.r2.lo), hi2 = vgpr(B.r2.hi);
        [[maybe_unused]] const unsigned xor1 = (unsigned)vgpr((int)B.r1.bias_xor), xor2 = (unsigned)vgpr((int)B.r2.bias_xor);
        [[maybe_unused]] const float sc1 = FQ == 1 ? requant_u8_scale(B.r1.n) : 0.0f, sc2 = FQ == 1 ? requant_u8_scale(B.r2.n) : 0.0f;
        if (k > 0) fill_border(B.r1.bias_xor);                    // (the previous block's last P2 is behind a barrier)
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc3[jj][r] = 0;

        for (int e = 0; e < nchunk; ++e) {
            const int nct = (B.E32 - 64 * e) >= 64 ? 2 : 1;    // 32-channel tiles in this chunk (the last chunk may be half)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                  // this chunk's weights, X and the patch border are in LDS; the previous P3 is done
            const int kn = e + 1 < nchunk ? k : k + 1, en = e + 1 < nchunk ? e + 1 : 0;
            const bool more = kn < a.nblk;
            if (more) load_w(a.blk[kn], en);               // in flight during P1 .. P3
            // ================= P1: expand -> patch   (items: (32-channel tile, pixel tile) pairs over the waves)
            for (int it = wave; it < npt * nct; it += NW) {
                const int i = it >= npt ? 1 : 0, pt = it - i * npt;
                v16i acc;
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    v4i bv = {0, 0, 0, 0};
                    if constexpr (FQ) bv = *(const v4i*)(wb + off_b0 + (i * 32 + 8 * gq + 4 * lh) * 4);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[4 * gq + q] = bv[q];
                }
                for (int kk = 0; kk < KK1; ++kk) {
                    const v4i xf = *(const v4i*)(X + ((size_t)kk * xp + pt * 32 + l31) * 32 + lh * 16);
                    const v4i wf = *(const v4i*)(wb + (kk * 64 + i * 32 + l31) * 32 + lh * 16);
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf, xf, acc, 0, 0, 0);
                }
                const int px = pt * 32 + l31;
                const bool ok = px < HW;
                int r, c;
                split_px(ok ? px : 0, r, c);
                unsigned d[4];
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    if constexpr (FQ) {
                        d[gq] = requant_u8x4_sel<FQ == 2 ? 2 : 1>(acc[4 * gq], acc[4 * gq + 1], acc[4 * gq + 2], acc[4 * gq + 3], B.r1.n, sc1) ^ 0x80808080u;
                    } else {
                        const v4i bv = *(const v4i*)(wb + off_b0 + (i * 32 + 8 * gq + 4 * lh) * 4);
                        int y[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) y[q] = requant1(max((int)((unsigned)acc[4 * gq + q] + (unsigned)bv[q]), floor_a), B.r1.n, lo1, hi1);
                        d[gq] = pack4(y[0], y[1], y[2], y[3]) ^ xor1;
                    }
                }
                auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
                auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
                if (ok) {
                    const v4i o = {(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
                    *(v4i*)(patch + (size_t)i * pct + ((size_t)(r + 1) * PW + c + 1) * 32 + lh * 16) = o;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                  // patch complete
            // ================= P2: depthwise 3x3 on the matrix cores: nine MFMAs with DIAGONAL weight fragments per 32-channel tile
            //                   (f8_ir.hip P2MMA: A[c][k] = w[tap][c] for k == c; B = the patch pixels as they lie in LDS)
            for (int pr = wave; pr < npt * nct; pr += NW) {
                const int ctd = pr >= npt ? 1 : 0, pt = pr - ctd * npt;
                v4i wa[9];
                {
                    const int cch = ctd * 32 + l31;
                    const unsigned* wq = (const unsigned*)(wb + off_dw + (cch >> 2) * 36);      // [wA0..3, wB0..3, wC]: dot4 image
                    const unsigned dA = wq[cch & 3], dB = wq[4 + (cch & 3)], dC = wq[8];
                    const bool mine = (l31 >> 4) == lh;
                    const int dsel = (l31 & 15) >> 2, bsh = 8 * (l31 & 3);
#pragma unroll
                    for (int t = 0; t < 9; ++t) {
                        const unsigned wv = t < 4 ? (dA >> (8 * t)) & 0xffu : t < 8 ? (dB >> (8 * (t - 4))) & 0xffu : (dC >> (8 * (cch & 3))) & 0xffu;
                        const int piece = mine ? (int)(wv << bsh) : 0;
                        wa[t] = v4i{dsel == 0 ? piece : 0, dsel == 1 ? piece : 0, dsel == 2 ? piece : 0, dsel == 3 ? piece : 0};
                    }
                }
                const int op = pt * 32 + l31;
                const bool ok2 = op < HW;
                int orow, ocol;
                split_px(ok2 ? op : 0, orow, ocol);
                const char* pp = patch + (size_t)ctd * pct + ((size_t)(orow * PW + ocol)) * 32 + lh * 16;
                v16i acc2;
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const v4i bv = *(const v4i*)(wb + off_dwb + (ctd * 32 + 8 * gq + 4 * lh) * 4);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc2[4 * gq + q] = bv[q];
                }
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const v4i xf = *(const v4i*)(pp + ((t / 3) * PW + t % 3) * 32);
                    acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(wa[t], xf, acc2, 0, 0, 0);
                }
                unsigned d[4];
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    if constexpr (FQ)
                        d[gq] = requant_u8x4_sel<FQ == 2 ? 2 : 1>(acc2[4 * gq], acc2[4 * gq + 1], acc2[4 * gq + 2], acc2[4 * gq + 3], B.r2.n, sc2) ^ 0x80808080u;
                    else
                        d[gq] = pack4(requant1(max(acc2[4 * gq], floor_b), B.r2.n, lo2, hi2), requant1(max(acc2[4 * gq + 1], floor_b), B.r2.n, lo2, hi2),
                                      requant1(max(acc2[4 * gq + 2], floor_b), B.r2.n, lo2, hi2), requant1(max(acc2[4 * gq + 3], floor_b), B.r2.n, lo2, hi2)) ^ xor2;
                }
                auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
                auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
                if (ok2) {
                    const v4i o = {(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
                    *(v4i*)(mid2 + ctd * mid_ct + op * 32 + lh * 16) = o;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                  // mid2 complete
            // ================= P3: project, accumulate over the chunks (pixel tile pw, output-channel tiles ch, ch + nch, ...)
            if (pw < npt) {
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    if (kk >= nct) continue;
                    const v4i xf = *(const v4i*)(mid2 + kk * mid_ct + (pw * 32 + l31) * 32 + lh * 16);
#pragma unroll
                    for (int jj = 0; jj < NJ; ++jj) {
                        const int j = ch + nch * jj;
                        if (j >= nco) continue;
                        const v4i wf = *(const v4i*)(wb + off_w4 + ((kk * cout) + j * 32 + l31) * 32 + lh * 16);
                        acc3[jj] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf, xf, acc3[jj], 0, 0, 0);
                    }
                }
            }
            if (more) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();              // every wave is done reading this chunk's weights
                store_w(a.blk[kn]);
            }
        }

        if (k + 1 < a.nblk) epilogue(B, std::false_type{});
    }
    epilogue(a.blk[a.nblk - 1], std::true_type{});
}

// The register shapes: S0 = every block <= 96 channels in and out, <= 8 pixel tiles (256 pixels: the 14x14 / 13x13 runs, the 8x8 / 12x12 pair of a
// 64x64 / 96x96 net); S1 = inputs <= 160, outputs <= 320 channels, <= 2 pixel tiles (64 pixels: the 7x7 run); S2 = the same channels on <= 4 pixel
// tiles (128 pixels: the 10x10 run at 320x320; five output-channel tiles per wave).
struct IRChainShape { int cin, cout, npw, nw; };
static const IRChainShape kIRChainShapes[3] = {{96, 96, 8, 8}, {160, 320, 2, 8}, {160, 320, 4, 8}};

// LDS bytes of a launch; the stream region holds the widest stream a later block joins (keep_max channels)
static int irchain_lds(int H, int W, int cin_max, int cout_max, int keep_max, IRChainArgs* a) {
    const int npt = (H * W + 31) / 32, xp = npt * 32;
    const int x_bytes = xp * cin_max;
    const int strm = (keep_max / 32) * npt * 4096;
    const int patch = (2 * (H + 2) * (W + 2) * 32 + 255) / 256 * 256;
    const int mid2 = 2 * xp * 32;
    const int wbuf = 64 * cin_max + 64 * cout_max + 640 + 256 + 256;
    if (a) { a->xp = xp; a->off_strm = x_bytes; a->off_patch = x_bytes + strm; a->off_mid2 = x_bytes + strm + patch; a->off_w = x_bytes + strm + patch + mid2; }
    return x_bytes + strm + patch + mid2 + wbuf;
}

static int irchain_shape(int H, int W, int cin_max, int cout_max) {
    const int npt = (H * W + 31) / 32;
    for (int s = 0; s < 3; ++s)
        if (cin_max <= kIRChainShapes[s].cin && cout_max <= kIRChainShapes[s].cout && npt <= kIRChainShapes[s].npw) return s;
    return -1;
}

bool irchain_supported(int H, int W, int cin_max, int cout_max, int keep_max) {
    if (H < 1 || W < 1 || cin_max < 32 || cout_max < 32 || cin_max % 32 || cout_max % 32 || keep_max % 32) return false;
    if (irchain_shape(H, W, cin_max, cout_max) < 0) return false;
    return irchain_lds(H, W, cin_max, cout_max, keep_max, nullptr) <= 160 * 1024;
}

// bits 0-1: FQ (as fused_ir_inst: 0 generic, 1 float-converter requantisation, 2 integer) — both inner requantisations of EVERY block are ReLU ->
// unsigned 8-bit right shifts; bits 2+: the register shape
int irchain_inst(const IRChainArgs& a) {
    bool fqf = a.nblk > 0, small = true;
    int cin_max = 0, cout_max = 0;
    for (int k = 0; k < a.nblk; ++k) {
        const IRChainBlk& B = a.blk[k];
        fqf = fqf && B.relu_a && B.relu_b && B.r1.u8_shr() && B.r2.u8_shr();
        small = small && B.r1.u8_float() && B.r2.u8_float();
        cin_max = cin_max > B.cin ? cin_max : B.cin; cout_max = cout_max > B.cout ? cout_max : B.cout;
    }
    const int fq = !fqf ? 0 : ((a.rq_int || !a.acc_ok || !small) ? 2 : 1);
    const int s = irchain_shape(a.H, a.W, cin_max, cout_max);
    return fq | ((s < 0 ? 0 : s) << 2);
}

int irchain_kernel_name(char* buf, size_t cap, int inst) {
    const IRChainShape& S = kIRChainShapes[(inst >> 2) % 3];
    return snprintf(buf, cap, "f8::irchain_kernel<%d, %d, %d, %d, %d>", S.cin, S.cout, S.npw, S.nw, inst & 3);
}

template <int CIN_MAX, int COUT_MAX, int NPW_MAX, int NW, int FQ>
static hipError_t launch_irchain_t(const IRChainArgs& a, int lds, hipStream_t s) {
    static unsigned long long done = 0;
    int dev = -1;
    if (!dyn_lds_opted_in(&done, &dev)) {
        hipError_t e = hipFuncSetAttribute((const void*)irchain_kernel<CIN_MAX, COUT_MAX, NPW_MAX, NW, FQ>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        if (dev >= 0) __atomic_fetch_or(&done, 1ull << dev, __ATOMIC_RELAXED);
    }
    hipLaunchKernelGGL((irchain_kernel<CIN_MAX, COUT_MAX, NPW_MAX, NW, FQ>), dim3(a.N), dim3(NW * 64), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_irchain(const IRChainArgs& a0, int inst, hipStream_t s) {
    IRChainArgs a = a0;
    if (a.nblk < 1 || a.nblk > kIRChainMaxBlocks || a.N < 1) return hipErrorInvalidValue;
    int cin_max = 0, cout_max = 0, keep_max = 0;
    for (int k = 0; k < a.nblk; ++k) {
        const IRChainBlk& B = a.blk[k];
        cin_max = cin_max > B.cin ? cin_max : B.cin; cout_max = cout_max > B.cout ? cout_max : B.cout;
        if (B.keep && B.cout > keep_max) keep_max = B.cout;
        if (k == 0 && B.res && B.cin > keep_max) keep_max = B.cin;
        if (k > 0 && B.cin != a.blk[k - 1].cout) return hipErrorInvalidValue;
        if (B.res && B.cin != B.cout) return hipErrorInvalidValue;
    }
    const int shape = (inst >> 2) % 3;
    const IRChainShape& S = kIRChainShapes[shape];
    if (cin_max > S.cin || cout_max > S.cout || (a.H * a.W + 31) / 32 > S.npw || !irchain_supported(a.H, a.W, cin_max, cout_max, keep_max)) return hipErrorInvalidValue;
    const int lds = irchain_lds(a.H, a.W, cin_max, cout_max, keep_max, &a);
    const int fq = inst & 3;
#define F8_IRC(C_, O_, P_, W_) return fq == 1 ? launch_irchain_t<C_, O_, P_, W_, 1>(a, lds, s) : fq == 2 ? launch_irchain_t<C_, O_, P_, W_, 2>(a, lds, s) : launch_irchain_t<C_, O_, P_, W_, 0>(a, lds, s);
    if (shape == 0) { F8_IRC(96, 96, 8, 8) }
    if (shape == 1) { F8_IRC(160, 320, 2, 8) }
    F8_IRC(160, 320, 4, 8)
#undef F8_IRC
}

}  // namespace f8
