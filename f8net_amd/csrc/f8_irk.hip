// f8_irk.hip — one launch for an inverted-residual block around a depthwise 5x5 or 7x7 (gfx950; option fuse_irk).
//
//   x8 (int8 NHWC, cin ch) --1x1 cin->E [ReLU]--> e1 --depthwise KxK / s, pad K/2 [ReLU]--> e2 --1x1 E->cout--> [+ x (int32)] -> y
//
// i.e. IntBlock.forward with every int_op_only_fix_quant in place, for the blocks of MnasNet-B1, ProxylessNAS and FBNet.  Unfused the block is
// three launches (conv1x1, dwconvKxK, conv1x1_res) and the 3 - 6x expanded tensors e1 / e2 go through HBM twice.
//
// The decomposition is f8_ir.hip's (text copied, not shared: that kernel's allocation is measured).  The expanded dimension E goes in CHUNKS of
// 64 channels; per chunk
//   P1  expand: e1[chunk] for the tile's input rows (MFMA, K = cin)           -> requant -> LDS patch (border = the depthwise input's pad value)
//   P2  depthwise KxK on the patch (v_dot4 over four ROWS of one input column) -> requant -> LDS mid2, in P3's operand order
//   P3  project: acc[out px][cout] += W4[:, chunk] . mid2 (MFMA, K = 64)      accumulators stay in registers across the chunks
// with the next chunk's weight slices loaded into registers while this one computes.  Two barriers per chunk + one in front.
//
// New against f8_ir.hip:
//   P2 is dwconvk_dot4_kernel's scheme (f8_dwk.hip) on the padded patch: one item = 4 channels x IRK_PIX adjacent output pixels of one row; the
//   item walks the (IRK_PIX - 1) * s + K patch columns of its pixels once, byte-transposes each column's K rows into one dword per channel and
//   row group and feeds it to every pixel whose window holds it.  The patch carries its own border, so there are no range checks; weights are
//   pack_dwk_weights' image, one chunk (16 quads) at a time.
//   cin and cout are run-time values (multiples of 32, cin <= 192); the kernel is instantiated by an output-channel CAP (96 / 192 / 320), as
//   irchain_kernel is.  All instances are f8_ir.hip's SPLIT form: 8 waves, four pixel tiles of 32 output pixels, waves 4 - 7 take the second
//   32 expanded channels of a chunk in P1 and the upper output-channel tiles in P3 / the epilogue.
//   Work unit: R output rows x full width (R * Wo <= 128; the last tile of an image may be ragged), or G whole images when a map has <= 128
//   output pixels.  P1 recomputes the halo rows: PR = (R - 1) * s + K patch rows for R output rows.
#include "f8_device.h"

namespace f8 {

namespace {
constexpr int IRK_NW = 8, IRK_NT = IRK_NW * 64;
constexpr int IRK_PXW = 4;                            // waves that own an output pixel tile (the other four: the same tiles' upper channels)
constexpr int IRK_MAX_PX = IRK_PXW * 32;              // output pixels of a tile
constexpr int IRK_CIN_MAX = 192;                      // widest block input (padded)
constexpr int IRK_PIX = 4;                            // adjacent output pixels per P2 item
constexpr int irk_dw_bytes(int K) { return 16 * K * ((K + 3) / 4) * 16; }   // one chunk (16 quads) of pack_dwk_weights' image
}

// P2, one item: 4 channels (one dword per patch pixel) x up to IRK_PIX adjacent output pixels of one row.
//   pp      the patch at (first input row, first input column) of pixel 0, this item's channel quad; PWB = bytes of a patch row
//   ncol    patch columns from there to the row's end: columns beyond it are read as the last one (only pixels beyond Wo see them)
//   wq      the quad's weights [K columns][G row groups][4 channels] dwords (LDS);  bv: the quad's bias
//   mo      mid2 at pixel 0, this quad (32 bytes per pixel);  npix: pixels to write
// The column loop is NOT unrolled (S is a run-time value): unrolled, the compiler hoists every column's loads and weights and the item alone takes ~170
// registers next to the project accumulators, which stay live through this phase.
template <int K, int FQ>
__device__ __forceinline__ void irk_p2_item(const char* pp, int PWB, int ncol, int S, const unsigned* wq, const v4i bv, char* mo, int npix,
                                            int n2, int lo2, int hi2, unsigned xor2, int floor_b) {
    constexpr int PIX = IRK_PIX;
    const int NCOL = (PIX - 1) * S + K;              // input columns the item's pixels read
    constexpr int G = (K + 3) / 4;                   // groups of four rows
    constexpr int LAST = K - 4 * (G - 1);            // rows of the last group: 3 (K = 7) or 1 (K = 5)
    static_assert(LAST == 1 || LAST == 3, "K is 5 or 7");
    int acc[PIX][4];
#pragma unroll
    for (int j = 0; j < PIX; ++j) { acc[j][0] = bv.x; acc[j][1] = bv.y; acc[j][2] = bv.z; acc[j][3] = bv.w; }
#pragma unroll 1
    for (int cc = 0; cc < NCOL; ++cc) {
        const char* pc = pp + min(cc, ncol - 1) * 32;
        unsigned t[K];                                // rows 0 .. K - 1 of this column, 4 channels each
#pragma unroll
        for (int r = 0; r < K; ++r) t[r] = *(const unsigned*)(pc + r * PWB);
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
        // every pixel j whose window [j * S, j * S + K) holds column cc: kernel column s = cc - j * S (wave-uniform)
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
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        unsigned d;
        if constexpr (FQ) d = requant_u8x4_int(acc[j][0], acc[j][1], acc[j][2], acc[j][3], n2) ^ 0x80808080u;
        else d = pack4(requant1(max(acc[j][0], floor_b), n2, lo2, hi2), requant1(max(acc[j][1], floor_b), n2, lo2, hi2),
                       requant1(max(acc[j][2], floor_b), n2, lo2, hi2), requant1(max(acc[j][3], floor_b), n2, lo2, hi2)) ^ xor2;
        if (j < npix) *(unsigned*)(mo + j * 32) = d;
    }
}

// K: depthwise kernel size (5 / 7).  COUT_MAX: cap of the padded output channels (the project accumulators: COUT_MAX / 32 tiles of 16 registers,
// half of them per wave).  FQ == 2: both inner requantisations are right shifts into UNSIGNED 8-bit behind a ReLU, in integer operations
// (requant_u8x4_int; the ReLU is the clamp's lower bound, the bias rides in the accumulators' start value); FQ == 0: any format (requant1).
template <int K, int COUT_MAX, int FQ>
__global__ void __launch_bounds__(IRK_NT, 2) fused_irk_kernel(const IRKArgs a) {
    constexpr int NT = IRK_NT, PXW = IRK_PXW;
    constexpr int MID2_CT = PXW * 1024;                    // bytes of one 32-channel plane of mid2: PXW pixel tiles x 32 px x 32 B
    constexpr int NCO = COUT_MAX / 32, NH = (NCO + 1) / 2;  // output-channel tiles; those a wave holds (the lower or the upper half)
    constexpr int PAD = K / 2, GK = (K + 3) / 4;
    constexpr int DWB = irk_dw_bytes(K), DW_SLOTS = DWB / 16, SM_SLOTS = DW_SLOTS + 16 + 16;   // dw weights, dw bias, expand bias
    static_assert(SM_SLOTS <= NT, "one slot per thread");
    constexpr int W0_L = (IRK_CIN_MAX * 4 + NT - 1) / NT, W4_L = (COUT_MAX * 4 + NT - 1) / NT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* const X = lds;                                   // [kk1][xp][32 B]
    char* const patch = lds + a.off_patch;                 // [2][G][PR][PW][32 B]: channel-tile planes
    char* const mid2 = lds + a.off_mid2;                   // [2][128][32 B]
    char* const wbuf = lds + a.off_w;                      // 2 x { W0 [kk1][64][32] | W4 [2][cout][32] | dw image DWB | dw bias 256 B | b0 256 B }
    const int cin = a.cin, cout = a.cout, kk1 = cin >> 5, nco = cout >> 5;
    const int w0_slots = cin * 4, w4_slots = cout * 4;
    const int OFF_W4 = 64 * cin, OFF_DW = OFF_W4 + cout * 64, OFF_DWB = OFF_DW + DWB, OFF_B0 = OFF_DWB + 256, WBUF = OFF_B0 + 256;
    const int jsplit = (nco + 1) >> 1;                     // output-channel tiles [0, jsplit) on waves 0 - 3, the rest on waves 4 - 7

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & (IRK_NW - 1);
    const int l31 = lane & 31, lh = lane >> 5;
    const int pw = wave & 3, ch = wave >> 2;
    const int j0 = ch * jsplit, j1 = ch == 0 ? jsplit : nco;   // this wave's output-channel tiles [j0, j1): accumulator jl holds tile j0 + jl
    const int s = a.stride, R = a.R, W = a.W, H = a.H, Wo = a.Wo, Ho = a.Ho, PW = W + 2 * PAD;
    const int PR = (R - 1) * s + K;
    const int pct = a.G * PR * PW * 32;                    // bytes of one 32-channel plane of the patch
    int t;
    {   // XCD-aware order: vertically adjacent row tiles share their halo rows in one XCD's L2
        const int nwg = gridDim.x, bid = blockIdx.x, xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
        t = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
    }
    int n0, p0;
    if (a.G > 1) { n0 = t * a.G; p0 = 0; } else { n0 = t / a.tiles_per_img; p0 = (t - n0 * a.tiles_per_img) * R; }
    const int Geff = (a.N - n0) < a.G ? (a.N - n0) : a.G;
    const int in_row0 = p0 * s - PAD;
    const int vr0 = in_row0 < 0 ? 0 : in_row0, vr1 = (in_row0 + PR) > H ? H : (in_row0 + PR), nvr = vr1 - vr0;
    const int P1_PX = Geff * nvr * W, np1 = (P1_PX + 31) >> 5;
    const int RWo = R * Wo, OUT_PX = Geff * RWo;
    const int nchunk = (a.E32 + 63) >> 6;
    // pixel index -> (image g, row, column) without hardware division (host magic numbers).  Row tiles (G == 1) have g == 0;
    // whole-image tiles (G > 1) have nvr == H.
    auto split_in = [&](int px, int& g, int& vr, int& c) {
        g = a.G > 1 ? (int)fast_div((unsigned)px, a.dHW) : 0;
        const int r = px - g * nvr * W;
        vr = (int)fast_div((unsigned)r, a.dW);
        c = r - vr * W;
    };
    auto split_out = [&](int op, int& g, int& orow, int& ocol) {
        g = a.G > 1 ? (int)fast_div((unsigned)op, a.dRWo) : 0;
        const int r = op - g * RWo;
        orow = (int)fast_div((unsigned)r, a.dWo);
        ocol = r - orow * Wo;
    };

    // ---- block input tile -> X (k-blocked: [kk][px][32 B], so a fragment read is 1 KB contiguous per wave)
    {
        const int per_kk = a.xp * 2, nslot = per_kk * kk1;
        for (int kk = 0; kk < kk1; ++kk)
            for (int rem = tid; rem < per_kk; rem += NT) {
                const int px = rem >> 1, half = rem & 1;
                v4i v = {0, 0, 0, 0};
                if (px < P1_PX) {
                    int g, vr, c;
                    split_in(px, g, vr, c);
                    const size_t gpx = ((size_t)(n0 + g) * H + vr0 + vr) * W + c;
                    v = *(const v4i*)(a.x8 + gpx * cin + kk * 32 + half * 16);
                }
                *(v4i*)(X + ((size_t)kk * per_kk + rem) * 16) = v;
            }
        (void)nslot;
    }
    // ---- patch <- the depthwise input's pad value (border columns, rows outside the image; P1 only ever writes interior pixels)
    {
        const v4i zv = {(int)a.xor1, (int)a.xor1, (int)a.xor1, (int)a.xor1};
        const int pb = a.G * PR * PW * 64;
        for (int o = tid * 16; o < pb; o += NT * 16) *(v4i*)(patch + o) = zv;
    }

    // ---- weight slices of one chunk: global -> registers (early) -> LDS (late)
    v4i rw0[W0_L], rw4[W4_L], rsm;
    auto load_w = [&](int e) {
        const int rows_ok = a.E32 - 64 * e;                // expanded channels left from this chunk on (>= 32)
#pragma unroll
        for (int i = 0; i < W0_L; ++i) {                   // W0 rows 64e .. 64e+63 -> [kk][row][32 B]
            const int sl = tid + i * NT;
            const int kk = sl >> 7, row = (sl >> 1) & 63, half = sl & 1;
            v4i v = {0, 0, 0, 0};
            if (sl < w0_slots && row < rows_ok) v = *(const v4i*)(a.w0 + (size_t)(64 * e + row) * cin + kk * 32 + half * 16);
            rw0[i] = v;
        }
#pragma unroll
        for (int i = 0; i < W4_L; ++i) {                   // W4 columns 64e .. 64e+63 of every row -> [kk][row][32 B]
            const int sl = tid + i * NT;
            const int kk = sl >= cout * 2 ? 1 : 0, rh = sl - kk * cout * 2, row = rh >> 1, half = rh & 1;
            v4i v = {0, 0, 0, 0};
            if (sl < w4_slots && kk * 32 < rows_ok) v = *(const v4i*)(a.w4 + (size_t)row * a.E32 + 64 * e + kk * 32 + half * 16);
            rw4[i] = v;
        }
        {   // depthwise weights (pack_dwk_weights' image: K * GK * 16 B per 4-channel quad), depthwise bias, expand bias: 64 channels each
            v4i v = {0, 0, 0, 0};
            if (tid < DW_SLOTS) { if (tid * 16 + 16 <= (rows_ok >= 64 ? DWB : DWB / 2)) v = *(const v4i*)(a.wd4 + (size_t)e * DWB + tid * 16); }
            else if (tid < DW_SLOTS + 16) { const int i = tid - DW_SLOTS; if (4 * i < rows_ok) v = *(const v4i*)(a.bd4 + 64 * e + 4 * i); }
            else if (tid < SM_SLOTS) { const int i = tid - DW_SLOTS - 16; if (4 * i < rows_ok) v = *(const v4i*)(a.b0 + 64 * e + 4 * i); }
            rsm = v;
        }
    };
    auto store_w = [&](int buf) {
        char* wb = wbuf + buf * WBUF;
#pragma unroll
        for (int i = 0; i < W0_L; ++i) { const int sl = tid + i * NT; if (sl < w0_slots) *(v4i*)(wb + sl * 16) = rw0[i]; }
#pragma unroll
        for (int i = 0; i < W4_L; ++i) { const int sl = tid + i * NT; if (sl < w4_slots) *(v4i*)(wb + OFF_W4 + sl * 16) = rw4[i]; }
        if (tid < DW_SLOTS) *(v4i*)(wb + OFF_DW + tid * 16) = rsm;
        else if (tid < DW_SLOTS + 16) *(v4i*)(wb + OFF_DWB + (tid - DW_SLOTS) * 16) = rsm;
        else if (tid < SM_SLOTS) *(v4i*)(wb + OFF_B0 + (tid - DW_SLOTS - 16) * 16) = rsm;
    };
    load_w(0);
    store_w(0);

    v16i acc3[NH];
#pragma unroll
    for (int j = 0; j < NH; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc3[j][r] = 0;
    const int floor_a = a.relu_a ? 0 : INT32_MIN, floor_b = a.relu_b ? 0 : INT32_MIN;
    (void)floor_a;
    const int QS = a.QS, RQS = R * QS, PWB = PW * 32;

    for (int e = 0; e < nchunk; ++e) {
        const char* wb = wbuf + (e & 1) * WBUF;
        const int nct = (a.E32 - 64 * e) >= 64 ? 2 : 1;    // 32-channel tiles in this chunk (the last chunk may be half)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                      // this chunk's weight slices are in LDS (chunk 0: also X and the patch border);
                                                           // every wave is done with the previous chunk's P3 (mid2) and P2 (patch)
        if (e + 1 < nchunk) load_w(e + 1);                 // in flight during P1 .. P3
        // ================= P1: expand -> patch (wave: pixel tiles pw, pw + 4, ..; channel tile ch of the chunk)
        if (ch < nct) {
            for (int pt = pw; pt < np1; pt += PXW) {
                v16i acc;
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    v4i bv = {0, 0, 0, 0};
                    if constexpr (FQ) bv = *(const v4i*)(wb + OFF_B0 + (ch * 32 + 8 * gq + 4 * lh) * 4);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[4 * gq + q] = bv[q];
                }
                for (int kk = 0; kk < kk1; ++kk) {
                    const v4i xf = *(const v4i*)(X + ((size_t)kk * a.xp + pt * 32 + l31) * 32 + lh * 16);
                    const v4i wf = *(const v4i*)(wb + (kk * 64 + ch * 32 + l31) * 32 + lh * 16);
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf, xf, acc, 0, 0, 0);
                }
                const int px = pt * 32 + l31;
                const bool ok = px < P1_PX;
                const int pxc = ok ? px : 0;
                int g, vr, c;
                split_in(pxc, g, vr, c);
                const int ent = (g * PR + (vr0 + vr - in_row0)) * PW + c + PAD;
                unsigned d[4];
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    if constexpr (FQ) {
                        d[gq] = requant_u8x4_int(acc[4 * gq], acc[4 * gq + 1], acc[4 * gq + 2], acc[4 * gq + 3], a.n1) ^ 0x80808080u;
                    } else {
                        int y[4];
                        const v4i bv = *(const v4i*)(wb + OFF_B0 + (ch * 32 + 8 * gq + 4 * lh) * 4);
#pragma unroll
                        for (int q = 0; q < 4; ++q) y[q] = requant1(max((int)((unsigned)acc[4 * gq + q] + (unsigned)bv[q]), floor_a), a.n1, a.lo1, a.hi1);
                        d[gq] = pack4(y[0], y[1], y[2], y[3]) ^ a.xor1;
                    }
                }
                auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
                auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
                if (ok) {
                    const v4i o = {(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
                    *(v4i*)(patch + (size_t)ch * pct + (size_t)ent * 32 + lh * 16) = o;
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                      // patch complete
        // ================= P2: depthwise KxK on the patch -> mid2 (item = channel quad x IRK_PIX pixels of one output row)
        {
            const int npg = Geff * RQS, nitems = npg * nct * 8;
            for (int it = tid; it < nitems; it += NT) {
                const int cq = it & 7;
                int rest = it >> 3;
                const int ct = rest >= npg ? 1 : 0;
                rest -= ct * npg;
                const int g = a.G > 1 ? (int)fast_div((unsigned)rest, a.dRQS) : 0;
                const int r2 = rest - g * RQS;
                const int orow = (int)fast_div((unsigned)r2, a.dQS);
                const int q0 = (r2 - orow * QS) * IRK_PIX;
                const char* pp = patch + (size_t)ct * pct + (size_t)((g * PR + orow * s) * PW + q0 * s) * 32 + cq * 4;
                const unsigned* wq = (const unsigned*)(wb + OFF_DW) + (ct * 8 + cq) * (K * GK * 4);
                const v4i bv = *(const v4i*)(wb + OFF_DWB + (ct * 32 + cq * 4) * 4);
                char* mo = mid2 + ct * MID2_CT + ((g * R + orow) * Wo + q0) * 32 + cq * 4;
                const int npix = min(IRK_PIX, Wo - q0), ncol = PW - q0 * s;
                irk_p2_item<K, FQ>(pp, PWB, ncol, s, wq, bv, mo, npix, a.n2, a.lo2, a.hi2, a.xor2, floor_b);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                      // mid2 complete
        // ================= P3: project, accumulate over the chunks (wave = output pixel tile pw, its half of the output-channel tiles)
        if (pw * 32 < OUT_PX) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                if (kk >= nct) continue;
                const v4i xf = *(const v4i*)(mid2 + kk * MID2_CT + (pw * 32 + l31) * 32 + lh * 16);
#pragma unroll
                for (int jl = 0; jl < NH; ++jl) {
                    if (j0 + jl >= j1) continue;
                    const v4i wf = *(const v4i*)(wb + OFF_W4 + ((kk * cout) + (j0 + jl) * 32 + l31) * 32 + lh * 16);
                    acc3[jl] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf, xf, acc3[jl], 0, 0, 0);
                }
            }
        }
        if (e + 1 < nchunk) store_w((e + 1) & 1);          // the other buffer was last read in the previous chunk (barriers above)
    }

    // ================= epilogue: bias, [align + int32 residual + clamp], int32 (I32T) and / or int8 copies
    const int opx = pw * 32 + l31;
    if (pw * 32 >= OUT_PX) return;
    int g, orow, ocol;
    split_out(opx < OUT_PX ? opx : 0, g, orow, ocol);
    const bool ok = opx < OUT_PX && p0 + orow < Ho;        // (the last row tile of an image may be ragged)
    if (!ok) { g = 0; orow = 0; ocol = 0; }
    const int m = ((n0 + g) * Ho + p0 + orow) * Wo + ocol;
    const int floor0 = a.relu0 ? 0 : INT32_MIN, floor1 = a.relu1 ? 0 : -2147483647;
#pragma unroll
    for (int jl = 0; jl < NH; ++jl) {
        if (j0 + jl >= j1) continue;
        const int cot = (j0 + jl) * 32;
        int y[4][4];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const v4i bv = *(const v4i*)(a.b4 + cot + 8 * gq + 4 * lh);
            v4i rv = {0, 0, 0, 0};
            if (a.xr && ok) rv = *(const v4i*)(a.xr + i32t_index(m, cot + 8 * gq + 4 * lh, cout));
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int v = max((int)((unsigned)acc3[jl][4 * gq + q] + (unsigned)bv[q]), floor0);
                if (a.xr) {
                    const unsigned sres = ((unsigned)v << a.acc_shl) + ((unsigned)rv[q] << a.res_shl);
                    v = max((int)sres, floor1);
                }
                y[gq][q] = v;
            }
        }
        if (a.out32 && ok) {
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const v4i o = {y[gq][0], y[gq][1], y[gq][2], y[gq][3]};
                *(v4i*)(a.out32 + i32t_index(m, cot + 8 * gq + 4 * lh, cout)) = o;
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!a.q[k].ptr) continue;
            unsigned d[4];
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
                d[gq] = requant_pack4(y[gq][0], y[gq][1], y[gq][2], y[gq][3], a.q[k]);
            auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
            auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
            if (ok) {
                const v4i o = {(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
                *(v4i*)(a.q[k].ptr + (size_t)m * cout + cot + 16 * lh) = o;
            }
        }
    }
}

// the output-channel cap of the instance that runs padded cout (0: none)
static int irk_cap(int coutS) { return coutS <= 96 ? 96 : coutS <= 192 ? 192 : coutS <= 320 ? 320 : 0; }

bool irk_supported(int K, int cinS, int coutS) {
    return (K == 5 || K == 7) && cinS >= 32 && cinS <= IRK_CIN_MAX && (cinS & 31) == 0 && coutS >= 32 && (coutS & 31) == 0 && irk_cap(coutS) != 0;
}

// LDS layout of a tile (bytes); false if it does not fit
static bool irk_layout(int K, int cinS, int coutS, int H, int W, int stride, int R, int G, IRKArgs* a, int* lds_bytes) {
    const int PR = (R - 1) * stride + K, PW = W + 2 * (K / 2);
    const int rows = PR < H ? PR : H;                       // valid input rows of a tile are at most this many
    const int xp = (G * rows * W + 31) / 32 * 32;
    const int x_bytes = xp * cinS;
    const int patch = (G * PR * PW * 64 + 255) / 256 * 256;
    const int wbuf = 64 * cinS + coutS * 64 + irk_dw_bytes(K) + 256 + 256;
    const int mid2 = 2 * IRK_MAX_PX * 32;
    const int total = x_bytes + patch + mid2 + 2 * wbuf;
    if (a) { a->xp = xp; a->off_patch = x_bytes; a->off_mid2 = x_bytes + patch; a->off_w = x_bytes + patch + mid2; }
    if (lds_bytes) *lds_bytes = total;
    return total <= 160 * 1024;
}

// Tile choice.  A map of at most 128 output pixels: G whole images (G <= 8, G * Ho * Wo <= 128), fewer while the layout does not fit — whole images
// need no halo recompute.  Else R output rows x full width: the fewest row tiles with R * Wo <= 128 that fit LDS, their rows evened out
// (R = ceil(Ho / tiles): the last tile is ragged when R does not divide Ho).
bool irk_config(int K, int cinS, int coutS, int H, int W, int stride, int* R, int* G) {
    if (!irk_supported(K, cinS, coutS) || (stride != 1 && stride != 2) || H < 1 || W < 1) return false;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if (Wo > IRK_MAX_PX) return false;
    if (Ho * Wo <= IRK_MAX_PX) {
        int g = IRK_MAX_PX / (Ho * Wo);
        if (g > 8) g = 8;
        while (g > 1 && !irk_layout(K, cinS, coutS, H, W, stride, Ho, g, nullptr, nullptr)) --g;
        if (irk_layout(K, cinS, coutS, H, W, stride, Ho, g, nullptr, nullptr)) { *R = Ho; *G = g; return true; }
    }
    int r = IRK_MAX_PX / Wo;
    if (r > Ho) r = Ho;
    while (r >= 1 && !irk_layout(K, cinS, coutS, H, W, stride, r, 1, nullptr, nullptr)) --r;
    if (r < 1) return false;
    const int tiles = (Ho + r - 1) / r;
    *R = (Ho + tiles - 1) / tiles; *G = 1;
    return true;
}

template <int K, int COUT_MAX, int FQ>
static hipError_t launch_irk_t(const IRKArgs& a, int lds, hipStream_t s) {
    // dynamic LDS above 64 KB must be opted into per kernel AND per device (a process may drive several GPUs): keep the maximum per device
    static int attr_lds[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || lds > attr_lds[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)fused_irk_kernel<K, COUT_MAX, FQ>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        if (dev >= 0) attr_lds[dev] = lds;
    }
    const int grid = a.G > 1 ? (a.N + a.G - 1) / a.G : a.N * a.tiles_per_img;
    hipLaunchKernelGGL((fused_irk_kernel<K, COUT_MAX, FQ>), dim3(grid), dim3(IRK_NT), lds, s, a);
    return hipGetLastError();
}

// 2: ReLU + right shift into unsigned 8-bit after the expand AND the depthwise conv, in integer operations (whatever requant_float says: the
// general depthwise launches have no float-converter form either); 0: any format
int irk_inst(const IRKArgs& a) {
    return (a.relu_a && a.relu_b && a.r1().u8_shr() && a.r2().u8_shr()) ? 2 : 0;
}

int irk_kernel_name(char* buf, size_t cap, int K, int coutS, int inst) {
    return snprintf(buf, cap, "f8::fused_irk_kernel<%d, %d, %d>", K, irk_cap(coutS), inst);
}

hipError_t launch_fused_irk(const IRKArgs& a0, int inst, hipStream_t s) {
    IRKArgs a = a0;
    int lds = 0;
    if (!irk_supported(a.K, a.cin, a.cout) || a.R < 1 || a.G < 1 || a.G * a.R * a.Wo > IRK_MAX_PX || (a.G > 1 && a.R != a.Ho) ||
        !irk_layout(a.K, a.cin, a.cout, a.H, a.W, a.stride, a.R, a.G, &a, &lds)) return hipErrorInvalidValue;
    const int cap = irk_cap(a.cout);
#define F8_IRK(K_, O_) if (a.K == K_ && cap == O_) return inst == 2 ? launch_irk_t<K_, O_, 2>(a, lds, s) : launch_irk_t<K_, O_, 0>(a, lds, s);
    F8_IRK(5, 96) F8_IRK(5, 192) F8_IRK(5, 320) F8_IRK(7, 96) F8_IRK(7, 192) F8_IRK(7, 320)
#undef F8_IRK
    return hipErrorInvalidValue;
}

}  // namespace f8
