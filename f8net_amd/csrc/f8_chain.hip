// f8_chain.hip — ALL consecutive bottleneck blocks of a ResNet stage in one launch; the int32 residual stream never leaves the chip.
//
// IntBlock.forward of /root/reference/models/fix_resnet.py:26-77, applied NBLK times in a row as IntModel.forward does for the
// blocks of one stage (fix_resnet.py:361-366), every int_op_only_fix_quant (fix_quant_ops.py:90-114) in place.
//
// Why: with one launch per block (f8_fused.hip) a block is bound by its int32 residual stream — 4 bytes in and 4 bytes out per
// element against 1 + 1 for the int8 activations: 80 % of the bytes of the 56x56 / 28x28 / 14x14 blocks, which together were 60 %
// of ResNet-50's kernel time at 0.44-0.56 of the HBM peak.  The stream only exists BETWEEN blocks.  Here a workgroup owns a tile of
// R rows x full width of one image and keeps the tile's int32 stream in REGISTERS (NPT x C/8 accumulator registers per lane: 112-128
// of the 256 a wave has) across all the blocks of the stage; per block it reads nothing but weights (L2-resident, streamed straight
// into registers in MFMA-fragment order) and writes nothing.  HBM sees the stage input once and the stage output once.
//
//   per block, per tile:   x8 (LDS, int8) --1x1, ReLU--> mid1 (LDS patch) --3x3, ReLU--> mid2 (LDS) --1x1--> + stream (registers)
//                          -> clamp, ReLU -> stream' (registers) -> requant -> x8' (LDS)
//
// The 3x3 needs one row of mid1 above and below the tile: vertically adjacent tiles of an image run on different CUs at the same
// time and swap those rows (3.5 KB each) through global memory once per block, by the protocol of f8_chain_common.h: write-through
// (sc0 sc1) stores, drain, barrier, one flag; one lane polls the neighbour's flag, barrier, sc0 sc1 loads
// (cdna_hip_programming.md Guideline 16, form {sc0 sc1 stores and loads on both sides}); nothing depends on placement or dispatch
// order: a workgroup's place in the grid is a TICKET it draws when it starts, so the set of started workgroups is always a prefix of
// the logical grid, the tiles of one image are consecutive tickets, and a group whose last member has not started yet is the only
// one that waits — on workgroups that start as soon as any other one finishes.  Every spin is bounded (error word, kernel exits).
//
// 512 threads = 8 waves.  P1 / P2: wave (mt, pg) computes mid channel tile mt for pixel tiles pg, pg + PG, ...; P3: wave w owns
// channel tiles [w CT/8, (w+1) CT/8) of the stream for all pixel tiles.  No barrier inside a K loop: B operands are read-only LDS,
// A operands rotate through NBUF register batches of NB K-steps; every (workgroup, wave) walks K in a rotated order (integer sums
// are exact in any order) so that the workgroups do not all ask the L2 for the same kilobyte at the same moment (f8_p12.hip).
#include "f8_chain_common.h"
#include <cstdio>
#include <cstdlib>

namespace f8 {

// BROT: only TWO blocks' biases are resident (the current block's and the next one's, which is fetched during the current block) instead of
// every block's: the TAIL instances need the 18-30 KB for the shortcut's operand
// ALIAS (round 6, the two-workgroups-per-CU instance): the shortcut's operand of a TAIL first block shares the patch's bytes — the join reads xin and
// mid2 only, the patch is first written (border fill, P1) behind the join's closing barrier, and the next image's operand is committed behind the
// barrier that ends the previous image
template <int C, int MID, int W, int H, int R, int CIN0, bool BROT_ = false, bool ALIAS_ = false>
struct ChainCfg {
    static constexpr bool BROT = BROT_, ALIAS = ALIAS_;
    static constexpr int BSLOTS = BROT ? 2 : kChainMaxBlocks;
#ifdef F8_CH_ABL_NORAG          // tuning build (results invalid): an ablation of the UNSTACKED form (run it with F8_CHAIN_STACK=0) — no ragged last
                                // tile, a 14x14 image runs 3 tiles of 4 rows, rows 12-13 are not computed; the host still sizes the groups for 4 tiles
    static constexpr int T = H / R;
#else
    static constexpr int T = (H + R - 1) / R;                  // tiles (workgroups) per image
#endif
    // STACKABLE: H rows are not whole tiles but 2H are (14x14, R = 4: 3.5 tiles per image, 7 per pair).  With ChainArgs::stack = 2 a tile column
    // is an image PAIR — in NHWC row 0 of image n + 1 follows row H - 1 of image n, so a pair is one contiguous 2H-row map — and T2 tiles cover it.
    // The 3x3 must not read across the seam between the two images: lanes of row H - 1 take their bottom taps, lanes of row H their top taps, from
    // ZPAD, three patch entries of biased zero at the end of LDS (the tile that spans the seam holds both rows; every other tile's lanes never point there)
    static constexpr bool STACKABLE = H % R != 0 && (2 * H) % R == 0;
    static constexpr int T2 = STACKABLE ? 2 * H / R : T;       // tiles per image pair
    static constexpr int PX = R * W, NPT = (PX + 31) / 32, ROWS = NPT * 32;
    static constexpr int PW = W + 2, PR = R + 2;
    // LDS rows are PADDED by 16 bytes instead of XOR-swizzled: the 16 lanes of a ds_read_b128 service group read consecutive rows
    // at one K offset, a row stride of 16 (mod 256) bytes spreads them over all 64 banks, and every address of the unrolled K loops
    // is ONE per-lane base register plus an immediate
    static constexpr int XS = C + 16, MS = MID + 16, IS = CIN0 + 16;
    static constexpr int X8_BYTES = ROWS * XS;
    static constexpr int PATCH_BYTES = (PR * PW * MS + 255) / 256 * 256;
    static constexpr int MID2_BYTES = ROWS * MS;
    static constexpr int XIN_BYTES = CIN0 != C ? ROWS * IS : 0;
    static constexpr int BIAS_INTS = 2 * MID + C;              // per block: b0 | b2 | b4
    static constexpr int BIAS_BYTES = (BSLOTS * BIAS_INTS + (CIN0 != C ? C : 0)) * 4;   // + bsc of the stage-opening block
    static constexpr int MISC_BYTES = 256;
    static_assert(!ALIAS || XIN_BYTES <= PATCH_BYTES, "ALIAS: the shortcut's operand fits the patch");
    static constexpr int ZPAD_BYTES = STACKABLE ? 3 * MS : 0;
    static constexpr int ZPAD_OFF = X8_BYTES + PATCH_BYTES + MID2_BYTES + (ALIAS ? 0 : XIN_BYTES) + BIAS_BYTES + MISC_BYTES;
    static constexpr int LDS_BYTES = ZPAD_OFF + ZPAD_BYTES;
    static constexpr int ROWB = W * MID;                       // one exchanged row of mid1
    static_assert(LDS_BYTES <= 160 * 1024 && ZPAD_OFF % 16 == 0, "LDS");
    static_assert(X8_BYTES < 65536 + 4096 && PATCH_BYTES < 65536 && MID2_BYTES < 65536, "immediate offsets");
    static_assert(ROWB / 16 <= 256 && (size_t)512 * 4 * ROWB <= kChainXchgBytes, "one 16-byte piece of a halo row per thread of a half workgroup");
};

// FAST: every block has ReLU after body.0 / body.2 / the join, every int8 format of the chain is unsigned with a right shift, and the
// stream itself is never shifted (res_shl == 0) — true for the real fraclen tables; the generic instance takes everything else.
// ROT: rotate the K order per (workgroup, wave) in coarse groups (L2-bound instance: all workgroups stream the same weights).
// TAIL (round 4): the first block is only the JOIN of a stage-opening block whose 3x3 and shortcut have stride 2 (fix_resnet.py:55-77): body.0 and
// body.2 ran in f8_opener.hip (P12) and left mid2 in HBM; here the tile loads mid2 and the shortcut's operand (pixels (2p, 2q) of the block input,
// CIN0 channels) into LDS and computes  stream = clamp(((Wsc . x + bsc) << sa) + ((W4 . mid2 + b4) << sr)) [ReLU]  straight into the stream
// registers, weights streamed — the block's int32 output (205 MB per 128 images in ResNet-50's stage 1) is neither written nor read back.
// NW (round 6): waves per workgroup.  8 = one workgroup per CU, two waves per SIMD in lock step through the phases.  4 (the 28x28 instances with R = 2:
// chain_shape) = HALF the tile per workgroup and TWO workgroups per CU, 256 registers per wave as before, one wave of each per SIMD: the two
// workgroups drift apart, so one's matrix-bound K loops run beside the other's vector-bound join / requantisation and one's barrier and halo waits
// under the other's work (tools/ubench/ubench_pingpong.hip mode 3: +10.5 % for the M + V pair alone).  Per wave the shapes are the 8-wave instance's
// (two pixel tiles per weight fragment in P1 / P2, CT / NW channel tiles x NPT pixel tiles of stream = 128 registers).
template <int C, int MID, int W, int H, int R, int CIN0, int NB, int NBUF, int FAST, bool ROT, bool TAIL = false, int NW = 8>
__global__ void __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu((R < 4 && NW == 8) ? 4 : 2, (R < 4 && NW == 8) ? 4 : 2)))
chain_kernel(const ChainArgs a) {
    using Cfg = ChainCfg<C, MID, W, H, R, CIN0, TAIL || R < 4, TAIL && NW == 4>;
    constexpr int NT = NW * 64;
    constexpr bool BROT = Cfg::BROT;
    constexpr int BSLOTS = Cfg::BSLOTS;
    constexpr bool DS0 = CIN0 != C;
    static_assert(!TAIL || (DS0 && ((R * W + 31) / 32) % 2 == 0), "TAIL: an opening block; an even number of pixel tiles");
    constexpr int T = Cfg::T, NPT = Cfg::NPT, PW = Cfg::PW, ROWB = Cfg::ROWB, BIAS_INTS = Cfg::BIAS_INTS;
    constexpr int XS = Cfg::XS, MS = Cfg::MS, IS = Cfg::IS;
    constexpr int CT = C / 32, CM = MID / 32, CTW = CT / NW;
    static_assert((NW == 8 || NW == 4) && CT % NW == 0 && (CM == 2 || CM == 4 || CM == 8) && CM <= NW, "whole channel tiles per wave in P3, whole pixel-tile groups in P1 / P2");
    constexpr int PG = NW / CM;                                 // pixel-tile groups in P1 / P2
    constexpr int NPW = (NPT + PG - 1) / PG;                    // pixel tiles per wave there
    constexpr int NK1 = C / 32, NK2 = 9 * CM, KK = CM, KS = CIN0 / 32;   // K32 steps of body.0 / body.2 / body.4 / the opening block's shortcut
    constexpr bool WSTAT = NPT > 2;                             // P3: this wave's weights stay in registers for all pixel tiles (else streamed, two tiles at a time)
    // EARLY (round 4): the halo rows are published STRAIGHT FROM THE REGISTERS of P1's epilogue (no patch read-back, no extra barrier: the
    // "patch complete" barrier is also the publish barrier), body.2 starts with its CENTRE-ROW taps, which read no halo row, and the
    // neighbours' rows are waited for and fetched only in front of the first tap that needs one: the flag's and the rows' round trips
    // through the fabric (~2 x 1 us) run under a third of the 3x3.  (Round 3 could not afford the consume point inside the unrolled K
    // loop: the kernel was at 256 registers; the weight streams as buffer loads and the peeled opening block freed 25-55.)
    // Tried on top and NOT kept (round 4): cutting the 3x3 by pixel tile as well — a wave's first tile never holds the tile's last row, its
    // second never the first, so two thirds of the MFMAs can run before the rows are needed, with the rows requested after the first third
    // and written to the patch after the second.  Bit-exact, no spills, and slower on every instance (same box, us per 128 images: 245 -> 257,
    // 192 -> 205, 222 -> 248): the top / bottom taps' weight fragments are then loaded twice and feed ONE MFMA each.
#ifndef F8_CH_EARLY
#define F8_CH_EARLY 1
#endif
#ifndef F8_CH_PRIO
#define F8_CH_PRIO 0              // 1: the second-dispatched half of the workgroup (waves 4-7: the arbitration losers on every SIMD) runs the second half of P3 at priority 1
#endif
#ifndef F8_CH_BREG
#define F8_CH_BREG 1              // channel tiles per wave whose body.4 bias is register-resident in P3 (weights-stationary instances)
#endif
    constexpr bool EARLY = F8_CH_EARLY != 0 && T > 1 && !ROT;
    // SPLIT (round 4, late): a wave's pixel tiles are CONSECUTIVE (pg * NPW + j instead of pg + PG * j), so a wave touches the tile's first row or its
    // last row, never both, and walks the taps of body.2 in the order that needs ITS halo row last: centre, bottom, top for the waves of the first
    // rows (and the waves in the middle, which need none), centre, top, bottom for the waves of the last row — the neighbours' rows are then waited for
    // after two thirds of the 3x3 instead of one (the wait is the neighbours' skew: §4.1 of DESIGN.md).  Instances whose tiles are whole (no ragged
    // last tile) and whose first pixel-tile group holds the whole first row and none of the last (the 56x56 and 28x28 instances).
#ifndef F8_CH_SPLIT
#define F8_CH_SPLIT 1
#endif
    // cache-policy bits of the halo rows' stores and loads: 17 = sc0 sc1 (agent scope: write-through / L2 bypass — what a neighbour on another XCD needs).
    // Tuning builds (results INVALID when neighbours sit on different XCDs): 1 = sc0 only, 0 = none: the rows stay in the producer's L2 — what the
    // write-through and the fabric round trip cost (profiles/chain_limiter_r06.md)
#ifndef F8_CH_HALO_AUX
#define F8_CH_HALO_AUX 17
#endif
    constexpr int PG_ = NW / (MID / 32), NPW_ = ((R * W + 31) / 32 + PG_ - 1) / PG_;
    constexpr bool SPLIT = F8_CH_SPLIT != 0 && EARLY && PG_ >= 2 && T * R == H && W <= NPW_ * 32 && (R - 1) * W >= NPW_ * 32;
    static_assert(!(Cfg::STACKABLE && SPLIT), "the seam's tap bases live in the plain EARLY tap order");
    static_assert(NB <= CM && CM % NB == 0 && NK1 % NB == 0, "a batch of K steps stays inside one 3x3 tap / one weight tile");
    static_assert(!DS0 || KS % NB == 0, "stage-opening block: whole batches");
    static_assert(!ROT || (NK1 % 8 == 0 && CM == 8), "rotation: groups of 8 K steps (256 bytes of a row), whole taps");
    static_assert(WSTAT || NPT == 2, "streamed P3: exactly one pixel pair");
    static_assert(W <= 62, "tile");

    if constexpr (FAST == 1) set_fp_round_nearest_even();
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* const x8 = lds;                                       // [NPT*32 px][XS] int8, body.0's input format of the NEXT P1
    char* const patch = x8 + Cfg::X8_BYTES;                     // [(R+2)][(W+2)][MS] mid1, border = biased zero
    char* const mid2 = patch + Cfg::PATCH_BYTES;                // [NPT*32 px][MS]
    char* const xin = Cfg::ALIAS ? patch : mid2 + Cfg::MID2_BYTES;   // DS0: [NPT*32 px][IS], the stage input tile (ALIAS: in the patch's bytes)
    int* const bias_lds = (int*)(mid2 + Cfg::MID2_BYTES + (Cfg::ALIAS ? 0 : Cfg::XIN_BYTES));   // every block's b0 | b2 | b4, then bsc of the opening block
    int* const misc = bias_lds + Cfg::BIAS_BYTES / 4;

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & (NW - 1);
    // Per-lane constants (lane, its pixel row and K half, LDS bases ...) are RE-DERIVED at the top of every phase from an opaque copy
    // of the thread id: kept live across the whole kernel next to the 112-128 stream registers they are what the allocator spills,
    // and a scratch reload (`s_waitcnt vmcnt(0)` behind it) in every tile epilogue cost the 56x56 instance a third of its P3.
#define F8_LANES                                                                                                                        \
    int tq_ = tid; asm volatile("" : "+v"(tq_));                                                                                        \
    const int lane = tq_ & 63, l31 = lane & 31, lh = lane >> 5;                                                                         \
    const unsigned wl16 = (unsigned)(lane * 16);                                                                                        \
    const unsigned xlane = (unsigned)(l31 * XS + lh * 16), mlane = (unsigned)(l31 * MS + lh * 16), ilane = (unsigned)(l31 * IS + lh * 16); \
    (void)wl16; (void)xlane; (void)mlane; (void)ilane
#define F8_LANES_P12                                                                                                                    \
    F8_LANES;                                                                                                                           \
    unsigned p12x[NPW], p12m[NPW], p12i[NPW]; int p12_pix[NPW];                                                                          \
    _Pragma("unroll") for (int j = 0; j < NPW; ++j) {                                                                                    \
        const int pt0_ = SPLIT ? pg * NPW + j : pg + PG * j;                                                                             \
        const int pt = pt0_ < NPT ? pt0_ : NPT - 1;                                                                                      \
        p12_pix[j] = pt * 32 + l31;                                                                                                     \
        p12x[j] = (unsigned)(pt * 32 * XS) + xlane; p12m[j] = (unsigned)(pt * 32 * MS) + mlane; p12i[j] = (unsigned)(pt * 32 * IS) + ilane; \
    }                                                                                                                                   \
    (void)p12x; (void)p12m; (void)p12i; (void)p12_pix

    // ---- place in the logical grid: a ticket
    if (tid == 0) { misc[0] = (int)chain_ticket(a.cs); misc[1] = 0; }
    // ---- biases of every block: once per workgroup, into LDS (a global bias load at the head of a phase costs its whole latency)
    constexpr int NBI = (BIAS_INTS + NT - 1) / NT;               // bias words per thread and block
    auto bias_fetch = [&](int b, int (&v)[NBI]) {               // BROT: block b's b0 | b2 | b4 -> registers (the tail block has no b0 / b2)
        const ChainBlk& B = a.blk[b];
        int tb = tid; asm volatile("" : "+v"(tb));
#pragma unroll
        for (int k = 0; k < NBI; ++k) {
            const int i = tb + k * NT;
            v[k] = 0;
            if (i < BIAS_INTS) v[k] = i < 2 * MID ? ((TAIL && b == 0) ? 0 : (i < MID ? B.b0[i] : B.b2[i - MID])) : B.b4[i - 2 * MID];
        }
    };
    auto bias_store = [&](int b, const int (&v)[NBI]) {         // ... -> slot b & 1
        int tb = tid; asm volatile("" : "+v"(tb));
#pragma unroll
        for (int k = 0; k < NBI; ++k) if (tb + k * NT < BIAS_INTS) bias_lds[(b & 1) * BIAS_INTS + tb + k * NT] = v[k];
    };
    if constexpr (!BROT) {
        for (int b = 0; b < a.nblk; ++b) {
            const ChainBlk& B = a.blk[b];
            for (int i = tid; i < BIAS_INTS; i += NT)
                bias_lds[b * BIAS_INTS + i] = i < 2 * MID ? ((TAIL && b == 0) ? 0 : (i < MID ? B.b0[i] : B.b2[i - MID])) : B.b4[i - 2 * MID];
        }
    }
    if constexpr (DS0) for (int i = tid; i < C; i += NT) bias_lds[BSLOTS * BIAS_INTS + i] = a.blk[0].bsc[i];
    __syncthreads();
    const int L = __builtin_amdgcn_readfirstlane(misc[0]);
    // STACK (Cfg::STACKABLE instances, ChainArgs::stack = 2): the tile column is an image pair, HS = 2H rows, T2 tiles; n below counts pairs
    constexpr bool STACKABLE = Cfg::STACKABLE && !ROT;          // (a K-rotated tuning instance keeps one image per column)
    const bool stk2 = STACKABLE && a.stack == 2;
    const int TC = stk2 ? Cfg::T2 : T, HS = stk2 ? 2 * H : H;
    const int grp = L / TC, ti = L - grp * TC;
    const int p0 = ti * R;
    // pairs of the launch; an odd N leaves ONE image in the last pair: the tiles below its row H - 1 have no rows there and stop one pair early
    // (they still count themselves out at the end), the tile that spans the seam runs as the ragged last tile of an unstacked image
    const int n_end = !stk2 ? a.N : ((a.N & 1) && p0 >= H ? a.N / 2 : (a.N + 1) / 2);
    // (the seam tile of an odd N's last pair is ragged: HS != H, 2 n + 1 == N, p0 == (H / R) R — tested from values that are live anyway)
    auto ragged = [&](int n) { return STACKABLE && HS != H && 2 * n + 1 == a.N && p0 == (H / R) * R; };
    const int rows0 = (HS - p0) < R ? (HS - p0) : R;
    const int npx0 = rows0 * W;
    const bool has_up = ti > 0, has_dn0 = ti < TC - 1;
    const int rot = ROT ? __builtin_amdgcn_readfirstlane(L * 5 + wave * 3) : 0;

    unsigned* const flags = chain_flags(a.cs);
    const unsigned long long t_limit = (unsigned long long)a.cs.timeout_ticks;
#ifdef F8_TRACE
    unsigned long long tt[16] = {}; unsigned long long t_prev = __builtin_readcyclecounter();
#define F8_CT(i) do { const unsigned long long now_ = __builtin_readcyclecounter(); tt[i] += now_ - t_prev; t_prev = now_; } while (0)
#else
#define F8_CT(i)
#endif

    // P1 / P2 roles: wave (mt, pg) computes mid channel tile mt for pixel tiles pg + PG j; a missing tile repeats the last one (same bytes twice)
    const int mt = wave & (CM - 1), pg = wave / CM;
    v16i res[NPT][CTW];                                         // the tile's int32 stream: pixel tile x this wave's channel tiles
    v4i wbuf[NBUF][NB];                                         // A operands in flight: NBUF batches of NB K32 steps (one 1 KB wave load each)
    unsigned seq = 0;

    // ---- weight streams (fragment order: [tile][K32 step][lane][16 B]).  step -> K index: identity, or rotated in coarse groups.
    auto k1_of = [&](int g, int nk) { return ROT ? (((g >> 3) + opaque(rot)) & (nk / 8 - 1)) * 8 + (g & 7) : g; };       // body.0: groups of 8 steps
    auto tap_of = [&](int t, int ord = 0) {                     // body.2: whole taps.  ord (SPLIT): 1 = centre, bottom, top; 0 = centre, top, bottom
        if constexpr (EARLY) return t < 3 ? t + 3 : (ord ? (t < 6 ? t + 3 : t - 6) : (t < 6 ? t - 3 : t));   // centre row first (taps 3, 4, 5), then the rows that read a halo row
        else if constexpr (!ROT) return t;
        else { int q = t + (int)((unsigned)opaque(rot) % 9u); return q >= 9 ? q - 9 : q; }
    };
    // A-operand loads: uniform base (+ a SCALAR step offset, kept scalar by `opaque`: as a constant it gets folded into a per-step
    // per-lane offset register that is hoisted out of the block loop and spilled) + ONE per-lane offset register per stream
    // Round 4: BUFFER loads (resource = the weight pointer, scalar step offset in soffset, the per-lane offset in voffset).  As a flat
    // `base + soff + voff` the optimiser re-associated to (base + voff) + soff: a hoisted 64-bit VGPR pair per stream plus two 64-bit
    // vector adds per load — the pairs were what the opening-block instance spilled.
    auto ldw = [](const int8_t* base, int soff, unsigned voff) {
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7ffffff0, 0x00020000);
        return __builtin_amdgcn_raw_buffer_load_b128(r, voff, opaque(soff), 0);
    };
    auto w1_load = [&](const int8_t* w0, auto nkc, v4i (&dst)[NB], int bi, unsigned wl) {
        constexpr int NK = decltype(nkc)::value;
        const unsigned w1off = (unsigned)(mt * NK * 1024) + wl;
        const int k0 = k1_of(bi * NB, NK);
#pragma unroll
        for (int s = 0; s < NB; ++s) dst[s] = ldw(w0, (k0 + s) * 1024, w1off);
    };
    auto w1_prime = [&](const int8_t* w0, auto nkc, unsigned wl) {
        constexpr int NBAT = decltype(nkc)::value / NB;
        static_for<(NBUF - 1 < NBAT ? NBUF - 1 : NBAT)>([&](auto bc) { constexpr int Bi = decltype(bc)::value; w1_load(w0, nkc, wbuf[Bi], Bi, wl); });
    };
    constexpr int NBAT2 = NK2 / NB, BPTAP = CM / NB;            // body.2: batches, batches per tap
    static_assert(!SPLIT || (NBUF - 1) * NB <= 3 * CM, "the batches requested ahead of body.2 lie in the centre taps, which both tap orders start with");
    auto w2_load = [&](const int8_t* w2, v4i (&dst)[NB], int bi, unsigned wl, int ord = 0) {
        const int k0 = tap_of(bi / BPTAP, ord) * CM + (bi % BPTAP) * NB;
#pragma unroll
        for (int s = 0; s < NB; ++s) dst[s] = ldw(w2, (k0 + s) * 1024, (unsigned)(mt * NK2 * 1024) + wl);
    };
    auto w2_prime = [&](const int8_t* w2, unsigned wl) {
        static_for<NBUF - 1>([&](auto bc) { constexpr int Bi = decltype(bc)::value; w2_load(w2, wbuf[Bi], Bi, wl); });
    };
    // TAIL: fragments of the join in use order: per channel tile I of this wave, per PAIR of pixel tiles, KS shortcut steps then KK body.4 steps
    constexpr int KT2 = KS + KK, NPAIR = NPT / 2, NFRT = CTW * NPAIR * KT2, NBT = NFRT / NB;
    auto wt_load = [&](const int8_t* wsc, const int8_t* w4, v4i (&dst)[NB], auto bic, unsigned wl) {
        constexpr int BI = decltype(bic)::value;
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            constexpr int dummy = 0; (void)dummy;
            const int f = BI * NB + s, I = f / (NPAIR * KT2), k = f % KT2;
            dst[s] = k < KS ? ldw(wsc, (I * KS + k) * 1024, (unsigned)(wave * CTW * KS * 1024) + wl) : ldw(w4, (I * KK + (k - KS)) * 1024, (unsigned)(wave * CTW * KK * 1024) + wl);
        }
    };
    // the MFMAs of a step must not be scheduled above the LDS reads of the NEXT step that are issued just before them
    auto pin = [](auto& xf) {
#pragma unroll
        for (int j = 0; j < (int)(sizeof(xf) / sizeof(xf[0])); ++j) asm volatile("" : "+v"(xf[j]));
    };

    // ---- stage-opening first blocks: the tile's int8 input is REQUESTED one image ahead — after the last block of the previous image, BEFORE that
    //      image's output stores (VMEM retires in order: loads issued behind 57 KB of stores would wait for their drain) — and lands in LDS at
    //      the top of the next round (round 4; the registers are free there: the stream is dead between the last finish and the next join)
    constexpr int CHX = CIN0 / 16, CHM = MID / 16;
    constexpr int NXI = DS0 ? (NPT * 32 * CHX + NT - 1) / NT : 0, NMI = TAIL ? (NPT * 32 * CHM + NT - 1) / NT : 0;
    v4i vin[NXI + NMI > 0 ? NXI + NMI : 1];
    auto in_issue = [&](int n, bool live) {     // !live: zeros (every register is (re)defined here on every path: nothing stays live through the blocks)
        if constexpr (DS0) {
            int tq0 = tid; asm volatile("" : "+v"(tq0));
            const int mt0 = (n * HS + p0) * W;
            const int npx = ragged(n) ? (H - p0) * W : npx0;  // (an odd N's last pair holds one image)
#pragma unroll
            for (int k = 0; k < NXI; ++k) {
                const int idx = tq0 + k * NT, row = idx / CHX, c16 = idx % CHX;
                vin[k] = v4i{0, 0, 0, 0};
                if constexpr (TAIL) {       // the shortcut's operand: pixels (2 (p0 + r), 2 c) of the block input (2H x 2W, CIN0 channels)
                    const int pr = row / W, pc = row - pr * W;
                    if constexpr (STACKABLE) {  // stacked row -> (image, its row): pairs are contiguous, so the global row is n HS + p0 + r
                        const int g = mt0 / W + pr, img = g / H, y = g - img * H;
                        if (live && row < npx) vin[k] = *(const v4i*)(a.x8in + ((size_t)(img * 2 * H + 2 * y) * (2 * W) + 2 * pc) * CIN0 + c16 * 16);
                    } else {
                        if (live && row < npx) vin[k] = *(const v4i*)(a.x8in + ((size_t)(n * 2 * H + 2 * (p0 + pr)) * (2 * W) + 2 * pc) * CIN0 + c16 * 16);
                    }
                } else {
                    if (live && row < npx) vin[k] = *(const v4i*)(a.x8in + (size_t)(mt0 + row) * CIN0 + c16 * 16);
                }
            }
#pragma unroll
            for (int k = 0; k < NMI; ++k) {   // TAIL: body.2's output
                const int idx = tq0 + k * NT, row = idx / CHM, c16 = idx % CHM;
                vin[NXI + k] = v4i{0, 0, 0, 0};
                if (live && row < npx) vin[NXI + k] = *(const v4i*)(a.m2in + (size_t)(mt0 + row) * MID + c16 * 16);
            }
        }
    };
    auto in_commit = [&]() {
        if constexpr (DS0) {
            int tq0 = tid; asm volatile("" : "+v"(tq0));
#pragma unroll
            for (int k = 0; k < NXI; ++k) { const int idx = tq0 + k * NT; if (idx < NPT * 32 * CHX) *(v4i*)(xin + (idx / CHX) * IS + (idx % CHX) * 16) = vin[k]; }
#pragma unroll
            for (int k = 0; k < NMI; ++k) { const int idx = tq0 + k * NT; if (idx < NPT * 32 * CHM) *(v4i*)(mid2 + (idx / CHM) * MS + (idx % CHM) * 16) = vin[NXI + k]; }
        }
    };
#ifndef F8_CH_PREFETCH
#define F8_CH_PREFETCH 1          // 0 (tuning builds): the input tile is requested at the top of its own round
#endif
    if (F8_CH_PREFETCH) in_issue(grp < n_end ? grp : 0, grp < n_end);

    for (int n = grp; n < n_end; n += a.NG) {
        const int m_tile = (n * HS + p0) * W;                   // global pixel index of the tile's first pixel
        const bool rag = ragged(n);              // an odd N's last pair: the seam tile is the image's ragged last tile
        const int rows = rag ? H - p0 : rows0, npx = rag ? (H - p0) * W : npx0;
        const bool has_dn = has_dn0 && !rag;
        if (!F8_CH_PREFETCH) in_issue(n, true);

        // =====================================================================================
        // stage input -> registers (identity first block) / LDS (stage-opening first block)
        // =====================================================================================
        if constexpr (TAIL) {
            static_assert(KT2 % NB == 0 && KS % NB == 0 && NPT % 2 == 0, "TAIL: whole batches per K loop, pixel-tile pairs");
            // xin <- the shortcut's operand, mid2 <- body.2's output: requested one image ahead (in_issue)
            int bv0[NBI], bv1[NBI];
            if constexpr (BROT) { bias_fetch(0, bv0); bias_fetch(a.nblk > 1 ? 1 : 0, bv1); }
            { F8_LANES; static_for<(NBUF - 1 < NBT ? NBUF - 1 : NBT)>([&](auto bc) { constexpr int Bi = decltype(bc)::value; wt_load(a.blk[0].wsc, a.blk[0].w4, wbuf[Bi], bc, wl16); }); }
            if constexpr (BROT) { bias_store(0, bv0); bias_store(1, bv1); }
            in_commit();
        } else if constexpr (!DS0) {
            F8_LANES;
            const ChainBlk& B0 = a.blk[0];
            const __amdgpu_buffer_rsrc_t rxr = __builtin_amdgcn_make_buffer_rsrc((void*)a.xr, 0, (unsigned)(((a.N * H * W + 31) & ~31) * C * 4), 0x00020000);
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt) {
                const int pix = pt * 32 + l31;
                const int mc = m_tile + (pix < npx ? pix : 0);
                // I32T: block (m >> 5, c >> 5) of 4 KB, inside it [g][lh * 32 + m & 31][4 ch] ints (f8_device.h)
                const unsigned vo = (unsigned)((mc >> 5) * (C * 128) + lh * 512 + (mc & 31) * 16);
#pragma unroll
                for (int i = 0; i < CTW; ++i) {
                    const int ct = wave * CTW + i;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const v4i v = __builtin_amdgcn_raw_buffer_load_b128(rxr, vo + g * 1024, ct * 4096, 0);
#pragma unroll
                        for (int e = 0; e < 4; ++e) res[pt][i][4 * g + e] = v[e];
                    }
                }
            }
            w1_prime(B0.w0, std::integral_constant<int, NK1>{}, wl16);
#pragma unroll
            for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
                for (int i = 0; i < CTW; ++i)
                    *(v4i*)(x8 + xlane + pt * 32 * XS + (wave * CTW + i) * 32) = quant_tile16<FAST>(res[pt][i], B0.rq.n, FAST ? 0 : B0.rq.lo, FAST ? 255 : B0.rq.hi, FAST ? 0x80808080u : B0.rq.bias_xor);
        } else {
            int bv0[NBI];
            if constexpr (BROT) bias_fetch(0, bv0);
            { F8_LANES; w1_prime(a.blk[0].w0, std::integral_constant<int, KS>{}, wl16); }
            if constexpr (BROT) bias_store(0, bv0);
            in_commit();                                        // the stage input tile, requested one image ahead (in_issue)
        }
        __syncthreads();
        F8_CT(0);

        // One block of the chain.  The stage-opening block is PEELED off the block loop below: inside the loop the stream registers are
        // loop-carried, i.e. allocated (though dead) throughout the opening block's P1 / P2 on top of its own live set — round 3's
        // opening-block instance spilled 144 bytes per lane that way (179 MB of scratch write-back per launch at the counters).
        // LASTC (round 5): 0 = not the chain's last block, 1 = the last block, 2 = decided at run time (the peeled first block).  As a run-time
        // flag `last` put three branches, two exec-mask updates and three SGPR reloads (v_readlane of spilled scalars) around EVERY (pixel tile,
        // channel tile) unit of P3 and kept the stage-output store code inside every block's instruction stream; P3 is bound by the number of
        // instructions a wave issues (one per ~4.7 cycles at two waves per SIMD: DESIGN 4.1), so the identity blocks are now two straight-line copies.
        auto block = [&](const int b, auto dsc, auto lastc) {
            {
                constexpr int LASTC = decltype(lastc)::value;
                constexpr bool TAILB = decltype(dsc)::value == 2;   // 0: identity block, 1: stage-opening block (same resolution), 2: only the join of one (TAIL)
                if constexpr (!TAILB) ++seq;
                int bnext[NBI];                                 // BROT: the next block's biases travel during P1 / P2 and land in the other slot before P3
                const bool bfetch = BROT && !TAILB && b + 1 < a.nblk;
                if constexpr (BROT && !TAILB) { if (bfetch) bias_fetch(b + 1, bnext); }
                const ChainBlk& B = a.blk[b];
                const int* const bl = bias_lds + (BROT ? (b & 1) : b) * BIAS_INTS;
                constexpr bool DSB = decltype(dsc)::value != 0; // this block is the stage-opening block (first block of a DS0 chain)
                constexpr int NK1B = DSB ? KS : NK1;
                constexpr bool ROT1 = ROT && !DSB;
                // the block's scalars, read once (FAST: formats are unsigned with a right shift, ReLUs present, the stream unshifted)
                const bool last = LASTC == 2 ? (b + 1 == a.nblk) : (LASTC == 1);
                const ChainBlk& BN = a.blk[last ? b : b + 1];
                const int8_t* const pw0 = B.w0; const int8_t* const pw2 = B.w2; const int8_t* const pw4 = B.w4; const int8_t* const pwsc = B.wsc;
                const int8_t* const pw0n = BN.w0;
                const int n1 = B.r1.n, n2 = B.r2.n, acc_shl = B.acc_shl, res_shl = B.res_shl;
                const int lo1 = FAST ? 0 : B.r1.lo, hi1 = FAST ? 255 : B.r1.hi, lo2 = FAST ? 0 : B.r2.lo, hi2 = FAST ? 255 : B.r2.hi;
                // (FAST: the constant lives in a scalar register — as a 32-bit literal every v_xor_b32 is an 8-byte instruction, 3.6 instead of 2.3 cycles: ubench_bank)
                const unsigned kx = FAST ? (unsigned)opaque((int)0x80808080u) : 0u;
                const unsigned xor1 = FAST ? kx : B.r1.bias_xor, xor2 = FAST ? kx : B.r2.bias_xor;
                const int relu_a = FAST ? 1 : B.relu_a, relu_b = FAST ? 1 : B.relu_b, relu1 = FAST ? 1 : B.relu1;
                // format of the int8 copy of the block's output in LDS: the next block's body.0 input, or the first int8 form of the stage output
                const int nq = last ? a.q[0].n : BN.rq.n;
                const int loq = FAST ? 0 : (last ? a.q[0].lo : BN.rq.lo), hiq = FAST ? 255 : (last ? a.q[0].hi : BN.rq.hi);
                const unsigned xorq = FAST ? kx : (last ? a.q[0].bias_xor : BN.rq.bias_xor);

                // this wave's P3 weights (WSTAT): requested when P2's K loop is over, so they travel during its epilogue
                constexpr int K0 = DSB ? KS : 0, KT = KK + K0;  // opening block: the shortcut's K steps come first
                v4i wst[(WSTAT && !TAILB) ? CTW * KT : 1];
                auto wst_load = [&](unsigned wl) {
                    if constexpr (WSTAT && !TAILB) {
#pragma unroll
                        for (int i = 0; i < CTW; ++i) {
                            if constexpr (DSB) {
#pragma unroll
                                for (int k = 0; k < KS; ++k) wst[i * KT + k] = ldw(pwsc, (i * KS + k) * 1024, (unsigned)(wave * CTW * KS * 1024) + wl);
                            }
#pragma unroll
                            for (int k = 0; k < KK; ++k) wst[i * KT + K0 + k] = ldw(pw4, (i * KK + k) * 1024, (unsigned)(wave * CTW * KK * 1024) + wl);
                        }
                    }
                };
                auto w3_load = [&](v4i (&dst)[NB], int qi, unsigned wl) {      // streamed P3: batch qi of this wave's CTW consecutive channel tiles
#pragma unroll
                    for (int s = 0; s < NB; ++s) dst[s] = ldw(pw4, (qi * NB + s) * 1024, (unsigned)(wave * CTW * KK * 1024) + wl);
                };
                if constexpr (!TAILB) {
                // ============================ P1: mid1 = requant(relu(W0 . x8 + b0)) -> patch interior   (its first weight batches are in flight)
                {
                    F8_LANES_P12;
#ifndef F8_CH_BFILL
#define F8_CH_BFILL 1             // 0 (tuning builds): the whole patch is filled, with a barrier between the fill and the epilogue's interior stores
#endif
                    {   // patch BORDER <- biased zero: row 0, the rows below the tile's last row (halo row; rows of a ragged last tile), the two side columns of the
                        // interior rows.  Round 4: only the border — disjoint from what the epilogue below writes, so no barrier stands between the two
                        // (the whole-patch fill of round 3 needed one); the halo rows of tiles with a neighbour are overwritten in consume()
                        const v4i zv = {(int)xor1, (int)xor1, (int)xor1, (int)xor1};
                        if constexpr (F8_CH_BFILL) {
                            constexpr int RB = PW * MS, CPM = MS / 16;
                            for (int o = tq_ * 16; o < RB; o += NT * 16) *(v4i*)(patch + o) = zv;
                            for (int o = (rows + 1) * RB + tq_ * 16; o < Cfg::PR * RB; o += NT * 16) *(v4i*)(patch + o) = zv;
                            if (tq_ < rows * 2 * CPM) {
                                const int r = tq_ / (2 * CPM), q = tq_ - r * 2 * CPM, sidec = q / CPM, c16 = q - sidec * CPM;
                                *(v4i*)(patch + ((r + 1) * PW + (sidec ? PW - 1 : 0)) * MS + c16 * 16) = zv;
                            }
                        } else {
                            for (int o = tq_ * 16; o < Cfg::PATCH_BYTES; o += NT * 16) *(v4i*)(patch + o) = zv;
                        }
                        if constexpr (STACKABLE) { if (tq_ < Cfg::ZPAD_BYTES / 16) *(v4i*)(lds + Cfg::ZPAD_OFF + tq_ * 16) = zv; }   // the seam's taps
                    }
                    v16i acc[NPW];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const v4i bv = *(const v4i*)(bl + mt * 32 + 8 * g + 4 * lh);
#pragma unroll
                        for (int j = 0; j < NPW; ++j)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[j][4 * g + e] = bv[e];
                    }
                    F8_CT(6);
                    constexpr int NBAT1 = NK1B / NB;
                    const char* const xsrc = DSB ? xin : x8;
                    auto rd = [&](v4i (&xf)[NPW], auto gc) {
                        constexpr int G = decltype(gc)::value;
                        if constexpr (ROT1) {
                            const unsigned ko = (unsigned)(k1_of(G & ~7, NK1B) * 32 + (G & 7) * 32);
#pragma unroll
                            for (int j = 0; j < NPW; ++j) xf[j] = *(const v4i*)(xsrc + p12x[j] + ko);
                        } else {
#pragma unroll
                            for (int j = 0; j < NPW; ++j) xf[j] = *(const v4i*)(xsrc + (DSB ? p12i[j] : p12x[j]) + G * 32);
                        }
                    };
                    v4i xfa[NPW], xfb[NPW];
                    rd(xfa, std::integral_constant<int, 0>{});
                    static_for<NK1B>([&](auto gc) {
                        constexpr int G = decltype(gc)::value, Bi = G / NB, S = G % NB;
                        if constexpr (S == 0 && Bi + NBUF - 1 < NBAT1) w1_load(pw0, std::integral_constant<int, NK1B>{}, wbuf[(Bi + NBUF - 1) % NBUF], Bi + NBUF - 1, wl16);
                        v4i (&cur)[NPW] = (G & 1) ? xfb : xfa;
                        v4i (&nxt)[NPW] = (G & 1) ? xfa : xfb;
                        if constexpr (G + 1 < NK1B) rd(nxt, std::integral_constant<int, G + 1>{});
                        pin(cur);
#pragma unroll
                        for (int j = 0; j < NPW; ++j) acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wbuf[Bi % NBUF][S], cur[j], acc[j], 0, 0, 0);
                    });
                    F8_CT(7);
                    w2_prime(pw2, wl16);                                // body.2's first weight batches travel during the epilogue and the halo exchange
                    if constexpr (!F8_CH_BFILL) __syncthreads();     // the (whole-patch) zero fill is complete
                    F8_CT(8);
                    const int floor0 = relu_a ? 0 : INT32_MIN;
                    const __amdgpu_buffer_rsrc_t rxp = __builtin_amdgcn_make_buffer_rsrc((void*)a.cs.xchg, 0, (unsigned)kChainXchgBytes, 0x00020000);
                    const unsigned pub0 = (unsigned)((L * 2 + (int)(seq & 1u)) * 2 * ROWB + mt * 32 + lh * 16);   // this block's parity, side 0 (my top row)
#pragma unroll
                    for (int j = 0; j < NPW; ++j) {
                        const int pix = p12_pix[j];
                        const int pr = pix / W, pc = pix - pr * W;
                        const int ent = (pr + 1) * PW + pc + 1;
                        if constexpr (!FAST) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[j][r] = max(acc[j][r], floor0);
                        }
                        const v4i o = quant_tile16<FAST, true>(acc[j], n1, lo1, hi1, xor1);   // FAST: lo1 == 0 is the ReLU
                        if (pix < npx) *(v4i*)(patch + ent * MS + mt * 32 + lh * 16) = o;
                        if constexpr (EARLY) {                  // my first / last row -> the neighbours, write-through (sc0 sc1), 16 bytes per lane
                            if (pix < npx && pr == 0 && has_up) __builtin_amdgcn_raw_buffer_store_b128(o, rxp, pub0 + (unsigned)(pc * MID), 0, F8_CH_HALO_AUX);
                            if (pix < npx && pr == rows - 1 && has_dn) __builtin_amdgcn_raw_buffer_store_b128(o, rxp, pub0 + (unsigned)(ROWB + pc * MID), 0, F8_CH_HALO_AUX);
                        }
                    }
                    if constexpr (EARLY) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains (the first body.2 weight batches land too)
                }
                F8_CT(1);
                __syncthreads();                                // the patch interior is complete (EARLY: and every halo store has been performed)
                if constexpr (EARLY) { if (tid == 0) chain_flag(flags + L, seq); }
                F8_CT(9);

                // ============================ halo rows: publish mine (EARLY: done above), fetch the neighbours' (EARLY: inside body.2's K loop)
                static_assert(NW == 8 || EARLY || T == 1, "the 4-wave instances publish their halo rows from P1's epilogue");
                if constexpr (T > 1 && !EARLY) {
                    constexpr int RCH = ROWB / 16, CPE = MID / 16;              // 16-byte pieces per row / per patch entry
                    const __amdgpu_buffer_rsrc_t rxc = __builtin_amdgcn_make_buffer_rsrc((void*)a.cs.xchg, 0, (unsigned)kChainXchgBytes, 0x00020000);
                    int th = tid; asm volatile("" : "+v"(th));                   // re-derived per block, not hoisted and spilled
                    const int side = th >> 8, idx = th & 255;                   // threads 0..255: top row / upper neighbour; 256..511: bottom / lower
                    const bool mine = idx < RCH && (side == 0 ? has_up : has_dn);
                    const int col = idx / CPE, c16 = idx % CPE;
                    const unsigned par = seq & 1u;
                    if (mine) {
                        const int ent = (side == 0 ? 1 : rows) * PW + col + 1;
                        const v4i v = *(const v4i*)(patch + ent * MS + c16 * 16);
                        __builtin_amdgcn_raw_buffer_store_b128(v, rxc, (unsigned)(((L * 2 + (int)par) * 2 + side) * ROWB + idx * 16), 0, F8_CH_HALO_AUX);   // sc0 sc1: write-through
                    }
                    F8_CT(10);
                    chain_signal(flags + L, seq);
                    F8_CT(11);
                }
                // (Tried in round 4 and not kept: ONE wave per neighbour doing the whole hand-over — lane 0 polls, its 64 lanes fetch four pieces each — which
                // saves the barrier between poll and fetch: no faster on any instance, 231-234 vs 234-237 us per 128 images on the 56x56 launch.)
                auto consume = [&]() {
                  if constexpr (T > 1) {
                    constexpr int RCH = ROWB / 16, CPE = MID / 16;
                    constexpr int HT = NT / 2, PPT = (RCH + HT - 1) / HT;       // threads per side; 16-byte pieces of a row per thread (1 with 8 waves, 2 with 4)
                    const __amdgpu_buffer_rsrc_t rxc = __builtin_amdgcn_make_buffer_rsrc((void*)a.cs.xchg, 0, (unsigned)kChainXchgBytes, 0x00020000);
                    int th = tid; asm volatile("" : "+v"(th));
                    const int side = th / HT, idx0 = th & (HT - 1);             // first half of the workgroup: top row / upper neighbour; second half: bottom / lower
                    const bool side_ok = side == 0 ? has_up : has_dn;
                    const unsigned par = seq & 1u;
                    // one lane per neighbour polls its flag
                    if ((tid == 0 && has_up) || (tid == HT && has_dn)) {
#ifndef F8_CH_ABL_NOPOLL        // (tuning build, results invalid: without the wait the neighbours' rows are taken as they are)
                        chain_wait_flag<0x40u, 2>(a.cs, flags + (tid == 0 ? L - 1 : L + 1), seq, t_limit);   // (a time-out runs on: f8_chain_common.h)
#endif
                    }
                    F8_CT(12);
                    __syncthreads();
                    const int nb_wg = side == 0 ? L - 1 : L + 1;                // upper neighbour's BOTTOM row / lower neighbour's TOP row
                    v4i hv[PPT];
#pragma unroll
                    for (int k = 0; k < PPT; ++k) {
                        const int idx = idx0 + k * HT;
                        hv[k] = v4i{0, 0, 0, 0};
                        if (idx < RCH && side_ok)
                            hv[k] = __builtin_amdgcn_raw_buffer_load_b128(rxc, (unsigned)(((nb_wg * 2 + (int)par) * 2 + (1 - side)) * ROWB + idx * 16), 0, F8_CH_HALO_AUX);
                    }
#pragma unroll
                    for (int k = 0; k < PPT; ++k) {
                        const int idx = idx0 + k * HT;
                        const int col = idx / CPE, c16 = idx % CPE;
                        const int ent = (side == 0 ? 0 : rows + 1) * PW + col + 1;
                        if (idx < RCH && side_ok) *(v4i*)(patch + ent * MS + c16 * 16) = hv[k];
                    }
                    __syncthreads();
                  }
                };
                if constexpr (!EARLY) consume();
                F8_CT(2);

                // ============================ P2: mid2 = requant(relu(conv3x3(mid1) + b2)) -> mid2
                {
                    F8_LANES_P12;
                    v16i acc[NPW];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const v4i bv = *(const v4i*)(bl + MID + mt * 32 + 8 * g + 4 * lh);
#pragma unroll
                        for (int j = 0; j < NPW; ++j)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[j][4 * g + e] = bv[e];
                    }
                    unsigned bpb[NPW];                          // LDS offset of tap (0, 0) of this lane's output pixel
#pragma unroll
                    for (int j = 0; j < NPW; ++j) {
                        const int pix = p12_pix[j], oc = pix < npx ? pix : npx - 1;   // padding lanes read a valid pixel, result unused
                        const int orow = oc / W, ocol = oc - orow * W;
                        bpb[j] = (unsigned)((orow * PW + ocol) * MS + lh * 16);
                    }
                    v4i xfa[NPW], xfb[NPW];
                    constexpr int GH = SPLIT ? 6 * CM : (EARLY ? 3 * CM : NK2 + 1);     // first K step of a tap that may read a halo row
                    // SPLIT: the waves whose tiles hold pixels of the LAST row take the bottom taps last (ord 0), every other wave the top taps (ord 1; no
                    // ragged tile: rows == R).  ONE copy of the K loop: the order only moves the patch ROW of the second and third tap group, i.e. two
                    // more per-lane base registers per pixel tile (two copies of the loop cost 29 registers here and spilled the 28x28 instances)
                    const int ord = (SPLIT && !((pg + 1) * NPW * 32 > (R - 1) * W)) ? 1 : 0;
                    unsigned bpb2[NPW], bpb3[NPW];
#pragma unroll
                    for (int j = 0; j < NPW; ++j) { bpb2[j] = bpb[j] + (unsigned)(ord ? 2 * PW * MS : 0); bpb3[j] = bpb[j] + (unsigned)(ord ? 0 : 2 * PW * MS); }
                    // STACKABLE: the top / bottom tap rows' own bases — a lane on the seam's second / first image row reads the zero pad there
                    // (chosen once per block here: the K loop gains no instruction)
                    unsigned bpbt[NPW], bpbb[NPW];
#pragma unroll
                    for (int j = 0; j < NPW; ++j) {
                        bpbt[j] = bpb[j]; bpbb[j] = bpb[j];
                        if constexpr (STACKABLE) {
                            const int pix = p12_pix[j], srow = p0 + (pix < npx ? pix : npx - 1) / W;
                            const unsigned zo = (unsigned)(Cfg::ZPAD_OFF - Cfg::X8_BYTES + lh * 16);
                            // (row H exists in pairs only; row H - 1 of a lone image has the border's zero row below it: the pad holds the same bytes)
                            if (srow == H) bpbt[j] = zo;
                            if (srow == H - 1) bpbb[j] = zo - (unsigned)(2 * PW * MS);
                        }
                    }
                    auto rd = [&](v4i (&xf)[NPW], auto gc) {
                        constexpr int G = decltype(gc)::value, TAP0 = G / CM, CI = G % CM;
                        if constexpr (SPLIT) {
                            constexpr int GRP = TAP0 / 3, DX = TAP0 % 3;             // tap group: centre row, then the two halo-side rows in this wave's order
#pragma unroll
                            for (int j = 0; j < NPW; ++j) {
                                if constexpr (GRP == 0) xf[j] = *(const v4i*)(patch + bpb[j] + (PW + DX) * MS + CI * 32);
                                else if constexpr (GRP == 1) xf[j] = *(const v4i*)(patch + bpb2[j] + DX * MS + CI * 32);
                                else xf[j] = *(const v4i*)(patch + bpb3[j] + DX * MS + CI * 32);
                            }
                        } else {
                            constexpr int TAP = EARLY ? (TAP0 < 3 ? TAP0 + 3 : (TAP0 < 6 ? TAP0 - 3 : TAP0)) : TAP0;
                            if constexpr (ROT) {
                                const int tp = tap_of(TAP);
                                const int tr = tp / 3, ts = tp - tr * 3;
                                const unsigned eo = (unsigned)((tr * PW + ts) * MS + CI * 32);
#pragma unroll
                                for (int j = 0; j < NPW; ++j) xf[j] = *(const v4i*)(patch + bpb[j] + eo);
                            } else {
#pragma unroll
                                for (int j = 0; j < NPW; ++j) xf[j] = *(const v4i*)(patch + (TAP < 3 ? bpbt[j] : TAP < 6 ? bpb[j] : bpbb[j]) + ((TAP / 3) * PW + TAP % 3) * MS + CI * 32);
                            }
                        }
                    };
                    rd(xfa, std::integral_constant<int, 0>{});
                    static_for<NK2>([&](auto gc) {
                        constexpr int G = decltype(gc)::value, Bi = G / NB, S = G % NB;
                        if constexpr (S == 0 && Bi + NBUF - 1 < NBAT2) w2_load(pw2, wbuf[(Bi + NBUF - 1) % NBUF], Bi + NBUF - 1, wl16, ord);
                        v4i (&cur)[NPW] = (G & 1) ? xfb : xfa;
                        v4i (&nxt)[NPW] = (G & 1) ? xfa : xfb;
                        if constexpr (G == GH) { F8_CT(3); consume(); F8_CT(2); rd(cur, gc); }
                        if constexpr (G + 1 < NK2 && G + 1 != GH) rd(nxt, std::integral_constant<int, G + 1>{});
                        pin(cur);
#pragma unroll
                        for (int j = 0; j < NPW; ++j) acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wbuf[Bi % NBUF][S], cur[j], acc[j], 0, 0, 0);
                    });
                    if constexpr (WSTAT) wst_load(wl16);
                    else static_for<NBUF - 1>([&](auto bc) { constexpr int Qi = decltype(bc)::value; w3_load(wbuf[Qi], Qi, wl16); });
                    const int floor0 = relu_b ? 0 : INT32_MIN;
#pragma unroll
                    for (int j = 0; j < NPW; ++j) {
                        if constexpr (!FAST) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[j][r] = max(acc[j][r], floor0);
                        }
                        *(v4i*)(mid2 + p12m[j] + mt * 32) = quant_tile16<FAST, true>(acc[j], n2, lo2, hi2, xor2);
                    }
                }
                F8_CT(3);
                if constexpr (BROT) { if (bfetch) bias_store(b + 1, bnext); }      // slot (b + 1) & 1 held block b - 1's: dead since that block's last barrier
                __syncthreads();                                // mid2 is complete; nobody reads the patch any more
                }   // !TAILB

                // ============================ P3: stream' = clamp((W4 . mid2 + b4) << sa + (stream << sr)) [ReLU]; x8' = requant(stream')
                {
                    F8_LANES;
                    const int floor1 = relu1 ? 0 : -2147483647;   // the join's clamp_(min=-(2^31-1)) and the ReLU floor are one max
                    // channel tile I of pixel tile PT is complete in `acc`: join, clamp, new stream, its int8 copy
                    auto finish = [&](auto ptc, auto ic, const v16i& acc) {
                        constexpr int PT = decltype(ptc)::value, I = decltype(ic)::value;
                        const int ct = wave * CTW + I;
                        const int pix = PT * 32 + l31;
                        v16i& rr = res[PT][I];
#ifdef F8_CH_ABL_NOFIN          // tuning build (results invalid): no join, no requantisation — what P3 costs without its vector work
                        { const v4i o = {acc[0] ^ rr[0], acc[5], acc[10], acc[15]}; *(v4i*)(x8 + xlane + PT * 32 * XS + ct * 32) = o; (void)pix; (void)floor1; return; }
#endif
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            // identity: (body.4 << acc_shl) + (stream << res_shl); opening block: (shortcut << acc_shl) + (body.4 << res_shl)
                            const unsigned v = DSB ? (unsigned)rr[r] : (unsigned)acc[r], o = DSB ? (unsigned)acc[r] : (unsigned)rr[r];
                            if constexpr (FAST && !DSB) rr[r] = max((int)((v << acc_shl) + o), 0);
                            else rr[r] = max((int)((v << acc_shl) + (o << res_shl)), floor1);
                        }
                        if (!last || a.q[0].ptr) *(v4i*)(x8 + xlane + PT * 32 * XS + ct * 32) = quant_tile16<FAST>(rr, nq, loq, hiq, xorq);
                        if (last && pix < npx) {
                            // (opaque: these addresses are NOT precomputed per pixel tile outside the block loop — 28 registers that spilled)
                            const int m = opaque(m_tile) + pix;
                            const unsigned tot = (unsigned)(((a.N * H * W + 31) & ~31) * C);
                            if (a.out32) {
                                const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)a.out32, 0, tot * 4u, 0x00020000);
                                const unsigned vo = (unsigned)((m >> 5) * (C * 128) + lh * 512 + (m & 31) * 16);
#pragma unroll
                                for (int g = 0; g < 4; ++g) {
                                    const v4i o = {rr[4 * g], rr[4 * g + 1], rr[4 * g + 2], rr[4 * g + 3]};
                                    __builtin_amdgcn_raw_buffer_store_b128(o, ro, vo + g * 1024, ct * 4096, 0);
                                }
                            }
                            if (a.q[1].ptr) {
                                const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)a.q[1].ptr, 0, tot, 0x00020000);
                                __builtin_amdgcn_raw_buffer_store_b128(quant_tile16<false>(rr, a.q[1].n, a.q[1].lo, a.q[1].hi, a.q[1].bias_xor), rq,
                                                                       (unsigned)(m * C + 16 * lh), ct * 32, 0);
                            }
                        }
                    };
                    auto bias_init = [&](v16i& acc, int ct) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const v4i bv = *(const v4i*)(bl + 2 * MID + ct * 32 + 8 * g + 4 * lh);
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[4 * g + e] = bv[e];
                        }
                    };
                    if constexpr (TAILB) {
                        // the join of the stride-2 opening block: per channel tile I and pair of pixel tiles, KS shortcut steps (B: xin) into the
                        // stream registers (they are born here), KK body.4 steps (B: mid2) into acc; weights streamed (each fragment twice)
                        auto rdt = [&](v4i (&xf)[2], auto gc) {
                            constexpr int G = decltype(gc)::value, H2 = (G / KT2) % NPAIR, K = G % KT2;
                            if constexpr (K < KS) { xf[0] = *(const v4i*)(xin + ilane + (2 * H2) * 32 * IS + K * 32); xf[1] = *(const v4i*)(xin + ilane + (2 * H2 + 1) * 32 * IS + K * 32); }
                            else { xf[0] = *(const v4i*)(mid2 + mlane + (2 * H2) * 32 * MS + (K - KS) * 32); xf[1] = *(const v4i*)(mid2 + mlane + (2 * H2 + 1) * 32 * MS + (K - KS) * 32); }
                        };
                        v4i xfa[2], xfb[2];
                        v16i acc[2];
                        rdt(xfa, std::integral_constant<int, 0>{});
                        static_for<NFRT>([&](auto gc) {
                            constexpr int G = decltype(gc)::value, I = G / (NPAIR * KT2), H2 = (G / KT2) % NPAIR, K = G % KT2, Bi = G / NB, S = G % NB;
                            const int ct = wave * CTW + I;
                            if constexpr (S == 0 && Bi + NBUF - 1 < NBT) wt_load(pwsc, pw4, wbuf[(Bi + NBUF - 1) % NBUF], std::integral_constant<int, Bi + NBUF - 1>{}, wl16);
                            if constexpr (K == 0) {
                                bias_init(acc[0], ct);
#pragma unroll
                                for (int g = 0; g < 4; ++g) {
                                    const v4i bs = *(const v4i*)(bias_lds + BSLOTS * BIAS_INTS + ct * 32 + 8 * g + 4 * lh);
#pragma unroll
                                    for (int e = 0; e < 4; ++e) { res[2 * H2][I][4 * g + e] = bs[e]; res[2 * H2 + 1][I][4 * g + e] = bs[e]; }
                                }
                            }
                            v4i (&cur)[2] = (G & 1) ? xfb : xfa;
                            v4i (&nxt)[2] = (G & 1) ? xfa : xfb;
                            if constexpr (G + 1 < NFRT) rdt(nxt, std::integral_constant<int, G + 1>{});
                            pin(cur);
                            if constexpr (K < KS) {
                                res[2 * H2][I] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wbuf[Bi % NBUF][S], cur[0], res[2 * H2][I], 0, 0, 0);
                                res[2 * H2 + 1][I] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wbuf[Bi % NBUF][S], cur[1], res[2 * H2 + 1][I], 0, 0, 0);
                            } else {
                                if constexpr (K == KS) acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wbuf[Bi % NBUF][S], cur[1], acc[0], 0, 0, 0);   // C = the bias still in acc[0]
                                acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wbuf[Bi % NBUF][S], cur[0], acc[0], 0, 0, 0);
                                if constexpr (K != KS) acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wbuf[Bi % NBUF][S], cur[1], acc[1], 0, 0, 0);
                            }
                            if constexpr (K == KT2 - 1) {
                                if constexpr (G == NFRT - 1) { if (!last) w1_prime(pw0n, std::integral_constant<int, NK1>{}, wl16); }
                                finish(std::integral_constant<int, 2 * H2>{}, std::integral_constant<int, I>{}, acc[0]);
                                finish(std::integral_constant<int, 2 * H2 + 1>{}, std::integral_constant<int, I>{}, acc[1]);
                            }
                        });
                    } else if constexpr (WSTAT) {
                        // one pixel tile at a time; the wave's weights (CTW x KT fragments) stay in registers; B fragments one step ahead
                        constexpr int NST = NPT * CTW * KT;
                        // BREG (round 5): body.4's bias of the wave's first BREG channel tiles stays in 16 registers each for the whole phase and is the C operand
                        // of the unit's first body.4 MFMA (v_mfma D, A, B, C with C != D: no copy) — instead of four ds_read_b128 into the accumulator in
                        // front of EVERY (pixel tile, channel tile) unit, whose latency the unit's MFMAs and all its vector work sat behind
                        // (tools/ubench/ubench_p3.hip: 7.2 k -> 6.5 k cycles per phase at 56x56; profiles/ubench_p3_r05.txt)
                        constexpr int BREG = F8_CH_BREG < CTW ? F8_CH_BREG : CTW;
                        v16i breg[BREG > 0 ? BREG : 1];
                        if constexpr (BREG > 0) {
#pragma unroll
                            for (int i = 0; i < BREG; ++i) bias_init(breg[i], wave * CTW + i);
                        }
                        auto rd = [&](v4i& xf, auto gc) {
                            constexpr int G = decltype(gc)::value, PT = G / (CTW * KT), KI = G % KT;
                            if constexpr (KI >= K0) xf = *(const v4i*)(mid2 + mlane + PT * 32 * MS + (KI - K0) * 32);
                            else xf = *(const v4i*)(xin + ilane + PT * 32 * IS + KI * 32);
                        };
                        v4i xfa, xfb;
                        v16i acc;
                        rd(xfa, std::integral_constant<int, 0>{});
                        static_for<NST>([&](auto gc) {
                            constexpr int G = decltype(gc)::value, PT = G / (CTW * KT), I = (G / KT) % CTW, KI = G % KT;
                            const int ct = wave * CTW + I;
                            if constexpr (F8_CH_PRIO != 0 && G == (NPT / 2) * CTW * KT) { if (wave >= 4) __builtin_amdgcn_s_setprio(1); }
                            if constexpr (KI == 0) {
                                if constexpr (I >= BREG) bias_init(acc, ct);
                                if constexpr (DSB) {    // the shortcut product accumulates straight into the stream registers (they are born here)
#pragma unroll
                                    for (int g = 0; g < 4; ++g) {
                                        const v4i bs = *(const v4i*)(bias_lds + BSLOTS * BIAS_INTS + ct * 32 + 8 * g + 4 * lh);
#pragma unroll
                                        for (int e = 0; e < 4; ++e) res[PT][I][4 * g + e] = bs[e];
                                    }
                                }
                            }
                            v4i& cur = (G & 1) ? xfb : xfa;
                            v4i& nxt = (G & 1) ? xfa : xfb;
                            if constexpr (G + 1 < NST) rd(nxt, std::integral_constant<int, G + 1>{});
                            asm volatile("" : "+v"(cur));
                            if constexpr (KI == K0 && I < BREG) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wst[I * KT + KI], cur, breg[I], 0, 0, 0);
                            else if constexpr (KI >= K0) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wst[I * KT + KI], cur, acc, 0, 0, 0);
                            else res[PT][I] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wst[I * KT + KI], cur, res[PT][I], 0, 0, 0);
                            if constexpr (KI == KT - 1) {
                                if constexpr (PT == NPT - 1 && I == CTW - 1) {   // the block's last weight use: the next block's body.0 starts to travel
                                    if (!last) w1_prime(pw0n, std::integral_constant<int, NK1>{}, wl16);
                                }
                                finish(std::integral_constant<int, PT>{}, std::integral_constant<int, I>{}, acc);
                            }
                        });
                    } else {
                        // both pixel tiles at once, this wave's CTW channel tiles in turn, weights streamed (read once)
                        static_assert(WSTAT || !DSB, "streamed P3 has no opening-block form");
                        constexpr int NQ = CTW * KK / NB, NST = CTW * KK;
                        auto rd = [&](v4i (&xf)[2], auto gc) {
                            constexpr int KI = decltype(gc)::value % KK;
                            xf[0] = *(const v4i*)(mid2 + mlane + KI * 32);
                            xf[1] = *(const v4i*)(mid2 + mlane + 32 * MS + KI * 32);
                        };
                        v4i xfa[2], xfb[2];
                        v16i acc[2];
                        rd(xfa, std::integral_constant<int, 0>{});
                        static_for<NST>([&](auto gc) {
                            constexpr int G = decltype(gc)::value, I = G / KK, KI = G % KK, Qi = G / NB, S = G % NB;
                            const int ct = wave * CTW + I;
                            if constexpr (F8_CH_PRIO != 0 && G == (CTW / 2) * KK) { if (wave >= 4) __builtin_amdgcn_s_setprio(1); }
                            if constexpr (S == 0 && Qi + NBUF - 1 < NQ) w3_load(wbuf[(Qi + NBUF - 1) % NBUF], Qi + NBUF - 1, wl16);
                            if constexpr (KI == 0) bias_init(acc[0], ct);
                            v4i (&cur)[2] = (G & 1) ? xfb : xfa;
                            v4i (&nxt)[2] = (G & 1) ? xfa : xfb;
                            if constexpr (G + 1 < NST) rd(nxt, std::integral_constant<int, G + 1>{});
                            pin(cur);
                            // a unit's first step: the SECOND tile's MFMA goes first and takes its C operand from acc[0], which still holds the bias — instead of a
                            // 16-register copy acc[1] = acc[0] per unit (round 5: vector instructions are what P3 is short of)
                            if constexpr (KI == 0) acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wbuf[Qi % NBUF][S], cur[1], acc[0], 0, 0, 0);
                            acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wbuf[Qi % NBUF][S], cur[0], acc[0], 0, 0, 0);
                            if constexpr (KI != 0) acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wbuf[Qi % NBUF][S], cur[1], acc[1], 0, 0, 0);
                            if constexpr (KI == KK - 1) {
                                if constexpr (I == CTW - 1) { if (!last) w1_prime(pw0n, std::integral_constant<int, NK1>{}, wl16); }
                                finish(std::integral_constant<int, 0>{}, std::integral_constant<int, I>{}, acc[0]);
                                finish(std::integral_constant<int, 1>{}, std::integral_constant<int, I>{}, acc[1]);
                            }
                        });
                    }
                }
                if constexpr (F8_CH_PRIO != 0) __builtin_amdgcn_s_setprio(0);
                F8_CT(4);
                __syncthreads();                                // x8 is complete (the next block's P1 reads it); mid2 may be rewritten
            }
        };
#ifndef F8_CH_PEEL_LAST
#define F8_CH_PEEL_LAST 1         // measured (round 5, same box, interleaved): alone — before BREG — 3 % SLOWER on the 56x56 launch (the launch grows from 41 to 52 KB of
#endif                            // code and P3 is bound by vector THROUGHPUT, not by what a wave issues beside it: DESIGN 4.1); together with BREG +1.0 % img/s in four of four pairs
        if constexpr (TAIL) block(0, std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{});
        else if constexpr (DS0) block(0, std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
        if constexpr (F8_CH_PEEL_LAST) {
            const int b0 = DS0 ? 1 : 0;
            for (int b = b0; b + 1 < a.nblk; ++b) block(b, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
            if (a.nblk > b0) block(a.nblk - 1, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
        } else {
            for (int b = DS0 ? 1 : 0; b < a.nblk; ++b) block(b, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
        }

        if (F8_CH_PREFETCH) in_issue(n + a.NG < n_end ? n + a.NG : n, n + a.NG < n_end);   // the next image's input tile: ahead of the output stores in the memory queue
        // ---- the int8 copy of the stage output: LDS rows -> whole NHWC rows in HBM
        if (a.q[0].ptr) {
            constexpr int CH = C / 16;
            int tq1 = tid; asm volatile("" : "+v"(tq1));
            for (int idx = tq1; idx < npx * CH; idx += NT) {
                const int row = idx / CH, c16 = idx % CH;
                const v4i v = *(const v4i*)(x8 + row * XS + c16 * 16);
                *(v4i*)(a.q[0].ptr + (size_t)(m_tile + row) * C + c16 * 16) = v;
            }
        }
        __syncthreads();                                        // before the next image's tile overwrites x8 / xin
        F8_CT(5);
    }
    chain_rearm<NT>(a.cs, flags, misc + 2);
#ifdef F8_TRACE
    if (a.trace && (tid & 63) == 0) {
        unsigned long long* tp = (unsigned long long*)a.trace + ((size_t)blockIdx.x * 8 + wave) * 16;
        for (int i = 0; i < 16; ++i) tp[i] = tt[i];
    }
#endif
}

// instances: ResNet-50 stage 0 (opening block + identity blocks, 56x56), stage 1 (28x28), stage 2 (14x14) identity chains
bool chain_supported(int C, int MID, int H, int W, int cin0) {
    if (cchain_supported(C, MID, H, W, cin0, false)) return true;     // 7x7: the cluster kernel (f8_cchain.hip)
    if (C == 256 && MID == 64 && H == 56 && W == 56 && (cin0 == 64 || cin0 == 256)) return true;
    if (C == 512 && MID == 128 && H == 28 && W == 28 && cin0 == 512) return true;
    if (C == 1024 && MID == 256 && H == 14 && W == 14 && cin0 == 1024) return true;
    return false;
}
// ... starting with the JOIN of a stride-2 opening block (TAIL): H, W = the stage's resolution, cin0 = the block input's channels
bool chain_tail_supported(int C, int MID, int H, int W, int cin0) {
    if (cchain_supported(C, MID, H, W, cin0, true)) return true;
    return (C == 512 && MID == 128 && H == 28 && W == 28 && cin0 == 256) || (C == 1024 && MID == 256 && H == 14 && W == 14 && cin0 == 512);
}
int chain_max_blocks(int C, int MID, int H, int W, int cin0, bool tail) { (void)C; (void)MID; (void)H; (void)W; (void)cin0; (void)tail; return kChainMaxBlocks; }
// Tried in round 4 and NOT kept in the default build: a 2-row instance of the 56x56 opening-block chain — half the tile, 64 stream registers, 128 VGPRs,
// 78 KB of LDS, TWO workgroups per CU (four waves per SIMD) so that one workgroup's exchange / barrier waits hide behind the other's work.  Bit-exact
// (tests/test_gpu_chain.py on a build with -DF8_CH_R2_S0=1) and SLOWER: 264-271 vs 231-234 us per 128 images, same box — twice the halo rows,
// 12.5 % padding in the 32-pixel tiles, a weight fragment feeds one MFMA instead of two in P1 / P2, 40 bytes per lane of scratch.
#ifndef F8_CH_R2_S0
#define F8_CH_R2_S0 0             // 1 (tuning builds): compile that instance and use it
#endif
// Round 6 (VERDICT r5 #1a), measured and NOT kept in the default build: the 28x28 TAIL instance as TWO 4-wave workgroups per CU over 2-row tiles
// (chain_kernel's NW = 4; 69 KB of LDS each, 227 - 232 registers, the 8-wave instance's per-wave shapes).  Bit-exact through the whole-network tests
// (ResNet-50 / -101, the chain tests of the TAIL form), and 8 % SLOWER: 207 - 214 vs 193 - 196 us per 128 images, three interleaved pairs on one box
// (profiles/ab_chain_nw4_r06.txt), ResNet-50 - 4 %.  The microbenchmark's + 10.5 % for two groups pulling work (ubench_pingpong mode 3) does not
// survive what halving the tile costs: every workgroup streams the block's 272 KB of weights for half the pixels (twice the L2 -> CU traffic), P3 loses
// its register-resident weights (two pixel tiles: the streamed form), twice the halo rows, and the per-block fixed work (bias fetch, border fill,
// five barriers) is spread over half the MFMAs.  Only the TAIL-first form is wired up; -DF8_CH_NW4_S1=1 builds it.
#ifndef F8_CH_NW4_S1
#define F8_CH_NW4_S1 0
#endif
static int chain_nw(int C, int MID, int H, int W, int cin0, bool tail) { return (F8_CH_NW4_S1 && tail && C == 512 && MID == 128 && H == 28 && W == 28 && cin0 == 256) ? 4 : 8; }
void chain_shape(int C, int MID, int H, int W, int cin0, bool tail, int* R, int* wg_per_cu) {
    *R = 4; *wg_per_cu = 1;
    if (F8_CH_R2_S0 && !tail && C == 256 && MID == 64 && H == 56 && W == 56 && cin0 == 64) { *R = 2; *wg_per_cu = 2; }
    if (chain_nw(C, MID, H, W, cin0, tail) == 4) { *R = 2; *wg_per_cu = 2; }
}

template <int C, int MID, int W, int H, int R, int CIN0, int NB, int NBUF, int FAST, bool ROT, bool TAIL = false, int NW = 8>
static hipError_t launch_chain_t(const ChainArgs& a, hipStream_t s) {
    using Cfg = ChainCfg<C, MID, W, H, R, CIN0, TAIL || R < 4, TAIL && NW == 4>;
    static unsigned long long attr_done = 0; int attr_dev = -1;
    if (!dyn_lds_opted_in(&attr_done, &attr_dev)) {
        hipError_t e = hipFuncSetAttribute((const void*)chain_kernel<C, MID, W, H, R, CIN0, NB, NBUF, FAST, ROT, TAIL, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES);
        if (e != hipSuccess) return e;
        if (attr_dev >= 0) attr_done |= 1ull << attr_dev;
    }
    const bool stk2 = a.stack == 2;
    if (stk2 && (!Cfg::STACKABLE || ROT)) return hipErrorInvalidValue;
    const int grid = a.NG * (stk2 ? Cfg::T2 : Cfg::T);
    if (grid < 1 || grid > (R < 4 ? 512 : 256)) return hipErrorInvalidValue;
#ifdef F8_TRACE
    static unsigned long long* tbuf = nullptr; static int count = 0;
    static const int want = [] { const char* e = getenv("F8_TRACE_CHAIN"); return e ? atoi(e) : -1; }();
    ChainArgs b = a;
    const bool tracing = (count++ == want);
    if (tracing) { if (!tbuf) (void)hipMalloc((void**)&tbuf, (size_t)1 << 19); (void)hipMemsetAsync(tbuf, 0, (size_t)grid * 1024, s); b.trace = tbuf; }
    hipLaunchKernelGGL((chain_kernel<C, MID, W, H, R, CIN0, NB, NBUF, FAST, ROT, TAIL, NW>), dim3(grid), dim3(NW * 64), Cfg::LDS_BYTES, s, b);
    if (tracing) {
        (void)hipStreamSynchronize(s);
        static unsigned long long hb[256 * 8 * 16];
        (void)hipMemcpy(hb, tbuf, (size_t)grid * 1024, hipMemcpyDeviceToHost);
        double ph[16] = {}, pw[8][16] = {}; int n = 0;
        for (int i = 0; i < grid; ++i) {
            ++n;
            for (int w = 0; w < 8; ++w) { unsigned long long* p = hb + ((size_t)i * 8 + w) * 16; for (int k = 0; k < 16; ++k) { pw[w][k] += (double)p[k]; if (w == 0) ph[k] += (double)p[k]; } }
        }

        fprintf(stderr, "[trace chain<%d,%d,%d>] grid %d, %d blocks, N %d: avg cycles per WG (whole launch): load %.0f | P1 %.0f | halo %.0f | P2 %.0f | P3 %.0f | out %.0f\n",
                C, MID, W, grid, a.nblk, a.N, ph[0] / n, (ph[1] + ph[6] + ph[7] + ph[8]) / n, (ph[2] + ph[9] + ph[10] + ph[11] + ph[12]) / n, ph[3] / n, ph[4] / n, ph[5] / n);
        fprintf(stderr, "    P1: P3-end barrier + zero fill + bias %.0f | K loop %.0f | barrier %.0f | epilogue %.0f    halo: barrier %.0f | publish %.0f | drain + barrier + flag %.0f | poll %.0f | fetch + barrier %.0f\n",
                ph[6] / n, ph[7] / n, ph[8] / n, ph[1] / n, ph[9] / n, ph[10] / n, ph[11] / n, ph[12] / n, ph[2] / n);
        for (int w = 0; w < 8; ++w)
            fprintf(stderr, "    wave %d: P1 wait+zero %.0f K %.0f bar %.0f epi %.0f | halo %.0f | P2 %.0f | P3 %.0f\n", w, pw[w][6] / n, pw[w][7] / n, pw[w][8] / n, pw[w][1] / n,
                    (pw[w][2] + pw[w][9] + pw[w][10] + pw[w][11] + pw[w][12]) / n, pw[w][3] / n, pw[w][4] / n);
    }
    return hipGetLastError();
#else
    hipLaunchKernelGGL((chain_kernel<C, MID, W, H, R, CIN0, NB, NBUF, FAST, ROT, TAIL, NW>), dim3(grid), dim3(NW * 64), Cfg::LDS_BYTES, s, a);
    return hipGetLastError();
#endif
}

// K steps per register batch, batches per stream (NB, NBUF) of the 56x56 / 28x28 / 14x14 instances (tuning builds override; measured:
// deeper batches than these spill — a scratch reload in front of a K loop waits for every weight load in flight — and are slower)
#ifndef F8_CH_S0
#define F8_CH_S0 2, 2
#endif
#ifndef F8_CH_S1
#define F8_CH_S1 2, 3
#endif
#ifndef F8_CH_S2
#define F8_CH_S2 2, 4
#endif
// FAST instance (see chain_kernel): 0 = generic, 1 = constant formats + float-converter requantisation, 2 = constant formats + integer requantisation
// (option requant_float = 0, accumulators the planner cannot bound, or a shift beyond the converter form's 16).  Decided once per plan (f8_net.cpp binds
// it at finalize), so it reads plan facts, not pointers: bit k of `shortcut_blocks` = block k joins a shortcut conv (wsc), q8 = q[0] is an output form
int chain_fast(const ChainArgs& a, unsigned shortcut_blocks, bool q8) {
    bool f16 = true;
    for (int k = 0; k < a.nblk; ++k) {
        const ChainBlk& B = a.blk[k];
        if (!(B.relu_a && B.relu_b && B.relu1 && B.r1.u8_shr() && B.r2.u8_shr() && B.rq.u8_shr())) return 0;
        if (!(shortcut_blocks >> k & 1u) && B.res_shl != 0) return 0;
        f16 = f16 && B.r1.u8_float() && B.r2.u8_float() && B.rq.u8_float();
    }
    if (q8) {
        if (!a.q[0].u8_shr()) return 0;
        f16 = f16 && a.q[0].u8_float();
    }
    return (a.rq_int || !a.acc_ok || !a.stream_ok || !f16) ? 2 : 1;
}

// The device symbol launch_chain starts for this geometry, as rocprofv3 prints it — built HERE, from the (NB, NBUF) macros and chain_shape the launcher
// below instantiates with, so that the planner's Step::kernel (bench.py joins its live timings with the counter files on that string) cannot drift
// from the instance that runs (round 4 kept a second copy of these constants in f8_net.cpp).  fast: 0 / 1 / 2 as chain_fast returns it.
#define F8_STR2(...) #__VA_ARGS__
#define F8_STR(...) F8_STR2(__VA_ARGS__)
// ROT of the instance launch_chain starts for a geometry (a -DF8_CH_ROT tuning build rotates the K order of the identity-first 14x14 instance only)
static bool chain_rot(int H, bool tail) {
#ifdef F8_CH_ROT
    return H == 14 && !tail;
#else
    (void)H; (void)tail; return false;
#endif
}
// ChainArgs::stack = 2 is a launch argument of the instance, not an instance of its own: the symbol is the same with and without it
bool chain_stackable(int C, int MID, int H, int W, int cin0, bool tail) {
    if (cchain_supported(C, MID, H, W, cin0, tail) || chain_rot(H, tail)) return false;
    int R = 4, wg = 1;
    chain_shape(C, MID, H, W, cin0, tail, &R, &wg);
    return H % R != 0 && (2 * H) % R == 0;
}
int chain_kernel_name(char* buf, size_t cap, int C, int MID, int H, int W, int cin0, bool tail, int fast) {
    if (cchain_supported(C, MID, H, W, cin0, tail)) return cchain_kernel_name(buf, cap, fast);
    int R = 4, wg = 1;
    chain_shape(C, MID, H, W, cin0, tail, &R, &wg);
    const char* nb = MID == 64 ? F8_STR(F8_CH_S0) : (MID == 128 ? F8_STR(F8_CH_S1) : F8_STR(F8_CH_S2));
    return snprintf(buf, cap, "f8::chain_kernel<%d, %d, %d, %d, %d, %d, %s, %d, %s, %s, %d>", C, MID, W, H, R, cin0, nb, fast, chain_rot(H, tail) ? "true" : "false", tail ? "true" : "false",
                    chain_nw(C, MID, H, W, cin0, tail));
}

// fast: the instance chain_fast chose when the plan was bound; chain_kernel_name(..., fast) names the symbol started here
hipError_t launch_chain(const ChainArgs& a, int fast, int C, int MID, int H, int W, int cin0, hipStream_t s) {
    if (a.nblk < 1 || a.nblk > kChainMaxBlocks) return hipErrorInvalidValue;
    if (cchain_supported(C, MID, H, W, cin0, a.tail != 0)) return launch_cchain(a, fast, s);
#define F8_CHAIN_INST(...) (fast == 1 ? launch_chain_t<__VA_ARGS__, 1, F8_CHAIN_ROT>(a, s) : fast == 2 ? launch_chain_t<__VA_ARGS__, 2, F8_CHAIN_ROT>(a, s) : launch_chain_t<__VA_ARGS__, 0, F8_CHAIN_ROT>(a, s))
#define F8_CHAIN_ROT false
#if F8_CH_R2_S0
    if (C == 256 && MID == 64 && H == 56 && W == 56 && cin0 == 64 && a.R == 2) return F8_CHAIN_INST(256, 64, 56, 56, 2, 64, F8_CH_S0);
#endif
    if (C == 256 && MID == 64 && H == 56 && W == 56 && cin0 == 64) return F8_CHAIN_INST(256, 64, 56, 56, 4, 64, F8_CH_S0);
    if (C == 256 && MID == 64 && H == 56 && W == 56 && cin0 == 256) return F8_CHAIN_INST(256, 64, 56, 56, 4, 256, F8_CH_S0);
    if (C == 512 && MID == 128 && H == 28 && W == 28 && cin0 == 512) return F8_CHAIN_INST(512, 128, 28, 28, 4, 512, F8_CH_S1);
#if F8_CH_NW4_S1
    if (C == 512 && MID == 128 && H == 28 && W == 28 && cin0 == 256 && a.tail && a.R == 2) {
        if (!a.m2in || !a.x8in) return hipErrorInvalidValue;
        return fast == 1 ? launch_chain_t<512, 128, 28, 28, 2, 256, F8_CH_S1, 1, false, true, 4>(a, s) : fast == 2 ? launch_chain_t<512, 128, 28, 28, 2, 256, F8_CH_S1, 2, false, true, 4>(a, s)
                                                                                                                  : launch_chain_t<512, 128, 28, 28, 2, 256, F8_CH_S1, 0, false, true, 4>(a, s);
    }
#else
    if (C == 512 && MID == 128 && H == 28 && W == 28 && cin0 == 256 && a.tail) {
        if (!a.m2in || !a.x8in) return hipErrorInvalidValue;
        return fast == 1 ? launch_chain_t<512, 128, 28, 28, 4, 256, F8_CH_S1, 1, false, true>(a, s) : fast == 2 ? launch_chain_t<512, 128, 28, 28, 4, 256, F8_CH_S1, 2, false, true>(a, s)
                                                                                                             : launch_chain_t<512, 128, 28, 28, 4, 256, F8_CH_S1, 0, false, true>(a, s);
    }
#endif
#undef F8_CHAIN_ROT
#ifdef F8_CH_ROT
#define F8_CHAIN_ROT true
#else
#define F8_CHAIN_ROT false      // measured on the 14x14 instance: 466 k cycles per workgroup without the K rotation, 512 k with it
#endif
    if (C == 1024 && MID == 256 && H == 14 && W == 14 && cin0 == 1024) return F8_CHAIN_INST(1024, 256, 14, 14, 4, 1024, F8_CH_S2);
    if (C == 1024 && MID == 256 && H == 14 && W == 14 && cin0 == 512 && a.tail) {
        if (!a.m2in || !a.x8in) return hipErrorInvalidValue;
        return fast == 1 ? launch_chain_t<1024, 256, 14, 14, 4, 512, F8_CH_S2, 1, false, true>(a, s) : fast == 2 ? launch_chain_t<1024, 256, 14, 14, 4, 512, F8_CH_S2, 2, false, true>(a, s)
                                                                                                             : launch_chain_t<1024, 256, 14, 14, 4, 512, F8_CH_S2, 0, false, true>(a, s);
    }
#undef F8_CHAIN_ROT
#undef F8_CHAIN_INST
    return hipErrorInvalidValue;
}

}  // namespace f8
