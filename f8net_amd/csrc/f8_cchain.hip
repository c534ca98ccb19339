// f8_cchain.hip — the bottleneck identity blocks of a 7x7 stage (ResNet-50 stage 3: C = 2048, MID = 512) in ONE launch over CLUSTERS of
// eight workgroups; the int32 residual stream stays in registers from block to block (gfx950).
//
// IntBlock.forward of /root/reference/models/fix_resnet.py:26-77 applied to consecutive blocks as IntModel.forward does (fix_resnet.py:361-366),
// every int_op_only_fix_quant (fix_quant_ops.py:90-114) in place.  Same arguments, same planner entry and the same tests as f8_chain.hip
// (ChainArgs, launch_chain); what differs is how the work is cut.
//
// Why a different cut.  A 7x7 map has 49 pixels and a block 4.4 MB of weights: a tile of rows (f8_chain.hip) would stream megabytes of weights
// per 49 pixels, and the launches this replaces (fused_p12 + the residual-carrying 1x1: 65 us per block and 128 images) do exactly that — every
// workgroup PAIR reads W0 twice and W2 once for ONE image at the L1's 32-64 B/clk, then the join launch moves the int32 stream (51 MB in, 51 MB
// out) through HBM.  Here a cluster of G = 8 workgroups (8 CUs) owns IMG = 4 images (196 pixels = 7 pixel tiles of 32) and cuts every
// convolution by OUTPUT CHANNEL:
//   * stream: workgroup c keeps channels [256 c, 256 c + 256) of all 196 pixels in registers — wave w one 32-channel tile x 7 pixel tiles
//     = 112 registers per lane, as in f8_chain.hip;
//   * P1 (1x1, K = 2048): workgroup c computes mid channels [64 c, 64 c + 64) for all pixels — it streams 128 KB of W0, not 1 MB;
//   * P2 (3x3, K = 4608): mid2 channels [64 c, 64 c + 64) — 288 KB of W2, not 1.18 MB;
//   * P3 (1x1, K = 512) + join: its 256 stream channels — 128 KB of W4, register-resident per wave.
// A cluster reads each block's weights ONCE for four images (the pair design: twice per image), and the stream never touches memory.
// The price: every phase needs ALL channels of its input, so the cluster exchanges its int8 activations three times per block through
// memory — x8 (448 KB), mid1 and mid2 (112 KB each), written by their producers in MFMA-B-FRAGMENT order ([pixel tile][K32 step][lane][16 B]:
// what a lane holds after the epilogue's two permlane swaps IS its 16 bytes of the consumer's B fragment), so every exchange store and load is a
// contiguous 1 KB per wave instruction and the consumers' LDS images are straight LDS-DMA copies.  Protocol: f8_chain_common.h's, one flag
// per workgroup and exchange number, consumers poll the seven others' flags — placement-independent: a workgroup's place is a ticket, the
// eight members of a cluster are consecutive tickets, so the set of started workgroups is a prefix of the logical grid and only the
// cluster whose last member has not started yet waits.
//
// Phases of a block on one workgroup (512 threads = 8 waves, 2 per SIMD, 256 registers each):
//   P1: operands through an LDS ring of D1 = 3 chunks (a chunk = 4 K32 steps: 7 x8 fragments + 2 weight fragments each, LDS-DMA, no registers
//       in flight — the stream holds 112 of them); wave (pp, kh) multiplies pixel tiles 2 pp, 2 pp + 1 by both channel tiles over K half kh
//       (2 x 2 register block), the halves are added through LDS, epilogue -> mid1 -> exchange;
//   P2: mid1 of the whole cluster in LDS (112 KB, fragment order; a tap of a lane's pixel is another lane's slot of another fragment: one per-lane
//       base per (pixel tile, tap), out-of-image taps point at 8 KB of biased zeros), W2 through a ring of D2 = 4 chunks of 8 fragments; same
//       wave roles, K cut by half a tap's channels; epilogue -> mid2 -> exchange;
//   P3: mid2 of the whole cluster in LDS, the wave's 16 W4 fragments and its bias in registers; per pixel tile 16 MFMAs, then the join with the
//       stream registers, ReLU, requantisation -> x8' -> exchange (or, after the last block, the stage's output forms).
#include "f8_chain_common.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace f8 {

struct CCfg {
    static constexpr int C = 2048, MID = 512, PXI = 49, IMG = 4, NPX = PXI * IMG, NPT = 7, G = 8;
    static constexpr int CT = C / 32, CM = MID / 32, CTC = CT / G, CMC = CM / G;      // channel tiles: stream 64, mid 16; per workgroup 8 / 2
    static constexpr int NK1 = C / 32, KK = MID / 32;                                   // K32 steps of body.0 / body.4 (body.2: 9 taps x KK)
    // exchange buffers of one cluster (fragment order)
    static constexpr int X8_BYTES = NPT * NK1 * 1024, M_BYTES = NPT * KK * 1024;
    static constexpr int OFF_M1 = X8_BYTES, OFF_M2 = X8_BYTES + M_BYTES, XCL_BYTES = X8_BYTES + 2 * M_BYTES;
    // LDS
    static constexpr int PATCH_BYTES = M_BYTES;                                         // mid1 (P2) / mid2 (P3) of the whole cluster
    static constexpr int ZERO_BYTES = 8192;                                             // biased zeros: what out-of-image taps read (8 K32 steps deep)
    static constexpr int D1 = 3, CH1_FR = 40, CH1_BYTES = CH1_FR * 1024;                 // P1 ring: 32 x8 fragments (tile 7 = dummy) + 8 weight fragments per chunk
    static constexpr int D2 = 4, CH2_BYTES = 8 * 1024;                                  // P2 ring: 8 weight fragments per chunk
    static constexpr int OFF_ZERO = PATCH_BYTES, OFF_RING2 = PATCH_BYTES + ZERO_BYTES;
    static constexpr int OFF_BIAS = OFF_RING2 + D2 * CH2_BYTES, BIAS_INTS = 32 * (2 * CMC + CTC);
    static constexpr int OFF_MISC = OFF_BIAS + BIAS_INTS * 4, LDS_BYTES = OFF_MISC + 256;
    static_assert(D1 * CH1_BYTES <= OFF_RING2, "the P1 ring lives in the patch's bytes (dead during P1)");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};
constexpr size_t kCChainXchgBytes = (size_t)32 * CCfg::XCL_BYTES;                        // 32 clusters = 256 workgroups

// (tuning builds that study the float-converter instance: which requantisation site runs which arithmetic — 0: the instance's own)
#ifndef F8_CC_Q_TAIL
#define F8_CC_Q_TAIL 0
#endif
#ifndef F8_CC_Q_P1
#define F8_CC_Q_P1 0
#endif
#ifndef F8_CC_Q_P2
#define F8_CC_Q_P2 0
#endif
#ifndef F8_CC_Q_P3
#define F8_CC_Q_P3 0
#endif
#define F8_CC_QI(fast, ov) ((fast) == 1 && (ov) != 0 ? (ov) : (fast))

// FAST as in chain_kernel: 0 = generic formats, 1 / 2 = ReLU everywhere, unsigned 8-bit formats with right shifts, the stream unshifted;
// requantisation through the float converter (1: bounded values, shifts <= 16) or in integer operations (2: the default plan)
template <int FAST>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
cchain_kernel(const ChainArgs a) {
    using Cfg = CCfg;
    constexpr int C = Cfg::C, NPT = Cfg::NPT, NK1 = Cfg::NK1, KK = Cfg::KK;
#ifndef F8_CC_DBG_NOSETREG
    if constexpr (FAST == 1) set_fp_round_nearest_even();
#endif
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* const ring2 = lds + Cfg::OFF_RING2;
    int* const bias_lds = (int*)(lds + Cfg::OFF_BIAS);         // b0 (64: this workgroup's two mid tiles) | b2 (64) | b4 (256: its eight stream tiles)
    int* const misc = (int*)(lds + Cfg::OFF_MISC);

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & 7;
    const int lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const unsigned l16 = (unsigned)(lane * 16);
    const int pp = wave & 3, kh = wave >> 2;                   // P1 / P2 role: pixel-tile pair, K half

    if (tid == 0) misc[0] = (int)chain_ticket(a.cs);
    __syncthreads();
    const int L = __builtin_amdgcn_readfirstlane(misc[0]);
    const int cl = L >> 3, c = L & 7;                          // cluster, member
    const int ncl = (int)(gridDim.x >> 3);
    const int ngroups = (a.N + Cfg::IMG - 1) / Cfg::IMG;
    const int npix = a.N * Cfg::PXI;
    unsigned* const flags = chain_flags(a.cs);
    const unsigned long long t_limit = (unsigned long long)a.cs.timeout_ticks;
    unsigned seq = 0;
#ifdef F8_TRACE
    unsigned tt[12] = {}; unsigned t_prev = (unsigned)__builtin_readcyclecounter();
#define F8_CT(i) do { const unsigned now_ = (unsigned)__builtin_readcyclecounter(); tt[i] += now_ - t_prev; t_prev = now_; } while (0)
#else
#define F8_CT(i)
#endif

    const __amdgpu_buffer_rsrc_t rxc = __builtin_amdgcn_make_buffer_rsrc((void*)(a.cs.xchg + (size_t)cl * Cfg::XCL_BYTES), 0, (unsigned)Cfg::XCL_BYTES, 0x00020000);
    auto wrsrc = [](const int8_t* p) { return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, 0x7ffffff0, 0x00020000); };

    // ---- exchange (f8_chain_common.h): signal; then the seven others' flags (bounded), barrier
    auto publish = [&]() { chain_signal(flags + L, ++seq); };
    auto wait_all = [&]() {
        if (tid < Cfg::G && tid != c) chain_wait_flag<0x80u, 1>(a.cs, flags + cl * Cfg::G + tid, seq, t_limit);
        __syncthreads();
    };
    // the whole cluster's mid1 / mid2 (112 fragments) -> LDS [0, 112 KB): 14 LDS-DMA instructions per wave
    auto load_patch = [&](int off) {
#pragma unroll
        for (int k = 0; k < 14; ++k) {
            const int e = wave * 14 + k;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rxc, F8_LDS3(lds + e * 1024), 16, l16, off + e * 1024, 0, 17);
        }
    };

    v16i res[NPT];                                             // the stream: this wave's channel tile (8 c + wave) x 7 pixel tiles
    const int ct = c * Cfg::CTC + wave;

    for (int grp = cl; grp < ngroups; grp += ncl) {
        const int m0 = grp * Cfg::NPX;                         // first global pixel of the group
        // =============================== stage input: the stream (I32T) -> registers; its int8 form -> exchange
        if (a.tail) {
            // TAIL: the stream is BORN here — the join of the stage-opening block whose 3x3 and shortcut have stride 2 (fix_resnet.py:55-77):
            //   stream = clamp(((Wsc . x(2p, 2q) + bsc) << sa) + ((W4 . mid2 + b4) << sr)) [ReLU],   K = 1024 + 512 for this wave's channel tile x 7 pixel tiles.
            // At most one of sa, sr is non-zero and everything wraps mod 2^32, so BOTH products accumulate in the stream registers: first the operand
            // that shifts, the shift, then the other one on top (one accumulator set instead of two: the registers hold nothing else yet).  K walks in six
            // chunks of 8 K32 steps; a chunk's B fragments (7 pixel tiles x 8 steps, gathered from the NHWC tensors by LDS-DMA: one pixel tile per wave,
            // the lane's pixel row is its offset) sit in one of two 64 KB LDS buffers, the wave's 8 weight fragments in registers, one chunk ahead.
            const ChainBlk& B = a.blk[0];
            const bool sc_first = B.res_shl == 0;                 // the shortcut's product shifts (or nothing does): it goes first
            const __amdgpu_buffer_rsrc_t rxs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x8in, 0, (unsigned)(a.N * 196 * 1024), 0x00020000);
            const __amdgpu_buffer_rsrc_t rm2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.m2in, 0, (unsigned)(npix * 512), 0x00020000);
            const __amdgpu_buffer_rsrc_t rwsc = wrsrc(B.wsc), rw4 = wrsrc(B.w4);
            unsigned vx, vm;                                       // this lane's pixel of pixel tile `wave` in the block input (stride 2) / in mid2
            {
                const int p = wave * 32 + l31, m = m0 + p;
                const int pi = p / Cfg::PXI, rem = p - pi * Cfg::PXI, r = rem / 7, cc = rem - r * 7;
                const bool ok = wave < NPT && p < Cfg::NPX && m < npix;
                vx = ok ? (unsigned)((((grp * Cfg::IMG + pi) * 14 + 2 * r) * 14 + 2 * cc) * 1024 + lh * 16) : kOOB;
                vm = ok ? (unsigned)(m * 512 + lh * 16) : kOOB;
            }
            auto chunk_is_sc = [&](int cq) { return sc_first ? cq < 4 : cq >= 2; };
            auto chunk_k = [&](int cq) { return sc_first ? (cq < 4 ? cq : cq - 4) : (cq < 2 ? cq : cq - 2); };   // the chunk's index inside its operand's K
            auto issue = [&](int cq) {                             // 8 fragments per wave: pixel tile `wave` (wave 7: nothing to fetch, zeros), K32 steps 8 k .. 8 k + 7
                char* const buf = lds + (cq & 1) * 65536 + wave * 8192;
                const bool sc = chunk_is_sc(cq);
                const int k0 = chunk_k(cq) * 256;
#pragma unroll
                for (int st = 0; st < 8; ++st) {
                    if (sc) __builtin_amdgcn_raw_ptr_buffer_load_lds(rxs, F8_LDS3(buf + st * 1024), 16, vx, k0 + st * 32, 0, 0);
                    else __builtin_amdgcn_raw_ptr_buffer_load_lds(rm2, F8_LDS3(buf + st * 1024), 16, vm, k0 + st * 32, 0, 0);
                }
            };
            v4i wa[2][8];
            auto load_w = [&](v4i (&dst)[8], int cq) {
                const bool sc = chunk_is_sc(cq);
                const int f0 = (ct * (sc ? 32 : 16) + chunk_k(cq) * 8) * 1024;
#pragma unroll
                for (int st = 0; st < 8; ++st) dst[st] = sc ? __builtin_amdgcn_raw_buffer_load_b128(rwsc, l16, f0 + st * 1024, 0) : __builtin_amdgcn_raw_buffer_load_b128(rw4, l16, f0 + st * 1024, 0);
            };
            issue(0);
            load_w(wa[0], 0);
            {   // the first operand's bias: the accumulators' start value
                const int32_t* const bf = sc_first ? B.bsc : B.b4;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const v4i bv = *(const v4i*)(bf + ct * 32 + 8 * g + 4 * lh);
#pragma unroll
                    for (int j = 0; j < NPT; ++j)
#pragma unroll
                        for (int e = 0; e < 4; ++e) res[j][4 * g + e] = bv[e];
                }
            }
            static_for<6>([&](auto qc) {
                constexpr int Q = decltype(qc)::value;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                lds_barrier();                                    // chunk Q is in LDS; everybody is past chunk Q - 1: its buffer takes chunk Q + 1
                if constexpr (Q + 1 < 6) { issue(Q + 1); load_w(wa[(Q + 1) & 1], Q + 1); }
                const char* const buf = lds + (Q & 1) * 65536;
#pragma unroll
                for (int st = 0; st < 8; ++st)
#pragma unroll
                    for (int j = 0; j < NPT; ++j) {
                        const v4i xf = *(const v4i*)(buf + (j * 8 + st) * 1024 + l16);
                        res[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wa[Q & 1][st], xf, res[j], 0, 0, 0);
                    }
                mfma_operands_read();
                if ((sc_first && Q == 3) || (!sc_first && Q == 1)) {       // the first operand is complete: its shift, then the second one's bias
                    const int sh = sc_first ? B.acc_shl : B.res_shl;
                    const int32_t* const bs = sc_first ? B.b4 : B.bsc;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const v4i bv = *(const v4i*)(bs + ct * 32 + 8 * g + 4 * lh);
#pragma unroll
                        for (int j = 0; j < NPT; ++j)
#pragma unroll
                            for (int e = 0; e < 4; ++e) res[j][4 * g + e] = (int)(((unsigned)res[j][4 * g + e] << sh) + (unsigned)bv[e]);
                    }
                }
            });
            const int floor1 = B.relu1 ? 0 : -2147483647;         // the join's clamp_(min=-(2^31-1)) and the ReLU floor are one max
            const ChainBlk& B1 = a.blk[1];
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
#pragma unroll
                for (int r = 0; r < 16; ++r) res[j][r] = max(res[j][r], floor1);
                const v4i o = quant_tile16<F8_CC_QI(FAST, F8_CC_Q_TAIL)>(res[j], B1.rq.n, FAST ? 0 : B1.rq.lo, FAST ? 255 : B1.rq.hi, FAST ? 0x80808080u : B1.rq.bias_xor);
                __builtin_amdgcn_raw_buffer_store_b128(o, rxc, l16, (j * NK1 + ct) * 1024, 17);
            }
            publish();
            F8_CT(0);
        } else {
            const ChainBlk& B0 = a.blk[0];
            const __amdgpu_buffer_rsrc_t rxr = __builtin_amdgcn_make_buffer_rsrc((void*)a.xr, 0, (unsigned)(((npix + 31) & ~31) * C * 4), 0x00020000);
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                const int p = j * 32 + l31, m = m0 + p;
                const unsigned vo = (p < Cfg::NPX && m < npix) ? (unsigned)((m >> 5) * (C * 128) + lh * 512 + (m & 31) * 16) : kOOB;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const v4i v = __builtin_amdgcn_raw_buffer_load_b128(rxr, vo + g * 1024, ct * 4096, 0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) res[j][4 * g + e] = v[e];
                }
            }
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                const v4i o = quant_tile16<FAST>(res[j], B0.rq.n, FAST ? 0 : B0.rq.lo, FAST ? 255 : B0.rq.hi, FAST ? 0x80808080u : B0.rq.bias_xor);
                __builtin_amdgcn_raw_buffer_store_b128(o, rxc, l16, (j * NK1 + ct) * 1024, 17);
            }
            publish();
            F8_CT(0);
        }

        for (int b = a.tail ? 1 : 0; b < a.nblk; ++b) {
            const ChainBlk& B = a.blk[b];
            const bool last = b + 1 == a.nblk;
            const ChainBlk& BN = a.blk[last ? b : b + 1];
            const int n1 = B.r1.n, n2 = B.r2.n, acc_shl = B.acc_shl, res_shl = B.res_shl;
            const int lo1 = FAST ? 0 : B.r1.lo, hi1 = FAST ? 255 : B.r1.hi, lo2 = FAST ? 0 : B.r2.lo, hi2 = FAST ? 255 : B.r2.hi;
            const unsigned xor1 = FAST ? 0x80808080u : B.r1.bias_xor, xor2 = FAST ? 0x80808080u : B.r2.bias_xor;
            const int relu_a = FAST ? 1 : B.relu_a, relu_b = FAST ? 1 : B.relu_b, relu1 = FAST ? 1 : B.relu1;
            const int nq = BN.rq.n, loq = FAST ? 0 : BN.rq.lo, hiq = FAST ? 255 : BN.rq.hi;
            const unsigned xorq = FAST ? 0x80808080u : BN.rq.bias_xor;

            // ---- this block's biases -> LDS (read from P1's epilogue on; the previous block's were last read at the top of its P3)
            {
                int bv = 0;
                if (tid < 64) bv = B.b0[c * 64 + tid];
                else if (tid < 128) bv = B.b2[c * 64 + tid - 64];
                else if (tid < Cfg::BIAS_INTS) bv = B.b4[c * 256 + tid - 128];
                if (tid < Cfg::BIAS_INTS) bias_lds[tid] = bv;
            }
            wait_all();                                         // x8 of the whole cluster is in memory
            F8_CT(1);

            // =============================== P1: mid1[64 c ..] = requant(relu(W0 . x8 + b0))
            {
                const __amdgpu_buffer_rsrc_t rw0 = wrsrc(B.w0);
                v16i acc[2][2];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[jj][i][r] = 0;
                constexpr int NCH = NK1 / 4, D = Cfg::D1, NI = 5;
                // chunk q: K32 steps 2q, 2q + 1 (K half 0) and 32 + 2q, 33 + 2q (K half 1); LDS image: fragment e = 4 j + t (x8, j = 0 .. 7) / 32 + 4 i + t (W0)
                auto issue = [&](int q) {
                    char* const slot = lds + (q % D) * Cfg::CH1_BYTES;
#pragma unroll
                    for (int k = 0; k < NI; ++k) {
                        const int e = wave * NI + k, t = e & 3;
                        const int step = t < 2 ? 2 * q + t : 32 + 2 * q + (t - 2);
                        if (e < 32) {
                            const int j = e >> 2;
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(rxc, F8_LDS3(slot + e * 1024), 16, j < NPT ? l16 : kOOB, (j * NK1 + step) * 1024, 0, 17);
                        } else {
                            const int i = (e - 32) >> 2;
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw0, F8_LDS3(slot + e * 1024), 16, l16, ((c * 2 + i) * NK1 + step) * 1024, 0, 0);
                        }
                    }
                };
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                issue(0); issue(1);
                const unsigned bb = (unsigned)((pp * 8 + kh * 2) * 1024) + l16, ab = (unsigned)((32 + kh * 2) * 1024) + l16;
                static_for<NCH>([&](auto qc) {
                    constexpr int Q = decltype(qc)::value;
                    constexpr int younger = (Q + D - 2 < NCH - 1 ? Q + D - 2 : NCH - 1) - Q;
                    wait_vmcnt<younger * NI>();
                    lds_barrier();
                    if constexpr (Q + D - 1 < NCH) issue(Q + D - 1);
                    const char* const slot = lds + (Q % D) * Cfg::CH1_BYTES;
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const v4i a0 = *(const v4i*)(slot + ab + s * 1024), a1 = *(const v4i*)(slot + ab + (4 + s) * 1024);
                        const v4i b0 = *(const v4i*)(slot + bb + s * 1024), b1 = *(const v4i*)(slot + bb + (4 + s) * 1024);
                        acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc[0][0], 0, 0, 0);
                        acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc[0][1], 0, 0, 0);
                        acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc[1][0], 0, 0, 0);
                        acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc[1][1], 0, 0, 0);
                    }
                });
                mfma_operands_read();                           // (no vector instruction reads an accumulator inside the loop: one guard behind it)
                F8_CT(2);
                __syncthreads();                                // the ring is dead: its bytes carry the K halves' exchange
                // wave (pp, kh) finishes channel tile kh of its two pixel tiles: it gives away its sums for tile 1 - kh and takes the partner's for tile kh
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        v4i o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = kh ? acc[jj][0][4 * g + e] : acc[jj][1][4 * g + e];
                        *(v4i*)(lds + (wave * 8 + jj * 4 + g) * 1024 + l16) = o;
                    }
                __syncthreads();
                const int floor0 = relu_a ? 0 : INT32_MIN;
                const int ctm = c * 2 + kh;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    v16i y;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const v4i o = *(const v4i*)(lds + ((wave ^ 4) * 8 + jj * 4 + g) * 1024 + l16);
                        const v4i bv = *(const v4i*)(bias_lds + kh * 32 + 8 * g + 4 * lh);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const unsigned mine = (unsigned)(kh ? acc[jj][1][4 * g + e] : acc[jj][0][4 * g + e]);
                            y[4 * g + e] = (int)(mine + (unsigned)o[e] + (unsigned)bv[e]);
                            if constexpr (!FAST) y[4 * g + e] = max(y[4 * g + e], floor0);
                        }
                    }
                    const int j = pp * 2 + jj;
                    const v4i o = quant_tile16<F8_CC_QI(FAST, F8_CC_Q_P1)>(y, n1, lo1, hi1, xor1);
                    if (j < NPT) __builtin_amdgcn_raw_buffer_store_b128(o, rxc, l16, Cfg::OFF_M1 + (j * KK + ctm) * 1024, 17);
                }
                publish();
                F8_CT(3);
            }
            {   // zeros for the out-of-image taps: [112 KB, 120 KB) — the barrier inside publish() is behind every read of the K-half exchange
                const v4i zv = {(int)xor1, (int)xor1, (int)xor1, (int)xor1};
                *(v4i*)(lds + Cfg::OFF_ZERO + tid * 16) = zv;
            }
            wait_all();                                         // mid1 of the whole cluster is in memory
            F8_CT(4);

            // =============================== P2: mid2[64 c ..] = requant(relu(conv3x3(mid1) + b2))
            {
                const __amdgpu_buffer_rsrc_t rw2 = wrsrc(B.w2);
                load_patch(Cfg::OFF_M1);
                constexpr int NCH = 36, D = Cfg::D2;
                // chunk q: tap q / 4, channel steps 2 (q % 4) + {0, 1} of each half-tap; LDS image: fragment e = 4 i + t
                auto issue = [&](int q) {
                    const int e = wave, i = e >> 2, t = e & 3;
                    const int step = (q >> 2) * KK + (t < 2 ? 0 : 8) + 2 * (q & 3) + (t & 1);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw2, F8_LDS3(ring2 + (q % D) * Cfg::CH2_BYTES + e * 1024), 16, l16, ((c * 2 + i) * (9 * KK) + step) * 1024, 0, 0);
                };
                issue(0); issue(1); issue(2);
                // LDS offset of tap (ty, tx) of this lane's pixel in the fragment-order patch, K half included; out-of-image: the zeros.  Derived per TAP from
                // the lane's row / column (kept: two registers per pixel tile; all 18 offsets at once were what the allocator spilled)
                int prow[2], pcol[2];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int p = (pp * 2 + jj) * 32 + l31;
                    const int rem = p % Cfg::PXI, r = rem / 7;
                    prow[jj] = p < Cfg::NPX ? r : 64; pcol[jj] = rem - r * 7;             // row 64: every tap of a padding lane is out of the image
                }
                unsigned tb[2] = {0u, 0u};
                auto tap_base = [&](auto tc) {
                    constexpr int T = decltype(tc)::value, TY = T / 3 - 1, TX = T % 3 - 1;
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        const int q = (pp * 2 + jj) * 32 + l31 + TY * 7 + TX;
                        const bool ok = (unsigned)(prow[jj] + TY) < 7u && (unsigned)(pcol[jj] + TX) < 7u;
                        tb[jj] = ok ? (unsigned)((q >> 5) * (KK * 1024) + kh * 8192 + lh * 512 + (q & 31) * 16) : (unsigned)Cfg::OFF_ZERO + l16;
                    }
                };
                v16i acc[2][2];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[jj][i][r] = 0;
                const unsigned ab = (unsigned)(kh * 2 * 1024) + l16;
                static_for<NCH>([&](auto qc) {
                    constexpr int Q = decltype(qc)::value, T = Q / 4;
                    constexpr int younger = (Q + D - 2 < NCH - 1 ? Q + D - 2 : NCH - 1) - Q;
                    wait_vmcnt<younger>();
                    lds_barrier();
                    if constexpr (Q + D - 1 < NCH) issue(Q + D - 1);
                    if constexpr (Q % 4 == 0) tap_base(std::integral_constant<int, T>{});
                    const char* const slot = ring2 + (Q % D) * Cfg::CH2_BYTES;
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const v4i a0 = *(const v4i*)(slot + ab + s * 1024), a1 = *(const v4i*)(slot + ab + (4 + s) * 1024);
                        const v4i b0 = *(const v4i*)(lds + tb[0] + (2 * (Q % 4) + s) * 1024), b1 = *(const v4i*)(lds + tb[1] + (2 * (Q % 4) + s) * 1024);
                        acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc[0][0], 0, 0, 0);
                        acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc[0][1], 0, 0, 0);
                        acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc[1][0], 0, 0, 0);
                        acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc[1][1], 0, 0, 0);
                    }
                });
                mfma_operands_read();                           // (no vector instruction reads an accumulator inside the loop: one guard behind it)
                F8_CT(5);
                __syncthreads();                                // nobody reads the patch any more: its bytes carry the K halves' exchange
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        v4i o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = kh ? acc[jj][0][4 * g + e] : acc[jj][1][4 * g + e];
                        *(v4i*)(lds + (wave * 8 + jj * 4 + g) * 1024 + l16) = o;
                    }
                __syncthreads();
                const int floor0 = relu_b ? 0 : INT32_MIN;
                const int ctm = c * 2 + kh;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    v16i y;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const v4i o = *(const v4i*)(lds + ((wave ^ 4) * 8 + jj * 4 + g) * 1024 + l16);
                        const v4i bv = *(const v4i*)(bias_lds + 64 + kh * 32 + 8 * g + 4 * lh);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const unsigned mine = (unsigned)(kh ? acc[jj][1][4 * g + e] : acc[jj][0][4 * g + e]);
                            y[4 * g + e] = (int)(mine + (unsigned)o[e] + (unsigned)bv[e]);
                            if constexpr (!FAST) y[4 * g + e] = max(y[4 * g + e], floor0);
                        }
                    }
                    const int j = pp * 2 + jj;
                    const v4i o = quant_tile16<F8_CC_QI(FAST, F8_CC_Q_P2)>(y, n2, lo2, hi2, xor2);
                    if (j < NPT) __builtin_amdgcn_raw_buffer_store_b128(o, rxc, l16, Cfg::OFF_M2 + (j * KK + ctm) * 1024, 17);
                }
                publish();
                F8_CT(6);
            }

            // =============================== P3: stream' = clamp((W4 . mid2 + b4) << sa + (stream << sr)) [ReLU]; x8' = requant(stream')
            {
                const __amdgpu_buffer_rsrc_t rw4 = wrsrc(B.w4);
                v4i wst[KK];                                    // this wave's weights: channel tile ct, all 16 K32 steps (requested before the wait)
#pragma unroll
                for (int k = 0; k < KK; ++k) wst[k] = __builtin_amdgcn_raw_buffer_load_b128(rw4, l16, (ct * KK + k) * 1024, 0);
                v16i breg;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const v4i bv = *(const v4i*)(bias_lds + 128 + wave * 32 + 8 * g + 4 * lh);
#pragma unroll
                    for (int e = 0; e < 4; ++e) breg[4 * g + e] = bv[e];
                }
                wait_all();                                     // mid2 of the whole cluster is in memory
                F8_CT(7);
                load_patch(Cfg::OFF_M2);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                F8_CT(8);
                const int floor1 = relu1 ? 0 : -2147483647;     // the join's clamp_(min=-(2^31-1)) and the ReLU floor are one max
                static_for<NPT>([&](auto jc) {
                    constexpr int J = decltype(jc)::value;
                    v16i acc;
#pragma unroll
                    for (int k = 0; k < KK; ++k) {
                        const v4i xf = *(const v4i*)(lds + (J * KK + k) * 1024 + l16);
                        if (k == 0) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wst[k], xf, breg, 0, 0, 0);
                        else acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wst[k], xf, acc, 0, 0, 0);
                    }
                    mfma_operands_read();
                    v16i& rr = res[J];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        if constexpr (FAST) rr[r] = max((int)(((unsigned)acc[r] << acc_shl) + (unsigned)rr[r]), 0);
                        else rr[r] = max((int)(((unsigned)acc[r] << acc_shl) + ((unsigned)rr[r] << res_shl)), floor1);
                    }
                    if (!last) {
                        const v4i o = quant_tile16<F8_CC_QI(FAST, F8_CC_Q_P3)>(rr, nq, loq, hiq, xorq);
                        __builtin_amdgcn_raw_buffer_store_b128(o, rxc, l16, (J * NK1 + ct) * 1024, 17);
                    } else if (!a.pool) {
                        const int p = J * 32 + l31, m = m0 + p;
                        if (p < Cfg::NPX && m < npix) {
                            const unsigned tot = (unsigned)(((npix + 31) & ~31) * C);
                            if (a.out32) {
                                const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)a.out32, 0, tot * 4u, 0x00020000);
                                const unsigned vo = (unsigned)((m >> 5) * (C * 128) + lh * 512 + (m & 31) * 16);
#pragma unroll
                                for (int g = 0; g < 4; ++g) {
                                    const v4i o = {rr[4 * g], rr[4 * g + 1], rr[4 * g + 2], rr[4 * g + 3]};
                                    __builtin_amdgcn_raw_buffer_store_b128(o, ro, vo + g * 1024, ct * 4096, 0);
                                }
                            }
#pragma unroll
                            for (int k = 0; k < 2; ++k)
                                if (a.q[k].ptr) {
                                    const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)a.q[k].ptr, 0, tot, 0x00020000);
                                    __builtin_amdgcn_raw_buffer_store_b128(quant_tile16<0>(rr, a.q[k].n, a.q[k].lo, a.q[k].hi, a.q[k].bias_xor), rq, (unsigned)(m * C + 16 * lh), ct * 32, 0);
                                }
                        }
                    }
                });
                if (last && a.pool) {
                    // FXQAvgPool2d (fix_quant_ops.py:126-134, int branch): the wrapping int32 sum over each image's 49 pixels, from the stream registers.  A lane holds
                    // pixel 32 j + l31 of the group's four images in tile j; per channel: the lane's share of each image (compile-time lane ranges), then a
                    // butterfly whose first two steps hand two / one of the four sums to the partner lane — every lane ends with the total of image (lane & 3)
                    const bool b0 = lane & 1, b1 = lane & 2;
                    const int n_img = grp * Cfg::IMG + (lane & 3);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        unsigned tot[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            unsigned sm[Cfg::IMG];
                            static_for<Cfg::IMG>([&](auto ic) {
                                constexpr int I = decltype(ic)::value, LO = I * Cfg::PXI, HI = LO + Cfg::PXI;
                                unsigned acc_i = 0;
                                static_for<NPT>([&](auto jc) {
                                    constexpr int J = decltype(jc)::value;
                                    if constexpr (J * 32 < HI && J * 32 + 32 > LO) {
                                        constexpr int L0 = LO - J * 32, L1 = HI - J * 32;      // this image's lanes of tile J: [L0, L1)
                                        acc_i += (l31 >= L0 && l31 < L1) ? (unsigned)res[J][4 * g + e] : 0u;
                                    }
                                });
                                sm[I] = acc_i;
                            });
                            const unsigned u0 = (b0 ? sm[1] : sm[0]) + (unsigned)__shfl_xor((int)(b0 ? sm[0] : sm[1]), 1);
                            const unsigned u1 = (b0 ? sm[3] : sm[2]) + (unsigned)__shfl_xor((int)(b0 ? sm[2] : sm[3]), 1);
                            unsigned v = (b1 ? u1 : u0) + (unsigned)__shfl_xor((int)(b1 ? u0 : u1), 2);
                            v += (unsigned)__shfl_xor((int)v, 4); v += (unsigned)__shfl_xor((int)v, 8); v += (unsigned)__shfl_xor((int)v, 16);
                            tot[e] = v;
                        }
                        if (l31 < Cfg::IMG && n_img < a.N) {
                            const int ch = ct * 32 + 8 * g + 4 * lh;
                            if (a.out32) { const v4i o = {(int)tot[0], (int)tot[1], (int)tot[2], (int)tot[3]}; *(v4i*)(a.out32 + i32t_index(n_img, ch, C)) = o; }
#pragma unroll
                            for (int k = 0; k < 2; ++k)
                                if (a.q[k].ptr)
                                    *(unsigned*)(a.q[k].ptr + (size_t)n_img * C + ch) =
                                        pack4(requant1((int)tot[0], a.q[k].n, a.q[k].lo, a.q[k].hi), requant1((int)tot[1], a.q[k].n, a.q[k].lo, a.q[k].hi),
                                              requant1((int)tot[2], a.q[k].n, a.q[k].lo, a.q[k].hi), requant1((int)tot[3], a.q[k].n, a.q[k].lo, a.q[k].hi)) ^ a.q[k].bias_xor;
                        }
                    }
                }
                F8_CT(9);
                if (!last) publish();
                else __syncthreads();                           // the next group's P1 ring overwrites mid2
                F8_CT(10);
            }
        }
    }
    chain_rearm<512>(a.cs, flags, misc + 2);
#ifdef F8_TRACE
    if (a.trace && lane == 0) {
        unsigned* tp = (unsigned*)a.trace + ((size_t)blockIdx.x * 8 + wave) * 16;
        for (int i = 0; i < 12; ++i) tp[i] = tt[i];
        tp[12] = (unsigned)L;
    }
#endif
}

// identity blocks only (cin0 = C: the stage's int32 stream comes in), or — tail — the JOIN of the stride-2 opening block first (cin0 = the block input's channels)
bool cchain_supported(int C, int MID, int H, int W, int cin0, bool tail) { return C == 2048 && MID == 512 && H == 7 && W == 7 && cin0 == (tail ? 1024 : 2048); }
size_t cchain_xchg_bytes() { return kCChainXchgBytes; }
// clusters (of 8 workgroups, 4 images per round) a launch over N images starts on a device with `slots` free compute units
int cchain_clusters(int N, int slots) {
    const int groups = (N + CCfg::IMG - 1) / CCfg::IMG, cap = std::min(slots / CCfg::G, 32);
    if (cap < 1) return 0;
    const int rounds = (groups + cap - 1) / cap;
    return (groups + rounds - 1) / rounds;                      // the fewest clusters that need no more rounds
}
int cchain_kernel_name(char* buf, size_t cap, int fast) { return snprintf(buf, cap, "f8::cchain_kernel<%d>", fast != 0 ? 2 : 0); }

template <int FAST>
static hipError_t launch_cchain_t(const ChainArgs& a, hipStream_t s) {
    static unsigned long long attr_done = 0; int attr_dev = -1;
    if (!dyn_lds_opted_in(&attr_done, &attr_dev)) {
        hipError_t e = hipFuncSetAttribute((const void*)cchain_kernel<FAST>, hipFuncAttributeMaxDynamicSharedMemorySize, CCfg::LDS_BYTES);
        if (e != hipSuccess) return e;
        if (attr_dev >= 0) attr_done |= 1ull << attr_dev;
    }
    const int grid = a.NG * CCfg::G;
    if (a.NG < 1 || grid > 256 || (a.tail ? (!a.x8in || !a.m2in || a.nblk < 2) : !a.xr)) return hipErrorInvalidValue;
#ifdef F8_TRACE
    static unsigned* tbuf = nullptr; static int count = 0;
    static const int want = [] { const char* e = getenv("F8_TRACE_CHAIN7"); return e ? atoi(e) : -1; }();
    ChainArgs b = a;
    const bool tracing = (count++ == want);
    if (tracing) { if (!tbuf) (void)hipMalloc((void**)&tbuf, (size_t)256 * 8 * 64); (void)hipMemsetAsync(tbuf, 0, (size_t)grid * 8 * 64, s); b.trace = tbuf; }
    hipLaunchKernelGGL((cchain_kernel<FAST>), dim3(grid), dim3(512), CCfg::LDS_BYTES, s, b);
    if (tracing) {
        (void)hipStreamSynchronize(s);
        static unsigned hb[256 * 8 * 16];
        (void)hipMemcpy(hb, tbuf, (size_t)grid * 8 * 64, hipMemcpyDeviceToHost);
        static const char* nm[11] = {"stage-in+publish", "wait x8", "P1 loop", "P1 epilogue+publish", "wait mid1", "P2 loop", "P2 epilogue+publish", "wait mid2", "P3 patch load", "P3 compute", "P3 publish"};
        for (int w : {0, 3, 4, 7}) {
            double ph[12] = {};
            for (int i = 0; i < grid; ++i) for (int k = 0; k < 12; ++k) ph[k] += (double)hb[((size_t)i * 8 + w) * 16 + k];
            fprintf(stderr, "[trace cchain<%d>] grid %d, %d blocks, N %d, wave %d: avg cycles per WG (whole launch):", FAST, grid, a.nblk, a.N, w);
            double tot = 0;
            for (int k = 0; k < 11; ++k) { fprintf(stderr, " %s %.0f |", nm[k], ph[k] / grid); tot += ph[k] / grid; }
            fprintf(stderr, " total %.0f\n", tot);
        }
    }
#else
    hipLaunchKernelGGL((cchain_kernel<FAST>), dim3(grid), dim3(512), CCfg::LDS_BYTES, s, a);
#endif
    return hipGetLastError();
}

// fast: chain_fast(a) (f8_chain.hip).  There is NO float-converter instance (1) of this kernel in the library: it was built, and its TAIL form returned a few wrong pixels in
// a third of the runs of a 130-image batch (tools/soak_chain7.py; tools/study_float_instance.sh on -DF8_CC_FLOAT_INSTANCE builds) — with the scheduling guard (mfma_operands_read, f8_chain_common.h) in place
// and the integer instance beside it exact in every run, soak and suite.  Isolated to ONE site: with the float arithmetic everywhere EXCEPT the requantisation of the
// freshly joined stream at the end of the TAIL phase (-DF8_CC_Q_TAIL=2) 0 of 300 runs differ, with it ONLY there 56 of 150; not the MODE write (same rate without
// s_setreg), not cured by wait states around the lane swaps; cause unknown.  The integer form is exact for every value the float form takes, so plans with
// requant_float = 1 run instance 2 here.
hipError_t launch_cchain(const ChainArgs& a, int fast, hipStream_t s) {
#ifdef F8_CC_FLOAT_INSTANCE      // (tuning builds: the float-converter instance, to study its failure)
    if (fast == 1) return launch_cchain_t<1>(a, s);
#endif
    return fast != 0 ? launch_cchain_t<2>(a, s) : launch_cchain_t<0>(a, s);
}

}  // namespace f8
