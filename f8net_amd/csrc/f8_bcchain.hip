// f8_bcchain.hip — the BasicBlocks of a 7x7 x 512 stage (ResNet-18 / 34 stage 3) and the average pool behind them in ONE launch over CLUSTERS of
// eight workgroups; the int32 residual stream stays in registers from block to block (gfx950).  Planning option fuse_bchain7 (off by default).
//
// BasicBlock.forward of the reference (two 3x3 convolutions, the join with the block input, every int_op_only_fix_quant in place) applied to
// consecutive blocks as IntModel.forward does.  This is f8_cchain.hip's cut (read its header first) re-cut for two 3x3s per block: a cluster of
// G = 8 workgroups with consecutive tickets owns IMG = 4 images (196 pixels = 7 pixel tiles of 32, plus a dummy eighth), and member c owns output
// channels [64 c, 64 c + 64) of BOTH 3x3s and of the stream:
//   * stream: wave (pp, kh) keeps pixel tile 2 pp + kh x the member's two channel tiles in registers (32 per lane);
//   * PA (3x3, K = 4608): mid[64 c ..] = requant(relu(Wa . x8 + ba)) over the whole cluster's x8 (112 KB, in LDS), 288 KB of Wa per member;
//   * PB (3x3, K = 4608): stream' = clamp(((Wb . mid + bb) << acc_shl) + (stream << res_shl)) [ReLU], x8' = requant(stream').
// Both phases are f8_cchain.hip's P2: the patch in MFMA-B-fragment order, out-of-image taps on 8 KB of biased zeros, the weights through a ring of
// 4 x 8 KB, wave (pp, kh) multiplies pixel tiles 2 pp, 2 pp + 1 by both channel tiles over K half kh; the halves then meet through LDS so that the
// wave ends with pixel tile 2 pp + kh (where its stream registers live) and both channel tiles.  Two exchanges per block (x8, mid: 112 KB each).
//
// TAIL (option value 2): the first block is only the JOIN of the stage-opening block — body.2 (3x3 over body.0's 7x7 int8 output, which an
// earlier launch wrote to HBM) and the 1x1 / 2 shortcut over the 14x14 block input:
//   stream = clamp(((Wb . mid0 + bb) << acc_shl) + ((Wsc . x(2p, 2q) + bsc) << res_shl)) [ReLU]
// The shortcut (K = 256, 8 steps) goes straight to the stream registers before the patch is loaded; mid0's patch is one LDS-DMA gather per
// fragment (a lane's 16 channels of one pixel: a per-lane pixel offset).  At most one of the two shifts is non-zero; everything wraps mod 2^32.
//
// Exchange protocol: f8_cchain.hip's, one flag per workgroup and exchange number (f8_chain_common.h).  ONE buffer per exchanged tensor
// (x8, mid), each rewritten two exchanges later.  Why that is safe: a member publishes exchange e only after its LDS-DMA loads of exchange e - 1's
// buffer have completed (the phase's K loop ends on vmcnt(0), publish() drains again), and a member writes a buffer for exchange e + 1 only after
// it has seen every member's flag of exchange e.  So nobody overwrites x8 (mid) while a member may still be reading it.  The next image group's
// stage input is one exchange behind the last block's PB, which read mid, not x8.
//
// requant_float = 1 plans run the integer instance (FAST = 2) here, as f8_cchain.hip: there is no float-converter instance of this kernel.
#include "f8_chain_common.h"
#include <algorithm>
#include <cstdio>

namespace f8 {

struct BCCfg {
    static constexpr int C = 512, PXI = 49, IMG = 4, NPX = PXI * IMG, NPT = 7, G = 8;
    static constexpr int KK = C / 32, KSC = C / 2 / 32;                                 // K32 steps of a tap / of the stride-2 shortcut (C / 2 channels)
    // exchange buffers of one cluster (fragment order [pixel tile][K32 step][lane][16 B])
    static constexpr int X_BYTES = NPT * KK * 1024, OFF_X8 = 0, OFF_MID = X_BYTES, XCL_BYTES = 2 * X_BYTES;
    // LDS
    static constexpr int PATCH_BYTES = X_BYTES;                                         // x8 (PA) / mid (PB) of the whole cluster
    static constexpr int ZERO_BYTES = 8192;                                             // biased zeros: what out-of-image taps read (8 K32 steps deep)
    static constexpr int D = 4, CH_BYTES = 8 * 1024;                                    // weight ring: 8 fragments per chunk
    static constexpr int OFF_ZERO = PATCH_BYTES, OFF_RING = PATCH_BYTES + ZERO_BYTES;
    static constexpr int OFF_BIAS = OFF_RING + D * CH_BYTES, BIAS_INTS = 128;           // ba (64: this member's channels) | bb (64)
    static constexpr int OFF_MISC = OFF_BIAS + BIAS_INTS * 4, LDS_BYTES = OFF_MISC + 256;
    static_assert(NPX * 64 * 4 <= PATCH_BYTES, "the pool's stream image fits in the patch's bytes");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};
constexpr size_t kBCChainXchgBytes = (size_t)32 * BCCfg::XCL_BYTES;                     // 32 clusters = 256 workgroups

// FAST: 0 = generic formats (signed, left shifts), 2 = ReLU everywhere, unsigned 8-bit formats with right shifts, the identity blocks' stream
// unshifted, integer requantisation (v_ashr_pk_u8_i32) — bchain_fast's rule
template <int FAST>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
bcchain_kernel(const BCChainArgs a) {
    using Cfg = BCCfg;
    constexpr int C = Cfg::C, NPT = Cfg::NPT, KK = Cfg::KK;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* const ring = lds + Cfg::OFF_RING;
    int* const bias_lds = (int*)(lds + Cfg::OFF_BIAS);
    int* const misc = (int*)(lds + Cfg::OFF_MISC);

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & 7;
    const int lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const unsigned l16 = (unsigned)(lane * 16);
    const int pp = wave & 3, kh = wave >> 2;                   // K loops: pixel-tile pair, K half
    const int jt = 2 * pp + kh;                                // the stream's pixel tile (7: the dummy)

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

    const __amdgpu_buffer_rsrc_t rxc = __builtin_amdgcn_make_buffer_rsrc((void*)(a.cs.xchg + (size_t)cl * Cfg::XCL_BYTES), 0, (unsigned)Cfg::XCL_BYTES, 0x00020000);
    auto wrsrc = [](const int8_t* p) { return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, 0x7ffffff0, 0x00020000); };

    // ---- exchange (f8_chain_common.h): signal; then the seven others' flags (bounded), barrier
    auto publish = [&]() { chain_signal(flags + L, ++seq); };
    auto wait_all = [&]() {
        if (tid < Cfg::G && tid != c) chain_wait_flag<0x80u, 1>(a.cs, flags + cl * Cfg::G + tid, seq, t_limit);
        __syncthreads();
    };
    // one exchanged tensor of the whole cluster (112 fragments) -> LDS [0, 112 KB): 14 LDS-DMA instructions per wave
    auto load_patch = [&](int off) {
#pragma unroll
        for (int k = 0; k < 14; ++k) {
            const int e = wave * 14 + k;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rxc, F8_LDS3(lds + e * 1024), 16, l16, off + e * 1024, 0, 17);
        }
    };
    // biased zeros of the format the next K loop reads: [112 KB, 120 KB)
    auto write_zeros = [&](unsigned x_or) {
        const v4i zv = {(int)x_or, (int)x_or, (int)x_or, (int)x_or};
        *(v4i*)(lds + Cfg::OFF_ZERO + tid * 16) = zv;
    };

    // ---- a 3x3, 512 -> 512 over the patch in LDS (the K loop: f8_cchain.hip P2's): y[i] = W . patch + bias for pixel tile jt, channel tiles 2 c + i
    auto conv3x3 = [&](const int8_t* w, const int* bias, v16i (&y)[2]) {
        const __amdgpu_buffer_rsrc_t rw = wrsrc(w);
        constexpr int NCH = 36, D = Cfg::D;
        // chunk q: tap q / 4, channel steps 2 (q % 4) + {0, 1} of each half-tap; LDS image: fragment e = 4 i + t
        auto issue = [&](int q) {
            const int e = wave, i = e >> 2, t = e & 3;
            const int step = (q >> 2) * KK + (t < 2 ? 0 : 8) + 2 * (q & 3) + (t & 1);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, F8_LDS3(ring + (q % D) * Cfg::CH_BYTES + e * 1024), 16, l16, ((c * 2 + i) * (9 * KK) + step) * 1024, 0, 0);
        };
        issue(0); issue(1); issue(2);
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
            const char* const slot = ring + (Q % D) * Cfg::CH_BYTES;
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
        mfma_operands_read();                        // (no vector instruction reads an accumulator inside the loop: one guard behind it)
        __syncthreads();                                // nobody reads the patch any more: its bytes carry the K halves' exchange
        // wave (pp, kh) keeps pixel tile 2 pp + kh: it gives away its sums for tile 2 pp + 1 - kh and takes the partner's (wave ^ 4) for tile 2 pp + kh
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                v4i o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = kh ? acc[0][i][4 * g + e] : acc[1][i][4 * g + e];
                *(v4i*)(lds + (wave * 8 + i * 4 + g) * 1024 + l16) = o;
            }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const v4i o = *(const v4i*)(lds + ((wave ^ 4) * 8 + i * 4 + g) * 1024 + l16);
                const v4i bv = *(const v4i*)(bias + i * 32 + 8 * g + 4 * lh);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned mine = (unsigned)(kh ? acc[1][i][4 * g + e] : acc[0][i][4 * g + e]);
                    y[i][4 * g + e] = (int)(mine + (unsigned)o[e] + (unsigned)bv[e]);
                }
            }
    };

    v16i res[2];                                               // the stream: pixel tile jt x channel tiles 2 c, 2 c + 1
    const bool jt_ok = jt < NPT;

    for (int grp = cl; grp < ngroups; grp += ncl) {
        const int m0 = grp * Cfg::NPX;                         // first global pixel of the group
        const int pj = jt * 32 + l31, mj = m0 + pj;            // this lane's pixel of the stream tile
        const bool px_ok = jt_ok && pj < Cfg::NPX && mj < npix;
        int b = 0;
        // =============================== stage input
        if (a.tail) {
            // TAIL: the stream is BORN here — the join of the stage-opening block (see the header)
            const BChainBlk& B = a.blk[0];
            {   // the shortcut, straight to the stream registers: Wsc . x(2 r, 2 q) + bsc, K = 256
                const __amdgpu_buffer_rsrc_t rxs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x8sc, 0, (unsigned)(a.N * 196 * (C / 2)), 0x00020000);
                const __amdgpu_buffer_rsrc_t rwsc = wrsrc(a.wsc);
                unsigned vx;
                {
                    const int pi = pj / Cfg::PXI, rem = pj - pi * Cfg::PXI, r = rem / 7, cc = rem - r * 7;
                    vx = px_ok ? (unsigned)((((grp * Cfg::IMG + pi) * 14 + 2 * r) * 14 + 2 * cc) * (C / 2) + lh * 16) : kOOB;
                }
                v4i xb[Cfg::KSC], wa[2][Cfg::KSC];
#pragma unroll
                for (int k = 0; k < Cfg::KSC; ++k) xb[k] = __builtin_amdgcn_raw_buffer_load_b128(rxs, vx, k * 32, 0);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int k = 0; k < Cfg::KSC; ++k) wa[i][k] = __builtin_amdgcn_raw_buffer_load_b128(rwsc, l16, ((c * 2 + i) * Cfg::KSC + k) * 1024, 0);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const v4i bv = *(const v4i*)(a.bsc + (c * 2 + i) * 32 + 8 * g + 4 * lh);
#pragma unroll
                        for (int e = 0; e < 4; ++e) res[i][4 * g + e] = bv[e];
                    }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
                for (int k = 0; k < Cfg::KSC; ++k)
#pragma unroll
                    for (int i = 0; i < 2; ++i) res[i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wa[i][k], xb[k], res[i], 0, 0, 0);
                mfma_operands_read();
            }
            if (tid < 64) bias_lds[64 + tid] = B.bb[c * 64 + tid];
            write_zeros(FAST ? 0x80808080u : B.r1.bias_xor);
            {   // mid0 of the group (NHWC in HBM) -> LDS in fragment order: fragment e = (pixel tile e / KK, K32 step e % KK), one gather per fragment
                const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc((void*)a.m0in, 0, (unsigned)(npix * C), 0x00020000);
#pragma unroll
                for (int k = 0; k < 14; ++k) {
                    const int e = wave * 14 + k, j = e / KK, st = e - j * KK;
                    const int p = j * 32 + l31, m = m0 + p;
                    const unsigned vm = (p < Cfg::NPX && m < npix) ? (unsigned)(m * C + lh * 16) : kOOB;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rm, F8_LDS3(lds + e * 1024), 16, vm, st * 32, 0, 0);
                }
            }
            v16i y[2];
            conv3x3(B.wb, bias_lds + 64, y);
            const int floor1 = FAST ? 0 : (B.relu1 ? 0 : -2147483647);   // the join's clamp_(min=-(2^31-1)) and the ReLU floor are one max
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) res[i][r] = max((int)(((unsigned)y[i][r] << B.acc_shl) + ((unsigned)res[i][r] << B.res_shl)), floor1);
            b = 1;
        } else {
            const __amdgpu_buffer_rsrc_t rxr = __builtin_amdgcn_make_buffer_rsrc((void*)a.xr, 0, (unsigned)(((npix + 31) & ~31) * C * 4), 0x00020000);
            const unsigned vo = px_ok ? (unsigned)((mj >> 5) * (C * 128) + lh * 512 + (mj & 31) * 16) : kOOB;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const v4i v = __builtin_amdgcn_raw_buffer_load_b128(rxr, vo + g * 1024, (c * 2 + i) * 4096, 0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) res[i][4 * g + e] = v[e];
                }
        }

        // =============================== the stage's output forms (after its last block): the pool, or int32 / int8 maps
        auto write_outputs = [&]() {
            if (!a.pool) {
                if (!px_ok) return;
                const unsigned tot = (unsigned)(((npix + 31) & ~31) * C);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int ct = c * 2 + i;
                    if (a.out32) {
                        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)a.out32, 0, tot * 4u, 0x00020000);
                        const unsigned vo = (unsigned)((mj >> 5) * (C * 128) + lh * 512 + (mj & 31) * 16);
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const v4i o = {res[i][4 * g], res[i][4 * g + 1], res[i][4 * g + 2], res[i][4 * g + 3]};
                            __builtin_amdgcn_raw_buffer_store_b128(o, ro, vo + g * 1024, ct * 4096, 0);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 2; ++k)
                        if (a.q[k].ptr) {
                            const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)a.q[k].ptr, 0, tot, 0x00020000);
                            __builtin_amdgcn_raw_buffer_store_b128(quant_tile16<0>(res[i], a.q[k].n, a.q[k].lo, a.q[k].hi, a.q[k].bias_xor), rq, (unsigned)(mj * C + 16 * lh), ct * 32, 0);
                        }
                }
                return;
            }
            // FXQAvgPool2d (the reference's int branch): the wrapping int32 sum over each image's 49 pixels.  The waves' stream registers -> an LDS image
            // [196 pixels][64 channels] (the patch's bytes: the barrier below is behind the last read of the K halves' exchange), then thread
            // (image, 4 channels) adds its image's 49 pixels
            __syncthreads();
            int* const simg = (int*)lds;
            if (jt_ok && pj < Cfg::NPX) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const v4i o = {res[i][4 * g], res[i][4 * g + 1], res[i][4 * g + 2], res[i][4 * g + 3]};
                        *(v4i*)(simg + pj * 64 + i * 32 + 8 * g + 4 * lh) = o;
                    }
            }
            __syncthreads();
            if (tid < Cfg::IMG * 16) {
                const int im = tid >> 4, ch4 = (tid & 15) * 4, n_img = grp * Cfg::IMG + im;
                if (n_img < a.N) {
                    unsigned s[4] = {0u, 0u, 0u, 0u};
                    for (int q = 0; q < Cfg::PXI; ++q) {
                        const v4i v = *(const v4i*)(simg + (im * Cfg::PXI + q) * 64 + ch4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) s[e] += (unsigned)v[e];
                    }
                    const int ch = c * 64 + ch4;
                    if (a.out32) { const v4i o = {(int)s[0], (int)s[1], (int)s[2], (int)s[3]}; *(v4i*)(a.out32 + i32t_index(n_img, ch, C)) = o; }
#pragma unroll
                    for (int k = 0; k < 2; ++k)
                        if (a.q[k].ptr)
                            *(unsigned*)(a.q[k].ptr + (size_t)n_img * C + ch) =
                                pack4(requant1((int)s[0], a.q[k].n, a.q[k].lo, a.q[k].hi), requant1((int)s[1], a.q[k].n, a.q[k].lo, a.q[k].hi),
                                      requant1((int)s[2], a.q[k].n, a.q[k].lo, a.q[k].hi), requant1((int)s[3], a.q[k].n, a.q[k].lo, a.q[k].hi)) ^ a.q[k].bias_xor;
                }
            }
        };
        // the int8 input of block bn (its first conv's format) -> the x8 exchange
        auto publish_x8 = [&](const BChainBlk& BN) {
            if (jt_ok) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const v4i o = quant_tile16<FAST>(res[i], BN.rq.n, FAST ? 0 : BN.rq.lo, FAST ? 255 : BN.rq.hi, FAST ? 0x80808080u : BN.rq.bias_xor);
                    __builtin_amdgcn_raw_buffer_store_b128(o, rxc, l16, Cfg::OFF_X8 + (jt * KK + c * 2 + i) * 1024, 17);
                }
            }
            publish();
        };

        if (b == a.nblk) write_outputs();                      // (a TAIL chain of one block: the opener's join alone)
        else publish_x8(a.blk[b]);

        for (; b < a.nblk; ++b) {
            const BChainBlk& B = a.blk[b];
            const bool last = b + 1 == a.nblk;
            // ---- this block's biases -> LDS (the previous ones were last read before the barrier inside publish())
            if (tid < 64) bias_lds[tid] = B.ba[c * 64 + tid];
            else if (tid < 128) bias_lds[tid] = B.bb[c * 64 + tid - 64];
            write_zeros(FAST ? 0x80808080u : B.rq.bias_xor);
            wait_all();                                         // x8 of the whole cluster is in memory

            // =============================== PA: mid[64 c ..] = requant(relu(Wa . x8 + ba))
            {
                load_patch(Cfg::OFF_X8);
                v16i y[2];
                conv3x3(B.wa, bias_lds, y);
                const int floor0 = (FAST || B.relu_a) ? 0 : INT32_MIN;
                if (jt_ok) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        if constexpr (!FAST)
#pragma unroll
                            for (int r = 0; r < 16; ++r) y[i][r] = max(y[i][r], floor0);
                        const v4i o = quant_tile16<FAST>(y[i], B.r1.n, FAST ? 0 : B.r1.lo, FAST ? 255 : B.r1.hi, FAST ? 0x80808080u : B.r1.bias_xor);
                        __builtin_amdgcn_raw_buffer_store_b128(o, rxc, l16, Cfg::OFF_MID + (jt * KK + c * 2 + i) * 1024, 17);
                    }
                }
                publish();
            }
            write_zeros(FAST ? 0x80808080u : B.r1.bias_xor);          // (the barrier inside publish() is behind every read of the K halves' exchange)
            wait_all();                                         // mid of the whole cluster is in memory

            // =============================== PB: stream' = clamp(((Wb . mid + bb) << acc_shl) + (stream << res_shl)) [ReLU]
            {
                load_patch(Cfg::OFF_MID);
                v16i y[2];
                conv3x3(B.wb, bias_lds + 64, y);
                const int acc_shl = B.acc_shl, res_shl = B.res_shl;
                const int floor1 = B.relu1 ? 0 : -2147483647;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        if constexpr (FAST) res[i][r] = max((int)(((unsigned)y[i][r] << acc_shl) + (unsigned)res[i][r]), 0);
                        else res[i][r] = max((int)(((unsigned)y[i][r] << acc_shl) + ((unsigned)res[i][r] << res_shl)), floor1);
                    }
                if (!last) publish_x8(a.blk[b + 1]);
                else write_outputs();
            }
        }
        __syncthreads();                                        // the next group's loads overwrite the LDS the pool / the epilogue read
    }
    chain_rearm<512>(a.cs, flags, misc + 2);
}

// identity blocks (or, opener: the join of the stage-opening block first) of a 7x7 x 512 BasicBlock stage
bool bcchain_supported(int C, int H, int W, bool opener) { (void)opener; return C == 512 && H == 7 && W == 7; }
size_t bcchain_xchg_bytes() { return kBCChainXchgBytes; }
int bcchain_inst(const BCChainArgs& a, bool q8) {          // bchain_fast's rule; its float-converter choice (1) runs the integer instance here
    for (int k = 0; k < a.nblk; ++k) {
        const BChainBlk& B = a.blk[k];
        if (!(B.relu_a && B.relu1 && B.r1.u8_shr())) return 0;
        if (k == 0 && a.tail) continue;                               // opening block: its input arrives as int8, its join shifts either operand
        if (!(B.rq.u8_shr() && B.res_shl == 0)) return 0;
    }
    if (q8 && !a.q[0].u8_shr()) return 0;
    return 2;
}
int bcchain_kernel_name(char* buf, size_t cap, int inst) { return snprintf(buf, cap, "f8::bcchain_kernel<%d>", inst != 0 ? 2 : 0); }

template <int FAST>
static hipError_t launch_bcchain_t(const BCChainArgs& a, hipStream_t s) {
    static unsigned long long attr_done = 0; int attr_dev = -1;
    if (!dyn_lds_opted_in(&attr_done, &attr_dev)) {
        hipError_t e = hipFuncSetAttribute((const void*)bcchain_kernel<FAST>, hipFuncAttributeMaxDynamicSharedMemorySize, BCCfg::LDS_BYTES);
        if (e != hipSuccess) return e;
        if (attr_dev >= 0) attr_done |= 1ull << attr_dev;
    }
    const int grid = a.NG * BCCfg::G;
    hipLaunchKernelGGL((bcchain_kernel<FAST>), dim3(grid), dim3(512), BCCfg::LDS_BYTES, s, a);
    return hipGetLastError();
}

hipError_t launch_bcchain(const BCChainArgs& a, int inst, hipStream_t s) {
    if (a.NG < 1 || a.NG * BCCfg::G > 256 || a.nblk < 1 || a.nblk > kBChainMaxBlocks) return hipErrorInvalidValue;
    if (a.tail ? !(a.m0in && a.x8sc && a.wsc && a.bsc) : !a.xr) return hipErrorInvalidValue;
    return inst != 0 ? launch_bcchain_t<2>(a, s) : launch_bcchain_t<0>(a, s);
}

}  // namespace f8
