// f8_gconvp.hip — grouped 1x1 (pointwise) convolution, cin != cout allowed, "group-aligned over flat pixels" on v_mfma_i32_32x32x32_i8 (gfx950 only).
//
// The shapes: kernel 1, stride 1, pad 0, 1 < groups < cin; cgi = cin / groups and cgo = cout / groups multiples of 4, 4 <= cgi <= 512, cgo >= 4; the
// int32 output form only where cgo is a multiple of 8.  A 1x1 at stride 1 has no halo and no image border: the conv is a batched GEMM over the
// M = N H W pixel rows of the NHWC tensor, flat — a tile of TP pixels may straddle images, no division by a map size anywhere, the one bound is M.
//
//   * UNITS are f8_gconvw.hip's: unit g NSUB + j = group g x 32-output subtile j (NSUB = ceil(cgo / 32)), live = min(32, cgo - 32 j) channels — a multiple
//     of 4 —, K = the group's own cgi input bytes over KS = ceil(cgi / 32) K32 steps.  The packer (f8_net.cpp pack_gconvp_weights) writes
//     [unit][kstep][lane][16 B] in MFMA-fragment order with zero rows past `live` and zero K bytes past cgi: the kernel has no notion of groups.  Where
//     the outputs' Cs > cout one all-zero unit behind the last group writes the padded channels cout .. Cs - 1 through the same epilogue.
//   * A WORKGROUP (4 waves) owns one tile of TP pixels (a multiple of 32, at most 256) x a SPAN of GS consecutive whole groups (gconvp_plan: as many as give
//     every wave four units, within 64 KB of LDS — two workgroups a CU).  The spans of one tile are consecutive workgroups: they read neighbouring pieces
//     of the same pixel rows while those are in L2.
//   * REGROUP ON THE WAY IN.  The span's bytes of every pixel go to LDS as [pixel][group in span][32 KS] + 16 bytes of pad a pixel — the pixel pitch is
//     an ODD number of 16-byte chunks, so 16 consecutive pixels cover the 16 chunk columns of a 256-byte bank row once (f8_gconvx.hip's pitch rule; the pad
//     stands once behind the pixel's groups, not behind each: an odd pitch needs no more).  Every group starts 16-byte aligned in LDS whatever g cgi is in
//     the row, so every operand read is ONE ds_read_b128.  Two loader instances, both LDS-direct, no register pass: SB = 16-byte slots where cgi is a
//     multiple of 8 (the source is then 8-byte aligned, which the 16-byte LDS-direct load takes: f8_gconvx.hip) and SB = 4-byte slots otherwise (dword
//     aligned, since cgi is a multiple of 4).  Only the ceil(cgi / SB) slots of a group that meet a non-zero weight are fetched; every other slot — the
//     rest of the group's 32 KS, the pad, groups past the last, pixels past M — is written as zeros by the buffer range check.  The last 16-byte slot of a
//     group may run 8 bytes past it: into the next group, the next pixel or (range check) past the tensor; those K bytes meet zero weights.
//   * COMPUTE.  A wave takes the span's units round-robin, keeps the unit's KS weight fragments in registers (at most 64 VGPRs at cgi = 512; instances
//     KSM = 1, 2, 4, 8, 16 are the register array's size, KS itself is a run-time bound under wave-uniform guards) and walks the tile's 32-pixel groups
//     against them — gconvw's role assignment: the weights of a pointwise group are small.  The NEXT unit's fragments are loaded into a second register
//     set under the current unit's pixel walk (two sets: 128 VGPRs at KSM = 16, inside the 256 of two waves a SIMD).
//   * MFMA SHAPE: v_mfma_i32_32x32x32_i8 throughout.  v_mfma_i32_16x16x64_i8 for cgo <= 16 is NOT built: at those widths a unit multiplies 32 rows of which
//     4 .. 16 are live, but the launch runs at 7 .. 27 % of its HBM floor (profiles/gconv_pw_r24.md): the matrix pipe is not what holds it.
//   * EPILOGUE from registers: per-channel bias (one class: no padding; the packer folds the storage bias of unsigned inputs into it), ReLU floor, the
//     tiled int32 form (16 bytes per lane and live 8-channel group) and / or up to two int8 forms — integer requantisation whatever
//     Options::requant_float says (requant_u8x4_int for an unsigned form by a right shift: 23.4 against 25.8 us on 60 -> 240 x 28 x 28 at 128 images; else requant1).  int8: the lane halves swap (half h holds channels 16 h .. + 15 of the unit); a unit's channel base is a multiple of 4,
//     so a lane stores its live quads as 16 bytes, as 8-byte pieces or as dwords — by the base's alignment, a wave-uniform choice made once a unit.  Units
//     are disjoint runs of whole dwords: no two workgroups ever write the same dword.  No residual join.
#include "f8_device.h"
#include <algorithm>

namespace f8 {

typedef int v2i __attribute__((ext_vector_type(2)));

namespace {
constexpr int GP_LDS_BUDGET = 64 * 1024;            // staged bytes per workgroup: two workgroups a CU
constexpr int GP_TP_MAX = 256;                      // pixels of a tile: eight 32-pixel groups
constexpr int GP_WG_TARGET = 512;                   // workgroups a launch should have before its tiles grow past 32 pixels: two per CU of a 256-CU device
}

template <int SB, int KSM>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) gconvp1x1_kernel(const GConvPArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;
    const int l31 = lane & 31, lh = lane >> 5;

    // ---- this workgroup's tile and span: span fastest
    const int tile = blockIdx.x / a.nspan, sp = blockIdx.x - tile * a.nspan;
    const int m0 = tile * a.TP;
    const int M = a.N * a.HW;
    const int tpx = min(a.TP, M - m0);                          // live pixels of the tile
    const int g0 = sp * a.GS;
    const int ng = min(a.GS, a.groups - g0);                    // live groups of the span
    const int KS = a.ks;

    // ---- regroup: every SB-byte slot of the live pixels once, linear in LDS: slot s = slot s % CHS of pixel s / CHS, slot c of a pixel = K bytes
    //      SB (c % GSL) .. of group c / GSL of the span (c / GSL == GS: the pad)
    const int CHS = a.pitch / SB, GSL = 32 * KS / SB;
    const int slots = tpx * CHS;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
    for (int i = 0; i * 256 + wave * 64 < slots; ++i) {         // wave-uniform bound
        const int s = i * 256 + tid;
        const int ppx = (int)fast_div((unsigned)s, a.dCHS), c = s - ppx * CHS;
        const int gl = (int)fast_div((unsigned)c, a.dGSL), kb = (c - gl * GSL) * SB;
        const bool ok = s < slots && gl < ng && kb < a.cgi;
        const unsigned off = ok ? (unsigned)((m0 + ppx) * a.Ci + (g0 + gl) * a.cgi + kb) : kOOB;
        auto* dst = (__attribute__((address_space(3))) void*)(lds + (i * 256 + wave * 64) * SB);      // (the size is a literal to the builtin)
        if constexpr (SB == 16) __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, dst, 16, off, 0, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, dst, 4, off, 0, 0, 0);
    }

    // ---- the span's units: NSUB subtiles of each live group, and behind the last group of the conv the pad unit
    const int nsub = a.nsub;
    const bool padu = a.Co > a.cout && sp == a.nspan - 1;
    const int nu = ng * nsub + (padu ? 1 : 0);
    const int npg = (tpx + 31) >> 5;
    const int floor0 = a.relu0 ? 0 : INT32_MIN;

    auto load_unit = [&](v4i (&wf)[KSM], int u) {
        const int gl = u / nsub, j = u - gl * nsub;             // (the pad unit: gl = ng, j = 0: packed unit groups * NSUB)
        const v4i* wp = (const v4i*)a.w + (size_t)((g0 + gl) * nsub + j) * (size_t)(KS * 64) + lane;
#pragma unroll
        for (int ks = 0; ks < KSM; ++ks)
            if (ks < KS) wf[ks] = wp[ks * 64];                  // wave-uniform
    };

    auto run_unit = [&](const v4i (&wf)[KSM], int u) {
        const int gl = u / nsub, j = u - gl * nsub;
        const bool pu = gl == ng;                               // the pad unit: zero weights against group 0's bytes
        const int co = pu ? a.cout : (g0 + gl) * a.cgo + 32 * j;       // first output channel: a multiple of 4
        const int live = pu ? a.Co - a.cout : min(32, a.cgo - 32 * j); // a multiple of 4
        const int al = co & 15;                                 // wave-uniform store width: 0: 16 bytes, 8: 8-byte pieces, else dwords
        const int n4 = min(4, max(0, (live - 16 * lh) >> 2));   // live channel quads of this lane half's 16 channels
        const unsigned xoff = (unsigned)((pu ? 0 : gl) * 32 * KS + 16 * lh);
        for (int pg = 0; pg < npg; ++pg) {
            const unsigned ad = (unsigned)((pg * 32 + l31) * a.pitch) + xoff;   // (pixels past tpx: stale or unwritten LDS inside the allocation, result unused)
            v16i acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
            for (int ks = 0; ks < KSM; ++ks) {
                if (ks >= KS) continue;                         // wave-uniform
                const v4i xb = *(const v4i*)(lds + ad + 32 * ks);
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[ks], xb, acc, 0, 0, 0);
            }

            // ---- epilogue: D register r of lane l = channel (r & 3) + 8 (r >> 2) + 4 (l >> 5) of pixel l & 31; rows past `live` are zero and unused
            const int m = m0 + pg * 32 + l31;
            const bool ok = pg * 32 + l31 < tpx;
            int y[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                v4i b = {0, 0, 0, 0};
                if (8 * g + 4 * lh < live) b = *(const v4i*)(a.bias + co + 8 * g + 4 * lh);
#pragma unroll
                for (int e = 0; e < 4; ++e) y[g][e] = max((int)((unsigned)acc[4 * g + e] + (unsigned)b[e]), floor0);
            }
            if (a.out32 && ok) {                                // (planned only where cgo, hence co and live, are multiples of 8)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (8 * g >= live) continue;                // wave-uniform
                    v4i o = {y[g][0], y[g][1], y[g][2], y[g][3]};
                    *(v4i*)(a.out32 + i32t_index(m, co + 8 * g + 4 * lh, a.Co)) = o;
                }
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!a.q[k].ptr) continue;                      // wave-uniform
                unsigned d[4];
                if (a.q[k].u8_shr()) {                          // wave-uniform: unsigned 8-bit by a right shift, the usual form: 2 3/4 integer operations a value
#pragma unroll
                    for (int g = 0; g < 4; ++g) d[g] = requant_u8x4_int(y[g][0], y[g][1], y[g][2], y[g][3], a.q[k].n) ^ a.q[k].bias_xor;
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g) d[g] = requant_pack4(y[g][0], y[g][1], y[g][2], y[g][3], a.q[k]);
                }
                // lane half 0 collects channels 0 .. 15 of its pixel, half 1 channels 16 .. 31
                auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
                auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
                if (!ok) continue;
                int8_t* dst = a.q[k].ptr + (size_t)m * a.Co + co + 16 * lh;
                const int v[4] = {(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
                if (al == 0 && n4 == 4) {
                    v4i o = {v[0], v[1], v[2], v[3]};
                    *(v4i*)dst = o;
                } else if ((al & 7) == 0) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        if (n4 >= 2 * h + 2) { v2i o = {v[2 * h], v[2 * h + 1]}; *(v2i*)(dst + 8 * h) = o; }
                        else if (n4 == 2 * h + 1) *(int*)(dst + 8 * h) = v[2 * h];
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < n4) *(int*)(dst + 4 * e) = v[e];
                }
            }
        }
    };

    // ---- units round-robin, two register sets: the next unit's fragments arrive under the current unit's pixel walk
    v4i wa[KSM], wb[KSM];
    if (wave < nu) load_unit(wa, wave);
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    for (int u = wave; u < nu; u += 8) {                        // wave-uniform
        if (u + 4 < nu) load_unit(wb, u + 4);
        run_unit(wa, u);
        if (u + 4 >= nu) break;
        if (u + 8 < nu) load_unit(wa, u + 8);
        run_unit(wb, u + 4);
    }
}

// The launch's geometry, chosen at finalize from the conv alone and the largest batch's pixel count M:
//   GS   groups a workgroup: as many as give each of the four waves four units (16 units of NSUB a group), at most what leaves a 32-pixel tile inside the LDS budget
//   TP   pixels a tile: the largest of 256 / 128 / 64 / 32 that fits the budget and still leaves GP_WG_TARGET workgroups (else 32)
void gconvp_plan(int groups, int cgi, int cgo, long M, int* GS, int* TP, int* pitch) {
    const int KS = (cgi + 31) / 32, nsub = (cgo + 31) / 32;
    *GS = std::max(1, std::min({groups, (16 + nsub - 1) / nsub, (GP_LDS_BUDGET / 32 - 16) / (32 * KS)}));
    *pitch = *GS * 32 * KS + 16;
    const long nspan = (groups + *GS - 1) / *GS;
    *TP = 32;
    for (int tp = GP_TP_MAX; tp > 32; tp >>= 1)
        if (tp * *pitch <= GP_LDS_BUDGET && (M + tp - 1) / tp * nspan >= GP_WG_TARGET) { *TP = tp; break; }
}

// Where option gconv_pw = 1 plans the kernel: MEASURED at 128 images on 19 layer shapes against the dense expansion (profiles/gconv_pw_r24.md).  The launch was
// faster by more than the spread of the repeated legs on three of them — 768 -> 192, 1536 -> 384 and 384 -> 1536 at 8 groups (1.37x, 1.24x, 1.13x) — and
// slower or inside the spread on the other sixteen (0.69x .. 0.98x): every shape of 2 or 3 groups, where the expansion wastes little and conv_igemm_kernel's
// 128-wide tiles are hard to beat, and at 8 groups the narrow ones (cgi 12 / 24, or a dense product cin x cout below 2^17).  The rule is the smallest box
// around the wins: 8 or more groups, cgi >= 48, cin x cout >= 2^17.  Everything else stays on the expansion under gconv_pw = 1; gconv_pw = 2 takes the whole set.
bool gconvp_rule(int groups, int cgi, int cgo) { return groups >= 8 && cgi >= 48 && (long)groups * cgi * groups * cgo >= (1L << 17); }

static int gconvp_ksm(int ks) { return ks <= 1 ? 1 : ks <= 2 ? 2 : ks <= 4 ? 4 : ks <= 8 ? 8 : 16; }

int gconvp_kernel_name(char* buf, size_t cap, const GConvPArgs& a) { return snprintf(buf, cap, "f8::gconvp1x1_kernel<%d, %d>", a.cgi % 8 ? 4 : 16, gconvp_ksm(a.ks)); }

template <int SB>
static auto gconvp_instance(int ksm) {
    switch (ksm) {
        case 1: return gconvp1x1_kernel<SB, 1>;
        case 2: return gconvp1x1_kernel<SB, 2>;
        case 4: return gconvp1x1_kernel<SB, 4>;
        case 8: return gconvp1x1_kernel<SB, 8>;
        default: return gconvp1x1_kernel<SB, 16>;
    }
}

hipError_t launch_gconvp(const GConvPArgs& a, hipStream_t s) {
    // the set, and what the kernel's addressing rests on: whole groups inside both rows, plus at most one pad unit up to Co; every K32 read of a group
    // inside its 32 KS bytes, every group 16-byte aligned in an odd pitch; bytes past a group meet zero weights (the packer), bytes past the tensor are
    // the range check's; the tiled int32 form per 8-channel group
    const long M = (long)a.N * a.HW;
    if (a.N < 1 || a.HW < 1 || M > 0x7fffffffL || a.groups < 2 || a.cgi % 4 || a.cgo % 4 || a.cgi < 4 || a.cgi > 512 || a.cgo < 4 ||
        a.cout != a.groups * a.cgo || a.groups * a.cgi > a.Ci || a.Ci % 32 || a.Co % 32 || a.cout > a.Co || a.Co - a.cout >= 32 ||
        a.ks != (a.cgi + 31) / 32 || a.nsub != (a.cgo + 31) / 32 || a.GS < 1 || a.nspan != (a.groups + a.GS - 1) / a.GS ||
        a.pitch != a.GS * 32 * a.ks + 16 || a.TP < 32 || a.TP > GP_TP_MAX || a.TP % 32 || a.TP * a.pitch > GP_LDS_BUDGET ||
        (a.out32 && a.cgo % 8) || (uint64_t)M * (uint64_t)a.Ci > (uint64_t)a.x_bytes || a.x_bytes >= kOOB)
        return hipErrorInvalidValue;
    const long grid = (M + a.TP - 1) / a.TP * a.nspan;
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    auto k = a.cgi % 8 ? gconvp_instance<4>(gconvp_ksm(a.ks)) : gconvp_instance<16>(gconvp_ksm(a.ks));
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(256), (a.TP * a.pitch + 1023) / 1024 * 1024, s, a);      // whole 1 KB wave pieces of the 16-byte loader
    return hipGetLastError();
}

}  // namespace f8
