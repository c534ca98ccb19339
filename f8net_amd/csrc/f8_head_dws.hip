// f8_head_dws.hip — MobileNet-V1 head and first depthwise-separable block in one launch (gfx950 only; option fuse_head_dws):
//   3x3 / 2 conv (cin <= 4 -> 32, ReLU) -> depthwise 3x3 / 1 / pad 1 (32 channels, ReLU) -> 1x1 (32 -> NT x 32 channels, NT = 1 or 2, [ReLU]).
//
// The skeleton and the data flow are those of the MobileNet-V2 head (f8_stem.hip, stem_rows_kernel<KIND, true>): 8 compute waves + 4 loader
// waves, a double-buffered patch of the raw input, persistent bands of 14 output rows, strips of 28 columns, XCD-aware band order; the
// head conv is two MFMAs per conv row, the depthwise nine diagonal-fragment MFMAs over three sliding conv rows (DPP lane shifts make the
// horizontal taps), and a requantised row becomes the next MFMA's B operand through quant_row + v_permlane32_swap.  Nothing but the input
// patch is in LDS.  The skeleton is a COPY, not a shared header: the measured instances of stem_rows_kernel keep their code.
// New here:
//   * the 1x1 has up to two 32-channel output tiles: one weight fragment and one bias vector per tile, both multiplies read the same B operand;
//   * the 1x1 may carry a ReLU: for an unsigned 8-bit reader format the clamp's lower bound IS the ReLU, for any other format the
//     accumulators are floored at 0 in front of the requantisation;
//   * outputs are NHWC int8 with the tensor's own channel stride Cs = 32 NT: a lane stores 16 bytes per output tile and reader format.
// Arithmetic: conv_igemm_kernel + dwconv3x3 + conv_igemm_kernel, bit for bit.
#include "f8_device.h"
#include <cstdlib>

namespace f8 {

typedef int v2i __attribute__((ext_vector_type(2)));

namespace {
// rint(x * scale) clamped (fix_train.py:683-692 through input_kernel's quant_in)
__device__ __forceinline__ int quant_in_head(float x, float scale, int lo, int hi) {
    const float r = rintf(__fmul_rn(x, scale));      // one IEEE multiply, as quant_in (f8_kernels.hip)
    return (int)fminf(fmaxf(r, (float)lo), (float)hi);
}
constexpr int SW = 28;                              // output columns per strip (lanes 28 .. 31 of a strip only feed the depthwise taps of their neighbours)
constexpr int RBK = 14;                             // output rows per band (2 * 14 + 5 = 33 input rows)
constexpr int RB_ROWS = 35;                         // rows of a patch buffer (the geometry of f8_stem.hip's buffers)

}

// KIND: the run's raw input (0 int32, 1 fp32, 2 uint8 planes; -1: the haloed NHWC4 copy); NT: 32-channel output tiles of the 1x1
template <int KIND, int NT>
__global__ void __launch_bounds__(768) __attribute__((amdgpu_waves_per_eu(3, 3))) head_dws_kernel(const StemPoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];      // 2 x [RB_ROWS][PWB pixels][4 B] (patch column pc = input column pc - 5) | 128 biases | u8 table
    set_fp_round_nearest_even();                                    // quant_lane16 / quant_row may take the float-converter form (f8_device.h)
    const int tid = threadIdx.x;
    const int lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // 0 .. 7 compute, 8 .. 11 loaders
    const int QW = a.rW >> 2;                                       // input width / 4
    const int PWB = 4 * QW + 8, ROWB = PWB * 4, SPR = PWB / 4;      // patch row: pixels, bytes, 16-byte slots
    const int PBUF = RB_ROWS * ROWB;
    const int bands = (a.P + RBK - 1) / RBK, ntiles = a.N * bands;
    // XCD-aware order: dispatch slot d (d % 8 = the XCD of a persistent workgroup's every slot) -> band tile; the bands of one image,
    // which share input rows, run on one XCD
    auto tile_of = [&](int d) {
        const int xcd = d & 7, qq = ntiles >> 3, rr = ntiles & 7;
        return (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (d >> 3);
    };
    // loaders' unit: one 16-byte SLOT = 4 pixels of one input row.  Raw planes: slots are image-aligned (columns 4j .. 4j + 3) and land 5
    // pixels to the right in the patch (four dword stores); the patch columns left and right of the image are written once, below.
    // Haloed form: slots are patch-aligned (a plain copy).
    const int SPI = KIND < 0 ? SPR : QW;                            // slots per input row (raw: rW / 4)
    struct Band { int n, p0, rp, r0, nslot; };
    auto band_of = [&](int d) {
        const int t = tile_of(d);
        Band B;
        B.n = t / bands; B.p0 = (t - B.n * bands) * RBK;
        B.rp = (a.P - B.p0) < RBK ? (a.P - B.p0) : RBK;             // output rows of this band
        B.r0 = 2 * B.p0 - 3; B.nslot = (2 * B.rp + 5) * SPI;        // conv rows p0 - 1 .. p0 + rp: input rows 2 p0 - 3 .. 2 (p0 + rp) + 1
        return B;
    };
    constexpr int NR = KIND < 0 ? 4 : (KIND == 2 ? 3 : 12);
    constexpr int LSLOTS = 8;                           // slots per loader thread and pass, all in flight
    const __amdgpu_buffer_rsrc_t rsrc = KIND < 0 ? __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000)
        : __builtin_amdgcn_make_buffer_rsrc((void*)(KIND == 0 ? (const void*)a.xi : KIND == 1 ? (const void*)a.xf : (const void*)a.xu8), 0,
                                            (unsigned)((size_t)a.N * a.rC * a.rH * a.rW * (KIND == 2 ? 1 : 4)), 0x00020000);
    const unsigned plane = (unsigned)(a.rH * a.rW);
    unsigned bad = 0;                                    // KIND 0: an int32 input value outside the head's 8-bit format was seen
    auto slot_issue = [&](const Band& B, int sl, int (&raw)[NR], unsigned& ok) {
        const int pr = sl / SPI, j = sl - pr * SPI;
        if constexpr (KIND < 0) {
            // haloed row / column = input row / column + 5 (org = 4 on top of the conv's pad: launch_head_dws): patch slot j = haloed pixels 4j .. 4j + 3
            const int hr = B.r0 + pr + 5, wc = 4 * j;
            ok = (sl < B.nslot && hr >= 0 && hr < a.Hp && wc + 4 <= a.Wp) ? 1u : 0u;
            const v4i v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, ok ? (unsigned)((((size_t)B.n * a.Hp + hr) * a.Wp + wc) * 4) : kOOB, 0, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) raw[q] = v[q];
        } else {
            const int row = B.r0 + pr;
            ok = (sl < B.nslot && row >= 0 && row < a.rH) ? 1u : 0u;
            const unsigned e0 = (unsigned)((B.n * a.rC * a.rH + row) * a.rW + 4 * j);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned e = (ok && c < a.rC) ? e0 + (unsigned)c * plane : kOOB;
                if constexpr (KIND == 2) raw[c] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, e, 0, 0);
                else {
                    const v4i q4 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, e == kOOB ? kOOB : e * 4u, 0, 0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) raw[c * 4 + q] = q4[q];
                }
            }
        }
    };
    auto slot_commit = [&](char* buf, const Band& B, int sl, const int (&raw)[NR], unsigned ok) {
        const int pr = sl / SPI, j = sl - pr * SPI;
        v4i o;
        if constexpr (KIND < 0) {
            const int z = (int)a.xor8;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = ok ? raw[q] : z;
            if (sl < B.nslot) *(v4i*)(buf + sl * 16) = o;
        } else {
            int v[3][4];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int x;
                    if constexpr (KIND == 0) { x = raw[c * 4 + q]; bad |= (ok && c < a.rC && (unsigned)(x - a.chk_lo) > (unsigned)(a.chk_hi - a.chk_lo)) ? 1u : 0u; }
                    else if constexpr (KIND == 1) x = quant_in_head(__builtin_bit_cast(float, raw[c * 4 + q]), a.scale, a.qlo, a.qhi);
                    else x = (int)((const short*)(lds + 2 * PBUF + 512))[c * 256 + ((raw[c] >> (8 * q)) & 0xff)];
                    v[c][q] = (ok && c < a.rC) ? x : 0;         // rows outside the image: (biased) zero
                }
            if (sl < B.nslot) {
                int* const dst = (int*)(buf + pr * ROWB + (4 * j + 5) * 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) dst[q] = (int)(pack4(v[0][q], v[1][q], v[2][q], 0) ^ a.xor8);
            }
        }
    };
    // a band's rows -> `buf`, by `nthr` threads (this one is number `t`): LSLOTS slots per thread in flight
    auto load_band = [&](const Band& B, char* buf, int t, int nthr) {
        for (int s0 = t; s0 < B.nslot; s0 += LSLOTS * nthr) {
            int raw[LSLOTS][NR]; unsigned ok[LSLOTS];
#pragma unroll
            for (int u = 0; u < LSLOTS; ++u) slot_issue(B, s0 + u * nthr, raw[u], ok[u]);
#pragma unroll
            for (int u = 0; u < LSLOTS; ++u) slot_commit(buf, B, s0 + u * nthr, raw[u], ok[u]);
        }
    };
    if constexpr (KIND == 2) {   // the u8 -> head-format table: LDS (a dynamically indexed kernel argument would live in scratch)
        for (int i = tid; i < 3 * 256; i += 768) ((short*)(lds + 2 * PBUF + 512))[i] = a.lut[i];
        __syncthreads();
    }
    if constexpr (KIND >= 0) {   // patch columns outside the image (5 on the left, 3 on the right) of both buffers: biased zero, once
        const int nside = PWB - 4 * QW;                             // 8
        for (int i = tid; i < 2 * RB_ROWS * nside; i += 768) {
            const int r = i / nside, c = i - r * nside;
            *(unsigned*)(lds + r * ROWB + (c < 5 ? c : 4 * QW + c) * 4) = a.xor8;
        }
    }

    const int G = gridDim.x;
    int d = blockIdx.x;
    if (d >= ntiles) return;
    load_band(band_of(d), lds, tid, 768);                           // the first band: every wave loads
    // head | depthwise | 1x1 biases (32 per output tile)
    if (tid < 64 + 32 * NT) *(int*)(lds + 2 * PBUF + tid * 4) = tid < 32 ? a.bias[tid] : tid < 64 ? a.bd[tid - 32] : a.b1[tid - 64];
    __syncthreads();

    if (wave >= 8) {
        // =================================================== loader waves: band it + 1 -> the other patch while band it is multiplied
        for (int it = 0; d < ntiles; d += G, ++it) {
            if (d + G < ntiles) load_band(band_of(d + G), lds + ((it & 1) ^ 1) * PBUF, tid - 512, 256);
            __syncthreads();
        }
        if constexpr (KIND == 0) { if (a.err && bad) atomicOr(a.err, 1u); }
        return;
    }
    if constexpr (KIND == 0) { if (a.err && bad) atomicOr(a.err, 1u); }   // (the first band's share of the check)

    // ======================================================= compute waves: (strip of 28 columns, half-band of 7 rows)
    //   * head conv 3x3 / 2: lane l <-> conv column c0 - 1 + l; a kernel row is 16 bytes (4 pixels x 4 channels, the 4th pixel's weights are
    //     zero), two kernel rows make one 32-byte K step: TWO MFMAs per conv row; requantised and turned by the permlane swap into 16
    //     channels per lane half — the B operand of a K = 32-channel MFMA step;
    //   * depthwise 3x3: nine MFMAs with diagonal weight fragments; horizontal taps = the conv row fragment and two DPP lane shifts of it,
    //     vertical taps = the last three conv rows, sliding; its padding (conv column -1 / Q, conv row -1 / P) is the biased zero;
    //   * 1x1: its B operand is the depthwise row after the same requant + swap: ONE MFMA per output tile.
    const int strip = wave & 3, sb = wave >> 2;
    const int cq = strip * SW - 1 + l31;                         // conv column of this lane = depthwise input column
    const bool cq_in = cq >= 0 && cq < a.Qc;
    const int cqa = cq < 0 ? 0 : (cq > a.Qc ? a.Qc : cq);       // for addresses only
    const unsigned offc = (unsigned)(8 * cqa + 16);             // input column 2 cq - 1 = patch column 2 cq + 4
    const int col = strip * SW + l31;                            // output column (lanes 0 .. 27)
    const bool lane_out = l31 < SW && col < a.Q;
    const v4i wh0 = *(const v4i*)(a.w + l31 * 96 + lh * 32);                                   // kernel rows 0 | 1
    const v4i wh1 = lh == 0 ? *(const v4i*)(a.w + l31 * 96 + 64) : v4i{0, 0, 0, 0};            // kernel row 2 | nothing
    v4i wd[9];                                                   // depthwise: diagonal fragments
    {
        const bool mine = (l31 >> 4) == lh;
        const int dsel = (l31 & 15) >> 2, bsh = 8 * (l31 & 3);
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) {
            const unsigned wv = (unsigned)(unsigned char)a.wd[tp * 32 + l31];
            const int piece = mine ? (int)(wv << bsh) : 0;
            wd[tp] = v4i{dsel == 0 ? piece : 0, dsel == 1 ? piece : 0, dsel == 2 ? piece : 0, dsel == 3 ? piece : 0};
        }
    }
    v4i w1f[NT];                                                 // 1x1: [32 NT couts][32 B], one fragment per output tile
#pragma unroll
    for (int t = 0; t < NT; ++t) w1f[t] = *(const v4i*)(a.w1 + (t * 32 + l31) * 32 + lh * 16);
    const char* const bl = lds + 2 * PBUF + 16 * lh;            // head | depthwise | 1x1 biases, 32 ints each
    const float sca = requant_u8_scale(a.na), scb = requant_u8_scale(a.nb);
    const v4i zq = {(int)0x80808080u, (int)0x80808080u, (int)0x80808080u, (int)0x80808080u};
    auto bias_acc = [&](int which) {
        v16i acc;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const v4i b = *(const v4i*)(bl + which * 128 + 8 * g * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[4 * g + q] = b[q];
        }
        return acc;
    };
    const bool rqi = a.rq_int != 0;                             // option requant_float = 0: integer requantisation (wave-uniform branch)
    auto quant_row = [&](const v16i& acc, float sc, int n) {  // ReLU + right shift (1 .. 16) into unsigned 8-bit, 16 channels per lane half
        unsigned dd[4];
        if (rqi) {
#pragma unroll
            for (int g = 0; g < 4; ++g) dd[g] = requant_u8x4_sel<2>(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3], n, 0.0f) ^ 0x80808080u;
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) dd[g] = requant_u8x4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3], sc) ^ 0x80808080u;
        }
        auto s0 = __builtin_amdgcn_permlane32_swap(dd[0], dd[2], false, false);
        auto s1 = __builtin_amdgcn_permlane32_swap(dd[1], dd[3], false, false);
        return v4i{(int)s0[0], (int)s0[1], (int)s1[0], (int)s1[1]};
    };
    // the 1x1's ReLU in front of a reader format whose clamp does not start at 0 (an unsigned 8-bit format's does: nothing to do)
    bool floor1[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) floor1[k] = a.relu1 != 0 && !(a.q[k].lo == 0 && a.q[k].hi == 255);
    struct Row3 { v4i f[3]; };
    for (int it = 0; d < ntiles; d += G, ++it) {
        const Band B = band_of(d);
        const char* const patch = lds + (it & 1) * PBUF;
        const int p0 = B.p0;
        auto conv_row = [&](int cp) {                            // conv row cp -> the three horizontal tap fragments of the depthwise conv
            Row3 R;
            v4i x = zq;
            if (cp >= 0 && cp < a.Pc) {                          // wave-uniform
                const char* const r0p = patch + (2 * cp - 1 - B.r0) * ROWB + offc;
                const char* const rA = r0p + lh * ROWB, * const rB = r0p + 2 * ROWB;
                const v2i a0 = *(const v2i*)rA, a1 = *(const v2i*)(rA + 8), b0 = *(const v2i*)rB, b1 = *(const v2i*)(rB + 8);
                v16i acc = bias_acc(0);
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wh0, v4i{a0.x, a0.y, a1.x, a1.y}, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wh1, v4i{b0.x, b0.y, b1.x, b1.y}, acc, 0, 0, 0);
                x = quant_row(acc, sca, a.na);
                if (!cq_in) x = zq;
            }
            R.f[0] = x;
#pragma unroll
            for (int k = 0; k < 4; ++k) R.f[1][k] = dpp_next_lane(x[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) R.f[2][k] = dpp_next_lane(R.f[1][k]);
            return R;
        };
        const int rps = (B.rp + 1) / 2;
        const int pb = sb * rps, pe = (pb + rps) < B.rp ? (pb + rps) : B.rp;
        if (pb < pe) {
            Row3 R0 = conv_row(p0 + pb - 1), R1 = conv_row(p0 + pb);
            for (int p = pb; p < pe; ++p) {
                const int P = p0 + p;
                const Row3 R2 = conv_row(P + 1);
                v16i acc = bias_acc(1);
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wd[kx], R0.f[kx], acc, 0, 0, 0);
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wd[3 + kx], R1.f[kx], acc, 0, 0, 0);
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wd[6 + kx], R2.f[kx], acc, 0, 0, 0);
                const v4i xb = quant_row(acc, scb, a.nb);
                v16i acc1[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) acc1[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(w1f[t], xb, bias_acc(2 + t), 0, 0, 0);
                const size_t m = ((size_t)B.n * a.P + P) * a.Q + (lane_out ? col : 0);
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int k = 0; k < 2; ++k)
                        if (a.q[k].ptr) {
                            v16i y = acc1[t];
                            if (floor1[k]) {
#pragma unroll
                                for (int q = 0; q < 16; ++q) y[q] = max(y[q], 0);
                            }
                            const v4i v = quant_lane16(y, a.q[k], !rqi);
                            if (lane_out) *(v4i*)(a.q[k].ptr + m * (32 * NT) + t * 32 + lh * 16) = v;
                        }
                R0 = R1; R1 = R2;
            }
        }
        __syncthreads();                                        // patch `it` is consumed, patch `it + 1` is complete
    }
}

// compute units of the CURRENT device, cached per device ordinal (a process may drive several GPUs)
static int head_dws_cus() {
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cus[dev]) { int v = 0; cus[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256; }
    return cus[dev];
}

// the kernel's first template argument is the kind of the run's raw input: named without arguments (as f8::stem_rows_kernel)
const char* head_dws_kernel_name() { return "f8::head_dws_kernel"; }

// instance 3 of launch_stem_pool (f8_stem.hip), which has checked a.h2 == 2
hipError_t launch_head_dws(const StemPoolArgs& a, hipStream_t s) {
    if (a.h2 != 2 || !head2_supported(a.rH, a.rW) || a.P != a.rH / 2 || a.Q != a.rW / 2 || a.Pc != a.P || a.Qc != a.Q || a.na < 1 || a.nb < 1 ||
        a.na > kRequantU8MaxShift || a.nb > kRequantU8MaxShift || (!a.acc_ok && !a.rq_int) || a.out32 || (a.Cs != 32 && a.Cs != 64) ||
        (a.relu1 != 0 && a.relu1 != 1) || a.rC < 1 || a.rC > 4 || (a.raw_kind < 0 && !(a.org == 4 && a.Wp % 4 == 0))) return hipErrorInvalidValue;
    const int lds_bytes = 2 * RB_ROWS * (a.rW + 8) * 4 + 512 + 1536;      // patches, 128 biases, the u8 table
    const int ntiles = a.N * ((a.P + RBK - 1) / RBK);
    const int gdiv = a.grid_div > 0 ? a.grid_div : 1;
    const int gmax = (head_dws_cus() / gdiv + 7) / 8 * 8;                 // a multiple of 8: tile_of's XCD arithmetic
    const int grid = ntiles < gmax ? ntiles : gmax;
#define F8_HEAD_DWS_LAUNCH(KIND) \
    do { if (a.Cs == 64) hipLaunchKernelGGL((head_dws_kernel<KIND, 2>), dim3(grid), dim3(768), lds_bytes, s, a); \
         else hipLaunchKernelGGL((head_dws_kernel<KIND, 1>), dim3(grid), dim3(768), lds_bytes, s, a); } while (0)
    switch (a.raw_kind) {
        case 0: F8_HEAD_DWS_LAUNCH(0); break;
        case 1: F8_HEAD_DWS_LAUNCH(1); break;
        case 2: F8_HEAD_DWS_LAUNCH(2); break;
        default: F8_HEAD_DWS_LAUNCH(-1); break;
    }
#undef F8_HEAD_DWS_LAUNCH
    return hipGetLastError();
}

}  // namespace f8
