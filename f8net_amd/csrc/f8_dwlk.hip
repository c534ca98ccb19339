// f8_dwlk.hip — large depthwise convolution (gfx950): square kernels 8 .. 31 at stride 1, int8 forms only, on v_mfma_i32_32x32x32_i8 (option dw_large = 1;
// instances 4 / 5 of launch_dwk, f8_dwk.hip: an output tile of one / two int8 forms.  Stride 2, an int32 form and dw_large = 2 run dwconvk_kernel.
//
// One GEMM per channel c and kernel row r:  out[p][q] += sum_s w[r][s] x[p + r - pad][q + s - pad]
//   M = 32 output columns q of one column tile, N = 32 output rows p (maps of <= 16 rows: the rows of 2 images stacked, RS = 16 rows each),
//   K = 32 input columns.  The A operand is the banded Toeplitz matrix of the channel's weight row: A_j[m][kk] = w[r][32 j + kk - m] (0 outside 0 .. k - 1).  The
//   band of 32 outputs spans 31 + k <= 62 input columns = TWO K chunks j = 0, 1, and A_j depends on chunk - tile only: two fragments per (c, r) serve
//   every column tile and every row of the workgroup's tile.  A lane (m, half) holds A_j[m][16 half .. + 15] = 16 consecutive bytes of the zero-extended weight
//   row Z (Z[31 + s] = w[r][s]) from t0 = 31 + 32 j + 16 half - m on.  pack_dwlk_weights stores Z in four byte-shifted copies ([Cs][k rows][4][DWLK_ROWB]
//   bytes), so the 16 bytes are four ALIGNED dwords of copy t0 & 3; A_1 is the same window 32 bytes on.  They are read from global memory, one row ahead of the
//   multiplies: a workgroup's channels' images (16 channels x 31 rows x 384 B = 186 KB at k = 31) do not fit in LDS beside the tile, every lane reads each
//   byte once per workgroup, and the 384 bytes of a (c, r) are read by one wave in one go — an LDS stage would only add a copy.
//   The B operand, lane (n, half): 16 consecutive input columns of ONE channel in input row n + r: one 16-byte LDS read from the channel-planar tile
//   [channel][row][column] (pitch 32 (TC + 1) + 16: an odd number of 16-byte units).  Chunk ct + j of the tile is B for column tile ct (j = 0) and ct - 1
//   (j = 1): TC + 1 reads feed 2 TC multiplies.
// Staging: the haloed tile (G image slots x IR = RS + k - 1 rows x 32 (TC + 1) columns x CG channels) is read as dwords of 4 channels, 4 adjacent columns per
//   thread, byte-transposed with the 8 v_perm_b32 of dwconvk_dot4_kernel and written as one dword per channel plane.  Out-of-image positions (and image slots
//   beyond N) are the biased zero, 128 * sum(w) sits in the bias (pack_dwk_weights' bias4).
// Output: D register i of lane (n, half) = column 8 (i / 4) + 4 half + i % 4 of row n.  Requantised in registers (requant1, ReLU floor, up to two forms),
//   bytes dropped into an LDS tile [form][row][column][CG] (row pitch + 16 bytes: the 32 rows of a byte store spread over the banks) and stored as 16-byte channel rows.
// Work split: a workgroup (4 waves) = CG channels (32 or 16: dwlk_geom) x 32 output rows (one row tile, or G stacked images) x TC <= 2 column tiles; wave w
//   walks channels w, w + 4, ..; its 2 TC accumulator tiles stay in registers over the k rows.
#include "f8_device.h"
#include <algorithm>

namespace f8 {

// The launch geometry of a DwArgs (k 8 .. 31, stride 1): false when no tile fits.  Prefers the LDS footprint that lets two workgroups share a CU.
bool dwlk_geom(const DwArgs& d, int nq, DwlkArgs* g) {
    DwlkArgs a{};
    a.x = d.x; a.w = d.w4; a.bias = d.bias4;
    a.N = d.N; a.H = d.H; a.W = d.W; a.P = d.P; a.Q = d.Q; a.Cs = d.Cs; a.k = d.k; a.pad = d.pad; a.in_signed = d.in_signed; a.relu0 = d.relu0;
    a.q[0] = d.q[0]; a.q[1] = d.q[1];
    a.RS = d.P <= 16 ? 16 : 32;
    a.G = 32 / a.RS;
    a.IR = a.RS + d.k - 1;
    a.tiles_r = a.G > 1 ? 1 : (d.P + 31) / 32;
    const int tc_max = d.Q > 32 ? 2 : 1;
    static const int budget[2] = {80 * 1024, 160 * 1024};
    for (int b = 0; b < 2; ++b)
        for (int cg = 32; cg >= 16; cg >>= 1)
            for (int tc = tc_max; tc >= 1; --tc) {
                const int pitch = 32 * (tc + 1) + 16;
                const size_t in = (size_t)cg * a.G * a.IR * pitch, out = (size_t)std::max(nq, 1) * 32 * (32 * tc * cg + 16);
                if (in + out > (size_t)budget[b]) continue;
                a.CG = cg; a.TC = tc; a.pitch = pitch; a.lds_in = (int32_t)in; a.opitch = 32 * tc * cg + 16; a.lds_out = 32 * a.opitch;
                a.tiles_c = (d.Q + 32 * tc - 1) / (32 * tc);
                *g = a;
                return true;
            }
    return false;
}

// Where option dw_large = 1 plans this kernel (profiles/dwlk_r22.md, batch 128, against dwconvk_kernel on the same graph): 2.3 .. 17.6 times faster on every
// measured map of 14 x 14 and more (k 9 .. 31), 0.76 times on RepLKNet's 13 x 13 over 7 x 7, where 7 of the 32 columns of an M tile are output.  So: output
// maps of more than 8 rows and columns; smaller ones keep the generic kernel (maps of 9 .. 13 were not measured and fall on this side with 14).
bool dwlk_rule(const DwArgs& d, int nq) { DwlkArgs g; return d.P > 8 && d.Q > 8 && dwlk_geom(d, nq, &g); }

template <int TC>
__global__ void __launch_bounds__(256) dwlk_kernel(const DwlkArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int WCOL = 32 * (TC + 1), TW = 32 * TC;      // staged input columns / output columns of the tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned b = blockIdx.x;
    const int ncg = a.Cs / a.CG;
    const int cgi = (int)(b % ncg); b /= ncg;
    const int tcol = (int)(b % a.tiles_c); b /= a.tiles_c;
    const int trow = (int)(b % a.tiles_r);
    const int n0 = (int)(b / a.tiles_r) * a.G;             // first image of the group
    const int c0 = cgi * a.CG, q0 = tcol * TW, p0 = trow * 32;
    const int ROWS = a.G * a.IR;
    const int rs_sh = a.RS == 32 ? 5 : 4;
    char* const otile = lds + a.lds_in;

    // ---- stage the haloed tile, channel-planar
    {
        const unsigned padv = a.in_signed ? 0u : 0x80808080u;
        const int cqs = a.CG >> 2;
        const int items = cqs * (WCOL / 4) * ROWS;
        for (int idx = tid; idx < items; idx += 256) {
            const int cq = idx % cqs;
            int t = idx / cqs;
            const int u4 = t % (WCOL / 4);
            const int row = t / (WCOL / 4);
            const int slot = row / a.IR, ir = row - slot * a.IR;
            const int img = n0 + slot, h = p0 - a.pad + ir, w0 = q0 - a.pad + 4 * u4;
            const bool rok = img < a.N && (unsigned)h < (unsigned)a.H;
            const int8_t* const xr = a.x + (((size_t)img * a.H + h) * a.W) * a.Cs + c0 + 4 * cq;
            unsigned v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = padv;
                if (rok && (unsigned)(w0 + j) < (unsigned)a.W) v[j] = *(const unsigned*)(xr + (ptrdiff_t)(w0 + j) * a.Cs);
            }
            const unsigned lo01 = __builtin_amdgcn_perm(v[1], v[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(v[1], v[0], 0x07030602u);
            const unsigned lo23 = __builtin_amdgcn_perm(v[3], v[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(v[3], v[2], 0x07030602u);
            char* const dst = lds + ((size_t)(4 * cq) * ROWS + row) * a.pitch + 4 * u4;
            const size_t plane = (size_t)ROWS * a.pitch;
            *(unsigned*)(dst) = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
            *(unsigned*)(dst + plane) = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
            *(unsigned*)(dst + 2 * plane) = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
            *(unsigned*)(dst + 3 * plane) = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
        }
    }
    __syncthreads();

    // ---- a wave walks its channels
    {
        const int n = lane & 31, half = lane >> 5;
        const int t0 = 31 + 16 * half - n, ph = t0 & 3;    // (the A fragment's row m is this lane's n)
        const int brow = (n >> rs_sh) * a.IR + (n & (a.RS - 1));
        const int floor0 = a.relu0 ? 0 : INT32_MIN;
        for (int cl = wave; cl < a.CG; cl += 4) {
            const int c = c0 + cl;
            const unsigned* wp = (const unsigned*)(a.w + ((size_t)c * a.k * 4 + ph) * DWLK_ROWB + (t0 - ph));
            const char* bp = lds + ((size_t)cl * ROWS + brow) * a.pitch + 16 * half;
            v16i acc[TC];
            {
                const int bv = a.bias[c];
#pragma unroll
                for (int ct = 0; ct < TC; ++ct)
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[ct][i] = bv;
            }
            v4i a0 = {(int)wp[0], (int)wp[1], (int)wp[2], (int)wp[3]}, a1 = {(int)wp[8], (int)wp[9], (int)wp[10], (int)wp[11]};
            for (int r = 0; r < a.k; ++r) {
                const v4i c0f = a0, c1f = a1;
                if (r + 1 < a.k) {                        // the next row's fragments, under this row's multiplies
                    wp += DWLK_ROWB;                      // (4 copies of DWLK_ROWB bytes = DWLK_ROWB dwords)
                    a0 = v4i{(int)wp[0], (int)wp[1], (int)wp[2], (int)wp[3]}; a1 = v4i{(int)wp[8], (int)wp[9], (int)wp[10], (int)wp[11]};
                }
                v4i xb[TC + 1];
#pragma unroll
                for (int j = 0; j <= TC; ++j) xb[j] = *(const v4i*)(bp + 32 * j);
                bp += a.pitch;
#pragma unroll
                for (int ct = 0; ct < TC; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(c0f, xb[ct], acc[ct], 0, 0, 0);
#pragma unroll
                for (int ct = 0; ct < TC; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(c1f, xb[ct + 1], acc[ct], 0, 0, 0);
            }
            // epilogue: register i = output column 8 (i / 4) + 4 half + i % 4 of row n
#pragma unroll
            for (int ct = 0; ct < TC; ++ct)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int y0 = max(acc[ct][4 * g], floor0), y1 = max(acc[ct][4 * g + 1], floor0);
                    const int y2 = max(acc[ct][4 * g + 2], floor0), y3 = max(acc[ct][4 * g + 3], floor0);
                    char* const o = otile + (size_t)n * a.opitch + (size_t)(32 * ct + 8 * g + 4 * half) * a.CG + cl;
#pragma unroll
                    for (int f = 0; f < 2; ++f) {
                        if (!a.q[f].ptr) continue;
                        const unsigned d = requant_pack4(y0, y1, y2, y3, a.q[f]);
                        char* const of = o + (size_t)f * a.lds_out;
                        of[0] = (char)d; of[a.CG] = (char)(d >> 8); of[2 * a.CG] = (char)(d >> 16); of[3 * a.CG] = (char)(d >> 24);
                    }
                }
        }
    }
    __syncthreads();

    // ---- store the tile: 16-byte channel rows
    {
        const int us = a.CG >> 4;
        const int items = 32 * TW * us;
        for (int idx = tid; idx < items; idx += 256) {
            const int u = idx % us, pix = idx / us;
            const int m = pix % TW, n = pix / TW;
            const int img = n0 + (n >> rs_sh), p = p0 + (n & (a.RS - 1)), q = q0 + m;
            if (img >= a.N || p >= a.P || q >= a.Q) continue;
            const size_t o = ((((size_t)img * a.P + p) * a.Q + q)) * a.Cs + c0 + 16 * u;
#pragma unroll
            for (int f = 0; f < 2; ++f)
                if (a.q[f].ptr) *(v4i*)(a.q[f].ptr + o) = *(const v4i*)(otile + (size_t)f * a.lds_out + (size_t)n * a.opitch + (size_t)m * a.CG + 16 * u);
        }
    }
}

int dwlk_kernel_name(char* buf, size_t cap, const DwArgs& a, int nq) {
    DwlkArgs g;
    return snprintf(buf, cap, "f8::dwlk_kernel<%d>", dwlk_geom(a, nq, &g) ? g.TC : 0);
}

hipError_t launch_dwlk(const DwArgs& d, int nq, hipStream_t s) {
    if (d.out32 || !d.w4 || d.stride != 1 || d.dil != 1 || d.k != d.kw || d.k < 8 || d.k > 31 || d.pad != d.pad_w || d.pad < 0 || d.pad > d.k / 2) return hipErrorInvalidValue;
    DwlkArgs a;
    if ((d.q[0].ptr ? 1 : 0) + (d.q[1].ptr ? 1 : 0) > nq || !dwlk_geom(d, nq, &a)) return hipErrorInvalidValue;
    const size_t groups = ((size_t)d.N + a.G - 1) / a.G;
    const size_t grid = groups * a.tiles_r * a.tiles_c * (a.Cs / a.CG);
    if (grid == 0 || grid > 0x7fffffffu) return hipErrorInvalidValue;
    const int ldsb = a.lds_in + std::max(nq, 1) * a.lds_out;
    const void* fn = a.TC == 2 ? (const void*)dwlk_kernel<2> : (const void*)dwlk_kernel<1>;
    if (ldsb > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, ldsb);
        if (e != hipSuccess) return e;
    }
    if (a.TC == 2) hipLaunchKernelGGL(dwlk_kernel<2>, dim3((unsigned)grid), dim3(256), ldsb, s, a);
    else hipLaunchKernelGGL(dwlk_kernel<1>, dim3((unsigned)grid), dim3(256), ldsb, s, a);
    return hipGetLastError();
}

}  // namespace f8
