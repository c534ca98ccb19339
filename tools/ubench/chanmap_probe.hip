// chanmap_probe.hip — the byte-mode kernels of f8_chanmap.hip (slice_i8_kernel, shuffle_i8_kernel, shuffle_i8_general_kernel) launched directly on
// sources whose PAD bytes [C, Cs) are poisoned (no byte of a source row is the format's zero), every output byte compared — pad bytes included, which
// no interface of a planned net shows: a conv multiplies them by zero weights.  What this pins: bytes past a slice's last channel and a source's own
// pad bytes never reach the output; the output's pad channels hold the format's zero (0x80 per byte for unsigned forms, 0 for signed ones).
//
//   hipcc --offload-arch=gfx950 -O2 tools/ubench/chanmap_probe.hip -o tools/ubench/chanmap_probe.bin      (f8net_amd/csrc/build.sh does)
//   ./chanmap_probe.bin      -> one line per case: `slice first=F channels=N C=C kernel=K mismatches=0`, `shuffle groups=G C=C kernel=K mismatches=0`
// Both output forms are written in every launch: form 0 unsigned (zero 0x80), form 1 signed (zero 0x00), each from a source of its own.
// tests/test_gpu_chanmap_probe.py runs it.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../f8net_amd/csrc/f8_internal.h"
#include "../../f8net_amd/csrc/f8_chanmap.hip"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

static const int M = 147;                                   // 3 images of 7 x 7
static int round32(int c) { return (c + 31) / 32 * 32; }
// a byte that is never 0x00 and never 0x80, different per (form, pixel, channel)
static uint8_t src_byte(int k, int m, int c) { const unsigned h = (unsigned)(k * 7919 + m * 131 + c * 31 + 17) % 126u; return (uint8_t)(1u + h + (c & 1 ? 128u : 0u)); }

// groups == 0: slice [first, first + channels) of C; else shuffle of C channels by groups
static long run(int groups, int first, int channels, int C, const char** kernel) {
    const int Cs_src = round32(C), Cout = groups ? C : channels, Cs = round32(Cout);
    std::vector<uint8_t> src[2], out[2];
    uint8_t *d_src[2], *d_out[2];
    for (int k = 0; k < 2; ++k) {
        src[k].resize((size_t)M * Cs_src);
        for (int m = 0; m < M; ++m)
            for (int c = 0; c < Cs_src; ++c) src[k][(size_t)m * Cs_src + c] = src_byte(k, m, c);      // pad channels poisoned too
        out[k].assign((size_t)M * Cs, 0x5a);
        HIP_OK(hipMalloc(&d_src[k], src[k].size()));
        HIP_OK(hipMalloc(&d_out[k], out[k].size()));
        HIP_OK(hipMemcpy(d_src[k], src[k].data(), src[k].size(), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_out[k], out[k].data(), out[k].size(), hipMemcpyHostToDevice));
    }
    f8::ChanMapArgs a{};
    a.groups = groups; a.K = groups ? groups : 1; a.Cg = groups ? C / groups : 0;
    a.M = M; a.C = Cout; a.Cs = Cs;
    for (int i = 0; i < a.K; ++i) {
        a.Cs_src[i] = Cs_src; a.off[i] = groups ? i * a.Cg : first;
        a.src[0][i] = d_src[0]; a.src[1][i] = d_src[1];
    }
    a.dG = f8::fast_divisor(groups ? (uint32_t)groups : 1u);
    for (int k = 0; k < 2; ++k) { static_cast<f8::Requant&>(a.q[k]) = f8::Requant::of(0, k == 1); a.q[k].ptr = (int8_t*)d_out[k]; }   // form 0 unsigned (stored biased), form 1 signed
    const int inst = f8::chanmap_inst(a, true);
    *kernel = f8::chanmap_kernel_name(inst);
    HIP_OK(f8::launch_chanmap(a, inst, nullptr));
    HIP_OK(hipDeviceSynchronize());
    long bad = 0;
    for (int k = 0; k < 2; ++k) {
        HIP_OK(hipMemcpy(out[k].data(), d_out[k], out[k].size(), hipMemcpyDeviceToHost));
        const uint8_t zero = k == 0 ? 0x80 : 0x00;
        for (int m = 0; m < M; ++m)
            for (int c = 0; c < Cs; ++c) {
                const int sc = groups ? (c % groups) * a.Cg + c / groups : first + c;
                const uint8_t want = c < Cout ? src[k][(size_t)m * Cs_src + sc] : zero;
                bad += out[k][(size_t)m * Cs + c] != want;
            }
        HIP_OK(hipFree(d_src[k]));
        HIP_OK(hipFree(d_out[k]));
    }
    return bad;
}

int main() {
    static const int slices[][3] = {{0, 58, 116}, {58, 58, 116}, {16, 32, 64}, {32, 16, 64}, {17, 30, 64}, {49, 15, 64}, {29, 29, 58}, {0, 1, 8}, {0, 17, 64}, {48, 10, 58}};
    static const int shuffles[][2] = {{2, 64}, {2, 352}, {2, 24}, {2, 232}, {2, 116}, {2, 58}, {3, 24}, {4, 16}, {4, 48}, {8, 24}, {8, 256}};
    long total = 0;
    const char* kernel = "";
    for (auto& s : slices) {
        const long bad = run(0, s[0], s[1], s[2], &kernel);
        printf("slice first=%d channels=%d C=%d kernel=%s mismatches=%ld\n", s[0], s[1], s[2], kernel, bad);
        total += bad;
    }
    for (auto& s : shuffles) {
        const long bad = run(s[0], 0, 0, s[1], &kernel);
        printf("shuffle groups=%d C=%d kernel=%s mismatches=%ld\n", s[0], s[1], kernel, bad);
        total += bad;
    }
    return total ? 1 : 0;
}
