// pixmap_probe.hip — the byte-mode kernels of f8_pixmap.hip (pixmap_run_i8_kernel, pixmap_crd2_i8_kernel, pixmap_i8_general_kernel) launched directly on
// sources whose PAD bytes [C, Cs) are poisoned (no byte of a source row is the format's zero), into destinations with a guard region in front of and
// behind them; every output byte is compared — pad bytes included, which no interface of a planned net shows: a conv multiplies them by zero weights
// — and the guards must be untouched.  What this pins: a source's pad bytes never reach the output, the output's pad channels hold the format's zero
// (0x80 per byte for unsigned forms, 0 for signed ones), and no launch writes outside its tensor.  Every launch is in bounds by construction:
// launch_pixmap validates the shapes, and the buffers have exactly the sizes it assumes.
//
//   hipcc --offload-arch=gfx950 -O2 tools/ubench/pixmap_probe.hip -o tools/ubench/pixmap_probe.bin      (f8net_amd/csrc/build.sh does)
//   ./pixmap_probe.bin           -> per (op, order, r, C) one line for the planned instance and, where that is a specialised one, one for the general
//                                   kernel: `d2s order=crd r=2 C=16 kernel=K mismatches=0 guard=0`            (tests/test_gpu_pixmap_probe.py runs it)
//   ./pixmap_probe.bin --bench   -> the measurement of tools/ab_pixmap.py: per shape the planned instance, the general byte kernel, the int32 mode and a
//                                   device-to-device copy of the output's bytes, interleaved, microseconds per launch (median and minimum of the rounds)
// Both output forms are written in every check launch: form 0 unsigned (zero 0x80), form 1 signed (zero 0x00), each from a source of its own.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../f8net_amd/csrc/f8_internal.h"
#include "../../f8net_amd/csrc/f8_pixmap.hip"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

static int round32(int c) { return (c + 31) / 32 * 32; }
// a byte that is never 0x00 and never 0x80, different per (form, pixel, channel)
static uint8_t src_byte(int k, int m, int c) { const unsigned h = (unsigned)(k * 7919 + m * 131 + c * 31 + 17) % 126u; return (uint8_t)(1u + h + (c & 1 ? 128u : 0u)); }

// the arguments of one launch; C = the channels of the SMALL side (a depth_to_space result, a space_to_depth source), h x w its map
static f8::PixMapArgs make_args(bool s2d, bool crd, int r, int C, int N, int h, int w) {
    f8::PixMapArgs a{};
    a.N = N; a.r = r; a.s2d = s2d; a.crd = crd;
    if (s2d) { a.Csrc = C; a.Hs = h * r; a.Ws = w * r; a.C = C * r * r; a.P = h; a.Q = w; }
    else { a.Csrc = C * r * r; a.Hs = h; a.Ws = w; a.C = C; a.P = h * r; a.Q = w * r; }
    a.Cs = round32(a.C); a.Cs_src = round32(a.Csrc);
    a.dPQ = f8::fast_divisor((uint32_t)(a.P * a.Q)); a.dQ = f8::fast_divisor((uint32_t)a.Q);
    a.dHsWs = f8::fast_divisor((uint32_t)(a.Hs * a.Ws)); a.dWs = f8::fast_divisor((uint32_t)a.Ws);
    a.dR = f8::fast_divisor((uint32_t)r); a.dRR = f8::fast_divisor((uint32_t)(r * r)); a.dC = f8::fast_divisor((uint32_t)a.Csrc);
    return a;
}

// (source pixel, source channel) of output pixel (n, oh, ow), channel oc: the formulas of include/f8net.h written out
static void source_of(const f8::PixMapArgs& a, int n, int oh, int ow, int oc, int* ms, int* sc) {
    const int r = a.r;
    int hh, ww;
    if (!a.s2d) {
        const int i = oh % r, j = ow % r;
        hh = oh / r; ww = ow / r;
        *sc = a.crd ? oc * r * r + i * r + j : (i * r + j) * a.C + oc;
    } else {
        int k;
        if (a.crd) { *sc = oc / (r * r); k = oc % (r * r); } else { k = oc / a.Csrc; *sc = oc % a.Csrc; }
        hh = oh * r + k / r; ww = ow * r + k % r;
    }
    *ms = (n * a.Hs + hh) * a.Ws + ww;
}

static const size_t GUARD = 256;

static void check(bool s2d, bool crd, int r, int C, int inst_or_planned, long* total) {
    const int N = 3, h = 5, w = 3;
    f8::PixMapArgs a = make_args(s2d, crd, r, C, N, h, w);
    const int M = N * a.P * a.Q, Ms = N * a.Hs * a.Ws;
    std::vector<uint8_t> src[2], out[2];
    uint8_t *d_src[2], *d_out[2];
    for (int k = 0; k < 2; ++k) {
        src[k].resize((size_t)Ms * a.Cs_src);
        for (int m = 0; m < Ms; ++m)
            for (int c = 0; c < a.Cs_src; ++c) src[k][(size_t)m * a.Cs_src + c] = src_byte(k, m, c);      // pad channels poisoned too
        out[k].assign(GUARD + (size_t)M * a.Cs + GUARD, 0xa5);
        HIP_OK(hipMalloc(&d_src[k], src[k].size()));
        HIP_OK(hipMalloc(&d_out[k], out[k].size()));
        HIP_OK(hipMemcpy(d_src[k], src[k].data(), src[k].size(), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_out[k], out[k].data(), out[k].size(), hipMemcpyHostToDevice));
        a.src[k] = d_src[k];
        static_cast<f8::Requant&>(a.q[k]) = f8::Requant::of(0, k == 1);      // form 0 unsigned (stored biased), form 1 signed
        a.q[k].ptr = (int8_t*)d_out[k] + GUARD;
    }
    const int inst = inst_or_planned < 0 ? f8::pixmap_inst(a, true) : inst_or_planned;
    HIP_OK(f8::launch_pixmap(a, inst, nullptr));
    HIP_OK(hipDeviceSynchronize());
    long bad = 0, guard = 0;
    for (int k = 0; k < 2; ++k) {
        HIP_OK(hipMemcpy(out[k].data(), d_out[k], out[k].size(), hipMemcpyDeviceToHost));
        const uint8_t zero = k == 0 ? 0x80 : 0x00;
        for (size_t g = 0; g < GUARD; ++g) guard += (out[k][g] != 0xa5) + (out[k][GUARD + (size_t)M * a.Cs + g] != 0xa5);
        for (int n = 0; n < N; ++n)
            for (int oh = 0; oh < a.P; ++oh)
                for (int ow = 0; ow < a.Q; ++ow) {
                    const int m = (n * a.P + oh) * a.Q + ow;
                    for (int c = 0; c < a.Cs; ++c) {
                        uint8_t want = zero;
                        if (c < a.C) { int ms, sc; source_of(a, n, oh, ow, c, &ms, &sc); want = src[k][(size_t)ms * a.Cs_src + sc]; }
                        bad += out[k][GUARD + (size_t)m * a.Cs + c] != want;
                    }
                }
        HIP_OK(hipFree(d_src[k]));
        HIP_OK(hipFree(d_out[k]));
    }
    printf("%s order=%s r=%d C=%d kernel=%s mismatches=%ld guard=%ld\n", s2d ? "s2d" : "d2s", crd ? "crd" : "dcr", r, C, f8::pixmap_kernel_name(inst), bad, guard);
    *total += bad + guard;
}

// ---- --bench
struct Shape { const char* name; bool s2d, crd; int r, C, h, w, N; bool out32; };      // C, h, w: the small side; out32: the int32 mode writes the int32 form (a network output)

static void bench(const Shape& sh) {
    f8::PixMapArgs a = make_args(sh.s2d, sh.crd, sh.r, sh.C, sh.N, sh.h, sh.w);
    const size_t M = (size_t)sh.N * a.P * a.Q, Ms = (size_t)sh.N * a.Hs * a.Ws;
    const size_t out8 = M * a.Cs, src8 = Ms * a.Cs_src;
    const size_t out32 = (M + 31) / 32 * 32 * a.Cs * 4, src32 = (Ms + 31) / 32 * 32 * a.Cs_src * 4;      // I32T: rows padded to 32 pixels
    uint8_t *d_src8, *d_out8, *d_copy, *d_src32, *d_out32;
    HIP_OK(hipMalloc(&d_src8, src8)); HIP_OK(hipMalloc(&d_out8, out8)); HIP_OK(hipMalloc(&d_copy, out8));
    HIP_OK(hipMalloc(&d_src32, src32)); HIP_OK(hipMalloc(&d_out32, out32));
    std::vector<uint8_t> host(size_t(32) << 20);                     // random bytes (zero-filled tensors read fast), tiled over the sources
    unsigned x = 12345u;
    for (auto& b : host) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 24); }
    auto fill = [&](uint8_t* d, size_t n) { for (size_t o = 0; o < n; o += host.size()) HIP_OK(hipMemcpy(d + o, host.data(), std::min(host.size(), n - o), hipMemcpyHostToDevice)); };
    fill(d_src8, src8); fill(d_src32, src32); fill(d_copy, out8);
    f8::PixMapArgs a8 = a, a32 = a;
    a8.src[0] = d_src8; static_cast<f8::Requant&>(a8.q[0]) = f8::Requant::of(0, false); a8.q[0].ptr = (int8_t*)d_out8;
    a32.src[0] = d_src32;
    if (sh.out32) a32.out32 = (int32_t*)d_out32;
    else { static_cast<f8::Requant&>(a32.q[0]) = f8::Requant::of(9, false); a32.q[0].ptr = (int8_t*)d_out8; }
    const int planned = f8::pixmap_inst(a8, true);
    const int L = 100, R = 7;
    enum { COPY, PLANNED, GENERAL, I32, LEGS };
    std::vector<float> us[LEGS];
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
    auto leg = [&](int which) {
        switch (which) {
            case COPY: HIP_OK(hipMemcpyAsync(d_out8, d_copy, out8, hipMemcpyDeviceToDevice, nullptr)); break;
            case PLANNED: HIP_OK(f8::launch_pixmap(a8, planned, nullptr)); break;
            case GENERAL: HIP_OK(f8::launch_pixmap(a8, 2, nullptr)); break;
            default: HIP_OK(f8::launch_pixmap(a32, 0, nullptr)); break;
        }
    };
    for (int which = 0; which < LEGS; ++which) for (int i = 0; i < 10; ++i) leg(which);      // warm-up
    HIP_OK(hipDeviceSynchronize());
    for (int round = 0; round < R; ++round)
        for (int which = 0; which < LEGS; ++which) {                                      // the legs interleaved, L launches between two events
            HIP_OK(hipEventRecord(e0, nullptr));
            for (int i = 0; i < L; ++i) leg(which);
            HIP_OK(hipEventRecord(e1, nullptr));
            HIP_OK(hipEventSynchronize(e1));
            float ms = 0;
            HIP_OK(hipEventElapsedTime(&ms, e0, e1));
            us[which].push_back(ms * 1000.0f / L);
        }
    auto med = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    auto mn = [](const std::vector<float>& v) { return *std::min_element(v.begin(), v.end()); };
    printf("bench %s op=%s order=%s r=%d C=%d map=%dx%d N=%d out_bytes=%zu planned=%s copy_us=%.2f/%.2f planned_us=%.2f/%.2f general_us=%.2f/%.2f i32_us=%.2f/%.2f i32_writes=%s\n",
           sh.name, sh.s2d ? "s2d" : "d2s", sh.crd ? "crd" : "dcr", sh.r, sh.C, sh.h, sh.w, sh.N, out8, f8::pixmap_kernel_name(planned),
           med(us[COPY]), mn(us[COPY]), med(us[PLANNED]), mn(us[PLANNED]), med(us[GENERAL]), mn(us[GENERAL]), med(us[I32]), mn(us[I32]), sh.out32 ? "int32" : "int8");
    HIP_OK(hipEventDestroy(e0)); HIP_OK(hipEventDestroy(e1));
    HIP_OK(hipFree(d_src8)); HIP_OK(hipFree(d_out8)); HIP_OK(hipFree(d_copy)); HIP_OK(hipFree(d_src32)); HIP_OK(hipFree(d_out32));
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--bench")) {
        // (C, h, w: the small side.)  EDSR 256 @ 48^2 -> 64 @ 96^2; ESPCN 27 @ 64^2 -> 3 @ 192^2 (the int32 output); DUC 1216 @ 28^2 -> 19 @ 224^2 at batch 32;
        // TResNet 3 @ 224^2 -> 48 @ 56^2; Focus 3 @ 320^2 -> 12 @ 160^2; nn.PixelUnshuffle(2) 64 @ 56^2 -> 256 @ 28^2; and the DCR forms of the two aligned ones
        static const Shape shapes[] = {
            {"edsr", false, true, 2, 64, 48, 48, 128, false}, {"espcn", false, true, 3, 3, 64, 64, 128, true}, {"duc", false, true, 8, 19, 28, 28, 32, false},
            {"tresnet", true, false, 4, 3, 56, 56, 128, false}, {"focus", true, false, 2, 3, 160, 160, 128, false}, {"unshuffle", true, true, 2, 64, 28, 28, 128, false},
            {"edsr_dcr", false, false, 2, 64, 48, 48, 128, false}, {"unshuffle_dcr", true, false, 2, 64, 28, 28, 128, false},
        };
        for (auto& s : shapes) bench(s);
        return 0;
    }
    // (op, order, r, C of the small side): the table of tests/pixmap_cases.py
    static const int cases[][4] = {
        {0, 0, 2, 64}, {0, 1, 2, 64}, {0, 0, 2, 16}, {0, 1, 2, 16}, {0, 0, 2, 48}, {0, 1, 2, 48}, {0, 0, 2, 12}, {0, 1, 2, 12}, {0, 0, 2, 20}, {0, 1, 2, 20},
        {0, 0, 2, 3}, {0, 1, 2, 3}, {0, 0, 2, 19}, {0, 1, 2, 19}, {0, 0, 2, 40}, {0, 1, 2, 40}, {0, 1, 3, 3}, {0, 0, 3, 3}, {0, 1, 3, 8}, {0, 0, 3, 8},
        {0, 1, 4, 16}, {0, 0, 4, 16}, {0, 1, 8, 19}, {0, 0, 8, 19},
        {1, 0, 4, 3}, {1, 1, 4, 3}, {1, 0, 2, 3}, {1, 1, 2, 3}, {1, 0, 2, 16}, {1, 1, 2, 16}, {1, 0, 2, 32}, {1, 1, 2, 32}, {1, 0, 2, 12}, {1, 1, 2, 12},
        {1, 0, 2, 19}, {1, 1, 2, 19}, {1, 0, 2, 40}, {1, 1, 2, 40}, {1, 0, 3, 8}, {1, 1, 3, 8},
    };
    long total = 0;
    for (auto& c : cases) {
        check(c[0] != 0, c[1] != 0, c[2], c[3], -1, &total);
        const f8::PixMapArgs a = make_args(c[0] != 0, c[1] != 0, c[2], c[3], 3, 5, 3);
        if (f8::pixmap_inst(a, true) != 2) check(c[0] != 0, c[1] != 0, c[2], c[3], 2, &total);      // ... and the general kernel on the specialised ones' shapes
    }
    return total ? 1 : 0;
}
