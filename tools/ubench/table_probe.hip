// table_probe.hip — the byte kernels of f8_table.hip (table_i8_kernel<V, R>, table_chmul_i8_kernel<V>) launched directly on sources whose PAD bytes
// [C, Cs) are poisoned, every output byte compared — pad bytes included, which no interface of a planned net shows: a conv multiplies them by zero
// weights.  What this pins: a real channel's byte is bt[stored source byte ^ 0x80] for both output forms of a launch and for every replica count R;
// the output's pad channels hold the format's zero (0x80 per byte for the unsigned form, 0 for the signed one) whatever the source's pads hold —
// bt[index of a pad byte] is never that zero here; the image index of the fused broadcast where a wave spans images (49 pixels an image).
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/ubench/table_probe.hip -o tools/ubench/table_probe.bin      (f8net_amd/csrc/build.sh does)
//   ./table_probe.bin          -> one line per case: `table V=V R=R C=C mismatches=0` / `table+chmul V=V C=C signs=SA,SB mismatches=0`
//   ./table_probe.bin bench N  -> the replica measurement of tools/ab_table.py: per EfficientNet-B0 activation shape at batch N and per R in 1, 4, 16 the
//                                 median time of table_i8_kernel<V, R> over 20 launches (HIP events), one output form, a random source
// tests/test_gpu_table_probe.py runs the first form.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../f8net_amd/csrc/f8_internal.h"
#include "../../f8net_amd/csrc/f8_table.hip"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

static const int HW = 49, NIMG = 3, M = HW * NIMG;          // 3 images of 7 x 7: lanes 49 .. 63 of the first wave belong to image 1
static int round32(int c) { return (c + 31) / 32 * 32; }
static unsigned hash(unsigned a, unsigned b, unsigned c) { unsigned h = a * 2654435761u ^ b * 40503u ^ c * 2246822519u; h ^= h >> 13; h *= 0x5bd1e995u; return h ^ (h >> 15); }

template <class T> static T* to_device(const std::vector<T>& v) {
    T* d = nullptr;
    HIP_OK(hipMalloc((void**)&d, v.size() * sizeof(T)));
    HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
// a byte table none of whose entries is the zero byte of its form (0x80 unsigned, 0x00 signed): a pad left as bt[.] cannot pass for a zero
static std::vector<uint8_t> byte_table(int which, bool sgn) {
    std::vector<uint8_t> t(256);
    for (int u = 0; u < 256; ++u) { uint8_t b = (uint8_t)hash(which, u, 11); if (b == (sgn ? 0x00 : 0x80)) b = 0x33; t[u] = b; }
    return t;
}
// a source of M (or rows) x Cs stored bytes: real channels any byte but 0x80 ^ 0x80 = index 0 of a signed format is avoided nowhere on purpose — the
// kernel must not care —, pads poisoned with bytes whose table entries are non-zero
static std::vector<uint8_t> source(int which, int rows, int C, int Cs) {
    std::vector<uint8_t> s((size_t)rows * Cs);
    for (int m = 0; m < rows; ++m)
        for (int c = 0; c < Cs; ++c) s[(size_t)m * Cs + c] = (uint8_t)hash(which, m, c);
    return s;
}

template <int V, int R>
static long run_table(int C) {
    const int Cs = round32(C);
    const std::vector<uint8_t> src = source(1, M, C, Cs), bt0 = byte_table(2, false), bt1 = byte_table(3, true);
    uint8_t* d_src = to_device(src); uint8_t* d_bt0 = to_device(bt0); uint8_t* d_bt1 = to_device(bt1);
    uint8_t* d_out[2];
    for (int k = 0; k < 2; ++k) { HIP_OK(hipMalloc((void**)&d_out[k], (size_t)M * Cs)); HIP_OK(hipMemset(d_out[k], 0x5a, (size_t)M * Cs)); }
    f8::TableArgs a{};
    a.src = (const int8_t*)d_src; a.M = M; a.C = C; a.Cs = Cs; a.dVpp = f8::fast_divisor((uint32_t)(Cs / V));
    a.bt[0] = d_bt0; a.bt[1] = d_bt1;
    static_cast<f8::Requant&>(a.q[0]) = f8::Requant::of(7, false); a.q[0].ptr = (int8_t*)d_out[0];
    static_cast<f8::Requant&>(a.q[1]) = f8::Requant::of(9, true); a.q[1].ptr = (int8_t*)d_out[1];
    hipLaunchKernelGGL((f8::table_i8_kernel<V, R>), dim3(3), dim3(256), 0, 0, a);      // 3 workgroups: the grid-stride loop runs more than once
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    long bad = 0;
    for (int k = 0; k < 2; ++k) {
        std::vector<uint8_t> out((size_t)M * Cs);
        HIP_OK(hipMemcpy(out.data(), d_out[k], out.size(), hipMemcpyDeviceToHost));
        const std::vector<uint8_t>& bt = k ? bt1 : bt0;
        for (int m = 0; m < M; ++m)
            for (int c = 0; c < Cs; ++c) {
                const uint8_t want = c < C ? bt[src[(size_t)m * Cs + c] ^ 0x80] : (k ? 0x00 : 0x80);
                bad += out[(size_t)m * Cs + c] != want;
            }
        HIP_OK(hipFree(d_out[k]));
    }
    HIP_OK(hipFree(d_src)); HIP_OK(hipFree(d_bt0)); HIP_OK(hipFree(d_bt1));
    printf("table V=%d R=%d C=%d mismatches=%ld\n", V, R, C, bad);
    return bad;
}

// int_op_only_fix_quant on one value (n > 0 here): round half to even, clamp
static int requant_ref(long long v, int n, bool sgn) {
    const long long half = 1ll << (n - 1);
    long long q = (v + half) >> n;
    if (((v + half) & ((1ll << n) - 1)) == 0 && (q & 1)) q -= 1;
    const long long lo = sgn ? -127 : 0, hi = sgn ? 127 : 255;
    return (int)(q < lo ? lo : q > hi ? hi : q);
}

template <int V>
static long run_chmul(int C, bool sa, bool sb) {
    const int Cs = round32(C);
    const std::vector<uint8_t> A = source(5, M, C, Cs), G = source(6, NIMG, C, Cs);
    std::vector<uint8_t> bt = byte_table(7, sb);
    if (sb) for (auto& b : bt) if (b == 0x80) b = 0x81;      // -128 is no value of a signed format
    uint8_t* d_a = to_device(A); uint8_t* d_g = to_device(G); uint8_t* d_bt = to_device(bt);
    uint8_t* d_out[2];
    for (int k = 0; k < 2; ++k) { HIP_OK(hipMalloc((void**)&d_out[k], (size_t)M * Cs)); HIP_OK(hipMemset(d_out[k], 0x5a, (size_t)M * Cs)); }
    f8::TableMulArgs ta{};
    f8::MulArgs& a = ta.m;
    a.a = (const int8_t*)d_a; a.b = d_g; a.M = M; a.C = C; a.Cs = Cs; a.HW = HW; a.dHW = f8::fast_divisor(HW); a.dVpp = f8::fast_divisor((uint32_t)(Cs / V));
    a.bcast = 1; a.ra = f8::Requant::of(0, sa); a.rb = f8::Requant::of(0, sb);
    ta.bt = d_bt;
    const int n[2] = {7, 9}; const bool sg[2] = {false, true};
    for (int k = 0; k < 2; ++k) { static_cast<f8::Requant&>(a.q[k]) = f8::Requant::of(n[k], sg[k]); a.q[k].ptr = (int8_t*)d_out[k]; }
    hipLaunchKernelGGL((f8::table_chmul_i8_kernel<V>), dim3(3), dim3(256), 0, 0, ta);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    auto val = [](uint8_t s, bool sgn) { return sgn ? (int)(int8_t)s : (int)(s ^ 0x80); };
    long bad = 0;
    for (int k = 0; k < 2; ++k) {
        std::vector<uint8_t> out((size_t)M * Cs);
        HIP_OK(hipMemcpy(out.data(), d_out[k], out.size(), hipMemcpyDeviceToHost));
        for (int m = 0; m < M; ++m)
            for (int c = 0; c < Cs; ++c) {
                uint8_t want = sg[k] ? 0x00 : 0x80;
                if (c < C) {
                    // (a signed a holding the byte 0x80 reads as u - 128 = -128 in the kernel and here alike)
                    const int av = sa ? (int)(A[(size_t)m * Cs + c] ^ 0x80) - 128 : (int)(A[(size_t)m * Cs + c] ^ 0x80);
                    const int bv = val(bt[G[(size_t)(m / HW) * Cs + c] ^ 0x80], sb);
                    const int q = requant_ref((long long)av * bv, n[k], sg[k]);
                    want = sg[k] ? (uint8_t)(int8_t)q : (uint8_t)(q ^ 0x80);
                }
                bad += out[(size_t)m * Cs + c] != want;
            }
        HIP_OK(hipFree(d_out[k]));
    }
    HIP_OK(hipFree(d_a)); HIP_OK(hipFree(d_g)); HIP_OK(hipFree(d_bt));
    printf("table+chmul V=%d C=%d signs=%d,%d mismatches=%ld\n", V, C, (int)sa, (int)sb, bad);
    return bad;
}

template <int V, int R>
static float time_table(const f8::TableArgs& a0, int reps) {
    f8::TableArgs a = a0;
    a.dVpp = f8::fast_divisor((uint32_t)(a.Cs / V));
    const size_t work = (size_t)a.M * (a.Cs / V);
    const dim3 grid((unsigned)std::min<size_t>((work + 255) / 256, 8192));
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int r = 0; r < reps + 2; ++r) {
        HIP_OK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL((f8::table_i8_kernel<V, R>), grid, dim3(256), 0, 0, a);
        HIP_OK(hipEventRecord(e1, 0));
        HIP_OK(hipEventSynchronize(e1));
        float t; HIP_OK(hipEventElapsedTime(&t, e0, e1));
        if (r >= 2) ms.push_back(t);
    }
    HIP_OK(hipEventDestroy(e0)); HIP_OK(hipEventDestroy(e1));
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2] * 1e3f;
}

static int bench(int N) {
    static const int shapes[][2] = {{32, 112}, {96, 112}, {144, 56}, {240, 28}, {480, 14}, {672, 14}, {1152, 7}};
    printf("| channels @ map | V | MB read + written | R = 1 us | R = 4 us | R = 16 us |\n|---|---:|---:|---:|---:|---:|\n");
    for (auto& s : shapes) {
        const int C = s[0], Cs = round32(C), Mx = N * s[1] * s[1];
        const size_t bytes = (size_t)Mx * Cs;
        std::vector<uint8_t> src(bytes);
        for (size_t i = 0; i < bytes; ++i) src[i] = (uint8_t)hash(9, (unsigned)i, (unsigned)(i >> 32));
        uint8_t* d_src = to_device(src); uint8_t* d_bt = to_device(byte_table(2, false)); uint8_t* d_out;
        HIP_OK(hipMalloc((void**)&d_out, bytes));
        f8::TableArgs a{};
        a.src = (const int8_t*)d_src; a.M = Mx; a.C = C; a.Cs = Cs; a.bt[0] = d_bt;
        static_cast<f8::Requant&>(a.q[0]) = f8::Requant::of(7, false); a.q[0].ptr = (int8_t*)d_out;
        float t[3];
        if (C % 16 == 0) { t[0] = time_table<16, 1>(a, 20); t[1] = time_table<16, 4>(a, 20); t[2] = time_table<16, 16>(a, 20); }
        else { t[0] = time_table<4, 1>(a, 20); t[1] = time_table<4, 4>(a, 20); t[2] = time_table<4, 16>(a, 20); }
        printf("| %d @ %d x %d | %d | %.1f | %.1f | %.1f | %.1f |\n", C, s[1], s[1], C % 16 ? 4 : 16, 2.0 * bytes / 1e6, t[0], t[1], t[2]);
        fflush(stdout);
        HIP_OK(hipFree(d_src)); HIP_OK(hipFree(d_bt)); HIP_OK(hipFree(d_out));
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "bench")) return bench(argc >= 3 ? atoi(argv[2]) : 128);
    long bad = 0;
    bad += run_table<16, 1>(64); bad += run_table<16, 4>(48); bad += run_table<16, 16>(16);
    bad += run_table<4, 1>(20); bad += run_table<4, 4>(8); bad += run_table<4, 16>(61); bad += run_table<4, 1>(64);
    bad += run_chmul<16>(64, false, false); bad += run_chmul<16>(48, true, true);
    bad += run_chmul<4>(20, true, false); bad += run_chmul<4>(8, false, true); bad += run_chmul<4>(61, false, false);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
