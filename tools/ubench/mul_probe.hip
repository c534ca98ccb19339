// mul_probe.hip — the byte kernels of f8_mul.hip (mul_i8_kernel<BCAST, GATE, V>) launched directly on operands whose PAD bytes [C, Cs) are poisoned
// (int8 rows: no pad byte is the format's zero; the int32 gate rows of the fused instances: pad channels hold large values), every output byte
// compared — pad bytes included, which no interface of a planned net shows: a conv multiplies them by zero weights.  What this pins: the real channels
// are the exact requantised products, for both output forms of a launch; the output's pad channels hold the format's zero (0x80 per byte for the
// unsigned form, 0 for the signed one) whatever the operands' pads hold; the image index of the broadcast where a wave spans images (49 pixels an image).
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/ubench/mul_probe.hip -o tools/ubench/mul_probe.bin      (f8net_amd/csrc/build.sh does)
//   ./mul_probe.bin      -> one line per case: `mul bcast=B gate=G C=C signs=SA,SB relu=R mismatches=0 kernel=K`
// Both output forms are written in every launch: form 0 unsigned by a right shift of 7 (ties occur: the products are integers of every residue),
// form 1 signed by a right shift of 9.  tests/test_gpu_mul_probe.py runs it.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../f8net_amd/csrc/f8_internal.h"
#include "../../f8net_amd/csrc/f8_mul.hip"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

static const int HW = 49, NIMG = 3, M = HW * NIMG;          // 3 images of 7 x 7: lanes 49 .. 63 of the first wave belong to image 1
static const int GATE_FL = 10, GATE_SHIFT = 7;              // the fused gate's source fraclen; its requantisation shift into b's format
static int round32(int c) { return (c + 31) / 32 * 32; }
static unsigned hash(unsigned a, unsigned b, unsigned c) { unsigned h = a * 2654435761u ^ b * 40503u ^ c * 2246822519u; h ^= h >> 13; h *= 0x5bd1e995u; return h ^ (h >> 15); }

// int_op_only_fix_quant on one value (n > 0 here): round half to even, clamp
static int requant_host(long long v, int n, bool sgn) {
    const long long half = 1ll << (n - 1);
    long long q = (v + half) >> n;
    if (((v + half) & ((1ll << n) - 1)) == 0 && (q & 1)) q -= 1;      // an exact tie went up to an odd value: the even neighbour is below
    const long long lo = sgn ? -127 : 0, hi = sgn ? 127 : 255;
    return (int)(q < lo ? lo : q > hi ? hi : q);
}
// the value of a real channel of an operand in its format, and its stored byte
static int value(int which, int m, int c, bool sgn) { const int h = (int)(hash(which, m, c) % (sgn ? 255u : 256u)); return sgn ? h - 127 : h; }
static uint8_t stored(int v, bool sgn) { return sgn ? (uint8_t)(int8_t)v : (uint8_t)(v ^ 0x80); }
// I32T index of (pixel m, channel c) in rows of Cs channels (f8_device.h)
static size_t i32t(int m, int c, int Cs) {
    return ((size_t)(m >> 5) * (Cs >> 5) + (c >> 5)) * 1024u + (size_t)(((((c & 31) >> 3) * 64 + ((c >> 2) & 1) * 32 + (m & 31)) << 2) + (c & 3));
}

static long run(bool bcast, bool gate, int C, bool sa, bool sb, bool relu, const char** kernel) {
    const int Cs = round32(C), rowsB = bcast ? NIMG : M;
    std::vector<uint8_t> A((size_t)M * Cs), B8((size_t)rowsB * Cs), out[2];
    std::vector<int32_t> G((size_t)round32(rowsB) * Cs, 0x12345678);
    std::vector<int> bval((size_t)rowsB * C);
    for (int m = 0; m < M; ++m)
        for (int c = 0; c < Cs; ++c)
            A[(size_t)m * Cs + c] = c < C ? stored(value(1, m, c, sa), sa) : (uint8_t)(1u + hash(7, m, c) % 126u + (c & 1 ? 128u : 0u));      // pads: never 0x00 / 0x80
    for (int r = 0; r < rowsB; ++r)
        for (int c = 0; c < Cs; ++c) {
            if (gate) {
                // the gate's source: values around +-4 * 2^fl, the clamp points and the int32 extremes among them; pads poisoned
                int32_t x = (int32_t)(hash(3, r, c) % (8u << GATE_FL)) - (4 << GATE_FL);
                const unsigned pick = hash(4, r, c) % 16u;
                if (pick == 0) x = INT32_MIN; else if (pick == 1) x = INT32_MAX; else if (pick == 2) x = 3 << GATE_FL; else if (pick == 3) x = -(3 << GATE_FL);
                if (c >= C) x = 0x7f000000 + c;
                G[i32t(r, c, Cs)] = x;
                if (c < C) {
                    long long g = x < -(3 << GATE_FL) ? -(3 << GATE_FL) : x > (3 << GATE_FL) ? (3 << GATE_FL) : x;
                    bval[(size_t)r * C + c] = requant_host(g + (3 << GATE_FL), GATE_SHIFT, sb);
                }
            } else {
                if (c < C) bval[(size_t)r * C + c] = value(2, r, c, sb);
                B8[(size_t)r * Cs + c] = c < C ? stored(bval[(size_t)r * C + c], sb) : (uint8_t)(1u + hash(9, r, c) % 126u + (c & 1 ? 0u : 128u));
            }
        }
    uint8_t *dA, *dB, *dO[2];
    const size_t bbytes = gate ? G.size() * 4 : B8.size();
    HIP_OK(hipMalloc(&dA, A.size())); HIP_OK(hipMalloc(&dB, bbytes));
    HIP_OK(hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dB, gate ? (const void*)G.data() : (const void*)B8.data(), bbytes, hipMemcpyHostToDevice));
    f8::MulArgs a{};
    a.a = (const int8_t*)dA; a.b = dB; a.M = M; a.C = C; a.Cs = Cs; a.HW = HW; a.dHW = f8::fast_divisor(HW);
    a.bcast = bcast; a.gate = gate; a.relu = relu; a.lim = gate ? 3 << GATE_FL : 0;
    a.ra = f8::Requant::of(0, sa); a.rb = f8::Requant::of(gate ? GATE_SHIFT : 0, sb);
    const int shift[2] = {7, 9};
    for (int k = 0; k < 2; ++k) {
        out[k].assign((size_t)M * Cs, 0x5a);
        HIP_OK(hipMalloc(&dO[k], out[k].size()));
        HIP_OK(hipMemcpy(dO[k], out[k].data(), out[k].size(), hipMemcpyHostToDevice));
        static_cast<f8::Requant&>(a.q[k]) = f8::Requant::of(shift[k], k == 1); a.q[k].ptr = (int8_t*)dO[k];      // form 0 unsigned (stored biased), form 1 signed
    }
    const int inst = f8::mul_inst(a, 2);
    a.dVpp = f8::fast_divisor((uint32_t)(Cs / f8::mul_vector_bytes(inst)));
    *kernel = f8::mul_kernel_name(inst);
    HIP_OK(f8::launch_mul(a, inst, nullptr));
    HIP_OK(hipDeviceSynchronize());
    long bad = 0, ties = 0;
    for (int k = 0; k < 2; ++k) {
        HIP_OK(hipMemcpy(out[k].data(), dO[k], out[k].size(), hipMemcpyDeviceToHost));
        for (int m = 0; m < M; ++m)
            for (int c = 0; c < Cs; ++c) {
                uint8_t want = k == 0 ? 0x80 : 0x00;
                if (c < C) {
                    long long p = (long long)value(1, m, c, sa) * bval[(size_t)(bcast ? m / HW : m) * C + c];
                    if (relu && p < 0) p = 0;
                    ties += (p & ((1 << shift[k]) - 1)) == (1 << (shift[k] - 1));
                    want = stored(requant_host(p, shift[k], k == 1), k == 1);
                }
                bad += out[k][(size_t)m * Cs + c] != want;
            }
        HIP_OK(hipFree(dO[k]));
    }
    HIP_OK(hipFree(dA)); HIP_OK(hipFree(dB));
    if (!ties) { fprintf(stderr, "no exact tie in the data\n"); return -1; }
    return bad;
}

int main() {
    // bcast, gate, C, a signed, b signed, relu
    static const int cases[][6] = {{0, 0, 8, 0, 0, 0}, {0, 0, 20, 1, 0, 1}, {0, 0, 48, 0, 1, 0}, {0, 0, 64, 1, 1, 1}, {0, 0, 6, 1, 1, 0},
                                   {1, 0, 8, 1, 0, 0}, {1, 0, 20, 0, 0, 0}, {1, 0, 48, 1, 1, 1}, {1, 0, 64, 0, 1, 0},
                                   {1, 1, 8, 0, 0, 0}, {1, 1, 20, 1, 0, 1}, {1, 1, 48, 1, 0, 0}, {1, 1, 64, 0, 1, 0}};
    long total = 0;
    for (auto& c : cases) {
        const char* kernel = "";
        const long bad = run(c[0], c[1], c[2], c[3], c[4], c[5], &kernel);
        printf("mul bcast=%d gate=%d C=%d signs=%d,%d relu=%d mismatches=%ld kernel=%s\n", c[0], c[1], c[2], c[3], c[4], c[5], bad, kernel);
        total += bad != 0;
    }
    return total ? 1 : 0;
}
