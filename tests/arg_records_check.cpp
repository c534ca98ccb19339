// Stand-alone check of the two argument records of f8_internal.h (tests/test_arg_records.py builds it with the host side under ASan + UBSan and runs it):
// fast_divisor against n / d by the documented formula, Requant::of's two triples, and the one fast-instance rule over every shift and both signs.
#include "../f8net_amd/csrc/f8_internal.h"
#include <stdio.h>

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;          // splitmix64, fixed seed
static uint64_t rng() {
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// q = (t + ((n - t) >> s1)) >> s2, t = high32(n * m), in the device's 32-bit unsigned arithmetic (fast_div, f8_device.h)
static uint32_t div_by(uint32_t n, const f8::FastDiv& d) {
    const uint32_t t = (uint32_t)(((uint64_t)n * d.m) >> 32);
    return (t + ((n - t) >> d.s1)) >> d.s2;
}

static long bad = 0;
static void check_div(uint32_t n, uint32_t d, const f8::FastDiv& f) {
    if (div_by(n, f) != n / d && bad++ < 10) printf("fast_divisor(%u): %u / d = %u, want %u\n", d, n, div_by(n, f), n / d);
}

int main() {
    const uint32_t divisors[] = {1, 2, 3, 5, 7, 14, 28, 49, 56, 112, 196, 784, 3136, 12544, 50176, 65535, 65536, 65537, 2147483647u};
    long checked = 0;
    for (uint32_t d : divisors) {
        const f8::FastDiv f = f8::fast_divisor(d);
        if (f.s1 < 0 || f.s1 > 1 || f.s2 < 0 || f.s2 > 31) { printf("fast_divisor(%u): shifts %d, %d\n", d, f.s1, f.s2); ++bad; continue; }
        const uint32_t fixed[] = {0, 1, d - 1, d, d + 1, 2147483647u, 2147483648u, 4294967295u};
        for (uint32_t n : fixed) check_div(n, d, f);
        const uint32_t kmax = 4294967295u / d;                  // k * d fits 32 bits
        for (int i = 0; i < 64; ++i) {
            const uint32_t k = 1 + (uint32_t)(rng() % kmax);
            check_div(k * d - 1, d, f); check_div(k * d, d, f);
        }
        for (int i = 0; i < 100000; ++i) check_div((uint32_t)rng(), d, f);
        checked += 8 + 128 + 100000;
    }
    for (int sgn = 0; sgn < 2; ++sgn)
        for (int n = -31; n <= 31; ++n) {
            const f8::Requant r = f8::Requant::of(n, sgn != 0);
            const bool triple = sgn ? (r.lo == -127 && r.hi == 127 && r.bias_xor == 0u) : (r.lo == 0 && r.hi == 255 && r.bias_xor == 0x80808080u);
            const bool shr = !sgn && n >= 1 && n <= 30;
            if (r.n != n || !triple || r.u8_shr() != shr || r.u8_float() != (shr && n <= 16)) {
                printf("Requant::of(%d, %d): n %d lo %d hi %d xor %08x u8_shr %d u8_float %d\n", n, sgn, r.n, r.lo, r.hi, r.bias_xor, (int)r.u8_shr(), (int)r.u8_float());
                ++bad;
            }
        }
    f8::QuantOut q{};                                           // a QuantOut is a Requant with a pointer: same member names, same rule
    static_cast<f8::Requant&>(q) = f8::Requant::of(8, false);
    if (!q.u8_float() || q.ptr != nullptr || f8::kRequantU8MaxShift != 16) { printf("QuantOut\n"); ++bad; }
    printf("%ld divisions checked, %ld bad\n%s\n", checked, bad, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
