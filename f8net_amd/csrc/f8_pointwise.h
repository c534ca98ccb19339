// f8_pointwise.h — what the pointwise launches on int8 operands share (f8_mul.hip, f8_table.hip): byte extraction, the four products, the output pack.
#pragma once
#include "f8_device.h"

namespace f8 {

// byte e of w as 0 .. 255
__device__ __forceinline__ int ubyte(unsigned w, int e) { return (int)__builtin_amdgcn_ubfe(w, 8u * (unsigned)e, 8u); }
// four values -> one dword in the format q, storage bias included: the integer pack-shift where the format is the fast one (Requant::u8_shr), else the general form
__device__ __forceinline__ unsigned quant4(const int (&y)[4], const QuantOut& q) {
    if (q.u8_shr()) return requant_u8x4_int(y[0], y[1], y[2], y[3], q.n) ^ q.bias_xor;
    return requant_pack4(y[0], y[1], y[2], y[3], q);
}
// four products of channels c .. c + 3: wa / wb the operand dwords already ^ 0x80808080, offa / offb 0 or 128; channels >= C give 0
__device__ __forceinline__ void products(int (&y)[4], unsigned wa, int offa, const int (&B)[4], int relu_floor, int rem) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int p = max((ubyte(wa, e) - offa) * B[e], relu_floor);
        y[e] = e < rem ? p : 0;
    }
}

}  // namespace f8
