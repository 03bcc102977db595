// Order-independent per-vertex sums of float terms (vertex normals and tangents: a scatter of per-face values onto their
// corners).  A float atomicAdd rounds after every term, so the result depends on the order in which the atomics land and
// two launches on the same mesh differ in the last bits.  Here every sum takes two passes over its terms:
//   pass 1  fx_note: the largest |term| of the sum (atomicMax on the bits of |x|, which order like the values);
//   pass 2  fx_add:  every term rounded once, to nearest, onto the grid 2^(e - FX_BITS), e = frexp exponent of that largest
//                    term, and added as a 64-bit integer: the integer sum is exact, so the order no longer matters;
//   then    fx_value: the integer sum * 2^(e - FX_BITS), rounded to double, then to float.
// |term| <= 2^e, so one rounded term is at most 2^FX_BITS in magnitude and a sum of fewer than 2^(62 - FX_BITS) = 4 M terms
// cannot overflow.  The rounding of a term is at most 2^(e - FX_BITS - 1) = 2^-41 of the largest term, far below float's 2^-24.
// A sum with a term that is not finite is NaN (its largest |term| is then >= the bits of infinity; such a term is not added).
// tests/_uvref.py restates the three steps bit for bit.
#pragma once

#include "common.h"

namespace sculpt {

constexpr int FX_BITS = 40;

__device__ __forceinline__ void fx_note(unsigned *mag, float x) {
    const unsigned b = __float_as_uint(x) & 0x7fffffffu;
    if (b) atomicMax(mag, b);
}

__device__ __forceinline__ int fx_exp(unsigned mag) {
    int e;
    (void)frexpf(__uint_as_float(mag), &e);
    return e;
}

constexpr unsigned FX_NONFINITE = 0x7f800000u;

__device__ __forceinline__ void fx_add(long long *acc, unsigned mag, float x) {
    if (x == 0.f || mag >= FX_NONFINITE) return;
    const long long q = __double2ll_rn(ldexp((double)x, FX_BITS - fx_exp(mag)));
    atomicAdd(reinterpret_cast<unsigned long long *>(acc), (unsigned long long)q);
}

__device__ __forceinline__ float fx_value(long long acc, unsigned mag) {
    if (mag >= FX_NONFINITE) return __uint_as_float(0x7fc00000u);
    return mag ? (float)ldexp((double)acc, fx_exp(mag) - FX_BITS) : 0.f;
}

// the mean of a sum of n terms: the integer sum scaled in double, divided by n in double, rounded once to float
__device__ __forceinline__ float fx_mean(long long acc, unsigned mag, int n) {
    if (mag >= FX_NONFINITE) return __uint_as_float(0x7fc00000u);
    return mag ? (float)(ldexp((double)acc, fx_exp(mag) - FX_BITS) / (double)n) : 0.f;
}

}  // namespace sculpt
