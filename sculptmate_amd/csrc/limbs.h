// The limb-tiled form of an fp32 matrix (the operands of gemm_l3p.hip) and the splits that produce it; shared by the kernels that
// WRITE activations as limbs (gemm_l3p.hip epilogues, norms.hip LayerNorm, attention_l3.hip) and by the ones that split while they
// stage (gemm_l3.hip, attention_l3.hip): Limb<FMT> is the one statement of each format's split, products and MFMA.
//
// Limb-tiled X [R][K] (K % 32 == 0), rows in blocks of 32, k in chunks of 8, NL limbs per element:
//     byte offset of limb l (0 = leading) of X[r][k] = (((r / 32) * (K / 8) + k / 8) * NL + l) * 512 + (r % 32) * 16 + (k % 8) * 2
// Formats:
//   LT_BF16X3  three bf16 limbs, x = x1 + x2 + x3 EXACTLY for every fp32 x (8 + 8 + 8 significant bits, the fp32 exponent range);
//              six limb products per multiply (gemm_l3.hip's arithmetic);
//   LT_F16X2   two fp16 limbs, x ~ h1 + h2: 22 significant bits while |x| >= 2^-3, an absolute error <= 2^-25 below that, and
//              |x| < 65504 (an fp16 limb has 5 exponent bits: weights are stored pre-multiplied by a power of two that puts their
//              largest magnitude in [2^14, 2^15), undone exactly by the GEMM's alpha; activations go in as they are); three limb
//              products per multiply, each exact in fp32 (11 x 11 bits).
#pragma once
#include "common.h"

namespace sculpt {

static constexpr int LT_BF16X3 = 0, LT_F16X2 = 1;
__host__ __device__ __forceinline__ int lt_limbs(int fmt) { return fmt == LT_F16X2 ? 2 : 3; }

typedef __bf16 lt_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 lt_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 lt_f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 lt_f16x8 __attribute__((ext_vector_type(8)));
typedef float lt_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned lt_u32x4 __attribute__((ext_vector_type(4)));

// What a format is made of: NL limbs, the MFMA operand fragment (8 limbs of 8 consecutive k), the NP limb products that are kept
// as (A limb, B limb) with the smallest terms first, two fp32 -> one packed limb pair (round to nearest even), its halves back as fp32, the MFMA.
template <int FMT> struct LimbFormat;

template <> struct LimbFormat<LT_BF16X3> {
    static constexpr int NL = 3, NP = 6;
    typedef lt_bf16x8 frag;
    static constexpr int PROD[NP][2] = {{0, 2}, {2, 0}, {1, 1}, {0, 1}, {1, 0}, {0, 0}};   // order >= 2^-16 (gemm_l3.hip)
    static __device__ __forceinline__ unsigned cvt_pk(float lo, float hi) {
        const lt_f32x2 v = {lo, hi};
        return __builtin_bit_cast(unsigned, __builtin_convertvector(v, lt_bf16x2));
    }
    static __device__ __forceinline__ float lo(unsigned p) { return __uint_as_float(p << 16); }
    static __device__ __forceinline__ float hi(unsigned p) { return __uint_as_float(p & 0xffff0000u); }
    static __device__ __forceinline__ f32x16 mfma(f32x16 acc, frag a, frag b) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
};

template <> struct LimbFormat<LT_F16X2> {
    static constexpr int NL = 2, NP = 3;
    typedef lt_f16x8 frag;
    static constexpr int PROD[NP][2] = {{1, 0}, {0, 1}, {0, 0}};   // each exact in fp32 (11 x 11 bits)
    static __device__ __forceinline__ unsigned cvt_pk(float lo, float hi) {
        const lt_f32x2 v = {lo, hi};
        return __builtin_bit_cast(unsigned, __builtin_convertvector(v, lt_f16x2));   // v_cvt_pk_f16_f32; |x| >= 65520 -> inf
    }
    static __device__ __forceinline__ float lo(unsigned p) { return (float)__builtin_bit_cast(lt_f16x2, p)[0]; }
    static __device__ __forceinline__ float hi(unsigned p) { return (float)__builtin_bit_cast(lt_f16x2, p)[1]; }
    static __device__ __forceinline__ f32x16 mfma(f32x16 acc, frag a, frag b) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
    }
};

template <int FMT> struct Limb : LimbFormat<FMT> {
    typedef LimbFormat<FMT> F;
    static constexpr int NL = F::NL;
    typedef typename F::frag frag;
    static __device__ __forceinline__ void unpack(unsigned p, float &lo, float &hi) { lo = F::lo(p); hi = F::hi(p); }

    // N pairs of fp32 values -> their packed limb pairs p[limb][pair], limb by limb: each limb the round-to-nearest of the exact
    // remainder of the ones before it.  bf16 x 3: x = x1 + x2 + x3 exactly (24 significant bits minus two 8-bit limbs leave <= 8
    // bits); fp16 x 2: h1 = fp16(x), h2 = fp16(x - h1), the difference is exact.  r is left holding the last remainders.
    template <int N> static __device__ __forceinline__ void split(float (&r)[2 * N], unsigned (&p)[NL][N]) {
#pragma clang fp contract(off)
#pragma unroll
        for (int l = 0; l < NL; ++l) {
#pragma unroll
            for (int i = 0; i < N; ++i) p[l][i] = F::cvt_pk(r[2 * i], r[2 * i + 1]);
#pragma unroll
            for (int i = 0; i < N && l + 1 < NL; ++i) {   // exact
                r[2 * i] = r[2 * i] - F::lo(p[l][i]);
                r[2 * i + 1] = r[2 * i + 1] - F::hi(p[l][i]);
            }
        }
    }
    // two fp32 values -> their NL packed limb pairs
    static __device__ __forceinline__ void split2(float a, float b, unsigned (&p)[NL]) {
        float r[2] = {a, b};
        unsigned q[NL][1];
        split<1>(r, q);
#pragma unroll
        for (int l = 0; l < NL; ++l) p[l] = q[l][0];
    }
    // four consecutive-k fp32 values -> the 8-byte piece of each limb
    static __device__ __forceinline__ void split4(float x0, float x1, float x2, float x3, uint2 (&p)[NL]) {
        float r[4] = {x0, x1, x2, x3};
        unsigned q[NL][2];
        split<2>(r, q);
#pragma unroll
        for (int l = 0; l < NL; ++l) p[l] = make_uint2(q[l][0], q[l][1]);
    }
    // eight fp32 values -> one MFMA operand fragment per limb
    static __device__ __forceinline__ void split8(const float (&x)[8], frag (&f)[NL]) {
        lt_u32x4 v[NL];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned c[NL];
            split2(x[2 * i], x[2 * i + 1], c);
#pragma unroll
            for (int l = 0; l < NL; ++l) v[l][i] = c[l];
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) f[l] = __builtin_bit_cast(frag, v[l]);
    }
    // X[row][col .. col + 3] (col % 4 == 0) of a limb-tiled matrix with k8 = K / 8 chunks per row: split and store the 8-byte pieces
    static __device__ __forceinline__ void store4(unsigned char *base, int k8, long row, int col, const float (&x)[4]) {
        uint2 p[NL];
        split4(x[0], x[1], x[2], x[3], p);
        unsigned char *d = base + (((row >> 5) * k8 + (col >> 3)) * NL) * 512 + (row & 31) * 16 + ((col >> 2) & 1) * 8;
#pragma unroll
        for (int l = 0; l < NL; ++l) *reinterpret_cast<uint2 *>(d + l * 512) = p[l];
    }
};

__device__ __forceinline__ void lt_split4(const float (&x)[4], uint2 &p1, uint2 &p2, uint2 &p3) {
    uint2 p[3];
    Limb<LT_BF16X3>::split4(x[0], x[1], x[2], x[3], p);
    p1 = p[0]; p2 = p[1]; p3 = p[2];
}

__device__ __forceinline__ void lt_split4_h(const float (&x)[4], uint2 &p1, uint2 &p2) {
    uint2 p[2];
    Limb<LT_F16X2>::split4(x[0], x[1], x[2], x[3], p);
    p1 = p[0]; p2 = p[1];
}

__device__ __forceinline__ void lt_store4(unsigned char *base, int k8, long row, int col, const float (&x)[4], int fmt = LT_BF16X3) {
    if (fmt == LT_F16X2) Limb<LT_F16X2>::store4(base, k8, row, col, x);   // kernel-uniform
    else Limb<LT_BF16X3>::store4(base, k8, row, col, x);
}

}  // namespace sculpt
