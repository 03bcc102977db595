// The tangent-frame arithmetic of the normal bakes: one copy, so that bake_scene_normal_kernel and corner_tangents_kernel
// (csrc/bake_normal.hip) and bake_scene_surface_kernel (csrc/bake_surface.hip) store the same bits.  Every operation is rounded
// on its own (contraction off); csrc/bake_normal.hip's header states the transform, tests/_nmapref.py restates it in NumPy.
#pragma once

#include "common.h"

namespace sculpt {

__device__ __forceinline__ float dot3_nc(const float (&a)[3], const float (&b)[3]) {
#pragma clang fp contract(off)
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

__device__ __forceinline__ void cross3_nc(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
#pragma clang fp contract(off)
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ bool positive_finite(float x) { return x > 0.f && x < INFINITY; }

// world normal n -> the vector a tangent-space normal map stores (csrc/bake_normal.hip's header: "The tangent-space transform")
__device__ __forceinline__ void to_tangent_space(const float (&n)[3], float u, float v, float w, const float *__restrict__ cn,
                                                 const float *__restrict__ ct, float (&out)[3]) {
#pragma clang fp contract(off)
    float N[3], T[3], C[3], B[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        N[c] = (cn[c] * u + cn[3 + c] * v) + cn[6 + c] * w;
        T[c] = (ct[c] * u + ct[4 + c] * v) + ct[8 + c] * w;
    }
    const float s = ct[3];
    cross3_nc(N, T, C);
#pragma unroll
    for (int c = 0; c < 3; ++c) B[c] = s * C[c];
    const float gtt = dot3_nc(T, T), gnn = dot3_nc(N, N), gtn = dot3_nc(T, N);
    const float D = gtt * gnn - gtn * gtn;
    const float nT = dot3_nc(n, T), nN = dot3_nc(n, N), nB = dot3_nc(n, B);
    const float x = nT * gnn - nN * gtn, y = nB, z = nN * gtt - nT * gtn;
    const float len = sqrtf((x * x + y * y) + z * z);
    const bool zero_n = n[0] == 0.f && n[1] == 0.f && n[2] == 0.f;
    if (D > 0.f && positive_finite(len) && !zero_n) {
        out[0] = x / len; out[1] = y / len; out[2] = z / len;
    } else {
        out[0] = 0.f; out[1] = 0.f; out[2] = 1.f;
    }
}

}  // namespace sculpt
