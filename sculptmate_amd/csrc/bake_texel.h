// The per-texel position rule of the atlas bakes: one copy, so that bake_scene_color_kernel (csrc/bake_scene.hip) and
// bake_scene_normal_kernel (csrc/bake_normal.hip) sample the field at the same bits, the ones bake_interpolate_kernel
// (csrc/baker.hip) gives.  bake_occlusion_kernel (csrc/mesh_ray.hip) takes its positions and its coverage from here too.
#pragma once

#include "common.h"

namespace sculpt {

struct Texel {
    float x[3];
    long i[3];  // the face's vertex rows (checked against nv) when covered, else 0: for callers that interpolate more than positions
    bool covered;
};

// rast = (u, v, w, tri) or (0, 0, 0, -1) -> interpolated position, or the box centre for a texel that is not covered
__device__ __forceinline__ Texel texel_position(const float4 r, const float *__restrict__ v_pos, long nv, const void *__restrict__ faces,
                                                int faces_i64, long nf) {
#pragma clang fp contract(off)
    Texel tx;
    tx.x[0] = tx.x[1] = tx.x[2] = 0.f;
    tx.i[0] = tx.i[1] = tx.i[2] = 0;
    tx.covered = false;
    if (!(r.w >= 0.f && r.w < 2147483648.f)) return tx;  // also a NaN
    const long t = (long)(int)r.w;
    if (t >= nf) return tx;
    long i[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        i[k] = faces_i64 ? (long)reinterpret_cast<const long long *>(faces)[3 * t + k] : (long)reinterpret_cast<const int *>(faces)[3 * t + k];
    if (i[0] < 0 || i[0] >= nv || i[1] < 0 || i[1] >= nv || i[2] < 0 || i[2] >= nv) return tx;
#pragma unroll
    for (int k = 0; k < 3; ++k) tx.x[k] = v_pos[3 * i[0] + k] * r.x + v_pos[3 * i[1] + k] * r.y + v_pos[3 * i[2] + k] * r.z;
#pragma unroll
    for (int k = 0; k < 3; ++k) tx.i[k] = i[k];
    tx.covered = true;
    return tx;
}

}  // namespace sculpt
