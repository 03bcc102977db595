// What every kernel that evaluates the triplane decoder from channel-last planes has in common, one copy of each: the kernel
// prologue (weights into LDS, the lane's place in its wave) and the host launch plan (the checks every entry makes, the LDS size,
// the grid).  Users: density_grad_kernel (csrc/field_normal.hip), project_kernel and project_along_kernel (csrc/mesh_project.hip),
// bake_scene_normal_kernel (csrc/bake_normal.hip), bake_scene_surface_kernel (csrc/bake_surface.hip), bake_scene_color_kernel
// (csrc/bake_scene.hip), render_rays_kernel and render_passes_kernel (csrc/render.hip).  query_points_kernel (csrc/triplane.hip)
// keeps its own text.
#pragma once

#include <algorithm>

#include "common.h"
#include "triplane_mlp.h"

namespace sculpt {

// what a lane knows once the workgroup's weights are staged
struct FieldCtx {
    LdsView L;          // hidden weights, biases and the last layer, in LDS
    int NH;             // hidden 64 x 64 layers
    const float *a0s;   // layer 0 in LDS (read when a0_lds) ...
    const float *A0g;   // ... and in global memory
    int lane, wave, nwave;
    int p, h;           // MFMA column (lane & 31) and half (lane >> 5: which layer-0 features and which neurons)
};

// `smem` is the kernel's dynamic LDS, sized by FieldPlan::lds; every thread of the workgroup calls this once, first.
template <int C>
__device__ __forceinline__ FieldCtx field_prologue(float *smem, const float *blob, int a0_lds) {
    const MlpPackHeader hd = *reinterpret_cast<const MlpPackHeader *>(blob);
    FieldCtx c;
    c.NH = hd.NH;
    float *a0s = smem + lds_floats_for(c.NH);
    if (a0_lds) stage_a0_in_lds<C>(a0s, blob, hd);
    load_weights_to_lds(smem, blob, hd);
    c.L = lds_view(smem, c.NH);
    c.a0s = a0s;
    c.A0g = blob + hd.off_a0;
    c.lane = threadIdx.x & 63, c.wave = threadIdx.x >> 6, c.nwave = blockDim.x >> 6;
    c.p = c.lane & 31, c.h = c.lane >> 5;
    return c;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
struct FieldPlan {
    const char *who;
    int n_hidden_64;
    size_t lds;    // dynamic LDS bytes: the hidden weights, and layer 0's behind them when both fit 160 KB
    int a0_lds;
    float span;    // the box's edge as the reference computes it: radius - (-radius)
};

// The checks every entry makes before its early return, in the order every entry made them: the planes, then `count_checks()`
// (the entry's own checks of its point / texel / ray count and flags; 0 or the error code), then the MLP and the radius; and the
// plan.  Messages begin with `who`.  Whether the weights fit LDS is field_grid's to say: that check comes after the early return.
template <class CountChecks>
static inline int field_plan(const char *who, int C, const void *planes_cl, const void *mlp_packed, int H, int W, int n_hidden_64,
                             float radius, FieldPlan &plan, CountChecks count_checks) {
    SC_REQUIRE(C == 40, "%s: built for C=40 channels per plane (got %d)", who, C);
    SC_REQUIRE(planes_cl && mlp_packed, "%s: null input", who);
    SC_REQUIRE(H >= 1 && W >= 1, "%s: bad plane size %d x %d", who, H, W);
    if (const int e = count_checks()) return e;
    SC_REQUIRE(n_hidden_64 >= 0, "%s: bad n_hidden_64", who);
    SC_REQUIRE(radius > 0.f, "%s: radius must be positive", who);
    plan.who = who;
    plan.n_hidden_64 = n_hidden_64;
    plan.lds = (size_t)lds_floats_for(n_hidden_64) * sizeof(float);
    const size_t a0_bytes = (size_t)3 * C * 64 * sizeof(float);
    plan.a0_lds = plan.lds + a0_bytes <= 160 * 1024 ? 1 : 0;
    if (plan.a0_lds) plan.lds += a0_bytes;
    plan.span = (float)((double)radius - (double)(-radius));
    return 0;
}

// `kern` gets the plan's dynamic LDS; grid <- the workgroups of 512 threads (8 waves, a wave per tile at a time) for `tiles` tiles
template <class Kernel>
static inline int field_grid(const FieldPlan &plan, Kernel kern, long tiles, int &grid) {
    SC_REQUIRE(plan.lds <= 160 * 1024, "%s: %d hidden layers do not fit LDS", plan.who, plan.n_hidden_64);
    SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    grid = (int)std::min<long>((tiles + 7) / 8, num_cus());
    return 0;
}

}  // namespace sculpt
