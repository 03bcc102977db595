// Volume renderer for gfx950 (MI355X): rays -> box test -> S samples -> fused triplane sample + NeRF-MLP -> alpha composite,
// one launch, nothing per sample in memory.
//
// Replaces (reference file:line):
//   rays_intersect_bbox                      TripoSR/tsr/utils.py:115-149
//   TriplaneNeRFRenderer._forward            TripoSR/tsr/models/nerf_renderer.py:93-152
//
// Shape ("ray renderer"):
//   * a wave owns 32 consecutive rays; lane p = lane & 31 is the ray, the two halves h = lane >> 5 split the layer-0 features
//     exactly as in query_points_kernel (csrc/triplane.hip).  Taps, layer 0, hidden layers, last layer and the two output
//     activations are the point query's own functions (triplane_mlp.h): a sample's density_act and color are the bits
//     ops.triplane_query gives at that point from channel-last planes.
//   * the wave walks s = 0 .. S-1 in order, one 32-point MFMA tile per depth (neighbouring rays at equal depth read neighbouring
//     texels).  T, sum w and the three colour sums stay in registers; the composite is a plain sequential fp32 product and sum:
//     no cross-lane operation, no atomics, and a ray's result depends on nothing but the ray -- not on the grid, not on which
//     rays share its tile.
//   * a tile with no valid ray is skipped; an invalid ray in a mixed tile samples the box centre and stores white.
//   * weights into LDS and the launch plan of all three kernels: field_prologue / field_plan / field_grid (field_kernel.h).
//   * ray geometry and composite are compiled with contraction off (every fp32 operation rounded on its own, as torch on the
//     CPU does): z_vals and xyz equal the reference's bit for bit.
// Three quirks of the reference are kept: |d| < 1e-6 becomes +1e-6 whatever the sign of d; delta is the step of the unit
// interval t_vals, not a world length; T is multiplied by (1 - alpha + 1e-10).
//
// Passes beside the colour (sculpt_render_passes, DESIGN.md section 3.1b "passes"): raw per-ray sums, exactly 0 for a miss.
//   * depth_sum = sum_s w_s z_s and premul = sum_s w_s c_s (the colour sums before the white background) alone come from the
//     colour kernel's second form, render_rays_kernel<C, float *, float *>: the same code with one more sum and two more stores.
//     render_rays_kernel<C> is the kernel it always was, instruction for instruction.
//   * normal_sum = sum_s w_s n_s needs the field's gradient at every sample: render_passes_kernel, in the forward-mode layout
//     of density_grad_kernel (csrc/field_normal.hip): a wave owns 8 rays x 4 columns {value, d/dx, d/dy, d/dz}, lane p serves
//     ray p >> 2 and kind p & 3, and a sample is one field_eval_fwd (field_fwd.h), which leaves what the last layer reads for
//     the colour rows.  The value column is the point query's own evaluation, so density_act and colour, and with
//     them w_s and every output of the colour kernel, have the colour kernel's bits (the same ray_box, t_mid block,
//     density_act_f, color_f, expf and composite); a call that asks for normal_sum is this ONE launch, not two.  n_s is
//     unit_normal_of (field_fwd.h), the rule and the bits of ops.field_normals at x_s = o + z_s d.  The value lane composites
//     what the colour kernel composites; the tangent lane of axis k keeps component k of normal_sum.
//   * exact skipping: once T == 0 on every ray of a tile, every later w_s is alpha * 0 = +0 (alpha is in [0, 1] for a finite
//     field) and adds nothing to any sum (n_s is finite by construction), so the tile stops evaluating; depths and zero weights
//     of the tail are still written.  No threshold.  SCULPT_RENDER_FORM=noskip walks every sample (A/B); the two forms differ
//     only for a field that is not finite (a NaN density where T == 0 gives w = NaN in the walk and +0 in the skip).
#include "common.h"
#include "field_fwd.h"
#include "triplane_mlp.h"

namespace sculpt {

struct RayHit {
    float t_near, t_far;
    bool valid;
};

// utils.py:115-149 with near = 0, valid_thresh = 0.01; `box` = fp32((1 - 1e-3)) * radius
__device__ __forceinline__ RayHit ray_box(const float o[3], const float d[3], float box) {
#pragma clang fp contract(off)
    float tn = 0.f, tf = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float dv = fabsf(d[k]) < 1e-6f ? 1e-6f : d[k];
        const float i0 = (box - o[k]) / dv, i1 = (-box - o[k]) / dv;
        const float lo = fminf(i0, i1), hi = fmaxf(i0, i1);
        tn = k == 0 ? lo : fmaxf(tn, lo);
        tf = k == 0 ? hi : fminf(tf, hi);
    }
    tn = fmaxf(tn, 0.f);
    RayHit r;
    r.valid = tf - tn > 0.01f;
    r.t_near = r.valid ? tn : 0.f;
    r.t_far = r.valid ? tf : 0.f;
    return r;
}

// Without `Passes` this is the colour kernel, argument for argument the one it always was.  render_rays_kernel<C, float *, float *>
// takes depth_sum [N] and premul [N][3] (each nullable) after a0_lds and is the same code with the two sums added.
template <int C, class... Passes>
__global__ __launch_bounds__(512) void render_rays_kernel(
    const float *__restrict__ planes, int H, int W, const float *__restrict__ blob, const float *__restrict__ rays_o,
    const float *__restrict__ rays_d, long N, float radius, float span, float box, float density_bias,
    const float *__restrict__ t_vals, int S, float *__restrict__ comp_rgb, float *__restrict__ opacity,
    float *__restrict__ z_vals, float *__restrict__ weights, int a0_lds, Passes... passes) {
    static_assert(sizeof...(Passes) == 0 || sizeof...(Passes) == 2, "no passes, or (float *depth_sum, float *premul)");
    constexpr bool PASSES = sizeof...(Passes) == 2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FieldCtx c = field_prologue<C>(smem, blob, a0_lds);
    const LdsView &L = c.L;
    const int lane = c.lane, p = c.p, h = c.h;
    const long ntiles = (N + 31) / 32;
    const long HW = (long)H * W;

    for (long tile = (long)blockIdx.x * c.nwave + c.wave; tile < ntiles; tile += (long)gridDim.x * c.nwave) {
        const long n = tile * 32 + p;
        const bool live = n < N, writer = live && h == 0;
        const long nc = live ? n : N - 1;
        float o[3], d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { o[k] = rays_o[3 * nc + k]; d[k] = rays_d[3 * nc + k]; }
        const RayHit hit = ray_box(o, d, box);
        const bool valid = live && hit.valid;
        float T = 1.f, sw = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, dz = 0.f;
        if (__builtin_amdgcn_ballot_w64(valid) != 0) {  // wave-uniform
            for (int s = 0; s < S; ++s) {
                float z, x[3], delta;
                {
#pragma clang fp contract(off)
                    const float ta = t_vals[s], tb = t_vals[s + 1];
                    const float t_mid = (ta + tb) / 2.0f;
                    z = hit.t_near * (1.0f - t_mid) + hit.t_far * t_mid;
#pragma unroll
                    for (int k = 0; k < 3; ++k) x[k] = valid ? o[k] + z * d[k] : 0.f;
                    delta = tb - ta;
                }
                int off[3][4];
                float wt[3][4];
                point_taps<false>(x[0], x[1], x[2], radius, span, H, W, off, wt);
                f32x16 acc0 = lds_bias16(L.bacc, 0, h, 0);
                f32x16 acc1 = lds_bias16(L.bacc, 0, h, 1);
                layer0_channel_last<C>(planes, HW, off, wt, c.a0s, c.A0g, a0_lds, lane, h, acc0, acc1);
                f32x16 x0 = silu16(acc0), x1 = silu16(acc1);
                hidden_layers(L, c.NH, lane, h, x0, x1);
                const float dens = density_act_f(last_dot(L, 0, h, x0, x1), density_bias);
                const float r = color_f(last_dot(L, 1, h, x0, x1));
                const float g = color_f(last_dot(L, 2, h, x0, x1));
                const float b = color_f(last_dot(L, 3, h, x0, x1));
                float w;
                {   // nerf_renderer.py:125-140, one sample further along the ray
#pragma clang fp contract(off)
                    const float alpha = 1.0f - expf(-delta * dens);
                    w = alpha * T;
                    sw = sw + w;
                    c0 = c0 + w * r;
                    c1 = c1 + w * g;
                    c2 = c2 + w * b;
                    if (PASSES) dz = dz + w * z;
                    T = T * ((1.0f - alpha) + 1e-10f);
                }
                if (writer) {
                    if (z_vals) z_vals[n * S + s] = valid ? z : 0.f;
                    if (weights) weights[n * S + s] = valid ? w : 0.f;
                }
            }
        } else if (writer) {
            for (int s = 0; s < S; ++s) {
                if (z_vals) z_vals[n * S + s] = 0.f;
                if (weights) weights[n * S + s] = 0.f;
            }
        }
        if (writer) {
#pragma clang fp contract(off)
            const float op = valid ? sw : 0.f;
            const float bg = 1.0f - op;  // nerf_renderer.py:149: white behind what the ray did not absorb
            comp_rgb[3 * n] = (valid ? c0 : 0.f) + bg;
            comp_rgb[3 * n + 1] = (valid ? c1 : 0.f) + bg;
            comp_rgb[3 * n + 2] = (valid ? c2 : 0.f) + bg;
            if (opacity) opacity[n] = op;
            if constexpr (PASSES) {
                float *const out[2] = {passes...};
                float *const depth_sum = out[0], *const premul = out[1];
                if (depth_sum) depth_sum[n] = valid ? dz : 0.f;
                if (premul) {
                    premul[3 * n] = valid ? c0 : 0.f;
                    premul[3 * n + 1] = valid ? c1 : 0.f;
                    premul[3 * n + 2] = valid ? c2 : 0.f;
                }
            }
        }
    }
}

// Every output in one launch, for a call that asks for normal_sum: 8 rays x 4 forward-mode columns per wave (see the head of this
// file).  The value lane of a ray composites what the colour kernel composites, from the same values in the same order; the
// tangent lane of axis k keeps component k of normal_sum.  All outputs but comp_rgb and normal_sum are nullable.
template <int C>
__global__ __launch_bounds__(512) void render_passes_kernel(
    const float *__restrict__ planes, int H, int W, const float *__restrict__ blob, const float *__restrict__ rays_o,
    const float *__restrict__ rays_d, long N, float radius, float span, float box, float density_bias,
    const float *__restrict__ t_vals, int S, float *__restrict__ comp_rgb, float *__restrict__ opacity,
    float *__restrict__ z_vals, float *__restrict__ weights, float *__restrict__ depth_sum, float *__restrict__ normal_sum,
    float *__restrict__ premul, int a0_lds, int noskip) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FieldCtx c = field_prologue<C>(smem, blob, a0_lds);
    const LdsView &L = c.L;
    const int p = c.p, h = c.h, kind = p & 3;
    const bool is_value = kind == 0;
    const long ntiles = (N + 7) / 8;

    for (long tile = (long)blockIdx.x * c.nwave + c.wave; tile < ntiles; tile += (long)gridDim.x * c.nwave) {
        const long n = tile * 8 + (p >> 2);
        const bool live = n < N, writer = live && is_value && h == 0;
        const long nc = live ? n : N - 1;
        float o[3], d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { o[k] = rays_o[3 * nc + k]; d[k] = rays_d[3 * nc + k]; }
        const RayHit hit = ray_box(o, d, box);
        const bool valid = live && hit.valid;
        float T = 1.f, sw = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, dz = 0.f;
        float nk_sum = 0.f;  // component kind - 1 of normal_sum (not used in the value lane)
        int s = 0;
        if (__builtin_amdgcn_ballot_w64(valid) != 0) {  // wave-uniform
            for (; s < S; ++s) {
                // every ray of the tile is opaque or a miss: each later weight is alpha * 0 = +0 and changes no sum
                if (!noskip && __builtin_amdgcn_ballot_w64(valid && T != 0.f) == 0) break;
                float z, x[3], delta;
                {   // the colour kernel's block, word for word: the same z and xyz bits
#pragma clang fp contract(off)
                    const float ta = t_vals[s], tb = t_vals[s + 1];
                    const float t_mid = (ta + tb) / 2.0f;
                    z = hit.t_near * (1.0f - t_mid) + hit.t_far * t_mid;
#pragma unroll
                    for (int k = 0; k < 3; ++k) x[k] = valid ? o[k] + z * d[k] : 0.f;
                    delta = tb - ta;
                }
                f32x16 x0, x1;
                const float q = field_eval_fwd<C, false>(c, planes, H, W, radius, span, a0_lds, kind, x[0], x[1], x[2], x0, x1);
                const float dens = density_act_f(quad_bcast<0>(q + L.blast[0]), density_bias);  // last_dot(L, 0, ...) of the value column
                const float r = color_f(last_dot(L, 1, h, x0, x1));  // the colour of the value column; unused elsewhere
                const float g = color_f(last_dot(L, 2, h, x0, x1));
                const float b = color_f(last_dot(L, 3, h, x0, x1));
                float nrm[3];
                unit_normal_of(quad_bcast<1>(q), quad_bcast<2>(q), quad_bcast<3>(q), nrm[0], nrm[1], nrm[2]);
                const float nk = kind == 1 ? nrm[0] : (kind == 2 ? nrm[1] : nrm[2]);
                float w;
                {   // the colour kernel's composite, then the two new sums
#pragma clang fp contract(off)
                    const float alpha = 1.0f - expf(-delta * dens);
                    w = alpha * T;
                    sw = sw + w;
                    c0 = c0 + w * r;
                    c1 = c1 + w * g;
                    c2 = c2 + w * b;
                    dz = dz + w * z;
                    nk_sum = nk_sum + w * nk;
                    T = T * ((1.0f - alpha) + 1e-10f);
                }
                if (writer) {
                    if (z_vals) z_vals[n * S + s] = valid ? z : 0.f;
                    if (weights) weights[n * S + s] = valid ? w : 0.f;
                }
            }
        }
        if (writer && (z_vals || weights)) {  // what a skipped tail or a tile of misses leaves: the depths, and weights of +0
            for (; s < S; ++s) {
#pragma clang fp contract(off)
                const float ta = t_vals[s], tb = t_vals[s + 1];
                const float t_mid = (ta + tb) / 2.0f;
                const float z = hit.t_near * (1.0f - t_mid) + hit.t_far * t_mid;
                if (z_vals) z_vals[n * S + s] = valid ? z : 0.f;
                if (weights) weights[n * S + s] = 0.f;
            }
        }
        if (writer) {
#pragma clang fp contract(off)
            const float op = valid ? sw : 0.f;
            const float bg = 1.0f - op;
            comp_rgb[3 * n] = (valid ? c0 : 0.f) + bg;
            comp_rgb[3 * n + 1] = (valid ? c1 : 0.f) + bg;
            comp_rgb[3 * n + 2] = (valid ? c2 : 0.f) + bg;
            if (opacity) opacity[n] = op;
            if (depth_sum) depth_sum[n] = valid ? dz : 0.f;
            if (premul) {
                premul[3 * n] = valid ? c0 : 0.f;
                premul[3 * n + 1] = valid ? c1 : 0.f;
                premul[3 * n + 2] = valid ? c2 : 0.f;
            }
        }
        if (live && !is_value && h == 0) normal_sum[3 * n + (kind - 1)] = valid ? nk_sum : 0.f;
    }
}

}  // namespace sculpt

using namespace sculpt;

extern "C" int sculpt_render_rays(const float *planes_cl, int C, int H, int W, const void *mlp_packed, int n_hidden_64,
                                  const float *rays_o, const float *rays_d, int64_t n_rays, float radius, float density_bias,
                                  const float *t_vals, int S, float *comp_rgb, float *opacity, float *z_vals, float *weights,
                                  sculpt_stream_t stream) {
    FieldPlan plan;
    if (const int e = field_plan("render_rays", C, planes_cl, mlp_packed, H, W, n_hidden_64, radius, plan, [&] {
            SC_REQUIRE(n_rays >= 0, "render_rays: negative ray count");
            SC_REQUIRE(S >= 1, "render_rays: need at least one sample per ray (got %d)", S);
            return 0;
        }))
        return e;
    if (n_rays == 0) return 0;
    SC_REQUIRE(rays_o && rays_d && t_vals && comp_rgb, "render_rays: null rays, t_vals or comp_rgb");
    auto kern = render_rays_kernel<40>;
    int grid;
    if (const int e = field_grid(plan, kern, ((long)n_rays + 31) / 32, grid)) return e;
    const float box = (float)(1.0 - 1.0e-3) * radius;  // utils.py:131-133, the product rounded once in fp32
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), plan.lds, as_stream(stream), planes_cl, H, W,
                       reinterpret_cast<const float *>(mlp_packed), rays_o, rays_d, (long)n_rays, radius, plan.span, box, density_bias,
                       t_vals, S, comp_rgb, opacity, z_vals, weights, plan.a0_lds);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sculpt_render_passes(const float *planes_cl, int C, int H, int W, const void *mlp_packed, int n_hidden_64,
                                    const float *rays_o, const float *rays_d, int64_t n_rays, float radius, float density_bias,
                                    const float *t_vals, int S, float *comp_rgb, float *opacity, float *z_vals, float *weights,
                                    float *depth_sum, float *normal_sum, float *premul, sculpt_stream_t stream) {
    if (!depth_sum && !normal_sum && !premul)  // the colour picture alone: sculpt_render_rays' own launch
        return sculpt_render_rays(planes_cl, C, H, W, mlp_packed, n_hidden_64, rays_o, rays_d, n_rays, radius, density_bias, t_vals, S,
                                  comp_rgb, opacity, z_vals, weights, stream);
    FieldPlan plan;
    if (const int e = field_plan("render_passes", C, planes_cl, mlp_packed, H, W, n_hidden_64, radius, plan, [&] {
            SC_REQUIRE(n_rays >= 0, "render_passes: negative ray count");
            SC_REQUIRE(S >= 1, "render_passes: need at least one sample per ray (got %d)", S);
            return 0;
        }))
        return e;
    if (n_rays == 0) return 0;
    SC_REQUIRE(rays_o && rays_d && t_vals && comp_rgb, "render_passes: null rays, t_vals or comp_rgb");
    const float box = (float)(1.0 - 1.0e-3) * radius;
    int grid;
    const float *blob = reinterpret_cast<const float *>(mlp_packed);
    if (normal_sum) {  // everything in the forward-mode layout, one launch
        auto kern = render_passes_kernel<40>;
        if (const int e = field_grid(plan, kern, ((long)n_rays + 7) / 8, grid)) return e;
        const int noskip = form_has("SCULPT_RENDER_FORM", "noskip") ? 1 : 0;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), plan.lds, as_stream(stream), planes_cl, H, W, blob, rays_o, rays_d, (long)n_rays,
                           radius, plan.span, box, density_bias, t_vals, S, comp_rgb, opacity, z_vals, weights, depth_sum, normal_sum, premul,
                           plan.a0_lds, noskip);
    } else {  // the colour kernel with its two more sums
        auto kern = render_rays_kernel<40, float *, float *>;
        if (const int e = field_grid(plan, kern, ((long)n_rays + 31) / 32, grid)) return e;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), plan.lds, as_stream(stream), planes_cl, H, W, blob, rays_o, rays_d, (long)n_rays,
                           radius, plan.span, box, density_bias, t_vals, S, comp_rgb, opacity, z_vals, weights, plan.a0_lds, depth_sum, premul);
    }
    SC_LAUNCH_CHECK();
    return 0;
}
