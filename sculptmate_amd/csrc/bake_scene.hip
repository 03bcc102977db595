// Texture bake of a TripoSR scene code for gfx950 (MI355X): rasterised UV atlas -> colour per covered texel, one launch,
// no position image in memory and no decoder work on texels between the charts.
//
// The hot step of upstream TripoSR's --bake-texture (the colour field queried once per covered texel of the unwrapped mesh);
// the composed route of this library is sculpt_bake_interpolate + sculpt_triplane_query_ex over every texel (what sf3d/bake.py
// does for its 1 M texels).
//
// Shape ("texture bake"):
//   * a wave owns 32 consecutive texels; lane p = lane & 31 is the texel, the two halves h = lane >> 5 split the layer-0
//     features exactly as in query_points_kernel (csrc/triplane.hip) and render_rays_kernel (csrc/render.hip).  Taps, layer 0,
//     hidden layers, the three colour rows of the last layer and the colour activation are the point query's own functions
//     (triplane_mlp.h): a covered texel's colour is the bits ops.triplane_query gives at the interpolated position from
//     channel-last planes.  The density row is not evaluated.
//   * the position (texel_position, bake_texel.h) is (a*u + b*v) + c*w per component with contraction off: the bits of bake_interpolate_kernel (csrc/baker.hip),
//     gathered through faces[t] from the indexed vertex array.
//   * weights into LDS and the launch plan: field_prologue / field_plan / field_grid (field_kernel.h), as in render_rays_kernel.
//   * a tile with no covered texel is skipped (wave-uniform ballot) and stores zeros; an uncovered texel in a mixed tile samples
//     the box centre and stores 0, 0, 0 and mask 0.  A texel's result depends on that texel alone.
//   * index guard: a texel whose triangle index is outside [0, nf) or whose vertex indices are outside [0, nv) is uncovered;
//     nothing is read through such an index.
#include "bake_texel.h"
#include "common.h"
#include "field_kernel.h"
#include "triplane_mlp.h"

namespace sculpt {

template <int C>
__global__ __launch_bounds__(512) void bake_scene_color_kernel(
    const float *__restrict__ planes, int H, int W, const float *__restrict__ blob, const float *__restrict__ v_pos, long nv,
    const void *__restrict__ faces, int faces_i64, long nf, const float4 *__restrict__ rast, long N, float radius, float span,
    float *__restrict__ color, uint8_t *__restrict__ mask, int a0_lds) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FieldCtx c = field_prologue<C>(smem, blob, a0_lds);
    const LdsView &L = c.L;
    const int lane = c.lane, p = c.p, h = c.h;
    const long ntiles = (N + 31) / 32;
    const long HW = (long)H * W;

    for (long tile = (long)blockIdx.x * c.nwave + c.wave; tile < ntiles; tile += (long)gridDim.x * c.nwave) {
        const long n = tile * 32 + p;
        const bool live = n < N, writer = live && h == 0;
        const Texel tx = texel_position(rast[live ? n : N - 1], v_pos, nv, faces, faces_i64, nf);
        const bool covered = live && tx.covered;
        float r = 0.f, g = 0.f, b = 0.f;
        if (__builtin_amdgcn_ballot_w64(covered) != 0) {  // wave-uniform
            int off[3][4];
            float wt[3][4];
            point_taps<false>(tx.x[0], tx.x[1], tx.x[2], radius, span, H, W, off, wt);
            f32x16 acc0 = lds_bias16(L.bacc, 0, h, 0);
            f32x16 acc1 = lds_bias16(L.bacc, 0, h, 1);
            layer0_channel_last<C>(planes, HW, off, wt, c.a0s, c.A0g, a0_lds, lane, h, acc0, acc1);
            f32x16 x0 = silu16(acc0), x1 = silu16(acc1);
            hidden_layers(L, c.NH, lane, h, x0, x1);
            r = color_f(last_dot(L, 1, h, x0, x1));
            g = color_f(last_dot(L, 2, h, x0, x1));
            b = color_f(last_dot(L, 3, h, x0, x1));
        }
        if (writer) {
            color[3 * n] = covered ? r : 0.f;
            color[3 * n + 1] = covered ? g : 0.f;
            color[3 * n + 2] = covered ? b : 0.f;
            if (mask) mask[n] = covered ? 1 : 0;
        }
    }
}

}  // namespace sculpt

using namespace sculpt;

extern "C" int sculpt_bake_scene_color(const float *planes_cl, int C, int H, int W, const void *mlp_packed, int n_hidden_64,
                                       const float *v_pos, size_t nv, const void *faces, int faces_i64, size_t nf, const float *rast,
                                       int res, float radius, float *color, uint8_t *mask, sculpt_stream_t stream) {
    FieldPlan plan;
    if (const int e = field_plan("bake_scene_color", C, planes_cl, mlp_packed, H, W, n_hidden_64, radius, plan, [&] {
            SC_REQUIRE(res >= 0, "bake_scene_color: negative resolution");
            return 0;
        }))
        return e;
    SC_REQUIRE(nv <= (size_t)1 << 40 && nf <= (size_t)1 << 40, "bake_scene_color: mesh too large");
    if (res == 0) return 0;
    SC_REQUIRE(rast && color, "bake_scene_color: null rast or color");
    SC_REQUIRE(nf == 0 || (v_pos && faces && nv > 0), "bake_scene_color: null mesh");
    auto kern = bake_scene_color_kernel<40>;
    const long N = (long)res * res;
    int grid;
    if (const int e = field_grid(plan, kern, (N + 31) / 32, grid)) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), plan.lds, as_stream(stream), planes_cl, H, W,
                       reinterpret_cast<const float *>(mlp_packed), v_pos, (long)nv, faces, faces_i64, (long)nf,
                       reinterpret_cast<const float4 *>(rast), N, radius, plan.span, color, mask, plan.a0_lds);
    SC_LAUNCH_CHECK();
    return 0;
}
