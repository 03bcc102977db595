// Bake at the surface, for gfx950 (MI355X): rasterised UV atlas -> per covered texel the point of the density field's iso-surface
// d(p) = target that the projection rule reaches from the texel's point on the low-poly face, and the field's unit normal THERE,
// in object space or in the tangent frame of the low-poly mesh; one launch (sculpt_bake_scene_surface).
//
// bake_scene_surface_kernel is three kernels the project already has, fused:
//   * the span compaction of bake_scene_normal_kernel (csrc/bake_normal.hip), the one copy in field_fwd.h: a wave owns 64
//     consecutive texels, one per lane; texel_position (bake_texel.h) gives p0 and the coverage; span_compact brings the covered
//     p0 to the low lanes in rank order and the wave runs ceil(count / 8) forward-mode tiles over ranks 8k .. 8k + 7.  An empty
//     span runs no tile.
//   * the loop of project_kernel (csrc/mesh_project.hip) inside each tile: proj_start, then one evaluation is field_eval_fwd
//     (field_fwd.h, density_grad_kernel's call), the eight lanes of a point all hold (d, g) afterwards and run rule_update
//     (csrc/project_rule.h, the one copy of the rule) redundantly in registers.  The loop leaves when a ballot finds no lane of
//     the tile active, at the latest after max_steps + 1 evaluations.  Columns past `count` in the last tile start inactive:
//     they evaluate with the wave (at the box centre, an uncovered texel's position) and take no step, so they never keep the
//     tile in the loop.
//   * the normal at the point the rule returns.  rule_update says when the evaluated candidate became the best iterate; the
//     lanes then keep that evaluation's RAW gradient (the rule itself masks frozen axes; the normal does not), and after the loop
//     unit_normal_of (field_fwd.h) of the kept gradient is sculpt_triplane_density_grad's `normal` at the returned point, bit
//     for bit: it is the same evaluation at the same point, and a column's bits depend on that column alone.  No further
//     evaluation is run.
//   After the last tile the nine results of a rank (point, normal, residual, status, evals) return to their texel's lane
//   (span_return); the frame transform (to_tangent_space, csrc/tangent_frame.h, at the texel's own barycentrics: the low-poly
//   face and its interpolated frame do not move) and the stores happen there.
//   * 512 threads, hidden weights (and layer 0's, when they fit) in LDS once per workgroup (field_prologue and the launch plan
//     of field_kernel.h) as in density_grad_kernel; the compaction uses lane permutes, no LDS of its own.  Nothing waits on
//     another wave.
//
// Uncovered texels: point, normal and residual exactly +0, status -1, evals 0, mask 0.  A texel's outputs depend on that texel
// alone.
#include "bake_texel.h"
#include "common.h"
#include "field_fwd.h"
#include "project_rule.h"
#include "tangent_frame.h"
#include "triplane_mlp.h"

namespace sculpt {

template <int C, bool FRAME>
__global__ __launch_bounds__(512) void bake_scene_surface_kernel(
    const float *__restrict__ planes, int H, int W, const float *__restrict__ blob, const float *__restrict__ v_pos, long nv,
    const void *__restrict__ faces, int faces_i64, long nf, const float4 *__restrict__ rast, long N, float radius, float span_w,
    const float *__restrict__ corner_n, const float *__restrict__ corner_t, float target, int K, float md2, float res_tol,
    float *__restrict__ out_point, float *__restrict__ out_normal, float *__restrict__ out_res, int *__restrict__ out_status,
    int *__restrict__ out_evals, uint8_t *__restrict__ out_mask, int a0_lds) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FieldCtx c = field_prologue<C>(smem, blob, a0_lds);
    const int lane = c.lane, p = c.p, kind = p & 3;
    const long nspans = (N + 63) / 64;

    for (long sp = (long)blockIdx.x * c.nwave + c.wave; sp < nspans; sp += (long)gridDim.x * c.nwave) {
        const long n = sp * 64 + lane;
        const bool live = n < N;
        const float4 r = rast[live ? n : N - 1];
        const Texel tx = texel_position(r, v_pos, nv, faces, faces_i64, nf);
        const bool covered = live && tx.covered;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(covered);
        float pt[3] = {0.f, 0.f, 0.f}, wn[3] = {0.f, 0.f, 0.f}, res = 0.f;
        int status = -1, evals = 0;
        if (m != 0) {  // wave-uniform
            const SpanRanks sr = span_compact(m, covered, lane, tx.x);
            // what rank `lane` ends with
            float rpx = 0.f, rpy = 0.f, rpz = 0.f, rnx = 0.f, rny = 0.f, rnz = 0.f, rres = 0.f;
            int rstatus = -1, revals = 0;
            for (int t = 0; t < span_tiles(sr); ++t) {
                float p0x, p0y, p0z;
                const int rank = span_tile_point(sr, t, p, p0x, p0y, p0z);
                const bool fx = fabsf(p0x) >= radius, fy = fabsf(p0y) >= radius, fz = fabsf(p0z) >= radius;
                ProjState s = proj_start(p0x, p0y, p0z, rank < sr.count);  // a column past the last covered texel takes no step
                float qx = p0x, qy = p0y, qz = p0z;
                float bgx = 0.f, bgy = 0.f, bgz = 0.f;  // the raw gradient at the best iterate
                for (int k = 0; k <= K; ++k) {  // K <= 64 (checked at the entry): at most K + 1 evaluations
                    const float sv = field_eval_fwd<C, false>(c, planes, H, W, radius, span_w, a0_lds, kind, qx, qy, qz);
                    const float d = quad_bcast<0>(sv) + c.L.blast[0];
                    const float gx = quad_bcast<1>(sv), gy = quad_bcast<2>(sv), gz = quad_bcast<3>(sv);
                    if (rule_update(s, k, K, d, gx, gy, gz, qx, qy, qz, p0x, p0y, p0z, fx, fy, fz, target, radius, md2, res_tol))
                        bgx = gx, bgy = gy, bgz = gz;
                    if (__ballot(s.active) == 0ull) break;  // wave-uniform: all eight points have stopped
                }
                float nx, ny, nz;
                unit_normal_of(bgx, bgy, bgz, nx, ny, nz);
                const float gpx = span_gather(s.bx, lane), gpy = span_gather(s.by, lane), gpz = span_gather(s.bz, lane);
                const float gnx = span_gather(nx, lane), gny = span_gather(ny, lane), gnz = span_gather(nz, lane);
                const float gres = span_gather(s.br, lane);
                const int gstatus = span_gather(s.status, lane), gevals = span_gather(s.evals, lane);
                if (span_keeps(t, lane)) {
                    rpx = gpx, rpy = gpy, rpz = gpz;
                    rnx = gnx, rny = gny, rnz = gnz;
                    rres = gres, rstatus = gstatus, revals = gevals;
                }
            }
            const float bpx = span_return(sr, rpx), bpy = span_return(sr, rpy), bpz = span_return(sr, rpz);
            const float bnx = span_return(sr, rnx), bny = span_return(sr, rny), bnz = span_return(sr, rnz);
            const float bres = span_return(sr, rres);
            const int bstatus = span_return(sr, rstatus), bevals = span_return(sr, revals);
            if (covered) {
                pt[0] = bpx, pt[1] = bpy, pt[2] = bpz;
                wn[0] = bnx, wn[1] = bny, wn[2] = bnz;
                res = bres, status = bstatus, evals = bevals;
            }
        }
        if (live) {
            if (out_point) out_point[3 * n] = pt[0], out_point[3 * n + 1] = pt[1], out_point[3 * n + 2] = pt[2];
            if (out_normal) {
                float o[3] = {wn[0], wn[1], wn[2]};
                if (FRAME && covered) {
                    const long t = (long)(int)r.w;  // in [0, nf): texel_position said so
                    to_tangent_space(wn, r.x, r.y, r.z, corner_n + 9 * t, corner_t + 12 * t, o);
                }
                out_normal[3 * n] = o[0], out_normal[3 * n + 1] = o[1], out_normal[3 * n + 2] = o[2];
            }
            if (out_res) out_res[n] = res;
            if (out_status) out_status[n] = status;
            if (out_evals) out_evals[n] = evals;
            if (out_mask) out_mask[n] = covered ? 1 : 0;
        }
    }
}

}  // namespace sculpt

using namespace sculpt;

extern "C" int sculpt_bake_scene_surface(const float *planes_cl, int C, int H, int W, const void *mlp_packed, int n_hidden_64,
                                         const float *v_pos, size_t nv, const void *faces, int faces_i64, size_t nf, const float *rast,
                                         int res, float radius, const float *corner_normals, const float *corner_tangents, float target,
                                         int max_steps, float max_dist, float res_tol, float *point, float *normal, float *residual,
                                         int *status, int *evals, uint8_t *mask, sculpt_stream_t stream) {
    FieldPlan plan;
    if (const int e = field_plan("bake_scene_surface", C, planes_cl, mlp_packed, H, W, n_hidden_64, radius, plan, [&] {
            SC_REQUIRE(res >= 0, "bake_scene_surface: negative resolution");
            return 0;
        }))
        return e;
    SC_REQUIRE(nv <= (size_t)1 << 40 && nf <= (size_t)1 << 40, "bake_scene_surface: mesh too large");
    SC_REQUIRE((corner_normals == nullptr) == (corner_tangents == nullptr),
               "bake_scene_surface: corner_normals and corner_tangents come together (both or neither)");
    SC_REQUIRE(max_steps >= 0 && max_steps <= 64, "bake_scene_surface: max_steps=%d (0 .. 64)", max_steps);
    SC_REQUIRE(max_dist > 0.f && max_dist < INFINITY, "bake_scene_surface: max_dist=%g must be positive and finite", (double)max_dist);   // a NaN fails
    SC_REQUIRE(res_tol > 0.f && res_tol < INFINITY, "bake_scene_surface: res_tol=%g must be positive and finite", (double)res_tol);
    SC_REQUIRE(target == target, "bake_scene_surface: target is NaN");
    if (res == 0) return 0;
    if (!point && !normal && !residual && !status && !evals && !mask) return 0;   // nothing asked for
    SC_REQUIRE(rast, "bake_scene_surface: null rast");
    SC_REQUIRE(nf == 0 || (v_pos && faces && nv > 0), "bake_scene_surface: null mesh");
    auto kern = corner_normals ? bake_scene_surface_kernel<40, true> : bake_scene_surface_kernel<40, false>;
    const long N = (long)res * res;
    int grid;
    if (const int e = field_grid(plan, kern, (N + 63) / 64, grid)) return e;
    const float md2 = max_dist * max_dist;   // one fp32 product, as the rule states it
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), plan.lds, as_stream(stream), planes_cl, H, W,
                       reinterpret_cast<const float *>(mlp_packed), v_pos, (long)nv, faces, faces_i64, (long)nf,
                       reinterpret_cast<const float4 *>(rast), N, radius, plan.span, corner_normals, corner_tangents, target, max_steps,
                       md2, res_tol, point, normal, residual, status, evals, mask, plan.a0_lds);
    SC_LAUNCH_CHECK();
    return 0;
}
