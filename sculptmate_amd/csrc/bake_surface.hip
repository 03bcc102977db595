// Bake at the surface, for gfx950 (MI355X): rasterised UV atlas -> per covered texel the point of the density field's iso-surface
// d(p) = target that the projection rule reaches from the texel's point on the low-poly face, and the field's unit normal THERE,
// in object space or in the tangent frame of the low-poly mesh; one launch (sculpt_bake_scene_surface).
//
// bake_scene_surface_kernel is three kernels the project already has, fused:
//   * the span compaction of bake_scene_normal_kernel (csrc/bake_normal.hip): a wave owns 64 consecutive texels, one per lane;
//     texel_position (bake_texel.h) gives p0 and the coverage; ballot, mbcnt rank and one ds_permute per coordinate bring the
//     covered p0 to the low lanes in rank order; the wave then runs ceil(count / 8) forward-mode tiles of field_fwd.h over ranks
//     8k .. 8k + 7.  An empty span runs no tile.
//   * the loop of project_kernel (csrc/mesh_project.hip) inside each tile: one evaluation is density_grad_kernel's sequence of
//     operations, the eight lanes of a point all hold (d, g) afterwards and run rule_update (csrc/project_rule.h, the one copy of
//     the rule) redundantly in registers.  The loop leaves when a ballot finds no lane of the tile active, at the latest after
//     max_steps + 1 evaluations.  Columns past `count` in the last tile start inactive: they evaluate with the wave (at the box
//     centre, an uncovered texel's position) and take no step, so they never keep the tile in the loop.
//   * the normal at the point the rule returns.  rule_update says when the evaluated candidate became the best iterate; the
//     lanes then keep that evaluation's RAW gradient (the rule itself masks frozen axes; the normal does not), and after the loop
//     unit_normal_of (field_fwd.h) of the kept gradient is sculpt_triplane_density_grad's `normal` at the returned point, bit
//     for bit: it is the same evaluation at the same point, and a column's bits depend on that column alone.  No further
//     evaluation is run.
//   After the last tile the nine results of a rank (point, normal, residual, status, evals) return to their texel's lane by
//   ds_bpermute through the compaction's permutation; the frame transform (to_tangent_space, csrc/tangent_frame.h, at the texel's
//   own barycentrics: the low-poly face and its interpolated frame do not move) and the stores happen there.
//   * 512 threads, hidden weights (and layer 0's, when they fit) in LDS once per workgroup as in density_grad_kernel; the
//     compaction uses lane permutes, no LDS of its own.  Nothing waits on another wave.
//
// Uncovered texels: point, normal and residual exactly +0, status -1, evals 0, mask 0.  A texel's outputs depend on that texel
// alone.
#include <algorithm>

#include "bake_texel.h"
#include "common.h"
#include "field_fwd.h"
#include "project_rule.h"
#include "tangent_frame.h"
#include "triplane_mlp.h"

namespace sculpt {

__device__ __forceinline__ float shfl_f(float v, int src) { return __shfl(v, src, 64); }

__device__ __forceinline__ float bpermute_f(int byte_addr, float v) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(byte_addr, __float_as_int(v)));
}

template <int C, bool FRAME>
__global__ __launch_bounds__(512) void bake_scene_surface_kernel(
    const float *__restrict__ planes, int H, int W, const float *__restrict__ blob, const float *__restrict__ v_pos, long nv,
    const void *__restrict__ faces, int faces_i64, long nf, const float4 *__restrict__ rast, long N, float radius, float span_w,
    const float *__restrict__ corner_n, const float *__restrict__ corner_t, float target, int K, float md2, float res_tol,
    float *__restrict__ out_point, float *__restrict__ out_normal, float *__restrict__ out_res, int *__restrict__ out_status,
    int *__restrict__ out_evals, uint8_t *__restrict__ out_mask, int a0_lds) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpPackHeader hd = *reinterpret_cast<const MlpPackHeader *>(blob);
    const int NH = hd.NH;
    float *a0s = smem + lds_floats_for(NH);
    if (a0_lds) stage_a0_in_lds<C>(a0s, blob, hd);
    load_weights_to_lds(smem, blob, hd);
    const LdsView L = lds_view(smem, NH);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int p = lane & 31, h = lane >> 5;
    const int kind = p & 3;
    const bool is_value = kind == 0;
    const long nspans = (N + 63) / 64;
    const float *A0g = blob + hd.off_a0;
    const long HW = (long)H * W;
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    for (long sp = (long)blockIdx.x * nwave + wave; sp < nspans; sp += (long)gridDim.x * nwave) {
        const long n = sp * 64 + lane;
        const bool live = n < N;
        const float4 r = rast[live ? n : N - 1];
        const Texel tx = texel_position(r, v_pos, nv, faces, faces_i64, nf);
        const bool covered = live && tx.covered;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(covered);
        float pt[3] = {0.f, 0.f, 0.f}, wn[3] = {0.f, 0.f, 0.f}, res = 0.f;
        int status = -1, evals = 0;
        if (m != 0) {  // wave-uniform
            const int count = __popcll(m);
            const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            const int slot = covered ? below : count + (lane - below);  // a permutation of 0 .. 63
            // lane `rank` <- the position of the covered texel of that rank
            const float cx = __int_as_float(__builtin_amdgcn_ds_permute(slot * 4, __float_as_int(tx.x[0])));
            const float cy = __int_as_float(__builtin_amdgcn_ds_permute(slot * 4, __float_as_int(tx.x[1])));
            const float cz = __int_as_float(__builtin_amdgcn_ds_permute(slot * 4, __float_as_int(tx.x[2])));
            // what rank `lane` ends with
            float rpx = 0.f, rpy = 0.f, rpz = 0.f, rnx = 0.f, rny = 0.f, rnz = 0.f, rres = 0.f;
            int rstatus = -1, revals = 0;
            const int ntile = (count + 7) >> 3;  // <= 8
            for (int t = 0; t < ntile; ++t) {
                const int src = t * 8 + (p >> 2);  // < 64
                const float p0x = shfl_f(cx, src), p0y = shfl_f(cy, src), p0z = shfl_f(cz, src);
                const bool fx = fabsf(p0x) >= radius, fy = fabsf(p0y) >= radius, fz = fabsf(p0z) >= radius;
                ProjState s;
                s.px = s.bx = p0x, s.py = s.by = p0y, s.pz = s.bz = p0z;
                s.r = s.br = 0.f;
                s.gx = s.gy = s.gz = 0.f;
                s.status = 1, s.evals = 0, s.active = src < count;  // a column past the last covered texel takes no step
                float qx = p0x, qy = p0y, qz = p0z;
                float bgx = 0.f, bgy = 0.f, bgz = 0.f;  // the raw gradient at the best iterate
                for (int k = 0; k <= K; ++k) {  // K <= 64 (checked at the entry): at most K + 1 evaluations
                    int off[3][4];
                    float wt[3][4];
                    point_taps<false>(qx, qy, qz, radius, span_w, H, W, off, wt);
                    tangent_weights<false>(kind, qx, qy, qz, radius, span_w, H, W, wt);
                    f32x16 x0 = is_value ? lds_bias16(L.bacc, 0, h, 0) : zero;
                    f32x16 x1 = is_value ? lds_bias16(L.bacc, 0, h, 1) : zero;
                    layer0_channel_last<C>(planes, HW, off, wt, a0s, A0g, a0_lds, lane, h, x0, x1);
                    hidden_layers_fwd(L, NH, lane, h, is_value, x0, x1);
                    const float sv = last_dot0_nobias(L, h, x0, x1);
                    const float d = quad_bcast<0>(sv) + L.blast[0];
                    const float gx = quad_bcast<1>(sv), gy = quad_bcast<2>(sv), gz = quad_bcast<3>(sv);
                    if (rule_update(s, k, K, d, gx, gy, gz, qx, qy, qz, p0x, p0y, p0z, fx, fy, fz, target, radius, md2, res_tol))
                        bgx = gx, bgy = gy, bgz = gz;
                    if (__ballot(s.active) == 0ull) break;  // wave-uniform: all eight points have stopped
                }
                float nx, ny, nz;
                unit_normal_of(bgx, bgy, bgz, nx, ny, nz);
                // point j of the tile sits in lane 4 j: into lane 8 t + j
                const int from = 4 * (lane & 7);
                const float gpx = shfl_f(s.bx, from), gpy = shfl_f(s.by, from), gpz = shfl_f(s.bz, from);
                const float gnx = shfl_f(nx, from), gny = shfl_f(ny, from), gnz = shfl_f(nz, from);
                const float gres = shfl_f(s.br, from);
                const int gstatus = __shfl(s.status, from, 64), gevals = __shfl(s.evals, from, 64);
                if ((lane >> 3) == t) {
                    rpx = gpx, rpy = gpy, rpz = gpz;
                    rnx = gnx, rny = gny, rnz = gnz;
                    rres = gres, rstatus = gstatus, revals = gevals;
                }
            }
            // back to the texel's own lane
            const int back = slot * 4;
            const float bpx = bpermute_f(back, rpx), bpy = bpermute_f(back, rpy), bpz = bpermute_f(back, rpz);
            const float bnx = bpermute_f(back, rnx), bny = bpermute_f(back, rny), bnz = bpermute_f(back, rnz);
            const float bres = bpermute_f(back, rres);
            const int bstatus = __builtin_amdgcn_ds_bpermute(back, rstatus), bevals = __builtin_amdgcn_ds_bpermute(back, revals);
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
    SC_REQUIRE(C == 40, "bake_scene_surface: built for C=40 channels per plane (got %d)", C);
    SC_REQUIRE(planes_cl && mlp_packed, "bake_scene_surface: null input");
    SC_REQUIRE(H >= 1 && W >= 1, "bake_scene_surface: bad plane size %d x %d", H, W);
    SC_REQUIRE(res >= 0, "bake_scene_surface: negative resolution");
    SC_REQUIRE(n_hidden_64 >= 0, "bake_scene_surface: bad n_hidden_64");
    SC_REQUIRE(radius > 0.f, "bake_scene_surface: radius must be positive");
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
    size_t lds = (size_t)lds_floats_for(n_hidden_64) * sizeof(float);
    SC_REQUIRE(lds <= 160 * 1024, "bake_scene_surface: %d hidden layers do not fit LDS", n_hidden_64);
    const size_t a0_bytes = (size_t)3 * C * 64 * sizeof(float);
    const int a0_lds = lds + a0_bytes <= 160 * 1024 ? 1 : 0;
    if (a0_lds) lds += a0_bytes;
    auto kern = corner_normals ? bake_scene_surface_kernel<40, true> : bake_scene_surface_kernel<40, false>;
    SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long N = (long)res * res;
    const long nspans = (N + 63) / 64;
    const int grid = (int)std::min<long>((nspans + 7) / 8, num_cus());
    const float span = (float)((double)radius - (double)(-radius));
    const float md2 = max_dist * max_dist;   // one fp32 product, as the rule states it
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, as_stream(stream), planes_cl, H, W,
                       reinterpret_cast<const float *>(mlp_packed), v_pos, (long)nv, faces, faces_i64, (long)nf,
                       reinterpret_cast<const float4 *>(rast), N, radius, span, corner_normals, corner_tangents, target, max_steps, md2,
                       res_tol, point, normal, residual, status, evals, mask, a0_lds);
    SC_LAUNCH_CHECK();
    return 0;
}
