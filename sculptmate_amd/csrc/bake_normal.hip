// Normal-map bake of a TripoSR scene code for gfx950 (MI355X): rasterised UV atlas -> the density field's unit normal per covered
// texel, in object space or in the tangent frame of the low-poly mesh, one launch; and the per-corner tangent frames it reads.
//
// Shape:
//   * bake_scene_normal_kernel.  A wave owns a SPAN of 64 consecutive texels, one per lane.  It computes the texel's position
//     with texel_position (bake_texel.h: the bits of bake_scene_color_kernel and bake_interpolate_kernel), ballots the coverage
//     and hands both to the span compaction of field_fwd.h (span_compact .. span_return: the covered positions to the low lanes
//     in rank order, ceil(count / 8) tiles over ranks 8k .. 8k + 7, every result back to its texel's lane).  A tile is one
//     field_eval_fwd -- 8 points x {value, d/dx, d/dy, d/dz}, the call density_grad_kernel (csrc/field_normal.hip) makes --
//     and unit_normal_of.  A span with no covered texel runs no tile and stores zeros.  Columns past `count` in the last tile
//     evaluate an uncovered texel's position (the box centre); nothing of theirs is stored.
//   * a column's bits depend on that column alone (an MFMA column reads its own B column), so a covered texel's world normal is
//     the `normal` of sculpt_triplane_density_grad at the position of sculpt_bake_interpolate, bit for bit, wherever in which
//     span the texel sits.
//   * 512 threads, hidden weights (and layer 0's, when they fit) in LDS: field_prologue and the launch plan of field_kernel.h,
//     as in density_grad_kernel; the compaction uses lane permutes, no LDS of its own.
//
// The tangent-space transform (frame given), per covered texel with barycentrics (u, v, w), face t, corner rows 3t, 3t+1, 3t+2 and
// world normal n; every operation rounded on its own (contraction off), in this order:
//     N_c = (N0_c*u + N1_c*v) + N2_c*w,  T_c = (T0_c*u + T1_c*v) + T2_c*w           c = x, y, z     (un-normalised, MikkTSpace)
//     C   = (N_y*T_z - N_z*T_y,  N_z*T_x - N_x*T_z,  N_x*T_y - N_y*T_x),  B = s*C,  s = corner_tangents[3t].w
//     dot(a, b) = (a_x*b_x + a_y*b_y) + a_z*b_z
//     gtt = dot(T,T), gnn = dot(N,N), gtn = dot(T,N), D = gtt*gnn - gtn*gtn
//     nT = dot(n,T), nN = dot(n,N), nB = dot(n,B)
//     x = nT*gnn - nN*gtn,  y = nB,  z = nN*gtt - nT*gtn
//     len = sqrt((x*x + y*y) + z*z);  stored = (x/len, y/len, z/len)
//   so that normalize(x*T + y*B + z*N) is n (B is perpendicular to N and T and B.B = D: the 3 x 3 system needs no division).
//   The flat (0, 0, 1) is stored when !(D > 0), when !(0 < len < inf) (which catches every non-finite component) or when n is 0.
//
// corner_tangents_kernel, one thread per face, contraction off, with p0 p1 p2 the face's vertices and uv0 uv1 uv2 its corners' uvs:
//     e1 = p1 - p0, e2 = p2 - p0, (du1, dv1) = uv1 - uv0, (du2, dv2) = uv2 - uv0,  det = du1*dv2 - du2*dv1
//     t_c = (e1_c*dv2 - e2_c*dv1) / det,  b_c = (e2_c*du1 - e1_c*du2) / det                          (dP/du and dP/dv)
//     per corner i with normal N:  d = dot(N,t),  q_c = t_c - N_c*d,  l = sqrt(dot(q,q)),  T = q / l,
//                                  w = dot(cross(N,T), b) >= 0 ? +1 : -1
//   Degenerate: when !(0 < |det| < inf), a vertex index is out of range (nothing is read through it) or !(0 < l < inf), the corner
//   gets T = normalize(cross(N, e_a)), a = the axis of N's smallest component in magnitude (the lowest axis on a tie), and w = +1;
//   if that is no finite unit vector either (N is 0 or not finite) it gets (1, 0, 0, +1).
#include "bake_texel.h"
#include "common.h"
#include "field_fwd.h"
#include "tangent_frame.h"
#include "triplane_mlp.h"

namespace sculpt {

template <int C, bool FRAME>
__global__ __launch_bounds__(512) void bake_scene_normal_kernel(
    const float *__restrict__ planes, int H, int W, const float *__restrict__ blob, const float *__restrict__ v_pos, long nv,
    const void *__restrict__ faces, int faces_i64, long nf, const float4 *__restrict__ rast, long N, float radius, float span_w,
    const float *__restrict__ corner_n, const float *__restrict__ corner_t, float *__restrict__ normal, uint8_t *__restrict__ mask,
    int a0_lds) {
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
        float wn[3] = {0.f, 0.f, 0.f};
        if (m != 0) {  // wave-uniform
            const SpanRanks sr = span_compact(m, covered, lane, tx.x);
            float rx = 0.f, ry = 0.f, rz = 0.f;  // the normal of rank `lane`
            for (int k = 0; k < span_tiles(sr); ++k) {
                float px, py, pz;
                span_tile_point(sr, k, p, px, py, pz);
                const float s = field_eval_fwd<C, false>(c, planes, H, W, radius, span_w, a0_lds, kind, px, py, pz);
                float nx, ny, nz;
                unit_normal_of(quad_bcast<1>(s), quad_bcast<2>(s), quad_bcast<3>(s), nx, ny, nz);
                const float qx = span_gather(nx, lane), qy = span_gather(ny, lane), qz = span_gather(nz, lane);
                if (span_keeps(k, lane)) { rx = qx; ry = qy; rz = qz; }
            }
            const float bx = span_return(sr, rx), by = span_return(sr, ry), bz = span_return(sr, rz);
            if (covered) { wn[0] = bx; wn[1] = by; wn[2] = bz; }
        }
        if (live) {
            float o[3] = {wn[0], wn[1], wn[2]};
            if (FRAME && covered) {
                const long t = (long)(int)r.w;  // in [0, nf): texel_position said so
                to_tangent_space(wn, r.x, r.y, r.z, corner_n + 9 * t, corner_t + 12 * t, o);
            }
            normal[3 * n] = o[0];
            normal[3 * n + 1] = o[1];
            normal[3 * n + 2] = o[2];
            if (mask) mask[n] = covered ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(256) void corner_tangents_kernel(const float *__restrict__ v_pos, long nv, const void *__restrict__ faces,
                                                              int faces_i64, long nf, const float *__restrict__ uvs,
                                                              const float *__restrict__ corner_n, float *__restrict__ out) {
#pragma clang fp contract(off)
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    long i[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        i[k] = faces_i64 ? (long)reinterpret_cast<const long long *>(faces)[3 * f + k] : (long)reinterpret_cast<const int *>(faces)[3 * f + k];
    const bool in_range = i[0] >= 0 && i[0] < nv && i[1] >= 0 && i[1] < nv && i[2] >= 0 && i[2] < nv;
    float t[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f};
    bool face_ok = false;
    if (in_range) {
        const float du1 = uvs[6 * f + 2] - uvs[6 * f], dv1 = uvs[6 * f + 3] - uvs[6 * f + 1];
        const float du2 = uvs[6 * f + 4] - uvs[6 * f], dv2 = uvs[6 * f + 5] - uvs[6 * f + 1];
        const float det = du1 * dv2 - du2 * dv1;
        face_ok = positive_finite(fabsf(det));
        if (face_ok) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float e1 = v_pos[3 * i[1] + c] - v_pos[3 * i[0] + c], e2 = v_pos[3 * i[2] + c] - v_pos[3 * i[0] + c];
                t[c] = (e1 * dv2 - e2 * dv1) / det;
                b[c] = (e2 * du1 - e1 * du2) / det;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *np = corner_n + 9 * f + 3 * k;
        const float Nn[3] = {np[0], np[1], np[2]};
        float T[3] = {1.f, 0.f, 0.f}, w = 1.f;
        bool done = false;
        if (face_ok) {
            const float d = dot3_nc(Nn, t);
            const float q[3] = {t[0] - Nn[0] * d, t[1] - Nn[1] * d, t[2] - Nn[2] * d};
            const float l = sqrtf(dot3_nc(q, q));
            if (positive_finite(l)) {
                T[0] = q[0] / l; T[1] = q[1] / l; T[2] = q[2] / l;
                float c[3];
                cross3_nc(Nn, T, c);
                w = dot3_nc(c, b) >= 0.f ? 1.f : -1.f;
                done = true;
            }
        }
        if (!done) {
            const float ax = fabsf(Nn[0]), ay = fabsf(Nn[1]), az = fabsf(Nn[2]);
            const int a = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
            const float e[3] = {a == 0 ? 1.f : 0.f, a == 1 ? 1.f : 0.f, a == 2 ? 1.f : 0.f};
            float c[3];
            cross3_nc(Nn, e, c);
            const float l = sqrtf(dot3_nc(c, c));
            if (positive_finite(l)) { T[0] = c[0] / l; T[1] = c[1] / l; T[2] = c[2] / l; }
        }
        float *o = out + 12 * f + 4 * k;
        o[0] = T[0]; o[1] = T[1]; o[2] = T[2]; o[3] = w;
    }
}

}  // namespace sculpt

using namespace sculpt;

extern "C" int sculpt_corner_tangents(const float *v_pos, size_t nv, const void *faces, int faces_i64, size_t nf, const float *uvs,
                                      const float *corner_normals, float *tangents, sculpt_stream_t stream) {
    SC_REQUIRE(nv <= (size_t)1 << 40 && nf <= (size_t)1 << 40, "corner_tangents: mesh too large");
    if (nf == 0) return 0;
    SC_REQUIRE(v_pos && faces && uvs && corner_normals && tangents, "corner_tangents: null input");
    const long blocks = ((long)nf + 255) / 256;
    SC_REQUIRE(blocks <= 0x7fffffffL, "corner_tangents: mesh too large");
    hipLaunchKernelGGL(corner_tangents_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), v_pos, (long)nv, faces,
                       faces_i64, (long)nf, uvs, corner_normals, tangents);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sculpt_bake_scene_normal(const float *planes_cl, int C, int H, int W, const void *mlp_packed, int n_hidden_64,
                                        const float *v_pos, size_t nv, const void *faces, int faces_i64, size_t nf, const float *rast,
                                        int res, float radius, const float *corner_normals, const float *corner_tangents,
                                        float *normal, uint8_t *mask, sculpt_stream_t stream) {
    FieldPlan plan;
    if (const int e = field_plan("bake_scene_normal", C, planes_cl, mlp_packed, H, W, n_hidden_64, radius, plan, [&] {
            SC_REQUIRE(res >= 0, "bake_scene_normal: negative resolution");
            return 0;
        }))
        return e;
    SC_REQUIRE(nv <= (size_t)1 << 40 && nf <= (size_t)1 << 40, "bake_scene_normal: mesh too large");
    SC_REQUIRE((corner_normals == nullptr) == (corner_tangents == nullptr),
               "bake_scene_normal: corner_normals and corner_tangents come together (both or neither)");
    if (res == 0) return 0;
    SC_REQUIRE(rast && normal, "bake_scene_normal: null rast or normal");
    SC_REQUIRE(nf == 0 || (v_pos && faces && nv > 0), "bake_scene_normal: null mesh");
    auto kern = corner_normals ? bake_scene_normal_kernel<40, true> : bake_scene_normal_kernel<40, false>;
    const long N = (long)res * res;
    int grid;
    if (const int e = field_grid(plan, kern, (N + 63) / 64, grid)) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), plan.lds, as_stream(stream), planes_cl, H, W,
                       reinterpret_cast<const float *>(mlp_packed), v_pos, (long)nv, faces, faces_i64, (long)nf,
                       reinterpret_cast<const float4 *>(rast), N, radius, plan.span, corner_normals, corner_tangents, normal, mask,
                       plan.a0_lds);
    SC_LAUNCH_CHECK();
    return 0;
}
