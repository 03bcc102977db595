// Mesh vertices onto the iso-surface of the density field, for gfx950 (MI355X): a fused Newton iteration along the field's own
// gradient (sculpt_triplane_project) and the fold guard that follows it (sculpt_mesh_unfold).  The rule is DESIGN.md section
// 3.1e; tests/_projref.py restates both halves.  sculpt_triplane_project_along is the same tile searching along a given line
// (section 3.1h, tests/_dispref.py).
//
// project_kernel
//   * density_grad_kernel's tile (csrc/field_normal.hip): a wave is 8 points x {value, d/dx, d/dy, d/dz}, the weights are staged
//     in LDS once per workgroup (field_prologue, csrc/field_kernel.h), and one evaluation is field_eval_fwd (csrc/field_fwd.h),
//     the call that kernel makes, so the raw density d and the gradient g of an iterate are ops.field_normals' bits at that
//     iterate.
//   * after an evaluation the eight lanes of a point all hold d and g (three quad broadcasts; the two halves agree after
//     last_dot0_nobias's xor-shuffle) and run the rule redundantly in registers: current iterate, residual, masked gradient, best
//     iterate, trust region, status, evaluation count.  No LDS, no memory traffic between two steps.
//   * a point that has stopped keeps its state; its lanes go on evaluating with the wave (at the point they stopped at) and
//     ignore the result.  The loop leaves when a 64-bit ballot finds no lane active, at the latest after max_steps + 1
//     evaluations.  Nothing waits on another wave.
//   * the rule (rule_update, csrc/project_rule.h: csrc/bake_surface.hip runs the same copy) is compiled without contraction:
//     every value is a fixed sequence of IEEE fp32 operations, which torch restates one call per operation (tests/_projref.py
//     composed_device).  The evaluator keeps the contraction it has in field_normal.hip, or its bits would differ from that
//     kernel's.
//
// unfold kernels: fp32 without contraction (tests/_projref.py unfold restates them in NumPy bit for bit).
#include "common.h"
#include "field_fwd.h"
#include "project_rule.h"
#include "triplane_mlp.h"

namespace sculpt {

template <int C, bool AC>
__global__ __launch_bounds__(512) void project_kernel(
    const float *__restrict__ planes, int H, int W, const float *__restrict__ blob, const float *__restrict__ pts, long N,
    float radius, float span, float target, int K, float md2, float res_tol, float *__restrict__ out_pts,
    float *__restrict__ out_res, int *__restrict__ out_status, int *__restrict__ out_evals, int a0_lds) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FieldCtx c = field_prologue<C>(smem, blob, a0_lds);
    const int p = c.p, kind = p & 3;
    const bool is_value = kind == 0;
    const long ntiles = (N + 7) / 8;

    for (long tile = (long)blockIdx.x * c.nwave + c.wave; tile < ntiles; tile += (long)gridDim.x * c.nwave) {
        long n = tile * 8 + (p >> 2);
        const bool valid = n < N;
        if (!valid) n = N - 1;   // a copy of the last point: it runs the same steps and stores nothing
        const float p0x = pts[3 * n], p0y = pts[3 * n + 1], p0z = pts[3 * n + 2];
        const bool fx = fabsf(p0x) >= radius, fy = fabsf(p0y) >= radius, fz = fabsf(p0z) >= radius;
        ProjState s = proj_start(p0x, p0y, p0z, true);
        float qx = p0x, qy = p0y, qz = p0z;
        for (int k = 0; k <= K; ++k) {   // K <= 64 (checked at the entry): at most K + 1 evaluations
            const float sv = field_eval_fwd<C, AC>(c, planes, H, W, radius, span, a0_lds, kind, qx, qy, qz);
            const float d = quad_bcast<0>(sv) + c.L.blast[0];
            const float gx = quad_bcast<1>(sv), gy = quad_bcast<2>(sv), gz = quad_bcast<3>(sv);
            rule_update(s, k, K, d, gx, gy, gz, qx, qy, qz, p0x, p0y, p0z, fx, fy, fz, target, radius, md2, res_tol);
            if (__ballot(s.active) == 0ull) break;   // wave-uniform: all eight points have stopped
        }
        if (valid && is_value && c.h == 0) {
            out_pts[3 * n] = s.bx, out_pts[3 * n + 1] = s.by, out_pts[3 * n + 2] = s.bz;
            if (out_res) out_res[n] = s.br;
            if (out_status) out_status[n] = s.status;
            if (out_evals) out_evals[n] = s.evals;
        }
    }
}

// The line search of DESIGN.md section 3.1h in project_kernel's shape: the same tile, the same evaluation, the rule
// (line_update, csrc/project_rule.h) run redundantly by the eight lanes of a point, the loop left on a ballot.  The point count
// comes as a value or from device memory (`count`, clamped to 0 .. cap: the covered-texel list of csrc/bake_displacement.hip is
// made without a host wait); result i goes to row scatter[i] when a scatter list is given (rows outside 0 .. out_rows are
// dropped).  A point whose direction has no finite positive length never starts: status 3, height +0, no evaluation.
template <int C, bool AC>
__global__ __launch_bounds__(512) void project_along_kernel(
    const float *__restrict__ planes, int H, int W, const float *__restrict__ blob, const float *__restrict__ pts,
    const float *__restrict__ dirs, long cap, const int *__restrict__ count, float radius, float span, float target, int K,
    float max_dist, float res_tol, const int *__restrict__ scatter, long out_rows, float *__restrict__ out_height,
    float *__restrict__ out_res, int *__restrict__ out_status, int *__restrict__ out_evals, int a0_lds) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FieldCtx c = field_prologue<C>(smem, blob, a0_lds);

    long N = cap;
    if (count) {
        const long cn = (long)*count;
        N = cn < 0 ? 0 : (cn < cap ? cn : cap);
    }
    const int p = c.p, kind = p & 3;
    const bool is_value = kind == 0;
    const long ntiles = (N + 7) / 8;

    for (long tile = (long)blockIdx.x * c.nwave + c.wave; tile < ntiles; tile += (long)gridDim.x * c.nwave) {
        long n = tile * 8 + (p >> 2);
        const bool valid = n < N;
        if (!valid) n = N - 1;   // a copy of the last point (N >= 1 here): it runs the same steps and stores nothing
        const float p0x = pts[3 * n], p0y = pts[3 * n + 1], p0z = pts[3 * n + 2];
        float nx, ny, nz;
        const bool has_dir = line_direction(dirs[3 * n], dirs[3 * n + 1], dirs[3 * n + 2], nx, ny, nz);
        LineState s;
        s.s = s.bs = s.br = 0.f;
        s.a = s.b = 0.f;
        s.has_a = s.has_b = false;
        s.status = has_dir ? 1 : 3, s.evals = 0, s.active = has_dir;
        for (int k = 0; k <= K; ++k) {   // K <= 64 (checked at the entry): at most K + 1 evaluations
            float qx, qy, qz;
            line_point(p0x, p0y, p0z, nx, ny, nz, s.s, qx, qy, qz);
            const float sv = field_eval_fwd<C, AC>(c, planes, H, W, radius, span, a0_lds, kind, qx, qy, qz);
            const float d = quad_bcast<0>(sv) + c.L.blast[0];
            const float gx = quad_bcast<1>(sv), gy = quad_bcast<2>(sv), gz = quad_bcast<3>(sv);
            line_update(s, k, K, d, gx, gy, gz, p0x, p0y, p0z, nx, ny, nz, target, radius, max_dist, res_tol);
            if (__ballot(s.active) == 0ull) break;   // wave-uniform: all eight points have stopped
        }
        if (valid && is_value && c.h == 0) {
            const long o = scatter ? (long)scatter[n] : n;
            if (o >= 0 && o < out_rows) {
                out_height[o] = s.bs;
                if (out_res) out_res[o] = s.br;
                if (out_status) out_status[o] = s.status;
                if (out_evals) out_evals[o] = s.evals;
            }
        }
    }
}

}  // namespace sculpt

// ---------------------------------------------------------------------------------------------------------------------------
// the fold guard
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

#pragma clang fp contract(off)

constexpr int UNFOLD_BLOCK = 256;

// n = (b - a) x (c - a), each component two products and one difference
__device__ __forceinline__ void face_cross(const float *__restrict__ P, long a, long b, long c, float &nx, float &ny, float &nz) {
    const float ux = P[3 * b] - P[3 * a], uy = P[3 * b + 1] - P[3 * a + 1], uz = P[3 * b + 2] - P[3 * a + 2];
    const float vx = P[3 * c] - P[3 * a], vy = P[3 * c + 1] - P[3 * a + 1], vz = P[3 * c + 2] - P[3 * a + 2];
    nx = uy * vz - uz * vy;
    ny = uz * vx - ux * vz;
    nz = ux * vy - uy * vx;
}

__device__ __forceinline__ bool face_inverted(const float *__restrict__ P0, const float *__restrict__ P, long a, long b, long c) {
    float ax, ay, az, bx, by, bz;
    face_cross(P0, a, b, c, ax, ay, az);
    face_cross(P, a, b, c, bx, by, bz);
    const float n00 = (ax * ax + ay * ay) + az * az;
    const float n01 = (ax * bx + ay * by) + az * bz;
    return n00 > 0.f && n01 <= 0.f;   // a NaN fails both: such a face is left alone
}

// mark words: 0 = untouched, 1 = to revert in this round, 2 = reverted.  A face stores 1 into the words of its vertices that
// are not yet reverted: every writer of a word writes the same value, so the result does not depend on the order.
__global__ __launch_bounds__(UNFOLD_BLOCK) void unfold_mark_kernel(const float *__restrict__ P0, const float *__restrict__ P,
                                                                   const int64_t *__restrict__ F, long nv, long nf, int *__restrict__ mark) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int64_t a = F[3 * f], b = F[3 * f + 1], c = F[3 * f + 2];
    if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) return;   // a face that names no vertex is skipped
    if (!face_inverted(P0, P, a, b, c)) return;
    if (mark[a] != 2) mark[a] = 1;
    if (mark[b] != 2) mark[b] = 1;
    if (mark[c] != 2) mark[c] = 1;
}

// stats[slot] += the number of lanes with `one`, one atomic per wave
__device__ __forceinline__ void wave_count(int *__restrict__ stats, int slot, bool one) {
    const unsigned long long m = __ballot(one);
    if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(stats + slot, (int)__popcll(m));
}

__global__ __launch_bounds__(UNFOLD_BLOCK) void unfold_revert_kernel(const float *__restrict__ P0, float *__restrict__ P, long nv,
                                                                     int *__restrict__ mark, int *__restrict__ stats) {
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool hit = v < nv && mark[v] == 1;
    if (hit) {
        P[3 * v] = P0[3 * v], P[3 * v + 1] = P0[3 * v + 1], P[3 * v + 2] = P0[3 * v + 2];
        mark[v] = 2;
    }
    wave_count(stats, 0, hit);
}

__global__ __launch_bounds__(UNFOLD_BLOCK) void unfold_count_kernel(const float *__restrict__ P0, const float *__restrict__ P,
                                                                    const int64_t *__restrict__ F, long nv, long nf, int *__restrict__ stats) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool inv = false;
    if (f < nf) {
        const int64_t a = F[3 * f], b = F[3 * f + 1], c = F[3 * f + 2];
        if (!(a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv)) inv = face_inverted(P0, P, a, b, c);
    }
    wave_count(stats, 1, inv);
}

}  // namespace

using namespace sculpt;

extern "C" int sculpt_triplane_project(const float *planes_cl, int C, int H, int W, const void *mlp_packed, int n_hidden_64,
                                       const float *points, long long N, float radius, int flags, float target, int max_steps,
                                       float max_dist, float res_tol, float *out_points, float *out_residual, int *out_status,
                                       int *out_evals, sculpt_stream_t stream) {
    FieldPlan plan;
    if (const int e = field_plan("triplane_project", C, planes_cl, mlp_packed, H, W, n_hidden_64, radius, plan, [&] {
            SC_REQUIRE(N >= 0, "triplane_project: negative point count %lld", N);
            SC_REQUIRE((flags & ~(int)SCULPT_QUERY_ALIGN_CORNERS) == 0, "triplane_project: unknown flags %d", flags);
            return 0;
        }))
        return e;
    SC_REQUIRE(max_steps >= 0 && max_steps <= 64, "triplane_project: max_steps=%d (0 .. 64)", max_steps);
    SC_REQUIRE(max_dist > 0.f && max_dist < INFINITY, "triplane_project: max_dist=%g must be positive and finite", (double)max_dist);   // a NaN fails
    SC_REQUIRE(res_tol > 0.f && res_tol < INFINITY, "triplane_project: res_tol=%g must be positive and finite", (double)res_tol);
    SC_REQUIRE(target == target, "triplane_project: target is NaN");
    if (N == 0) return 0;   // empty arrays have no address: nothing to refuse, nothing to launch
    SC_REQUIRE(out_points, "triplane_project: null out_points");
    SC_REQUIRE(points, "triplane_project: null points");
    auto kern = (flags & (int)SCULPT_QUERY_ALIGN_CORNERS) ? project_kernel<40, true> : project_kernel<40, false>;
    int grid;
    if (const int e = field_grid(plan, kern, ((long)N + 7) / 8, grid)) return e;
    const float md2 = max_dist * max_dist;   // one fp32 product, as the rule states it
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), plan.lds, as_stream(stream), planes_cl, H, W,
                       reinterpret_cast<const float *>(mlp_packed), points, (long)N, radius, plan.span, target, max_steps, md2,
                       res_tol, out_points, out_residual, out_status, out_evals, plan.a0_lds);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sculpt_triplane_project_along(const float *planes_cl, int C, int H, int W, const void *mlp_packed, int n_hidden_64,
                                             const float *points, const float *directions, long long N, const int *count,
                                             float radius, int flags, float target, int max_steps, float max_dist, float res_tol,
                                             const int *scatter, long long out_rows, float *out_height, float *out_residual,
                                             int *out_status, int *out_evals, sculpt_stream_t stream) {
    FieldPlan plan;
    if (const int e = field_plan("triplane_project_along", C, planes_cl, mlp_packed, H, W, n_hidden_64, radius, plan, [&] {
            SC_REQUIRE(N >= 0, "triplane_project_along: negative point count %lld", N);
            SC_REQUIRE((flags & ~(int)SCULPT_QUERY_ALIGN_CORNERS) == 0, "triplane_project_along: unknown flags %d", flags);
            return 0;
        }))
        return e;
    SC_REQUIRE(max_steps >= 0 && max_steps <= 64, "triplane_project_along: max_steps=%d (0 .. 64)", max_steps);
    SC_REQUIRE(max_dist > 0.f && max_dist < INFINITY, "triplane_project_along: max_dist=%g must be positive and finite", (double)max_dist);   // a NaN fails
    SC_REQUIRE(res_tol > 0.f && res_tol < INFINITY, "triplane_project_along: res_tol=%g must be positive and finite", (double)res_tol);
    SC_REQUIRE(target == target, "triplane_project_along: target is NaN");
    SC_REQUIRE(scatter ? out_rows >= 0 : out_rows == N, "triplane_project_along: out_rows=%lld (the rows of the outputs; N without a scatter list)", out_rows);
    if (N == 0 || (scatter && out_rows == 0)) return 0;   // empty arrays have no address: nothing to refuse, nothing to launch
    SC_REQUIRE(out_height, "triplane_project_along: null out_height");
    SC_REQUIRE(points && directions, "triplane_project_along: null points or directions");
    auto kern = (flags & (int)SCULPT_QUERY_ALIGN_CORNERS) ? project_along_kernel<40, true> : project_along_kernel<40, false>;
    int grid;
    if (const int e = field_grid(plan, kern, ((long)N + 7) / 8, grid)) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), plan.lds, as_stream(stream), planes_cl, H, W,
                       reinterpret_cast<const float *>(mlp_packed), points, directions, (long)N, count, radius, plan.span, target,
                       max_steps, max_dist, res_tol, scatter, (long)out_rows, out_height, out_residual, out_status, out_evals,
                       plan.a0_lds);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sculpt_mesh_unfold(const float *P0, float *P, const int64_t *faces, int64_t Nv, int64_t Nf, int rounds, int *mark_ws,
                                  int *stats, sculpt_stream_t stream) {
    SC_REQUIRE(Nv >= 0 && Nv < ((int64_t)1 << 31) && Nf >= 0 && Nf < ((int64_t)1 << 31), "mesh_unfold: Nv=%lld, Nf=%lld out of range",
               (long long)Nv, (long long)Nf);
    SC_REQUIRE(rounds >= 0 && rounds <= 16, "mesh_unfold: rounds=%d (0 .. 16)", rounds);
    SC_REQUIRE(stats, "mesh_unfold: null stats");
    SC_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(int), as_stream(stream)));
    if (Nv == 0 || Nf == 0) return 0;
    SC_REQUIRE(P0 && P && faces, "mesh_unfold: null array");
    SC_REQUIRE(P0 != P, "mesh_unfold: P0 and P must be distinct arrays");
    SC_REQUIRE(rounds == 0 || mark_ws, "mesh_unfold: null mark workspace");
    hipStream_t st = as_stream(stream);
    const dim3 fgrid((unsigned)cdiv(Nf, UNFOLD_BLOCK)), vgrid((unsigned)cdiv(Nv, UNFOLD_BLOCK)), block(UNFOLD_BLOCK);
    if (rounds > 0) SC_HIP(hipMemsetAsync(mark_ws, 0, (size_t)Nv * sizeof(int), st));
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(unfold_mark_kernel, fgrid, block, 0, st, P0, P, faces, (long)Nv, (long)Nf, mark_ws);
        SC_LAUNCH_CHECK();
        hipLaunchKernelGGL(unfold_revert_kernel, vgrid, block, 0, st, P0, P, (long)Nv, mark_ws, stats);
        SC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(unfold_count_kernel, fgrid, block, 0, st, P0, P, faces, (long)Nv, (long)Nf, stats);
    SC_LAUNCH_CHECK();
    return 0;
}
