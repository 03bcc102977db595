// Mesh simplification ON THE DEVICE: quadric-error edge collapse (sculpt_rmd_qem_*, include/sculpt_hip.h; driven by
// sculptmate_amd/sf3d/remesh_device.py simplify_device).  The rounds are the device remesher's (csrc/remesh_device.hip): the
// topology is rebuilt from the faces, every candidate claims its footprint with a 64-bit atomicMin of (priority << 32 | edge
// id), a candidate that holds its whole footprint applies, winners share no vertex.  What this file adds is the metric:
//   vertex quadrics   Q[nv][10] fp64, the symmetric 4x4 matrix {aa ab ac ad bb bc bd cc cd dd} of Garland & Heckbert: per vertex
//                     the sum, in the order of its CSR corners, of the plane quadric (unit normal n, d = -n . p0) of every
//                     incident face; a gather, one thread per vertex, no float atomics.  Built once, then Q[kept] += Q[removed].
//   cost and target   per edge, q = Q[u] + Q[v]: the minimiser of the error when q's 3x3 block is regular and the edge is not
//                     on the border, else the best of p_u, p_v and the midpoint; the target rounded once to fp32 and stored,
//                     the cost = the error at that rounded point, clamped at 0; link condition and fold-over test
//   claim             only candidates whose key is at most the round's cap (a device scalar: the k-th smallest key)
//   apply             faces on the edge die, u -> v in the others, P[v] = the stored target, Q[v] += Q[u]
// Predicates in fp64 from the fp32 positions; the output does not depend on scheduling.
//
// The whole unit is compiled with floating-point contraction OFF (the pragma below, set before the shared helpers are
// included so that they obey it too): no multiply is fused with an add.  Every value is then a sequence of IEEE fp64
// operations in the order written, which tests/_qemref.py restates in NumPy operation for operation -- keys, targets and
// quadrics are compared bit for bit.
#pragma clang fp contract(off)

#include "remesh_topo.h"

namespace {

constexpr double kCollinear = 0.999;  // fold-over: the two edges at the target nearly on one line
constexpr double kMinNormalDot = 0.2;  // fold-over: new unit normal . current unit normal below this

// unit normal of face f, false when the face has none (zero or non-finite cross product)
__device__ inline bool unit_normal(const float *P, const int32_t *F, int f, D3 &n) {
    const D3 c = face_normal(P, F, f);
    const double l = norm(c);
    if (!(l > 0) || !isfinite(l)) return false;
    n = {c.x / l, c.y / l, c.z / l};
    return true;
}

__global__ void qem_quadrics_kernel(Topo T, const float *__restrict__ P, double *__restrict__ Q) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= T.nv) return;
    double q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = T.vfs[u]; j < T.vfs[u + 1]; ++j) {
        const int f = fan_face(T, j);
        D3 n;
        if (!unit_normal(P, T.F, f, n)) continue;  // a face without a normal contributes nothing
        const double d = -dot(n, ld(P, T.F[3 * f]));
        q[0] += n.x * n.x, q[1] += n.x * n.y, q[2] += n.x * n.z, q[3] += n.x * d;
        q[4] += n.y * n.y, q[5] += n.y * n.z, q[6] += n.y * d;
        q[7] += n.z * n.z, q[8] += n.z * d;
        q[9] += d * d;
    }
    for (int k = 0; k < 10; ++k) Q[10 * u + k] = q[k];
}

__device__ inline double det3(const double *m, int a11, int a12, int a13, int a21, int a22, int a23, int a31, int a32, int a33) {
    return m[a11] * m[a22] * m[a33] + m[a13] * m[a21] * m[a32] + m[a12] * m[a23] * m[a31] - m[a13] * m[a22] * m[a31] -
           m[a11] * m[a23] * m[a32] - m[a12] * m[a21] * m[a33];
}

__device__ inline double vertex_error(const double *q, double x, double y, double z) {
    return q[0] * x * x + 2 * q[1] * x * y + 2 * q[2] * x * z + 2 * q[3] * x + q[4] * y * y + 2 * q[5] * y * z + 2 * q[6] * y +
           q[7] * z * z + 2 * q[8] * z + q[9];
}

// the fan of x without the faces on the edge: false when moving x to p folds or flattens one of them
__device__ bool fan_keeps_shape(const Topo &T, const float *P, int x, int other, D3 p) {
    for (int j = T.vfs[x]; j < T.vfs[x + 1]; ++j) {
        const int f = fan_face(T, j);
        if (has(T.F, f, other)) continue;  // dies with the edge
        D3 n0;
        if (!unit_normal(P, T.F, f, n0)) continue;  // degenerate before the collapse: exempt
        const int k = T.vfc[j] - 3 * f;
        const D3 d1 = ld(P, T.F[3 * f + (k + 1) % 3]) - p, d2 = ld(P, T.F[3 * f + (k + 2) % 3]) - p;
        const double l1 = norm(d1), l2 = norm(d2);
        if (!(l1 > 0) || !(l2 > 0)) return false;  // the face would lose its normal
        const D3 e1 = {d1.x / l1, d1.y / l1, d1.z / l1}, e2 = {d2.x / l2, d2.y / l2, d2.z / l2};
        if (fabs(dot(e1, e2)) > kCollinear) return false;
        const D3 c = cross(e1, e2);
        const double lc = norm(c);
        if (!(lc > 0)) return false;
        const D3 n = {c.x / lc, c.y / lc, c.z / lc};
        if (dot(n, n0) < kMinNormalDot) return false;
    }
    return true;
}

__global__ void qem_cost_kernel(Topo T, const float *__restrict__ P, const double *__restrict__ Q, unsigned long long *__restrict__ cand,
                                float *__restrict__ tgt) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne) return;
    cand[e] = kNoClaim;
    for (int k = 0; k < 3; ++k) tgt[3 * e + k] = 0.0f;
    const int nef = T.es[e + 1] - T.es[e];
    if (nef != 1 && nef != 2) return;
    int u, v;  // u < v: u goes, v stays
    edge_ends(T, (int)e, u, v);
    if ((T.bnd[u] != 0) != (T.bnd[v] != 0)) return;
    double q[10];
    for (int k = 0; k < 10; ++k) q[k] = Q[10 * u + k] + Q[10 * v + k];
    float pf[3];
    double err;
    bool solved = false;
    const double det = det3(q, 0, 1, 2, 1, 4, 5, 2, 5, 7);
    if (!(T.bnd[u] && T.bnd[v]) && det != 0) {
        const double x = -1 / det * det3(q, 1, 2, 3, 4, 5, 6, 5, 7, 8);
        const double y = 1 / det * det3(q, 0, 2, 3, 1, 5, 6, 2, 7, 8);
        const double z = -1 / det * det3(q, 0, 1, 3, 1, 4, 6, 2, 5, 8);
        pf[0] = (float)x, pf[1] = (float)y, pf[2] = (float)z;
        solved = isfinite(pf[0]) && isfinite(pf[1]) && isfinite(pf[2]);
        if (solved) err = vertex_error(q, (double)pf[0], (double)pf[1], (double)pf[2]);
    }
    if (!solved) {
        float pm[3];
        midpoint(P, u, v, pm);
        const D3 pu = ld(P, u), pv = ld(P, v);
        const double e1 = vertex_error(q, pu.x, pu.y, pu.z), e2 = vertex_error(q, pv.x, pv.y, pv.z);
        const double e3 = vertex_error(q, (double)pm[0], (double)pm[1], (double)pm[2]);
        if (e1 <= e2 && e1 <= e3) {
            err = e1;
            for (int k = 0; k < 3; ++k) pf[k] = P[3 * u + k];
        } else if (e2 <= e3) {
            err = e2;
            for (int k = 0; k < 3; ++k) pf[k] = P[3 * v + k];
        } else {
            err = e3;
            for (int k = 0; k < 3; ++k) pf[k] = pm[k];
        }
    }
    if (!isfinite(err)) return;  // inf - inf in the error of huge coordinates: no candidate, never the cheapest one
    if (!link_ok(T, u, v, (int)e)) return;
    const D3 p = {(double)pf[0], (double)pf[1], (double)pf[2]};
    if (!fan_keeps_shape(T, P, u, v, p) || !fan_keeps_shape(T, P, v, u, p)) return;
    const float cost = err > 0 ? (float)err : 0.0f;  // non-negative fp32 bits order like the values
    cand[e] = ((unsigned long long)__float_as_uint(cost) << 32) | (unsigned long long)e;
    for (int k = 0; k < 3; ++k) tgt[3 * e + k] = pf[k];
}

__global__ void qem_claim_kernel(Topo T, const unsigned long long *__restrict__ cand, const unsigned long long *__restrict__ cap,
                                 unsigned long long *__restrict__ claim) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne) return;
    const unsigned long long key = cand[e];
    if (key == kNoClaim || key > *cap) return;
    int u, v;
    edge_ends(T, (int)e, u, v);
    for (int side = 0; side < 2; ++side) {
        const int x = side ? v : u;
        for (int j = T.vfs[x]; j < T.vfs[x + 1]; ++j) {
            const int f = fan_face(T, j);
            for (int k = 0; k < 3; ++k) atomicMin(&claim[T.F[3 * f + k]], key);
        }
    }
}

// the winners (sculpt_rmd_collapse_select, mode 0: the same footprint): no other winner reads or writes u, v, their faces or
// their rows of P and Q
__global__ void qem_apply_kernel(Topo T, float *__restrict__ P, int32_t *__restrict__ F, double *__restrict__ Q, const float *__restrict__ tgt,
                                 const int32_t *__restrict__ win, uint8_t *__restrict__ falive) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne || win[e] == 0) return;
    int u, v;
    edge_ends(T, (int)e, u, v);
    for (int j = T.vfs[u]; j < T.vfs[u + 1]; ++j) {
        const int f = fan_face(T, j);
        const int ku = T.vfc[j] - 3 * f;
        if (has(F, f, v))
            falive[f] = 0;
        else
            F[3 * f + ku] = v;
    }
    for (int k = 0; k < 3; ++k) P[3 * v + k] = tgt[3 * e + k];
    for (int k = 0; k < 10; ++k) Q[10 * v + k] += Q[10 * u + k];
}

}  // namespace

extern "C" {

int sculpt_rmd_qem_quadrics(const sculpt_rmd_topo_t *topo, const float *P, double *Q, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_qem_quadrics")) return rc;
    SC_REQUIRE(topo->nv == 0 || (P && Q), "rmd_qem_quadrics: null positions or quadrics");
    if (topo->nf == 0) {  // no face: every quadric is zero, and the CSR may be absent
        if (topo->nv > 0) SC_HIP(hipMemsetAsync(Q, 0, (size_t)topo->nv * 10 * sizeof(double), as_stream(stream)));
        return 0;
    }
    RMD_LAUNCH(qem_quadrics_kernel, topo->nv, topo_of(topo), P, Q);
    return 0;
}

int sculpt_rmd_qem_cost(const sculpt_rmd_topo_t *topo, const float *P, const double *Q, unsigned long long *cand, float *target,
                        sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_qem_cost")) return rc;
    SC_REQUIRE(topo->ne == 0 || (P && Q && cand && target), "rmd_qem_cost: null array");
    RMD_LAUNCH(qem_cost_kernel, topo->ne, topo_of(topo), P, Q, cand, target);
    return 0;
}

int sculpt_rmd_qem_claim(const sculpt_rmd_topo_t *topo, const unsigned long long *cand, const unsigned long long *cap,
                         unsigned long long *claim, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_qem_claim")) return rc;
    SC_REQUIRE(topo->ne == 0 || (cand && cap && claim), "rmd_qem_claim: null array");
    RMD_LAUNCH(qem_claim_kernel, topo->ne, topo_of(topo), cand, cap, claim);
    return 0;
}

int sculpt_rmd_qem_apply(const sculpt_rmd_topo_t *topo, float *P, int32_t *F, double *Q, const float *target, const int32_t *win,
                         uint8_t *face_alive, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_qem_apply")) return rc;
    SC_REQUIRE(F == topo->F, "rmd_qem_apply: F must be the topology's face array");
    SC_REQUIRE(topo->ne == 0 || (P && Q && target && win && face_alive), "rmd_qem_apply: null array");
    RMD_LAUNCH(qem_apply_kernel, topo->ne, topo_of(topo), P, F, Q, target, win, face_alive);
    return 0;
}

}  // extern "C"
