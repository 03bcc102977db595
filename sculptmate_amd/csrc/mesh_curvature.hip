// Discrete curvature ON THE DEVICE after Meyer, Desbrun, Schroeder, Barr 2003 (sculpt_curvature_*, sculpt_surface_attribute_at,
// include/sculpt_hip.h; driven by sculptmate_amd/sf3d/remesh_device.py curvature_device).  The faces do not change,
// so everything topological is the one topology of the call (sculpt_rmd_topo_t with the boundary flags of a zero carry) and, for
// the rings, the neighbour table of the smoothing filter; every kernel is a pure gather, one thread per vertex or point:
//   terms     per vertex u, its corners in vfc order (ascending corner index).  Corner c of face t = (i, j, k) in the face's own
//             cyclic order seen from i = u, positions fp32 widened to fp64:
//                 e1 = pj - pi, e2 = pk - pi, g = e1 x e2, a2 = sqrt(g . g); unless 0 < a2 < inf the corner adds nothing
//                 di = e1 . e2, dj = (pi - pj) . (pk - pj), dk = (pi - pk) . (pj - pk), cot_j = dj / a2, cot_k = dk / a2
//                 theta = atan2(a2, di)
//                 area: none of di, dj, dk < 0: ((e1 . e1) cot_k + (e2 . e2) cot_j) / 8; else di < 0: a2 / 4; else a2 / 8
//                 Kv += cot_k (pi - pj) + cot_j (pi - pk) per component; N += g; A += area; Th += theta; n += 1
//             valid = no edge at u without exactly two faces (bnd[u] == 0), a face names u, and A > 0.  A valid vertex writes
//                 area = A, deficit = 6.283185307179586 - Th, hint = outward sign(Kv . N) sqrt(Kv . Kv) / 4   (= H A, the integrated
//             mean curvature; Kv = 4 H A n); an invalid one writes zeros.
//   ring      one round: X'_u = X_u + sum of X_v over the VALID v of row u of the neighbour table, in row order, for the three
//             channels (hint, deficit, area); an invalid u stays zero.  It reads one buffer and writes the other.
//   finish    H = (float)(hint / area), K = (float)(deficit / area), NaN where invalid.
//   attribute a value per vertex read at a point of a face by clamped barycentric weights (below).
// The unit is compiled with floating-point contraction OFF (the pragma below, before the shared helpers): every value is a fixed
// sequence of IEEE fp64 operations, which tests/_curvref.py restates in NumPy operation for operation; only atan2 is the
// device library's own.  No atomics, no LDS, any valence.
#pragma clang fp contract(off)

#include "remesh_topo.h"

namespace {

constexpr double kTwoPi = 6.283185307179586;
constexpr int kMaxChannels = 8;

struct __attribute__((aligned(32))) Row {  // one vertex of the ring rounds: two 16-byte loads
    double hint, deficit, area, valid;
};

__global__ void curvature_pack_kernel(const float *__restrict__ P, long nv, float4 *__restrict__ p4) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nv) return;
    p4[u] = make_float4(P[3 * u], P[3 * u + 1], P[3 * u + 2], 0.0f);
}

__device__ inline D3 ld4(const float4 *__restrict__ p4, int i) {
    const float4 p = p4[i];
    return {(double)p.x, (double)p.y, (double)p.z};
}

__global__ void curvature_terms_kernel(Topo T, const float4 *__restrict__ p4, double outward, double *__restrict__ area,
                                       double *__restrict__ deficit, double *__restrict__ hint, uint8_t *__restrict__ valid) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= T.nv) return;
    const int b = T.vfs[u], e = T.vfs[u + 1];
    double A = 0.0, Th = 0.0;
    D3 Kv = {0.0, 0.0, 0.0}, N = {0.0, 0.0, 0.0};
    const D3 pi = ld4(p4, (int)u);
    for (int c = b; c < e; ++c) {
        const int corner = T.vfc[c];
        const int t = corner / 3, s = corner - 3 * t;
        const int j = T.F[3 * t + (s + 1) % 3], k = T.F[3 * t + (s + 2) % 3];
        const D3 pj = ld4(p4, j), pk = ld4(p4, k);
        const D3 e1 = pj - pi, e2 = pk - pi;
        const D3 g = cross(e1, e2);
        const double a2 = sqrt(dot(g, g));
        if (!(a2 > 0.0 && a2 < INFINITY)) continue;  // a degenerate face, an overflow: nothing
        const D3 ij = pi - pj, ik = pi - pk;
        const double di = dot(e1, e2), dj = dot(ij, pk - pj), dk = dot(ik, pj - pk);
        const double cot_j = dj / a2, cot_k = dk / a2;
        const double theta = atan2(a2, di);
        double a;
        if (!(di < 0.0 || dj < 0.0 || dk < 0.0))
            a = (dot(e1, e1) * cot_k + dot(e2, e2) * cot_j) / 8.0;
        else if (di < 0.0)
            a = a2 / 4.0;
        else
            a = a2 / 8.0;
        A = A + a;
        Th = Th + theta;
        Kv = Kv + (cot_k * ij + cot_j * ik);
        N = N + g;
    }
    const bool ok = !T.bnd[u] && e > b && A > 0.0;
    double h = 0.0;
    if (ok) {
        const double kn = dot(Kv, N);
        const double sg = kn > 0.0 ? 1.0 : (kn < 0.0 ? -1.0 : 0.0);
        h = ((outward * sg) * sqrt(dot(Kv, Kv))) / 4.0;
    }
    area[u] = ok ? A : 0.0;
    deficit[u] = ok ? kTwoPi - Th : 0.0;
    hint[u] = h;
    valid[u] = ok ? 1 : 0;
}

__global__ void curvature_ring_pack_kernel(const double *__restrict__ area, const double *__restrict__ deficit,
                                           const double *__restrict__ hint, const uint8_t *__restrict__ valid, long nv,
                                           Row *__restrict__ x) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nv) return;
    const bool ok = valid[u] != 0;
    x[u] = {ok ? hint[u] : 0.0, ok ? deficit[u] : 0.0, ok ? area[u] : 0.0, ok ? 1.0 : 0.0};
}

__global__ void curvature_ring_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ nb, long nv,
                                      const Row *__restrict__ x, Row *__restrict__ y) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nv) return;
    Row r = x[u];
    if (r.valid != 0.0) {
        const int b = start[u], e = start[u + 1];
#pragma unroll 4
        for (int j = b; j < e; ++j) {  // any degree: the loads of an unrolled group are independent, the adds stay in row order
            const Row t = x[nb[j]];
            if (t.valid != 0.0) {
                r.hint = r.hint + t.hint;
                r.deficit = r.deficit + t.deficit;
                r.area = r.area + t.area;
            }
        }
    }
    y[u] = r;
}

__global__ void curvature_ring_unpack_kernel(const Row *__restrict__ x, long nv, double *__restrict__ area,
                                             double *__restrict__ deficit, double *__restrict__ hint) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nv) return;
    const Row r = x[u];
    area[u] = r.area, deficit[u] = r.deficit, hint[u] = r.hint;
}

__global__ void curvature_finish_kernel(const double *__restrict__ area, const double *__restrict__ deficit,
                                        const double *__restrict__ hint, const uint8_t *__restrict__ valid, long nv,
                                        float *__restrict__ mean, float *__restrict__ gauss) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nv) return;
    const bool ok = valid[u] != 0;
    const double a = area[u];
    mean[u] = ok ? (float)(hint[u] / a) : NAN;
    gauss[u] = ok ? (float)(deficit[u] / a) : NAN;
}

__device__ inline double clamp01(double w) { return w < 0.0 ? 0.0 : (w > 1.0 ? 1.0 : w); }  // a NaN stays

// A value per vertex at a point q of face f = (a, b, c), fp64 from the fp32 inputs: g = (pb - pa) x (pc - pa),
// w0 = clamp(((pb - q) x (pc - q)) . g / (g . g)), w1 = clamp(((pc - q) x (pa - q)) . g / (g . g)), w2 = clamp((1 - w0) - w1);
// per channel s = 0, then s = s + w_m v_m over the corners m = 0, 1, 2 whose value is no NaN, ws likewise the sum of their weights;
// out = (float)s when all three count, (float)(s / ws) when one or two do, NaN when none does.  f < 0, f >= nf or a corner outside
// [0, nv): NaN.  A face without area has NaN weights, hence NaN.
__global__ void surface_attribute_at_kernel(const float *__restrict__ Q, const int32_t *__restrict__ face, long m,
                                            const float *__restrict__ P, const int32_t *__restrict__ F, long nf, long nv,
                                            const float *__restrict__ values, int nc, float *__restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int f = face[i];
    int v[3] = {-1, -1, -1};
    if (f >= 0 && f < nf)
        for (int k = 0; k < 3; ++k) v[k] = F[3 * (long)f + k];
    bool inside = true;
    for (int k = 0; k < 3; ++k) inside = inside && v[k] >= 0 && v[k] < nv;
    if (!inside) {
        for (int ch = 0; ch < nc; ++ch) out[i * nc + ch] = NAN;
        return;
    }
    const D3 pa = ld(P, v[0]), pb = ld(P, v[1]), pc = ld(P, v[2]);
    const D3 q = {(double)Q[3 * i], (double)Q[3 * i + 1], (double)Q[3 * i + 2]};
    const D3 g = cross(pb - pa, pc - pa);
    const double gg = dot(g, g);
    const D3 qa = pa - q, qb = pb - q, qc = pc - q;
    double w[3];
    w[0] = clamp01(dot(cross(qb, qc), g) / gg);
    w[1] = clamp01(dot(cross(qc, qa), g) / gg);
    w[2] = clamp01((1.0 - w[0]) - w[1]);
    for (int ch = 0; ch < nc; ++ch) {
        double s = 0.0, ws = 0.0;
        int n = 0;
        for (int k = 0; k < 3; ++k) {
            const float x = values[(long)v[k] * nc + ch];
            if (x != x) continue;
            s = s + w[k] * (double)x;
            ws = ws + w[k];
            ++n;
        }
        out[i * nc + ch] = n == 3 ? (float)s : (n == 0 ? NAN : (float)(s / ws));
    }
}

inline bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool count31(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31); }

}  // namespace

extern "C" {

int sculpt_curvature_terms(const sculpt_rmd_topo_t *topo, const float *P, double outward, float *work, double *area, double *deficit,
                           double *hint, uint8_t *valid, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "curvature_terms")) return rc;
    SC_REQUIRE(count31(topo->nv), "curvature_terms: nv=%lld out of range", (long long)topo->nv);
    SC_REQUIRE(outward == 1.0 || outward == -1.0, "curvature_terms: outward=%g (+1 or -1)", outward);  // a NaN fails both
    if (topo->nv == 0) return 0;
    SC_REQUIRE(topo->vfs && topo->bnd, "curvature_terms: null topology array");
    SC_REQUIRE(P && work && area && deficit && hint && valid, "curvature_terms: null array");
    SC_REQUIRE(aligned(work, 16), "curvature_terms: the work buffer must be 16-byte aligned");
    float4 *p4 = reinterpret_cast<float4 *>(work);
    RMD_LAUNCH(curvature_pack_kernel, topo->nv, P, (long)topo->nv, p4);
    RMD_LAUNCH(curvature_terms_kernel, topo->nv, topo_of(topo), p4, outward, area, deficit, hint, valid);
    return 0;
}

int sculpt_curvature_ring(const int32_t *start, const int32_t *nb, const uint8_t *valid, int64_t nv, int64_t n_nb, int rounds,
                          const double *area, const double *deficit, const double *hint, double *work_a, double *work_b,
                          double *area_out, double *deficit_out, double *hint_out, sculpt_stream_t stream) {
    SC_REQUIRE(count31(nv) && count31(n_nb), "curvature_ring: nv=%lld, n_nb=%lld out of range", (long long)nv, (long long)n_nb);
    SC_REQUIRE(rounds >= 0 && rounds <= 8, "curvature_ring: rounds=%d (0 .. 8)", rounds);
    if (nv == 0) return 0;
    SC_REQUIRE(start && valid && area && deficit && hint && work_a && work_b && area_out && deficit_out && hint_out,
               "curvature_ring: null array");
    SC_REQUIRE(n_nb == 0 || nb, "curvature_ring: null neighbour table");
    SC_REQUIRE(aligned(work_a, 32) && aligned(work_b, 32) && work_a != work_b,
               "curvature_ring: the two work buffers must be distinct and 32-byte aligned");
    Row *a = reinterpret_cast<Row *>(work_a), *b = reinterpret_cast<Row *>(work_b);
    RMD_LAUNCH(curvature_ring_pack_kernel, nv, area, deficit, hint, valid, (long)nv, a);
    for (int r = 0; r < rounds; ++r) {
        RMD_LAUNCH(curvature_ring_kernel, nv, start, nb, (long)nv, a, b);
        Row *t = a;
        a = b;
        b = t;
    }
    RMD_LAUNCH(curvature_ring_unpack_kernel, nv, a, (long)nv, area_out, deficit_out, hint_out);
    return 0;
}

int sculpt_curvature_finish(const double *area, const double *deficit, const double *hint, const uint8_t *valid, int64_t nv, float *mean,
                            float *gauss, sculpt_stream_t stream) {
    SC_REQUIRE(count31(nv), "curvature_finish: nv=%lld out of range", (long long)nv);
    if (nv == 0) return 0;
    SC_REQUIRE(area && deficit && hint && valid && mean && gauss, "curvature_finish: null array");
    RMD_LAUNCH(curvature_finish_kernel, nv, area, deficit, hint, valid, (long)nv, mean, gauss);
    return 0;
}

int sculpt_surface_attribute_at(const float *points, const int32_t *face, int64_t m, const float *P, const int32_t *F, int64_t nf,
                                int64_t nv, const float *values, int channels, float *out, sculpt_stream_t stream) {
    SC_REQUIRE(count31(m) && count31(nv) && nf >= 0 && 3 * nf < ((int64_t)1 << 31), "surface_attribute_at: m=%lld, nv=%lld, nf=%lld out of range",
               (long long)m, (long long)nv, (long long)nf);
    SC_REQUIRE(channels >= 1 && channels <= kMaxChannels, "surface_attribute_at: channels=%d (1 .. %d)", channels, kMaxChannels);
    SC_REQUIRE(m * channels < ((int64_t)1 << 31) && nv * channels < ((int64_t)1 << 31), "surface_attribute_at: too many values for int32 indices");
    if (m == 0) return 0;
    SC_REQUIRE(points && face && out, "surface_attribute_at: null array");
    SC_REQUIRE(nf == 0 || nv == 0 || (P && F && values), "surface_attribute_at: null surface array");
    RMD_LAUNCH(surface_attribute_at_kernel, m, points, face, (long)m, P, F, (long)nf, (long)nv, values, channels, out);
    return 0;
}

}  // extern "C"
