// Loop subdivision ON THE DEVICE: one level of the Loop scheme with Warren's weights (sculpt_subdiv_*, include/sculpt_hip.h;
// driven by sculptmate_amd/sf3d/remesh_device.py loop_subdivide_device).  The faces and the numbering of the new vertices are
// those of the midpoint subdivision (sculpt_rmd_first_halfedge, sculpt_rmd_subdivide); the positions are the scheme's masks.
// Two launches per level on a topology (sculpt_rmd_topo_t):
//   classify   one thread per edge and per vertex.  An edge with two faces is interior, with one a border edge, with three or
//              more non-manifold -- from es[e + 1] - es[e] alone (NOT bnd: that also flags vertices of more than 64 neighbours,
//              which are subdivided like any other).  Per vertex, with integer atomics on zeroed words (one possible result):
//                  cls[u] = { border edges at u, max(other end) + 1, nv - min(other end), touches a non-manifold edge }
//              and the positions go into 16-byte rows (x y z -), so that a neighbour costs one load.
//   loop       one thread per vertex, edge and face.  Per component in fp64 from the fp32 values, the operations as written,
//              rounded once to fp32:
//                  odd vertex of edge {u, v}    interior, its two faces' third vertices a, b:
//                                                   0.375 * (P[u] + P[v]) + 0.125 * (P[a] + P[b])
//                                               border or non-manifold:  0.5 * (P[u] + P[v])
//                  even vertex u, fan n = vfs[u + 1] - vfs[u]
//                      n == 0, a non-manifold edge at u, or border edges at u neither 0 nor 2 (a corner):  its bits
//                      two border edges, other ends a, b (a crease):  0.75 * P[u] + 0.125 * (P[a] + P[b])
//                      otherwise  beta = n == 3 ? 0.1875 : 3.0 / (8.0 * n);  S = the sum, left to right over the corners
//                                 3 f + k of u's fan in vfc order, of P[F[3 f + (k + 1) % 3]], then P[F[3 f + (k + 2) % 3]]
//                                 (S starts as the first term; every neighbour enters twice);
//                                 (1.0 - n * beta) * P[u] + (0.5 * beta) * S
//              An attribute array [nv][C], 1 <= C <= 8, goes through the same masks.
// No float atomics, a fixed order of summation: the result does not depend on scheduling.  The unit is compiled with
// floating-point contraction OFF (the pragma below, before the shared helpers); tests/_loopref.py restates it in NumPy operation
// for operation and positions, faces and attributes are compared bit for bit.
#pragma clang fp contract(off)

#include <algorithm>

#include "remesh_topo.h"

namespace {

constexpr int kMaxChannels = 8;

struct PosRows {  // positions as 16-byte rows
    const float4 *p;
    __device__ void load(int w, double (&x)[3]) const {
        const float4 t = p[w];
        x[0] = (double)t.x, x[1] = (double)t.y, x[2] = (double)t.z;
    }
};

struct AttrRows {  // [nv][C] floats; the channels past C are zeroes nobody stores
    const float *a;
    int C;
    __device__ void load(int w, double (&x)[kMaxChannels]) const {
#pragma unroll
        for (int c = 0; c < kMaxChannels; ++c) x[c] = c < C ? (double)a[(long)w * C + c] : 0.0;
    }
};

// cls[u]: see the head of the file
__global__ void subdiv_classify_kernel(Topo T, const float *__restrict__ P, int32_t *__restrict__ cls, float4 *__restrict__ p4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < T.nv) p4[i] = make_float4(P[3 * i], P[3 * i + 1], P[3 * i + 2], 0.0f);
    if (i >= T.ne) return;
    const int nef = T.es[i + 1] - T.es[i];
    if (nef == 2) return;
    int u, v;
    edge_ends(T, (int)i, u, v);
    if (nef == 1) {
        atomicAdd(&cls[4 * u], 1);
        atomicMax(&cls[4 * u + 1], v + 1);
        atomicMax(&cls[4 * u + 2], (int)T.nv - v);
        atomicAdd(&cls[4 * v], 1);
        atomicMax(&cls[4 * v + 1], u + 1);
        atomicMax(&cls[4 * v + 2], (int)T.nv - u);
    } else {
        atomicOr(&cls[4 * u + 3], 1);
        atomicOr(&cls[4 * v + 3], 1);
    }
}

// the odd vertex of edge e -> q; N components of `rows`
template <int N, class Rows>
__device__ inline void odd_rule(const Topo &T, int e, const Rows &rows, double (&q)[N]) {
    int u, v;
    edge_ends(T, e, u, v);
    double pu[N], pv[N];
    rows.load(u, pu);
    rows.load(v, pv);
    if (T.es[e + 1] - T.es[e] == 2) {
        const int a = third(T.F, T.she[T.es[e]] / 3, u, v), b = third(T.F, T.she[T.es[e] + 1] / 3, u, v);
        double pa[N], pb[N];
        rows.load(a, pa);
        rows.load(b, pb);
#pragma unroll
        for (int c = 0; c < N; ++c) q[c] = 0.375 * (pu[c] + pv[c]) + 0.125 * (pa[c] + pb[c]);
    } else {
#pragma unroll
        for (int c = 0; c < N; ++c) q[c] = 0.5 * (pu[c] + pv[c]);
    }
}

// the even vertex u -> q; false: u keeps its bits (q is not written)
template <int N, class Rows>
__device__ inline bool even_rule(const Topo &T, const int4 cl, int u, const Rows &rows, double (&q)[N]) {
    const int b = T.vfs[u], e = T.vfs[u + 1], n = e - b;
    if (n == 0 || cl.w != 0 || (cl.x != 0 && cl.x != 2)) return false;
    double pu[N];
    rows.load(u, pu);
    if (cl.x == 2) {  // a crease: the other ends of the two border edges
        double pa[N], pb[N];
        rows.load((int)T.nv - cl.z, pa);
        rows.load(cl.y - 1, pb);
#pragma unroll
        for (int c = 0; c < N; ++c) q[c] = 0.75 * pu[c] + 0.125 * (pa[c] + pb[c]);
        return true;
    }
    const double beta = n == 3 ? 0.1875 : 3.0 / (8.0 * (double)n);
    double S[N], t[N];
    for (int j = b; j < e; ++j) {  // any valence; the sum stays in corner order
        const int corner = T.vfc[j], f = corner / 3, k = corner - 3 * f;
        const int w1 = T.F[3 * f + (k + 1) % 3], w2 = T.F[3 * f + (k + 2) % 3];
        rows.load(w1, t);
        if (j == b) {
#pragma unroll
            for (int c = 0; c < N; ++c) S[c] = t[c];
        } else {
#pragma unroll
            for (int c = 0; c < N; ++c) S[c] = S[c] + t[c];
        }
        rows.load(w2, t);
#pragma unroll
        for (int c = 0; c < N; ++c) S[c] = S[c] + t[c];
    }
    const double keep = 1.0 - (double)n * beta, share = 0.5 * beta;
#pragma unroll
    for (int c = 0; c < N; ++c) q[c] = keep * pu[c] + share * S[c];
    return true;
}

__device__ inline void store_attr(float *__restrict__ Ao, long row, int C, const double (&q)[kMaxChannels]) {
#pragma unroll
    for (int c = 0; c < kMaxChannels; ++c)
        if (c < C) Ao[row * C + c] = (float)q[c];
}

// rank_incl: inclusive prefix sum of sculpt_rmd_first_halfedge; A == nullptr: no attributes
__global__ void subdiv_loop_kernel(Topo T, const int4 *__restrict__ cls, const float4 *__restrict__ p4, const int32_t *__restrict__ rank_incl,
                                   const float *__restrict__ A, int C, float *__restrict__ Po, int32_t *__restrict__ Fo, float *__restrict__ Ao) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const PosRows pos{p4};
    const AttrRows att{A, C};
    if (i < T.nv) {
        const int4 cl = cls[i];
        double q[3];
        if (even_rule<3>(T, cl, (int)i, pos, q)) {
            for (int k = 0; k < 3; ++k) Po[3 * i + k] = (float)q[k];
        } else {
            const float4 p = p4[i];
            Po[3 * i] = p.x, Po[3 * i + 1] = p.y, Po[3 * i + 2] = p.z;
        }
        if (A) {
            double a[kMaxChannels];
            if (even_rule<kMaxChannels>(T, cl, (int)i, att, a)) {
                store_attr(Ao, i, C, a);
            } else {
                for (int c = 0; c < C; ++c) Ao[i * C + c] = A[i * C + c];
            }
        }
    }
    if (i < T.ne) {
        const long o = T.nv + rank_incl[T.she[T.es[i]]] - 1;
        double q[3];
        odd_rule<3>(T, (int)i, pos, q);
        for (int k = 0; k < 3; ++k) Po[3 * o + k] = (float)q[k];
        if (A) {
            double a[kMaxChannels];
            odd_rule<kMaxChannels>(T, (int)i, att, a);
            store_attr(Ao, o, C, a);
        }
    }
    if (i < T.nf) {  // remesh_device.hip subdivide_kernel's template
        const int a = T.F[3 * i], b = T.F[3 * i + 1], c = T.F[3 * i + 2];
        int mid[3];
        for (int k = 0; k < 3; ++k) mid[k] = (int)(T.nv + rank_incl[T.she[T.es[T.fe[3 * i + k]]]] - 1);
        const int ab = mid[0], bc = mid[1], ca = mid[2];
        const int t[12] = {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca};
        for (int k = 0; k < 12; ++k) Fo[12 * i + k] = t[k];
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

int check_counts(const sculpt_rmd_topo_t *t, const char *who) {
    if (int rc = check_topo(t, who)) return rc;
    SC_REQUIRE(t->nv < ((int64_t)1 << 31) && t->ne <= 3 * t->nf && t->nv + t->ne < ((int64_t)1 << 31) && 12 * t->nf < ((int64_t)1 << 31),
               "%s: %lld vertices, %lld edges, %lld faces do not fit int32 indices after a level", who, (long long)t->nv, (long long)t->ne,
               (long long)t->nf);
    return 0;
}

}  // namespace

extern "C" {

int sculpt_subdiv_classify(const sculpt_rmd_topo_t *topo, const float *P, int32_t *cls, float *rows, sculpt_stream_t stream) {
    if (int rc = check_counts(topo, "subdiv_classify")) return rc;
    if (topo->nf == 0) return 0;  // nothing to refine: the caller returns copies
    SC_REQUIRE(topo->nv > 0, "subdiv_classify: faces without vertices");
    SC_REQUIRE(P && cls && rows, "subdiv_classify: null array");
    SC_REQUIRE(aligned16(cls) && aligned16(rows), "subdiv_classify: cls and rows must be 16-byte aligned");
    SC_HIP(hipMemsetAsync(cls, 0, (size_t)topo->nv * 4 * sizeof(int32_t), as_stream(stream)));
    RMD_LAUNCH(subdiv_classify_kernel, std::max(topo->nv, topo->ne), topo_of(topo), P, cls, reinterpret_cast<float4 *>(rows));
    return 0;
}

int sculpt_subdiv_loop(const sculpt_rmd_topo_t *topo, const int32_t *cls, const float *rows, const int32_t *rank_incl, const float *A,
                       int channels, float *Po, int32_t *Fo, float *Ao, sculpt_stream_t stream) {
    if (int rc = check_counts(topo, "subdiv_loop")) return rc;
    SC_REQUIRE((A == nullptr) == (Ao == nullptr), "subdiv_loop: attributes in and out go together");
    SC_REQUIRE(!A || (channels >= 1 && channels <= kMaxChannels), "subdiv_loop: channels=%d (1 .. %d)", channels, kMaxChannels);
    if (topo->nf == 0) return 0;  // nothing to refine: the caller returns copies
    SC_REQUIRE(topo->nv > 0, "subdiv_loop: faces without vertices");
    SC_REQUIRE(cls && rows && rank_incl && Po && Fo, "subdiv_loop: null array");
    SC_REQUIRE(aligned16(cls) && aligned16(rows), "subdiv_loop: cls and rows must be 16-byte aligned");
    SC_REQUIRE(Po != rows && (!A || A != Ao), "subdiv_loop: the outputs must not be the inputs");
    const long n = (long)std::max(topo->nv, std::max(topo->ne, topo->nf));
    RMD_LAUNCH(subdiv_loop_kernel, n, topo_of(topo), reinterpret_cast<const int4 *>(cls), reinterpret_cast<const float4 *>(rows), rank_incl, A,
               A ? channels : 0, Po, Fo, Ao);
    return 0;
}

}  // extern "C"
