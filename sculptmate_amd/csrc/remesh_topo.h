// What every device mesh pass shares (csrc/remesh_device.hip, csrc/mesh_simplify.hip): fp64 vector helpers on fp32 positions, the
// topology view a pass rebuilds from the faces (sculpt_rmd_topo_t, include/sculpt_hip.h), its accessors, the link condition
// and the launch macro.  One copy; every translation unit that includes it gets its own (anonymous namespace).  A unit that
// wants its arithmetic uncontracted sets `#pragma clang fp contract(off)` BEFORE including this file, so that the helpers here
// are compiled under it too.
#pragma once
#include <math.h>

#include "common.h"

using namespace sculpt;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxNeighbours = 64;  // a vertex with more distinct neighbours is a feature: boundary (remesh_host.h scan_boundary_vertex)
constexpr unsigned long long kNoClaim = ~0ull;

struct D3 {
    double x, y, z;
};
__device__ inline D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline D3 operator*(double s, D3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ inline double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline double norm(D3 a) { return sqrt(dot(a, a)); }
__device__ inline D3 ld(const float *P, int i) { return {(double)P[3 * i], (double)P[3 * i + 1], (double)P[3 * i + 2]}; }
// fp32 midpoint: equal to the fp64 midpoint of the two fp32 points rounded once to fp32
__device__ inline void midpoint(const float *P, int a, int b, float m[3]) {
    for (int k = 0; k < 3; ++k) m[k] = 0.5f * (P[3 * a + k] + P[3 * b + k]);
}

struct Topo {
    const int32_t *F;
    const int64_t *skeys;
    const int32_t *she, *es, *fe, *vfs, *vfc;
    const uint8_t *bnd;
    long nf, nv, ne;
};

Topo topo_of(const sculpt_rmd_topo_t *t) {
    return {t->F, t->skeys, t->she, t->es, t->fe, t->vfs, t->vfc, t->bnd, (long)t->nf, (long)t->nv, (long)t->ne};
}

__device__ inline int slot_of(const int32_t *F, int f, int x) {
    return F[3 * f] == x ? 0 : (F[3 * f + 1] == x ? 1 : (F[3 * f + 2] == x ? 2 : -1));
}
__device__ inline bool has(const int32_t *F, int f, int x) { return slot_of(F, f, x) >= 0; }
__device__ inline int third(const int32_t *F, int f, int u, int v) {
    const int a = F[3 * f], b = F[3 * f + 1], c = F[3 * f + 2];
    return a != u && a != v ? a : (b != u && b != v ? b : c);
}
__device__ inline bool directed(const int32_t *F, int f, int u, int v) {
    const int k = slot_of(F, f, u);
    return k >= 0 && F[3 * f + (k + 1) % 3] == v;
}
__device__ inline int fan(const Topo &T, int u) { return T.vfs[u + 1] - T.vfs[u]; }
__device__ inline int fan_face(const Topo &T, int j) { return T.vfc[j] / 3; }
__device__ inline void edge_ends(const Topo &T, int e, int &u, int &v) {
    const int64_t key = T.skeys[T.es[e]];
    u = (int)(key >> 32);
    v = (int)(key & 0xffffffff);
}
// faces around u that contain w
__device__ inline int faces_with(const Topo &T, int u, int w) {
    int n = 0;
    for (int j = T.vfs[u]; j < T.vfs[u + 1]; ++j) n += has(T.F, fan_face(T, j), w);
    return n;
}
__device__ inline D3 face_normal(const float *P, const int32_t *F, int f) {
    const D3 a = ld(P, F[3 * f]), b = ld(P, F[3 * f + 1]), c = ld(P, F[3 * f + 2]);
    return cross(b - a, c - a);
}

// remesh_host.h Mesh::can_collapse: the link condition with the boundary closed by a virtual vertex at infinity
__device__ bool link_ok(const Topo &T, int u, int v, int e) {
    const int nef = T.es[e + 1] - T.es[e];
    if (nef != 1 && nef != 2) return false;
    const int f0 = T.she[T.es[e]] / 3;
    int common = 0;
    for (int j = T.vfs[u]; j < T.vfs[u + 1]; ++j) {
        const int f = fan_face(T, j);
        for (int k = 0; k < 3; ++k) {
            const int w = T.F[3 * f + k];
            if (w == u || w == v) continue;
            bool seen = false;  // count each neighbour of u once: at its first face around u
            for (int j2 = T.vfs[u]; j2 < j && !seen; ++j2) seen = has(T.F, fan_face(T, j2), w);
            if (seen) continue;
            if (faces_with(T, v, w) > 0) ++common;
        }
    }
    if (common != nef) return false;
    if (nef == 2 && T.bnd[u] && T.bnd[v]) return false;
    if (nef == 2) {
        const int f1 = T.she[T.es[e] + 1] / 3;
        const int a = third(T.F, f0, u, v), b = third(T.F, f1, u, v);
        bool at_u = false, at_v = false;
        for (int j = T.vfs[a]; j < T.vfs[a + 1]; ++j) {
            const int f = fan_face(T, j);
            if (has(T.F, f, b)) {
                at_u = at_u || has(T.F, f, u);
                at_v = at_v || has(T.F, f, v);
            }
        }
        if (at_u && at_v) return false;
    } else {
        const int a = third(T.F, f0, u, v);
        if (faces_with(T, u, a) == 1 && faces_with(T, v, a) == 1) return false;
    }
    return true;
}

inline int blocks(long n) { return (int)((n + kThreads - 1) / kThreads); }

int check_topo(const sculpt_rmd_topo_t *t, const char *who) {
    SC_REQUIRE(t, "%s: null topology", who);
    SC_REQUIRE(t->nf >= 0 && t->nv >= 0 && t->ne >= 0 && 3 * t->nf < ((int64_t)1 << 31), "%s: mesh too large for int32 indices", who);
    SC_REQUIRE(t->nf == 0 || (t->F && t->skeys && t->she && t->es && t->fe && t->vfs && t->vfc && t->bnd), "%s: null topology array", who);
    return 0;
}

}  // namespace

#define RMD_LAUNCH(kernel, n, ...)                                                             \
    do {                                                                                       \
        if ((n) > 0) hipLaunchKernelGGL(kernel, dim3(blocks(n)), dim3(kThreads), 0, as_stream(stream), __VA_ARGS__); \
        SC_LAUNCH_CHECK();                                                                     \
    } while (0)
