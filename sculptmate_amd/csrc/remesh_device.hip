// Triangle remeshing ON THE DEVICE: the per-element steps of decimate / Botsch-Kobbelt remeshing / midpoint subdivision
// (sculpt_rmd_*, include/sculpt_hip.h).  The host restatement of the same operations is csrc/remesh_host.h; this file keeps its
// rules and replaces its sequential order by rounds of independent local operations.
//
// State between passes: positions (fp32 [nv][3]) and the face list (int32 [nf][3]).  Every pass rebuilds what it needs from the
// faces (sf3d/remesh_device.py does the sorts and prefix sums through torch):
//   half-edge h = 3 f + k runs F[f][k] -> F[f][(k + 1) % 3]; its undirected key is (min << 32 | max)
//   the keys sorted (stable): edge e owns the sorted range [es[e], es[e + 1]); she[] are the half-edge ids in that order, fe[h]
//     the edge of half-edge h
//   vertex -> corner CSR (stable sort of the corners by vertex): corners vfc[vfs[u] .. vfs[u + 1]) of vertex u, face = corner / 3
//   bnd[u]: some edge at u does not have exactly two faces, or a flag the caller carries from earlier passes: a vertex with more
//     than 64 distinct neighbours in the input stays a feature for the whole call (remesh_host.h Mesh::build scans once)
// Local operations (collapse, flip) run as propose / select / apply: every valid candidate claims every vertex of its footprint
// with a 64-bit atomicMin of (priority << 32 | edge id); only a candidate that holds its whole footprint applies.  Two winners
// never share a footprint vertex, so neither reads or writes anything the other changes and a round is the same as applying
// its winners one after the other in any order.  No float atomics: the result does not depend on scheduling.
// Predicates (fold-over, crease, closest point) are evaluated in fp64 from the fp32 positions.
#include <algorithm>

#include "remesh_topo.h"
#include "surface_grid.h"

namespace {

// ---- topology --------------------------------------------------------------------------------------------------------------
__global__ void halfedge_keys_kernel(const int32_t *__restrict__ F, long nf, int64_t *__restrict__ keys) {
    const long h = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= 3 * nf) return;
    const long f = h / 3;
    const int k = (int)(h - 3 * f);
    const uint32_t a = (uint32_t)F[3 * f + k], b = (uint32_t)F[3 * f + (k + 1) % 3];
    keys[h] = (int64_t)(((uint64_t)min(a, b) << 32) | max(a, b));
}

__global__ void edge_heads_kernel(const int64_t *__restrict__ skeys, long nh, int32_t *__restrict__ head) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nh) head[i] = i == 0 || skeys[i] != skeys[i - 1];
}

// eid: inclusive prefix sum of the heads
__global__ void edge_fill_kernel(const int64_t *__restrict__ sperm, const int32_t *__restrict__ eid, long nh, int32_t *__restrict__ she,
                                 int32_t *__restrict__ fe, int32_t *__restrict__ es) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nh) return;
    const int h = (int)sperm[i], e = eid[i] - 1;
    she[i] = h;
    fe[h] = e;
    if (i == 0 || eid[i - 1] != eid[i]) es[e] = (int)i;
    if (i == nh - 1) es[e + 1] = (int)nh;
}

__global__ void boundary_kernel(Topo T, uint8_t *__restrict__ bnd) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne) return;
    if (T.es[e + 1] - T.es[e] != 2) {  // every writer stores the same value
        int u, v;
        edge_ends(T, (int)e, u, v);
        bnd[u] = 1;
        bnd[v] = 1;
    }
}

// a vertex with more than kMaxNeighbours distinct neighbours is flagged like a boundary vertex (the host's "absurd valence:
// treat as a feature", scanned once per input; the caller carries the flag through the passes); a fan of f faces has at most 2 f neighbours, so only fans above kMaxNeighbours / 2 are scanned, and
// the scan stops at the first neighbour past the limit: O(fan x kMaxNeighbours)
__global__ void high_valence_kernel(Topo T, uint8_t *__restrict__ flags) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= T.nv || fan(T, (int)u) <= kMaxNeighbours / 2) return;
    int nb[kMaxNeighbours], n = 0;
    for (int j = T.vfs[u]; j < T.vfs[u + 1]; ++j) {
        const int f = fan_face(T, j);
        for (int k = 0; k < 3; ++k) {
            const int w = T.F[3 * f + k];
            if (w == (int)u) continue;
            int i = 0;
            while (i < n && nb[i] != w) ++i;
            if (i < n) continue;
            if (n == kMaxNeighbours) {
                flags[u] = 1;
                return;
            }
            nb[n++] = w;
        }
    }
}

// ---- collapse (shared by decimate and the Botsch-Kobbelt pass) -----------------------------------------------------------
// mode 0 = decimate: any edge, remove min(u, v), keep max at the midpoint, link condition only (remesh_host.h decimate()).
// mode 1 = Botsch: edges shorter than `low`, never both ends on the boundary, the interior end goes, a boundary end stays put,
// no edge of the merged vertex longer than `high`, no face turns over (remesh_host.h collapse_short_edges()).
__device__ bool collapse_target(const Topo &T, const float *P, int mode, int e, int &u, int &v, float p[3]) {
    edge_ends(T, e, u, v);
    if (mode == 1) {
        if (T.bnd[u] && T.bnd[v]) return false;
        if (T.bnd[u]) {
            const int t = u;
            u = v;
            v = t;
        }
        if (T.bnd[v]) {
            for (int k = 0; k < 3; ++k) p[k] = P[3 * v + k];
            return true;
        }
    }
    midpoint(P, u, v, p);
    return true;
}

__global__ void collapse_propose_kernel(Topo T, const float *__restrict__ P, int mode, double low, double high,
                                        unsigned long long *__restrict__ claim, unsigned long long *__restrict__ cand) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne) return;
    cand[e] = kNoClaim;
    int u, v;
    float pf[3];
    {
        int a, b;
        edge_ends(T, (int)e, a, b);
        const int nef = T.es[e + 1] - T.es[e];
        if (nef != 1 && nef != 2) return;
        if (mode == 1 && !(norm(ld(P, a) - ld(P, b)) < low)) return;
    }
    if (!collapse_target(T, P, mode, (int)e, u, v, pf)) return;
    if (!link_ok(T, u, v, (int)e)) return;
    const D3 p = {(double)pf[0], (double)pf[1], (double)pf[2]};
    if (mode == 1) {
        for (int side = 0; side < 2; ++side) {
            const int x = side ? v : u, other = side ? u : v;
            for (int j = T.vfs[x]; j < T.vfs[x + 1]; ++j) {
                const int f = fan_face(T, j);
                for (int k = 0; k < 3; ++k) {
                    const int w = T.F[3 * f + k];
                    if (w != u && w != v && norm(ld(P, w) - p) > high) return;
                }
                if (has(T.F, f, other)) continue;  // dies with the edge
                D3 q[3];
                for (int k = 0; k < 3; ++k) q[k] = T.F[3 * f + k] == x ? p : ld(P, T.F[3 * f + k]);
                if (dot(face_normal(P, T.F, f), cross(q[1] - q[0], q[2] - q[0])) <= 0) return;
            }
        }
    }
    // priority: the edge length (non-negative fp32 bits order like the values), ties by edge id
    const float len = (float)norm(ld(P, u) - ld(P, v));
    const unsigned long long key = ((unsigned long long)__float_as_uint(len) << 32) | (unsigned long long)e;
    cand[e] = key;
    for (int side = 0; side < 2; ++side) {
        const int x = side ? v : u;
        for (int j = T.vfs[x]; j < T.vfs[x + 1]; ++j) {
            const int f = fan_face(T, j);
            for (int k = 0; k < 3; ++k) atomicMin(&claim[T.F[3 * f + k]], key);
        }
    }
}

// win[e] = faces the collapse removes (1 or 2), 0 if e does not hold its whole footprint
__global__ void collapse_select_kernel(Topo T, const float *__restrict__ P, int mode, const unsigned long long *__restrict__ claim,
                                       const unsigned long long *__restrict__ cand, int32_t *__restrict__ win) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne) return;
    win[e] = 0;
    const unsigned long long key = cand[e];
    if (key == kNoClaim) return;
    int u, v;
    float pf[3];
    collapse_target(T, P, mode, (int)e, u, v, pf);
    for (int side = 0; side < 2; ++side) {
        const int x = side ? v : u;
        for (int j = T.vfs[x]; j < T.vfs[x + 1]; ++j) {
            const int f = fan_face(T, j);
            for (int k = 0; k < 3; ++k)
                if (claim[T.F[3 * f + k]] != key) return;
        }
    }
    win[e] = T.es[e + 1] - T.es[e];
}

// the winners: faces on the edge die, u is replaced by v in the others, v moves to the target point
__global__ void collapse_apply_kernel(Topo T, float *__restrict__ P, int32_t *__restrict__ F, int mode, const int32_t *__restrict__ win,
                                      uint8_t *__restrict__ falive) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne || win[e] == 0) return;
    int u, v;
    float p[3];
    collapse_target(T, P, mode, (int)e, u, v, p);
    for (int j = T.vfs[u]; j < T.vfs[u + 1]; ++j) {
        const int f = fan_face(T, j);
        const int ku = T.vfc[j] - 3 * f;
        if (has(F, f, v))
            falive[f] = 0;
        else
            F[3 * f + ku] = v;
    }
    for (int k = 0; k < 3; ++k) P[3 * v + k] = p[k];
}

// ---- flip ---------------------------------------------------------------------------------------------------------------
// remesh_host.h equalize_valences(): an interior edge between two consistently oriented faces (u, v, a), (v, u, b) becomes
// (a, b) when that brings the four valences closer to 6 (4 on the boundary), the old pair is no sharp crease and the new pair
// does not fold over.  Footprint {u, v, a, b}.
__device__ bool flip_target(const Topo &T, const float *P, int e, int &u, int &v, int &a, int &b, int &f1, int &f2, int &gain) {
    if (T.es[e + 1] - T.es[e] != 2) return false;
    edge_ends(T, e, u, v);
    f1 = T.she[T.es[e]] / 3;
    f2 = T.she[T.es[e] + 1] / 3;
    if (!directed(T.F, f1, u, v)) {
        const int t = f1;
        f1 = f2;
        f2 = t;
    }
    if (!directed(T.F, f1, u, v) || !directed(T.F, f2, v, u)) return false;
    a = third(T.F, f1, u, v);
    b = third(T.F, f2, u, v);
    if (a == b) return false;
    if (faces_with(T, a, b) != 0) return false;  // the new edge exists already
    auto val = [&](int x) { return fan(T, x) + (T.bnd[x] ? 1 : 0); };
    auto tgt = [&](int x) { return T.bnd[x] ? 4 : 6; };
    auto sq = [](int x) { return x * x; };
    const int before = sq(val(u) - tgt(u)) + sq(val(v) - tgt(v)) + sq(val(a) - tgt(a)) + sq(val(b) - tgt(b));
    const int after = sq(val(u) - 1 - tgt(u)) + sq(val(v) - 1 - tgt(v)) + sq(val(a) + 1 - tgt(a)) + sq(val(b) + 1 - tgt(b));
    gain = before - after;
    return gain > 0;
}

__global__ void flip_propose_kernel(Topo T, const float *__restrict__ P, unsigned long long *__restrict__ claim,
                                    unsigned long long *__restrict__ cand) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne) return;
    cand[e] = kNoClaim;
    int u, v, a, b, f1, f2, gain;
    if (!flip_target(T, P, (int)e, u, v, a, b, f1, f2, gain)) return;
    const D3 n1 = face_normal(P, T.F, f1), n2 = face_normal(P, T.F, f2);
    const double l1 = norm(n1), l2 = norm(n2);
    if (l1 == 0 || l2 == 0 || dot(n1, n2) < 0.5 * l1 * l2) return;
    const D3 pu = ld(P, u), pv = ld(P, v), pa = ld(P, a), pb = ld(P, b);
    const D3 m1 = cross(pb - pu, pa - pu), m2 = cross(pv - pb, pa - pb);
    const D3 avg = (1.0 / l1) * n1 + (1.0 / l2) * n2;
    if (dot(m1, avg) <= 0 || dot(m2, avg) <= 0) return;
    // larger valence gain first, ties by edge id
    const unsigned long long key = ((unsigned long long)(1024 - min(gain, 1023)) << 32) | (unsigned long long)e;
    cand[e] = key;
    atomicMin(&claim[u], key);
    atomicMin(&claim[v], key);
    atomicMin(&claim[a], key);
    atomicMin(&claim[b], key);
}

// select and apply are two launches: a loser's re-evaluation must not read faces a winner is rewriting
__global__ void flip_select_kernel(Topo T, const float *__restrict__ P, const unsigned long long *__restrict__ claim,
                                   const unsigned long long *__restrict__ cand, int32_t *__restrict__ win) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne) return;
    win[e] = 0;
    const unsigned long long key = cand[e];
    if (key == kNoClaim) return;
    int u, v, a, b, f1, f2, gain;
    flip_target(T, P, (int)e, u, v, a, b, f1, f2, gain);
    win[e] = claim[u] == key && claim[v] == key && claim[a] == key && claim[b] == key;
}

__global__ void flip_apply_kernel(Topo T, const float *__restrict__ P, const int32_t *__restrict__ win, int32_t *__restrict__ F) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne || !win[e]) return;
    // a winner's faces and the faces around its a are read and written by no other winner (their vertices are in its footprint)
    int u, v, a, b, f1, f2, gain;
    flip_target(T, P, (int)e, u, v, a, b, f1, f2, gain);
    F[3 * f1] = u, F[3 * f1 + 1] = b, F[3 * f1 + 2] = a;
    F[3 * f2] = b, F[3 * f2 + 1] = v, F[3 * f2 + 2] = a;
}

// ---- split --------------------------------------------------------------------------------------------------------------
__global__ void split_mark_kernel(Topo T, const float *__restrict__ P, double high, int32_t *__restrict__ mark) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne) return;
    const int nef = T.es[e + 1] - T.es[e];
    int u, v;
    edge_ends(T, (int)e, u, v);
    mark[e] = (nef == 1 || nef == 2) && norm(ld(P, u) - ld(P, v)) > high;
}

__device__ inline int split_children(const Topo &T, const int32_t *mark, long f) {
    const int m = mark[T.fe[3 * f]] + mark[T.fe[3 * f + 1]] + mark[T.fe[3 * f + 2]];
    return m == 3 ? 4 : m + 1;
}

__global__ void split_count_kernel(Topo T, const int32_t *__restrict__ mark, int32_t *__restrict__ cnt) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < T.nf) cnt[f] = split_children(T, mark, f);
}

// new vertex of marked edge e: nv + mark_incl[e] - 1, at the midpoint; written only below the capacity
__global__ void split_vertices_kernel(Topo T, float *__restrict__ P, const int32_t *__restrict__ mark, const int32_t *__restrict__ mark_incl,
                                      long vcap) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T.ne || !mark[e]) return;
    const long m = T.nv + mark_incl[e] - 1;
    if (m >= vcap) return;
    int u, v;
    edge_ends(T, (int)e, u, v);
    float p[3];
    midpoint(P, u, v, p);
    for (int k = 0; k < 3; ++k) P[3 * m + k] = p[k];
}

// children of face f at [off_incl[f] - cnt, off_incl[f]), by template; orientation kept; written only below the capacity
__global__ void split_faces_kernel(Topo T, const float *__restrict__ P, const int32_t *__restrict__ mark,
                                   const int32_t *__restrict__ mark_incl, const int32_t *__restrict__ off_incl, long fcap,
                                   int32_t *__restrict__ Fo) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= T.nf) return;
    int c[3], mk[3], M[3];
    for (int k = 0; k < 3; ++k) {
        c[k] = T.F[3 * f + k];
        const int e = T.fe[3 * f + k];
        mk[k] = mark[e];
        M[k] = mk[k] ? (int)(T.nv + mark_incl[e] - 1) : -1;
    }
    const int n = mk[0] + mk[1] + mk[2];
    const long first = off_incl[f] - (n == 3 ? 4 : n + 1);
    if (first + (n == 3 ? 4 : n + 1) > fcap) return;
    int t[12], nt = 0;
    auto put = [&](int a, int b, int d) { t[3 * nt] = a, t[3 * nt + 1] = b, t[3 * nt + 2] = d, ++nt; };
    if (n == 0) {
        put(c[0], c[1], c[2]);
    } else if (n == 1) {
        const int k = mk[0] ? 0 : (mk[1] ? 1 : 2);
        put(c[k], M[k], c[(k + 2) % 3]);
        put(M[k], c[(k + 1) % 3], c[(k + 2) % 3]);
    } else if (n == 2) {
        const int k = !mk[0] ? 0 : (!mk[1] ? 1 : 2);  // the unmarked edge c_k -> c_k+1
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        put(M[k1], c[k2], M[k2]);  // the corner at c_k+2
        // quad c_k, c_k+1, M_k+1, M_k+2: the shorter diagonal (midpoints as split_vertices_kernel writes them)
        float m1[3], m2[3];
        int u, v;
        edge_ends(T, T.fe[3 * f + k1], u, v);
        midpoint(P, u, v, m1);
        edge_ends(T, T.fe[3 * f + k2], u, v);
        midpoint(P, u, v, m2);
        const D3 q1 = {(double)m1[0], (double)m1[1], (double)m1[2]}, q2 = {(double)m2[0], (double)m2[1], (double)m2[2]};
        if (norm(q1 - ld(P, c[k])) <= norm(q2 - ld(P, c[k1]))) {
            put(c[k], c[k1], M[k1]);
            put(c[k], M[k1], M[k2]);
        } else {
            put(c[k], c[k1], M[k2]);
            put(c[k1], M[k1], M[k2]);
        }
    } else {
        put(c[0], M[0], M[2]);
        put(c[1], M[1], M[0]);
        put(c[2], M[2], M[1]);
        put(M[0], M[1], M[2]);
    }
    for (int i = 0; i < 3 * nt; ++i) Fo[3 * first + i] = t[i];
}

// ---- closest point on the input surface (uniform grid: Grid, grid_range and closest_on_triangle are surface_grid.h) ---------
__global__ void grid_count_kernel(Grid G, int32_t *__restrict__ cnt) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= G.nf) return;
    int a[3], b[3];
    grid_range(G, f, a, b);
    cnt[f] = (b[0] - a[0] + 1) * (b[1] - a[1] + 1) * (b[2] - a[2] + 1);
}

// (cell, face) pairs of face f at [off_incl[f] - cnt[f], off_incl[f]); a stable sort by cell then lists every cell's faces in
// face order
__global__ void grid_fill_kernel(Grid G, const int32_t *__restrict__ off_incl, int32_t *__restrict__ cell, int32_t *__restrict__ face) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= G.nf) return;
    int a[3], b[3];
    grid_range(G, f, a, b);
    long o = off_incl[f] - (long)(b[0] - a[0] + 1) * (b[1] - a[1] + 1) * (b[2] - a[2] + 1);
    for (int z = a[2]; z <= b[2]; ++z)
        for (int y = a[1]; y <= b[1]; ++y)
            for (int x = a[0]; x <= b[0]; ++x) {
                cell[o] = (int32_t)(((long)z * G.n[1] + y) * G.n[0] + x);
                face[o++] = (int32_t)f;
            }
}

// expanding Chebyshev shells of cells around p's cell until nothing unvisited can be closer (remesh_host.h SurfaceGrid::closest)
__device__ D3 grid_closest(const Grid &G, D3 p) {
    if (G.nf == 0) return p;
    const double q[3] = {(p.x - G.lo[0]) / G.cell, (p.y - G.lo[1]) / G.cell, (p.z - G.lo[2]) / G.cell};
    int c[3];
    for (int k = 0; k < 3; ++k) c[k] = grid_clamp(q[k], G.n[k]);
    double best = INFINITY;
    D3 bp = p;
    const int rmax = max(G.n[0], max(G.n[1], G.n[2]));
    for (int r = 0; r <= rmax; ++r) {
        for (int z = c[2] - r; z <= c[2] + r; ++z) {
            if (z < 0 || z >= G.n[2]) continue;
            for (int y = c[1] - r; y <= c[1] + r; ++y) {
                if (y < 0 || y >= G.n[1]) continue;
                const bool inner = abs(z - c[2]) != r && abs(y - c[1]) != r;
                const int step = inner ? max(1, 2 * r) : 1;
                for (int x = c[0] - r; x <= c[0] + r; x += step) {
                    if (x < 0 || x >= G.n[0]) continue;
                    const long ci = ((long)z * G.n[1] + y) * G.n[0] + x;
                    for (int i = G.start[ci]; i < G.start[ci + 1]; ++i) {
                        const int f = G.items[i];
                        const D3 cp = closest_on_triangle(p, ld(G.P, G.F[3 * f]), ld(G.P, G.F[3 * f + 1]), ld(G.P, G.F[3 * f + 2]));
                        const double d = dot(cp - p, cp - p);
                        if (d < best) {
                            best = d;
                            bp = cp;
                        }
                    }
                }
            }
        }
        double reach = INFINITY;
        for (int k = 0; k < 3; ++k) {
            if (c[k] - r > 0) reach = fmin(reach, q[k] - (c[k] - r));
            if (c[k] + r < G.n[k] - 1) reach = fmin(reach, (c[k] + r + 1) - q[k]);
        }
        if (reach == INFINITY) break;
        reach = fmax(0.0, reach) * G.cell;
        if (best <= reach * reach) break;
    }
    return bp;
}

// ---- tangential relaxation (Jacobi) + projection ---------------------------------------------------------------------------
__global__ void relax_kernel(Topo T, const float *__restrict__ P, Grid G, int project, float *__restrict__ Q) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= T.nv) return;
    for (int k = 0; k < 3; ++k) Q[3 * u + k] = P[3 * u + k];
    if (fan(T, (int)u) == 0 || T.bnd[u]) return;
    D3 N = {0, 0, 0}, c = {0, 0, 0};
    int deg = 0;
    for (int j = T.vfs[u]; j < T.vfs[u + 1]; ++j) {
        const int f = fan_face(T, j);
        N = N + face_normal(P, T.F, f);  // length = 2 area: area-weighted vertex normal
        // the centroid of the distinct neighbours, each at its first face around u (remesh_host.h Mesh::neighbours): the "next
        // corner" of every face is the same set only where the fan is consistently oriented.  An interior vertex has at most
        // kMaxNeighbours neighbours, so this is O(fan^2) with a small fan.
        for (int k = 0; k < 3; ++k) {
            const int w = T.F[3 * f + k];
            if (w == (int)u) continue;
            bool seen = false;
            for (int j2 = T.vfs[u]; j2 < j && !seen; ++j2) seen = has(T.F, fan_face(T, j2), w);
            if (seen) continue;
            c = c + ld(P, w);
            ++deg;
        }
    }
    c = (1.0 / deg) * c;
    const double ln = norm(N);
    if (ln == 0) return;
    const D3 n = (1.0 / ln) * N;
    const D3 pu = ld(P, (int)u);
    D3 p = c + dot(n, pu - c) * n;
    for (int j = T.vfs[u]; j < T.vfs[u + 1]; ++j) {
        const int f = fan_face(T, j);
        D3 q[3];
        for (int k = 0; k < 3; ++k) q[k] = T.F[3 * f + k] == (int)u ? p : ld(P, T.F[3 * f + k]);
        if (dot(face_normal(P, T.F, f), cross(q[1] - q[0], q[2] - q[0])) <= 0) return;
    }
    if (project) p = grid_closest(G, p);
    Q[3 * u] = (float)p.x, Q[3 * u + 1] = (float)p.y, Q[3 * u + 2] = (float)p.z;
}

// second pass: every vertex of a face that turned over (old positions vs new) takes its move back.  Taking back one vertex can
// turn over another face whose other corners moved, so the pass repeats until it marks no new vertex (*grew = 0); the marks only
// grow, so this ends.
__global__ void undo_mark_kernel(const int32_t *__restrict__ F, long nf, const float *__restrict__ P, const float *__restrict__ Q,
                                 uint8_t *__restrict__ undo, int32_t *__restrict__ grew) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    if (dot(face_normal(P, F, (int)f), face_normal(Q, F, (int)f)) <= 0)
        for (int k = 0; k < 3; ++k)
            if (!undo[F[3 * f + k]]) {
                undo[F[3 * f + k]] = 1;  // every writer stores the same value
                *grew = 1;
            }
}

__global__ void undo_apply_kernel(const float *__restrict__ P, const uint8_t *__restrict__ undo, long nv, float *__restrict__ Q) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < nv && undo[u])
        for (int k = 0; k < 3; ++k) Q[3 * u + k] = P[3 * u + k];
}

// ---- compaction, subdivision, checks ---------------------------------------------------------------------------------------
__global__ void compact_faces_kernel(const int32_t *__restrict__ F, const uint8_t *__restrict__ alive, const int32_t *__restrict__ incl,
                                     long nf, int32_t *__restrict__ Fo) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf || !alive[f]) return;
    const long o = incl[f] - 1;
    for (int k = 0; k < 3; ++k) Fo[3 * o + k] = F[3 * f + k];
}

__global__ void mark_used_kernel(const int32_t *__restrict__ F, long nf, int32_t *__restrict__ used) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * nf) used[F[i]] = 1;  // every writer stores the same value
}

__global__ void compact_vertices_kernel(const float *__restrict__ P, const int32_t *__restrict__ used, const int32_t *__restrict__ incl,
                                        long nv, float *__restrict__ Po) {
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nv || !used[u]) return;
    const long o = incl[u] - 1;
    for (int k = 0; k < 3; ++k) Po[3 * o + k] = P[3 * u + k];
}

__global__ void remap_faces_kernel(int32_t *__restrict__ F, long nf, const int32_t *__restrict__ incl) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * nf) F[i] = incl[F[i]] - 1;
}

// first[h] = 1 when h is the lowest half-edge of its edge (the stable sort put it first)
__global__ void first_halfedge_kernel(Topo T, int32_t *__restrict__ first) {
    const long h = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (h < 3 * T.nf) first[h] = T.she[T.es[T.fe[h]]] == (int)h;
}

// remesh_host.h subdivide_once: edge vertices numbered after the old ones in order of first appearance over the faces
// (rank_incl: inclusive prefix sum of first[]), face (a, b, c) -> (a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)
__global__ void subdivide_kernel(Topo T, const float *__restrict__ P, const int32_t *__restrict__ rank_incl, float *__restrict__ Po,
                                 int32_t *__restrict__ Fo) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < T.nv)
        for (int k = 0; k < 3; ++k) Po[3 * i + k] = P[3 * i + k];
    if (i < T.ne) {
        const int h = T.she[T.es[i]];
        int u, v;
        edge_ends(T, (int)i, u, v);
        float m[3];
        midpoint(P, u, v, m);
        const long o = T.nv + rank_incl[h] - 1;
        for (int k = 0; k < 3; ++k) Po[3 * o + k] = m[k];
    }
    if (i < T.nf) {
        const int a = T.F[3 * i], b = T.F[3 * i + 1], c = T.F[3 * i + 2];
        int mid[3];
        for (int k = 0; k < 3; ++k) mid[k] = (int)(T.nv + rank_incl[T.she[T.es[T.fe[3 * i + k]]]] - 1);
        const int ab = mid[0], bc = mid[1], ca = mid[2];
        const int t[12] = {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca};
        for (int k = 0; k < 12; ++k) Fo[12 * i + k] = t[k];
    }
}

// bit 0: a face index out of range, bit 1: a repeated index in a face, bit 2: a non-finite position
__global__ void validate_kernel(const float *__restrict__ P, long nv, const int32_t *__restrict__ F, long nf, int32_t *__restrict__ status) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int s = 0;
    if (i < nf) {
        const int a = F[3 * i], b = F[3 * i + 1], c = F[3 * i + 2];
        if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) s |= 1;
        if (a == b || b == c || a == c) s |= 2;
    }
    if (i < nv && !(isfinite(P[3 * i]) && isfinite(P[3 * i + 1]) && isfinite(P[3 * i + 2]))) s |= 4;
    if (s) atomicOr(status, s);
}

__global__ void halfedge_lengths_kernel(const float *__restrict__ P, const int32_t *__restrict__ F, long nf, double *__restrict__ len) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    double s = 0;
    for (int k = 0; k < 3; ++k) s += norm(ld(P, F[3 * f + k]) - ld(P, F[3 * f + (k + 1) % 3]));
    len[f] = s;
}

}  // namespace

extern "C" {

int sculpt_rmd_halfedge_keys(const int32_t *F, int64_t nf, int64_t *keys, sculpt_stream_t stream) {
    SC_REQUIRE(nf >= 0 && 3 * nf < ((int64_t)1 << 31), "rmd_halfedge_keys: nf=%lld out of range", (long long)nf);
    RMD_LAUNCH(halfedge_keys_kernel, 3 * nf, F, (long)nf, keys);
    return 0;
}

int sculpt_rmd_edge_heads(const int64_t *skeys, int64_t nh, int32_t *head, sculpt_stream_t stream) {
    RMD_LAUNCH(edge_heads_kernel, nh, skeys, (long)nh, head);
    return 0;
}

int sculpt_rmd_edge_fill(const int64_t *sperm, const int32_t *eid_incl, int64_t nh, int32_t *she, int32_t *fe, int32_t *es,
                         sculpt_stream_t stream) {
    RMD_LAUNCH(edge_fill_kernel, nh, sperm, eid_incl, (long)nh, she, fe, es);
    return 0;
}

int sculpt_rmd_boundary(const sculpt_rmd_topo_t *topo, uint8_t *bnd, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_boundary")) return rc;
    RMD_LAUNCH(boundary_kernel, topo->ne, topo_of(topo), bnd);
    return 0;
}

int sculpt_rmd_high_valence(const sculpt_rmd_topo_t *topo, uint8_t *flags, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_high_valence")) return rc;
    RMD_LAUNCH(high_valence_kernel, topo->nv, topo_of(topo), flags);
    return 0;
}

int sculpt_rmd_collapse_propose(const sculpt_rmd_topo_t *topo, const float *P, int mode, double low, double high,
                                unsigned long long *claim, unsigned long long *cand, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_collapse_propose")) return rc;
    SC_REQUIRE(mode == 0 || mode == 1, "rmd_collapse_propose: mode=%d", mode);
    RMD_LAUNCH(collapse_propose_kernel, topo->ne, topo_of(topo), P, mode, low, high, claim, cand);
    return 0;
}

int sculpt_rmd_collapse_select(const sculpt_rmd_topo_t *topo, const float *P, int mode, const unsigned long long *claim,
                               const unsigned long long *cand, int32_t *win, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_collapse_select")) return rc;
    RMD_LAUNCH(collapse_select_kernel, topo->ne, topo_of(topo), P, mode, claim, cand, win);
    return 0;
}

int sculpt_rmd_collapse_apply(const sculpt_rmd_topo_t *topo, float *P, int32_t *F, int mode, const int32_t *win, uint8_t *face_alive,
                              sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_collapse_apply")) return rc;
    SC_REQUIRE(F == topo->F, "rmd_collapse_apply: F must be the topology's face array");
    RMD_LAUNCH(collapse_apply_kernel, topo->ne, topo_of(topo), P, F, mode, win, face_alive);
    return 0;
}

int sculpt_rmd_flip_propose(const sculpt_rmd_topo_t *topo, const float *P, unsigned long long *claim, unsigned long long *cand,
                            sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_flip_propose")) return rc;
    RMD_LAUNCH(flip_propose_kernel, topo->ne, topo_of(topo), P, claim, cand);
    return 0;
}

int sculpt_rmd_flip_apply(const sculpt_rmd_topo_t *topo, const float *P, const unsigned long long *claim,
                          const unsigned long long *cand, int32_t *F, int32_t *win, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_flip_apply")) return rc;
    SC_REQUIRE(F == topo->F, "rmd_flip_apply: F must be the topology's face array");
    RMD_LAUNCH(flip_select_kernel, topo->ne, topo_of(topo), P, claim, cand, win);
    RMD_LAUNCH(flip_apply_kernel, topo->ne, topo_of(topo), P, win, F);
    return 0;
}

int sculpt_rmd_split_mark(const sculpt_rmd_topo_t *topo, const float *P, double high, int32_t *mark, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_split_mark")) return rc;
    RMD_LAUNCH(split_mark_kernel, topo->ne, topo_of(topo), P, high, mark);
    return 0;
}

int sculpt_rmd_split_count(const sculpt_rmd_topo_t *topo, const int32_t *mark, int32_t *cnt, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_split_count")) return rc;
    RMD_LAUNCH(split_count_kernel, topo->nf, topo_of(topo), mark, cnt);
    return 0;
}

int sculpt_rmd_split_emit(const sculpt_rmd_topo_t *topo, float *P, int64_t vcap, const int32_t *mark, const int32_t *mark_incl,
                          const int32_t *off_incl, int64_t fcap, int32_t *Fo, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_split_emit")) return rc;
    SC_REQUIRE(vcap >= topo->nv && fcap >= 0, "rmd_split_emit: capacity below the input");
    RMD_LAUNCH(split_vertices_kernel, topo->ne, topo_of(topo), P, mark, mark_incl, (long)vcap);
    RMD_LAUNCH(split_faces_kernel, topo->nf, topo_of(topo), P, mark, mark_incl, off_incl, (long)fcap, Fo);
    return 0;
}

int sculpt_rmd_grid_count(const float *GP, const int32_t *GF, int64_t gnf, const double *params_host, int32_t *cnt,
                          sculpt_stream_t stream) {
    SC_REQUIRE(params_host, "rmd_grid_count: null params");
    RMD_LAUNCH(grid_count_kernel, gnf, grid_of(GP, GF, (long)gnf, nullptr, nullptr, params_host), cnt);
    return 0;
}

int sculpt_rmd_grid_fill(const float *GP, const int32_t *GF, int64_t gnf, const double *params_host, const int32_t *off_incl,
                         int32_t *cell, int32_t *face, sculpt_stream_t stream) {
    SC_REQUIRE(params_host, "rmd_grid_fill: null params");
    RMD_LAUNCH(grid_fill_kernel, gnf, grid_of(GP, GF, (long)gnf, nullptr, nullptr, params_host), off_incl, cell, face);
    return 0;
}

int sculpt_rmd_relax(const sculpt_rmd_topo_t *topo, const float *P, const float *GP, const int32_t *GF, int64_t gnf,
                     const int32_t *items, const int32_t *start, const double *params_host, int project, float *Q, uint8_t *undo,
                     sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_relax")) return rc;
    SC_REQUIRE(!project || (params_host && (gnf == 0 || (GP && GF && items && start))), "rmd_relax: projection without a grid");
    const Grid G = grid_of(GP, GF, project ? (long)gnf : 0, items, start, project ? params_host : nullptr);
    SC_REQUIRE(((uintptr_t)undo & 3) == 0, "rmd_relax: undo scratch must be 4-byte aligned");
    RMD_LAUNCH(relax_kernel, topo->nv, topo_of(topo), P, G, project, Q);
    if (topo->nf == 0 || topo->nv == 0) return 0;
    hipStream_t st = as_stream(stream);
    SC_HIP(hipMemsetAsync(undo, 0, (size_t)topo->nv, st));
    int32_t *grew = reinterpret_cast<int32_t *>(undo + (SCULPT_RMD_UNDO_BYTES(topo->nv) - 4));
    for (int32_t h = 1; h;) {  // the undo pass to a fixed point: one readback per pass, usually one or two
        h = 0;
        SC_HIP(hipMemsetAsync(grew, 0, sizeof(int32_t), st));
        RMD_LAUNCH(undo_mark_kernel, topo->nf, topo->F, (long)topo->nf, P, Q, undo, grew);
        RMD_LAUNCH(undo_apply_kernel, topo->nv, P, undo, (long)topo->nv, Q);
        SC_HIP(hipMemcpyAsync(&h, grew, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        SC_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

int sculpt_rmd_compact_faces(const int32_t *F, const uint8_t *alive, const int32_t *incl, int64_t nf, int32_t *Fo, sculpt_stream_t stream) {
    RMD_LAUNCH(compact_faces_kernel, nf, F, alive, incl, (long)nf, Fo);
    return 0;
}

int sculpt_rmd_mark_used(const int32_t *F, int64_t nf, int32_t *used, sculpt_stream_t stream) {
    RMD_LAUNCH(mark_used_kernel, 3 * nf, F, (long)nf, used);
    return 0;
}

int sculpt_rmd_compact_vertices(const float *P, const int32_t *used, const int32_t *incl, int64_t nv, float *Po, int32_t *F, int64_t nf,
                                sculpt_stream_t stream) {
    RMD_LAUNCH(compact_vertices_kernel, nv, P, used, incl, (long)nv, Po);
    RMD_LAUNCH(remap_faces_kernel, 3 * nf, F, (long)nf, incl);
    return 0;
}

int sculpt_rmd_first_halfedge(const sculpt_rmd_topo_t *topo, int32_t *first, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_first_halfedge")) return rc;
    RMD_LAUNCH(first_halfedge_kernel, 3 * topo->nf, topo_of(topo), first);
    return 0;
}

int sculpt_rmd_subdivide(const sculpt_rmd_topo_t *topo, const float *P, const int32_t *rank_incl, float *Po, int32_t *Fo,
                         sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "rmd_subdivide")) return rc;
    const long n = (long)std::max(topo->nv, std::max(topo->ne, topo->nf));
    RMD_LAUNCH(subdivide_kernel, n, topo_of(topo), P, rank_incl, Po, Fo);
    return 0;
}

int sculpt_rmd_validate(const float *P, int64_t nv, const int32_t *F, int64_t nf, int32_t *status, sculpt_stream_t stream) {
    SC_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), as_stream(stream)));
    RMD_LAUNCH(validate_kernel, std::max(nv, nf), P, (long)nv, F, (long)nf, status);
    return 0;
}

int sculpt_rmd_halfedge_lengths(const float *P, const int32_t *F, int64_t nf, double *len, sculpt_stream_t stream) {
    RMD_LAUNCH(halfedge_lengths_kernel, nf, P, F, (long)nf, len);
    return 0;
}

}  // extern "C"
