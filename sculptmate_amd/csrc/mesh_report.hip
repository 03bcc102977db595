// What a mesh IS, asked ON THE DEVICE (sculpt_mesh_edge_census, sculpt_mesh_face_measures, sculpt_surface_self_count,
// sculpt_surface_self_emit, include/sculpt_hip.h; driven by sculptmate_amd/ops.py mesh_report / mesh_self_intersections): the edge
// census behind "watertight" and the Euler number, the per-face area and signed volume, and which pairs of faces pass through
// each other.  The unit is compiled with floating-point contraction OFF (the pragma below, before the shared helpers): positions
// are fp32 widened to fp64, each operation rounded on its own, and tests/_reportref.py restates all of it in NumPy.
//
// ---- the rule (the contract) ------------------------------------------------------------------------------------------------
// orient(a, b, c, d) for four vertex INDICES:
//   - if any two of the four indices are equal: 0.  Mandatory, not an optimisation: the determinant of a repeated row does not
//     cancel exactly in floating point, and without this clause neighbouring faces of a clean mesh "intersect";
//   - otherwise, with u = P[b] - P[a], v = P[c] - P[a], w = P[d] - P[a], the sign of
//       (u0 (v1 w2 - v2 w1) - u1 (v0 w2 - v2 w0)) + u2 (v0 w1 - v1 w0)        in exactly that association.
// segment (p, q) MEETS triangle (a, b, c) when both hold:
//   - orient(a, b, c, p) orient(a, b, c, q) < 0, strictly: an end point in the plane does not count, which is what keeps faces
//     that share a vertex or an edge from counting;
//   - the three signs orient(p, q, a, b), orient(p, q, b, c), orient(p, q, c, a) are all >= 0 or all <= 0, and not all zero: the
//     triangle is closed, a segment through the shared edge of two triangles meets both.
// faces i < j INTERSECT when both hold:
//   - their fp32 bounding boxes overlap, both ends closed (the box clause is part of the rule, as in the ray and winding families);
//   - some edge (F[i][k], F[i][(k + 1) % 3]) meets triangle (F[j][0], F[j][1], F[j][2]), or some edge of j meets triangle i,
//     k = 0, 1, 2.
// One rule for all pairs, no adjacency special case.  What is NOT claimed: coplanar overlaps are not reported; a soup that repeats
// positions under different indices is judged by the arithmetic alone; geometric truth holds only where the arithmetic is exact
// (small-integer coordinates, where the tests pin it).
//
// Edge census, over the undirected sorted half-edge keys of the topology (sculpt_rmd_topo_t): an edge with 1 half-edge is a border
// edge, with >= 3 non-manifold, with exactly 2 that START AT THE SAME VERTEX inconsistently wound.  A face with a repeated index
// contributes its half-edges like any other, self-loops included.  A vertex is referenced when a face names it.  All integers:
// a ballot per wave, a sum per workgroup, one integer atomic per workgroup and figure.
//
// Per-face measures, fp64: area2[f] = |cross(b - a, c - a)| (csrc/mesh_distance.hip area_kernel's value: the same helpers, the
// same association), vol6[f] = (a0 (b1 c2 - b2 c1) - a1 (b0 c2 - b2 c0)) + a2 (b0 c1 - b1 c0); a face is degenerate when it repeats
// an index or area2 == 0.  The totals are the caller's fp64 sums.
//
// ---- acceleration (only decides which pairs are SKIPPED) ---------------------------------------------------------------------
// The remesher's uniform grid (surface_grid.h) lists a face in EVERY cell of its box's cell range (grid_fill_kernel).  Face i
// walks the cells of its own range and looks at the listed j > i.  A pair whose boxes overlap shares the cells
// max(lo_i, lo_j) .. min(hi_i, hi_j) per axis -- not empty: the cell of a coordinate is one monotone function for every face,
// clamps included, so mn_i <= mx_j gives lo_i <= hi_j -- and is evaluated only in the FIRST of them, the component-wise maximum
// of the two boxes' lowest cells: each pair is tested once, however many cells it shares.  A pair whose boxes do not overlap
// fails the box clause wherever it is met.
//
// ---- two phases, two forms -----------------------------------------------------------------------------------------------------
// sculpt_surface_self_count writes n[i] = the number of j > i that intersect i, and sets flag[i] and flag[j] (uint8, every writer
// stores 1).  The caller scans n and reads the total; sculpt_surface_self_emit walks again and writes the keys i << 32 | j at
// offsets[i] ..; the caller sorts them.  SCULPT_DISTANCE_FORM (read by ops.mesh_self_intersections):
//   plain     one thread per face in input order; j's box from its corners through the indices.
//   default   faces in the order of their first cell (`order`), so that a wave walks neighbouring lists; j's box from the packed
//             64-byte records (sculpt_surface_pack), whose first two 16-byte loads hold it.
// After the box clause both read j's indices from F (the index clause needs them) and the positions from P: the same integers on
// every input.  Every loop is bounded by a list length or a cell range; nothing waits on another thread.
#pragma clang fp contract(off)

#include "remesh_topo.h"
#include "surface_grid.h"
#include "block_scan.h"

namespace {

constexpr int kWaves = kThreads / 64;

// ---- edge census -------------------------------------------------------------------------------------------------------------
enum { kEdges = 0, kBorder = 1, kNonManifold = 2, kInconsistent = 3, kReferenced = 4, kCensusWords = 8 };

__global__ void __launch_bounds__(kThreads) census_kernel(Topo T, unsigned long long *__restrict__ counts) {
    __shared__ unsigned s_w[4][kWaves];
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool border = false, nonmanifold = false, inconsistent = false, referenced = false;
    if (t < T.ne) {
        const int first = T.es[t], c = T.es[t + 1] - first;
        border = c == 1;
        nonmanifold = c >= 3;
        if (c == 2) inconsistent = T.F[T.she[first]] == T.F[T.she[first + 1]];  // half-edge h = 3 f + k starts at F[h]
    }
    if (t < T.nv) referenced = T.vfs[t + 1] > T.vfs[t];
    const unsigned nb = block_flag_count<kWaves>(border, s_w[0]);
    const unsigned nn = block_flag_count<kWaves>(nonmanifold, s_w[1]);
    const unsigned ni = block_flag_count<kWaves>(inconsistent, s_w[2]);
    const unsigned nr = block_flag_count<kWaves>(referenced, s_w[3]);
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) atomicAdd(&counts[kEdges], (unsigned long long)T.ne);
        if (nb) atomicAdd(&counts[kBorder], (unsigned long long)nb);
        if (nn) atomicAdd(&counts[kNonManifold], (unsigned long long)nn);
        if (ni) atomicAdd(&counts[kInconsistent], (unsigned long long)ni);
        if (nr) atomicAdd(&counts[kReferenced], (unsigned long long)nr);
    }
}

// ---- per-face measures ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
measures_kernel(const float *__restrict__ P, const int32_t *__restrict__ F, long nf, double *__restrict__ area2, double *__restrict__ vol6,
                unsigned long long *__restrict__ n_degenerate) {
    __shared__ unsigned s_w[kWaves];
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool degenerate = false;
    if (f < nf) {
        const int ia = F[3 * f], ib = F[3 * f + 1], ic = F[3 * f + 2];
        const D3 a = ld(P, ia), b = ld(P, ib), c = ld(P, ic);
        const double a2 = norm(face_normal(P, F, (int)f));
        area2[f] = a2;
        vol6[f] = (a.x * (b.y * c.z - b.z * c.y) - a.y * (b.x * c.z - b.z * c.x)) + a.z * (b.x * c.y - b.y * c.x);
        degenerate = ia == ib || ib == ic || ia == ic || a2 == 0.0;
    }
    const unsigned nd = block_flag_count<kWaves>(degenerate, s_w);
    if (threadIdx.x == 0 && nd) atomicAdd(n_degenerate, (unsigned long long)nd);
}

// ---- the pair rule -------------------------------------------------------------------------------------------------------------
// Six corners of a pair: slots 0 .. 2 are face i's, 3 .. 5 face j's.  Every slot number below is a compile-time constant after
// inlining, so the arrays live in registers.
struct Pair {
    D3 X[6];
    int id[6];
};

__device__ __forceinline__ int orient(const Pair &q, int a, int b, int c, int d) {
    const int ia = q.id[a], ib = q.id[b], ic = q.id[c], id = q.id[d];
    if (ia == ib || ia == ic || ia == id || ib == ic || ib == id || ic == id) return 0;
    const D3 u = q.X[b] - q.X[a], v = q.X[c] - q.X[a], w = q.X[d] - q.X[a];
    const double det = (u.x * (v.y * w.z - v.z * w.y) - u.y * (v.x * w.z - v.z * w.x)) + u.z * (v.x * w.y - v.y * w.x);
    return (det > 0.0) - (det < 0.0);
}

// segment (p, q) meets triangle (a, b, c); sp, sq = orient(a, b, c, p), orient(a, b, c, q), which the edges of a face share
__device__ __forceinline__ bool segment_meets(const Pair &x, int p, int q, int a, int b, int c, int sp, int sq) {
    if (sp * sq >= 0) return false;
    const int s0 = orient(x, p, q, a, b), s1 = orient(x, p, q, b, c), s2 = orient(x, p, q, c, a);
    const bool ge = s0 >= 0 && s1 >= 0 && s2 >= 0, le = s0 <= 0 && s1 <= 0 && s2 <= 0;
    return (ge || le) && (s0 != 0 || s1 != 0 || s2 != 0);
}

// some edge of the face at slots e .. e + 2 meets the triangle at slots t .. t + 2
template <int E, int T>
__device__ __forceinline__ bool edges_meet(const Pair &x) {
    const int s0 = orient(x, T, T + 1, T + 2, E), s1 = orient(x, T, T + 1, T + 2, E + 1), s2 = orient(x, T, T + 1, T + 2, E + 2);
    return segment_meets(x, E, E + 1, T, T + 1, T + 2, s0, s1) || segment_meets(x, E + 1, E + 2, T, T + 1, T + 2, s1, s2) ||
           segment_meets(x, E + 2, E, T, T + 1, T + 2, s2, s0);
}

__device__ inline bool pair_meets(const float *__restrict__ P, const int fi[3], const int32_t *__restrict__ F, long j) {
    Pair x;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x.id[k] = fi[k];
        x.id[3 + k] = F[3 * j + k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) x.X[k] = ld(P, x.id[k]);
    return edges_meet<0, 3>(x) || edges_meet<3, 0>(x);
}

__device__ inline void face_box(const float *__restrict__ P, const int32_t *__restrict__ F, long f, float mn[3], float mx[3]) {
    const long ia = F[3 * f], ib = F[3 * f + 1], ic = F[3 * f + 2];
    for (int k = 0; k < 3; ++k) {
        const float a = P[3 * ia + k], b = P[3 * ib + k], c = P[3 * ic + k];
        mn[k] = fminf(a, fminf(b, c));
        mx[k] = fmaxf(a, fmaxf(b, c));
    }
}

template <bool kPacked>
__device__ inline void load_box(const Grid &G, const float4 *__restrict__ rec, long f, float mn[3], float mx[3]) {
    if (kPacked) {
        const float4 r0 = rec[4 * f], r1 = rec[4 * f + 1];
        mn[0] = r0.x, mn[1] = r0.y, mn[2] = r0.z, mx[0] = r0.w, mx[1] = r1.x, mx[2] = r1.y;
    } else {
        face_box(G.P, G.F, f, mn, mx);
    }
}

// kEmit false: n[i] and the flags; true: the keys of face i at offsets[i] .. offsets[i + 1], never past `cap`
template <bool kPacked, bool kEmit>
__global__ void __launch_bounds__(kThreads)
self_kernel(Grid G, const float4 *__restrict__ rec, const int64_t *__restrict__ order, int32_t *__restrict__ n, uint8_t *__restrict__ flag,
            const int64_t *__restrict__ offsets, int64_t *__restrict__ keys, long cap) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= G.nf) return;
    const long i = kPacked ? (long)order[t] : t;
    if (i < 0 || i >= G.nf) return;
    float mn[3], mx[3];
    load_box<kPacked>(G, rec, i, mn, mx);
    int lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = grid_clamp(((double)mn[k] - G.lo[k]) / G.cell, G.n[k]);
        hi[k] = grid_clamp(((double)mx[k] - G.lo[k]) / G.cell, G.n[k]);
    }
    const int fi[3] = {G.F[3 * i], G.F[3 * i + 1], G.F[3 * i + 2]};
    int count = 0;
    long at = kEmit ? (long)offsets[i] : 0;
    const long stop = kEmit ? min((long)offsets[i + 1], cap) : 0;
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y)
            for (int x = lo[0]; x <= hi[0]; ++x) {
                const long ci = ((long)z * G.n[1] + y) * G.n[0] + x;
                const int end = G.start[ci + 1];
#pragma nounroll  // unrolled, the fp64 pair test of several listings at once spills (DESIGN.md 3.3m saw 256 VGPRs)
                for (int it = G.start[ci]; it < end; ++it) {
                    const long j = G.items[it];
                    if (j <= i || j >= G.nf) continue;
                    float jn[3], jx[3];
                    load_box<kPacked>(G, rec, j, jn, jx);
                    if (!(mn[0] <= jx[0] && jn[0] <= mx[0] && mn[1] <= jx[1] && jn[1] <= mx[1] && mn[2] <= jx[2] && jn[2] <= mx[2]))
                        continue;                                                       // the box clause
                    const int c0 = max(lo[0], grid_clamp(((double)jn[0] - G.lo[0]) / G.cell, G.n[0]));
                    const int c1 = max(lo[1], grid_clamp(((double)jn[1] - G.lo[1]) / G.cell, G.n[1]));
                    const int c2 = max(lo[2], grid_clamp(((double)jn[2] - G.lo[2]) / G.cell, G.n[2]));
                    if (x != c0 || y != c1 || z != c2) continue;                        // not the pair's first common cell
                    if (!pair_meets(G.P, fi, G.F, j)) continue;
                    if (kEmit) {
                        if (at < stop) keys[at++] = (int64_t)(((uint64_t)i << 32) | (uint64_t)j);
                    } else {
                        ++count;
                        flag[j] = 1;
                    }
                }
            }
    if (!kEmit) {
        n[i] = count;
        if (count) flag[i] = 1;
    }
}

int check_self(const char *who, const float *GP, const int32_t *GF, int64_t gnf, const int64_t *order, const float *records,
               const int32_t *items, const int32_t *start, const double *params_host) {
    if (int rc = check_grid(who, GP, GF, gnf, params_host)) return rc;
    SC_REQUIRE((order == nullptr) == (records == nullptr), "%s: the sorted form takes both the order and the records", who);
    SC_REQUIRE(gnf == 0 || (items && start), "%s: null grid lists", who);
    SC_REQUIRE(!records || aligned16(records), "%s: records not 16-byte aligned", who);
    return 0;
}

}  // namespace

extern "C" {

int sculpt_mesh_edge_census(const sculpt_rmd_topo_t *topo, int64_t *counts, sculpt_stream_t stream) {
    if (int rc = check_topo(topo, "mesh_edge_census")) return rc;
    SC_REQUIRE(counts, "mesh_edge_census: null counts");
    SC_REQUIRE(topo->nv == 0 || topo->vfs, "mesh_edge_census: null vertex table");
    SC_HIP(hipMemsetAsync(counts, 0, kCensusWords * sizeof(int64_t), as_stream(stream)));
    const long n = (long)std::max(topo->ne, topo->nv);
    RMD_LAUNCH(census_kernel, n, topo_of(topo), reinterpret_cast<unsigned long long *>(counts));
    return 0;
}

int sculpt_mesh_face_measures(const float *P, const int32_t *F, int64_t nf, double *area2, double *vol6, int64_t *n_degenerate,
                              sculpt_stream_t stream) {
    SC_REQUIRE(nf >= 0 && 3 * nf < ((int64_t)1 << 31), "mesh_face_measures: %lld faces do not fit int32 indices", (long long)nf);
    SC_REQUIRE(n_degenerate, "mesh_face_measures: null count");
    SC_HIP(hipMemsetAsync(n_degenerate, 0, sizeof(int64_t), as_stream(stream)));
    if (nf == 0) return 0;
    SC_REQUIRE(P && F && area2 && vol6, "mesh_face_measures: null array");
    RMD_LAUNCH(measures_kernel, nf, P, F, (long)nf, area2, vol6, reinterpret_cast<unsigned long long *>(n_degenerate));
    return 0;
}

int sculpt_surface_self_count(const float *GP, const int32_t *GF, int64_t gnf, const int64_t *order, const float *records,
                              const int32_t *items, const int32_t *start, const double *params_host, int32_t *n, uint8_t *flag,
                              sculpt_stream_t stream) {
    if (int rc = check_self("surface_self_count", GP, GF, gnf, order, records, items, start, params_host)) return rc;
    if (gnf == 0) return 0;
    SC_REQUIRE(n && flag, "surface_self_count: null array");
    const Grid G = grid_of(GP, GF, (long)gnf, items, start, params_host);
    if (order)
        RMD_LAUNCH((self_kernel<true, false>), gnf, G, reinterpret_cast<const float4 *>(records), order, n, flag, nullptr, nullptr, 0L);
    else
        RMD_LAUNCH((self_kernel<false, false>), gnf, G, nullptr, nullptr, n, flag, nullptr, nullptr, 0L);
    return 0;
}

int sculpt_surface_self_emit(const float *GP, const int32_t *GF, int64_t gnf, const int64_t *order, const float *records,
                             const int32_t *items, const int32_t *start, const double *params_host, const int64_t *offsets,
                             int64_t *keys, int64_t capacity, sculpt_stream_t stream) {
    if (int rc = check_self("surface_self_emit", GP, GF, gnf, order, records, items, start, params_host)) return rc;
    SC_REQUIRE(capacity >= 0, "surface_self_emit: capacity=%lld", (long long)capacity);
    if (gnf == 0 || capacity == 0) return 0;
    SC_REQUIRE(offsets && keys, "surface_self_emit: null array");
    const Grid G = grid_of(GP, GF, (long)gnf, items, start, params_host);
    if (order)
        RMD_LAUNCH((self_kernel<true, true>), gnf, G, reinterpret_cast<const float4 *>(records), order, nullptr, nullptr, offsets, keys,
                   (long)capacity);
    else
        RMD_LAUNCH((self_kernel<false, true>), gnf, G, nullptr, nullptr, nullptr, nullptr, offsets, keys, (long)capacity);
    return 0;
}

}  // extern "C"
