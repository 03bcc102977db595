// Inside / outside of a triangle surface ON THE DEVICE (sculpt_surface_winding*, sculpt_lattice_active_corners, sculpt_sdf_fill,
// include/sculpt_hip.h; driven by sculptmate_amd/ops.py mesh_winding / mesh_contains / mesh_signed_distance / mesh_sdf_grid /
// mesh_voxel_remesh): an INTEGER winding count of a point along the three coordinate axes with a watertight crossing rule, the
// sign lattice of a voxel grid, the lattice points marching cubes will read, and the banded signed-distance volume.  The unit
// is compiled with floating-point contraction OFF (the pragma below, before the shared helpers): everything is fp64 on fp32
// inputs widened, each operation rounded on its own, and tests/_windref.py restates it in NumPy bit for bit.
//
// ---- the rule (the contract) ------------------------------------------------------------------------------------------------
// For a query p, an axis a in {0, 1, 2} with u = (a + 1) % 3, v = (a + 2) % 3, and a face with corners A, B, C:
//   1 Box clause (part of the rule, as in the ray family).  The face takes part only if min_u <= p_u <= max_u and
//     min_v <= p_v <= max_v: min and max over the three fp32 corners, both ends closed, compared as fp32 values.
//   2 Translate.  A' = A - p, B' = B - p, C' = C - p, per component.
//   3 Edge sign.  sgn(X', Y') of a directed edge uses e = X'_u Y'_v - X'_v Y'_u (two products, one difference).
//       e != 0:                  sign(e)
//       else Y'_v - X'_v != 0:   -sign(Y'_v - X'_v)
//       else:                    sign(Y'_u - X'_u), which may be 0
//     This is the symbolic perturbation of p by (eps, eps^2) in (u, v).  It is antisymmetric under swapping the end points, as
//     e itself is in IEEE arithmetic: two faces that traverse a shared edge in opposite directions always see opposite signs.
//   4 Agreement.  s_A = sgn(B', C') with e_A its e, s_B = sgn(C', A') with e_B, s_C = sgn(A', B') with e_C.  The face is crossed
//     only if s_A == s_B == s_C != 0; call that common sign s.
//   5 Ahead.  T = (e_A A'_a + e_B B'_a) + e_C C'_a.  The crossing counts only if T s > 0, strictly: a point on the surface is
//     not ahead of it.
//   6 Count.  w_a(p) = the sum of s over all faces that pass 1, 4 and 5, as an int32.  No fp32 input can overflow any of this
//     in fp64, and the sum is over integers: thread order, atomics and the form of the kernel cannot change it.
//
// ---- consequences -----------------------------------------------------------------------------------------------------------
//   - a closed surface wound counter-clockwise seen from outside gives w_a = +1 inside and 0 outside on all three axes; wound
//     inward, -1 inside; traversed twice, +-2; an open surface gives axes that may disagree;
//   - inside(p) holds iff at least two of the three w_a are nonzero (the majority vote; it ignores orientation);
//   - a non-finite query gives w = (INT32_MIN, INT32_MIN, INT32_MIN) and inside = false, and the grid is never entered;
//   - no faces gives zeros; n == 0 launches nothing.
// What is NOT claimed: with rounding, the pairwise antisymmetry of 3 is exact, but the consistency of the signs of all the edges
// around one vertex is exact only when the arithmetic is (small-integer coordinates, where the tests pin it).  On general
// coordinates a ray within rounding of a vertex may be counted once too often or once too seldom on that axis.
//
// ---- acceleration (only decides which faces are SKIPPED) -------------------------------------------------------------------
// The remesher's uniform grid (surface_grid.h) lists a face in every cell of its box range.  For axis a the kernel walks the
// column of cells (cell(p_u), cell(p_v), i) from i = cell(p_a) to n_a - 1, cells clamped as grid_clamp does, and evaluates a
// face only at i == max(lo_a(face), cell(p_a)): its first listing in the walk.  Nothing is lost:
//   (a) by the box clause a face that can count has p_u and p_v inside its box; the cell of a coordinate is the same monotone
//       function for the faces (grid_range) and for p, clamps included, so cell(p_u) and cell(p_v) lie in the face's range and
//       the face is listed in this column at every i of lo_a .. hi_a;
//   (b) a face with max_a <= p_a may be skipped: all of A'_a, B'_a, C'_a are <= 0 (rounding is monotone), every e has the sign
//       s or is 0, so every term of T has the sign -s or is 0 and T s <= 0 exactly.  A face whose hi_a lies below cell(p_a)
//       has max_a < p_a by monotonicity, so the faces the walk never meets are among these.
//
// ---- two forms (SCULPT_DISTANCE_FORM, read by ops.mesh_winding) --------------------------------------------------------------
//   plain     one thread per query in input order, corners read through the indices.
//   default   the queries sorted by grid cell (sculpt_surface_cells + the caller's stable sort); faces come from the packed
//             64-byte records (sculpt_surface_pack), whose first two 16-byte loads hold the box: enough for 1, (b) and lo_a.
// Both run the same steps 2 - 5 on the same fp64 inputs: the same integers on every input (tests/test_gpu_winding.py).
//
// ---- the lattice --------------------------------------------------------------------------------------------------------------
// sculpt_surface_winding_lattice generates its queries in the kernel: lattice point (i0, i1, i2) has x_k = (float)(lo_k + i_k h),
// product and sum in fp64, then one rounding, and gets the counts sculpt_surface_winding gives at those coordinates.  The work
// is shared along the lattice's lines: the points of a line along axis a have the same p_u and p_v, hence the same column of
// cells, the same box clause and the same edge signs for every face; only step 5 differs.  One launch per axis gives a wave a
// line: it walks the column ONCE, its lanes taking 64 listings at a time, and a face whose signs agree is tested against all the
// line's points (lattice_line_kernel).  Both this and the per-point walk equal the sum over all faces, so they agree.  The
// counts int32 [n0][n1][n2][3] are where the three launches meet; a fourth takes the vote: a wave covers 64 consecutive i2 of
// one (i0, i1) row, and its ballot of inside(p) is two words of the sign planes marching cubes takes (uint32 [n0 n1]
// [ceil(n2 / 32)], bit i2 % 32 of word i2 / 32, bits past n2 zero), stored by lane 0 with ordinary stores.
//
// ---- active corners and the fill ----------------------------------------------------------------------------------------------
// A lattice point is ACTIVE iff it is a corner of a cell (2 x 2 x 2 points) whose 8 bits are not all equal: exactly the points
// whose value marching cubes reads.  sculpt_lattice_active_corners lists their linear indices (i0 n1 + i1) n2 + i2 in ascending
// order: a count per workgroup, one workgroup's exclusive scan (block_scan.h), and an emit by rank.
// sculpt_sdf_fill writes +band / -band at every lattice point by its bit, then at listed point j: d = (float)fmin(sqrt(d2[j]),
// band) (a NaN d2 gives band); inside: d if d > 0 else 2^-126; outside: -d.  So (vol > 0) == bit at EVERY lattice point.
#pragma clang fp contract(off)

#include <limits.h>

#include "remesh_topo.h"
#include "surface_grid.h"
#include "block_scan.h"

namespace {

constexpr int kWaves = kThreads / 64;

__device__ inline int sign_of(double x) { return (x > 0.0) - (x < 0.0); }

// step 3: the sign of the directed edge X' -> Y' seen along the axis, and its e
__device__ inline int edge_sign(double xu, double xv, double yu, double yv, double &e) {
    e = xu * yv - xv * yu;
    if (e != 0.0) return sign_of(e);
    const double dv = yv - xv;
    if (dv != 0.0) return -sign_of(dv);
    return sign_of(yu - xu);
}

// steps 2 - 5 for axis A: the face's term of w_A(p), in {-1, 0, +1}
template <int A>
__device__ inline int crossing(const float p[3], const float a[3], const float b[3], const float c[3]) {
    constexpr int U = (A + 1) % 3, V = (A + 2) % 3;
    const double au = (double)a[U] - (double)p[U], av = (double)a[V] - (double)p[V], aa = (double)a[A] - (double)p[A];
    const double bu = (double)b[U] - (double)p[U], bv = (double)b[V] - (double)p[V], ba = (double)b[A] - (double)p[A];
    const double cu = (double)c[U] - (double)p[U], cv = (double)c[V] - (double)p[V], ca = (double)c[A] - (double)p[A];
    double ea, eb, ec;
    const int sa = edge_sign(bu, bv, cu, cv, ea);
    const int sb = edge_sign(cu, cv, au, av, eb);
    const int sc = edge_sign(au, av, bu, bv, ec);
    if (sa == 0 || sa != sb || sb != sc) return 0;
    const double T = (ea * aa + eb * ba) + ec * ca;
    return T * (double)sa > 0.0 ? sa : 0;
}

template <bool kPacked, int A>
__device__ inline int winding_axis(const Grid &G, const float4 *__restrict__ rec, const float p[3], const int c[3]) {
    constexpr int U = (A + 1) % 3, V = (A + 2) % 3;
    int cc[3] = {c[0], c[1], c[2]};
    int sum = 0;
    for (int i = c[A]; i < G.n[A]; ++i) {
        cc[A] = i;
        const long ci = ((long)cc[2] * G.n[1] + cc[1]) * G.n[0] + cc[0];
        const int end = G.start[ci + 1];
#pragma nounroll  // unrolled, the plain form's three axes need 256 VGPRs and spill
        for (int it = G.start[ci]; it < end; ++it) {
            const int f = G.items[it];
            float a[3], b[3], d[3], mn[3], mx[3];
            if (kPacked) {
                const float4 r0 = rec[4 * (long)f], r1 = rec[4 * (long)f + 1];
                mn[0] = r0.x, mn[1] = r0.y, mn[2] = r0.z, mx[0] = r0.w, mx[1] = r1.x, mx[2] = r1.y;
                a[0] = r1.z, a[1] = r1.w;
            } else {
                const long ia = G.F[3 * (long)f], ib = G.F[3 * (long)f + 1], ic = G.F[3 * (long)f + 2];
                for (int k = 0; k < 3; ++k) {
                    a[k] = G.P[3 * ia + k], b[k] = G.P[3 * ib + k], d[k] = G.P[3 * ic + k];
                    mn[k] = fminf(a[k], fminf(b[k], d[k]));
                    mx[k] = fmaxf(a[k], fmaxf(b[k], d[k]));
                }
            }
            if (!(mn[U] <= p[U] && p[U] <= mx[U] && mn[V] <= p[V] && p[V] <= mx[V])) continue;  // the box clause
            if (mx[A] <= p[A]) continue;                                                          // (b)
            const int lo = grid_clamp(((double)mn[A] - G.lo[A]) / G.cell, G.n[A]);
            if (i != max(lo, c[A])) continue;                                                     // not its first listing
            if (kPacked) {
                const float4 r2 = rec[4 * (long)f + 2], r3 = rec[4 * (long)f + 3];
                a[2] = r2.x, b[0] = r2.y, b[1] = r2.z, b[2] = r2.w, d[0] = r3.x, d[1] = r3.y, d[2] = r3.z;
            }
            sum += crossing<A>(p, a, b, d);
        }
    }
    return sum;
}

__device__ inline bool majority(const int w[3]) { return (w[0] != 0) + (w[1] != 0) + (w[2] != 0) >= 2; }

// w[3] of the query p and inside(p): one function for the point kernels and the lattice kernel
template <bool kPacked>
__device__ inline bool winding_at(const Grid &G, const float4 *__restrict__ rec, const float p[3], int w[3]) {
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) {
        w[0] = w[1] = w[2] = INT_MIN;
        return false;
    }
    w[0] = w[1] = w[2] = 0;
    if (G.nf == 0) return false;
    int c[3];
    for (int k = 0; k < 3; ++k) c[k] = grid_clamp(((double)p[k] - G.lo[k]) / G.cell, G.n[k]);
    w[0] = winding_axis<kPacked, 0>(G, rec, p, c);
    w[1] = winding_axis<kPacked, 1>(G, rec, p, c);
    w[2] = winding_axis<kPacked, 2>(G, rec, p, c);
    return majority(w);
}

template <bool kPacked>
__global__ void __launch_bounds__(kThreads)
winding_kernel(Grid G, const float *__restrict__ Q, long n, const int64_t *__restrict__ order, const float4 *__restrict__ rec,
               int32_t *__restrict__ wo) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long j = kPacked ? (long)order[i] : i;
    const float p[3] = {Q[3 * j], Q[3 * j + 1], Q[3 * j + 2]};
    int w[3];
    winding_at<kPacked>(G, rec, p, w);
    wo[3 * j] = w[0], wo[3 * j + 1] = w[1], wo[3 * j + 2] = w[2];
}

struct Lattice {
    double lo[3], h;
    int n[3];
};

constexpr int kLinePoints = 1024 / 64;  // lattice points of a line per lane (a side has at most 1024)

__device__ inline float lattice_coord(const Lattice &L, int k, int i) { return (float)(L.lo[k] + (double)i * L.h); }

// w_A of every point of one lattice line along axis A, by ONE wave (a workgroup of 64): the points share p_u and p_v, so they
// share the column of cells, the box clause and the edge signs of every face; only `ahead` differs from point to point.  The
// lanes take the column's listings 64 at a time (a face at its first listing in the column, i == lo_A); a face whose signs
// agree is handed to all lanes by shuffles, and each lane tests it against its own points: step 5 with the same operands as
// crossing<A>, so the same integers.  The skip (b) is not needed: such a face adds 0.
template <int A>
__global__ void __launch_bounds__(64) lattice_line_kernel(Grid G, const float4 *__restrict__ rec, Lattice L, int32_t *__restrict__ counts) {
    constexpr int U = (A + 1) % 3, V = (A + 2) % 3;
    const int lane = threadIdx.x;
    const long line = blockIdx.x;                      // iu * n_V + iv
    const int iv = (int)(line % L.n[V]), iu = (int)(line / L.n[V]);
    const float pu = lattice_coord(L, U, iu), pv = lattice_coord(L, V, iv);
    int acc[kLinePoints];
#pragma unroll
    for (int j = 0; j < kLinePoints; ++j) acc[j] = 0;
    const bool line_finite = isfinite(pu) && isfinite(pv);
    if (line_finite && G.nf > 0) {
        int cc[3];
        cc[U] = grid_clamp(((double)pu - G.lo[U]) / G.cell, G.n[U]);
        cc[V] = grid_clamp(((double)pv - G.lo[V]) / G.cell, G.n[V]);
        for (int i = 0; i < G.n[A]; ++i) {
            cc[A] = i;
            const long ci = ((long)cc[2] * G.n[1] + cc[1]) * G.n[0] + cc[0];
            const int begin = G.start[ci], end = G.start[ci + 1];
            for (int base = begin; base < end; base += 64) {   // uniform bounds: every lane makes every trip
                const int it = base + lane;
                int s = 0;
                double ea = 0.0, eb = 0.0, ec = 0.0;
                float fa = 0.0f, fb = 0.0f, fc = 0.0f;          // the corners' coordinate along A
                if (it < end) {
                    const long f = G.items[it];
                    const float4 r0 = rec[4 * f], r1 = rec[4 * f + 1];
                    const float mn[3] = {r0.x, r0.y, r0.z}, mx[3] = {r0.w, r1.x, r1.y};
                    const bool box = mn[U] <= pu && pu <= mx[U] && mn[V] <= pv && pv <= mx[V];
                    if (box && i == grid_clamp(((double)mn[A] - G.lo[A]) / G.cell, G.n[A])) {
                        const float4 r2 = rec[4 * f + 2], r3 = rec[4 * f + 3];
                        const float a[3] = {r1.z, r1.w, r2.x}, b[3] = {r2.y, r2.z, r2.w}, c[3] = {r3.x, r3.y, r3.z};
                        const double au = (double)a[U] - (double)pu, av = (double)a[V] - (double)pv;
                        const double bu = (double)b[U] - (double)pu, bv = (double)b[V] - (double)pv;
                        const double cu = (double)c[U] - (double)pu, cv = (double)c[V] - (double)pv;
                        const int sa = edge_sign(bu, bv, cu, cv, ea);
                        const int sb = edge_sign(cu, cv, au, av, eb);
                        const int sc = edge_sign(au, av, bu, bv, ec);
                        if (sa != 0 && sa == sb && sb == sc) s = sa, fa = a[A], fb = b[A], fc = c[A];
                    }
                }
                unsigned long long m = __ballot(s != 0);
                while (m) {                                     // uniform: m is the same in every lane
                    const int src = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int ws = __shfl(s, src, 64);
                    const double wea = __shfl(ea, src, 64), web = __shfl(eb, src, 64), wec = __shfl(ec, src, 64);
                    const double wa = (double)__shfl(fa, src, 64), wb = (double)__shfl(fb, src, 64), wc = (double)__shfl(fc, src, 64);
#pragma unroll
                    for (int j = 0; j < kLinePoints; ++j) {
                        const int k = lane + 64 * j;
                        if (k < L.n[A]) {
                            const double pa = (double)lattice_coord(L, A, k);
                            const double T = (wea * (wa - pa) + web * (wb - pa)) + wec * (wc - pa);
                            if (T * (double)ws > 0.0) acc[j] += ws;
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kLinePoints; ++j) {
        const int k = lane + 64 * j;
        if (k < L.n[A]) {
            int i3[3];
            i3[A] = k, i3[U] = iu, i3[V] = iv;
            const bool finite = line_finite && isfinite(lattice_coord(L, A, k));
            counts[3 * (((long)i3[0] * L.n[1] + i3[1]) * L.n[2] + i3[2]) + A] = finite ? acc[j] : INT_MIN;
        }
    }
}

// the vote: one wave per 64 consecutive i2 of a row (i0, i1); `chunks` waves per row, `words` plane words per row
__global__ void __launch_bounds__(kThreads)
lattice_vote_kernel(const int32_t *__restrict__ counts, int n0, int n1, int n2, int chunks, int words, uint32_t *__restrict__ planes) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long wave = t >> 6;
    const int lane = (int)(t & 63);
    if (wave >= (long)n0 * n1 * chunks) return;  // the whole wave leaves together
    const int chunk = (int)(wave % chunks);
    const long row = wave / chunks;
    const int i2 = chunk * 64 + lane;
    bool in = false;
    if (i2 < n2) {
        const long o = 3 * (row * n2 + i2);
        const int w[3] = {counts[o], counts[o + 1], counts[o + 2]};
        in = w[0] != INT_MIN && majority(w);     // (a non-finite point has INT_MIN on all three axes)
    }
    const unsigned long long m = __ballot(in);
    if (lane == 0) {
        planes[row * words + 2 * chunk] = (uint32_t)m;
        if (2 * chunk + 1 < words) planes[row * words + 2 * chunk + 1] = (uint32_t)(m >> 32);
    }
}

// ---- active corners ----------------------------------------------------------------------------------------------------------
struct Dims {
    int n0, n1, n2, words;
};

// bits i2 - 1, i2, i2 + 1 of row (i0, i1) in bits 0 .. 2; a point outside the lattice reads as 0 (its cells are never tested)
__device__ inline unsigned three_bits(const uint32_t *__restrict__ planes, Dims D, int i0, int i1, int i2) {
    if (i0 < 0 || i0 >= D.n0 || i1 < 0 || i1 >= D.n1) return 0u;
    const uint32_t *row = planes + ((long)i0 * D.n1 + i1) * D.words;
    unsigned r = 0u;
    for (int d = 0; d < 3; ++d) {
        const int z = i2 - 1 + d;
        if (z >= 0 && z < D.n2) r |= ((row[z >> 5] >> (z & 31)) & 1u) << d;
    }
    return r;
}

__device__ inline bool active_corner(const uint32_t *__restrict__ planes, Dims D, long idx) {
    const int i2 = (int)(idx % D.n2);
    const long r = idx / D.n2;
    const int i1 = (int)(r % D.n1), i0 = (int)(r / D.n1);
    unsigned nb[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) nb[a][b] = three_bits(planes, D, i0 - 1 + a, i1 - 1 + b, i2);
    for (int a = 0; a < 2; ++a) {  // the cell with low corner (i0 - 1 + a, i1 - 1 + b, i2 - 1 + c)
        if (i0 - 1 + a < 0 || i0 + a >= D.n0) continue;
        for (int b = 0; b < 2; ++b) {
            if (i1 - 1 + b < 0 || i1 + b >= D.n1) continue;
            for (int c = 0; c < 2; ++c) {
                if (i2 - 1 + c < 0 || i2 + c >= D.n2) continue;
                const unsigned pair = 3u << c;
                const unsigned all = (nb[a][b] & nb[a][b + 1] & nb[a + 1][b] & nb[a + 1][b + 1]) & pair;
                const unsigned any = (nb[a][b] | nb[a][b + 1] | nb[a + 1][b] | nb[a + 1][b + 1]) & pair;
                if (any != 0u && all != pair) return true;
            }
        }
    }
    return false;
}

__global__ void __launch_bounds__(kThreads) corners_count_kernel(const uint32_t *__restrict__ planes, Dims D, long total, int32_t *__restrict__ offs) {
    __shared__ unsigned s_w[kWaves];
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool flag = idx < total && active_corner(planes, D, idx);
    const unsigned cnt = block_flag_count<kWaves>(flag, s_w);
    if (threadIdx.x == 0) offs[blockIdx.x] = (int32_t)cnt;
}

// one workgroup: offs[0 .. nb) -> its exclusive scan, offs[nb] = the total
__global__ void __launch_bounds__(kThreads) corners_scan_kernel(int32_t *__restrict__ offs, int nb) {
    __shared__ int32_t s_w[kWaves];
    const int32_t total = block_scan_in_place<kWaves>(offs, nb, s_w);
    if (threadIdx.x == 0) offs[nb] = total;
}

__global__ void __launch_bounds__(kThreads) corners_emit_kernel(const uint32_t *__restrict__ planes, Dims D, long total, const int32_t *__restrict__ offs,
                                                                int32_t *__restrict__ list, long cap) {
    __shared__ unsigned s_w[kWaves];
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool flag = idx < total && active_corner(planes, D, idx);
    const unsigned rank = block_flag_rank<kWaves>(flag, s_w);
    const long at = (long)offs[blockIdx.x] + rank;
    if (flag && at < cap) list[at] = (int32_t)idx;
}

// ---- the fill ------------------------------------------------------------------------------------------------------------------
__global__ void fill_band_kernel(float *__restrict__ vol, const uint32_t *__restrict__ planes, Dims D, long total, float band) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int i2 = (int)(idx % D.n2);
    const long row = idx / D.n2;
    const bool in = (planes[row * D.words + (i2 >> 5)] >> (i2 & 31)) & 1u;
    vol[idx] = in ? band : -band;
}

__global__ void fill_list_kernel(float *__restrict__ vol, const uint32_t *__restrict__ planes, Dims D, long total, const int32_t *__restrict__ list,
                                 const double *__restrict__ d2, long n, double band) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long idx = list[j];
    if (idx < 0 || idx >= total) return;
    const int i2 = (int)(idx % D.n2);
    const long row = idx / D.n2;
    const bool in = (planes[row * D.words + (i2 >> 5)] >> (i2 & 31)) & 1u;
    const float d = (float)fmin(sqrt(d2[j]), band);
    vol[idx] = in ? (d > 0.0f ? d : 0x1p-126f) : -d;
}

int check_lattice(const char *who, int n0, int n1, int n2) {
    SC_REQUIRE(n0 >= 1 && n0 <= 1024 && n1 >= 1 && n1 <= 1024 && n2 >= 1 && n2 <= 1024, "%s: lattice %d x %d x %d (each side 1 .. 1024)", who,
               n0, n1, n2);
    return 0;
}

}  // namespace

extern "C" {

int sculpt_surface_winding(const float *Q, int64_t n, const int64_t *order, const float *GP, const int32_t *GF, int64_t gnf,
                           const float *records, const int32_t *items, const int32_t *start, const double *params_host, int32_t *w,
                           sculpt_stream_t stream) {
    if (int rc = check_surface_query("surface_winding", n, 0.0 /* the counts take no amax */, gnf, items, start, records, false)) return rc;
    if (int rc = check_grid("surface_winding", GP, GF, gnf, params_host)) return rc;
    SC_REQUIRE((order == nullptr) == (records == nullptr), "surface_winding: the sorted form takes both the order and the records");
    if (n == 0) return 0;
    SC_REQUIRE(Q && w, "surface_winding: null array");
    const Grid G = grid_of(GP, GF, (long)gnf, items, start, params_host);
    if (order)
        RMD_LAUNCH(winding_kernel<true>, n, G, Q, (long)n, order, reinterpret_cast<const float4 *>(records), w);
    else
        RMD_LAUNCH(winding_kernel<false>, n, G, Q, (long)n, nullptr, nullptr, w);
    return 0;
}

int sculpt_surface_winding_lattice(const double *lo_host, double h, int n0, int n1, int n2, const float *GP, const int32_t *GF, int64_t gnf,
                                   const float *records, const int32_t *items, const int32_t *start, const double *params_host,
                                   uint32_t *planes, int32_t *counts, sculpt_stream_t stream) {
    if (int rc = check_lattice("surface_winding_lattice", n0, n1, n2)) return rc;
    if (int rc = check_grid("surface_winding_lattice", GP, GF, gnf, params_host)) return rc;
    SC_REQUIRE(lo_host && planes && counts, "surface_winding_lattice: null array");
    SC_REQUIRE(isfinite(lo_host[0]) && isfinite(lo_host[1]) && isfinite(lo_host[2]) && h > 0 && h < INFINITY,
               "surface_winding_lattice: lo must be finite and h > 0, got h=%g", h);
    SC_REQUIRE(gnf == 0 || (items && start && records && aligned16(records)), "surface_winding_lattice: null grid lists or records (16-byte aligned)");
    const Grid G = grid_of(GP, GF, (long)gnf, items, start, params_host);
    Lattice L;
    for (int k = 0; k < 3; ++k) L.lo[k] = lo_host[k];
    L.h = h;
    L.n[0] = n0, L.n[1] = n1, L.n[2] = n2;
    const int chunks = (n2 + 63) / 64, words = (n2 + 31) / 32;
    const float4 *rec = reinterpret_cast<const float4 *>(records);
    hipLaunchKernelGGL(lattice_line_kernel<0>, dim3(n1 * n2), dim3(64), 0, as_stream(stream), G, rec, L, counts);
    hipLaunchKernelGGL(lattice_line_kernel<1>, dim3(n2 * n0), dim3(64), 0, as_stream(stream), G, rec, L, counts);
    hipLaunchKernelGGL(lattice_line_kernel<2>, dim3(n0 * n1), dim3(64), 0, as_stream(stream), G, rec, L, counts);
    SC_LAUNCH_CHECK();
    const long threads = (long)n0 * n1 * chunks * 64;
    RMD_LAUNCH(lattice_vote_kernel, threads, counts, n0, n1, n2, chunks, words, planes);
    return 0;
}

int64_t sculpt_lattice_active_blocks(int n0, int n1, int n2) {
    if (n0 < 1 || n1 < 1 || n2 < 1 || n0 > 1024 || n1 > 1024 || n2 > 1024) return 0;
    return ((int64_t)n0 * n1 * n2 + kThreads - 1) / kThreads;
}

int sculpt_lattice_active_corners(const uint32_t *planes, int n0, int n1, int n2, int32_t *offsets, int32_t *list, int64_t capacity,
                                  sculpt_stream_t stream) {
    if (int rc = check_lattice("lattice_active_corners", n0, n1, n2)) return rc;
    SC_REQUIRE(planes && offsets, "lattice_active_corners: null array");
    SC_REQUIRE(capacity >= 0 && (list || capacity == 0), "lattice_active_corners: a list of %lld entries without storage", (long long)capacity);
    const Dims D = {n0, n1, n2, (n2 + 31) / 32};
    const long total = (long)n0 * n1 * n2;
    const int nb = blocks(total);
    if (!list) {
        RMD_LAUNCH(corners_count_kernel, total, planes, D, total, offsets);
        hipLaunchKernelGGL(corners_scan_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), offsets, nb);
        SC_LAUNCH_CHECK();
    } else {
        RMD_LAUNCH(corners_emit_kernel, total, planes, D, total, offsets, list, (long)capacity);
    }
    return 0;
}

int sculpt_sdf_fill(float *vol, const uint32_t *planes, int n0, int n1, int n2, const int32_t *list, const double *d2, int64_t n, double band,
                    sculpt_stream_t stream) {
    if (int rc = check_lattice("sdf_fill", n0, n1, n2)) return rc;
    SC_REQUIRE(vol && planes, "sdf_fill: null array");
    SC_REQUIRE(n >= 0 && (n == 0 || (list && d2)), "sdf_fill: %lld listed points without a list or distances", (long long)n);
    SC_REQUIRE(band > 0 && band < INFINITY && (float)band > 0.0f && (float)band < INFINITY, "sdf_fill: band=%g", band);
    const Dims D = {n0, n1, n2, (n2 + 31) / 32};
    const long total = (long)n0 * n1 * n2;
    RMD_LAUNCH(fill_band_kernel, total, vol, planes, D, total, (float)band);
    RMD_LAUNCH(fill_list_kernel, n, vol, planes, D, total, list, d2, (long)n, band);
    return 0;
}

}  // extern "C"
