// Distance between triangle surfaces ON THE DEVICE (sculpt_surface_*, include/sculpt_hip.h; driven by sculptmate_amd/ops.py
// mesh_closest_points / mesh_sample_surface / mesh_distance): area-uniform sample points on a mesh, and the closest point of a
// mesh to each of N query points.  The unit is compiled with floating-point contraction OFF (the pragma below, before the shared
// helpers), so every value is a fixed sequence of IEEE operations that tests/_distref.py restates in NumPy bit for bit.
//
// ---- closest points: the result contract ------------------------------------------------------------------------------------
// For a query p (fp32, widened to fp64) and the faces 0 .. nf-1 (fp32 corners, widened):
//     q_f  = closest_on_triangle(p, a, b, c)                    surface_grid.h, Ericson 5.1.5
//     d2_f = dot(q_f - p, q_f - p)                              (x x + y y) + z z
//     answer = the lexicographic minimum of (d2_f, f) over ALL faces whose d2_f is not NaN
// (a collinear face can give NaN through 1 / (va + vb + vc); it never wins).  No face, or only NaN: d2 = +inf, face = -1,
// closest = p.  A non-finite query: d2 = NaN, face = -1, closest = p, and the grid is never entered.  The answer is a property
// of the inputs alone: the grid, the order of the threads and the form of the kernel only decide which faces are SKIPPED, and a
// face is skipped only when it provably cannot be that minimum.
//
// ---- why a skipped face cannot win ------------------------------------------------------------------------------------------
// Notation: D_f the exact distance from p to face f, best the least computed d2 so far, S = max(|p|_inf, amax) with amax the
// caller's bound on |coordinate| of every vertex a face names, E = 2^-40 S.
// (A) What is assumed of the evaluation: sqrt(d2_f) >= D_f (1 - 2^-40) - E.  The corners are fp32 values held in fp64, so the
//     differences p - a, b - a, c - a carry at most one rounding of 2^-53 relative, the vertex and edge branches return a corner
//     or a + t ab with 0 <= t <= 1 (monotone rounding), and the last a + ..., q - p and the three products of d2 each add a few
//     units of 2^-53 of |coordinate| <= S.  A few units of 2^-53 S would do for a triangle of ordinary shape; 2^-40 S = 8192 of
//     them leaves room for the cancellation in va, vb, vc of a sliver, and costs nothing: it is 1e-12 of the coordinates, far
//     below a grid cell.  (A needle thin enough to break this bound also breaks any bound: its NaN or wild q_f is then reported
//     by both forms alike only if they evaluate it, which is why the tests hold both forms to the brute force.)
// (B) Shell termination (both forms).  After the Chebyshev shells 0 .. r around p's cell, a face listed in no visited cell has
//     its bounding box outside them.  The cell of a coordinate x is floor(g(x)), g(x) = fl(fl(x - lo) / cell), the same
//     monotone function for the faces (grid_range) and for p; clamping moves a face's range only towards cells that are
//     visited no later.  So for an unvisited face on the + side g(min corner) >= c + r + 1, on the - side
//     g(max corner) < c - r, and its exact distance is at least reach * cell - 2^-51 |x - lo| >= reach * cell - E, where reach =
//     min over the sides that still have cells of (c + r + 1) - g(p) and g(p) - (c - r), computed with one more rounding.
//     The walk stops only when   reach * cell > t,   t = sqrt(best) (1 + 2^-39) + 3 E   (strictly).  Then by (A) an unvisited
//     face has sqrt(d2_f) >= (t - E)(1 - 2^-40) - E > sqrt(best) + E (1 - 2^-39) > sqrt(best): it loses even a tie.  The
//     remesher's `best <= reach * reach` lacks both the slack and the strictness.
// (C) Bounding-box cull (default form).  LB = exact distance from p to the face's axis-aligned box <= D_f.  The record holds
//     the box in fp32 (exact: min / max of fp32 corners); lb = dx dx + dy dy + dz dz in fp32 has relative error below 2^-21
//     (a flush to zero only lowers it).  The face is skipped only when   lb > thr,   thr = (float)(t^2 (1 + 2^-18))
//     (strictly; never `>=`: a face AT the bound may tie with a lower index and must be evaluated).  Then LB^2 >= lb (1 - 2^-21)
//     > t^2 (1 + 2^-18)(1 - 2^-24)(1 - 2^-21) > t^2, and (A) gives sqrt(d2_f) > sqrt(best) as in (B) with t - E replaced by t.
//     thr is refreshed whenever best improves; best = inf gives thr = inf and nothing is skipped.
//
// ---- two forms (SCULPT_DISTANCE_FORM, read by ops.mesh_closest_points) ----------------------------------------------------
//   plain     one thread per query in input order; a face is three index loads and three dependent position gathers.
//   default   the queries sorted by grid cell (sculpt_surface_cells + the caller's stable sort), so that the 64 lanes of a wave
//             walk the same cells and read the same faces: their loads fall on one address and are served as one.  Faces come
//             from a 64-byte record (sculpt_surface_pack: box min, box max, a, b, c, pad -- four aligned 16-byte loads, the
//             first two enough to skip a face) and results are scattered back through the permutation.
// Both evaluate the same closest_on_triangle on the same fp64 inputs, so a face has one d2_f and one q_f; the forms give the
// same bits on every input (tests/test_gpu_mesh_distance.py).
//
// ---- area-uniform samples ----------------------------------------------------------------------------------------------------
// Integer wherever order could matter (tests/_distref.py restates it with Python ints):
//   A2_f = sqrt(cx cx + cy cy + cz cz) of cross(b - a, c - a), fp64; m = max_f A2_f by atomicMax on the bits of the non-negative
//   double; e = frexp exponent of m; B = min(40, 62 - bit_length(nf)); w_f = llrint(ldexp(A2_f, B - e)) <= 2^B (nearest even).
//   cdf = the caller's inclusive int64 prefix sum of w (exact); W = cdf[nf - 1] < 2^62.
//   Sample i takes words 3i, 3i + 1, 3i + 2 of splitmix64(seed): face = first f with cdf[f] > mulhi64(r0, W) (binary search; a
//   zero-weight face is never drawn); u = (r1 >> 40) 2^-24, v = (r2 >> 40) 2^-24, reflected (1 - u, 1 - v) when u + v > 1 in
//   fp32, all exact; point = (a + u (b - a)) + v (c - a) per component in fp32.
#pragma clang fp contract(off)

#include <limits.h>

#include <algorithm>

#include "remesh_topo.h"
#include "surface_grid.h"

namespace {

constexpr double kSlackAbs = 0x1p-40;             // E = kSlackAbs * S
constexpr double kSlackRel = 1.0 + 0x1p-39;
constexpr double kCullRel = 1.0 + 0x1p-18;
constexpr int kRecord = 16;                       // floats per packed face

struct Best {
    double d;
    int f;
    D3 q;
};

__device__ inline void consider(Best &B, D3 p, D3 a, D3 b, D3 c, int f) {
    const D3 q = closest_on_triangle(p, a, b, c);
    const D3 e = q - p;
    const double d = dot(e, e);
    if (d < B.d || (d == B.d && f < B.f)) {  // a NaN fails both
        B.d = d;
        B.f = f;
        B.q = q;
    }
}

// t of (B) / (C) in the header
__device__ inline double guard_radius(double best, double E) { return sqrt(best) * kSlackRel + 3.0 * E; }

__global__ void pack_kernel(const float *__restrict__ P, const int32_t *__restrict__ F, long nf, float4 *__restrict__ rec) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    float c[3][3];
    for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) c[j][k] = P[3 * (long)F[3 * f + j] + k];
    float mn[3], mx[3];
    for (int k = 0; k < 3; ++k) {
        mn[k] = fminf(c[0][k], fminf(c[1][k], c[2][k]));
        mx[k] = fmaxf(c[0][k], fmaxf(c[1][k], c[2][k]));
    }
    rec[4 * f] = make_float4(mn[0], mn[1], mn[2], mx[0]);
    rec[4 * f + 1] = make_float4(mx[1], mx[2], c[0][0], c[0][1]);
    rec[4 * f + 2] = make_float4(c[0][2], c[1][0], c[1][1], c[1][2]);
    rec[4 * f + 3] = make_float4(c[2][0], c[2][1], c[2][2], 0.0f);
}

__device__ inline bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// key = the linear index of the query's (clamped) cell; a non-finite query sorts last and never enters the grid
__global__ void cells_kernel(Grid G, const float *__restrict__ Q, long n, int32_t *__restrict__ key) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = Q[3 * i], y = Q[3 * i + 1], z = Q[3 * i + 2];
    if (!finite3(x, y, z)) {
        key[i] = G.n[0] * G.n[1] * G.n[2];
        return;
    }
    const int cx = grid_clamp(((double)x - G.lo[0]) / G.cell, G.n[0]);
    const int cy = grid_clamp(((double)y - G.lo[1]) / G.cell, G.n[1]);
    const int cz = grid_clamp(((double)z - G.lo[2]) / G.cell, G.n[2]);
    key[i] = (cz * G.n[1] + cy) * G.n[0] + cx;
}

template <bool kPacked>
__global__ void __launch_bounds__(kThreads)
closest_kernel(Grid G, const float *__restrict__ Q, long n, const int64_t *__restrict__ order, const float4 *__restrict__ rec, double amax,
               double *__restrict__ d2o, int32_t *__restrict__ fo, float *__restrict__ co) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long j = kPacked ? (long)order[i] : i;
    const float px = Q[3 * j], py = Q[3 * j + 1], pz = Q[3 * j + 2];
    if (!finite3(px, py, pz)) {
        d2o[j] = NAN;
        fo[j] = -1;
        co[3 * j] = px, co[3 * j + 1] = py, co[3 * j + 2] = pz;
        return;
    }
    const D3 p = {(double)px, (double)py, (double)pz};
    Best B = {INFINITY, INT_MAX, p};
    if (G.nf > 0) {
        const double E = kSlackAbs * fmax(amax, fmax(fabs(p.x), fmax(fabs(p.y), fabs(p.z))));
        const double q[3] = {(p.x - G.lo[0]) / G.cell, (p.y - G.lo[1]) / G.cell, (p.z - G.lo[2]) / G.cell};
        int c[3];
        for (int k = 0; k < 3; ++k) c[k] = grid_clamp(q[k], G.n[k]);
        float thr = INFINITY;
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
                        const int end = G.start[ci + 1];
                        for (int it = G.start[ci]; it < end; ++it) {
                            const int f = G.items[it];
                            if (kPacked) {
                                const float4 r0 = rec[4 * (long)f], r1 = rec[4 * (long)f + 1];
                                const float dx = fmaxf(fmaxf(r0.x - px, px - r0.w), 0.0f);
                                const float dy = fmaxf(fmaxf(r0.y - py, py - r1.x), 0.0f);
                                const float dz = fmaxf(fmaxf(r0.z - pz, pz - r1.y), 0.0f);
                                if (dx * dx + dy * dy + dz * dz > thr) continue;
                                D3 ca, cb, cc;
                                face_corners(rec, f, ca, cb, cc);   // after the box test
                                const double was = B.d;
                                consider(B, p, ca, cb, cc, f);
                                if (B.d < was) {
                                    const double t = guard_radius(B.d, E);
                                    thr = (float)(t * t * kCullRel);
                                }
                            } else {
                                consider(B, p, ld(G.P, G.F[3 * f]), ld(G.P, G.F[3 * f + 1]), ld(G.P, G.F[3 * f + 2]), f);
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
            if (reach == INFINITY) break;  // every cell has been visited
            if (fmax(0.0, reach) * G.cell > guard_radius(B.d, E)) break;
        }
    }
    const bool found = B.f != INT_MAX;
    d2o[j] = B.d;
    fo[j] = found ? B.f : -1;
    co[3 * j] = found ? (float)B.q.x : px;
    co[3 * j + 1] = found ? (float)B.q.y : py;
    co[3 * j + 2] = found ? (float)B.q.z : pz;
}

// ---- samples -----------------------------------------------------------------------------------------------------------------
__global__ void area_kernel(const float *__restrict__ P, const int32_t *__restrict__ F, long nf, double *__restrict__ A2,
                            unsigned long long *__restrict__ m) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bits = 0;
    if (f < nf) {
        const D3 a = ld(P, F[3 * f]), b = ld(P, F[3 * f + 1]), c = ld(P, F[3 * f + 2]);
        const D3 n = cross(b - a, c - a);
        const double v = sqrt(n.x * n.x + n.y * n.y + n.z * n.z);
        A2[f] = v;
        bits = (unsigned long long)__double_as_longlong(v);  // v >= 0: the bits order like the values
    }
    for (int s = 32; s > 0; s >>= 1) {  // every lane of the wave reaches this: one atomic per wave
        const unsigned long long o = __shfl_xor(bits, s);
        bits = o > bits ? o : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(m, bits);
}

__global__ void weight_kernel(const double *__restrict__ A2, long nf, const unsigned long long *__restrict__ m, int B, int64_t *__restrict__ w) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const double mm = __longlong_as_double((long long)*m);
    long long v = 0;
    if (mm > 0 && isfinite(mm)) {
        int e;
        frexp(mm, &e);
        v = llrint(ldexp(A2[f], B - e));
    }
    w[f] = v;
}

__device__ inline uint64_t splitmix64(uint64_t seed, uint64_t j) {
    uint64_t z = seed + (j + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void sample_kernel(const float *__restrict__ P, const int32_t *__restrict__ F, long nf, const int64_t *__restrict__ cdf, long n,
                              uint64_t seed, float *__restrict__ pts, int32_t *__restrict__ face, float *__restrict__ uv) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t W = (uint64_t)cdf[nf - 1];
    const uint64_t r0 = splitmix64(seed, 3 * (uint64_t)i), r1 = splitmix64(seed, 3 * (uint64_t)i + 1), r2 = splitmix64(seed, 3 * (uint64_t)i + 2);
    const uint64_t t = __umul64hi(r0, W);  // < W = cdf[nf - 1]: the search ends on a face
    long lo = 0, hi = nf - 1;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if ((uint64_t)cdf[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    float u = (float)(r1 >> 40) * 0x1p-24f, v = (float)(r2 >> 40) * 0x1p-24f;
    if (u + v > 1.0f) {
        u = 1.0f - u;
        v = 1.0f - v;
    }
    const int ia = F[3 * lo], ib = F[3 * lo + 1], ic = F[3 * lo + 2];
    for (int k = 0; k < 3; ++k) {
        const float a = P[3 * (long)ia + k], b = P[3 * (long)ib + k], c = P[3 * (long)ic + k];
        pts[3 * i + k] = (a + u * (b - a)) + v * (c - a);
    }
    face[i] = (int32_t)lo;
    uv[2 * i] = u, uv[2 * i + 1] = v;
}

}  // namespace

extern "C" {

int sculpt_surface_pack(const float *GP, const int32_t *GF, int64_t gnf, float *records, sculpt_stream_t stream) {
    SC_REQUIRE(gnf >= 0 && 3 * gnf < ((int64_t)1 << 31), "surface_pack: %lld faces do not fit int32 indices", (long long)gnf);
    if (gnf == 0) return 0;
    SC_REQUIRE(GP && GF && records && aligned16(records), "surface_pack: null mesh, or records not 16-byte aligned");
    RMD_LAUNCH(pack_kernel, gnf, GP, GF, (long)gnf, reinterpret_cast<float4 *>(records));
    return 0;
}

int sculpt_surface_cells(const float *Q, int64_t n, const double *params_host, int32_t *key, sculpt_stream_t stream) {
    SC_REQUIRE(n >= 0 && 3 * n < ((int64_t)1 << 40), "surface_cells: n=%lld out of range", (long long)n);
    if (int rc = check_grid("surface_cells", nullptr, nullptr, 0, params_host)) return rc;
    if (n == 0) return 0;
    SC_REQUIRE(Q && key, "surface_cells: null array");
    RMD_LAUNCH(cells_kernel, n, grid_of(nullptr, nullptr, 0, nullptr, nullptr, params_host), Q, (long)n, key);
    return 0;
}

int sculpt_surface_closest(const float *Q, int64_t n, const int64_t *order, const float *GP, const int32_t *GF, int64_t gnf,
                           const float *records, const int32_t *items, const int32_t *start, const double *params_host, double amax,
                           double *d2, int32_t *face, float *closest, sculpt_stream_t stream) {
    if (int rc = check_surface_query("surface_closest", n, amax, gnf, items, start, records, false)) return rc;
    if (int rc = check_grid("surface_closest", GP, GF, gnf, params_host)) return rc;
    SC_REQUIRE((order == nullptr) == (records == nullptr), "surface_closest: the sorted form takes both the order and the records");
    if (n == 0) return 0;
    SC_REQUIRE(Q && d2 && face && closest, "surface_closest: null array");
    const Grid G = grid_of(GP, GF, (long)gnf, items, start, params_host);
    if (order)
        RMD_LAUNCH(closest_kernel<true>, n, G, Q, (long)n, order, reinterpret_cast<const float4 *>(records), amax, d2, face, closest);
    else
        RMD_LAUNCH(closest_kernel<false>, n, G, Q, (long)n, nullptr, nullptr, amax, d2, face, closest);
    return 0;
}

int sculpt_surface_weights(const float *P, const int32_t *F, int64_t nf, double *area2, unsigned long long *max_bits, int64_t *w,
                           sculpt_stream_t stream) {
    SC_REQUIRE(nf >= 0 && 3 * nf < ((int64_t)1 << 31), "surface_weights: %lld faces do not fit int32 indices", (long long)nf);
    if (nf == 0) return 0;
    SC_REQUIRE(P && F && area2 && max_bits && w, "surface_weights: null array");
    int bits = 0;
    for (int64_t x = nf; x; x >>= 1) ++bits;
    SC_HIP(hipMemsetAsync(max_bits, 0, sizeof(unsigned long long), as_stream(stream)));
    RMD_LAUNCH(area_kernel, nf, P, F, (long)nf, area2, max_bits);
    RMD_LAUNCH(weight_kernel, nf, area2, (long)nf, max_bits, std::min(40, 62 - bits), w);
    return 0;
}

int sculpt_surface_sample(const float *P, const int32_t *F, int64_t nf, const int64_t *cdf, int64_t n, unsigned long long seed,
                          float *points, int32_t *face, float *uv, sculpt_stream_t stream) {
    SC_REQUIRE(nf >= 0 && 3 * nf < ((int64_t)1 << 31), "surface_sample: %lld faces do not fit int32 indices", (long long)nf);
    SC_REQUIRE(n >= 0 && 3 * n < ((int64_t)1 << 40), "surface_sample: n=%lld out of range", (long long)n);
    if (n == 0) return 0;
    SC_REQUIRE(nf > 0, "surface_sample: no face to sample");
    SC_REQUIRE(P && F && cdf && points && face && uv, "surface_sample: null array");
    RMD_LAUNCH(sample_kernel, n, P, F, (long)nf, cdf, (long)n, (uint64_t)seed, points, face, uv);
    return 0;
}

}  // extern "C"
