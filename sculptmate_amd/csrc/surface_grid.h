// The uniform grid over a triangle surface and the closest point of one triangle, shared by the remesher's projection
// (csrc/remesh_device.hip: grid_closest, relax_kernel), the surface distance queries (csrc/mesh_distance.hip) and the ray
// queries (csrc/mesh_ray.hip, which uses the grid and its checks, not the closest point).  One copy;
// every translation unit that includes it gets its own (anonymous namespace).  Include it after remesh_topo.h's D3 helpers and,
// like that file, AFTER `#pragma clang fp contract(off)` in a unit that wants its arithmetic uncontracted: the two units compile
// closest_on_triangle under different contraction settings on purpose (the remesher keeps the bits it always had, the distance
// queries are restated operation for operation in NumPy).
#pragma once

#include "remesh_topo.h"

namespace {

struct Grid {
    const float *P;
    const int32_t *F, *items, *start;
    double lo[3], cell;
    int n[3];
    long nf;
};

__device__ inline int grid_clamp(double q, int n) { return max(0, min(n - 1, (int)floor(q))); }

__device__ void grid_range(const Grid &G, long f, int lo[3], int hi[3]) {
    for (int k = 0; k < 3; ++k) {
        double mn = 1e300, mx = -1e300;
        for (int j = 0; j < 3; ++j) {
            const double c = (double)G.P[3 * G.F[3 * f + j] + k];
            mn = fmin(mn, c);
            mx = fmax(mx, c);
        }
        lo[k] = grid_clamp((mn - G.lo[k]) / G.cell, G.n[k]);
        hi[k] = grid_clamp((mx - G.lo[k]) / G.cell, G.n[k]);
    }
}

// Ericson, Real-Time Collision Detection, 5.1.5 (remesh_host.h closest_on_triangle)
__device__ D3 closest_on_triangle(D3 p, D3 a, D3 b, D3 c) {
    const D3 ab = b - a, ac = c - a, ap = p - a;
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0 && d2 <= 0) return a;
    const D3 bp = p - b;
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0 && d4 <= d3) return b;
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0 && d1 >= 0 && d3 <= 0) return a + (d1 / (d1 - d3)) * ab;
    const D3 cp = p - c;
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0 && d5 <= d6) return c;
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0 && d2 >= 0 && d6 <= 0) return a + (d2 / (d2 - d6)) * ac;
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) return b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) * (c - b);
    const double den = 1.0 / (va + vb + vc);
    return a + (vb * den) * ab + (vc * den) * ac;
}

// the grid of params = {lo x, y, z, cell, nx, ny, nz} (include/sculpt_hip.h sculpt_rmd_grid_*); null params: one unit cell
Grid grid_of(const float *GP, const int32_t *GF, long gnf, const int32_t *items, const int32_t *start, const double *params) {
    Grid G;
    G.P = GP;
    G.F = GF;
    G.items = items;
    G.start = start;
    G.nf = gnf;
    for (int k = 0; k < 3; ++k) {
        G.lo[k] = params ? params[k] : 0.0;
        G.n[k] = params ? (int)params[4 + k] : 1;
    }
    G.cell = params ? params[3] : 1.0;
    return G;
}

// The packed record of face f (sculpt_surface_pack, csrc/mesh_distance.hip), 16 floats as four float4: words 0 .. 5 the box (min
// x, y, z, max x, y, z), words 6 .. 14 the corners a, b, c, word 15 zero.  The corners lie in the last three float4.
__device__ __forceinline__ void face_corners(const float4 *__restrict__ rec, long f, D3 &a, D3 &b, D3 &c) {
    const float4 r1 = rec[4 * f + 1], r2 = rec[4 * f + 2], r3 = rec[4 * f + 3];
    a = {(double)r1.z, (double)r1.w, (double)r2.x};
    b = {(double)r2.y, (double)r2.z, (double)r2.w};
    c = {(double)r3.x, (double)r3.y, (double)r3.z};
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

constexpr int kMaxDirections = 1024;

// what the surface queries (csrc/mesh_distance.hip, csrc/mesh_winding.hip, csrc/mesh_ray.hip) ask of a grid before they launch
inline int check_grid(const char *who, const float *GP, const int32_t *GF, int64_t gnf, const double *params) {
    SC_REQUIRE(gnf >= 0 && 3 * gnf < ((int64_t)1 << 31), "%s: %lld faces do not fit int32 indices", who, (long long)gnf);
    SC_REQUIRE(params, "%s: null grid params", who);
    SC_REQUIRE(gnf == 0 || (GP && GF), "%s: null mesh", who);
    for (int k = 0; k < 3; ++k) SC_REQUIRE(params[4 + k] >= 1 && params[4 + k] <= 1024, "%s: grid side %g (1 .. 1024)", who, params[4 + k]);
    SC_REQUIRE(params[3] > 0 && params[3] < INFINITY, "%s: grid cell %g", who, params[3]);
    return 0;
}

// ... of the n queries themselves: a bad n or amax is refused whatever n is, the grid's lists and the records only when there is
// something to launch (n > 0).  needs_records: the kernel has the packed form only (else null records select the plain form).
inline int check_surface_query(const char *who, int64_t n, double amax, int64_t gnf, const int32_t *items, const int32_t *start,
                               const float *records, bool needs_records) {
    SC_REQUIRE(n >= 0 && 3 * n < ((int64_t)1 << 40), "%s: n=%lld out of range", who, (long long)n);
    SC_REQUIRE(amax >= 0 && amax < INFINITY, "%s: amax=%g", who, amax);  // a NaN fails the comparison
    if (n == 0) return 0;
    SC_REQUIRE(gnf == 0 || (items && start && (records || !needs_records)), "%s: null grid lists%s", who, needs_records ? " or records" : "");
    SC_REQUIRE(aligned16(records), "%s: records not 16-byte aligned", who);
    return 0;
}

// ... and of a set of k rays per query that start `offset` off the point and reach max_distance
inline int check_ray_set(const char *who, int k, float max_distance, float offset) {
    SC_REQUIRE(k >= 1 && k <= kMaxDirections, "%s: %d directions (1 .. %d)", who, k, kMaxDirections);
    SC_REQUIRE(max_distance >= 0, "%s: max_distance=%g", who, (double)max_distance);
    SC_REQUIRE(isfinite(offset), "%s: offset=%g", who, (double)offset);
    return 0;
}

}  // namespace
