// Rays against a triangle surface ON THE DEVICE (sculpt_surface_ray_cast, sculpt_surface_occlusion, include/sculpt_hip.h; driven
// by sculptmate_amd/ops.py mesh_ray_cast / mesh_occlusion): the closest face a ray hits, and the ambient occlusion of points under
// a shared set of directions.  The unit is compiled with floating-point contraction OFF (the pragma below, before the shared
// helpers), so every value is a fixed sequence of IEEE operations that tests/_rayref.py restates in NumPy bit for bit.
//
// ---- the per-face rule (the contract) ----------------------------------------------------------------------------------------
// Ray (o, d): fp32 widened to fp64.  Corners a, b, c: fp32 widened to fp64.  Range 0 <= tmin <= tmax, tmax may be +inf.  The face
// is two-sided.  dot(x, y) = (x.x y.x + x.y y.y) + x.z y.z, cross as written in remesh_topo.h (two products, one difference).
//     e1 = b - a; e2 = c - a; pv = cross(d, e2); det = dot(e1, pv)
//     miss unless det det > 2^-60 (dot(e1, e1) dot(pv, pv))         (parallel, degenerate, NaN: all misses)
//     inv = 1 / det; tv = o - a; u = dot(tv, pv) inv;               miss unless u >= 0 && u <= 1
//     qv = cross(tv, e1);        v = dot(d, qv) inv;                miss unless v >= 0 && u + v <= 1
//     t = dot(e2, qv) inv;                                          miss unless t >= tmin && t <= tmax
//     h = o + t d (per component: the product rounded, then the sum)
//                                miss unless box_min - E <= h <= box_max + E in every component
// box_min / box_max: the min / max of the fp32 corners; E = 2^-40 S, S = max(|o|_inf, amax), amax the caller's bound on |coordinate|
// of every vertex a face names (as in sculpt_surface_closest).  The BOX CLAUSE is part of the rule, not an optimisation: it makes
// every reported hit a geometric fact -- the computed hit point lies within E of the face's box -- and the grid walk below is
// proven against that fact alone.  A face seen nearly edge-on can give a wild t that "hits" far from the face; the clause
// discards it.  On rays of ordinary shape it discards nothing.  (An infinite t passes t <= +inf and fails the clause.)
// Answer per ray: the lexicographic minimum of (t_f, f) over ALL faces that hit; t, face and (u, v) are the winner's, (u, v)
// rounded once to fp32.  No hit: t = +inf, face = -1, uv = 0.  A zero direction hits nothing.  A non-finite origin or direction:
// t = NaN, face = -1, uv = 0, and the grid is never entered.  Watertightness along shared edges is NOT promised: u, v and
// u + v are rounded per face, so a ray through an edge may pass between the two faces.
// The answer is a property of the inputs alone: the grid, the order of the threads and the form of the kernel only decide which
// faces are SKIPPED, and a face is skipped only when it provably cannot be that minimum.
//
// ---- why a skipped face cannot win -------------------------------------------------------------------------------------------
// Notation: f a face that hits at t_f with computed hit point h; h' = h clamped into f's box, so |h' - h|_inf <= E; best the least
// t found so far (+inf at first); W = 4 E the walk's slack; x(t) = o + t d exactly; a the dominant axis (|d_a| >= |d_k|, d_a != 0).
// What the grid must be: lo_k <= every coordinate of a named vertex <= up_k, up_k = lo_k + n_k cell when n_k < 1024 (the
// remesher's n_k = floor(extent / cell) + 1, up to its roundings of a few 2^-52 S) and up_k = amax when n_k is at its cap.
// (A) Roundings.  |h_k|, |o_k|, |lo_k| <= 2 S and |up_k| <= 4 S, so |h_k - x_k(t_f)| <= 2^-53 (|t_f d_k| + |h_k|) <= 2^-50 S.  A
//     plane parameter t(X) = fl(fl(X - o_k) fl(1 / d_k)) has a relative error below 2^-51, that is |t(X) d_k - (X - o_k)| <= 2^-48 S,
//     and a position fl(o_k + fl(t d_k)) the walk computes at a parameter inside the clipped range is within 2^-49 S of x_k(t).
//     All of these together stay below E = 2^-40 S, which is why W - E = 3 E of room is left on every comparison below.
// (B) Slab lemma (used three times).  If every hit point of f has h_k >= X - E (h_k <= X + E), then t_f is not on the far side
//     of the COMPUTED parameter of the plane X - W (X + W): by (A) x_k(t_f) >= X - E - 2^-50 S, while the computed parameter
//     stands for a plane no higher than X - W + 2^-47 S < X - E - 2^-50 S.  With d_k == 0, h_k = o_k exactly and the test is
//     o_k < X - W.  So: (B1) clipping the ray to [lo - W, up + W] on every axis removes no hit (box clause: h is within E of f's
//     box, which lies inside [lo, up]); a ray that misses those bounds hits nothing.  (B2) The cull of the default form -- the
//     same slab test against f's own box widened by W, over [tmin, min(tmax, best)], f skipped only when the interval is empty
//     STRICTLY (lo_t > hi_t) -- skips no face with t_f <= best.  The box is exact in fp32 (min / max of fp32 corners).
// (C) The walk.  The cell of a coordinate is floor(g(x)) clamped to 0 .. n - 1, g(x) = fl(fl(x - lo) / cell), the same monotone
//     function that lists the faces (grid_range); f is listed in every cell of its box's clamped range, hence in cell(h').
//     The walk steps the cell layers i along a in the direction of d, from the layer of x_a(t0) - W to that of x_a(t1) + W
//     ([t0, t1] the clipped range; signs for d_a > 0); monotone g and (A) put the layer i* of h'_a in between.  For a layer i it
//     takes ts = the computed parameter of the layer's entry plane lo_a + i cell moved W outwards (t0 for the first layer, whose
//     entry side may be the unbounded end layer) and te likewise for the exit plane (t1 for the last layer), te also cut to
//     best.  floor(g(h'_a)) = i* bounds h'_a by the layer's planes up to 2^-49 S, so by (B) ts(i*) <= t_f <= te(i*) unless
//     t_f > best.  In that layer it visits, on each other axis k, the cells from cell(min(p0, p1) - W) to cell(max(p0, p1) + W),
//     p0, p1 the computed positions at ts, te: x_k is linear, so x_k(t_f) lies between x_k(ts) and x_k(te), h'_k within
//     E + 2^-49 S + 2^-50 S < W of it, and monotone g puts cell(h'_k) inside the visited range.  So every face with
//     t_f <= best that is listed in no visited cell of a visited layer does not exist: cell(h') is visited.
//     The walk keeps the minimum over every face it evaluates, wherever the hit lies -- it never asks that the hit be in the
//     current cell -- so evaluating a face early (it is listed in several cells) is harmless.
// (D) Stopping.  ts(i) is monotone along the walk (each operation in it is monotone), and a face whose layer i* is still ahead
//     has t_f >= ts(i*) >= ts(i).  The walk stops before layer i only when ts(i) > best STRICTLY: then every face still ahead
//     has t_f > best and loses.  A face that TIES the best, t_f == best, sits in a layer with ts <= best and is still
//     visited: it may carry a lower index.  `>=` would drop it.  The slack is in ts itself (the plane moved W outwards).
//
// ---- forms (SCULPT_DISTANCE_FORM, read by ops: the family of csrc/mesh_distance.hip) ---------------------------------------
//   plain     one thread per ray in input order; a face is three index loads and three dependent position gathers; no cull.
//   default   the rays sorted by the grid cell of their origin (sculpt_surface_cells + the caller's stable sort); faces come from
//             the packed 64-byte records (sculpt_surface_pack), the first two 16-byte loads enough for the cull (B2).
// Both evaluate the same rule on the same fp64 inputs: the same bits on every input (tests/test_gpu_mesh_ray.py).
//
// ---- occlusion ---------------------------------------------------------------------------------------------------------------
// One thread per point (sorted by cell), a loop over the K directions shared by all points, so the 64 lanes of a wave cast nearly
// the same ray at the same time.  fp32 without contraction: w_k = (n.x D.x + n.y D.y) + n.z D.z; the direction takes part iff
// w_k > 0; origin = p + offset n per component (the product rounded, then the sum); the ray (origin, D_k) over [0, max_distance]
// is occluded iff the rule above reports a face (the walk returns at the first face that hits: best stays +inf until then, so
// nothing is cut short); open = sum of w_k of the rays that hit nothing, all = sum of every taking-part w_k, both in the order of
// k in registers; ao = open / all, 1 when all == 0, NaN for a non-finite p or n.  A non-finite origin or direction hits nothing,
// as in the closest-hit form.  No atomics, no ray is written to memory.
//
// ---- thickness (sculpt_surface_thickness; ops.mesh_thickness, Mesh.thickness, TSR.bake_thickness_map) --------
// The shape diameter of a point: how far the rays of a cone about its INWARD normal travel before they leave the body again.
// Per point p with normal n, the cone set C of K unit vectors about +z shared by all points (ops.thickness_directions), offset,
// max_distance and outward (+1 when the faces wind counter-clockwise seen from outside, else -1).  Steps 1 - 3 and 5 - 6 are fp32
// without contraction, every operation rounded on its own; tests/_thickref.py restates the rule in NumPy and
// ops.mesh_thickness_composed in torch, bit for bit.
//   1  m = unit(n) of the mesh render below.  A non-finite p or n: thickness = thinnest = NaN, valid = 0.  unit does not apply
//      (a zero or overflowing normal): +inf, +inf, 0, nothing is cast.  A surface without faces: +inf, +inf, 0.
//   2  the branch-free orthonormal frame of Duff et al.: sg = copysign(1, m.z), a = -1 / (sg + m.z), b = (m.x m.y) a,
//      T = (1 + (sg (m.x m.x)) a, sg b, -(sg m.x)), B = (b, sg + (m.y m.y) a, -m.y)
//   3  o = p - offset m per component (the product rounded, then the difference)
//   4  per direction j = 0 .. K - 1, in that order: d = (C_j.x T + C_j.y B) - C_j.z m per component; (t, f) = the closest hit of
//      (o, d) over [0, max_distance] by the rule above, exactly what sculpt_surface_ray_cast reports (a non-finite o or d and a
//      zero d hit nothing).  The hit is VALID iff a face was hit and the ray leaves through its back: with g = cross(b - a, c - a)
//      of f's corners in fp64 (as in the snap) and d widened, dot(g, d) outward > 0, strictly.  A ray that enters another body
//      through a front face, or that hits nothing, contributes nothing.
//   5  valid rays only, in registers: dist = fp32(t); w = C_j.z; sw += w; swt += w dist (the product rounded, then the sum);
//      thin = min(thin, dist); valid += 1
//   6  thickness = swt / sw when valid > 0, else +inf; thinnest = thin (+inf when none); valid as int32
// Shape: one lane per point, the points in the order of their grid cell; m, T, B, o and the four accumulators stay in registers
// over the loop; cast<true, false> serves the hit and the corners of the back-face test come from the packed record the walk
// has just read.  Every one of the K rays of every point takes part -- the frame turns the cone onto the point's own normal, so
// no lane idles on a direction its normal excludes, which a shared global set cannot avoid.  Neighbouring points have
// neighbouring normals, so the 64 lanes of a wave cast nearly parallel rays from nearby origins at every j.  Nothing per ray is
// written to memory, no atomics.
// ---- the atlas bake (sculpt_bake_occlusion; ops.bake_occlusion, TSR.bake_occlusion_map) ---------------------
// The occlusion above at every covered texel of a rasterised atlas of a LOW mesh, against the surface S the grid is built over
// (the low mesh itself, or the high-poly surface it was simplified from), in one launch.  Per texel, fp32 unless said otherwise:
//   1  coverage and position p: texel_position (bake_texel.h), index guard included; not covered: ao = 0, mask = 0
//   2  normal n_c = (v_nrm[i0]_c u + v_nrm[i1]_c v) + v_nrm[i2]_c w: sculpt_bake_interpolate's bits on v_nrm
//   3  a non-finite p or n: ao = NaN, mask = 1
//   4  snap, only with cage > 0: c = cage n, o = p + c, d = -c; the closest hit of (o, d) over [0, 2] by the rule above.  No hit
//      (a non-finite o or a zero d included): (q, m) = (p, n).  A hit (t, f): q_k = fp32(o_k + t d_k) (fp64: the product rounded,
//      the sum rounded, then one rounding to fp32); g = cross(b - a, c - a) of f's corners in fp64, negated when dot(g, n) < 0;
//      len = sqrt(dot(g, g)); m = fp32(g / len) per component when 0 < len < inf, else m = n.  cage == 0: (q, m) = (p, n).
//   5  ao = the occlusion above at q with normal m; mask = 1
// Shape: a tile of 32 x 32 texels is read by workgroups of 256, four rast rows per thread, in the order of the sixteen 8 x 8
// sub-blocks (a wave reads one sub-block per pass).  Covered finite texels are ranked in that order (block_scan.h) and compacted
// into LDS as (p, n, where), so the 64 texels of a wave come from at most a few neighbouring 8 x 8 blocks and cast nearly
// parallel rays from nearby origins -- without keys, sort or permutation.  One texel's 64 rays take a lane milliseconds, so a
// lane computes ONE texel: a tile is launched as four workgroups (blockIdx.z), each of which reads the whole tile (64 KB of
// rast, nothing beside the rays), ranks it, keeps ranks 256 z .. 256 z + 255 and ends after the read when it has none.  The
// first of the four writes the texels no list holds (not covered: 0; not finite: NaN).  The tiling only decides where a texel
// is computed: its value depends on its own rast row alone.  What this shape costs against a global sorted list on a
// fragmented atlas (part-filled waves), and what else was measured, is in DESIGN.md 3.3h.
// ---- the mesh render (sculpt_surface_render; ops.mesh_render, Mesh.render, TSR.render_mesh) ------------------
// A camera ray followed to the surface and the hit shaded from the mesh's own attributes and baked maps, in one launch: the
// inverse of every convention the bakes define.  Per ray (o, d), fp32 without contraction unless said otherwise, every operation
// rounded on its own; tests/_meshrenderref.py restates it in NumPy and ops.mesh_render_composed in torch, bit for bit.
//   hit      (t, f, u, v): the closest hit of (o, d) over [0, +inf] by the rule above (cast<true, false>).  A miss, a zero
//            direction and a non-finite origin or direction give the BACKGROUND of every pass; depth is NaN for the non-finite.
//   weights  w1 = fp32(u), w2 = fp32(v), w0 = (1 - w1) - w2.  An attribute with rows A0, A1, A2 -- per vertex through faces[f], or
//            per corner at 3f, 3f+1, 3f+2 -- is (A0 w0 + A1 w1) + A2 w2 (bake_interpolate_kernel's expression order).
//   lookup   of a map of side R (row 0 at the top, C channels) at the interpolated uvs (U, V): X = U R, Y = (1 - V) R -- the
//            inverse of the rasteriser's rule (csrc/baker.hip: texel (x, y) holds the value at (x / R, 1 - y / R)), so X is a texel
//            INDEX, not a texel-centre coordinate.  A non-finite X or Y (every non-finite U or V gives one): X = Y = 0.
//            x0 = floor(X), fx = X - x0, columns x0 and x0 + 1 each clamped to [0, R - 1] AFTER the fraction is taken; y likewise.
//            value = ((T00 (1 - fx) + T10 fx) (1 - fy)) + ((T01 (1 - fx) + T11 fx) fy), Txy the texel of column x., row y.
//            Nothing is read through an unclamped index.
//   albedo   the first the mesh has of: the texture looked up; vertex_colors interpolated (the first three channels); 0.8.
//   g        the geometric normal: cross(b - a, c - a) of f's corners in fp64, each component times `outward`, len =
//            sqrt(dot(g, g)); fp32(g / len) per component when 0 < len < inf, else (0, 0, 0).
//   unit(x)  s = (x.x x.x + x.y x.y) + x.z x.z, len = sqrt(s) (correctly rounded), x / len per component; applies only when
//            0 < len < inf.
//   n        the shading normal, the first of these that applies:
//            1  an object-space normal map: unit(m), m = 2 lookup - 1
//            2  a tangent-space normal map: N, T the corner normals and tangents interpolated un-normalised (csrc/bake_normal.hip),
//               B = s cross(N, T) with s = corner_tangents[3f].w, m = 2 lookup - 1, unit((m.x T + m.y B) + m.z N) per component --
//               the inverse that bake's header promises
//            3  unit(vertex_normals interpolated)
//            4  g
//   a        the occlusion map looked up, else vertex_occlusion interpolated, else 1.
//   passes   color = albedo [1, 1, 1]; opacity = 1 [0]; rgba = (albedo, 1) [0, 0, 0, 0]; depth = fp32(t) [0; NaN]; normal = n
//            [0, 0, 0]; occlusion = a [1]; face = f [-1]; shaded = albedo k [1, 1, 1] with
//            k = ambient a + (1 - ambient) max(0, (n.x l.x + n.y l.y) + n.z l.z), the max 0 unless the dot is > 0, and l the
//            caller's unit light direction or, without one, the headlight unit(-d) ((0, 0, 0) when that does not apply).
// Shape: a wave owns an 8 x 8 pixel tile (rays [n_images][H][W][3]; one row of rays, H == 1, is cut into runs of 64 instead), so
// its 64 rays enter the grid through neighbouring cells and walk the same layers; a workgroup is 2 x 2 such tiles, one ray per
// lane from start to end, idle lanes at the image's edges.  A tile whose rays all miss the grid's bounds ends at the clip (B1).
// The material comes by value as nullable pointers and sizes, so which maps exist is a wave-uniform branch on kernel arguments,
// and it is read only in the second phase, after the walk has its final hit.  Only the passes whose pointer is given are
// computed and stored.  The value of a ray depends on that ray alone.
#pragma clang fp contract(off)

#include <limits.h>

#include "remesh_topo.h"
#include "surface_grid.h"
#include "bake_texel.h"
#include "block_scan.h"

namespace {

constexpr double kBoxSlack = 0x1p-40;   // E = kBoxSlack * S
constexpr double kDetRel = 0x1p-60;
constexpr double kWalkSlack = 4.0;      // W = kWalkSlack * E

struct Ray {
    D3 o, d;
    double tmin, tmax, E;
};

struct Hit {
    double t;
    int f;
    double u, v;
};

// the per-face rule of the header
__device__ inline bool hit_face(const Ray &R, D3 a, D3 b, D3 c, double &t, double &u, double &v) {
    const D3 e1 = b - a, e2 = c - a, pv = cross(R.d, e2);
    const double det = dot(e1, pv);
    if (!(det * det > kDetRel * (dot(e1, e1) * dot(pv, pv)))) return false;
    const double inv = 1.0 / det;
    const D3 tv = R.o - a;
    u = dot(tv, pv) * inv;
    if (!(u >= 0.0 && u <= 1.0)) return false;
    const D3 qv = cross(tv, e1);
    v = dot(R.d, qv) * inv;
    if (!(v >= 0.0 && u + v <= 1.0)) return false;
    t = dot(e2, qv) * inv;
    if (!(t >= R.tmin && t <= R.tmax)) return false;
    const D3 h = R.o + t * R.d;
    const double E = R.E;
    return h.x >= fmin(a.x, fmin(b.x, c.x)) - E && h.x <= fmax(a.x, fmax(b.x, c.x)) + E &&
           h.y >= fmin(a.y, fmin(b.y, c.y)) - E && h.y <= fmax(a.y, fmax(b.y, c.y)) + E &&
           h.z >= fmin(a.z, fmin(b.z, c.z)) - E && h.z <= fmax(a.z, fmax(b.z, c.z)) + E;
}

__device__ inline void consider(Hit &B, const Ray &R, D3 a, D3 b, D3 c, int f) {
    double t, u, v;
    if (!hit_face(R, a, b, c, t, u, v)) return;
    if (t < B.t || (t == B.t && f < B.f)) {
        B.t = t;
        B.f = f;
        B.u = u;
        B.v = v;
    }
}

// (B): the parameters at which axis k is inside [mn - W, mx + W], intersected into [lo_t, hi_t]; false: never inside
__device__ inline bool slab(double o, double d, double inv, double mn, double mx, double W, double &lo_t, double &hi_t) {
    if (d == 0.0) return !(o < mn - W || o > mx + W);
    const double ta = ((mn - W) - o) * inv, tb = ((mx + W) - o) * inv;
    lo_t = fmax(lo_t, fmin(ta, tb));
    hi_t = fmin(hi_t, fmax(ta, tb));
    return true;
}

__device__ inline double pick(double x, double y, double z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

// floor(q) clamped to 0 .. n - 1: grid_clamp's value, clamped before the conversion so that no q leaves the range of int
__device__ inline int cell_of(double q, int n) { return (int)fmin(fmax(floor(q), 0.0), (double)(n - 1)); }

// The walk of (C) / (D) for a finite ray with d != 0 over a surface with faces.  kAny: return at the first face that hits.
template <bool kPacked, bool kAny>
__device__ void cast(const Grid &G, const float4 *__restrict__ rec, D3 o, D3 d, double tmin, double tmax, double amax, Hit &B) {
    const double S = fmax(amax, fmax(fabs(o.x), fmax(fabs(o.y), fabs(o.z))));
    const double E = kBoxSlack * S, W = kWalkSlack * E;
    const Ray R = {o, d, tmin, tmax, E};
    const D3 inv = {d.x == 0.0 ? 0.0 : 1.0 / d.x, d.y == 0.0 ? 0.0 : 1.0 / d.y, d.z == 0.0 ? 0.0 : 1.0 / d.z};
    const double ax = fabs(d.x), ay = fabs(d.y), az = fabs(d.z);
    const int a = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    // axis 0 of the walk is the dominant one; 1 and 2 follow it cyclically
    double po[3], pd[3], pi[3], plo[3];
    int pn[3];
    long ps[3];
    const long stride[3] = {1, G.n[0], (long)G.n[0] * G.n[1]};
    double t0 = tmin, t1 = tmax;
    for (int j = 0; j < 3; ++j) {
        const int k = (a + j) % 3;
        po[j] = pick(o.x, o.y, o.z, k);
        pd[j] = pick(d.x, d.y, d.z, k);
        pi[j] = pick(inv.x, inv.y, inv.z, k);
        plo[j] = pick(G.lo[0], G.lo[1], G.lo[2], k);
        pn[j] = k == 0 ? G.n[0] : (k == 1 ? G.n[1] : G.n[2]);
        ps[j] = k == 0 ? stride[0] : (k == 1 ? stride[1] : stride[2]);
        const double up = pn[j] < 1024 ? plo[j] + pn[j] * G.cell : amax;
        if (!slab(po[j], pd[j], pi[j], plo[j], up, W, t0, t1)) return;  // (B1)
    }
    if (t0 > t1) return;
    const double sg = pd[0] > 0.0 ? 1.0 : -1.0;
    const int step = pd[0] > 0.0 ? 1 : -1;
    const int i0 = cell_of((((po[0] + t0 * pd[0]) - sg * W) - plo[0]) / G.cell, pn[0]);
    const int i1 = cell_of((((po[0] + t1 * pd[0]) + sg * W) - plo[0]) / G.cell, pn[0]);
    for (int i = i0; step > 0 ? i <= i1 : i >= i1; i += step) {
        const double xin = plo[0] + (step > 0 ? i : i + 1) * G.cell, xout = plo[0] + (step > 0 ? i + 1 : i) * G.cell;
        const double ts = i == i0 ? t0 : fmax(t0, ((xin - sg * W) - po[0]) * pi[0]);
        if (ts > B.t) break;  // (D): strictly
        const double te = fmin(i == i1 ? t1 : fmin(t1, ((xout + sg * W) - po[0]) * pi[0]), B.t);
        if (ts > te) continue;
        int lo[3], hi[3];
        for (int j = 1; j < 3; ++j) {
            const double p0 = po[j] + ts * pd[j], p1 = po[j] + te * pd[j];
            lo[j] = cell_of(((fmin(p0, p1) - W) - plo[j]) / G.cell, pn[j]);
            hi[j] = cell_of(((fmax(p0, p1) + W) - plo[j]) / G.cell, pn[j]);
        }
        for (int z = lo[2]; z <= hi[2]; ++z) {
            for (int y = lo[1]; y <= hi[1]; ++y) {
                const long ci = i * ps[0] + y * ps[1] + z * ps[2];
                const int end = G.start[ci + 1];
                for (int it = G.start[ci]; it < end; ++it) {
                    const int f = G.items[it];
                    if (kPacked) {
                        const float4 r0 = rec[4 * (long)f], r1 = rec[4 * (long)f + 1];
                        double lo_t = tmin, hi_t = fmin(tmax, B.t);  // (B2)
                        if (!slab(o.x, d.x, inv.x, (double)r0.x, (double)r0.w, W, lo_t, hi_t)) continue;
                        if (!slab(o.y, d.y, inv.y, (double)r0.y, (double)r1.x, W, lo_t, hi_t)) continue;
                        if (!slab(o.z, d.z, inv.z, (double)r0.z, (double)r1.y, W, lo_t, hi_t)) continue;
                        if (lo_t > hi_t) continue;
                        // face_corners' decoding, spelt out: r1 is in registers already (through the helper every kernel that inlines
                        // this walk came out 8 bytes longer), and r2 and r3 are read only for a face that passes the box test
                        const float4 r2 = rec[4 * (long)f + 2], r3 = rec[4 * (long)f + 3];
                        consider(B, R, {(double)r1.z, (double)r1.w, (double)r2.x}, {(double)r2.y, (double)r2.z, (double)r2.w},
                                 {(double)r3.x, (double)r3.y, (double)r3.z}, f);
                    } else {
                        consider(B, R, ld(G.P, G.F[3 * f]), ld(G.P, G.F[3 * f + 1]), ld(G.P, G.F[3 * f + 2]), f);
                    }
                    if (kAny && B.f != INT_MAX) return;
                }
            }
        }
    }
}

__device__ inline bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

template <bool kPacked>
__global__ void __launch_bounds__(kThreads)
ray_kernel(Grid G, const float *__restrict__ O, const float *__restrict__ Dr, long n, const int64_t *__restrict__ order,
           const float4 *__restrict__ rec, double amax, double tmin, double tmax, double *__restrict__ to, int32_t *__restrict__ fo,
           float *__restrict__ uvo) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long j = kPacked ? (long)order[i] : i;
    const float ox = O[3 * j], oy = O[3 * j + 1], oz = O[3 * j + 2];
    const float dx = Dr[3 * j], dy = Dr[3 * j + 1], dz = Dr[3 * j + 2];
    Hit B = {INFINITY, INT_MAX, 0.0, 0.0};
    const bool finite = finite3(ox, oy, oz) && finite3(dx, dy, dz);
    if (finite && G.nf > 0 && !(dx == 0.0f && dy == 0.0f && dz == 0.0f))
        cast<kPacked, false>(G, rec, {(double)ox, (double)oy, (double)oz}, {(double)dx, (double)dy, (double)dz}, tmin, tmax, amax, B);
    const bool found = B.f != INT_MAX;
    to[j] = finite ? B.t : (double)NAN;
    fo[j] = found ? B.f : -1;
    uvo[2 * j] = found ? (float)B.u : 0.0f;
    uvo[2 * j + 1] = found ? (float)B.v : 0.0f;
}

// The occlusion rule of the header at one FINITE point p with normal n: one copy for the point list and for the atlas bake.
__device__ __forceinline__ float occlusion_at(const Grid &G, const float4 *__restrict__ rec, float px, float py, float pz, float nx,
                                              float ny, float nz, const float *__restrict__ dirs, int K, float offset,
                                              float max_distance, double amax) {
    const float ox = px + offset * nx, oy = py + offset * ny, oz = pz + offset * nz;
    const bool castable = finite3(ox, oy, oz) && G.nf > 0;
    const D3 o = {(double)ox, (double)oy, (double)oz};
    float open = 0.0f, all = 0.0f;
    for (int k = 0; k < K; ++k) {
        const float dx = dirs[3 * k], dy = dirs[3 * k + 1], dz = dirs[3 * k + 2];
        const float w = (nx * dx + ny * dy) + nz * dz;
        if (!(w > 0.0f)) continue;
        all += w;
        Hit B = {INFINITY, INT_MAX, 0.0, 0.0};
        if (castable && finite3(dx, dy, dz))  // w > 0: the direction is not zero
            cast<true, true>(G, rec, o, {(double)dx, (double)dy, (double)dz}, 0.0, (double)max_distance, amax, B);
        if (B.f == INT_MAX) open += w;
    }
    return all == 0.0f ? 1.0f : open / all;
}

__global__ void __launch_bounds__(kThreads)
occlusion_kernel(Grid G, const float *__restrict__ P, const float *__restrict__ Nr, long n, const int64_t *__restrict__ order,
                 const float *__restrict__ dirs, int K, float offset, float max_distance, const float4 *__restrict__ rec, double amax,
                 float *__restrict__ ao) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long j = order ? (long)order[i] : i;
    const float px = P[3 * j], py = P[3 * j + 1], pz = P[3 * j + 2];
    const float nx = Nr[3 * j], ny = Nr[3 * j + 1], nz = Nr[3 * j + 2];
    if (!(finite3(px, py, pz) && finite3(nx, ny, nz))) {
        ao[j] = NAN;
        return;
    }
    ao[j] = occlusion_at(G, rec, px, py, pz, nx, ny, nz, dirs, K, offset, max_distance, amax);
}

// unit(x) of the header ("the mesh render") in place; false (x untouched) when it does not apply
__device__ inline bool unit3(float (&x)[3]) {
    const float s = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    const float len = (float)sqrt((double)s);   // the correctly rounded fp32 root
    if (!(len > 0.0f && len < INFINITY)) return false;
    x[0] = x[0] / len;
    x[1] = x[1] / len;
    x[2] = x[2] / len;
    return true;
}

// The thickness rule of the header: a lane keeps one point's frame, origin and sums in registers over the K rays of its cone.
__global__ void __launch_bounds__(kThreads)
thickness_kernel(Grid G, const float *__restrict__ P, const float *__restrict__ Nr, long n, const int64_t *__restrict__ order,
                 const float *__restrict__ cone, int K, float offset, float max_distance, double outward,
                 const float4 *__restrict__ rec, double amax, float *__restrict__ thickness, float *__restrict__ thinnest,
                 int32_t *__restrict__ valid) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long at = order ? (long)order[i] : i;
    const float px = P[3 * at], py = P[3 * at + 1], pz = P[3 * at + 2];
    float m[3] = {Nr[3 * at], Nr[3 * at + 1], Nr[3 * at + 2]};
    if (!(finite3(px, py, pz) && finite3(m[0], m[1], m[2]))) {
        thickness[at] = thinnest[at] = NAN;
        valid[at] = 0;
        return;
    }
    float sw = 0.0f, swt = 0.0f, thin = INFINITY;
    int count = 0;
    if (unit3(m) && G.nf > 0) {
        const float sg = copysignf(1.0f, m[2]);
        const float a = -1.0f / (sg + m[2]);   // |sg + m.z| >= 1: the two have one sign
        const float b = (m[0] * m[1]) * a;
        const float T[3] = {1.0f + (sg * (m[0] * m[0])) * a, sg * b, -(sg * m[0])};
        const float Bv[3] = {b, sg + (m[1] * m[1]) * a, -m[1]};
        const float ox = px - offset * m[0], oy = py - offset * m[1], oz = pz - offset * m[2];
        const bool castable = finite3(ox, oy, oz);
        const D3 o = {(double)ox, (double)oy, (double)oz};
        for (int j = 0; j < K; ++j) {
            const float cx = cone[3 * j], cy = cone[3 * j + 1], cz = cone[3 * j + 2];
            const float dx = (cx * T[0] + cy * Bv[0]) - cz * m[0];
            const float dy = (cx * T[1] + cy * Bv[1]) - cz * m[1];
            const float dz = (cx * T[2] + cy * Bv[2]) - cz * m[2];
            if (!(castable && finite3(dx, dy, dz)) || (dx == 0.0f && dy == 0.0f && dz == 0.0f)) continue;
            const D3 d = {(double)dx, (double)dy, (double)dz};
            Hit H = {INFINITY, INT_MAX, 0.0, 0.0};
            cast<true, false>(G, rec, o, d, 0.0, (double)max_distance, amax, H);
            if (H.f == INT_MAX) continue;
            D3 ca, cb, cc;
            face_corners(rec, H.f, ca, cb, cc);
            if (!(dot(cross(cb - ca, cc - ca), d) * outward > 0.0)) continue;   // through a front face: into another body
            const float dist = (float)H.t;
            sw += cz;
            swt += cz * dist;
            thin = fminf(thin, dist);
            ++count;
        }
    }
    thickness[at] = count > 0 ? swt / sw : INFINITY;
    thinnest[at] = thin;
    valid[at] = count;
}

// Step 4 of the atlas bake: (p, n) -> (q, m) in place.
__device__ inline void snap_to_surface(const Grid &G, const float4 *__restrict__ rec, float cage, double amax, float (&p)[3], float (&n)[3]) {
    const float cx = cage * n[0], cy = cage * n[1], cz = cage * n[2];
    const float ox = p[0] + cx, oy = p[1] + cy, oz = p[2] + cz;
    const float dx = -cx, dy = -cy, dz = -cz;
    if (!(finite3(ox, oy, oz) && finite3(dx, dy, dz)) || G.nf <= 0 || (dx == 0.0f && dy == 0.0f && dz == 0.0f)) return;
    const D3 o = {(double)ox, (double)oy, (double)oz}, d = {(double)dx, (double)dy, (double)dz};
    Hit B = {INFINITY, INT_MAX, 0.0, 0.0};
    cast<true, false>(G, rec, o, d, 0.0, 2.0, amax, B);
    if (B.f == INT_MAX) return;
    const D3 h = o + B.t * d;
    D3 a, b, c;
    face_corners(rec, B.f, a, b, c);
    D3 g = cross(b - a, c - a);
    if (dot(g, {(double)n[0], (double)n[1], (double)n[2]}) < 0.0) g = {-g.x, -g.y, -g.z};
    const double len = sqrt(dot(g, g));
    p[0] = (float)h.x;
    p[1] = (float)h.y;
    p[2] = (float)h.z;
    if (len > 0.0 && len < (double)INFINITY) {
        n[0] = (float)(g.x / len);
        n[1] = (float)(g.y / len);
        n[2] = (float)(g.z / len);
    }
}

constexpr int kTile = 32;                    // texels per side of a workgroup's tile: 16 or 32 (DESIGN.md 3.3h has both measured)
constexpr int kTileTexels = kTile * kTile;
constexpr int kPasses = kTileTexels / kThreads;   // passes of the read: every wave takes one 8 x 8 sub-block per pass
constexpr int kSubs = kTile / 8;                  // sub-blocks per side
static_assert(kThreads == 256 && (kTile == 16 || kTile == 32), "the sub-block order below is written for 4 waves and 8 x 8 sub-blocks");

// blockIdx.z = which 256 entries of the tile's list this workgroup computes (kPasses workgroups per tile, every one reads the
// tile: 64 KB of rast against milliseconds of rays); a lane computes at most one texel, so no workgroup outlives one texel's rays.
template <bool kSnap>
__global__ void __launch_bounds__(kThreads)
bake_occlusion_kernel(Grid G, const float4 *__restrict__ rast, int res, const float *__restrict__ v_pos, long nv,
                      const void *__restrict__ faces, int faces_i64, long nf, const float *__restrict__ v_nrm,
                      const float *__restrict__ dirs, int K, float offset, float max_distance, float cage,
                      const float4 *__restrict__ rec, double amax, float *__restrict__ ao, uint8_t *__restrict__ mask) {
    __shared__ float s_pn[6][kThreads];          // this workgroup's share of the compacted list: p.xyz, n.xyz
    __shared__ unsigned short s_where[kThreads];  // (y << 5) | x inside the tile
    __shared__ unsigned s_w[kPasses][kThreads / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
    const unsigned first = blockIdx.z * kThreads;  // the share: ranks first .. first + 255
    unsigned base = 0u;
    for (int pass = 0; pass < kPasses; ++pass) {
        const int sub = pass * 4 + wave;  // the 8 x 8 sub-block, row-major in the tile
        const int tx = (sub % kSubs) * 8 + (lane & 7), ty = (sub / kSubs) * 8 + (lane >> 3);
        const int x = x0 + tx, y = y0 + ty;
        const bool live = x < res && y < res;
        bool listed = false;
        float p[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f};
        if (live) {
            const long at = (long)y * res + x;
            const float4 r = rast[at];
            const Texel t = texel_position(r, v_pos, nv, faces, faces_i64, nf);
            if (t.covered) {
                for (int k = 0; k < 3; ++k) {
                    p[k] = t.x[k];
                    n[k] = (v_nrm[3 * t.i[0] + k] * r.x + v_nrm[3 * t.i[1] + k] * r.y) + v_nrm[3 * t.i[2] + k] * r.z;
                }
                listed = finite3(p[0], p[1], p[2]) && finite3(n[0], n[1], n[2]);
            }
            if (blockIdx.z == 0) {  // the texels no list holds are written once, by the tile's first workgroup
                if (!listed) ao[at] = t.covered ? NAN : 0.0f;
                mask[at] = t.covered ? 1 : 0;
            }
        }
        const unsigned rank = base + block_flag_rank<kThreads / 64>(listed, s_w[pass]) - first;  // one barrier; a row of s_w per pass
        if (listed && rank < (unsigned)kThreads) {  // (a rank below `first` wraps to a large number)
            for (int k = 0; k < 3; ++k) {
                s_pn[k][rank] = p[k];
                s_pn[3 + k][rank] = n[k];
            }
            s_where[rank] = (unsigned short)((ty << 5) | tx);
        }
        for (int w = 0; w < kThreads / 64; ++w) base += s_w[pass][w];
    }
    __syncthreads();
    if (base <= first || (unsigned)tid >= base - first) return;  // base: the tile's count, the same in every thread
    float p[3] = {s_pn[0][tid], s_pn[1][tid], s_pn[2][tid]}, n[3] = {s_pn[3][tid], s_pn[4][tid], s_pn[5][tid]};
    const int where = s_where[tid];
    if (kSnap) snap_to_surface(G, rec, cage, amax, p, n);
    const long at = (long)(y0 + (where >> 5)) * res + (x0 + (where & 31));
    // a snapped point is finite (a hit has a finite t inside [0, 2]) unless the sum overflowed: the rule's NaN then
    ao[at] = finite3(p[0], p[1], p[2]) && finite3(n[0], n[1], n[2])
                 ? occlusion_at(G, rec, p[0], p[1], p[2], n[0], n[1], n[2], dirs, K, offset, max_distance, amax)
                 : NAN;
}

// ---- the mesh render ---------------------------------------------------------------------------------------------------------
struct Material {
    const float *uvs;             // [3 nf][2] per corner, or null
    const float *texture;         // [tex_res][tex_res][3]
    const float *normal_map;      // [nmap_res][nmap_res][3]
    const float *corner_n;        // [3 nf][3]: a tangent-space normal map's frame (null: the map is in object space)
    const float *corner_t;        // [3 nf][4]
    const float *occlusion_map;   // [occ_res][occ_res]
    const float *v_col;           // [nv][col_stride]
    const float *v_nrm;           // [nv][3]
    const float *v_occ;           // [nv]
    int tex_res, nmap_res, occ_res, col_stride;
};

struct RenderOut {
    float *color, *shaded, *opacity, *rgba, *depth, *normal, *occlusion;
    int32_t *face;
};

// the lookup of the header: kC channels of a map of side R at (U, V)
template <int kC>
__device__ inline void map_lookup(const float *__restrict__ map, int R, float U, float V, float (&out)[kC]) {
    const float Rf = (float)R;
    float X = U * Rf, Y = (1.0f - V) * Rf;
    if (!(isfinite(X) && isfinite(Y))) X = Y = 0.0f;
    const float xf = floorf(X), yf = floorf(Y), top = (float)(R - 1);
    const float fx = X - xf, fy = Y - yf, gx = 1.0f - fx, gy = 1.0f - fy;
    const long x0 = (long)fminf(fmaxf(xf, 0.0f), top), x1 = (long)fminf(fmaxf(xf + 1.0f, 0.0f), top);
    const long y0 = (long)fminf(fmaxf(yf, 0.0f), top), y1 = (long)fminf(fmaxf(yf + 1.0f, 0.0f), top);
    const float *r0 = map + (y0 * R) * kC, *r1 = map + (y1 * R) * kC;
#pragma unroll
    for (int c = 0; c < kC; ++c)
        out[c] = ((r0[x0 * kC + c] * gx + r0[x1 * kC + c] * fx) * gy) + ((r1[x0 * kC + c] * gx + r1[x1 * kC + c] * fx) * fy);
}

// the second phase: everything after the hit (B.f a face) is final
__device__ void shade_hit(const Grid &G, const float4 *__restrict__ rec, const Material &M, const RenderOut &O, const Hit &B,
                          float dx, float dy, float dz, float ambient, int has_light, float lx, float ly, float lz, double outward,
                          long at) {
    const long f = B.f;
    const float w1 = (float)B.u, w2 = (float)B.v, w0 = (1.0f - w1) - w2;
    const long i0 = G.F[3 * f], i1 = G.F[3 * f + 1], i2 = G.F[3 * f + 2];
    float U = 0.0f, V = 0.0f;
    if (M.uvs) {
        const float *q = M.uvs + 6 * f;
        U = (q[0] * w0 + q[2] * w1) + q[4] * w2;
        V = (q[1] * w0 + q[3] * w1) + q[5] * w2;
    }
    const bool want_albedo = O.color || O.shaded || O.rgba;
    float albedo[3] = {0.8f, 0.8f, 0.8f};
    if (want_albedo) {
        if (M.texture) {
            map_lookup<3>(M.texture, M.tex_res, U, V, albedo);
        } else if (M.v_col) {
            const long s = M.col_stride;
            for (int c = 0; c < 3; ++c) albedo[c] = (M.v_col[s * i0 + c] * w0 + M.v_col[s * i1 + c] * w1) + M.v_col[s * i2 + c] * w2;
        }
    }
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (O.normal || O.shaded) {
        bool done = false;
        if (M.normal_map) {
            float m[3];
            map_lookup<3>(M.normal_map, M.nmap_res, U, V, m);
            for (int c = 0; c < 3; ++c) m[c] = 2.0f * m[c] - 1.0f;
            if (M.corner_n) {
                const float *cn = M.corner_n + 9 * f, *ct = M.corner_t + 12 * f;
                float N[3], T[3];
                for (int c = 0; c < 3; ++c) {
                    N[c] = (cn[c] * w0 + cn[3 + c] * w1) + cn[6 + c] * w2;
                    T[c] = (ct[c] * w0 + ct[4 + c] * w1) + ct[8 + c] * w2;
                }
                const float s = ct[3];
                const float Bv[3] = {s * (N[1] * T[2] - N[2] * T[1]), s * (N[2] * T[0] - N[0] * T[2]), s * (N[0] * T[1] - N[1] * T[0])};
                for (int c = 0; c < 3; ++c) n[c] = (m[0] * T[c] + m[1] * Bv[c]) + m[2] * N[c];
            } else {
                for (int c = 0; c < 3; ++c) n[c] = m[c];
            }
            done = unit3(n);
        }
        if (!done && M.v_nrm) {
            for (int c = 0; c < 3; ++c) n[c] = (M.v_nrm[3 * i0 + c] * w0 + M.v_nrm[3 * i1 + c] * w1) + M.v_nrm[3 * i2 + c] * w2;
            done = unit3(n);
        }
        if (!done) {
            D3 a, b, c;
            face_corners(rec, f, a, b, c);
            D3 g = cross(b - a, c - a);
            g = {g.x * outward, g.y * outward, g.z * outward};
            const double len = sqrt(dot(g, g));
            const bool ok = len > 0.0 && len < (double)INFINITY;
            n[0] = ok ? (float)(g.x / len) : 0.0f;
            n[1] = ok ? (float)(g.y / len) : 0.0f;
            n[2] = ok ? (float)(g.z / len) : 0.0f;
        }
    }
    float ao = 1.0f;
    if (O.occlusion || O.shaded) {
        if (M.occlusion_map) {
            float v[1];
            map_lookup<1>(M.occlusion_map, M.occ_res, U, V, v);
            ao = v[0];
        } else if (M.v_occ) {
            ao = (M.v_occ[i0] * w0 + M.v_occ[i1] * w1) + M.v_occ[i2] * w2;
        }
    }
    if (O.color) {
        O.color[3 * at] = albedo[0];
        O.color[3 * at + 1] = albedo[1];
        O.color[3 * at + 2] = albedo[2];
    }
    if (O.shaded) {
        float l[3] = {lx, ly, lz};
        if (!has_light) {
            l[0] = -dx;
            l[1] = -dy;
            l[2] = -dz;
            if (!unit3(l)) l[0] = l[1] = l[2] = 0.0f;
        }
        const float ndl = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2];
        const float k = ambient * ao + (1.0f - ambient) * (ndl > 0.0f ? ndl : 0.0f);
        O.shaded[3 * at] = albedo[0] * k;
        O.shaded[3 * at + 1] = albedo[1] * k;
        O.shaded[3 * at + 2] = albedo[2] * k;
    }
    if (O.opacity) O.opacity[at] = 1.0f;
    if (O.rgba) {
        O.rgba[4 * at] = albedo[0];
        O.rgba[4 * at + 1] = albedo[1];
        O.rgba[4 * at + 2] = albedo[2];
        O.rgba[4 * at + 3] = 1.0f;
    }
    if (O.depth) O.depth[at] = (float)B.t;
    if (O.normal) {
        O.normal[3 * at] = n[0];
        O.normal[3 * at + 1] = n[1];
        O.normal[3 * at + 2] = n[2];
    }
    if (O.occlusion) O.occlusion[at] = ao;
    if (O.face) O.face[at] = (int32_t)f;
}

__device__ inline void store_background(const RenderOut &O, long at, bool finite) {
    if (O.color) O.color[3 * at] = O.color[3 * at + 1] = O.color[3 * at + 2] = 1.0f;
    if (O.shaded) O.shaded[3 * at] = O.shaded[3 * at + 1] = O.shaded[3 * at + 2] = 1.0f;
    if (O.opacity) O.opacity[at] = 0.0f;
    if (O.rgba) O.rgba[4 * at] = O.rgba[4 * at + 1] = O.rgba[4 * at + 2] = O.rgba[4 * at + 3] = 0.0f;
    if (O.depth) O.depth[at] = finite ? 0.0f : NAN;
    if (O.normal) O.normal[3 * at] = O.normal[3 * at + 1] = O.normal[3 * at + 2] = 0.0f;
    if (O.occlusion) O.occlusion[at] = 1.0f;
    if (O.face) O.face[at] = -1;
}

// kRow: H == 1, a wave takes 64 consecutive rays; else a wave takes an 8 x 8 tile and the workgroup 16 x 16 pixels
template <bool kRow>
__global__ void __launch_bounds__(kThreads)
render_kernel(Grid G, const float *__restrict__ Ro, const float *__restrict__ Rd, int H, long W, const float4 *__restrict__ rec,
              double amax, Material M, RenderOut O, float ambient, int has_light, float lx, float ly, float lz, double outward) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    long x;
    int y;
    if (kRow) {
        x = (long)blockIdx.x * kThreads + tid;
        y = 0;
    } else {
        x = (long)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
        y = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    }
    if (x >= W || y >= H) return;
    const long at = ((long)blockIdx.z * H + y) * W + x;
    const float ox = Ro[3 * at], oy = Ro[3 * at + 1], oz = Ro[3 * at + 2];
    const float dx = Rd[3 * at], dy = Rd[3 * at + 1], dz = Rd[3 * at + 2];
    Hit B = {INFINITY, INT_MAX, 0.0, 0.0};
    const bool finite = finite3(ox, oy, oz) && finite3(dx, dy, dz);
    if (finite && G.nf > 0 && !(dx == 0.0f && dy == 0.0f && dz == 0.0f))
        cast<true, false>(G, rec, {(double)ox, (double)oy, (double)oz}, {(double)dx, (double)dy, (double)dz}, 0.0, (double)INFINITY, amax, B);
    if (B.f == INT_MAX) {
        store_background(O, at, finite);
        return;
    }
    shade_hit(G, rec, M, O, B, dx, dy, dz, ambient, has_light, lx, ly, lz, outward, at);
}

}  // namespace

extern "C" {

int sculpt_surface_ray_cast(const float *O, const float *D, int64_t n, const int64_t *order, const float *GP, const int32_t *GF,
                            int64_t gnf, const float *records, const int32_t *items, const int32_t *start, const double *params_host,
                            double amax, double tmin, double tmax, double *t, int32_t *face, float *uv, sculpt_stream_t stream) {
    if (int rc = check_surface_query("surface_ray_cast", n, amax, gnf, items, start, records, false)) return rc;
    SC_REQUIRE(tmin >= 0 && tmin <= tmax, "surface_ray_cast: the range must satisfy 0 <= tmin <= tmax, got [%g, %g]", tmin, tmax);
    SC_REQUIRE((order == nullptr) == (records == nullptr), "surface_ray_cast: the sorted form takes both the order and the records");
    if (n == 0) return 0;
    if (int rc = check_grid("surface_ray_cast", GP, GF, gnf, params_host)) return rc;
    SC_REQUIRE(O && D && t && face && uv, "surface_ray_cast: null array");
    const Grid G = grid_of(GP, GF, (long)gnf, items, start, params_host);
    if (order)
        RMD_LAUNCH(ray_kernel<true>, n, G, O, D, (long)n, order, reinterpret_cast<const float4 *>(records), amax, tmin, tmax, t, face, uv);
    else
        RMD_LAUNCH(ray_kernel<false>, n, G, O, D, (long)n, nullptr, nullptr, amax, tmin, tmax, t, face, uv);
    return 0;
}

int sculpt_surface_occlusion(const float *P, const float *N, int64_t n, const int64_t *order, const float *dirs, int k, float offset,
                             float max_distance, const float *GP, const int32_t *GF, int64_t gnf, const float *records,
                             const int32_t *items, const int32_t *start, const double *params_host, double amax, float *ao,
                             sculpt_stream_t stream) {
    if (int rc = check_surface_query("surface_occlusion", n, amax, gnf, items, start, records, true)) return rc;
    if (int rc = check_ray_set("surface_occlusion", k, max_distance, offset)) return rc;
    if (n == 0) return 0;
    if (int rc = check_grid("surface_occlusion", GP, GF, gnf, params_host)) return rc;
    SC_REQUIRE(P && N && dirs && ao, "surface_occlusion: null array");
    const Grid G = grid_of(GP, GF, (long)gnf, items, start, params_host);
    RMD_LAUNCH(occlusion_kernel, n, G, P, N, (long)n, order, dirs, k, offset, max_distance, reinterpret_cast<const float4 *>(records), amax, ao);
    return 0;
}

int sculpt_surface_thickness(const float *P, const float *N, int64_t n, const int64_t *order, const float *cone_dirs, int k, float offset,
                             float max_distance, double outward, const float *GP, const int32_t *GF, int64_t gnf, const float *records,
                             const int32_t *items, const int32_t *start, const double *params_host, double amax, float *thickness,
                             float *thinnest, int32_t *valid, sculpt_stream_t stream) {
    if (int rc = check_surface_query("surface_thickness", n, amax, gnf, items, start, records, true)) return rc;
    if (int rc = check_ray_set("surface_thickness", k, max_distance, offset)) return rc;
    SC_REQUIRE(outward == 1.0 || outward == -1.0, "surface_thickness: outward=%g (+1 or -1)", outward);
    if (n == 0) return 0;
    if (int rc = check_grid("surface_thickness", GP, GF, gnf, params_host)) return rc;
    SC_REQUIRE(P && N && cone_dirs && thickness && thinnest && valid, "surface_thickness: null array");
    const Grid G = grid_of(GP, GF, (long)gnf, items, start, params_host);
    RMD_LAUNCH(thickness_kernel, n, G, P, N, (long)n, order, cone_dirs, k, offset, max_distance, outward,
               reinterpret_cast<const float4 *>(records), amax, thickness, thinnest, valid);
    return 0;
}

int sculpt_bake_occlusion(const float *rast, int res, const float *v_pos, size_t nv, const void *faces, int faces_i64, size_t nf,
                          const float *v_nrm, const float *dirs, int k, float offset, float max_distance, float cage, const float *GP,
                          const int32_t *GF, int64_t gnf, const float *records, const int32_t *items, const int32_t *start,
                          const double *params_host, double amax, float *ao, uint8_t *mask, sculpt_stream_t stream) {
    SC_REQUIRE(res >= 0 && res <= 32768, "bake_occlusion: resolution %d (0 .. 32768)", res);
    SC_REQUIRE(nv <= (size_t)1 << 40 && nf <= (size_t)1 << 40, "bake_occlusion: mesh too large");
    if (int rc = check_surface_query("bake_occlusion", res, amax, gnf, items, start, records, true)) return rc;   // n: the side, in range
    if (int rc = check_ray_set("bake_occlusion", k, max_distance, offset)) return rc;
    SC_REQUIRE(cage >= 0 && isfinite(cage), "bake_occlusion: cage=%g (0: no snap, or positive and finite)", (double)cage);
    if (res == 0) return 0;
    if (int rc = check_grid("bake_occlusion", GP, GF, gnf, params_host)) return rc;
    SC_REQUIRE(rast && dirs && ao && mask, "bake_occlusion: null array");
    SC_REQUIRE(aligned16(rast), "bake_occlusion: rast not 16-byte aligned");
    SC_REQUIRE(nf == 0 || (v_pos && faces && v_nrm && nv > 0), "bake_occlusion: null mesh");
    const Grid G = grid_of(GP, GF, (long)gnf, items, start, params_host);
    const unsigned tiles = (unsigned)((res + kTile - 1) / kTile);
    hipLaunchKernelGGL(cage > 0.0f ? bake_occlusion_kernel<true> : bake_occlusion_kernel<false>, dim3(tiles, tiles, kPasses),
                       dim3(kThreads), 0, as_stream(stream), G,
                       reinterpret_cast<const float4 *>(rast), res, v_pos, (long)nv, faces, faces_i64, (long)nf, v_nrm, dirs, k, offset,
                       max_distance, cage, reinterpret_cast<const float4 *>(records), amax, ao, mask);
    SC_LAUNCH_CHECK();
    return 0;
}

int sculpt_surface_render(const float *rays_o, const float *rays_d, int64_t n_images, int64_t height, int64_t width, const float *GP,
                          const int32_t *GF, int64_t gnf, const float *records, const int32_t *items, const int32_t *start,
                          const double *params_host, double amax, const sculpt_render_material *material, float ambient,
                          const float *light, double outward, const sculpt_render_outputs *out, sculpt_stream_t stream) {
    SC_REQUIRE(n_images >= 0 && height >= 0 && width >= 0, "surface_render: negative image size");
    SC_REQUIRE(n_images <= 65535 && height <= ((int64_t)1 << 19) && width < ((int64_t)1 << 31),
               "surface_render: %lld images of %lld x %lld are too many or too large", (long long)n_images, (long long)height, (long long)width);
    SC_REQUIRE((double)n_images * (double)height * (double)width * 4.0 < 0x1p40, "surface_render: too many rays");
    if (int rc = check_surface_query("surface_render", n_images * height * width, amax, gnf, items, start, records, true)) return rc;   // n in range
    SC_REQUIRE(isfinite(ambient) && isfinite(outward), "surface_render: ambient=%g, outward=%g", (double)ambient, outward);
    SC_REQUIRE(material && out, "surface_render: null material or outputs");
    if (n_images == 0 || height == 0 || width == 0) return 0;
    if (int rc = check_grid("surface_render", GP, GF, gnf, params_host)) return rc;
    SC_REQUIRE(rays_o && rays_d, "surface_render: null rays");
    SC_REQUIRE(out->color || out->shaded || out->opacity || out->rgba || out->depth || out->normal || out->occlusion || out->face,
               "surface_render: no pass asked for");
    const sculpt_render_material &m = *material;
    SC_REQUIRE(!m.texture || (m.uvs && m.texture_res >= 1), "surface_render: a texture needs uvs and a side >= 1");
    SC_REQUIRE(!m.normal_map || (m.uvs && m.normal_map_res >= 1), "surface_render: a normal map needs uvs and a side >= 1");
    SC_REQUIRE(!m.occlusion_map || (m.uvs && m.occlusion_map_res >= 1), "surface_render: an occlusion map needs uvs and a side >= 1");
    SC_REQUIRE(m.texture_res <= 32768 && m.normal_map_res <= 32768 && m.occlusion_map_res <= 32768, "surface_render: map side above 32768");
    SC_REQUIRE((m.corner_normals == nullptr) == (m.corner_tangents == nullptr),
               "surface_render: corner_normals and corner_tangents come together (both or neither)");
    SC_REQUIRE(!m.corner_normals || m.normal_map, "surface_render: a tangent frame without a normal map");
    SC_REQUIRE(!m.vertex_colors || m.vertex_color_channels == 3 || m.vertex_color_channels == 4, "surface_render: vertex colours of %d channels",
               m.vertex_color_channels);
    const Grid G = grid_of(GP, GF, (long)gnf, items, start, params_host);
    const Material M = {m.uvs, m.texture, m.normal_map, m.corner_normals, m.corner_tangents, m.occlusion_map, m.vertex_colors,
                        m.vertex_normals, m.vertex_occlusion, m.texture_res, m.normal_map_res, m.occlusion_map_res, m.vertex_color_channels};
    const RenderOut O = {out->color, out->shaded, out->opacity, out->rgba, out->depth, out->normal, out->occlusion, out->face};
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const float *l = light ? light : zero;
    const float4 *rec = reinterpret_cast<const float4 *>(records);
    if (height == 1) {
        hipLaunchKernelGGL(render_kernel<true>, dim3((unsigned)((width + kThreads - 1) / kThreads), 1, (unsigned)n_images), dim3(kThreads), 0,
                           as_stream(stream), G, rays_o, rays_d, 1, (long)width, rec, amax, M, O, ambient, light ? 1 : 0, l[0], l[1], l[2],
                           outward);
    } else {
        hipLaunchKernelGGL(render_kernel<false>, dim3((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16), (unsigned)n_images),
                           dim3(kThreads), 0, as_stream(stream), G, rays_o, rays_d, (int)height, (long)width, rec, amax, M, O, ambient,
                           light ? 1 : 0, l[0], l[1], l[2], outward);
    }
    SC_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
