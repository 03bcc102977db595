// The projection rule of DESIGN.md section 3.1e: one copy, so that project_kernel (csrc/mesh_project.hip) and
// bake_scene_surface_kernel (csrc/bake_surface.hip) move a point by the same sequence of IEEE fp32 operations.  The rule is
// compiled without contraction; tests/_projref.py restates it (newton in NumPy, composed_device one torch call per operation).
#pragma once

#include "common.h"

namespace sculpt {

// what a point carries from one evaluation to the next
struct ProjState {
    float px, py, pz;     // current iterate
    float r;              // its residual d - target
    float gx, gy, gz;     // its masked gradient
    float bx, by, bz, br; // best iterate and its residual
    int status, evals;
    bool active;
};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < INFINITY; }

// the state of a point before its first evaluation, which is at p0; `active` false: the point never takes a step
__device__ __forceinline__ ProjState proj_start(float p0x, float p0y, float p0z, bool active) {
    ProjState s;
    s.px = s.bx = p0x, s.py = s.by = p0y, s.pz = s.bz = p0z;
    s.r = s.br = 0.f;
    s.gx = s.gy = s.gz = 0.f;
    s.status = 1, s.evals = 0, s.active = active;
    return s;
}

// One turn of the rule after the evaluation (d, g) at the candidate (qx, qy, qz): accept it (k == 0: it is p0), then the
// checks and the step that lead to the next candidate, which is left in (qx, qy, qz).  DESIGN.md section 3.1e numbers the
// operations.  -> whether the candidate that was just evaluated is now the best iterate (bx, by, bz): a caller that wants
// something else of the best iterate than its residual -- the raw gradient, for the normal there -- keeps it on true.
__device__ __forceinline__ bool rule_update(ProjState &s, int k, int K, float d, float gx, float gy, float gz, float &qx, float &qy,
                                            float &qz, float p0x, float p0y, float p0z, bool fx, bool fy, bool fz, float target,
                                            float radius, float md2, float res_tol) {
#pragma clang fp contract(off)
    bool took = false;
    if (s.active) {
        s.evals += 1;
        const float rq = d - target;
        if (!finite_f(rq)) {
            s.status = 3;
            s.active = false;
            if (k == 0) s.br = rq, took = true;   // the best iterate is p0, which is the candidate
        } else {
            s.px = qx, s.py = qy, s.pz = qz;
            s.r = rq;
            s.gx = fx ? 0.f : gx, s.gy = fy ? 0.f : gy, s.gz = fz ? 0.f : gz;
            if (k == 0 || fabsf(rq) < fabsf(s.br)) s.bx = qx, s.by = qy, s.bz = qz, s.br = rq, took = true;
        }
    }
    if (!s.active) return took;
    if (k == K) {
        s.status = fabsf(s.r) <= res_tol ? 0 : 1;
        s.active = false;
        return took;
    }
    if (fabsf(s.r) <= res_tol) {
        s.status = 0;
        s.active = false;
        return took;
    }
    const float g2 = (s.gx * s.gx + s.gy * s.gy) + s.gz * s.gz;
    if (!(g2 > 0.f) || !finite_f(g2)) {
        s.status = 3;
        s.active = false;
        return took;
    }
    const float st = s.r / g2;
    float nx = s.px - st * s.gx, ny = s.py - st * s.gy, nz = s.pz - st * s.gz;
    const float lo = -radius;
    nx = nx < lo ? lo : nx, ny = ny < lo ? lo : ny, nz = nz < lo ? lo : nz;   // comparisons, not fmin / fmax: a NaN stays a NaN
    nx = nx > radius ? radius : nx, ny = ny > radius ? radius : ny, nz = nz > radius ? radius : nz;
    nx = fx ? p0x : nx, ny = fy ? p0y : ny, nz = fz ? p0z : nz;
    const float dx = nx - p0x, dy = ny - p0y, dz = nz - p0z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 > md2) {
        s.status = 2;
        s.active = false;
        return took;
    }
    qx = nx, qy = ny, qz = nz;
    return took;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The line rule of DESIGN.md section 3.1h: a safeguarded Newton search for d(p0 + s n) = target along the fixed unit direction n
// (sculpt_triplane_project_along, csrc/mesh_project.hip).  tests/_dispref.py restates it (line_search in NumPy, composed_device
// one torch call per operation).
// ---------------------------------------------------------------------------------------------------------------------------
struct LineState {
    float s;              // current parameter along the line
    float bs, br;         // best parameter (the height) and its residual
    float a, b;           // the last parameters with r < 0 and with r > 0: a sign change once both are set
    bool has_a, has_b;
    int status, evals;
    bool active;
};

// N -> the unit direction n = N / sqrt(N.N); false (and n = 0) when N.N is not finite or not > 0
__device__ __forceinline__ bool line_direction(float Nx, float Ny, float Nz, float &nx, float &ny, float &nz) {
#pragma clang fp contract(off)
    const float nn = (Nx * Nx + Ny * Ny) + Nz * Nz;
    if (!(nn > 0.f) || !finite_f(nn)) {
        nx = ny = nz = 0.f;
        return false;
    }
    const float len = sqrtf(nn);
    nx = Nx / len, ny = Ny / len, nz = Nz / len;
    return true;
}

// the point of the line at parameter s: one product and one sum per axis
__device__ __forceinline__ void line_point(float p0x, float p0y, float p0z, float nx, float ny, float nz, float s, float &qx, float &qy,
                                           float &qz) {
#pragma clang fp contract(off)
    qx = p0x + s * nx, qy = p0y + s * ny, qz = p0z + s * nz;
}

// One turn of the line rule after the evaluation (d, g) at line_point(st.s): steps 1 .. 10 of section 3.1h.  A point that has
// stopped is left as it is.
__device__ __forceinline__ void line_update(LineState &st, int k, int K, float d, float gx, float gy, float gz, float p0x, float p0y,
                                            float p0z, float nx, float ny, float nz, float target, float radius, float max_dist,
                                            float res_tol) {
#pragma clang fp contract(off)
    if (!st.active) return;
    st.evals += 1;
    const float r = d - target;
    if (!finite_f(r)) {
        st.status = 3;
        st.active = false;
        if (k == 0) st.bs = 0.f, st.br = r;
        return;
    }
    if (k == 0 || fabsf(r) < fabsf(st.br)) st.bs = st.s, st.br = r;
    if (fabsf(r) <= res_tol) {
        st.status = 0;
        st.active = false;
        return;
    }
    if (k == K) {
        st.status = 1;
        st.active = false;
        return;
    }
    if (r < 0.f) st.a = st.s, st.has_a = true;
    if (r > 0.f) st.b = st.s, st.has_b = true;
    const float gn = (gx * nx + gy * ny) + gz * nz;
    float c = st.s - r / gn;
    const float lo = -max_dist;
    c = c < lo ? lo : c;   // comparisons, not fmin / fmax: a NaN stays a NaN
    c = c > max_dist ? max_dist : c;
    if (st.has_a && st.has_b) {
        const float blo = st.a < st.b ? st.a : st.b, bhi = st.a < st.b ? st.b : st.a;
        if (!(c > blo && c < bhi)) c = 0.5f * (st.a + st.b);
    }
    if (!finite_f(c)) {
        st.status = 3;
        st.active = false;
        return;
    }
    if (c == st.s) {   // pinned at the end of the trust interval
        st.status = 2;
        st.active = false;
        return;
    }
    float cx, cy, cz;
    line_point(p0x, p0y, p0z, nx, ny, nz, c, cx, cy, cz);
    if (fabsf(cx) > radius || fabsf(cy) > radius || fabsf(cz) > radius) {   // the box is part of the trust region
        st.status = 2;
        st.active = false;
        return;
    }
    st.s = c;
}

}  // namespace sculpt
