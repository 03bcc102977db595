"""Restatements for the displacement bake: the line rule of DESIGN.md 3.1h (csrc/project_rule.h line_update).

    line_search       the rule in NumPy on _projref.value_grad, in any dtype (the fp64 run of it is the tests' reference);
                      safeguard=False leaves step 7 (the bisection of the sign change) out
    composed_device   the same rule on the device with ops.field_normals per evaluation and one torch fp32 call per operation:
                      what sculpt_triplane_project_along has to equal bit for bit
    face_points       the tests' points on set A: one per face, np.random.default_rng(0).dirichlet(ones(3), Nf), with the
                      interpolated area-weighted vertex normal as direction

Plain NumPy; torch is touched by composed_device alone (through the tensors it is handed)."""
import functools

import numpy as np

import _projref

RADIUS = _projref.RADIUS


def line_search(planes, Ws, bs, points, directions, target, steps, max_dist, res_tol, dtype, radius=RADIUS, align_corners=False,
                safeguard=True, plain=False):
    """-> dict(height [N], residual [N], status i32 [N], evals i32 [N], r0 [N] the residual at the start, near [N] the smallest
    distance of an evaluated |r| from res_tol: how close the point came to the other side of the convergence test)."""
    dt = np.dtype(dtype).type
    p0 = np.asarray(points).astype(dtype).reshape(-1, 3)
    Nd = np.asarray(directions).astype(dtype).reshape(-1, 3)
    N = p0.shape[0]
    t, tol, rad, md = dt(np.float32(target)), dt(np.float32(res_tol)), dt(np.float32(radius)), dt(np.float32(max_dist))
    K = int(steps)
    with np.errstate(all="ignore"):
        nn = (Nd[:, 0] * Nd[:, 0] + Nd[:, 1] * Nd[:, 1]) + Nd[:, 2] * Nd[:, 2]
        ok = (nn > 0) & np.isfinite(nn)
        n = np.where(ok[:, None], Nd / np.sqrt(nn)[:, None], dt(0))
        s = np.zeros(N, dtype)
        bs_, br = np.zeros(N, dtype), np.zeros(N, dtype)
        a, b = np.zeros(N, dtype), np.zeros(N, dtype)
        has_a, has_b = np.zeros(N, bool), np.zeros(N, bool)
        status = np.where(ok, 1, 3).astype(np.int32)
        evals = np.zeros(N, np.int32)
        active = ok.copy()
        r0 = np.zeros(N, dtype)
        near = np.full(N, np.inf)
        for k in range(K + 1):
            if not active.any():
                break
            q = p0 + s[:, None] * n
            d, g = _projref.value_grad(planes, Ws, bs, q, dtype, radius, align_corners)
            r = d - t
            if k == 0:
                r0 = r.copy()
            evals = evals + active.astype(np.int32)
            near = np.where(active, np.minimum(near, np.abs(np.abs(r) - tol)), near)
            bad = active & ~np.isfinite(r)
            status[bad] = 3
            if k == 0:
                bs_ = np.where(bad, dt(0), bs_)
                br = np.where(bad, r, br)
            active = active & ~bad
            better = active & (np.abs(r) < np.abs(br)) if k else active
            bs_ = np.where(better, s, bs_)
            br = np.where(better, r, br)
            conv = active & (np.abs(r) <= tol)
            status[conv] = 0
            active = active & ~conv
            if k == K:
                status[active] = 1
                active = active & False
                break
            neg, pos = active & (r < 0), active & (r > 0)
            a, has_a = np.where(neg, s, a), has_a | neg
            b, has_b = np.where(pos, s, b), has_b | pos
            gn = (g[:, 0] * n[:, 0] + g[:, 1] * n[:, 1]) + g[:, 2] * n[:, 2]
            c = s - r / gn
            if plain:   # the unguarded step: it stops where the rule clamps
                left = active & ((c < -md) | (c > md))
                status[left] = 2
                active = active & ~left
            c = np.where(c < -md, -md, c)
            c = np.where(c > md, md, c)
            if safeguard and not plain:
                both = has_a & has_b
                lo, hi = np.where(a < b, a, b), np.where(a < b, b, a)
                c = np.where(both & ~((c > lo) & (c < hi)), dt(0.5) * (a + b), c)
            nonfin = active & ~np.isfinite(c)
            status[nonfin] = 3
            active = active & ~nonfin
            pinned = active & (c == s)
            status[pinned] = 2
            active = active & ~pinned
            out = active & (np.abs(p0 + c[:, None] * n) > rad).any(1)
            status[out] = 2
            active = active & ~out
            s = np.where(active, c, s)
    return {"height": bs_, "residual": br, "status": status, "evals": evals, "r0": r0, "near": near}


def composed_device(ops, planes, mlp, points, directions, target, steps, max_dist, res_tol, radius=RADIUS, align_corners=False):
    """The line rule on the device without the fused kernel: ops.field_normals(want=("grad", "density")) per evaluation and one
    torch fp32 call per operation of the rule, in the rule's order, with masks for the points that have stopped; every step
    runs over all points (no compaction, no early exit, no host wait).
    -> (height [N], residual [N], status i32 [N], evals i32 [N]) as device tensors."""
    import torch

    t = float(np.float32(target))
    tol = float(np.float32(res_tol))
    rad = float(np.float32(radius))
    md = float(np.float32(max_dist))
    p0 = points.reshape(-1, 3).to(torch.float32).contiguous()
    Nd = directions.reshape(-1, 3).to(torch.float32).contiguous()
    K = int(steps)
    xx = Nd[:, 0] * Nd[:, 0]
    yy = Nd[:, 1] * Nd[:, 1]
    zz = Nd[:, 2] * Nd[:, 2]
    nn = xx + yy
    nn = nn + zz
    ok = (nn > 0) & torch.isfinite(nn)
    ln = torch.sqrt(nn)
    n = torch.where(ok[:, None], Nd / ln[:, None], torch.zeros_like(Nd))
    s = torch.zeros_like(nn)
    best_s, best_r = torch.zeros_like(nn), torch.zeros_like(nn)
    a, b = torch.zeros_like(nn), torch.zeros_like(nn)
    has_a, has_b = torch.zeros_like(ok), torch.zeros_like(ok)
    status = torch.where(ok, 1, 3).to(torch.int32)
    evals = torch.zeros_like(status)
    active = ok.clone()
    lo_md, hi_md = torch.full_like(nn, -md), torch.full_like(nn, md)
    zero = torch.zeros_like(nn)

    def put(st, mask, value):
        return torch.where(mask, torch.full_like(st, value), st)

    for k in range(K + 1):
        sn = s[:, None] * n
        q = p0 + sn
        o = ops.field_normals(planes, mlp, q.contiguous(), radius=radius, align_corners=align_corners, want=("grad", "density"))
        d, g = o["density"][:, 0], o["grad"]
        r = d - t
        evals = evals + active.to(torch.int32)
        bad = active & ~torch.isfinite(r)
        status = put(status, bad, 3)
        if k == 0:
            best_s = torch.where(bad, zero, best_s)
            best_r = torch.where(bad, r, best_r)
        active = active & ~bad
        better = active & (r.abs() < best_r.abs()) if k else active
        best_s = torch.where(better, s, best_s)
        best_r = torch.where(better, r, best_r)
        conv = active & (r.abs() <= tol)
        status = put(status, conv, 0)
        active = active & ~conv
        if k == K:
            status = put(status, active, 1)
            break
        neg, pos = active & (r < 0), active & (r > 0)
        a, has_a = torch.where(neg, s, a), has_a | neg
        b, has_b = torch.where(pos, s, b), has_b | pos
        gn0 = g[:, 0] * n[:, 0]
        gn1 = g[:, 1] * n[:, 1]
        gn2 = g[:, 2] * n[:, 2]
        gn = gn0 + gn1
        gn = gn + gn2
        st = r / gn
        c = s - st
        c = torch.where(c < lo_md, lo_md, c)
        c = torch.where(c > hi_md, hi_md, c)
        both = has_a & has_b
        blo, bhi = torch.where(a < b, a, b), torch.where(a < b, b, a)
        ab = a + b
        mid = 0.5 * ab
        c = torch.where(both & ~((c > blo) & (c < bhi)), mid, c)
        nonfin = active & ~torch.isfinite(c)
        status = put(status, nonfin, 3)
        active = active & ~nonfin
        pinned = active & (c == s)
        status = put(status, pinned, 2)
        active = active & ~pinned
        cn = c[:, None] * n
        qc = p0 + cn
        out = active & (qc.abs() > rad).any(1)
        status = put(status, out, 2)
        active = active & ~out
        s = torch.where(active, c, s)
    return best_s, best_r, status, evals


def vertex_normals(vertices, faces, dtype=np.float64):
    """Area-weighted vertex normals (the sum of the faces' cross products), not normalised."""
    v = np.asarray(vertices).astype(dtype)
    f = np.asarray(faces, np.int64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    out = np.zeros_like(v)
    for k in range(3):
        np.add.at(out, f[:, k], fn)
    return out


@functools.lru_cache(maxsize=1)
def face_points():
    """One point per face of set A (rng(0) Dirichlet barycentrics) and the interpolated, outward, area-weighted vertex normal
    there, normalised -> (points f32 [Nf, 3], directions f32 [Nf, 3]).  Cached: treat it as read-only."""
    A = _projref.mesh_set_a()
    v, f = A["vertices"].astype(np.float64), A["faces"]
    w = np.random.default_rng(0).dirichlet(np.ones(3), len(f))
    vn = vertex_normals(v, f)
    vn = vn / np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-30)
    p = (v[f] * w[:, :, None]).sum(1)
    n = (vn[f] * w[:, :, None]).sum(1)
    n = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    # outward: against the density's gradient (the density falls towards the outside)
    d, g = _projref.value_grad(A["planes"], A["Ws"], A["bs"], p, np.float64)
    if np.median((g * n).sum(1)) > 0:
        n = -n
    return np.ascontiguousarray(p, np.float32), np.ascontiguousarray(n, np.float32)
