"""NumPy restatement of the curvature kernels (csrc/mesh_curvature.hip), operation for operation: fp64 on the fp32 positions,
every product, sum, quotient and square root its own rounded operation, sums in the kernels' order.  Needs no device.  Only
`deficit` goes through a library function (arctan2), where host and device may differ by a few ulps per angle.

Also the small meshes the curvature tests share."""
import math

import numpy as np

TWO_PI = 6.283185307179586


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


# ---------------------------------------------------------------------------------------------- topology
def corner_csr(F, nv):
    """(vfs [nv + 1], vfc): the corners of every vertex in ascending corner index (a stable sort of the flattened faces)."""
    flat = np.asarray(F, np.int64).reshape(-1)
    vfc = np.argsort(flat, kind="stable")
    vfs = np.searchsorted(flat[vfc], np.arange(nv + 1))
    return vfs, vfc


def _edges(F):
    F = np.asarray(F, np.int64).reshape(-1, 3)
    a = np.concatenate([F[:, 0], F[:, 1], F[:, 2]])
    b = np.concatenate([F[:, 1], F[:, 2], F[:, 0]])
    return np.minimum(a, b), np.maximum(a, b)


def fixed_vertices(F, nv):
    """fixed[u] = an edge at u does not have exactly two faces (the smoothing filter's flags)."""
    lo, hi = _edges(F)
    fixed = np.zeros(nv, bool)
    if len(lo):
        keys, counts = np.unique(lo * (nv + 1) + hi, return_counts=True)
        bad = keys[counts != 2]
        fixed[bad // (nv + 1)] = True
        fixed[bad % (nv + 1)] = True
    return fixed


def neighbour_csr(F, nv):
    """(start [nv + 1], nb): row u = the distinct neighbours of u in ascending order."""
    lo, hi = _edges(F)
    pairs = np.unique(np.concatenate([lo * (nv + 1) + hi, hi * (nv + 1) + lo])) if len(lo) else np.zeros(0, np.int64)
    u, v = pairs // (nv + 1), pairs % (nv + 1)
    return np.searchsorted(u, np.arange(nv + 1)), v


# ---------------------------------------------------------------------------------------------- the rule
def corner_terms(V, F):
    """Per corner c = 3 t + s of the faces, seen from i = F[t, s]: dict of arrays [3 Nf] (and vectors [3 Nf, 3])."""
    P = np.asarray(V, np.float32).astype(np.float64)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    i, j, k = F.reshape(-1), np.roll(F, -1, 1).reshape(-1), np.roll(F, -2, 1).reshape(-1)
    pi, pj, pk = P[i], P[j], P[k]
    with np.errstate(all="ignore"):
        e1, e2 = pj - pi, pk - pi
        g = _cross(e1, e2)
        a2 = np.sqrt(_dot(g, g))
        used = (a2 > 0.0) & (a2 < np.inf)
        ij, ik = pi - pj, pi - pk
        di, dj, dk = _dot(e1, e2), _dot(ij, pk - pj), _dot(ik, pj - pk)
        cot_j, cot_k = dj / a2, dk / a2
        theta = np.arctan2(a2, di)
        voronoi = ~((di < 0.0) | (dj < 0.0) | (dk < 0.0))
        at_i = ~voronoi & (di < 0.0)
        area = np.where(voronoi, (_dot(e1, e1) * cot_k + _dot(e2, e2) * cot_j) / 8.0, np.where(at_i, a2 / 4.0, a2 / 8.0))
        kv = cot_k[:, None] * ij + cot_j[:, None] * ik
    return {"used": used, "area": area, "theta": theta, "kv": kv, "g": g, "voronoi": voronoi & used, "obtuse_here": at_i & used,
            "obtuse_elsewhere": ~voronoi & ~at_i & used}


def terms(V, F, outward=1.0):
    """-> (area, deficit, hint f64 [nv], valid bool [nv], n int [nv] the contributing faces)."""
    nv = len(V)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    c = corner_terms(V, F)
    vfs, vfc = corner_csr(F, nv)
    fixed = fixed_vertices(F, nv)
    area, deficit, hint = np.zeros(nv), np.zeros(nv), np.zeros(nv)
    valid, count = np.zeros(nv, bool), np.zeros(nv, np.int64)
    for u in range(nv):
        A, Th, n = np.float64(0.0), np.float64(0.0), 0
        Kv, N = np.zeros(3), np.zeros(3)
        for x in vfc[vfs[u]:vfs[u + 1]]:
            if not c["used"][x]:
                continue
            A = A + c["area"][x]
            Th = Th + c["theta"][x]
            Kv = Kv + c["kv"][x]
            N = N + c["g"][x]
            n += 1
        count[u] = n
        ok = (not fixed[u]) and vfs[u + 1] > vfs[u] and A > 0.0
        if ok:
            kn = _dot(Kv, N)
            sg = 1.0 if kn > 0.0 else (-1.0 if kn < 0.0 else 0.0)
            area[u], deficit[u], valid[u] = A, TWO_PI - Th, True
            hint[u] = ((outward * sg) * np.sqrt(_dot(Kv, Kv))) / 4.0
    return area, deficit, hint, valid, count


def ring(channels, valid, start, nb, rounds):
    """channels: f64 arrays [nv] (any number); `rounds` times x'_u = x_u + the sum over the valid v of row u, in row order."""
    xs = [np.where(valid, np.asarray(x, np.float64), 0.0) for x in channels]
    for _ in range(rounds):
        ys = [x.copy() for x in xs]
        for u in np.nonzero(valid)[0]:
            for v in nb[start[u]:start[u + 1]]:
                if valid[v]:
                    for x, y in zip(xs, ys):
                        y[u] = y[u] + x[v]
        xs = ys
    return xs


def finish(area, deficit, hint, valid):
    with np.errstate(all="ignore"):
        mean = np.where(valid, (hint / area).astype(np.float32), np.float32(np.nan))
        gauss = np.where(valid, (deficit / area).astype(np.float32), np.float32(np.nan))
    return mean.astype(np.float32), gauss.astype(np.float32)


def curvature(V, F, rings=0, outward=1.0):
    """-> (mean f32, gauss f32, valid bool), the whole rule."""
    area, deficit, hint, valid, _ = terms(V, F, outward)
    if rings:
        start, nb = neighbour_csr(F, len(V))
        hint, deficit, area = ring([hint, deficit, area], valid, start, nb, rings)
    return finish(area, deficit, hint, valid) + (valid,)


def principal(mean, gauss):
    h, k = np.asarray(mean, np.float32).astype(np.float64), np.asarray(gauss, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        d = h * h - k
        root = np.sqrt(np.where(d < 0.0, 0.0, d))
        return (h + root).astype(np.float32), (h - root).astype(np.float32)


def _clamp01(w):
    return np.where(w < 0.0, 0.0, np.where(w > 1.0, 1.0, w))


def attribute_at(points, face, V, F, values):
    """values f32 [nv, C] at points on faces -> f32 [M, C] (sculpt_surface_attribute_at)."""
    P = np.asarray(V, np.float32).astype(np.float64)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    vals = np.asarray(values, np.float32)
    flat = vals.ndim == 1
    vals = vals.reshape(len(P), -1)
    q = np.asarray(points, np.float32).astype(np.float64)
    face = np.asarray(face, np.int64)
    inside = (face >= 0) & (face < len(F))
    idx = F[np.where(inside, face, 0)]
    pa, pb, pc = P[idx[:, 0]], P[idx[:, 1]], P[idx[:, 2]]
    out = np.full((len(q), vals.shape[1]), np.nan, np.float32)
    with np.errstate(all="ignore"):
        g = _cross(pb - pa, pc - pa)
        gg = _dot(g, g)
        qa, qb, qc = pa - q, pb - q, pc - q
        w0 = _clamp01(_dot(_cross(qb, qc), g) / gg)
        w1 = _clamp01(_dot(_cross(qc, qa), g) / gg)
        w2 = _clamp01((1.0 - w0) - w1)
        for ch in range(vals.shape[1]):
            s, ws, n = np.zeros(len(q)), np.zeros(len(q)), np.zeros(len(q), np.int64)
            for m, w in enumerate((w0, w1, w2)):
                x = vals[idx[:, m], ch]
                use = ~np.isnan(x)
                s = np.where(use, s + w * x.astype(np.float64), s)
                ws = np.where(use, ws + w, ws)
                n += use
            r = np.where(n == 3, s.astype(np.float32), np.where(n == 0, np.float32(np.nan), (s / ws).astype(np.float32)))
            out[:, ch] = np.where(inside, r, np.float32(np.nan))
    return out[:, 0] if flat else out


# ---------------------------------------------------------------------------------------------- meshes (faces wind outward)
def icosphere(level, radius=1.0):
    t = (1.0 + math.sqrt(5.0)) / 2.0
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in V]
    for _ in range(level):
        mid, G = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = V[a] + V[b]
                V.append(p / np.linalg.norm(p))
                mid[key] = len(V) - 1
            return mid[key]

        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            G += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = G
    return (np.asarray(V) * radius).astype(np.float32), np.asarray(F, np.int32)


def grid(nx, ny, sx=1.0, sy=1.0, shear=0.0):
    """An open planar nx x ny vertex grid in z = 0, two triangles a cell, normals +z; vertex (i, j) at ((i + shear j) sx, j sy)."""
    xs, ys = np.meshgrid(np.arange(nx) * 1.0, np.arange(ny) * sy, indexing="ij")
    xs = (xs + shear * np.arange(ny)[None, :]) * sx
    V = np.stack([xs, ys, np.zeros_like(xs)], -1).reshape(-1, 3).astype(np.float32)
    F = []
    for i in range(nx - 1):
        for j in range(ny - 1):
            a, b, c, d = i * ny + j, (i + 1) * ny + j, (i + 1) * ny + j + 1, i * ny + j + 1
            F += [(a, b, c), (a, c, d)]
    return V, np.asarray(F, np.int32)


def torus(n=12, m=8, R=2.0, r=0.75):
    V, F = [], []
    for i in range(n):
        for j in range(m):
            a, b = 2 * math.pi * i / n, 2 * math.pi * j / m
            V.append(((R + r * math.cos(b)) * math.cos(a), (R + r * math.cos(b)) * math.sin(a), r * math.sin(b)))
            p, q, s, t = i * m + j, ((i + 1) % n) * m + j, ((i + 1) % n) * m + (j + 1) % m, i * m + (j + 1) % m
            F += [(p, q, s), (p, s, t)]
    return np.asarray(V, np.float32), np.asarray(F, np.int32)


def cube(flip_diagonals=False):
    V = np.asarray([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    F = []
    for a, b, c, d in quads:
        F += [(b, c, d), (b, d, a)] if flip_diagonals else [(a, b, c), (a, c, d)]
    return V, np.asarray(F, np.int32)


def stretched_grid():
    """A 6 x 6 grid of half-sheared cells stretched 8 : 1 and bent into a shallow bowl: every triangle is obtuse, so an interior
    vertex meets both obtuse branches (the obtuse angle at itself, and at another corner).  A pure stretch of right-angled
    cells would keep their right angles."""
    V, F = grid(6, 6, 8.0, 1.0, shear=0.5)
    V[:, 2] = (0.002 * (V[:, 0] - 30.0) ** 2 + 0.05 * (V[:, 1] - 2.5) ** 2).astype(np.float32)
    return V, F


def pinch():
    """Two tetrahedra that share vertex 0 alone: every edge has two faces, vertex 0 is a bow-tie."""
    V = np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)], np.float32)
    F = np.asarray([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3), (0, 4, 5), (0, 6, 4), (0, 5, 6), (4, 6, 5)], np.int32)
    return V, F


def fin():
    """A tetrahedron with one more face on the edge (0, 1): that edge has three faces."""
    V = np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0.5, -1, -1)], np.float32)
    F = np.asarray([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3), (0, 1, 4)], np.int32)
    return V, F


def double_cone(n=70):
    """A closed double cone: two apexes of valence n over an n-gon."""
    ring_ = [(math.cos(2 * math.pi * i / n), math.sin(2 * math.pi * i / n), 0.0) for i in range(n)]
    V = np.asarray(ring_ + [(0, 0, 1.5), (0, 0, -1.0)], np.float32)
    F = []
    for i in range(n):
        j = (i + 1) % n
        F += [(i, j, n), (j, i, n + 1)]
    return V, np.asarray(F, np.int32)


def with_unreferenced():
    V, F = icosphere(0)
    return np.concatenate([V[:5], np.asarray([[9, 9, 9]], np.float32), V[5:]]), np.where(F >= 5, F + 1, F).astype(np.int32)


def with_zero_area_face():
    """A tetrahedron whose edge (1, 2) is split at its exact midpoint 4, with the sliver (1, 4, 2) of three distinct collinear
    vertices between the two halves and the face it was cut from: closed, every edge with two faces."""
    V = np.asarray([(0, 0, 0), (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0)], np.float32)
    F = np.asarray([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 4, 3), (4, 2, 3), (1, 2, 4)], np.int32)
    return V, F


def permuted(F, seed):
    return np.ascontiguousarray(np.asarray(F)[np.random.default_rng(seed).permutation(len(F))])


MESHES = {"icosphere2": lambda: icosphere(2), "cube": cube, "torus": torus, "stretched": stretched_grid, "open_grid": lambda: grid(5, 5),
          "pinch": pinch, "fin": fin, "double_cone": double_cone, "unreferenced": with_unreferenced,
          "zero_area": with_zero_area_face}
