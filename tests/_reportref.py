"""NumPy restatement of the mesh report (sculptmate_amd/csrc/mesh_report.hip; ops.mesh_report, ops.mesh_self_intersections) --
test infrastructure, written for reading, not for speed.  It shares no code with the ops.

Self-intersections are the rule at the top of csrc/mesh_report.hip by brute force over ALL pairs i < j, box clause included and no
grid: fp64 on the fp32 positions widened, every operation a NumPy call of its own (NumPy never contracts), so the integers are the
device's.  The edge census is a dictionary over the undirected edges."""
import itertools

import numpy as np


# ------------------------------------------------------------------------------------------------------------------ the rule
def orient(P, a, b, c, d):
    """Sign (int64) of the determinant of (P[b] - P[a], P[c] - P[a], P[d] - P[a]) for index arrays; 0 wherever two of the four
    indices are equal.  P is fp64."""
    u, v, w = P[b] - P[a], P[c] - P[a], P[d] - P[a]
    det = (u[:, 0] * (v[:, 1] * w[:, 2] - v[:, 2] * w[:, 1]) - u[:, 1] * (v[:, 0] * w[:, 2] - v[:, 2] * w[:, 0])) \
        + u[:, 2] * (v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0])
    repeated = (a == b) | (a == c) | (a == d) | (b == c) | (b == d) | (c == d)
    return np.where(repeated, 0, np.sign(det)).astype(np.int64)


def segment_meets(P, p, q, a, b, c):
    """bool per row: the segment (p, q) meets the closed triangle (a, b, c), end points in the plane not counting."""
    through = orient(P, a, b, c, p) * orient(P, a, b, c, q) < 0
    s = np.stack([orient(P, p, q, a, b), orient(P, p, q, b, c), orient(P, p, q, c, a)], 1)
    one_side = ((s >= 0).all(1) | (s <= 0).all(1)) & (s != 0).any(1)
    return through & one_side


def faces_meet(P, Fi, Fj):
    """bool per row of two [m, 3] index arrays: some edge of one face meets the other triangle (the box clause is the caller's)."""
    hit = np.zeros(len(Fi), bool)
    for k in range(3):
        hit |= segment_meets(P, Fi[:, k], Fi[:, (k + 1) % 3], Fj[:, 0], Fj[:, 1], Fj[:, 2])
        hit |= segment_meets(P, Fj[:, k], Fj[:, (k + 1) % 3], Fi[:, 0], Fi[:, 1], Fi[:, 2])
    return hit


def self_intersections(vertices, faces):
    """(pairs int64 [count, 2] lexicographic with i < j, flags bool [Nf]) over ALL pairs."""
    P32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    nf = len(F)
    flags = np.zeros(nf, bool)
    if nf < 2:
        return np.zeros((0, 2), np.int64), flags
    P = P32.astype(np.float64)
    corners = P32[F]                                   # [nf, 3, 3], fp32: the box clause compares fp32 values
    mn, mx = corners.min(1), corners.max(1)
    out = []
    step = max(1, 2_000_000 // nf)
    for s in range(0, nf, step):
        i = np.arange(s, min(nf, s + step))
        box = ((mn[i][:, None, :] <= mx[None, :, :]) & (mn[None, :, :] <= mx[i][:, None, :])).all(2)
        ii, jj = np.nonzero(box)
        ii = i[ii]
        keep = ii < jj
        ii, jj = ii[keep], jj[keep]
        hit = faces_meet(P, F[ii], F[jj])
        out.append(np.stack([ii[hit], jj[hit]], 1))
    pairs = np.concatenate(out).astype(np.int64)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    flags[pairs.reshape(-1)] = True
    return pairs, flags


# ------------------------------------------------------------------------------------------------------------------ census
def edge_census(faces):
    """dict of ints over the undirected edges: every face gives three half-edges (F[k], F[(k + 1) % 3]), self-loops included."""
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    starts = {}
    for f in F.tolist():
        for k in range(3):
            a, b = f[k], f[(k + 1) % 3]
            starts.setdefault((min(a, b), max(a, b)), []).append(a)
    n = [len(s) for s in starts.values()]
    return {"edges": len(starts), "border_edges": sum(1 for c in n if c == 1), "nonmanifold_edges": sum(1 for c in n if c >= 3),
            "inconsistent_edges": sum(1 for s in starts.values() if len(s) == 2 and s[0] == s[1]),
            "referenced_vertices": len(set(F.reshape(-1).tolist()))}


def face_measures(vertices, faces):
    """(area2 f64 [Nf], vol6 f64 [Nf], degenerate bool [Nf])."""
    P = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = P[F[:, 0]], P[F[:, 1]], P[F[:, 2]]
    u, v = b - a, c - a
    n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    area2 = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    vol6 = (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) - a[:, 1] * (b[:, 0] * c[:, 2] - b[:, 2] * c[:, 0])) \
        + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])
    repeated = (F[:, 0] == F[:, 1]) | (F[:, 1] == F[:, 2]) | (F[:, 0] == F[:, 2])
    return area2, vol6, repeated | (area2 == 0)


def components(faces):
    """The number of connected components that have a face (union-find over the vertices the faces name)."""
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in F.tolist():
        ra = find(a)
        for o in (b, c):
            ro = find(o)
            if ro != ra:
                parent[ro] = ra
    return len({find(x) for x in list(parent)})


def report(vertices, faces, self_intersections_too=True):
    """The dict of ops.mesh_report, with the sums in NumPy's order."""
    V = np.asarray(vertices, np.float32).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    r = {"vertices": len(V), "faces": len(F)}
    r.update(edge_census(F))
    area2, vol6, deg = face_measures(V, F)
    r["degenerate_faces"] = int(deg.sum())
    r["components"] = components(F)
    r["euler"] = r["referenced_vertices"] - r["edges"] + r["faces"]
    r["is_watertight"] = r["faces"] > 0 and r["border_edges"] == 0 and r["nonmanifold_edges"] == 0
    r["is_winding_consistent"] = r["inconsistent_edges"] == 0 and r["nonmanifold_edges"] == 0
    g2 = 2 * r["components"] - r["euler"]
    r["genus"] = g2 // 2 if r["is_watertight"] and r["is_winding_consistent"] and g2 >= 0 and g2 % 2 == 0 else None
    r["area"] = float(area2.sum()) / 2.0
    r["volume"] = float(vol6.sum()) / 6.0
    r["is_volume"] = bool(r["is_watertight"] and r["is_winding_consistent"] and r["volume"] > 0)
    if self_intersections_too:
        pairs, flags = self_intersections(V, F)
        r["self_intersections"] = len(pairs)
        r["self_intersecting_faces"] = int(flags.sum())
    return r


# ------------------------------------------------------------------------------------------------------------------ meshes
CUBE_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                       [1, 5, 7], [1, 7, 3]], np.int64)


def cube(side=4.0, offset=(0.0, 0.0, 0.0)):
    """The fixed triangulation of a cube: corners itertools.product([0, 1], repeat=3) scaled and moved."""
    v = np.array(list(itertools.product([0, 1], repeat=3)), np.float64) * side + np.asarray(offset, np.float64)
    return v.astype(np.float32), CUBE_FACES.copy()


def join(*meshes):
    """Several meshes as one, indices shifted, no vertex shared."""
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32))
        fs.append(np.asarray(f, np.int64) + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def torus(nu=48, nv=24, R=2.0, r=0.75):
    """A closed nu x nv torus, two triangles a quad, consistently wound."""
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = 2 * np.pi * i / nu, 2 * np.pi * j / nv
    v = np.stack([(R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)], -1).reshape(-1, 3)
    idx = lambda x, y: ((x % nu) * nv + (y % nv)).reshape(-1)   # noqa: E731
    q = [idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)]
    f = np.concatenate([np.stack([q[0], q[1], q[2]], 1), np.stack([q[0], q[2], q[3]], 1)])
    return v.astype(np.float32), f.astype(np.int64)


def icosphere(levels=3, radius=1.0, center=(0.0, 0.0, 0.0)):
    """20 * 4^levels faces on a sphere (levels=3: 1 280)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return (np.asarray(v) * radius + np.asarray(center, np.float64)).astype(np.float32), np.asarray(f, np.int64)
