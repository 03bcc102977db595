"""NumPy restatement of the device smoother (csrc/mesh_smooth.hip, sf3d/remesh_device.py smooth_device): the neighbour table,
the fixed flags and Taubin's lambda|mu iterations with the kernel's order of operations -- per vertex the sum of the
neighbours' positions in ascending index order, one IEEE division by the degree, then p + k * (c - p) as a subtraction, a
product and a sum.  NumPy fuses nothing, so in float32 `taubin` equals the device bit for bit; in float64 it is the
yard-stick.  Also the small meshes both test files use."""
import numpy as np

LAMBDA, MU = 0.5, -0.53


# ------------------------------------------------------------------------------------------------------------- topology
def unique_edges(F):
    """(edges [ne, 2] with u < v in ascending (u, v) order, faces per edge [ne])."""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    if len(F) == 0:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
    he = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    he.sort(axis=1)
    return np.unique(he, axis=0, return_counts=True)


def neighbour_table(F, nv):
    """CSR (start i32 [nv + 1], nb i32 [2 ne]): row u = the distinct neighbours of u, ascending."""
    E, _ = unique_edges(F)
    d = np.concatenate([E, E[:, ::-1]])
    d = d[np.lexsort((d[:, 1], d[:, 0]))]
    start = np.searchsorted(d[:, 0], np.arange(nv + 1)).astype(np.int32)
    return start, d[:, 1].astype(np.int32)


def fixed_flags(F, nv):
    """u8 [nv]: 1 where an edge at the vertex does not have exactly two faces (open border, non-manifold edge)."""
    E, count = unique_edges(F)
    fixed = np.zeros(nv, np.uint8)
    fixed[E[count != 2].reshape(-1)] = 1
    return fixed


# ------------------------------------------------------------------------------------------------------------ the filter
def half_step(p, k, start, nb, move):
    """One half-step on p [nv, 3] (float32 or float64) with factor k of the same type -> q."""
    deg = np.diff(start)
    s = np.zeros_like(p)
    rows = np.nonzero(deg > 0)[0]
    s[rows] = p[nb[start[rows]]]
    for j in range(1, int(deg.max()) if len(deg) else 0):     # column j of every row that has one: the sum stays in row order
        rows = np.nonzero(deg > j)[0]
        s[rows] = s[rows] + p[nb[start[rows] + j]]
    q = p.copy()
    m = np.nonzero(move)[0]
    c = s[m] / deg[m].astype(p.dtype)[:, None]
    q[m] = p[m] + k * (c - p[m])
    return q


def taubin(P, F, n, lam=LAMBDA, mu=MU, dtype=np.float32):
    """n iterations of (lam, then mu; mu == 0: lam alone) on the positions P rounded once to `dtype` -> [nv, 3] of that type."""
    dtype = np.dtype(dtype).type
    p = np.ascontiguousarray(np.asarray(P).reshape(-1, 3), dtype)
    nv = len(p)
    start, nb = neighbour_table(F, nv)
    move = (np.diff(start) > 0) & (fixed_flags(F, nv) == 0)
    for _ in range(int(n)):
        for k in ((lam,) if mu == 0 else (lam, mu)):
            p = half_step(p, dtype(k), start, nb, move)
    return p


# --------------------------------------------------------------------------------------------------------------- measures
def signed_volume(P, F):
    a, b, c = (np.asarray(P, np.float64)[np.asarray(F)[:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def radius_rms(P):
    r = np.linalg.norm(np.asarray(P, np.float64), axis=1)
    return float(np.sqrt(np.mean((r - r.mean()) ** 2)))


# ----------------------------------------------------------------------------------------------------------------- meshes
def tetrahedron():
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    return P, F


def octahedron():
    P = np.array([[1, 0, 0], [-1, 0, 0], [0, 1.25, 0], [0, -0.75, 0], [0, 0, 1.5], [0.125, 0, -0.5]], np.float32)
    F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return P, F


def grid_patch(n=5, seed=3):
    """An n x n-vertex open patch, two triangles per cell, with some relief so that the interior moves in every coordinate."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:n, 0:n]
    P = np.stack([x / (n - 1.0), y / (n - 1.0), 0.1 * rng.standard_normal((n, n))], -1).reshape(-1, 3).astype(np.float32)
    i = (y[:-1, :-1] * n + x[:-1, :-1]).reshape(-1)
    F = np.concatenate([np.stack([i, i + 1, i + n + 1], 1), np.stack([i, i + n + 1, i + n], 1)]).astype(np.int32)
    return P, F


def patch_border(n=5):
    y, x = np.mgrid[0:n, 0:n]
    return ((x == 0) | (x == n - 1) | (y == 0) | (y == n - 1)).reshape(-1)


def double_cone(n=70, seed=4):
    """Closed: a ring of n vertices (2 .. n + 1) between two apexes (0, 1), each with n neighbours; n + 2 vertices, 2 n faces."""
    rng = np.random.default_rng(seed)
    t = 2 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(t), np.sin(t), 0.05 * rng.standard_normal(n)], 1)
    P = np.concatenate([[[0.1, -0.05, 1.0], [-0.05, 0.1, -1.25]], ring]).astype(np.float32)
    a, b = 2 + np.arange(n), 2 + (np.arange(n) + 1) % n
    F = np.concatenate([np.stack([np.zeros(n, int), a, b], 1), np.stack([np.ones(n, int), b, a], 1)]).astype(np.int32)
    return P, F


def two_components_and_an_orphan():
    """A tetrahedron, an octahedron and, between them in index order, a vertex no face names."""
    P1, F1 = tetrahedron()
    P2, F2 = octahedron()
    P = np.concatenate([P1, [[7.0, -3.0, 2.5]], P2 + np.float32(3.0)]).astype(np.float32)
    return P, np.concatenate([F1, F2 + 5]).astype(np.int32)


ORPHAN = 4


def three_face_edge():
    """The octahedron with a fin: a third face on the edge {0, 2}.  That edge has three faces (both its ends are fixed), the
    fin's other two edges have one (the fin's tip, vertex 6, is fixed too); vertices 1, 3, 4, 5 move."""
    P, F = octahedron()
    P = np.concatenate([P, [[1.5, 1.5, 0.25]]]).astype(np.float32)
    return P, np.concatenate([F, [[0, 6, 2]]]).astype(np.int32)


def icosphere(subdivisions=4):
    """Unit icosphere: 10 x 4^s + 2 vertices (float64), outward faces."""
    g = (1 + 5 ** 0.5) / 2
    P = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    P = [np.array(p, np.float64) / np.linalg.norm(p) for p in P]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = P[a] + P[b]
                P.append(x / np.linalg.norm(x))
                mid[key] = len(P) - 1
            return mid[key]

        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = out
    return np.array(P, np.float64), np.array(F, np.int32)


def noisy_icosphere(subdivisions=4, sigma=0.01, seed=0):
    """The icosphere with Gaussian noise of `sigma` per coordinate -> (P float32, F)."""
    P, F = icosphere(subdivisions)
    return (P + sigma * np.random.default_rng(seed).standard_normal(P.shape)).astype(np.float32), F
