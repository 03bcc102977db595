"""NumPy restatement of the device Loop subdivision (csrc/mesh_subdivide.hip, sf3d/remesh_device.py loop_subdivide_device), built
from the faces F alone: the unique edges in the order of their sorted (min, max) keys with their half-edges in ascending order,
the vertex fans in ascending corner order, the numbering of the new vertices by the first appearance of their edge over the
half-edges, the face template, and the masks in float64 with the kernel's order of operations, rounded once to float32.  NumPy
fuses nothing and the kernel is compiled without contraction, so `subdivide` equals the device bit for bit.  The mesh builders
are those of tests/_smoothref.py."""
import numpy as np

from _smoothref import (double_cone, grid_patch, icosphere, octahedron, patch_border, tetrahedron, three_face_edge,  # noqa: F401
                        two_components_and_an_orphan, ORPHAN)


def two_tetrahedra_sharing_a_vertex():
    """Two closed tetrahedra that meet in vertex 0 alone: every edge has two faces, vertex 0 has a fan of six faces in two
    umbrellas -- it takes the interior rule with n = 6."""
    P1, F1 = tetrahedron()
    P = np.concatenate([P1, -P1[1:] - np.float32(0.25)]).astype(np.float32)
    F2 = F1.copy()
    F2[F1 > 0] += 3
    return P, np.concatenate([F1, F2]).astype(np.int32)


def flat_grid(n=5, z=0.25):
    """An n x n-vertex planar patch of valence 6 inside, coordinates k / 8 (dyadic: every mask is exact), z constant."""
    y, x = np.mgrid[0:n, 0:n]
    P = np.stack([x / 8.0, y / 8.0, np.full((n, n), z)], -1).reshape(-1, 3).astype(np.float32)
    return P, grid_patch(n)[1]


# ------------------------------------------------------------------------------------------------------------- topology
class Topology:
    """What a level needs of F [nf, 3] over nv vertices, in the device's orders:
        edges [ne, 2]    (u, v) with u < v, ascending by (u, v) -- the order of the sorted half-edge keys
        count [ne]       faces per edge
        first_he [ne]    the lowest half-edge 3 f + k of the edge (the stable sort puts it first)
        opposite [ne, 2] the third vertices of the edge's first two faces in half-edge order (-1 where there is none)
        new_index [ne]   nv + (rank of first_he among all first half-edges) - 1
        fan_start [nv+1], fan_corner [3 nf]   the corners 3 f + k of every vertex, ascending"""

    def __init__(self, F, nv):
        F = np.asarray(F, np.int64).reshape(-1, 3)
        self.F, self.nv, self.nf = F, int(nv), len(F)
        h = np.arange(3 * self.nf)
        a, b = F.reshape(-1), F[:, [1, 2, 0]].reshape(-1)          # half-edge h = 3 f + k runs F[f][k] -> F[f][(k + 1) % 3]
        key = (np.minimum(a, b) << 32) | np.maximum(a, b)
        order = np.argsort(key, kind="stable")
        skey = key[order]
        head = np.ones(len(skey), bool)
        head[1:] = skey[1:] != skey[:-1]
        start = np.nonzero(head)[0]
        self.ne = len(start)
        self.edges = np.stack([skey[start] >> 32, skey[start] & 0xFFFFFFFF], 1).reshape(-1, 2)
        self.count = np.diff(np.append(start, len(skey)))
        self.first_he = order[start] if self.ne else np.zeros(0, np.int64)
        third = F[h // 3, (h % 3 + 2) % 3]                           # the vertex of the half-edge's face that is not on it
        self.opposite = np.full((self.ne, 2), -1, np.int64)
        self.opposite[:, 0] = third[order[start]] if self.ne else 0
        two = self.count >= 2
        self.opposite[two, 1] = third[order[start[two] + 1]]
        is_first = np.zeros(3 * self.nf, np.int64)
        is_first[self.first_he] = 1
        rank = np.cumsum(is_first)
        self.new_index = self.nv + rank[self.first_he] - 1
        self.edge_of_he = np.empty(3 * self.nf, np.int64)
        self.edge_of_he[order] = np.cumsum(head) - 1
        corners = np.argsort(F.reshape(-1), kind="stable")
        self.fan_corner = corners
        self.fan_start = np.searchsorted(F.reshape(-1)[corners], np.arange(self.nv + 1))

    def classes(self):
        """(border edges per vertex, touches a non-manifold edge, smallest / largest other end of a border edge (-1: none))."""
        nb = np.zeros(self.nv, np.int64)
        nm = np.zeros(self.nv, bool)
        lo, hi = np.full(self.nv, self.nv, np.int64), np.full(self.nv, -1, np.int64)
        for (u, v), c in zip(self.edges, self.count):
            if c == 1:
                for x, y in ((u, v), (v, u)):
                    nb[x] += 1
                    lo[x], hi[x] = min(lo[x], y), max(hi[x], y)
            elif c >= 3:
                nm[u] = nm[v] = True
        lo[lo == self.nv] = -1
        return nb, nm, lo, hi


# --------------------------------------------------------------------------------------------------------------- a level
def _masks(T, X):
    """The masks on the rows X [nv, C] float32 -> [nv + ne, C] float32: float64 arithmetic, the kernel's operations, one
    rounding.  Rows that keep their bits are copied."""
    X32 = np.ascontiguousarray(X, np.float32)
    X = X32.astype(np.float64)
    out = np.empty((T.nv + T.ne, X.shape[1]), np.float32)
    out[:T.nv] = X32
    nb, nm, lo, hi = T.classes()
    F = T.F
    for u in range(T.nv):
        b, e = T.fan_start[u], T.fan_start[u + 1]
        n = int(e - b)
        if n == 0 or nm[u] or nb[u] not in (0, 2):
            continue
        if nb[u] == 2:
            out[u] = 0.75 * X[u] + 0.125 * (X[lo[u]] + X[hi[u]])
            continue
        beta = 0.1875 if n == 3 else 3.0 / (8.0 * n)
        S = None
        for corner in T.fan_corner[b:e]:
            f, k = divmod(int(corner), 3)
            first, second = X[F[f, (k + 1) % 3]], X[F[f, (k + 2) % 3]]
            S = first if S is None else S + first
            S = S + second
        out[u] = (1.0 - n * beta) * X[u] + (0.5 * beta) * S
    for e in range(T.ne):
        u, v = T.edges[e]
        if T.count[e] == 2:
            a, b = T.opposite[e]
            q = 0.375 * (X[u] + X[v]) + 0.125 * (X[a] + X[b])
        else:
            q = 0.5 * (X[u] + X[v])
        out[T.new_index[e]] = q
    return out


def child_faces(T):
    """Face (a, b, c) -> (a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca) at rows 4 f .. 4 f + 3 -> int32 [4 nf, 3]."""
    mid = T.new_index[T.edge_of_he].reshape(-1, 3) if T.nf else np.zeros((0, 3), np.int64)
    a, b, c = T.F[:, 0], T.F[:, 1], T.F[:, 2]
    ab, bc, ca = mid[:, 0], mid[:, 1], mid[:, 2]
    return np.stack([a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca], 1).reshape(-1, 3).astype(np.int32)


def level(P, F, A=None):
    """One Loop level -> (P' f32 [nv + ne, 3], F' int32 [4 nf, 3], A' f32 or None)."""
    P = np.ascontiguousarray(np.asarray(P).reshape(-1, 3), np.float32)
    T = Topology(F, len(P))
    return _masks(T, P), child_faces(T), None if A is None else _masks(T, np.asarray(A, np.float32))


def subdivide(P, F, levels=1, A=None):
    """`levels` Loop levels; no faces: copies."""
    P = np.ascontiguousarray(np.asarray(P).reshape(-1, 3), np.float32).copy()
    F = np.ascontiguousarray(np.asarray(F).reshape(-1, 3), np.int32).copy()
    A = None if A is None else np.ascontiguousarray(A, np.float32).copy()
    if len(F):
        for _ in range(int(levels)):
            P, F, A = level(P, F, A)
    return P, F, A


def midpoint(P, F, levels=1):
    """The midpoint upsampling with the same numbering and faces: every new vertex the float32 midpoint."""
    P = np.ascontiguousarray(np.asarray(P).reshape(-1, 3), np.float32)
    F = np.ascontiguousarray(np.asarray(F).reshape(-1, 3), np.int32)
    for _ in range(int(levels)):
        T = Topology(F, len(P))
        Q = np.empty((T.nv + T.ne, 3), np.float32)
        Q[:T.nv] = P
        Q[T.new_index] = np.float32(0.5) * (P[T.edges[:, 0]] + P[T.edges[:, 1]])
        P, F = Q, child_faces(T)
    return P, F


# --------------------------------------------------------------------------------------------------------------- measures
def edge_face_counts(F):
    return Topology(F, int(np.asarray(F).max()) + 1 if len(F) else 0).count


def euler(nv, F):
    """V - E + F over the vertices the faces name."""
    T = Topology(F, nv)
    return len(np.unique(T.F)) - T.ne + T.nf
