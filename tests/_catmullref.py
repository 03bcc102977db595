"""NumPy restatement of the device Catmull-Clark subdivision (csrc/mesh_catmull.hip, sf3d/remesh_device.py catmull_clark_device;
the rule is stated in include/sculpt_hip.h), built from the faces F [nf, k] alone, k = 3 or 4: the unique edges in the order of
their sorted (min, max) keys with their half-edges in ascending order, the vertex fans in ascending corner order, the edge
points numbered by the first appearance of their edge over the half-edges, the quad template, the masks in float64 with the
kernel's order of operations, rounded once to float32, and the shorter-diagonal split on the refined float32 positions.  NumPy
fuses nothing and the kernel is compiled without contraction, so `subdivide` equals the device bit for bit.  The sums over a
fan run over the fan position with all vertices at once: the order within each vertex is the kernel's."""
import numpy as np


# ------------------------------------------------------------------------------------------------------------- topology
class Topology:
    """What a level needs of F [nf, k] over nv vertices, in the device's orders:
        edges [ne, 2]     (u, v) with u < v, ascending by (u, v) -- the order of the sorted half-edge keys
        count [ne]        faces per edge
        first_he [ne]     the lowest half-edge k f + c of the edge (the stable sort puts it first)
        faces2 [ne, 2]    the edge's first two faces in half-edge order (-1 where there is none)
        rank [ne]         the edge's rank by first appearance: its edge point is nv + nf + rank
        edge_of_he [k nf] the sorted edge of every half-edge
        fan_start [nv+1], fan_corner [k nf]   the corners k f + c of every vertex, ascending"""

    def __init__(self, F, nv):
        F = np.asarray(F, np.int64)
        assert F.ndim == 2 and F.shape[1] in (3, 4), F.shape
        self.F, self.nv, (self.nf, self.k) = F, int(nv), F.shape
        k = self.k
        a, b = F.reshape(-1), np.roll(F, -1, axis=1).reshape(-1)   # half-edge h = k f + c runs F[f][c] -> F[f][(c + 1) % k]
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
        self.faces2 = np.full((self.ne, 2), -1, np.int64)
        if self.ne:
            self.faces2[:, 0] = order[start] // k
            two = self.count >= 2
            self.faces2[two, 1] = order[start[two] + 1] // k
        is_first = np.zeros(k * self.nf, np.int64)
        is_first[self.first_he] = 1
        self.rank = np.cumsum(is_first)[self.first_he] - 1
        self.edge_of_he = np.empty(k * self.nf, np.int64)
        self.edge_of_he[order] = np.cumsum(head) - 1
        corners = np.argsort(F.reshape(-1), kind="stable")
        self.fan_corner = corners
        self.fan_start = np.searchsorted(F.reshape(-1)[corners], np.arange(self.nv + 1))

    def classes(self):
        """(border edges per vertex, touches a non-manifold edge, smallest / largest other end of a border edge (-1: none))."""
        nb = np.zeros(self.nv, np.int64)
        nm = np.zeros(self.nv, bool)
        lo, hi = np.full(self.nv, self.nv, np.int64), np.full(self.nv, -1, np.int64)
        for (u, v), c in zip(self.edges[self.count != 2], self.count[self.count != 2]):
            if c == 1:
                for x, y in ((u, v), (v, u)):
                    nb[x] += 1
                    lo[x], hi[x] = min(lo[x], y), max(hi[x], y)
            else:
                nm[u] = nm[v] = True
        lo[lo == self.nv] = -1
        return nb, nm, lo, hi


# --------------------------------------------------------------------------------------------------------------- a level
def face_points(T, X):
    """The UNROUNDED face points, float64 [nf, C]: (((X[c0] + X[c1]) + X[c2]) [+ X[c3]]) / k."""
    s = X[T.F[:, 0]] + X[T.F[:, 1]]
    for c in range(2, T.k):
        s = s + X[T.F[:, c]]
    return s / float(T.k)


def _masks(T, X32):
    """The masks on the rows X32 [nv, C] float32 -> [nv + nf + ne, C] float32: float64 arithmetic, the kernel's operations, one
    rounding.  Rows that keep their bits are copied."""
    X32 = np.ascontiguousarray(X32, np.float32)
    X = X32.astype(np.float64)
    nv, nf, ne, k, F = T.nv, T.nf, T.ne, T.k, T.F
    out = np.empty((nv + nf + ne, X.shape[1]), np.float32)
    out[:nv] = X32
    Fp = face_points(T, X)
    out[nv:nv + nf] = Fp
    # edge points
    u, v = T.edges[:, 0], T.edges[:, 1]
    q = 0.5 * (X[u] + X[v])
    two = T.count == 2
    f0, f1 = T.faces2[two, 0], T.faces2[two, 1]
    q[two] = 0.25 * ((X[u[two]] + X[v[two]]) + (Fp[f0] + Fp[f1]))
    out[nv + nf + T.rank] = q
    # old vertices
    nb, nm, lo, hi = T.classes()
    n = np.diff(T.fan_start)
    keeps = (n == 0) | nm | ((nb != 0) & (nb != 2))
    crease = ~keeps & (nb == 2)
    out[:nv][crease] = 0.75 * X[crease] + 0.125 * (X[lo[crease]] + X[hi[crease]])
    smooth = np.nonzero(~keeps & (nb == 0))[0]
    if len(smooth):
        SN = np.zeros((len(smooth), X.shape[1]))
        SQ = np.zeros_like(SN)
        for j in range(int(n[smooth].max())):        # fan position j of every vertex that has one: in corner order per vertex
            has = n[smooth] > j
            corner = T.fan_corner[T.fan_start[smooth[has]] + j]
            f, c = corner // k, corner % k
            nxt, prv = X[F[f, (c + 1) % k]], X[F[f, (c - 1) % k]]
            if j == 0:
                SN[has], SQ[has] = nxt, Fp[f]
            else:
                SN[has], SQ[has] = SN[has] + nxt, SQ[has] + Fp[f]
            SN[has] = SN[has] + prv
        m = n[smooth].astype(np.float64)[:, None]
        out[:nv][smooth] = ((m - 2.0) * X[smooth] + (0.5 * SN + SQ) / m) / m
    return out


def child_quads(T):
    """Corner c of face f -> row k f + c = (F[f, c], edge point of (f, c), nv + f, edge point of (f, (c - 1) % k)) -> int32."""
    k = T.k
    ep = (T.nv + T.nf + T.rank[T.edge_of_he]).reshape(-1, k) if T.nf else np.zeros((0, k), np.int64)
    fp = np.repeat(T.nv + np.arange(T.nf), k).reshape(-1, k)
    return np.stack([T.F, ep, fp, np.roll(ep, 1, axis=1)], -1).reshape(-1, 4).astype(np.int32)


def split(P32, Q):
    """Rows 2 q, 2 q + 1: quad q along its shorter diagonal -- float64 squared lengths (dx dx + dy dy) + dz dz of the float32
    positions; d13 < d02: (q0, q1, q3), (q1, q2, q3), otherwise (a tie included) (q0, q1, q2), (q0, q2, q3)."""
    P = np.asarray(P32, np.float32).astype(np.float64)
    Q = np.asarray(Q)

    def d2(a, b):
        d = P[a] - P[b]
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]

    q0, q1, q2, q3 = Q[:, 0], Q[:, 1], Q[:, 2], Q[:, 3]
    other = d2(q1, q3) < d2(q0, q2)
    a = np.stack([q0, q1, np.where(other, q3, q2)], 1)
    b = np.stack([np.where(other, q1, q0), q2, q3], 1)
    return np.stack([a, b], 1).reshape(-1, 3).astype(Q.dtype)


def level(P, F, A=None):
    """One level -> (P' f32 [nv + nf + ne, 3], quads int32 [k nf, 4], triangles int32 [2 k nf, 3], A' f32 or None)."""
    P = np.ascontiguousarray(np.asarray(P).reshape(-1, 3), np.float32)
    T = Topology(F, len(P))
    Pn, Q = _masks(T, P), child_quads(T)
    return Pn, Q, split(Pn, Q), None if A is None else _masks(T, np.asarray(A, np.float32))


def subdivide(P, F, levels=1, A=None):
    """`levels` levels (the first on F [nf, 3 or 4], the rest on its own quads); no faces: copies, empty quads and triangles."""
    P = np.ascontiguousarray(np.asarray(P).reshape(-1, 3), np.float32).copy()
    F = np.ascontiguousarray(np.asarray(F), np.int32)
    A = None if A is None else np.ascontiguousarray(A, np.float32).copy()
    Q, Tr = np.zeros((0, 4), np.int32), np.zeros((0, 3), np.int32)
    if len(F):
        for _ in range(int(levels)):
            P, Q, Tr, A = level(P, F, A)
            F = Q
    return P, Q, Tr, A


# ----------------------------------------------------------------------------------------------------------------- meshes
def cube(offset=(0.0, 0.0, 0.0)):
    """The cube [-1, 1]^3 (+ offset) as six quads wound counter-clockwise seen from outside."""
    P = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float32) + np.asarray(offset, np.float32)
    Q = np.array([[0, 2, 3, 1], [4, 5, 7, 6], [0, 1, 5, 4], [2, 6, 7, 3], [0, 4, 6, 2], [1, 3, 7, 5]], np.int32)
    return P, Q


def tetrahedron():
    P = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32)
    return P, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)


def single_quad():
    P = np.array([[0, 0, 0], [1, 0, 0.25], [1.5, 1, 0], [0, 1, 0.5]], np.float32)
    return P, np.array([[0, 1, 2, 3]], np.int32)


def quad_grid(n=4, z=0.25):
    """n x n quads over (n + 1)^2 vertices in the plane z, coordinates j / 8 (dyadic: every mask is exact)."""
    y, x = np.mgrid[0:n + 1, 0:n + 1]
    P = np.stack([x / 8.0, y / 8.0, np.full(x.shape, z)], -1).reshape(-1, 3).astype(np.float32)
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    return P, np.stack([i, i + 1, i + n + 2, i + n + 1], 1).astype(np.int32)


def two_cubes_sharing_an_edge():
    """Two cubes that meet along one edge: four faces on it (non-manifold), its ends corners."""
    P1, Q1 = cube()
    P2, _ = cube((2.0, 2.0, 0.0))
    # cube 1's edge x = y = 1 is vertices 3 (z = -1), 7 (z = 1); cube 2's edge x = y = 1 is its vertices 0, 4
    remap = np.array([3, 8, 9, 10, 7, 11, 12, 13])
    P = np.concatenate([P1, P2[[1, 2, 3, 5, 6, 7]]]).astype(np.float32)
    return P, np.concatenate([Q1, remap[Q1]]).astype(np.int32)


def two_cubes_sharing_a_vertex():
    """Two closed cubes that meet in one vertex alone: every edge has two faces, the shared vertex a fan of six in two umbrellas."""
    P1, Q1 = cube()
    P2, _ = cube((2.0, 2.0, 2.0))
    remap = np.array([7, 8, 9, 10, 11, 12, 13, 14])
    return np.concatenate([P1, P2[1:]]).astype(np.float32), np.concatenate([Q1, remap[Q1]]).astype(np.int32)


def closed_fan(n=70):
    """n triangles around an apex over a regular n-gon, closed by n triangles to a base centre: the apex (vertex 0) and the base
    centre (vertex 1) are interior vertices of valence n."""
    t = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(t), np.sin(t), 0.1 * np.cos(3 * t)], 1)
    P = np.concatenate([[[0, 0, 1.0]], [[0, 0, -0.5]], ring]).astype(np.float32)
    i, j = 2 + np.arange(n), 2 + (np.arange(n) + 1) % n
    top = np.stack([np.zeros(n, np.int64), i, j], 1)
    bottom = np.stack([np.ones(n, np.int64), j, i], 1)
    return P, np.concatenate([top, bottom]).astype(np.int32)


def strip_with_valence_two():
    """Two quads that share TWO consecutive edges (a - m - b): the middle vertex m is interior with valence 2."""
    P = np.array([[0, 0, 0], [1, 0.25, 0.5], [2, 0, 0], [1, 1, 0], [1, -1, 0.25]], np.float32)
    return P, np.array([[0, 1, 2, 3], [2, 1, 0, 4]], np.int32)


def wound_pair(opposite):
    """Two quads sharing an edge; opposite=True winds the second one the other way round."""
    P = np.array([[0, 0, 0], [1, 0, 0.25], [1, 1, 0], [0, 1, 0.5], [2, 0, 0.125], [2, 1, 0.75]], np.float32)
    second = [1, 2, 5, 4] if opposite else [1, 4, 5, 2]
    return P, np.array([[0, 1, 2, 3], second], np.int32)


def quad_torus(n=6, m=5):
    """A torus of n x m quads: closed, every vertex of valence 4, Euler characteristic 0."""
    a, b = 2 * np.pi * np.arange(n) / n, 2 * np.pi * np.arange(m) / m
    A, B = np.meshgrid(a, b, indexing="ij")
    P = np.stack([(2 + np.cos(B)) * np.cos(A), (2 + np.cos(B)) * np.sin(A), np.sin(B)], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    idx = lambda i, j: (i % n) * m + (j % m)   # noqa: E731
    return P, np.stack([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)], -1).reshape(-1, 4).astype(np.int32)


# --------------------------------------------------------------------------------------------------------------- measures
def euler(F):
    """V - E + F over the vertices the faces name."""
    F = np.asarray(F)
    T = Topology(F, int(F.max()) + 1)
    return len(np.unique(F)) - T.ne + T.nf


def directed_edges(F):
    """The set of directed edges (a, b) of the faces' boundaries."""
    F = np.asarray(F, np.int64)
    return set(zip(F.reshape(-1).tolist(), np.roll(F, -1, axis=1).reshape(-1).tolist()))
