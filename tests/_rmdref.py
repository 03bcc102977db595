"""A plain fp64 NumPy restatement of the host remesher's rules (sculptmate_amd/csrc/remesh_host.h), for the stage-by-stage tests
of the device remesher (tests/test_gpu_remesh_kernels.py) -- test infrastructure, written for reading, not for speed.

The device holds fp32 positions; every predicate here is evaluated in fp64 from those fp32 values, the way the kernels do.  A
position the device writes is an fp64 value rounded once to fp32 (a midpoint, a relaxed or projected point), so the restatement
rounds at the same places.

Sign tests near zero.  Where a rule compares a dot product with zero (fold-over, crease, flip fold) or two lengths with each
other (`low`, `high`, the split diagonal), two correct fp64 evaluations may disagree when the value lies within rounding of the
threshold (a fused multiply-add in one of them is enough).  Each such test reports "ambiguous" when the value lies within

    MARGIN (1e-9) x the scale of its terms     (products of the side lengths that enter the cross products, or the lengths)

of the threshold.  The tests accept either outcome for an ambiguous candidate, and assert that the regular meshes have none, so
that the bit-exact comparisons there are comparisons of rules, not of rounding.

Vertices with more than MAX_NEIGHBOURS (64) distinct neighbours are features on both paths: Mesh::scan_boundary_vertex flags them
as boundary, and so does the device's boundary pass.
"""
import numpy as np

NO_CLAIM = 0xFFFFFFFFFFFFFFFF
MAX_NEIGHBOURS = 64
MARGIN = 1e-9
LEN_MARGIN = 1e-12


def f64(P):
    """fp32 positions as the kernels read them."""
    return np.asarray(P, np.float32).astype(np.float64)


def norm(a):
    return float(np.sqrt(np.dot(a, a)))


def f32_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


# ---------------------------------------------------------------------------------------------------------------- topology
def topo(F, nv):
    """The device topology of faces F (int [nf, 3]) over nv vertices (csrc/remesh_device.hip header), restated with np.unique:
    dict of keys, skeys, sperm, she, fe, es (es[ne] = 3 nf), ne, vfc, vfs, and the flags of a first pass over an input: bnd =
    edge_bnd (an edge with other than two faces) | high_valence (more than 64 distinct neighbours)."""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    nf = len(F)
    a = F.reshape(-1)
    b = F[:, [1, 2, 0]].reshape(-1)
    keys = (np.minimum(a, b) << 32) | np.maximum(a, b)
    sperm = np.argsort(keys, kind="stable")
    skeys = keys[sperm]
    uk, first, inv = np.unique(skeys, return_index=True, return_inverse=True)
    ne = len(uk)
    es = np.concatenate([first, [3 * nf]]).astype(np.int64)
    fe = np.empty(3 * nf, np.int64)
    fe[sperm] = inv.reshape(-1)
    order = np.argsort(a, kind="stable")
    vfs = np.searchsorted(a[order], np.arange(nv + 1))
    cnt = np.diff(es)
    edge_bnd = np.zeros(max(nv, 1), np.uint8)
    odd = uk[cnt != 2]
    edge_bnd[(odd >> 32).astype(np.int64)] = 1
    edge_bnd[(odd & 0xFFFFFFFF).astype(np.int64)] = 1
    high = np.zeros(max(nv, 1), np.uint8)
    for u in range(nv):
        high[u] = len(set(F[order[vfs[u]:vfs[u + 1]] // 3].reshape(-1)) - {u}) > MAX_NEIGHBOURS
    return dict(keys=keys, skeys=skeys, sperm=sperm, she=sperm, fe=fe, es=es, ne=ne, vfc=order, vfs=vfs, bnd=edge_bnd | high,
                edge_bnd=edge_bnd, high_valence=high, F=F, nf=nf, nv=nv)


def edge_ends(T, e):
    k = int(T["skeys"][T["es"][e]])
    return k >> 32, k & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------- mesh
class Mesh:
    """remesh_host.h Mesh on fp32 positions: faces with tombstones, incident-face lists (ascending face id for a freshly built
    mesh), boundary flags as Mesh::build computes them (plus the high-valence rule) and then keeps them through collapses."""

    def __init__(self, P, F, bnd=None):
        self.P = np.array(P, np.float32).reshape(-1, 3)
        self.Pd = self.P.astype(np.float64)
        self.F = np.array(F, np.int64).reshape(-1, 3).tolist()
        self.alive = np.ones(len(self.F), bool)
        self.vf = [[] for _ in range(len(self.P))]
        for f, t in enumerate(self.F):
            for x in t:
                self.vf[x].append(f)
        self._nb = {}
        self.bnd = np.array([self.scan_boundary_vertex(u) for u in range(len(self.P))], bool) if bnd is None else np.array(bnd, bool)

    def p(self, i):
        return self.Pd[i]

    def has(self, f, x):
        return x in self.F[f]

    def edge_faces(self, u, v):
        return [f for f in self.vf[u] if self.has(f, v)]

    def third(self, f, u, v):
        return next(int(x) for x in self.F[f] if x != u and x != v)

    def directed(self, f, u, v):
        t = self.F[f]
        return u in t and t[(t.index(u) + 1) % 3] == v

    def neighbours(self, u):
        if u not in self._nb:
            out = []
            for f in self.vf[u]:
                for w in self.F[f]:
                    if w != u and w not in out:
                        out.append(w)
            self._nb[u] = out
        return self._nb[u]

    def scan_boundary_vertex(self, u):
        nb = {}
        for f in self.vf[u]:
            for w in self.F[f]:
                if w != u:
                    nb[w] = nb.get(w, 0) + 1
        if len(nb) > MAX_NEIGHBOURS:
            return True  # absurd valence: a feature
        return any(c != 2 for c in nb.values()) or not nb

    def normal(self, f):
        a, b, c = (self.p(x) for x in self.F[f])
        return np.cross(b - a, c - a)

    # ---- remesh_host.h Mesh::can_collapse
    def can_collapse(self, u, v):
        ef = self.edge_faces(u, v)
        nef = len(ef)
        if nef not in (1, 2):
            return False
        nu, nv = self.neighbours(u), self.neighbours(v)
        if sum(1 for w in nu if w in nv) != nef:
            return False
        if nef == 2 and self.bnd[u] and self.bnd[v]:
            return False
        if nef == 2:
            a, b = self.third(ef[0], u, v), self.third(ef[1], u, v)
            at_u = at_v = False
            for f in self.vf[a]:
                if self.has(f, b):
                    at_u = at_u or self.has(f, u)
                    at_v = at_v or self.has(f, v)
            return not (at_u and at_v)
        a = self.third(ef[0], u, v)
        return not (len(self.edge_faces(u, a)) == 1 and len(self.edge_faces(v, a)) == 1)

    def collapse(self, u, v, p):
        """remesh_host.h Mesh::collapse: remove u, keep v at p (fp32)."""
        self._nb = {}
        for f in self.edge_faces(u, v)[:2]:
            for x in self.F[f]:
                self.vf[x].remove(f)
            self.alive[f] = False
        for f in self.vf[u]:
            self.F[f][self.F[f].index(u)] = v
            self.vf[v].append(f)
        self.vf[u] = []
        self.bnd[v] = self.bnd[v] or self.bnd[u]
        self.P[v] = p
        self.Pd[v] = self.P[v].astype(np.float64)

    def flip(self, u, v):
        """remesh_host.h Mesh::flip."""
        ef = self.edge_faces(u, v)
        if len(ef) != 2:
            return False
        f1, f2 = ef
        if not self.directed(f1, u, v):
            f1, f2 = f2, f1
        if not self.directed(f1, u, v) or not self.directed(f2, v, u):
            return False
        a, b = self.third(f1, u, v), self.third(f2, u, v)
        if a == b or self.edge_faces(a, b):
            return False
        self._nb = {}
        self.F[f1] = [u, b, a]
        self.F[f2] = [b, v, a]
        self.vf[v].remove(f1)
        self.vf[u].remove(f2)
        self.vf[b].append(f1)
        self.vf[a].append(f2)
        return True

    def faces(self):
        return np.array(self.F, np.int64).reshape(-1, 3)[self.alive]


def _side_scale(q):
    a, b, c = q
    return norm(b - a) * norm(c - a)


def turns_over(before, after):
    """dot(n_before, n_after) <= 0 for two triangles (3 x 3 fp64 corners each) -> (verdict, ambiguous)."""
    d = float(np.dot(np.cross(before[1] - before[0], before[2] - before[0]), np.cross(after[1] - after[0], after[2] - after[0])))
    return d <= 0, abs(d) <= MARGIN * _side_scale(before) * _side_scale(after)


def midpoint32(M, u, v):
    return (0.5 * (M.p(u) + M.p(v))).astype(np.float32)


# -------------------------------------------------------------------------------------------------------------- collapse
def collapse_rule(M, a, b, mode, low=0.0, high=0.0):
    """The host rule for edge (a < b): decimate() (mode 0) or collapse_short_edges() (mode 1).  Returns
    (ok, u, v, p32, ambiguous): u is removed, v stays at p32."""
    ef = M.edge_faces(a, b)
    if len(ef) not in (1, 2):
        return False, a, b, None, False
    amb = False
    u, v = a, b
    if mode == 1:
        ln = norm(M.p(a) - M.p(b))
        amb = abs(ln - low) <= LEN_MARGIN * low
        if not ln < low:
            return False, u, v, None, amb
        if M.bnd[u] and M.bnd[v]:
            return False, u, v, None, amb
        if M.bnd[u]:
            u, v = v, u
        p = M.P[v].copy() if M.bnd[v] else midpoint32(M, u, v)
    else:
        p = midpoint32(M, u, v)
    if not M.can_collapse(u, v):
        return False, u, v, p, amb
    if mode == 1:
        pd = p.astype(np.float64)
        ok = True
        for x, other in ((u, v), (v, u)):
            for w in M.neighbours(x):
                if w != other:
                    d = norm(M.p(w) - pd)
                    amb = amb or abs(d - high) <= LEN_MARGIN * high
                    ok = ok and not d > high
            for f in M.vf[x]:
                if M.has(f, other):
                    continue
                before = np.array([M.p(y) for y in M.F[f]])
                after = np.array([pd if y == x else M.p(y) for y in M.F[f]])
                t, am = turns_over(before, after)
                amb = amb or am
                ok = ok and not t
        if not ok:
            return False, u, v, p, amb
    return True, u, v, p, amb


def collapse_key(M, u, v, e):
    ln = norm(M.p(u) - M.p(v))
    return (f32_bits(ln) << 32) | e


def collapse_footprint(M, u, v):
    return {int(w) for x in (u, v) for f in M.vf[x] for w in M.F[f]}


def collapse_proposals(P, F, mode, low=0.0, high=0.0):
    """cand[e] (NO_CLAIM or key), the footprints, the removed-face counts and the ambiguity of every edge of the device topology."""
    T = topo(F, len(P))
    M = Mesh(P, F, bnd=T["bnd"][:len(P)].astype(bool))
    cand, fp, nef, amb = [], [], [], []
    for e in range(T["ne"]):
        a, b = edge_ends(T, e)
        ok, u, v, _, am = collapse_rule(M, a, b, mode, low, high)
        cand.append(collapse_key(M, u, v, e) if ok else NO_CLAIM)
        fp.append(collapse_footprint(M, u, v))
        nef.append(int(T["es"][e + 1] - T["es"][e]))
        amb.append(am)
    return T, M, cand, fp, nef, amb


def claims(nv, cand, fp):
    claim = [NO_CLAIM] * max(nv, 1)
    for key, s in zip(cand, fp):
        if key != NO_CLAIM:
            for x in s:
                claim[x] = min(claim[x], key)
    return claim


def winners(claim, cand, fp, weight):
    return [w if key != NO_CLAIM and all(claim[x] == key for x in s) else 0 for key, s, w in zip(cand, fp, weight)]


# ------------------------------------------------------------------------------------------------------------------ flip
def flip_rule(M, u, v):
    """remesh_host.h equalize_valences() for edge (u < v) -> (gain or None, (u, v, a, b), ambiguous)."""
    ef = M.edge_faces(u, v)
    if len(ef) != 2:
        return None, None, False
    f1, f2 = ef
    if not M.directed(f1, u, v):
        f1, f2 = f2, f1
    if not M.directed(f1, u, v) or not M.directed(f2, v, u):
        return None, None, False
    a, b = M.third(f1, u, v), M.third(f2, u, v)
    if a == b or M.edge_faces(a, b):
        return None, None, False
    val = lambda x: len(M.vf[x]) + (1 if M.bnd[x] else 0)  # noqa: E731
    tgt = lambda x: 4 if M.bnd[x] else 6  # noqa: E731
    before = (val(u) - tgt(u)) ** 2 + (val(v) - tgt(v)) ** 2 + (val(a) - tgt(a)) ** 2 + (val(b) - tgt(b)) ** 2
    after = (val(u) - 1 - tgt(u)) ** 2 + (val(v) - 1 - tgt(v)) ** 2 + (val(a) + 1 - tgt(a)) ** 2 + (val(b) + 1 - tgt(b)) ** 2
    if after >= before:
        return None, None, False
    q1 = np.array([M.p(x) for x in M.F[f1]])
    q2 = np.array([M.p(x) for x in M.F[f2]])
    n1, n2 = M.normal(f1), M.normal(f2)
    l1, l2 = norm(n1), norm(n2)
    s1, s2 = _side_scale(q1), _side_scale(q2)
    if l1 == 0 or l2 == 0:
        return None, None, False
    c = float(np.dot(n1, n2)) - 0.5 * l1 * l2
    amb = abs(c) <= MARGIN * s1 * s2
    if c < 0:
        return None, None, amb
    pu, pv, pa, pb = M.p(u), M.p(v), M.p(a), M.p(b)
    m1, m2 = np.cross(pb - pu, pa - pu), np.cross(pv - pb, pa - pb)
    avg = (1.0 / l1) * n1 + (1.0 / l2) * n2
    w = s1 / l1 + s2 / l2
    d1, d2 = float(np.dot(m1, avg)), float(np.dot(m2, avg))
    amb = amb or abs(d1) <= MARGIN * norm(pb - pu) * norm(pa - pu) * w or abs(d2) <= MARGIN * norm(pv - pb) * norm(pa - pb) * w
    if d1 <= 0 or d2 <= 0:
        return None, None, amb
    return before - after, (u, v, a, b), amb


def flip_proposals(P, F):
    T = topo(F, len(P))
    M = Mesh(P, F, bnd=T["bnd"][:len(P)].astype(bool))
    cand, fp, amb = [], [], []
    for e in range(T["ne"]):
        u, v = edge_ends(T, e)
        gain, quad, am = flip_rule(M, u, v)
        cand.append(((1024 - min(gain, 1023)) << 32 | e) if gain is not None else NO_CLAIM)
        fp.append(set(quad) if quad else set())
        amb.append(am)
    return T, M, cand, fp, amb


# ----------------------------------------------------------------------------------------------------------------- split
def split_reference(P, F, high):
    """Mark edges longer than `high` (one or two faces), the new vertex of marked edge e at nv + (marked edges up to e) - 1 (the
    fp32 midpoint), and the children of every face by the templates of the include/sculpt_hip.h block: one marked edge -> two
    faces, two -> the corner triangle and the quad split along its shorter diagonal, three -> four.  Returns (T, mark, cnt,
    new_rows, Fo, ambiguous faces)."""
    T = topo(F, len(P))
    Pd = f64(P)
    nv = len(P)
    mark = np.zeros(T["ne"], np.int64)
    amb_e = np.zeros(T["ne"], bool)
    for e in range(T["ne"]):
        u, v = edge_ends(T, e)
        nef = T["es"][e + 1] - T["es"][e]
        ln = norm(Pd[u] - Pd[v])
        amb_e[e] = abs(ln - high) <= LEN_MARGIN * high
        mark[e] = nef in (1, 2) and ln > high
    incl = np.cumsum(mark)
    mid = {}
    rows = np.zeros((int(mark.sum()), 3), np.float32)
    for e in np.nonzero(mark)[0]:
        u, v = edge_ends(T, e)
        rows[incl[e] - 1] = (0.5 * (Pd[u] + Pd[v])).astype(np.float32)
        mid[e] = nv + incl[e] - 1
    allP = np.concatenate([Pd, rows.astype(np.float64)]) if len(rows) else Pd
    out, cnt, amb_f = [], [], []
    for f in range(T["nf"]):
        c = [int(x) for x in T["F"][f]]
        es_ = [int(T["fe"][3 * f + k]) for k in range(3)]
        mk = [int(mark[e]) for e in es_]
        M = [mid.get(e, -1) for e in es_]
        n = sum(mk)
        am = False
        if n == 0:
            t = [(c[0], c[1], c[2])]
        elif n == 1:
            k = mk.index(1)
            t = [(c[k], M[k], c[(k + 2) % 3]), (M[k], c[(k + 1) % 3], c[(k + 2) % 3])]
        elif n == 2:
            k = mk.index(0)
            k1, k2 = (k + 1) % 3, (k + 2) % 3
            d1, d2 = norm(allP[M[k1]] - Pd[c[k]]), norm(allP[M[k2]] - Pd[c[k1]])
            am = abs(d1 - d2) <= LEN_MARGIN * max(d1, d2)
            t = [(M[k1], c[k2], M[k2])]
            t += [(c[k], c[k1], M[k1]), (c[k], M[k1], M[k2])] if d1 <= d2 else [(c[k], c[k1], M[k2]), (c[k1], M[k1], M[k2])]
        else:
            t = [(c[0], M[0], M[2]), (c[1], M[1], M[0]), (c[2], M[2], M[1]), (M[0], M[1], M[2])]
        cnt.append(len(t))
        out += t
        amb_f += [am or any(amb_e[e] for e in es_)] * len(t)
    return T, mark, np.array(cnt, np.int64), rows, np.array(out, np.int64).reshape(-1, 3), np.array(amb_f, bool), amb_e


# ------------------------------------------------------------------------------------------------------------------- grid
def grid_params(GP, GF):
    """remesh_host.h SurfaceGrid::build: (lo[3], cell, n[3])."""
    pts = f64(GP)[np.asarray(GF, np.int64).reshape(-1)]
    lo, hi = pts.min(0), pts.max(0)
    ext = hi - lo
    longest = float(ext.max())
    nf = len(GF)
    per_side = max(1.0, min(np.sqrt(nf / 2.0), (4.0 * nf) ** (1.0 / 3.0)))
    cell = longest / per_side if longest > 0 else 1.0
    n = [max(1, min(1024, int(np.floor(e / cell)) + 1)) for e in ext]
    return lo, cell, n


def grid_cells(GP, GF, lo, cell, n):
    """(cell, face) pairs, face-major, z / y / x inside a face (the grid_fill order), and the CSR after a stable sort by cell."""
    Pd = f64(GP)
    GF = np.asarray(GF, np.int64).reshape(-1, 3)
    pairs, cnt = [], []
    for f, t in enumerate(GF):
        q = Pd[t]
        a = [max(0, min(n[k] - 1, int(np.floor((q[:, k].min() - lo[k]) / cell)))) for k in range(3)]
        b = [max(0, min(n[k] - 1, int(np.floor((q[:, k].max() - lo[k]) / cell)))) for k in range(3)]
        cnt.append((b[0] - a[0] + 1) * (b[1] - a[1] + 1) * (b[2] - a[2] + 1))
        for z in range(a[2], b[2] + 1):
            for y in range(a[1], b[1] + 1):
                for x in range(a[0], b[0] + 1):
                    pairs.append(((z * n[1] + y) * n[0] + x, f))
    pairs = np.array(pairs, np.int64).reshape(-1, 2)
    order = np.argsort(pairs[:, 0], kind="stable")
    items = pairs[order, 1]
    start = np.searchsorted(pairs[order, 0], np.arange(n[0] * n[1] * n[2] + 1))
    return np.array(cnt, np.int64), pairs, items, start


def closest_on_triangles(p, A, B, C):
    """Ericson, Real-Time Collision Detection 5.1.5 (remesh_host.h closest_on_triangle), for one point p against arrays of
    triangles A, B, C [m, 3]; the first branch that applies wins, as in the scalar code."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ab, ac, ap = B - A, C - A, p - A
        d1, d2 = (ab * ap).sum(1), (ac * ap).sum(1)
        bp = p - B
        d3, d4 = (ab * bp).sum(1), (ac * bp).sum(1)
        vc = d1 * d4 - d3 * d2
        cp = p - C
        d5, d6 = (ab * cp).sum(1), (ac * cp).sum(1)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        den = 1.0 / (va + vb + vc)
        out = A + (vb * den)[:, None] * ab + (vc * den)[:, None] * ac
        cases = [((d1 <= 0) & (d2 <= 0), A),
                 ((d3 >= 0) & (d4 <= d3), B),
                 ((vc <= 0) & (d1 >= 0) & (d3 <= 0), A + (d1 / (d1 - d3))[:, None] * ab),
                 ((d6 >= 0) & (d5 <= d6), C),
                 ((vb <= 0) & (d2 >= 0) & (d6 <= 0), A + (d2 / (d2 - d6))[:, None] * ac),
                 ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), B + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (C - B))]
        for cond, val in reversed(cases):
            out = np.where(cond[:, None], val, out)
    return out


def closest_point(p, GP, GF):
    """Brute force over every face: (point, squared distance) of the first face (in face order) at the least distance."""
    Pd = f64(GP)
    GF = np.asarray(GF, np.int64).reshape(-1, 3)
    if len(GF) == 0:
        return p, 0.0
    q = closest_on_triangles(p, Pd[GF[:, 0]], Pd[GF[:, 1]], Pd[GF[:, 2]])
    d = ((q - p) ** 2).sum(1)
    i = int(np.argmin(d))
    return q[i], float(d[i])


# ------------------------------------------------------------------------------------------------------------------ relax
def relax(P, F, GP=None, GF=None, fixed_point=True):
    """remesh_host.h tangential_relaxation on fp32 positions: for every vertex that is referenced and not on the boundary, the
    centroid of its DISTINCT neighbours (in order of first appearance over its faces in face order), moved into the tangent
    plane of the area-weighted normal, kept only if no face of its 1-ring turns over, then projected (brute force closest
    point of GP / GF when given) and rounded to fp32.  Then every vertex of a face that turned over takes its move back, until
    no face turns over (fixed_point) or once.  Returns (Q fp32, relaxed-before-undo fp32, pre-projection fp64 points,
    per-vertex moved flag, undone flags, ambiguous flags)."""
    T = topo(F, len(P))
    M = Mesh(P, F, bnd=T["bnd"][:len(P)].astype(bool))
    Pd = f64(P)
    nv = len(P)
    Q = np.array(P, np.float32).reshape(-1, 3).copy()
    pre = Pd.copy()
    moved = np.zeros(nv, bool)
    amb = np.zeros(nv, bool)
    for u in range(nv):
        if not M.vf[u] or M.bnd[u]:
            continue
        nb = M.neighbours(u)
        c = np.zeros(3)
        for w in nb:
            c = c + Pd[w]
        c = (1.0 / len(nb)) * c
        N = np.zeros(3)
        for f in M.vf[u]:
            N = N + M.normal(f)
        ln = norm(N)
        if ln == 0:
            continue
        n = (1.0 / ln) * N
        p = c + float(np.dot(n, Pd[u] - c)) * n
        ok = True
        for f in M.vf[u]:
            before = Pd[M.F[f]]
            after = np.array([p if y == u else Pd[y] for y in M.F[f]])
            t, am = turns_over(before, after)
            amb[u] = amb[u] or am
            ok = ok and not t
        if not ok:
            continue
        pre[u] = p
        if GF is not None:
            p = closest_point(p, GP, GF)[0]
        Q[u] = p.astype(np.float32)
        moved[u] = True
    relaxed = Q.copy()
    undo = np.zeros(nv, bool)
    while True:
        Qd = Q.astype(np.float64)
        new = False
        for f, t in enumerate(M.F):
            nb_ = np.cross(Pd[t[1]] - Pd[t[0]], Pd[t[2]] - Pd[t[0]])
            na = np.cross(Qd[t[1]] - Qd[t[0]], Qd[t[2]] - Qd[t[0]])
            if float(np.dot(nb_, na)) <= 0:
                for x in t:
                    if not undo[x]:
                        undo[x] = new = True
        Q[undo] = np.asarray(P, np.float32).reshape(-1, 3)[undo]
        if not new or not fixed_point:
            break
    return Q, relaxed, pre, moved, undo, amb


# ------------------------------------------------------------------------------------------------------------ invariants
def boundary_loops(F):
    """Number of closed loops of boundary edges (edges with one face) of an edge-manifold mesh."""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    if len(F) == 0:
        return 0
    d = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]], 0)
    und = np.sort(d, 1)
    uk, cnt = np.unique(und, axis=0, return_counts=True)
    be = uk[cnt == 1]
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in be:
        parent[find(int(a))] = find(int(b))
    return len({find(int(x)) for x in be.reshape(-1)})


def euler(nv_used, F):
    F = np.asarray(F, np.int64).reshape(-1, 3)
    if len(F) == 0:
        return 0
    und = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]], 0), 1)
    return nv_used - len(np.unique(und, axis=0)) + len(F)


def max_edge_faces(F):
    F = np.asarray(F, np.int64).reshape(-1, 3)
    if len(F) == 0:
        return 0
    und = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]], 0), 1)
    return int(np.unique(und, axis=0, return_counts=True)[1].max())
