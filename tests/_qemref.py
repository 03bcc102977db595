"""A plain fp64 NumPy restatement of the device simplifier's rules (sculptmate_amd/csrc/mesh_simplify.hip, the rounds of
sculptmate_amd/sf3d/remesh_device.py simplify_device), in the manner of tests/_rmdref.py, whose topology, link condition and
collapse it reuses -- test infrastructure, written for reading, not for speed.

The kernels are compiled without floating-point contraction, so every value there is a sequence of IEEE fp64 operations in the
order written.  The expressions below keep that order (a * b * c is (a * b) * c, sums run left to right, NumPy's elementwise
multiply and add do not fuse), so quadrics, targets and keys are comparable bit for bit.  np.dot / np.cross / np.linalg are not
used for anything that is compared: their order of operations is not specified.

Rules (include/sculpt_hip.h, the sculpt_rmd_qem_* block):
  quadric    per vertex, over its faces in CSR order (ascending corner 3 f + k): the plane (unit normal n, d = -n . p0) of every
             face that has a normal; {aa ab ac ad bb bc bd cc cd dd}
  edge       u < v, u goes, v stays; one or two faces; bnd[u] == bnd[v]; q = Q[u] + Q[v]; target = the minimiser when neither
             end is flagged, det != 0 and the fp32 point is finite, else the best of p_u, p_v, the fp32 midpoint (ties in that
             order); cost = error at the fp32 target, clamped at 0, no candidate when it is not finite; link condition (_rmdref.Mesh.can_collapse); fold-over: every
             surviving face of both fans that has a normal keeps one, |d1 . d2| <= 0.999, new normal . old normal >= 0.2
  round      cap = the k-th smallest key, k = ceil((nf - target) / 2); candidates at or under it claim their footprint
             (sequential atomic-min emulation: _rmdref.claims / winners); in a round that would pass the target the winners are
             kept in key order while more than `target` faces are left
  apply      _rmdref.Mesh.collapse with the stored target, Q[v] += Q[u], bnd[v] |= bnd[u]

Thresholds.  A comparison against 0.999 or 0.2 reports "ambiguous" when the value lies within _rmdref.MARGIN of the threshold;
det == 0 reports it when det is not zero but within MARGIN x (the sum of the magnitudes of its six products).
"""
import functools
import math

import numpy as np

import _rmdref
from _rmdref import MARGIN, NO_CLAIM, edge_ends, topo  # noqa: F401

COLLINEAR = 0.999
MIN_NORMAL_DOT = 0.2
I64_MAX = (1 << 63) - 1


# ------------------------------------------------------------------------------------------------------- vector pieces
def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def face_unit_normals(P, F):
    """(n [nf, 3] fp64, has [nf] bool): the unit normal of every face that has one (zero or non-finite cross product: none)."""
    Pd = _rmdref.f64(P).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    a, b, c = Pd[F[:, 0]], Pd[F[:, 1]], Pd[F[:, 2]]
    with np.errstate(all="ignore"):
        cr = _cross(b - a, c - a)
        ln = np.sqrt(_dot(cr, cr))
        has = (ln > 0) & np.isfinite(ln)
        n = np.where(has[:, None], cr / np.where(has, ln, 1.0)[:, None], 0.0)
    return n, has


def quadrics(P, T):
    """Q [nv, 10] fp64: the sum over every vertex's CSR corners, in their order, of its faces' plane quadrics."""
    Pd = _rmdref.f64(P).reshape(-1, 3)
    F, nv = T["F"], T["nv"]
    n, has = face_unit_normals(P, F)
    d = -_dot(n, Pd[F[:, 0]]) if len(F) else np.zeros(0)
    K = np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 0] * d, n[:, 1] * n[:, 1], n[:, 1] * n[:, 2],
                  n[:, 1] * d, n[:, 2] * n[:, 2], n[:, 2] * d, d * d], 1) if len(F) else np.zeros((0, 10))
    Q = np.zeros((max(nv, 1), 10))
    fan = np.diff(T["vfs"])
    for j in range(int(fan.max()) if nv else 0):   # the j-th corner of every vertex that has one
        us = np.nonzero(fan > j)[0]
        f = T["vfc"][T["vfs"][us] + j] // 3
        ok = has[f]
        Q[us[ok]] = Q[us[ok]] + K[f[ok]]
    return Q


def _det3(m, a11, a12, a13, a21, a22, a23, a31, a32, a33):
    t = [m[:, a11] * m[:, a22] * m[:, a33], m[:, a13] * m[:, a21] * m[:, a32], m[:, a12] * m[:, a23] * m[:, a31],
         m[:, a13] * m[:, a22] * m[:, a31], m[:, a11] * m[:, a23] * m[:, a32], m[:, a12] * m[:, a21] * m[:, a33]]
    return t[0] + t[1] + t[2] - t[3] - t[4] - t[5], sum(np.abs(x) for x in t)


def vertex_error(q, x, y, z):
    return (q[:, 0] * x * x + 2 * q[:, 1] * x * y + 2 * q[:, 2] * x * z + 2 * q[:, 3] * x + q[:, 4] * y * y + 2 * q[:, 5] * y * z
            + 2 * q[:, 6] * y + q[:, 7] * z * z + 2 * q[:, 8] * z + q[:, 9])


def edge_costs(P, Q, T, bnd):
    """For every edge of T: (eligible [ne] -- one or two faces and equal flags --, key without the link / fold-over tests
    [ne] Python ints, target fp32 [ne, 3], branch [ne]: 0 solved, 1 p_u, 2 p_v, 3 midpoint, ambiguous det [ne])."""
    ne = T["ne"]
    P = np.asarray(P, np.float32).reshape(-1, 3)
    Pd = P.astype(np.float64)
    k = T["skeys"][T["es"][:ne]]
    u, v = (k >> 32).astype(np.int64), (k & 0xFFFFFFFF).astype(np.int64)
    nef = np.diff(T["es"])
    bu, bv = bnd[u] != 0, bnd[v] != 0
    eligible = ((nef == 1) | (nef == 2)) & (bu == bv)
    q = Q[u] + Q[v]
    with np.errstate(all="ignore"):
        det, scale = _det3(q, 0, 1, 2, 1, 4, 5, 2, 5, 7)
        x = -1 / det * _det3(q, 1, 2, 3, 4, 5, 6, 5, 7, 8)[0]
        y = 1 / det * _det3(q, 0, 2, 3, 1, 5, 6, 2, 7, 8)[0]
        z = -1 / det * _det3(q, 0, 1, 3, 1, 4, 6, 2, 5, 8)[0]
        s32 = np.stack([x, y, z], 1).astype(np.float32)
        solved = ~(bu & bv) & (det != 0) & np.isfinite(s32).all(1)
        amb = ~(bu & bv) & (det != 0) & (np.abs(det) <= MARGIN * scale)
        sd = s32.astype(np.float64)
        es = vertex_error(q, sd[:, 0], sd[:, 1], sd[:, 2])
        pm = (np.float32(0.5) * (P[u] + P[v])).astype(np.float32)
        pmd = pm.astype(np.float64)
        e1 = vertex_error(q, Pd[u, 0], Pd[u, 1], Pd[u, 2])
        e2 = vertex_error(q, Pd[v, 0], Pd[v, 1], Pd[v, 2])
        e3 = vertex_error(q, pmd[:, 0], pmd[:, 1], pmd[:, 2])
    first = (e1 <= e2) & (e1 <= e3)
    second = ~first & (e2 <= e3)
    branch = np.where(solved, 0, np.where(first, 1, np.where(second, 2, 3)))
    err = np.where(solved, es, np.where(first, e1, np.where(second, e2, e3)))
    eligible = eligible & np.isfinite(err)   # inf - inf for huge coordinates: no candidate
    tgt = np.where(solved[:, None], s32, np.where(first[:, None], P[u], np.where(second[:, None], P[v], pm))).astype(np.float32)
    with np.errstate(all="ignore"):
        cost = np.where(err > 0, err, 0.0).astype(np.float32)
    bits = cost.view(np.uint32).astype(np.uint64)
    keys = [(int(b) << 32) | e for e, b in enumerate(bits)]
    return eligible, keys, tgt, branch, amb & eligible


# ------------------------------------------------------------------------------------------------------- scalar pieces
def _unit_normal(Pl, t):
    a, b, c = Pl[t[0]], Pl[t[1]], Pl[t[2]]
    e1 = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
    e2 = (c[0] - a[0], c[1] - a[1], c[2] - a[2])
    cx, cy, cz = e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]
    ln = math.sqrt(cx * cx + cy * cy + cz * cz)
    if not ln > 0 or not math.isfinite(ln):
        return None
    return cx / ln, cy / ln, cz / ln


def fan_keeps_shape(M, Pl, x, other, p):
    """The fold-over test for the faces around x that survive the collapse of (x, other) to p -> (ok, ambiguous)."""
    ok, amb = True, False
    for f in M.vf[x]:
        t = M.F[f]
        if other in t:
            continue
        n0 = _unit_normal(Pl, t)
        if n0 is None:
            continue   # degenerate before the collapse: exempt
        k = t.index(x)
        a, b = Pl[t[(k + 1) % 3]], Pl[t[(k + 2) % 3]]
        d1 = (a[0] - p[0], a[1] - p[1], a[2] - p[2])
        d2 = (b[0] - p[0], b[1] - p[1], b[2] - p[2])
        l1 = math.sqrt(d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2])
        l2 = math.sqrt(d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2])
        if not l1 > 0 or not l2 > 0:
            ok = False
            continue
        e1 = (d1[0] / l1, d1[1] / l1, d1[2] / l1)
        e2 = (d2[0] / l2, d2[1] / l2, d2[2] / l2)
        c = abs(e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2])
        amb = amb or abs(c - COLLINEAR) <= MARGIN
        if c > COLLINEAR:
            ok = False
            continue
        cx, cy, cz = e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]
        lc = math.sqrt(cx * cx + cy * cy + cz * cz)
        if not lc > 0:
            ok = False
            continue
        d = (cx / lc) * n0[0] + (cy / lc) * n0[1] + (cz / lc) * n0[2]
        amb = amb or abs(d - MIN_NORMAL_DOT) <= MARGIN
        if d < MIN_NORMAL_DOT:
            ok = False
    return ok, amb


# -------------------------------------------------------------------------------------------------------------- rounds
class State:
    """Positions (fp32), faces, quadrics and the carried flags between rounds; vertices keep their indices."""

    def __init__(self, P, F):
        self.P = np.array(P, np.float32).reshape(-1, 3)
        self.F = np.array(F, np.int64).reshape(-1, 3)
        self.nv = len(self.P)
        self.T = topo(self.F, self.nv)
        self.bnd = self.T["bnd"].copy()   # first pass: edge flags | the high-valence feature flag
        self.Q = quadrics(self.P, self.T)

    def retopo(self, F):
        self.F = np.array(F, np.int64).reshape(-1, 3)
        self.T = topo(self.F, self.nv)
        self.bnd = self.bnd | self.T["edge_bnd"]


def proposals(S, k=None):
    """The candidates of a round on S: cand [ne] (NO_CLAIM or key), targets fp32 [ne, 3], branch, ambiguous [ne], the mesh M the
    rules were evaluated on and the cap.  k None: every edge is evaluated (cap = the largest key possible); otherwise edges are
    evaluated in key order until k candidates are found -- the cap is the k-th smallest candidate key and nothing above it
    matters to the round."""
    T = S.T
    M = _rmdref.Mesh(S.P, S.F, bnd=S.bnd[:S.nv].astype(bool))
    eligible, keys, tgt, branch, amb_det = edge_costs(S.P, S.Q, T, S.bnd)
    Pl = M.Pd.tolist()
    cand = [NO_CLAIM] * T["ne"]
    amb = [False] * T["ne"]
    order = sorted((keys[e] for e in np.nonzero(eligible)[0]))
    found, cap = 0, I64_MAX
    for key in order:
        e = key & 0xFFFFFFFF
        u, v = edge_ends(T, e)
        am = bool(amb_det[e])
        ok = M.can_collapse(u, v)
        if ok:
            p = tuple(float(c) for c in tgt[e])
            ok1, a1 = fan_keeps_shape(M, Pl, u, v, p)
            ok2, a2 = fan_keeps_shape(M, Pl, v, u, p)
            ok, am = ok1 and ok2, am or a1 or a2
        amb[e] = am
        if ok:
            cand[e] = key
            found += 1
            if k is not None and found == k:
                cap = key
                break
    tgt = np.where(np.array([c != NO_CLAIM for c in cand], bool)[:, None], tgt, np.float32(0)) if T["ne"] else tgt
    return dict(cand=cand, target=tgt, branch=branch, ambiguous=amb, M=M, cap=cap)


def cap_rank(nf, target, ne):
    return max(1, min(ne, (nf - target + 1) // 2))


def round_winners(S, pr, target=None):
    """win [ne]: faces removed by every winner (0: lost), after the trim of a round that would pass `target`."""
    T, M, cand = S.T, pr["M"], pr["cand"]
    fp, weight = [], []
    for e in range(T["ne"]):
        if cand[e] != NO_CLAIM and cand[e] <= pr["cap"]:
            u, v = edge_ends(T, e)
            fp.append(_rmdref.collapse_footprint(M, u, v))
        else:
            fp.append(set())
        weight.append(int(T["es"][e + 1] - T["es"][e]))
    live = [c if c != NO_CLAIM and c <= pr["cap"] else NO_CLAIM for c in cand]
    claim = _rmdref.claims(S.nv, live, fp)
    win = _rmdref.winners(claim, live, fp, weight)
    if target is not None and T["nf"] - sum(win) < target:
        left = T["nf"]
        for key, e in sorted((cand[e], e) for e in range(T["ne"]) if win[e]):
            if left > target:
                left -= win[e]
            else:
                win[e] = 0
    return win


def apply_round(S, pr, win):
    """The winners applied one after the other (they share no footprint vertex): S after the round, faces compacted."""
    M = pr["M"]
    for e in range(S.T["ne"]):
        if win[e]:
            u, v = edge_ends(S.T, e)
            M.collapse(u, v, pr["target"][e])
            S.Q[v] = S.Q[v] + S.Q[u]
    S.P = M.P.copy()
    S.bnd = S.bnd.copy()
    S.bnd[:S.nv] = M.bnd.astype(np.uint8)
    S.retopo(M.faces())
    return S


def simplify(P, F, target, max_rounds=100000):
    """The whole call -> (P' fp32, F' int64, vertex_index, stats): rounds until at most `target` faces are left or a round
    collapses nothing, then the referenced vertices in index order."""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    P = np.asarray(P, np.float32).reshape(-1, 3)
    stats = dict(rounds=0, collapses=0, ambiguous=0)
    if target >= len(F):
        return P, F, np.arange(len(P)), stats
    S = State(P, F)
    while S.T["nf"] > target and stats["rounds"] < max_rounds:
        stats["rounds"] += 1
        pr = proposals(S, k=cap_rank(S.T["nf"], target, S.T["ne"]))
        stats["ambiguous"] += sum(pr["ambiguous"])
        win = round_winners(S, pr, target)
        n = sum(1 for w in win if w)
        if n == 0:
            break
        stats["collapses"] += n
        apply_round(S, pr, win)
    used = np.zeros(S.nv, bool)
    used[S.F.reshape(-1)] = True
    index = np.nonzero(used)[0]
    remap = np.cumsum(used) - 1
    return S.P[index], remap[S.F], index, stats


@functools.lru_cache(maxsize=None)
def reference(name, ratio=0.1):
    """The restatement's result for cube() / patch() at floor(ratio x faces), computed once per process and shared by the tests
    that need it (read only): (P', F', vertex_index, stats)."""
    P, F = {"cube": cube, "patch": patch}[name]()
    return simplify(P, F, int(math.floor(ratio * len(F))))


# -------------------------------------------------------------------------------------------------------------- meshes
def cube(n=8):
    """The axis-aligned unit cube [0, 1]^3, every side an n x n grid of quads split into two triangles, outward orientation:
    (P fp32 [6 n^2 + 2, 3], F int32 [12 n^2, 3]); coordinates are multiples of 1 / n (dyadic for n a power of two)."""
    ids, faces = {}, []

    def vid(c):
        return ids.setdefault(c, len(ids))

    for axis in range(3):
        for side in (0, n):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            for i in range(n):
                for j in range(n):
                    def pt(di, dj):
                        c = [0, 0, 0]
                        c[axis], c[a], c[b] = side, i + di, j + dj
                        return vid(tuple(c))
                    q = [pt(0, 0), pt(1, 0), pt(1, 1), pt(0, 1)]   # counter-clockwise seen from +axis
                    if side == 0:
                        q = q[::-1]
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    P = np.zeros((len(ids), 3), np.float32)
    for c, i in ids.items():
        P[i] = np.array(c, np.float64) / n
    return P, np.array(faces, np.int32)


def patch(n=16):
    """A flat (n + 1) x (n + 1) grid in z = 0 over [0, 1]^2 with a boundary, normals +z."""
    P = np.zeros(((n + 1) ** 2, 3), np.float32)
    for i in range(n + 1):
        for j in range(n + 1):
            P[i * (n + 1) + j] = (i / n, j / n, 0)
    faces = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
            faces += [(a, b, c), (a, c, d)]
    return P, np.array(faces, np.int32)


def tetrahedron():
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    return P, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)


def two_triangles():
    P = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    return P, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def fan(n=70):
    """Fans of n faces around vertex 0 and around vertex 1, glued along their common rim (a flat bipyramid, closed): with n > 64
    both hubs have more than 64 neighbours and carry the feature flag, the rim vertices (four neighbours) do not.  The hubs
    stand 2^-6 off the rim's plane: flat enough that, without the flag, collapsing a hub into the rim passes the fold-over test."""
    P = np.zeros((n + 2, 3), np.float32)
    P[0], P[1] = (0, 0, 2.0 ** -6), (0, 0, -2.0 ** -6)
    for i in range(n):
        t = 2 * np.pi * i / n
        P[i + 2] = (np.cos(t), np.sin(t), 0)
    top = [(0, 2 + i, 2 + (i + 1) % n) for i in range(n)]
    bottom = [(1, 2 + (i + 1) % n, 2 + i) for i in range(n)]
    return P, np.array(top + bottom, np.int32)


def bipyramid_with_slivers():
    """A closed mesh with two coincident vertices and zero-area faces: a hexagonal bipyramid whose apex (0, 0, 1) was split into
    vertices 7 and 8 at the same position, three faces each, the cut closed by the two zero-area faces on the zero-length edge
    (7, 8) -- a closed mesh has two faces on every edge, so a zero-length edge brings two of them, not one."""
    P = [[0, 0, -1]] + [[np.cos(np.pi * i / 3), np.sin(np.pi * i / 3), 0] for i in range(6)] + [[0, 0, 1], [0, 0, 1]]
    F = [(7, 1, 2), (7, 2, 3), (7, 3, 4), (8, 4, 5), (8, 5, 6), (8, 6, 1), (7, 4, 8), (8, 1, 7)]
    F += [(0, 1 + (i + 1) % 6, 1 + i) for i in range(6)]
    return np.array(P, np.float32), np.array(F, np.int32)


def sphere_volume(R=32, radius=0.6):
    """r - |x| on the R^3 lattice of [-1, 1]^3: positive inside (like density - threshold); the iso-surface 0 is the sphere."""
    g = np.linspace(-1.0, 1.0, R)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    return (radius - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- properties
def edge_face_counts(F):
    F = np.asarray(F, np.int64).reshape(-1, 3)
    und = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]], 0), 1)
    return np.unique(und, axis=0, return_counts=True)


def closed_manifold(F):
    """Every edge in exactly two faces, with opposite directions (consistent orientation)."""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    if len(F) == 0:
        return False
    d = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]], 0)
    directed = set(map(tuple, d.tolist()))
    return bool((edge_face_counts(F)[1] == 2).all()) and len(directed) == len(d) and all((b, a) in directed for a, b in directed)


def euler(P, F):
    return _rmdref.euler(len(np.unique(np.asarray(F).reshape(-1))), F)


def signed_volume(P, F):
    Pd = np.asarray(P, np.float64)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    a, b, c = Pd[F[:, 0]], Pd[F[:, 1]], Pd[F[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def face_normals(P, F):
    Pd = np.asarray(P, np.float64)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    return np.cross(Pd[F[:, 1]] - Pd[F[:, 0]], Pd[F[:, 2]] - Pd[F[:, 0]])


def cube_checks(P, F):
    """The properties of a simplified unit cube (tests/test_*mesh_simplify*): closed 2-manifold, Euler characteristic 2, the
    eight corners present exactly -- bit for bit but for the sign of a zero: the minimiser is -1 / det * 0 = -0.0 there --,
    every face flat on one side with its normal along that side's outward axis -> the enclosed volume."""
    P = np.asarray(P, np.float32)
    assert closed_manifold(F) and euler(P, F) == 2
    have = {tuple(r) for r in (P + np.float32(0)).view(np.uint32).tolist()}   # -0.0 + 0.0 = +0.0; nothing else changes
    for c in np.ndindex(2, 2, 2):
        assert tuple(np.array(c, np.float32).view(np.uint32).tolist()) in have, c
    n = face_normals(P, F)
    for t, nn in zip(np.asarray(F), n):
        q = P[t].astype(np.float64)
        side = [(ax, s) for ax in range(3) for s in (0.0, 1.0) if (q[:, ax] == s).all()]
        assert len(side) == 1, (t, q)
        ax, s = side[0]
        out = np.zeros(3)
        out[ax] = 1.0 if s == 1.0 else -1.0
        assert float(nn @ out) > 0 and abs(float(nn @ out)) == np.abs(nn).sum(), (t, nn)
    return signed_volume(P, F)


def patch_checks(P, F):
    """The properties of a simplified unit patch: a disk (Euler characteristic 1, one border loop, no edge with more than two
    faces), every vertex in z = 0, every normal +z, every border vertex on the unit square's outline -> the area (at most 1)."""
    P = np.asarray(P, np.float32)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    assert len(F) and (P[:, 2] == 0).all()
    uk, cnt = edge_face_counts(F)
    assert cnt.max() <= 2 and euler(P, F) == 1 and _rmdref.boundary_loops(F) == 1
    n = face_normals(P, F)
    assert (n[:, 0] == 0).all() and (n[:, 1] == 0).all() and (n[:, 2] > 0).all()
    border = np.unique(uk[cnt == 1].reshape(-1))
    assert ((P[border, :2] == 0) | (P[border, :2] == 1)).any(1).all()
    assert ((P[:, :2] >= 0) & (P[:, :2] <= 1)).all()
    area = float(n[:, 2].sum() / 2)
    assert 0 < area <= 1
    return area


PATCH_AREA = 0.5625   # what the rules leave of the unit patch at a tenth of its faces (no border quadric: corners are cut)


def sphere_checks(P, F, centre, r, target):
    """Closed 2-manifold, Euler characteristic 2, at most `target` faces, outward orientation and a volume within the
    polyhedral deficit of the ball's -> (max radial error at the vertices, max radial error of the surface sampled at the
    vertices and the face centroids, |volume error|).
    Deficit: a flat face of area A on a sphere of radius r stands off it by at most rho^2 / (2 r), rho the face's circumradius;
    for n equilateral faces of area 4 pi r^2 / n, rho^2 = 4 A / (3 sqrt 3), so the relative volume error is at most
    3 rho^2 / (2 r^2) = 8 pi / (sqrt 3 n); a factor 2 covers faces that are not equilateral: 16 pi / (sqrt 3 n)."""
    P = np.asarray(P, np.float64)
    assert closed_manifold(F) and euler(P, F) == 2
    assert len(F) <= target
    vol = signed_volume(P - centre, F)
    ball = 4.0 / 3.0 * np.pi * r ** 3
    assert vol > 0 and abs(vol - ball) / ball <= 16 * np.pi / (np.sqrt(3) * len(F)), (vol, ball, len(F))
    rad = np.abs(np.sqrt(((P - centre) ** 2).sum(1)) - r).max()
    cen = P[np.asarray(F, np.int64)].mean(1)
    surf = max(rad, np.abs(np.sqrt(((cen - centre) ** 2).sum(1)) - r).max())
    return float(rad), float(surf), float(abs(vol - ball))
