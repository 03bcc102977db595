"""NumPy restatement of fill holes (sculptmate_amd/csrc/mesh_holes.hip; ops.mesh_border_loops, ops.mesh_fill_holes) -- test
infrastructure, written for reading, not for speed.  It shares no code with the ops: the loops are found by plain walking of
`next`, the device finds them by pointer doubling.

The rule.  Half-edge h = 3 f + k runs from start(h) = F[f][k] to end(h) = F[f][(k + 1) % 3].  It is a BORDER half-edge when its
undirected edge has exactly one half-edge.  Over the border half-edges: out(v) / in(v) count those that start / end at v; a vertex
they touch is PINCHED unless out(v) == 1 and in(v) == 1; a border half-edge is BLOCKED when its start or its end is pinched;
next(h) of an unblocked h is the one border half-edge that starts at end(h).  An unblocked half-edge lies on a pure cycle of
unblocked half-edges -- a LOOP, its LEADER the smallest h, its length n -- or its chain runs into a blocked one; every border
half-edge not on a loop is OPEN.  A loop is FILLED when n <= limit (max_edges when given) and n <= 2^22 - 1.
V' = V + one CENTROID per filled loop with n >= 4, in ascending leader order.  F' = F + the new faces in ascending order of the
half-edge that emits them: in a filled loop with n >= 4 every h = (a -> b) emits (b, a, centroid); in a filled loop with n == 3
the leader alone emits (b, a, end(next(h))).  The centroid, per coordinate over the n starts, is csrc/fixsum.h's sum: the largest
|x| gives e = its frexp exponent, every term is rounded once onto the grid 2^(e - 40) and added as an integer, and the value is
(float)(ldexp((double)acc, e - 40) / (double)n).  A per-vertex attribute gets the same mean; a non-finite term gives NaN."""
import os

import numpy as np

import _reportref as R

FX_BITS = 40
MAX_LOOP = 2 ** 22 - 1
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
GOLDEN_NAMES = ("gyroid", "ints", "noise_a", "noise_b", "slab", "tiny")


# ------------------------------------------------------------------------------------------------------------------ the rule
def _ends(F, h):
    f, k = divmod(h, 3)
    return int(F[f, k]), int(F[f, (k + 1) % 3])


def border_loops(faces):
    """dict: half_edges (ascending), labels (leader or -1), leaders, lengths (ascending leader order) as int64 arrays, and the
    counts border_half_edges, loops, open_half_edges, pinched_vertices; plus `next` {h: next(h)} of the unblocked half-edges."""
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    users = {}
    for h in range(3 * len(F)):
        a, b = _ends(F, h)
        users.setdefault((min(a, b), max(a, b)), []).append(h)
    border = sorted(hs[0] for hs in users.values() if len(hs) == 1)
    out, inn, starts = {}, {}, {}
    for h in border:
        a, b = _ends(F, h)
        out[a] = out.get(a, 0) + 1
        inn[b] = inn.get(b, 0) + 1
        starts.setdefault(a, []).append(h)
    touched = set(out) | set(inn)
    pinched = {v for v in touched if not (out.get(v, 0) == 1 and inn.get(v, 0) == 1)}
    blocked = {h for h in border if _ends(F, h)[0] in pinched or _ends(F, h)[1] in pinched}
    nxt = {h: starts[_ends(F, h)[1]][0] for h in border if h not in blocked}
    label = {h: -1 for h in blocked}
    for h in border:
        if h in label:
            continue
        path, cur, status = [], h, None
        while status is None:
            if cur in label:                      # a blocked half-edge, or a chain already known to reach one
                status = label[cur]
            else:
                path.append(cur)
                cur = nxt[cur]
                if cur == h:
                    status = min(path)
        for g in path:
            label[g] = status
    labels = np.array([label[h] for h in border], np.int64)
    leaders = np.array(sorted({x for x in labels.tolist() if x >= 0}), np.int64)
    lengths = np.array([int((labels == x).sum()) for x in leaders], np.int64)
    return dict(half_edges=np.array(border, np.int64), labels=labels, leaders=leaders, lengths=lengths, next=nxt,
                border_half_edges=len(border), loops=len(leaders), open_half_edges=int((labels < 0).sum()),
                pinched_vertices=len(pinched))


def fixed_point_mean(terms):
    """The mean of the rows of terms f32 [n, K], per column, by the three steps of csrc/fixsum.h and its fx_mean."""
    x = np.asarray(terms, np.float32)
    n = len(x)
    mag = (np.ascontiguousarray(x).view(np.uint32) & np.uint32(0x7FFFFFFF)).max(0)
    nonfinite = mag >= np.uint32(0x7F800000)
    e = np.frexp(np.where(nonfinite, np.uint32(0), mag).astype(np.uint32).view(np.float32))[1].astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(np.ldexp(np.where(np.isfinite(x), x, np.float32(0)).astype(np.float64), (FX_BITS - e)[None, :])).astype(np.int64)
        acc = q.sum(0, dtype=np.int64)
        out = (np.ldexp(acc.astype(np.float64), e - FX_BITS) / np.float64(n)).astype(np.float32)
    return np.where(nonfinite, np.float32(np.nan), np.where(mag != 0, out, np.float32(0.0))).astype(np.float32)


def limit_of(fill_holes):
    return MAX_LOOP if fill_holes is True else min(int(fill_holes), MAX_LOOP)


def fill_holes(vertices, faces, fill_holes=True, attributes=None):
    """(V' f32, F' int64, A' f32 or None, info) of ops.mesh_fill_holes."""
    V = np.asarray(vertices).astype(np.float32).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    A = None if attributes is None else np.asarray(attributes).astype(np.float32)
    L = border_loops(F)
    limit = limit_of(fill_holes)
    length = dict(zip(L["leaders"].tolist(), L["lengths"].tolist()))
    filled = [x for x in L["leaders"].tolist() if length[x] <= limit]
    centroid, new_v, new_a = {}, [], []
    for x in filled:                               # ascending leader order
        if length[x] >= 4:
            members = L["half_edges"][L["labels"] == x]
            rows = np.array([_ends(F, int(h))[0] for h in members], np.int64)
            centroid[x] = len(V) + len(new_v)
            new_v.append(fixed_point_mean(V[rows]))
            if A is not None:
                new_a.append(fixed_point_mean(A[rows]))
    new_f = []
    for h, x in zip(L["half_edges"].tolist(), L["labels"].tolist()):   # ascending half-edge order
        if x < 0 or length[x] > limit:
            continue
        a, b = _ends(F, h)
        if length[x] >= 4:
            new_f.append((b, a, centroid[x]))
        elif h == x:
            new_f.append((b, a, _ends(F, L["next"][h])[1]))
    info = {k: L[k] for k in ("border_half_edges", "loops", "open_half_edges", "pinched_vertices")}
    info.update(filled_loops=len(filled), filled_edges=sum(length[x] for x in filled), skipped_loops=L["loops"] - len(filled),
                new_vertices=len(new_v), new_faces=len(new_f))
    Vo = np.concatenate([V, np.array(new_v, np.float32).reshape(-1, 3)])
    Fo = np.concatenate([F, np.array(new_f, np.int64).reshape(-1, 3)])
    Ao = None if A is None else np.concatenate([A, np.array(new_a, np.float32).reshape(-1, A.shape[1])])
    return Vo, Fo, Ao, info


def skipped_edges(faces, fill_holes):
    """The edges of the loops that `fill_holes` leaves alone."""
    L = border_loops(faces)
    return int(L["lengths"][L["lengths"] > limit_of(fill_holes)].sum())


# ------------------------------------------------------------------------------------------------------------------ meshes
def golden(name):
    z = np.load(os.path.join(GOLDEN, "mc_skimage.npz"))
    return z[name + "_verts"].astype(np.float32), z[name + "_faces"].astype(np.int64)


def lidless(side=4.0, offset=(0.0, 0.0, 0.0)):
    """The cube without the two faces of its x = 0 side: one loop of 4."""
    v, f = R.cube(side, offset)
    return v, f[2:]


def rim_fan(n=5000):
    """A disc of n triangles round a centre vertex: one loop of n edges."""
    t = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0.0, 0.0, 0.25]], np.stack([np.cos(t), np.sin(t), 0 * t], 1)]).astype(np.float32)
    i = np.arange(n)
    return v, np.stack([0 * i, 1 + i, 1 + (i + 1) % n], 1).astype(np.int64)


def bow_tie():
    """Two lidless cubes whose openings share one corner: both rims are open, nothing is filled."""
    v, f = R.join(lidless(4.0), lidless(4.0, (0, 4, 4)))
    f = f.copy()
    f[f == 8] = 3                                 # the second cube's (0, 4, 4) is the first's corner 3
    return v, f


def flipped_beside_hole():
    """A lidless cube with one face at the rim wound the other way: its rim edge runs against the others."""
    v, f = lidless(4.0)
    f = f.copy()
    k = next(i for i, t in enumerate(f.tolist()) if 0 in t and 1 in t)
    f[k] = f[k][::-1]
    return v, f


def punched_grid(n=33):
    """An n x n lattice of vertices, two triangles a quad, without the quads (i, j) with i % 3 == 1 and j % 3 == 1: the 4-loops
    do not touch each other or the rim."""
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    keep = ~((i % 3 == 1) & (j % 3 == 1))
    i, j = i[keep], j[keep]
    a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
    x, y = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([x, y, 0.125 * ((x * 7 + y * 3) % 5)], -1).reshape(-1, 3).astype(np.float32)
    return v, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int64)


def triangle():
    return np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.int64([[0, 1, 2]])
