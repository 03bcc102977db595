"""Surface nets, restated in NumPy operation for operation (the rule of include/sculpt_hip.h, sculpt_surface_nets_*): what
csrc/surface_nets.hip must give bit for bit.  Two forms: `surface_nets` (vectorised fp64) and `surface_nets_loops` (one cell
and one edge at a time in Python floats, for cross-checking at tiny sizes).  Both return a dict:
    lattice  f32 [Nv, 3]  the lattice-unit positions            verts  f32 [Nv, 3]  their affine map (what the kernel returns)
    quads    [Nq, 4]      faces  [2 Nq, 3]                       (index_dtype, int32 by default)
An empty result (no active cell) is returned as it is (Nv = 0); raising is the business of ops.surface_nets."""
import itertools

import numpy as np


def level_float(level):
    """The largest float32 <= level: f32 value > double level  <=>  value > level_float(level)."""
    with np.errstate(over="ignore"):
        lf = np.float32(level)
    if float(lf) > float(level):
        lf = np.nextafter(lf, np.float32(-np.inf))
    return lf


def inside_of(vol, level):
    with np.errstate(invalid="ignore"):
        return np.asarray(vol, np.float32) > level_float(level)   # a NaN is outside


def sign_planes(vol, level=0.0):
    """int32 [n0 * n1][ceil(n2 / 32)]: bit i2 % 32 of word i2 / 32 of row i0 * n1 + i1 = inside, bits past n2 zero."""
    ins = inside_of(vol, level)
    n0, n1, n2 = ins.shape
    W = (n2 + 31) // 32
    bits = np.zeros((n0 * n1, W * 32), np.uint64)
    bits[:, :n2] = ins.reshape(n0 * n1, n2)
    words = (bits.reshape(n0 * n1, W, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2)
    return words.astype(np.uint32).view(np.int32)


# the 12 edges of a cell in the rule's order: (axis, low corner offset)
def cell_edges():
    out = []
    for axis in range(3):
        others = [c for c in range(3) if c != axis]   # the lower axis first
        for a, b in itertools.product((0, 1), (0, 1)):
            lo = [0, 0, 0]
            lo[others[0]], lo[others[1]] = a, b
            out.append((axis, tuple(lo)))
    return out


def affine(lattice, vert_div, vert_mul, vert_add):
    """marching cubes' map in fp32, one rounding per operation: (p / div) * mul + add."""
    o = np.asarray(lattice, np.float32) / np.float32(vert_div)
    o = o * np.float32(vert_mul)
    return o + np.float32(vert_add)


def _split(lattice, quads):
    """faces[2q], faces[2q + 1] of quad q: along the shorter diagonal, from the fp32 lattice-unit positions in fp64."""
    P = lattice.astype(np.float64)

    def d2(a, b):
        d = P[a] - P[b]
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]

    q0, q1, q2, q3 = (quads[:, k] for k in range(4))
    flip = d2(q1, q3) < d2(q0, q2)
    first = np.where(flip[:, None], np.stack([q0, q1, q3], 1), np.stack([q0, q1, q2], 1))
    second = np.where(flip[:, None], np.stack([q1, q2, q3], 1), np.stack([q0, q2, q3], 1))
    return np.stack([first, second], 1).reshape(-1, 3).astype(quads.dtype)


def surface_nets(vol, level=0.0, vert_div=1.0, vert_mul=1.0, vert_add=0.0, index_dtype=np.int32):
    vol = np.asarray(vol, np.float32)
    n = vol.shape
    assert vol.ndim == 3 and min(n) >= 2
    level = float(level)
    ins = inside_of(vol, level)
    c = tuple(k - 1 for k in n)

    def corner(x, lo):
        return x[lo[0]:lo[0] + c[0], lo[1]:lo[1] + c[1], lo[2]:lo[2] + c[2]]

    corners = [corner(ins, lo) for lo in itertools.product((0, 1), repeat=3)]
    active = np.logical_or.reduce(corners) & ~np.logical_and.reduce(corners)
    vid = np.full(c, -1, np.int64)
    vid[active] = np.arange(int(active.sum()))

    v64 = vol.astype(np.float64)
    s = [np.zeros(c, np.float64) for _ in range(3)]
    cnt = np.zeros(c, np.float64)
    for axis, lo in cell_edges():
        hi = tuple(lo[k] + (k == axis) for k in range(3))
        a, b = corner(v64, lo), corner(v64, hi)
        cross = corner(ins, lo) != corner(ins, hi)
        with np.errstate(all="ignore"):
            t = (level - a) / (b - a)
        t = np.where(np.isfinite(t), t, 0.5)
        for k in range(3):
            term = float(lo[k]) + (t if k == axis else 0.0)
            s[k] = np.where(cross, s[k] + term, s[k])
        cnt = np.where(cross, cnt + 1.0, cnt)
    idx = np.nonzero(active)
    lattice = np.stack([idx[k].astype(np.float64) + s[k][idx] / cnt[idx] for k in range(3)], 1).astype(np.float32)
    lattice = lattice.reshape(-1, 3)

    keys, rows = [], []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[a], hi[a] = slice(0, n[a] - 1), slice(1, n[a])
        elig = np.zeros(n, bool)
        elig[tuple(lo)] = ins[tuple(lo)] != ins[tuple(hi)]
        keep = np.zeros(n, bool)
        box = [slice(None)] * 3
        box[u], box[v] = slice(1, n[u] - 1), slice(1, n[v] - 1)
        keep[tuple(box)] = True
        p = np.argwhere(elig & keep)
        if not len(p):
            continue

        def cell(du, dv):
            q = p.copy()
            q[:, u] += du
            q[:, v] += dv
            return vid[q[:, 0], q[:, 1], q[:, 2]]

        quad = np.stack([cell(-1, -1), cell(0, -1), cell(0, 0), cell(-1, 0)], 1)
        assert (quad >= 0).all()
        outside = ~ins[p[:, 0], p[:, 1], p[:, 2]]
        quad[outside] = quad[outside][:, ::-1]
        keys.append(((p[:, 0] * n[1] + p[:, 1]) * n[2] + p[:, 2]) * 3 + a)
        rows.append(quad)
    if rows:
        order = np.argsort(np.concatenate(keys), kind="stable")
        quads = np.concatenate(rows)[order].astype(index_dtype)
    else:
        quads = np.zeros((0, 4), index_dtype)
    return dict(lattice=lattice, verts=affine(lattice, vert_div, vert_mul, vert_add), quads=quads, faces=_split(lattice, quads))


def surface_nets_loops(vol, level=0.0, vert_div=1.0, vert_mul=1.0, vert_add=0.0, index_dtype=np.int32):
    vol = np.asarray(vol, np.float32)
    n0, n1, n2 = n = vol.shape
    level = float(level)
    lf = level_float(level)

    def inside(p):
        x = vol[p]
        return bool(x > lf) if x == x else False

    edges = cell_edges()
    vid, lattice = {}, []
    for i in itertools.product(range(n0 - 1), range(n1 - 1), range(n2 - 1)):
        signs = [inside((i[0] + d[0], i[1] + d[1], i[2] + d[2])) for d in itertools.product((0, 1), repeat=3)]
        if all(signs) or not any(signs):
            continue
        s, cnt = [0.0, 0.0, 0.0], 0.0
        for axis, lo in edges:
            pa = tuple(i[k] + lo[k] for k in range(3))
            pb = tuple(pa[k] + (k == axis) for k in range(3))
            if inside(pa) == inside(pb):
                continue
            a, b = np.float64(vol[pa]), np.float64(vol[pb])
            with np.errstate(all="ignore"):
                t = float((np.float64(level) - a) / (b - a))
            if not np.isfinite(t):
                t = 0.5
            for k in range(3):
                s[k] = s[k] + (float(lo[k]) + (t if k == axis else 0.0))
            cnt = cnt + 1.0
        vid[i] = len(lattice)
        lattice.append([np.float32(float(i[k]) + s[k] / cnt) for k in range(3)])
    lattice = np.array(lattice, np.float32).reshape(-1, 3)
    quads = []
    for p in itertools.product(range(n0), range(n1), range(n2)):
        for a in range(3):
            u, v = (a + 1) % 3, (a + 2) % 3
            if not (p[a] <= n[a] - 2 and 1 <= p[u] <= n[u] - 2 and 1 <= p[v] <= n[v] - 2):
                continue
            hi = tuple(p[k] + (k == a) for k in range(3))
            if inside(p) == inside(hi):
                continue

            def cell(du, dv):
                q = list(p)
                q[u] += du
                q[v] += dv
                return vid[tuple(q)]

            quad = [cell(-1, -1), cell(0, -1), cell(0, 0), cell(-1, 0)]
            quads.append(quad if inside(p) else quad[::-1])
    quads = np.array(quads, index_dtype).reshape(-1, 4)
    faces = []
    for q0, q1, q2, q3 in quads.tolist():
        def d2(a, b):
            d = [float(lattice[a][k]) - float(lattice[b][k]) for k in range(3)]
            return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]

        if d2(q1, q3) < d2(q0, q2):
            faces += [[q0, q1, q3], [q1, q2, q3]]
        else:
            faces += [[q0, q1, q2], [q0, q2, q3]]
    faces = np.array(faces, index_dtype).reshape(-1, 3)
    return dict(lattice=lattice, verts=affine(lattice, vert_div, vert_mul, vert_add), quads=quads, faces=faces)


def edge_report(faces):
    """Undirected edges of a triangle or polygon list by the number of faces at them -> dict(edges, border, non_manifold)."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([np.stack([f[:, k], f[:, (k + 1) % f.shape[1]]], 1) for k in range(f.shape[1])])
    e.sort(axis=1)
    _, counts = np.unique(e[:, 0] * (int(e.max()) + 1 if len(e) else 1) + e[:, 1], return_counts=True)
    return dict(edges=int(len(counts)), border=int((counts == 1).sum()), non_manifold=int((counts > 2).sum()))


def min_angles_deg(vertices, faces):
    """The smallest interior angle of every triangle, in degrees (fp64)."""
    P = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    out = np.full(len(P), 180.0)
    for k in range(3):
        a, b = P[:, (k + 1) % 3] - P[:, k], P[:, (k + 2) % 3] - P[:, k]
        with np.errstate(all="ignore"):
            cos = (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        out = np.minimum(out, np.degrees(np.arccos(np.clip(np.nan_to_num(cos, nan=1.0), -1.0, 1.0))))
    return out
