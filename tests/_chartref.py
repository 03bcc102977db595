"""The UV chart atlas rule (include/sculpt_hip.h, "UV CHART ATLAS ON THE DEVICE") restated in NumPy, operation by operation, with
a plain rasteriser that follows the stated semantics of rasterize_cpu (csrc/baker.hip: pixel (x, y) samples (x / res,
1 - y / res) in fp32; a face covers the sample when its three fp32 barycentrics are >= 0).  Nothing here uses the library.

    unwrap(v, f, island_padding=0.02, raster_resolution=256, max_layers=4) -> dict(uv f32 [3 Nf, 2], direction, layer, chart
        int32 [Nf], rect f32 [C, 4], extent f64 [C, 2], cell int64 [C, 2], scale, n_charts, rows, rounds, evicted (per round),
        conflicts, first_round_charts)

and the test meshes of the chart tests (mesh(name))."""
import numpy as np

GUTTER_DIVISOR = 8.0
MAX_ROUNDS = 8
ONE = 1 << 20
MAX_HALVINGS, REFINE_STEPS = 80, 11


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def directions(v, f):
    """1: d int32 [Nf], pq f32 [Nf, 3, 2]."""
    c = v[f].astype(np.float32)                           # [Nf, 3 corners, 3]
    c64 = c.astype(np.float64)
    u, w = c64[:, 1] - c64[:, 0], c64[:, 2] - c64[:, 0]
    n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    k = np.argmax(np.abs(n), 1)                           # the first maximum: ties to the lowest k
    neg = n[np.arange(len(f)), k] < 0
    d = (2 * k + neg).astype(np.int32)
    rows = np.arange(len(f))[:, None]
    p, q = c[rows, np.arange(3)[None], ((k + 1) % 3)[:, None]], c[rows, np.arange(3)[None], ((k + 2) % 3)[:, None]]
    pq = np.stack([np.where(neg[:, None], q, p), np.where(neg[:, None], p, q)], 2).astype(np.float32)
    return d, pq


def halfedge_pairs(f):
    """Pairs (f0, f1) of faces across an undirected edge that has exactly two half-edges, in opposite directions."""
    nf = len(f)
    a, b = f.reshape(-1).astype(np.int64), np.roll(f, -1, 1).reshape(-1).astype(np.int64)   # half-edge 3 f + j: a -> b
    key = (np.minimum(a, b) << 32) | np.maximum(a, b)
    order = np.argsort(key, kind="stable")
    sk = key[order]
    head = np.r_[True, sk[1:] != sk[:-1]]
    start = np.flatnonzero(head)
    count = np.diff(np.r_[start, 3 * nf])
    two = start[count == 2]
    h0, h1 = order[two], order[two + 1]
    keep = (a[h0] != a[h1]) & (h0 // 3 != h1 // 3)
    return h0[keep] // 3, h1[keep] // 3


def labels(nf, pairs, d, layer, max_layers):
    """2: label[f] = the smallest face of f's chart."""
    f0, f1 = pairs
    ok = (d[f0] == d[f1]) & (layer[f0] == layer[f1]) & (layer[f0] < max_layers)
    parent = np.arange(nf)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for x, y in zip(f0[ok].tolist(), f1[ok].tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(x) for x in range(nf)], np.int32)


def f32_to_ordered(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ordered_to_f32(o):
    o = np.asarray(o, np.uint32)
    return np.where(o & np.uint32(0x80000000), o & np.uint32(0x7fffffff), ~o).astype(np.uint32).view(np.float32)


def rectangles(pq, chart, n):
    """3: rect f32 [n, 4] (pmin, pmax, qmin, qmax), extent f64 [n, 2] (w >= h, after the turn), the stable order of the pack."""
    kp, kq = f32_to_ordered(pq[:, :, 0]), f32_to_ordered(pq[:, :, 1])
    lo = np.full((n, 2), 0xffffffff, np.uint32)
    hi = np.zeros((n, 2), np.uint32)
    c3 = np.repeat(chart, 3)
    np.minimum.at(lo[:, 0], c3, kp.reshape(-1)); np.maximum.at(hi[:, 0], c3, kp.reshape(-1))
    np.minimum.at(lo[:, 1], c3, kq.reshape(-1)); np.maximum.at(hi[:, 1], c3, kq.reshape(-1))
    rect = np.stack([ordered_to_f32(lo[:, 0]), ordered_to_f32(hi[:, 0]), ordered_to_f32(lo[:, 1]), ordered_to_f32(hi[:, 1])], 1)
    w = rect[:, 1].astype(np.float64) - rect[:, 0].astype(np.float64)
    h = rect[:, 3].astype(np.float64) - rect[:, 2].astype(np.float64)
    turned = h > w
    extent = np.stack([np.where(turned, h, w), np.where(turned, w, h)], 1)
    key = -extent[:, 1].copy().view(np.int64)
    return rect, extent, np.argsort(key, kind="stable")


def quant(s, e, g):
    return np.ceil((s * e + g) * 1048576.0).astype(np.int64)


def evaluate(s, extent, order, g):
    """Is `s` feasible? -> (feasible, cum [C + 1], row starts, row ys)."""
    wq = quant(s, extent[order, 0], g)
    cum = np.r_[0, np.cumsum(wq)].astype(np.int64)
    C = len(order)
    starts, ys = [], []
    if (wq > ONE).any():
        return False, cum, starts, ys
    start, y = 0, 0
    while start < C:
        starts.append(start); ys.append(y)
        y += int(quant(s, extent[order[start], 1], g))
        if y > ONE:
            return False, cum, starts, ys
        # the smallest j in [start + 1, C) with cum[j + 1] > cum[start] + 2^20, else C
        start = max(start + 1, int(np.searchsorted(cum, cum[start] + ONE, side="right")) - 1)
    return True, cum, starts, ys


def pack(extent, order, g):
    """4: (scale, cell int64 [C, 2], rows)."""
    C = len(order)
    m = float(extent[:, 0].max()) if C else 0.0
    s = 1.0
    if m > 0.0:
        s = float(np.ldexp(1.0, 1 - int(np.frexp(m)[1])))
    halvings = 0
    while not evaluate(s, extent, order, g)[0]:
        if halvings == MAX_HALVINGS:
            raise RuntimeError("no feasible scale")
        halvings += 1
        s *= 0.5
    chosen = s
    if halvings > 0:
        t = 2.0 * s
        for _ in range(REFINE_STEPS):
            t = t * 0.9375
            if evaluate(t, extent, order, g)[0]:
                chosen = t
                break
    ok, cum, starts, ys = evaluate(chosen, extent, order, g)
    assert ok
    starts_a, ys_a = np.asarray(starts, np.int64), np.asarray(ys, np.int64)
    row = np.searchsorted(starts_a, np.arange(C), side="right") - 1
    cell = np.zeros((C, 2), np.int64)
    cell[order, 0] = cum[:C] - cum[starts_a[row]]
    cell[order, 1] = ys_a[row]
    return chosen, cell, len(starts)


def place(pq, chart, rect, cell, s, g):
    """5: uv f32 [3 Nf, 2]."""
    r = rect[chart].astype(np.float64)                    # [Nf, 4]
    w, h = r[:, 1] - r[:, 0], r[:, 3] - r[:, 2]
    turned = (h > w)[:, None]
    p, q = pq[:, :, 0].astype(np.float64), pq[:, :, 1].astype(np.float64)
    pp = np.where(turned, q - r[:, 2:3], p - r[:, 0:1])
    qq = np.where(turned, r[:, 1:2] - p, q - r[:, 2:3])
    x0 = cell[chart, 0].astype(np.float64)[:, None] * (1.0 / 1048576.0) + 0.5 * g
    y0 = cell[chart, 1].astype(np.float64)[:, None] * (1.0 / 1048576.0) + 0.5 * g
    uv = np.stack([x0 + s * pp, y0 + s * qq], 2)
    return uv.astype(np.float32).reshape(-1, 2)


def _bary32(px, py, t):
    """csrc/baker.hip barycentric(), fp32, every operation rounded on its own; t = the face's uv [3, 2]."""
    f = np.float32
    ax, ay, bx, by, cx, cy = (f(t[0, 0]), f(t[0, 1]), f(t[1, 0]), f(t[1, 1]), f(t[2, 0]), f(t[2, 1]))
    e1x, e1y, e2x, e2y = bx - ax, by - ay, cx - ax, cy - ay
    qx, qy = px - ax, py - ay
    d00 = e1x * e1x + e1y * e1y
    d01 = e1x * e2x + e1y * e2y
    d11 = e2x * e2x + e2y * e2y
    d20 = qx * e1x + qy * e1y
    d21 = qx * e2x + qy * e2y
    denom = d00 * d11 - d01 * d01
    with np.errstate(all="ignore"):
        v = (d11 * d20 - d01 * d21) / denom
        w = (d00 * d21 - d01 * d20) / denom
        u = f(1.0) - v - w
    return u, v, w


def rasterize(uv, res):
    """The lowest and the highest covering face per texel: int32 [res, res] each, -1 where no face covers."""
    f = np.float32
    R = f(res)
    low = np.full((res, res), np.iinfo(np.int32).max, np.int32)
    high = np.full((res, res), -1, np.int32)
    tri = uv.reshape(-1, 3, 2)
    mn, mx = tri.min(1), tri.max(1)
    with np.errstate(all="ignore"):
        x0 = np.maximum(np.floor(mn[:, 0] * R).astype(np.int64) - 1, 0)
        x1 = np.minimum(np.ceil(mx[:, 0] * R).astype(np.int64) + 1, res - 1)
        y0 = np.maximum(np.floor((f(1.0) - mx[:, 1]) * R).astype(np.int64) - 1, 0)
        y1 = np.minimum(np.ceil((f(1.0) - mn[:, 1]) * R).astype(np.int64) + 1, res - 1)
    xs_all = np.arange(res, dtype=f) / R
    ys_all = f(1.0) - np.arange(res, dtype=f) / R
    bw, bh = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
    todo = np.argsort(bw * bh, kind="stable")
    todo = todo[(bw * bh)[todo] > 0]
    lowf, highf = low.reshape(-1), high.reshape(-1)
    at = 0
    while at < len(todo):          # faces of similar bounding boxes together, each box padded to the group's largest
        n = min(len(todo) - at, 4096)
        while n > 1 and n * int(bw[todo[at:at + n]].max()) * int(bh[todo[at:at + n]].max()) > (1 << 22):
            n //= 2
        t = todo[at:at + n]
        at += n
        W, H = int(bw[t].max()), int(bh[t].max())
        xs, ys = x0[t, None] + np.arange(W)[None], y0[t, None] + np.arange(H)[None]
        okx, oky = xs <= x1[t, None], ys <= y1[t, None]
        px = xs_all[np.minimum(xs, res - 1)][:, None, :]
        py = ys_all[np.minimum(ys, res - 1)][:, :, None]
        u, v, w = _bary32(px, py, tri[t].transpose(1, 2, 0)[:, :, :, None, None])
        cover = (u >= 0) & (v >= 0) & (w >= 0) & okx[:, None, :] & oky[:, :, None]
        idx = (ys[:, :, None] * res + xs[:, None, :])[cover]
        face = np.broadcast_to(t[:, None, None], cover.shape)[cover].astype(np.int32)
        np.minimum.at(lowf, idx, face)
        np.maximum.at(highf, idx, face)
    low[low == np.iinfo(np.int32).max] = -1
    return low, high


def strictly_inside(uv, t, px, py):
    """6: the fp64 edge functions of faces t (arrays) at the samples (px, py) (fp32 values, widened)."""
    tri = uv.reshape(-1, 3, 2)[t].astype(np.float64)
    ax, ay, bx, by, cx, cy = tri[:, 0, 0], tri[:, 0, 1], tri[:, 1, 0], tri[:, 1, 1], tri[:, 2, 0], tri[:, 2, 1]
    px, py = px.astype(np.float64), py.astype(np.float64)
    e0 = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    e1 = (cx - bx) * (py - by) - (cy - by) * (px - bx)
    e2 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx)
    return ((e0 > 0) & (e1 > 0) & (e2 > 0)) | ((e0 < 0) & (e1 < 0) & (e2 < 0))


def conflicts(uv, chart, res):
    """6: (evicted bool [Nf], chart_conflict bool [C slots = Nf])."""
    nf = len(chart)
    low, high = rasterize(uv, res)
    y, x = np.nonzero((low >= 0) & (low != high))
    lo, hi = low[y, x], high[y, x]
    f = np.float32
    px, py = x.astype(f) / f(res), f(1.0) - y.astype(f) / f(res)
    both = strictly_inside(uv, lo, px, py) & strictly_inside(uv, hi, px, py)
    evicted = np.zeros(nf, bool)
    flagged = np.zeros(nf, bool)
    evicted[hi[both]] = True
    flagged[chart[lo[both]]] = True
    flagged[chart[hi[both]]] = True
    return evicted, flagged


def unwrap(v, f, island_padding=0.02, raster_resolution=256, max_layers=4):
    v, f = np.asarray(v, np.float32), np.asarray(f).astype(np.int64)
    nf = len(f)
    g = float(island_padding) / GUTTER_DIVISOR
    d, pq = directions(v, f)
    pairs = halfedge_pairs(f)
    layer = np.zeros(nf, np.int32)
    out = dict(direction=d, first_round_charts=None)

    def one_round():
        label = labels(nf, pairs, d, layer, max_layers)
        roots = np.flatnonzero(label == np.arange(nf))
        cid = np.full(nf, -1, np.int32)
        cid[roots] = np.arange(len(roots), dtype=np.int32)
        chart = cid[label]
        rect, extent, order = rectangles(pq, chart, len(roots))
        s, cell, rows = pack(extent, order, g)
        uv = place(pq, chart, rect, cell, s, g)
        ev, flagged = conflicts(uv, chart, raster_resolution)
        out.update(uv=uv, chart=chart, rect=rect, extent=extent, cell=cell, scale=s, n_charts=len(roots), rows=rows)
        return ev, flagged, chart

    evicted, final = [], 0
    for r in range(MAX_ROUNDS):
        ev, flagged, chart = one_round()
        if r == 0:
            out["first_round_charts"] = out["n_charts"]
        evicted.append(int(ev.sum()))
        if r == MAX_ROUNDS - 1:
            layer[flagged[chart]] = max_layers
        else:
            layer[ev] += 1
        if evicted[-1] == 0:
            break
    else:
        ev, _, _ = one_round()
        final = int(ev.sum())
    out.update(layer=layer.copy(), rounds=len(evicted), evicted=evicted, conflicts=final)
    return out


def overlapping_samples(uv, res):
    """An independent count: samples of the res x res grid strictly inside two or more faces (every face against every sample
    of its bounding box; no winner maps)."""
    f = np.float32
    tri = uv.reshape(-1, 3, 2)
    count = np.zeros((res, res), np.int32)
    xs = (np.arange(res, dtype=f) / f(res)).astype(np.float64)
    ys = (f(1.0) - np.arange(res, dtype=f) / f(res)).astype(np.float64)
    for t in range(len(tri)):
        a, b, c = tri[t].astype(np.float64)
        x0, x1 = np.searchsorted(xs, min(a[0], b[0], c[0])), np.searchsorted(xs, max(a[0], b[0], c[0]), side="right")
        inside_y = np.flatnonzero((ys >= min(a[1], b[1], c[1])) & (ys <= max(a[1], b[1], c[1])))
        if x1 <= x0 or not len(inside_y):
            continue
        px, py = xs[x0:x1][None, :], ys[inside_y][:, None]
        e0 = (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])
        e1 = (c[0] - b[0]) * (py - b[1]) - (c[1] - b[1]) * (px - b[0])
        e2 = (a[0] - c[0]) * (py - c[1]) - (a[1] - c[1]) * (px - c[0])
        ins = ((e0 > 0) & (e1 > 0) & (e2 > 0)) | ((e0 < 0) & (e1 < 0) & (e2 < 0))
        count[inside_y[0]:inside_y[-1] + 1, x0:x1] += ins
    return int((count >= 2).sum())


# ---- the test meshes -------------------------------------------------------------------------------------------------------------
def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]   # outward
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int64)
    return v, f


def icosphere(levels=3, radius=1.0):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int64)


def nested_icospheres():
    vs, fs, off = [], [], 0
    for r in (1.0, 0.7, 0.4):
        v, f = icosphere(3, r)
        vs.append(v); fs.append(f + off); off += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def torus(nu=48, nv=24, R=1.0, r=0.4):
    a, b = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing="ij")
    v = np.stack([(R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)], 2).reshape(-1, 3)
    f = []
    for i in range(nu):
        for j in range(nv):
            p, q, s, t = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [(p, q, s), (p, s, t)]
    return v.astype(np.float32), np.array(f, np.int64)


def helicoid(turns=2.5, na=120, nr=6, r0=0.5, r1=1.0, pitch=0.5):
    a = np.linspace(0.0, 2 * np.pi * turns, na)
    rad = np.linspace(r0, r1, nr)
    A, Rr = np.meshgrid(a, rad, indexing="ij")
    v = np.stack([Rr * np.cos(A), Rr * np.sin(A), pitch * A / (2 * np.pi)], 2).reshape(-1, 3)
    f = []
    for i in range(na - 1):
        for j in range(nr - 1):
            p, q, s, t = i * nr + j, i * nr + j + 1, (i + 1) * nr + j + 1, (i + 1) * nr + j
            f += [(p, q, s), (p, s, t)]                   # normals face +z
    return v.astype(np.float32), np.array(f, np.int64)


def soup(n=3000, seed=7):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3))
    v = (c + rng.uniform(-0.05, 0.05, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.int64).reshape(-1, 3)


def one_face():
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int64)


def degenerate_face():
    """A good face and, on one of its edges, a face of zero area (three collinear corners)."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 3, 1]], np.int64)


def three_on_an_edge():
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0], [0.5, 0.5, 0.1]], np.float32)
    return v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int64)


def same_direction_pair():
    """Two coplanar faces over the edge (0, 1), both running 0 -> 1: inconsistent winding."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 1, 3]], np.int64)


def tall_chart():
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 3, 0], [0, 3, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int64)


MESHES = dict(cube=cube, icosphere=icosphere, nested=nested_icospheres, torus=torus, helicoid=helicoid, soup=soup, one_face=one_face,
              degenerate=degenerate_face, three_on_an_edge=three_on_an_edge, same_direction=same_direction_pair, tall=tall_chart)

_cache = {}


def mesh(name):
    if ("mesh", name) not in _cache:
        v, f = MESHES[name]()
        v.setflags(write=False); f.setflags(write=False)
        _cache[("mesh", name)] = (v, f)
    return _cache[("mesh", name)]


def reference(name, v=None, f=None):
    """unwrap() of a test mesh at R = 256, computed once per process and shared (read-only)."""
    if ("ref", name) not in _cache:
        if v is None:
            v, f = mesh(name)
        _cache[("ref", name)] = unwrap(v, f, 0.02, 256, 4)
    return _cache[("ref", name)]
