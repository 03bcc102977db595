"""A plain NumPy restatement of the box-projection UV unwrapper's kernels (sculptmate_amd/csrc/uv_unwrap.hip) and of the
fixed-point vertex sums they share with the geometry tail (csrc/fixsum.h), for the stage tests in
tests/test_gpu_uv_unwrap_stages.py -- test infrastructure, written for reading, not for speed.

Float32 in the kernels' operation order, so the device must match bit for bit, wherever the kernel spells its arithmetic
with _rn intrinsics or uses exact operations (min / max, comparisons, the fixed-point sums):
  rotate_mesh        uv_rotate_mesh_kernel                rotation + bounding box
  box_project        uv_box_project_kernel + _finish      unit_coord, summed corner normals, six-way argmax, u / v, ST_DIV
  vertex_tangents    uv_face_tangent_kernel + uv_vertex_tangent_kernel  (fixed-point sums: exact given the terms)
  expected_tangents  expected_tangent
  rotate_charts      uv_rotate_chart_kernel + uv_rescale_chart_kernel
  assign_atlas       uv_zbuffer_kernel (both passes, both levels, the sub-pixel rule), uv_copy_chart_kernel
  place              uv_slice_stats_kernel, uv_scan_blocks_kernel, uv_place_kernel
Float64 with a bound, where the device adds doubles in an order of its own:
  moments            uv_moments_kernel
  chart_sums         uv_chart_sums_kernel + uv_chart_reduce_kernel
"""
import math

import numpy as np

# min / max follow fminf / fmaxf: a NaN operand loses (np.fmin / np.fmax / np.nanmin / np.nanmax)

F = np.float32
U64 = np.uint64
EDGE_EPS = F(1e-4)
FX_BITS = 40
THIRD = F(1.0) / F(3.0)


def f32(x):
    return np.asarray(x, F)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, F)).view(np.uint32)


def same_bits(a, b):
    """Bit-identical, NaN payloads aside (0/0 is 0x7fc00000 on the device, 0xffc00000 on x86)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


# ------------------------------------------------------------------------------------------------------------- moments
def moments(v):
    """uv_moments_kernel:90-103 -> (sums9 fp64, bound): x y z xx xy xz yy yz zz.  The device adds fp64 products in its own
    order (per thread, shuffle tree, block atomics): |error| <= (n - 1) * 2^-53 * sum |term| per sum, doubled for safety."""
    d = np.asarray(v, F).astype(np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    terms = [x, y, z, x * x, x * y, x * z, y * y, y * z, z * z]
    s = np.array([t.sum() for t in terms])
    bound = np.array([2.0 * len(d) * 2.0 ** -53 * np.abs(t).sum() for t in terms]) + 1e-300
    return s, bound


# ----------------------------------------------------------------------------------------------------- box projection
def rotate_mesh(pos, nrm, rot):
    """uv_rotate_mesh_kernel:108-138: row r = (R[r,0] p0 + R[r,1] p1) + R[r,2] p2, each step rounded; bbox = exact min / max."""
    R = f32(rot).reshape(3, 3)
    p, n = f32(pos), f32(nrm)
    rp = np.stack([(R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2] for r in range(3)], 1).astype(F)
    rn = np.stack([(R[r, 0] * n[:, 0] + R[r, 1] * n[:, 1]) + R[r, 2] * n[:, 2] for r in range(3)], 1).astype(F)
    return rp, rn, np.nanmin(rp, 0), np.nanmax(rp, 0)


def box_project(rp, rn, faces, lo, hi):
    """uv_box_project_kernel:145-192 + uv_box_finish_kernel:194-201 -> (face_uv [nf,3,2], chart [nf] int32)."""
    f = np.asarray(faces, np.int64)
    tri = (F(2.0) * ((rp[f] - lo) / (hi - lo)) - F(1.0)).astype(F)           # unit_coord, [nf,3,3]
    ns = ((rn[f[:, 0]] + rn[f[:, 1]]) + rn[f[:, 2]]).astype(F)
    ln = np.sqrt((ns[:, 0] * ns[:, 0] + ns[:, 1] * ns[:, 1]) + ns[:, 2] * ns[:, 2]).astype(F)
    fn = (ns / np.fmax(ln, F(1e-6))[:, None]).astype(F)
    cand = np.stack([fn[:, 0], -fn[:, 0], fn[:, 1], -fn[:, 1], fn[:, 2], -fn[:, 2]], 1)
    chart = np.zeros(len(f), np.int32)
    best = cand[:, 0].copy()
    for k in range(1, 6):                                                       # strict >: the first maximum wins
        m = cand[:, k] > best
        best[m], chart[m] = cand[m, k], k
    ax = chart >> 1
    us = np.where(ax == 0, 1, 0)
    vs = np.where(ax == 2, 1, 2)
    r = np.arange(len(f))
    uc = tri[r[:, None], np.arange(3)[None], us[:, None]]
    vc = tri[r[:, None], np.arange(3)[None], vs[:, None]]
    vc = np.where((chart == 4)[:, None], vc, -vc)
    div = np.fmax(np.nanmax(np.abs(tri[r[:, None], np.arange(3)[None], ax[:, None]]), 0), F(0.0))  # ST_DIV: per corner slot
    fin = lambda c: np.fmin(np.fmax(((c / div[None]) + F(1.0)) * F(0.5), F(0)), F(1)).astype(F)  # noqa: E731
    return np.stack([fin(uc), fin(vc)], -1).astype(F), chart


# ------------------------------------------------------------------------------------------------------------ tangents
def fixed_point_sum(idx, terms, n):
    """fixsum.h: per (vertex, component) sum of float terms -> float32 [n, 3] (0 where a vertex has no non-zero term, NaN
    where one of its terms is not finite)."""
    terms = f32(terms)
    mag = np.zeros((n, 3), np.uint32)
    tb = bits(np.abs(terms)) & np.uint32(0x7FFFFFFF)
    for r in range(3):
        np.maximum.at(mag[:, r], idx, tb[:, r])
    nonfinite = mag >= np.uint32(0x7F800000)
    _, e = np.frexp(np.where(nonfinite, np.uint32(0), mag).view(F))
    e = e.astype(np.int64)
    with np.errstate(invalid="ignore"):
        q = np.rint(np.ldexp(np.where(np.isfinite(terms), terms, F(0)).astype(np.float64), FX_BITS - e[idx])).astype(np.int64)
    q[nonfinite[idx]] = 0
    acc = np.zeros((n, 3), np.int64)
    for r in range(3):
        np.add.at(acc[:, r], idx, q[:, r])
    out = np.ldexp(acc.astype(np.float64), e - FX_BITS).astype(F)
    return np.where(nonfinite, F(np.nan), np.where(mag != 0, out, F(0.0)))


def face_tangents(rp, faces, uv):
    """uv_face_tangent_kernel: per-face UV tangent, float32 in the kernel's order."""
    f = np.asarray(faces, np.int64)
    t = f32(uv).reshape(-1, 6)
    du1, dv1, du2, dv2 = t[:, 2] - t[:, 0], t[:, 3] - t[:, 1], t[:, 4] - t[:, 0], t[:, 5] - t[:, 1]
    den = np.fmax(du1 * dv2 - dv1 * du2, F(1e-6)).astype(F)
    p0 = rp[f[:, 0]]
    d1, d2 = rp[f[:, 1]] - p0, rp[f[:, 2]] - p0
    return ((d1 * dv2[:, None] - d2 * dv1[:, None]) / den[:, None]).astype(F)


def vertex_tangents(rp, rn, faces, uv):
    """uv_face_tangent_kernel + uv_vertex_tangent_kernel -> vt [nv, 4] float32 (xyz, corner count); NaN where unreferenced."""
    f = np.asarray(faces, np.int64)
    nv = len(rp)
    tg = face_tangents(rp, faces, uv)
    idx = f.reshape(-1)
    s = fixed_point_sum(idx, np.repeat(tg, 3, 0), nv)
    cnt = np.bincount(idx, minlength=nv).astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (s / cnt[:, None]).astype(F)
        ln = np.fmax(np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]), F(1e-12)).astype(F)
        t = (t / ln[:, None]).astype(F)
        d = ((t[:, 0] * rn[:, 0] + t[:, 1] * rn[:, 1]) + t[:, 2] * rn[:, 2]).astype(F)
        t = (t - d[:, None] * rn).astype(F)
        ln = np.fmax(np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]), F(1e-12)).astype(F)
        t = (t / ln[:, None]).astype(F)
    return np.concatenate([t, cnt[:, None]], 1).astype(F)


def expected_tangents(rp, rn):
    """expected_tangent: n x (side x n), divided by the p = -1 "norm" (F.normalize(x, -1)), float32 in the kernel's order."""
    p, n = f32(rp), f32(rn)
    s = [-p[:, 1], p[:, 0], np.zeros_like(p[:, 0])]
    cr = lambda a, b, c, d: (a * b - c * d).astype(F)  # noqa: E731
    c1 = [cr(s[1], n[:, 2], s[2], n[:, 1]), cr(s[2], n[:, 0], s[0], n[:, 2]), cr(s[0], n[:, 1], s[1], n[:, 0])]
    c2 = [cr(n[:, 1], c1[2], n[:, 2], c1[1]), cr(n[:, 2], c1[0], n[:, 0], c1[2]), cr(n[:, 0], c1[1], n[:, 1], c1[0])]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = ((F(1) / np.abs(c2[0]) + F(1) / np.abs(c2[1])) + F(1) / np.abs(c2[2])).astype(F)
        nm = np.fmax(F(1) / inv, F(1e-12)).astype(F)
        return np.stack([c2[k] / nm for k in range(3)], 1).astype(F)


def chart_sums(rp, rn, faces, chart, vt):
    """uv_chart_sums_kernel -> (sums [6,7] fp64, bound [6,7]): per chart the corner sums of vt, of the expected tangent and the
    corner count.  Terms are the device's floats; the device adds them in fp64 in an order of its own, so
    |error| <= (number of terms) * 2^-53 * sum |term|, doubled for safety; the counts are exact."""
    f = np.asarray(faces, np.int64)
    e = expected_tangents(rp, rn)
    c = np.asarray(chart) % 6
    s = np.zeros((6, 7))
    b = np.zeros((6, 7))
    for cc in range(6):
        m = c == cc
        if not m.any():
            continue
        corners = f[m].reshape(-1)
        t = np.concatenate([vt[corners, :3].astype(np.float64), e[corners].astype(np.float64)], 1)
        s[cc, :6] = t.sum(0)
        s[cc, 6] = 3.0 * m.sum()
        b[cc, :6] = 2.0 * len(t) * 2.0 ** -53 * np.abs(t).sum(0)
    return s, b


def chart_angles(sums):
    """unwrap.py BoxProjectionUnwrapper.chart_angles, from the [6,7] sums."""
    angles = np.zeros(6, F)
    for c in range(6):
        if sums[c, 6] == 0:
            continue
        a = (sums[c, 0:3] / sums[c, 6]).astype(F)
        e = (sums[c, 3:6] / sums[c, 6]).astype(F)
        angles[c] = F(math.atan2(float(a[0] * e[1] - a[1] * e[0]), float((a * e).sum(dtype=F))))
    return angles


# ------------------------------------------------------------------------------------------------------- chart rotation
def rotate_charts(uv, chart, cos6, sin6):
    """uv_rotate_chart_kernel:300-341 + uv_rescale_chart_kernel:343-352 (charts without faces are untouched)."""
    t = f32(uv).reshape(-1, 3, 2).copy()
    c = np.asarray(chart) % 6
    co, si = f32(cos6)[c][:, None], f32(sin6)[c][:, None]
    x = (t[..., 0] * F(2) - F(1)).astype(F)
    y = (t[..., 1] * F(2) - F(1)).astype(F)
    u = (co * x + (-si) * y).astype(F)
    v = (si * x + co * y).astype(F)
    out = np.stack([u, v], -1)
    for cc in range(6):
        m = c == cc
        if not m.any():
            continue
        lo, hi = np.nanmin(out[m]), np.nanmax(out[m])
        out[m] = ((out[m] - lo) / (hi - lo)).astype(F)
    return out.astype(F)


def rotation_cos_sin(angles):
    """BoxProjectionUnwrapper.rotate_charts: float32(cos), float32(sin) of every chart's angle."""
    return (np.array([F(math.cos(float(a))) for a in angles], F), np.array([F(math.sin(float(a))) for a in angles], F))


# ----------------------------------------------------------------------------------------------------- atlas assignment
def _raster(t, res):
    """make_raster for a batch of faces t [n,3,2] -> (x [n,3], y [n,3], inv_area, degenerate, x0, x1, y0, y1)."""
    r = F(res)
    x, y = (t[..., 0] * r).astype(F), (t[..., 1] * r).astype(F)
    area = ((x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])).astype(F)
    deg = np.abs(area) < F(1e-12)
    with np.errstate(divide="ignore"):
        inv = np.where(deg, F(0), F(1) / np.where(deg, F(1), area)).astype(F)
    x0 = np.fmax(0, np.floor(x.min(1) - F(0.5)).astype(np.int64))
    x1 = np.fmin(res - 1, np.ceil(x.max(1) - F(0.5)).astype(np.int64))
    y0 = np.fmax(0, np.floor(y.min(1) - F(0.5)).astype(np.int64))
    y1 = np.fmin(res - 1, np.ceil(y.max(1) - F(0.5)).astype(np.int64))
    return x, y, inv, deg, x0, x1, y0, y1


def _inside(x, y, inv, deg, px, py):
    """inside_strict, float32 in the kernel's order; rows of x / y / inv / deg broadcast against px / py."""
    dx, dy = (px - x[:, 0]).astype(F), (py - y[:, 0]).astype(F)
    l1 = ((dx * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * dy) * inv).astype(F)
    l2 = (((x[:, 1] - x[:, 0]) * dy - dx * (y[:, 1] - y[:, 0])) * inv).astype(F)
    return ~deg & (l1 > EDGE_EPS) & (l2 > EDGE_EPS) & (((F(1) - l1) - l2).astype(F) > EDGE_EPS)


def _ord(x):
    u = bits(x).astype(np.uint64)
    return np.where(u & U64(0x80000000), ~u & U64(0xFFFFFFFF), u | U64(0x80000000))


def assign_atlas(rp, faces, uv, chart, res):
    """uv_zbuffer_kernel:395-433 over the two levels of sculpt_uv_assign_atlas -> assigned [nf] int32.
    Key = ordered depth << 32 | (0xffffffff - face id): further out along the chart's direction wins, then the lowest id.
    Samples: pixel centres with all three barycentrics > EDGE_EPS.  A face without samples is tested at its centroid against
    the triangle that owns that pixel (if that one's key is larger)."""
    f = np.asarray(faces, np.int64)
    t = f32(uv).reshape(-1, 3, 2)
    nf = len(f)
    assigned = np.asarray(chart, np.int32).copy()
    c_all = assigned % 6
    ax = c_all >> 1
    r = np.arange(nf)
    cen = ((((rp[f[:, 0], ax] + rp[f[:, 1], ax]).astype(F) + rp[f[:, 2], ax]).astype(F)) * THIRD).astype(F)
    depth = np.where(c_all & 1, -cen, cen).astype(F)
    key = (_ord(depth) << U64(32)) | (U64(0xFFFFFFFF) - r.astype(np.uint64))
    x, y, inv, deg, x0, x1, y0, y1 = _raster(t, res)
    nx, ny = np.fmax(x1 - x0 + 1, 0), np.fmax(y1 - y0 + 1, 0)
    for level in range(2):
        ids = np.nonzero(assigned // 6 == level)[0]
        c = assigned[ids] % 6
        cnt = nx[ids] * ny[ids]
        fi = np.repeat(np.arange(len(ids)), cnt)                   # candidate samples (face, pixel) of the bounding boxes
        start = np.repeat(np.cumsum(cnt) - cnt, cnt)
        k = np.arange(len(fi)) - start
        g = ids[fi]
        px = x0[g] + k % nx[g]
        py = y0[g] + k // nx[g]
        ins = _inside(x[g], y[g], inv[g], deg[g], (px.astype(F) + F(0.5)), (py.astype(F) + F(0.5)))
        g, px, py = g[ins], px[ins], py[ins]
        cell = (c[np.searchsorted(ids, g)].astype(np.int64) * res + py) * res + px
        zb = np.zeros(6 * res * res, np.uint64)
        np.maximum.at(zb, cell, key[g])
        lost = np.zeros(nf, bool)
        lost[g[zb[cell] != key[g]]] = True
        has = np.zeros(nf, bool)
        has[g] = True
        sub = ids[~has[ids]]                                        # smaller than a pixel: the centroid rule
        if len(sub):
            cx = ((((x[sub, 0] + x[sub, 1]).astype(F) + x[sub, 2]).astype(F)) * THIRD).astype(F)
            cy = ((((y[sub, 0] + y[sub, 1]).astype(F) + y[sub, 2]).astype(F)) * THIRD).astype(F)
            pxs = np.clip(np.trunc(cx).astype(np.int64), 0, res - 1)
            pys = np.clip(np.trunc(cy).astype(np.int64), 0, res - 1)
            w = zb[((assigned[sub] % 6).astype(np.int64) * res + pys) * res + pxs]
            front = w > key[sub]
            wf = (U64(0xFFFFFFFF) - (w & U64(0xFFFFFFFF))).astype(np.int64)
            wf = np.where(front, wf, 0)
            hid = front & _inside(x[wf], y[wf], inv[wf], deg[wf], cx, cy)
            lost[sub[hid]] = True
        mv = ids[lost[ids]]
        assigned[mv] = (assigned[mv] % 6 + 6) if level == 0 else 12
    return assigned


def subpixel_faces(uv, assigned, res):
    """Faces of levels 0 / 1 without a sample at resolution res: the ones the centroid rule decides."""
    t = f32(uv).reshape(-1, 3, 2)
    x, y, inv, deg, x0, x1, y0, y1 = _raster(t, res)
    out = np.zeros(len(t), bool)
    for i in np.nonzero(np.asarray(assigned) < 12)[0]:
        px = np.arange(x0[i], x1[i] + 1)
        py = np.arange(y0[i], y1[i] + 1)
        if len(px) == 0 or len(py) == 0:
            out[i] = True
            continue
        PX, PY = np.meshgrid(px.astype(F) + F(0.5), py.astype(F) + F(0.5))
        n = PX.size
        out[i] = not _inside(np.repeat(x[i:i + 1], n, 0), np.repeat(y[i:i + 1], n, 0), np.repeat(inv[i:i + 1], n), np.repeat(deg[i:i + 1], n),
                             PX.reshape(-1), PY.reshape(-1)).any()
    return out


# ------------------------------------------------------------------------------------------------------------ placement
def _clamp01(x):
    return np.fmin(np.fmax(x, F(0)), F(1)).astype(F)


def place(uv, assigned, pad):
    """uv_slice_stats_kernel + uv_scan_blocks_kernel + uv_place_kernel:440-598 -> out [nf*3, 2] float32."""
    t = f32(uv).reshape(-1, 3, 2)
    a = np.asarray(assigned, np.int64)
    uc, vc = t[..., 0].copy(), t[..., 1].copy()
    for s in range(6, 12):                                         # _handle_slice_uvs
        m = a == s
        if not m.any():
            continue
        ulo, uhi, vlo, vhi = np.nanmin(uc[m]), np.nanmax(uc[m]), np.nanmin(vc[m]), np.nanmax(vc[m])
        us, vs = np.fmax(F(uhi - ulo), F(0.5)), np.fmax(F(vhi - vlo), F(0.5))
        uc[m] = ((uc[m] - ulo) / us).astype(F)
        vc[m] = ((vc[m] - vlo) / vs).astype(F)
    pad = float(pad)
    m1, a1 = F(1.0 - 2.0 * pad), F(pad)
    uc = _clamp01(uc * m1 + a1)
    vc = _clamp01(vc * m1 + a1)
    rem = a >= 12
    left = int(rem.sum())
    if left:                                                       # _handle_remaining_uvs, rank = order of face ids
        nw = int(math.ceil(0.5 * math.sqrt(left / (0.5 * (1.0 / 3.0)))))
        nh = int(math.ceil(left / float(nw)))
        w, h = 1.0 / nw, 1.0 / nh
        lim = F(min(w, h) * 1.5)
        ru, rv = uc[rem], vc[rem]
        ulo, uhi, vlo, vhi = ru.min(1, keepdims=True), ru.max(1, keepdims=True), rv.min(1, keepdims=True), rv.max(1, keepdims=True)
        us, vs = np.fmax((uhi - ulo).astype(F), lim), np.fmax((vhi - vlo).astype(F), lim)
        mu, au = F(1.0 - pad * nw * 0.5), F(pad * nw * 0.25)
        mv, av = F(1.0 - pad * nh * 0.5), F(pad * nh * 0.25)
        wf, hf = F(w), F(h)
        rank = np.arange(left)
        xo = ((rank % nw).astype(F) * wf).astype(F)[:, None]
        yo = ((rank // nw).astype(F) * hf).astype(F)[:, None]
        m2, a2 = F(1.0 - 2.0 * pad * 0.5), F(pad * 0.5)
        u = _clamp01(((ru - ulo) / us).astype(F) * mu + au)
        v = _clamp01(((rv - vlo) / vs).astype(F) * mv + av)
        u = (u * wf + xo).astype(F)
        v = (v * hf + yo).astype(F)
        uc[rem] = _clamp01(u * m2 + a2)
        vc[rem] = _clamp01(v * m2 + a2)
    lvl, six = a // 6, a % 6
    gx, gy = six % 3, six // 3
    ox = np.where(lvl == 0, (1.0 / 3.0) * gx, (1.0 / 6.0) * gx + np.fmin(lvl - 1, 1) * 0.5).astype(F)
    oy = np.where(lvl == 0, (1.0 / 3.0) * gy, (1.0 / 6.0) * gy + (1.0 / 3.0) * 2.0).astype(F)
    dx = np.where(lvl == 0, F(3), np.where(lvl >= 2, F(2), F(6))).astype(F)
    dy = np.where(lvl == 0, F(3), np.where(lvl >= 2, F(3), F(6))).astype(F)
    u = (uc / dx[:, None] + ox[:, None]).astype(F)
    v = (vc / dy[:, None] + oy[:, None]).astype(F)
    return np.stack([u, v], -1).reshape(-1, 2).astype(F)


# ------------------------------------------------------------------------------------------------------- geometry tail
def vertex_normals64(v, faces):
    """mesh.py:66-92 in fp64 from the fp32 positions -> (normals [nv,3], bound [nv]).  The kernel rounds the edge vectors and
    the cross products in fp32 (maybe fused), then sums fixed-point: per face |dn| <= 8 u |a| |b| (u = 2^-24); the direction of
    the sum moves by at most 2 sum|dn| / |sum n|, plus the fp32 normalisation (8 u)."""
    p = np.asarray(v, F).astype(np.float64)
    f = np.asarray(faces, np.int64)
    a, b = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
    n = np.cross(a, b)
    err = 8 * 2.0 ** -24 * np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)
    acc = np.zeros_like(p)
    e = np.zeros(len(p))
    for k in range(3):
        np.add.at(acc, f[:, k], n)
        np.add.at(e, f[:, k], err)
    sq = (acc * acc).sum(1)
    zero = ~(sq > 1e-20)
    acc[zero] = [0.0, 0.0, 1.0]
    ln = np.sqrt((acc * acc).sum(1))
    bound = np.where(zero, 8 * 2.0 ** -24, 2 * e / np.fmax(ln, 1e-300) + 8 * 2.0 ** -24)
    return acc / ln[:, None], bound, zero, sq


def vertex_tangents64(v, tex, nrm, faces):
    """mesh.py:94-139 in fp64 from the fp32 inputs (nrm: the device's normals) -> (tangents [nv,3], bound [nv]).
    Per face, the fp32 numerator and the clipped denominator carry a relative error of at most 8 u of their terms' scale, so
    |dt_f| <= 16 u (|dp1| |duv2| + |dp2| |duv1|) / den + |t_f| * 16 u sum|duv| terms / den; the mean moves by sum |dt_f| / count,
    the unit vector by 2 x that / |mean|, the projection off the normal by 2 x that / |t - (t.n) n| (plus 16 u)."""
    p = np.asarray(v, F).astype(np.float64)
    t = np.asarray(tex, F).astype(np.float64)
    n = np.asarray(nrm, F).astype(np.float64)
    f = np.asarray(faces, np.int64)
    duv1, duv2 = t[f[:, 1]] - t[f[:, 0]], t[f[:, 2]] - t[f[:, 0]]
    dp1, dp2 = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
    nom = dp1 * duv2[:, 1:2] - dp2 * duv1[:, 1:2]
    den = duv1[:, 0] * duv2[:, 1] - duv1[:, 1] * duv2[:, 0]
    dsafe = np.fmax(den, 1e-6)
    tang = nom / dsafe[:, None]
    u = 2.0 ** -24
    scale_den = np.abs(duv1[:, 0] * duv2[:, 1]) + np.abs(duv1[:, 1] * duv2[:, 0])
    near_clip = np.abs(den - 1e-6) <= 16 * u * scale_den + 1e-12
    scale_nom = np.abs(dp1) * np.abs(duv2[:, 1:2]) + np.abs(dp2) * np.abs(duv1[:, 1:2])
    err = (16 * u * scale_nom / dsafe[:, None] + np.abs(tang) * 16 * u * (scale_den / dsafe)[:, None]).max(1)
    err = np.where(near_clip, np.inf, err)
    acc = np.zeros_like(p)
    e = np.zeros(len(p))
    cnt = np.zeros(len(p))
    for k in range(3):
        np.add.at(acc, f[:, k], tang)
        np.add.at(e, f[:, k], err)
        np.add.at(cnt, f[:, k], 1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = acc / cnt[:, None]
        lm = np.linalg.norm(m, axis=1)
        tt = m / np.fmax(lm, 1e-12)[:, None]
        q = tt - (tt * n).sum(1, keepdims=True) * n
        lq = np.linalg.norm(q, axis=1)
        out = q / np.fmax(lq, 1e-12)[:, None]
        bound = 2 * (e / cnt) / lm / np.fmax(lq, 1e-30) * 2 + 32 * u / np.fmax(lq, 1e-30)
    return out, bound
