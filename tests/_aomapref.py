"""NumPy restatement of the occlusion bake over an atlas (sculptmate_amd/csrc/mesh_ray.hip "the atlas bake";
ops.bake_occlusion) -- test infrastructure, written for reading, not for speed.

Per texel: texel_position's coverage and position, the normal by the same expression, the snap onto the source surface by the
brute-force closest hit of _rayref, and _rayref's occlusion at the result.  NumPy does not contract, so every line is the
kernel's sequence of IEEE operations."""
import numpy as np

import _rmdref as R
from _rayref import amax_of, cross, dot, occlusion, ray_cast


def texel_position(rast, V, F):
    """rast f32 [n, 4], V f32 [nv, 3], F int [nf, 3] -> (covered bool [n], rows i64 [n, 3] (0 where not covered), p f32 [n, 3])."""
    rast = np.asarray(rast, np.float32).reshape(-1, 4)
    V = np.asarray(V, np.float32).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    nv, nf = len(V), len(F)
    w = rast[:, 3]
    with np.errstate(invalid="ignore"):
        ok = (w >= 0) & (w < np.float32(2147483648.0))        # a NaN fails both
    t = np.where(ok, w, 0).astype(np.int64)                   # truncation, as (int) does
    ok &= t < nf
    rows = np.zeros((len(rast), 3), np.int64)
    if nf:
        rows[ok] = F[t[ok]]
    ok &= ((rows >= 0) & (rows < nv)).all(1)
    rows[~ok] = 0
    return ok, rows, interpolate(V, rows, rast, ok)


def interpolate(A, rows, rast, ok):
    """(A[i0] u + A[i1] v) + A[i2] w per component in fp32; 0 where not ok."""
    A = np.asarray(A, np.float32).reshape(-1, 3)
    out = np.zeros((len(rows), 3), np.float32)
    if ok.any():
        r, i = rast[ok], rows[ok]
        with np.errstate(all="ignore"):
            out[ok] = (A[i[:, 0]] * r[:, 0:1] + A[i[:, 1]] * r[:, 1:2]) + A[i[:, 2]] * r[:, 2:3]
    return out


def snap(p, n, SP, SF, cage, amax=None):
    """Step 4 for points p, normals n f32 [m, 3] against the surface (SP, SF) -> (q f32, m f32, hit bool, flipped bool)."""
    p, n = np.asarray(p, np.float32), np.asarray(n, np.float32)
    cage = np.float32(cage)
    with np.errstate(all="ignore"):
        c = cage * n
        o, d = p + c, -c
    t, face, _ = ray_cast(o, d, SP, SF, 0.0, 2.0, amax)
    hit = face >= 0
    q, m, flipped = p.copy(), n.copy(), np.zeros(len(p), bool)
    if hit.any():
        Pd = R.f64(SP).reshape(-1, 3)
        Fh = np.asarray(SF, np.int64).reshape(-1, 3)[face[hit]]
        od, dd = o[hit].astype(np.float64), d[hit].astype(np.float64)
        q[hit] = (od + t[hit][:, None] * dd).astype(np.float32)
        a, b, cc = Pd[Fh[:, 0]], Pd[Fh[:, 1]], Pd[Fh[:, 2]]
        g = cross(b - a, cc - a)
        flip = dot(g, n[hit].astype(np.float64)) < 0
        g = np.where(flip[:, None], -g, g)
        with np.errstate(all="ignore"):
            ln = np.sqrt(dot(g, g))
            unit = (g / ln[:, None]).astype(np.float32)
        good = (ln > 0) & (ln < np.inf)
        m[hit] = np.where(good[:, None], unit, n[hit])
        flipped[hit] = flip
    return q, m, hit, flipped


def bake_occlusion(rast, V, F, N, SP, SF, dirs, offset, max_distance=np.inf, cage=0.0, want_info=False):
    """(ao f32 [res, res], mask bool [res, res]) of the rule; want_info: also dict(hit, flipped, listed) per texel, flat."""
    rast = np.asarray(rast, np.float32)
    res = rast.shape[0]
    flat = rast.reshape(-1, 4)
    covered, rows, p = texel_position(flat, V, F)
    n = interpolate(N, rows, flat, covered)
    finite = np.isfinite(p).all(1) & np.isfinite(n).all(1)
    listed = covered & finite
    ao = np.zeros(len(flat), np.float32)
    ao[covered & ~finite] = np.nan
    hit, flipped = np.zeros(len(flat), bool), np.zeros(len(flat), bool)
    amax = amax_of(SP, SF)
    if listed.any():
        q, m = p[listed], n[listed]
        if float(np.float32(cage)) > 0.0:
            q, m, h, fl = snap(q, m, SP, SF, cage, amax)
            hit[listed], flipped[listed] = h, fl
        ao[listed] = occlusion(q, m, dirs, SP, SF, offset, max_distance, amax)
    out = ao.reshape(res, res), covered.reshape(res, res)
    return out + (dict(hit=hit, flipped=flipped, listed=listed),) if want_info else out


# ---------------------------------------------------------------------------------------------- inputs made without a device
def cell_rast(n_faces, res, pad=0.08):
    """A rast image for n_faces triangles, one per cell of a square grid (the layout of ops.uv_cell_atlas, computed here in
    fp64 and rounded: to the bake a rast is an input like any other).  Texel (x, y) samples (x / res, 1 - y / res)."""
    cols = max(1, int(np.ceil(np.sqrt(n_faces))))
    rast = np.zeros((res, res, 4), np.float32)
    rast[..., 3] = -1.0
    y, x = np.mgrid[0:res, 0:res]
    px, py = x / res, 1.0 - y / res
    for t in range(n_faces):
        cx, cy = (t % cols) / cols, (t // cols) / cols
        s = 1.0 / cols
        ax, ay = cx + pad * s, cy + pad * s
        ex, ey = s * (1 - 2 * pad), s * (1 - 2 * pad)
        v = (px - ax) / ex
        w = (py - ay) / ey
        u = 1.0 - v - w
        inside = (u >= 0) & (v >= 0) & (w >= 0) & (rast[..., 3] < 0)
        rast[inside] = np.stack([u, v, w, np.full_like(u, t)], -1)[inside].astype(np.float32)
    return rast


def source_case(scale, small_cage=False, res=32, k=16):
    """The source-mode case of tests/test_gpu_bake_occlusion.py: the low mesh is an icosphere of level 1 scaled by `scale`, with
    its unit vertex directions as normals; the high surface an icosphere of level 3 and a small cube hovering just above its
    north pole (so that the occlusion is not 1 everywhere, and a snap ray that starts inside the cube hits its bottom face
    from behind: a flipped facet normal).  -> dict of host arrays and the rule's parameters."""
    from test_remesh import icosphere

    lv, lf = icosphere(1)
    hv, hf = icosphere(3)
    unit = (lv / np.linalg.norm(lv, axis=1, keepdims=True)).astype(np.float32)
    cube = np.array([[x, y, z] for z in (1.02, 1.32) for y in (-0.15, 0.15) for x in (-0.15, 0.15)], np.float64)
    cf = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                   [1, 3, 5], [3, 7, 5]], np.int64)
    SP = np.concatenate([hv, cube]).astype(np.float32)
    SF = np.concatenate([np.asarray(hf, np.int64), cf + len(hv)]).astype(np.int32)
    V = (lv * scale).astype(np.float32)
    F = np.asarray(lf, np.int32)
    used = SP[np.unique(SF)]
    longest = float((used.max(0).astype(np.float64) - used.min(0).astype(np.float64)).max())
    cage = 2.0 ** -20 * longest if small_cage else None
    return dict(V=V, F=F, N=unit, SP=SP, SF=SF, rast=cell_rast(len(F), res), k=k, cage=cage,
                cage_value=float(np.float32(2.0 ** -6 * longest if cage is None else cage)),
                offset=float(np.float32(2.0 ** -13 * longest)))
