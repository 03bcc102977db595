"""NumPy restatement of the bake at the surface (csrc/bake_surface.hip), put together from the restatements of
the parts it fuses:

    interpolate    the texel's point on the low-poly face (texel_position of csrc/bake_texel.h, ops.bake_interpolate)
    unit_normal    -g / |g| of the raw gradient (unit_normal_of of csrc/field_fwd.h)
    bake_surface   interpolate -> _projref.newton on the covered texels -> _projref.value_grad at the returned points ->
                   unit_normal -> _nmapref.texel_transform (with a frame) -> images that are 0 / -1 where nothing is covered

In np.float64 it is the yardstick of tests/test_bake_surface_host.py; the device is held to the composed route of ops, not to
this file's fp32 run (NumPy's matrix products have another order than the MFMA tiles)."""
import numpy as np

import _nmapref
import _projref


def interpolate(v, f, rast, dtype=np.float32):
    """v [Nv,3], f [Nf,3], rast [res,res,4] -> (p0 [M,3] in `dtype`, bary [M,3] fp32, tri [M], covered [res,res]): the points of
    the covered texels (rast[..., 3] >= 0) in row-major order, (a u + b v) + c w per coordinate."""
    rast = np.asarray(rast, np.float32)
    covered = rast[..., 3] >= 0
    r = rast[covered]
    bary, tri = r[:, :3], r[:, 3].astype(np.int64)
    P = np.asarray(v).astype(dtype)
    F = np.asarray(f).astype(np.int64)
    b = bary.astype(dtype)
    with np.errstate(all="ignore"):
        p0 = (P[F[tri, 0]] * b[:, 0:1] + P[F[tri, 1]] * b[:, 1:2]) + P[F[tri, 2]] * b[:, 2:3]
    return p0, bary, tri, covered


def unit_normal(g):
    """-g / |g| per row, exactly 0 where g is 0 or not finite; the components are scaled by the power of two of the largest
    first, as unit_normal_of does, so that no square overflows."""
    g = np.asarray(g)
    out = np.zeros_like(g)
    with np.errstate(all="ignore"):
        m = np.abs(g).max(axis=1)
        ok = np.isfinite(g).all(axis=1) & (m > 0)
        e = -np.floor(np.log2(m[ok])).astype(np.int64)
        u = np.ldexp(g[ok], e[:, None])
        length = np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2])
        out[ok] = -u / length[:, None]
    return out


def bake_surface(planes, Ws, bs, v, f, rast, target, steps, max_dist, res_tol, dtype, frame=None, radius=_projref.RADIUS):
    """-> dict(point [res,res,3], normal [res,res,3], residual, status i32, evals i32, mask bool [res,res], p0 [M,3]) in `dtype`."""
    p0, bary, tri, covered = interpolate(v, f, rast, dtype)
    res = covered.shape[0]
    out = {"point": np.zeros((res, res, 3), dtype), "normal": np.zeros((res, res, 3), dtype), "residual": np.zeros((res, res), dtype),
           "status": np.full((res, res), -1, np.int32), "evals": np.zeros((res, res), np.int32), "mask": covered, "p0": p0}
    if len(p0) == 0:
        return out
    got = _projref.newton(planes, Ws, bs, p0, target, steps, max_dist, res_tol, dtype, radius)
    _, g = _projref.value_grad(planes, Ws, bs, got["points"], dtype, radius)
    n = unit_normal(g)
    if frame is not None:
        n = _nmapref.texel_transform(n, bary, tri, frame[0], frame[1], dtype)[0]
    out["point"][covered] = got["points"]
    out["normal"][covered] = n
    out["residual"][covered] = got["residual"]
    out["status"][covered] = got["status"]
    out["evals"][covered] = got["evals"]
    return out
