"""NumPy restatements of the surface distance feature (sculptmate_amd/csrc/mesh_distance.hip; ops.mesh_sample_surface,
ops.mesh_closest_points, ops.mesh_distance) -- test infrastructure, written for reading, not for speed.

Sampling is integer wherever order could matter (uint64 arithmetic by Python ints), so the restatement is bit for bit.  Closest
points are brute force over every face on top of _rmdref.closest_on_triangles, with the device's rule: the lexicographic minimum
of (d2_f, f) over the faces whose d2_f is not NaN.  The metrics sum with math.fsum."""
import math

import numpy as np

import _rmdref as R

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def splitmix64(seed, j):
    """Output j (0-based) of the splitmix64 stream seeded with `seed`."""
    z = (seed + (j + 1) * GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def area2(P, F):
    """Twice the area of every face in fp64 from the fp32 positions: sqrt(cx cx + cy cy + cz cz), left to right."""
    Pd = R.f64(P).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    a, b, c = Pd[F[:, 0]], Pd[F[:, 1]], Pd[F[:, 2]]
    u, v = b - a, c - a
    cx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    cy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    cz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    return np.sqrt(cx * cx + cy * cy + cz * cz)


def weight_bits(nf):
    return min(40, 62 - int(nf).bit_length())


def weights(P, F):
    """w int64 [nf]: rint(ldexp(A2, B - e)) (nearest even), e the frexp exponent of the largest A2."""
    A2 = area2(P, F)
    if len(A2) == 0 or not A2.max() > 0:
        return np.zeros(len(A2), np.int64)
    e = math.frexp(float(A2.max()))[1]
    return np.rint(np.ldexp(A2, weight_bits(len(A2)) - e)).astype(np.int64)


def sample(P, F, n, seed, w=None):
    """(points f32 [n, 3], face i64 [n], uv f32 [n, 2]) by the rule of csrc/mesh_distance.hip; w: the weights to use (default:
    the restated ones)."""
    P = np.asarray(P, np.float32).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    w = weights(P, F) if w is None else np.asarray(w, np.int64)
    cdf = [int(x) for x in np.cumsum(w.astype(object))] if len(w) else []
    W = cdf[-1] if cdf else 0
    pts, face, uv = np.zeros((n, 3), np.float32), np.zeros(n, np.int64), np.zeros((n, 2), np.float32)
    if n:
        assert W > 0, "nothing to sample"
    cdf_a = np.array(cdf, np.int64)
    scale = np.float32(2.0 ** -24)
    one = np.float32(1.0)
    for i in range(n):
        r0, r1, r2 = (splitmix64(seed, 3 * i + k) for k in range(3))
        t = (r0 * W) >> 64
        f = int(np.searchsorted(cdf_a, t, side="right"))     # the first f with cdf[f] > t
        u, v = np.float32(r1 >> 40) * scale, np.float32(r2 >> 40) * scale
        if np.float32(u + v) > one:
            u, v = np.float32(one - u), np.float32(one - v)
        a, b, c = P[F[f, 0]], P[F[f, 1]], P[F[f, 2]]
        pts[i] = (a + u * (b - a)) + v * (c - a)
        face[i] = f
        uv[i] = (u, v)
    return pts, face, uv


def closest(points, P, F):
    """Brute force: (d2 f64 [N], face i64 [N], closest f32 [N, 3]) of every query (fp32, widened) against every face."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    Pd = R.f64(P).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    A, B, C = Pd[F[:, 0]], Pd[F[:, 1]], Pd[F[:, 2]]
    n, nf = len(pts), len(F)
    d2, face, cl = np.full(n, np.inf), np.full(n, -1, np.int64), pts.copy()
    finite = np.isfinite(pts).all(1)
    d2[~finite] = np.nan
    rows = np.nonzero(finite)[0]
    step = max(1, 500_000 // max(nf, 1))                # queries x faces pairs per pass, one pair per row
    for s in range(0, len(rows) if nf else 0, step):
        idx = rows[s:s + step]
        p = np.repeat(pts[idx].astype(np.float64), nf, axis=0)
        with np.errstate(all="ignore"):
            q = R.closest_on_triangles(p, np.tile(A, (len(idx), 1)), np.tile(B, (len(idx), 1)), np.tile(C, (len(idx), 1)))
            e = q - p
            d = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).reshape(len(idx), nf)
        q = q.reshape(len(idx), nf, 3)
        ok = ~np.isnan(d)
        f = np.argmin(np.where(ok, d, np.inf), axis=1)   # argmin: the first face at the least distance
        first_ok = np.argmax(ok, axis=1)                 # (every face left at +inf: the first that is not NaN)
        k = np.arange(len(idx))
        f = np.where(ok[k, f], f, first_ok)
        won = ok[k, f]
        d2[idx[won]], face[idx[won]], cl[idx[won]] = d[k, f][won], f[won], q[k, f][won].astype(np.float32)
    return d2, face, cl


def one_way(d2):
    d = np.sqrt(np.asarray(d2, np.float64))
    n = len(d)
    return {"mean": math.fsum(d) / n, "rms": math.sqrt(math.fsum(d2) / n), "max": float(d.max())}


def metrics(d2_ab, d2_ba, threshold=None):
    """What ops.mesh_distance reports, from the two directions' squared distances."""
    ab, ba = one_way(d2_ab), one_way(d2_ba)
    out = {"a_to_b": ab, "b_to_a": ba, "chamfer": 0.5 * (ab["mean"] + ba["mean"]), "hausdorff": max(ab["max"], ba["max"])}
    if threshold is not None:
        p = int((np.sqrt(d2_ab) < threshold).sum()) / len(d2_ab)
        r = int((np.sqrt(d2_ba) < threshold).sum()) / len(d2_ba)
        out.update(precision=p, recall=r, fscore=2.0 * p * r / (p + r) if p + r > 0 else 0.0)
    return out


def soup(nf=50, seed=7, degenerate=(17,)):
    """A triangle soup with areas over two decades and zero-area faces (three equal corners): (P f32 [3 nf, 3], F i64 [nf, 3])."""
    rng = np.random.default_rng(seed)
    size = 10.0 ** rng.uniform(-1.0, 0.0, nf)            # side 0.1 .. 1: areas over two decades
    centre = rng.uniform(-1.0, 1.0, (nf, 1, 3))
    P = (centre + size[:, None, None] * rng.uniform(-0.5, 0.5, (nf, 3, 3))).astype(np.float32)
    for f in degenerate:
        P[f, 1] = P[f, 0]
        P[f, 2] = P[f, 0]
    return P.reshape(-1, 3), np.arange(3 * nf, dtype=np.int64).reshape(-1, 3)
