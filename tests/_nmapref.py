"""NumPy restatement of csrc/bake_normal.hip's two rules, each in the kernel's own order of operations: with dtype=np.float32
every operation is one IEEE fp32 operation, as on the device with contraction off (the kernels must give these bits); with
dtype=np.float64 the same formulas are the yardstick the fp32 form is measured against.

  corner_tangents   corner_tangents_kernel                          (per-corner tangent frames)
  texel_transform   to_tangent_space of bake_scene_normal_kernel    (world normal -> the vector a tangent-space map stores)
  decode            what a shader does with the stored vector, in fp64

and the small inputs the tests share (octahedron, icosphere, a NumPy cell atlas, a mirrored chart, a face without UV area)."""
import numpy as np


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _positive_finite(x):
    return (x > 0) & (x < np.inf)


def corner_tangents(P, F, uvs, corner_normals, dtype=np.float32):
    """P [Nv,3], F [Nf,3] (in range), uvs [3Nf,2], corner_normals [3Nf,3] -> [3Nf,4] = (T.xyz, w) in `dtype`."""
    P, uv = np.asarray(P).astype(dtype), np.asarray(uvs).astype(dtype).reshape(-1, 3, 2)
    cn = np.asarray(corner_normals).astype(dtype).reshape(-1, 3, 3)
    F = np.asarray(F).astype(np.int64)
    nf = len(F)
    assert F.min(initial=0) >= 0 and F.max(initial=0) < max(len(P), 1)
    one, zero = dtype(1), dtype(0)
    with np.errstate(all="ignore"):
        p0, p1, p2 = P[F[:, 0]], P[F[:, 1]], P[F[:, 2]]
        du1, dv1 = uv[:, 1, 0] - uv[:, 0, 0], uv[:, 1, 1] - uv[:, 0, 1]
        du2, dv2 = uv[:, 2, 0] - uv[:, 0, 0], uv[:, 2, 1] - uv[:, 0, 1]
        det = du1 * dv2 - du2 * dv1
        face_ok = _positive_finite(np.abs(det))
        e1, e2 = p1 - p0, p2 - p0
        t = (e1 * dv2[:, None] - e2 * dv1[:, None]) / det[:, None]
        b = (e2 * du1[:, None] - e1 * du2[:, None]) / det[:, None]
        out = np.empty((nf, 3, 4), dtype)
        for k in range(3):
            N = cn[:, k]
            d = _dot(N, t)
            q = t - N * d[:, None]
            l = np.sqrt(_dot(q, q))
            ok = face_ok & _positive_finite(l)
            T = q / l[:, None]
            w = np.where(_dot(_cross(N, T), b) >= 0, one, -one)
            # the fallback: cross(N, axis of the smallest component), or (1, 0, 0)
            ax, ay, az = np.abs(N[:, 0]), np.abs(N[:, 1]), np.abs(N[:, 2])
            a = np.where((ax <= ay) & (ax <= az), 0, np.where(ay <= az, 1, 2))
            e = np.eye(3, dtype=dtype)[a]
            c = _cross(N, e)
            lc = np.sqrt(_dot(c, c))
            Tf = np.where(_positive_finite(lc)[:, None], c / lc[:, None], np.array([one, zero, zero], dtype))
            out[:, k, :3] = np.where(ok[:, None], T, Tf)
            out[:, k, 3] = np.where(ok, w, one)
    return out.reshape(3 * nf, 4)


def interpolated_frame(bary, tri, corner_normals, corner_tangents_, dtype=np.float32):
    """-> N, T, B (un-normalised, B = s cross(N, T)) per texel in `dtype`."""
    bary = np.asarray(bary).astype(dtype)
    cn = np.asarray(corner_normals).astype(dtype).reshape(-1, 3, 3)[tri]
    ct = np.asarray(corner_tangents_).astype(dtype).reshape(-1, 3, 4)[tri]
    u, v, w = bary[:, 0:1], bary[:, 1:2], bary[:, 2:3]
    N = (cn[:, 0] * u + cn[:, 1] * v) + cn[:, 2] * w
    T = (ct[:, 0, :3] * u + ct[:, 1, :3] * v) + ct[:, 2, :3] * w
    B = ct[:, 0, 3:4] * _cross(N, T)
    return N, T, B


def texel_transform(n, bary, tri, corner_normals, corner_tangents_, dtype=np.float32):
    """World normals n [M,3], barycentrics [M,3], face index [M] -> (stored [M,3] in `dtype`, D [M])."""
    n = np.asarray(n).astype(dtype)
    with np.errstate(all="ignore"):
        N, T, B = interpolated_frame(bary, tri, corner_normals, corner_tangents_, dtype)
        gtt, gnn, gtn = _dot(T, T), _dot(N, N), _dot(T, N)
        D = gtt * gnn - gtn * gtn
        nT, nN, nB = _dot(n, T), _dot(n, N), _dot(n, B)
        x, y, z = nT * gnn - nN * gtn, nB, nN * gtt - nT * gtn
        length = np.sqrt((x * x + y * y) + z * z)
        zero_n = (n == 0).all(1)
        ok = (D > 0) & _positive_finite(length) & ~zero_n
        out = np.stack([x / length, y / length, z / length], 1)
        out = np.where(ok[:, None], out, np.array([0, 0, 1], dtype))
    return out.astype(dtype), D


def decode(stored, bary, tri, corner_normals, corner_tangents_):
    """normalize(x T + y B + z N) in fp64, with the frame interpolated from the given (fp32) corner rows."""
    s = np.asarray(stored, np.float64)
    N, T, B = interpolated_frame(bary, tri, corner_normals, corner_tangents_, np.float64)
    g = s[:, 0:1] * T + s[:, 1:2] * B + s[:, 2:3] * N
    return g / np.linalg.norm(g, axis=1, keepdims=True)


def angle(a, b):
    """Angle in radians between rows of unit-ish vectors, fp64, accurate near 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    return 2.0 * np.arctan2(np.linalg.norm(a - b, axis=1), np.linalg.norm(a + b, axis=1))


# ---------------------------------------------------------------------------------------------- inputs
def octahedron():
    """The octahedron of tests/test_gpu_bake_scene.py."""
    v = np.array([[0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0], [0, -0.5, 0], [0, 0, 0.5], [0, 0, -0.5]], np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)
    return v, f


def icosphere(subdivisions=1, radius=0.5):
    from _smoothref import icosphere as unit

    P, F = unit(subdivisions)
    return (radius * P).astype(np.float32), F.astype(np.int64)


def cell_atlas(P, F, padding=0.05):
    """One grid cell per triangle, drawn isometrically (the layout of ops.uv_cell_atlas; an input here, not held to its bits)."""
    P = np.asarray(P, np.float64)
    nf = len(F)
    cols = max(1, int(np.ceil(np.sqrt(nf))))
    rows = max(1, -(-nf // cols))
    a, e1, e2 = P[F[:, 0]], P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]]
    l1 = np.linalg.norm(e1, axis=1)
    cx = (e1 * e2).sum(1) / l1
    cy = np.sqrt(np.maximum((e2 * e2).sum(1) - cx * cx, 0))
    minx, maxx = np.minimum(0, cx), np.maximum(l1, cx)
    ext = np.maximum(np.maximum(maxx - minx, cy), 1e-20)
    cw, ch = 1.0 / cols, 1.0 / rows
    sx, sy = cw * (1 - 2 * padding) / ext, ch * (1 - 2 * padding) / ext
    i = np.arange(nf)
    ox, oy = (i % cols) * cw + padding * cw, (i // cols) * ch + padding * ch
    uv = np.stack([np.stack([ox - minx * sx, oy], 1), np.stack([ox + (l1 - minx) * sx, oy], 1),
                   np.stack([ox + (cx - minx) * sx, oy + cy * sy], 1)], 1)
    return uv.reshape(3 * nf, 2).astype(np.float32)


def mirror_chart(uvs, face):
    """The chart of `face` mirrored in u about its own middle: it keeps its place in the atlas."""
    uv = np.array(uvs, np.float32).reshape(-1, 3, 2)
    lo, hi = uv[face, :, 0].min(), uv[face, :, 0].max()
    uv[face, :, 0] = (lo + hi) - uv[face, :, 0]
    return uv.reshape(-1, 2)


def zero_area_chart(uvs, face):
    """The chart of `face` collapsed onto the segment between its first two corners: UV determinant exactly 0."""
    uv = np.array(uvs, np.float32).reshape(-1, 3, 2)
    uv[face, 2] = uv[face, 1]
    return uv.reshape(-1, 2)


def vertex_normals(P, F):
    """Area-weighted unit vertex normals (fp64 -> fp32): an input."""
    P = np.asarray(P, np.float64)
    fn = np.cross(P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]])
    vn = np.zeros_like(P)
    for k in range(3):
        np.add.at(vn, F[:, k], fn)
    return (vn / np.linalg.norm(vn, axis=1, keepdims=True)).astype(np.float32)


def bary_grid(n=6):
    """Barycentrics on a triangular lattice, corners and edges included, as fp32 the way a rasteriser hands them over."""
    pts = [(i / n, j / n, (n - i - j) / n) for i in range(n + 1) for j in range(n + 1 - i)]
    return np.array(pts, np.float32)


def samples(F, n=6):
    """Every face x bary_grid -> (bary [M,3], tri [M])."""
    g = bary_grid(n)
    return np.tile(g, (len(F), 1)), np.repeat(np.arange(len(F)), len(g))


def bumpy_normals(P, F, bary, tri, seed=0, sigma=0.3):
    """Unit fp32 'world normals' for host tests: the interpolated vertex normal plus noise (a stand-in for the field's)."""
    rng = np.random.default_rng(seed)
    vn = vertex_normals(P, F).astype(np.float64)
    b = np.asarray(bary, np.float64)
    n = sum(vn[F[tri, k]] * b[:, k:k + 1] for k in range(3))
    n = n / np.linalg.norm(n, axis=1, keepdims=True) + sigma * rng.standard_normal(n.shape)
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
