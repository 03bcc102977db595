"""The box-projection UV unwrapper (csrc/uv_unwrap.hip) stage by stage through the C ABI, against the restatement in
tests/_uvref.py: bit for bit where the kernels' arithmetic is exact, within a derived bound where the device adds doubles in
an order of its own.  The meshes cross the kernels' size boundaries: one block (255 / 256 / 257 faces), the scan's rounds of
1024 block counts (> 262 144 faces), the grid cap of num_cus * 32 workgroups (> num_cus * 32 * 256 faces), and take in the
shapes where a rule decides: exact ties between axes, empty charts, several layers, duplicate and degenerate faces, far
offsets, faces smaller than a raster pixel.  Every output buffer starts as a sentinel and has guard words past its end.
The last tests run the whole unwrapper, and the geometry tail, three times and ask for the same bits."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _uvref as R
from sculptmate_amd import ops
from sculptmate_amd._lib import lib
from sculptmate_amd.sf3d.unwrap import BoxProjectionUnwrapper, axis_rotation, principal_axes

pytestmark = pytest.mark.gpu

G = 64                                   # guard elements past every buffer
SENT = {torch.float32: float("nan"), torch.float64: float("nan"), torch.int32: 0x7F7F7F7F, torch.int64: 0x7F7F7F7F7F7F7F7F,
        torch.uint8: 0x7F}


def _num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------------------------------------------- meshes
def _grid_faces(nu, nv, wrap_u, wrap_v):
    f = []
    iu = nu if wrap_u else nu - 1
    iv = nv if wrap_v else nv - 1
    i, j = np.meshgrid(np.arange(iu), np.arange(iv), indexing="ij")
    a = i * nv + j
    b = ((i + 1) % nu) * nv + j
    c = ((i + 1) % nu) * nv + (j + 1) % nv
    d = i * nv + (j + 1) % nv
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return f.astype(np.int64)


def torus(nu, nv, R0=0.6, r0=0.25):
    u, v = np.meshgrid(np.linspace(0, 2 * np.pi, nu, endpoint=False), np.linspace(0, 2 * np.pi, nv, endpoint=False), indexing="ij")
    n = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], -1).reshape(-1, 3)
    c = np.stack([R0 * np.cos(u), R0 * np.sin(u), 0 * u], -1).reshape(-1, 3)
    return (c + r0 * n).astype(np.float32), n.astype(np.float32), _grid_faces(nu, nv, True, True)


def height_field(n):
    x, y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n), indexing="ij")
    z = 0.2 * np.sin(3 * x) * np.cos(2 * y)
    gx, gy = 0.6 * np.cos(3 * x) * np.cos(2 * y), -0.4 * np.sin(3 * x) * np.sin(2 * y)
    nrm = np.stack([-gx, -gy, np.ones_like(z)], -1)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32), nrm.reshape(-1, 3).astype(np.float32), _grid_faces(n, n, False, False)


def octahedron():
    """Every face's summed corner normals tie exactly between two or three axes."""
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    f = []
    for sx in (0, 1):
        for sy in (2, 3):
            for sz in (4, 5):
                f.append([sx, sy, sz] if (sx + sy + sz) % 2 == 0 else [sx, sz, sy])
    return v, v.copy(), np.array(f, np.int64)


def bevelled_cube(n=6, bevel=0.2):
    """A rounded box: flat sides, and bevels whose corner normals sum to exact ties between axes."""
    lin = np.linspace(-1, 1, n)
    pts, nrm, faces = [], [], []
    for ax in range(3):
        for s in (1, -1):
            a, b = [k for k in range(3) if k != ax]
            u, w = np.meshgrid(lin, lin, indexing="ij")
            p = np.zeros(u.shape + (3,))
            p[..., ax], p[..., a], p[..., b] = s * (1 + bevel), u, w
            nn = np.zeros_like(p)
            nn[..., ax] = s
            edge = (np.abs(u) == 1) | (np.abs(w) == 1)
            nn[..., a] += np.where(np.abs(u) == 1, np.sign(u), 0)
            nn[..., b] += np.where(np.abs(w) == 1, np.sign(w), 0)
            nn[edge] /= np.linalg.norm(nn[edge], axis=-1, keepdims=True)
            base = len(pts) and sum(len(x) for x in pts)
            f = _grid_faces(n, n, False, False) + base
            faces.append(f if s > 0 else f[:, ::-1])
            pts.append(p.reshape(-1, 3))
            nrm.append(nn.reshape(-1, 3))
    return np.concatenate(pts).astype(np.float32), np.concatenate(nrm).astype(np.float32), np.concatenate(faces)


def shells(nu=48, radii=(0.9, 0.7, 0.5)):
    """Concentric spheres: three layers in every chart, so level 1 sends faces to 'remaining'."""
    vs, ns, fs = [], [], []
    for r in radii:
        u, w = np.meshgrid(np.linspace(0, 2 * np.pi, nu, endpoint=False), np.linspace(0.05, np.pi - 0.05, nu // 2), indexing="ij")
        n = np.stack([np.sin(w) * np.cos(u), np.sin(w) * np.sin(u), np.cos(w)], -1).reshape(-1, 3)
        fs.append(_grid_faces(nu, nu // 2, True, False) + sum(len(x) for x in vs))
        vs.append(r * n)
        ns.append(n)
    return np.concatenate(vs).astype(np.float32), np.concatenate(ns).astype(np.float32), np.concatenate(fs)


def with_duplicates(mesh):
    v, n, f = mesh
    return v, n, np.concatenate([f, f[::3]])


def with_degenerates(mesh):
    v, n, f = mesh
    v = np.concatenate([v, [[0.25, 0.5, 0.75], [0.5, 1.0, 1.5], [0.75, 1.5, 2.25]]]).astype(np.float32)
    n = np.concatenate([n, [[0, 0, 1], [0, 0, 1], [0, 0, 1]]]).astype(np.float32)
    k = len(v) - 3
    extra = np.array([[f[0, 0], f[0, 0], f[0, 1]], [f[1, 0], f[1, 1], f[1, 1]], [k, k + 1, k + 2], [k, k, k]])  # repeated index, collinear
    return v, n, np.concatenate([f, extra])


def offset_scaled(mesh):
    v, n, f = mesh
    return (v * np.float32(1e-3) + np.float32(1e3)).astype(np.float32), n, f


def tiled(mesh, k):
    """k copies of a mesh side by side (their bounding box grows along x)."""
    v, n, f = mesh
    vs = [v + np.float32([2.1 * i, 0, 0]) for i in range(k)]
    return np.concatenate(vs).astype(np.float32), np.concatenate([n] * k), np.concatenate([f + i * len(v) for i in range(k)])


def first_faces(mesh, k):
    v, n, f = mesh
    return v, n, f[:k]


def mc_mesh(cuda, n, kind):
    lin = np.linspace(-1, 1, n, dtype=np.float32)
    x, y, zz = np.meshgrid(lin, lin, lin, indexing="ij")
    if kind == "sphere":
        sdf = 0.7 - np.sqrt(x * x + 1.3 * y * y + 0.8 * zz * zz)
    elif kind == "ball":
        sdf = 0.7 - np.sqrt(x * x + y * y + zz * zz)
    else:
        sdf = 0.25 - np.sqrt((np.sqrt(x * x + y * y) - 0.6) ** 2 + zz * zz)
    v, f = ops.marching_cubes(torch.from_numpy(sdf.astype(np.float32)).to(cuda), 0.0)
    nrm = ops.vertex_normals(v, f)
    return v.cpu().numpy(), nrm.cpu().numpy(), f.cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ ABI helpers
def _buf(n, dtype, cuda):
    t = torch.full((n + G,), SENT[dtype], dtype=dtype, device=cuda)
    return t


def _guard_ok(t, n):
    g = t[n:].cpu()
    if t.dtype.is_floating_point:
        return bool(torch.isnan(g).all())
    return bool((g == SENT[t.dtype]).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run_stages(cuda, mesh, idx64, res, rot=None):
    """Every stage through the ABI, each against the restatement given the device's own inputs to that stage."""
    v, n, f = mesh
    nv, nf = len(v), len(f)
    fd = torch.from_numpy(f.astype(np.int64 if idx64 else np.int32)).to(cuda)
    vd, nd = torch.from_numpy(v).to(cuda), torch.from_numpy(n).to(cuda)
    S = lambda: torch.cuda.synchronize()  # noqa: E731

    # moments
    m9 = _buf(9, torch.float64, cuda)
    mwb = int(lib.sculpt_uv_moments_workspace_bytes())
    mws = _buf(mwb, torch.uint8, cuda)
    assert lib.sculpt_uv_moments(_p(vd), nv, _p(m9), _p(mws), _s()) == 0
    S()
    want, bound = R.moments(v)
    got = m9[:9].cpu().numpy()
    assert np.all(np.abs(got - want) <= bound), (got, want, bound)
    assert _guard_ok(m9, 9) and _guard_ok(mws, mwb)
    if rot is None:                                                        # the principal frame, as the unwrapper takes it
        rot = axis_rotation(*principal_axes(got, nv))

    # box projection
    W = int(lib.sculpt_uv_stats_words())
    st = _buf(W, torch.int32, cuda)
    rp, rn = _buf(3 * nv, torch.float32, cuda), _buf(3 * nv, torch.float32, cuda)
    uv, chart = _buf(6 * nf, torch.float32, cuda), _buf(nf, torch.int32, cuda)
    r9 = (ctypes.c_float * 9)(*[float(x) for x in rot.reshape(-1)])
    assert lib.sculpt_uv_box_project(_p(vd), _p(nd), nv, _p(fd), int(idx64), nf, ctypes.cast(r9, ctypes.c_void_p), _p(rp), _p(rn), _p(uv),
                                     _p(chart), _p(st), _s()) == 0
    S()
    rp_h, rn_h = rp[:3 * nv].cpu().numpy().reshape(nv, 3), rn[:3 * nv].cpu().numpy().reshape(nv, 3)
    rp_r, rn_r, lo, hi = R.rotate_mesh(v, n, rot)
    assert R.same_bits(rp_h, rp_r) and R.same_bits(rn_h, rn_r)
    uv_r, chart_r = R.box_project(rp_r, rn_r, f, lo, hi)
    chart_h = chart[:nf].cpu().numpy()
    assert np.array_equal(chart_h, chart_r)
    uv_h = uv[:6 * nf].cpu().numpy().reshape(nf, 3, 2)
    assert R.same_bits(uv_h, uv_r)
    for t, k in ((st, W), (rp, 3 * nv), (rn, 3 * nv), (uv, 6 * nf), (chart, nf)):
        assert _guard_ok(t, k)

    # chart tangents
    wsb = int(lib.sculpt_uv_chart_tangents_workspace_bytes(nv))
    ws, vt, sums = _buf(wsb, torch.uint8, cuda), _buf(4 * nv, torch.float32, cuda), _buf(42, torch.float64, cuda)
    assert lib.sculpt_uv_chart_tangents(_p(rp), _p(rn), nv, _p(fd), int(idx64), nf, _p(uv), _p(chart), _p(vt), _p(sums), _p(ws), _s()) == 0
    S()
    vt_h = vt[:4 * nv].cpu().numpy().reshape(nv, 4)
    assert R.same_bits(vt_h, R.vertex_tangents(rp_h, rn_h, f, uv_h))
    s_h = sums[:42].cpu().numpy().reshape(6, 7)
    s_r, s_b = R.chart_sums(rp_h, rn_h, f, chart_h, vt_h)
    assert np.all(np.abs(s_h - s_r) <= s_b), (s_h, s_r, s_b)
    assert np.array_equal(s_h[:, 6], s_r[:, 6])
    for t, k in ((ws, wsb), (vt, 4 * nv), (sums, 42)):
        assert _guard_ok(t, k)
    uw = BoxProjectionUnwrapper(res)
    angles = R.chart_angles(s_h)
    a_r = R.chart_angles(s_r)
    for c in range(6):                                   # the angle moves by at most its condition x the sums' bound
        if s_r[c, 6] == 0:
            assert angles[c] == 0
            continue
        ma, me = s_r[c, :3] / s_r[c, 6], s_r[c, 3:6] / s_r[c, 6]
        da, de = s_b[c, :3] / s_r[c, 6], s_b[c, 3:6] / s_r[c, 6]
        r = math.hypot(ma[0] * me[1] - ma[1] * me[0], float(ma @ me))
        dr = 2 * (np.linalg.norm(ma) * np.linalg.norm(de) + np.linalg.norm(me) * np.linalg.norm(da)) + 1e-6 * np.linalg.norm(ma) * np.linalg.norm(me)
        if r > 100 * dr:
            d = (float(angles[c]) - float(a_r[c]) + math.pi) % (2 * math.pi) - math.pi
            assert abs(d) <= 10 * dr / r + 1e-6, (c, angles, a_r)

    # chart rotation (in place) with the device's angles
    co, si = R.rotation_cos_sin(angles)
    uw.rotate_charts(uv[:6 * nf].view(nf, 3, 2), chart[:nf], angles, st[:W])
    S()
    uv_h2 = uv[:6 * nf].cpu().numpy().reshape(nf, 3, 2)
    assert R.same_bits(uv_h2, R.rotate_charts(uv_h, chart_h, co, si))
    assert _guard_ok(uv, 6 * nf) and _guard_ok(st, W)

    # atlas assignment
    zb, asg = _buf(6 * res * res, torch.int64, cuda), _buf(nf, torch.int32, cuda)
    assert lib.sculpt_uv_assign_atlas(_p(rp), _p(fd), int(idx64), nf, _p(uv), _p(chart), res, _p(zb), _p(asg), _s()) == 0
    S()
    a_h = asg[:nf].cpu().numpy()
    assert _guard_ok(zb, 6 * res * res) and _guard_ok(asg, nf)
    assert np.all((a_h == chart_h) | (a_h == chart_h + 6) | (a_h == 12))
    assert np.array_equal(a_h, R.assign_atlas(rp_h, f, uv_h2, chart_h, res))

    # placement, with the device's assignment
    nb = (nf + 255) // 256
    blk, out = _buf(nb, torch.int32, cuda), _buf(6 * nf, torch.float32, cuda)
    assert lib.sculpt_uv_place(_p(uv), _p(asg), nf, ctypes.c_double(0.02), _p(st), _p(blk), _p(out), _s()) == 0
    S()
    assert R.same_bits(out[:6 * nf].cpu().numpy().reshape(-1, 2), R.place(uv_h2, a_h, 0.02))
    assert int(st[45].item()) == int((a_h >= 12).sum())
    for t, k in ((blk, nb), (out, 6 * nf), (st, W)):
        assert _guard_ok(t, k)
    return dict(chart=chart_h, assigned=a_h, uv=uv_h2)


@pytest.fixture(scope="module")
def meshes(cuda):
    base = torus(160, 80)                                                  # 25 600 faces
    return {
        "octahedron": octahedron(),
        "bevelled_cube": bevelled_cube(),
        "height_field": height_field(60),
        "shells": shells(),
        "duplicates": with_duplicates(torus(40, 20)),
        "degenerates": with_degenerates(torus(40, 20)),
        "offset_scaled": offset_scaled(torus(40, 20)),
        "mc_sphere_24": mc_mesh(cuda, 24, "sphere"),
        "mc_torus_48": mc_mesh(cuda, 48, "torus"),
        "mc_sphere_96": mc_mesh(cuda, 96, "sphere"),
        "f1": first_faces(base, 1),
        "f255": first_faces(base, 255),
        "f256": first_faces(base, 256),
        "f257": first_faces(base, 257),
        "f70k": tiled(base, 3),
    }


EYE = np.eye(3, dtype=np.float32)
AXIS_ALIGNED = ("octahedron", "bevelled_cube", "height_field")      # isotropic or flat: their principal frame is not unique
SMALL = ["octahedron", "bevelled_cube", "height_field", "shells", "duplicates", "degenerates", "offset_scaled", "mc_sphere_24",
         "mc_torus_48", "mc_sphere_96", "f1", "f255", "f256", "f257", "f70k"]


@pytest.mark.parametrize("idx64", [False, True], ids=["i32", "i64"])
@pytest.mark.parametrize("name", SMALL)
def test_stages_vs_restatement(cuda, meshes, name, idx64):
    res = 64 if name in ("mc_sphere_96", "f70k") else 256
    _run_stages(cuda, meshes[name], idx64, res, rot=EYE if name in AXIS_ALIGNED else None)


def test_rules_decide_on_the_adversarial_meshes(cuda, meshes):
    """The shapes do reach the rules they are there for."""
    c = _run_stages(cuda, meshes["octahedron"], False, 64, rot=EYE)["chart"]
    assert np.array_equal(c, [0, 0, 0, 0, 1, 1, 1, 1])                    # (x, y, z) ties: +x / -x, the first maximum
    r = _run_stages(cuda, meshes["height_field"], False, 64, rot=EYE)
    assert not np.any(r["chart"] == 5)                                     # an empty chart
    r = _run_stages(cuda, meshes["shells"], False, 256)
    assert (r["assigned"] == 12).sum() > 500                               # level 1 sends the third layer to 'remaining'
    r = _run_stages(cuda, meshes["duplicates"], False, 256)
    nf0 = 2 * 40 * 20
    dup = np.arange(nf0, len(meshes["duplicates"][2]))
    assert np.all(r["assigned"][dup] != r["chart"][dup])                   # equal depth: the lower id keeps the front layer
    # faces smaller than a pixel at res 16: the centroid rule decides some of them
    r = _run_stages(cuda, meshes["mc_sphere_96"], False, 16)
    sub = R.subpixel_faces(r["uv"][:4000], r["assigned"][:4000], 16)
    assert sub.sum() > 100


@pytest.mark.parametrize("idx64", [False, True], ids=["i32", "i64"])
def test_stages_past_the_scan_round_with_many_remaining(cuda, idx64):
    """> 262 144 faces (several rounds of 1024 block counts in the scan) with thousands of 'remaining' faces."""
    m = tiled(shells(192), 3)
    assert len(m[2]) > 262_144
    r = _run_stages(cuda, m, idx64, 128)
    assert (r["assigned"] == 12).sum() > 2000


@pytest.mark.parametrize("idx64", [False, True], ids=["i32", "i64"])
def test_stages_past_the_grid_cap(cuda, idx64):
    """More faces AND more vertices than num_cus * 32 workgroups of 256 threads: every grid-stride loop, over faces and over
    vertices, takes a second pass.  The extra vertices come first and are unreferenced copies of mesh vertices (the bounding
    box stays), so every referenced one sits past the first pass of the vertex loops."""
    cap = _num_cus() * 32 * 256
    base = torus(400, 200)                                                 # 160 000 faces, 80 000 vertices
    k = cap // len(base[2]) + 1
    v, n, f = tiled(base, k)
    pick = np.arange(cap) % len(v)
    m = (np.concatenate([v[pick], v]), np.concatenate([n[pick], n]), f + cap)
    assert len(m[2]) > cap and m[2].min() >= cap                          # every referenced vertex is past the first pass
    _run_stages(cuda, m, idx64, 128)


def _assign_direct(cuda, px_tris, depth, res):
    """sculpt_uv_assign_atlas on hand-made faces of chart 0: px_tris [nf,3,2] in pixel units, depth [nf] (rot_pos x)."""
    nf = len(px_tris)
    uv = (np.asarray(px_tris, np.float32) / np.float32(res)).astype(np.float32)
    assert np.array_equal(uv * np.float32(res), np.asarray(px_tris, np.float32))          # the kernel sees these pixel values
    rp = np.zeros((3 * nf, 3), np.float32)
    rp[:, 0] = np.repeat(np.asarray(depth, np.float32), 3)
    f = np.arange(3 * nf).reshape(nf, 3)
    chart = np.zeros(nf, np.int32)
    zb, asg = _buf(6 * res * res, torch.int64, cuda), _buf(nf, torch.int32, cuda)
    rpd, fd = torch.from_numpy(rp).to(cuda), torch.from_numpy(f.astype(np.int32)).to(cuda)
    uvd, cd = torch.from_numpy(uv.reshape(-1)).to(cuda), torch.from_numpy(chart).to(cuda)
    assert lib.sculpt_uv_assign_atlas(_p(rpd), _p(fd), 0, nf, _p(uvd), _p(cd), res, _p(zb), _p(asg), _s()) == 0
    torch.cuda.synchronize()
    assert _guard_ok(zb, 6 * res * res) and _guard_ok(asg, nf)
    a = asg[:nf].cpu().numpy()
    assert np.array_equal(a, R.assign_atlas(rp, f, uv, chart, res))
    return a, uv


def test_assignment_sample_exactly_on_edge_eps(cuda):
    """A pixel centre whose barycentric is exactly EDGE_EPS is not a sample (strict >).  Face 0 (in front) has its whole left
    pixel column at l1 == 1e-4f exactly: area 78.125 x 128 = 10 000 px, fl(1 / 10000) == 1e-4f, and the centres lie 1/128 px
    right of its left edge.  Face 1, behind it, holds only the centre (10.5, 40.5) of that column: it keeps its chart because
    face 0 does not draw there.  Under >= face 0 would draw it and send face 1 to the overlap slice."""
    x0 = 10.5 - 1.0 / 128
    a_tri = [[x0, 20.0], [x0 + 78.125, 20.0], [x0, 148.0]]
    b_tri = [[9.9, 39.9], [11.3, 40.1], [10.3, 41.2]]
    x, y, inv, deg, *_ = R._raster(np.float32([a_tri]), 1)
    l1 = ((np.float32(10.5) - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (np.float32(40.5) - y[:, 0])) * inv
    assert l1[0] == R.EDGE_EPS                                                              # the rule decides on equality
    a, _ = _assign_direct(cuda, [a_tri, b_tri], [1.0, 0.5], 256)
    assert np.array_equal(a, [0, 0])


def test_assignment_subpixel_centroid_rule(cuda):
    """Faces without a sample are judged at their centroid: hidden behind the face that owns that pixel (-> 6), kept when in
    front of it, kept when the pixel is empty."""
    big = [[100.0, 100.0], [200.0, 100.0], [100.0, 200.0]]
    tiny = lambda x, y: [[x + 0.2, y + 0.2], [x + 0.45, y + 0.2], [x + 0.2, y + 0.45]]  # noqa: E731  (no centre inside)
    tris = [big, tiny(120, 120), tiny(150, 120), tiny(220, 220)]
    a, uv = _assign_direct(cuda, tris, [1.0, 0.5, 2.0, 0.5], 256)
    assert R.subpixel_faces(uv, a, 256).tolist() == [False, True, True, True]
    assert np.array_equal(a, [0, 6, 0, 0])


# --------------------------------------------------------------------------------------------------------- reproducibility
def test_whole_unwrap_and_tail_reproducible(cuda):
    """Three runs of BoxProjectionUnwrapper on >= 600 k faces give the same bits; so do ops.vertex_normals / vertex_tangents."""
    v, n, f = tiled(torus(400, 200), 4)                                    # 640 000 faces
    assert len(f) >= 600_000
    vd, fd = torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda)
    nd = ops.vertex_normals(vd, fd)
    runs = []
    for _ in range(3):
        uw = BoxProjectionUnwrapper(1024)
        uv, _ = uw(vd, nd, fd, 0.02)
        torch.cuda.synchronize()
        runs.append((uv.cpu().numpy(), uw.last["chart"].cpu().numpy(), uw.last["angles"].copy(), uw.last["assigned"].cpu().numpy()))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert a.tobytes() == b.tobytes()
    tex = torch.from_numpy(runs[0][0][: len(v)].copy()).to(cuda)
    nrm = [ops.vertex_normals(vd, fd).cpu().numpy() for _ in range(3)]
    tng = [ops.vertex_tangents(vd, tex, nd, fd).cpu().numpy() for _ in range(3)]
    assert nrm[0].tobytes() == nrm[1].tobytes() == nrm[2].tobytes()
    assert tng[0].tobytes() == tng[1].tobytes() == tng[2].tobytes()


def test_unwrap_reproducible_on_an_isotropic_ball(cuda):
    """A ball's covariance is nearly isotropic: its principal frame is ill-conditioned, so a last-bit change in the moments
    could turn every chart.  Three runs give the same rotation and the same UVs."""
    v, n, f = mc_mesh(cuda, 160, "ball")
    vd, nd, fd = (torch.from_numpy(x).to(cuda) for x in (v, n, f))
    runs = []
    for _ in range(3):
        uw = BoxProjectionUnwrapper(512)
        uv, _ = uw(vd, nd, fd, 0.02)
        runs.append((np.asarray(uw.last["rot"]).tobytes(), uv.cpu().numpy().tobytes()))
    assert runs[0] == runs[1] == runs[2]


# ---------------------------------------------------------------------------------------------------------- geometry tail
def _tail_mesh(kind):
    if kind == "small":
        v, _, f = with_degenerates(torus(40, 20))
        v = np.concatenate([v, [[7, 7, 7], [8, 8, 8]]]).astype(np.float32)            # unreferenced vertices
        return v, f
    v, _, f = tiled(torus(400, 200), 2 if kind == "scan" else 14)                   # 320 000 / 2 240 000 faces
    return v, f


@pytest.mark.parametrize("idx64", [False, True], ids=["i32", "i64"])
@pytest.mark.parametrize("kind", ["small", "scan", "cap"])
def test_vertex_normals_and_tangents_vs_fp64(cuda, kind, idx64):
    """sf3d_tail.hip against mesh.py:66-139 in fp64: zero-area faces (the (0, 0, 1) fallback), unreferenced vertices, UV
    triangles of negative area (the denominator clipped to 1e-6 from below only), int32 and int64 faces, and sizes past the
    grid of one launch."""
    v, f = _tail_mesh(kind)
    rng = np.random.default_rng(len(f))
    tex = rng.random((len(v), 2)).astype(np.float32)                                # about half the UV triangles are flipped
    vd, fd = torch.from_numpy(v).to(cuda), torch.from_numpy(f.astype(np.int64 if idx64 else np.int32)).to(cuda)
    n = ops.vertex_normals(vd, fd)
    t = ops.vertex_tangents(vd, torch.from_numpy(tex).to(cuda), n, fd)
    n_h, t_h = n.cpu().numpy(), t.cpu().numpy()
    want, bound, fallback, sq = R.vertex_normals64(v, f)
    clear = (sq > 2e-20) | (sq == 0)                                                   # away from the 1e-20 threshold
    err = np.abs(n_h - want).max(1)
    assert np.all(err[clear] <= bound[clear]), (err[clear] - bound[clear]).max()
    assert np.array_equal(n_h[fallback & clear], np.tile(np.float32([0, 0, 1]), ((fallback & clear).sum(), 1)))
    if kind == "small":
        assert fallback[-2:].all() and fallback[-5:].all()                          # unreferenced; on collinear faces only
    tw, tb = R.vertex_tangents64(v, tex, n_h, f)
    used = np.bincount(f.reshape(-1), minlength=len(v)) > 0
    ok = used & np.isfinite(tb)
    assert ok.mean() > 0.9
    terr = np.abs(t_h - tw).max(1)
    assert np.all(terr[ok] <= tb[ok]), (terr[ok] - tb[ok]).max()
    assert np.isnan(t_h[~used]).all()


@pytest.mark.parametrize("H,W,iters", [(3, 3, 2), (3, 17, 3), (29, 3, 1), (40, 64, 0), (33, 70, 5), (2048, 2048, 2048 // 150)])
def test_dilate_fill_shapes(cuda, H, W, iters):
    from oracle import sf3d_tail as ref

    rng = np.random.default_rng(H * W)
    m = torch.from_numpy(rng.random((1, 1, H, W)) > 0.8)
    im = torch.from_numpy(rng.random((1, 3, H, W)).astype(np.float32)) * m
    got = ops.dilate_fill(im.to(cuda), m.to(cuda), iters).cpu().numpy()
    want = ref.dilate_fill(im, m, iters).numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-6)
    if iters == 0:
        assert np.array_equal(got, im.numpy())


def test_vertex_tangents_nan_uv_propagates(cuda):
    """A NaN texture coordinate makes the tangents of every vertex of its faces NaN, as the reference's sums do, and leaves
    the others finite."""
    v, _, f = torus(40, 20)
    tex = np.random.default_rng(1).random((len(v), 2)).astype(np.float32)
    tex[7] = np.nan
    vd, fd = torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda)
    n = ops.vertex_normals(vd, fd)
    t = ops.vertex_tangents(vd, torch.from_numpy(tex).to(cuda), n, fd).cpu().numpy()
    bad = np.zeros(len(v), bool)
    bad[f[(f == 7).any(1)].reshape(-1)] = True
    assert np.isnan(t[bad]).all(1).all() and np.isfinite(t[~bad]).all()
