"""Surface nets on the device (csrc/surface_nets.hip, ops.surface_nets, TSR.extract_meshes(isosurface="surface_nets")) against
the NumPy restatement of the rule (tests/_snref.py) BIT FOR BIT: vertices compared as uint32, quads and faces exactly, in int32
and int64, at the smallest shapes that reach each edge of the kernels; the sign-plane path; the two-pass grid; the chain."""
import numpy as np
import pytest
import torch

import _snref as sn
import _tsrmodel

pytestmark = pytest.mark.gpu

# one cell; the first interior edge; odd sizes; axis 2 across the 32-bit word, the 64-lane ballot and a partial last word; the
# other two axes long (more than one workgroup of words: 33 * 9 * 2 = 594 > 256)
SHAPES = [(2, 2, 2), (3, 3, 3), (5, 6, 7), (9, 33, 70), (33, 9, 35)]


def _noise(shape, seed=0):
    return np.random.default_rng(1000 + seed + sum(shape)).standard_normal(shape).astype(np.float32)


def _smooth(shape):
    """A sphere about an off-centre point, positive inside, that crosses the box's walls on the short axes."""
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    c = [0.43 * (n - 1) + 0.2 for n in shape]
    d = np.sqrt(sum((g[k] - c[k]) ** 2 for k in range(3)))
    return (0.3 * max(shape) + 0.05 - d).astype(np.float32)


def _run(cuda, vol, sign_planes=None, **kw):
    from sculptmate_amd import ops

    planes = None if sign_planes is None else torch.from_numpy(sign_planes).to(cuda)
    got = ops.surface_nets(torch.from_numpy(vol).to(cuda), sign_planes=planes, **kw)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in got]


def _check(cuda, vol, sign_planes=None, **kw):
    """Both index types against the restatement -> the int32 result."""
    ref_kw = {k: v for k, v in kw.items() if k != "faces_i64"}
    out = None
    for i64 in (False, True):
        dt = np.int64 if i64 else np.int32
        want = sn.surface_nets(vol, index_dtype=dt, **ref_kw)
        verts, quads, faces = _run(cuda, vol, sign_planes, faces_i64=i64, **kw)
        assert verts.dtype == np.float32 and quads.dtype == dt and faces.dtype == dt
        assert verts.shape == want["verts"].shape and quads.shape == want["quads"].shape and faces.shape == want["faces"].shape
        assert np.array_equal(verts.view(np.uint32), want["verts"].view(np.uint32))
        assert np.array_equal(quads, want["quads"]) and np.array_equal(faces, want["faces"])
        out = out or (verts, quads, faces)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("field", ["noise", "smooth"])
def test_kernel_equals_the_restatement(cuda, shape, field):
    vol = _noise(shape) if field == "noise" else _smooth(shape)
    verts, quads, faces = _check(cuda, vol)
    assert len(verts) > 0
    if shape == (2, 2, 2):
        assert len(verts) == 1 and len(quads) == 0 and len(faces) == 0     # Nv > 0 with Nq == 0 is a valid result
    else:
        assert len(quads) > 0
    if field == "noise" and min(shape) >= 5:
        assert len(verts) > 0.95 * np.prod([n - 1 for n in shape])        # (nearly) every cell active: the scans and ranks


def test_plane_into_all_six_walls(cuda):
    """A tilted plane through the box's centre meets every wall: sign changes on the boundary give no quad, and nothing is
    read outside the cells."""
    shape = (7, 9, 37)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    vol = ((g[0] - 3.0) / 7 + (g[1] - 4.0) / 9 - (g[2] - 18.0) / 37 + 0.013).astype(np.float32)
    ins = vol > 0
    for axis in range(3):
        for side in (0, -1):
            wall = np.take(ins, side, axis=axis)
            assert wall.any() and not wall.all()
    verts, quads, faces = _check(cuda, vol)
    assert quads.min() >= 0 and quads.max() < len(verts) and len(np.unique(quads)) <= len(verts)
    assert sn.edge_report(quads)["border"] > 0


def test_values_equal_to_the_level(cuda):
    vol = _noise((6, 7, 40), seed=3)
    vol[np.random.default_rng(5).random(vol.shape) < 0.2] = 0.0
    vol[2, 3, 31:34] = 0.0
    _check(cuda, vol)
    vol2 = np.round(_noise((6, 7, 40), seed=4) * 2) / 2          # many exact ties at a non-zero level too
    _check(cuda, vol2.astype(np.float32), level=0.5)


def test_infinities_and_nans_next_to_the_surface(cuda):
    vol = _noise((6, 9, 34), seed=7)
    r = np.random.default_rng(8).random(vol.shape)
    vol[r < 0.05], vol[(r >= 0.05) & (r < 0.10)], vol[(r >= 0.10) & (r < 0.15)] = np.inf, -np.inf, np.nan
    verts, _, _ = _check(cuda, vol)
    assert np.isfinite(verts).all()


def test_a_level_that_is_no_float_and_the_models_affine_map(cuda):
    vol = _noise((9, 10, 33), seed=9)
    _check(cuda, vol, level=0.1)
    _check(cuda, vol, level=-0.3)
    R, r = 32, 0.87
    _check(cuda, _smooth((R, R, R)), vert_div=R - 1.0, vert_mul=r - (-r), vert_add=-r)
    _check(cuda, vol, level=0.1, vert_div=R - 1.0, vert_mul=r - (-r), vert_add=-r)


def test_no_active_cell_raises(cuda):
    from sculptmate_amd import ops

    for value in (-1.0, 1.0, float("nan")):
        with pytest.raises(RuntimeError, match="surface_nets"):
            ops.surface_nets(torch.full((5, 6, 7), value, device=cuda))
    # and the next call is fine
    _check(cuda, _noise((5, 6, 7)))


@pytest.mark.parametrize("shape", [(32, 32, 32), (9, 33, 70)], ids=lambda s: "x".join(map(str, s)))
def test_sign_planes_give_the_same_bits(cuda, shape):
    for vol, level in ((_noise(shape, seed=2), 0.0), (_smooth(shape), 0.0), (_noise(shape, seed=2), 0.1)):
        planes = sn.sign_planes(vol, level)
        assert planes.shape == (shape[0] * shape[1], (shape[2] + 31) // 32)
        plain = _check(cuda, vol, level=level)
        signed = _check(cuda, vol, sign_planes=planes, level=level)
        assert all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
                   for a, b in zip(plain, signed))
        # rows longer than needed, and bits past n2 set: both are ignored
        wide = np.full((planes.shape[0], planes.shape[1] + 2), -1, np.int32)
        wide[:, :planes.shape[1]] = planes
        if shape[2] % 32:
            wide[:, planes.shape[1] - 1] |= np.int32(-1) << np.int32(shape[2] % 32)
        _check(cuda, vol, sign_planes=wide, level=level)


@pytest.fixture(scope="module")
def model(cuda):
    return _tsrmodel.small_model(cuda, 32, project_keys=True)


def _mesh_bits(mesh):
    return (mesh.vertices.cpu().numpy().view(np.uint32), mesh.faces.cpu().numpy(), None if mesh.quads is None else mesh.quads.cpu().numpy())


def test_filtered_grid_gives_the_bits_of_the_full_evaluation(model):
    m = model["m"]
    before = dict(m.filter_info)
    filtered = m.extract_meshes(model["codes"], isosurface="surface_nets", **model["kw"])[0]
    # a run the guard sent to the fallback does not test the claim
    assert m.filter_info["filtered"] == before["filtered"] + 1 and m.filter_info["fallbacks"] == before["fallbacks"]
    try:
        m.decoder_filter = False
        full = m.extract_meshes(model["codes"], isosurface="surface_nets", **model["kw"])[0]
    finally:
        m.decoder_filter = True
    assert m.filter_info["filtered"] == before["filtered"] + 1
    a, b = _mesh_bits(filtered), _mesh_bits(full)
    assert len(a[0]) > 1000 and a[2] is not None and a[1].dtype == np.int64 and a[2].dtype == np.int64
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # and the full evaluation is the restatement of its own volume
    from sculptmate_amd import ops

    cfg, R = m.renderer.cfg, 32
    vol = ops.density_grid(model["codes"][0].contiguous(), m.decoder, R, precision="bf16l3", radius=cfg.radius,
                           density_bias=cfg.density_bias, out_add=-model["threshold"]).view(R, R, R).cpu().numpy()
    want = sn.surface_nets(vol, 0.0, R - 1.0, cfg.radius - (-cfg.radius), -cfg.radius, index_dtype=np.int64)
    assert np.array_equal(b[0], want["verts"].view(np.uint32)) and np.array_equal(b[1], want["faces"]) and np.array_equal(b[2], want["quads"])


def test_chain_keeps_the_quads(model):
    from sculptmate_amd import ops

    m, kw = model["m"], model["kw"]
    base = m.extract_meshes(model["codes"], isosurface="surface_nets", **kw)[0]
    got = m.extract_meshes(model["codes"], isosurface="surface_nets", smooth=2, project=True, **kw)[0]
    assert got.quads is not None and torch.equal(got.quads, base.quads) and torch.equal(got.faces, base.faces)
    q, f = got.quads.cpu().numpy(), got.faces.cpu().numpy()
    assert len(f) == 2 * len(q)
    pairs = f.reshape(-1, 6)
    assert np.array_equal(np.array([np.unique(p) for p in pairs]), np.sort(q, axis=1))          # faces 2q, 2q + 1 are quad q
    assert (pairs[:, 0] == q[:, 0]).all() and (pairs[:, 1] == q[:, 1]).all() and (pairs[:, 5] == q[:, 3]).all()
    v = ops.mesh_smooth(base.vertices, base.faces, 2)
    steps, cells = ops.project_rule(True)
    v = ops.mesh_project(model["codes"][0].contiguous(), m.decoder, v, base.faces, model["target"], cells * model["cell"], steps=steps,
                         radius=model["radius"])[0]
    assert np.array_equal(got.vertices.cpu().numpy().view(np.uint32), v.cpu().numpy().view(np.uint32))
    for drop in (dict(keep_components="largest"), dict(simplify=0.5), dict(subdivide=1)):
        assert m.extract_meshes(model["codes"], isosurface="surface_nets", **drop, **kw)[0].quads is None


def test_the_default_is_untouched(model):
    m = model["m"]
    again = m.extract_meshes(model["codes"], **model["kw"])[0]
    named = m.extract_meshes(model["codes"], isosurface="marching_cubes", **model["kw"])[0]
    plain = model["plain"]
    for mesh in (again, named):
        assert mesh.quads is None
        assert np.array_equal(mesh.vertices.cpu().numpy().view(np.uint32), plain.vertices.cpu().numpy().view(np.uint32))
        assert torch.equal(mesh.faces, plain.faces)
