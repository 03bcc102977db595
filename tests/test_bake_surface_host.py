"""The bake at the surface without a GPU: the names and defaults it adds, what it refuses before any device or weight is looked
at, and the fp64 run of its NumPy restatement (tests/_surfbakeref.py) on the texels of the octahedron's atlas over the smoke
field.  tests/test_gpu_bake_surface.py then holds the device to the composed route bit for bit."""
import inspect

import numpy as np
import pytest

import _nmapref as N
import _projref as P
import _surfbakeref as S


def test_api_surface():
    import torch

    from sculptmate_amd import ops
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr import mesh
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import TSR

    assert TSR(SMALL_CFG).bake_project is None and TSR.__new__(TSR).bake_project is None
    assert TripoGenerator(torch.device("cpu")).bake_project is None
    assert len(mesh.FIELDS) == 12
    for fn in (ops.bake_scene_surface, ops.bake_scene_surface_composed):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["planes", "mlp", "v_pos", "faces", "rast", "target", "max_dist", "steps", "res_tol", "radius",
                                        "frame", "want"]
        d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
        assert d == {"steps": ops.PROJECT_STEPS, "res_tol": ops.PROJECT_RES_TOL, "radius": 0.87, "frame": None, "want": ()}
    sig = inspect.signature(TSR.bake_surface_maps)
    assert list(sig.parameters) == ["self", "mesh", "scene_code", "threshold", "project", "resolution", "atlas_resolution", "texture",
                                    "normal_map", "island_padding", "unwrapper"]
    d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == {"threshold": 25.0, "project": True, "resolution": None, "atlas_resolution": None, "texture": True,
                 "normal_map": "tangent", "island_padding": 0.02, "unwrapper": None}


def test_the_route_switch(monkeypatch):
    """The composed route is the default: the fused kernel did not meet the rule of DESIGN.md 3.1e on the flagship atlas
    (3.1g has the figures).  One new token of the existing switch selects the fused kernel."""
    from sculptmate_amd import ops

    monkeypatch.delenv("SCULPT_DISTANCE_FORM", raising=False)
    assert ops.bake_surface_route() is ops.bake_scene_surface_composed
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", "plain,fusedsurface")
    assert ops.bake_surface_route() is ops.bake_scene_surface
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", "plain")
    assert ops.bake_surface_route() is ops.bake_scene_surface_composed


@pytest.mark.parametrize("kw", [dict(project=False), dict(project=None), dict(project=0), dict(project=65), dict(project=(8, 0.0)),
                                dict(project="8"), dict(normal_map="world"), dict(normal_map=True),
                                dict(texture=False, normal_map=None), dict(threshold=0.0)])
def test_bake_surface_maps_refuses_before_anything_is_looked_at(kw):
    """No weights, no device, not even an initialised model: the ValueError comes first."""
    from sculptmate_amd.tsr.system import TSR, Mesh

    v, f = N.octahedron()
    with pytest.raises(ValueError):
        TSR.__new__(TSR).bake_surface_maps(Mesh(v, f), None, **kw)


def test_extract_meshes_refuses_a_bad_bake_project_before_anything_is_launched():
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import TSR

    m = TSR(SMALL_CFG)
    m.bake_project = (8, 0.0)
    with pytest.raises(ValueError):
        m.extract_meshes([None], enable_texture=True, bake_texture=64)


def test_cpu_tensors_and_bad_parameters_are_refused():
    import torch

    from sculptmate_amd import ops

    v, f = N.octahedron()
    planes, rast = torch.zeros((3, 40, 8, 8)), torch.zeros((4, 4, 4))
    for fn in (ops.bake_scene_surface, ops.bake_scene_surface_composed):
        with pytest.raises(ops.SculptError):
            fn(planes, None, torch.from_numpy(v), torch.from_numpy(f), rast, 4.2, 0.05)
        with pytest.raises(ops.SculptError, match="unknown output"):
            fn(planes, None, torch.from_numpy(v), torch.from_numpy(f), rast, 4.2, 0.05, want=("points",))
        for bad in (dict(steps=-1), dict(steps=65), dict(steps=1.0), dict(res_tol=0.0), dict(res_tol=float("nan"))):
            with pytest.raises(ValueError):
                fn(planes, None, torch.from_numpy(v), torch.from_numpy(f), rast, 4.2, 0.05, **bad)
        for target, max_dist in ((float("nan"), 0.05), (4.2, 0.0), (4.2, float("inf"))):
            with pytest.raises(ValueError):
                fn(planes, None, torch.from_numpy(v), torch.from_numpy(f), rast, target, max_dist)


def test_covered_texels_is_the_coverage_rule_of_the_kernels():
    """ops._covered_texels, the one torch statement of texel_position's coverage (csrc/bake_texel.h), on CPU tensors: a 4 x 4
    rast over 4 vertices and 2 faces whose tri holds -1, NaN, 2^31, nf, other values out of range, fractions (the kernel
    truncates) and valid faces; a face that names vertex nv, one that names vertex -1; no face; no vertex.  The masks are
    written out by hand."""
    import torch

    from sculptmate_amd import ops

    nan, inf = float("nan"), float("inf")
    tri = torch.tensor([[0.0, 1.0, -1.0, nan],
                        [2.0 ** 31, 2.0, 0.0, 1.0],
                        [1.9, -0.5, inf, 0.0],
                        [-inf, 3.0, 1.0, 0.0]])
    rast = torch.cat([torch.tensor([0.2, 0.3, 0.5]).expand(4, 4, 3), tri[..., None]], -1)
    v = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    T, F = True, False
    cases = [
        ([[0, 1, 2], [0, 2, 3]], v, [[T, T, F, F], [F, F, T, T], [T, F, F, T], [F, F, T, T]]),
        ([[0, 1, 2], [0, 2, 4]], v, [[T, F, F, F], [F, F, T, F], [F, F, F, T], [F, F, F, T]]),    # face 1 names vertex nv
        ([[-1, 1, 2], [0, 2, 3]], v, [[F, T, F, F], [F, F, F, T], [T, F, F, F], [F, F, T, F]]),   # face 0 names vertex -1
        ([], v, [[F] * 4] * 4),                                                                   # nf == 0
        ([[0, 1, 2], [0, 2, 3]], v[:0], [[F] * 4] * 4),                                           # nv == 0
    ]
    for faces, verts, want in cases:
        for dtype in (torch.int32, torch.int64):
            f = torch.tensor(faces, dtype=dtype).reshape(-1, 3)
            covered, clean = ops._covered_texels(rast, verts, f)
            want_t = torch.tensor(want)
            assert covered.dtype == torch.bool and torch.equal(covered, want_t)
            assert clean.is_contiguous() and torch.equal(clean[want_t], rast[want_t])
            assert torch.equal(clean[~want_t], torch.tensor([0.0, 0.0, 0.0, -1.0]).expand(int((~want_t).sum()), 4))


@pytest.fixture(scope="module")
def octahedron_bake():
    """The fp64 run of the restatement on the octahedron's cell atlas at 37^2 over the smoke field (decoder seed 1,
    synth.smooth_triplane(seed=2, scale=3.0), the calibrated bias of _projref.mesh_set_a): steps = 8, max_dist = 2 cells of the
    32^3 lattice, res_tol = 1e-3; and the steps = 0 run beside it."""
    from oracle import capi

    a = P.mesh_set_a()
    v, f = N.octahedron()
    uv = N.cell_atlas(v, f)
    rast = capi.bake_rasterize(uv, np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3), 37)
    vc = v[f].reshape(-1, 3)                                  # per corner, as the rasterised indices name them
    fc = np.arange(3 * len(f)).reshape(-1, 3)
    cn = N.vertex_normals(v, f)[f.reshape(-1)]
    ct = N.corner_tangents(v, f, uv, cn)
    args = (a["planes"], a["Ws"], a["bs"], vc, fc, rast, a["target"])
    max_dist, tol = 2.0 * a["cell"], 1e-3
    out = S.bake_surface(*args, 8, max_dist, tol, np.float64, frame=(cn, ct))
    world = S.bake_surface(*args, 8, max_dist, tol, np.float64)
    start = S.bake_surface(*args, 0, max_dist, tol, np.float64)
    return dict(out=out, world=world, start=start, max_dist=max_dist, tol=tol, rast=rast, cn=cn, ct=ct, cell=a["cell"])


def test_fp64_rule_on_the_octahedron(octahedron_bake):
    b = octahedron_bake
    out, start, m = b["out"], b["start"], b["out"]["mask"]
    assert 0 < m.sum() < m.size and np.array_equal(m, b["rast"][..., 3] >= 0)
    r, r0 = np.abs(out["residual"][m]), np.abs(start["residual"][m])
    moved = np.linalg.norm(out["point"][m] - out["p0"], axis=1)
    hist = np.bincount(out["status"][m], minlength=4)
    print("octahedron 37^2: %d covered texels; median |d - t| %.3e -> %.3e; status histogram %s; mean evals %.2f; displacement "
          "median %.3f cell, largest %.3f cell" % (m.sum(), np.median(r0), np.median(r), hist.tolist(), out["evals"][m].mean(),
                                                    np.median(moved) / b["cell"], moved.max() / b["cell"]))
    assert np.array_equal(start["point"][m], out["p0"]) and (start["evals"][m] == 1).all()       # steps = 0: the texel's own point
    assert (r <= r0).all()                                         # never worse than the start
    # the trust region in the rule's own arithmetic: (dx dx + dy dy) + dz dz against the square of max_dist as the kernel sees it
    dl = out["point"][m] - out["p0"]
    d2 = (dl[:, 0] * dl[:, 0] + dl[:, 1] * dl[:, 1]) + dl[:, 2] * dl[:, 2]
    md = np.float64(np.float32(b["max_dist"]))
    assert (d2 <= md * md).all()
    assert (r[out["status"][m] == 0] <= np.float32(b["tol"])).all()
    assert (out["evals"][m] >= 1).all() and (out["evals"][m] <= 9).all()
    # uncovered texels: exact zeros, status -1
    for key in ("point", "normal", "residual", "evals"):
        assert not out[key][~m].any()
    assert (out["status"][~m] == -1).all()


def test_fp64_normals_are_unit_and_the_frame_transform_decodes_to_them(octahedron_bake):
    b = octahedron_bake
    m = b["out"]["mask"]
    world, stored = b["world"]["normal"][m], b["out"]["normal"][m]
    ok = b["out"]["status"][m] != 3
    assert ok.all()                                                # the octahedron lies inside the box: every texel has a gradient
    assert np.abs(np.linalg.norm(world, axis=1) - 1).max() <= 1e-12
    r = b["rast"][m]
    back = N.decode(stored, r[:, :3], r[:, 3].astype(np.int64), b["cn"], b["ct"])
    assert N.angle(back, world).max() <= 1e-9
    # how much the projection changes the map: the normal at the projected point against the one at the texel's own point
    turned = N.angle(world, b["start"]["normal"][m])
    print("angle between the normal at p0 and at the projected point: median %.4f rad, 95th percentile %.4f rad" % (
        np.median(turned), np.percentile(turned, 95)))
    assert np.isfinite(turned).all() and turned.max() > 0
