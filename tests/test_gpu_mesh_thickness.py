"""Wall thickness on the device (csrc/mesh_ray.hip sculpt_surface_thickness; ops.mesh_thickness / bake_thickness, Mesh.thickness,
TSR.bake_thickness_map): the fused kernel against the composed route and the NumPy restatement (tests/_thickref.py), bit for
bit in all three outputs; the odd points of the rule; the bake over small atlases; one end-to-end run on the small model."""
import numpy as np
import pytest
import torch

import _aomapref as A
import _thickref as TH
import _tsrmodel
from sculptmate_amd import ops
from test_gpu_bake_occlusion import _self_case
from test_gpu_mesh_distance import MESHES as DISTANCE_MESHES
from test_remesh import icosphere

pytestmark = pytest.mark.gpu

NAMES = ("thickness", "thinnest", "valid")


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _same(got, want, what):
    """The three outputs equal bit for bit, a NaN equal to any NaN."""
    assert len(got) == len(want)
    for g, w, part in zip(got, want, NAMES + ("mask",)):
        g, w = np.ascontiguousarray(_host(g)), np.ascontiguousarray(_host(w))
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, g.shape, w.dtype, w.shape)
        if g.dtype.kind == "f":
            bad = np.argwhere((g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w)))
        else:
            bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s %s: %d of %d differ, first at %r: %r vs %r" % (what, part, len(bad), g.size, tuple(bad[0]),
                                                                                 g[tuple(bad[0])], w[tuple(bad[0])])


def _nested():
    """The nested spheres of tests/test_gpu_mesh_ray.py: radius 1 (80 faces) inside an inverted sphere of radius 3 (320 faces)."""
    v1, f1 = icosphere(1)
    v2, f2 = icosphere(2)
    v = np.concatenate([v1, 3.0 * v2]).astype(np.float32)
    return v, np.concatenate([f1, f2[:, ::-1] + len(v1)]).astype(np.int32)


_meshes = {}


def _mesh_case(cuda, name):
    """(P, F, points, normals, offset or None) on the host, made once and shared, never modified; the normals of the two sphere
    cases are the device's own ops.vertex_normals, read back for the restatement."""
    if name not in _meshes:
        if name in ("cavity", "blob"):
            _meshes[name] = TH.nested_cubes_case(inverted=name == "cavity")
        else:
            P, F = DISTANCE_MESHES["sphere"]() if name == "sphere" else _nested()
            nrm = ops.vertex_normals(torch.from_numpy(P).to(cuda), torch.from_numpy(F).to(cuda)).cpu().numpy()
            _meshes[name] = (P, F, P, nrm, None)
    return _meshes[name]


def _default_offset(P, F):
    used = P[np.unique(F)].astype(np.float64)
    return np.float32(ops.OCCLUSION_OFFSET * float((used.max(0) - used.min(0)).max()))


_refs = {}


def _reference(cuda, name, k, far, cone, outward=1.0, seed=0):
    """The restatement's outputs for a case, computed once and shared, never modified."""
    key = (name, k, far, cone, outward, seed)
    if key not in _refs:
        P, F, pts, nrm, offset = _mesh_case(cuda, name)
        offset = _default_offset(P, F) if offset is None else offset
        _refs[key] = TH.thickness(pts, nrm, ops.thickness_directions(k, cone, seed), P, F, offset, np.inf if far is None else far, outward)
    return _refs[key]


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(cuda) for x in arrays]


# ------------------------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("cone", [60.0, 30.0])
@pytest.mark.parametrize("k,far", [(32, None), (32, 0.6), (1, None)])
@pytest.mark.parametrize("name", ["sphere", "nested", "cavity", "blob"])
def test_fused_composed_and_restatement_agree_bit_for_bit(cuda, name, k, far, cone):
    P, F, pts, nrm, offset = _mesh_case(cuda, name)
    want = _reference(cuda, name, k, far, cone)
    t = _dev(cuda, pts, nrm, P, F)
    kw = dict(thickness=(k, far), cone=cone, offset=None if offset is None else float(offset))
    fused = ops.mesh_thickness(*t, **kw)
    assert fused[0].dtype == torch.float32 and fused[1].dtype == torch.float32 and fused[2].dtype == torch.int32
    assert all(x.shape == (len(pts),) for x in fused)
    _same(fused, want, "%s fused vs restatement" % name)
    _same(ops.mesh_thickness_composed(*t, **kw), want, "%s composed vs restatement" % name)
    thick, thin, valid = want
    print("%s k=%d far=%r cone=%g: valid %d .. %d, thinnest %.4f .. %.4f" % (name, k, far, cone, valid.min(), valid.max(),
                                                                           thin.min(), thin[np.isfinite(thin)].max(initial=0)))
    if name == "sphere" and far is None:      # the polyhedron's chords; R = 1.  No closed form is claimed
        assert (valid == k).all() and (thin > 0).all() and (thick < 2.0).all()
        if k > 1:
            assert (thin <= thick).all()
        else:
            # one ray: thickness = fl(fl(w t) / w) is t up to the two roundings of the rule's own arithmetic, each 2^-24
            # relative, so it may come out an ulp BELOW thinnest (it does at some of the 162 points): the order of the two
            # holds to within those roundings, 2 ulp to be safe
            assert (np.abs(thick.astype(np.float64) - thin) <= 2.0 * np.spacing(thin)).all()
    if name == "sphere" and far is not None:  # every chord inside a 60 degree cone is longer than 2 R cos 60 = 1 > 0.6
        assert (valid == 0).all() and np.isinf(thick).all()
    if name == "cavity" and far is None:
        assert (valid == k).all()
    if name == "blob" and far is None and k == 32 and cone == 60.0:
        assert (valid >= 8).all() and (valid <= 16).all() and (thin > 0.45).all()


@pytest.mark.parametrize("name", ["nested", "blob"])
def test_outward_minus_one(cuda, name):
    """The sign of the back-face clause: with outward = -1 the rays that were dropped are the ones that count."""
    P, F, pts, nrm, offset = _mesh_case(cuda, name)
    want = _reference(cuda, name, 32, None, 60.0, outward=-1.0)
    t = _dev(cuda, pts, nrm, P, F)
    kw = dict(thickness=32, offset=None if offset is None else float(offset), outward=-1.0)
    _same(ops.mesh_thickness(*t, **kw), want, "%s outward=-1 fused" % name)
    _same(ops.mesh_thickness_composed(*t, **kw), want, "%s outward=-1 composed" % name)
    plus = _reference(cuda, name, 32, None, 60.0)
    assert not np.array_equal(plus[2], want[2])
    if name == "blob":
        assert np.array_equal(plus[2] + want[2], np.full(len(pts), 32, np.int32))    # every ray of this case hits a face


def test_a_seed_and_an_explicit_offset(cuda):
    P, F, pts, nrm, _ = _mesh_case(cuda, "sphere")
    t = _dev(cuda, pts, nrm, P, F)
    want = TH.thickness(pts, nrm, ops.thickness_directions(8, 45.0, 5), P, F, np.float32(0.01), 1.9)
    _same(ops.mesh_thickness(*t, thickness=(8, 1.9), cone=45.0, seed=5, offset=0.01), want, "seed/offset fused")
    _same(ops.mesh_thickness_composed(*t, thickness=(8, 1.9), cone=45.0, seed=5, offset=0.01), want, "seed/offset composed")
    # the default offset is 2^-13 of the longest side
    _same(ops.mesh_thickness(*t, thickness=8, offset=float(_default_offset(P, F))), ops.mesh_thickness(*t, thickness=8), "default offset")
    # fp64 inputs are converted first
    _same(ops.mesh_thickness(t[0].double(), t[1].double(), t[2].double(), t[3], thickness=8), ops.mesh_thickness(*t, thickness=8), "fp64")


# ------------------------------------------------------------------------------------------------- counts, order, dtypes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_point_counts_around_the_wave_and_block_sizes(cuda, n):
    P, F, pts, nrm, _ = _mesh_case(cuda, "sphere")
    want = _reference(cuda, "sphere", 32, None, 60.0)
    rows = np.arange(n) % len(pts)
    t = _dev(cuda, pts[rows], nrm[rows], P, F)
    got = ops.mesh_thickness(*t)
    assert all(x.shape == (n,) for x in got)
    _same(got, [w[rows] for w in want], "n=%d" % n)
    _same(ops.mesh_thickness_composed(*t), [w[rows] for w in want], "n=%d composed" % n)


def test_a_permutation_of_the_points_permutes_the_outputs(cuda):
    P, F, pts, nrm, _ = _mesh_case(cuda, "nested")
    want = _reference(cuda, "nested", 32, None, 60.0)
    perm = np.random.default_rng(3).permutation(len(pts))
    got = ops.mesh_thickness(*_dev(cuda, pts[perm], nrm[perm], P, F))
    _same(got, [w[perm] for w in want], "permuted")


def test_int64_faces(cuda):
    P, F, pts, nrm, _ = _mesh_case(cuda, "nested")
    want = _reference(cuda, "nested", 32, None, 60.0)
    p, n, v, f = _dev(cuda, pts, nrm, P, F)
    _same(ops.mesh_thickness(p, n, v, f.long()), want, "int64 fused")
    _same(ops.mesh_thickness_composed(p, n, v, f.long()), want, "int64 composed")


# ------------------------------------------------------------------------------------------------------------- odd points
def test_odd_points(cuda):
    P, F, _, _, _ = _mesh_case(cuda, "sphere")
    pts = np.array([[0, 0, 1], [np.nan, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 2.5], [0, 0, 1], [0, np.inf, 0]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 0], [0, np.inf, 0], [0, 0, -1], [3e38, 3e38, 0], [0, 0, 1]], np.float32)
    pts[0] = nrm[0] = P[0]                                          # an ordinary point: a vertex of the unit sphere, normal outwards
    p, n, v, f = _dev(cuda, pts, nrm, P, F)
    want = TH.thickness(pts, nrm, ops.thickness_directions(16, 60.0, 3), P, F, _default_offset(P, F))
    got = ops.mesh_thickness(p, n, v, f, thickness=16, seed=3)
    _same(got, want, "odd fused")
    _same(ops.mesh_thickness_composed(p, n, v, f, thickness=16, seed=3), want, "odd composed")
    thick, thin, valid = (_host(x) for x in got)
    assert valid.tolist() == [16, 0, 0, 0, 0, 0, 0]
    assert 0 < thin[0] < 2.0 and 0 < thick[0] < 2.0
    for i in (1, 3, 6):                                              # a non-finite position or normal
        assert np.isnan(thick[i]) and np.isnan(thin[i])
    for i in (2, 4, 5):                                              # a zero normal, a point outside the body, an overflowing normal
        assert thick[i] == np.inf and thin[i] == np.inf
    # a surface without faces: +inf, +inf, 0 (NaN still for the non-finite points); and no points at all
    for fn in (ops.mesh_thickness, ops.mesh_thickness_composed):
        thick, thin, valid = (_host(x) for x in fn(p, n, v, f[:0], thickness=16))
        assert (valid == 0).all() and np.isnan(thick[[1, 3, 6]]).all() and np.isnan(thin[[1, 3, 6]]).all()
        assert (thick[[0, 2, 4, 5]] == np.inf).all() and (thin[[0, 2, 4, 5]] == np.inf).all()
        none = fn(p[:0], n[:0], v, f)
        assert [x.shape for x in none] == [(0,)] * 3 and none[2].dtype == torch.int32 and none[0].dtype == torch.float32


def test_refusals(cuda):
    P, F, pts, nrm, _ = _mesh_case(cuda, "sphere")
    p, n, v, f = _dev(cuda, pts, nrm, P, F)
    for fn in (ops.mesh_thickness, ops.mesh_thickness_composed):
        with pytest.raises(ops.SculptError):
            fn(p.cpu(), n.cpu(), v.cpu(), f.cpu())
        with pytest.raises(ops.SculptError):
            fn(p.cpu(), n, v, f)
        with pytest.raises(ops.SculptError):
            fn(p, n[:-1], v, f)
        for kw in (dict(thickness=False), dict(thickness=(8, 0.0)), dict(thickness=2000), dict(cone=0.0), dict(cone=91.0),
                   dict(seed=-1), dict(seed=0.5), dict(outward=0.0)):
            with pytest.raises(ValueError):
                fn(p, n, v, f, **kw)


def test_the_route_switch(monkeypatch):
    monkeypatch.delenv("SCULPT_DISTANCE_FORM", raising=False)
    assert ops.mesh_thickness_route() is ops.mesh_thickness
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", "composedthickness")
    assert ops.mesh_thickness_route() is ops.mesh_thickness_composed


def test_the_mesh_method(cuda, monkeypatch):
    from sculptmate_amd.tsr.system import Mesh

    P, F, _, _, _ = _mesh_case(cuda, "nested")
    v, f = _dev(cuda, P, F)
    mesh = Mesh(v, f)
    for outward in (1.0, -1.0):
        normals = outward * ops.vertex_normals(v, f)
        want = ops.mesh_thickness(v, normals, v, f, thickness=(16, 2.5), cone=45.0, seed=2, outward=outward)
        _same(mesh.thickness((16, 2.5), cone=45.0, seed=2, outward=outward), want, "Mesh.thickness outward=%g" % outward)
    assert not hasattr(mesh, "vertex_thickness") and callable(mesh.thickness)      # returned, never stored
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", "composedthickness")
    _same(mesh.thickness(16), ops.mesh_thickness(v, ops.vertex_normals(v, f), v, f, thickness=16), "the composed route")
    with pytest.raises(ops.SculptError):
        Mesh(P, F).thickness()


# --------------------------------------------------------------------------------------------------- the bake, small atlases
@pytest.mark.parametrize("name", ["cube", "icosphere"])
def test_bake_without_a_source_equals_the_restatement(cuda, name):
    v, f, n, rast = _self_case(cuda, name, 64)
    covered = rast[..., 3] >= 0
    assert 0 < int(covered.sum()) < 64 * 64
    P, F = v.cpu().numpy(), f.cpu().numpy()
    want = TH.bake_thickness(rast.cpu().numpy(), P, F, n.cpu().numpy(), P, F, ops.thickness_directions(8, 60.0, 1), _default_offset(P, F))
    got = ops.bake_thickness(v, f, n, rast, thickness=8, seed=1)
    assert [x.dtype for x in got] == [torch.float32, torch.float32, torch.int32, torch.bool] and all(x.shape == (64, 64) for x in got)
    _same(got, want, "%s bake" % name)
    thick, thin, valid, mask = got
    assert torch.equal(mask, covered)
    for x in (thick, thin):
        assert bool((x[~mask] == 0).all()) and not bool(torch.signbit(x[~mask]).any())      # exactly +0
    assert bool((valid[~mask] == 0).all())
    # a closed convex body: a ray that starts inside leaves through a back face, unless it slips through an edge (watertightness
    # along edges is not promised), so most texels count every ray; a counted ray has a positive length (the origin lies
    # offset x cos(angle to the face normal) inside, far above the roundings)
    counted = mask & (valid > 0)
    assert float((valid[mask] == 8).float().mean()) > 0.5 and bool((thin[counted] > 0).all())
    print("%s: %d covered texels, thickness %.4f .. %.4f" % (name, int(mask.sum()), float(thick[mask].min()), float(thick[mask].max())))


_source = {}


def _source_case(scale):
    """The source-mode case of tests/test_gpu_bake_occlusion.py and its restatement, computed once and shared, never modified."""
    if scale not in _source:
        c = A.source_case(scale, k=8)
        c["want"] = TH.bake_thickness(c["rast"], c["V"], c["F"], c["N"], c["SP"], c["SF"], ops.thickness_directions(8, 60.0), c["offset"],
                                      np.inf, 1.0, c["cage_value"])
        _source[scale] = c
    return _source[scale]


@pytest.mark.parametrize("scale", [0.97, 1.03])
def test_bake_with_a_source_equals_the_restatement(cuda, scale):
    c = _source_case(scale)
    v, f, n, rast = _dev(cuda, c["V"], c["F"], c["N"], c["rast"])
    source = tuple(_dev(cuda, c["SP"], c["SF"]))
    got = ops.bake_thickness(v, f, n, rast, thickness=8, source=source, cage=c["cage"])
    _same(got, c["want"], "source bake, scale %g" % scale)
    thick, thin, valid, mask = got
    assert int(mask.sum()) > 100 and bool((thick[~mask] == 0).all()) and bool((valid[~mask] == 0).all())
    assert bool((valid[mask] > 0).any())
    # an explicit cage of the default's value, and the composed point route: the same bits
    _same(ops.bake_thickness(v, f, n, rast, thickness=8, source=source, cage=c["cage_value"]), c["want"], "explicit cage")
    with pytest.raises(ValueError):
        ops.bake_thickness(v, f, n, rast, cage=0.1)
    empty = ops.bake_thickness(v, f, n, rast[:0, :0], thickness=8)
    assert all(x.shape == (0, 0) for x in empty)
    none = ops.bake_thickness(v, f[:0], n, rast, thickness=8, source=source)
    assert not bool(none[3].any()) and bool((none[0] == 0).all()) and bool((none[2] == 0).all())


def test_bake_follows_the_route_switch(cuda, monkeypatch):
    v, f, n, rast = _self_case(cuda, "cube", 24)
    fused = ops.bake_thickness(v, f, n, rast, thickness=(8, 2.0))
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", "composedthickness")
    _same(ops.bake_thickness(v, f, n, rast, thickness=(8, 2.0)), fused, "bake, composed point route")


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def model(cuda):
    out = _tsrmodel.small_model(cuda, 32, enable_texture=True)
    m = out["m"]
    out["ekw"] = dict(enable_texture=True, resolution=32, threshold=out["threshold"], bake_texture=64, keep_components="largest")
    out["mesh"] = m.extract_meshes(out["codes"], **out["ekw"])[0]
    return out


def test_bake_thickness_map_end_to_end(model, tmp_path):
    from PIL import Image

    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr.thickness import ThicknessMap

    m, mesh = model["m"], model["mesh"]
    out, tmap = m.bake_thickness_map(mesh, thickness=8)
    assert out is mesh and isinstance(tmap, ThicknessMap) and tmap.rule == (8, None) and tmap.resolution == 64
    for x, dtype in ((tmap.thickness, torch.float32), (tmap.thinnest, torch.float32), (tmap.valid, torch.int32), (tmap.mask, torch.bool)):
        assert x.shape == (64, 64) and x.dtype == dtype and x.is_cuda
    # the coverage is the occlusion bake's over the same atlas
    v, f = mesh.vertices, mesh.faces
    rast = ops.bake_rasterize(mesh.uvs, torch.arange(3 * f.shape[0], device=v.device, dtype=torch.int32).view(-1, 3), 64)
    normals = (TSR.WINDING_OUTWARD * ops.vertex_normals(v, f)).contiguous()
    ao_mask = ops.bake_occlusion_composed(v, f, normals, rast, occlusion=1)[1]
    assert torch.equal(tmap.mask, ao_mask) and 0 < int(ao_mask.sum()) < 64 * 64
    inside = tmap.thickness[tmap.mask]
    finite = inside[torch.isfinite(inside)]
    assert finite.numel() > 0 and bool((finite > 0).all())
    assert 64 // 150 == 0 and bool((tmap.thickness[~tmap.mask] == 0).all())        # no round of padding at 64
    info = tmap.info()
    print("thickness map:", info)
    assert info["covered"] == int(ao_mask.sum()) and 0 <= info["no_valid_ray_share"] < 1 and 0 < info["valid_rays_per_texel"] <= 8
    # the map is the point query at the texels: the direct bake gives the same values
    direct = ops.bake_thickness(v, f, normals, rast, thickness=8, outward=TSR.WINDING_OUTWARD)
    _same((tmap.thickness, tmap.thinnest, tmap.valid, tmap.mask), direct, "map vs ops.bake_thickness")
    path = tmp_path / "thickness.png"
    tmap.save(path)
    back = Image.open(str(path))
    assert back.mode in ("I;16", "I;16B", "I") and np.array_equal(np.asarray(back).astype(np.uint16), tmap.image())
    # a second call gives the same bits
    again = m.bake_thickness_map(mesh, thickness=8)[1]
    _same((again.thickness, again.thinnest, again.valid, again.mask), (tmap.thickness, tmap.thinnest, tmap.valid, tmap.mask), "second call")
    # a mesh without uvs is unwrapped and comes back with them
    bare = m.extract_meshes(model["codes"], **dict(model["ekw"], bake_texture=0, enable_texture=False))[0]
    with_uvs, bare_map = m.bake_thickness_map(bare, resolution=48, thickness=4)
    assert bare.uvs is None and with_uvs.uvs is not None and torch.equal(with_uvs.vertices, bare.vertices) and bare_map.resolution == 48
    with pytest.raises(ValueError):
        m.bake_thickness_map(mesh, cage=0.1)
    with pytest.raises(ValueError):
        m.bake_thickness_map(mesh, thickness=0)


def test_the_model_setting_leaves_the_map_on_the_mesh(model):
    from sculptmate_amd.tsr.thickness import ThicknessMap

    m, plain = model["m"], model["mesh"]
    assert m.thickness_map is None and not isinstance(getattr(plain, "thickness"), ThicknessMap)
    try:
        m.thickness_map = 8
        auto = m.extract_meshes(model["codes"], **model["ekw"])[0]
        bare = m.extract_meshes(model["codes"], **dict(model["ekw"], bake_texture=0))[0]
        m.thickness_map = "thick"
        with pytest.raises(ValueError):
            m.extract_meshes(model["codes"], **model["ekw"])
    finally:
        m.thickness_map = None
    assert isinstance(auto.thickness, ThicknessMap) and auto.thickness.rule == (8, None) and auto.thickness.resolution == 64
    assert not isinstance(bare.thickness, ThicknessMap)                       # no texture bake, no map
    for key in ("vertices", "faces", "uvs", "texture"):                       # everything else is what it was
        a, b = getattr(auto, key), getattr(plain, key)
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                  b.view(torch.int32) if b.dtype == torch.float32 else b), key
    explicit = m.bake_thickness_map(plain, thickness=8)[1]
    _same((auto.thickness.thickness, auto.thickness.thinnest, auto.thickness.valid, auto.thickness.mask),
          (explicit.thickness, explicit.thinnest, explicit.valid, explicit.mask), "model setting vs explicit call")
