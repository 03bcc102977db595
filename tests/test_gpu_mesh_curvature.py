"""Discrete curvature on the device (csrc/mesh_curvature.hip; ops.mesh_curvature_terms / curvature_ring / mesh_curvature /
surface_attribute_at / bake_curvature, Mesh.curvature, TSR.bake_curvature_map) against the NumPy restatement
(tests/_curvref.py): bit for bit wherever the arithmetic is + - x / sqrt, within n 2^-47 where it goes through atan2."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _curvref as C
import _tsrmodel
from sculptmate_amd import _lib, ops
from test_gpu_bake_occlusion import _same

pytestmark = pytest.mark.gpu

CASES = [(name, perm) for name in C.MESHES for perm in (False, True)]
IDS = ["%s%s" % (name, "-permuted" if perm else "") for name, perm in CASES]
_runs = {}


def _dev(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def _np(x):
    return x.detach().cpu().numpy()


def _run(cuda, name, perm):
    """The mesh, the restatement's terms and the device's, computed once and shared, never modified."""
    key = (name, perm)
    if key not in _runs:
        V, F = C.MESHES[name]()
        if perm:
            F = C.permuted(F, seed=len(name))
        v, f = _dev(V, cuda), _dev(F, cuda)
        r = dict(V=V, F=F, v=v, f=f, ref=C.terms(V, F), dev=ops.mesh_curvature_terms(v, f), table=C.neighbour_csr(F, len(V)))
        _runs[key] = r
    return _runs[key]


# ------------------------------------------------------------------------------------------------------------ 1. terms
@pytest.mark.parametrize("name, perm", CASES, ids=IDS)
def test_terms(cuda, name, perm):
    r = _run(cuda, name, perm)
    area, deficit, hint, valid, n = r["ref"]
    d_area, d_deficit, d_hint, d_valid = r["dev"]
    assert d_valid.dtype == torch.bool and d_area.dtype == d_deficit.dtype == d_hint.dtype == torch.float64
    assert np.array_equal(_np(d_valid), valid)
    if perm:    # the order of the faces is part of the rule for the values, not for what is valid
        assert np.array_equal(valid, _run(cuda, name, False)["ref"][3])
    _same(d_area, area, "area")
    _same(d_hint, hint, "hint")
    diff = np.abs(_np(d_deficit) - deficit)
    print("%s: deficit differs from the host's by at most %.2f ulp of pi (2^-51), %d valid of %d"
          % (name, float(diff.max()) / 2.0 ** -51 if diff.size else 0.0, int(valid.sum()), len(valid)))
    assert (diff <= n * 2.0 ** -47).all()
    assert not _np(d_deficit)[~valid].any() and not _np(d_area)[~valid].any()
    if name == "stretched":   # both obtuse branches are taken at the vertices that count
        c = C.corner_terms(r["V"], r["F"])
        at_valid = valid[np.asarray(r["F"]).reshape(-1)]
        assert (c["obtuse_here"] & at_valid).any() and (c["obtuse_elsewhere"] & at_valid).any()
    if name == "double_cone":
        assert n.max() == 70 and valid.all()
    if name == "zero_area":
        assert (n < np.bincount(np.asarray(r["F"]).reshape(-1), minlength=len(valid))).any()


def test_outward_flips_the_sign_of_the_hint_only(cuda):
    r = _run(cuda, "icosphere2", False)
    area, deficit, hint, valid = ops.mesh_curvature_terms(r["v"], r["f"].long(), outward=-1.0)   # int64 faces too
    _same(area, r["dev"][0], "area")
    _same(deficit, r["dev"][1], "deficit")
    _same(hint, -r["dev"][2], "hint")
    assert (r["dev"][2] > 0).all()


# ------------------------------------------------------------------------------------------------------------ 2. rings
@pytest.mark.parametrize("name, perm", CASES, ids=IDS)
def test_rings(cuda, name, perm):
    from sculptmate_amd.sf3d import remesh_device as rmd

    r = _run(cuda, name, perm)
    start, nb, fixed = rmd._smooth_table(rmd._Ctx(), r["f"], len(r["V"]))
    assert np.array_equal(_np(start), r["table"][0]) and np.array_equal(_np(nb), r["table"][1])
    area, deficit, hint, valid = (_np(t) for t in r["dev"])
    for rounds in (1, 2, 8):
        got = ops.curvature_ring(r["dev"], start, nb, rounds)
        want = C.ring([area, deficit, hint], valid, r["table"][0], r["table"][1], rounds)
        for g, w, what in zip(got[:3], want, ("area", "deficit", "hint")):
            _same(g, w, "%s after %d rounds" % (what, rounds))
        assert torch.equal(got[3], r["dev"][3])
    same = ops.curvature_ring(r["dev"], start, nb, 0)
    for g, w in zip(same[:3], r["dev"][:3]):
        _same(g, w, "no round")


# ------------------------------------------------------------------------------------------------------------ 3. finish
@pytest.mark.parametrize("name, perm", CASES, ids=IDS)
def test_finish(cuda, name, perm):
    from sculptmate_amd.sf3d import remesh_device as rmd

    r = _run(cuda, name, perm)
    area, deficit, hint, valid, n = r["ref"]
    start, nb, _ = rmd._smooth_table(rmd._Ctx(), r["f"], len(r["V"]))
    for rings in (0, 3):
        mean, gauss, ok = ops.mesh_curvature(r["v"], r["f"], rings)
        assert mean.dtype == gauss.dtype == torch.float32 and ok.dtype == torch.bool and np.array_equal(_np(ok), valid)
        d_area, d_deficit, d_hint, _ = (_np(t) for t in ops.curvature_ring(r["dev"], start, nb, rings))
        want_mean, want_gauss = C.finish(d_area, d_deficit, d_hint, valid)
        _same(mean, want_mean, "mean, rings=%d" % rings)
        _same(gauss, want_gauss, "gauss, rings=%d" % rings)
        assert np.isnan(_np(mean)[~valid]).all() and np.isnan(_np(gauss)[~valid]).all()
    mean, gauss, _ = ops.mesh_curvature(r["v"], r["f"], True)
    ref_mean, ref_gauss = C.finish(area, deficit, hint, valid)
    _same(mean, ref_mean, "mean against the whole restatement")
    g, w = _np(gauss)[valid].astype(np.float64), ref_gauss[valid].astype(np.float64)
    bound = n[valid] * 2.0 ** -47 / area[valid] + np.spacing(np.abs(ref_gauss[valid])).astype(np.float64)
    assert (np.abs(g - w) <= bound).all()


def test_principal_curvatures_on_the_device(cuda):
    r = _run(cuda, "torus", False)
    mean, gauss, _ = ops.mesh_curvature(r["v"], r["f"])
    k1, k2 = ops.principal_curvatures(mean, gauss)
    w1, w2 = C.principal(_np(mean), _np(gauss))
    _same(k1, w1, "k1")
    _same(k2, w2, "k2")


# ------------------------------------------------------------------------------------------------------------ 4. attribute
def test_surface_attribute_at(cuda):
    V, F = C.icosphere(2)
    P = V.astype(np.float64)
    rng = np.random.default_rng(3)
    t = rng.integers(0, len(F), 64)
    a, b, c = P[F[t, 0]], P[F[t, 1]], P[F[t, 2]]
    g = np.cross(b - a, c - a)
    centre = (a + b + c) / 3
    pts = np.concatenate([a, c, (a + b) / 2, (b + c) / 2, centre, centre + 0.01 * g, centre - 0.02 * g,
                          a + 1.5 * (a - centre), (a + b) / 2 + ((a + b) / 2 - c)]).astype(np.float32)     # off the face: the clamp
    face = np.tile(t, 9).astype(np.int32)
    face[::7] = -1
    values = rng.standard_normal((len(V), 3)).astype(np.float32)
    values[F[t[:8], 1], 0] = np.nan                       # one NaN corner
    values[F[t[8:12]].reshape(-1), 1] = np.nan            # all three
    values[F[t[12], 0], 2] = np.inf
    want = C.attribute_at(pts, face, V, F, values)
    listed = face >= 0
    centroids = np.arange(4 * 64, 5 * 64)[listed[4 * 64:5 * 64]]
    assert not np.isnan(want[centroids[centroids < 4 * 64 + 8], 0]).any()      # one NaN corner does not blank the point
    assert np.isnan(want[listed, 1]).any() and not np.isnan(want[listed, 1]).all()   # three do
    assert np.isnan(want[~listed]).all() and (~np.isnan(want[:, 0])).sum() > 300
    v, f = _dev(V, cuda), _dev(F, cuda)
    got = ops.surface_attribute_at(_dev(pts, cuda), _dev(face, cuda), v, f, _dev(values, cuda))
    _same(got, want, "three channels")
    _same(ops.surface_attribute_at(_dev(pts, cuda), _dev(face.astype(np.int64), cuda), v, f.long(), _dev(values[:, 2].copy(), cuda)),
          want[:, 2].copy(), "one flat channel, int64 indices")
    wide = rng.standard_normal((len(V), 8)).astype(np.float32)
    _same(ops.surface_attribute_at(_dev(pts, cuda), _dev(face, cuda), v, f, _dev(wide, cuda)), C.attribute_at(pts, face, V, F, wide), "eight")
    assert ops.surface_attribute_at(_dev(pts[:0], cuda), _dev(face[:0], cuda), v, f, _dev(values, cuda)).shape == (0, 3)
    with pytest.raises(ops.SculptError):
        ops.surface_attribute_at(_dev(pts, cuda), _dev(face, cuda), v, f, _dev(np.zeros((len(V), 9), np.float32), cuda))
    with pytest.raises(ops.SculptError):
        ops.surface_attribute_at(_dev(pts, cuda), _dev(face[:5], cuda), v, f, _dev(values, cuda))


# ------------------------------------------------------------------------------------------------------------ 5. the bake
def _box_atlas(cuda, V, F, res):
    from sculptmate_amd.sf3d.unwrap import BoxProjectionUnwrapper

    v, f = _dev(V, cuda), _dev(F, cuda)
    normals = ops.vertex_normals(v, f).contiguous()
    uv, corner = BoxProjectionUnwrapper()(v, normals, f, 0.02)
    uv = uv.to(torch.float32)[corner.reshape(-1).long()].contiguous()
    rast = ops.bake_rasterize(uv, torch.arange(3 * f.shape[0], device=cuda, dtype=torch.int32).view(-1, 3), res)
    return v, f, normals, rast


def _own_texels(v, f, rast, mean, gauss):
    """bake_interpolate of the per-vertex values with the NaN rule, on the host from the device's own interpolation."""
    ok = ~(torch.isnan(mean) | torch.isnan(gauss))
    attr = torch.stack([torch.nan_to_num(mean, nan=0.0), torch.nan_to_num(gauss, nan=0.0), ok.float()], 1).contiguous()
    img = _np(ops.bake_interpolate(attr, rast, f))
    tri = _np(rast[..., 3]).astype(np.int64)
    cov = tri >= 0
    n = _np(ok)[_np(f)[np.where(cov, tri, 0)]].sum(-1)
    out = []
    with np.errstate(all="ignore"):
        for ch in (0, 1):
            x = np.where(n == 3, img[..., ch], np.where(n == 0, np.float32(np.nan), img[..., ch] / img[..., 2]))
            out.append(np.where(cov, x, np.float32(0)).astype(np.float32))
    return out[0], out[1], cov, n


@pytest.mark.parametrize("name", ["icosphere1", "stretched"])
def test_bake_curvature_of_the_mesh_itself(cuda, name):
    V, F = C.icosphere(1) if name == "icosphere1" else C.stretched_grid()
    v, f, normals, rast = _box_atlas(cuda, V, F, 32)
    for rings in (True, 2):
        mean, gauss, mask = ops.bake_curvature(v, f, normals, rast, curvature=rings)
        H, K, _ = ops.mesh_curvature(v, f, rings)
        want_mean, want_gauss, cov, n = _own_texels(v, f, rast, H, K)
        assert mask.dtype == torch.bool and np.array_equal(_np(mask), cov) and 50 < cov.sum() < 32 * 32
        _same(mean, want_mean, "mean")
        _same(gauss, want_gauss, "gauss")
        assert not _np(mean)[~cov].any() and not _np(gauss)[~cov].any()       # exactly 0 where not covered
    if name == "stretched":      # the border's NaN: texels with one or two corners that count, and with none
        assert ((n == 0) & cov).any() and (((n == 1) | (n == 2)) & cov).any() and ((n == 3) & cov).any()
        assert np.isnan(_np(mean)[(n == 0) & cov]).all() and not np.isnan(_np(mean)[(n > 0) & cov]).any()
    empty = ops.bake_curvature(v, f, normals, rast[:0, :0].contiguous())
    assert [tuple(x.shape) for x in empty] == [(0, 0)] * 3


def test_bake_curvature_of_a_source(cuda):
    V, F = C.icosphere(1)
    SV, SF = C.icosphere(3, 1.01)
    v, f, normals, rast = _box_atlas(cuda, V, F, 32)
    source = (_dev(SV, cuda), _dev(SF, cuda))
    mean, gauss, mask = ops.bake_curvature(v, f, normals, rast, curvature=1, source=source)
    # the composition: the mesh's own texels, the snap with its faces, the source's values at the snapped points
    H, K, _ = ops.mesh_curvature(v, f, 1)
    own_mean, own_gauss, cov, _ = _own_texels(v, f, rast, H, K)
    SH, SK, _ = ops.mesh_curvature(*source, 1)
    index = ops._SurfaceIndex(*ops._surface(source[0], source[1], "test"))
    cage = float(np.float32(ops.OCCLUSION_CAGE * index.longest_side()))
    at = torch.nonzero(_dev(cov, cuda).reshape(-1))[:, 0]
    pts = ops.bake_interpolate(v, rast, f).reshape(-1, 3)[at].contiguous()
    nr = ops.bake_interpolate(normals, rast, f).reshape(-1, 3)[at].contiguous()
    q, _, hit, face = ops._snap_composed(index, pts, nr, cage, want_stats=True, want_face=True)
    assert torch.equal(hit, face >= 0) and 0 < int(hit.sum()) < len(at)          # some texels snap, some fall back
    hk = _np(ops.surface_attribute_at(q, face, source[0], source[1], torch.stack([SH, SK], 1).contiguous()))
    want_mean, want_gauss = own_mean.reshape(-1).copy(), own_gauss.reshape(-1).copy()
    at_h, hit_h = _np(at), _np(hit)
    want_mean[at_h[hit_h]], want_gauss[at_h[hit_h]] = hk[hit_h, 0], hk[hit_h, 1]
    assert np.array_equal(_np(mask), cov)
    _same(mean.reshape(-1), want_mean, "mean")
    _same(gauss.reshape(-1), want_gauss, "gauss")
    assert not _np(mean)[~cov].any() and not _np(gauss)[~cov].any()
    # a cage that reaches nothing: every texel falls back to the mesh's own value
    small = ops.bake_curvature(v, f, normals, rast, curvature=1, source=source, cage=1e-4)
    _same(small[0], own_mean, "all fall back")


# ------------------------------------------------------------------------------------------------------------ 6. errors
def test_errors(cuda):
    V, F = C.icosphere(0)
    v, f = _dev(V, cuda), _dev(F, cuda)
    bad_f = f.clone()
    bad_f[3, 1] = 12
    rep_f = f.clone()
    rep_f[2, 2] = rep_f[2, 0]
    bad_v = v.clone()
    bad_v[4, 1] = math.inf
    for vv, ff in ((v, bad_f), (v, rep_f), (bad_v, f), (v.cpu(), f), (v, f.cpu()), (v, f.float())):
        for call in (ops.mesh_curvature, ops.mesh_curvature_terms):
            with pytest.raises(ops.SculptError):
                call(vv, ff)
    for kw in (dict(curvature=9), dict(curvature=False), dict(curvature=1.0), dict(outward=0.5), dict(outward=float("nan"))):
        with pytest.raises(ValueError):
            ops.mesh_curvature(v, f, **kw)
    terms = ops.mesh_curvature_terms(v, f)
    start, nb = (_dev(x.astype(np.int32), cuda) for x in C.neighbour_csr(F, len(V)))
    with pytest.raises(ValueError):
        ops.curvature_ring(terms, start, nb, 9)
    with pytest.raises(ops.SculptError):
        ops.curvature_ring(terms, start[:-1].contiguous(), nb, 1)
    # the C entries refuse on their own
    lib, null, stream = _lib.lib, ctypes.c_void_p(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    topo = _lib.RmdTopo()
    assert lib.sculpt_curvature_terms(ctypes.byref(topo), null, 0.5, null, null, null, null, null, stream) != 0
    assert "outward" in _lib.last_error()
    assert lib.sculpt_curvature_terms(None, null, 1.0, null, null, null, null, null, stream) != 0
    assert lib.sculpt_curvature_ring(null, null, null, 4, 0, 9, null, null, null, null, null, null, null, null, stream) != 0
    assert "rounds" in _lib.last_error()
    assert lib.sculpt_curvature_ring(null, null, null, 4, 0, 1, null, null, null, null, null, null, null, null, stream) != 0   # null arrays
    assert lib.sculpt_curvature_ring(null, null, null, 1 << 31, 0, 1, null, null, null, null, null, null, null, null, stream) != 0
    assert lib.sculpt_curvature_finish(null, null, null, null, 4, null, null, stream) != 0
    assert lib.sculpt_curvature_finish(null, null, null, null, -1, null, null, stream) != 0
    assert lib.sculpt_surface_attribute_at(null, null, 4, null, null, 0, 0, null, 1, null, stream) != 0
    assert lib.sculpt_surface_attribute_at(null, null, 0, null, null, 0, 0, null, 9, null, stream) != 0
    # no faces: NaN and nothing valid; no vertices: empty
    mean, gauss, valid = ops.mesh_curvature(v, f[:0])
    assert np.isnan(_np(mean)).all() and np.isnan(_np(gauss)).all() and not valid.any() and mean.shape == (12,)
    area, deficit, hint, valid = ops.mesh_curvature_terms(v, f[:0])
    assert not area.any() and not hint.any() and not valid.any() and area.dtype == torch.float64
    assert ops.mesh_curvature(v[:0], f[:0])[0].shape == (0,)


# ------------------------------------------------------------------------------------------------------------ 7. end to end
@pytest.fixture(scope="module")
def model(cuda):
    out = _tsrmodel.small_model(cuda, 32, enable_texture=True)
    m = out["m"]
    out["ekw"] = dict(enable_texture=True, resolution=32, threshold=out["threshold"], bake_texture=64, keep_components="largest")
    out["mesh"] = m.extract_meshes(out["codes"], **out["ekw"])[0]
    return out


def test_mesh_curvature_end_to_end(model):
    from sculptmate_amd.sf3d import remesh_device as rmd
    from sculptmate_amd.tsr import TSR

    mesh = model["mesh"]
    nv = mesh.vertices.shape[0]
    mean, gauss, valid = mesh.curvature(outward=TSR.WINDING_OUTWARD)
    assert mean.shape == gauss.shape == valid.shape == (nv,) and valid.dtype == torch.bool and valid.any()
    fixed = rmd._smooth_table(rmd._Ctx(), mesh.faces.to(torch.int32).contiguous(), nv)[2]
    assert not valid[fixed.bool()].any()                      # whatever the smoothing filter holds fixed is invalid here
    assert torch.isfinite(mean[valid]).all() and torch.isnan(mean[~valid]).all()
    smooth = mesh.curvature(4, outward=TSR.WINDING_OUTWARD)
    assert torch.equal(smooth[2], valid)
    with pytest.raises(ValueError):
        mesh.curvature(9)


def test_bake_curvature_map_end_to_end(model, tmp_path):
    from PIL import Image

    from sculptmate_amd.tsr.curvature import CurvatureMap

    m, mesh = model["m"], model["mesh"]
    out, cmap = m.bake_curvature_map(mesh, curvature=2)
    assert out is mesh and isinstance(cmap, CurvatureMap) and cmap.rule == 2 and cmap.resolution == 64
    for x, dtype in ((cmap.mean, torch.float32), (cmap.gauss, torch.float32), (cmap.mask, torch.bool)):
        assert x.shape == (64, 64) and x.dtype == dtype and x.is_cuda
    img = cmap.image()
    assert img.dtype == np.uint16 and img.shape == (64, 64)
    reached = _np(cmap.mask) | (_np(cmap.mean) != 0) | (_np(cmap.gauss) != 0)
    assert (~reached).any() and (img[~reached] == 32768).all() and (cmap.image(which="gauss")[~reached] == 32768).all()
    assert len(np.unique(img[_np(cmap.mask)])) > 16
    path = tmp_path / "curvature.png"
    cmap.save(path)
    back = Image.open(str(path))
    assert np.array_equal(np.asarray(back).astype(np.uint16), img)
    again = m.bake_curvature_map(mesh, curvature=2)[1]
    _same(again.mean, cmap.mean, "second call")
    _same(again.gauss, cmap.gauss, "second call")
    assert cmap.info()["covered"] == int(cmap.mask.sum())
    with pytest.raises(ValueError):
        m.bake_curvature_map(mesh, cage=0.1)
    with pytest.raises(ValueError):
        m.bake_curvature_map(mesh, curvature=False)


def test_the_model_setting_leaves_the_map_on_the_mesh(model):
    from sculptmate_amd.tsr.curvature import CurvatureMap

    m, plain = model["m"], model["mesh"]
    assert m.curvature_map is None and not isinstance(getattr(plain, "curvature"), CurvatureMap)
    try:
        m.curvature_map = True
        auto = m.extract_meshes(model["codes"], **model["ekw"])[0]
        bare = m.extract_meshes(model["codes"], **dict(model["ekw"], bake_texture=0))[0]
        m.curvature_map = "bumpy"
        with pytest.raises(ValueError):
            m.extract_meshes(model["codes"], **model["ekw"])
    finally:
        m.curvature_map = None
    assert isinstance(auto.curvature, CurvatureMap) and auto.curvature.rule == 0 and auto.curvature.resolution == 64
    assert not isinstance(bare.curvature, CurvatureMap)                       # no texture bake, no map
    for key in ("vertices", "faces", "uvs", "texture"):                       # everything else is what it was
        a, b = getattr(auto, key), getattr(plain, key)
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                  b.view(torch.int32) if b.dtype == torch.float32 else b), key
    explicit = m.bake_curvature_map(plain, curvature=True)[1]
    _same(auto.curvature.mean, explicit.mean, "model setting vs explicit call")


def test_generator_curvature_map_leaves_the_map_on_the_mesh(cuda, tmp_path):
    import types

    from test_host_logic import _write_checkpoint

    from sculptmate_amd import synth
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr.curvature import CurvatureMap
    from sculptmate_amd.tsr.spec import SMALL_CFG

    _write_checkpoint(str(tmp_path), SMALL_CFG, seed=61)
    g = TripoGenerator(cuda)
    assert g.curvature_map is None and "`curvature_map`" in TripoGenerator.__doc__
    g.checkpoint_dir = str(tmp_path)
    g.mc_resolution = 32
    g.bake_texture_resolution = 64
    g.keep_components = "largest"
    assert g.initiate_model() == 0
    g.model.mesh_sink = lambda *a: None
    orig = g.model.extract_mesh

    def reachable(self, codes, **kw):   # random weights never reach the default threshold: take the grid's median
        return orig(codes, **dict(kw, threshold=float(ops.density_grid(codes[0].contiguous(), self.decoder, kw["resolution"]).median())))

    g.model.extract_mesh = types.MethodType(reachable, g.model)
    img = (synth.composite_rgb(synth.image_rgba(seed=62, size=SMALL_CFG["cond_image_size"])) * 255).astype(np.uint8)
    assert g.generate_mesh(img, "plain", enable_texture=True) == 0
    assert not isinstance(g.last_meshes[0].curvature, CurvatureMap)
    g.curvature_map = True
    assert g.generate_mesh(img, "curved", enable_texture=True) == 0 and g.model.curvature_map is True
    cmap = g.last_meshes[0].curvature
    assert isinstance(cmap, CurvatureMap) and cmap.resolution == 64 and cmap.rule == 0 and bool(cmap.mask.any())
