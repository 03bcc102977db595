"""The occlusion bake over an atlas on the device (csrc/mesh_ray.hip sculpt_bake_occlusion; ops.bake_occlusion,
TSR.bake_occlusion_map): the fused kernel against the composed route and the NumPy restatement (tests/_aomapref.py), bit for bit."""
import numpy as np
import pytest
import torch

import _aomapref as A
import _tsrmodel
from sculptmate_amd import ops
from test_gpu_mesh_ray import MESHES
from test_remesh import icosphere

pytestmark = pytest.mark.gpu


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want, what):
    """Equal bit for bit, a NaN equal to any NaN."""
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    w = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, g.shape, w.dtype, w.shape)
    bad = np.argwhere((_bits(g) != _bits(w)) & ~(np.isnan(g) & np.isnan(w))) if g.dtype.kind == "f" else np.argwhere(g != w)
    assert len(bad) == 0, "%s: %d of %d differ, first at %r: %r vs %r" % (what, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])],
                                                                         w[tuple(bad[0])])


def _self_mesh(name):
    if name == "icosphere":
        v, f = icosphere(2)
        return v.astype(np.float32), np.asarray(f, np.int32)
    return MESHES[name]()


def _self_case(cuda, name, res, face_dtype=torch.int32):
    """(v, f, normals, rast) on the device under ops.uv_cell_atlas UVs; the normals are the device's own facet averages."""
    P, F = _self_mesh(name)
    v = torch.from_numpy(P).to(cuda)
    f = torch.from_numpy(F.astype(np.int64)).to(cuda).to(face_dtype)
    uv, idx = ops.uv_cell_atlas(v, f)
    rast = ops.bake_rasterize(uv, idx, res)
    return v, f, ops.vertex_normals(v, f).contiguous(), rast


def _restated(v, f, n, rast, k, seed=0, source=None, cage=0.0, offset=None):
    SP, SF = (v.cpu().numpy(), f.cpu().numpy()) if source is None else source
    used = np.asarray(SP, np.float32)[np.unique(SF)].astype(np.float64)
    longest = float((used.max(0) - used.min(0)).max())
    offset = np.float32(ops.OCCLUSION_OFFSET * longest) if offset is None else np.float32(offset)
    return A.bake_occlusion(rast.cpu().numpy(), v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy(), SP, SF,
                            ops.occlusion_directions(k, seed), offset, np.inf, cage)


# ---------------------------------------------------------------------------------------------------------- self mode
@pytest.mark.parametrize("face_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("name", ["icosphere", "cube", "doubled_cube"])
def test_self_mode_equals_the_composed_route_and_the_restatement(cuda, name, face_dtype):
    v, f, n, rast = _self_case(cuda, name, 32, face_dtype)
    covered = rast[..., 3] >= 0
    assert 0 < int(covered.sum()) < 32 * 32
    for k in (1, 16, 65):
        ao, mask = ops.bake_occlusion(v, f, n, rast, occlusion=k, seed=3)
        assert ao.dtype == torch.float32 and ao.shape == (32, 32) and mask.dtype == torch.bool and mask.shape == (32, 32)
        ao_c, mask_c = ops.bake_occlusion_composed(v, f, n, rast, occlusion=k, seed=3)
        _same(ao, ao_c, "%s k=%d fused vs composed" % (name, k))
        assert torch.equal(mask, mask_c) and torch.equal(mask, covered)
        assert bool((ao[~mask] == 0).all()) and not bool(torch.signbit(ao[~mask]).any())      # exactly +0
        assert bool(((ao[mask] >= 0) & (ao[mask] <= 1)).all())
        if k <= 16 and face_dtype == torch.int32:
            want, want_mask = _restated(v, f, n, rast, k, seed=3)
            _same(ao, want, "%s k=%d fused vs restatement" % (name, k))
            assert np.array_equal(mask.cpu().numpy(), want_mask)
            print("%s k=%d: %d covered texels, ao in [%.3f, %.3f]" % (name, k, int(mask.sum()), float(ao[mask].min()), float(ao[mask].max())))


def test_self_mode_with_a_far_limit_and_an_offset(cuda):
    v, f, n, rast = _self_case(cuda, "doubled_cube", 24)
    n = -n   # into the cube: every ray meets a wall, unless the far limit stops it first
    for occlusion, offset in (((8, 0.25), None), ((8, 2.5), 0.01), (8, -0.01)):
        ao, mask = ops.bake_occlusion(v, f, n, rast, occlusion=occlusion, offset=offset)
        ao_c, mask_c = ops.bake_occlusion_composed(v, f, n, rast, occlusion=occlusion, offset=offset)
        _same(ao, ao_c, "far/offset %r %r" % (occlusion, offset))
        assert torch.equal(mask, mask_c)
    assert bool((ops.bake_occlusion(v, f, n, rast, occlusion=(8, 2.5))[0][mask] < 1).any())


# ---------------------------------------------------------------------------------------------------------- tile edges
@pytest.mark.parametrize("res", [1, 7, 37, 64])
def test_resolutions_that_are_no_multiple_of_the_tile(cuda, res):
    v, f, n, rast = _self_case(cuda, "icosphere", res)
    ao, mask = ops.bake_occlusion(v, f, n, rast, occlusion=8)
    ao_c, mask_c = ops.bake_occlusion_composed(v, f, n, rast, occlusion=8)
    _same(ao, ao_c, "res %d" % res)
    assert torch.equal(mask, mask_c) and torch.equal(mask, rast[..., 3] >= 0) and bool((ao[~mask] == 0).all())


def test_empty_tiles_a_single_texel_and_bad_rows(cuda):
    v, f, n, rast = _self_case(cuda, "icosphere", 96)          # 3 x 3 tiles
    covered = rast[..., 3] >= 0
    empty = torch.tensor([0.0, 0.0, 0.0, -1.0], device=cuda)
    # the charts squeezed into the top-left tile and a bit of its neighbours: whole tiles stay empty
    r = empty.expand(96, 96, 4).clone()
    r[:40, :40] = rast[:40, :40]
    # a tile with exactly one covered texel (tile (2, 2), a texel taken from the charts)
    ys, xs = torch.nonzero(covered, as_tuple=True)
    r[70, 91] = rast[ys[0], xs[0]]
    # rows that count as not covered: tri out of range, negative, NaN, huge, infinite
    bad = [float(f.shape[0]), float(f.shape[0] + 5), -3.0, float("nan"), 3.0e9, float("inf"), -float("inf")]
    for i, t in enumerate(bad):
        r[5 + i, 50] = torch.tensor([0.3, 0.3, 0.4, t], device=cuda)
    r = r.contiguous()
    ao, mask = ops.bake_occlusion(v, f, n, r, occlusion=8)
    ao_c, mask_c = ops.bake_occlusion_composed(v, f, n, r, occlusion=8)
    _same(ao, ao_c, "edited rast")
    assert torch.equal(mask, mask_c)
    want = torch.zeros_like(covered)
    want[:40, :40] = covered[:40, :40]
    want[70, 91] = True
    assert torch.equal(mask, want) and int(mask[64:, 64:].sum()) == 1 and int(mask[64:, :64].sum()) == 0
    assert bool((ao[~mask] == 0).all())
    # a texel depends on that texel alone: the kept ones hold what the full atlas gives them
    full = ops.bake_occlusion(v, f, n, rast, occlusion=8)[0]
    _same(ao[:40, :40][covered[:40, :40]], full[:40, :40][covered[:40, :40]], "kept texels")
    _same(ao[70, 91], full[ys[0], xs[0]], "the single texel")
    # a face that names a vertex out of range covers nothing, and nothing is read through it
    f_bad = f.clone()
    f_bad[0, 1] = v.shape[0] + 7
    f_bad[1, 2] = -1
    ao_b, mask_b = ops.bake_occlusion(v, f_bad, n, rast, occlusion=8, source=(v, f), cage=1e-9)
    ao_bc, mask_bc = ops.bake_occlusion_composed(v, f_bad, n, rast, occlusion=8, source=(v, f), cage=1e-9)
    _same(ao_b, ao_bc, "bad faces")
    tri = rast[..., 3]
    assert torch.equal(mask_b, mask_bc) and torch.equal(mask_b, covered & (tri != 0) & (tri != 1))
    # no faces at all, and the empty image
    none = f[:0]
    ao_n, mask_n = ops.bake_occlusion(v, none, n, rast, occlusion=8, source=(v, f))
    assert not bool(mask_n.any()) and bool((ao_n == 0).all())
    ao_0, mask_0 = ops.bake_occlusion(v, f, n, rast[:0, :0], occlusion=8)
    assert ao_0.shape == (0, 0) and mask_0.shape == (0, 0)


# ---------------------------------------------------------------------------------------------------------- source mode
SOURCE_CASES = [(0.97, False), (0.97, True), (1.03, False), (1.03, True)]
_source = {}


def _source_case(scale, small):
    """The case and its restatement, computed once and shared, never modified."""
    key = (scale, small)
    if key not in _source:
        c = A.source_case(scale, small)
        dirs = ops.occlusion_directions(c["k"], 0)
        c["want"] = A.bake_occlusion(c["rast"], c["V"], c["F"], c["N"], c["SP"], c["SF"], dirs, c["offset"], np.inf, c["cage_value"],
                                     want_info=True)
        _source[key] = c
    return _source[key]


def test_the_source_cases_hold_what_they_are_meant_to():
    """On the restatement alone (no device): over the two scales with the default cage at least one texel each snaps, falls
    back, has its facet normal flipped and gets 0 < ao < 1; with the small cage every texel falls back."""
    snapped = fell = flipped = partial = 0
    for scale, small in SOURCE_CASES:
        c = _source_case(scale, small)
        ao, mask, info = c["want"]
        listed = info["listed"]
        assert int(listed.sum()) == int(mask.sum()) > 100
        if small:
            assert not info["hit"].any()
            continue
        a = ao.reshape(-1)[listed]
        snapped += int(info["hit"].sum())
        fell += int((listed & ~info["hit"]).sum())
        flipped += int(info["flipped"].sum())
        partial += int(((a > 0) & (a < 1)).sum())
    print("snapped %d, fell back %d, flipped %d, 0 < ao < 1 at %d" % (snapped, fell, flipped, partial))
    assert snapped > 0 and fell > 0 and flipped > 0 and partial > 0


@pytest.mark.parametrize("scale,small", SOURCE_CASES)
def test_source_mode_equals_the_composed_route_and_the_restatement(cuda, scale, small):
    c = _source_case(scale, small)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)   # noqa: E731
    v, f, n, rast = dev(c["V"]), dev(c["F"]), dev(c["N"]), dev(c["rast"])
    source = (dev(c["SP"]), dev(c["SF"]))
    kw = dict(occlusion=c["k"], source=source, cage=c["cage"])
    ao, mask = ops.bake_occlusion(v, f, n, rast, **kw)
    ao_c, mask_c = ops.bake_occlusion_composed(v, f, n, rast, **kw)
    _same(ao, ao_c, "fused vs composed")
    assert torch.equal(mask, mask_c)
    want, want_mask, _ = c["want"]
    _same(ao, want, "fused vs restatement")
    assert np.array_equal(mask.cpu().numpy(), want_mask)


# ---------------------------------------------------------------------------------------------------------- non-finite
def test_a_nan_vertex_gives_nan_at_the_texels_of_its_faces_only(cuda):
    c = _source_case(1.03, False)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)   # noqa: E731
    v, f, n, rast = dev(c["V"]), dev(c["F"]), dev(c["N"]), dev(c["rast"])
    source = (dev(c["SP"]), dev(c["SF"]))
    clean = ops.bake_occlusion(v, f, n, rast, occlusion=c["k"], source=source)[0]
    v_bad = v.clone()
    v_bad[5, 1] = float("nan")
    ao, mask = ops.bake_occlusion(v_bad, f, n, rast, occlusion=c["k"], source=source)
    ao_c, mask_c = ops.bake_occlusion_composed(v_bad, f, n, rast, occlusion=c["k"], source=source)
    _same(ao, ao_c, "NaN vertex")
    touched = (f == 5).any(1)[rast[..., 3].clamp(min=0).long()] & mask
    assert torch.equal(mask, mask_c) and torch.equal(mask, rast[..., 3] >= 0) and int(touched.sum()) > 0
    assert bool(torch.isnan(ao[touched]).all()) and not bool(torch.isnan(ao[~touched]).any())
    _same(ao[~touched], clean[~touched], "the neighbours")


# ---------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def model(cuda):
    out = _tsrmodel.small_model(cuda, 32, enable_texture=True)
    m = out["m"]
    kw = dict(enable_texture=True, resolution=32, threshold=out["threshold"], bake_texture=64, keep_components="largest")
    out["ekw"] = kw
    out["high"] = m.extract_meshes(out["codes"], **kw)[0]
    out["low"] = m.extract_meshes(out["codes"], simplify=0.5, **kw)[0]
    out["mapped"] = m.bake_occlusion_map(out["low"], source=out["high"], resolution=64)
    return out


def test_bake_occlusion_map_end_to_end(model, tmp_path, monkeypatch):
    from sculptmate_amd import meshio

    low, high, got = model["low"], model["high"], model["mapped"]
    # the route TSR takes by default is the composed one; the fused kernel, asked for by its token, gives the same map
    assert ops.bake_occlusion_route() is ops.bake_occlusion_composed
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", "fusedbake")
    assert ops.bake_occlusion_route() is ops.bake_occlusion
    _same(model["m"].bake_occlusion_map(low, source=high, resolution=64).occlusion_map, got.occlusion_map, "fused route vs composed route")
    monkeypatch.delenv("SCULPT_DISTANCE_FORM")
    assert low.faces.shape[0] < high.faces.shape[0]
    assert got.vertices is low.vertices and got.faces is low.faces and got.uvs is low.uvs and got.texture is low.texture
    amap = got.occlusion_map
    assert amap.shape == (64, 64) and amap.dtype == torch.float32 and amap.is_cuda and got.occlusion_map_rule == (64, None)
    assert bool(torch.isfinite(amap).all()) and float(amap.min()) >= 0.0 and float(amap.max()) <= 1.0
    nf = low.faces.shape[0]
    rast = ops.bake_rasterize(got.uvs, torch.arange(3 * nf, device=amap.device, dtype=torch.int32).view(-1, 3), 64)
    covered = rast[..., 3] >= 0
    assert 0 < int(covered.sum()) < 64 * 64
    assert 64 // 150 == 0 and bool((amap[~covered] == 1).all())     # no round of padding at 64: outside the charts the map is 1
    inside = amap[covered]
    print("covered %d texels, ao in [%.3f, %.3f], mean %.3f" % (int(covered.sum()), float(inside.min()), float(inside.max()),
                                                                float(inside.mean())))
    assert float(inside.max()) > float(inside.min())
    path = str(tmp_path / "low.glb")
    got.export(path)
    back = meshio.read_glb(path)
    assert np.array_equal(back["occlusion_tex"], np.asarray(got.occlusion_map_image()))
    assert back["basecolor_tex"] is not None and back["normal_tex"] is None


def test_the_model_setting_equals_the_explicit_call(model):
    m = model["m"]
    assert m.occlusion_map is None
    try:
        m.occlusion_map = True
        auto = m.extract_meshes(model["codes"], simplify=0.5, **model["ekw"])[0]
        self_mode = m.extract_meshes(model["codes"], **model["ekw"])[0]              # no simplify: against itself
        bare = m.extract_meshes(model["codes"], simplify=0.5, **dict(model["ekw"], bake_texture=0))[0]
    finally:
        m.occlusion_map = None
    after = m.extract_meshes(model["codes"], simplify=0.5, **model["ekw"])[0]
    assert after.occlusion_map is None and bare.occlusion_map is None and m._occlusion_source is None
    for key in ("vertices", "uvs", "texture"):
        assert np.array_equal(_bits(getattr(auto, key)), _bits(getattr(model["low"], key))), key
        assert np.array_equal(_bits(getattr(after, key)), _bits(getattr(model["low"], key))), key
    _same(auto.occlusion_map, model["mapped"].occlusion_map, "model setting vs explicit call")
    assert auto.occlusion_map_rule == (64, None)
    explicit = m.bake_occlusion_map(model["high"], resolution=64)
    _same(self_mode.occlusion_map, explicit.occlusion_map, "self mode")
