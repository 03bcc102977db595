"""Wall thickness (ops.mesh_thickness / bake_thickness, Mesh.thickness, TSR.bake_thickness_map, tsr.thickness.ThicknessMap): what
needs no GPU -- the rule and the cone set, the NumPy restatement (tests/_thickref.py) against closed forms, the map's image, the
ABI's argument checks and the signatures."""
import ctypes
import inspect
import io
import math

import numpy as np
import pytest
import torch

import _thickref as TH
from sculptmate_amd import _lib, ops
from sculptmate_amd.generate import TripoGenerator
from sculptmate_amd.tsr import mesh as mesh_module
from sculptmate_amd.tsr.spec import SMALL_CFG
from sculptmate_amd.tsr.system import TSR, Mesh
from sculptmate_amd.tsr.thickness import ThicknessMap

f32 = np.float32


def _ulps(got, want):
    """|got - want| in units of the fp32 spacing at want."""
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / np.spacing(np.abs(want).astype(f32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------- the rule, the cone set
def test_thickness_rule_accepts_and_refuses():
    assert ops.thickness_rule(True) == (32, None) and ops.thickness_rule(np.bool_(True)) == (32, None)
    assert ops.thickness_rule(1) == (1, None) and ops.thickness_rule(1024) == (1024, None)
    assert ops.thickness_rule((8, None)) == (8, None) and ops.thickness_rule((8, 0.5)) == (8, 0.5)
    assert ops.thickness_rule((8, math.inf)) == (8, math.inf)
    assert ops.thickness_rule(ops.thickness_rule(True)) == (32, None)          # a rule's own result is a rule
    for bad in (False, None, 0, -1, 1025, 1.5, "32", (8,), (8, 0.0), (8, -1.0), (8, math.nan), (0, 1.0), [8, 1.0], (8, 1.0, 2.0)):
        with pytest.raises(ValueError):
            ops.thickness_rule(bad)


@pytest.mark.parametrize("k,cone", [(1, 60.0), (32, 60.0), (32, 30.0), (7, 90.0), (1024, 1.0)])
def test_thickness_directions(k, cone):
    d = ops.thickness_directions(k, cone, seed=3)
    assert d.dtype == np.float32 and d.shape == (k, 3)
    assert np.array_equal(d, ops.thickness_directions(k, cone, seed=3))       # deterministic
    norm = np.sqrt((d.astype(np.float64) ** 2).sum(1))
    assert np.abs(norm - 1.0).max() < 1e-7
    c = math.cos(math.radians(cone))
    assert (d[:, 2] > c).all() and (d[:, 2] < 1.0).all()
    assert (np.diff(d[:, 2]) < 0).all() if k > 1 else True                    # the spiral runs from the axis to the rim
    if k > 1:
        assert not np.array_equal(d, ops.thickness_directions(k, cone, seed=4))
        turned, base = ops.thickness_directions(k, cone, seed=4), ops.thickness_directions(k, cone, seed=0)
        assert np.array_equal(turned[:, 2], base[:, 2])                        # the seed turns the set about z


def test_thickness_directions_defaults_and_refusals():
    assert np.array_equal(ops.thickness_directions(32), ops.thickness_directions(32, 60.0, 0))
    for k, cone, seed in ((0, 60.0, 0), (1025, 60.0, 0), (1.5, 60.0, 0), (8, 0.0, 0), (8, -5.0, 0), (8, 90.5, 0), (8, math.nan, 0),
                          (8, "60", 0), (8, 60.0, -1), (8, 60.0, 2 ** 31), (8, 60.0, 0.5)):
        with pytest.raises(ValueError):
            ops.thickness_directions(k, cone, seed)


def test_the_two_ray_count_rules_are_one_rule():
    """occlusion_rule and thickness_rule differ in what True means (64 directions, 32 rays) and in nothing else."""
    for x in (True, np.True_):
        assert ops.occlusion_rule(x) == (64, None) and ops.thickness_rule(x) == (32, None)
    for x in (False, None, 0, 1, 1024, 1025, 1.5, "8", (8, None), (8, 2.0), (8, math.inf), (8, 0.0), (8, math.nan), (8,), [8, 2.0]):
        results = []
        for rule in (ops.occlusion_rule, ops.thickness_rule):
            try:
                results.append(rule(x))
            except ValueError:
                results.append(ValueError)
        assert results[0] == results[1], (x, results)
    assert ops.occlusion_rule(1) == (1, None) and ops.occlusion_rule((8, 2.0)) == (8, 2.0)      # the table is not all refusals
    with pytest.raises(ValueError):
        ops.occlusion_rule((8, 0.0))


@pytest.mark.parametrize("k", [1, 7, 64])
@pytest.mark.parametrize("seed", [0, 3])
def test_the_two_direction_sets_are_one_spiral(k, seed):
    """Unit rows, and row i of both sets at the one azimuth phi_i = i x the golden angle + seed.  A unit vector rounded to fp32 has
    a squared norm within 3 * 2^-24 of 1: each component is off by at most 2^-24 of itself, so the sum of squares by at most
    2 * 2^-24 (1 + 2^-25) of the whole."""
    occ, thick = ops.occlusion_directions(k, seed), ops.thickness_directions(k, 90.0, seed)
    assert occ.dtype == thick.dtype == np.float32 and occ.shape == thick.shape == (k, 3)
    for d in (occ, thick):
        assert np.abs((d.astype(np.float64) ** 2).sum(1) - 1.0).max() <= 3.0 * 2.0 ** -24

    def apart(a, b):   # the angle between two azimuths, whichever side of +-pi each was reported on
        return np.abs((a - b + math.pi) % (2.0 * math.pi) - math.pi)

    az_occ, az_thick = np.arctan2(occ[:, 1].astype(np.float64), occ[:, 0]), np.arctan2(thick[:, 1].astype(np.float64), thick[:, 0])
    assert apart(az_occ, az_thick).max() <= 1e-6
    phi = np.arange(k, dtype=np.float64) * ops.GOLDEN_ANGLE + float(seed)
    assert apart(az_occ, phi).max() <= 1e-6 and apart(az_thick, phi).max() <= 1e-6


# ------------------------------------------------------------------------------------------------- restatement vs closed forms
def test_the_cubes_wind_outwards():
    from _rayref import cube

    v, f = cube()
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    assert abs(float((a * np.cross(b, c)).sum()) / 6.0 - 1.0) < 1e-12        # signed volume +1
    v, f = TH.box([0, 0, 0], [1, 1, 1], inverted=True)
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    assert abs(float((a * np.cross(b, c)).sum()) / 6.0 + 1.0) < 1e-12


def test_slab_thickness_is_the_closed_form():
    P, F, pts, nrm, offset = TH.slab_case()
    assert len(pts) == 100 and (np.abs(pts[:, :2]) <= 1).all()
    C = ops.thickness_directions(32, 60.0)
    thick, thin, valid = TH.thickness(pts, nrm, C, P, F, offset)
    assert thick.dtype == np.float32 and thin.dtype == np.float32 and valid.dtype == np.int32
    assert (valid == 32).all()
    h = 0.25 - float(offset)
    cz = C[:, 2].astype(np.float64)
    want_thin, want_thick = h / cz.max(), 32 * h / cz.sum()
    print("slab: thinnest %.7f (closed form %.7f), thickness %.7f (closed form %.7f); worst %.2f and %.2f ulp"
          % (thin[0], want_thin, thick[0], want_thick, _ulps(thin, want_thin).max(), _ulps(thick, want_thick).max()))
    assert abs(want_thin - 0.2514764) < 1e-6 and abs(want_thick - 0.3326823) < 1e-6
    assert _ulps(thin, want_thin).max() <= 4 and _ulps(thick, want_thick).max() <= 4


def test_cavity_counts_every_ray_and_an_overlapping_body_drops_front_faces():
    C = ops.thickness_directions(32, 60.0)
    P, F, pts, nrm, offset = TH.nested_cubes_case(inverted=True)
    assert len(pts) == 50
    thick, thin, valid, rays = TH.thickness(pts, nrm, C, P, F, offset, want_rays=True)
    assert (valid == 32).all() and (thin > 0.25).all() and (thin < 0.26).all() and (thick >= thin).all()
    assert rays[2].all() and (rays[1] >= 0).all()
    # the inner cube wound like the outer one: the rays that meet it enter through a front face and count for nothing
    P, F, pts, nrm, offset = TH.nested_cubes_case(inverted=False)
    thick, thin, valid, rays = TH.thickness(pts, nrm, C, P, F, offset, want_rays=True)
    print("overlapping body: valid rays %d .. %d, thinnest %.4f .. %.4f" % (valid.min(), valid.max(), thin.min(), thin.max()))
    assert (valid >= 8).all() and (valid <= 16).all()
    assert (thin > 0.45).all()
    assert (rays[1] >= 0).all() and (~rays[2]).any()                          # every ray hits; the front-face hits are the dropped ones
    assert np.array_equal(valid, rays[2].sum(1).astype(np.int32))
    # outward = -1 on the same mesh reverses the clause: only the front-face hits count
    flipped = TH.thickness(pts, nrm, C, P, F, offset, outward=-1.0)[2]
    assert np.array_equal(flipped, 32 - valid)


def test_the_frame_gives_unit_directions():
    rng = np.random.default_rng(7)
    n = np.concatenate([rng.normal(size=(200, 3)), [[0, 0, 1], [0, 0, -1], [1, 0, -0.0]]]).astype(f32)
    m, ok = TH.unit(n)
    assert ok.all()
    T, B = TH.frame(m)
    for c in ops.thickness_directions(32, 60.0):
        d = TH.directions(m, T, B, c).astype(np.float64)
        assert np.abs(np.sqrt((d * d).sum(1)) - 1.0).max() < 1e-6
        # the cone turns about the INWARD normal: the angle to -m is the cone direction's angle to +z
        assert np.abs(-(d * m.astype(np.float64)).sum(1) - float(c[2])).max() < 1e-6


def test_odd_points_of_the_restatement():
    P, F, _, _, offset = TH.nested_cubes_case(inverted=True)
    C = ops.thickness_directions(8, 60.0)
    pts = f32([[0.5, 0.5, 1], [np.nan, 0.5, 1], [0.5, 0.5, 1], [0.5, 0.5, 1], [0.5, 0.5, 3.0]])
    nrm = f32([[0, 0, 1], [0, 0, 1], [0, 0, 0], [0, np.inf, 0], [0, 0, -1]])
    thick, thin, valid = TH.thickness(pts, nrm, C, P, F, offset)
    assert valid.tolist() == [8, 0, 0, 0, 0]
    assert np.isnan(thick[1]) and np.isnan(thin[1]) and np.isnan(thick[3]) and np.isnan(thin[3])
    assert thick[2] == np.inf and thin[2] == np.inf and thick[4] == np.inf and thin[4] == np.inf
    huge = TH.thickness(pts[:1], f32([[3e38, 3e38, 0]]), C, P, F, offset)       # the squares overflow: unit does not apply
    assert huge[0][0] == np.inf and huge[2][0] == 0
    none = TH.thickness(pts, nrm, C, P, F[:0], offset)
    assert none[2].tolist() == [0] * 5 and none[0][0] == np.inf and np.isnan(none[0][1])


# ------------------------------------------------------------------------------------------------- the map
def test_thickness_map_image_and_png():
    from PIL import Image

    th = f32([[0.0, 0.25, 0.5], [1.0, np.inf, 2.0], [np.nan, 0.75, 3.0]])
    mask = np.ones((3, 3), bool)
    mask[2, 2] = False                                                        # 3.0 is outside the charts: not in the scale
    m = ThicknessMap(th, th.copy(), np.full((3, 3), 4, np.int32), mask, rule=(32, None))
    assert m.resolution == 3 and m.default_scale() == 2.0
    img = m.image()
    assert img.dtype == np.uint16 and img.shape == (3, 3)
    # scale=None: the largest finite covered value, 2.0; round(min(th / 2, 1) * 65535), a NaN 0
    assert np.array_equal(img, np.rint(np.array([[0, .125, .25], [.5, 1, 1], [0, .375, 1]]) * 65535).astype(np.uint16))
    assert img[0, 1] == 8192 and img[1, 0] == 32768
    assert img[1, 1] == 65535                                                  # +inf is white
    assert np.array_equal(m.image(scale=4.0), np.rint(np.array([[0, .0625, .125], [.25, 1, .5], [0, .1875, .75]]) * 65535).astype(np.uint16))
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            m.image(scale=bad)
    back = np.asarray(Image.open(io.BytesIO(m.png_bytes())))
    assert back.dtype == np.uint16 and np.array_equal(back, img)              # the 16-bit round trip
    info = m.info()
    assert info["covered"] == 8 and info["no_valid_ray_share"] == 0.0 and info["valid_rays_per_texel"] == 4.0
    # the finite thinnest values of the covered texels: 0, 0.25, 0.5, 0.75, 1, 2
    assert info["thinnest_min"] == 0.0 and info["thinnest_median"] == 0.625 and 0.0 <= info["thinnest_p5"] <= 0.25
    empty = ThicknessMap(np.zeros((2, 2), f32), np.zeros((2, 2), f32), np.zeros((2, 2), np.int32), np.zeros((2, 2), bool))
    assert empty.default_scale() == 1.0 and empty.info()["covered"] == 0 and (empty.image() == 0).all()


# ------------------------------------------------------------------------------------------------- ABI and checks
def test_abi_symbol_and_its_argument_checks():
    """Refused with a code and a message, never a crash (nothing is launched: the checks come first)."""
    lib = _lib.lib
    assert "sculpt_surface_thickness" in _lib.SIGNATURES and hasattr(lib, "sculpt_surface_thickness")
    assert lib.sculpt_version() == 4   # a new symbol only
    params = (ctypes.c_double * 7)(0, 0, 0, 1, 1, 1, 1)
    inf, nan = math.inf, math.nan

    def th(n, params=params, k=8, amax=0.0, offset=0.0, far=inf, outward=1.0):
        return lib.sculpt_surface_thickness(None, None, n, None, None, k, offset, far, outward, None, None, 0, None, None, None, params,
                                            amax, None, None, None, None)

    assert th(-1) != 0 and "out of range" in _lib.last_error()
    assert th(4, params=None) != 0 and "null grid params" in _lib.last_error()
    assert th(4, amax=nan) != 0 and "amax" in _lib.last_error()
    for k in (0, -1, 1025):
        assert th(4, k=k) != 0 and "directions" in _lib.last_error()
    assert th(4, far=-1.0) != 0 and th(4, far=nan) != 0 and "max_distance" in _lib.last_error()
    assert th(4, offset=inf) != 0 and "offset" in _lib.last_error()
    for outward in (0.0, 2.0, nan):
        assert th(4, outward=outward) != 0 and "outward" in _lib.last_error()
    assert th(4) != 0 and "null array" in _lib.last_error()
    assert th(0) == 0 and th(0, outward=-1.0) == 0


def test_bad_arguments_are_value_errors_before_any_device_work():
    for kw in (dict(thickness=False), dict(thickness=0), dict(thickness=(8, 0.0)), dict(cone=0.0), dict(cone=120.0), dict(seed=-1),
               dict(seed=1.5), dict(offset=math.inf), dict(offset="x"), dict(outward=0.5), dict(outward=math.nan)):
        for fn in (ops.mesh_thickness, ops.mesh_thickness_composed):
            with pytest.raises(ValueError):   # before the tensors are even looked at
                fn(None, None, None, None, **kw)
        with pytest.raises(ValueError):
            ops.bake_thickness(None, None, None, None, **kw)
    with pytest.raises(ValueError):
        ops.bake_thickness(None, None, None, None, cage=0.1)                  # a cage without a source
    with pytest.raises(ValueError):
        ops.bake_thickness(None, None, None, None, source="mesh")
    v, f = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32)
    for kw in (dict(thickness=0), dict(cone=0.0), dict(seed=-1), dict(outward=0.0)):
        with pytest.raises(ValueError):
            Mesh(v, f).thickness(**kw)
    with pytest.raises(ops.SculptError):
        Mesh(v, f).thickness()                                                # host arrays are refused
    with pytest.raises(ValueError):
        TSR.bake_thickness_map(TSR.__new__(TSR), Mesh(v, f), thickness=0)


def test_the_route_switch(monkeypatch):
    monkeypatch.delenv("SCULPT_DISTANCE_FORM", raising=False)
    assert ops.mesh_thickness_route() is ops.mesh_thickness
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", "composedthickness")
    assert ops.mesh_thickness_route() is ops.mesh_thickness_composed
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", "plain,composedthickness")
    assert ops.mesh_thickness_route() is ops.mesh_thickness_composed
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", "plain")
    assert ops.mesh_thickness_route() is ops.mesh_thickness


# ------------------------------------------------------------------------------------------------- signatures
def _names(fn):
    return list(inspect.signature(fn).parameters)


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def test_signatures():
    point = ["points", "normals", "vertices", "faces", "thickness", "cone", "offset", "seed", "outward"]
    want = dict(thickness=True, cone=60.0, offset=None, seed=0, outward=1.0)
    for fn in (ops.mesh_thickness, ops.mesh_thickness_composed):
        assert _names(fn) == point and _defaults(fn) == want
    assert _names(ops.bake_thickness) == ["v_pos", "faces", "normals", "rast", "thickness", "cone", "offset", "seed", "outward", "source",
                                          "cage"]
    assert _defaults(ops.bake_thickness) == dict(want, source=None, cage=None)
    assert _names(ops.thickness_rule) == ["thickness"]
    assert _names(ops.thickness_directions) == ["k", "cone", "seed"] and _defaults(ops.thickness_directions) == dict(cone=60.0, seed=0)
    assert _names(ops._SurfaceIndex.thickness) == ["self", "points", "normals", "cone_dirs", "offset", "max_distance", "outward"]
    assert _names(Mesh.thickness) == ["self", "thickness", "cone", "seed", "outward"]
    assert _defaults(Mesh.thickness) == dict(thickness=True, cone=60.0, seed=0, outward=1.0)
    assert _names(TSR.bake_thickness_map)[:8] == ["self", "mesh", "source", "resolution", "thickness", "cone", "cage", "seed"]
    d = _defaults(TSR.bake_thickness_map)
    assert (d["source"], d["resolution"], d["thickness"], d["cone"], d["cage"], d["seed"]) == (None, None, True, 60.0, None, 0)
    assert _names(ThicknessMap.image) == ["self", "scale"] and _defaults(ThicknessMap.image) == dict(scale=None)
    for name in ("thickness", "thinnest", "valid", "mask", "rule"):
        assert name in _names(ThicknessMap.__init__)
    for name in ("pil_image", "png_bytes", "save", "info"):
        assert callable(getattr(ThicknessMap, name))


def test_the_settings_default_to_none_and_nothing_pinned_moved():
    assert TSR.thickness_map is None and TSR(SMALL_CFG).thickness_map is None and TSR.__new__(TSR).thickness_map is None
    assert TripoGenerator(torch.device("cpu")).thickness_map is None and "`thickness_map`" in TripoGenerator.__doc__
    assert _names(TSR.extract_meshes)[-2:] == ["subdivide", "occlusion"]
    assert _names(TSR.extract_mesh)[-2:] == ["subdivide", "occlusion"]
    assert "thickness" not in _names(TSR.extract_meshes) and "thickness" not in _names(TSR.extract_mesh)
    assert len(mesh_module.FIELDS) == 12 and "thickness" not in mesh_module.FIELDS and "thickness" not in mesh_module.VERTEX_FIELDS
    assert mesh_module.ATLAS_FIELDS == ("texture", "normal_map", "occlusion_map")
    assert "displacement" not in _names(Mesh.__init__) and "thickness" not in _names(Mesh.__init__)
    assert "thickness" not in _names(Mesh.export)
