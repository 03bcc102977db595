"""Ray queries (ops.mesh_ray_cast / mesh_occlusion, Mesh.ray_cast / ambient_occlusion, the occlusion option of extract_meshes and
the writers): the rules that need no GPU -- the NumPy restatement's own known answers (tests/_rayref.py), the direction set,
argument checks before any launch, the ABI, the signatures, the files."""
import ctypes
import hashlib
import inspect
import math

import numpy as np
import pytest
import torch

import _rayref as RR
from sculptmate_amd import _lib, meshio, ops
from sculptmate_amd.tsr.system import TSR, Mesh
from test_remesh import icosphere

TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
TRI_F = np.array([[0, 1, 2]], np.int32)


def _cast(o, d, P, F, **kw):
    return RR.ray_cast(np.array(o, np.float32).reshape(-1, 3), np.array(d, np.float32).reshape(-1, 3), P, F, **kw)


# ------------------------------------------------------------------------------------------------------- the restatement
def test_single_triangle_hit_miss_and_uv():
    t, face, uv = _cast([[0.25, 0.5, 2.0], [0.75, 0.75, 2.0], [0.25, 0.5, -3.0], [0.25, 0.5, 2.0]],
                        [[0, 0, -1], [0, 0, -1], [0, 0, 2], [0, 0, 1]], TRI, TRI_F)
    assert t[0] == 2.0 and face[0] == 0 and np.array_equal(uv[0], np.float32([0.25, 0.5]))
    assert t[1] == np.inf and face[1] == -1 and np.array_equal(uv[1], [0, 0])      # beside the face (u + v > 1)
    assert t[2] == 1.5 and face[2] == 0                                            # two-sided; t in units of |d|
    assert t[3] == np.inf and face[3] == -1                                        # behind the origin
    assert t.dtype == np.float64 and face.dtype == np.int64 and uv.dtype == np.float32


def test_a_ray_in_the_plane_of_a_face_misses_it():
    t, face, _ = _cast([[-1, 0.25, 0], [0.25, 0.25, 0]], [[1, 0, 0], [1, 1, 0]], TRI, TRI_F)   # det == 0
    assert (t == np.inf).all() and (face == -1).all()


def test_the_range_is_closed():
    o, d = [[0.25, 0.5, 2.0]], [[0, 0, -1]]
    assert _cast(o, d, TRI, TRI_F, tmax=2.0)[1][0] == 0
    assert _cast(o, d, TRI, TRI_F, tmax=float(np.nextafter(2.0, 0.0)))[1][0] == -1
    assert _cast(o, d, TRI, TRI_F, tmin=2.0)[1][0] == 0
    assert _cast(o, d, TRI, TRI_F, tmin=float(np.nextafter(2.0, 3.0)))[1][0] == -1


def test_zero_direction_and_non_finite_rays():
    t, face, uv = _cast([[0.25, 0.5, 0.0], [0.25, 0.5, 1.0], [np.nan, 0, 1], [0.25, 0.5, 1.0], [np.inf, 0, 0]],
                        [[0, 0, 0], [-0.0, 0, 0], [0, 0, -1], [0, np.nan, -1], [0, 0, -1]], TRI, TRI_F)
    assert (t[:2] == np.inf).all() and np.isnan(t[2:]).all() and (face == -1).all() and (uv == 0).all()
    t, face, _ = _cast([[0.25, 0.5, 1.0]], [[0, 0, -1]], TRI, np.zeros((0, 3), np.int32))
    assert t[0] == np.inf and face[0] == -1


def test_the_lowest_face_index_wins_a_tie_on_the_doubled_cube():
    P, F = RR.cube()
    rng = np.random.default_rng(2)
    o = rng.uniform(-2, 3, (400, 3))
    d = rng.uniform(0, 1, (400, 3)) - o
    t, face, _, ties = RR.ray_cast(o, d, P, np.concatenate([F, F]), want_ties=True)
    assert (face >= 0).sum() > 200 and (face < 12).all() and (ties[face >= 0] >= 2).all()
    single = RR.ray_cast(o, d, P, F)
    assert np.array_equal(single[1], face) and np.array_equal(single[0], t)


def test_every_ray_from_inside_the_closed_cube_hits():
    P, F = RR.cube()
    rng = np.random.default_rng(3)
    o = rng.uniform(0.05, 0.95, (500, 3))
    d = rng.normal(size=(500, 3))
    t, face, _ = RR.ray_cast(o, d, P, F)
    assert (face >= 0).all() and (t > 0).all() and np.isfinite(t).all()
    hit = o.astype(np.float32).astype(np.float64) + t[:, None] * d.astype(np.float32).astype(np.float64)
    assert np.abs(np.abs(hit - 0.5).max(1) - 0.5).max() < 1e-12                    # on the cube's surface


# ---------------------------------------------------------------------------------------------------- the direction set
@pytest.mark.parametrize("k, seed", [(1, 0), (2, 0), (3, 9), (64, 0), (64, 7), (1024, 1)])
def test_occlusion_directions_are_unit_vectors_that_balance(k, seed):
    d = ops.occlusion_directions(k, seed)
    assert d.dtype == np.float32 and d.shape == (k, 3)
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -23      # 1 ulp of fp32 at 1
    if k > 1:
        assert np.linalg.norm(d.astype(np.float64).mean(0)) <= 1.0 / k
    assert np.array_equal(d, ops.occlusion_directions(k, seed))
    assert np.array_equal(d[:, 2], ops.occlusion_directions(k, seed + 1)[:, 2])                # the seed turns it about z


def test_occlusion_directions_digest():
    d = ops.occlusion_directions(64, 0)
    assert hashlib.sha256(d.tobytes()).hexdigest()[:16] == "ba08cc5a7cc9cce0"
    assert not np.array_equal(d, ops.occlusion_directions(64, 1))


@pytest.mark.parametrize("k, seed", [(0, 0), (1025, 0), (True, 0), (8.0, 0), ("8", 0), (None, 0), (8, -1), (8, 2 ** 31), (8, 0.5), (8, True)])
def test_occlusion_directions_refuse(k, seed):
    with pytest.raises(ValueError):
        ops.occlusion_directions(k, seed)


@pytest.mark.parametrize("x, want", [(True, (64, None)), (np.bool_(True), (64, None)), (1, (1, None)), (1024, (1024, None)),
                                     (np.int64(16), (16, None)), ((16, 2.5), (16, 2.5)), ((16, 1), (16, 1.0)),
                                     ((16, math.inf), (16, math.inf)), ((16, None), (16, None))])
def test_occlusion_rule_accepts(x, want):
    assert ops.occlusion_rule(x) == want
    assert ops.occlusion_rule(ops.occlusion_rule(x)) == want                      # a rule's own result is a rule


@pytest.mark.parametrize("x", [False, np.bool_(False), None, 0, 1025, -3, 16.0, "16", (16,), (16, 0), (16, -1.0), (16, float("nan")),
                               (0, 1.0), (16.0, 1.0), (True, 1.0), (16, True), (16, "1"), (16, 1.0, 2.0), [16, 1.0]])
def test_occlusion_rule_refuses(x):
    with pytest.raises(ValueError):
        ops.occlusion_rule(x)


# ------------------------------------------------------------------------------------------------ occlusion, restated
def test_a_convex_body_sees_nothing_of_itself():
    v, f = icosphere(2)
    v = v.astype(np.float32)
    assert len(f) == 320
    ao = RR.occlusion(v, RR.area_normals(v, f), ops.occlusion_directions(64, 0), v, f, 2.0 ** -13 * 2.0)
    assert ao.dtype == np.float32 and np.array_equal(ao, np.ones(len(v), np.float32))


def test_points_inside_the_closed_cube_are_fully_occluded():
    P, F = RR.cube()
    rng = np.random.default_rng(4)
    pts = rng.uniform(0.05, 0.95, (60, 3)).astype(np.float32)
    nrm = rng.normal(size=(60, 3)).astype(np.float32)
    ao = RR.occlusion(pts, nrm, ops.occlusion_directions(64, 0), P, F, 1e-3)
    assert np.array_equal(ao, np.zeros(60, np.float32))
    short = RR.occlusion(pts, nrm, ops.occlusion_directions(64, 0), P, F, 1e-3, max_distance=0.01)
    assert (short > 0).any()                                                       # a short ray ends before the wall
    odd = RR.occlusion(np.float32([[0.5, 0.5, 0.5]] * 3), np.float32([[0, 0, 0], [np.nan, 0, 0], [0, 0, 1]]),
                       ops.occlusion_directions(8, 0), P, F, 0.0)
    assert odd[0] == 1.0 and np.isnan(odd[1]) and odd[2] == 0.0


# ------------------------------------------------------------------------------------------------------- ABI and checks
def test_abi_symbols_are_present():
    for name in ("sculpt_surface_ray_cast", "sculpt_surface_occlusion"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.sculpt_version() == 4   # new symbols only


def test_host_side_argument_checks_of_the_c_entry_points():
    """Refused with a code and a message, never a crash (nothing is launched: the checks come first)."""
    lib = _lib.lib
    params = (ctypes.c_double * 7)(0, 0, 0, 1, 1, 1, 1)
    inf, nan = math.inf, math.nan

    def cast(n, params=params, amax=0.0, tmin=0.0, tmax=inf):
        return lib.sculpt_surface_ray_cast(None, None, n, None, None, None, 0, None, None, None, params, amax, tmin, tmax, None, None, None, None)

    def occ(n, params=params, k=8, amax=0.0, offset=0.0, far=inf):
        return lib.sculpt_surface_occlusion(None, None, n, None, None, k, offset, far, None, None, 0, None, None, None, params, amax, None, None)

    assert cast(-1) != 0 and "out of range" in _lib.last_error()
    assert cast(4, params=None) != 0 and "null grid params" in _lib.last_error()
    assert cast(4, amax=nan) != 0 and "amax" in _lib.last_error()
    assert cast(4, tmin=2.0, tmax=1.0) != 0 and "tmin <= tmax" in _lib.last_error()
    assert cast(4, tmin=-1.0) != 0 and cast(4, tmin=nan) != 0 and cast(4, tmax=nan) != 0
    assert cast(4) != 0 and "null array" in _lib.last_error()
    assert cast(0) == 0 and cast(0, params=None) == 0
    bad = (ctypes.c_double * 7)(0, 0, 0, 1, 2000, 1, 1)
    assert cast(4, params=bad) != 0 and "grid side" in _lib.last_error()
    assert occ(-1) != 0 and "out of range" in _lib.last_error()
    assert occ(4, params=None) != 0 and "null grid params" in _lib.last_error()
    assert occ(4, amax=nan) != 0 and "amax" in _lib.last_error()
    for k in (0, -1, 1025):
        assert occ(4, k=k) != 0 and "directions" in _lib.last_error()
    assert occ(4, far=-1.0) != 0 and occ(4, far=nan) != 0 and "max_distance" in _lib.last_error()
    assert occ(4, offset=inf) != 0 and "offset" in _lib.last_error()
    assert occ(4) != 0 and "null array" in _lib.last_error()
    assert occ(0) == 0


def test_bad_arguments_are_value_errors_before_any_device_work():
    for bad in ((-1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("nan")), ("0", 1.0), (0.0, None), (True, 2.0)):
        with pytest.raises(ValueError):   # before the tensors are even looked at
            ops.mesh_ray_cast(None, None, None, None, *bad)
    for bad in (False, None, 0, 2000, 1.5, (8, 0.0)):
        with pytest.raises(ValueError):
            ops.mesh_occlusion(None, None, None, None, occlusion=bad)
        with pytest.raises(ValueError):
            Mesh(TRI, TRI_F).ambient_occlusion(bad)
    with pytest.raises(ValueError):
        ops.mesh_occlusion(None, None, None, None, offset=float("inf"))
    with pytest.raises(ValueError):
        ops.mesh_occlusion(None, None, None, None, seed=-1)
    with pytest.raises(ValueError):
        Mesh(TRI, TRI_F).ambient_occlusion(outward=float("nan"))


def test_cpu_tensors_and_host_array_meshes_are_refused():
    v, f = torch.from_numpy(TRI), torch.from_numpy(TRI_F)
    with pytest.raises(ops.SculptError):
        ops.mesh_ray_cast(v, v, v, f)
    with pytest.raises(ops.SculptError):
        ops.mesh_occlusion(v, v, v, f)
    with pytest.raises(ops.SculptError):
        ops.mesh_occlusion_composed(v, v, v, f)
    m = Mesh(TRI, TRI_F)
    with pytest.raises(ops.SculptError):
        m.ray_cast(TRI, TRI)
    with pytest.raises(ops.SculptError):
        m.ambient_occlusion()
    with pytest.raises(ops.SculptError):
        Mesh(v, f).ambient_occlusion(16)


def test_signatures_and_defaults():
    from sculptmate_amd.generate import TripoGenerator

    for name in ("extract_meshes", "extract_mesh"):
        p = inspect.signature(getattr(TSR, name)).parameters
        assert list(p)[-1] == "occlusion" and p["occlusion"].default is None
    for name in ("run", "run_async", "run_batched", "run_pipelined", "extract_mesh_sharded"):
        assert "occlusion" not in inspect.signature(getattr(TSR, name)).parameters
    p = inspect.signature(Mesh.__init__).parameters
    assert list(p)[-1] == "vertex_occlusion" and p["vertex_occlusion"].default is None
    p = inspect.signature(Mesh.ambient_occlusion).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [("occlusion", True), ("seed", 0), ("outward", 1.0)]
    p = inspect.signature(Mesh.ray_cast).parameters
    assert [(k, v.default) for k, v in p.items()][3:] == [("t_min", 0.0), ("t_max", math.inf)]
    p = inspect.signature(ops.mesh_ray_cast).parameters
    assert list(p) == ["origins", "directions", "vertices", "faces", "t_min", "t_max"] and p["t_max"].default == math.inf
    p = inspect.signature(ops.mesh_occlusion).parameters
    assert [(k, v.default) for k, v in p.items()][4:] == [("occlusion", True), ("offset", None), ("seed", 0)]
    assert TSR.WINDING_OUTWARD in (1.0, -1.0)
    g = TripoGenerator.__new__(TripoGenerator)
    TripoGenerator.__init__(g, "cpu")
    assert g.occlusion is None and "occlusion" in TripoGenerator.__doc__
    assert Mesh(TRI, TRI_F).vertex_occlusion is None


def test_a_bad_occlusion_raises_before_a_launch():
    m = TSR.__new__(TSR)   # no weights, no device: the rule must fire before either is needed
    for bad in (False, 0, 1.5, (8, -1.0)):
        with pytest.raises(ValueError, match="occlusion"):
            TSR.extract_meshes(m, [None], occlusion=bad)
        with pytest.raises(ValueError, match="occlusion"):
            TSR.extract_mesh(m, [None], occlusion=bad)


# --------------------------------------------------------------------------------------------------------------- writers
@pytest.fixture()
def sphere_mesh():
    v, f = icosphere(1)
    v = v.astype(np.float32)
    rng = np.random.default_rng(6)
    return v, f.astype(np.int64), rng.uniform(0, 1, len(v)).astype(np.float32), rng.uniform(0, 1, (len(v), 3)).astype(np.float32)


def test_ply_and_glb_round_trip_the_occlusion(tmp_path, sphere_mesh):
    v, f, ao, col = sphere_mesh
    nrm = RR.area_normals(v, f)
    m = Mesh(v, f, col, vertex_normals=nrm, vertex_occlusion=ao)
    m.export(tmp_path / "a.ply")
    back = meshio.read_ply(tmp_path / "a.ply")
    assert np.array_equal(back.occlusion, ao) and np.array_equal(back.normals, nrm) and np.array_equal(back[0], v) and np.array_equal(back[1], f)
    assert b"property float ao\n" in (tmp_path / "a.ply").read_bytes()
    m.export(tmp_path / "a.glb")
    back = meshio.read_glb(tmp_path / "a.glb")
    assert np.array_equal(back["occlusion"], ao) and np.array_equal(back["vertices"], v) and np.array_equal(back["faces"], f)
    assert b'"_OCCLUSION"' in (tmp_path / "a.glb").read_bytes()
    Mesh(v, f, vertex_occlusion=ao).export(tmp_path / "b.ply")
    assert np.array_equal(meshio.read_ply(tmp_path / "b.ply").occlusion, ao)
    m.export(tmp_path / "a.obj")                                  # no slot: written without it
    plain = tmp_path / "p.obj"
    Mesh(v, f, col, vertex_normals=nrm).export(plain)
    assert (tmp_path / "a.obj").read_bytes() == plain.read_bytes()
    with pytest.raises(ValueError, match="occlusion"):
        meshio.write_ply(str(tmp_path / "c.ply"), v, f, occlusion=ao[:-1])
    with pytest.raises(ValueError, match="occlusion"):
        meshio.write_glb(str(tmp_path / "c.glb"), v, f, occlusion=ao[:, None])


def test_the_textured_glb_takes_the_occlusion_per_corner(tmp_path, sphere_mesh):
    v, f, ao, _ = sphere_mesh
    rng = np.random.default_rng(7)
    uv = rng.uniform(0, 1, (3 * len(f), 2)).astype(np.float32)
    tex = rng.uniform(0, 1, (8, 8, 3)).astype(np.float32)
    Mesh(v, f, uvs=uv, texture=tex, vertex_occlusion=ao).export(tmp_path / "t.glb")
    back = meshio.read_glb(tmp_path / "t.glb")
    assert np.array_equal(back["occlusion"], ao[f.reshape(-1)]) and np.array_equal(back["vertices"], v[f.reshape(-1)])


def test_files_without_the_occlusion_are_byte_identical(tmp_path, sphere_mesh):
    """Against the parent's writers' output for the same mesh: tests/golden/mesh_ray_writers.json holds the sha256 of each file
    as the writers gave it before the keyword existed."""
    import json
    import os

    v, f, _, col = sphere_mesh
    nrm = RR.area_normals(v, f)
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "mesh_ray_writers.json")))
    made = {}
    for ext in ("ply", "glb", "obj"):
        for name, mesh in (("plain", Mesh(v, f)), ("full", Mesh(v, f, col, vertex_normals=nrm))):
            path = tmp_path / ("%s.%s" % (name, ext))
            mesh.export(path)
            made["%s.%s" % (name, ext)] = hashlib.sha256(path.read_bytes()).hexdigest()
    meshio.write_ply(str(tmp_path / "kw.ply"), v, f, vertex_colors=col, normals=nrm, occlusion=None)
    meshio.write_glb(str(tmp_path / "kw.glb"), v, f, vertex_colors=col, normals=nrm, occlusion=None)
    made["kw.ply"], made["kw.glb"] = (hashlib.sha256((tmp_path / n).read_bytes()).hexdigest() for n in ("kw.ply", "kw.glb"))
    assert made["kw.ply"] == made["full.ply"] and made["kw.glb"] == made["full.glb"]
    del made["kw.ply"], made["kw.glb"]
    assert made == golden
