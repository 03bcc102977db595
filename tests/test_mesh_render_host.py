"""The mesh render without a device (csrc/mesh_ray.hip "the mesh render"; ops.mesh_render, Mesh.render, TSR.render_mesh): the
NumPy restatement (tests/_meshrenderref.py) against cases derivable by hand, the rules that are checked before any launch, the
refusals and the signatures."""
import inspect

import numpy as np
import pytest
import torch

import _meshrenderref as MR
import _rayref as RR


def _cube():
    """The unit cube [-0.5, 0.5]^3: every coordinate, and so every step of a ray aimed along an axis, is exact.  Faces 2 and 3
    are the +z side, a = (-.5, -.5), b = (.5, -.5), c = (-.5, .5) and a = (.5, -.5), b = (.5, .5), c = (-.5, .5) in (x, y); they
    share the diagonal b - c of face 2."""
    v, f = RR.cube()
    return (v - np.float32(0.5)).astype(np.float32), f


def _uvs(nf):
    """Per corner: a -> (0, 1), b -> (1, 1), c -> (0, 0) on every face."""
    return np.tile(np.array([[0, 1], [1, 1], [0, 0]], np.float32), (nf, 1))


TEXELS = np.array([[0.0, 0.25], [0.5, 1.0]], np.float32)       # [row y][column x]


def _texture():
    return np.stack([TEXELS, TEXELS * np.float32(0.5), 1 - TEXELS], -1).astype(np.float32)


def test_the_restatement_on_the_cube_by_hand():
    P, F = _cube()
    assert np.array_equal(P[F[2]], np.array([[-.5, -.5, .5], [.5, -.5, .5], [-.5, .5, .5]], np.float32))
    assert np.array_equal(P[F[3]], np.array([[.5, -.5, .5], [.5, .5, .5], [-.5, .5, .5]], np.float32))
    o = np.array([[0, 0, 3], [-0.25, -0.25, 3], [0.5, -0.5, 3], [2, 2, 3]], np.float32)
    d = np.tile(np.array([[0, 0, -1]], np.float32), (4, 1))
    got = MR.render(o, d, P, F, tuple(MR.PASSES), uvs=_uvs(len(F)), texture=_texture())
    # ray 0 runs through the shared diagonal: both faces hit at t = 2.5 exactly, the lower index wins
    t, face, uv, ties = RR.ray_cast(o, d, P, F, want_ties=True)
    assert ties[0] == 2 and face[0] == 2 and t[0] == 2.5
    assert got["face"].dtype == np.int32 and got["face"].tolist() == [2, 2, 2, -1]
    assert got["depth"].dtype == np.float32 and got["depth"].tolist() == [2.5, 2.5, 2.5, 0.0]
    assert got["opacity"].tolist() == [1.0, 1.0, 1.0, 0.0]
    # ray 1: u = v = 0.25, w0 = 0.5 -> U = 0.25, V = 0.75 -> X = 0.5, Y = 0.5: the mean of the four texels
    assert got["color"][1, 0] == np.float32((0.0 + 0.25 + 0.5 + 1.0) / 4) == np.float32(0.4375)
    assert got["color"][1, 1] == np.float32(0.21875) and got["color"][1, 2] == np.float32(1 - 0.4375)
    # ray 0: u = v = 0.5 -> U = 0.5, V = 0.5 -> X = 1, Y = 1: texel (1, 1) itself, its right and lower neighbours clamped
    assert got["color"][0, 0] == TEXELS[1, 1]
    # ray 2 hits corner b of face 2: U = 1, V = 1 -> X = 2 (column 2 clamped to 1, fraction 0), Y = 0: texel (x 1, y 0)
    assert got["color"][2, 0] == TEXELS[0, 1]
    # the miss holds every background
    assert got["color"][3].tolist() == [1, 1, 1] and got["shaded"][3].tolist() == [1, 1, 1] and got["rgba"][3].tolist() == [0, 0, 0, 0]
    assert got["normal"][3].tolist() == [0, 0, 0] and got["occlusion"][3] == 1
    # the +z face seen from +z under the headlight: n = l = (0, 0, 1), no occlusion -> k = 0.3 + (1 - 0.3) * 1 in fp32
    assert got["normal"][1].tolist() == [0, 0, 1] and got["occlusion"][1] == 1
    k = np.float32(0.3) * np.float32(1) + (np.float32(1) - np.float32(0.3)) * np.float32(1)
    assert np.array_equal(got["shaded"][1], got["color"][1] * k)
    assert np.array_equal(got["rgba"][1], np.append(got["color"][1], np.float32(1)))
    # outward = -1 turns the face normal away from the headlight: only the ambient share is left
    back = MR.render(o, d, P, F, ("normal", "shaded"), uvs=_uvs(len(F)), texture=_texture(), outward=-1.0)
    assert back["normal"][1].tolist() == [0, 0, -1]
    assert np.array_equal(back["shaded"][1], got["color"][1] * (np.float32(0.3) * np.float32(1) + (np.float32(1) - np.float32(0.3)) * np.float32(0)))
    # a fixed light along +x leaves the +z face at its ambient share as well
    side = MR.render(o, d, P, F, ("shaded",), light=(2.0, 0.0, 0.0))
    assert np.array_equal(side["shaded"][1], np.full(3, MR.GREY * np.float32(0.3), np.float32))


def test_the_lookup_by_hand():
    img = _texture()
    U = np.array([0.0, 1.0, 0.5, 0.25, np.nan, 0.5, -3.0, 7.0], np.float32)
    V = np.array([1.0, 0.0, 0.5, 0.75, 0.5, np.inf, 9.0, -2.0], np.float32)
    got = MR.lookup(img[..., 0], U, V)
    # (0, 1): texel (0, 0).  (1, 0): X = Y = 2, both clamped: texel (1, 1).  non-finite: texel (0, 0).  far outside: the corner
    assert got.tolist() == [0.0, 1.0, 1.0, 0.4375, 0.0, 0.0, 0.0, 1.0]
    one = np.full((1, 1, 3), 0.625, np.float32)          # a map of side 1 is its one texel everywhere
    assert np.array_equal(MR.lookup(one, U, V), np.full((8, 3), 0.625, np.float32))


def test_tangent_space_decoding_of_the_flat_value_returns_the_interpolated_normal():
    P, F = _cube()
    rng = np.random.default_rng(5)
    cn = rng.normal(size=(3 * len(F), 3)).astype(np.float32)
    ct = np.concatenate([rng.normal(size=(3 * len(F), 3)), rng.choice([-1.0, 1.0], (3 * len(F), 1))], 1).astype(np.float32)
    o = np.array([[-0.25, -0.25, 3], [0.125, -0.375, 3]], np.float32)
    d = np.tile(np.array([[0, 0, -1]], np.float32), (2, 1))
    flat = np.broadcast_to(np.array([0.5, 0.5, 1.0], np.float32), (3, 3, 3))
    got = MR.render(o, d, P, F, ("normal", "face"), uvs=_uvs(len(F)), normal_map=flat, normal_map_space="tangent",
                    corner_normals=cn, corner_tangents=ct)
    face, uv = RR.ray_cast(o, d, P, F)[1:]
    assert got["face"].tolist() == face.tolist() and (face >= 0).all()
    w1, w2 = uv[:, 0], uv[:, 1]
    w0 = (np.float32(1) - w1) - w2
    N = MR.interp(cn[3 * face], cn[3 * face + 1], cn[3 * face + 2], w0, w1, w2)
    want, ok = MR.unit(N)
    assert ok.all() and np.array_equal(got["normal"], want)
    # and a tilted value comes back through the frame: x picks T, y picks B = s cross(N, T)
    T = np.array([[1, 0, 0]], np.float32)
    Nn = np.array([[0, 0, 1]], np.float32)
    assert MR.tangent_decode(np.array([[1, 0, 0]], np.float32), Nn, T, np.float32([1])).tolist() == [[1, 0, 0]]
    assert MR.tangent_decode(np.array([[0, 1, 0]], np.float32), Nn, T, np.float32([1])).tolist() == [[0, 1, 0]]
    assert MR.tangent_decode(np.array([[0, 1, 0]], np.float32), Nn, T, np.float32([-1])).tolist() == [[0, -1, 0]]
    # the object-space map is 2 x - 1 normalised, and a map that decodes to no direction falls through to the face normal
    obj = MR.render(o, d, P, F, ("normal",), uvs=_uvs(len(F)), normal_map=np.full((2, 2, 3), 0.5, np.float32) + np.float32([0.5, 0, 0]),
                    normal_map_space="object")
    assert obj["normal"].tolist() == [[1, 0, 0], [1, 0, 0]]
    grey = MR.render(o, d, P, F, ("normal",), uvs=_uvs(len(F)), normal_map=np.full((2, 2, 3), 0.5, np.float32), normal_map_space="object")
    assert grey["normal"].tolist() == [[0, 0, 1], [0, 0, 1]]


def test_pass_and_material_rules_are_checked_before_anything_else():
    from sculptmate_amd import ops

    assert ops.MESH_RENDER_GREY == 0.8 and tuple(ops.MESH_RENDER_PASSES) == tuple(MR.PASSES)
    for p, (shape, dtype, bg) in MR.PASSES.items():
        assert ops.MESH_RENDER_PASSES[p][0] == shape and ops.MESH_RENDER_PASSES[p][2] == bg
    assert ops.mesh_render_passes("depth") == ("depth",) and ops.mesh_render_passes(["face", "color", "face"]) == ("face", "color")
    z = torch.zeros(4, 3)
    f = torch.zeros((1, 3), dtype=torch.int64)
    for fn in (ops.mesh_render, ops.mesh_render_composed):
        for bad in ((), [], ("colour",), ("color", "albedo"), "z_vals"):
            with pytest.raises(ValueError, match="pass"):
                fn(z, z, z, f, passes=bad)
        nm = torch.zeros(2, 2, 3)
        uv = torch.zeros(3, 2)
        with pytest.raises(ValueError, match="normal_map_space"):
            fn(z, z, z, f, uvs=uv, normal_map=nm)
        with pytest.raises(ValueError, match="normal_map_space"):
            fn(z, z, z, f, uvs=uv, normal_map=nm, normal_map_space="world")
        with pytest.raises(ValueError, match="corner_normals and corner_tangents"):
            fn(z, z, z, f, uvs=uv, normal_map=nm, normal_map_space="tangent")
        with pytest.raises(ValueError, match="corner_normals and corner_tangents"):
            fn(z, z, z, f, uvs=uv, normal_map=nm, normal_map_space="tangent", corner_normals=torch.zeros(3, 3))
        for name, value in (("texture", nm), ("normal_map", nm), ("occlusion_map", torch.zeros(2, 2))):
            with pytest.raises(ValueError, match="uvs"):
                fn(z, z, z, f, normal_map_space="object", **{name: value})
        for kw in (dict(ambient=float("nan")), dict(ambient="0.3"), dict(outward=float("inf")), dict(light=(0, 0, 0)),
                   dict(light=(1.0, 2.0)), dict(light=(1.0, float("nan"), 0.0)), dict(light="up")):
            with pytest.raises(ValueError):
                fn(z, z, z, f, **kw)
    assert ops.mesh_render_light(None) is None
    l = ops.mesh_render_light((0.0, 3.0, 4.0))
    assert l.dtype == np.float32 and l.tolist() == [0.0, np.float32(0.6), np.float32(0.8)]


def test_refusals():
    from sculptmate_amd import ops
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd._facade import STATUS_NOT_LOADED
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import TSR, Mesh

    P, F = _cube()
    v, f = torch.from_numpy(P), torch.from_numpy(F)
    o = torch.zeros(2, 5, 5, 3)
    for fn in (ops.mesh_render, ops.mesh_render_composed):
        with pytest.raises(ops.SculptError, match="no CPU fallback"):
            fn(o, o, v, f)
        with pytest.raises(ops.SculptError, match="no CPU fallback"):
            fn(o.reshape(-1, 3), o.reshape(-1, 3), v, f, passes=("face",))
    with pytest.raises(ops.SculptError, match="no CPU fallback"):
        Mesh(v, f).render(o, o)
    with pytest.raises(ops.SculptError, match="no CPU fallback"):
        Mesh(P, F).render(o, o, passes=("shaded",))
    m = TSR(SMALL_CFG)
    with pytest.raises(ValueError, match="pass"):
        m.render_mesh(Mesh(v, f), 2, passes=("weights",))
    with pytest.raises(ValueError, match="return_type"):
        m.render_mesh(Mesh(v, f), 2, return_type="jpeg")
    with pytest.raises(ops.SculptError, match="no device"):
        m.render_mesh(Mesh(v, f), 2)
    g = TripoGenerator(torch.device("cpu"))
    assert g.render_mesh_views(Mesh(v, f)) == STATUS_NOT_LOADED and g.render_mesh_views(Mesh(v, f), passes=("color",)) == STATUS_NOT_LOADED


def test_signatures():
    import ctypes

    from sculptmate_amd import _lib, ops
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr.system import TSR, Mesh

    res, args = _lib.SIGNATURES["sculpt_surface_render"]
    assert res is ctypes.c_int and len(args) == 19 and hasattr(_lib.lib, "sculpt_surface_render")
    assert [n for n, _ in _lib.RenderMaterial._fields_] == ["uvs", "texture", "normal_map", "corner_normals", "corner_tangents", "occlusion_map",
                                                            "vertex_colors", "vertex_normals", "vertex_occlusion", "texture_res",
                                                            "normal_map_res", "occlusion_map_res", "vertex_color_channels"]
    assert [n for n, _ in _lib.RenderOutputs._fields_] == ["color", "shaded", "opacity", "rgba", "depth", "normal", "occlusion", "face"]
    want = ("(rays_o, rays_d, vertices, faces, passes=('color',), uvs=None, texture=None, normal_map=None, normal_map_space=None, "
            "corner_normals=None, corner_tangents=None, occlusion_map=None, vertex_colors=None, vertex_normals=None, "
            "vertex_occlusion=None, ambient=0.3, light=None, outward=1.0)")
    assert str(inspect.signature(ops.mesh_render)) == want and str(inspect.signature(ops.mesh_render_composed)) == want
    assert str(inspect.signature(Mesh.render)) == "(self, rays_o, rays_d, passes=('color',), ambient=0.3, light=None, outward=1.0)"
    p = inspect.signature(TSR.render_mesh).parameters
    assert list(p) == ["self", "mesh", "n_views", "elevation_deg", "camera_distance", "fovy_deg", "height", "width", "passes",
                       "return_type", "ambient", "light"]
    assert [p[k].default for k in list(p)[3:]] == [0.0, 1.9, 40.0, 256, 256, ("color",), "pt", 0.3, None]
    q = inspect.signature(TSR.render).parameters
    assert all(p[k].default == q[k].default for k in ("elevation_deg", "camera_distance", "fovy_deg", "height", "width"))
    p = inspect.signature(TripoGenerator.render_mesh_views).parameters
    assert list(p) == ["self", "mesh", "n_views", "passes", "camera"] and p["n_views"].default == 8 and p["passes"].default is None
    assert ops.mesh_render_route() in (ops.mesh_render, ops.mesh_render_composed)
