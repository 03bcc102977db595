"""The occlusion bake over an atlas on the host: rules and refusals raised before anything is launched, signatures and defaults,
the pinned signature tails, and the way out of the library (Mesh.export to .glb and .obj, keep_components, the sinks).  Runs on
the CPU."""
import inspect
import json
import math

import numpy as np
import pytest

import _aomapref as A


def _baked_arrays():
    """The data of test_bake_texture_host.py's `baked` fixture."""
    rng = np.random.default_rng(7)
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int64)
    uvs = rng.random((12, 2)).astype(np.float32)
    tex = rng.random((6, 5, 3)).astype(np.float32)
    return v, f, uvs, tex


@pytest.fixture()
def shaded():
    """The baked tetrahedron with a 4 x 4 occlusion map that holds the edge values 0 and 1."""
    from sculptmate_amd.tsr.system import Mesh

    v, f, uvs, tex = _baked_arrays()
    m = Mesh(v, f, None, uvs=uvs, texture=tex)
    m.occlusion_map = np.random.default_rng(13).random((4, 4)).astype(np.float32)
    m.occlusion_map[0, 0], m.occlusion_map[0, 1], m.occlusion_map[0, 2] = 0.0, 1.0, 0.5
    m.occlusion_map_rule = (64, None)
    return m


# ---------------------------------------------------------------------------------------------- rules and refusals
def test_rules_are_raised_before_anything_is_launched(monkeypatch):
    import torch

    from sculptmate_amd import ops

    def launched(*a, **k):
        raise AssertionError("a rule error must come before the first launch")

    monkeypatch.setattr(ops, "_surface", launched)
    monkeypatch.setattr(ops, "_SurfaceIndex", launched)
    v = torch.zeros((4, 3))
    f = torch.zeros((4, 3), dtype=torch.int64)
    rast = torch.zeros((4, 4, 4))
    for fn in (ops.bake_occlusion, ops.bake_occlusion_composed):
        for bad in (False, None, 0, 1025, 2.5, "64", (8, -1.0), (8, math.nan), (8, 1.0, 2.0)):
            with pytest.raises(ValueError, match="occlusion"):
                fn(v, f, v, rast, occlusion=bad)
        for cage in (0.5, 0.0, True):
            with pytest.raises(ValueError, match="cage"):                     # a cage without a source
                fn(v, f, v, rast, cage=cage)
        for cage in (0.0, -1.0, math.nan, math.inf, "1", 1e-60):                # 1e-60 is 0 in fp32
            with pytest.raises(ValueError, match="cage"):
                fn(v, f, v, rast, source=(v, f), cage=cage)
        with pytest.raises(ValueError, match="source"):
            fn(v, f, v, rast, source=v)
        for offset in (math.nan, math.inf, "0"):
            with pytest.raises(ValueError, match="offset"):
                fn(v, f, v, rast, offset=offset)
        with pytest.raises(ValueError, match="seed"):
            fn(v, f, v, rast, seed=-1)
        # the rules pass: CPU tensors are refused, there is no CPU fallback
        with pytest.raises(ops.SculptError, match="no CPU fallback"):
            fn(v, f, v, rast)
        with pytest.raises(ops.SculptError, match="no CPU fallback"):
            fn(v, f, v, rast, source=(v, f), cage=0.25)


def test_tsr_rules_need_no_device():
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import TSR, Mesh

    v, f, uvs, tex = _baked_arrays()
    with pytest.raises(ValueError, match="occlusion"):
        TSR.__new__(TSR).bake_occlusion_map(Mesh(v, f), occlusion=False)
    m = TSR(SMALL_CFG)
    with pytest.raises(ValueError, match="source"):
        m.device = "cpu"
        m.bake_occlusion_map(Mesh(v, f), source=(v, f))
    with pytest.raises(ValueError, match="cage"):
        m.bake_occlusion_map(Mesh(v, f), cage=0.1)
    with pytest.raises(ValueError, match="resolution"):
        m.bake_occlusion_map(Mesh(v, f), resolution=0)
    m.occlusion_map = "yes"
    with pytest.raises(ValueError, match="occlusion"):                          # extract_meshes checks the setting first
        m.extract_meshes([None])


def test_signatures_and_defaults():
    import torch

    from sculptmate_amd import _lib, meshio, ops
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import TSR, Mesh

    for fn in (ops.bake_occlusion, ops.bake_occlusion_composed):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["v_pos", "faces", "normals", "rast", "occlusion", "offset", "seed", "source", "cage"]
        d = {k: p.default for k, p in sig.parameters.items()}
        assert d["occlusion"] is True and d["offset"] is None and d["seed"] == 0 and d["source"] is None and d["cage"] is None
    assert ops.OCCLUSION_CAGE == 2.0 ** -6
    sig = inspect.signature(TSR.bake_occlusion_map)
    assert list(sig.parameters) == ["self", "mesh", "source", "resolution", "occlusion", "cage", "seed", "island_padding", "unwrapper"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["source"] is None and d["resolution"] is None and d["occlusion"] is True and d["cage"] is None and d["seed"] == 0
    assert d["island_padding"] == 0.02 and d["unwrapper"] is None
    assert TSR(SMALL_CFG).occlusion_map is None and TripoGenerator(torch.device("cpu")).occlusion_map is None
    assert "sculpt_bake_occlusion" in _lib.SIGNATURES and len(_lib.SIGNATURES["sculpt_bake_occlusion"][1]) == 24
    # the pinned tails are where they were
    params = list(inspect.signature(meshio.write_glb).parameters)
    assert params[-2:] == ["tangents", "extra_images"] and params[params.index("occlusion") + 1] == "occlusion_tex"
    assert inspect.signature(meshio.write_glb).parameters["occlusion_tex"].default is None
    assert list(inspect.signature(meshio.write_obj_textured).parameters)[-1] == "occlusion_map"
    assert list(inspect.signature(Mesh.__init__).parameters)[-1] == "vertex_occlusion"
    assert list(inspect.signature(TSR.extract_meshes).parameters)[-2:] == ["subdivide", "occlusion"]
    assert list(inspect.signature(TSR.extract_mesh).parameters)[-2:] == ["subdivide", "occlusion"]
    plain = Mesh(*_baked_arrays()[:2])
    assert plain.occlusion_map is None and plain.occlusion_map_rule is None
    with pytest.raises(ValueError):
        plain.occlusion_map_image()


# ---------------------------------------------------------------------------------------------- the way out
def test_occlusion_map_image(shaded):
    img = shaded.occlusion_map_image()
    assert img.mode == "RGB" and img.size == (4, 4)
    a = np.asarray(img)
    want = np.clip(np.floor(256.0 * shaded.occlusion_map), 0, 255).astype(np.uint8)
    assert np.array_equal(a[..., 0], want) and np.array_equal(a[..., 1], want) and np.array_equal(a[..., 2], want)
    assert a[0, 0].tolist() == [0, 0, 0] and a[0, 1].tolist() == [255, 255, 255] and a[0, 2].tolist() == [128, 128, 128]


def test_export_glb_round_trip(shaded, tmp_path):
    from sculptmate_amd import meshio
    from sculptmate_amd.tsr.system import Mesh

    path = str(tmp_path / "shaded.glb")
    shaded.export(path)
    got = meshio.read_glb(path)
    assert np.array_equal(got["occlusion_tex"], np.asarray(shaded.occlusion_map_image()))
    assert np.array_equal(got["basecolor_tex"], np.asarray(shaded.texture_image())) and got["normal_tex"] is None
    assert np.array_equal(got["vertices"], shaded.vertices[shaded.faces.reshape(-1)]) and got["occlusion"] is None
    raw = open(path, "rb").read()
    doc = json.loads(raw[20:20 + int.from_bytes(raw[12:16], "little")])
    assert doc["materials"][0]["occlusionTexture"] == {"index": 1} and len(doc["textures"]) == 2     # strength: glTF's default
    # the map alone (no texture, no normal map) still goes out with its UVs
    v, f, uvs, _ = _baked_arrays()
    alone = Mesh(v, f, None, uvs=uvs)
    alone.occlusion_map = shaded.occlusion_map
    alone.export(path)
    got = meshio.read_glb(path)
    assert got["basecolor_tex"] is None and np.array_equal(got["occlusion_tex"], np.asarray(shaded.occlusion_map_image()))
    assert np.array_equal(got["uvs"][:, 0], uvs[:, 0]) and got["uvs"].shape == uvs.shape     # (v goes through 1 - v twice)
    # beside a normal map: both textures, each under its own slot
    both = Mesh(v, f, None, uvs=uvs, texture=shaded.texture)
    both.occlusion_map = shaded.occlusion_map
    both.normal_map, both.normal_map_space = np.full((4, 4, 3), 0.5, np.float32), "tangent"
    both.export(path)
    got = meshio.read_glb(path)
    assert np.array_equal(got["occlusion_tex"], np.asarray(shaded.occlusion_map_image()))
    assert np.array_equal(got["normal_tex"], np.asarray(both.normal_map_image()))


def test_export_without_a_map_writes_the_bytes_it_wrote_before(tmp_path):
    from sculptmate_amd import meshio
    from sculptmate_amd.tsr.system import Mesh

    v, f, uvs, tex = _baked_arrays()
    m = Mesh(v, f, None, uvs=uvs, texture=tex)
    a, b, c = (str(tmp_path / n) for n in ("a.glb", "b.glb", "c.glb"))
    m.export(a)
    picture = np.asarray(m.texture_image())
    flat = v[f.reshape(-1)], np.arange(f.size, dtype=np.int64).reshape(-1, 3)
    meshio.write_glb(b, *flat, uvs=uvs, basecolor_tex=picture, normals=None)                       # today's call
    meshio.write_glb(c, *flat, uvs=uvs, basecolor_tex=picture, normals=None, occlusion_tex=None)
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    assert b"occlusionTexture" not in open(a, "rb").read()
    assert meshio.read_glb(a)["occlusion_tex"] is None
    m.export(str(tmp_path / "a.obj"))
    assert "map_Ka" not in open(str(tmp_path / "a.mtl")).read() and not (tmp_path / "a_ao.png").exists()


def test_export_obj_writes_map_ka_and_the_png(shaded, tmp_path):
    from sculptmate_amd import meshio

    path = str(tmp_path / "shaded.obj")
    shaded.export(path)
    mtl = open(str(tmp_path / "shaded.mtl")).read().splitlines()
    assert "map_Kd shaded.png" in mtl and "map_Ka shaded_ao.png" in mtl and not any(x.startswith("map_Bump") for x in mtl)
    with open(str(tmp_path / "shaded_ao.png"), "rb") as fh:
        assert np.array_equal(meshio.decode_png(fh.read()), np.asarray(shaded.occlusion_map_image()))
    v, f, c = meshio.read_obj(path)
    assert np.array_equal(v, shaded.vertices) and np.array_equal(f, shaded.faces)


def test_keep_components_carries_the_map(shaded, monkeypatch):
    from sculptmate_amd import ops

    keep_faces = np.array([2, 0])
    monkeypatch.setattr(ops, "mesh_keep_components", lambda v, f, keep: (v, f[keep_faces], np.arange(len(v)), keep_faces))
    out = shaded.keep_components("largest")
    assert out.occlusion_map is shaded.occlusion_map and out.occlusion_map_rule == (64, None)
    corner = (keep_faces[:, None] * 3 + np.arange(3)).reshape(-1)
    assert np.array_equal(out.uvs, shaded.uvs[corner]) and out.texture is shaded.texture
    # the methods that refuse a baked atlas refuse this one too (it comes with uvs)
    alone = type(shaded)(shaded.vertices, shaded.faces, None, uvs=shaded.uvs)
    alone.occlusion_map = shaded.occlusion_map
    with pytest.raises(ValueError, match="baked"):
        alone.simplify(0.5)
    with pytest.raises(ValueError, match="baked"):
        alone.subdivide(1)


def test_extract_mesh_hands_the_sink_nothing_new(shaded):
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import TSR

    m = TSR(SMALL_CFG)
    assert m.occlusion_map is None
    m.extract_meshes = lambda codes, *a, **k: [shaded]
    calls = []
    m.textured_mesh_sink = lambda v, f, uv, image, name, **kw: calls.append(kw)
    m.extract_mesh(None, enable_texture=True, mesh_name="A", bake_texture=8)
    m.occlusion_map = True          # the Blender sink has no occlusion input: the map stays on the mesh
    m.extract_mesh(None, enable_texture=True, mesh_name="B", bake_texture=8)
    assert calls == [{}, {}]


def test_reshaped_and_textured_launch_nothing_new_without_the_setting(monkeypatch):
    """With TSR.occlusion_map None, _reshaped keeps no source and _textured never reaches bake_occlusion_map."""
    from sculptmate_amd import ops
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import TSR

    m = TSR(SMALL_CFG)
    monkeypatch.setattr(ops, "mesh_simplify", lambda v, f, s: (v[:3], f[:1], None))
    v, f = _baked_arrays()[:2]
    out = m._reshaped(v, f, None, 1.0, 8, simplify=0.5)
    assert len(out) == 2 and out[0] is not v and m._occlusion_source is None
    m.occlusion_map = 8
    m._reshaped(v, f, None, 1.0, 8, simplify=0.5)
    assert m._occlusion_source.vertices is v and m._occlusion_source.faces is f
    m._reshaped(v, f, None, 1.0, 8)                                              # no simplify: no source
    assert m._occlusion_source is None
    m.occlusion_map = None
    monkeypatch.setattr(m, "bake_occlusion_map", lambda *a, **k: (_ for _ in ()).throw(AssertionError("not asked for")))
    mesh = m._textured(v, f, None, False, 0)
    assert mesh.occlusion_map is None and mesh.vertices is v


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_the_restatement_on_a_case_worked_by_hand():
    """One triangle under a ceiling: texel_position's guard, the interpolation, the snap and the flip, with values that can be
    checked by eye."""
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    F = np.array([[0, 1, 2]], np.int32)
    N = np.array([[0, 0, 1]] * 3, np.float32)
    # S: the same triangle lifted by 1/8 and wound the other way (its normal points down), large enough to cover the texels
    SP = np.array([[-4, -4, 0.125], [-4, 8, 0.125], [8, -4, 0.125]], np.float32)
    SF = np.array([[0, 1, 2]], np.int32)
    rast = np.zeros((2, 2, 4), np.float32)
    rast[..., 3] = -1
    rast[0, 0] = [0.5, 0.25, 0.25, 0]
    rast[0, 1] = [0.5, 0.25, 0.25, 1]          # tri out of range
    rast[1, 0] = [0.5, 0.25, 0.25, np.nan]
    covered, rows, p = A.texel_position(rast.reshape(-1, 4), V, F)
    assert covered.tolist() == [True, False, False, False] and p[0].tolist() == [0.25, 0.25, 0.0]
    dirs = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0]], np.float32)
    # no snap: the point is below the ceiling, the one direction that takes part (+z) is blocked
    ao, mask = A.bake_occlusion(rast, V, F, N, SP, SF, dirs, 0.0)
    assert mask.tolist() == [[True, False], [False, False]] and ao.tolist() == [[0.0, 0.0], [0.0, 0.0]]
    # cage 1/4: the ray from z = 1/4 down hits the ceiling at t = 1/2; the facet normal (0, 0, -1) is flipped to n's side; from
    # the ceiling itself +z is free (the ray starts on the face, offset 2^-10 above it)
    ao, mask, info = A.bake_occlusion(rast, V, F, N, SP, SF, dirs, 2.0 ** -10, cage=0.25, want_info=True)
    assert info["hit"].tolist() == [True, False, False, False] and info["flipped"].tolist() == [True, False, False, False]
    assert ao.tolist() == [[1.0, 0.0], [0.0, 0.0]]
    q, m, hit, flipped = A.snap(p[:1], N[:1], SP, SF, 0.25)
    assert q.tolist() == [[0.25, 0.25, 0.125]] and m.tolist() == [[0.0, 0.0, 1.0]]
    # cage 1/16 does not reach: the texel falls back to its own point and normal
    ao, mask, info = A.bake_occlusion(rast, V, F, N, SP, SF, dirs, 2.0 ** -10, cage=0.0625, want_info=True)
    assert not info["hit"].any() and ao[0, 0] == 0.0
