"""The normal-map bake on the host: the fp32 NumPy restatement of csrc/bake_normal.hip's two rules (tests/_nmapref.py) against its
fp64 form, the round trip through the decoded frame, handedness and the degenerate cases; the way out of the library (Mesh.export
to .glb and .obj, the textured Blender sink on tests/fake_bpy.py); signatures and refusals.  Runs on the CPU."""
import inspect
import json
import sys

import numpy as np
import pytest

import _nmapref as R
import fake_bpy

MIRRORED, FLATTENED = 3, 5      # the face whose chart is mirrored in u, and the face whose chart has no area

# fp32 against fp64 of the same formulas, largest component error, as this test prints it (numpy 1.26, any machine: IEEE fp32):
#   octahedron     tangents 1.2e-08   stored vector 1.0e-07
#   icosphere      tangents 9.5e-08   stored vector 1.3e-07
#   zero UV area   tangents 9.5e-08   stored vector 1.3e-07
# These figures are the yardstick the GPU leg refers to (there the kernels must equal the fp32 form bit for bit).  The bound
# below is not taken from them: both rules are chains of fewer than 32 fp32 roundings on quantities of magnitude <= 2 (unit
# normals, tangents of length <= 1, their products), with one division by a length and none by D; the final normalisation
# divides by a length >= sqrt(D) times the vector's scale, and D >= 0.2 on these inputs (the test below asserts 0.01 and prints
# the value).  32 roundings x 2^-24 x 2 (magnitude) x 2.5 (1 / sqrt(0.2), rounded up) = 160 x 2^-24.
FP32_BOUND = 160 * 2.0 ** -24        # 9.5e-06
# The largest angle between the world normal and what the fp32 restatement's stored vector decodes to (fp64 decode), over the
# three inputs, as test_round_trip prints it: 1.6e-07 rad.  The assertion allows 4 x that (a different but legal summation
# order of the final normalisation in a later refactor of the restatement; the kernel must equal the restatement bit for bit).
ROUND_TRIP_FP32 = 1.6e-07


def _inputs(name):
    """-> P, F, uvs, corner normals (f32) of one of the three inputs."""
    if name == "octahedron":
        P, F = R.octahedron()
        uv = R.cell_atlas(P, F)
    else:
        P, F = R.icosphere(1)
        uv = R.mirror_chart(R.cell_atlas(P, F), MIRRORED)
        if name == "zero_uv_area":
            uv = R.zero_area_chart(uv, FLATTENED)
    cn = R.vertex_normals(P, F)[F].reshape(-1, 3)
    return P, F, uv, cn


@pytest.fixture(scope="module", params=["octahedron", "icosphere_mirrored", "zero_uv_area"])
def case(request):
    P, F, uv, cn = _inputs(request.param)
    t32 = R.corner_tangents(P, F, uv, cn)
    bary, tri = R.samples(F, 12)
    n = R.bumpy_normals(P, F, bary, tri)
    s32, D = R.texel_transform(n, bary, tri, cn, t32)
    return dict(name=request.param, P=P, F=F, uv=uv, cn=cn, t32=t32, bary=bary, tri=tri, n=n, s32=s32, D=D)


def test_fp32_restatement_against_fp64(case):
    c = case
    t64 = R.corner_tangents(c["P"], c["F"], c["uv"], c["cn"], np.float64)
    s64, _ = R.texel_transform(c["n"], c["bary"], c["tri"], c["cn"], c["t32"], np.float64)
    assert c["t32"].dtype == np.float32 and c["s32"].dtype == np.float32
    et, es = np.abs(c["t32"] - t64).max(), np.abs(c["s32"] - s64).max()
    print("%s: fp32 against fp64, largest component error: tangents %.2g, stored vector %.2g" % (c["name"], et, es))
    assert np.array_equal(c["t32"][:, 3], t64[:, 3])                  # the same handedness and the same fallbacks
    assert et <= FP32_BOUND and es <= FP32_BOUND
    assert np.abs(np.linalg.norm(c["t32"][:, :3].astype(np.float64), axis=1) - 1).max() <= 4 * 2.0 ** -24
    assert np.abs(np.linalg.norm(c["s32"].astype(np.float64), axis=1) - 1).max() <= 4 * 2.0 ** -24


def test_round_trip(case):
    """Decoding the stored vector with the interpolated frame, as a shader does, gives back the world normal."""
    c = case
    back = R.decode(c["s32"], c["bary"], c["tri"], c["cn"], c["t32"])
    a = R.angle(back, c["n"]).max()
    print("%s: largest angle between the world normal and the decoded stored vector: %.3g rad" % (c["name"], a))
    assert a <= 4 * ROUND_TRIP_FP32


def test_the_frames_are_well_conditioned(case):
    """Condition, not measurement: D = |N x T|^2 >= 0.01 on every sample, so that the flat fallback is reached only by the
    dedicated degenerate case below."""
    print("%s: smallest D %.3g" % (case["name"], case["D"].min()))
    assert case["D"].min() >= 0.01
    assert not (case["s32"] == np.array([0, 0, 1], np.float32)).all(1).any()


def test_handedness_and_the_mirrored_chart():
    P, F, uv, cn = _inputs("icosphere_mirrored")
    t = R.corner_tangents(P, F, uv, cn).reshape(-1, 3, 4)
    assert (t[MIRRORED, :, 3] == -1).all() and (np.delete(t, MIRRORED, 0)[:, :, 3] == 1).all()
    # cross(N, T) * w points along dP/dv (fp64, from the definition)
    P64, u = P.astype(np.float64), uv.astype(np.float64).reshape(-1, 3, 2)
    e1, e2 = P64[F[:, 1]] - P64[F[:, 0]], P64[F[:, 2]] - P64[F[:, 0]]
    d1, d2 = u[:, 1] - u[:, 0], u[:, 2] - u[:, 0]
    det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
    dpdu = (e1 * d2[:, 1:2] - e2 * d1[:, 1:2]) / det[:, None]
    dpdv = (e2 * d1[:, 0:1] - e1 * d2[:, 0:1]) / det[:, None]
    assert (det[MIRRORED] < 0) and (np.delete(det, MIRRORED) > 0).all()
    N = cn.astype(np.float64).reshape(-1, 3, 3)
    B = np.cross(N, t[:, :, :3].astype(np.float64)) * t[:, :, 3:4]
    assert ((B * dpdv[:, None, :]).sum(-1) > 0).all()
    assert ((t[:, :, :3] * dpdu[:, None, :]).sum(-1) > 0).all()       # and T along dP/du
    assert np.abs((t[:, :, :3] * N).sum(-1)).max() <= 8 * 2.0 ** -24    # perpendicular to the corner's normal


def test_degenerate_cases_take_the_stated_fallback():
    P, F, uv, cn = _inputs("zero_uv_area")
    t = R.corner_tangents(P, F, uv, cn).reshape(-1, 3, 4)
    # the face without UV area: w = +1 and cross(N, axis of the smallest component), normalised
    assert (t[FLATTENED, :, 3] == 1).all()
    for k in range(3):
        N = cn.reshape(-1, 3, 3)[FLATTENED, k].astype(np.float64)
        e = np.eye(3)[np.argmin(np.abs(N))]
        want = np.cross(N, e) / np.linalg.norm(np.cross(N, e))
        assert np.abs(t[FLATTENED, k, :3] - want).max() <= 4 * 2.0 ** -24
    # a non-finite determinant, a normal parallel to dP/du, a zero normal and a NaN normal
    P1 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    F1 = np.array([[0, 1, 2]])
    uv1 = np.array([[0, 0], [1, 0], [0, 1]], np.float32)
    up = np.array([[0, 0, 1]] * 3, np.float32)
    assert np.array_equal(R.corner_tangents(P1, F1, uv1, up), np.array([[1, 0, 0, 1]] * 3, np.float32))
    assert np.array_equal(R.corner_tangents(P1, F1, np.array([[0, 0], [np.inf, 0], [0, 1]], np.float32), up)[:, 3], np.ones(3, np.float32))
    along = np.array([[1, 0, 0]] * 3, np.float32)                      # dP/du of this face is +x: t - N (N.t) = 0
    got = R.corner_tangents(P1, F1, uv1, along)
    assert np.array_equal(got, np.array([[0, 0, 1, 1]] * 3, np.float32))        # cross(x, y): y is the lower of the two tied axes
    assert np.array_equal(R.corner_tangents(P1, F1, uv1, 0 * up), np.array([[1, 0, 0, 1]] * 3, np.float32))
    assert np.array_equal(R.corner_tangents(P1, F1, uv1, np.nan * up), np.array([[1, 0, 0, 1]] * 3, np.float32))
    # the texel transform: a frame whose tangent is its normal has D = 0 -> the flat vector; so has a zero world normal
    bary = np.array([[0.25, 0.25, 0.5]], np.float32)
    tri = np.array([0])
    n = np.array([[0.6, 0, 0.8]], np.float32)
    flat = np.array([[0, 0, 1]], np.float32)
    s, D = R.texel_transform(n, bary, tri, up, np.concatenate([up, np.ones((3, 1), np.float32)], 1))
    assert D[0] == 0 and np.array_equal(s, flat)
    good = R.corner_tangents(P1, F1, uv1, up)
    assert np.array_equal(R.texel_transform(0 * n, bary, tri, up, good)[0], flat)
    assert np.array_equal(R.texel_transform(np.nan * n, bary, tri, up, good)[0], flat)
    assert np.array_equal(R.texel_transform(n, bary, tri, up, good)[0], n)      # the identity frame stores n itself


# ---------------------------------------------------------------------------------------------- the way out of the library
def _baked_arrays():
    """The data of test_bake_texture_host.py's `baked` fixture."""
    rng = np.random.default_rng(7)
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int64)
    uvs = rng.random((12, 2)).astype(np.float32)
    tex = rng.random((6, 5, 3)).astype(np.float32)
    return v, f, uvs, tex


@pytest.fixture()
def mapped():
    """The baked tetrahedron with a 4 x 4 tangent-space normal map and its frame."""
    from sculptmate_amd.tsr.system import Mesh

    v, f, uvs, tex = _baked_arrays()
    rng = np.random.default_rng(11)
    m = Mesh(v, f, None, uvs=uvs, texture=tex)
    n = rng.standard_normal((4, 4, 3))
    m.normal_map = (0.5 + 0.5 * n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)
    m.normal_map[0, 0] = [0.5, 0.5, 1.0]
    m.normal_map_space = "tangent"
    m.corner_normals = R.vertex_normals(v, f)[f].reshape(-1, 3)
    m.corner_tangents = R.corner_tangents(v, f, uvs, m.corner_normals)
    return m


def test_mesh_attributes_and_normal_map_image(mapped):
    from sculptmate_amd.tsr.system import Mesh

    plain = Mesh(mapped.vertices, mapped.faces)
    assert plain.normal_map is None and plain.normal_map_space is None and plain.corner_normals is None and plain.corner_tangents is None
    assert list(inspect.signature(Mesh.__init__).parameters)[-1] == "vertex_occlusion"      # no new constructor parameter
    img = mapped.normal_map_image()
    assert img.mode == "RGB" and img.size == (4, 4)
    want = np.clip(np.floor(256.0 * mapped.normal_map), 0, 255).astype(np.uint8)
    assert np.array_equal(np.asarray(img), want) and np.asarray(img)[0, 0].tolist() == [128, 128, 255]
    with pytest.raises(ValueError):
        plain.normal_map_image()


def test_export_glb_round_trip(mapped, tmp_path):
    from sculptmate_amd import meshio
    from sculptmate_amd.tsr.system import Mesh

    path = str(tmp_path / "mapped.glb")
    mapped.export(path)
    got = meshio.read_glb(path)
    assert np.array_equal(got["normal_tex"], np.asarray(mapped.normal_map_image()))
    assert np.array_equal(got["basecolor_tex"], np.asarray(mapped.texture_image()))
    assert np.array_equal(got["tangents"], mapped.corner_tangents) and got["tangents"].shape == (12, 4)
    assert np.array_equal(got["normals"], mapped.corner_normals)
    assert np.array_equal(got["vertices"], mapped.vertices[mapped.faces.reshape(-1)])
    assert np.array_equal(meshio.read_glb(path, uv_origin="top_left")["uvs"], np.stack([mapped.uvs[:, 0], np.float32(1.0) - mapped.uvs[:, 1]], 1))
    assert got["extra_images"] == {}
    raw = open(path, "rb").read()
    doc = json.loads(raw[20:20 + int.from_bytes(raw[12:16], "little")])
    assert "TANGENT" in doc["meshes"][0]["primitives"][0]["attributes"] and "normalTexture" in doc["materials"][0]
    # an object-space map never becomes normalTexture: a further image, named in the mesh's extras
    mapped.normal_map_space = "object"
    mapped.export(path)
    got = meshio.read_glb(path)
    assert got["normal_tex"] is None and got["tangents"] is None
    assert np.array_equal(got["extra_images"]["normal_map_object"], np.asarray(mapped.normal_map_image()))
    assert np.array_equal(got["basecolor_tex"], np.asarray(mapped.texture_image()))
    # a normal map alone (no texture) still goes out with its UVs
    v, f, uvs, _ = _baked_arrays()
    alone = Mesh(v, f, None, uvs=uvs)
    alone.normal_map, alone.normal_map_space = mapped.normal_map, "tangent"
    alone.corner_normals, alone.corner_tangents = mapped.corner_normals, mapped.corner_tangents
    alone.export(path)
    got = meshio.read_glb(path)
    assert got["basecolor_tex"] is None and np.array_equal(got["normal_tex"], np.asarray(mapped.normal_map_image()))


def test_export_without_a_map_writes_the_bytes_of_the_call_it_made_before(tmp_path):
    """normal_map None: Mesh.export's .glb is the file of the write_glb call it has always made (no tangents keyword, no
    extras), and write_glb(tangents=None) is write_glb without the keyword."""
    from sculptmate_amd import meshio
    from sculptmate_amd.tsr.system import Mesh

    v, f, uvs, tex = _baked_arrays()
    m = Mesh(v, f, None, uvs=uvs, texture=tex)
    assert m.normal_map is None
    a, b, c = (str(tmp_path / n) for n in ("a.glb", "b.glb", "c.glb"))
    m.export(a)
    picture = np.asarray(m.texture_image())
    meshio.write_glb(b, v[f.reshape(-1)], np.arange(f.size, dtype=np.int64).reshape(-1, 3), uvs=uvs, basecolor_tex=picture, normals=None)
    meshio.write_glb(c, v[f.reshape(-1)], np.arange(f.size, dtype=np.int64).reshape(-1, 3), uvs=uvs, basecolor_tex=picture, normals=None,
                     tangents=None, extra_images=None)
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    assert list(inspect.signature(meshio.write_glb).parameters)[-2:] == ["tangents", "extra_images"]
    assert inspect.signature(meshio.write_glb).parameters["tangents"].default is None
    m.export(str(tmp_path / "a.obj"))
    assert "map_Bump" not in open(str(tmp_path / "a.mtl")).read() and not (tmp_path / "a_normal.png").exists()
    with pytest.raises(ValueError):
        meshio.write_glb(c, v, f, tangents=np.zeros((3, 4), np.float32))


def test_export_obj_writes_map_bump_and_the_png(mapped, tmp_path):
    from sculptmate_amd import meshio

    path = str(tmp_path / "mapped.obj")
    mapped.export(path)
    mtl = open(str(tmp_path / "mapped.mtl")).read().splitlines()
    assert "map_Kd mapped.png" in mtl and "map_Bump -bm 1 mapped_normal.png" in mtl
    with open(str(tmp_path / "mapped_normal.png"), "rb") as fh:
        assert np.array_equal(meshio.decode_png(fh.read()), np.asarray(mapped.normal_map_image()))
    with open(str(tmp_path / "mapped.png"), "rb") as fh:
        assert np.array_equal(meshio.decode_png(fh.read()), np.asarray(mapped.texture_image()))
    v, f, c = meshio.read_obj(path)
    assert np.array_equal(v, mapped.vertices) and np.array_equal(f, mapped.faces)


def test_keep_components_carries_the_map_through_face_index(mapped, monkeypatch):
    from sculptmate_amd import ops

    keep_faces = np.array([2, 0])
    monkeypatch.setattr(ops, "mesh_keep_components", lambda v, f, keep: (v, f[keep_faces], np.arange(len(v)), keep_faces))
    out = mapped.keep_components("largest")
    corner = (keep_faces[:, None] * 3 + np.arange(3)).reshape(-1)
    assert out.normal_map is mapped.normal_map and out.normal_map_space == "tangent"
    assert np.array_equal(out.corner_normals, mapped.corner_normals[corner])
    assert np.array_equal(out.corner_tangents, mapped.corner_tangents[corner]) and np.array_equal(out.uvs, mapped.uvs[corner])


@pytest.fixture()
def bpy():
    keep = sys.modules.get("bpy")
    mod = fake_bpy.install()
    yield mod
    if keep is None:
        sys.modules.pop("bpy", None)
    else:
        sys.modules["bpy"] = keep


def test_textured_blender_sink_with_and_without_a_normal_image(mapped, bpy):
    from sculptmate_amd.tsr.blender_sink import import_textured_blender

    assert inspect.signature(import_textured_blender).parameters["normal_image"].default is None
    import_textured_blender(mapped.vertices, mapped.faces, mapped.uvs, mapped.texture_image(), "Plain")
    import_textured_blender(mapped.vertices, mapped.faces, mapped.uvs, mapped.texture_image(), "Bumpy", normal_image=mapped.normal_map_image())
    s = fake_bpy.summary(bpy)
    meta = json.loads(str(s["meta"]))
    plain, bumpy = meta["materials"]
    assert sorted(n["id"] for n in plain["nodes"]) == ["ShaderNodeBsdfPrincipled#0", "ShaderNodeOutputMaterial#0", "ShaderNodeTexImage#0"]
    assert len(plain["links"]) == 2
    assert sorted(n["id"] for n in bumpy["nodes"]) == ["ShaderNodeBsdfPrincipled#0", "ShaderNodeNormalMap#0", "ShaderNodeOutputMaterial#0",
                                                       "ShaderNodeTexImage#0", "ShaderNodeTexImage#1"]
    assert sorted(bumpy["links"]) == sorted([["ShaderNodeTexImage#0", "Color", "ShaderNodeBsdfPrincipled#0", "Base Color"],
                                             ["ShaderNodeBsdfPrincipled#0", "BSDF", "ShaderNodeOutputMaterial#0", "Surface"],
                                             ["ShaderNodeTexImage#1", "Color", "ShaderNodeNormalMap#0", "Color"],
                                             ["ShaderNodeNormalMap#0", "Normal", "ShaderNodeBsdfPrincipled#0", "Normal"]])
    images = {im["name"]: im for im in meta["images"]}
    assert len(images) == 3 and images["Bumpy_Normal"]["colorspace"] == "Non-Color" and images["Bumpy_BaseColor"]["colorspace"] == "sRGB"
    assert images["Bumpy_Normal"]["size"] == [4, 4]
    nodes = {n["id"]: n for n in bumpy["nodes"]}
    assert nodes["ShaderNodeTexImage#1"]["image"] == "Bumpy_Normal" and nodes["ShaderNodeTexImage#0"]["image"] == "Bumpy_BaseColor"


def test_extract_mesh_hands_the_normal_image_over_only_when_the_model_asks(mapped):
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import TSR

    m = TSR(SMALL_CFG)
    m.extract_meshes = lambda codes, *a, **k: [mapped]
    calls = []
    m.textured_mesh_sink = lambda v, f, uv, image, name, **kw: calls.append(kw)
    m.extract_mesh(None, enable_texture=True, mesh_name="A", bake_texture=8)
    m.normal_map = "tangent"
    m.extract_mesh(None, enable_texture=True, mesh_name="B", bake_texture=8)
    assert calls[0] == {} and list(calls[1]) == ["normal_image"]
    assert np.array_equal(np.asarray(calls[1]["normal_image"]), np.asarray(mapped.normal_map_image()))


# ---------------------------------------------------------------------------------------------- signatures and refusals
def test_signatures_defaults_and_refusals():
    import torch

    from sculptmate_amd import ops
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import TSR, Mesh

    assert TSR(SMALL_CFG).normal_map is None
    assert TripoGenerator(torch.device("cpu")).normal_map is None
    sig = inspect.signature(ops.bake_scene_normal)
    assert list(sig.parameters) == ["planes", "mlp", "v_pos", "faces", "rast", "radius", "frame"]
    assert sig.parameters["radius"].default == 0.87 and sig.parameters["frame"].default is None
    assert list(inspect.signature(ops.corner_tangents).parameters) == ["v_pos", "faces", "uvs", "corner_normals"]
    sig = inspect.signature(TSR.bake_normal_map)
    assert list(sig.parameters) == ["self", "mesh", "scene_code", "resolution", "space", "island_padding", "unwrapper"]
    assert sig.parameters["resolution"].default is None and sig.parameters["space"].default == "tangent"
    assert sig.parameters["island_padding"].default == 0.02 and sig.parameters["unwrapper"].default is None
    # the pinned signatures are where they were
    assert list(inspect.signature(TSR.extract_meshes).parameters)[-2:] == ["subdivide", "occlusion"]
    assert list(inspect.signature(TSR.extract_mesh).parameters)[-2:] == ["subdivide", "occlusion"]
    # a bad space is refused before anything else is looked at (no weights, no device, not even an initialised model)
    v, f, uvs, tex = _baked_arrays()
    with pytest.raises(ValueError, match="space"):
        TSR.__new__(TSR).bake_normal_map(Mesh(v, f), None, space="world")
    # CPU tensors are refused: no CPU fallback
    cpu = torch.zeros((4, 4, 4))
    with pytest.raises(ops.SculptError):
        ops.bake_scene_normal(torch.zeros((3, 40, 8, 8)), None, torch.from_numpy(v), torch.from_numpy(f), cpu)
    with pytest.raises(ops.SculptError):
        ops.corner_tangents(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(uvs), torch.zeros((12, 3)))
