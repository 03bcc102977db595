"""The displacement bake without a GPU: the fp64 run of the line rule (tests/_dispref.py line_search) on set A,
the rule's invariants, ops.displacement_rule, the DisplacementMap's 16-bit coding, the writers and the Blender sink.
tests/test_gpu_displacement.py then holds the device to the restatement bit for bit."""
import inspect
import json
import os
import sys

import numpy as np
import pytest

import _dispref as D
import _nmapref as N
import _projref as P
import fake_bpy

RES_TOL = 1e-3
# (start along n in cells, steps, cells): the cases of the issue
CASES = {"face_8_1": (0.0, 8, 1.0), "face_8_2": (0.0, 8, 2.0), "plus_8_1": (0.5, 8, 1.0), "plus_8_2": (0.5, 8, 2.0), "minus_8_1": (-0.5, 8, 1.0)}


def _run(start, steps, cells, **kw):
    A = P.mesh_set_a()
    p, n = D.face_points()
    p0 = p.astype(np.float64) + start * A["cell"] * n.astype(np.float64)
    out = D.line_search(A["planes"], A["Ws"], A["bs"], p0, n, A["target"], steps, cells * A["cell"], RES_TOL, np.float64, **kw)
    out["p0"], out["n"], out["max_dist"] = p0, n.astype(np.float64), float(np.float32(cells * A["cell"]))
    return out


@pytest.fixture(scope="module")
def runs():
    return {name: _run(*case) for name, case in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp64_rule_converges_on_set_a(runs, name):
    """At least 90 % of the 15 508 face points converge.  The reference alone, as this test prints it:
    face (8, 1) 96.2 %, face (8, 2) 96.7 %, +0.5 cell (8, 1) 96.1 %, +0.5 cell (8, 2) 97.2 %, -0.5 cell (8, 1) 93.9 %, at 2.9 .. 4.1
    evaluations per point and a median |r| of 2.2e-5 .. 3.4e-5.  What remains is mostly status 2: no root within max_dist."""
    o = runs[name]
    st = o["status"]
    share = float((st == 0).mean())
    print("%s: converged %.1f %% (%d of %d), statuses %s, %.2f evals, median |r| %.2e"
          % (name, 100 * share, (st == 0).sum(), st.size, np.bincount(st, minlength=4).tolist(), o["evals"].mean(),
             np.median(np.abs(o["residual"]))))
    assert st.size == 15508
    assert share >= 0.90


def test_the_safeguard_is_what_converges(runs):
    """From +0.5 cell at (8 steps, 1 cell) the unguarded Newton step -- the step of the rule's item 6 alone, which stops where
    the rule would pull it back (it leaves the trust interval) -- converges on at most 75 % of the points: 67.7 % here, the
    67.6 % of DESIGN.md 3.1h's table, against 96.1 % with the rule.  The share of the rule with item 7 alone taken out (the
    clamp of item 6 kept) is printed beside it: 92.5 %, so on this field the clamp carries most of the safeguard and the
    bisection the rest; the bound is held against the unguarded step, which is the run the 67.6 % was measured on."""
    plain = _run(*CASES["plus_8_1"], plain=True)
    no_bisect = _run(*CASES["plus_8_1"], safeguard=False)
    share = float((plain["status"] == 0).mean())
    print("unguarded step: %.1f %%; item 7 alone removed: %.1f %%; the rule: %.1f %%"
          % (100 * share, 100 * (no_bisect["status"] == 0).mean(), 100 * (runs["plus_8_1"]["status"] == 0).mean()))
    assert share <= 0.75
    assert (no_bisect["status"] == 0).mean() < (runs["plus_8_1"]["status"] == 0).mean()


@pytest.mark.parametrize("name", sorted(CASES))
def test_invariants(runs, name):
    o = runs[name]
    h, r = o["height"], o["residual"]
    assert np.all(np.abs(h) <= o["max_dist"])
    rad = np.float64(np.float32(P.RADIUS))
    inside = (np.abs(o["p0"] + h[:, None] * o["n"]) <= rad).all(1)
    started_outside = (np.abs(o["p0"]) > rad).any(1)     # a start shifted off a face near the box's side: only h = 0 stays out there
    print("%s: %d of %d points start outside the box" % (name, started_outside.sum(), h.size))
    assert np.all(inside | (started_outside & (h == 0)))
    assert np.all(np.abs(r) <= np.abs(o["r0"]))
    assert np.all(np.abs(r[o["status"] == 0]) <= np.float64(np.float32(RES_TOL)))
    assert np.all((o["evals"] >= 1) & (o["evals"] <= 9))


def test_fp32_rule_agrees_with_fp64_on_a_sample():
    """The same rule in np.float32: the heights of the points that converge in both differ by no more than the residual noise
    over the slope allows (|dh| <= 2 res_tol / |gn|, |gn| >= 1 on these points asserted)."""
    A = P.mesh_set_a()
    p, n = D.face_points()
    p, n = p[::31], n[::31]
    args = (A["planes"], A["Ws"], A["bs"], p, n, A["target"], 8, 2 * A["cell"], RES_TOL)
    lo, hi = D.line_search(*args, np.float32), D.line_search(*args, np.float64)
    both = (lo["status"] == 0) & (hi["status"] == 0)
    assert both.mean() > 0.9
    _, g = P.value_grad(A["planes"], A["Ws"], A["bs"], p.astype(np.float64) + hi["height"][:, None] * n, np.float64)
    gn = np.abs((g * n).sum(1))[both]
    assert gn.min() >= 1.0
    assert np.all(np.abs(lo["height"].astype(np.float64) - hi["height"])[both] <= 2 * RES_TOL / gn)


def test_hostile_inputs_in_numpy():
    A = P.mesh_set_a()
    p, n = D.face_points()
    p, n = p[:6].copy(), n[:6].copy()
    n[0] = 0.0
    n[1] = np.nan
    n[2, 0] = np.inf
    p[3] = np.nan
    p[4] = [2.0, 0.0, 0.0]
    o = D.line_search(A["planes"], A["Ws"], A["bs"], p, n, A["target"], 8, A["cell"], RES_TOL, np.float32)
    assert o["status"][:4].tolist() == [3, 3, 3, 3] and o["evals"][:4].tolist() == [0, 0, 0, 1]
    assert np.all(o["height"][:5] == 0)
    assert o["status"][5] in (0, 1, 2)


@pytest.mark.parametrize("value, want", [(True, (8, 2.0)), (np.bool_(True), (8, 2.0)), (1, (1, 2.0)), (64, (64, 2.0)), ((3, 0.5), (3, 0.5)),
                                         ((8, 8), (8, 8.0)), ((np.int64(5), np.float32(1.5)), (5, 1.5))])
def test_displacement_rule_accepts(value, want):
    from sculptmate_amd import ops

    assert ops.displacement_rule(value) == want


@pytest.mark.parametrize("value", [False, None, 0, 65, -1, 2.0, "8", (8,), (8, 0.0), (8, 8.5), (8, float("nan")), (0, 1.0), (65, 1.0),
                                   (8, "1"), [8, 1.0], (8, 1.0, 2)])
def test_displacement_rule_refuses(value):
    from sculptmate_amd import ops

    with pytest.raises(ValueError):
        ops.displacement_rule(value)


def test_api_surface(monkeypatch):
    import torch

    from sculptmate_amd import ops
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr import mesh
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import TSR

    assert TSR(SMALL_CFG).displacement_map is None and TSR.__new__(TSR).displacement_map is None
    assert TripoGenerator(torch.device("cpu")).displacement_map is None
    assert len(mesh.FIELDS) == 12 and "displacement" not in mesh.FIELDS     # the map is no Mesh field
    sig = inspect.signature(ops.project_along)
    assert list(sig.parameters)[:11] == ["planes", "mlp", "points", "directions", "target", "max_dist", "steps", "res_tol", "radius",
                                         "align_corners", "want"]
    for fn in (ops.bake_displacement, ops.bake_displacement_composed):
        assert list(inspect.signature(fn).parameters) == ["planes", "mlp", "v_pos", "faces", "normals", "rast", "target", "max_dist",
                                                          "steps", "res_tol", "radius", "want"]
    sig = inspect.signature(TSR.bake_displacement_map)
    assert list(sig.parameters) == ["self", "mesh", "scene_code", "threshold", "displacement", "resolution", "atlas_resolution",
                                    "island_padding", "unwrapper"]
    d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == {"threshold": 25.0, "displacement": True, "resolution": None, "atlas_resolution": None, "island_padding": 0.02,
                 "unwrapper": None}
    assert list(inspect.signature(mesh.Mesh.export).parameters) == ["self", "path", "displacement"]
    monkeypatch.delenv("SCULPT_DISTANCE_FORM", raising=False)
    assert ops.bake_displacement_route() is ops.bake_displacement       # the route without a host wait met the rule of 3.1e (3.1h)
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", "plain,composeddisplacement")
    assert ops.bake_displacement_route() is ops.bake_displacement_composed
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", "plain")
    assert ops.bake_displacement_route() is ops.bake_displacement


@pytest.mark.parametrize("kw", [dict(displacement=False), dict(displacement=None), dict(displacement=0), dict(displacement=65),
                                dict(displacement=(8, 0.0)), dict(displacement="8"), dict(threshold=0.0)])
def test_bake_displacement_map_refuses_before_anything_is_looked_at(kw):
    from sculptmate_amd.tsr.system import TSR, Mesh

    v, f = N.octahedron()
    with pytest.raises(ValueError):
        TSR.__new__(TSR).bake_displacement_map(Mesh(v, f), None, **kw)


def test_extract_meshes_refuses_a_bad_displacement_map_before_anything_is_launched():
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import TSR

    m = TSR(SMALL_CFG)
    m.displacement_map = (8, 0.0)
    with pytest.raises(ValueError):
        m.extract_meshes([None], resolution=32)


# ------------------------------------------------------------------------------------------------------------------------------
# the map, the writers, the sink
# ------------------------------------------------------------------------------------------------------------------------------
def _map(res=16, max_dist=0.03, seed=5):
    from sculptmate_amd.tsr.displacement import DisplacementMap

    rng = np.random.default_rng(seed)
    h = rng.uniform(-max_dist, max_dist, (res, res)).astype(np.float32)
    h[0, 0], h[0, 1], h[0, 2] = -max_dist, max_dist, 0.0
    mask = rng.random((res, res)) < 0.7
    status = np.where(mask, 0, -1).astype(np.int32)
    return DisplacementMap(h, mask, status, max_dist, evals=np.where(mask, 3, 0).astype(np.int32),
                           residual0=np.full((res, res), 0.5, np.float32), residual=np.full((res, res), 1e-5, np.float32))


def test_displacement_map_coding_and_png(tmp_path):
    from PIL import Image

    from sculptmate_amd.tsr.displacement import decode16

    m = _map()
    assert m.midlevel == 0.5 and m.scale == 2 * m.max_dist
    code = m.image()
    assert code.dtype == np.uint16 and code.shape == (16, 16)
    assert code[0, 0] == 0 and code[0, 1] == 65535 and code[0, 2] == 32768          # round(0.5 * 65535) = 32768 (ties to even)
    back = decode16(code, m.scale, m.midlevel)
    bound = m.scale / 65535 / 2 + np.spacing(np.float32(m.max_dist))
    err = np.abs(back.astype(np.float64) - m.height.astype(np.float64)).max()
    print("16-bit coding error %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    path = tmp_path / "d.png"
    m.save(path)
    with Image.open(path) as im:
        assert im.mode in ("I;16", "I;16B", "I")
        assert np.array_equal(np.asarray(im).astype(np.uint16), code)
    info = m.info()
    assert info["covered"] == int(m.mask.sum()) and info["status"][0] == info["covered"] and info["evals_per_texel"] == 3.0
    assert info["median_abs_residual_before"] == 0.5 and abs(info["median_abs_residual_after"] - 1e-5) < 1e-9


def _baked():
    from sculptmate_amd.tsr.system import Mesh

    v, f = N.octahedron()
    uvs = N.cell_atlas(v, f).astype(np.float32)
    tex = np.random.default_rng(3).random((16, 16, 3)).astype(np.float32)
    return Mesh(v, f, None, uvs=uvs, texture=tex)


def _files(folder):
    return {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}


def test_export_without_the_keyword_is_what_it_was(tmp_path):
    from sculptmate_amd import meshio
    from sculptmate_amd.tsr.system import Mesh

    m = _baked()
    plain = Mesh(m.vertices, m.faces, np.random.default_rng(1).random((len(m.vertices), 3)).astype(np.float32))
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (a, b, c):
        d.mkdir()
    for ext in ("obj", "ply", "glb"):
        m.export(str(a / ("baked." + ext)))
        m.export(str(b / ("baked." + ext)), displacement=None)
        plain.export(str(a / ("plain." + ext)))
        plain.export(str(b / ("plain." + ext)), displacement=None)
    # the writers' own output for the arguments export hands them: what the files were before the keyword existed
    f = np.asarray(m.faces)
    picture = np.asarray(m.texture_image())
    meshio.write_obj_textured(str(c / "baked.obj"), m.vertices, f, m.uvs, picture, normals=None)
    meshio.write_glb(str(c / "baked.glb"), np.asarray(m.vertices)[f.reshape(-1)], np.arange(f.size, dtype=np.int64).reshape(-1, 3),
                     uvs=m.uvs, basecolor_tex=picture, normals=None)
    meshio.write_ply(str(c / "baked.ply"), m.vertices, m.faces, vertex_colors=None, normals=None)
    for ext, w in (("obj", meshio.write_obj), ("ply", meshio.write_ply), ("glb", meshio.write_glb)):
        w(str(c / ("plain." + ext)), plain.vertices, plain.faces, vertex_colors=plain.vertex_colors, normals=None)
    fa, fb, fc = _files(a), _files(b), _files(c)
    assert sorted(fa) == sorted(fb) == sorted(fc) and "baked.mtl" in fa and "baked.png" in fa
    assert fa == fb and fa == fc


def test_export_with_a_displacement_map(tmp_path):
    from PIL import Image

    from sculptmate_amd import meshio
    from sculptmate_amd.tsr.system import Mesh

    m, dm = _baked(), _map()
    m.export(str(tmp_path / "d.obj"), displacement=dm)
    m.export(str(tmp_path / "p.obj"))
    mtl = open(tmp_path / "d.mtl").read()
    assert mtl.replace("d_material", "p_material").replace("d.png", "p.png") == open(tmp_path / "p.mtl").read() \
        + "disp -mm %.9g %.9g d_disp.png\n" % (-dm.scale / 2, dm.scale)
    assert mtl.endswith("disp -mm %.9g %.9g d_disp.png\n" % (-dm.scale / 2, dm.scale))
    assert open(tmp_path / "d.obj").read().replace("d.mtl", "p.mtl").replace("d_material", "p_material") == open(tmp_path / "p.obj").read()
    with Image.open(tmp_path / "d_disp.png") as im:
        assert np.array_equal(np.asarray(im).astype(np.uint16), dm.image())
    m.export(str(tmp_path / "d.glb"), displacement=dm)
    m.export(str(tmp_path / "p.glb"))
    got, ref = meshio.read_glb(str(tmp_path / "d.glb")), meshio.read_glb(str(tmp_path / "p.glb"))
    for k in ("vertices", "faces", "uvs", "basecolor_tex"):
        assert np.array_equal(got[k], ref[k])
    import struct

    data = open(tmp_path / "d.glb", "rb").read()
    n_json = struct.unpack("<I", data[12:16])[0]
    doc = json.loads(data[20:20 + n_json])
    extras = doc["meshes"][0]["extras"]["displacement"]
    assert extras["scale"] == dm.scale and extras["midlevel"] == 0.5
    image = doc["images"][extras["image"]]
    assert image["name"] == "displacement" and image["mimeType"] == "image/png"
    view = doc["bufferViews"][image["bufferView"]]
    blob = data[28 + n_json:]
    import io

    with Image.open(io.BytesIO(blob[view["byteOffset"]:view["byteOffset"] + view["byteLength"]])) as im:
        assert np.array_equal(np.asarray(im).astype(np.uint16), dm.image())
    assert all(i != extras["image"] for i in [t["source"] for t in doc.get("textures", [])])   # no material refers to it
    # a map without an atlas is refused; .ply has no slot and stays what it was
    v, f = N.octahedron()
    with pytest.raises(ValueError):
        Mesh(v, f).export(str(tmp_path / "x.obj"), displacement=dm)
    m.export(str(tmp_path / "d.ply"), displacement=dm)
    m.export(str(tmp_path / "p.ply"))
    assert open(tmp_path / "d.ply", "rb").read() == open(tmp_path / "p.ply", "rb").read()


@pytest.fixture()
def bpy():
    keep = sys.modules.get("bpy")
    mod = fake_bpy.install()
    yield mod
    if keep is None:
        sys.modules.pop("bpy", None)
    else:
        sys.modules["bpy"] = keep


def test_blender_displacement_sink(bpy):
    from sculptmate_amd.tsr.blender_sink import add_displacement_blender, import_textured_blender

    m, dm = _baked(), _map()
    import_textured_blender(m.vertices, m.faces, m.uvs, m.texture_image(), "Plain")
    before = json.loads(str(fake_bpy.summary(bpy)["meta"]))["materials"][0]
    obj = import_textured_blender(m.vertices, m.faces, m.uvs, m.texture_image(), "Moved")
    node = add_displacement_blender(obj, dm)
    s = fake_bpy.summary(bpy)
    meta = json.loads(str(s["meta"]))
    plain, moved = meta["materials"]
    assert plain["nodes"] == before["nodes"] and plain["links"] == before["links"]             # the existing sink's graph is what it was
    assert sorted(n["id"] for n in moved["nodes"]) == ["ShaderNodeBsdfPrincipled#0", "ShaderNodeDisplacement#0", "ShaderNodeOutputMaterial#0",
                                                       "ShaderNodeTexImage#0", "ShaderNodeTexImage#1"]
    assert [l for l in moved["links"] if l not in plain["links"]] == sorted(
        [["ShaderNodeDisplacement#0", "Displacement", "ShaderNodeOutputMaterial#0", "Displacement"],
         ["ShaderNodeTexImage#1", "Color", "ShaderNodeDisplacement#0", "Height"]])
    values = {n["id"]: n["input_values"] for n in moved["nodes"]}["ShaderNodeDisplacement#0"]
    assert values == {"Midlevel": 0.5, "Scale": dm.scale}
    assert node.type == "ShaderNodeDisplacement"
    images = {im["name"]: (i, im) for i, im in enumerate(meta["images"])}
    i, im = images["Moved_Displacement"]
    assert im["colorspace"] == "Non-Color" and im["size"] == [16, 16]
    px = s["image%d.pixels" % i].reshape(16, 16, 4)
    assert np.array_equal(px[..., 0], np.flip(dm.image().astype(np.float32) / np.float32(65535.0), 0)) and np.all(px[..., 3] == 1)
