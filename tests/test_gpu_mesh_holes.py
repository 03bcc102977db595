"""Fill holes on the device (csrc/mesh_holes.hip; ops.mesh_border_loops, ops.mesh_fill_holes) against the NumPy restatement
(tests/_holesref.py), bit for bit: the vertices as fp32 bits, the faces, every count of `info`, and the labels and lengths of the
border loops -- on the smallest meshes at which each part can go wrong (loops of 3 and 4, loops longer than a wave and than a
workgroup, scattered half-edge ids, pinched vertices, a loop of 5 000 edges that needs 14 doubling rounds); then the `fill_holes`
keyword end to end on the small model."""
import functools

import numpy as np
import pytest
import torch

import _holesref as H
import _reportref as R
from sculptmate_amd import ops

pytestmark = pytest.mark.gpu

MESHES = {name: functools.partial(H.golden, name) for name in H.GOLDEN_NAMES}
MESHES.update(lidless=H.lidless, rim_fan=H.rim_fan, bow_tie=H.bow_tie, flipped=H.flipped_beside_hole, punched_grid=H.punched_grid,
              triangle=H.triangle, icosphere=lambda: R.icosphere(2), torus=lambda: R.torus(12, 8))
COUNTS = ("border_half_edges", "loops", "open_half_edges", "pinched_vertices")
RULES = [True, 3, 4, 8, 6000]          # 6000: above the longest loop of every mesh here


@functools.lru_cache(maxsize=None)
def _mesh(name):
    v, f = MESHES[name]()
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int64)


@functools.lru_cache(maxsize=None)
def _loops(name):
    return H.border_loops(_mesh(name)[1])


@functools.lru_cache(maxsize=None)
def _filled(name, rule):
    """The restatement of one mesh under one rule, computed once and shared by the tests (never modified)."""
    return H.fill_holes(*_mesh(name), rule)


def _dev(cuda, v, f, vdtype=torch.float32, fdtype=torch.int64):
    return torch.from_numpy(v).to(cuda).to(vdtype), torch.from_numpy(f).to(cuda).to(fdtype)


def _same(got, want, f_dtype=torch.int64):
    """The device's (V, F, A, info) equal the restatement's, NaN payloads aside."""
    V, F, A, info = got
    rV, rF, rA, rinfo = want
    assert info == rinfo, (info, rinfo)
    assert V.dtype == torch.float32 and F.dtype == f_dtype and V.shape == rV.shape and F.shape == rF.shape
    assert np.array_equal(V.cpu().numpy().view(np.uint32), rV.view(np.uint32))
    assert np.array_equal(F.cpu().numpy().astype(np.int64), rF)
    assert (A is None) == (rA is None)
    if A is not None:
        a = A.cpu().numpy()
        nan = np.isnan(rA)
        assert a.shape == rA.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.uint32), rA[~nan].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------- the loops
@pytest.mark.parametrize("name", list(MESHES))
def test_border_loops_equal_the_restatement(cuda, name):
    v, f = _mesh(name)
    want = _loops(name)
    got = ops.mesh_border_loops(*_dev(cuda, v, f, fdtype=torch.int32))
    print(name, {k: got[k] for k in COUNTS}, "longest", int(want["lengths"].max()) if want["loops"] else 0)
    assert {k: got[k] for k in COUNTS} == {k: want[k] for k in COUNTS}
    for k in ("half_edges", "labels", "leaders", "lengths"):
        assert got[k].dtype == torch.int32 and np.array_equal(got[k].cpu().numpy().astype(np.int64), want[k]), k
    again = ops.mesh_border_loops(*_dev(cuda, v, f))
    assert all(torch.equal(again[k], got[k]) for k in ("half_edges", "labels", "leaders", "lengths"))


# -------------------------------------------------------------------------------------------------------------- the fill
@pytest.mark.parametrize("name", list(MESHES))
def test_fill_equals_the_restatement(cuda, name):
    v, f = _mesh(name)
    got = ops.mesh_fill_holes(*_dev(cuda, v, f))
    print(name, got[3])
    _same(got, _filled(name, True))
    again = ops.mesh_fill_holes(*_dev(cuda, v, f))                        # two runs: the same bits
    assert torch.equal(again[0].view(torch.int32), got[0].view(torch.int32)) and torch.equal(again[1], got[1]) and again[3] == got[3]
    _same(ops.mesh_fill_holes(*_dev(cuda, v, f, fdtype=torch.int32)), _filled(name, True), torch.int32)
    # what the report says of the result
    before, after, info = R.report(v, f, False), ops.mesh_report(got[0], got[1], self_intersections=False), got[3]
    assert after["border_edges"] == info["open_half_edges"]
    for k in ("nonmanifold_edges", "inconsistent_edges", "components"):
        assert after[k] == before[k], k
    assert after["euler"] == before["euler"] + info["filled_loops"]
    assert after["referenced_vertices"] == before["referenced_vertices"] + info["new_vertices"]


@pytest.mark.parametrize("rule", RULES[1:])
@pytest.mark.parametrize("name", ["gyroid", "ints", "noise_a", "slab", "lidless", "triangle", "punched_grid", "rim_fan"])
def test_max_edges(cuda, name, rule):
    v, f = _mesh(name)
    got = ops.mesh_fill_holes(*_dev(cuda, v, f), rule)
    _same(got, _filled(name, rule))
    after = ops.mesh_report(got[0], got[1], self_intersections=False)
    assert after["border_edges"] == got[3]["open_half_edges"] + H.skipped_edges(f, rule)
    if rule == 6000:
        assert got[3] == _filled(name, True)[3]


@pytest.mark.parametrize("name", ["noise_b", "ints", "lidless"])
def test_fp16_positions(cuda, name):
    v, f = _mesh(name)
    v16 = v.astype(np.float16)
    _same(ops.mesh_fill_holes(*_dev(cuda, v16.astype(np.float32), f, vdtype=torch.float16)), H.fill_holes(v16, f))


@pytest.mark.parametrize("channels", [3, 8])
def test_attributes(cuda, channels):
    v, f = _mesh("noise_a")
    a = np.random.default_rng(channels).random((len(v), channels), dtype=np.float32)
    V, F = _dev(cuda, v, f)
    _same(ops.mesh_fill_holes(V, F, True, attributes=torch.from_numpy(a).to(cuda)), H.fill_holes(v, f, True, a))
    L = _loops("noise_a")
    poisoned = a.copy()
    poisoned[f.reshape(-1)[L["half_edges"][5]], 1] = np.nan             # one term of one loop
    got = ops.mesh_fill_holes(V, F, True, attributes=torch.from_numpy(poisoned).to(cuda))
    want = H.fill_holes(v, f, True, poisoned)
    _same(got, want)
    assert np.isnan(want[2][len(v):]).sum() == 1 and np.isnan(got[2][len(v):].cpu().numpy()).sum() == 1
    with pytest.raises(ops.SculptError):
        ops.mesh_fill_holes(V, F, True, attributes=torch.zeros((len(v), 9), device=cuda))


@pytest.mark.parametrize("name", ["noise_a", "ints", "punched_grid"])
def test_a_permutation_of_the_faces(cuda, name):
    v, f = _mesh(name)
    g = np.ascontiguousarray(f[np.random.default_rng(17).permutation(len(f))])
    _same(ops.mesh_fill_holes(*_dev(cuda, v, g)), H.fill_holes(v, g))
    got, want = ops.mesh_border_loops(*_dev(cuda, v, g)), H.border_loops(g)
    for k in ("half_edges", "labels", "leaders", "lengths"):
        assert np.array_equal(got[k].cpu().numpy().astype(np.int64), want[k]), k


def test_known_truths(cuda):
    V, F, _, info = ops.mesh_fill_holes(*_dev(cuda, *_mesh("lidless")))
    r = ops.mesh_report(V, F)
    assert (info["loops"], len(V), len(F)) == (1, 9, 14) and V[8].tolist() == [0.0, 2.0, 2.0]
    assert r["is_watertight"] and r["is_winding_consistent"] and r["genus"] == 0 and r["self_intersections"] == 0
    assert r["area"] == 96.0 and abs(r["volume"]) == 64.0
    V, F, _, info = ops.mesh_fill_holes(*_dev(cuda, *_mesh("triangle")))
    assert F.tolist() == [[0, 1, 2], [1, 0, 2]] and len(V) == 3
    for name in ("bow_tie", "flipped"):
        v, f = _mesh(name)
        V, F, _, info = ops.mesh_fill_holes(*_dev(cuda, v, f))
        assert info["loops"] == 0 and info["open_half_edges"] == info["border_half_edges"] > 0 and info["pinched_vertices"] > 0
        assert np.array_equal(F.cpu().numpy(), f) and np.array_equal(V.cpu().numpy(), v)
    # idempotent once nothing is open
    V, F, _, info = ops.mesh_fill_holes(*_dev(cuda, *_mesh("noise_a")))
    V2, F2, _, again = ops.mesh_fill_holes(V, F)
    assert info["open_half_edges"] == 0 and again["border_half_edges"] == 0 and torch.equal(F2, F) and torch.equal(V2, V)


def test_closed_and_empty_meshes_come_back(cuda):
    for name in ("icosphere", "torus"):
        v, f = _mesh(name)
        V, F, A, info = ops.mesh_fill_holes(*_dev(cuda, v, f))
        assert A is None and not any(info.values()) and np.array_equal(V.cpu().numpy(), v) and np.array_equal(F.cpu().numpy(), f)
        assert ops.mesh_border_loops(*_dev(cuda, v, f))["half_edges"].shape == (0,)
    V0, F0 = torch.zeros((3, 3), device=cuda), torch.zeros((0, 3), dtype=torch.int64, device=cuda)
    V, F, A, info = ops.mesh_fill_holes(V0, F0)
    assert torch.equal(V, V0) and F.shape == (0, 3) and F.dtype == torch.int64 and not any(info.values())
    assert set(info) == {"border_half_edges", "loops", "open_half_edges", "pinched_vertices", "filled_loops", "filled_edges",
                         "skipped_loops", "new_vertices", "new_faces"}
    got = ops.mesh_border_loops(V0, F0)
    assert got["loops"] == 0 and got["labels"].shape == (0,) and got["lengths"].shape == (0,)


def test_refusals(cuda):
    V, F = _dev(cuda, *_mesh("lidless"))
    for fn in (ops.mesh_border_loops, ops.mesh_fill_holes):
        with pytest.raises(ops.SculptError):
            fn(V.cpu(), F.cpu())
        bad = F.clone()
        bad[3, 1] = len(V)
        with pytest.raises(ops.SculptError, match="out of range"):
            fn(V, bad)
        bad = F.clone()
        bad[3, 1] = bad[3, 0]
        with pytest.raises(ops.SculptError, match="repeated"):
            fn(V, bad)
        nan = V.clone()
        nan[2, 0] = float("nan")
        with pytest.raises(ops.SculptError, match="non-finite"):
            fn(nan, F)
    with pytest.raises(ValueError, match="fill_holes"):
        ops.mesh_fill_holes(V, F, 2)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_mesh_methods(cuda):
    from sculptmate_amd.tsr import mesh as M

    v, f = _mesh("slab")
    V, F = _dev(cuda, v, f)
    colors = torch.rand((len(v), 3), device=cuda, generator=torch.Generator(cuda).manual_seed(3))
    m = M.Mesh(V, F, colors, vertex_normals=torch.zeros_like(V), vertex_occlusion=torch.zeros(len(v), device=cuda))
    m.quads = torch.zeros((1, 4), dtype=torch.int64, device=cuda)
    L = _loops("slab")
    assert m.border_loops() == dict({k: L[k] for k in COUNTS}, lengths=sorted(L["lengths"].tolist()))
    out = m.fill_holes()
    _same((out.vertices, out.faces, out.vertex_colors, _filled("slab", True)[3]), H.fill_holes(v, f, True, colors.cpu().numpy()))
    assert all(getattr(out, name) is None for name in M.FIELDS if name != "vertex_colors") and len(M.FIELDS) == 12
    assert out.is_watertight and not m.is_watertight
    assert len(m.fill_holes(4).faces) == len(f) + _filled("slab", 4)[3]["new_faces"]


def test_extract_meshes_fill_holes(cuda):
    from _tsrmodel import small_model

    s = small_model(cuda, 32)
    m, plain = s["m"], s["plain"]
    nv, nf = len(plain.vertices), len(plain.faces)
    same = m.extract_meshes(s["codes"], fill_holes=None, **s["kw"])[0]
    assert torch.equal(same.vertices.view(torch.int32), plain.vertices.view(torch.int32)) and torch.equal(same.faces, plain.faces)
    filled = m.extract_meshes(s["codes"], fill_holes=True, report=True, **s["kw"])[0]
    info = ops.mesh_fill_holes(plain.vertices, plain.faces)[3]
    print("the small model's mesh:", info)
    assert info["border_half_edges"] > 0 and info["skipped_loops"] == 0
    assert m.last_reports[0]["border_edges"] == info["open_half_edges"] + 0      # True skips no loop
    assert len(filled.vertices) == nv + info["new_vertices"] and len(filled.faces) == nf + info["new_faces"]
    assert torch.equal(filled.vertices[:nv].view(torch.int32), plain.vertices.view(torch.int32))
    assert torch.equal(filled.faces[:nf], plain.faces) and filled.faces.dtype == plain.faces.dtype
    _same(ops.mesh_fill_holes(plain.vertices, plain.faces), H.fill_holes(plain.vertices.cpu().numpy(), plain.faces.cpu().numpy()),
          plain.faces.dtype)
    some = m.extract_meshes(s["codes"], fill_holes=4, report=True, **s["kw"])[0]
    info4 = ops.mesh_fill_holes(plain.vertices, plain.faces, 4)[3]
    assert m.last_reports[0]["border_edges"] == info4["open_half_edges"] + H.skipped_edges(plain.faces.cpu().numpy(), 4)
    assert len(some.faces) == nf + info4["new_faces"]
    with pytest.raises(ValueError, match="fill_holes"):
        m.extract_meshes(None, fill_holes=2, **s["kw"])


def test_generator_fill_holes_reaches_the_model(cuda, tmp_path):
    import types

    from test_host_logic import _write_checkpoint

    from sculptmate_amd import synth
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr.spec import SMALL_CFG

    _write_checkpoint(str(tmp_path), SMALL_CFG, seed=61)
    g = TripoGenerator(cuda)
    assert g.fill_holes is None
    g.checkpoint_dir = str(tmp_path)
    g.mc_resolution = 32
    assert g.initiate_model() == 0
    g.model.mesh_sink = lambda *a: None
    orig, seen = g.model.extract_mesh, []

    def reachable(self, codes, **kw):   # random weights never reach the default threshold: take the grid's median
        seen.append(kw.get("fill_holes"))
        return orig(codes, **dict(kw, threshold=float(ops.density_grid(codes[0].contiguous(), self.decoder, kw["resolution"]).median())))

    g.model.extract_mesh = types.MethodType(reachable, g.model)
    img = (synth.composite_rgb(synth.image_rgba(seed=62, size=SMALL_CFG["cond_image_size"])) * 255).astype(np.uint8)
    assert g.generate_mesh(img, "plain") == 0
    plain = g.last_meshes[0]
    g.fill_holes = 8
    assert g.generate_mesh(img, "filled") == 0 and seen == [None, 8]
    want = ops.mesh_fill_holes(plain.vertices, plain.faces, 8)
    got = g.last_meshes[0]
    assert torch.equal(got.faces, want[1]) and torch.equal(got.vertices.view(torch.int32), want[0].view(torch.int32))
    assert want[3]["border_half_edges"] > 0
