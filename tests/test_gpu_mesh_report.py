"""The mesh report on the device (csrc/mesh_report.hip; ops.mesh_report, ops.mesh_self_intersections) against the NumPy
restatement (tests/_reportref.py): every integer of the report, the flags and the sorted pair list equal the brute force over all
pairs in both kernel forms; area2 and vol6 bit for bit per face; the two sums within the bound of a reordered fp64 sum,
|S - S_ref| <= Nf 2^-52 sum|x|; and the `report` keyword end to end on the small model."""
import functools
import os

import numpy as np
import pytest
import torch

import _reportref as R
from sculptmate_amd import ops

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FORMS = ["default", "plain"]
INTEGERS = ("vertices", "faces", "referenced_vertices", "edges", "border_edges", "nonmanifold_edges", "inconsistent_edges",
            "degenerate_faces", "components", "euler", "is_watertight", "is_winding_consistent", "genus", "is_volume",
            "self_intersections", "self_intersecting_faces")


# ---------------------------------------------------------------------------------------------------------------- meshes
def _lidless():
    v, f = R.cube(4.0)
    return v, f[2:]


def _joined():
    v, f = R.join(R.cube(4.0), R.cube(4.0, (4, 4, 0)))
    f = f.copy()
    f[f == 8] = 6
    f[f == 9] = 7
    return v, f


def _flipped():
    v, f = R.cube(4.0)
    f = f.copy()
    f[5] = f[5][::-1]
    return v, f


def _degenerate():
    v, f = R.cube(4.0)
    return np.concatenate([v, np.float32([[1, 1, 1], [2, 2, 2], [3, 3, 3], [9, 9, 9]])]), np.concatenate([f, [[0, 0, 5], [8, 9, 10]]])


def _triangles(v, f):
    return lambda: (np.float32(v), np.int64(f))


def _golden(name):
    def load():
        z = np.load(os.path.join(GOLDEN, "mc_skimage.npz"))
        return z[name + "_verts"], z[name + "_faces"].astype(np.int64)
    return load


def _soup(n, seed=5, size=0.3):
    """n random triangles of about `size` in the unit cube: many of them cross."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 1, (n, 1, 3))
    return (c + rng.uniform(-size, size, (n, 3, 3))).reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int64).reshape(n, 3)


def _hedgehog(n=200):
    """Long thin triangles that all cross near one point: the middle cell lists every face, and nearly every pair intersects."""
    rng = np.random.default_rng(11)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    w = np.cross(d, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    c = rng.uniform(-0.01, 0.01, (n, 3))
    v = np.stack([c - 2.0 * d, c + 2.0 * d - 0.3 * w, c + 2.0 * d + 0.3 * w], 1)   # c lies on the median, well inside
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int64).reshape(n, 3)


def _giant():
    """One very large triangle (in the MIDDLE of the face list: it is the walker of half its pairs and the listed face of the
    others) through a cloud of 2 000 tiny ones: its box spans the grid, so every pair of it shares many cells."""
    v, f = _soup(2000, seed=7, size=0.02)
    big = np.float32([[-0.6, -0.5, 0.45], [1.7, -0.4, 0.5], [0.4, 1.8, 0.56]])
    f = np.concatenate([f[:1000], [[len(v), len(v) + 1, len(v) + 2]], f[1000:]])
    return np.concatenate([v, big]), f


def _corners():
    """Crossing pairs in the grid's first and last cell along every axis -- their boxes END at the bounds, where the cell index is
    clamped -- with a filler cloud in between so that the grid has many cells."""
    fv, ff = _soup(300, seed=9, size=0.05)
    fv = fv * np.float32(0.8) + np.float32(0.1)
    vs, fs = [fv], [ff]
    base = len(fv)
    for corner in np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64):
        s = 1.0 - 2.0 * corner                                       # pointing into the box
        a = np.array([[0, 0, 0], [0.06, 0, 0], [0, 0.06, 0.03]]) * s + corner          # its first corner IS the box's
        b = np.array([[0.02, 0.02, 0], [0.02, 0.02, 0.04], [0.03, 0.025, 0.04]]) * s + corner   # its first edge pierces a
        vs += [a, b]
        fs += [np.int64([[base, base + 1, base + 2], [base + 3, base + 4, base + 5]])]
        base += 6
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs)


def _two_icospheres():
    return R.join(R.icosphere(3), R.icosphere(3, center=(0.71, 0.23, 0.117)))


MESHES = {
    "cube": lambda: R.cube(4.0),
    "torus48x24": R.torus,
    "lidless": _lidless,
    "joined": _joined,
    "flipped": _flipped,
    "degenerate": _degenerate,
    "cubes_integer": lambda: R.join(R.cube(4.0), R.cube(4.0, (1, 1, 1))),
    "cubes_generic": lambda: R.join(R.cube(4.0), R.cube(4.0, (0.5, 1.5, 2.25))),
    "cubes_touching": lambda: R.join(R.cube(4.0), R.cube(4.0, (4, 0, 0))),
    "pierced": _triangles([[0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 1, -1], [1, 1, 1], [5, 5, 1]], [[0, 1, 2], [3, 4, 5]]),
    "shared_vertex": _triangles([[0, 0, 0], [4, 0, 0], [0, 4, 0], [2, 2, -2], [2, 2, 2]], [[0, 1, 2], [0, 3, 4]]),
    "coplanar": _triangles([[0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 0]], [[0, 1, 2], [1, 3, 2], [0, 1, 3]]),
    "mc_sphere": _golden("sphere"),
    "mc_torus": _golden("torus"),
    "mc_noise_a": _golden("noise_a"),
    "mc_gyroid": _golden("gyroid"),
    "mc_ints": _golden("ints"),
    "two_icospheres": _two_icospheres,
    "hedgehog": _hedgehog,
    "giant": _giant,
    "corners": _corners,
}
for _n in (1, 2, 63, 65, 257):
    MESHES["soup%d" % _n] = functools.partial(_soup, _n)

# the counts tests/test_mesh_report_host.py pins on the restatement: the device must give them too
KNOWN_PAIRS = {"cube": 0, "cubes_integer": 18, "cubes_generic": 12, "cubes_touching": 0, "pierced": 1, "shared_vertex": 1, "coplanar": 0,
               "mc_sphere": 0, "mc_torus": 0, "mc_noise_a": 0, "mc_gyroid": 0, "mc_ints": 38}


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The restatement of one mesh, computed once and shared by the tests (never modified)."""
    v, f = MESHES[name]()
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int64)
    pairs, flags = R.self_intersections(v, f)
    return dict(v=v, f=f, report=R.report(v, f, self_intersections_too=False), pairs=pairs, flags=flags, measures=R.face_measures(v, f))


def _dev(cuda, v, f, dtype=torch.int32):
    return torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda).to(dtype)


def _set_form(monkeypatch, form):
    if form == "plain":
        monkeypatch.setenv("SCULPT_DISTANCE_FORM", "plain")
    else:
        monkeypatch.delenv("SCULPT_DISTANCE_FORM", raising=False)


def _sum_bound(x):
    return len(x) * 2.0 ** -52 * float(np.abs(x).sum())


# ---------------------------------------------------------------------------------------------------------------- the report
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("name", list(MESHES))
def test_report_equals_the_restatement(cuda, name, dtype):
    ref = _ref(name)
    want = dict(ref["report"], self_intersections=len(ref["pairs"]), self_intersecting_faces=int(ref["flags"].sum()))
    V, F = _dev(cuda, ref["v"], ref["f"], dtype)
    got = ops.mesh_report(V, F)
    print(name, {k: got[k] for k in INTEGERS})
    assert {k: got[k] for k in INTEGERS} == {k: want[k] for k in INTEGERS}
    assert set(got) == set(INTEGERS) | {"area", "volume"}
    if name in KNOWN_PAIRS:
        assert got["self_intersections"] == KNOWN_PAIRS[name]
    # per face bit for bit; the sums within the bound of a reordered sum
    area2, vol6 = ops.mesh_face_measures(V, F)
    ra, rv, _ = ref["measures"]
    assert np.array_equal(area2.cpu().numpy().view(np.int64), ra.view(np.int64))
    assert np.array_equal(vol6.cpu().numpy().view(np.int64), rv.view(np.int64))
    sa, sv = float(area2.sum()), float(vol6.sum())
    print("  sums: area2 %r (ref %r, bound %.3g), vol6 %r (ref %r, bound %.3g)" % (sa, float(ra.sum()), _sum_bound(ra), sv, float(rv.sum()), _sum_bound(rv)))
    assert abs(sa - float(ra.sum())) <= _sum_bound(ra) and abs(sv - float(rv.sum())) <= _sum_bound(rv)
    assert got["area"] == sa / 2.0 and got["volume"] == sv / 6.0
    without = ops.mesh_report(V, F, self_intersections=False)
    assert without == {k: x for k, x in got.items() if not k.startswith("self_")}


def test_known_truths(cuda):
    r = ops.mesh_report(*_dev(cuda, *R.cube(4.0)))
    assert r["is_watertight"] and r["is_winding_consistent"] and r["euler"] == 2 and r["genus"] == 0
    assert r["area"] == 96.0 and abs(r["volume"]) == 64.0 and r["is_volume"] == (r["volume"] > 0)
    r = ops.mesh_report(*_dev(cuda, *R.torus()), self_intersections=False)
    assert r["euler"] == 0 and r["genus"] == 1
    assert ops.mesh_report(*_dev(cuda, *_lidless()))["border_edges"] == 4
    assert ops.mesh_report(*_dev(cuda, *_flipped()))["inconsistent_edges"] == 3
    assert ops.mesh_report(*_dev(cuda, *_degenerate()))["degenerate_faces"] == 2


# ------------------------------------------------------------------------------------------------------ self-intersections
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(MESHES))
def test_self_intersections_equal_the_brute_force(cuda, name, form, monkeypatch):
    ref = _ref(name)
    _set_form(monkeypatch, form)
    V, F = _dev(cuda, ref["v"], ref["f"])
    got = ops.mesh_self_intersections(V, F, pairs=True)
    print(name, form, got["count"], "pairs,", int(got["faces"].sum()), "faces of", len(ref["f"]))
    assert got["count"] == len(ref["pairs"]) and got["pairs"].dtype == torch.int64 and got["pairs"].shape == (got["count"], 2)
    assert np.array_equal(got["pairs"].cpu().numpy(), ref["pairs"])
    assert got["faces"].dtype == torch.bool and np.array_equal(got["faces"].cpu().numpy(), ref["flags"])
    again = ops.mesh_self_intersections(V, F.long(), pairs=True)
    assert again["count"] == got["count"] and torch.equal(again["pairs"], got["pairs"]) and torch.equal(again["faces"], got["faces"])
    counted = ops.mesh_self_intersections(V, F)
    assert counted["pairs"] is None and counted["count"] == got["count"] and torch.equal(counted["faces"], got["faces"])


def test_the_constructions_do_what_they_are_for():
    """The hedgehog fills one cell and nearly every pair of it crosses; the giant triangle meets many tiny ones; every corner of the
    clamp mesh has its pair."""
    h = _ref("hedgehog")
    assert len(h["pairs"]) > 0.8 * 200 * 199 / 2
    g = _ref("giant")
    assert ((g["pairs"] == 1000).any(1)).sum() >= 10 and (g["pairs"][:, 0] == 1000).any() and (g["pairs"][:, 1] == 1000).any()
    c = _ref("corners")
    own = c["pairs"][(c["pairs"][:, 0] >= 300) & (c["pairs"][:, 1] == c["pairs"][:, 0] + 1)]
    assert len(own) == 8
    lo, hi = c["v"][c["f"].reshape(-1)].min(0), c["v"][c["f"].reshape(-1)].max(0)
    assert (lo == 0).all() and (hi == 1).all()


def test_no_faces_launches_nothing(cuda):
    V = torch.zeros((3, 3), device=cuda)
    F = torch.zeros((0, 3), dtype=torch.int64, device=cuda)
    got = ops.mesh_self_intersections(V, F, pairs=True)
    assert got["count"] == 0 and got["faces"].shape == (0,) and got["pairs"].shape == (0, 2)
    r = ops.mesh_report(V, F)
    want = R.report(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int64))
    assert r == dict(want, self_intersections=0, self_intersecting_faces=0)


def test_refusals(cuda):
    ref = _ref("cubes_integer")
    V, F = _dev(cuda, ref["v"], ref["f"])
    with pytest.raises(ops.SculptError, match="max_pairs"):
        ops.mesh_self_intersections(V, F, pairs=True, max_pairs=17)
    assert ops.mesh_self_intersections(V, F, pairs=True, max_pairs=18)["count"] == 18
    assert ops.mesh_self_intersections(V, F, max_pairs=0)["count"] == 18          # without the list there is nothing to bound
    for fn in (ops.mesh_report, ops.mesh_self_intersections):
        with pytest.raises(ops.SculptError):
            fn(V.cpu(), F.cpu())
        bad = F.clone()
        bad[3, 1] = len(V)
        with pytest.raises(ops.SculptError, match="out of range"):
            fn(V, bad)
        nan = V.clone()
        nan[2, 0] = float("nan")
        with pytest.raises(ops.SculptError, match="non-finite"):
            fn(nan, F)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_mesh_methods_and_properties(cuda):
    from sculptmate_amd.tsr import mesh as M

    ref = _ref("cubes_generic")
    m = M.Mesh(*_dev(cuda, ref["v"], ref["f"]))
    r = m.report()
    assert r == ops.mesh_report(m.vertices, m.faces) and r["self_intersections"] == 12
    assert m.report(self_intersections=False) == ops.mesh_report(m.vertices, m.faces, self_intersections=False)
    assert (m.is_watertight, m.is_winding_consistent, m.euler_number, m.area, m.volume) == \
        (r["is_watertight"], r["is_winding_consistent"], r["euler"], r["area"], r["volume"])
    assert m.euler_number == 4 and m.area == 192.0
    s = m.self_intersections(pairs=True)
    assert s["count"] == 12 and np.array_equal(s["pairs"].cpu().numpy(), ref["pairs"])
    assert len(M.FIELDS) == 12 and "report" not in vars(m)


def test_extract_meshes_report(cuda):
    from _tsrmodel import small_model

    s = small_model(cuda, 32)
    m, plain = s["m"], s["plain"]
    assert m.last_reports is None
    same = m.extract_meshes(s["codes"], report=None, **s["kw"])[0]
    assert m.last_reports is None
    full = m.extract_meshes(s["codes"], report="full", **s["kw"])[0]
    for got in (same, full):
        assert torch.equal(got.vertices.view(torch.int32), plain.vertices.view(torch.int32)) and torch.equal(got.faces, plain.faces)
    assert len(m.last_reports) == 1 and m.last_reports[0] == ops.mesh_report(full.vertices, full.faces)
    v, f = full.vertices.cpu().numpy(), full.faces.cpu().numpy()
    want = R.report(v, f)
    print("the small model's mesh:", m.last_reports[0])
    assert {k: m.last_reports[0][k] for k in INTEGERS} == {k: want[k] for k in INTEGERS}
    m.extract_meshes(s["codes"], report=True, keep_components="largest", **s["kw"])
    assert "self_intersections" not in m.last_reports[0] and m.last_reports[0]["components"] == 1
    with pytest.raises(ValueError, match="report"):
        m.extract_meshes(None, report="all", **s["kw"])


def test_generator_report_reaches_the_model(cuda, tmp_path):
    import types

    from test_host_logic import _write_checkpoint

    from sculptmate_amd import synth
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr.spec import SMALL_CFG

    _write_checkpoint(str(tmp_path), SMALL_CFG, seed=61)
    g = TripoGenerator(cuda)
    assert g.report is None
    g.checkpoint_dir = str(tmp_path)
    g.mc_resolution = 32
    assert g.initiate_model() == 0
    g.model.mesh_sink = lambda *a: None
    orig = g.model.extract_mesh

    def reachable(self, codes, **kw):   # random weights never reach the default threshold: take the grid's median
        return orig(codes, **dict(kw, threshold=float(ops.density_grid(codes[0].contiguous(), self.decoder, kw["resolution"]).median())))

    g.model.extract_mesh = types.MethodType(reachable, g.model)
    img = (synth.composite_rgb(synth.image_rgba(seed=62, size=SMALL_CFG["cond_image_size"])) * 255).astype(np.uint8)
    assert g.generate_mesh(img, "plain") == 0 and g.model.last_reports is None
    g.report = "full"
    assert g.generate_mesh(img, "reported") == 0
    mesh = g.last_meshes[0]
    assert g.model.last_reports == [ops.mesh_report(mesh.vertices, mesh.faces)]
