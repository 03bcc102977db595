"""Catmull-Clark subdivision without a GPU: the NumPy restatement of the rule (tests/_catmullref.py) against closed forms and
invariants, and the public surface -- the scheme value, ops.mesh_catmull_clark, Mesh.subdivide, the quads' way through
extract_meshes, the .obj quad lines.  tests/test_gpu_catmull_clark.py then holds the device to the restatement bit for bit."""
import inspect

import numpy as np
import pytest
import torch

import _catmullref as cc
import _snref as sn


def _sphere_quads():
    g = np.mgrid[0:32, 0:32, 0:32].astype(np.float64)
    d = np.sqrt((g[0] - 15.3) ** 2 + (g[1] - 15.7) ** 2 + (g[2] - 16.1) ** 2)
    r = sn.surface_nets((10.2 - d).astype(np.float32))
    return r["verts"], r["quads"]


# ------------------------------------------------------------------------------------------------- the rule, closed forms
def test_cube_values():
    P, Q = cc.cube()
    V, Q1, T1, A = cc.subdivide(P, Q, 1)
    assert V.shape == (26, 3) and Q1.shape == (24, 4) and T1.shape == (48, 3) and A is None and V.dtype == np.float32
    assert np.array_equal(V[:8], (P.astype(np.float64) * (5.0 / 9.0)).astype(np.float32))        # old vertices -> +-5/9
    centres = np.array([[0, 0, -1], [0, 0, 1], [0, -1, 0], [0, 1, 0], [-1, 0, 0], [1, 0, 0]], np.float32)
    assert np.array_equal(V[8:14], centres)                                                       # face points: the face centres
    E = V[14:]
    assert len(E) == 12 and np.array_equal(np.sort(np.abs(E), axis=1), np.tile(np.float32([0, 0.75, 0.75]), (12, 1)))
    assert len(np.unique(E, axis=0)) == 12


@pytest.mark.parametrize("mesh", [cc.cube, cc.tetrahedron, cc.single_quad, cc.quad_grid, cc.two_cubes_sharing_an_edge,
                                  cc.two_cubes_sharing_a_vertex, cc.closed_fan, cc.strip_with_valence_two, cc.quad_torus],
                         ids=lambda f: f.__name__)
def test_counts_numbering_and_orientation(mesh):
    P, F = mesh()
    T = cc.Topology(F, len(P))
    k = F.shape[1]
    V, Q, Tr, _ = cc.subdivide(P, F, 1)
    assert len(V) == len(P) + len(F) + T.ne and len(Q) == k * len(F) and len(Tr) == 2 * len(Q)
    assert Q.dtype == np.int32 and Tr.dtype == np.int32
    # row k f + c = (F[f, c], an edge point, the face point nv + f, an edge point)
    assert np.array_equal(Q[:, 0], F.reshape(-1)) and np.array_equal(Q[:, 2], len(P) + np.repeat(np.arange(len(F)), k))
    assert (Q[:, [1, 3]] >= len(P) + len(F)).all() and Q.max() == len(V) - 1
    # edge points are numbered by first appearance over the half-edges
    seen = []
    for e in Q[:, 1]:
        if e not in seen:
            seen.append(int(e))
    assert seen == list(range(len(P) + len(F), len(V)))
    # orientation: the child of corner c runs F[f, c] -> point of edge (F[f, c], F[f, c + 1]); that edge's other half is the
    # next corner's child running edge point -> ... -> so every parent half-edge a -> b is covered by a -> e and e -> b
    D = cc.directed_edges(Q)
    nxt = np.roll(F, -1, axis=1).reshape(-1)
    for a, b, e in zip(F.reshape(-1), nxt, Q[:, 1]):
        assert (int(a), int(e)) in D and (int(e), int(b)) in D
    # the triangles are the quads' two halves
    assert np.array_equal(np.array([np.unique(pair) for pair in Tr.reshape(-1, 6)]), np.sort(Q, axis=1))


def test_euler_characteristic_is_kept():
    for (P, F), levels, chi in ((cc.cube(), 3, 2), (cc.tetrahedron(), 1, 2), (cc.quad_torus(), 2, 0), (_sphere_quads(), 1, 2)):
        assert cc.euler(F) == chi
        for n in range(1, levels + 1):
            V, Q, Tr, _ = cc.subdivide(P, F, n)
            assert cc.euler(Q) == chi and cc.euler(Tr) == chi and len(np.unique(Q)) == len(V)
    P, F = cc.tetrahedron()
    V, Q, _, _ = cc.subdivide(P, F, 1)
    assert len(V) == 14 and len(Q) == 12


def test_convex_hull_property_over_three_levels():
    """Every mask is a convex combination: the largest norm, and the extent along any direction, never grow."""
    rng = np.random.default_rng(3)
    dirs = rng.standard_normal((16, 3))
    for P, F in (cc.cube(), cc.tetrahedron(), cc.closed_fan(), cc.two_cubes_sharing_an_edge(), cc.strip_with_valence_two()):
        norm, ext = np.linalg.norm(P.astype(np.float64), axis=1).max(), (P.astype(np.float64) @ dirs.T).max(0)
        for _ in range(3):
            P, F, _, _ = cc.level(P, F)
            n2, e2 = np.linalg.norm(P.astype(np.float64), axis=1).max(), (P.astype(np.float64) @ dirs.T).max(0)
            assert n2 <= norm * (1 + 1e-6) and (e2 <= ext + 1e-6).all()
            norm, ext = n2, e2


def test_planar_grid_keeps_interior_and_border_bits_and_moves_the_corners():
    P, F = cc.quad_grid(4)
    V, Q, _, _ = cc.subdivide(P, F, 1)
    corners = np.array([0, 4, 20, 24])
    rest = np.setdiff1d(np.arange(25), corners)
    assert np.array_equal(V[rest].view(np.uint32), P[rest].view(np.uint32))
    assert (V[corners] != P[corners]).any(axis=1).all()           # two border edges: a crease, as in the Loop rule here
    assert np.array_equal(V[:, 2], np.full(len(V), np.float32(0.25)))
    # every new point lies where bilinear refinement puts it
    assert np.array_equal(V[25], np.float32([1 / 16, 1 / 16, 0.25]))


def test_opposite_winding_gives_the_same_positions():
    Pa, Fa = cc.wound_pair(False)
    Pb, Fb = cc.wound_pair(True)
    Va, Qa, _, _ = cc.subdivide(Pa, Fa, 1)
    Vb, Qb, _, _ = cc.subdivide(Pb, Fb, 1)
    # old vertices and face points keep their rows; the second quad's edges appear in another order, so its edge points are
    # compared as a set.  Every neighbour enters SN twice, so the shared vertices do not feel the winding: the same bits.
    assert np.array_equal(Va[:8].view(np.uint32), Vb[:8].view(np.uint32))
    rows = lambda V: sorted(map(tuple, V[8:].view(np.uint32).tolist()))   # noqa: E731
    assert rows(Va) == rows(Vb) and len(Va) == 6 + 2 + 7 and not np.array_equal(Qa, Qb)


def test_valence_two_and_high_valence_follow_the_rule():
    P, F = cc.strip_with_valence_two()
    V, _, _, _ = cc.subdivide(P, F, 1)
    X = P.astype(np.float64)
    fp = [(((X[a] + X[b]) + X[c]) + X[d]) / 4.0 for a, b, c, d in F]
    sn_ = ((X[2] + X[0]) + X[0]) + X[2]
    want = ((2.0 - 2.0) * X[1] + (0.5 * sn_ + (fp[0] + fp[1])) / 2.0) / 2.0
    assert np.array_equal(V[1], want.astype(np.float32))
    P, F = cc.closed_fan(70)
    V, Q, _, _ = cc.subdivide(P, F, 1)
    assert np.isfinite(V).all() and abs(float(V[0, 2]) - 1.0) < 0.1 and V[0, 2] < 1.0


def test_attributes_go_through_the_same_masks():
    P, F = cc.cube()
    V, _, _, A = cc.subdivide(P, F, 2, A=P)
    assert np.array_equal(A.view(np.uint32), V.view(np.uint32))
    rng = np.random.default_rng(1)
    for C in (1, 8):
        A0 = rng.random((8, C)).astype(np.float32)
        A = cc.subdivide(P, F, 2, A=A0)[3]
        assert A.shape == (98, C) and A.min() >= A0.min() and A.max() <= A0.max()


def test_no_faces_gives_copies():
    P = np.zeros((3, 3), np.float32)
    V, Q, T, A = cc.subdivide(P, np.zeros((0, 4), np.int32), 2, A=P[:, :1])
    assert np.array_equal(V, P) and Q.shape == (0, 4) and T.shape == (0, 3) and A.shape == (3, 1)


# ------------------------------------------------------------------------------------------------------- the interface
GOOD_RULES = [((1, "catmull_clark"), (1, "catmull_clark")), ((6, "catmull_clark"), (6, "catmull_clark")),
              ((np.int64(2), "catmull_clark"), (2, "catmull_clark")), (3, (3, "loop")), ((2, "midpoint"), (2, "midpoint"))]
BAD_RULES = [(2, "catmull-clark"), (2, "Catmull_Clark"), (0, "catmull_clark"), (7, "catmull_clark"), (True, "catmull_clark"),
             (1.0, "catmull_clark"), "catmull_clark", ("catmull_clark", 1), (1, "catmull_clark", 1), [1, "catmull_clark"], (1, "cc")]


@pytest.mark.parametrize("rule,want", GOOD_RULES, ids=repr)
def test_good_rules(rule, want):
    from sculptmate_amd import ops

    assert ops.subdivide_rule(rule) == want and ops.subdivide_rule(ops.subdivide_rule(rule)) == want
    assert "catmull_clark" in ops.SUBDIVIDE_SCHEMES


@pytest.mark.parametrize("rule", BAD_RULES, ids=repr)
def test_bad_rule_is_a_value_error_before_any_device_work(rule):
    from sculptmate_amd import ops
    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr.system import Mesh

    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)   # CPU tensors: the rule is checked first
    with pytest.raises(ValueError, match="subdivide"):
        ops.subdivide_rule(rule)
    with pytest.raises(ValueError, match="subdivide"):
        ops.mesh_subdivide(v, f, rule)
    with pytest.raises(ValueError, match="subdivide"):
        Mesh(v, f).subdivide(rule)
    with pytest.raises(ValueError, match="subdivide"):
        TSR.extract_meshes(TSR.__new__(TSR), [None], subdivide=rule)


def test_cpu_tensors_and_bad_levels_are_refused():
    from sculptmate_amd import ops
    from sculptmate_amd.tsr.system import Mesh

    v, f = torch.zeros((4, 3)), torch.tensor([[0, 1, 2, 3]], dtype=torch.int32)
    with pytest.raises(ops.SculptError):
        ops.mesh_catmull_clark(v, f, 1)                    # no CPU fallback
    with pytest.raises(ops.SculptError):
        ops.mesh_catmull_clark(v.numpy(), f.numpy(), 1)
    with pytest.raises(ops.SculptError):
        ops.mesh_subdivide(v, f[:, :3], (1, "catmull_clark"))
    with pytest.raises(ops.SculptError):
        Mesh(v, f[:, :3]).subdivide((1, "catmull_clark"))
    for levels in (0, 7, True, 1.0, None, "1"):
        with pytest.raises(ops.SculptError, match="levels"):
            ops.mesh_catmull_clark(v, f, levels)


def test_signatures_and_defaults():
    from sculptmate_amd import _lib, ops
    from sculptmate_amd.sf3d import remesh_device as rd
    from sculptmate_amd.tsr.mesh import FACE_FIELDS, FIELDS
    from sculptmate_amd.tsr.system import Mesh

    p = inspect.signature(ops.mesh_catmull_clark).parameters
    assert list(p) == ["vertices", "faces", "levels", "attributes"] and p["attributes"].default is None
    p = inspect.signature(rd.catmull_clark_device).parameters
    assert list(p) == ["v", "f", "levels", "attributes"] and p["attributes"].default is None
    assert list(inspect.signature(ops.mesh_subdivide).parameters) == ["vertices", "faces", "subdivide", "attributes"]
    assert list(inspect.signature(Mesh.subdivide).parameters) == ["self", "subdivide"]
    assert FACE_FIELDS == ("quads",) and len(FIELDS) == 12          # the scheme adds no field
    names = ["sculpt_catmull_validate", "sculpt_catmull_halfedge_keys", "sculpt_catmull_first_halfedge", "sculpt_catmull_classify",
             "sculpt_catmull_refine"]
    assert [n for n in sorted(_lib.SIGNATURES) if n.startswith("sculpt_catmull_")] == sorted(names)
    assert all(hasattr(_lib.lib, n) for n in names)
    assert [name for name, _ in _lib.CatmullTopo._fields_] == ["F", "skeys", "she", "es", "fe", "vfs", "vfc", "nf", "nv", "ne", "k"]


# ---------------------------------------------------------------------------------------------- Mesh and extract_meshes
def test_mesh_subdivide_sets_quads_for_catmull_clark_and_drops_them_for_loop(monkeypatch):
    from sculptmate_amd import ops
    from sculptmate_amd.tsr.system import Mesh

    calls = []

    def fake_cc(v, f, levels, attributes=None):
        calls.append(("cc", f.shape[1], levels))
        return cc.subdivide(v, f, levels, attributes)

    def fake_sub(v, f, rule, attributes=None):
        calls.append(("sub", rule))
        return v, f, attributes

    monkeypatch.setattr(ops, "mesh_catmull_clark", fake_cc)
    monkeypatch.setattr(ops, "mesh_subdivide", fake_sub)
    P, Q = cc.cube()
    T = cc.split(P, Q)
    col = np.random.default_rng(2).random((8, 3)).astype(np.float32)
    m = Mesh(P, T, col, vertex_normals=col, vertex_occlusion=col[:, 0])
    m.quads = Q
    got = m.subdivide((2, "catmull_clark"))
    V, Q2, T2, A = cc.subdivide(P, Q, 2, col)
    assert calls == [("cc", 4, 2)]                                             # it starts from the quads
    assert np.array_equal(got.vertices, V) and np.array_equal(got.quads, Q2) and np.array_equal(got.faces, T2)
    assert np.array_equal(got.vertex_colors, A) and got.vertex_normals is None and got.vertex_occlusion is None
    tri = Mesh(P, T)
    got = tri.subdivide((1, "catmull_clark"))
    assert calls[-1] == ("cc", 3, 1) and len(got.quads) == 3 * len(T) and np.array_equal(got.faces, cc.subdivide(P, T, 1)[2])
    for rule in (1, (1, "loop"), (2, "midpoint")):
        assert m.subdivide(rule).quads is None and calls[-1] == ("sub", rule)  # the triangle schemes still drop the quads
    uvs = np.zeros((3 * len(T), 2), np.float32)
    with pytest.raises(ValueError, match="subdivide before baking"):
        Mesh(P, T, uvs=uvs).subdivide((1, "catmull_clark"))


def test_extract_meshes_refines_the_quads_while_they_are_valid(monkeypatch):
    """On recorders: with surface nets and neither keep_components nor simplify the scheme gets the extractor's quads, otherwise
    the triangles; the mesh carries the refined quads and their split, also behind project."""
    from sculptmate_amd import ops
    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr.spec import SMALL_CFG

    calls = []

    class Vol:
        def view(self, *shape):
            return self

    def fake_cc(v, f, levels, attributes=None):
        calls.append((f, levels))
        return v + "'", "Q'(%s)" % f, "T'(%s)" % f, None

    monkeypatch.setattr(ops, "surface_nets", lambda vol, level=0.0, **kw: ("V", "Q", "F"))
    monkeypatch.setattr(ops, "marching_cubes", lambda vol, level=0.0, **kw: ("V", "T"))
    monkeypatch.setattr(ops, "density_grid", lambda *a, **k: Vol())
    monkeypatch.setattr(ops, "mesh_catmull_clark", fake_cc)
    monkeypatch.setattr(ops, "mesh_smooth", lambda v, f, s: v + "s")
    monkeypatch.setattr(ops, "mesh_simplify", lambda v, f, s: (v + "d", f + "d", None))
    monkeypatch.setattr(ops, "mesh_keep_components", lambda v, f, s: (v + "k", f + "k", None, None))
    monkeypatch.setattr(ops, "mesh_subdivide", lambda v, f, s, attributes=None: (v + "l", f + "l", None))
    m = TSR(SMALL_CFG, decoder_filter=False)
    monkeypatch.setattr(m, "set_marching_cubes_resolution", lambda R: None)
    monkeypatch.setattr(m, "_projected", lambda v, f, planes, thr, rule, R: v + "p")
    code = torch.zeros(3, 4, 8, 8)
    rule = (2, "catmull_clark")
    kw = dict(resolution=32, threshold=2.0, subdivide=rule)
    got = m.extract_meshes([code], isosurface="surface_nets", **kw)[0]
    assert calls[-1] == ("Q", 2) and (got.vertices, got.faces, got.quads) == ("V'", "T'(Q)", "Q'(Q)")
    got = m.extract_meshes([code], isosurface="surface_nets", smooth=2, project=True, **kw)[0]
    assert calls[-1] == ("Q", 2) and (got.vertices, got.faces, got.quads) == ("Vs'p", "T'(Q)", "Q'(Q)")   # project keeps the quads
    got = m.extract_meshes([code], isosurface="surface_nets", simplify=0.5, **kw)[0]
    assert calls[-1] == ("Fd", 2) and (got.faces, got.quads) == ("T'(Fd)", "Q'(Fd)")
    got = m.extract_meshes([code], isosurface="surface_nets", keep_components="largest", **kw)[0]
    assert calls[-1] == ("Fk", 2) and got.quads == "Q'(Fk)"
    got = m.extract_meshes([code], simplify=0.1, **kw)[0]                                                # marching cubes
    assert calls[-1] == ("Td", 2) and (got.faces, got.quads) == ("T'(Td)", "Q'(Td)")
    n = len(calls)
    got = m.extract_meshes([code], isosurface="surface_nets", resolution=32, threshold=2.0, subdivide=(1, "loop"))[0]
    assert len(calls) == n and got.quads is None and got.faces == "Fl"                                    # Loop still drops them
    got = m.extract_meshes([code, code], isosurface="surface_nets", **kw)
    assert [g.quads for g in got] == ["Q'(Q)", "Q'(Q)"] and m._quads is None


def test_obj_round_trip_of_a_refined_mesh(tmp_path):
    from sculptmate_amd import meshio
    from sculptmate_amd.tsr.system import Mesh

    P, Q = cc.cube()
    V, Q1, T1, _ = cc.subdivide(P, Q, 1)
    m = Mesh(V, T1.astype(np.int64))
    m.quads = Q1.astype(np.int64)
    path = str(tmp_path / "cc.obj")
    m.export(path)
    lines = [l.split() for l in open(path) if l.startswith("f ")]
    assert len(lines) == 24 and all(len(l) == 5 for l in lines)
    back = meshio.read_obj(path)
    assert np.array_equal(back[1], m.quads) and np.array_equal(back[0], V)
    m.export(str(tmp_path / "cc.ply"))
    assert np.array_equal(meshio.read_ply(str(tmp_path / "cc.ply"))[1], m.faces)
