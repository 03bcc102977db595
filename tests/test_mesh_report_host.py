"""The NumPy restatement of the mesh report (tests/_reportref.py) on its own, against known truths: no GPU.  The device is held
to this restatement in tests/test_gpu_mesh_report.py; the rule itself stands at the top of sculptmate_amd/csrc/mesh_report.hip."""
import inspect
import os

import numpy as np
import pytest

import _reportref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _pairs(v, f):
    return len(R.self_intersections(v, f)[0])


# ------------------------------------------------------------------------------------------------------------------ census
def test_integer_cube():
    r = R.report(*R.cube(4.0))
    assert r["is_watertight"] and r["is_winding_consistent"] and r["euler"] == 2 and r["genus"] == 0 and r["components"] == 1
    assert r["edges"] == 18 and r["border_edges"] == 0 and r["nonmanifold_edges"] == 0 and r["inconsistent_edges"] == 0
    assert r["area"] == 96.0 and abs(r["volume"]) == 64.0 and r["degenerate_faces"] == 0 and r["self_intersections"] == 0
    assert r["is_volume"] == (r["volume"] > 0)


def test_torus():
    r = R.report(*R.torus(48, 24), self_intersections_too=False)
    assert r["faces"] == 2 * 48 * 24 and r["euler"] == 0 and r["genus"] == 1 and r["is_watertight"] and r["is_winding_consistent"]
    assert "self_intersections" not in r


def test_cube_without_a_lid():
    v, f = R.cube(4.0)
    r = R.report(v, f[2:])                       # faces 0 and 1 are one side
    assert r["border_edges"] == 4 and not r["is_watertight"] and r["genus"] is None and not r["is_volume"]
    assert r["euler"] == 1 and r["is_winding_consistent"]


def test_two_cubes_joined_along_an_edge():
    v, f = R.join(R.cube(4.0), R.cube(4.0, (4, 4, 0)))
    f = f.copy()
    f[f == 8] = 6                                # the second cube's (4, 4, 0) and (4, 4, 4) are the first's corners 6 and 7
    f[f == 9] = 7
    r = R.report(v, f, self_intersections_too=False)
    assert r["nonmanifold_edges"] == 1 and not r["is_watertight"] and not r["is_winding_consistent"] and r["genus"] is None
    assert r["referenced_vertices"] == 14 and r["vertices"] == 16 and r["components"] == 1


def test_one_face_flipped():
    v, f = R.cube(4.0)
    f = f.copy()
    f[5] = f[5][::-1]
    r = R.report(v, f)
    assert r["inconsistent_edges"] == 3 and r["is_watertight"] and not r["is_winding_consistent"] and r["genus"] is None


def test_degenerate_faces():
    v, f = R.cube(4.0)
    v = np.concatenate([v, np.float32([[1, 1, 1], [2, 2, 2], [3, 3, 3]])])
    f = np.concatenate([f, [[0, 0, 5], [8, 9, 10]]])          # a repeated index; three collinear corners
    r = R.report(v, f)
    assert r["degenerate_faces"] == 2 and r["area"] == 96.0
    assert r["self_intersections"] == 0                       # neither can straddle a plane or span one


def test_components_and_unreferenced_vertices():
    v, f = R.join(R.cube(1.0), R.cube(1.0, (3, 0, 0)))
    v = np.concatenate([v, np.float32([[9, 9, 9]])])
    r = R.report(v, f)
    assert r["components"] == 2 and r["vertices"] == 17 and r["referenced_vertices"] == 16 and r["euler"] == 4 and r["genus"] == 0


def test_no_faces():
    r = R.report(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int64))
    assert r["faces"] == 0 and r["edges"] == 0 and not r["is_watertight"] and r["is_winding_consistent"] and r["genus"] is None
    assert r["area"] == 0.0 and r["volume"] == 0.0 and r["self_intersections"] == 0


# ------------------------------------------------------------------------------------------------------- self-intersections
def test_two_integer_cubes_offset_by_one():
    """Edges pass through face diagonals and through edges: the closed triangle counts them (a strict rule would miss them)."""
    assert _pairs(*R.join(R.cube(4.0), R.cube(4.0, (1, 1, 1)))) == 18


def test_two_cubes_at_a_generic_offset():
    assert _pairs(*R.join(R.cube(4.0), R.cube(4.0, (0.5, 1.5, 2.25)))) == 12


def test_two_cubes_that_touch_across_a_face():
    assert _pairs(*R.join(R.cube(4.0), R.cube(4.0, (4, 0, 0)))) == 0


def test_a_triangle_pierced_through_its_interior():
    v = np.float32([[0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 1, -1], [1, 1, 1], [5, 5, 1]])
    pairs, flags = R.self_intersections(v, [[0, 1, 2], [3, 4, 5]])
    assert pairs.tolist() == [[0, 1]] and flags.tolist() == [True, True]


def test_a_shared_vertex_and_a_crossing_through_the_hypotenuse():
    """The two faces share vertex 0; the second's opposite edge passes through (2, 2, 0), ON the first's hypotenuse."""
    v = np.float32([[0, 0, 0], [4, 0, 0], [0, 4, 0], [2, 2, -2], [2, 2, 2]])
    assert R.self_intersections(v, [[0, 1, 2], [0, 3, 4]])[0].tolist() == [[0, 1]]


def test_coplanar_triangles_sharing_an_edge():
    v = np.float32([[0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 0]])
    assert _pairs(v, [[0, 1, 2], [1, 3, 2]]) == 0
    assert _pairs(v, [[0, 1, 2], [0, 1, 3]]) == 0             # overlapping, coplanar: not claimed, not reported


def test_faces_sharing_an_edge_never_count():
    v, f = R.icosphere(2)
    assert _pairs(v, f) == 0


@pytest.mark.parametrize("name,want", [("sphere", 0), ("torus", 0), ("noise_a", 0), ("gyroid", 0), ("ints", 38)])
def test_marching_cubes_goldens(name, want):
    """Clean marching-cubes meshes do not intersect themselves; `ints` has an integer volume, which puts vertices on lattice
    points, so faces touch."""
    z = np.load(os.path.join(GOLDEN, "mc_skimage.npz"))
    v, f = z[name + "_verts"], z[name + "_faces"]
    assert len(f) == {"sphere": 1772, "torus": 2112, "noise_a": 4395, "gyroid": 3508, "ints": 1072}[name]
    assert _pairs(v, f) == want


def test_pairs_are_lexicographic_and_flags_cover_them():
    v, f = R.join(R.icosphere(1), R.icosphere(1, center=(0.7, 0.2, 0.1)))
    pairs, flags = R.self_intersections(v, f)
    assert len(pairs) > 0 and (pairs[:, 0] < pairs[:, 1]).all()
    assert pairs.tolist() == sorted(pairs.tolist()) and set(np.nonzero(flags)[0]) == set(pairs.reshape(-1).tolist())


# ------------------------------------------------------------------------------------------------------------- the interface
def test_signatures_and_defaults():
    import torch

    from sculptmate_amd import ops
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr import mesh as M

    p = inspect.signature(ops.mesh_self_intersections).parameters
    assert [(k, v.default) for k, v in p.items()][2:] == [("pairs", False), ("max_pairs", 1 << 26)]
    p = inspect.signature(ops.mesh_report).parameters
    assert list(p) == ["vertices", "faces", "self_intersections"] and p["self_intersections"].default is True
    for name in ("extract_meshes", "extract_mesh"):
        assert inspect.signature(getattr(TSR, name)).parameters["report"].default is None
    assert TSR.last_reports is None and TripoGenerator(torch.device("cpu")).report is None and "`report`" in TripoGenerator.__doc__
    assert len(M.FIELDS) == 12                                # the report is a returned dict, never a field
    for name in ("is_watertight", "is_winding_consistent", "euler_number", "area", "volume"):
        assert isinstance(getattr(M.Mesh, name), property) and getattr(M.Mesh, name).fset is None
    assert list(inspect.signature(M.Mesh.report).parameters) == ["self", "self_intersections"]
    assert list(inspect.signature(M.Mesh.self_intersections).parameters) == ["self", "pairs"]


def test_a_bad_report_raises_before_a_launch():
    from sculptmate_amd.tsr import TSR

    m = TSR.__new__(TSR)   # no weights, no device: the rule must fire before either is needed
    for bad in (False, 1, "all", 2.0):
        with pytest.raises(ValueError, match="report"):
            TSR.extract_meshes(m, [None], report=bad)
    assert m.last_reports is None


def test_cpu_tensors_are_refused():
    import torch

    from sculptmate_amd import ops

    v, f = R.cube(4.0)
    for fn in (ops.mesh_report, ops.mesh_self_intersections):
        with pytest.raises(ops.SculptError):
            fn(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(ValueError):
        ops.mesh_self_intersections(torch.from_numpy(v), torch.from_numpy(f), pairs=True, max_pairs=-1)
