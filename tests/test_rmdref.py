"""The fp64 restatement of the host remesher's rules (tests/_rmdref.py) on hand-built meshes whose answer is known by
construction, so that the reference of the device kernel tests can be checked without a GPU."""
import numpy as np

import _rmdref as R
from test_remesh import icosahedron, open_sheet


def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    return v, f


def test_topology_of_a_tetrahedron():
    v, f = tetrahedron()
    T = R.topo(f, 4)
    assert T["ne"] == 6 and T["es"][-1] == 12 and (np.diff(T["es"]) == 2).all()
    assert (T["bnd"] == 0).all() and list(T["vfs"]) == [0, 3, 6, 9, 12]
    assert R.euler(4, f) == 2 and R.boundary_loops(f) == 0


def test_every_tetrahedron_edge_fails_the_link_condition():
    v, f = tetrahedron()
    for mode in (0, 1):
        _, _, cand, _, _, amb = R.collapse_proposals(v, f, mode, low=10.0, high=10.0)
        assert cand == [R.NO_CLAIM] * 6 and not any(amb)


def test_every_icosahedron_edge_passes_the_link_condition_and_one_round_is_independent():
    v, f = icosahedron()
    v = v.astype(np.float32)
    T, M, cand, fp, nef, amb = R.collapse_proposals(v, f, 0)
    assert T["ne"] == 30 and R.NO_CLAIM not in cand and not any(amb)
    assert all(len(s) == 8 for s in fp)  # both ends, their other 4 + 4 neighbours, the two apexes counted once
    win = R.winners(R.claims(12, cand, fp), cand, fp, nef)
    assert sum(1 for w in win if w) >= 1 and all(w in (0, 2) for w in win)


def test_a_lone_triangle_never_collapses():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    assert R.collapse_proposals(v, f, 0)[2] == [R.NO_CLAIM] * 3


def grid3():
    """3 x 3 vertices in the plane z = 0, cells split along (i, j) -> (i + 1, j + 1) (open_sheet's pattern)."""
    v, f = open_sheet(3)
    v = v.astype(np.float32)
    v[:, 2] = 0
    return v, f


def test_a_flat_regular_grid_has_no_flip():
    v, f = grid3()
    _, _, cand, _, amb = R.flip_proposals(v, f)
    assert cand == [R.NO_CLAIM] * len(cand) and not any(amb)


def test_the_flip_that_restores_a_flat_grid():
    """Cell (0, 0) split along the other diagonal (1, 3): corner 0 has one face (valence 2, target 4), the centre five (valence
    5, target 6), 1 and 3 valence 5 (target 4).  Flipping (1, 3) into (0, 4) gains 7 - 1 = 6; flipping (1, 5) into (2, 4) gains
    6 - 2 = 4 (2: valence 2 -> 3, the centre 5 -> 6, 1: 5 -> 4, 5: 4 -> 3), and (3, 7) likewise.  The three footprints overlap
    at 1 and 3: (1, 3) alone wins, and applying it restores the grid."""
    v, f = grid3()
    f = f.copy()
    f[0], f[1] = [0, 3, 1], [3, 4, 1]
    T, M, cand, fp, amb = R.flip_proposals(v, f)
    valid = {R.edge_ends(T, e): (cand[e] >> 32, fp[e]) for e in range(T["ne"]) if cand[e] != R.NO_CLAIM}
    assert not any(amb)
    assert valid == {(1, 3): (1024 - 6, {0, 1, 3, 4}), (1, 5): (1024 - 4, {1, 2, 4, 5}), (3, 7): (1024 - 4, {3, 4, 6, 7})}
    win = R.winners(R.claims(9, cand, fp), cand, fp, [1] * T["ne"])
    assert [R.edge_ends(T, e) for e in range(T["ne"]) if win[e]] == [(1, 3)]
    assert M.flip(1, 3)
    assert sorted(map(tuple, np.sort(M.F, 1))) == sorted(map(tuple, np.sort(grid3()[1], 1)))


def test_relaxation_centroid_of_a_fan_with_a_reversed_face():
    """A flat hexagonal fan around vertex 0, off centre: the relaxed position is the centroid of the six ring vertices, with or
    without one face reversed (the host's neighbours are distinct vertices, not next corners)."""
    ring = [[np.cos(t), np.sin(t), 0.0] for t in np.arange(6) * np.pi / 3]
    v = np.array([[0.1, -0.05, 0.0]] + ring, np.float32)
    f = np.array([[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)], np.int32)
    want = v[1:].astype(np.float64).mean(0)
    # a closed fan needs a cap for the centre to be interior: the ring's other side
    cap = np.array([[1 + (k + 1) % 6, 1 + k, 7] for k in range(6)], np.int32)
    v = np.concatenate([v, [[0, 0, -1]]]).astype(np.float32)
    for rev in (False, True):
        ff = np.concatenate([f, cap]).astype(np.int32)
        if rev:
            ff[2] = ff[2][::-1]
        Q = R.relax(v, ff)[0]
        assert np.allclose(Q[0], want, atol=1e-7), (rev, Q[0], want)


def test_split_templates_of_a_right_triangle():
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    T, mark, cnt, rows, Fo, amb_f, amb_e = R.split_reference(v, f, 2.0)  # edges (0, 1) and (1, 2) are longer than 2
    assert list(cnt) == [3] and not amb_f.any()
    m01, m12 = 3 + mark[:T["fe"][0] + 1].sum() - 1, 3 + mark[:T["fe"][1] + 1].sum() - 1
    assert np.array_equal(rows[m01 - 3], [2, 0, 0]) and np.array_equal(rows[m12 - 3], [2, 0.5, 0])
    # diagonals of the quad 2, 0, m01, m12: |m01 - v2| = sqrt 5 > |m12 - v0| = sqrt 4.25 -> the second
    assert Fo.tolist() == [[m01, 1, m12], [2, 0, m12], [0, m01, m12]]
    _, _, cnt, _, Fo, _, _ = R.split_reference(v, f, 0.5)
    assert list(cnt) == [4] and len(Fo) == 4


def test_closest_point_branches():
    a, b, c = np.array([[0.0, 0, 0]]), np.array([[1.0, 0, 0]]), np.array([[0.0, 1, 0]])
    for p, want in (([-1, -1, 0], [0, 0, 0]), ([2, -0.5, 0], [1, 0, 0]), ([0.5, -1, 3], [0.5, 0, 0]), ([-1, 2, 0], [0, 1, 0]),
                    ([-1, 0.5, 0], [0, 0.5, 0]), ([1, 1, 0], [0.5, 0.5, 0]), ([0.2, 0.3, -2], [0.2, 0.3, 0])):
        assert np.allclose(R.closest_on_triangles(np.array(p, float), a, b, c)[0], want), p


def closed_fan(n):
    """A ring of n vertices with an apex above and one below: both apexes have n neighbours, every edge two faces."""
    ring = [[np.cos(t), np.sin(t), 0.0] for t in np.arange(n) * 2 * np.pi / n]
    v = np.array([[0, 0, 1]] + ring + [[0, 0, -1]], np.float32)
    f = [[0, 1 + k, 1 + (k + 1) % n] for k in range(n)] + [[n + 1, 1 + (k + 1) % n, 1 + k] for k in range(n)]
    return v, np.array(f, np.int32)


def test_high_valence_threshold():
    """64 neighbours is not a feature, 65 is (Mesh::scan_boundary_vertex); the ring vertices are interior either way."""
    for n in (63, 64, 65, 96):
        v, f = closed_fan(n)
        T = R.topo(f, n + 2)
        want = n > 64
        assert T["high_valence"][0] == want and T["high_valence"][n + 1] == want and T["edge_bnd"].sum() == 0
        assert T["bnd"][1:n + 1].sum() == 0
        M = R.Mesh(v, f)
        assert M.scan_boundary_vertex(0) == want and M.scan_boundary_vertex(n + 1) == want and not M.bnd[1:n + 1].any()


def test_a_feature_survives_the_collapse_that_removes_it():
    """Mesh::collapse ORs the removed end's flag into the kept end, and a flag stays when the valence drops."""
    v, f = closed_fan(65)
    M = R.Mesh(v, f)
    assert M.bnd[0] and not M.bnd[1]
    ok, u, w, p, _ = R.collapse_rule(M, 0, 1, 0)
    assert ok and (u, w) == (0, 1)
    M.collapse(u, w, p)
    assert M.bnd[1] and len(M.neighbours(1)) == 65
