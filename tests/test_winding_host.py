"""The inside / outside rule of csrc/mesh_winding.hip as tests/_windref.py restates it, on coordinates where the arithmetic is
exact, and the host-side rules of ops.voxel_rule / the CPU-tensor refusals (no GPU needed)."""
import itertools

import numpy as np
import pytest
import torch

import _windref as W
from sculptmate_amd import ops


def _lattice(lo, hi):
    r = np.arange(lo, hi + 1, dtype=np.float32)
    return np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)


def _octahedron(radius=8, levels=3):
    """|x| + |y| + |z| = radius, every face split 1 -> 4 at its edge midpoints `levels` times: 8 * 4^levels faces whose vertices
    are integer points of the flat faces (radius a multiple of 2^levels), wound counter-clockwise seen from outside."""
    r = float(radius)
    tris = []
    for sx, sy, sz in itertools.product((1, -1), repeat=3):
        t = [np.array([sx * r, 0, 0]), np.array([0, sy * r, 0]), np.array([0, 0, sz * r])]
        tris.append(t if sx * sy * sz > 0 else [t[0], t[2], t[1]])
    for _ in range(levels):
        nxt = []
        for a, b, c in tris:
            ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
            nxt += [[a, ab, ca], [ab, b, bc], [ca, bc, c], [ab, bc, ca]]
        tris = nxt
    pts = np.array(tris).reshape(-1, 3)
    assert np.array_equal(pts, np.round(pts))
    v, inv = np.unique(pts, axis=0, return_inverse=True)
    return v.astype(np.float32), inv.reshape(-1, 3).astype(np.int64)


def test_integer_cube_inside_outside_and_on_the_surface():
    v, f = W.integer_cube(4)
    q = _lattice(-2, 6)
    w = W.winding(q, v, f)
    strictly_in = ((q > 0) & (q < 4)).all(1)
    strictly_out = ((q < 0) | (q > 4)).any(1)
    assert strictly_in.sum() == 27 and strictly_out.sum() == 9 ** 3 - 5 ** 3
    assert (w[strictly_in] == 1).all()
    # outside: among them the points whose rays pass exactly through corners, edges and the faces' diagonals
    assert (w[strictly_out] == 0).all()
    through_corner = strictly_out & (np.isin(q[:, 0], (0, 4)) & np.isin(q[:, 1], (0, 4)))
    through_diagonal = strictly_out & (q[:, 0] == q[:, 1]) & (q[:, 0] > 0) & (q[:, 0] < 4)
    assert through_corner.sum() >= 16 and through_diagonal.sum() >= 12
    assert W.contains(q, v, f)[strictly_in].all() and not W.contains(q, v, f)[strictly_out].any()
    # a point on the surface is not ahead of it: on the far side of axis a nothing is left to cross, on the near side only the
    # far face is
    for a in range(3):
        p = q[strictly_in].copy()
        p[:, a] = 4
        assert (W.winding(p, v, f)[:, a] == 0).all()
        p[:, a] = 0
        assert (W.winding(p, v, f)[:, a] == 1).all()


def test_octahedron_rays_through_vertices_count_once():
    v, f = _octahedron()
    assert len(f) == 512
    q = _lattice(-9, 9)
    l1 = np.abs(q).sum(1)
    w = W.winding(q, v, f)
    assert (w[l1 < 8] == 1).all() and (w[l1 > 8] == 0).all()
    # many of those rays pass exactly through a vertex of the mesh
    vs = {tuple(x) for x in v}
    through = sum(1 for p in q[l1 < 8] if any((p[0] + t, p[1], p[2]) in vs for t in range(1, 18)))
    assert through >= 100


def test_reversed_and_doubled_surfaces():
    from test_gpu_mesh_ray import MESHES

    v, f = W.integer_cube(4)
    q = _lattice(1, 3)
    assert (W.winding(q, v, f[:, ::-1]) == -1).all()
    assert W.contains(q, v, f[:, ::-1]).all()
    dv, df = MESHES["doubled_cube"]()
    inner = np.array([[0.5, 0.5, 0.5], [0.25, 0.75, 0.5], [0.125, 0.125, 0.875]], np.float32)
    assert (W.winding(inner, dv, df) == 2).all()
    assert (W.winding(inner + 2, dv, df) == 0).all()


def test_open_cube_is_inside_by_majority():
    v, f = W.integer_cube(4)
    top = (v[f][:, :, 2] == 4).all(1)
    assert top.sum() == 2
    q = _lattice(1, 3)
    w = W.winding(q, v, f[~top])
    assert (w[:, 2] == 0).all() and (w[:, :2] == 1).all()     # the z ray leaves through the hole, the other two still count
    assert W.contains(q, v, f[~top]).all()
    assert not W.contains(_lattice(5, 6), v, f[~top]).any()


def test_non_finite_queries_and_no_faces():
    v, f = W.integer_cube(4)
    q = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, 1]], np.float32)
    w = W.winding(q, v, f)
    assert (w[:2] == W.INT_MIN).all() and (w[2] == 1).all()
    assert list(W.inside_of(w)) == [False, False, True]
    assert (W.winding(q[2:], v, f[:0]) == 0).all()


def test_voxel_rule():
    assert ops.voxel_rule(8) == (8, 2) and ops.voxel_rule(1024) == (1024, 2) and ops.voxel_rule(np.int64(24)) == (24, 2)
    assert ops.voxel_rule((64, 1)) == (64, 1) and ops.voxel_rule((64, 16)) == (64, 16)
    for bad in (7, 1025, 0, -8, True, 24.0, "24", None, (24,), (24, 0), (24, 17), (24, True), (True, 2), (24, 2.0), [24, 2], (24, 2, 1)):
        with pytest.raises(ValueError):
            ops.voxel_rule(bad)


def test_cpu_tensors_are_refused():
    v, f = (torch.from_numpy(x) for x in W.integer_cube(4))
    q = torch.zeros((4, 3))
    for call in (lambda: ops.mesh_winding(q, v, f), lambda: ops.mesh_contains(q, v, f), lambda: ops.mesh_signed_distance(q, v, f),
                 lambda: ops.mesh_sdf_grid(v, f, 16), lambda: ops.mesh_voxel_remesh(v, f, 16)):
        with pytest.raises(ops.SculptError):
            call()
    with pytest.raises(ValueError):      # the rule comes first
        ops.mesh_voxel_remesh(v, f, 4)


def test_the_restated_fill_never_disagrees_with_the_planes():
    """(vol > 0) == bit at every lattice point, zero-distance points included: a lattice that has the cube's own corners, edges
    and faces among its points (h = 1, lo = -2)."""
    v, f = W.integer_cube(4)
    lo, h, n, band = W.grid_rule(v, f, 4)
    assert h == 1.0 and lo == [-2.0] * 3 and n == [9, 9, 9] and band == 2.0
    vol, planes, listed, _, _ = W.sdf_grid(v, f, 4)
    pts = W.lattice_points(lo, h, n)
    inside = W.contains(pts, v, f).reshape(n)
    assert np.array_equal(W.unpack_planes(planes, n), inside)
    assert np.array_equal(vol > 0, inside)
    d2 = W.D.closest(pts[listed], v, f)[0]
    assert (d2 == 0).sum() >= 50                               # points on the surface are listed ...
    on_surface_in = inside.reshape(-1)[listed] & (d2 == 0)
    assert on_surface_in.any() and (vol.reshape(-1)[listed][on_surface_in] == W.TINY).all()   # ... and an inside one is not 0
    assert (np.abs(vol) <= np.float32(band)).all()
    unlisted = np.ones(vol.size, bool)
    unlisted[listed] = False
    assert (np.abs(vol.reshape(-1)[unlisted]) == np.float32(band)).all()
    # the planes' bits past n2 are zero and the list is ascending
    assert planes.shape == (81, 1) and (planes.view(np.uint32) >> 9 == 0).all() and (np.diff(listed) > 0).all()
