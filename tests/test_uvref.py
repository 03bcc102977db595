"""tests/_uvref.py (the restatement of the UV unwrapper's kernels) against the reference's own stage outputs in
tests/golden/sf3d_unwrap.npz, at the tolerances the golden GPU tests use: this ties the restatement to the reference before
the GPU tests compare the kernels with it bit for bit."""
import os

import numpy as np
import pytest

import _uvref as R
from conftest import GOLDEN
from oracle import sf3d_unwrap_ref as U


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "sf3d_unwrap.npz"))


@pytest.mark.parametrize("name", ["ell", "tor"])
def test_restatement_matches_reference_goldens(z, name):
    g = lambda k: z[name + "." + k]  # noqa: E731
    rp, rn, faces = g("rot_pos"), g("rot_nrm"), g("faces")
    rp2, rn2, lo, hi = R.rotate_mesh(rp, rn, np.eye(3, dtype=np.float32))
    assert R.same_bits(rp2, rp) and R.same_bits(rn2, rn)
    uv, chart = R.box_project(rp, rn, faces, lo, hi)
    assert np.array_equal(chart, g("face_index"))
    assert np.abs(uv - g("uv_box")).max() < 1e-6
    vt = R.vertex_tangents(rp, rn, faces, uv)
    assert np.abs(vt[:, :3] - g("tangents")).max() < 3e-5
    assert np.array_equal(vt[:, 3], np.bincount(faces.reshape(-1), minlength=len(rp)))
    sums, bound = R.chart_sums(rp, rn, faces, chart, vt)
    angles = R.chart_angles(sums)
    _, ref_angles = U.rotate_charts(rp, rn, faces, g("uv_box"), g("face_index"))
    assert np.abs(angles - ref_angles).max() < 2e-5
    co, si = R.rotation_cos_sin(angles)
    rot = R.rotate_charts(uv, chart, co, si)
    assert np.abs(rot - g("uv_rot")).max() < 3e-5
    placed = R.place(g("uv_rot"), g("assigned"), 0.02)
    assert placed.shape == g("placed").shape and np.abs(placed - g("placed")).max() < 1e-6
    # the oracle's placement with the same assignment is the same arithmetic
    assert np.abs(placed - U.place_in_atlas(g("uv_rot"), g("assigned"), 0.02)).max() < 1e-6


def test_restated_assignment_keeps_the_contract(z):
    """The assignment rule restated: index in {c, c + 6, 12}; a convex body stays in its front layer; on the torus the front
    layer and the overlap slices have no overlapping pairs, and the hidden wall moves."""
    for name in ("ell", "tor"):
        g = lambda k: z[name + "." + k]  # noqa: E731
        c = g("face_index")
        a = R.assign_atlas(g("rot_pos"), g("faces"), g("uv_rot"), c, 512)
        assert np.all((a == c) | (a == c + 6) | (a == 12))
        if name == "ell":
            assert np.array_equal(a, c)
            continue
        assert 0.2 < (a != c).mean() < 0.6
        keep = a < 12
        assert U.overlapping_pairs(g("uv_rot")[keep], a[keep]) == []


def test_restated_place_remaining_grid_in_face_order():
    """Every remaining face gets its own cell of the nw x nh grid, in face order; slices fill their patch."""
    rng = np.random.default_rng(0)
    nf = 1000
    uv = rng.random((nf, 3, 2)).astype(np.float32)
    a = rng.integers(0, 13, nf).astype(np.int32)
    out = R.place(uv, a, 0.02).reshape(nf, 3, 2)
    rem = np.nonzero(a == 12)[0]
    left = len(rem)
    nw = int(np.ceil(0.5 * np.sqrt(left / (0.5 / 3))))
    nh = int(np.ceil(left / nw))
    cell = np.floor(out[rem].mean(1) * [2 * nw, 3 * nh] - [nw, 2 * nh]).astype(int)   # lower-right sixth of the atlas
    assert np.array_equal(cell[:, 0] + nw * cell[:, 1], np.arange(left))
    assert out.min() >= 0 and out.max() <= 1
