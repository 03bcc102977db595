"""Discrete curvature, the parts that need no device: the NumPy restatement (tests/_curvref.py) of csrc/mesh_curvature.hip
against what the operators must give -- Gauss-Bonnet on closed meshes, a flat grid, the unit sphere under refinement -- and the
host rules: ops.curvature_rule, CurvatureMap's 16-bit encoding, ops.principal_curvatures."""
import math

import numpy as np
import pytest
import torch

import _curvref as C


def _euler(V, F):
    lo, hi = C._edges(F)
    return len(V) - len(np.unique(lo * (len(V) + 1) + hi)) + len(F)


@pytest.mark.parametrize("name, chi", [("icosphere2", 2), ("torus", 0)])
def test_gauss_bonnet_on_closed_meshes(name, chi):
    V, F = C.MESHES[name]()
    assert _euler(V, F) == chi
    area, deficit, hint, valid, n = C.terms(V, F)
    assert valid.all() and (n > 0).all() and (area > 0).all()
    total, want, bound = float(deficit.sum()), 2.0 * math.pi * chi, 3 * len(F) * 2.0 ** -47
    print("%s: sum of deficits %.17g, 2 pi chi %.17g, difference %.3g, bound %.3g" % (name, total, want, abs(total - want), bound))
    assert abs(total - want) <= bound


@pytest.mark.parametrize("flip", [False, True])
def test_cube_corners_are_right_angle_ties(flip):
    """Every corner of the 12-face cube has the deficit pi / 2, whichever way the diagonals run, and every triangle -- a right
    angle, dot == 0 exactly -- takes the Voronoi branch."""
    V, F = C.cube(flip_diagonals=flip)
    c = C.corner_terms(V, F)
    assert c["voronoi"].all() and not c["obtuse_here"].any() and not c["obtuse_elsewhere"].any()
    area, deficit, hint, valid, n = C.terms(V, F)
    err = np.abs(deficit - math.pi / 2)
    print("cube (flip=%s): largest |deficit - pi/2| = %.3g" % (flip, err.max()))
    assert valid.all() and (err <= 3 * 2.0 ** -50).all()
    assert abs(float(deficit.sum()) - 4 * math.pi) <= 36 * 2.0 ** -47
    assert float(area.sum()) == 6.0 and (hint > 0).all()          # the mixed areas tile the surface; a cube is convex


def test_flat_grid():
    V, F = C.grid(5, 5)
    area, deficit, hint, valid, n = C.terms(V, F)
    interior = np.zeros((5, 5), bool)
    interior[1:-1, 1:-1] = True
    interior = interior.reshape(-1)
    assert np.array_equal(valid, interior)                         # border vertices are invalid, and zero
    assert not area[~interior].any() and not deficit[~interior].any() and not hint[~interior].any()
    mean, gauss, _ = C.curvature(V, F)
    assert (mean[interior] == 0).all() and np.isnan(mean[~interior]).all() and np.isnan(gauss[~interior]).all()
    assert (np.abs(deficit[interior]) <= n[interior] * 2.0 ** -50).all()      # |K A|
    # the rounds leave a flat grid flat, and the border out
    mean4, gauss4, valid4 = C.curvature(V, F, rings=4)
    assert np.array_equal(valid4, interior) and (mean4[interior] == 0).all()


def test_sphere_signs_and_convergence():
    errs = []
    for k in (2, 3, 4):
        R = 1.0
        V, F = C.icosphere(k, R)
        mean, gauss, valid = C.curvature(V, F)
        assert valid.all() and (mean > 0).all()
        errs.append((float(np.abs(mean.astype(np.float64) - 1 / R).max()), float(np.abs(gauss.astype(np.float64) - 1 / R ** 2).max())))
        print("icosphere(%d): max |H - 1/R| = %.3e, max |K - 1/R^2| = %.3e" % ((k,) + errs[-1]))
        if k == 2:
            inward, _, _ = C.curvature(V, F, outward=-1.0)
            turned, gauss_t, _ = C.curvature(V, F[:, ::-1])
            assert (inward < 0).all() and (turned < 0).all() and np.array_equal(np.abs(inward), mean)
            assert np.allclose(gauss_t, gauss, rtol=1e-6)          # the Gaussian curvature does not see the winding
    assert errs[0][0] > errs[1][0] > errs[2][0] and errs[0][1] > errs[1][1] > errs[2][1]


def test_scaled_sphere_and_rings():
    """H scales as 1 / R, K as 1 / R^2; summing over rings keeps the quotient of a constant-curvature surface."""
    V, F = C.icosphere(2, 4.0)
    mean, gauss, _ = C.curvature(V, F, rings=2)
    assert np.abs(mean - 0.25).max() < 2e-3 and np.abs(gauss - 0.0625).max() < 5e-3


def test_degenerate_and_nonmanifold_vertices():
    V, F = C.pinch()
    area, deficit, hint, valid, n = C.terms(V, F)
    assert valid.all() and n[0] == 6 and abs(deficit[0] - (2 * math.pi - 6 * math.pi / 2)) < 1e-12   # the full angle sum of both fans
    V, F = C.fin()
    assert np.array_equal(C.terms(V, F)[3], [False, False, True, True, False])   # the fin's edge, and the fin's open tip
    V, F = C.with_unreferenced()
    valid = C.terms(V, F)[3]
    assert not valid[5] and valid.sum() == 12
    V, F = C.with_zero_area_face()
    area, deficit, hint, valid, n = C.terms(V, F)
    assert valid.all() and list(n) == [3, 3, 3, 4, 2]              # the sliver adds nothing to any of its corners
    V, F = C.stretched_grid()
    c = C.corner_terms(V, F)
    assert c["obtuse_here"].any() and c["obtuse_elsewhere"].any()


def test_curvature_rule():
    from sculptmate_amd import ops

    assert ops.curvature_rule(True) == 0 and ops.curvature_rule(0) == 0 and ops.curvature_rule(8) == 8
    assert ops.curvature_rule(np.int64(3)) == 3
    for bad in (False, None, 9, -1, 1.0, 2.5, float("nan"), "2", (1,), np.bool_(True), np.float32(1)):
        with pytest.raises(ValueError):
            ops.curvature_rule(bad)
    for bad in (0.5, 0, True, float("nan"), "1", None):
        with pytest.raises(ValueError):
            ops.mesh_curvature(None, None, True, outward=bad)      # the rule comes before the tensors
    with pytest.raises(ValueError):
        ops.mesh_curvature(None, None, 9)
    with pytest.raises(ValueError):
        ops.bake_curvature(None, None, None, None, curvature=False)
    with pytest.raises(ValueError):
        ops.bake_curvature(None, None, None, None, cage=0.1)       # a cage without a source
    with pytest.raises(ops.SculptError):                           # and CPU tensors are refused
        ops.mesh_curvature(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64))


def test_curvature_map_encoding():
    from sculptmate_amd.tsr.curvature import CurvatureMap, encode16

    x = np.array([[0.0, 2.0, -2.0], [np.nan, 1.0, -5.0], [4.0, np.inf, -np.inf]], np.float32)
    assert np.array_equal(encode16(x, 2.0), [[32768, 65535, 0], [32768, 49151, 0], [65535, 65535, 0]])
    mask = np.ones((3, 3), bool)
    mask[2] = False
    m = CurvatureMap(torch.from_numpy(x), torch.from_numpy(-x), torch.from_numpy(mask), rule=0)
    assert m.resolution == 3 and m.default_scale() == 5.0 and m.default_scale("gauss") == 5.0     # finite, covered
    img = m.image()
    assert img.dtype == np.uint16 and img.shape == (3, 3) and img[0, 0] == 32768 and img[1, 0] == 32768 and img[1, 2] == 0
    assert np.array_equal(m.image(2.0, which="gauss"), encode16(-x, 2.0))
    assert CurvatureMap(torch.zeros(2, 2), torch.zeros(2, 2), torch.zeros(2, 2, dtype=torch.bool)).default_scale() == 1.0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            m.image(bad)
    with pytest.raises(ValueError):
        m.image(which="max")
    info = m.info()
    assert info["covered"] == 6 and info["mean_max"] == 2.0 and info["mean_min"] == -5.0 and info["mean_not_finite_share"] == pytest.approx(1 / 6)
    assert len(m.png_bytes()) > 8 and m.png_bytes()[:8] == b"\x89PNG\r\n\x1a\n"


def test_principal_curvatures_bit_for_bit():
    from sculptmate_amd import ops

    rng = np.random.default_rng(5)
    h = rng.standard_normal(4096).astype(np.float32)
    k = (rng.standard_normal(4096) * 2).astype(np.float32)
    h[:4], k[:4] = [0.0, 1.0, np.nan, 2.0], [0.0, 1.0, 1.0, np.nan]
    k1, k2 = ops.principal_curvatures(torch.from_numpy(h), torch.from_numpy(k))
    r1, r2 = C.principal(h, k)
    assert np.array_equal(k1.numpy().view(np.uint32), r1.view(np.uint32)) and np.array_equal(k2.numpy().view(np.uint32), r2.view(np.uint32))
    fin = ~np.isnan(r1)
    assert (r1[fin] >= r2[fin]).all() and k1[0] == 0 and k1[1] == 1 and k2[1] == 1 and np.isnan(r1[2:4]).all()
    with pytest.raises(ops.SculptError):
        ops.principal_curvatures(torch.zeros(3), torch.zeros(4))
