"""Surface distance on the device (csrc/mesh_distance.hip) against the NumPy restatement (tests/_distref.py): closest points bit
for bit against the brute force in both kernel forms, samples bit for bit against the integer rule, the metrics against the
composed NumPy route, and one end-to-end run on the small model's mesh."""
import math

import numpy as np
import pytest
import torch

import _distref as D
import _rmdref as R
from sculptmate_amd import ops
from test_remesh import icosphere, open_sheet

pytestmark = pytest.mark.gpu

FORMS = ["default", "plain"]


# ---------------------------------------------------------------------------------------------------------------- meshes
def _sphere():
    v, f = icosphere(2)
    assert len(f) == 320
    return v.astype(np.float32), f.astype(np.int32)


def _planar_sheet():
    v, f = open_sheet(9)
    v[:, 2] = 0.0                                   # one grid layer
    return v.astype(np.float32), f.astype(np.int32)


def _strip(n=40):
    v = np.array([[i, w, 0.0] for i in range(n + 1) for w in (0.0, 0.01)], np.float32)
    f = np.array([t for i in range(n) for t in ([2 * i, 2 * i + 2, 2 * i + 3], [2 * i, 2 * i + 3, 2 * i + 1])], np.int32)
    return v, f


def _triangle():
    return np.array([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.1, 0.6]], np.float32), np.array([[0, 1, 2]], np.int32)


def _cube():
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32)
    f = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                  [1, 3, 5], [3, 7, 5]], np.int32)
    return v, f


def _degenerate_sphere():
    """A sphere with a face that names one vertex three times, a face of three equal positions, and two faces of three collinear
    corners (one an exact midpoint, one not)."""
    v, f = _sphere()
    nv = len(v)
    extra = np.array([[0.3, 0.3, 1.2]] * 3 + [[-1.5, 0.1, 0.2], [-1.0, 0.1, 0.2], [-0.5, 0.1, 0.2]]
                     + [[0.1, -1.5, 0.3], [0.7, -1.2, 0.1], [0.4, -1.35, 0.2]], np.float32)
    f = f.copy()
    f[7] = [f[7, 0]] * 3
    more = np.array([[nv, nv + 1, nv + 2], [nv + 3, nv + 4, nv + 5], [nv + 6, nv + 7, nv + 8]], np.int32)
    return np.concatenate([v, extra]), np.concatenate([f[:100], more, f[100:]])


MESHES = {"sphere": _sphere, "sheet": _planar_sheet, "strip": _strip, "triangle": _triangle, "cube": _cube,
          "degenerate": _degenerate_sphere}


def _queries(P, F, seed, n_in=800, n_out=500, n_cell=200):
    """About 2000 queries: inside the bounds; up to ten box sizes outside; exactly on vertices and (fp32) edge midpoints, where
    many faces are at d2 == 0 or tie; the centre of the bounds; points on the grid's cell borders; NaN and +-inf."""
    rng = np.random.default_rng(seed)
    used = P[np.unique(F)]
    lo, hi = used.min(0).astype(np.float64), used.max(0).astype(np.float64)
    size = float((hi - lo).max())
    parts = [rng.uniform(lo, hi, (n_in, 3)), rng.uniform(lo - 10 * size, hi + 10 * size, (n_out, 3)), used[:300]]
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])[:300]
    parts.append((np.float32(0.5) * (P[e[:, 0]] + P[e[:, 1]])))
    parts.append(0.5 * (lo + hi)[None])
    glo, cell, gn = R.grid_params(P, F)
    k = np.stack([rng.integers(0, gn[a] + 1, n_cell) for a in range(3)], 1)
    on_border = glo + k * cell                      # integer grid coordinates, up to the fp32 rounding of the point
    on_border[:, 1:] += rng.uniform(0, 1, (n_cell, 2)) * cell * (rng.uniform(size=(n_cell, 1)) < 0.5)
    parts.append(on_border)
    parts.append(np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.5, 0.5, -np.inf]]))
    return np.concatenate([np.asarray(p, np.float64) for p in parts]).astype(np.float32)


_cases = {}


def _case(name):
    """(P, F, queries, brute-force reference): computed once per mesh and shared, never modified."""
    if name not in _cases:
        P, F = MESHES[name]()
        q = _queries(P, F, seed=len(_cases) + 1)
        _cases[name] = (P, F, q, D.closest(q, P, F))
    return _cases[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _assert_same(got, want, what):
    for g, w, part in zip(got, want, ("d2", "face", "closest")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, g.shape)
        rows = (len(w), int(np.prod(w.shape[1:])))
        bad = np.nonzero((_bits(g) != _bits(w)).reshape(rows).any(1) & ~(np.isnan(w) & np.isnan(g)).reshape(rows).all(1))[0]
        assert len(bad) == 0, "%s %s: %d of %d differ, first %d: %r vs %r" % (what, part, len(bad), len(w), bad[0], g[bad[0]], w[bad[0]])


def _run(cuda, q, P, F, form, monkeypatch, face_dtype=torch.int32):
    if form == "plain":
        monkeypatch.setenv("SCULPT_DISTANCE_FORM", "plain")
    else:
        monkeypatch.delenv("SCULPT_DISTANCE_FORM", raising=False)
    return ops.mesh_closest_points(torch.from_numpy(q).to(cuda), torch.from_numpy(P).to(cuda),
                                   torch.from_numpy(F.astype(np.int64)).to(cuda).to(face_dtype))


# -------------------------------------------------------------------------------------------------------- closest points
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(MESHES))
def test_closest_points_equal_the_brute_force_bit_for_bit(cuda, monkeypatch, name, form):
    P, F, q, want = _case(name)
    got = _run(cuda, q, P, F, form, monkeypatch)
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.int64 and got[2].dtype == torch.float32
    _assert_same(got, want, "%s/%s" % (name, form))


def test_the_cases_hold_what_they_are_meant_to():
    """Ties at d2 == 0 that the lowest index must win, a NaN face, the edge answers of the non-finite queries."""
    P, F, q, (d2, face, cl) = _case("degenerate")
    assert (d2 == 0).sum() >= 100
    on_vertex = D.closest(P[F[0, :1]], P, F)
    shared = int((F == F[0, 0]).any(1).sum())
    assert shared >= 5 and on_vertex[1][0] == np.nonzero((F == F[0, 0]).any(1))[0][0] and on_vertex[0][0] == 0
    assert np.isnan(d2[-3:]).all() and (face[-3:] == -1).all() and np.array_equal(_bits(cl[-3:]), _bits(q[-3:]))
    assert np.isfinite(d2[:-3]).all() and (face[:-3] >= 0).all()


@pytest.mark.parametrize("form", FORMS)
def test_int64_faces(cuda, monkeypatch, form):
    P, F, q, want = _case("cube")
    _assert_same(_run(cuda, q, P, F, form, monkeypatch, face_dtype=torch.int64), want, "cube/int64/" + form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_query_counts_around_the_wave_and_block_sizes(cuda, monkeypatch, n, form):
    P, F, q, want = _case("sphere")
    got = _run(cuda, q[:n].copy(), P, F, form, monkeypatch)
    assert got[0].shape == (n,) and got[1].shape == (n,) and got[2].shape == (n, 3)
    _assert_same(got, [w[:n] for w in want], "n=%d/%s" % (n, form))


@pytest.mark.parametrize("form", FORMS)
def test_no_faces(cuda, monkeypatch, form):
    P, _, q, _ = _case("triangle")
    q = q[-40:]
    d2, face, cl = _run(cuda, q, P, np.zeros((0, 3), np.int32), form, monkeypatch)
    finite = np.isfinite(q).all(1)
    d2 = d2.cpu().numpy()
    assert (d2[finite] == np.inf).all() and np.isnan(d2[~finite]).all() and (face.cpu().numpy() == -1).all()
    assert np.array_equal(_bits(cl.cpu().numpy()), _bits(q))


def test_two_calls_and_two_forms_give_the_same_bits(cuda, monkeypatch):
    P, F, q, _ = _case("sheet")
    runs = [_run(cuda, q, P, F, form, monkeypatch) for form in ("default", "default", "plain")]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))


def test_bad_meshes_are_refused(cuda):
    P, F = (torch.from_numpy(x).to(cuda) for x in _triangle())
    q = torch.zeros((4, 3), device=cuda)
    with pytest.raises(ops.SculptError, match="out of range"):
        ops.mesh_closest_points(q, P, torch.tensor([[0, 1, 3]], dtype=torch.int32, device=cuda))
    with pytest.raises(ops.SculptError, match="out of range"):
        ops.mesh_sample_surface(P, torch.tensor([[0, -1, 2]], dtype=torch.int64, device=cuda), 4)
    bad = P.clone()
    bad[1, 2] = float("nan")
    with pytest.raises(ops.SculptError, match="non-finite"):
        ops.mesh_closest_points(q, bad, F)
    with pytest.raises(ops.SculptError, match="non-finite"):
        ops.mesh_distance(bad, F, P, F, samples=None)
    with pytest.raises(ops.SculptError):
        ops.mesh_closest_points(torch.zeros((4, 2), device=cuda), P, F)
    with pytest.raises(ops.SculptError, match="no face with area"):
        ops.mesh_sample_surface(P, torch.tensor([[1, 1, 1]], dtype=torch.int32, device=cuda), 4)
    with pytest.raises(ops.SculptError, match="no face with area"):
        ops.mesh_sample_surface(P, torch.zeros((0, 3), dtype=torch.int32, device=cuda), 4)
    for tau in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ops.mesh_distance(P, F, P, F, samples=None, threshold=tau)


# --------------------------------------------------------------------------------------------------------------- samples
@pytest.fixture(scope="module")
def soup():
    P, F = D.soup(50, degenerate=(17, 30))
    return P, F, D.weights(P, F)


def test_weights_equal_the_restatement(cuda, soup):
    P, F, w = soup
    got = ops.surface_weights(torch.from_numpy(P).to(cuda), torch.from_numpy(F).to(cuda)).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, w), np.abs(got - w).max()
    assert w[17] == 0 and w[30] == 0 and (w > 0).sum() == 48


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 + 5])
@pytest.mark.parametrize("n", [0, 1, 1000, 4097])
def test_samples_equal_the_restatement_bit_for_bit(cuda, soup, n, seed):
    P, F, w = soup
    pts, face, uv = ops.mesh_sample_surface(torch.from_numpy(P).to(cuda), torch.from_numpy(F).to(cuda), n, seed)
    assert pts.dtype == torch.float32 and face.dtype == torch.int64 and uv.dtype == torch.float32
    assert pts.shape == (n, 3) and face.shape == (n,) and uv.shape == (n, 2)
    rp, rf, ruv = D.sample(P, F, n, seed, w=w)
    assert np.array_equal(face.cpu().numpy(), rf)
    assert np.array_equal(_bits(uv.cpu().numpy()), _bits(ruv))
    assert np.array_equal(_bits(pts.cpu().numpy()), _bits(rp))
    if n:
        assert not np.isin(rf, (17, 30)).any()


def test_int32_faces_and_the_mesh_method_sample_alike(cuda, soup):
    from sculptmate_amd.tsr.system import Mesh

    P, F, _ = soup
    v, f = torch.from_numpy(P).to(cuda), torch.from_numpy(F).to(cuda)
    a = ops.mesh_sample_surface(v, f, 300, 9)
    b = Mesh(v, f.to(torch.int32)).sample_surface(300, seed=9)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# --------------------------------------------------------------------------------------------------------------- metrics
def _close(got, want, n):
    """A mean of n non-negative doubles summed in any order: within n 2^-52 relative, twice the first-order bound."""
    return abs(got - want) <= n * 2.0 ** -52 * abs(want)


def _check_metrics(got, want, n_ab, n_ba):
    for way, n in (("a_to_b", n_ab), ("b_to_a", n_ba)):
        assert got[way]["max"] == want[way]["max"], (way, got[way], want[way])
        assert _close(got[way]["mean"], want[way]["mean"], n) and _close(got[way]["rms"], want[way]["rms"], n), (way, got[way], want[way])
    assert got["hausdorff"] == want["hausdorff"]
    assert _close(got["chamfer"], want["chamfer"], max(n_ab, n_ba))
    for key in ("precision", "recall"):
        if key in want:
            assert got[key] == want[key], (key, got[key], want[key])
    if "fscore" in want:
        assert abs(got["fscore"] - want["fscore"]) <= 4 * 2.0 ** -52 * want["fscore"]
    assert set(got) == set(want) and all(type(v) is float for k, v in got.items() if k not in ("a_to_b", "b_to_a"))


@pytest.fixture(scope="module")
def pair():
    P, F = _sphere()
    rng = np.random.default_rng(5)
    Q = (P * np.float32(1.03) + rng.normal(0, 0.01, P.shape)).astype(np.float32)
    return P, F, Q, F[::-1].copy()


@pytest.mark.parametrize("threshold", [None, 0.03])
def test_mesh_distance_equals_the_composed_numpy_route_with_samples(cuda, pair, threshold):
    PA, FA, PB, FB = pair
    n, seed = 600, 2 ** 64 - 1                       # the second stream's seed wraps to 0
    qa, qb = D.sample(PA, FA, n, seed)[0], D.sample(PB, FB, n, 0)[0]
    want = D.metrics(D.closest(qa, PB, FB)[0], D.closest(qb, PA, FA)[0], threshold)
    t = [torch.from_numpy(x).to(cuda) for x in (PA, FA, PB, FB)]
    got = ops.mesh_distance(*t, samples=n, seed=seed, threshold=threshold)
    _check_metrics(got, want, n, n)
    if threshold:
        assert 0 < got["precision"] < 1 and 0 < got["recall"] < 1


def test_mesh_distance_from_the_vertices(cuda, pair):
    PA, FA, PB, FB = pair
    want = D.metrics(D.closest(PA, PB, FB)[0], D.closest(PB, PA, FA)[0], 0.03)
    t = [torch.from_numpy(x).to(cuda) for x in (PA, FA, PB, FB)]
    _check_metrics(ops.mesh_distance(*t, samples=None, threshold=0.03), want, len(PA), len(PB))


def test_a_mesh_against_itself(cuda):
    P, F = _sphere()
    P = (P + np.float32([3.0, -2.0, 0.5])).astype(np.float32)
    v, f = torch.from_numpy(P).to(cuda), torch.from_numpy(F).to(cuda)
    zero = ops.mesh_distance(v, f, v, f, samples=None, threshold=1e-9)
    assert zero["a_to_b"] == zero["b_to_a"] == {"mean": 0.0, "rms": 0.0, "max": 0.0}
    assert zero["chamfer"] == 0.0 and zero["hausdorff"] == 0.0 and zero["precision"] == zero["recall"] == zero["fscore"] == 1.0
    # A sample is (a + u (b - a)) + v (c - a) in fp32, six roundings per component, each at most 2^-25 of its result: the two
    # differences and the two products are at most an edge long (0.33 here, and u, v <= 1), the two sums at most max|coordinate|
    # (a convex combination).  Per component that is 2^-25 (4 edge + 2 max|coordinate|) <= 2^-24 (max|coordinate| + 1), over
    # three components sqrt(3) times it, below 4 2^-24 (max|coordinate| + 1).  The exact point lies on its face, so the
    # sample's distance to the surface is at most that offset.
    bound = 4 * 2.0 ** -24 * (float(np.abs(P).max()) + 1.0)
    near = ops.mesh_distance(v, f, v, f, samples=3000, seed=4)
    assert 0 < near["hausdorff"] <= bound, (near["hausdorff"], bound)
    assert near["chamfer"] < bound


@pytest.mark.parametrize("samples", [None, 4000])
def test_scaled_icosphere_is_a_hundredth_away(cuda, samples):
    v, f = icosphere(3)
    v = v.astype(np.float32)
    w = (v.astype(np.float64) * 1.01).astype(np.float32)
    e = w[f[:, 0]].astype(np.float64) - w[f[:, 1]].astype(np.float64)
    sagitta = float((e * e).sum(1).max()) / 8.0      # of the longest edge's chord on the (near-)unit sphere
    t = [torch.from_numpy(x).to(cuda) for x in (v, f, w, f)]
    got = ops.mesh_distance(*t, samples=samples, seed=11)
    for way in ("a_to_b", "b_to_a"):
        assert abs(got[way]["mean"] - 0.01) <= sagitta, (way, got[way], sagitta)
    assert abs(got["chamfer"] - 0.01) <= sagitta and got["hausdorff"] <= 0.0101 + sagitta


# ------------------------------------------------------------------------------------------------------------ end to end
def test_smoothing_moves_the_model_mesh_by_less_than_a_cell(cuda):
    from _tsrmodel import small_model

    s = small_model(cuda, 32, project_keys=True)
    plain = s["plain"]
    smooth = plain.smooth(3)
    got = plain.distance_to(smooth, samples=None)
    direct = ops.mesh_distance(plain.vertices, plain.faces, smooth.vertices, smooth.faces, samples=None)
    assert got == direct
    for way in ("a_to_b", "b_to_a"):
        assert all(math.isfinite(x) for x in got[way].values())
        assert 0 < got[way]["mean"] < s["cell"], (got[way], s["cell"])
    assert 0 < got["chamfer"] < s["cell"] and got["hausdorff"] >= got["a_to_b"]["max"]
    pts, face, uv = plain.sample_surface(1000, seed=3)
    assert pts.shape == (1000, 3) and int(face.max()) < plain.faces.shape[0]
    assert plain.distance_to(plain, samples=None)["hausdorff"] == 0.0
