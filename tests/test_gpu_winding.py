"""Inside / outside on the device (csrc/mesh_winding.hip) against the NumPy restatement (tests/_windref.py): the axis winding
counts bit for bit against the brute force in both kernel forms, the lattice kernel against the point kernel, the sign planes,
the active-corner list and the filled volume against their restatements, the voxel remesh's topology, and one end-to-end run on
the small model's mesh."""
import numpy as np
import pytest
import torch

import _distref as D
import _windref as W
from sculptmate_amd import ops
from test_gpu_mesh_ray import MESHES as RAY_MESHES
from test_remesh import icosphere

pytestmark = pytest.mark.gpu

FORMS = ["default", "plain"]


# ---------------------------------------------------------------------------------------------------------------- meshes
def _edge_on():
    """The integer cube, and inside and across it: one triangle in a plane x = const, one in y = const, one in z = const (each
    edge-on to two axes), a face of three equal positions and a face of three collinear corners."""
    v, f = W.integer_cube(4)
    extra = np.array([[2, 1, 1], [2, 3, 1], [2, 1, 3],      # x = 2
                      [1, 2, 1], [1, 2, 3], [5, 2, 1],      # y = 2, sticks out of the cube
                      [1, 1, 2], [3, 1, 2], [1, 3, 2],      # z = 2
                      [1, 1, 1], [1, 1, 1], [1, 1, 1],      # a point
                      [0, 0, 0], [2, 2, 2], [4, 4, 4]], np.float32)   # the cube's diagonal
    more = len(v) + np.arange(15, dtype=np.int64).reshape(5, 3)
    return np.concatenate([v, extra]), np.concatenate([f[:5], more, f[5:]])


def _open_cube():
    v, f = W.integer_cube(4)
    return v, f[~(v[f][:, :, 2] == 4).all(1)]


def _two_spheres():
    v, f = icosphere(2)
    v = v.astype(np.float32)
    return np.concatenate([v, v + np.float32([1.0, 0.25, 0.125])]), np.concatenate([f, f + len(v)]).astype(np.int64)


MESHES = dict(RAY_MESHES, edge_on=_edge_on, open_cube=_open_cube)


def _queries(P, F, seed, n_box=1200, n_each=100):
    """About 2000 queries: uniform in 1.3 x the bounds; the mesh's own vertices; vertices and (fp32) edge midpoints displaced along
    ONE axis, so that this axis' ray passes exactly through a vertex or an edge; the integer points around a small mesh; a query
    far outside the grid whose z ray still meets the bounds, two that meet nothing; NaN and +-inf."""
    rng = np.random.default_rng(seed)
    F = np.asarray(F, np.int64)
    used = P[np.unique(F)]
    lo, hi = used.min(0).astype(np.float64), used.max(0).astype(np.float64)
    c, size = 0.5 * (lo + hi), hi - lo
    size = np.where(size > 0, size, size.max())
    parts = [rng.uniform(c - 0.65 * size, c + 0.65 * size, (n_box, 3)), used[:300]]
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])[:n_each]
    mid = np.float32(0.5) * (P[e[:, 0]] + P[e[:, 1]])
    for a in range(3):
        for src in (used[:n_each], mid):
            moved = src.astype(np.float64).copy()
            moved[:, a] = rng.uniform(c[a] - 0.65 * size[a], c[a] + 0.65 * size[a], len(src))
            parts.append(moved)
    if size.max() <= 8:
        r = np.arange(np.floor(lo.min()) - 1, np.ceil(hi.max()) + 2)
        parts.append(np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)[:400])
    parts.append(np.array([[c[0], c[1], -1e6], [1e6, 1e6, 1e6], [-1e30, c[1], c[2]]]))
    parts.append(np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.5, 0.5, -np.inf]]))
    return np.concatenate([np.asarray(p, np.float64) for p in parts]).astype(np.float32)


_cases = {}


def _case(name):
    """(P, F, queries, brute-force counts): computed once per mesh and shared, never modified."""
    if name not in _cases:
        P, F = MESHES[name]()
        P, F = np.asarray(P, np.float32), np.asarray(F, np.int64)
        q = _queries(P, F, seed=40 + len(_cases))
        _cases[name] = (P, F, q, W.winding(q, P, F))
    return _cases[name]


def _form(form, monkeypatch):
    if form == "plain":
        monkeypatch.setenv("SCULPT_DISTANCE_FORM", "plain")
    else:
        monkeypatch.delenv("SCULPT_DISTANCE_FORM", raising=False)


def _dev(cuda, P, F, face_dtype=torch.int32):
    return torch.from_numpy(P).to(cuda), torch.from_numpy(np.asarray(F, np.int64)).to(cuda).to(face_dtype)


def _run(cuda, q, P, F, form, monkeypatch, face_dtype=torch.int32):
    _form(form, monkeypatch)
    return ops.mesh_winding(torch.from_numpy(q).to(cuda), *_dev(cuda, P, F, face_dtype))


def _same(got, want, what):
    got = got.cpu()
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    if not torch.equal(got, want):
        bad = np.nonzero((got != want).reshape(len(want), -1).any(1).numpy())[0]
        raise AssertionError("%s: %d of %d differ, first %d: %r vs %r" % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]]))


# ----------------------------------------------------------------------------------------------------------------- counts
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(MESHES))
def test_winding_equals_the_brute_force_bit_for_bit(cuda, monkeypatch, name, form):
    P, F, q, want = _case(name)
    got = _run(cuda, q, P, F, form, monkeypatch)
    assert got.dtype == torch.int32
    _same(got, want, "%s/%s" % (name, form))
    inside = ops.mesh_contains(torch.from_numpy(q).to(cuda), *_dev(cuda, P, F))
    assert inside.dtype == torch.bool
    _same(inside, W.inside_of(want), "%s/%s inside" % (name, form))


def test_the_cases_hold_what_they_are_meant_to():
    P, F, q, w = _case("sphere")
    finite = np.isfinite(q).all(1)
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    deep, far = finite & (r < 0.9), finite & (r > 1.01)
    assert deep.sum() > 100 and (w[deep] == 1).all() and far.sum() > 300 and (w[far] == 0).all()
    assert (w[~finite] == W.INT_MIN).all() and (~finite).sum() == 3
    assert (_case("doubled_cube")[3] == 2).any() and (_case("open_cube")[3][:, 2] != _case("open_cube")[3][:, 0]).any()
    P, F, q, w = _case("edge_on")
    cube = ((q > 0) & (q < 4)).all(1) & np.isfinite(q).all(1)
    assert cube.sum() > 200 and W.inside_of(w)[cube].all()     # the faces inside it cancel or do not count: still inside


@pytest.mark.parametrize("form", FORMS)
def test_int64_faces(cuda, monkeypatch, form):
    P, F, q, want = _case("cube")
    _same(_run(cuda, q, P, F, form, monkeypatch, face_dtype=torch.int64), want, "cube/int64/" + form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_query_counts_around_the_wave_and_block_sizes(cuda, monkeypatch, n, form):
    P, F, q, want = _case("sphere")
    got = _run(cuda, q[:n].copy(), P, F, form, monkeypatch)
    assert got.shape == (n, 3)
    _same(got, want[:n], "n=%d/%s" % (n, form))


@pytest.mark.parametrize("form", FORMS)
def test_no_faces(cuda, monkeypatch, form):
    P, _, q, _ = _case("triangle")
    q = q[-40:]
    got = _run(cuda, q, P, np.zeros((0, 3), np.int64), form, monkeypatch).cpu().numpy()
    finite = np.isfinite(q).all(1)
    assert (got[finite] == 0).all() and (got[~finite] == W.INT_MIN).all() and (~finite).sum() == 3


def test_bad_meshes_are_refused(cuda):
    P, F = _dev(cuda, *RAY_MESHES["triangle"]())
    q = torch.zeros((4, 3), device=cuda)
    with pytest.raises(ops.SculptError, match="out of range"):
        ops.mesh_winding(q, P, torch.tensor([[0, 1, 3]], dtype=torch.int32, device=cuda))
    bad = P.clone()
    bad[1, 2] = float("nan")
    with pytest.raises(ops.SculptError, match="non-finite"):
        ops.mesh_contains(q, bad, F)
    with pytest.raises(ops.SculptError):
        ops.mesh_winding(torch.zeros((4, 2), device=cuda), P, F)
    with pytest.raises(ops.SculptError, match="without faces"):
        ops.mesh_sdf_grid(P, F[:0], 16)
    with pytest.raises(ops.SculptError, match="no extent"):
        ops.mesh_voxel_remesh(P[:1], torch.zeros((1, 3), dtype=torch.int64, device=cuda), 16)


# ---------------------------------------------------------------------------------------------------------------- lattice
LATTICE = ((-1.3, -1.2, -1.1), 0.11, (20, 24, 37))     # n2 no multiple of 32, and an odd tail of the second wave's 64


@pytest.mark.parametrize("form", FORMS)
def test_the_lattice_kernel_equals_the_point_kernel(cuda, monkeypatch, form):
    P, F, _, _ = _case("sphere")
    lo, h, n = LATTICE
    _form(form, monkeypatch)
    planes, counts = ops.mesh_winding_lattice(*_dev(cuda, P, F), lo, h, n, want_counts=True)
    pts = W.lattice_points(lo, h, n)                    # the coordinate rule, restated
    at_points = ops.mesh_winding(torch.from_numpy(pts).to(cuda), *_dev(cuda, P, F))
    assert counts.dtype == torch.int32 and counts.shape == (*n, 3)
    assert torch.equal(counts.reshape(-1, 3), at_points)
    inside = W.inside_of(at_points.cpu().numpy()).reshape(n)
    assert 1000 < inside.sum() < inside.size // 4
    assert planes.dtype == torch.int32 and planes.shape == (n[0] * n[1], 2)
    _same(planes, W.pack_planes(inside), "planes")      # bits past n2 zero included
    only, none = ops.mesh_winding_lattice(*_dev(cuda, P, F), lo, h, n)
    assert none is None and torch.equal(only, planes)


def test_the_lattice_counts_equal_the_brute_force(cuda):
    P, F, _, _ = _case("sphere")
    lo, h, n = (-1.25, -1.25, -1.25), 0.25, (11, 11, 11)      # exact coordinates: lattice points on the sphere's poles and axes
    counts = ops.mesh_winding_lattice(*_dev(cuda, P, F), lo, h, n, want_counts=True)[1]
    _same(counts.reshape(-1, 3), W.winding(W.lattice_points(lo, h, n), P, F), "lattice/brute force")


def test_long_lines_and_crowded_cells(cuda):
    """What the line-sharing lattice kernel has beyond one trip: lines of more than 64 points (several points a lane) along
    every axis in turn, and cells with more than 64 listings (forty copies of the cube: 480 faces over about ten cells a side).
    Coordinates are multiples of 1/8, so the rays pass through edges and corners exactly; the brute force is the reference."""
    v, f = RAY_MESHES["cube"]()
    P, F = np.asarray(v, np.float32), np.concatenate([np.asarray(f, np.int64)] * 40)
    for n in ((70, 5, 12), (12, 70, 5), (5, 12, 130)):
        lo, h = (-0.25, -0.25, -0.25), 0.125
        planes, counts = ops.mesh_winding_lattice(*_dev(cuda, P, F), lo, h, n, want_counts=True)
        pts = W.lattice_points(lo, h, n)
        want = W.winding(pts, P, F)
        assert (want == 40).any() and (want == 0).any()
        _same(counts.reshape(-1, 3), want, "crowded %r" % (n,))
        _same(planes, W.pack_planes(W.inside_of(want).reshape(n)), "crowded planes %r" % (n,))
        assert torch.equal(ops.mesh_winding(torch.from_numpy(pts).to(cuda), *_dev(cuda, P, F)), counts.reshape(-1, 3))


# -------------------------------------------------------------------------------------------------------- signed distance
def test_signed_distance(cuda):
    P, F, q, w = _case("sphere")
    Q, (Pd, Fd) = torch.from_numpy(q).to(cuda), _dev(cuda, P, F)
    sd, face, closest = ops.mesh_signed_distance(Q, Pd, Fd)
    d2, face0, closest0 = ops.mesh_closest_points(Q, Pd, Fd)
    inside = ops.mesh_contains(Q, Pd, Fd)
    assert sd.dtype == torch.float64 and torch.equal(face, face0) and torch.equal(closest.view(torch.int32), closest0.view(torch.int32))
    want = torch.where(inside, -torch.sqrt(d2), torch.sqrt(d2))
    assert torch.equal(sd.view(torch.int64), want.view(torch.int64))          # NaN of the non-finite queries included
    finite = torch.isfinite(sd)
    assert torch.equal((sd < 0)[finite], (inside & (d2 > 0))[finite]) and int(inside.sum()) > 100
    assert bool(torch.isnan(sd[-3:]).all())
    empty = ops.mesh_signed_distance(Q[:0], Pd, Fd)
    assert empty[0].shape == (0,) and empty[1].dtype == torch.int64 and empty[2].shape == (0, 3)
    none = ops.mesh_signed_distance(Q[:5], Pd, Fd[:0])
    assert bool((none[0] == float("inf")).all()) and bool((none[1] == -1).all())


# --------------------------------------------------------------------------------------------------------------- sdf grid
@pytest.mark.parametrize("name", ["sphere", "open_cube"])
def test_sdf_grid_equals_the_restatement(cuda, name):
    P, F, _, _ = _case(name)
    vol, planes, lo, h = ops.mesh_sdf_grid(*_dev(cuda, P, F), 16)
    want_vol, want_planes, want_list, want_lo, want_h = W.sdf_grid(P, F, 16)
    assert lo == want_lo and h == want_h and vol.dtype == torch.float32
    _same(planes, want_planes, name + " planes")
    listed = ops.lattice_active_corners(planes, vol.shape)
    _same(listed, want_list, name + " list")
    assert len(want_list) > 500
    assert torch.equal(vol.cpu().view(torch.int32), torch.from_numpy(want_vol).view(torch.int32))
    bits = torch.from_numpy(W.unpack_planes(want_planes, tuple(vol.shape)))
    assert torch.equal(vol.cpu() > 0, bits) and int(bits.sum()) > 200
    wide = ops.mesh_sdf_grid(*_dev(cuda, P, F), (16, 5))[0]
    assert float(wide.abs().max()) == float(np.float32(5 * h)) and torch.equal(wide > 0, vol > 0)


# ----------------------------------------------------------------------------------------------------------- voxel remesh
def _edge_counts(f):
    f = f.cpu().numpy()
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    directed = np.unique(e, axis=0, return_counts=True)[1]
    undirected = np.unique(np.sort(e, 1), axis=0, return_counts=True)[1]
    return directed, undirected


def _signed_volume(v, f):
    a, b, c = (v[f[:, k]].double() for k in range(3))
    return float((a * torch.linalg.cross(b, c)).sum() / 6.0)


def test_voxel_remesh_of_the_icosphere(cuda):
    v0, f0 = icosphere(2)
    P, F = _dev(cuda, v0.astype(np.float32), f0)
    v, f = ops.mesh_voxel_remesh(P, F, 24)
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and int(f.max()) == len(v) - 1 and len(f) > 2000
    directed, undirected = _edge_counts(f)
    assert (directed == 1).all() and (undirected == 2).all()            # a closed, consistently oriented 2-manifold
    assert len(v) - len(undirected) + len(f) == 2
    comp = ops.mesh_components(f, len(v))
    assert len(comp["roots"]) == 1
    h = W.grid_rule(v0.astype(np.float32), f0, 24)[1]
    # wound outward: the signed volume is positive; every vertex lies within h = 1/12 of a surface between the spheres of radius
    # 0.96 (the icosphere's inscribed one) and 1, so the volume lies between those of the radii 0.96 - 2 h and 1 + 2 h
    assert 4.19 * 0.79 ** 3 < _signed_volume(v, f) < 4.19 * 1.17 ** 3
    d2 = ops.mesh_closest_points(v, P, F)[0]
    print("voxel remesh R=24: %d vertices, %d faces, farthest vertex %.3f h from the input" % (len(v), len(f), float(d2.max()) ** 0.5 / h))
    assert float(d2.max()) <= h * h                                       # a vertex lies on a lattice edge the surface crosses
    # ... and it is marching cubes of the restated volume
    want_vol, _, _, lo, h = W.sdf_grid(v0.astype(np.float32), f0, 24)
    rv, rf = ops.marching_cubes(torch.from_numpy(want_vol).to(cuda), 0.0, reference_order=True)
    rv = rv.cpu().numpy() * np.float32(h) + np.array(lo, np.float64).astype(np.float32)
    assert torch.equal(f, rf) and torch.equal(v.cpu().view(torch.int32), torch.from_numpy(rv).view(torch.int32))


def test_voxel_remesh_fuses_two_overlapping_spheres(cuda):
    P, F = _dev(cuda, *_two_spheres())
    assert len(ops.mesh_components(F, len(P))["roots"]) == 2
    v, f = ops.mesh_voxel_remesh(P, F, 24)
    comp = ops.mesh_components(f, len(v))
    assert len(comp["roots"]) == 1 and int(comp["face_counts"][0]) == len(f)
    directed, undirected = _edge_counts(f)
    assert (directed == 1).all() and (undirected == 2).all() and len(v) - len(undirected) + len(f) == 2
    centre = torch.tensor([[0.5, 0.125, 0.0625]], device=cuda)            # in both spheres: wound twice
    assert ops.mesh_winding(centre, P, F).tolist() == [[2, 2, 2]]
    assert ops.mesh_winding(centre, v, f).tolist() == [[1, 1, 1]]


# ------------------------------------------------------------------------------------------------------------ end to end
def test_extract_meshes_voxel_remesh(cuda):
    from _tsrmodel import small_model
    from sculptmate_amd.tsr.mesh import Mesh

    s = small_model(cuda, 32, enable_texture=True)
    m, plain = s["m"], s["plain"]
    same = m.extract_meshes(s["codes"], enable_texture=True, voxel_remesh=None, **s["kw"])[0]
    assert torch.equal(same.vertices.view(torch.int32), plain.vertices.view(torch.int32)) and torch.equal(same.faces, plain.faces)
    assert torch.equal(same.vertex_colors.view(torch.int32), plain.vertex_colors.view(torch.int32))
    alone = m.extract_meshes(s["codes"], voxel_remesh=24, **s["kw"])[0]
    v, f = ops.mesh_voxel_remesh(plain.vertices, plain.faces, 24)
    assert torch.equal(alone.vertices.view(torch.int32), v.view(torch.int32)) and torch.equal(alone.faces, f) and alone.quads is None
    # its place in the chain: after keep_components, before smooth
    chained = m.extract_meshes(s["codes"], keep_components="largest", voxel_remesh=(24, 3), smooth=2, **s["kw"])[0]
    by_hand = Mesh(plain.vertices, plain.faces).keep_components("largest").voxel_remesh((24, 3)).smooth(2)
    assert torch.equal(chained.vertices.view(torch.int32), by_hand.vertices.view(torch.int32)) and torch.equal(chained.faces, by_hand.faces)
    # the method carries nothing over, and the queries of a Mesh are the ops'
    remeshed = plain.voxel_remesh(24)
    assert plain.vertex_colors is not None and remeshed.vertex_colors is None and remeshed.uvs is None and remeshed.quads is None
    assert torch.equal(remeshed.faces, f)
    q = plain.vertices[:100] * 0.5
    assert torch.equal(plain.winding_number(q), ops.mesh_winding(q, plain.vertices, plain.faces))
    assert torch.equal(plain.contains(q), ops.mesh_contains(q, plain.vertices, plain.faces))
    assert torch.equal(remeshed.signed_distance(q)[0].view(torch.int64), ops.mesh_signed_distance(q, v, f)[0].view(torch.int64))
    # a bad value raises before any launch: scene codes that cannot even be iterated are never reached
    for bad in (4, True, 24.0, (24, 0)):
        with pytest.raises(ValueError, match="voxel_remesh"):
            m.extract_meshes(None, voxel_remesh=bad, **s["kw"])
