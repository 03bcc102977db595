"""Ray queries on the device (csrc/mesh_ray.hip) against the NumPy restatement (tests/_rayref.py): the closest hit bit for bit
against the brute force in both kernel forms, the fused occlusion bit for bit against the composed route and the restatement,
and one end-to-end run on the small model's mesh."""
import numpy as np
import pytest
import torch

import _rayref as RR
from sculptmate_amd import ops
from test_gpu_mesh_distance import MESHES as DISTANCE_MESHES
from test_remesh import icosphere

pytestmark = pytest.mark.gpu

FORMS = ["default", "plain"]


def _doubled_cube():
    v, f = DISTANCE_MESHES["cube"]()
    return v, np.concatenate([f, f])


MESHES = dict(DISTANCE_MESHES, doubled_cube=_doubled_cube)

_cases = {}


def _case(name):
    """(P, F, origins, directions, parts, reference with tie counts, second pass): computed once per mesh and shared, never
    modified.  The second pass: for three rays that hit (the quartiles of the positive hit t), the whole ray set again with
    t_max equal to that ray's reference t and one ulp below it -> [(t_max, reference), ...], equal and below in turn."""
    if name not in _cases:
        P, F = MESHES[name]()
        O, D, parts = RR.ray_set(P, F, seed=11 + len(_cases))
        want = RR.ray_cast(O, D, P, F, want_ties=True)
        finite_hits = np.sort(want[0][(want[1] >= 0) & (want[0] > 0)])
        second = []
        for q in (0.25, 0.5, 0.75):
            t = float(finite_hits[int(q * (len(finite_hits) - 1))])
            for t_max in (t, float(np.nextafter(t, 0.0))):
                second.append((t_max, RR.ray_cast(O, D, P, F, 0.0, t_max)))
        _cases[name] = (P, F, O, D, parts, want, second)
    return _cases[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _assert_same(got, want, what):
    for g, w, part in zip(got, want, ("t", "face", "uv")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, g.shape)
        rows = (len(w), int(np.prod(w.shape[1:])))
        bad = np.nonzero((_bits(g) != _bits(w)).reshape(rows).any(1) & ~(np.isnan(w) & np.isnan(g)).reshape(rows).all(1))[0]
        assert len(bad) == 0, "%s %s: %d of %d differ, first %d: %r vs %r" % (what, part, len(bad), len(w), bad[0], g[bad[0]], w[bad[0]])


def _form(form, monkeypatch):
    if form == "plain":
        monkeypatch.setenv("SCULPT_DISTANCE_FORM", "plain")
    else:
        monkeypatch.delenv("SCULPT_DISTANCE_FORM", raising=False)


def _run(cuda, O, D, P, F, form, monkeypatch, t_max=np.inf, face_dtype=torch.int32):
    _form(form, monkeypatch)
    return ops.mesh_ray_cast(torch.from_numpy(O).to(cuda), torch.from_numpy(D).to(cuda), torch.from_numpy(P).to(cuda),
                             torch.from_numpy(F.astype(np.int64)).to(cuda).to(face_dtype), 0.0, t_max)


# ----------------------------------------------------------------------------------------------------------- closest hit
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(MESHES))
def test_ray_cast_equals_the_brute_force_bit_for_bit(cuda, monkeypatch, name, form):
    P, F, O, D, _, want, second = _case(name)
    got = _run(cuda, O, D, P, F, form, monkeypatch)
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.int64 and got[2].dtype == torch.float32
    _assert_same(got, want[:3], "%s/%s" % (name, form))
    for t_max, ref in second:
        _assert_same(_run(cuda, O, D, P, F, form, monkeypatch, t_max=t_max), ref, "%s/%s/t_max=%r" % (name, form, t_max))


def test_the_cases_hold_what_they_are_meant_to():
    """Asserted on the REFERENCE: the comparison above is not empty of hits, of ties or of the odd answers."""
    for name in ("sphere", "cube", "doubled_cube"):
        P, F, O, D, parts, (t, face, uv, ties), second = _case(name)
        share = float((face >= 0).mean())
        print("%s: %.1f %% of %d rays hit" % (name, 100 * share, len(O)))
        assert 0.25 <= share <= 0.75, (name, share)
        assert len(second) == 6
        for (t_max, ref), (_, below) in zip(second[::2], second[1::2]):   # equal still hits that face; one ulp below does not
            at = np.nonzero(t == t_max)[0]
            assert len(at) and (ref[1][at] == face[at]).all() and (ref[0][at] == t_max).all() and not (below[0][at] == t_max).any()
    P, F, O, D, parts, (t, face, uv, ties), _ = _case("sphere")
    aimed = parts["targets"]
    n_tied = int((ties[aimed] >= 2).sum())
    print("sphere: %d of %d aimed rays have two or more faces at the winning t" % (n_tied, aimed.stop - aimed.start))
    assert n_tied >= 40
    edges = parts["edges"]
    assert edges.stop - edges.start == 320 and (t[edges] == 0).all() and (ties[edges] >= 2).all()
    odd = parts["odd"]
    assert np.isinf(t[odd][:2]).all() and np.isnan(t[odd][2:]).all() and (face[odd] == -1).all() and (uv[odd] == 0).all()
    P, F, O, D, parts, (t, face, uv, ties), _ = _case("doubled_cube")
    assert (face < 12).all() and (ties[face >= 0] >= 2).all()
    P, F, O, D, parts, (t, face, uv, ties), _ = _case("sheet")
    assert (face[parts["plane"]] == -1).all()                   # rays in the sheet's plane miss it


@pytest.mark.parametrize("form", FORMS)
def test_int64_faces(cuda, monkeypatch, form):
    P, F, O, D, _, want, _ = _case("cube")
    _assert_same(_run(cuda, O, D, P, F, form, monkeypatch, face_dtype=torch.int64), want[:3], "cube/int64/" + form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_ray_counts_around_the_wave_and_block_sizes(cuda, monkeypatch, n, form):
    P, F, O, D, parts, want, _ = _case("sphere")
    s = parts["targets"].start - 20                               # ordinary rays, then rays at vertices
    got = _run(cuda, O[s:s + n].copy(), D[s:s + n].copy(), P, F, form, monkeypatch)
    assert got[0].shape == (n,) and got[1].shape == (n,) and got[2].shape == (n, 2)
    _assert_same(got, [w[s:s + n] for w in want[:3]], "n=%d/%s" % (n, form))


@pytest.mark.parametrize("form", FORMS)
def test_no_faces(cuda, monkeypatch, form):
    P, _, O, D, _, _, _ = _case("triangle")
    O, D = O[-40:], D[-40:]
    t, face, uv = _run(cuda, O, D, P, np.zeros((0, 3), np.int32), form, monkeypatch)
    finite = np.isfinite(O).all(1) & np.isfinite(D).all(1)
    t = t.cpu().numpy()
    assert (t[finite] == np.inf).all() and np.isnan(t[~finite]).all() and (face.cpu().numpy() == -1).all()
    assert (uv.cpu().numpy() == 0).all()


def test_the_mesh_method_and_a_bad_range(cuda):
    from sculptmate_amd.tsr.system import Mesh

    P, F, O, D, _, want, _ = _case("cube")
    v, f = torch.from_numpy(P).to(cuda), torch.from_numpy(F).to(cuda)
    o, d = torch.from_numpy(O).to(cuda), torch.from_numpy(D).to(cuda)
    _assert_same(Mesh(v, f).ray_cast(o, d), want[:3], "Mesh.ray_cast")
    _assert_same(ops.mesh_ray_cast(o.double(), d.double(), v.double(), f), want[:3], "fp64 inputs")
    for bad in ((-1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("nan"))):
        with pytest.raises(ValueError):
            ops.mesh_ray_cast(o, d, v, f, *bad)
    with pytest.raises(ops.SculptError):
        ops.mesh_ray_cast(o, d[:-1], v, f)
    with pytest.raises(ops.SculptError, match="out of range"):
        ops.mesh_ray_cast(o, d, v, torch.tensor([[0, 1, 8]], dtype=torch.int32, device=cuda))


# ------------------------------------------------------------------------------------------------------------- occlusion
def _nested():
    """A sphere of radius 1 (80 faces) inside an inverted sphere of radius 3 (320 faces, its normals point inwards)."""
    v1, f1 = icosphere(1)
    v2, f2 = icosphere(2)
    v = np.concatenate([v1, 3.0 * v2]).astype(np.float32)
    return v, np.concatenate([f1, f2[:, ::-1] + len(v1)]).astype(np.int32)


_occ = {}


def _occlusion_case(cuda, name):
    """(mesh tensors, points, normals) of an occlusion case; the normals of the two sphere cases are the device's own
    ops.vertex_normals, read back for the restatement."""
    if name not in _occ:
        if name == "cube":
            P, F = RR.cube()
            rng = np.random.default_rng(5)
            pts = rng.uniform(0.05, 0.95, (100, 3)).astype(np.float32)
            nrm = rng.normal(size=(100, 3)).astype(np.float32)
        else:
            P, F = DISTANCE_MESHES["sphere"]() if name == "sphere" else _nested()
            pts = P
            nrm = ops.vertex_normals(torch.from_numpy(P).to(cuda), torch.from_numpy(F).to(cuda)).cpu().numpy()
        _occ[name] = (P, F, pts, nrm)
    return _occ[name]


@pytest.mark.parametrize("far", [None, 2.5])
@pytest.mark.parametrize("name", ["sphere", "cube", "nested"])
def test_occlusion_equals_the_composed_route_and_the_restatement_bit_for_bit(cuda, name, far):
    P, F, pts, nrm = _occlusion_case(cuda, name)
    rule = (64, far)
    t = [torch.from_numpy(x).to(cuda) for x in (pts, nrm, P, F)]
    offset = 2.0 ** -13 * float((P.max(0).astype(np.float64) - P.min(0).astype(np.float64)).max())
    want = RR.occlusion(pts, nrm, ops.occlusion_directions(64, 0), P, F, np.float32(offset), np.inf if far is None else far)
    fused = ops.mesh_occlusion(*t, occlusion=rule).cpu().numpy()
    composed = ops.mesh_occlusion_composed(*t, occlusion=rule).cpu().numpy()
    explicit = ops.mesh_occlusion(*t, occlusion=rule, offset=offset).cpu().numpy()
    assert fused.dtype == np.float32 and fused.shape == (len(pts),)
    assert np.array_equal(_bits(fused), _bits(composed)), int((_bits(fused) != _bits(composed)).sum())
    assert np.array_equal(_bits(fused), _bits(want)), int((_bits(fused) != _bits(want)).sum())
    assert np.array_equal(_bits(fused), _bits(explicit))       # the default offset is 2^-13 of the longest side
    if name == "sphere":
        assert (want == 1.0).all()                              # a convex body sees nothing of itself
    elif name == "cube":
        assert (want == 0.0).all()                              # from inside a closed body every ray hits
    else:
        assert (want >= 0).all() and (want <= 1).all()          # bits only: no analytic value is stated for this case
        if far is not None:
            assert ((want > 0) & (want < 1)).any()              # ... but with short rays it is not all 0 or all 1


def test_occlusion_of_odd_points(cuda):
    P, F, _, _ = _occlusion_case(cuda, "sphere")
    pts = np.array([[0, 0, 2], [0, 0, 2], [np.nan, 0, 0], [0, 0, 2], [0, 0, 0]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, 0], [0, 0, 1], [0, np.inf, 0], [0, 0, -1]], np.float32)
    t = [torch.from_numpy(x).to(cuda) for x in (pts, nrm, P, F)]
    got = ops.mesh_occlusion(*t, occlusion=16, seed=3).cpu().numpy()
    want = RR.occlusion(pts, nrm, ops.occlusion_directions(16, 3), P, F, np.float32(2.0 ** -13 * 2.0))
    assert np.array_equal(got, want, equal_nan=True), (got, want)
    assert got[0] == 1.0 and got[1] == 1.0 and np.isnan(got[2]) and np.isnan(got[3]) and got[4] == 0.0
    assert ops.mesh_occlusion(t[0][:0], t[1][:0], t[2], t[3]).shape == (0,)
    none = ops.mesh_occlusion(t[0][:2], t[1][:2], t[2], t[3][:0])
    assert (none.cpu().numpy() == 1.0).all()                    # no face: nothing occludes


# ------------------------------------------------------------------------------------------- one index, every query method
_TETRA = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32),
          np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32))       # wound outwards


def _every_query(cuda, P, F, pts, nrm, O, D, occ_dirs, cone_dirs, offset):
    """The five point and ray queries of ONE _SurfaceIndex over (P, F), as NumPy arrays."""
    dev = [torch.from_numpy(np.ascontiguousarray(x)).to(cuda) for x in (P, F, pts, nrm, O, D, occ_dirs, cone_dirs)]
    P_, F_, pts_, nrm_, O_, D_, occ_, cone_ = dev
    index = ops._SurfaceIndex(P_, F_)
    got = dict(closest=index.closest(pts_), winding=index.winding(pts_), ray_cast=index.ray_cast(O_, D_),
               occlusion=index.occlusion(pts_, nrm_, occ_, offset, np.inf),
               thickness=index.thickness(pts_, nrm_, cone_, offset, np.inf, 1.0))
    return {k: [x.cpu().numpy() for x in (v if isinstance(v, tuple) else (v,))] for k, v in got.items()}


@pytest.mark.parametrize("form", FORMS)
def test_every_query_of_one_index_without_faces(cuda, monkeypatch, form):
    """Every null pointer of the launch path at once: no mesh, no lists, no records, no order."""
    _form(form, monkeypatch)
    P = _TETRA[0]
    pts = np.array([[0.2, 0.2, 0.2], [1, 1, 1], [-3, 0.5, 2]], np.float32)
    nrm = np.array([[0, 0, 1], [1, 1, 1], [0, -1, 0]], np.float32)
    D = np.array([[1, 0, 0], [-1, -1, -1], [0, 0, -2]], np.float32)
    got = _every_query(cuda, P, np.zeros((0, 3), np.int32), pts, nrm, pts, D, ops.occlusion_directions(4), ops.thickness_directions(4),
                       2.0 ** -10)
    d2, face, closest = got["closest"]
    assert d2.dtype == np.float64 and (d2 == np.inf).all() and face.dtype == np.int32 and (face == -1).all()
    assert closest.dtype == np.float32 and np.array_equal(closest, pts)
    assert got["winding"][0].dtype == np.int32 and got["winding"][0].shape == (3, 3) and (got["winding"][0] == 0).all()
    t, face, uv = got["ray_cast"]
    assert t.dtype == np.float64 and (t == np.inf).all() and face.dtype == np.int32 and (face == -1).all()
    assert uv.dtype == np.float32 and uv.shape == (3, 2) and (uv == 0).all()
    assert got["occlusion"][0].dtype == np.float32 and (got["occlusion"][0] == 1.0).all()
    thick, thin, valid = got["thickness"]
    assert thick.dtype == thin.dtype == np.float32 and (thick == np.inf).all() and (thin == np.inf).all()
    assert valid.dtype == np.int32 and (valid == 0).all()


@pytest.mark.parametrize("form", FORMS)
def test_every_query_of_one_index_equals_the_brute_force(cuda, monkeypatch, form):
    """A tetrahedron, one point inside and one outside, k = 4: every method of one index against its restatement, bit for bit."""
    import _distref
    import _thickref
    import _windref

    _form(form, monkeypatch)
    P, F = _TETRA
    pts = np.array([[0.2, 0.2, 0.2], [1, 1, 1]], np.float32)
    nrm = np.array([[0, 0, 1], [0.5, 0.5, 0.70703125]], np.float32)
    D = np.array([[1, 0.25, 0], [-1, -1, -1]], np.float32)
    occ_dirs, cone_dirs, offset = ops.occlusion_directions(4), ops.thickness_directions(4), np.float32(2.0 ** -10)
    got = _every_query(cuda, P, F, pts, nrm, pts, D, occ_dirs, cone_dirs, float(offset))
    want = dict(closest=_distref.closest(pts, P, F), winding=(_windref.winding(pts, P, F),), ray_cast=RR.ray_cast(pts, D, P, F),
                occlusion=(RR.occlusion(pts, nrm, occ_dirs, P, F, offset),), thickness=_thickref.thickness(pts, nrm, cone_dirs, P, F, offset))
    for name in want:
        assert len(got[name]) == len(want[name])
        for g, w in zip(got[name], want[name]):
            if g.dtype == np.int32 and w.dtype == np.int64:       # the index reports faces as int32, the restatements as int64
                g = g.astype(np.int64)
            assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
            assert np.array_equal(_bits(g), _bits(w)), (name, form, g, w)
    # asserted on the REFERENCE: the case holds what it is meant to
    assert want["closest"][0][0] > 0 and want["ray_cast"][1][0] >= 0 and want["ray_cast"][1][1] >= 0
    assert (want["winding"][0][0] == 1).all() and (want["winding"][0][1] == 0).all()
    assert want["thickness"][2][0] == 4 and want["thickness"][2][1] == 0            # inside: every ray leaves through a back face
    assert want["occlusion"][0][0] == 0.0 and want["occlusion"][0][1] == 1.0        # inside a closed body; outside, facing away


# ------------------------------------------------------------------------------------------------------------ end to end
def test_extract_meshes_sets_the_vertex_occlusion(cuda):
    from _tsrmodel import small_model
    from sculptmate_amd.tsr import TSR

    s = small_model(cuda, 32)
    m, plain = s["m"], s["plain"]
    mesh = m.extract_meshes(s["codes"], occlusion=16, **s["kw"])[0]
    assert torch.equal(mesh.vertices, plain.vertices) and torch.equal(mesh.faces, plain.faces)
    assert plain.vertex_occlusion is None
    ao = mesh.vertex_occlusion
    assert ao.dtype == torch.float32 and ao.shape == (plain.vertices.shape[0],)
    assert bool((ao >= 0).all()) and bool((ao <= 1).all()) and 0 < float(ao.mean()) < 1
    again = plain.ambient_occlusion(16, outward=TSR.WINDING_OUTWARD)
    assert torch.equal(ao.view(torch.int32), again.view(torch.int32))
    # the sign constant: a binary choice, so the majority decides
    facet = TSR.WINDING_OUTWARD * ops.vertex_normals(plain.vertices, plain.faces)
    field = m.field_normals(plain.vertices, s["codes"][0])
    share = float(((facet * field).sum(1) > 0).float().mean())
    print("WINDING_OUTWARD x facet normals agree with the field normals at %.1f %% of %d vertices" % (100 * share, len(ao)))
    assert share > 0.5
    kept = mesh.keep_components("largest")
    assert kept.vertex_occlusion.shape == (kept.vertices.shape[0],)
    assert mesh.smooth(1).vertex_occlusion is None and mesh.simplify(0.5).vertex_occlusion is None
