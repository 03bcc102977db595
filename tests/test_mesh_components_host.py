"""Connected components of a mesh, without a GPU: the numpy restatement tests/_ccref.py against scipy and against marching
cubes of an analytic volume, argument validation of the public surface, and Mesh.keep_components on host arrays."""
import numpy as np
import pytest
import torch

import _ccref

BAD_KEEPS = ["biggest", 0, -3, 1.0, 0.0, True]


def _fixtures():
    tri = (np.array([[0, 1, 2]], np.int32), 3)
    two = (np.array([[0, 1, 2], [3, 4, 5]], np.int32), 6)
    return {"triangle": tri, "two": two, "strip_perm": _ccref.strip(65, "perm", 3), "strip_desc": _ccref.strip(64, "desc"),
            "comb": _ccref.comb(), "dust": _ccref.dust(), "degenerate": _ccref.degenerate()}


@pytest.mark.parametrize("name", sorted(_fixtures()))
def test_ccref_against_scipy(name):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components

    f, nv = _fixtures()[name]
    f64 = f.astype(np.int64)
    a = np.concatenate([f64[:, 0], f64[:, 0]])
    b = np.concatenate([f64[:, 1], f64[:, 2]])
    n, ids = connected_components(sp.coo_matrix((np.ones(len(a)), (a, b)), shape=(nv, nv)), directed=False)
    smallest = np.full(n, nv, np.int64)
    np.minimum.at(smallest, ids, np.arange(nv))
    comp = _ccref.components(f, nv)
    assert np.array_equal(comp["labels"], smallest[ids])
    assert len(comp["roots"]) == n and np.array_equal(comp["roots"], np.sort(smallest))
    assert comp["face_counts"].sum() == len(f) and comp["vertex_counts"].sum() == nv
    assert np.array_equal(comp["face_counts"], np.bincount(ids[f64[:, 0]], minlength=n)[np.argsort(smallest)])


def test_ccref_rules_on_the_comb():
    f, nv = _ccref.comb()
    comp = _ccref.components(f, nv)
    assert sorted(comp["face_counts"]) == list(range(1, 301))
    assert len(_ccref.kept_roots(comp, "largest")) == 1 and len(_ccref.kept_roots(comp, 150)) == 151
    assert len(_ccref.kept_roots(comp, 0.5)) == 151   # count >= 150.0
    v = np.random.default_rng(0).random((nv, 3)).astype(np.float32)
    v2, f2, vi, fi = _ccref.keep_components(v, f, "largest")
    assert len(f2) == 300 and len(v2) == 302 and f2.dtype == f.dtype and np.array_equal(v2[f2], v[f[fi]])
    assert (np.diff(vi) > 0).all() and (np.diff(fi) > 0).all()


def test_ccref_degenerate_and_isolated():
    f, nv = _ccref.degenerate()
    comp = _ccref.components(f, nv)
    assert comp["roots"].tolist() == [0, 8, 11, 12, 14, 15]
    assert comp["face_counts"].tolist() == [8, 1, 0, 1, 0, 0] and comp["vertex_counts"].tolist() == [8, 3, 1, 2, 1, 1]
    for keep in ("largest", 1, 0.1):
        vi = _ccref.keep_components(np.zeros((nv, 3), np.float32), f, keep)[2]
        assert not set(vi.tolist()) & {11, 14, 15}


def test_blobs_through_marching_cubes():
    """Lewiner marching cubes (the oracle's) over seven well-separated blobs gives seven components, and keeping the largest
    gives the mesh of the large sphere's volume alone: vertices bit for bit, faces equal after re-indexing, IN THE SAME ORDER --
    marching cubes emits vertices and faces in the scan order of the cells, so deleting the other blobs' rows leaves the large
    sphere's own sequence (the order claim holds; no comparison of coordinate triples was needed)."""
    from oracle import capi

    v, f = capi.marching_cubes(_ccref.blob_volume(), 0.0)
    comp = _ccref.components(f, len(v))
    assert len(comp["roots"]) == len(_ccref.BLOBS) == 7 and (comp["face_counts"] > 0).all()
    v1, f1 = capi.marching_cubes(_ccref.blob_volume(_ccref.BLOBS[:1]), 0.0)
    v2, f2, vi, fi = _ccref.keep_components(v, f, "largest")
    assert np.array_equal(v2.view(np.uint32), v1.view(np.uint32)) and np.array_equal(f2, f1)
    # the border blob is open (edges with one face), the others closed
    lab = comp["labels"][f[:, 0]]
    open_components = 0
    for r in comp["roots"]:
        e = np.sort(np.concatenate([f[lab == r][:, [0, 1]], f[lab == r][:, [1, 2]], f[lab == r][:, [2, 0]]]), axis=1)
        open_components += int((np.unique(e, axis=0, return_counts=True)[1] == 1).any())
    assert open_components == 1
    # the two equal blobs: equal counts, and every rule keeps or drops them together
    fc = np.sort(comp["face_counts"])
    assert (np.diff(fc) == 0).sum() == 1
    assert len(_ccref.kept_roots(comp, int(fc[-1]))) == 1 and len(_ccref.kept_roots(comp, 1)) == 7


@pytest.mark.parametrize("keep", BAD_KEEPS, ids=repr)
def test_bad_keep_is_a_value_error_before_any_device_work(keep):
    from sculptmate_amd import ops
    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import Mesh

    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)   # CPU tensors: the check comes first
    with pytest.raises(ValueError):
        ops.mesh_keep_components(v, f, keep)
    with pytest.raises(ValueError):
        Mesh(v, f).keep_components(keep)
    with pytest.raises(ValueError):
        TSR(SMALL_CFG).extract_meshes([], keep_components=keep)


def test_good_keeps_and_cpu_tensors():
    from sculptmate_amd import _lib, ops

    assert ops.keep_rule("largest") == (_lib.CC_KEEP_LARGEST, 0, 0.0)
    assert ops.keep_rule(7) == ops.keep_rule(np.int64(7)) == (_lib.CC_KEEP_MIN_FACES, 7, 0.0)
    assert ops.keep_rule(0.25) == ops.keep_rule(np.float32(0.25)) == (_lib.CC_KEEP_FRACTION, 0, 0.25)
    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(ops.SculptError):     # no CPU fallback
        ops.mesh_keep_components(v, f, "largest")
    with pytest.raises(ops.SculptError):
        ops.mesh_components(f, 3)
    with pytest.raises(ops.SculptError):
        ops.mesh_component_labels(f, 3)
    assert _lib.lib.sculpt_mesh_components_workspace_bytes(2 ** 31, 1) == 0 and _lib.lib.sculpt_mesh_components_workspace_bytes(1, -1) == 0
    n = _lib.lib.sculpt_mesh_components_workspace_bytes(907205, 1814000)
    assert 16 * 907205 < n < 16 * 907205 + 4 * (2 * 886 + 1772) + 2048


def test_generator_attribute_defaults_to_none():
    from sculptmate_amd.generate import TripoGenerator

    assert TripoGenerator(torch.device("cpu")).keep_components is None


def test_mesh_keep_components_gathers_per_vertex_and_per_corner(monkeypatch):
    """A baked-shape mesh on host arrays, ops.mesh_keep_components replaced by the restatement: colours and normals follow
    vertex_index, the per-corner uvs follow face_index in threes, the texture is the same object."""
    from sculptmate_amd import ops
    from sculptmate_amd.tsr.system import Mesh

    monkeypatch.setattr(ops, "mesh_keep_components", _ccref.keep_components)
    f, nv = _ccref.shuffled([_ccref.strip(5), _ccref.strip(9), _ccref.strip(2)], 11, extra_vertices=2)
    rng = np.random.default_rng(12)
    v, col, nrm = (rng.random((nv, 3)).astype(np.float32) for _ in range(3))
    uv = rng.random((3 * len(f), 2)).astype(np.float32)
    tex = rng.random((4, 4, 3)).astype(np.float32)
    got = Mesh(v, f, col, uvs=uv, texture=tex, vertex_normals=nrm).keep_components("largest")
    v2, f2, vi, fi = _ccref.keep_components(v, f, "largest")
    assert len(f2) == 9 and np.array_equal(got.vertices, v2) and np.array_equal(got.faces, f2)
    assert np.array_equal(got.vertex_colors, col[vi]) and np.array_equal(got.vertex_normals, nrm[vi])
    assert got.uvs.shape == (27, 2) and np.array_equal(got.uvs.reshape(-1, 3, 2), uv.reshape(-1, 3, 2)[fi])
    assert got.texture is tex
    plain = Mesh(v, f).keep_components(4)
    assert plain.vertex_colors is None and plain.uvs is None and plain.vertex_normals is None and len(plain.faces) == 14
