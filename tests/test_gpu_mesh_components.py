"""ops.mesh_components / ops.mesh_keep_components (csrc/mesh_components.hip) and the layers above them on the GPU, against the
numpy restatement tests/_ccref.py.  Integer work: every comparison is equality (vertex rows bit for bit)."""
import numpy as np
import pytest
import torch

import _ccref
import _tsrmodel

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a).view(np.uint32)


def _vertices(nv, seed=1):
    return np.random.default_rng(seed).random((nv, 3)).astype(np.float32)


def _check(cuda, f, nv, keeps=("largest", 1, 2, 0.5), v=None):
    """mesh_components, mesh_component_labels and mesh_keep_components under every rule of `keeps` against _ccref."""
    from sculptmate_amd import ops

    ft = torch.from_numpy(np.ascontiguousarray(f)).to(cuda)
    want = _ccref.components(f, nv)
    got = ops.mesh_components(ft, nv)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == torch.int32 and got[k].is_cuda and np.array_equal(_np(got[k]), want[k]), k
    assert np.array_equal(_np(ops.mesh_component_labels(ft, nv)), want["labels"])
    v = _vertices(nv) if v is None else v
    vt = torch.from_numpy(v).to(cuda)
    for keep in keeps:
        wv, wf, wvi, wfi = _ccref.keep_components(v, f, keep)
        gv, gf, gvi, gfi = ops.mesh_keep_components(vt, ft, keep)
        assert gv.dtype == torch.float32 and gf.dtype == ft.dtype and gvi.dtype == torch.int64 and gfi.dtype == torch.int64
        assert gv.shape == wv.shape and np.array_equal(_bits(gv), wv.view(np.uint32)), keep
        assert gf.shape == wf.shape and np.array_equal(_np(gf), wf), keep
        assert np.array_equal(_np(gvi), wvi) and np.array_equal(_np(gfi), wfi), keep
    return want


def test_one_triangle_and_no_face(cuda):
    from sculptmate_amd import ops

    want = _check(cuda, np.array([[0, 1, 2]], np.int32), 3)
    assert want["roots"].tolist() == [0] and want["face_counts"].tolist() == [1] and want["vertex_counts"].tolist() == [3]
    want = _check(cuda, np.zeros((0, 3), np.int32), 3)     # nothing is launched: no component has a face
    assert want["labels"].tolist() == [0, 1, 2] and len(want["roots"]) == 0
    out = ops.mesh_keep_components(torch.zeros((3, 3), device=cuda), torch.zeros((0, 3), dtype=torch.int64, device=cuda), "largest")
    assert [tuple(t.shape) for t in out] == [(0, 3), (0, 3), (0,), (0,)] and out[1].dtype == torch.int64


def test_a_tie_goes_to_the_smaller_root_not_to_the_first_face(cuda):
    from sculptmate_amd import ops

    v = torch.from_numpy(_vertices(6)).to(cuda)
    for f, kept_face in (([[0, 1, 2], [3, 4, 5]], 0), ([[3, 4, 5], [0, 1, 2]], 1), ([[5, 3, 4], [2, 1, 0]], 1)):
        f = np.array(f, np.int32)
        _check(cuda, f, 6)
        out = ops.mesh_keep_components(v, torch.from_numpy(f).to(cuda), "largest")
        assert _np(out[3]).tolist() == [kept_face] and _np(out[2]).tolist() == [0, 1, 2]


@pytest.mark.parametrize("order", ["asc", "desc", "perm"])
@pytest.mark.parametrize("n", [63, 64, 65, 4097])
def test_strip_is_one_component(cuda, n, order):
    """Ascending and descending numbers make the longest parent chains, the permutation the hook races."""
    f, nv = _ccref.strip(n, order, seed=n)
    want = _check(cuda, f, nv, keeps=("largest", n, 0.999))
    assert not want["labels"].any() and want["face_counts"].tolist() == [n] and want["vertex_counts"].tolist() == [nv]


def test_comb_of_300_strips(cuda):
    from sculptmate_amd import ops

    f, nv = _ccref.comb()
    want = _check(cuda, f, nv, keeps=("largest", 150, 0.5, 300, 1))
    assert sorted(want["face_counts"].tolist()) == list(range(1, 301))
    v, ft = torch.from_numpy(_vertices(nv)).to(cuda), torch.from_numpy(f).to(cuda)
    assert ops.mesh_keep_components(v, ft, "largest")[1].shape[0] == 300
    for keep in (150, 0.5):   # 151 strips: 150 .. 300 faces
        kept = ops.mesh_keep_components(v, ft, keep)[1]
        assert kept.shape[0] == sum(range(150, 301)) and len(ops.mesh_components(kept, int(kept.max()) + 1)["roots"]) == 151


def test_dust(cuda):
    """20 000 lone triangles and one strip: scans over many workgroups, 20 001 roots ascending."""
    f, nv = _ccref.dust()
    assert nv == 65002
    want = _check(cuda, f, nv, keeps=("largest", 2, 1))
    assert len(want["roots"]) == 20001 and (np.diff(want["roots"]) > 0).all() and want["face_counts"].max() == 5000


def test_more_than_1024_chunks(cuda):
    """Nv above 1024 x 1024: the scan of the per-1024 totals takes a second trip and carries."""
    nv = 1024 * 1024 + 1500
    rng = np.random.default_rng(9)
    ids = np.concatenate([[nv - 1, 1024 * 1024 + 7, 5], 10 + rng.choice(1024 * 1024 - 20, 297, replace=False)])
    f = np.concatenate([ids[:102][_ccref.strip(100)[0]], ids[102:].reshape(-1, 3)]).astype(np.int32)   # a strip of 100 and 66 triangles
    want = _check(cuda, f, nv, keeps=("largest", 1))
    assert len(want["roots"]) == nv - 300 + 67


def test_degenerate_faces_and_isolated_vertices(cuda):
    f, nv = _ccref.degenerate()
    want = _check(cuda, f, nv, keeps=("largest", 1, 2, 0.1))
    assert want["roots"].tolist() == [0, 8, 11, 12, 14, 15] and want["face_counts"].tolist() == [8, 1, 0, 1, 0, 0]


def test_index_types_and_strides(cuda):
    from sculptmate_amd import ops

    f, nv = _ccref.comb(seed=21)
    v = torch.from_numpy(_vertices(nv)).to(cuda)
    f32, f64 = torch.from_numpy(f).to(cuda), torch.from_numpy(f.astype(np.int64)).to(cuda)
    _check(cuda, f.astype(np.int64), nv, keeps=("largest", 40))
    a, b = ops.mesh_keep_components(v, f32, 40), ops.mesh_keep_components(v, f64, 40)
    assert a[1].dtype == torch.int32 and b[1].dtype == torch.int64
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].long(), b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert torch.equal(ops.mesh_components(f32, nv)["labels"], ops.mesh_components(f64, nv)["labels"])
    wide = torch.zeros((len(f), 6), dtype=torch.int32, device=cuda)
    wide[:, ::2] = f32
    view = wide[:, ::2]
    assert not view.is_contiguous()
    c = ops.mesh_keep_components(v, view, 40)
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    assert torch.equal(ops.mesh_components(view, nv)["labels"], ops.mesh_components(f32, nv)["labels"])
    with pytest.raises(ops.SculptError):
        ops.mesh_components(f32.float(), nv)
    with pytest.raises(ops.SculptError):
        ops.mesh_keep_components(v[:, :2], f32, "largest")


def test_determinism_and_face_order(cuda):
    from sculptmate_amd import ops

    f, nv = _ccref.dust(seed=33)
    v, ft = torch.from_numpy(_vertices(nv)).to(cuda), torch.from_numpy(f).to(cuda)
    a, b = ops.mesh_components(ft, nv), ops.mesh_components(ft, nv)
    assert all(torch.equal(a[k], b[k]) for k in a)
    x, y = ops.mesh_keep_components(v, ft, 2), ops.mesh_keep_components(v, ft, 2)
    assert all(torch.equal(p, q) for p, q in zip(x, y))
    perm = torch.from_numpy(np.random.default_rng(34).permutation(len(f))).to(cuda)
    c = ops.mesh_components(ft[perm].contiguous(), nv)
    assert all(torch.equal(a[k], c[k]) for k in a)


@pytest.mark.parametrize("reference_order", [False, True])
def test_blobs_through_marching_cubes(cuda, reference_order):
    """The host test's volume through ops.marching_cubes: seven components, and "largest" is marching cubes of the large
    sphere's volume alone -- vertices bit for bit, faces equal, same order (the comparison the host test settled on)."""
    from sculptmate_amd import ops

    vol = torch.from_numpy(_ccref.blob_volume()).to(cuda)
    v, f = ops.marching_cubes(vol, 0.0, reference_order=reference_order)
    want = _check(cuda, _np(f), v.shape[0], keeps=("largest", 1, 0.05), v=_np(v))
    assert len(want["roots"]) == 7
    v1, f1 = ops.marching_cubes(torch.from_numpy(_ccref.blob_volume(_ccref.BLOBS[:1])).to(cuda), 0.0, reference_order=reference_order)
    v2, f2, _, _ = ops.mesh_keep_components(v, f, "largest")
    assert f2.dtype == f.dtype == (torch.int64 if reference_order else torch.int32)
    assert np.array_equal(_bits(v2), _bits(v1)) and torch.equal(f2, f1)


@pytest.fixture(scope="module")
def model(cuda):
    """The shared small model at resolution 64; the plain mesh carries colours and field normals."""
    return _tsrmodel.small_model(cuda, 64, enable_texture=True, normals="field")


def test_extract_meshes_keeps_the_rows_the_restatement_selects(model):
    m, plain, kw = model["m"], model["plain"], model["kw"]
    comp = _ccref.components(_np(plain.faces), plain.vertices.shape[0])
    print("unfiltered: %d vertices, %d faces, %d components, largest %d faces" % (
        plain.vertices.shape[0], plain.faces.shape[0], len(comp["roots"]), comp["face_counts"].max()))
    assert len(comp["roots"]) >= 2, "one component only: the comparison below would show nothing"
    for keep in ("largest", 0.5, 8):
        kept = m.extract_meshes(model["codes"], enable_texture=True, normals="field", keep_components=keep, **kw)[0]
        wv, wf, vi, fi = _ccref.keep_components(_np(plain.vertices), _np(plain.faces), keep)
        assert 0 < len(wf) < plain.faces.shape[0]
        assert np.array_equal(_bits(kept.vertices), wv.view(np.uint32)) and np.array_equal(_np(kept.faces), wf)
        assert kept.faces.dtype == plain.faces.dtype
        # colours and normals are functions of their vertex alone
        assert np.array_equal(_bits(kept.vertex_colors), _bits(plain.vertex_colors)[vi])
        assert np.array_equal(_bits(kept.vertex_normals), _bits(plain.vertex_normals)[vi])
        again = plain.keep_components(keep)   # Mesh.keep_components: the same rows, gathered
        assert torch.equal(again.vertices, kept.vertices) and torch.equal(again.faces, kept.faces)
        assert torch.equal(again.vertex_colors, kept.vertex_colors) and torch.equal(again.vertex_normals, kept.vertex_normals)


def test_baked_and_host_meshes_have_the_kept_sizes(model):
    m, plain, kw = model["m"], model["plain"], model["kw"]
    wv, wf, _, fi = _ccref.keep_components(_np(plain.vertices), _np(plain.faces), "largest")
    baked = m.extract_meshes(model["codes"], enable_texture=True, bake_texture=64, keep_components="largest", **kw)[0]
    assert tuple(baked.uvs.shape) == (3 * len(wf), 2) and tuple(baked.texture.shape) == (64, 64, 3)
    assert np.array_equal(_np(baked.faces), wf) and np.array_equal(_bits(baked.vertices), wv.view(np.uint32))
    full = m.extract_meshes(model["codes"], enable_texture=True, bake_texture=64, **kw)[0]
    cut = full.keep_components("largest")
    assert cut.texture is full.texture and torch.equal(cut.uvs.view(-1, 3, 2), full.uvs.view(-1, 3, 2)[torch.from_numpy(fi).to(full.uvs.device)])
    host = m.run([model["img"]], mc_resolution=64, threshold=model["threshold"], keep_components="largest")[0]
    assert isinstance(host.vertices, np.ndarray) and host.vertices.shape == wv.shape and host.faces.shape == wf.shape
    two = m.run([model["img"], model["img"]], mc_resolution=64, threshold=model["threshold"], keep_components="largest")
    assert [x.faces.shape for x in two] == [wf.shape, wf.shape] and np.array_equal(two[0].faces, two[1].faces)
    seen = []
    m.mesh_sink = lambda v, f, c, name: seen.append((v.shape, f.shape))
    try:
        m.extract_mesh(model["codes"], keep_components="largest", **kw)
    finally:
        m.mesh_sink = None
    assert seen == [(wv.shape, wf.shape)]


def test_none_launches_nothing_new_and_changes_nothing(model, monkeypatch):
    from sculptmate_amd import ops

    m, plain, kw = model["m"], model["plain"], model["kw"]

    def refuse(*a, **k):
        raise AssertionError("keep_components=None must not reach the component kernels")

    monkeypatch.setattr(ops, "mesh_keep_components", refuse)
    monkeypatch.setattr(ops, "_cc_launch", refuse)
    for extra in ({}, {"keep_components": None}):
        again = m.extract_meshes(model["codes"], enable_texture=True, normals="field", **kw, **extra)[0]
        assert np.array_equal(_bits(again.vertices), _bits(plain.vertices)) and torch.equal(again.faces, plain.faces)
        assert np.array_equal(_bits(again.vertex_colors), _bits(plain.vertex_colors))
        assert np.array_equal(_bits(again.vertex_normals), _bits(plain.vertex_normals))
    host = m.run([model["img"]], mc_resolution=64, threshold=model["threshold"])[0]
    assert host.vertices.shape == tuple(plain.vertices.shape) and np.array_equal(host.faces, _np(plain.faces))
