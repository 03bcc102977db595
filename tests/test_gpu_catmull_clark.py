"""Catmull-Clark subdivision on the device (csrc/mesh_catmull.hip, ops.mesh_catmull_clark) against its NumPy restatement
(tests/_catmullref.py): positions, quads, triangles and attributes BIT FOR BIT, no tolerance -- the kernel is compiled without
contraction and computes every component in fp64 in the restatement's order.  Then the contract of the call, the refusals and
the scheme's way through Mesh.subdivide and TSR.extract_meshes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _catmullref as cc
import _tsrmodel

pytestmark = pytest.mark.gpu


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _dev(cuda, *arrays):
    return tuple(None if a is None else torch.from_numpy(np.array(a)).to(cuda) for a in arrays)   # (a copy: a shared case is read-only)


def _same_bits(got, want, what):
    """got: the device's (vertices, quads, triangles, attributes); want: the restatement's."""
    for g, w, name in zip(got, want, ("vertices", "quads", "triangles", "attributes")):
        if w is None:
            assert g is None, (what, name)
            continue
        g = _np(g)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if w.dtype == np.float32:
            assert g.dtype == np.float32
            bad = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(len(g), -1).any(1))[0]
        else:
            bad = np.nonzero((g.astype(np.int64) != w.astype(np.int64)).any(1))[0]
        assert len(bad) == 0, "%s: %d of %d %s rows differ, first %d: %r != %r" % (what, len(bad), len(g), name, bad[0], g[bad[0]], w[bad[0]])


MESHES = {"cube": cc.cube, "tetrahedron": cc.tetrahedron, "single_quad": cc.single_quad, "grid": cc.quad_grid,
          "cubes_sharing_an_edge": cc.two_cubes_sharing_an_edge, "cubes_sharing_a_vertex": cc.two_cubes_sharing_a_vertex,
          "fan70": cc.closed_fan, "valence_two": cc.strip_with_valence_two, "opposite_pair": lambda: cc.wound_pair(True)}
CHANNELS = {1: 3, 2: 1, 3: 8}   # attributes per level tested: C = 3, 1 and 8


@functools.lru_cache(maxsize=None)
def _case(name, levels):
    """(P, F, A, the restatement's result) of a hand mesh; computed once and never modified."""
    P, F = MESHES[name]()
    A = np.random.default_rng(len(P) + levels).random((len(P), CHANNELS[levels])).astype(np.float32)
    want = cc.subdivide(P, F, levels, A)
    for x in (P, F, A) + want:
        x.setflags(write=False)
    return P, F, A, want


@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(MESHES))
def test_hand_meshes_bit_for_bit(cuda, name, levels):
    from sculptmate_amd import ops

    P, F, A, want = _case(name, levels)
    v, f, a = _dev(cuda, P, F, A)
    f = f.long() if levels == 2 else f                                   # int64 faces at level 2, int32 at 1 and 3
    keep = (v.clone(), f.clone(), a.clone())
    got = ops.mesh_catmull_clark(v, f, levels, attributes=a)
    _same_bits(got, want, "%s x %d" % (name, levels))
    assert got[1].dtype == f.dtype and got[2].dtype == f.dtype
    assert torch.equal(v, keep[0]) and torch.equal(f, keep[1]) and torch.equal(a, keep[2])   # the inputs are untouched
    again = ops.mesh_catmull_clark(v, f, levels, attributes=a)
    assert all(torch.equal(x, y) for x, y in zip(got, again))           # two calls give the same bits
    _same_bits(ops.mesh_catmull_clark(v, f, levels)[:3] + (None,), want[:3] + (None,), "%s x %d, no attributes" % (name, levels))
    if levels > 1:                                                      # level n equals n single levels
        step = (v, f, None, a)
        for _ in range(levels):
            step = ops.mesh_catmull_clark(step[0], step[1], 1, attributes=step[3])
        assert all(torch.equal(x, y) for x, y in zip(got, step))


def _sphere_volume():
    g = np.mgrid[0:32, 0:32, 0:32].astype(np.float64)
    d = np.sqrt((g[0] - 15.3) ** 2 + (g[1] - 15.7) ** 2 + (g[2] - 16.1) ** 2)
    return (10.2 - d).astype(np.float32)


def _noise_volume():
    return np.random.default_rng(1016).standard_normal((16, 16, 16)).astype(np.float32)


@pytest.mark.parametrize("volume", [_sphere_volume, _noise_volume], ids=["sphere32", "noise16"])
def test_surface_nets_lattices_two_levels_bit_for_bit(cuda, volume):
    """The quads of ops.surface_nets: a closed manifold (the sphere), and box borders and non-manifold edges (the noise)."""
    from sculptmate_amd import ops

    v, q, t = ops.surface_nets(torch.from_numpy(volume()).to(cuda), 0.0, vert_div=31.0, vert_mul=2.0, vert_add=-1.0)
    P, Q = _np(v), _np(q)
    T = cc.Topology(Q, len(P))
    if volume is _noise_volume:
        assert (T.count == 1).any() and (T.count >= 3).any()             # the case is what it is meant to be
    else:
        assert (T.count == 2).all()
    A = np.random.default_rng(7).random((len(P), 3)).astype(np.float32)
    want = cc.subdivide(P, Q, 2, A)
    got = ops.mesh_catmull_clark(v, q, 2, attributes=torch.from_numpy(A).to(cuda))
    _same_bits(got, want, volume.__name__)
    assert len(got[1]) == 16 * len(Q)
    # and from the extractor's triangles: k = 3 on a large mesh, one level
    _same_bits(ops.mesh_catmull_clark(v, t, 1), cc.subdivide(P, _np(t), 1), volume.__name__ + " triangles")


def test_mesh_subdivide_returns_the_triangles(cuda):
    from sculptmate_amd import ops

    P, F = cc.tetrahedron()
    v, f = _dev(cuda, P, F)
    a = torch.rand((4, 2), device=cuda)
    gv, gt, ga = ops.mesh_subdivide(v, f, (2, "catmull_clark"), attributes=a)
    wv, wq, wt, wa = ops.mesh_catmull_clark(v, f, 2, attributes=a)
    assert torch.equal(gv, wv) and torch.equal(gt, wt) and torch.equal(ga, wa) and len(gt) == 2 * 3 * 4 * 4
    lv, lf, _ = ops.mesh_subdivide(v, f, 2)                               # the Loop result is what it was
    import _loopref

    LV, LF, _ = _loopref.subdivide(P, F, 2)
    assert np.array_equal(_np(lv).view(np.uint32), LV.view(np.uint32)) and np.array_equal(_np(lf), LF)


def test_no_faces_gives_copies(cuda):
    from sculptmate_amd import ops

    v = torch.rand((5, 3), device=cuda)
    a = torch.rand((5, 2), device=cuda)
    for k, dtype in ((3, torch.int32), (4, torch.int64)):
        gv, gq, gt, ga = ops.mesh_catmull_clark(v, torch.zeros((0, k), dtype=dtype, device=cuda), 3, attributes=a)
        assert torch.equal(gv, v) and gv.data_ptr() != v.data_ptr() and torch.equal(ga, a) and ga.data_ptr() != a.data_ptr()
        assert gq.shape == (0, 4) and gt.shape == (0, 3) and gq.dtype == dtype and gt.dtype == dtype


def test_refusals(cuda):
    from sculptmate_amd import ops

    P, F = cc.cube()
    v, f = _dev(cuda, P, F)
    E = ops.SculptError
    with pytest.raises(E):
        ops.mesh_catmull_clark(v.cpu(), f, 1)
    with pytest.raises(E):
        ops.mesh_catmull_clark(v, f.cpu(), 1)
    with pytest.raises(E):
        ops.mesh_catmull_clark(v, f, 1, attributes=torch.zeros((8, 3)))
    for bad in (8, -1):
        g = f.clone()
        g[2, 1] = bad
        with pytest.raises(E, match="out of range"):
            ops.mesh_catmull_clark(v, g, 1)
        with pytest.raises(E, match="out of range"):
            ops.mesh_catmull_clark(v, g[:, :3].contiguous(), 1)
    g = f.long()
    g[0, 0] = (1 << 32) + 1                                               # would wrap into range as int32
    with pytest.raises(E, match="out of range"):
        ops.mesh_catmull_clark(v, g, 1)
    for k in (3, 4):
        g = f[:, :k].clone()
        g[3, k - 1] = g[3, 0]
        with pytest.raises(E, match="repeated"):
            ops.mesh_catmull_clark(v, g, 1)
    g = f.clone()
    g[1, 3] = g[1, 1]                                                     # opposite corners of a quad
    with pytest.raises(E, match="repeated"):
        ops.mesh_catmull_clark(v, g, 1)
    for bad in (float("nan"), float("inf")):
        w = v.clone()
        w[5, 1] = bad
        with pytest.raises(E, match="non-finite"):
            ops.mesh_catmull_clark(w, f, 1)
    for faces in (torch.zeros((2, 5), dtype=torch.int32, device=cuda), torch.zeros((2, 2), dtype=torch.int32, device=cuda),
                  torch.zeros(8, dtype=torch.int32, device=cuda), f.float(), f.to(torch.int16)):
        with pytest.raises(E, match="faces"):
            ops.mesh_catmull_clark(v, faces, 1)
    with pytest.raises(E, match="vertices"):
        ops.mesh_catmull_clark(v[:, :2], f, 1)
    for attributes in (torch.zeros((7, 3), device=cuda), torch.zeros((8, 9), device=cuda), torch.zeros((8, 0), device=cuda),
                       torch.zeros(8, device=cuda), torch.zeros((8, 3), dtype=torch.int32, device=cuda)):
        with pytest.raises(E, match="attributes"):
            ops.mesh_catmull_clark(v, f, 1, attributes=attributes)
    for levels in (0, 7, True, 2.0):
        with pytest.raises(E, match="levels"):
            ops.mesh_catmull_clark(v, f, levels)
    # a level whose 4 x quads would leave int32: 2^17 quads x 4^5 x 4 = 2^31 index entries at the sixth level -- refused before
    # any level runs
    n = 1 << 17
    i = 2 * torch.arange(n, dtype=torch.int32, device=cuda)
    strip = torch.stack([i, i + 2, i + 3, i + 1], 1)
    pts = torch.rand((2 * n + 2, 3), device=cuda)
    with pytest.raises(E, match="int32"):
        ops.mesh_catmull_clark(pts, strip, 6)
    assert len(ops.mesh_catmull_clark(pts, strip, 1)[1]) == 4 * n         # the mesh itself is fine


def test_entry_points_exist_and_refuse_bad_arguments(cuda):
    from sculptmate_amd import _lib

    lib = _lib.lib
    for name in ("sculpt_catmull_validate", "sculpt_catmull_halfedge_keys", "sculpt_catmull_first_halfedge", "sculpt_catmull_classify",
                 "sculpt_catmull_refine"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    F = torch.tensor([[0, 1, 2, 3]], dtype=torch.int32, device=cuda)
    keys = torch.empty(4, dtype=torch.int64, device=cuda)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    assert lib.sculpt_catmull_halfedge_keys(p(F), 1, 5, p(keys), s) != 0 and "corners" in _lib.last_error()
    assert lib.sculpt_catmull_halfedge_keys(None, 1, 4, p(keys), s) != 0
    assert lib.sculpt_catmull_halfedge_keys(p(F), 1, 4, p(keys), s) == 0
    torch.cuda.synchronize()
    assert keys.tolist() == [(0 << 32) | 1, (1 << 32) | 2, (2 << 32) | 3, (0 << 32) | 3]
    assert lib.sculpt_catmull_validate(None, 4, p(F), 1, 4, None, s) != 0
    assert lib.sculpt_catmull_classify(None, None, None, None, s) != 0 and "null topology" in _lib.last_error()
    assert lib.sculpt_catmull_refine(None, None, None, None, None, 0, None, None, None, None, s) != 0
    bad = _lib.CatmullTopo(0, 0, 0, 0, 0, 0, 0, 1, 4, 4, 5)
    assert lib.sculpt_catmull_first_halfedge(ctypes.c_void_p(ctypes.addressof(bad)), None, s) != 0 and "corners" in _lib.last_error()
    null = _lib.CatmullTopo(0, 0, 0, 0, 0, 0, 0, 1, 4, 4, 4)
    assert lib.sculpt_catmull_classify(ctypes.c_void_p(ctypes.addressof(null)), None, None, None, s) != 0


def test_mesh_subdivide_method(cuda):
    from sculptmate_amd.tsr.system import Mesh

    P, Q = cc.quad_grid(3)
    T = cc.split(P, Q)
    v, q, t = _dev(cuda, P, Q, T)
    col = torch.rand((len(P), 3), device=cuda)
    m = Mesh(v, t, col, vertex_normals=torch.rand((len(P), 3), device=cuda))
    m.quads = q
    got = m.subdivide((2, "catmull_clark"))
    _same_bits((got.vertices, got.quads, got.faces, got.vertex_colors), cc.subdivide(P, Q, 2, _np(col)), "Mesh.subdivide on quads")
    assert got.vertex_normals is None and m.quads is q
    got = Mesh(v, t).subdivide((1, "catmull_clark"))
    _same_bits((got.vertices, got.quads, got.faces, None), cc.subdivide(P, T, 1), "Mesh.subdivide on triangles")
    assert m.subdivide(1).quads is None and m.subdivide((1, "midpoint")).quads is None


@pytest.fixture(scope="module")
def model(cuda):
    """tests/_tsrmodel.py's small model at 32^3."""
    return _tsrmodel.small_model(cuda, 32)


def test_extract_meshes_refines_the_surface_nets_quads(cuda, model):
    m, codes, kw = model["m"], model["codes"], model["kw"]
    base = m.extract_meshes(codes, isosurface="surface_nets", **kw)[0]
    rule = (1, "catmull_clark")
    plain = m.extract_meshes(codes, isosurface="surface_nets", subdivide=rule, **kw)[0]
    want = cc.subdivide(_np(base.vertices), _np(base.quads), 1)
    _same_bits((plain.vertices, plain.quads, plain.faces, None), want, "extract_meshes")
    assert plain.quads.dtype == base.quads.dtype and plain.faces.dtype == base.faces.dtype
    got = m.extract_meshes(codes, isosurface="surface_nets", subdivide=rule, project=True, **kw)[0]
    assert got.quads is not None and len(got.quads) == 4 * len(base.quads) and len(got.faces) == 2 * len(got.quads)
    # the faces are the quads' split (taken on the refined positions, before project moved them), the quads survive project
    assert torch.equal(got.quads, plain.quads) and torch.equal(got.faces, plain.faces)
    assert np.array_equal(_np(got.faces), cc.split(_np(plain.vertices), _np(got.quads)))
    assert got.vertices.shape == plain.vertices.shape and not torch.equal(got.vertices, plain.vertices)
    assert torch.isfinite(got.vertices).all()
    with_normals = m.extract_meshes(codes, isosurface="surface_nets", subdivide=rule, normals="faces", **kw)[0]
    assert with_normals.vertex_normals.shape == plain.vertices.shape                 # normals= sees the final mesh


def test_extract_meshes_turns_simplified_triangles_into_quads(cuda, model):
    m, codes, kw = model["m"], model["codes"], model["kw"]
    low = m.extract_meshes(codes, simplify=0.5, **kw)[0]
    got = m.extract_meshes(codes, simplify=0.5, subdivide=(1, "catmull_clark"), **kw)[0]
    assert low.quads is None and len(got.quads) == 3 * len(low.faces) and len(got.faces) == 6 * len(low.faces)
    _same_bits((got.vertices, got.quads, got.faces, None), cc.subdivide(_np(low.vertices), _np(low.faces), 1), "simplify + catmull_clark")
