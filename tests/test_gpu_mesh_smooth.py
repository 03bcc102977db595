"""ops.mesh_smooth (csrc/mesh_smooth.hip, sf3d/remesh_device.py smooth_device) and the layers above it on the GPU.  The kernels
run without floating-point contraction and tests/_smoothref.py keeps their order of operations, so positions are compared as
bits; the neighbour table and the fixed flags are compared entry for entry; then the contract of the call, Mesh.smooth and the
`smooth` keyword through the model.  What the restatement itself is worth is shown in tests/test_mesh_smooth_host.py."""
import numpy as np
import pytest
import torch

import _smoothref as ref
import _tsrmodel
from sculptmate_amd import synth

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _dev(cuda, P, F):
    return torch.from_numpy(np.ascontiguousarray(P)).to(cuda), torch.from_numpy(np.ascontiguousarray(F)).to(cuda)


def _equal_bits(cuda, P, F, rule):
    """ops.mesh_smooth against the float32 restatement -> the result on the host."""
    from sculptmate_amd import ops

    v, f = _dev(cuda, P, F)
    got = ops.mesh_smooth(v, f, rule)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(v.shape) and got.data_ptr() != v.data_ptr()
    want = ref.taubin(P, F, *ops.smooth_rule(rule))
    bad = np.nonzero((_bits(got) != _bits(want)).any(1))[0]
    assert len(bad) == 0, "vertices %s differ: %s against %s" % (bad[:5], _np(got)[bad[:5]], want[bad[:5]])
    return _np(got)


MESHES = {
    "tetrahedron": ref.tetrahedron,                       # degree 3, the smallest closed mesh
    "octahedron": ref.octahedron,
    "patch": ref.grid_patch,                              # open: the border is fixed
    "cone70": lambda: ref.double_cone(70),                # 70 neighbours: past any unroll width and the wave size
    "cone255": lambda: ref.double_cone(255),              # 257 vertices: one past a 256-thread workgroup
    "two_and_orphan": ref.two_components_and_an_orphan,
    "three_face_edge": ref.three_face_edge,
}


@pytest.mark.parametrize("rule", [10, (3, 0.6, -0.7), (4, 0.5, 0)], ids=repr)
@pytest.mark.parametrize("name", sorted(MESHES))
def test_hand_meshes_bit_for_bit(cuda, name, rule):
    P, F = MESHES[name]()
    Q = _equal_bits(cuda, P, F, rule)
    moved = (Q.view(np.uint32) != P.view(np.uint32)).any(1)
    if name == "patch":
        assert np.array_equal(moved, ~ref.patch_border())           # boundary bits unchanged, the interior moved
    elif name == "two_and_orphan":
        assert not moved[ref.ORPHAN] and np.delete(moved, ref.ORPHAN).all()
    elif name == "three_face_edge":
        assert moved.tolist() == [False, True, False, True, True, True, False]
    else:
        assert moved.all()                                           # the 70- and 255-neighbour apexes are NOT treated as fixed
    if name == "cone255":
        assert len(P) == 257


@pytest.fixture(scope="module")
def sphere():
    return ref.noisy_icosphere(4, 0.01, 0)


@pytest.mark.parametrize("rule", [10, (3, 0.6, -0.7), (4, 0.5, 0)], ids=repr)
def test_noisy_icosphere_bit_for_bit(cuda, sphere, rule):
    P, F = sphere
    assert P.shape == (2562, 3)
    Q = _equal_bits(cuda, P, F, rule)
    if rule == 10:
        assert ref.radius_rms(Q) <= 0.5 * ref.radius_rms(P)
        assert abs(ref.signed_volume(Q, F) / ref.signed_volume(P, F) - 1) <= 0.01


# --------------------------------------------------------------------------------------------------- through the model
@pytest.fixture(scope="module")
def model(cuda):
    """The shared small model at resolution 64; the plain mesh carries colours and field normals."""
    return _tsrmodel.small_model(cuda, 64, enable_texture=True, normals="field")


def test_marching_cubes_mesh_of_a_synthetic_field_bit_for_bit(cuda, model):
    """The 32^3 density field of the synthetic model through ops.marching_cubes: lattice-ordered vertices, open where the surface
    leaves the grid (those vertices are fixed), thousands of rows of mixed degree."""
    from sculptmate_amd import ops

    vol = ops.density_grid(model["codes"][0].contiguous(), model["m"].decoder, 32)
    v, f = ops.marching_cubes((vol - vol.median()).view(32, 32, 32).contiguous(), 0.0)
    P, F = _np(v), _np(f)
    assert len(F) > 1000
    Q = _equal_bits(cuda, P, F, 5)
    fixed = ref.fixed_flags(F, len(P)).astype(bool)
    assert np.array_equal(Q[fixed].view(np.uint32), P[fixed].view(np.uint32)) and (Q != P).any(1).sum() > len(P) // 2


# ------------------------------------------------------------------------------------------ neighbour table, fixed flags
@pytest.mark.parametrize("name", ["patch", "cone70", "three_face_edge", "two_and_orphan"])
def test_neighbour_table_and_fixed_flags(cuda, name):
    """The two table kernels on sentinel-filled outputs (an unwritten slot shows), then the driver's table."""
    from sculptmate_amd._lib import check, lib
    from sculptmate_amd.sf3d import remesh_device as rd

    P, F = MESHES[name]()
    nv = len(P)
    start, nb = ref.neighbour_table(F, nv)
    ctx = rd._Ctx()
    Fd = torch.from_numpy(F).to(cuda)
    T = rd._Topo(ctx, Fd, nv, carry=torch.zeros(nv, dtype=torch.uint8, device=cuda))
    assert 2 * T.ne == len(nb)
    keys = torch.full((2 * T.ne + 2,), -7, dtype=torch.int64, device=cuda)
    check(lib.sculpt_smooth_edge_keys(T.ref(), rd._p(keys), ctx.stream))
    k = _np(keys)
    assert k[-2:].tolist() == [-7, -7]                                 # nothing past 2 ne
    rows = np.repeat(np.arange(nv), np.diff(start)).astype(np.int64)
    want = (rows << 32) | nb.astype(np.int64)
    assert np.array_equal(np.sort(k[:-2]), want)
    pairs = k[:-2].reshape(-1, 2)
    assert np.array_equal(pairs[:, 0] >> 32, pairs[:, 1] & 0xFFFFFFFF) and ((pairs[:, 0] >> 32) < (pairs[:, 0] & 0xFFFFFFFF)).all()
    out = torch.full((2 * T.ne + 2,), -9, dtype=torch.int32, device=cuda)
    skeys = torch.from_numpy(want).to(cuda)
    check(lib.sculpt_smooth_neighbours(rd._p(skeys), 2 * T.ne, rd._p(out), ctx.stream))
    assert np.array_equal(_np(out)[:-2], nb) and _np(out)[-2:].tolist() == [-9, -9]
    s, n, fixed = rd._smooth_table(rd._Ctx(), Fd, nv)
    assert s.dtype == n.dtype == torch.int32 and fixed.dtype == torch.uint8
    assert np.array_equal(_np(s), start) and np.array_equal(_np(n), nb) and np.array_equal(_np(fixed), ref.fixed_flags(F, nv))


def test_entry_points_refuse_bad_arguments(cuda):
    """Error codes with a message, nothing launched."""
    from sculptmate_amd import _lib
    from sculptmate_amd.sf3d import remesh_device as rd

    lib = _lib.lib
    P, F = ref.octahedron()
    v, f = _dev(cuda, P, F)
    ctx = rd._Ctx()
    start, nb, fixed = rd._smooth_table(ctx, f, 6)
    work = torch.zeros((2, 6, 4), dtype=torch.float32, device=cuda)
    out = torch.full((6, 3), 7.0, dtype=torch.float32, device=cuda)
    p = rd._p

    def call(**kw):
        a = dict(start=p(start), nb=p(nb), fixed=p(fixed), nv=6, n_nb=nb.shape[0], P=p(v), n=2, lam=0.5, mu=-0.53, a=p(work[0]),
                 b=p(work[1]), out=p(out))
        a.update(kw)
        return lib.sculpt_smooth_taubin(a["start"], a["nb"], a["fixed"], a["nv"], a["n_nb"], a["P"], a["n"], a["lam"], a["mu"], a["a"],
                                        a["b"], a["out"], ctx.stream)

    for bad, word in ((dict(n=0), "iterations"), (dict(n=1001), "iterations"), (dict(lam=0.0), "lambda"), (dict(lam=float("nan")), "lambda"),
                      (dict(mu=-0.4), "mu"), (dict(mu=float("nan")), "mu"), (dict(mu=0.3), "mu"), (dict(nv=-1), "out of range"),
                      (dict(start=None), "null"), (dict(nb=None), "null"), (dict(fixed=None), "null"), (dict(P=None), "null"),
                      (dict(out=None), "null"), (dict(a=None), "null"), (dict(b=p(work[0])), "distinct"),
                      (dict(a=work.data_ptr() + 4), "aligned")):
        assert call(**bad) != 0 and word in _lib.last_error(), (bad, _lib.last_error())
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert lib.sculpt_smooth_edge_keys(None, p(work), ctx.stream) != 0 and "null topology" in _lib.last_error()
    assert lib.sculpt_smooth_neighbours(None, 4, p(work), ctx.stream) != 0 and "null" in _lib.last_error()
    assert lib.sculpt_smooth_neighbours(p(work), -1, p(work), ctx.stream) != 0 and "out of range" in _lib.last_error()
    assert call(nv=0) == 0 and call() == 0                             # and the good call still works
    assert np.array_equal(_bits(out), _bits(ref.taubin(P, F, 2)))


# ---------------------------------------------------------------------------------------------------------- the contract
def test_contract_of_the_call(cuda, sphere):
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d import remesh_device as rd

    P, F = sphere
    v, f = _dev(cuda, P, F)
    v0, f0 = v.clone(), f.clone()
    a = ops.mesh_smooth(v, f, 10)
    stats = rd.last_stats()
    assert stats["passes"] == 1 and stats["readbacks"] == 1 and stats["smooth_iterations"] == 10   # one topology, its one read
    assert torch.equal(v, v0) and torch.equal(f, f0)                   # inputs unchanged
    b = ops.mesh_smooth(v, f, 10)
    assert np.array_equal(_bits(a), _bits(b)) and a.data_ptr() != b.data_ptr()      # two calls, the same bits
    c = ops.mesh_smooth(v, f.long(), 10)                               # int64 faces
    assert np.array_equal(_bits(a), _bits(c))
    P64 = P.astype(np.float64) + 1e-9                                  # float64 vertices: rounded once to float32
    d = ops.mesh_smooth(torch.from_numpy(P64).to(cuda), f, 10)
    assert d.dtype == torch.float32 and np.array_equal(_bits(d), _bits(ref.taubin(P64.astype(np.float32), F, 10)))
    e = ops.mesh_smooth(v, f[:0], 3)                                   # no faces: a copy
    assert torch.equal(e, v) and e.data_ptr() != v.data_ptr()
    none = ops.mesh_smooth(v[:0], f[:0], 3)
    assert tuple(none.shape) == (0, 3)


def test_refusals(cuda):
    """Refused on the host side of the call (remesh_device._inputs): nothing that could fault is launched."""
    from sculptmate_amd import ops

    P, F = ref.octahedron()
    v, f = _dev(cuda, P, F)
    bad = f.clone()
    bad[3, 1] = 6
    with pytest.raises(ops.SculptError, match="out of range"):
        ops.mesh_smooth(v, bad, 3)
    bad[3, 1] = -1
    with pytest.raises(ops.SculptError, match="out of range"):
        ops.mesh_smooth(v, bad, 3)
    bad[3, 1] = bad[3, 0]
    with pytest.raises(ops.SculptError, match="repeated"):
        ops.mesh_smooth(v, bad, 3)
    nan = v.clone()
    nan[2, 1] = float("nan")
    with pytest.raises(ops.SculptError, match="non-finite"):
        ops.mesh_smooth(nan, f, 3)
    for vv, ff in ((v[:, :2], f), (v, f[:, :2]), (v.long(), f), (v, f.float()), (v, f.to(torch.int16))):
        with pytest.raises(ops.SculptError):
            ops.mesh_smooth(vv, ff, 3)
    with pytest.raises(ValueError):
        ops.mesh_smooth(v, f, 0.5)
    assert np.array_equal(_bits(ops.mesh_smooth(v, f, 3)), _bits(ref.taubin(P, F, 3)))   # and the good call still works


def test_mesh_smooth_method(cuda):
    from sculptmate_amd.tsr.system import Mesh

    P, F = ref.grid_patch()
    v, f = _dev(cuda, P, F)
    col, nrm = torch.rand((25, 3), device=cuda), torch.rand((25, 3), device=cuda)
    uvs, tex = torch.rand((3 * len(F), 2), device=cuda), torch.rand((4, 4, 3), device=cuda)
    got = Mesh(v, f, col, uvs=uvs, texture=tex, vertex_normals=nrm).smooth((3, 0.6, -0.7))
    assert np.array_equal(_bits(got.vertices), _bits(ref.taubin(P, F, 3, 0.6, -0.7)))
    assert got.faces is f and got.vertex_colors is col and got.uvs is uvs and got.texture is tex
    assert got.vertex_normals is None
    plain = Mesh(v, f).smooth(2)
    assert plain.vertex_colors is None and plain.uvs is None and plain.vertex_normals is None


def test_none_launches_nothing_new_and_changes_nothing(model, monkeypatch):
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d import remesh_device as rd

    m, plain, kw = model["m"], model["plain"], model["kw"]

    def refuse(*a, **k):
        raise AssertionError("smooth=None must not reach the smoother")

    monkeypatch.setattr(ops, "mesh_smooth", refuse)
    monkeypatch.setattr(ops, "smooth_rule", refuse)
    monkeypatch.setattr(rd, "smooth_device", refuse)
    for name in ("sculpt_smooth_edge_keys", "sculpt_smooth_neighbours", "sculpt_smooth_taubin"):
        monkeypatch.setattr(rd.lib, name, refuse)
    for extra in ({}, {"smooth": None}):
        again = m.extract_meshes(model["codes"], enable_texture=True, normals="field", **kw, **extra)[0]
        assert np.array_equal(_bits(again.vertices), _bits(plain.vertices)) and torch.equal(again.faces, plain.faces)
        assert np.array_equal(_bits(again.vertex_colors), _bits(plain.vertex_colors))
        assert np.array_equal(_bits(again.vertex_normals), _bits(plain.vertex_normals))


def test_extract_meshes_is_the_calls_in_order(model):
    """marching cubes -> keep_components -> smooth -> simplify, then colours and normals at the final vertices."""
    from sculptmate_amd import ops

    m, plain, kw = model["m"], model["plain"], model["kw"]
    kv, kf = ops.mesh_keep_components(plain.vertices, plain.faces, "largest")[:2]
    mv = ops.mesh_smooth(kv, kf, 5)
    assert not torch.equal(mv, kv)
    sv, sf, _ = ops.mesh_simplify(mv, kf, 0.5)
    assert 0 < sf.shape[0] <= kf.shape[0] // 2
    got = m.extract_meshes(model["codes"], keep_components="largest", smooth=5, simplify=0.5, **kw)[0]
    assert np.array_equal(_bits(got.vertices), _bits(sv)) and torch.equal(got.faces, sf) and got.faces.dtype == plain.faces.dtype
    assert got.vertex_colors is None and got.vertex_normals is None
    only = m.extract_meshes(model["codes"], keep_components="largest", smooth=5, **kw)[0]      # smoothing alone: the same faces
    assert np.array_equal(_bits(only.vertices), _bits(mv)) and torch.equal(only.faces, kf)
    full = m.extract_meshes(model["codes"], enable_texture=True, normals="field", keep_components="largest", smooth=5, simplify=0.5,
                            **kw)[0]
    assert np.array_equal(_bits(full.vertices), _bits(sv)) and torch.equal(full.faces, sf)
    planes = model["codes"][0].contiguous()
    color = m.renderer.query_triplane(m.decoder, sv, planes)["color"]
    assert np.array_equal(_bits(full.vertex_colors), _bits(color))                       # evaluated at the returned vertices
    assert np.array_equal(_bits(full.vertex_normals), _bits(m.field_normals(sv, planes)))
    again = plain.keep_components("largest").smooth(5)                                    # Mesh.smooth: the same geometry
    assert np.array_equal(_bits(again.vertices), _bits(mv)) and again.vertex_normals is None
    assert tuple(again.vertex_colors.shape) == tuple(mv.shape)
    host = m.run([model["img"]], mc_resolution=64, threshold=model["threshold"], keep_components="largest", smooth=5)[0]
    assert isinstance(host.vertices, np.ndarray) and host.vertices.shape == tuple(mv.shape) and np.array_equal(host.faces, _np(kf))


def test_generator_attribute_reaches_extract_mesh(cuda, tmp_path):
    import types

    from test_host_logic import _write_checkpoint

    from sculptmate_amd import ops
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr.spec import SMALL_CFG

    _write_checkpoint(str(tmp_path), SMALL_CFG, seed=61)
    g = TripoGenerator(cuda)
    assert g.smooth is None
    g.checkpoint_dir = str(tmp_path)
    g.mc_resolution = 32
    assert g.initiate_model() == 0
    g.model.mesh_sink = lambda v, f, c, name: None
    orig, seen = g.model.extract_mesh, []

    def reachable(self, codes, **kw):   # random weights never reach the default threshold: take the grid's median
        seen.append(kw["smooth"])
        return orig(codes, **dict(kw, threshold=float(ops.density_grid(codes[0].contiguous(), self.decoder, kw["resolution"]).median())))

    g.model.extract_mesh = types.MethodType(reachable, g.model)
    img = (synth.composite_rgb(synth.image_rgba(seed=62, size=SMALL_CFG["cond_image_size"])) * 255).astype(np.uint8)
    assert g.generate_mesh(img, "plain") == 0
    plain = g.last_meshes[0]
    g.smooth = 5
    assert g.generate_mesh(img, "smoothed") == 0
    mesh = g.last_meshes[0]
    assert seen == [None, 5] and torch.equal(mesh.faces, plain.faces)
    assert np.array_equal(_bits(mesh.vertices), _bits(ops.mesh_smooth(plain.vertices, plain.faces, 5)))
