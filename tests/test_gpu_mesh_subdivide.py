"""ops.mesh_subdivide (csrc/mesh_subdivide.hip, sf3d/remesh_device.py loop_subdivide_device) and the layers above it on the GPU.
The kernels compute every value in fp64 without contraction in the order tests/_loopref.py keeps, and round once: positions,
faces and attributes are compared as bits.  The one tolerance in this file is the one-ulp bound of the face-permutation test,
where only the order of an fp64 sum moves.  What the restatement itself is worth is shown in tests/test_mesh_subdivide_host.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _loopref as ref
import _tsrmodel
from sculptmate_amd import synth

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _dev(cuda, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays)


def _same_bits(got, want, what):
    assert tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    bad = np.nonzero((_bits(got) != _bits(want)).reshape(len(want), -1).any(1))[0]
    assert len(bad) == 0, "%s: rows %s differ: %s against %s" % (what, bad[:5], _np(got)[bad[:5]], want[bad[:5]])


MESHES = {
    "tetrahedron": ref.tetrahedron,                         # valence 3: the beta = 3/16 branch
    "octahedron": ref.octahedron,
    "icosphere": lambda: (ref.icosphere(1)[0].astype(np.float32), ref.icosphere(1)[1]),   # valences 5 and 6
    "patch": ref.grid_patch,                                # open: crease and corner rules
    "cone70": lambda: ref.double_cone(70),                  # valence above 64: the interior rule, not the bnd feature flag
    "cone255": lambda: ref.double_cone(255),                # 257 vertices: one past a 256-thread workgroup
    "two_and_orphan": ref.two_components_and_an_orphan,
    "three_face_edge": ref.three_face_edge,
    "two_tetrahedra": ref.two_tetrahedra_sharing_a_vertex,
}


@functools.lru_cache(maxsize=None)
def _case(name, levels):
    """(P, F, A, the restatement's (P', F', A')) of a hand mesh, computed once and never modified."""
    P, F = MESHES[name]()
    A = np.random.default_rng(len(P)).random((len(P), 3)).astype(np.float32)
    return P, F, A, ref.subdivide(P, F, levels, A)


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("name", sorted(MESHES))
def test_hand_meshes_bit_for_bit(cuda, name, levels):
    from sculptmate_amd import ops

    P, F, A, (Q, G, B) = _case(name, levels)
    v, f, a = _dev(cuda, P, F, A)
    gv, gf, ga = ops.mesh_subdivide(v, f, levels, attributes=a)
    assert gv.dtype == ga.dtype == torch.float32 and gf.dtype == f.dtype
    assert np.array_equal(_np(gf), G)
    _same_bits(gv, Q, "positions")
    _same_bits(ga, B, "attributes")
    if levels == 1:
        moved = (_bits(gv)[:len(P)] != _bits(P)).any(1)
        if name == "cone70" or name == "cone255":
            assert moved[:2].all() and len(P) == int(name[4:]) + 2           # the apexes are NOT treated as features
        elif name == "two_and_orphan":
            assert not moved[ref.ORPHAN] and np.delete(moved, ref.ORPHAN).all()
        elif name == "three_face_edge":
            assert moved.tolist() == [False, True, False, True, True, True, True]
        elif name == "two_tetrahedra":
            assert moved.all()                                                   # vertex 0, fan 6 in two umbrellas, included


# --------------------------------------------------------------------------------------------------- through the model
@pytest.fixture(scope="module")
def model(cuda):
    """The shared small model at resolution 32; the plain mesh carries colours and field normals."""
    return _tsrmodel.small_model(cuda, 32, enable_texture=True, normals="field")


def test_marching_cubes_mesh_of_a_synthetic_field_bit_for_bit(cuda, model):
    """One level on the 32^3 density field of the synthetic model through ops.marching_cubes: lattice-ordered vertices, open
    where the surface leaves the grid, thousands of fans of mixed valence."""
    from sculptmate_amd import ops

    vol = ops.density_grid(model["codes"][0].contiguous(), model["m"].decoder, 32)
    v, f = ops.marching_cubes((vol - vol.median()).view(32, 32, 32).contiguous(), 0.0)
    P, F = _np(v), _np(f)
    assert len(F) > 1000
    A = np.random.default_rng(7).random((len(P), 3)).astype(np.float32)
    Q, G, B = ref.subdivide(P, F, 1, A)
    gv, gf, ga = ops.mesh_subdivide(v, f, 1, attributes=torch.from_numpy(A).to(cuda))
    assert np.array_equal(_np(gf), G)
    _same_bits(gv, Q, "positions")
    _same_bits(ga, B, "attributes")
    nb = ref.Topology(F, len(P)).classes()[0]
    assert (nb == 2).any() and (nb == 0).any()                                   # creases and interior fans both occur


# ---------------------------------------------------------------------------------------------------------- the contract
@pytest.fixture(scope="module")
def sphere(cuda):
    P, F = ref.icosphere(2)
    P = (P + 0.01 * np.random.default_rng(0).standard_normal(P.shape)).astype(np.float32)
    return (P, F) + _dev(cuda, P, F)


def test_faces_are_subdivide_devices_and_midpoint_is_subdivide_device(cuda, sphere):
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d import remesh_device as rd

    for P, F, v, f in (sphere, MESHES["patch"]() + _dev(cuda, *MESHES["patch"]()), MESHES["three_face_edge"]() + _dev(cuda, *MESHES["three_face_edge"]())):
        mv, mf = rd.subdivide_device(v, f, 2)
        lv, lf, _ = ops.mesh_subdivide(v, f, 2)
        assert torch.equal(lf, mf) and tuple(lv.shape) == tuple(mv.shape) and not torch.equal(lv, mv)
        A = torch.rand((len(P), 4), device=cuda)
        gv, gf, ga = ops.mesh_subdivide(v, f, (2, "midpoint"), attributes=A)
        assert torch.equal(gf, mf) and np.array_equal(_bits(gv), _bits(mv))
        An = np.pad(_np(A), ((0, 0), (0, 2)))                                    # 4 channels as two groups of three columns
        want = np.concatenate([ref.midpoint(An[:, c:c + 3], F, 2)[0] for c in (0, 3)], 1)[:, :4]
        _same_bits(ga, np.ascontiguousarray(want), "midpoint attributes")       # linear refinement: fp32 midpoints
        assert ops.mesh_subdivide(v, f, (2, "midpoint"))[2] is None
        rP, rF = ref.midpoint(P, F, 2)
        assert np.array_equal(_np(mf), rF) and np.array_equal(_bits(mv), _bits(rP))


def test_contract_of_the_call(cuda, sphere):
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d import remesh_device as rd

    P, F, v, f = sphere
    A = torch.rand((len(P), 8), device=cuda)                               # the most channels
    v0, f0, A0 = v.clone(), f.clone(), A.clone()
    a = ops.mesh_subdivide(v, f, 2, attributes=A)
    stats = rd.last_stats()
    assert stats["passes"] == 2 and stats["readbacks"] == 2               # a topology per level, its one read
    assert torch.equal(v, v0) and torch.equal(f, f0) and torch.equal(A, A0)   # inputs unchanged
    b = ops.mesh_subdivide(v, f, 2, attributes=A)
    for x, y in zip(a, b):                                                  # two calls, the same bits, new tensors
        assert torch.equal(x, y) and x.data_ptr() != y.data_ptr()
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[2]), _bits(b[2]))
    _same_bits(a[2], ref.subdivide(P, F, 2, _np(A))[2], "8 channels")
    one = ops.mesh_subdivide(v, f, 2, attributes=A[:, :1].contiguous())[2]   # the fewest
    assert np.array_equal(_bits(one), _bits(a[2][:, :1].contiguous()))
    c = ops.mesh_subdivide(v, f.long(), 2)                                  # int64 faces: the dtype follows, as in mesh_simplify
    assert c[1].dtype == torch.int64 and torch.equal(c[1], a[1].long()) and np.array_equal(_bits(c[0]), _bits(a[0])) and c[2] is None
    assert ops.mesh_simplify(v, f.long(), 0.5)[1].dtype == torch.int64 and ops.mesh_simplify(v, f, 0.5)[1].dtype == f.dtype
    P64 = P.astype(np.float64) + 1e-9                                       # float64 vertices: rounded once to float32
    d = ops.mesh_subdivide(torch.from_numpy(P64).to(cuda), f, 1)
    _same_bits(d[0], ref.subdivide(P64.astype(np.float32), F, 1)[0], "float64 input")
    for rule in (3, (3, "midpoint")):                                       # no faces: copies
        e = ops.mesh_subdivide(v, f[:0], rule, attributes=A)
        assert torch.equal(e[0], v) and e[0].data_ptr() != v.data_ptr() and tuple(e[1].shape) == (0, 3) and e[1].dtype == f.dtype
        assert torch.equal(e[2], A) and e[2].data_ptr() != A.data_ptr()
    none = ops.mesh_subdivide(v[:0], f[:0], 1)
    assert tuple(none[0].shape) == (0, 3) and tuple(none[1].shape) == (0, 3)


def test_a_permutation_of_the_faces_moves_a_component_by_at_most_one_ulp(cuda, sphere):
    """The permutation changes the numbering of the new vertices and the order of every fan, nothing else: the new vertex of
    an edge is found through the faces.  Each value is an fp64 expression rounded once to fp32; reordering the fp64 sum moves
    it by a few fp64 ulps, which can cross at most one fp32 rounding boundary."""
    from sculptmate_amd import ops

    P, F, v, f = sphere
    perm = np.random.default_rng(11).permutation(len(F))
    a = ops.mesh_subdivide(v, f, 1)
    b = ops.mesh_subdivide(v, torch.from_numpy(F[perm]).to(cuda), 1)
    av, af, bv, bf = _np(a[0]), _np(a[1]), _np(b[0]), _np(b[1])
    nv = len(P)

    def ordered(x):
        """float32 -> integers in the order of the values: adjacent floats are adjacent integers, across zero too."""
        i = np.ascontiguousarray(x).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    def ulps(x, y):
        return np.abs(ordered(x) - ordered(y))

    assert ulps(av[:nv], bv[:nv]).max() <= 1
    # child rows 4 j .. 4 j + 3 of the permuted call are the children of face perm[j]: the same corners, the same edge vertices
    got, want = bv[bf.reshape(-1, 4, 3)], av[af.reshape(-1, 4, 3)[perm]]
    assert ulps(got, want).max() <= 1
    odd_got, odd_want = bv[bf.reshape(-1, 4, 3)[:, 3]], av[af.reshape(-1, 4, 3)[perm][:, 3]]
    assert np.array_equal(_bits(odd_got), _bits(odd_want))                    # an edge vertex has no order to move: the same bits
    print("even vertices: max %d ulp; all corners of all children: max %d ulp" % (ulps(av[:nv], bv[:nv]).max(), ulps(got, want).max()))


def test_refusals(cuda):
    """Refused on the host side of the call: nothing that could fault is launched."""
    from sculptmate_amd import ops

    P, F = ref.octahedron()
    v, f = _dev(cuda, P, F)
    for rule in (1, (1, "midpoint")):
        with pytest.raises(ops.SculptError):
            ops.mesh_subdivide(v.cpu(), f.cpu(), rule)
        with pytest.raises(ops.SculptError):
            ops.mesh_subdivide(v, f, rule, attributes=torch.zeros((6, 3)))        # a CPU attribute array
        bad = f.clone()
        bad[3, 1] = 6
        with pytest.raises(ops.SculptError, match="out of range"):
            ops.mesh_subdivide(v, bad, rule)
        bad[3, 1] = -1
        with pytest.raises(ops.SculptError, match="out of range"):
            ops.mesh_subdivide(v, bad, rule)
        bad[3, 1] = bad[3, 0]
        with pytest.raises(ops.SculptError, match="repeated"):
            ops.mesh_subdivide(v, bad, rule)
        nan = v.clone()
        nan[2, 1] = float("nan")
        with pytest.raises(ops.SculptError, match="non-finite"):
            ops.mesh_subdivide(nan, f, rule)
        for attributes in (torch.zeros((5, 3), device=cuda), torch.zeros((7, 3), device=cuda), torch.zeros((6, 9), device=cuda),
                           torch.zeros((6, 0), device=cuda), torch.zeros(6, device=cuda), torch.zeros((6, 3), dtype=torch.int32, device=cuda)):
            with pytest.raises(ops.SculptError, match="attributes"):
                ops.mesh_subdivide(v, f, rule, attributes=attributes)
    for vv, ff in ((v[:, :2], f), (v, f[:, :2]), (v.long(), f), (v, f.float()), (v, f.to(torch.int16))):
        with pytest.raises(ops.SculptError):
            ops.mesh_subdivide(vv, ff, 1)
    with pytest.raises(ValueError):
        ops.mesh_subdivide(v, f, 7)
    # 366 300 faces x 4^6 = 1.5004e9: three times that leaves int32 -- refused before a level runs
    n = 366_300
    i = torch.arange(n, dtype=torch.int32, device=cuda)
    strip, pts = torch.stack([i, i + 1, i + 2], 1), torch.rand((n + 2, 3), device=cuda)
    for rule in (6, (6, "midpoint")):
        with pytest.raises(ops.SculptError, match="int32"):
            ops.mesh_subdivide(pts, strip, rule)
    _same_bits(ops.mesh_subdivide(v, f, 1)[0], ref.subdivide(P, F, 1)[0], "the good call still works")


def test_entry_points_refuse_bad_arguments(cuda):
    """Error codes with a message, nothing launched: the sentinel-filled outputs keep their values."""
    from sculptmate_amd import _lib
    from sculptmate_amd.sf3d import remesh_device as rd

    lib, p = _lib.lib, rd._p
    P, F = ref.octahedron()
    v, f = _dev(cuda, P, F)
    ctx = rd._Ctx()
    T = rd._loop_topology(ctx, f, 6)
    assert T.ne == 12
    first = torch.empty(24, dtype=torch.int32, device=cuda)
    _lib.check(lib.sculpt_rmd_first_halfedge(T.ref(), p(first), ctx.stream))
    rank = torch.cumsum(first, 0, dtype=torch.int32)
    cls = torch.full((7, 4), -5, dtype=torch.int32, device=cuda)
    rows = torch.full((7, 4), -5.0, dtype=torch.float32, device=cuda)
    Po, Fo = torch.full((19, 3), 7.0, device=cuda), torch.full((33, 3), 7, dtype=torch.int32, device=cuda)
    A, Ao = torch.rand((6, 2), device=cuda), torch.full((19, 2), 7.0, device=cuda)

    def topo(**kw):
        c = T.c
        vals = dict(F=c.F, skeys=c.skeys, she=c.she, es=c.es, fe=c.fe, vfs=c.vfs, vfc=c.vfc, bnd=c.bnd, nf=c.nf, nv=c.nv, ne=c.ne)
        vals.update(kw)
        t = _lib.RmdTopo(*(vals[k] for k in ("F", "skeys", "she", "es", "fe", "vfs", "vfc", "bnd", "nf", "nv", "ne")))
        return t, ctypes.c_void_p(ctypes.addressof(t))

    def classify(**kw):
        a = dict(topo=T.ref(), P=p(v), cls=p(cls), rows=p(rows))
        a.update(kw)
        return lib.sculpt_subdiv_classify(a["topo"], a["P"], a["cls"], a["rows"], ctx.stream)

    def loop(**kw):
        a = dict(topo=T.ref(), cls=p(cls), rows=p(rows), rank=p(rank), A=p(A), C=2, Po=p(Po), Fo=p(Fo), Ao=p(Ao))
        a.update(kw)
        return lib.sculpt_subdiv_loop(a["topo"], a["cls"], a["rows"], a["rank"], a["A"], a["C"], a["Po"], a["Fo"], a["Ao"], ctx.stream)

    keep = []
    for field, value, word in (("nv", 1 << 31, "int32"), ("nv", -1, "too large"), ("ne", 25, "int32"), ("nf", 1 << 30, "too large"),
                               ("nv", (1 << 31) - 6, "int32"), ("nv", 0, "without vertices"), ("F", None, "null topology array"),
                               ("vfc", None, "null topology array")):
        t, r = topo(**{field: value})
        keep.append(t)
        assert classify(topo=r) != 0 and word in _lib.last_error(), (field, value, _lib.last_error())
        assert loop(topo=r) != 0 and word in _lib.last_error(), (field, value, _lib.last_error())
    for bad, word in ((dict(topo=None), "null topology"), (dict(P=None), "null"), (dict(cls=None), "null"), (dict(rows=None), "null"),
                      (dict(cls=cls.data_ptr() + 4), "aligned"), (dict(rows=rows.data_ptr() + 8), "aligned")):
        assert classify(**bad) != 0 and word in _lib.last_error(), (bad, _lib.last_error())
    for bad, word in ((dict(topo=None), "null topology"), (dict(cls=None), "null"), (dict(rows=None), "null"), (dict(rank=None), "null"),
                      (dict(Po=None), "null"), (dict(Fo=None), "null"), (dict(A=None), "together"), (dict(Ao=None), "together"),
                      (dict(C=0), "channels"), (dict(C=9), "channels"), (dict(C=-1), "channels"), (dict(cls=cls.data_ptr() + 4), "aligned"),
                      (dict(rows=rows.data_ptr() + 4), "aligned"), (dict(Po=p(rows)), "must not be"), (dict(Ao=p(A)), "must not be")):
        assert loop(**bad) != 0 and word in _lib.last_error(), (bad, _lib.last_error())
    torch.cuda.synchronize()
    assert (cls == -5).all() and (rows == -5.0).all() and (Po == 7.0).all() and (Fo == 7).all() and (Ao == 7.0).all()
    t, r = topo(nf=0, ne=0)                                           # no faces: nothing launched, no error
    assert classify(topo=r) == 0 and loop(topo=r) == 0
    torch.cuda.synchronize()
    assert (cls == -5).all() and (Po == 7.0).all()
    # and the good calls still work, and write nothing past their counts
    assert classify() == 0 and loop() == 0
    Q, G, B = ref.subdivide(P, F, 1, _np(A))
    _same_bits(Po[:18], Q, "positions")
    _same_bits(Ao[:18], B, "attributes")
    assert np.array_equal(_np(Fo[:32]), G)
    assert (Po[18] == 7.0).all() and (Fo[32] == 7).all() and (Ao[18] == 7.0).all() and (cls[6] == -5).all() and (rows[6] == -5.0).all()
    assert (cls[:6] == 0).all() and np.array_equal(_bits(rows[:6, :3].contiguous()), _bits(P))      # closed: nothing to classify
    assert loop(A=None, Ao=None, C=0) == 0                            # without attributes


def test_classification(cuda):
    """cls on the meshes that have borders and non-manifold edges, against the restatement's classes."""
    from sculptmate_amd import _lib
    from sculptmate_amd.sf3d import remesh_device as rd

    for name in ("patch", "three_face_edge", "cone70"):
        P, F = MESHES[name]()
        v, f = _dev(cuda, P, F)
        ctx = rd._Ctx()
        T = rd._loop_topology(ctx, f, len(P))
        cls = torch.full((len(P), 4), -5, dtype=torch.int32, device=cuda)
        rows = torch.empty((len(P), 4), dtype=torch.float32, device=cuda)
        _lib.check(_lib.lib.sculpt_subdiv_classify(T.ref(), rd._p(v), rd._p(cls), rd._p(rows), ctx.stream))
        c = _np(cls)
        nb, nm, lo, hi = ref.Topology(F, len(P)).classes()
        assert np.array_equal(c[:, 0], nb) and np.array_equal(c[:, 3], nm.astype(np.int32))
        has = nb > 0
        assert np.array_equal(c[has, 1] - 1, hi[has]) and np.array_equal(len(P) - c[has, 2], lo[has])
        assert (c[~has, 1] == 0).all() and (c[~has, 2] == 0).all()


# --------------------------------------------------------------------------------------------------------- Mesh.subdivide
def test_mesh_subdivide_method(cuda):
    from sculptmate_amd.tsr.system import Mesh

    P, F = ref.grid_patch()
    v, f = _dev(cuda, P, F)
    col = torch.rand((25, 3), device=cuda)
    col[:5] = 1.0                                                                  # saturated rows: the masks must not leave [0, 1]
    col[5:10] = 0.0
    nrm, ao = torch.rand((25, 3), device=cuda), torch.rand(25, device=cuda)
    got = Mesh(v, f, col, vertex_normals=nrm, vertex_occlusion=ao).subdivide(2)
    Q, G, B = ref.subdivide(P, F, 2, _np(col))
    _same_bits(got.vertices, Q, "positions")
    _same_bits(got.vertex_colors, B, "colours")
    assert np.array_equal(_np(got.faces), G)
    assert got.vertex_normals is None and got.vertex_occlusion is None and got.uvs is None and got.texture is None
    c = _np(got.vertex_colors)
    assert c.min() >= 0.0 and c.max() <= np.nextafter(np.float32(1), np.float32(2))    # within [0, 1] up to one ulp
    plain = Mesh(v, f).subdivide((1, "midpoint"))
    assert plain.vertex_colors is None and tuple(plain.faces.shape) == (4 * len(F), 3)
    uvs, tex = torch.rand((3 * len(F), 2), device=cuda), torch.rand((4, 4, 3), device=cuda)
    for baked in (Mesh(v, f, uvs=uvs, texture=tex), Mesh(v, f, uvs=uvs), Mesh(v, f, texture=tex)):
        with pytest.raises(ValueError, match="subdivide before baking"):
            baked.subdivide(1)


# --------------------------------------------------------------------------------------------------- through the model
def test_none_launches_nothing_new_and_changes_nothing(model, monkeypatch):
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d import remesh_device as rd

    m, plain, kw = model["m"], model["plain"], model["kw"]

    def refuse(*a, **k):
        raise AssertionError("subdivide=None must not reach the subdivision")

    monkeypatch.setattr(ops, "mesh_subdivide", refuse)
    monkeypatch.setattr(ops, "subdivide_rule", refuse)
    monkeypatch.setattr(rd, "loop_subdivide_device", refuse)
    monkeypatch.setattr(rd, "subdivide_device", refuse)
    for name in ("sculpt_subdiv_classify", "sculpt_subdiv_loop", "sculpt_rmd_subdivide", "sculpt_rmd_first_halfedge"):
        monkeypatch.setattr(rd.lib, name, refuse)
    for extra in ({}, {"subdivide": None}):
        again = m.extract_meshes(model["codes"], enable_texture=True, normals="field", **kw, **extra)[0]
        assert np.array_equal(_bits(again.vertices), _bits(plain.vertices)) and torch.equal(again.faces, plain.faces)
        assert np.array_equal(_bits(again.vertex_colors), _bits(plain.vertex_colors))
        assert np.array_equal(_bits(again.vertex_normals), _bits(plain.vertex_normals))


def test_extract_meshes_is_the_composed_route(model):
    """marching cubes -> keep_components -> simplify -> subdivide -> project, then colours and normals at the final vertices."""
    m, plain, kw, code = model["m"], model["plain"], model["kw"], model["codes"][0]
    options = dict(keep_components="largest", simplify=0.25, subdivide=1, project=True)
    cage = plain.keep_components("largest").simplify(0.25)
    fine = cage.subdivide(1)
    want = m.project_mesh(fine, code, threshold=model["threshold"], project=True, resolution=32)
    got = m.extract_meshes(model["codes"], **options, **kw)[0]
    assert got.faces.shape[0] == 4 * cage.faces.shape[0] > 0 and got.faces.dtype == plain.faces.dtype
    assert torch.equal(got.faces, fine.faces) and torch.equal(got.faces, want.faces)
    assert np.array_equal(_bits(got.vertices), _bits(want.vertices)) and not np.array_equal(_bits(got.vertices), _bits(fine.vertices))
    assert got.vertex_colors is None and got.vertex_normals is None
    assert tuple(fine.vertex_colors.shape) == tuple(fine.vertices.shape)              # Mesh.subdivide carried the colours
    print("32^3: %d faces -> cage %d -> refined %d" % (plain.faces.shape[0], cage.faces.shape[0], got.faces.shape[0]))
    full = m.extract_meshes(model["codes"], enable_texture=True, normals="field", **options, **kw)[0]
    assert np.array_equal(_bits(full.vertices), _bits(want.vertices)) and torch.equal(full.faces, want.faces)
    planes = code.contiguous()
    color = m.renderer.query_triplane(m.decoder, want.vertices, planes)["color"]
    assert np.array_equal(_bits(full.vertex_colors), _bits(color))                    # evaluated at the returned vertices
    assert np.array_equal(_bits(full.vertex_normals), _bits(m.field_normals(want.vertices, planes)))
    host = m.run([model["img"]], mc_resolution=32, threshold=model["threshold"], keep_components="largest", simplify=0.25,
                 subdivide=(1, "midpoint"))[0]
    assert isinstance(host.vertices, np.ndarray) and np.array_equal(host.faces, _np(fine.faces))


def test_generator_attribute_reaches_extract_mesh(cuda, tmp_path):
    import types

    from test_host_logic import _write_checkpoint

    from sculptmate_amd import ops
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr.spec import SMALL_CFG

    _write_checkpoint(str(tmp_path), SMALL_CFG, seed=61)
    g = TripoGenerator(cuda)
    assert g.subdivide is None
    g.checkpoint_dir = str(tmp_path)
    g.mc_resolution = 32
    assert g.initiate_model() == 0
    g.model.mesh_sink = lambda v, f, c, name: None
    orig, seen = g.model.extract_mesh, []

    def reachable(self, codes, **kw):   # random weights never reach the default threshold: take the grid's median
        seen.append(kw["subdivide"])
        return orig(codes, **dict(kw, threshold=float(ops.density_grid(codes[0].contiguous(), self.decoder, kw["resolution"]).median())))

    g.model.extract_mesh = types.MethodType(reachable, g.model)
    img = (synth.composite_rgb(synth.image_rgba(seed=62, size=SMALL_CFG["cond_image_size"])) * 255).astype(np.uint8)
    assert g.generate_mesh(img, "plain") == 0
    plain = g.last_meshes[0]
    g.subdivide = 1
    assert g.generate_mesh(img, "refined") == 0
    mesh = g.last_meshes[0]
    want = ops.mesh_subdivide(plain.vertices, plain.faces, 1)
    assert seen == [None, 1] and torch.equal(mesh.faces, want[1]) and np.array_equal(_bits(mesh.vertices), _bits(want[0]))
