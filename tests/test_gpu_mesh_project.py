"""Projection of mesh vertices onto the field's iso-surface on the GPU (csrc/mesh_project.hip: sculpt_triplane_project,
sculpt_mesh_unfold) against its restatements in tests/_projref.py.

Point sets:
  (A) the 7924 vertices of the 32^3 oracle mesh of the smoke() field, t = ln 25 + 1, max_dist = one cell of that lattice;
  (B) the 2043 points of tests/golden/field_normal.npz on their hostile field (zero-padding band, cut-off plane pairs, 128 points
      outside every plane, an 8-aligned run), t = the median of density64 over its set (a), max_dist = one cell of a 64^3 lattice.
res_tol = 1e-3 throughout.  One fused result per set (steps = 8, every output) is computed once and shared; nothing modifies it."""
import os

import numpy as np
import pytest
import torch

import _projref as ref
import _tsrmodel
from conftest import GOLDEN
from sculptmate_amd import synth

pytestmark = pytest.mark.gpu

RADIUS = 0.87
RES_TOL = 1e-3
WANT = ("residual", "status", "evals")


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def sets(cuda):
    from sculptmate_amd import ops

    a = ref.mesh_set_a()
    A = dict(name="A", planes_np=a["planes"], Ws=a["Ws"], bs=a["bs"], pts_np=a["vertices"], faces_np=a["faces"], t=a["target"],
             max_dist=a["cell"])
    g = np.load(os.path.join(GOLDEN, "field_normal.npz"))
    Ws, bs = synth.decoder_lists(synth.decoder_state(seed=1))
    o = g["set_offsets"]
    B = dict(name="B", planes_np=synth.triplane(seed=2, scale=4.0), Ws=Ws, bs=bs, pts_np=g["points"],
             t=float(np.float32(np.median(g["density64"][:int(o[1])]))), max_dist=2 * RADIUS / 63, outside=slice(int(o[3]), int(o[4])))
    for S in (A, B):
        S["mlp"] = ops.PackedMLP(S["Ws"], S["bs"], cuda)
        S["raw"] = torch.from_numpy(S["planes_np"]).to(cuda)
        S["planes"] = ops.ChannelLastPlanes(S["raw"])
        S["pts"] = torch.from_numpy(S["pts_np"]).to(cuda)
        p, ex = ops.project_to_isosurface(S["planes"], S["mlp"], S["pts"], S["t"], S["max_dist"], steps=8, res_tol=RES_TOL, radius=RADIUS,
                                          want=WANT)
        S["got"] = dict(ex, points=p)
        S["host"] = {k: v.cpu().numpy() for k, v in S["got"].items()}
    return {"A": A, "B": B}


@pytest.mark.parametrize("steps", [0, 1, 3, 8])
@pytest.mark.parametrize("name", ["A", "B"])
def test_fused_equals_composed_bit_for_bit(sets, name, steps):
    """Points, residual, status and evals of the one-launch kernel against the rule written with ops.field_normals and one torch
    fp32 call per operation (composed_device).  On (B) the points outside every plane (zero gradient) come back with their input
    bits and status 3 as soon as a step is tried; with steps = 0 no step is tried and the rule's item 3 gives them 0 or 1."""
    from sculptmate_amd import ops

    S = sets[name]
    if steps == 8:
        got = S["got"]
    else:
        p, ex = ops.project_to_isosurface(S["planes"], S["mlp"], S["pts"], S["t"], S["max_dist"], steps=steps, res_tol=RES_TOL,
                                          radius=RADIUS, want=WANT)
        got = dict(ex, points=p)
    cp, cr, cs, ce = ref.composed_device(ops, S["planes"], S["mlp"], S["pts"], S["t"], steps, S["max_dist"], RES_TOL, RADIUS)
    N = len(S["pts_np"])
    assert got["points"].shape == (N, 3) and got["points"].dtype == torch.float32
    assert got["residual"].shape == (N,) and got["residual"].dtype == torch.float32
    assert got["status"].shape == (N,) and got["status"].dtype == torch.int32 and got["evals"].dtype == torch.int32
    status = got["status"].cpu().numpy()
    print("set (%s), steps %d: status histogram %s, mean evals %.2f" % (name, steps, np.bincount(status, minlength=4).tolist(),
                                                                         float(got["evals"].float().mean())))
    assert _same(got["status"], cs), np.flatnonzero(status != cs.cpu().numpy())[:8]
    assert _same(got["evals"], ce)
    assert _same(got["points"], cp)
    assert _same(got["residual"], cr)
    if steps == 0:
        assert _same(got["points"], S["pts"]) and bool((got["evals"] == 1).all()) and set(np.unique(status)) <= {0, 1}
    if name == "B":
        d = S["outside"]
        assert _same(got["points"][d], S["pts"][d])
        if steps >= 1:
            assert (status[d] == 3).all() and bool((got["evals"][d] == 1).all())


@pytest.mark.parametrize("name", ["A", "B"])
def test_the_residual_is_the_point_querys(sets, name):
    from sculptmate_amd import ops

    S = sets[name]
    d = ops.triplane_query(S["planes"], S["mlp"], S["got"]["points"], radius=RADIUS, want=("density",))["density"][:, 0]
    assert bool(torch.isfinite(d).all())
    assert _same(S["got"]["residual"], d - S["t"])


def test_a_points_result_is_its_own(sets):
    from sculptmate_amd import ops

    for name in ("A", "B"):
        S = sets[name]
        got, pts = S["got"], S["pts"]
        kw = dict(steps=8, res_tol=RES_TOL, radius=RADIUS, want=WANT)
        perm = torch.from_numpy(np.random.default_rng(5).permutation(len(pts))).to(pts.device)
        p, ex = ops.project_to_isosurface(S["planes"], S["mlp"], pts[perm].contiguous(), S["t"], S["max_dist"], **kw)
        assert _same(p, got["points"][perm])
        for k in WANT:
            assert _same(ex[k], got[k][perm]), (name, k)
    for n in (1, 7, 8, 9, 33):       # on (B), the last of the loop above
        p, ex = ops.project_to_isosurface(S["planes"], S["mlp"], pts[:n].contiguous(), S["t"], S["max_dist"], **kw)
        assert p.shape == (n, 3) and _same(p, got["points"][:n]), n
        for k in WANT:
            assert ex[k].shape == (n,) and _same(ex[k], got[k][:n]), (k, n)
    # a leading shape, the reference layout of the planes, and no extras
    S = sets["B"]
    got = S["got"]
    p, ex = ops.project_to_isosurface(S["raw"], S["mlp"], S["pts"][:2040].view(8, 255, 3), S["t"], S["max_dist"], **kw)
    assert p.shape == (8, 255, 3) and ex["status"].shape == (8, 255) and ex["residual"].shape == (8, 255)
    assert _same(p.reshape(2040, 3), got["points"][:2040])
    for k in WANT:
        assert _same(ex[k].reshape(2040), got[k][:2040]), k
    p, ex = ops.project_to_isosurface(S["planes"], S["mlp"], S["pts"], S["t"], S["max_dist"], steps=8, res_tol=RES_TOL, radius=RADIUS)
    assert ex == {} and _same(p, got["points"])


@pytest.mark.parametrize("name", ["A", "B"])
def test_invariants(sets, name):
    S = sets[name]
    p0, h = S["pts_np"], S["host"]
    moved = np.linalg.norm(h["points"].astype(np.float64) - p0.astype(np.float64), axis=1)
    assert moved.max() <= S["max_dist"] * (1 + 1e-6), moved.max() / S["max_dist"]
    frozen = np.abs(p0) >= np.float32(RADIUS)
    assert np.array_equal(h["points"].view(np.uint32)[frozen], p0.view(np.uint32)[frozen])
    inside = (np.abs(p0) <= np.float32(RADIUS)).all(axis=1)
    assert (np.abs(h["points"][inside]) <= np.float32(RADIUS)).all()
    assert h["evals"].min() >= 1 and h["evals"].max() <= 9
    assert set(np.unique(h["status"])) <= {0, 1, 2, 3}
    print("set (%s): %d frozen coordinates, %d points inside the box, largest displacement %.3f of max_dist" % (
        name, frozen.sum(), inside.sum(), moved.max() / S["max_dist"]))


@pytest.mark.parametrize("name", ["A", "B"])
def test_against_the_fp64_field(sets, name):
    """r64 = the fp64 restatement's density - t.  E32d = the fp32 error of the restatement on the returned points (fp32 run
    against fp64 run, in-test).  The device picks its best iterate by its own residual, each within 4 E32d of the fp64 one, so
    |r64(p')| <= |r64(p0)| + 8 E32d for every point; a status-0 point has |r64(p')| <= res_tol + 4 E32d; and on (A) at least
    98.5 % of the points are status 0 (the fp64 rule alone gives >= 99 %, tests/test_project_host.py; 0.5 % for decisions that
    fp32 takes the other way at the trust region)."""
    S = sets[name]
    h, t = S["host"], S["t"]
    args = (S["planes_np"], S["Ws"], S["bs"])
    d64_0, _ = ref.value_grad(*args, S["pts_np"], np.float64)
    d64_1, _ = ref.value_grad(*args, h["points"], np.float64)
    d32_1, _ = ref.value_grad(*args, h["points"], np.float32)
    e32d = float(np.abs(d32_1.astype(np.float64) - d64_1).max())
    r0, r1 = np.abs(d64_0 - t), np.abs(d64_1 - t)
    want = ref.newton(*args, S["pts_np"], t, 8, S["max_dist"], RES_TOL, np.float64)
    dist = np.linalg.norm(h["points"].astype(np.float64) - want["points"], axis=1)
    ok = h["status"] == 0
    dev_err = float(np.abs(h["residual"].astype(np.float64) - (d64_1 - t)).max())
    print("set (%s): E32d %.3e; device residual vs fp64 %.3e; median |r64| %.3e -> %.3e; status 0 on %.2f %% (fp64 rule %.2f %%); "
          "distance to the fp64 result: median %.3e, largest %.3e (%.3e among points both converged)" % (
              name, e32d, dev_err, np.median(r0), np.median(r1), 100 * ok.mean(), 100 * (want["status"] == 0).mean(), np.median(dist),
              dist.max(), dist[ok & (want["status"] == 0)].max()))
    assert (r1 <= r0 + 8 * e32d).all(), float((r1 - r0).max())
    assert (r1[ok] <= RES_TOL + 4 * e32d).all(), float(r1[ok].max())
    if name == "A":
        assert ok.mean() >= 0.985


@pytest.mark.parametrize("rounds", [0, 1, 4])
def test_the_guard_equals_its_restatement(sets, rounds):
    from sculptmate_amd import ops

    S = sets["A"]
    v0, v1 = S["pts"], S["got"]["points"]
    F = torch.from_numpy(S["faces_np"]).to(v0.device)
    keep0, keep1 = v0.clone(), v1.clone()
    v, stats = ops.mesh_unfold(v0, v1, F, rounds)
    want, reverted, left = ref.unfold(S["pts_np"], S["host"]["points"], S["faces_np"], rounds)
    assert stats.dtype == torch.int32 and stats.shape == (2,) and stats.is_cuda
    got = ops.unfold_stats(stats)
    print("guard, rounds %d: %d faces inverted before, %s" % (rounds, ref.inverted(S["pts_np"], S["host"]["points"], S["faces_np"]).sum(), got))
    assert got == {"reverted": reverted, "inverted": left}
    assert v.shape == v1.shape and _same(v, want)
    assert torch.equal(v0, keep0) and torch.equal(v1, keep1) and v.data_ptr() != v1.data_ptr()      # the inputs are untouched
    if rounds == 0:
        assert _same(v, v1) and got["reverted"] == 0 and got["inverted"] > 0     # this mesh does fold: the guard has work
    if rounds == 4:
        assert got["inverted"] == 0
        v32, s32 = ops.mesh_unfold(v0, v1, F.to(torch.int32), 4)               # int32 faces
        assert _same(v32, v) and ops.unfold_stats(s32) == got
        vp, info = ops.mesh_project(S["planes"], S["mlp"], v0, F, S["t"], S["max_dist"], steps=8, res_tol=RES_TOL, radius=RADIUS,
                                    want=("status",))
        assert _same(vp, v) and ops.unfold_stats(info["stats"]) == got and _same(info["status"], S["got"]["status"])


# --------------------------------------------------------------------------------------------------------------------------------
# the model surface
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(cuda):
    """The shared small model at resolution 32, its bare plain mesh and the projection's target / cell / radius."""
    return _tsrmodel.small_model(cuda, 32, project_keys=True)


def test_model_surface(model):
    from sculptmate_amd import ops
    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr.spec import SMALL_CFG

    m, plain, code = model["m"], model["plain"], model["codes"][0]
    kw = dict(resolution=32, threshold=model["threshold"])

    def project(v, f, steps=8, cells=1.0):
        return ops.mesh_project(code, m.decoder, v, f, model["target"], cells * model["cell"], steps=steps, radius=model["radius"])[0]

    none = m.extract_meshes(model["codes"], project=None, **kw)[0]
    assert _same(none.vertices, plain.vertices) and torch.equal(none.faces, plain.faces)
    got = m.extract_meshes(model["codes"], project=True, **kw)[0]
    want = project(plain.vertices, plain.faces)
    assert torch.equal(got.faces, plain.faces) and _same(got.vertices, want) and not _same(want, plain.vertices)
    assert got.vertex_normals is None and got.vertex_colors is None
    moved = torch.linalg.norm((want - plain.vertices).double(), dim=1)
    print("model mesh: %d vertices, %.1f %% moved, largest displacement %.3f cell" % (
        len(want), 100 * float((moved > 0).float().mean()), float(moved.max()) / model["cell"]))
    assert float(moved.max()) <= model["cell"] * (1 + 1e-6)
    # the other forms of the rule
    few = m.extract_meshes(model["codes"], project=(2, 0.5), **kw)[0]
    assert _same(few.vertices, project(plain.vertices, plain.faces, 2, 0.5))
    assert _same(m.extract_meshes(model["codes"], project=8, **kw)[0].vertices, want)
    # normals, colours and the bake are evaluated at the projected vertices
    field = m.extract_meshes(model["codes"], project=True, normals="field", **kw)[0]
    assert _same(field.vertices, want) and _same(field.vertex_normals, m.field_normals(want, code))
    coloured = m.extract_meshes(model["codes"], project=True, enable_texture=True, **kw)[0]
    colour = m.renderer.query_triplane(m.decoder, want, code)["color"]
    assert coloured.vertex_colors is not None and _same(coloured.vertex_colors, colour) and _same(coloured.vertices, want)
    baked = m.extract_meshes(model["codes"], project=True, enable_texture=True, bake_texture=64, **kw)[0]
    assert baked.texture is not None and baked.texture.shape == (64, 64, 3) and baked.uvs is not None and _same(baked.vertices, want)
    # the order: keep_components, smooth, simplify, then the projection
    both = m.extract_meshes(model["codes"], smooth=2, simplify=0.5, project=True, **kw)[0]
    sv = ops.mesh_smooth(plain.vertices, plain.faces, 2)
    qv, qf = ops.mesh_simplify(sv, plain.faces, 0.5)[:2]
    assert torch.equal(both.faces, qf) and _same(both.vertices, project(qv, qf))
    # TSR.project_mesh: the same vertices, colours and atlas carried over, normals dropped
    again = m.project_mesh(plain, code, model["threshold"], resolution=32)
    assert _same(again.vertices, want) and again.faces is plain.faces
    m.set_marching_cubes_resolution(32)
    assert _same(m.project_mesh(plain, code[None], model["threshold"]).vertices, want)       # the helper's resolution, a batch of one
    assert _same(m.project_mesh(plain, ops.ChannelLastPlanes(code.contiguous()), model["threshold"], project=(2, 0.5), resolution=32).vertices,
                 few.vertices)
    old = m.extract_meshes(model["codes"], enable_texture=True, normals="field", **kw)[0]
    carried = m.project_mesh(old, code, model["threshold"], resolution=32)
    assert carried.vertex_colors is old.vertex_colors and carried.vertex_normals is None and _same(carried.vertices, want)
    # refusals: before anything is launched
    for bad in (False, 0, 65, 0.5, (8, 9.0), "x"):
        with pytest.raises(ValueError):
            m.extract_meshes(model["codes"], project=bad, **kw)
        with pytest.raises(ValueError):
            m.project_mesh(plain, code, model["threshold"], project=bad, resolution=32)
    with pytest.raises(ValueError):
        m.extract_meshes(model["codes"], resolution=32, threshold=0.0, project=True)
    with pytest.raises(ValueError):
        m.project_mesh(plain, code, threshold=-1.0, resolution=32)
    with pytest.raises(ops.SculptError, match="no weights on a device"):
        TSR(SMALL_CFG, pos_embed_mode="size").project_mesh(plain, code, model["threshold"], resolution=32)


def test_run_returns_host_arrays(model):
    m = model["m"]
    plain = m.run([model["img"]], mc_resolution=32, threshold=model["threshold"])[0]
    meshes = m.run([model["img"], model["img"]], mc_resolution=32, threshold=model["threshold"], project=True, normals="field")
    assert len(meshes) == 2
    for mesh in meshes:
        assert isinstance(mesh.vertices, np.ndarray) and mesh.vertices.dtype == np.float32 and mesh.vertices.shape == plain.vertices.shape
        assert np.array_equal(mesh.faces, plain.faces) and not np.array_equal(mesh.vertices, plain.vertices)
        assert mesh.vertex_normals.shape == mesh.vertices.shape
        assert np.abs(mesh.vertices - plain.vertices).max() <= model["cell"] * (1 + 1e-6)
    assert np.array_equal(meshes[0].vertices.view(np.uint32), meshes[1].vertices.view(np.uint32))
    single = m.run([model["img"]], mc_resolution=32, threshold=model["threshold"], project=(8, 1.0))[0]
    assert np.array_equal(single.vertices.view(np.uint32), meshes[0].vertices.view(np.uint32))


def test_generator_projects_last_meshes(cuda, tmp_path):
    import types

    from test_host_logic import _write_checkpoint

    from sculptmate_amd import ops
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr.spec import SMALL_CFG

    _write_checkpoint(str(tmp_path), SMALL_CFG, seed=61)
    g = TripoGenerator(cuda)
    assert g.project is None
    g.checkpoint_dir = str(tmp_path)
    g.mc_resolution = 32
    assert g.initiate_model() == 0
    g.model.mesh_sink = lambda v, f, c, name: None
    orig, seen = g.model.extract_mesh, []

    def reachable(self, codes, **kw):   # random weights never reach the default threshold: take the grid's median
        seen.append(kw.get("project"))
        return orig(codes, **dict(kw, threshold=float(ops.density_grid(codes[0].contiguous(), self.decoder, kw["resolution"]).median())))

    g.model.extract_mesh = types.MethodType(reachable, g.model)
    img = (synth.composite_rgb(synth.image_rgba(seed=62, size=SMALL_CFG["cond_image_size"])) * 255).astype(np.uint8)
    assert g.generate_mesh(img, "plain") == 0
    plain = g.last_meshes[0]
    g.project = True
    assert g.generate_mesh(img, "projected") == 0
    mesh = g.last_meshes[0]
    assert seen == [None, True]
    assert mesh.vertices.shape == plain.vertices.shape and not _same(mesh.vertices, plain.vertices)
    assert np.array_equal(np.asarray(_host(mesh.faces)), np.asarray(_host(plain.faces)))
    g.project = "yes"
    assert g.generate_mesh(img, "refused") != 0          # the ValueError becomes the generator's failure status


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def test_refusals_at_the_c_entry(sets, cuda):
    from sculptmate_amd import _lib, ops

    S = sets["B"]
    planes, mlp, pts = S["planes"], S["mlp"], S["pts"]
    out = torch.zeros((8, 3), device=cuda)
    P = _lib.lib.sculpt_triplane_project

    def call(N=8, steps=8, max_dist=0.01, res_tol=1e-3, out_points=out.data_ptr(), C=40, flags=0):
        return P(planes.data.data_ptr(), C, 64, 64, mlp.blob.data_ptr(), mlp.n_hidden, pts.data_ptr(), N, RADIUS, flags, 0.0, steps,
                 max_dist, res_tol, out_points, None, None, None, None)

    assert call() == 0
    for kw in (dict(N=-1), dict(steps=65), dict(steps=-1), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("nan")),
               dict(res_tol=0.0), dict(res_tol=-1e-3), dict(out_points=None), dict(C=32), dict(flags=8)):
        with pytest.raises(_lib.SculptError):
            _lib.check(call(**kw))
    assert call(N=0, out_points=None) == 0
    p, ex = ops.project_to_isosurface(planes, mlp, pts[:0], 0.0, 0.01, want=WANT)
    assert p.shape == (0, 3) and ex["residual"].shape == (0,) and ex["status"].shape == (0,) and ex["evals"].dtype == torch.int32
    with pytest.raises(_lib.SculptError):
        ops.project_to_isosurface(planes, mlp, pts.cpu(), 0.0, 0.01)
    with pytest.raises(_lib.SculptError):
        ops.project_to_isosurface(planes, mlp, pts, 0.0, 0.01, want=("curvature",))
    # the guard
    F = torch.tensor([[0, 1, 2]], dtype=torch.int64, device=cuda)
    v0, v1 = pts[:8].contiguous(), out
    stats = torch.zeros(2, dtype=torch.int32, device=cuda)
    mark = torch.zeros(8, dtype=torch.int32, device=cuda)
    U = _lib.lib.sculpt_mesh_unfold
    assert U(v0.data_ptr(), v1.data_ptr(), F.data_ptr(), 8, 1, 16, mark.data_ptr(), stats.data_ptr(), None) == 0
    for args in ((v0.data_ptr(), v1.data_ptr(), F.data_ptr(), 8, 1, 17, mark.data_ptr(), stats.data_ptr()),
                 (v0.data_ptr(), v1.data_ptr(), F.data_ptr(), 8, 1, -1, mark.data_ptr(), stats.data_ptr()),
                 (v0.data_ptr(), v1.data_ptr(), F.data_ptr(), -1, 1, 4, mark.data_ptr(), stats.data_ptr()),
                 (v0.data_ptr(), v1.data_ptr(), F.data_ptr(), 8, 1, 4, mark.data_ptr(), None),
                 (v0.data_ptr(), v1.data_ptr(), F.data_ptr(), 8, 1, 4, None, stats.data_ptr()),
                 (v0.data_ptr(), None, F.data_ptr(), 8, 1, 4, mark.data_ptr(), stats.data_ptr()),
                 (v0.data_ptr(), v0.data_ptr(), F.data_ptr(), 8, 1, 4, mark.data_ptr(), stats.data_ptr())):
        with pytest.raises(_lib.SculptError):
            _lib.check(U(*args, None))
    with pytest.raises(ValueError):
        ops.mesh_unfold(v0, v1, F, 17)
    with pytest.raises(_lib.SculptError):
        ops.mesh_unfold(v0.cpu(), v1, F, 4)
    with pytest.raises(_lib.SculptError):
        ops.mesh_unfold(v0, v1[:7], F, 4)
    v, st = ops.mesh_unfold(v0[:0], v1[:0], F[:0], 4)
    assert v.shape == (0, 3) and ops.unfold_stats(st) == {"reverted": 0, "inverted": 0}
    torch.cuda.synchronize()
