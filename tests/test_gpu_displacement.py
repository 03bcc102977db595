"""The displacement bake on the GPU: sculpt_triplane_project_along against the rule restated with one torch call
per operation (tests/_dispref.py composed_device) and against its fp64 run, sculpt_bake_texel_list against torch.nonzero,
ops.bake_displacement (no host wait) against ops.bake_displacement_composed, and TSR.bake_displacement_map.  Float outputs are
compared as 32-bit words, so a NaN's payload and a -0 count."""
import numpy as np
import pytest
import torch

import _dispref as D
import _nmapref as R
import _projref as P
import _tsrmodel
from sculptmate_amd import synth

pytestmark = pytest.mark.gpu

RADIUS = 0.87
RES_TOL = 1e-3
E32D = 6.1e-5          # the fp32 error of the point query's density on set A
WANT = ("residual", "status", "evals")
CASES = [(5, 1.0), (37, 1.0), (64, 0.25), (256, 1.0)]      # (resolution, scale of the UVs): 64 has mostly empty rows
STEPS = [0, 1, 3, 8]


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------- the point-list kernel
@pytest.fixture(scope="module")
def field(cuda):
    """Set A on the device: its field, the face points of tests/_dispref.py with their normals, and the hostile points."""
    from sculptmate_amd import ops

    A = P.mesh_set_a()
    p, n = D.face_points()
    rad32 = np.float32(RADIUS)
    hp, hn = p[:16].copy(), n[:16].copy()
    hp[0] = [1.5, 0.0, 0.0]                                # outside the box
    hp[1] = [0.0, -2.0, 0.3]
    hp[2, 0] = rad32                                       # a coordinate exactly +radius, -radius
    hp[3, 2] = -rad32
    hp[4] = [0.86, 0.0, 0.0]                               # a direction that leaves the box within max_dist
    hn[4] = [1.0, 0.0, 0.0]
    hp[5] = [0.0, 0.86, 0.0]
    hn[5] = [0.0, -3.0, 0.0]                               # and one that is not normalised, pointing in
    hn[6] = 0.0                                            # zero / NaN / Inf directions
    hn[7] = [0.0, np.nan, 0.0]
    hn[8] = [np.inf, 0.0, 0.0]
    hn[9] = [1e30, 1e30, 0.0]                              # N.N overflows
    hn[10] = [1e-30, 0.0, 0.0]                             # N.N underflows to 0
    hp[11] = [0.86, 0.0, 0.0]                              # the twin of 4 pointing in
    hn[11] = [-1.0, 0.0, 0.0]
    hp[12] = np.nan                                        # non-finite points
    hp[13, 1] = np.inf
    hp[14, 2] = -np.inf
    pts = np.concatenate([p, hp]).astype(np.float32)
    dirs = np.concatenate([n, hn]).astype(np.float32)
    return dict(A=A, mlp=ops.PackedMLP(A["Ws"], A["bs"], cuda), planes_cf=torch.from_numpy(A["planes"]).to(cuda),
                planes=ops.ChannelLastPlanes(torch.from_numpy(A["planes"]).to(cuda)), n_face=len(p),
                pts=torch.from_numpy(pts).to(cuda), dirs=torch.from_numpy(dirs).to(cuda), target=A["target"], max_dist=2.0 * A["cell"])


def _along(ops, F, pts, dirs, steps, planes=None, **kw):
    h, ex = ops.project_along(F["planes"] if planes is None else planes, F["mlp"], pts, dirs, F["target"], F["max_dist"], steps=steps,
                              res_tol=RES_TOL, radius=RADIUS, want=WANT, **kw)
    return h, ex["residual"], ex["status"], ex["evals"]


@pytest.fixture(scope="module")
def reference(field):
    """composed_device at every step count, computed once."""
    from sculptmate_amd import ops

    return {k: D.composed_device(ops, field["planes"], field["mlp"], field["pts"], field["dirs"], field["target"], k, field["max_dist"],
                                 RES_TOL, radius=RADIUS) for k in STEPS}


@pytest.mark.parametrize("steps", STEPS)
def test_project_along_equals_the_composed_rule_bit_for_bit(field, reference, steps):
    from sculptmate_amd import ops

    got = _along(ops, field, field["pts"], field["dirs"], steps)
    want = reference[steps]
    for name, a, b in zip(("height", "residual", "status", "evals"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert _same(a, b), (steps, name, int(torch.as_tensor(_bits(a) != _bits(b)).sum()))
    h, r, st, ev = (x.cpu().numpy() for x in got)
    nf = field["n_face"]
    print("steps %d: status histogram %s on the %d face points, mean evals %.2f; hostile: status %s evals %s" % (
        steps, np.bincount(st[:nf], minlength=4).tolist(), nf, ev[:nf].mean(), st[nf:].tolist(), ev[nf:].tolist()))
    assert ev.max() <= steps + 1 and np.all(np.abs(h) <= np.float32(field["max_dist"]))
    hs, he, hh = st[nf:], ev[nf:], h[nf:]
    assert hs[6:11].tolist() == [3] * 5 and he[6:11].tolist() == [0] * 5 and not _bits(hh[6:11]).any() and not _bits(r[nf + 6:nf + 11]).any()
    # (a NaN or +inf coordinate gives no density; at -inf every tap is out of range and the density is the empty field's, finite:
    # the point then cannot move, as no point of its line is in the box)
    assert hs[12:14].tolist() == [3] * 2 and he[12:15].tolist() == [1] * 3 and not _bits(hh[12:15]).any() and hs[14] in (1, 2, 3)
    assert hs[5] != 3 and he[5] >= 1                             # a direction of length 3 is a direction
    if steps >= 1:
        # a point further outside the box than max_dist: whatever the first step is, it does not reach the box -- the point stays
        assert hs[:2].tolist() == [2, 2] and he[:2].tolist() == [1, 1] and not _bits(hh[:2]).any()
    if steps >= 3:
        assert len(np.unique(st[:nf])) >= 2 and ev[:nf].max() > 2      # the loop is really taken, unevenly


def test_the_residual_is_the_point_querys(field):
    from sculptmate_amd import ops

    nf = field["n_face"]
    pts, dirs = field["pts"][:nf], field["dirs"][:nf]
    h, r, st, _ = _along(ops, field, pts, dirs, 8)
    n = dirs / torch.sqrt((dirs[:, 0] * dirs[:, 0] + dirs[:, 1] * dirs[:, 1]) + dirs[:, 2] * dirs[:, 2])[:, None]
    q = pts + h[:, None] * n
    d = ops.triplane_query(field["planes"], field["mlp"], q.contiguous(), radius=RADIUS, want=("density",))["density"][:, 0]
    assert bool(torch.isfinite(d).all())
    assert _same(r, d - float(np.float32(field["target"])))
    assert bool((r[st == 0].abs() <= float(np.float32(RES_TOL))).all()) and bool(((st != 0) | (r.abs() <= float(np.float32(RES_TOL)))).all())


def test_a_point_depends_on_that_point_alone(field, reference):
    from sculptmate_amd import ops

    want = reference[8]
    N = field["pts"].shape[0]
    perm = torch.from_numpy(np.random.default_rng(3).permutation(N)).to(field["pts"].device)
    got = _along(ops, field, field["pts"][perm].contiguous(), field["dirs"][perm].contiguous(), 8)
    for a, b in zip(got, want):
        assert _same(a, b[perm])
    for n in (1, 7, 8, 9, 33):
        got = _along(ops, field, field["pts"][:n].contiguous(), field["dirs"][:n].contiguous(), 8)
        for a, b in zip(got, want):
            assert a.shape == (n,) and _same(a, b[:n])
    tail = slice(N - 33, N)                                   # the hostile points among them, as a leading shape [3, 11]
    got = _along(ops, field, field["pts"][tail].reshape(3, 11, 3), field["dirs"][tail].reshape(3, 11, 3), 8)
    for a, b in zip(got, want):
        assert a.shape == (3, 11) and _same(a.reshape(-1), b[tail])
    got = _along(ops, field, field["pts"], field["dirs"], 8, planes=field["planes_cf"])     # [3, C, H, W] planes
    for a, b in zip(got, want):
        assert _same(a, b)
    empty = _along(ops, field, field["pts"][:0], field["dirs"][:0], 8)
    assert all(x.shape == (0,) for x in empty)


def test_a_device_count_leaves_the_tail_untouched(field, reference):
    from sculptmate_amd import ops

    want = reference[8]
    N = field["pts"].shape[0]
    dev = field["pts"].device
    for count in (0, 1, 13, 1000, N, N + 5, -3):
        out = {"height": torch.full((N,), 7.5, device=dev), "residual": torch.full((N,), -2.5, device=dev),
               "status": torch.full((N,), 99, dtype=torch.int32, device=dev), "evals": torch.full((N,), 77, dtype=torch.int32, device=dev)}
        keep = {k: v.clone() for k, v in out.items()}
        got = _along(ops, field, field["pts"], field["dirs"], 8, count=torch.tensor([count], dtype=torch.int32, device=dev), out=out)
        n = min(max(count, 0), N)
        for name, a, b in zip(("height", "residual", "status", "evals"), got, want):
            assert _same(a[:n], b[:n]), (count, name)
            assert _same(a[n:], keep[name][n:]), (count, name)


def test_status_histogram_against_the_fp64_rule(field):
    """Set A's face points, 8 steps within 2 cells: the device's statuses are the fp64 rule's, except where an fp64 residual
    the rule compared with res_tol lies within E32d of it (either side of the test is then right in fp32)."""
    from sculptmate_amd import ops

    A, nf = field["A"], field["n_face"]
    p, n = D.face_points()
    ref = D.line_search(A["planes"], A["Ws"], A["bs"], p, n, A["target"], 8, field["max_dist"], RES_TOL, np.float64)
    _, _, st, ev = _along(ops, field, field["pts"][:nf], field["dirs"][:nf], 8)
    st = st.cpu().numpy()
    differ = st != ref["status"]
    borderline = ref["near"] <= E32D
    print("device status histogram %s, fp64 rule %s; %d points differ, %d points lie within E32d of res_tol, %d differ outside them; "
          "mean evals %.2f (fp64 %.2f)" % (np.bincount(st, minlength=4).tolist(), np.bincount(ref["status"], minlength=4).tolist(),
                                          differ.sum(), borderline.sum(), (differ & ~borderline).sum(), ev.float().mean(), ref["evals"].mean()))
    assert not (differ & ~borderline).any()
    assert (st == 0).mean() >= 0.9


# ---------------------------------------------------------------------------------------------- the texel list
@pytest.fixture(scope="module")
def scene(cuda):
    """The field and the octahedron atlases of tests/test_gpu_bake_surface.py, with per-vertex normals."""
    from sculptmate_amd import ops

    Ws, bs = synth.decoder_lists(synth.decoder_state(seed=1))
    mlp = ops.PackedMLP(Ws, bs, cuda)
    planes = ops.ChannelLastPlanes(torch.from_numpy(synth.triplane(seed=2, scale=4.0)).to(cuda))
    v_np, f_np = R.octahedron()
    v, f = torch.from_numpy(v_np).to(cuda), torch.from_numpy(f_np).to(cuda)
    uv, corner = ops.uv_cell_atlas(v, f)
    normals = ops.vertex_normals(v, f)
    rasts = {res: ops.bake_rasterize((uv * scale).contiguous(), corner, res) for res, scale in CASES}
    r37 = rasts[37]
    p37 = ops.bake_interpolate(v, r37, f)[r37[..., 3] >= 0]
    target = float(ops.field_normals(planes, mlp, p37, radius=RADIUS, want=("density",))["density"].median())
    return dict(mlp=mlp, planes=planes, v=v, f=f, normals=normals, rasts=rasts, target=target, max_dist=0.05)


def _hostile_rast(S):
    """tests/test_gpu_bake_surface.py's: tris past the face count, NaN, 2^31, inf; faces 6 and 7 name rows out of range."""
    rast = S["rasts"][37].clone()
    flat = rast.view(-1, 4)
    at = (flat[:, 3] >= 0).nonzero()[:, 0]
    for k, tri in enumerate((8.0, 1.0e6, float("nan"), 2147483648.0, float("inf"))):
        flat[at[k], 3] = tri
    f = S["f"].clone()
    f[6, 1] = S["v"].shape[0]
    f[7, 2] = -1
    return rast, f, (rast[..., 3] >= 0) & (rast[..., 3] < 6)


def _check_list(ops, S, rast, f, covered):
    got = ops.bake_texel_list(S["v"], f, rast, normals=S["normals"])
    idx = covered.reshape(-1).nonzero()[:, 0]
    n = int(got["count"].item())
    assert n == idx.numel() and got["count"].dtype == torch.int32 and got["list"].dtype == torch.int32
    assert torch.equal(got["list"][:n].long(), idx)
    assert torch.equal(got["mask"], covered)
    safe = torch.where(covered[..., None], rast, rast.new_tensor([0.0, 0.0, 0.0, -1.0])).contiguous()
    assert _same(got["p0"][:n], ops.bake_interpolate(S["v"], safe, f).reshape(-1, 3)[idx])
    assert _same(got["directions"][:n], ops.bake_interpolate(S["normals"], safe, f).reshape(-1, 3)[idx])
    return n


@pytest.mark.parametrize("res", [c[0] for c in CASES])
def test_texel_list_is_nonzero_of_the_coverage(scene, res):
    from sculptmate_amd import ops

    S, rast = scene, scene["rasts"][res]
    covered = rast[..., 3] >= 0
    rows = covered.any(1)
    if res == 64:
        assert int((~rows).sum()) > int(rows.sum()) > 0          # mostly empty rows
    if res == 256:
        assert res * res > 512 * 100                             # many blocks, several trips of the scan
    for dt in (torch.int32, torch.int64):
        n = _check_list(ops, S, rast, S["f"].to(dt), covered)
    print("res %d: %d covered texels of %d" % (res, n, res * res))
    assert 0 < n < res * res


def test_texel_list_with_a_rast_that_names_no_face_or_vertex(scene):
    from sculptmate_amd import ops

    S = scene
    rast, f, want_mask = _hostile_rast(S)
    assert int(((rast[..., 3] == 6) | (rast[..., 3] == 7)).sum()) > 0
    for dt in (torch.int32, torch.int64):
        _check_list(ops, S, rast, f.to(dt), want_mask)
    nothing = torch.zeros((37, 37, 4), dtype=torch.float32, device=rast.device)
    nothing[..., 3] = -1.0
    got = ops.bake_texel_list(S["v"], S["f"], nothing)
    assert int(got["count"].item()) == 0 and not got["mask"].any() and "directions" not in got
    everything = S["rasts"][37].clone()
    everything[..., :3] = 1.0 / 3.0
    everything[..., 3] = 2.0
    got = ops.bake_texel_list(S["v"], S["f"], everything)
    assert int(got["count"].item()) == 37 * 37 and torch.equal(got["list"].long(), torch.arange(37 * 37, device=rast.device))


# ---------------------------------------------------------------------------------------------- the two routes of the bake
def _assert_same_bake(got, want, what):
    for name, a, b in (("height", got[0], want[0]), ("mask", got[1], want[1])) + tuple((k, got[2][k], want[2][k]) for k in WANT):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name)
        assert _same(a, b), (what, name, int(torch.as_tensor(_bits(a) != _bits(b)).sum()))
    assert set(got[2]) == set(WANT) == set(want[2])


def _both(ops, S, rast, steps, faces=None, v=None, normals=None):
    args = (S["planes"], S["mlp"], S["v"] if v is None else v, S["f"] if faces is None else faces, S["normals"] if normals is None else normals,
            rast, S["target"], S["max_dist"])
    kw = dict(steps=steps, res_tol=RES_TOL, radius=RADIUS, want=WANT)
    return ops.bake_displacement(*args, **kw), ops.bake_displacement_composed(*args, **kw)


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("res", [c[0] for c in CASES])
def test_bake_displacement_equals_composed_bit_for_bit(scene, res, steps):
    from sculptmate_amd import ops

    S, rast = scene, scene["rasts"][res]
    covered = rast[..., 3] >= 0
    composed = None
    for dt in (torch.int32, torch.int64):
        listed, c = _both(ops, S, rast, steps, faces=S["f"].to(dt))
        composed = composed or c
        _assert_same_bake(listed, composed, (res, steps, dt))
    height, mask, ex = listed
    assert height.shape == (res, res) and mask.dtype == torch.bool and torch.equal(mask, covered) and int(covered.sum()) > 0
    off = ~covered
    assert not _bits(height[off]).any() and not _bits(ex["residual"][off]).any()          # +0
    assert bool((ex["status"][off] == -1).all()) and bool((ex["evals"][off] == 0).all())
    status = ex["status"][covered].cpu().numpy()
    print("res %d, steps %d: %d covered texels; status histogram %s, mean evals %.2f" % (
        res, steps, int(covered.sum()), np.bincount(status, minlength=4).tolist(), float(ex["evals"][covered].float().mean())))
    assert status.min() >= 0 and int(ex["evals"][covered].max()) <= steps + 1
    assert bool((height.abs() <= float(np.float32(S["max_dist"]))).all())


def test_bake_displacement_on_hostile_inputs(scene):
    """The rast that names no face or vertex; a vertex outside the box, one on its side, a non-finite one; a zero and a NaN
    vertex normal: both routes give the same bits."""
    from sculptmate_amd import ops

    S = scene
    rast, f, want_mask = _hostile_rast(S)
    for dt in (torch.int32, torch.int64):
        listed, composed = _both(ops, S, rast, 3, faces=f.to(dt))
        _assert_same_bake(listed, composed, ("guard", dt))
        assert torch.equal(listed[1], want_mask) and bool((listed[2]["status"][~want_mask] == -1).all())
    v = S["v"].clone()
    v[0] = torch.tensor([1.5, 0.0, 0.0])
    v[2] = torch.tensor([0.0, RADIUS, 0.0], dtype=torch.float32)
    v[5] = torch.tensor([0.0, 0.0, float("nan")])
    nrm = S["normals"].clone()
    nrm[1] = 0.0
    nrm[3] = float("nan")
    listed, composed = _both(ops, S, S["rasts"][37], 8, v=v, normals=nrm)
    _assert_same_bake(listed, composed, "hostile")
    covered = S["rasts"][37][..., 3] >= 0
    st = listed[2]["status"][covered].cpu().numpy()
    print("hostile: status histogram %s" % np.bincount(st, minlength=4).tolist())
    assert (st == 3).any() and (st != 3).any()
    nothing = torch.zeros((37, 37, 4), dtype=torch.float32, device=rast.device)
    nothing[..., 3] = -1.0
    for fn in (ops.bake_displacement, ops.bake_displacement_composed):
        height, mask, ex = fn(S["planes"], S["mlp"], S["v"], S["f"], S["normals"], nothing, S["target"], S["max_dist"], want=WANT)
        assert not _bits(height).any() and not mask.any() and bool((ex["status"] == -1).all()) and not ex["evals"].any()
        empty = fn(S["planes"], S["mlp"], S["v"], S["f"], S["normals"], torch.zeros((0, 0, 4), dtype=torch.float32, device=rast.device),
                   S["target"], S["max_dist"], want=WANT)
        assert empty[0].shape == (0, 0) and empty[1].shape == (0, 0) and empty[2]["status"].shape == (0, 0)


def test_a_texel_depends_on_that_texel_alone(scene):
    """Rows reversed, and the flat image rolled by 7: the same bits for every texel at its new place (the list then holds other
    neighbours, the tiles other companions with other step counts)."""
    from sculptmate_amd import ops

    S, res = scene, 37
    rast = S["rasts"][res]
    kw = dict(steps=8, res_tol=RES_TOL, radius=RADIUS, want=WANT)
    args = (S["planes"], S["mlp"], S["v"], S["f"], S["normals"])
    base = ops.bake_displacement(*args, rast, S["target"], S["max_dist"], **kw)
    flipped = ops.bake_displacement(*args, rast.flip(0).contiguous(), S["target"], S["max_dist"], **kw)
    rolled = ops.bake_displacement(*args, rast.reshape(-1, 4).roll(-7, 0).reshape(res, res, 4).contiguous(), S["target"], S["max_dist"], **kw)
    for name, a, b, c in [("height", base[0], flipped[0], rolled[0]), ("mask", base[1], flipped[1], rolled[1])] + [
            (k, base[2][k], flipped[2][k], rolled[2][k]) for k in WANT]:
        assert _same(b, a.flip(0)), name
        assert _same(c.reshape(-1), a.reshape(-1).roll(-7, 0)), name


# ---------------------------------------------------------------------------------------------- the simplified model mesh, TSR
@pytest.fixture(scope="module")
def model(cuda):
    from sculptmate_amd import ops
    from sculptmate_amd.tsr.system import Mesh

    out = _tsrmodel.small_model(cuda, 32, project_keys=True)
    m = out["m"]
    v, f = ops.mesh_simplify(out["plain"].vertices, out["plain"].faces, 0.25)[:2]
    out.update(low=Mesh(v, f), planes=m._field(out["codes"][0]))
    return out


def test_simplified_mesh_both_routes(model):
    from sculptmate_amd import ops

    m = model["m"]
    v, f, uv, rast = m._atlas(model["low"], 256, 0.02, None)
    normals = (m.WINDING_OUTWARD * ops.vertex_normals(v, f)).contiguous()
    args = (model["planes"], m.decoder, v, f, normals, rast, model["target"], 2.0 * model["cell"])
    kw = dict(steps=8, res_tol=RES_TOL, radius=model["radius"], want=WANT)
    listed = ops.bake_displacement(*args, **kw)
    _assert_same_bake(listed, ops.bake_displacement_composed(*args, **kw), "simplified")
    height, mask, ex = listed
    hist = np.bincount(ex["status"][mask].cpu().numpy(), minlength=4)
    start = ops.bake_displacement(*args, steps=0, res_tol=RES_TOL, radius=model["radius"], want=("residual",))[2]["residual"]
    r, r0 = ex["residual"][mask], start[mask]
    ok = torch.isfinite(r0)
    print("simplified mesh: %d faces, %d covered texels of %d; status histogram %s, mean evals %.2f; median |d - t| %.3e -> %.3e; "
          "median |h| %.3f cell" % (f.shape[0], int(mask.sum()), mask.numel(), hist.tolist(), float(ex["evals"][mask].float().mean()),
                                   float(r0[ok].abs().median()), float(r[ok].abs().median()), float(height[mask].abs().median()) / model["cell"]))
    assert torch.equal(mask, rast[..., 3] >= 0) and int(mask.sum()) > 1000
    assert bool((r[ok].abs() <= r0[ok].abs()).all())                                   # never worse than h = 0
    assert bool((height.abs() <= float(np.float32(2.0 * model["cell"]))).all())


def test_bake_displacement_map(model, monkeypatch):
    from sculptmate_amd import ops
    from sculptmate_amd.tsr.displacement import DisplacementMap

    m, code, low = model["m"], model["codes"][0], model["low"]
    res = 192                                        # 192 // 150 == 1: one round of padding
    kw = dict(threshold=model["threshold"], displacement=(8, 2.0), resolution=32)
    mesh, dm = m.bake_displacement_map(low, code, atlas_resolution=res, **kw)          # without uvs: unwrapped, returned with them
    assert isinstance(dm, DisplacementMap) and mesh is not low and mesh.uvs is not None and low.uvs is None
    assert mesh.vertices is low.vertices and mesh.faces is low.faces
    assert dm.height.shape == (res, res) and dm.height.dtype == torch.float32 and dm.mask.dtype == torch.bool
    assert dm.midlevel == 0.5 and dm.scale == 2 * dm.max_dist and abs(dm.max_dist - 2.0 * model["cell"]) < 1e-12
    # by hand: the composed route, +0 where not converged, one round of padding
    v, f, uv, rast = m._atlas(mesh, res, 0.02, None, keep_uvs=True)
    normals = (m.WINDING_OUTWARD * ops.vertex_normals(v, f)).contiguous()
    height, mask, ex = ops.bake_displacement_composed(model["planes"], m.decoder, v, f, normals, rast, model["target"], dm.max_dist,
                                                      steps=8, radius=model["radius"], want=WANT)
    kept = torch.where(ex["status"] == 0, height, torch.zeros_like(height))
    assert not _bits(kept[~mask]).any() and not _bits(kept[mask & (ex["status"] != 0)]).any()      # +0 before the padding
    assert int((mask & (ex["status"] != 0)).sum()) > 0 and int((kept != 0).sum()) > 0
    padded = m._padded(kept[..., None].expand(res, res, 3), mask, res)[..., 0]
    assert _same(dm.height, padded) and torch.equal(dm.mask, mask) and torch.equal(dm.status, ex["status"])
    assert _same(dm.height[mask], kept[mask])                                          # the padding leaves the charts alone
    textured = m.bake_texture(low, code, texture_resolution=res)                       # with uvs: kept, the texture's resolution
    same_mesh, dm2 = m.bake_displacement_map(textured, code, **kw)
    assert same_mesh is textured and dm2.height.shape == (res, res)
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", "composeddisplacement")                 # the same call through the other route
    assert ops.bake_displacement_route() is ops.bake_displacement_composed
    _, dm3 = m.bake_displacement_map(mesh, code, **kw, atlas_resolution=res)
    monkeypatch.delenv("SCULPT_DISTANCE_FORM")
    assert _same(dm3.height, dm.height) and torch.equal(dm3.status, dm.status)
    info = dm.info()
    print("displacement map: %s" % info)
    assert info["covered"] == int(mask.sum()) and sum(info["status"].values()) == info["covered"]
    assert info["median_abs_residual_after"] <= info["median_abs_residual_before"] and 1.0 <= info["evals_per_texel"] <= 9.0
    assert dm.image().dtype == np.uint16


def test_extract_meshes_with_and_without_displacement_map(model, monkeypatch):
    from sculptmate_amd import ops

    m = model["m"]
    kw = dict(enable_texture=True, bake_texture=64, simplify=0.25, **model["kw"])
    assert m.displacement_map is None

    def refuse(*a, **k):
        raise AssertionError("the displacement bake was called although TSR.displacement_map is None")

    with monkeypatch.context() as mp:
        for name in ("bake_displacement", "bake_displacement_composed", "project_along", "bake_texel_list"):
            mp.setattr(ops, name, refuse)
        first = m.extract_meshes(model["codes"], **kw)[0]
    assert not hasattr(first, "displacement")
    try:
        m.displacement_map = True
        second = m.extract_meshes(model["codes"], **kw)[0]
    finally:
        m.displacement_map = None
    for key in ("vertices", "uvs", "texture"):
        assert _same(getattr(first, key), getattr(second, key)), key
    assert torch.equal(first.faces, second.faces)
    dm = second.displacement
    _, want = m.bake_displacement_map(first, model["codes"][0], threshold=model["threshold"], displacement=True, resolution=32)
    assert dm.height.shape == (64, 64) and _same(dm.height, want.height) and torch.equal(dm.status, want.status)
    after = m.extract_meshes(model["codes"], **kw)[0]
    assert _same(after.texture, first.texture) and not hasattr(after, "displacement")
