"""The bake at the surface on the GPU: sculpt_bake_scene_surface (csrc/bake_surface.hip) against the composed route it fuses --
ops.bake_interpolate, ops.project_to_isosurface, ops.field_normals and the frame transform, ops.bake_scene_surface_composed --
bit for bit in every output and both spaces, the guarantees of the rule exactly, and the surface built on it
(TSR.bake_surface_maps, TSR.bake_project).  Float outputs are compared as 32-bit words, so a NaN's payload and a -0 count."""
import numpy as np
import pytest
import torch

import _nmapref as R
import _tsrmodel
from sculptmate_amd import synth

pytestmark = pytest.mark.gpu

RADIUS = 0.87
RES_TOL = 1e-3
WANT = ("residual", "status", "evals")
# (resolution, scale of the UVs): the spans of tests/test_gpu_bake_normal.py.  5: one partial span.  37: a ragged last span.  64 with
# the charts scaled into a corner: most spans empty, covered counts that are no multiple of the 8 points of a tile.  256: spans
# of several tiles, up to all 8.
CASES = [(5, 1.0), (37, 1.0), (64, 0.25), (256, 1.0)]
STEPS = [0, 1, 3, 8]


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _assert_same_bake(got, want, what):
    """(point, normal, mask, extras) of two routes: every output, bit for bit."""
    for name, a, b in (("point", got[0], want[0]), ("normal", got[1], want[1]), ("mask", got[2], want[2])) + tuple(
            (k, got[3][k], want[3][k]) for k in WANT):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name)
        assert _same(a, b), (what, name, int((torch.as_tensor(_bits(a) != _bits(b))).sum()))
    assert set(got[3]) == set(WANT) == set(want[3])


def _span_counts(mask):
    m = mask.reshape(-1).to(torch.int32)
    return torch.cat([m, m.new_zeros(-m.numel() % 64)]).view(-1, 64).sum(1).cpu().numpy()


def _frame(ops, v, f, uv):
    cn = ops.vertex_normals(v, f)[f.reshape(-1)].contiguous()
    return cn, ops.corner_tangents(v, f, uv, cn)


@pytest.fixture(scope="module")
def scene(cuda):
    """The field of the normal-bake tests (decoder seed 1, synth.triplane(seed=2, scale=4.0)), the octahedron with its cell atlas
    and frame, the rasterised atlas of every case, and a target that the octahedron's texels straddle: the median raw density at
    the covered texels of the 37^2 atlas (an input; nothing is tuned to the kernel).  max_dist: a tenth of the octahedron's arm."""
    from sculptmate_amd import ops

    Ws, bs = synth.decoder_lists(synth.decoder_state(seed=1))
    mlp = ops.PackedMLP(Ws, bs, cuda)
    planes = ops.ChannelLastPlanes(torch.from_numpy(synth.triplane(seed=2, scale=4.0)).to(cuda))
    v_np, f_np = R.octahedron()
    v, f = torch.from_numpy(v_np).to(cuda), torch.from_numpy(f_np).to(cuda)
    uv, corner = ops.uv_cell_atlas(v, f)
    cn, ct = _frame(ops, v, f, uv)
    rasts = {res: ops.bake_rasterize((uv * scale).contiguous(), corner, res) for res, scale in CASES}
    r37 = rasts[37]
    p37 = ops.bake_interpolate(v, r37, f)[r37[..., 3] >= 0]
    target = float(ops.field_normals(planes, mlp, p37, radius=RADIUS, want=("density",))["density"].median())
    return dict(mlp=mlp, planes=planes, v=v, f=f, uv=uv, corner=corner, cn=cn, ct=ct, rasts=rasts, target=target, max_dist=0.05)


def _both(ops, S, rast, steps, frame, faces=None, v=None):
    args = (S["planes"], S["mlp"], S["v"] if v is None else v, S["f"] if faces is None else faces, rast, S["target"], S["max_dist"])
    kw = dict(steps=steps, res_tol=RES_TOL, radius=RADIUS, frame=frame, want=WANT)
    return ops.bake_scene_surface(*args, **kw), ops.bake_scene_surface_composed(*args, **kw)


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("res", [c[0] for c in CASES])
def test_fused_equals_composed_bit_for_bit(scene, res, steps):
    from sculptmate_amd import ops

    S, rast = scene, scene["rasts"][res]
    covered = rast[..., 3] >= 0
    counts = _span_counts(covered)
    if res == 5:
        assert len(counts) == 1 and 0 < counts[0] < 25
    if res == 37:
        assert (37 * 37) % 64 == 25
    if res == 64:
        assert (counts == 0).sum() > (counts > 0).sum() > 0 and (counts[counts > 0] % 8 != 0).all()
    if res == 256:
        assert counts.max() > 56 and (counts == 0).any()
    for frame in (None, (S["cn"], S["ct"])):
        composed = None
        for dt in (torch.int32, torch.int64):
            fused, c = _both(ops, S, rast, steps, frame, faces=S["f"].to(dt))
            composed = composed or c
            _assert_same_bake(fused, composed, (res, steps, "tangent" if frame else "object", dt))
        point, normal, mask, ex = fused
        assert point.shape == (res, res, 3) and normal.shape == (res, res, 3) and mask.shape == (res, res) and mask.dtype == torch.bool
        assert ex["residual"].dtype == torch.float32 and ex["status"].dtype == torch.int32 and ex["evals"].dtype == torch.int32
        assert torch.equal(mask, covered) and int(covered.sum()) > 0
    status = ex["status"][covered].cpu().numpy()
    print("res %d, steps %d: %d covered texels in %d spans (%d empty, up to %d tiles); status histogram %s, mean evals %.2f" % (
        res, steps, int(covered.sum()), len(counts), int((counts == 0).sum()), -(-int(counts.max()) // 8),
        np.bincount(status, minlength=4).tolist(), float(ex["evals"][covered].float().mean())))
    assert status.min() >= 0 and int(ex["evals"][covered].min()) >= 1 and int(ex["evals"][covered].max()) <= steps + 1
    if steps == 8 and res >= 37:
        assert len(np.unique(status)) >= 2 and int(ex["evals"][covered].max()) > 2        # the loop is really taken, unevenly


def test_steps_0_is_the_plain_normal_bake(scene):
    from sculptmate_amd import ops

    S = scene
    for res in (37, 256):
        rast = S["rasts"][res]
        pos = ops.bake_interpolate(S["v"], rast, S["f"])
        covered = rast[..., 3] >= 0
        for frame in (None, (S["cn"], S["ct"])):
            point, normal, mask, ex = ops.bake_scene_surface(S["planes"], S["mlp"], S["v"], S["f"], rast, S["target"], S["max_dist"], steps=0,
                                                             radius=RADIUS, frame=frame, want=WANT)
            plain, pmask = ops.bake_scene_normal(S["planes"], S["mlp"], S["v"], S["f"], rast, radius=RADIUS, frame=frame)
            assert _same(normal, plain) and torch.equal(mask, pmask)
            assert _same(point[covered], pos[covered]) and bool((ex["evals"][covered] == 1).all())
            assert set(np.unique(ex["status"][covered].cpu().numpy())) <= {0, 1}


def test_the_residual_is_the_point_querys(scene):
    from sculptmate_amd import ops

    S, rast = scene, scene["rasts"][256]
    point, _, mask, ex = ops.bake_scene_surface(S["planes"], S["mlp"], S["v"], S["f"], rast, S["target"], S["max_dist"], steps=8,
                                                res_tol=RES_TOL, radius=RADIUS, want=("residual",))
    d = ops.triplane_query(S["planes"], S["mlp"], point[mask], radius=RADIUS, want=("density",))["density"][:, 0]
    assert bool(torch.isfinite(d).all())
    assert _same(ex["residual"][mask], d - S["target"])


def test_a_texel_depends_on_that_texel_alone(scene):
    """Rows reversed, and the flat image rolled by 7: the same bits for every texel at its new place, in every output and both
    spaces (the spans then hold other neighbours and other ranks, the tiles other companions with other step counts)."""
    from sculptmate_amd import ops

    S, res = scene, 37
    rast = S["rasts"][res]
    for frame in (None, (S["cn"], S["ct"])):
        kw = dict(steps=8, res_tol=RES_TOL, radius=RADIUS, frame=frame, want=WANT)
        args = (S["planes"], S["mlp"], S["v"], S["f"])
        base = ops.bake_scene_surface(*args, rast, S["target"], S["max_dist"], **kw)
        flipped = ops.bake_scene_surface(*args, rast.flip(0).contiguous(), S["target"], S["max_dist"], **kw)
        rolled = ops.bake_scene_surface(*args, rast.reshape(-1, 4).roll(-7, 0).reshape(res, res, 4).contiguous(), S["target"],
                                        S["max_dist"], **kw)
        for name, a, b, c in [("point", base[0], flipped[0], rolled[0]), ("normal", base[1], flipped[1], rolled[1]),
                              ("mask", base[2], flipped[2], rolled[2])] + [(k, base[3][k], flipped[3][k], rolled[3][k]) for k in WANT]:
            w = a.shape[2:]
            assert _same(b, a.flip(0)), name
            assert _same(c.reshape(-1, *w), a.reshape(-1, *w).roll(-7, 0)), name


def test_uncovered_texels(scene):
    from sculptmate_amd import ops

    S = scene
    for res in (64, 37):
        rast = S["rasts"][res]
        for frame in (None, (S["cn"], S["ct"])):
            point, normal, mask, ex = ops.bake_scene_surface(S["planes"], S["mlp"], S["v"], S["f"], rast, S["target"], S["max_dist"],
                                                             steps=8, radius=RADIUS, frame=frame, want=WANT)
            off = ~(rast[..., 3] >= 0)
            assert torch.equal(mask, ~off) and bool(off.any())
            assert not _bits(point[off]).any() and not _bits(normal[off]).any() and not _bits(ex["residual"][off]).any()    # +0
            assert bool((ex["status"][off] == -1).all()) and bool((ex["evals"][off] == 0).all())
    nothing = torch.zeros((37, 37, 4), dtype=torch.float32, device=rast.device)
    nothing[..., 3] = -1.0
    for fn in (ops.bake_scene_surface, ops.bake_scene_surface_composed):
        point, normal, mask, ex = fn(S["planes"], S["mlp"], S["v"], S["f"], nothing, S["target"], S["max_dist"], want=WANT)
        assert not _bits(point).any() and not _bits(normal).any() and not mask.any() and bool((ex["status"] == -1).all())
        empty = fn(S["planes"], S["mlp"], S["v"], S["f"], torch.zeros((0, 0, 4), dtype=torch.float32, device=rast.device), S["target"],
                   S["max_dist"], want=WANT)
        assert empty[0].shape == (0, 0, 3) and empty[2].shape == (0, 0) and empty[3]["status"].shape == (0, 0)


def test_hostile_vertices(scene):
    """One vertex outside the box (the texels near it have |x| > radius: x is frozen and keeps p0's bits), one with a coordinate
    exactly +radius and one exactly -radius, and one non-finite (every texel of its faces: status 3, the point keeps p0's bits):
    everything still equals the composed route.  No texel centre of the atlas sits on a chart corner, so six covered texels are
    rewritten to the barycentrics of the corner that names the vertex on the box: their p0 is (0, +-radius, 0) exactly, |y| ==
    radius, the equality case of the frozen-axis test."""
    from sculptmate_amd import ops

    S, res = scene, 37
    rast = S["rasts"][res].clone()
    flat = rast.view(-1, 4)
    # face 0 = (0, 2, 4) and face 2 = (1, 3, 4) name the vertex on the box second, face 1 = (2, 1, 4) names it first
    for face, bary in ((0, (0.0, 1.0, 0.0)), (2, (0.0, 1.0, 0.0)), (1, (1.0, 0.0, 0.0))):
        at = (flat[:, 3] == face).nonzero()[:2, 0]
        assert at.numel() == 2
        flat[at] = torch.tensor([*bary, float(face)], device=rast.device)
    covered = rast[..., 3] >= 0
    v = S["v"].clone()
    v[0] = torch.tensor([1.5, 0.0, 0.0])                      # outside the box
    v[2] = torch.tensor([0.0, RADIUS, 0.0], dtype=torch.float32)                   # on a face of the box
    v[3] = torch.tensor([0.0, -RADIUS, 0.0], dtype=torch.float32)
    v[5] = torch.tensor([0.0, 0.0, float("nan")])
    rad32 = float(np.float32(RADIUS))
    for frame in (None, (S["cn"], S["ct"])):
        fused, composed = _both(ops, S, rast, 8, frame, v=v)
        _assert_same_bake(fused, composed, ("hostile", "tangent" if frame else "object"))
    point, normal, mask, ex = fused
    p0 = ops.bake_interpolate(v, rast, S["f"])
    tri = rast[..., 3].long().clamp(min=0)
    nan_face = covered & (S["f"][tri] == 5).any(-1) & ~torch.isfinite(p0).all(-1)
    assert int(nan_face.sum()) > 0
    assert bool((ex["status"][nan_face] == 3).all()) and _same(point[nan_face], p0[nan_face]) and bool((ex["evals"][nan_face] == 1).all())
    beyond = covered & (p0[..., 0].abs() > rad32)
    on_face = covered & (p0[..., 1].abs() == rad32)
    assert int(beyond.sum()) > 0 and int(on_face.sum()) == 6
    assert int((p0[..., 1][on_face] == rad32).sum()) == 4 and int((p0[..., 1][on_face] == -rad32).sum()) == 2
    assert _same(point[..., 0][beyond], p0[..., 0][beyond])
    assert _same(point[..., 1][on_face], p0[..., 1][on_face])                      # |y| == radius is frozen: the bits of p0
    for axis in range(3):
        frozen = covered & (p0[..., axis].abs() >= rad32) & torch.isfinite(p0).all(-1)
        assert _same(point[..., axis][frozen], p0[..., axis][frozen])
    print("hostile: %d texels with a non-finite point, %d with |y| exactly the radius (status %s, evals %s), %d with |x| beyond it; "
          "status histogram %s" % (int(nan_face.sum()), int(on_face.sum()), ex["status"][on_face].tolist(), ex["evals"][on_face].tolist(),
                                   int(beyond.sum()), np.bincount(ex["status"][covered].cpu().numpy(), minlength=4).tolist()))


def test_a_face_in_the_side_of_the_box(scene):
    """Face 0 with all three vertices at y = radius: the interpolation (radius u + radius v) + radius w gives radius exactly on
    some texels, an ulp above on some and below on others; the texels at or above are frozen in y, take steps in x and z (the
    trust radius is larger than the box here, so no first step is cut off) and keep y's bits; those below are free.  All equal
    the composed route, which freezes through project_kernel's own test."""
    from sculptmate_amd import ops

    S = scene
    rast = S["rasts"][256]
    rad32 = float(np.float32(RADIUS))
    v = S["v"].clone()
    v[[0, 2, 4], 1] = rad32
    args = (S["planes"], S["mlp"], v, S["f"], rast, S["target"], 4.0)
    kw = dict(steps=8, res_tol=RES_TOL, radius=RADIUS, want=WANT)
    for frame in (None, (S["cn"], S["ct"])):
        fused = ops.bake_scene_surface(*args, frame=frame, **kw)
        _assert_same_bake(fused, ops.bake_scene_surface_composed(*args, frame=frame, **kw), ("side", "tangent" if frame else "object"))
    point, _, mask, ex = fused
    p0 = ops.bake_interpolate(v, rast, S["f"])
    y = p0[..., 1]
    on_face, above, below = mask & (y == rad32), mask & (y > rad32), mask & (rast[..., 3] == 0) & (y < rad32)
    frozen = on_face | above
    print("side of the box: %d texels with y exactly the radius, %d above, %d of the face below; of the frozen ones %d took a step, "
          "status histogram %s" % (int(on_face.sum()), int(above.sum()), int(below.sum()), int((ex["evals"][frozen] > 1).sum()),
                                   np.bincount(ex["status"][frozen].cpu().numpy(), minlength=4).tolist()))
    assert int(on_face.sum()) > 0
    assert _same(point[..., 1][frozen], y[frozen])
    took = frozen & (ex["evals"] > 1)
    assert int((took & on_face).sum()) > 0                        # the equality case took a step, and y stayed
    assert bool(((point[..., 0][took] != p0[..., 0][took]) | (point[..., 2][took] != p0[..., 2][took])).any())


def test_rast_that_names_no_face_or_vertex(scene):
    """The index guard of bake_scene_color_kernel in both routes: a tri at or past the face count, a NaN tri, 2^31, and a face
    whose vertex row is out of range (negative, or past the vertex count) count as not covered; nothing is read through them."""
    from sculptmate_amd import ops

    S, res = scene, 37
    rast = S["rasts"][res].clone()
    flat = rast.view(-1, 4)
    at = (flat[:, 3] >= 0).nonzero()[:, 0]
    for k, tri in enumerate((8.0, 1.0e6, float("nan"), 2147483648.0, float("inf"))):
        flat[at[k], 3] = tri
    f = S["f"].clone()
    f[6, 1] = S["v"].shape[0]                                     # face 6 names a row past the end
    f[7, 2] = -1                                                  # face 7 a negative one
    bad = (rast[..., 3] == 6) | (rast[..., 3] == 7)
    want_mask = (rast[..., 3] >= 0) & (rast[..., 3] < 6)
    assert int(bad.sum()) > 0
    for dt in (torch.int32, torch.int64):
        for frame in (None, (S["cn"], S["ct"])):
            fused, composed = _both(ops, S, rast, 3, frame, faces=f.to(dt))
            _assert_same_bake(fused, composed, ("guard", dt))
            assert torch.equal(fused[2], want_mask)
            off = ~want_mask
            assert not _bits(fused[0][off]).any() and not _bits(fused[1][off]).any() and bool((fused[3]["status"][off] == -1).all())


def test_a_view_of_a_larger_image_is_copied(scene):
    """rast as a non-contiguous view: taken as _bake_scene_args takes it for the other bakes, by a copy."""
    from sculptmate_amd import ops

    S, res = scene, 37
    rast = S["rasts"][res]
    wide = torch.zeros((res, 2 * res, 4), dtype=torch.float32, device=rast.device)
    wide[:, ::2] = rast
    view = wide[:, ::2]
    assert not view.is_contiguous()
    for fn in (ops.bake_scene_surface, ops.bake_scene_surface_composed):
        _assert_same_bake(fn(S["planes"], S["mlp"], S["v"], S["f"], view, S["target"], S["max_dist"], want=WANT),
                          fn(S["planes"], S["mlp"], S["v"], S["f"], rast, S["target"], S["max_dist"], want=WANT), "view")


# ---------------------------------------------------------------------------------------------- the simplified model mesh
@pytest.fixture(scope="module")
def model(cuda):
    """The shared small model at resolution 32, its mesh after ops.mesh_simplify(0.25) with the model's own atlas at 256^2, the
    bake at the surface with max_dist = 2 cells by both routes and the steps = 0 bake beside it (computed once, never modified)."""
    from sculptmate_amd import ops
    from sculptmate_amd.tsr.system import Mesh

    out = _tsrmodel.small_model(cuda, 32, project_keys=True)
    m, code = out["m"], out["codes"][0]
    v, f = ops.mesh_simplify(out["plain"].vertices, out["plain"].faces, 0.25)[:2]
    low = Mesh(v, f)
    v, f, uv, rast = m._atlas(low, 256, 0.02, None)
    cn = (m.WINDING_OUTWARD * ops.vertex_normals(v, f))[f.reshape(-1).long()].contiguous()
    ct = ops.corner_tangents(v, f, uv, cn)
    planes = m._field(code)
    args = (planes, m.decoder, v, f, rast, out["target"], 2.0 * out["cell"])
    kw = dict(res_tol=RES_TOL, radius=out["radius"], want=WANT)
    out.update(low=low, v=v, f=f, uv=uv, rast=rast, cn=cn, ct=ct, planes=planes, args=args, bake_kw=kw,
               fused={sp: ops.bake_scene_surface(*args, steps=8, frame=fr, **kw) for sp, fr in (("object", None), ("tangent", (cn, ct)))},
               start=ops.bake_scene_surface(*args, steps=0, **kw))
    return out


@pytest.mark.parametrize("space", ["object", "tangent"])
def test_simplified_mesh_fused_equals_composed(model, space):
    from sculptmate_amd import ops

    frame = (model["cn"], model["ct"]) if space == "tangent" else None
    composed = ops.bake_scene_surface_composed(*model["args"], steps=8, frame=frame, **model["bake_kw"])
    _assert_same_bake(model["fused"][space], composed, ("simplified", space))
    point, normal, mask, ex = model["fused"][space]
    status = ex["status"][mask].cpu().numpy()
    hist = np.bincount(status, minlength=4)
    print("simplified mesh, %s: %d faces, %d covered texels of %d; status histogram %s, mean evals %.2f" % (
        space, model["f"].shape[0], int(mask.sum()), mask.numel(), hist.tolist(), float(ex["evals"][mask].float().mean())))
    assert torch.equal(mask, model["rast"][..., 3] >= 0) and int(mask.sum()) > 1000
    assert hist[0] > hist[1:].sum()                  # near-surface texels: mostly converged


def test_rule_guarantees_exactly(model):
    """Per covered texel, in the rule's own fp32 arithmetic: never worse than the start, status 0 only within res_tol, never
    outside the trust region."""
    point, _, mask, ex = model["fused"]["object"]
    p0, _, mask0, ex0 = model["start"]
    assert torch.equal(mask, mask0)
    r, r0 = ex["residual"][mask], ex0["residual"][mask]
    ok = torch.isfinite(r0)
    assert bool((r[ok].abs() <= r0[ok].abs()).all())
    tol = float(np.float32(RES_TOL))
    assert bool((r[ex["status"][mask] == 0].abs() <= tol).all())
    assert bool(((ex["status"][mask] != 0) | (r.abs() <= tol)).all())
    dl = point[mask] - p0[mask]
    sq = dl * dl
    d2 = sq[:, 0] + sq[:, 1]
    d2 = d2 + sq[:, 2]
    md = np.float32(model["args"][6])
    assert bool((d2[ok] <= float(md * md)).all())
    moved = d2[ok].sqrt() / model["cell"]
    print("simplified mesh: median |d - t| %.3e -> %.3e; displacement median %.3f cell, largest %.3f cell" % (
        float(r0[ok].abs().median()), float(r[ok].abs().median()), float(moved.median()), float(moved.max())))


# ---------------------------------------------------------------------------------------------- TSR
def _maps_by_hand(model, space, res, mesh):
    """TSR.bake_surface_maps(project=(8, 2.0)) assembled from ops.bake_scene_surface_composed and the padding that was there."""
    from sculptmate_amd import ops

    m = model["m"]
    v, f, uv, rast = m._atlas(mesh, res, 0.02, None, keep_uvs=True)
    cn = (m.WINDING_OUTWARD * ops.vertex_normals(v, f))[f.reshape(-1).long()].contiguous()
    ct = ops.corner_tangents(v, f, uv, cn)
    point, n, mask, _ = ops.bake_scene_surface_composed(model["planes"], m.decoder, v, f, rast, model["target"], 2.0 * model["cell"], steps=8,
                                                        radius=model["radius"], frame=(cn, ct) if space == "tangent" else None)
    color = torch.zeros_like(point)
    color[mask] = ops.triplane_query(model["planes"], m.decoder, point[mask], radius=model["radius"],
                                     density_bias=m.renderer.cfg.density_bias, want=("color",))["color"]
    texture = m._padded(color, mask, res)
    coded = m._padded(torch.where(mask[..., None], 0.5 + 0.5 * n, torch.zeros_like(n)), mask, res)
    flat = torch.tensor(m.NORMAL_MAP_FLAT[space], dtype=torch.float32, device=coded.device)
    return uv, texture, torch.where((coded != 0).any(-1, keepdim=True), coded, flat), cn, ct


@pytest.mark.parametrize("space", ["tangent", "object"])
def test_bake_surface_maps_equals_the_maps_assembled_by_hand(model, space, monkeypatch):
    m, code = model["m"], model["codes"][0]
    res = 192                                       # 192 // 150 == 1: one round of padding
    textured = m.bake_texture(model["low"], code, texture_resolution=res)         # a mesh that has uvs keeps them
    got = m.bake_surface_maps(textured, code, threshold=model["threshold"], project=(8, 2.0), resolution=32, normal_map=space)
    uv, texture, normal_map, cn, ct = _maps_by_hand(model, space, res, textured)
    assert got.vertices is textured.vertices and got.faces is textured.faces and got.uvs is textured.uvs and got.vertex_colors is None
    assert got.texture.shape == (res, res, 3) and got.normal_map.shape == (res, res, 3) and got.normal_map_space == space
    assert _same(got.texture, texture) and _same(got.normal_map, normal_map)
    assert _same(got.corner_normals, cn) and _same(got.corner_tangents, ct)
    assert not _same(got.texture, textured.texture)                                # the projection changes the texture
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", "fusedsurface")                     # the same call through the fused kernel
    fused = m.bake_surface_maps(textured, code, threshold=model["threshold"], project=(8, 2.0), resolution=32, normal_map=space)
    monkeypatch.delenv("SCULPT_DISTANCE_FORM")
    assert _same(fused.texture, texture) and _same(fused.normal_map, normal_map)
    only_normals = m.bake_surface_maps(textured, code, threshold=model["threshold"], project=(8, 2.0), resolution=32, texture=False,
                                       normal_map=space)
    assert only_normals.texture is textured.texture and _same(only_normals.normal_map, normal_map)
    only_texture = m.bake_surface_maps(textured, code, threshold=model["threshold"], project=(8, 2.0), resolution=32, normal_map=None)
    assert only_texture.normal_map is None and only_texture.corner_tangents is None and _same(only_texture.texture, texture)


def test_extract_meshes_with_and_without_bake_project(model, monkeypatch):
    from sculptmate_amd import ops

    m = model["m"]
    kw = dict(enable_texture=True, bake_texture=64, simplify=0.25, **model["kw"])
    assert m.bake_project is None and m.normal_map is None
    # None: the fused op is never called, and the maps are those of a second plain call

    def refuse(*a, **k):
        raise AssertionError("ops.bake_scene_surface called although TSR.bake_project is None")

    with monkeypatch.context() as mp:
        mp.setattr(ops, "bake_scene_surface", refuse)
        mp.setattr(ops, "bake_scene_surface_composed", refuse)
        m.normal_map = "tangent"
        try:
            first = m.extract_meshes(model["codes"], **kw)[0]
            second = m.extract_meshes(model["codes"], **kw)[0]
        finally:
            m.normal_map = None
    for key in ("vertices", "uvs", "texture", "normal_map", "corner_normals", "corner_tangents"):
        assert _same(getattr(first, key), getattr(second, key)), key
    # True: the result is bake_surface_maps on the same mesh
    geometry = m.extract_meshes(model["codes"], simplify=0.25, **model["kw"])[0]
    assert _same(geometry.vertices, first.vertices) and torch.equal(geometry.faces, first.faces)
    try:
        m.bake_project = True
        m.normal_map = "tangent"
        both = m.extract_meshes(model["codes"], **kw)[0]
        m.normal_map = None
        texture_only = m.extract_meshes(model["codes"], **kw)[0]
    finally:
        m.bake_project = None
        m.normal_map = None
    want = m.bake_surface_maps(geometry, model["codes"][0], threshold=model["threshold"], project=True, resolution=32, atlas_resolution=64,
                               normal_map="tangent")
    for key in ("vertices", "uvs", "texture", "normal_map", "corner_normals", "corner_tangents"):
        assert _same(getattr(both, key), getattr(want, key)), key
    assert both.normal_map_space == "tangent" and both.vertex_colors is None
    assert texture_only.normal_map is None and _same(texture_only.texture, want.texture)
    assert not _same(both.texture, first.texture)
    after = m.extract_meshes(model["codes"], **kw)[0]
    assert _same(after.texture, first.texture) and after.normal_map is None
