"""Normal-map bake of a TripoSR scene code on the GPU: sculpt_bake_scene_normal and sculpt_corner_tangents
(csrc/bake_normal.hip) against the composed route the bake fuses -- ops.bake_interpolate followed by ops.field_normals -- bit for
bit, against the fp32 NumPy restatement of the frame rules (tests/_nmapref.py) bit for bit, and the surface built on them
(ops.bake_scene_normal, ops.corner_tangents, TSR.bake_normal_map, TSR.normal_map, TripoGenerator.normal_map).  The restatement's
own distance from fp64 is what tests/test_bake_normal_host.py prints (about 1.3e-07 per component)."""
import math

import numpy as np
import pytest
import torch

import _nmapref as R
import _tsrmodel
from sculptmate_amd import synth

pytestmark = pytest.mark.gpu

RADIUS = 0.87
# (resolution, scale of the UVs): the cases of tests/test_gpu_bake_scene.py, seen in spans of 64 consecutive texels, the unit a
# wave of bake_scene_normal_kernel owns.  5: 25 texels, one partial span.  37: 1369 texels, the last span has 25 live texels.
# 64 with the charts scaled into one corner: most spans empty, and covered counts that are no multiple of the 8 points of a tile.
# 256: spans of every count up to 8 tiles' worth -- but none FULL: a cell of the octahedron's 3 x 3 atlas is 85 texels wide and
# its padded chart at most 77, and no chart's widest row contains a whole 64-aligned span of its image row (the charts start at
# x = 4, 90 and 175).  512 (a chart up to 154 texels wide) is the smallest power of two at which full spans occur, and is here
# for that.
CASES = [(5, 1.0), (37, 1.0), (64, 0.25), (256, 1.0), (512, 1.0)]
MIRRORED, FLATTENED = 3, 5


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)


def _span_counts(mask):
    """Covered texels per span of 64 consecutive texels -> (counts, live texels per span)."""
    m = mask.reshape(-1).to(torch.int32)
    counts = torch.cat([m, m.new_zeros(-m.numel() % 64)]).view(-1, 64).sum(1)
    live = torch.full_like(counts, 64)
    live[-1] = 64 - (-mask.numel() % 64)
    return counts.cpu().numpy(), live.cpu().numpy()


def _frame(ops, v, f, uv):
    cn = ops.vertex_normals(v, f)[f.reshape(-1)].contiguous()
    return cn, ops.corner_tangents(v, f, uv, cn)


@pytest.fixture(scope="module")
def scene(cuda):
    """Planes, decoder, the octahedron with its cell atlas and frame and, per case, the rasterised atlas, the composed route's
    world normals (computed once, never modified) and the fused kernel's results."""
    from sculptmate_amd import ops

    tri_np = synth.triplane(seed=2, scale=4.0)
    Ws, bs = synth.decoder_lists(synth.decoder_state(seed=1))
    mlp = ops.PackedMLP(Ws, bs, cuda)
    planes = ops.ChannelLastPlanes(torch.from_numpy(tri_np).to(cuda))
    v_np, f_np = R.octahedron()
    v, f = torch.from_numpy(v_np).to(cuda), torch.from_numpy(f_np).to(cuda)
    uv, corner = ops.uv_cell_atlas(v, f)
    cn, ct = _frame(ops, v, f, uv)
    cases = {}
    for res, scale in CASES:
        rast = ops.bake_rasterize((uv * scale).contiguous(), corner, res)
        pos = ops.bake_interpolate(v[f].reshape(-1, 3), rast, corner)
        ref = ops.field_normals(planes, mlp, pos, radius=RADIUS)["normal"]
        world = {dt: ops.bake_scene_normal(planes, mlp, v, f.to(dt), rast, radius=RADIUS) for dt in (torch.int32, torch.int64)}
        tangent = ops.bake_scene_normal(planes, mlp, v, f, rast, radius=RADIUS, frame=(cn, ct))
        cases[res] = dict(rast=rast, ref=ref, world=world, tangent=tangent, covered=rast[..., 3] >= 0)
    return dict(mlp=mlp, planes=planes, v=v, f=f, uv=uv, cn=cn, ct=ct, cases=cases)


@pytest.mark.parametrize("faces_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("res", [c[0] for c in CASES])
def test_world_normals_equal_the_composed_route_bit_for_bit(scene, res, faces_dtype):
    c = scene["cases"][res]
    normal, mask = c["world"][faces_dtype]
    covered = c["covered"]
    assert normal.shape == (res, res, 3) and normal.dtype == torch.float32 and mask.shape == (res, res) and mask.dtype == torch.bool
    assert torch.equal(mask, covered) and int(covered.sum()) > 0
    counts, live = _span_counts(covered)
    empty, full = int((counts == 0).sum()), int((counts == live).sum())
    mixed = len(counts) - empty - full
    print("res %d: %d texels, %d covered; spans: %d empty, %d mixed, %d full; tiles per span up to %d, %d spans with a count that "
          "is no multiple of 8" % (res, res * res, int(covered.sum()), empty, mixed, full, -(-int(counts.max()) // 8),
                                    int((counts % 8 != 0).sum())))
    if res == 5:
        assert len(counts) == 1 and live[0] == 25 and 0 < counts[0] < 25
    if res == 37:
        assert live[-1] == 25
    if res == 64:
        assert empty > mixed > 0 and (counts % 8 != 0).any()
    if res == 256:
        assert empty > 0 and mixed > 0 and counts.max() > 56         # spans that run all 8 tiles (none is full: see CASES)
    if res == 512:
        assert empty > 0 and mixed > 0 and full > 0
    assert np.array_equal(_bits(normal[covered]), _bits(c["ref"][covered]))
    assert not _bits(normal[~covered]).any()        # exactly +0, not the composed route's normal at the box centre
    length = normal[covered].double().norm(dim=1)
    assert float((length - 1).abs().max()) <= 4 * 2.0 ** -24


def test_a_texel_depends_on_that_texel_alone(scene):
    """Rows reversed, and the first 7 texels rolled to the end of the flat image: the same bits for every texel at its new
    place, in both spaces (the spans then hold other neighbours and other ranks, and the last, partial span other texels)."""
    from sculptmate_amd import ops

    res = 37
    c = scene["cases"][res]
    for frame, (normal, mask) in ((None, c["world"][torch.int64]), ((scene["cn"], scene["ct"]), c["tangent"])):
        flipped = c["rast"].flip(0).contiguous()
        n2, m2 = ops.bake_scene_normal(scene["planes"], scene["mlp"], scene["v"], scene["f"], flipped, radius=RADIUS, frame=frame)
        assert np.array_equal(_bits(n2), _bits(normal.flip(0))) and torch.equal(m2, mask.flip(0))
        rolled = c["rast"].reshape(-1, 4).roll(-7, 0).reshape(res, res, 4).contiguous()
        n3, m3 = ops.bake_scene_normal(scene["planes"], scene["mlp"], scene["v"], scene["f"], rolled, radius=RADIUS, frame=frame)
        assert np.array_equal(_bits(n3.reshape(-1, 3)), _bits(normal.reshape(-1, 3).roll(-7, 0)))
        assert torch.equal(m3.reshape(-1), mask.reshape(-1).roll(-7, 0))


def _check_tangent_space(rast, world, tangent, cn, ct):
    """The tangent-space output against the restatement fed the kernel's own world normals -> smallest D over covered texels."""
    covered = (rast[..., 3] >= 0).cpu().numpy()
    r = rast.cpu().numpy()[covered]
    want, D = R.texel_transform(world.cpu().numpy()[covered], r[:, :3], r[:, 3].astype(np.int64), cn.cpu().numpy(), ct.cpu().numpy())
    got = tangent.cpu().numpy()
    assert np.array_equal(_bits(got[covered]), _bits(want))
    assert not _bits(got[~covered]).any()
    return float(D.min())


@pytest.mark.parametrize("res", [c[0] for c in CASES])
def test_tangent_space_equals_the_restatement_bit_for_bit(scene, res):
    c = scene["cases"][res]
    tangent, mask = c["tangent"]
    assert torch.equal(mask, c["covered"])
    dmin = _check_tangent_space(c["rast"], c["world"][torch.int64][0], tangent, scene["cn"], scene["ct"])
    print("res %d: smallest D over covered texels %.3g" % (res, dmin))
    assert dmin >= 0.01      # the condition of the host test, on the rasteriser's own barycentrics: no texel takes the flat fallback
    # and the stored vector decodes to the world normal (fp64), within 4 x what the restatement itself shows (host test)
    covered = c["covered"].cpu().numpy()
    r = c["rast"].cpu().numpy()[covered]
    back = R.decode(tangent.cpu().numpy()[covered], r[:, :3], r[:, 3].astype(np.int64), scene["cn"].cpu().numpy(), scene["ct"].cpu().numpy())
    assert R.angle(back, c["world"][torch.int64][0].cpu().numpy()[covered]).max() <= 4 * 1.6e-07


def test_corner_tangents_equal_the_restatement_bit_for_bit(scene, cuda):
    """The octahedron with the device's cell atlas; the icosphere with one chart mirrored in u (w = -1) and one without UV area
    (the fallback, w = +1), int32 and int64 faces; and the tangent-space bake over that atlas."""
    from sculptmate_amd import ops

    v, f, uv, cn = scene["v"], scene["f"], scene["uv"], scene["cn"]
    assert np.array_equal(_bits(scene["ct"]), _bits(R.corner_tangents(v.cpu().numpy(), f.cpu().numpy(), uv.cpu().numpy(), cn.cpu().numpy())))
    P, F = R.icosphere(1)
    uvs = R.zero_area_chart(R.mirror_chart(R.cell_atlas(P, F), MIRRORED), FLATTENED)
    v, f, uv = torch.from_numpy(P).to(cuda), torch.from_numpy(F).to(cuda), torch.from_numpy(uvs).to(cuda)
    cn = ops.vertex_normals(v, f)[f.reshape(-1)].contiguous()
    want = R.corner_tangents(P, F, uvs, cn.cpu().numpy())
    for dt in (torch.int32, torch.int64):
        got = ops.corner_tangents(v, f.to(dt), uv, cn)
        assert got.shape == (3 * len(F), 4) and got.dtype == torch.float32
        assert np.array_equal(_bits(got), _bits(want))
    w = got.cpu().numpy().reshape(-1, 3, 4)[:, :, 3]
    assert (w[MIRRORED] == -1).all() and (np.delete(w, MIRRORED, 0) == 1).all()
    res = 96
    rast = ops.bake_rasterize(uv, torch.arange(3 * len(F), device=cuda, dtype=torch.int32).view(-1, 3), res)
    tris = rast[..., 3][rast[..., 3] >= 0].long().unique().cpu().numpy()
    assert MIRRORED in tris and FLATTENED not in tris           # a chart without area covers no texel
    world, _ = ops.bake_scene_normal(scene["planes"], scene["mlp"], v, f, rast, radius=RADIUS)
    tangent, _ = ops.bake_scene_normal(scene["planes"], scene["mlp"], v, f, rast, radius=RADIUS, frame=(cn, got))
    assert _check_tangent_space(rast, world, tangent, cn, got) >= 0.01
    # the dedicated degenerate frame: a tangent that is the normal has D = 0 -> every covered texel stores the flat (0, 0, 1)
    bad = torch.cat([cn, torch.ones_like(cn[:, :1])], 1).contiguous()
    flat, mask = ops.bake_scene_normal(scene["planes"], scene["mlp"], v, f, rast, radius=RADIUS, frame=(cn, bad))
    assert _check_tangent_space(rast, world, flat, cn, bad) <= 0
    assert bool((flat[mask] == torch.tensor([0.0, 0.0, 1.0], device=cuda)).all())


def test_refusals_and_the_empty_image(scene, cuda):
    from sculptmate_amd import ops

    p, mlp, v, f, cn, ct = scene["planes"], scene["mlp"], scene["v"], scene["f"], scene["cn"], scene["ct"]
    rast = scene["cases"][5]["rast"]
    for bad in ((cn[:-1].contiguous(), ct), (cn, ct[:-1].contiguous()), (cn, ct[:, :3].contiguous()), (cn.double(), ct), (cn, ct.half()),
                (cn.cpu(), ct), (cn,), cn):
        with pytest.raises(ops.SculptError):
            ops.bake_scene_normal(p, mlp, v, f, rast, frame=bad)
    wide = torch.zeros((5, 10, 4), dtype=torch.float32, device=cuda)
    with pytest.raises(ops.SculptError, match="contiguous"):
        ops.bake_scene_normal(p, mlp, v, f, wide[:, ::2])
    for args in ((v.cpu(), f, rast), (v, f.cpu(), rast), (v, f, rast.cpu()), (v, f, rast[..., :3].contiguous()), (v, f, rast[:4].contiguous()),
                 (v, f.to(torch.float32), rast)):
        with pytest.raises(ops.SculptError):
            ops.bake_scene_normal(p, mlp, *args)
    with pytest.raises(ops.SculptError):
        ops.corner_tangents(v, f, scene["uv"][:-1].contiguous(), cn)
    with pytest.raises(ops.SculptError):
        ops.corner_tangents(v, f, scene["uv"], cn.double())
    nothing = torch.zeros((37, 37, 4), dtype=torch.float32, device=cuda)
    nothing[..., 3] = -1.0
    for frame in (None, (cn, ct)):
        normal, mask = ops.bake_scene_normal(p, mlp, v, f, nothing, frame=frame)
        assert normal.shape == (37, 37, 3) and not _bits(normal).any() and not mask.any()
        normal, mask = ops.bake_scene_normal(p, mlp, v, f, torch.zeros((0, 0, 4), dtype=torch.float32, device=cuda), frame=frame)
        assert normal.shape == (0, 0, 3) and mask.shape == (0, 0) and mask.dtype == torch.bool


# ---------------------------------------------------------------------------------------------- the model surface
@pytest.fixture(scope="module")
def model(cuda):
    """The shared small model at resolution 32, its plain mesh (vertex colours), that mesh baked at 64 and the normal maps."""
    out = _tsrmodel.small_model(cuda, 32, enable_texture=True)
    m, code = out["m"], out["codes"][0]
    out["baked"] = m.bake_texture(out["plain"], code, texture_resolution=64)
    out["maps"] = {(name, space): m.bake_normal_map(out[name], code, resolution=64 if name == "plain" else None, space=space)
                   for name in ("plain", "baked") for space in ("tangent", "object")}
    return out


@pytest.mark.parametrize("space", ["tangent", "object"])
@pytest.mark.parametrize("name", ["plain", "baked"])
def test_bake_normal_map(model, name, space):
    from sculptmate_amd import ops

    src, got = model[name], model["maps"][(name, space)]
    nf = src.faces.shape[0]
    assert got.vertices is src.vertices and got.faces is src.faces and got.texture is src.texture and got.vertex_colors is src.vertex_colors
    if name == "baked":
        assert got.uvs is src.uvs                                   # the atlas of the texture, untouched
    else:
        assert src.uvs is None and got.uvs.shape == (3 * nf, 2)
    nm = got.normal_map
    assert nm.shape == (64, 64, 3) and nm.dtype == torch.float32 and nm.is_cuda and got.normal_map_space == space
    assert got.corner_normals.shape == (3 * nf, 3) and got.corner_tangents.shape == (3 * nf, 4)
    assert bool(((got.corner_tangents[:, 3] == 1) | (got.corner_tangents[:, 3] == -1)).all())
    rast = ops.bake_rasterize(got.uvs, torch.arange(3 * nf, device=nm.device, dtype=torch.int32).view(-1, 3), 64)
    covered = rast[..., 3] >= 0
    assert 0 < int(covered.sum()) < 64 * 64
    flat = torch.tensor((0.5, 0.5, 1.0) if space == "tangent" else (0.5, 0.5, 0.5), device=nm.device)
    assert 64 // 150 == 0 and bool((nm[~covered] == flat).all())    # no round of padding at 64: every uncovered texel is flat
    n, mask = ops.bake_scene_normal(model["codes"][0], model["m"].decoder, got.vertices, got.faces, rast, radius=model["m"].renderer.cfg.radius,
                                    frame=(got.corner_normals, got.corner_tangents) if space == "tangent" else None)
    assert torch.equal(mask, covered) and np.array_equal(_bits(nm[covered]), _bits((0.5 + 0.5 * n)[covered]))
    # every covered texel of the 8-bit picture decodes to unit length within the quantisation step: floor(256 x) is at most
    # half a step (0.5 / 256) from its bin's centre, a step of n is twice that, and there are three components
    img = torch.from_numpy(np.asarray(got.normal_map_image()).astype(np.float64)).to(nm.device)
    length = (2.0 * (img[covered] + 0.5) / 256.0 - 1.0).norm(dim=1)
    worst = float((length - 1).abs().max())
    print("%s, %s: covered %d texels; |decoded 8-bit normal| - 1 at most %.4f" % (name, space, int(covered.sum()), worst))
    assert worst <= math.sqrt(3.0) / 256.0 + 1e-6
    assert float(((nm[covered].double() * 2 - 1).norm(dim=1) - 1).abs().max()) <= 8 * 2.0 ** -24      # and the fp32 map itself


def test_extract_meshes_adds_the_map_when_the_model_asks(model):
    m = model["m"]
    kw = dict(enable_texture=True, resolution=32, threshold=model["threshold"], bake_texture=64)
    assert m.normal_map is None
    before = m.extract_meshes(model["codes"], **kw)[0]
    try:
        m.normal_map = "tangent"
        mapped = m.extract_meshes(model["codes"], **kw)[0]
        bare = m.extract_meshes(model["codes"], **dict(kw, bake_texture=0))[0]       # no bake, no atlas: no map
    finally:
        m.normal_map = None
    after = m.extract_meshes(model["codes"], **kw)[0]
    assert mapped.normal_map is not None and mapped.normal_map.shape == (64, 64, 3) and mapped.normal_map_space == "tangent"
    assert bare.normal_map is None and bare.vertex_colors is not None
    for x in (before, after):
        assert x.normal_map is None and x.normal_map_space is None and x.corner_normals is None and x.corner_tangents is None
        assert torch.equal(x.faces, mapped.faces) and x.vertex_colors is None and mapped.vertex_colors is None
        for key in ("vertices", "uvs", "texture"):
            assert np.array_equal(_bits(getattr(x, key)), _bits(getattr(mapped, key))), key
    assert np.array_equal(_bits(before.texture), _bits(model["baked"].texture)) and np.array_equal(_bits(before.uvs), _bits(model["baked"].uvs))
    again = model["maps"][("baked", "tangent")]
    assert np.array_equal(_bits(mapped.normal_map), _bits(again.normal_map))


def test_generator_normal_map_reaches_last_meshes(cuda, tmp_path):
    import types

    from test_host_logic import _write_checkpoint

    from sculptmate_amd import ops
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr.spec import SMALL_CFG

    _write_checkpoint(str(tmp_path), SMALL_CFG, seed=61)
    g = TripoGenerator(cuda)
    assert g.normal_map is None
    g.checkpoint_dir = str(tmp_path)
    g.mc_resolution = 32
    assert g.initiate_model() == 0
    calls = []
    g.model.textured_mesh_sink = lambda v, f, uv, image, name, **kw: calls.append(kw)
    orig = g.model.extract_mesh

    def reachable(self, codes, **kw):   # random weights never reach the default threshold: take the grid's median
        return orig(codes, **dict(kw, threshold=float(ops.density_grid(codes[0].contiguous(), self.decoder, kw["resolution"]).median())))

    g.model.extract_mesh = types.MethodType(reachable, g.model)
    img = (synth.composite_rgb(synth.image_rgba(seed=62, size=SMALL_CFG["cond_image_size"])) * 255).astype(np.uint8)
    g.bake_texture_resolution = 64
    g.normal_map = "tangent"
    assert g.generate_mesh(img, "mapped", enable_texture=True) == 0
    mesh = g.last_meshes[0]
    assert g.model.normal_map == "tangent" and mesh.normal_map is not None and mesh.normal_map.shape == (64, 64, 3)
    assert len(calls) == 1 and calls[0]["normal_image"].size == (64, 64)
    g.normal_map = None
    assert g.generate_mesh(img, "plain", enable_texture=True) == 0
    assert g.last_meshes[0].normal_map is None and g.last_meshes[0].texture is not None and calls[1] == {}
