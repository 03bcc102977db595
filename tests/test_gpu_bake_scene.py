"""Texture bake of a TripoSR scene code: sculpt_bake_scene_color (csrc/bake_scene.hip) against the composed route it fuses --
ops.bake_interpolate followed by ops.triplane_query on channel-last planes -- bit for bit, against the CPU oracle within the point
query's own tolerance, and the surface built on it (ops.bake_scene_color, TSR.bake_texture, extract_meshes(bake_texture=),
TripoGenerator.bake_texture_resolution)."""
import numpy as np
import pytest
import torch

import _tsrmodel
from oracle import capi
from sculptmate_amd import synth

pytestmark = pytest.mark.gpu

RADIUS = 0.87
RTOL, ATOL = 3e-5, 3e-5     # what tests/test_gpu_triplane.py applies to `color` against the same oracle
# (resolution, scale of the UVs).  5: 25 texels, one partial tile.  37: 1369 texels, the last tile has 25 live lanes.  64 with the
# charts scaled into one corner: most tiles empty, the rest mixed.  A cell of the octahedron's 3 x 3 atlas is at most 21 texels
# wide there, so no tile of 32 consecutive texels can be full at 64; 256 unscaled (a cell is 85 texels wide) is the smallest
# power of two at which full tiles occur beside empty and mixed ones.
CASES = [(5, 1.0), (37, 1.0), (64, 0.25), (256, 1.0)]


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)


def _tile_kinds(mask):
    """Covered texels per tile of 32 consecutive texels -> (n_empty, n_mixed, n_full)."""
    m = mask.reshape(-1).to(torch.int32)
    m = torch.cat([m, m.new_zeros(-m.numel() % 32)]).view(-1, 32).sum(1)
    live = torch.full_like(m, 32)
    live[-1] = 32 - (-mask.numel() % 32)
    return int((m == 0).sum()), int(((m > 0) & (m < live)).sum()), int((m == live).sum())


@pytest.fixture(scope="module")
def scene(cuda):
    """Planes, decoder, the octahedron with its cell atlas and, per case, the rasterised atlas, the composed route's result
    (computed once, never modified) and the fused kernel's result with int32 and int64 faces."""
    from sculptmate_amd import ops

    tri_np = synth.triplane(seed=2, scale=4.0)
    Ws, bs = synth.decoder_lists(synth.decoder_state(seed=1))
    mlp = ops.PackedMLP(Ws, bs, cuda)
    planes = ops.ChannelLastPlanes(torch.from_numpy(tri_np).to(cuda))
    v = torch.tensor([[0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0], [0, -0.5, 0], [0, 0, 0.5], [0, 0, -0.5]], dtype=torch.float32, device=cuda)
    f = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=torch.int64, device=cuda)
    uv, corner = ops.uv_cell_atlas(v, f)
    cases = {}
    for res, scale in CASES:
        rast = ops.bake_rasterize((uv * scale).contiguous(), corner, res)
        pos = ops.bake_interpolate(v[f].reshape(-1, 3), rast, corner)
        ref = ops.triplane_query(planes, mlp, pos, radius=RADIUS, want=("color",))["color"]
        got = {dt: ops.bake_scene_color(planes, mlp, v, f.to(dt), rast, radius=RADIUS) for dt in (torch.int32, torch.int64)}
        cases[res] = dict(rast=rast, pos=pos, ref=ref, got=got, covered=rast[..., 3] >= 0)
    return dict(tri_np=tri_np, Ws=Ws, bs=bs, mlp=mlp, planes=planes, v=v, f=f, cases=cases)


@pytest.mark.parametrize("faces_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("res", [c[0] for c in CASES])
def test_covered_texels_equal_the_composed_route_bit_for_bit(scene, res, faces_dtype):
    c = scene["cases"][res]
    color, mask = c["got"][faces_dtype]
    covered = c["covered"]
    assert color.shape == (res, res, 3) and color.dtype == torch.float32 and mask.shape == (res, res) and mask.dtype == torch.bool
    assert torch.equal(mask, covered) and int(covered.sum()) > 0
    empty, mixed, full = _tile_kinds(covered)
    print("res %d: %d texels, %d covered; tiles: %d empty, %d mixed, %d full" % (res, res * res, int(covered.sum()), empty, mixed, full))
    if res == 64:
        assert empty > mixed > 0 and full == 0      # most tiles empty, some mixed (see CASES for why none can be full here)
    if res == 256:
        assert empty > 0 and mixed > 0 and full > 0
    if res == 37:
        assert (res * res) % 32 == 25
    assert np.array_equal(_bits(color[covered]), _bits(c["ref"][covered]))
    assert not _bits(color[~covered]).any()        # exactly +0, not the composed route's colour of the box centre


def test_a_texel_depends_on_that_texel_alone(scene):
    """Rows reversed, and the first 7 texels rolled to the end of the flat image: the same bits for every texel at its new
    place (the tiles then hold other neighbours, and the last, partial tile holds texels that sat in full ones)."""
    from sculptmate_amd import ops

    res = 37
    c = scene["cases"][res]
    color, mask = c["got"][torch.int64]
    flipped = c["rast"].flip(0).contiguous()
    col2, mask2 = ops.bake_scene_color(scene["planes"], scene["mlp"], scene["v"], scene["f"], flipped, radius=RADIUS)
    assert np.array_equal(_bits(col2), _bits(color.flip(0))) and torch.equal(mask2, mask.flip(0))
    rolled = c["rast"].reshape(-1, 4).roll(-7, 0).reshape(res, res, 4).contiguous()
    col3, mask3 = ops.bake_scene_color(scene["planes"], scene["mlp"], scene["v"], scene["f"], rolled, radius=RADIUS)
    assert np.array_equal(_bits(col3.reshape(-1, 3)), _bits(color.reshape(-1, 3).roll(-7, 0)))
    assert torch.equal(mask3.reshape(-1), mask.reshape(-1).roll(-7, 0))


def test_colour_against_the_cpu_oracle(scene):
    c = scene["cases"][37]
    covered = c["covered"].cpu().numpy()
    pts = c["pos"].cpu().numpy()[covered]
    ref = capi.query_triplane(scene["tri_np"], pts, scene["Ws"], scene["bs"])["color"]
    got = c["got"][torch.int64][0].cpu().numpy()[covered]
    print("max |color - oracle| over %d texels: %.3g" % (len(pts), np.abs(got - ref).max()))
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)


def test_refusals_and_the_empty_image(scene, cuda):
    from sculptmate_amd import ops

    p, mlp, v, f = scene["planes"], scene["mlp"], scene["v"], scene["f"]
    rast = scene["cases"][5]["rast"]
    with pytest.raises(ops.SculptError):
        ops.bake_scene_color(p, mlp, v.cpu(), f, rast)
    with pytest.raises(ops.SculptError):
        ops.bake_scene_color(p, mlp, v, f.cpu(), rast)
    with pytest.raises(ops.SculptError):
        ops.bake_scene_color(p, mlp, v, f, rast.cpu())
    with pytest.raises(ops.SculptError):
        ops.bake_scene_color(p, mlp, v, f, rast[..., :3].contiguous())
    with pytest.raises(ops.SculptError):
        ops.bake_scene_color(p, mlp, v, f, rast[:4].contiguous())
    with pytest.raises(ops.SculptError):
        ops.bake_scene_color(p, mlp, v, f.to(torch.float32), rast)
    nothing = torch.zeros((37, 37, 4), dtype=torch.float32, device=cuda)
    nothing[..., 3] = -1.0
    color, mask = ops.bake_scene_color(p, mlp, v, f, nothing)
    assert color.shape == (37, 37, 3) and not _bits(color).any() and not mask.any()
    color, mask = ops.bake_scene_color(p, mlp, v, f, torch.zeros((0, 0, 4), dtype=torch.float32, device=cuda))
    assert color.shape == (0, 0, 3) and mask.shape == (0, 0)


@pytest.fixture(scope="module")
def model(cuda):
    """The shared small model at resolution 32; the plain mesh carries vertex colours."""
    return _tsrmodel.small_model(cuda, 32, enable_texture=True)


def _dilate(mask, steps):
    for _ in range(steps):
        mask = torch.nn.functional.max_pool2d(mask[None, None].float(), 3, 1, 1)[0, 0] > 0
    return mask


@pytest.mark.parametrize("res", [64, 300])
def test_model_surface_default_unwrapper(model, res):
    """extract_meshes(bake_texture=res) through the box-projection unwrapper; 300 is the smallest resolution with two rounds of
    padding (res // 150)."""
    from sculptmate_amd import ops

    m, plain = model["m"], model["plain"]
    baked = m.extract_meshes(model["codes"], enable_texture=True, resolution=32, threshold=model["threshold"], bake_texture=res)[0]
    assert np.array_equal(_bits(baked.vertices), _bits(plain.vertices)) and torch.equal(baked.faces, plain.faces)
    nf = baked.faces.shape[0]
    assert baked.vertex_colors is None and plain.vertex_colors is not None and plain.texture is None and plain.uvs is None
    assert baked.uvs.shape == (3 * nf, 2) and baked.uvs.dtype == torch.float32
    assert float(baked.uvs.min()) >= 0.0 and float(baked.uvs.max()) <= 1.0
    t = baked.texture
    assert t.shape == (res, res, 3) and t.dtype == torch.float32 and t.is_cuda
    assert bool(torch.isfinite(t).all()) and float(t.min()) >= 0.0 and float(t.max()) <= 1.0
    rast = ops.bake_rasterize(baked.uvs, torch.arange(3 * nf, device=t.device, dtype=torch.int32).view(-1, 3), res)
    covered = rast[..., 3] >= 0
    share = float(covered.float().mean())
    print("res %d: covered share of the atlas %.3f" % (res, share))
    assert share > 0.0
    color, mask = ops.bake_scene_color(model["codes"][0], m.decoder, baked.vertices, baked.faces, rast, radius=m.renderer.cfg.radius)
    assert torch.equal(mask, covered)
    # a sigmoid of a finite feature is above zero: wherever the covered colour is non-zero, so is every texel the padding reaches
    assert bool((color[covered] > 0).all())
    reach = _dilate(covered, res // 150)
    assert bool((t[reach] > 0).all())
    assert np.array_equal(_bits(t[covered]), _bits(color[covered]))     # padding leaves covered texels alone
    if res // 150 == 0:
        assert np.array_equal(_bits(t), _bits(color))
    else:
        assert int(reach.sum()) > int(covered.sum())


def test_model_surface_without_baking_is_unchanged(model):
    m, plain = model["m"], model["plain"]
    again = m.extract_meshes(model["codes"], enable_texture=True, resolution=32, threshold=model["threshold"], bake_texture=0)[0]
    want = m.renderer.query_triplane(m.decoder, plain.vertices, model["codes"][0].contiguous())["color"]
    assert np.array_equal(_bits(again.vertex_colors), _bits(want)) and np.array_equal(_bits(plain.vertex_colors), _bits(want))
    assert again.texture is None and again.uvs is None
    # bake_texture without enable_texture: geometry only, as before
    bare = m.extract_meshes(model["codes"], enable_texture=False, resolution=32, threshold=model["threshold"], bake_texture=64)[0]
    assert bare.vertex_colors is None and bare.texture is None and torch.equal(bare.faces, plain.faces)


def test_model_surface_cell_atlas_equals_the_op_by_hand(model):
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d.bake import cell_atlas_unwrapper

    m, plain = model["m"], model["plain"]
    baked = m.bake_texture(plain, model["codes"][0], texture_resolution=64, unwrapper=cell_atlas_unwrapper)
    uv, corner = ops.uv_cell_atlas(plain.vertices, plain.faces, padding=0.05)
    assert np.array_equal(_bits(baked.uvs), _bits(uv))
    rast = ops.bake_rasterize(uv, corner, 64)
    color, _ = ops.bake_scene_color(model["codes"][0], m.decoder, plain.vertices, plain.faces, rast, radius=m.renderer.cfg.radius)
    assert 64 // 150 == 0 and np.array_equal(_bits(baked.texture), _bits(color))
    assert baked.vertices is plain.vertices and baked.faces is plain.faces and baked.vertex_colors is None
    picture = baked.texture_image()
    assert picture.size == (64, 64) and picture.mode == "RGB"
    assert np.array_equal(np.asarray(picture), np.clip(np.floor(256.0 * color.cpu().numpy()), 0, 255).astype(np.uint8))


def test_generator_bakes_when_the_attribute_is_set(cuda, tmp_path):
    import types

    from test_host_logic import _write_checkpoint

    from sculptmate_amd import ops
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr.spec import SMALL_CFG

    _write_checkpoint(str(tmp_path), SMALL_CFG, seed=61)
    g = TripoGenerator(cuda)
    assert g.bake_texture_resolution == 0
    g.checkpoint_dir = str(tmp_path)
    g.mc_resolution = 32
    assert g.initiate_model() == 0
    plain, baked = [], []
    g.model.mesh_sink = lambda v, f, c, name: plain.append((v, f, c, name))
    g.model.textured_mesh_sink = lambda v, f, uv, image, name: baked.append((v, f, uv, image, name))
    orig = g.model.extract_mesh

    def reachable(self, codes, **kw):   # random weights never reach the default threshold: take the grid's median
        return orig(codes, **dict(kw, threshold=float(ops.density_grid(codes[0].contiguous(), self.decoder, kw["resolution"]).median())))

    g.model.extract_mesh = types.MethodType(reachable, g.model)
    img = (synth.composite_rgb(synth.image_rgba(seed=62, size=SMALL_CFG["cond_image_size"])) * 255).astype(np.uint8)
    g.bake_texture_resolution = 64
    assert g.generate_mesh(img, "baked", enable_texture=True) == 0
    mesh = g.last_meshes[0]
    assert mesh.texture is not None and mesh.texture.shape == (64, 64, 3) and mesh.vertex_colors is None
    assert len(baked) == 1 and not plain
    v, f, uv, image, name = baked[0]
    assert name == "baked" and v.dtype == np.float32 and f.dtype == np.int64 and uv.shape == (f.size, 2) and image.size == (64, 64)
    g.bake_texture_resolution = 0
    assert g.generate_mesh(img, "coloured", enable_texture=True) == 0
    assert g.last_meshes[0].texture is None and g.last_meshes[0].vertex_colors is not None and len(plain) == 1 and len(baked) == 1
