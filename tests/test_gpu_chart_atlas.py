"""The UV chart atlas on the device (csrc/uv_charts.hip, sf3d.unwrap.ChartUnwrapper) against its NumPy restatement
(tests/_chartref.py), bit for bit, on small meshes at R = 256; and the `atlas` setting through TSR and TripoGenerator."""
import numpy as np
import pytest
import torch

import _chartref as cr

pytestmark = pytest.mark.gpu

R = 256
NAMES = ["cube", "icosphere", "nested", "torus", "helicoid", "soup", "one_face", "degenerate", "three_on_an_edge", "same_direction",
         "tall", "mc32"]


@pytest.fixture(scope="module")
def model(cuda):
    from _tsrmodel import small_model

    return small_model(cuda, 32)


def _mesh(name, model):
    if name == "mc32":   # the marching-cubes mesh of the 32^3 test model: noisy, many layers, many components
        plain = model["plain"]
        return (np.ascontiguousarray(torch.as_tensor(plain.vertices).cpu().numpy(), np.float32),
                torch.as_tensor(plain.faces).cpu().numpy().astype(np.int64))
    return cr.mesh(name)


def _reference(name, model):
    if name == "mc32":
        return cr.reference(name, *_mesh(name, model))
    return cr.reference(name)


def _run(cuda, v, f, dtype):
    from sculptmate_amd.sf3d.unwrap import ChartUnwrapper

    un = ChartUnwrapper(raster_resolution=R)
    vt = torch.from_numpy(np.array(v)).to(cuda)
    ft = torch.from_numpy(np.array(f)).to(cuda).to(dtype)
    uv, idx = un(vt, torch.zeros_like(vt), ft, 0.02)
    return un, uv, idx


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_restatement_bit_for_bit(cuda, model, name, dtype):
    v, f = _mesh(name, model)
    ref = _reference(name, model)
    un, uv, idx = _run(cuda, v, f, dtype)
    last = un.last
    print("%s: %d faces, %d charts, %d rows, scale %.6g, rounds %d, evicted %s, conflicts %d, %d scale evaluations"
          % (name, len(f), last["n_charts"], last["rows"], last["scale"], last["rounds"], last["evicted"], last["conflicts"],
             last["evaluations"]))
    assert idx.dtype == dtype and idx.shape == (len(f), 3)
    assert np.array_equal(idx.cpu().numpy().reshape(-1), np.arange(3 * len(f)))
    assert uv.dtype == torch.float32 and uv.shape == (3 * len(f), 2)
    assert last["evicted"] == ref["evicted"] and last["rounds"] == ref["rounds"] and last["conflicts"] == ref["conflicts"]
    assert last["n_charts"] == ref["n_charts"] and last["rows"] == ref["rows"]
    assert np.array_equal(last["direction"].cpu().numpy(), ref["direction"])
    assert np.array_equal(last["layer"].cpu().numpy(), ref["layer"])
    assert np.array_equal(last["chart"].cpu().numpy(), ref["chart"])
    assert np.array_equal(_bits(last["rect"].cpu().numpy()), _bits(ref["rect"]))
    assert np.array_equal(_bits(last["extent"].cpu().numpy()), _bits(ref["extent"]))
    assert np.array_equal(last["cell"].cpu().numpy(), ref["cell"])
    assert np.float64(last["scale"]).view(np.uint64) == np.float64(ref["scale"]).view(np.uint64)
    assert np.array_equal(_bits(uv.cpu().numpy()), _bits(ref["uv"]))


@pytest.mark.parametrize("name", ["helicoid", "soup", "mc32"])
def test_two_calls_give_the_same_bits(cuda, model, name):
    v, f = _mesh(name, model)
    a, uva, _ = _run(cuda, v, f, torch.int32)
    b, uvb, _ = _run(cuda, v, f, torch.int32)
    assert torch.equal(uva.view(torch.int32), uvb.view(torch.int32))
    assert torch.equal(a.last["chart"], b.last["chart"]) and torch.equal(a.last["layer"], b.last["layer"])
    assert a.last["evicted"] == b.last["evicted"] and a.last["scale"] == b.last["scale"]


def test_refusals_and_the_empty_mesh(cuda):
    from sculptmate_amd._lib import SculptError
    from sculptmate_amd.sf3d.unwrap import ChartUnwrapper

    un = ChartUnwrapper(raster_resolution=R)
    v, f = cr.mesh("cube")
    vt, ft = torch.from_numpy(np.array(v)).to(cuda), torch.from_numpy(np.array(f)).to(cuda)
    uv, idx = un(vt, vt, ft[:0], 0.02)
    assert uv.shape == (0, 2) and idx.shape == (0, 3)
    with pytest.raises(SculptError, match="out of range"):
        un(vt, vt, ft + 1, 0.02)
    bad = vt.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(SculptError, match="non-finite"):
        un(bad, vt, ft, 0.02)
    with pytest.raises(SculptError, match="no CPU fallback"):
        un(vt.cpu(), vt.cpu(), ft.cpu(), 0.02)


def test_bake_texture_over_the_chart_atlas(cuda, model):
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d.unwrap import ChartUnwrapper

    m, codes, plain = model["m"], model["codes"], model["plain"]
    res = 128
    assert m.atlas == "box"
    default = m.bake_texture(plain, codes[0], texture_resolution=res)
    try:
        m.atlas = "box"
        box = m.bake_texture(plain, codes[0], texture_resolution=res)
        m.atlas = "charts"
        charts = m.bake_texture(plain, codes[0], texture_resolution=res)
        v, f, uv_c, rast_c = m._atlas(plain, res, 0.02, ChartUnwrapper())   # the unwrapper given explicitly
        m.atlas = "bogus"
        with pytest.raises(ValueError, match="atlas"):
            m.bake_texture(plain, codes[0], texture_resolution=res)
    finally:
        del m.atlas
    assert m.atlas == "box"
    v, f, uv_b, rast_b = m._atlas(plain, res, 0.02, None)   # the route before the setting: unwrapper=None, box projection
    assert torch.equal(default.uvs, uv_b) and torch.equal(box.uvs, uv_b)
    assert torch.equal(default.texture, box.texture)
    color_b, mask_b = ops.bake_scene_color(m._field(codes[0]), m.decoder, v, f, rast_b, radius=m.renderer.cfg.radius)
    assert torch.equal(box.texture[mask_b.bool()], color_b[mask_b.bool()])
    assert torch.equal(box.texture, m._padded(color_b, mask_b, res))
    # the chart atlas: other uvs, and its covered texels are the fused bake over _atlas with the unwrapper given explicitly
    assert charts.texture.shape == (res, res, 3) and torch.equal(charts.uvs, uv_c) and not torch.equal(uv_c, uv_b)
    color_c, mask_c = ops.bake_scene_color(m._field(codes[0]), m.decoder, v, f, rast_c, radius=m.renderer.cfg.radius)
    assert int(mask_c.sum()) > 0
    assert torch.equal(charts.texture[mask_c.bool()], color_c[mask_c.bool()])
    assert torch.equal(charts.texture, m._padded(color_c, mask_c, res))
    print("covered texels at %d^2: box %d, charts %d" % (res, int(mask_b.sum()), int(mask_c.sum())))


def test_generator_atlas_reaches_the_model(cuda, tmp_path):
    import types

    from test_host_logic import _write_checkpoint

    from sculptmate_amd import ops, synth
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr.spec import SMALL_CFG

    _write_checkpoint(str(tmp_path), SMALL_CFG, seed=61)
    g = TripoGenerator(cuda)
    assert g.atlas == "box"
    g.checkpoint_dir = str(tmp_path)
    g.mc_resolution = 32
    assert g.initiate_model() == 0
    g.model.mesh_sink = lambda *a: None
    g.model.textured_mesh_sink = lambda *a: None
    orig = g.model.extract_mesh

    def reachable(self, codes, **kw):   # random weights never reach the default threshold: take the grid's median
        return orig(codes, **dict(kw, threshold=float(ops.density_grid(codes[0].contiguous(), self.decoder, kw["resolution"]).median())))

    g.model.extract_mesh = types.MethodType(reachable, g.model)
    img = (synth.composite_rgb(synth.image_rgba(seed=62, size=SMALL_CFG["cond_image_size"])) * 255).astype(np.uint8)
    g.bake_texture_resolution = 64
    g.atlas = "charts"
    assert g.generate_mesh(img, "charts", enable_texture=True) == 0
    assert g.model.atlas == "charts" and g.model._chart_unwrapper is not None and g.model._unwrapper is None
    assert g.model._chart_unwrapper.last["n_charts"] >= 1
    assert g.last_meshes[0].texture is not None and g.last_meshes[0].uvs.shape[1] == 2
