"""extract_meshes' geometry chain behind the PLAIN density grid (decoder_filter=False: ops.density_grid + marching cubes), the
route the other mesh-feature tests -- whose models all take the two-pass grid -- do not run."""
import pytest
import torch

import _tsrmodel

pytestmark = pytest.mark.gpu


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_all_four_options_on_the_plain_grid_are_the_four_calls_in_order(cuda):
    from sculptmate_amd import ops

    model = _tsrmodel.small_model(cuda, 32, project_keys=True, decoder_filter=False)
    m, plain, code = model["m"], model["plain"], model["codes"][0].contiguous()
    got = m.extract_meshes(model["codes"], enable_texture=True, normals="field", keep_components="largest", smooth=3, simplify=0.5,
                           project=True, **model["kw"])[0]
    assert m.filter_info["filtered"] == 0                      # not one call went through the two-pass grid
    v, f = ops.mesh_keep_components(plain.vertices, plain.faces, "largest")[:2]
    v = ops.mesh_smooth(v, f, 3)
    v, f = ops.mesh_simplify(v, f, 0.5)[:2]
    v = ops.mesh_project(code, m.decoder, v, f, model["target"], 1.0 * model["cell"], steps=8, radius=model["radius"])[0]
    print("plain grid: %d faces -> %d faces" % (plain.faces.shape[0], f.shape[0]))
    assert 0 < f.shape[0] < plain.faces.shape[0]
    assert _same(got.vertices, v) and _same(got.faces, f)
    assert _same(got.vertex_colors, m.renderer.query_triplane(m.decoder, v, code)["color"])
    assert _same(got.vertex_normals, m.field_normals(v, code))
