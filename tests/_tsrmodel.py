"""The small synthetic TSR that the GPU tests of the mesh features share: built in one place, so that the tests of a new mesh
option run the model the others run."""
import math

import numpy as np

from sculptmate_amd import synth


def small_model(cuda, resolution, enable_texture=False, normals=None, project_keys=False, decoder_filter=True):
    """TSR(SMALL_CFG, pos_embed_mode="size") with synth.tsr_state(31) on `cuda`, the scene code of image seed 32, a density
    threshold its random weights reach (the median of the `resolution`^3 grid: a noisy surface of many components) and ONE plain
    mesh at that resolution, extracted with enable_texture / normals as given (shared by a module's tests, never modified).
    -> dict(m, img, codes, threshold, kw, plain); project_keys adds what a caller of ops.mesh_project needs: target (the
    iso-value in the raw density), cell (the lattice spacing) and radius.  decoder_filter is TSR's: False gives the
    plain-grid route of extract_meshes."""
    from sculptmate_amd import ops
    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr.spec import SMALL_CFG

    m = TSR(SMALL_CFG, pos_embed_mode="size", decoder_filter=decoder_filter)
    m.load_state_dict(synth.tsr_state(31, SMALL_CFG))
    m.to(cuda)
    img = synth.composite_rgb(synth.image_rgba(seed=32, size=SMALL_CFG["cond_image_size"]))
    codes = m([img], device=cuda)
    threshold = float(ops.density_grid(codes[0].contiguous(), m.decoder, resolution).median())
    kw = dict(resolution=resolution, threshold=threshold)
    plain = m.extract_meshes(codes, enable_texture=enable_texture, normals=normals, **kw)[0]
    out = dict(m=m, img=img, codes=codes, threshold=threshold, kw=kw, plain=plain)
    if project_keys:
        cfg = m.renderer.cfg
        out.update(target=float(np.float32(math.log(threshold) - float(cfg.density_bias))),
                   cell=2.0 * float(cfg.radius) / (resolution - 1), radius=float(cfg.radius))
    return out
