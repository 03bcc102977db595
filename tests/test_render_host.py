"""Host side of the volume renderer, no GPU: cameras, rays and the box test against the reference's own results
(tests/golden/render.npz, made by tests/golden/make_render_goldens.py), the numpy restatement of the composite that the GPU
tests measure against, and the C ABI of the new entry."""
import os
import re

import numpy as np
import pytest
import torch

import _renderref
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "render.npz"))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_spherical_cameras_and_directions_equal_the_reference_bit_for_bit(g):
    from sculptmate_amd.tsr import cameras

    rays_o, rays_d = cameras.get_spherical_cameras(3, 20.0, 1.9, 40.0, 9, 8)
    assert rays_o.shape == (3, 9, 8, 3) and rays_o.dtype == torch.float32
    assert _same_bits(rays_o.numpy(), g["cam3_rays_o"]) and _same_bits(rays_d.numpy(), g["cam3_rays_d"])
    assert _same_bits(cameras.get_ray_directions(9, 8, 1.0).numpy(), g["dirs_9x8"])
    o16, d16 = cameras.get_spherical_cameras(1, 0.0, 1.9, 40.0, 16, 16)
    assert _same_bits(o16.reshape(-1, 3).numpy(), g["view_rays_o"]) and _same_bits(d16.reshape(-1, 3).numpy(), g["view_rays_d"])


def test_spherical_cameras_are_cached_per_argument_tuple():
    from sculptmate_amd.tsr import cameras

    cameras._spherical_cameras.cache_clear()
    a = cameras.get_spherical_cameras(2, 10.0, 1.9, 40.0, 4, 5)
    a[0].zero_()                                          # the caller's copy; the cached tensors are untouched
    b = cameras.get_spherical_cameras(2, 10.0, 1.9, 40.0, 4, 5)
    info = cameras._spherical_cameras.cache_info()
    assert (info.hits, info.misses) == (1, 1) and float(b[0].abs().max()) > 1.0
    cameras.get_spherical_cameras(2, 11.0, 1.9, 40.0, 4, 5)
    assert cameras._spherical_cameras.cache_info().misses == 2


def test_get_rays_forms_agree():
    """[H, W, 3] with one pose, with a batch of poses, [B, H, W, 3] and flat [N, 3] give the same rays."""
    from sculptmate_amd.tsr import cameras

    dirs = cameras.get_ray_directions(3, 4, 1.5)
    c2w = torch.eye(4)[None].repeat(2, 1, 1)
    c2w[1, :3, :3] = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    c2w[:, :3, 3] = torch.tensor([[0.1, 0.2, 0.3], [1.0, 2.0, 3.0]])
    o_b, d_b = cameras.get_rays(dirs, c2w, keepdim=True)
    o_1, d_1 = cameras.get_rays(dirs, c2w[1], keepdim=True)
    o_4, d_4 = cameras.get_rays(dirs[None].repeat(2, 1, 1, 1), c2w, keepdim=True)
    o_n, d_n = cameras.get_rays(dirs.reshape(-1, 3), c2w[1])
    assert o_b.shape == (2, 3, 4, 3) and torch.equal(d_b[1], d_1) and torch.equal(o_b[1], o_1)
    assert torch.equal(d_4, d_b) and torch.equal(o_4, o_b)
    assert torch.equal(d_n, d_1.reshape(-1, 3)) and torch.equal(o_n, o_1.reshape(-1, 3))
    assert torch.equal(d_b[0], dirs)                      # identity pose


@pytest.mark.parametrize("case", ["hand_", "view_", "short_"])
def test_box_test_equals_the_reference_bit_for_bit(g, case):
    from sculptmate_amd.tsr import cameras

    o, d = torch.from_numpy(g[case + "rays_o"]), torch.from_numpy(g[case + "rays_d"])
    t_near, t_far, valid = cameras.rays_intersect_bbox(o, d, 0.87)
    assert t_near.shape == (len(o), 1) and valid.shape == (len(o),)
    assert np.array_equal(valid.numpy(), g[case + "rays_valid"])
    assert _same_bits(t_near.numpy(), g[case + "t_near"]) and _same_bits(t_far.numpy(), g[case + "t_far"])
    # leading shapes pass through
    tn2, _, v2 = cameras.rays_intersect_bbox(o[:6].reshape(2, 3, 3), d[:6].reshape(2, 3, 3), 0.87)
    assert tn2.shape == (2, 3, 1) and v2.shape == (2, 3) and torch.equal(tn2.reshape(-1, 1), t_near[:6])


def test_hand_made_rays_cover_what_they_claim(g):
    """Golden (b): an odd count that is no multiple of 32, a whole tile of misses, mixed tiles, grazing rays on both sides of the
    threshold, an origin inside the box (t_near == 0 on a valid ray), tiny direction components of both signs and zero."""
    d, valid, tn, tf = g["hand_rays_d"], g["hand_rays_valid"], g["hand_t_near"][:, 0], g["hand_t_far"][:, 0]
    n = len(d)
    assert n % 2 == 1 and n % 32 != 0 and n <= 256
    tiles = [valid[i:i + 32] for i in range(0, n, 32)]
    assert any(not t.any() for t in tiles) and sum(t.any() and not t.all() for t in tiles) >= 2
    chord = (tf - tn)[valid]
    assert (chord < 0.0102).any() and not valid[12:16].all() and valid[12:16].any()
    assert (valid & (tn == 0)).any()
    tiny = np.abs(d) < 1e-6
    assert (d[tiny] > 0).any() and (d[tiny] < 0).any() and (d[tiny] == 0).any() and valid[tiny.any(1)].any()


@pytest.mark.parametrize("case", ["hand_", "short_"])
def test_sample_depths_restated_in_numpy_equal_the_reference(g, case):
    S = int(g[case + "n_samples"])
    t_vals = torch.linspace(0, 1, S + 1).numpy()
    valid = g[case + "rays_valid"]
    z = _renderref.sample_z(g[case + "t_near"], g[case + "t_far"], t_vals)
    assert z.dtype == np.float32 and _same_bits(z[valid], g[case + "z_vals"][valid])
    assert not g[case + "z_vals"][~valid].any()


def test_composite_restatements_reproduce_the_reference(g):
    """Fed with the reference's own per-sample density_act and color (stored for the first rays of golden (b)), the fp64 form
    reproduces the reference's fp64 picture to 1e-12 and the sequential fp32 form lands within E_ref of it -- E_ref being the
    reference's own fp32 error on the same rays."""
    n = int(g["hand_per_sample_rays"])
    valid = g["hand_rays_valid"][:n]
    t_vals = torch.linspace(0, 1, int(g["hand_n_samples"]) + 1).numpy()

    def full(a):
        out = np.zeros((n,) + a.shape[1:], a.dtype)
        out[valid] = a
        return out

    ref64 = g["hand_comp_rgb64"][:n]
    c64 = _renderref.composite64(full(g["hand_density_act64"]), full(g["hand_color64"]), t_vals, valid)
    assert np.abs(c64["comp_rgb"] - ref64).max() <= 1e-12
    assert np.array_equal(c64["comp_rgb"][~valid], np.ones(((~valid).sum(), 3))) and not c64["opacity"][~valid].any()
    c32 = _renderref.composite32(full(g["hand_density_act"]), full(g["hand_color"]), t_vals, valid)
    err = np.abs(c32["comp_rgb"].astype(np.float64) - ref64)[valid].max()
    print("sequential fp32 composite vs reference fp64: %.3e, E_ref %.3e" % (err, float(g["hand_E_ref"])))
    assert err <= float(g["hand_E_ref"])
    assert np.array_equal(c32["comp_rgb"][~valid], np.ones(((~valid).sum(), 3), np.float32))
    # the golden's own conditions: partial opacity is exercised, and so is the 1e-10 term of a saturated ray
    op = c64["opacity"][valid]
    assert ((op > 0.05) & (op < 0.95)).any() and (op >= 0.999).any()


def test_render_rays_is_declared_and_bound():
    """sculpt_render_rays: declared in the header with the issue's argument list, bound in _lib with matching ctypes, exported by
    the library; the ABI version is unchanged."""
    import ctypes

    from sculptmate_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "sculpt_hip.h")).read()
    m = re.search(r"\bint\s+sculpt_render_rays\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m, "sculpt_render_rays is not declared in include/sculpt_hip.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    kinds = []
    for a in args:
        if "*" in a or a.startswith("sculpt_stream_t"):
            kinds.append(ctypes.c_void_p)
        else:
            kinds.append({"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[a.split()[0]])
    res, argtypes = _lib.SIGNATURES["sculpt_render_rays"]
    assert res is ctypes.c_int and argtypes == kinds and len(kinds) == 18
    assert hasattr(_lib.lib, "sculpt_render_rays")
    assert int(re.search(r"#define\s+SCULPT_ABI_VERSION\s+(\d+)", hdr).group(1)) == 4 == _lib.lib.sculpt_version()


def test_render_rays_refuses_bad_arguments_without_a_device():
    """Argument validation runs before anything touches the GPU: errors come back as a code with a message; no rays is a success."""
    from sculptmate_amd import _lib

    lib = _lib.lib
    one = 1  # a non-null pointer value that is never dereferenced: every call below returns before a launch

    def call(planes=one, C=40, H=4, W=4, mlp=one, nh=1, ro=one, rd=one, n=0, radius=0.87, t=one, S=8, rgb=one):
        return lib.sculpt_render_rays(planes, C, H, W, mlp, nh, ro, rd, n, radius, -1.0, t, S, rgb, None, None, None, None)

    assert call() == 0                                                     # n_rays == 0
    assert call(C=32) != 0 and "C=40" in _lib.last_error()
    assert call(planes=None) != 0 and "null" in _lib.last_error()
    assert call(S=0) != 0 and "sample" in _lib.last_error()
    assert call(n=-1) != 0 and call(nh=-1) != 0 and call(radius=0.0) != 0 and call(H=0) != 0
    assert call(n=5, ro=None) != 0 and "null" in _lib.last_error()
    assert call(n=5, t=None) != 0 and call(n=5, rgb=None) != 0
    assert call(n=5, nh=12) != 0 and "LDS" in _lib.last_error()


def test_renderer_surface_without_a_device():
    from sculptmate_amd.tsr import TSR, TriplaneNeRFRenderer
    from sculptmate_amd.tsr.spec import DEFAULT_CFG, SMALL_CFG

    r = TriplaneNeRFRenderer(DEFAULT_CFG["renderer"])
    assert r.num_samples_per_ray == 128 and callable(r) and r.__call__.__func__ is TriplaneNeRFRenderer.forward
    cfg = dict(DEFAULT_CFG["renderer"])
    del cfg["num_samples_per_ray"]
    assert TriplaneNeRFRenderer(cfg).num_samples_per_ray == 128
    noisy = TriplaneNeRFRenderer(dict(cfg, randomized=True))
    with pytest.raises(NotImplementedError, match="randomized"):
        noisy(None, torch.zeros(3, 40, 4, 4), torch.zeros(2, 3), torch.zeros(2, 3))
    m = TSR(SMALL_CFG)
    with pytest.raises(ValueError):
        m.render([], 2, return_type="jpeg")
    from sculptmate_amd._facade import STATUS_NOT_LOADED
    from sculptmate_amd.generate import TripoGenerator

    assert TripoGenerator("cuda:0").render_views(None) == STATUS_NOT_LOADED
