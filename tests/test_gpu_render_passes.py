"""The render passes on the GPU (csrc/render.hip: sculpt_render_passes; ops.render_passes; TSR.render_passes): raw per-ray sums
beside the colour picture, against the colour kernel's own outputs, ops.field_normals at the very sample points and the
sequential fp32 / fp64 sums of tests/_passref.py.

Cases, rays and scene are those of tests/test_gpu_render.py: hand_ = 171 hand-made rays x 128 samples (misses, mixed tiles, ragged
tails: 171 = 5 * 32 + 11 = 21 * 8 + 3), view_ = one 16 x 16 view x 128, short_ = the rays of hand_ x 5; synth.decoder_state(seed=1),
synth.triplane(seed=2, scale=4.0)."""
import os

import numpy as np
import pytest
import torch

import _passref
import _tsrmodel
from conftest import GOLDEN
from sculptmate_amd import synth

pytestmark = pytest.mark.gpu

CASES = ["hand_", "view_", "short_"]
RADIUS, BIAS = 0.87, -1.0
OLD = ("opacity", "z_vals", "weights")
NEW = ("depth_sum", "normal_sum", "premul")
NO_NORMAL = ("depth_sum", "premul")        # without normal_sum: the colour kernel's second form, not the forward-mode kernel


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)


def _host(rgb, extra):
    return dict({k: v.cpu().numpy() for k, v in extra.items()}, comp_rgb=rgb.cpu().numpy())


@pytest.fixture(scope="module")
def scene(cuda):
    """Golden, decoder, channel-last planes and, per case, ONE render_rays, ONE render_passes with every output (the forward-mode
    kernel) and ONE with every output but normal_sum (the colour kernel's second form), plus the field's normals at the sample
    points (xyz made on the CPU from the golden depths); shared, never modified."""
    from sculptmate_amd import ops

    g = np.load(os.path.join(GOLDEN, "render.npz"))
    Ws, bs = synth.decoder_lists(synth.decoder_state(seed=1))
    mlp = ops.PackedMLP(Ws, bs, cuda)
    planes = ops.ChannelLastPlanes(torch.from_numpy(synth.triplane(seed=2, scale=4.0)).to(cuda))
    rays, old, got, two, normals = {}, {}, {}, {}, {}
    for case in CASES:
        o, d = torch.from_numpy(g[case + "rays_o"]).to(cuda), torch.from_numpy(g[case + "rays_d"]).to(cuda)
        S = int(g[case + "n_samples"])
        rays[case] = (o, d, S)
        old[case] = _host(*ops.render_rays(planes, mlp, o, d, radius=RADIUS, density_bias=BIAS, n_samples=S, want=OLD))
        got[case] = _host(*ops.render_passes(planes, mlp, o, d, radius=RADIUS, density_bias=BIAS, n_samples=S, want=OLD + NEW))
        two[case] = _host(*ops.render_passes(planes, mlp, o, d, radius=RADIUS, density_bias=BIAS, n_samples=S, want=OLD + NO_NORMAL))
        valid = g[case + "rays_valid"]
        oc, dc, z = (torch.from_numpy(g[case + k]) for k in ("rays_o", "rays_d", "z_vals"))
        xyz = oc[:, None, :] + z[..., None] * dc[:, None, :]
        xyz[torch.from_numpy(~valid)] = 0.0                   # a miss is never sampled; its weights are 0
        normals[case] = ops.field_normals(planes, mlp, xyz.to(cuda), radius=RADIUS)["normal"].cpu().numpy()
    return {"g": g, "mlp": mlp, "planes": planes, "rays": rays, "old": old, "got": got, "two": two, "normals": normals}


def _render(scene, case, want, bias=BIAS, o=None, d=None):
    from sculptmate_amd import ops

    oo, dd, S = scene["rays"][case]
    rgb, extra = ops.render_passes(scene["planes"], scene["mlp"], oo if o is None else o, dd if d is None else d, radius=RADIUS,
                                   density_bias=bias, n_samples=S, want=want)
    return dict(extra, comp_rgb=rgb)


@pytest.mark.parametrize("case", CASES)
def test_old_outputs_keep_render_rays_bits_whatever_else_is_asked(scene, case):
    old = scene["old"][case]
    for extra in ((), NEW, ("depth_sum",), ("premul",), ("normal_sum",), ("depth_sum", "normal_sum")):
        got = scene["got"][case] if extra == NEW else _render(scene, case, OLD + extra)
        assert set(got) == set(OLD + extra + ("comp_rgb",))
        for key in OLD + ("comp_rgb",):
            assert np.array_equal(_bits(got[key]), _bits(old[key])), (case, extra, key)


@pytest.mark.parametrize("form", ["two", "got"])
@pytest.mark.parametrize("case", CASES)
def test_depth_and_premultiplied_colour(scene, case, form):
    """Both kernels that write depth_sum and premul: the colour kernel's second form ("two": no normal_sum asked) and the
    forward-mode kernel ("got"), each against its own weights, depths, opacity and picture; and the two agree bit for bit."""
    g, got = scene["g"], dict(scene[form][case])
    valid = g[case + "rays_valid"]
    assert set(got) == set(OLD + (NO_NORMAL if form == "two" else NEW) + ("comp_rgb",))
    for key in OLD + NO_NORMAL + ("comp_rgb",):
        assert np.array_equal(_bits(got[key]), _bits(scene["got"][case][key])), (case, form, key)
    got.setdefault("normal_sum", scene["got"][case]["normal_sum"])
    assert got["depth_sum"].shape == valid.shape and got["premul"].shape == valid.shape + (3,)
    assert got["depth_sum"].dtype == got["premul"].dtype == np.float32
    ref = _passref.sums32(got["weights"], got["z_vals"], np.zeros(got["weights"].shape + (3,), np.float32))
    assert np.array_equal(_bits(got["depth_sum"]), _bits(ref["depth_sum"]))
    over = got["premul"] + (np.float32(1) - got["opacity"])[:, None]
    assert over.dtype == np.float32 and np.array_equal(_bits(over), _bits(got["comp_rgb"]))
    assert not got["depth_sum"][~valid].any() and not got["premul"][~valid].any() and not got["normal_sum"][~valid].any()
    assert (got["depth_sum"][valid] > 0).all()
    # the weighted mean depth lies between the ray's first and last sample
    depth = _passref.depth_of(got["depth_sum"], got["opacity"])[valid].astype(np.float64)
    z = got["z_vals"][valid].astype(np.float64)
    assert (depth >= z[:, 0] * (1 - 1e-5)).all() and (depth <= z[:, -1] * (1 + 1e-5)).all()


@pytest.mark.parametrize("case", CASES)
def test_normal_sum_is_the_composed_rule_bit_for_bit(scene, case):
    """sum_s w_s n_s with the call's own weights and ops.field_normals at the sample points, summed one sample after the other
    in fp32: the kernel equals the composed rule bit for bit."""
    got, n = scene["got"][case], scene["normals"][case]
    assert got["normal_sum"].shape == n.shape[:1] + (3,) and got["normal_sum"].dtype == np.float32
    ref = _passref.sums32(got["weights"], got["z_vals"], n)["normal_sum"]
    same = _bits(got["normal_sum"]) == _bits(ref)
    print("%snormal_sum: %d of %d values equal the composed rule's bits; max |diff| %.3e" % (
        case, same.sum(), same.size, np.abs(got["normal_sum"].astype(np.float64) - ref).max()))
    assert same.all()
    assert (np.linalg.norm(n, axis=-1) > 0.5).any() and got["normal_sum"].any()


@pytest.mark.parametrize("case", CASES)
def test_normal_sum_against_the_fp64_sum(scene, case):
    """|normal_sum - fp64 sum| <= 4 x E32, E32 = the error of the sequential fp32 sum of the same values against the fp64 one."""
    got, n = scene["got"][case], scene["normals"][case]
    s32 = _passref.sums32(got["weights"], got["z_vals"], n)["normal_sum"]
    s64 = _passref.sums64(got["weights"], got["z_vals"], n)["normal_sum"]
    e32 = np.abs(s32.astype(np.float64) - s64).max()
    err = np.abs(got["normal_sum"].astype(np.float64) - s64).max()
    print("%snormal_sum: device %.3e, E32 %.3e, ratio %.2f" % (case, err, e32, err / e32))
    assert e32 > 0 and err <= 4 * e32, (case, err, e32)


def test_new_outputs_do_not_depend_on_grouping(scene):
    """hand_ whole, in two halves cut at an odd index, and reversed: the same bits for every ray."""
    whole = scene["got"]["hand_"]
    o, d, _ = scene["rays"]["hand_"]
    cut = 77
    a, b = _render(scene, "hand_", NEW, o=o[:cut], d=d[:cut]), _render(scene, "hand_", NEW, o=o[cut:], d=d[cut:])
    rev = _render(scene, "hand_", NEW, o=o.flip(0), d=d.flip(0))
    for key in NEW + ("comp_rgb",):
        assert np.array_equal(_bits(torch.cat([a[key], b[key]])), _bits(whole[key])), key
        assert np.array_equal(_bits(rev[key].flip(0)), _bits(whole[key])), key
    # the same without normal_sum: the colour kernel's second form, tiles of 32
    a, b = _render(scene, "hand_", NO_NORMAL, o=o[:cut], d=d[:cut]), _render(scene, "hand_", NO_NORMAL, o=o[cut:], d=d[cut:])
    rev = _render(scene, "hand_", NO_NORMAL, o=o.flip(0), d=d.flip(0))
    for key in NO_NORMAL + ("comp_rgb",):
        assert np.array_equal(_bits(torch.cat([a[key], b[key]])), _bits(whole[key])), key
        assert np.array_equal(_bits(rev[key].flip(0)), _bits(whole[key])), key


def test_the_skip_is_exact(scene, monkeypatch):
    """A saturated field (the tiles stop early), an empty one and the plain one, with and without SCULPT_RENDER_FORM=noskip:
    every output has the same bits."""
    valid = scene["g"]["hand_rays_valid"]
    want = OLD + NEW
    runs = {}
    for name, bias in (("saturated", 20.0), ("empty", -60.0), ("plain", BIAS)):
        monkeypatch.delenv("SCULPT_RENDER_FORM", raising=False)
        skip = {k: v.cpu().numpy() for k, v in _render(scene, "hand_", want, bias=bias).items()}
        monkeypatch.setenv("SCULPT_RENDER_FORM", "noskip")
        full = {k: v.cpu().numpy() for k, v in _render(scene, "hand_", want, bias=bias).items()}
        runs[name] = (skip, full)
    monkeypatch.delenv("SCULPT_RENDER_FORM", raising=False)
    # the test is not vacuous: the saturated field has rays whose weights end in exact zeros well before the last sample ...
    w = runs["saturated"][0]["weights"][valid]
    last = np.where(w != 0, np.arange(w.shape[1])[None], -1).max(-1)          # index of the last non-zero weight, -1 if none
    print("saturated: last non-zero weight per valid ray: min %d, median %d, max %d of %d; tiles of 8 that stop early: %d" % (
        last.min(), np.median(last), last.max(), w.shape[1] - 1,
        sum(1 for t in range(0, 171, 8) if valid[t:t + 8].any() and
            np.where(runs["saturated"][0]["weights"][t:t + 8] != 0, np.arange(w.shape[1])[None], -1).max() < w.shape[1] - 2)))
    assert (last < w.shape[1] - 2).any() and (runs["saturated"][0]["opacity"][valid] > 0).all()
    # ... and the empty one has no weight at all
    e = runs["empty"][0]
    print("empty: max weight %.3e" % e["weights"].max())
    assert not e["weights"].any() and not e["opacity"][valid].any() and not e["depth_sum"][valid].any()
    assert not e["normal_sum"][valid].any()
    for name, (skip, full) in runs.items():
        for key in want + ("comp_rgb",):
            assert np.array_equal(_bits(skip[key]), _bits(full[key])), (name, key)
    for key in want + ("comp_rgb",):
        assert np.array_equal(_bits(runs["plain"][0][key]), _bits(scene["got"]["hand_"][key])), key


def test_ops_render_passes_shapes_and_refusals(scene, cuda):
    from sculptmate_amd import ops

    o, d, _ = scene["rays"]["view_"]
    planes, mlp, view = scene["planes"], scene["mlp"], scene["got"]["view_"]
    rgb, extra = ops.render_passes(planes, mlp, o.view(2, 8, 16, 3), d.view(2, 8, 16, 3), RADIUS, BIAS, 128, want=OLD + NEW)
    assert rgb.shape == (2, 8, 16, 3) and set(extra) == set(OLD + NEW)
    for key, tail in (("opacity", ()), ("z_vals", (128,)), ("weights", (128,)), ("depth_sum", ()), ("normal_sum", (3,)),
                      ("premul", (3,))):
        assert extra[key].shape == (2, 8, 16) + tail and extra[key].dtype == torch.float32, key
        assert np.array_equal(_bits(extra[key].reshape(view[key].shape)), _bits(view[key])), key
    rgb0, none = ops.render_passes(planes, mlp, o, d, RADIUS, BIAS, 128)
    assert none == {} and np.array_equal(_bits(rgb0), _bits(view["comp_rgb"]))
    empty, ex = ops.render_passes(planes, mlp, o[:0], d[:0], RADIUS, BIAS, 128, want=NEW)
    assert empty.shape == (0, 3) and ex["depth_sum"].shape == (0,) and ex["normal_sum"].shape == ex["premul"].shape == (0, 3)
    with pytest.raises(ops.SculptError):
        ops.render_passes(planes, mlp, o, d, RADIUS, BIAS, 128, want=("depth",))
    with pytest.raises(ops.SculptError):
        ops.render_passes(planes, mlp, o.cpu(), d.cpu(), RADIUS, BIAS, 128, want=NEW)
    with pytest.raises(ops.SculptError):
        ops.render_passes(planes, mlp, o, d[:5], RADIUS, BIAS, 128, want=NEW)
    with pytest.raises(ops.SculptError):
        ops.render_passes(planes, mlp, o, d, RADIUS, BIAS, 0, want=NEW)
    with pytest.raises(ops.SculptError):
        ops.render_rays(planes, mlp, o, d, want=("depth",))                  # render_rays is what it was


def test_model_surface(cuda):
    """TSR.render_passes on the small synthetic model: 2 views of 9 x 8, two stacked scene codes."""
    from PIL import Image

    from sculptmate_amd.generate import TripoGenerator

    model = _tsrmodel.small_model(cuda, 32)
    m, codes = model["m"], model["codes"]
    codes = torch.cat([codes, codes * 0.5])
    cam = dict(n_views=2, elevation_deg=10.0, height=9, width=8)
    every = ("color", "opacity", "rgba", "depth", "normal")
    pt = m.render_passes(codes, passes=every, return_type="pt", **cam)
    arr = m.render_passes(codes, passes=every, return_type="np", **cam)
    pil = m.render_passes(codes, passes=every, return_type="pil", **cam)
    color = m.render(codes, return_type="pt", **cam)
    shapes = {"color": (9, 8, 3), "opacity": (9, 8), "rgba": (9, 8, 4), "depth": (9, 8), "normal": (9, 8, 3)}
    modes = {"color": "RGB", "opacity": "L", "rgba": "RGBA", "depth": "F", "normal": "RGB"}
    assert len(pt) == len(arr) == len(pil) == 2
    for s in range(2):
        assert len(pt[s]) == len(arr[s]) == len(pil[s]) == 2
        for v in range(2):
            assert set(pt[s][v]) == set(arr[s][v]) == set(pil[s][v]) == set(every)
            for name in every:
                t = pt[s][v][name]
                assert t.shape == shapes[name] and t.dtype == torch.float32 and t.is_cuda, name
                a = arr[s][v][name]
                assert isinstance(a, np.ndarray) and a.dtype == np.float32 and np.array_equal(_bits(a), _bits(t)), name
                im = pil[s][v][name]
                assert isinstance(im, Image.Image) and im.mode == modes[name] and im.size == (8, 9), name
            host = arr[s][v]
            assert np.array_equal(_bits(host["color"]), _bits(color[s][v]))
            assert np.array_equal(np.asarray(pil[s][v]["color"]), (host["color"] * 255.0).astype(np.uint8))
            op, depth, normal = host["opacity"], host["depth"], host["normal"]
            assert np.isfinite(depth).all() and (depth >= 0).all() and not depth[op == 0].any() and (depth[op > 0] > 0).all()
            length = np.linalg.norm(normal.astype(np.float64), axis=-1)
            assert np.isfinite(normal).all() and ((np.abs(length - 1) <= 1e-6) | (length == 0)).all()
            assert not normal[op == 0].any()
            over = host["rgba"][..., :3] + (np.float32(1) - host["rgba"][..., 3:])
            assert np.array_equal(_bits(over), _bits(host["color"])) and np.array_equal(_bits(host["rgba"][..., 3]), _bits(op))
    assert (arr[0][0]["opacity"] > 0).any() and np.linalg.norm(arr[0][0]["normal"], axis=-1).max() > 0.5
    # a stack of scenes is the scenes one by one
    for s in range(2):
        one = m.render_passes(codes[s:s + 1], passes=every, return_type="pt", **cam)
        assert len(one) == 1
        for v in range(2):
            for name in every:
                assert np.array_equal(_bits(one[0][v][name]), _bits(pt[s][v][name])), (s, v, name)
    assert not torch.equal(pt[0][0]["depth"], pt[1][0]["depth"])
    # the renderer itself: a stack of scene codes [B, 3, C, H, W] with rays [B, ...] is the scenes one by one
    from sculptmate_amd.tsr.cameras import get_spherical_cameras

    rays_o, rays_d = get_spherical_cameras(2, 10.0, 1.9, 40.0, 9, 8)
    stack = m.renderer.render_passes(m.decoder, codes, torch.stack([rays_o, rays_o]), torch.stack([rays_d, rays_d]), every)
    assert set(stack) == set(every)
    for name in every:
        assert stack[name].shape == (2, 2) + shapes[name]
        for s in range(2):
            assert np.array_equal(_bits(stack[name][s]), _bits(torch.stack([pt[s][v][name] for v in range(2)]))), (s, name)
    # without "normal" the views come from the colour kernel's second form: the same pictures
    flat = m.render_passes(codes, passes=("rgba", "depth", "opacity"), return_type="pt", **cam)
    for s in range(2):
        for v in range(2):
            assert set(flat[s][v]) == {"rgba", "depth", "opacity"}
            for name in flat[s][v]:
                assert np.array_equal(_bits(flat[s][v][name]), _bits(pt[s][v][name])), (s, v, name)
    # only what is asked for
    only = m.render_passes(codes[:1], passes=("opacity",), **cam)
    assert all(set(view) == {"opacity"} for view in only[0])
    assert np.array_equal(_bits(only[0][1]["opacity"]), _bits(pt[0][1]["opacity"]))
    with pytest.raises(ValueError):
        m.render_passes(codes, passes=("alpha",), **cam)
    # the facade: passes=None is what it returned before, passes a list of dicts of PIL pictures
    gen = TripoGenerator(cuda)
    gen.model = m
    views = gen.render_views(model["img"], **cam)
    again = m.render(model["codes"], return_type="pil", **cam)[0]
    assert isinstance(views, list) and len(views) == 2 and all(isinstance(x, Image.Image) and x.mode == "RGB" for x in views)
    assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(views, again))
    dicts = gen.render_views(model["img"], passes=("rgba", "depth"), **cam)
    assert len(dicts) == 2 and all(set(x) == {"rgba", "depth"} for x in dicts)
    assert dicts[0]["rgba"].mode == "RGBA" and dicts[0]["depth"].mode == "F" and dicts[0]["depth"].size == (8, 9)
    assert np.array_equal(np.asarray(dicts[1]["depth"]), arr[0][1]["depth"])
    from sculptmate_amd._facade import STATUS_FAILED

    assert gen.render_views(model["img"], passes=("alpha",), **cam) == STATUS_FAILED
