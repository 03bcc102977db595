"""Host side of the render passes, no GPU: the finishing rules of sculptmate_amd/tsr/passes.py on hand-made raw sums, the numpy
restatement the GPU tests measure against (tests/_passref.py), and the validation of `passes`."""
import numpy as np
import pytest
import torch

import _passref
from sculptmate_amd.tsr import passes as P


def _sums():
    """Raw sums of a 2 x 3 view: [0,0] a miss, [0,1] one sample of weight 1, [0,2] a thin ray, the second row random."""
    rng = np.random.default_rng(5)
    op = np.array([[0.0, 1.0, 1e-3], [0.3, 0.9, 0.999]], np.float32)
    z = np.array([[0.0, 1.75, 2.0], [1.2, 1.9, 2.5]], np.float32)
    n = rng.standard_normal((2, 3, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    col = rng.random((2, 3, 3)).astype(np.float32)
    ex = {"opacity": op, "depth_sum": op * z, "normal_sum": op[..., None] * n, "premul": op[..., None] * col}
    ex["normal_sum"][0, 0] = 0.0
    rgb = ex["premul"] + (np.float32(1) - op)[..., None]
    return {k: torch.from_numpy(v) for k, v in ex.items()}, torch.from_numpy(rgb), z, n


def test_finishing_rules_on_hand_made_sums():
    ex, rgb, z, n = _sums()
    out = P.finish(P.PASSES, rgb, ex)
    assert set(out) == set(P.PASSES)
    assert out["color"] is rgb and out["opacity"] is ex["opacity"]
    depth, normal, rgba = out["depth"].numpy(), out["normal"].numpy(), out["rgba"].numpy()
    assert depth.shape == (2, 3) and normal.shape == (2, 3, 3) and rgba.shape == (2, 3, 4)
    assert depth.dtype == normal.dtype == rgba.dtype == np.float32
    # opacity 0: depth 0 and normal 0, exactly
    assert depth[0, 0] == 0.0 and not normal[0, 0].any() and not rgba[0, 0].any()
    # one sample of weight 1: its depth and its normal
    assert depth[0, 1] == z[0, 1]
    assert np.abs(normal[0, 1] - n[0, 1]).max() <= 2e-7
    assert np.abs(depth - z)[0, 1:].max() <= 4e-7 and np.abs(depth - z)[1].max() <= 4e-7
    assert np.abs(np.linalg.norm(normal.reshape(-1, 3)[1:], axis=-1) - 1).max() <= 1e-6
    assert np.abs(normal - n).reshape(-1, 3)[1:].max() <= 1e-6
    # the cut-out over white is the colour picture: the same fp32 operation, the same bits
    over = rgba[..., :3] + (np.float32(1) - rgba[..., 3:])
    assert over.dtype == np.float32 and np.array_equal(over.view(np.uint32), rgb.numpy().view(np.uint32))
    # the numpy restatement of the rules agrees
    assert np.array_equal(_passref.depth_of(ex["depth_sum"].numpy(), ex["opacity"].numpy()), depth)
    assert np.abs(_passref.normal_of(ex["normal_sum"].numpy()) - normal).max() <= 1e-6
    assert np.array_equal(_passref.rgba_of(ex["premul"].numpy(), ex["opacity"].numpy()), rgba)


def test_a_short_normal_sum_keeps_its_direction():
    """|normal_sum| of a thin ray is far below the square root of the smallest fp32: the rule scales before it squares."""
    s = torch.tensor([[3e-30, -4e-30, 0.0], [0.0, 0.0, 0.0], [float("inf"), 1.0, 0.0]])
    n = P.normal_of(s).numpy()
    assert np.abs(n[0] - np.array([0.6, -0.8, 0.0], np.float32)).max() <= 1e-6
    assert not n[1].any() and not n[2].any()


def test_only_what_the_passes_need_is_asked_for():
    assert P.wanted(("color",)) == ()
    assert P.wanted(("opacity",)) == ("opacity",)
    assert "normal_sum" not in P.wanted(("color", "opacity", "rgba", "depth"))
    assert set(P.wanted(P.PASSES)) == {"opacity", "premul", "depth_sum", "normal_sum"}


def test_pil_modes_and_sizes():
    from PIL import Image

    ex, rgb, _, _ = _sums()
    views = {k: v[None] for k, v in P.finish(P.PASSES, rgb, ex).items()}     # one view of 2 x 3
    pt, arr, pil = (P.convert(views, t) for t in P.RETURN_TYPES)
    assert len(pt) == len(arr) == len(pil) == 1
    modes = {"color": "RGB", "opacity": "L", "rgba": "RGBA", "depth": "F", "normal": "RGB"}
    for name, mode in modes.items():
        assert isinstance(pt[0][name], torch.Tensor) and isinstance(arr[0][name], np.ndarray) and arr[0][name].dtype == np.float32
        assert np.array_equal(arr[0][name], pt[0][name].numpy())
        im = pil[0][name]
        assert isinstance(im, Image.Image) and im.mode == mode and im.size == (3, 2), name
    a = arr[0]
    assert np.array_equal(np.asarray(pil[0]["color"]), (a["color"] * 255.0).astype(np.uint8))
    assert np.array_equal(np.asarray(pil[0]["opacity"]), (a["opacity"] * 255.0).astype(np.uint8))
    assert np.array_equal(np.asarray(pil[0]["depth"]), a["depth"])
    assert np.array_equal(np.asarray(pil[0]["normal"]), ((a["normal"] * 0.5 + 0.5) * 255.0).astype(np.uint8))
    straight = np.asarray(pil[0]["rgba"])
    assert not straight[0, 0].any()                                           # alpha 0: colour 0
    assert np.array_equal(straight[..., 3], (a["rgba"][..., 3] * 255.0).astype(np.uint8))
    want = np.clip(a["rgba"][0, 1:, :3] / a["rgba"][0, 1:, 3:], 0, 1)
    assert np.array_equal(straight[0, 1:, :3], (want * 255.0).astype(np.uint8))


def test_passref_fp32_and_fp64_sums_agree_within_fp32_error():
    rng = np.random.default_rng(11)
    N, S = 64, 128
    w = rng.random((N, S)).astype(np.float32)
    w /= w.sum(-1, keepdims=True) * np.float32(1.25)                          # sum of the weights 0.8
    z = (1.0 + 1.8 * rng.random((N, S))).astype(np.float32)
    n = rng.standard_normal((N, S, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    s32, s64 = _passref.sums32(w, z, n), _passref.sums64(w, z, n)
    # S roundings of at most half an ulp of the running sum each, plus one per product: (S + 1) * 2^-24 * sum |terms|
    eps = 2.0 ** -24
    for key, mag in (("depth_sum", (w * z).sum(-1)), ("normal_sum", np.abs(w[..., None] * n).sum(-2))):
        err = np.abs(s32[key].astype(np.float64) - s64[key])
        assert s32[key].dtype == np.float32 and (err <= (S + 1) * eps * mag).all() and err.max() > 0, key
    # one sample of weight 1
    one = _passref.sums32(np.ones((1, 1)), np.full((1, 1), 1.75), np.array([[[0.0, 0.6, -0.8]]]))
    assert one["depth_sum"][0] == np.float32(1.75) and np.array_equal(one["normal_sum"][0], np.array([0.0, 0.6, -0.8], np.float32))


def test_passes_are_validated_before_anything_else():
    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr.spec import SMALL_CFG

    m = TSR(SMALL_CFG)                      # no weights, no device: only the validation can answer
    for bad in ((), [], ("colour",), ("color", "z"), "depht"):
        with pytest.raises(ValueError):
            m.render_passes([], 2, passes=bad)
        with pytest.raises(ValueError):
            m.renderer.render_passes(None, None, None, None, passes=bad)
    with pytest.raises(ValueError):
        m.render_passes([], 2, return_type="jpeg")
    assert P.check_passes("depth") == ("depth",) and P.check_passes(["normal", "color", "normal"]) == ("normal", "color")
    from sculptmate_amd._facade import STATUS_NOT_LOADED
    from sculptmate_amd.generate import TripoGenerator

    assert TripoGenerator("cuda:0").render_views(None, passes=("depth",)) == STATUS_NOT_LOADED
