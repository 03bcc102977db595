"""The passes of a rendered view and the rules that finish them from the ray kernel's raw sums (ops.render_passes).  Pure
torch on whatever device the sums live on, CPU included: nothing here launches a kernel of the library.

    pass       from                       shape        rule
    color      comp_rgb                   [..., 3]     as TSR.render: the picture on white
    opacity    opacity                    [...]        sum of the weights; the mask of the other passes
    rgba       premul, opacity            [..., 4]     premultiplied: rgba[..., :3] + (1 - rgba[..., 3:]) is `color`, the same fp32 sum
    depth      depth_sum, opacity         [...]        depth_sum / opacity where opacity > 0, else 0
    normal     normal_sum                 [..., 3]     normal_sum / |normal_sum| where the length is > 0, else 0; world space

`depth` is the expected distance from the camera along the ray (TSR's rays are unit vectors), over what the ray absorbed.  Where
opacity is small it is a quotient of two small sums and noisy: `opacity` is the mask to read it with.  `normal` is the weighted
mean of the field's normals (ops.field_normals) at the samples, renormalised.
"""
import numpy as np
import torch

PASSES = ("color", "opacity", "rgba", "depth", "normal")
# what each pass asks of ops.render_passes beside comp_rgb
NEEDS = {"color": (), "opacity": ("opacity",), "rgba": ("opacity", "premul"), "depth": ("opacity", "depth_sum"),
         "normal": ("normal_sum",)}
RETURN_TYPES = ("pt", "np", "pil")


def check_passes(passes):
    """-> the passes as a tuple without repeats, in the order given; ValueError when there is none or one is unknown."""
    if isinstance(passes, str):
        passes = (passes,)
    passes = tuple(dict.fromkeys(passes))
    unknown = [p for p in passes if p not in PASSES]
    if unknown:
        raise ValueError("unknown pass %s (any of %s)" % (unknown, ", ".join(PASSES)))
    if not passes:
        raise ValueError("passes is empty (any of %s)" % ", ".join(PASSES))
    return passes


def wanted(passes):
    """The `want` of ops.render_passes that `passes` need, and nothing more (no "normal": no normal_sum, and the call stays the colour kernel)."""
    return tuple(dict.fromkeys(k for p in passes for k in NEEDS[p]))


def depth_of(depth_sum, opacity):
    return torch.where(opacity > 0, depth_sum / opacity, torch.zeros_like(depth_sum))


def normal_of(normal_sum):
    # scaled by the largest component first, so that the squares of a short sum do not vanish
    m = normal_sum.abs().amax(dim=-1, keepdim=True)
    ok = (m > 0) & torch.isfinite(m)
    u = normal_sum / torch.where(ok, m, torch.ones_like(m))
    n = u / torch.sqrt((u * u).sum(dim=-1, keepdim=True))
    return torch.where(ok, n, torch.zeros_like(n))


def rgba_of(premul, opacity):
    return torch.cat([premul, opacity[..., None]], dim=-1)


def finish(passes, comp_rgb, extras):
    """comp_rgb and the extras of ops.render_passes(want=wanted(passes)) -> {pass: tensor} with the rays' leading shape."""
    out = {}
    for p in passes:
        if p == "color":
            out[p] = comp_rgb
        elif p == "opacity":
            out[p] = extras["opacity"]
        elif p == "rgba":
            out[p] = rgba_of(extras["premul"], extras["opacity"])
        elif p == "depth":
            out[p] = depth_of(extras["depth_sum"], extras["opacity"])
        else:
            out[p] = normal_of(extras["normal_sum"])
    return out


def _u8(x):
    return (np.clip(x, 0.0, 1.0) * 255.0).astype(np.uint8)   # truncated, as TSR.render's pictures are


def to_pil(name, image):
    """One view of pass `name` (a float32 numpy array) as a PIL image: color RGB, opacity L, rgba RGBA with straight alpha (the
    colour divided by alpha, 0 where alpha is 0), normal RGB of n * 0.5 + 0.5, depth mode F (float32, untouched)."""
    from PIL import Image

    image = np.asarray(image, np.float32)
    if name == "color":
        return Image.fromarray((image * 255.0).astype(np.uint8))
    if name == "opacity":
        return Image.fromarray(_u8(image))
    if name == "depth":
        return Image.fromarray(np.ascontiguousarray(image))
    if name == "normal":
        return Image.fromarray(_u8(image * np.float32(0.5) + np.float32(0.5)))
    alpha = image[..., 3:]
    straight = np.divide(image[..., :3], alpha, out=np.zeros_like(image[..., :3]), where=alpha > 0)
    return Image.fromarray(_u8(np.concatenate([straight, alpha], axis=-1)))


def convert(views, return_type):
    """{pass: tensor [n_views, H, W, ...]} -> a list of n_views dicts in `return_type` ("pt" waits for nothing)."""
    n_views = next(iter(views.values())).shape[0]
    if return_type == "pt":
        return [{p: v[i] for p, v in views.items()} for i in range(n_views)]
    host = {p: v.cpu().numpy() for p, v in views.items()}
    if return_type == "np":
        return [{p: v[i] for p, v in host.items()} for i in range(n_views)]
    return [{p: to_pil(p, v[i]) for p, v in host.items()} for i in range(n_views)]
