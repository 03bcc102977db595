"""CurvatureMap -- what TSR.bake_curvature_map returns beside the mesh: mean and Gaussian curvature per texel of the mesh's atlas,
the map a baker ships beside normal, AO and thickness (grey = flat, white = convex, black = concave; edge wear and dirt masks
are made from it).  Not a Mesh field: it travels beside the mesh and has its own save()."""
import io

import numpy as np
import torch


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def encode16(curvature, scale):
    """curvature (1 / world units, or their square for the Gaussian) -> uint16, 32768 = flat, white = convex:
    round((0.5 + 0.5 clip(x / scale, -1, 1)) * 65535), computed in double; a NaN gives 32768."""
    x = np.asarray(curvature, np.float64)
    with np.errstate(all="ignore"):
        unit = np.clip(x / float(scale), -1.0, 1.0)
    return np.rint((0.5 + 0.5 * np.where(np.isnan(unit), 0.0, unit)) * 65535.0).astype(np.uint16)


class CurvatureMap:
    """mean f32 [res, res]: the mean curvature, 1 / world units, row 0 at the top, positive where the surface is convex
       (ops.bake_curvature), NaN where a covered texel has no valid value, then padded around the charts like the other maps; 0
       where neither a chart nor the padding reaches.
    gauss f32 [res, res]: the Gaussian curvature, 1 / world units squared, likewise.
    mask bool [res, res]: the covered texels.  rule: the rings of ops.curvature_rule."""
    WHICH = ("mean", "gauss")

    def __init__(self, mean, gauss, mask, rule=None):
        self.mean, self.gauss, self.mask = mean, gauss, mask
        self.rule = rule

    @property
    def resolution(self):
        return int(self.mean.shape[0])

    def _channel(self, which):
        if which not in self.WHICH:
            raise ValueError("which must be 'mean' or 'gauss', got %r" % (which,))
        return _host(getattr(self, which))

    def default_scale(self, which="mean"):
        """The largest finite |value| over the covered texels (1 when there is none, or when it is 0)."""
        x = self._channel(which)[_host(self.mask).astype(bool)]
        x = np.abs(x[np.isfinite(x)])
        top = float(x.max()) if x.size else 0.0
        return top if top > 0.0 else 1.0

    def image(self, scale=None, which="mean"):
        """The map as 16-bit grey, uint16 [res, res]: round((0.5 + 0.5 clip(x / scale, -1, 1)) * 65535) -- 32768 is flat, 65535
        convex at `scale` or beyond, 0 as concave; a NaN gives 32768.  scale=None: the largest finite |x| over the covered
        texels."""
        x = self._channel(which)
        if scale is None:
            scale = self.default_scale(which)
        elif not (float(scale) > 0.0 and float(scale) < float("inf")):   # a NaN fails the comparison
            raise ValueError("scale must be None or a finite number > 0, got %r" % (scale,))
        return encode16(x, scale)

    def pil_image(self, scale=None, which="mean"):
        from PIL import Image

        return Image.fromarray(self.image(scale, which))   # uint16 -> mode I;16

    def png_bytes(self, scale=None, which="mean"):
        buf = io.BytesIO()
        self.pil_image(scale, which).save(buf, format="PNG")
        return buf.getvalue()

    def save(self, path, scale=None, which="mean"):
        """A 16-bit grey PNG through Pillow."""
        self.pil_image(scale, which).save(str(path), format="PNG")

    def info(self):
        """Host statistics over the covered texels (this waits for the device): their number, the share without a finite
        value, and the minimum, median and maximum of the finite mean and Gaussian curvature."""
        mask = _host(self.mask).astype(bool)
        out = {"covered": int(mask.sum())}
        nan = float("nan")
        for which in self.WHICH:
            x = self._channel(which)[mask]
            fin = x[np.isfinite(x)]
            out[which + "_not_finite_share"] = float(1.0 - fin.size / x.size) if x.size else 0.0
            for name, fn in (("min", np.min), ("median", np.median), ("max", np.max)):
                out["%s_%s" % (which, name)] = float(fn(fin)) if fin.size else nan
        return out
