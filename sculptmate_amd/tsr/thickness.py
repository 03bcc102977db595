"""ThicknessMap -- what TSR.bake_thickness_map returns beside the mesh: the wall thickness (the shape diameter) per texel of the
mesh's atlas, the map a baker ships beside normal and AO (subsurface / translucency and wear masks) and the scalar field part
segmentation starts from.  Not a Mesh field: it travels beside the mesh and has its own save()."""
import io

import numpy as np
import torch


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def encode16(thickness, scale):
    """thickness (world units) -> uint16, white = thick: round(min(th / scale, 1) * 65535), computed in double; +inf (no wall was
    found) gives 65535, a NaN and a negative value 0."""
    th = np.asarray(thickness, np.float64)
    with np.errstate(all="ignore"):
        unit = np.minimum(th / float(scale), 1.0)
    return np.rint(np.where(np.isnan(unit), 0.0, np.maximum(unit, 0.0)) * 65535.0).astype(np.uint16)


class ThicknessMap:
    """thickness f32 [res, res]: world units, row 0 at the top; per covered texel the mean length, weighted by the cosine to the
       inward normal, of the cone's rays that leave the body through the back of a face (ops.mesh_thickness), +inf where no ray
       did, then padded around the charts like the other maps; 0 where neither a chart nor the padding reaches.
    thinnest f32 [res, res]: the shortest of those rays (+inf when none; 0 outside the charts, not padded).
    valid i32 [res, res]: how many of the rule's rays counted (0 outside the charts).
    mask bool [res, res]: the covered texels.  rule: (k, max_distance) of ops.thickness_rule."""

    def __init__(self, thickness, thinnest, valid, mask, rule=None):
        self.thickness, self.thinnest, self.valid, self.mask = thickness, thinnest, valid, mask
        self.rule = rule

    @property
    def resolution(self):
        return int(self.thickness.shape[0])

    def default_scale(self):
        """The largest finite thickness over the covered texels (1 when there is none, or when it is not positive)."""
        th = _host(self.thickness)[_host(self.mask).astype(bool)]
        th = th[np.isfinite(th)]
        top = float(th.max()) if th.size else 0.0
        return top if top > 0.0 else 1.0

    def image(self, scale=None):
        """The map as 16-bit grey, uint16 [res, res], white = thick: round(min(th / scale, 1) * 65535); scale=None: the largest
        finite value over the covered texels; +inf gives 65535."""
        if scale is None:
            scale = self.default_scale()
        elif not (float(scale) > 0.0 and float(scale) < float("inf")):   # a NaN fails the comparison
            raise ValueError("scale must be None or a finite number > 0, got %r" % (scale,))
        return encode16(_host(self.thickness), scale)

    def pil_image(self, scale=None):
        from PIL import Image

        return Image.fromarray(self.image(scale))   # uint16 -> mode I;16

    def png_bytes(self, scale=None):
        buf = io.BytesIO()
        self.pil_image(scale).save(buf, format="PNG")
        return buf.getvalue()

    def save(self, path, scale=None):
        """A 16-bit grey PNG through Pillow."""
        self.pil_image(scale).save(str(path), format="PNG")

    def info(self):
        """Host statistics over the covered texels (this waits for the device): their number, the share with no valid ray, the
        mean number of valid rays per texel, and the median, 5th percentile and minimum of the finite `thinnest`."""
        mask = _host(self.mask).astype(bool)
        valid = _host(self.valid)[mask]
        thin = _host(self.thinnest)[mask]
        thin = thin[np.isfinite(thin)]
        nan = float("nan")
        return {"covered": int(mask.sum()),
                "no_valid_ray_share": float((valid == 0).mean()) if valid.size else 0.0,
                "valid_rays_per_texel": float(valid.mean()) if valid.size else 0.0,
                "thinnest_median": float(np.median(thin)) if thin.size else nan,
                "thinnest_p5": float(np.percentile(thin, 5)) if thin.size else nan,
                "thinnest_min": float(thin.min()) if thin.size else nan}
