"""DisplacementMap -- what TSR.bake_displacement_map returns beside the mesh: a scalar height per texel along the low-poly
normal, the map a Multires / displacement workflow applies after subdividing.  Not a Mesh field: it travels
beside the mesh and goes into Mesh.export(path, displacement=...)."""
import io

import numpy as np
import torch

MIDLEVEL = 0.5


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def encode16(height, scale, midlevel=MIDLEVEL):
    """height (world units) -> uint16: round((midlevel + h / scale) * 65535), clamped to 0 .. 65535; computed in double."""
    h = np.asarray(height, np.float64)
    return np.clip(np.rint((float(midlevel) + h / float(scale)) * 65535.0), 0, 65535).astype(np.uint16)


def decode16(code, scale, midlevel=MIDLEVEL):
    """What a displacement node makes of the stored value: (code / 65535 - midlevel) * scale, f32."""
    return ((np.asarray(code, np.float64) / 65535.0 - float(midlevel)) * float(scale)).astype(np.float32)


class DisplacementMap:
    """height f32 [res, res]: world units, row 0 at the top, positive along the mesh's outward normal; the rule's height where
       the texel's search converged (status 0), +0 elsewhere, then padded around the charts like the other maps.
    mask bool [res, res]: the covered texels.  status i32 [res, res]: 0 converged, 1 out of steps, 2 left the trust region, 3 no
       usable value, gradient or direction; -1 not covered.
    max_dist: the trust interval |h| <= max_dist of the search, so every height fits midlevel +- 0.5 at scale = 2 max_dist.
    midlevel, scale: what a displacement node needs: displaced = P + (texel - midlevel) * scale * N.
    evals i32 [res, res], residual0 / residual f32 [res, res]: evaluations per texel and d - target before and after (info())."""

    def __init__(self, height, mask, status, max_dist, evals=None, residual0=None, residual=None, rule=None):
        self.height, self.mask, self.status = height, mask, status
        self.max_dist = float(max_dist)
        self.midlevel = MIDLEVEL
        self.scale = 2.0 * self.max_dist
        self.evals, self.residual0, self.residual = evals, residual0, residual
        self.rule = rule

    @property
    def resolution(self):
        return int(self.height.shape[0])

    def image(self):
        """The map as 16-bit grey, uint16 [res, res]: round((0.5 + h / scale) * 65535), clamped."""
        return encode16(_host(self.height), self.scale, self.midlevel)

    def pil_image(self):
        from PIL import Image

        return Image.fromarray(self.image())   # uint16 -> mode I;16

    def png_bytes(self):
        buf = io.BytesIO()
        self.pil_image().save(buf, format="PNG")
        return buf.getvalue()

    def save(self, path):
        """A 16-bit grey PNG through Pillow."""
        self.pil_image().save(str(path), format="PNG")

    def info(self):
        """Host statistics over the covered texels (this waits for the device): the status histogram, evaluations per texel and
        the median |d - target| before and after the search."""
        mask = _host(self.mask).astype(bool)
        status = _host(self.status)[mask]
        out = {"covered": int(mask.sum()), "status": {int(k): int((status == k).sum()) for k in (0, 1, 2, 3)}}
        if self.evals is not None:
            out["evals_per_texel"] = float(_host(self.evals)[mask].mean()) if mask.any() else 0.0
        for key, value in (("median_abs_residual_before", self.residual0), ("median_abs_residual_after", self.residual)):
            if value is not None:
                r = np.abs(_host(value)[mask])
                r = r[np.isfinite(r)]
                out[key] = float(np.median(r)) if r.size else float("nan")
        return out
