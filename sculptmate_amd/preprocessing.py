"""The add-on's input-side caller of the generators, with the reference's name and behaviour:
`preprocess_image(img_path, ratio=0.85, use_alpha=False)` (/root/reference/preprocessing.py:73-127; called at
GUIPanel.py:158 with ratio=0.75 for TripoSR and at :160 with ratio=0.85, use_alpha=True for StableFast-3D).

Background removal runs on the MI355X U^2-Net (sculptmate_amd.rembg); the rest is a handful of host-side array
operations on one image (bounding box of alpha > 0 with the reference's exclusive max, square padding, border so the
object fills `ratio` of the side, grey composite, LANCZOS to 1024^2).  The reference opens a new onnxruntime session on
every call (rembg/bg.py:200-201); here one session per device is kept for the process lifetime.
"""
import numpy as np
from PIL import Image

image_size = (1024, 1024)
_sessions = {}


def _session(device):
    from .rembg.session import new_session

    key = str(device)
    if key not in _sessions:
        _sessions[key] = new_session("u2net", device=device)
    return _sessions[key]


def _cutout(raw, session=None, device="cuda:0"):
    """rembg's remove() on the HIP U^2-Net -> RGBA PIL image."""
    from .rembg.bg import remove

    return remove(raw, session=session if session is not None else _session(device))


def frame_layout(h, w, ratio):
    """The frame of an h x w box: (side of the frame, top, left of the box in it) -- zero padding to the square max(h, w), then to
    int(that / ratio); an odd remainder goes to the bottom / right both times.  Shared by frame_foreground and the device path."""
    square = max(h, w)
    side = int(square / ratio)
    if side < square:
        raise ValueError("frame_layout: ratio %r would crop the object (a %d-pixel frame for %d pixels)" % (ratio, side, square))
    border = (side - square) // 2
    return side, (square - h) // 2 + border, (square - w) // 2 + border


def frame_foreground(rgba: np.ndarray, ratio: float) -> np.ndarray:
    """uint8 RGBA cut-out -> square RGBA with the object's bounding box scaled to `ratio` of the side
    (preprocessing.py:81-110).  The box is [min, max) on both axes, as the reference slices it."""
    ys, xs = np.nonzero(rgba[..., 3] > 0)
    if ys.size == 0:
        raise ValueError("preprocess_image: the cut-out is empty (alpha is zero everywhere)")
    fg = rgba[ys.min():ys.max(), xs.min():xs.max()]
    side, top, left = frame_layout(fg.shape[0], fg.shape[1], ratio)
    out = np.zeros((side, side, fg.shape[2]), fg.dtype)
    out[top:top + fg.shape[0], left:left + fg.shape[1]] = fg
    return out


def preprocess_image(img_path, ratio=0.85, use_alpha=False, session=None, device="cuda:0"):
    """Image file -> the generator's input.  use_alpha=True: framed RGBA at native size (StableFast-3D composites it
    itself); otherwise RGB composited on 0.5 grey and resized to 1024 x 1024, or None when the framed image is
    narrower than 250 px.  `session`: a rembg session to reuse (default: one U2netSession per device)."""
    raw = Image.open(img_path)
    if use_alpha:
        raw = raw.convert("RGBA")
    return _preprocess_decoded(raw, ratio, use_alpha, session, device)


def _preprocess_decoded(raw, ratio, use_alpha, session, device):
    """preprocess_image after the file is decoded (and converted to RGBA for use_alpha)."""
    cut = _cutout(raw, session, device)
    framed = frame_foreground(np.array(cut), ratio)
    if use_alpha:
        return Image.fromarray(framed, mode="RGBA")
    x = framed.astype(np.float32) / 255.0
    rgb = x[:, :, :3] * x[:, :, 3:4] + (1 - x[:, :, 3:4]) * 0.5
    out = Image.fromarray((rgb * 255.0).astype(np.uint8))
    if out.size[0] < 250:
        return None
    return out.resize(image_size, Image.Resampling.LANCZOS)


def preprocess_image_device(img_path, ratio=0.85, use_alpha=False, session=None, device="cuda:0"):
    """preprocess_image with everything after the decode on the device: the decoded uint8 picture is uploaded once and the result
    stays in HBM -- a float32 [1024, 1024, 3] tensor, what TSR.forward / TripoGenerator.generate_mesh would have made of
    preprocess_image's PIL image (or None where that returns None); for use_alpha=True the framed uint8 [S, S, 4] RGBA tensor.
    Every value equals the host path's bit for bit given the same network output.  The only readback is the cut-out's bounding
    box (four integers), which sizes the frame.  `img_path`: a file or a PIL image.  Pictures whose mode is neither RGB nor RGBA
    take the host path and are uploaded at the end.  A `session` runs on its own device; `device` picks the default session."""
    import torch

    from . import ops
    from .rembg.bg import fix_image_orientation

    raw = img_path if isinstance(img_path, Image.Image) else Image.open(img_path)
    if use_alpha:
        raw = raw.convert("RGBA")
    sess = session if session is not None else _session(device)
    if raw.mode not in ("RGB", "RGBA"):
        out = _preprocess_decoded(raw, ratio, use_alpha, sess, device)
        if out is None:
            return None
        a = np.array(out)
        return torch.from_numpy(a if use_alpha else a.astype(np.float32) / 255.0).to(sess.device)
    img = torch.from_numpy(np.array(fix_image_orientation(raw))).to(sess.device)
    mask = sess.predict_device(img)
    box = ops.cutout_bbox(img, mask)
    if box is None:
        raise ValueError("preprocess_image: the cut-out is empty (alpha is zero everywhere)")
    ymin, ymax, xmin, xmax = box
    h, w = ymax - ymin, xmax - xmin          # the box is [min, max) on both axes, as frame_foreground slices it
    side, top, left = frame_layout(h, w, ratio)
    if use_alpha:
        return ops.cutout_frame(img, mask, ymin, xmin, h, w, top, left, side, grey=False)
    if side < 250:
        return None
    grey = ops.cutout_frame(img, mask, ymin, xmin, h, w, top, left, side, grey=True)
    return ops.u8_to_unit_f32(ops.resample_lanczos_u8(grey, image_size[1], image_size[0]))
