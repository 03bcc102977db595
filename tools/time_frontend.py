"""Time the image front end: the host path (preprocessing.preprocess_image) against the device path
(preprocessing.preprocess_image_device) on the same box and the same commit.

    python tools/time_frontend.py [--runs 21] [--warmup 3] [--out profiles/time_frontend.json]

Inputs are synthetic pictures (a textured disc on a flat background) of 1024 x 1024, 2048 x 2048 and 4096 x 3072, written as
uncompressed BMP files so that the decode, which both paths share, stays small.  Every figure is wall clock around the whole
call including a final torch.cuda.synchronize(), after warm-up calls, as the median over the runs with the quartiles beside it.
U^2-Net runs with seeded weights in both paths (its time is reported on its own); because seeded weights give no usable mask,
the network's output is replaced AFTER it ran by a stored disc-shaped d0, so that the bounding box, the frame and the last
resize see a realistic object.  The device path's stages are timed in a separate pass with a synchronize after each stage.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from _timing import stats, timed  # noqa: E402

SIZES = [(1024, 1024), (2048, 2048), (4096, 3072)]


def disc_picture(width, height, seed):
    from sculptmate_amd import synth

    yy, xx = np.mgrid[0:height, 0:width]
    r = np.hypot((xx - 0.52 * width) / (0.30 * width), (yy - 0.47 * height) / (0.36 * height))
    tile = synth.image_rgba(seed, 512)[..., :3]
    tex = np.tile(tile, (height // 512 + 1, width // 512 + 1, 1))[:height, :width]
    pic = np.where((r < 1.0)[..., None], tex, np.uint8(230)).astype(np.uint8)
    y3, x3 = np.mgrid[0:320, 0:320]
    r3 = np.hypot((x3 + 0.5 - 0.52 * 320) / (0.30 * 320), (y3 + 0.5 - 0.47 * 320) / (0.36 * 320))
    d0 = 1.0 / (1.0 + np.exp((r3 - 1.0) * 14.0)) * 0.98 + 0.01
    return pic, d0.astype(np.float32)


def device_stages(path, ratio, sess, runs, warmup):
    """The device path once more, stage by stage, with a synchronize after each (so the sum exceeds the whole call's time)."""
    from sculptmate_amd import ops, preprocessing
    from sculptmate_amd.rembg import session as S

    acc = {}

    def lap(name, t0):
        torch.cuda.synchronize()
        acc.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)

    for i in range(warmup + runs):
        if i == warmup:
            acc.clear()
        t = time.perf_counter()
        raw = np.array(Image.open(path))
        lap("decode", t)
        t = time.perf_counter()
        img = torch.from_numpy(raw).to(sess.device)
        lap("upload", t)
        t = time.perf_counter()
        small = ops.resample_lanczos_u8(img, 320, 320)
        x = ops.u2net_input(small, S.MEAN, S.STD)
        lap("resize_320_and_input", t)
        t = time.perf_counter()
        d0 = sess.net.forward(x)
        lap("u2net", t)
        t = time.perf_counter()
        mask = ops.resample_lanczos_u8(ops.u2net_mask(d0), img.shape[0], img.shape[1])
        lap("mask_and_resize_back", t)
        t = time.perf_counter()
        ymin, ymax, xmin, xmax = ops.cutout_bbox(img, mask)
        lap("bbox_readback", t)
        t = time.perf_counter()
        h, w = ymax - ymin, xmax - xmin
        side, top, left = preprocessing.frame_layout(h, w, ratio)
        grey = ops.cutout_frame(img, mask, ymin, xmin, h, w, top, left, side, grey=True)
        lap("cutout_frame_grey", t)
        t = time.perf_counter()
        ops.u8_to_unit_f32(ops.resample_lanczos_u8(grey, 1024, 1024))
        lap("resize_1024_and_float", t)
    return {k: stats(v) for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=0.75)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_frontend.json"))
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    from sculptmate_amd import preprocessing, synth
    from sculptmate_amd.rembg import session as S
    from sculptmate_amd.tsr.system import _to_float_hwc

    dev = torch.device("cuda:0")
    sess = S.U2netSession(device=dev, state_dict=synth.u2net_state(0))
    real_forward = sess.net.forward
    stored = {}

    def forward(x):
        real_forward(x)
        return stored["d0"].clone()

    x320 = torch.randn(3, 320, 320, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "ratio": a.ratio, "u2net_forward_320": timed(lambda: real_forward(x320), a.runs, a.warmup)[1],
              "sizes": {}}
    sess.net.forward = forward
    with tempfile.TemporaryDirectory() as tmp:
        for width, height in SIZES:
            pic, d0 = disc_picture(width, height, 7)
            stored["d0"] = torch.from_numpy(d0).to(dev)
            path = os.path.join(tmp, "disc_%dx%d.bmp" % (width, height))
            Image.fromarray(pic, mode="RGB").save(path)

            def host():
                # what the add-on's call site does today: the PIL image, then TSR's conversion and upload
                return _to_float_hwc(preprocessing.preprocess_image(path, ratio=a.ratio, session=sess)).to(dev)

            def device():
                return preprocessing.preprocess_image_device(path, ratio=a.ratio, session=sess)

            same = bool(torch.equal(host(), device()))
            entry = {"host": timed(host, a.runs, a.warmup)[1], "device": timed(device, a.runs, a.warmup)[1], "bit_identical": same,
                     "device_stages": device_stages(path, a.ratio, sess, a.runs, a.warmup)}
            result["sizes"]["%dx%d" % (width, height)] = entry
            print("%dx%d: host %.1f ms, device %.1f ms, identical %s" % (width, height, entry["host"]["median_ms"],
                                                                        entry["device"]["median_ms"], same), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"u2net_forward_320_ms": result["u2net_forward_320"]["median_ms"], "out": a.out}))


if __name__ == "__main__":
    main()
