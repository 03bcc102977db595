"""Time the render passes: one 256^2 view of a synthetic scene code, 128 samples per ray, median of 21 calls (HIP events) after
3 warm-up calls, for the colour picture alone through both entry points, each added pass, all passes (with and without the exact
skip of the forward-mode kernel) and the composed route the passes replace: render_rays with weights and z_vals, xyz in torch,
ops.field_normals at the 8.4 M sample points, torch sums.  Writes profiles/time_render_passes.json and prints it.

    python tools/time_render_passes.py
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sculptmate_amd import ops, synth  # noqa: E402
from sculptmate_amd.tsr.cameras import get_spherical_cameras  # noqa: E402

SIDE, S = 256, 128


def timed(fn):
    for _ in range(3):
        fn()
    times = []
    for _ in range(21):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    q = statistics.quantiles(times, n=4)
    return {"median": round(statistics.median(times), 3), "q1": round(q[0], 3), "q3": round(q[2], 3), "min": round(min(times), 3),
            "max": round(max(times), 3)}


def main():
    dev = torch.device("cuda:0")
    Ws, bs = synth.decoder_lists(synth.decoder_state(seed=1))
    mlp = ops.PackedMLP(Ws, bs, dev)
    planes = ops.ChannelLastPlanes(torch.from_numpy(synth.smooth_triplane(seed=2, scale=3.0)).to(dev))
    o, d = (t.to(dev).reshape(-1, 3) for t in get_spherical_cameras(1, 0.0, 1.9, 40.0, SIDE, SIDE))
    every = ("opacity", "depth_sum", "normal_sum", "premul")

    def passes(want):
        return lambda: ops.render_passes(planes, mlp, o, d, n_samples=S, want=want)

    def composed():
        _, ex = ops.render_rays(planes, mlp, o, d, n_samples=S, want=("opacity", "weights", "z_vals"))
        w, z = ex["weights"], ex["z_vals"]
        xyz = o[:, None, :] + z[..., None] * d[:, None, :]
        n = ops.field_normals(planes, mlp, xyz)["normal"]
        return (w * z).sum(-1), (w[..., None] * n).sum(-2)

    out = {"device": torch.cuda.get_device_name(0), "view": "%d x %d x %d" % (SIDE, SIDE, S), "hidden_layers": mlp.n_hidden,
           "unit": "ms", "field": "synth.smooth_triplane(seed=2, scale=3.0), synth.decoder_state(seed=1)"}
    os.environ.pop("SCULPT_RENDER_FORM", None)
    out["color_render_rays"] = timed(lambda: ops.render_rays(planes, mlp, o, d, n_samples=S))
    out["color_render_passes"] = timed(passes(()))
    out["color_opacity"] = timed(passes(("opacity",)))
    out["color_depth_sum"] = timed(passes(("depth_sum",)))
    out["color_premul"] = timed(passes(("premul",)))
    out["color_normal_sum"] = timed(passes(("normal_sum",)))
    out["all_passes"] = timed(passes(every))
    os.environ["SCULPT_RENDER_FORM"] = "noskip"
    out["all_passes_noskip"] = timed(passes(every))
    os.environ.pop("SCULPT_RENDER_FORM")
    out["composed_route"] = timed(composed)
    # what the skip had to work with on this field: the share of (tile of 8 rays, sample) steps up to each tile's last weight != 0
    _, ex = ops.render_rays(planes, mlp, o, d, n_samples=S, want=("weights",))
    nz = (ex["weights"] != 0).reshape(-1, 8, S).any(1)
    steps = torch.where(nz, torch.arange(1, S + 1, device=dev)[None], torch.zeros((), dtype=torch.long, device=dev)).amax(1)
    out["tile_steps_up_to_the_last_nonzero_weight"] = round(float(steps.double().mean()) / S, 4)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "time_render_passes.json"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
