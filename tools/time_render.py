"""Time the ray kernel: one 256^2 and one 512^2 view of a synthetic scene code, 128 samples per ray, median of 21 launches
(HIP events), after 3 warm-up launches.

    python tools/time_render.py
"""
import json
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sculptmate_amd import ops, synth  # noqa: E402
from sculptmate_amd.tsr.cameras import get_spherical_cameras  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    Ws, bs = synth.decoder_lists(synth.decoder_state(seed=1))
    mlp = ops.PackedMLP(Ws, bs, dev)
    planes = ops.ChannelLastPlanes(torch.from_numpy(synth.smooth_triplane(seed=2, scale=3.0)).to(dev))
    out = {"device": torch.cuda.get_device_name(0), "n_samples": 128, "hidden_layers": mlp.n_hidden}
    for side in (256, 512):
        o, d = (t.to(dev) for t in get_spherical_cameras(1, 0.0, 1.9, 40.0, side, side))
        for _ in range(3):
            ops.render_rays(planes, mlp, o, d)
        times = []
        for _ in range(21):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.render_rays(planes, mlp, o, d)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        out["view_%d_ms" % side] = {"median": round(statistics.median(times), 3), "min": round(min(times), 3),
                                    "max": round(max(times), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
