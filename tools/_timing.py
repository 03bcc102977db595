"""What the tools/time_*.py scripts share: the timer, and the full-size seeded model with the mesh they time on."""
import statistics
import time

import torch


def stats(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 2 else [ms[0]] * 3
    return {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4),
            "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def timed(fn, runs, warmup):
    """-> (what the last fn() returned, stats of `runs` calls): wall clock around each call with a final
    torch.cuda.synchronize(), after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, stats(ms)


def seeded_mesh(dev, mc_resolution, threshold):
    """-> (model, code, mesh): the full-size TSR with seeded weights, its density bias shifted so that `threshold` gives a
    surface (as bench.py does), the scene code of one synthetic picture and extract_meshes of it at mc_resolution^3."""
    from sculptmate_amd import synth
    from sculptmate_amd.tsr import TSR

    sd = synth.tsr_state(seed=0)
    model = TSR(pos_embed_mode="scale_factor")
    model.load_state_dict(sd)
    model.to(dev)
    img = torch.from_numpy(synth.composite_rgb(synth.image_rgba(seed=100))).to(dev).contiguous()
    with torch.no_grad():
        synth.calibrate_tsr_density_bias(model, sd, img, 0.015, threshold)
        code = model([img], device=dev)[0].contiguous()
        mesh = model.extract_meshes([code], False, mc_resolution, threshold)[0]
    return model, code, mesh
