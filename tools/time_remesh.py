"""Triangle remesh at the add-on's 'high' setting (vertex_count = 0.75 x vertices), host (sf3d/remesh.py native_remesher) vs
device (sf3d/remesh_device.py device_remesher), on the two meshes bench.py uses: the first 600k faces of the full-size SF3D
Kuhn-grid mesh (vertices compacted), and the whole mesh.

    python tools/time_remesh.py [--runs N] [--host-full] [--json PATH]

Device times: HIP events around the call, after one warm-up call, median of N.  Host times: wall clock, one call (the full mesh
on the host takes about a minute: only with --host-full; otherwise extrapolated from the slab, labelled so).  Per device call:
ms, us per input face, vertices out, topology passes and host readbacks."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sculptmate_amd import synth  # noqa: E402
from sculptmate_amd.sf3d import remesh as rm  # noqa: E402
from sculptmate_amd.sf3d import remesh_device as rd  # noqa: E402
from sculptmate_amd.sf3d.spec import DEFAULT_CFG  # noqa: E402
from sculptmate_amd.sf3d.system import SF3D, Mesh  # noqa: E402


def full_mesh(dev):
    """The SF3D mesh of bench.py's config 4: full-size networks, synthetic weights, density calibrated to ~10 % inside."""
    cfg = dict(DEFAULT_CFG)
    sd = synth.sf3d_state(0, cfg)
    m = SF3D(cfg)
    m.load_state_dict(sd)
    m.to(dev)
    img = torch.from_numpy(synth.composite_rgb(synth.image_rgba(0, 512))).to(dev)
    codes = m.scene_code(img)
    q = m.query_triplane(m._grid_world, codes)
    pre = m.decoder(q, include=["density"])["density"].reshape(-1).log().cpu().numpy()
    shift = np.log(cfg["isosurface_threshold"]) - np.quantile(pre.astype(np.float64), 0.9)
    sd["decoder.heads.density.4.bias"] = (sd["decoder.heads.density.4.bias"] + np.float32(shift)).astype(np.float32)
    m.load_state_dict(sd)
    planes = m.post_process(m.backbone_tokens(m.image_tokens(img)))
    mesh = m.triplane_to_meshes(planes[None])[0]
    del m, q, codes, planes
    torch.cuda.empty_cache()
    return mesh


def slab_of(mesh, nf=600_000):
    nf = min(nf, mesh.t_pos_idx.shape[0])
    used, inv = torch.unique(mesh.t_pos_idx[:nf].reshape(-1), return_inverse=True)
    return Mesh(mesh.v_pos[used].contiguous(), inv.reshape(-1, 3).contiguous())


def time_device(mesh, runs):
    budget = round(0.75 * mesh.v_pos.shape[0])
    rd.device_remesher(mesh, "triangle", budget)  # warm-up
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = rd.device_remesher(mesh, "triangle", budget)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    # passes / readbacks of the whole call: decimate + remesh_botsch (+ subdivide when the budget exceeds the vertices)
    stats = rd.last_stats()
    return float(np.median(ts)), out, stats


def time_host(mesh):
    budget = round(0.75 * mesh.v_pos.shape[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = rm.native_remesher(mesh, "triangle", budget)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


class _Counting:
    """Sums the counters of the device calls of one device_remesher call (last_stats() holds the last call's only)."""

    def __init__(self):
        self.total = {}

    def wrap(self, fn):
        def run(*a, **k):
            r = fn(*a, **k)
            for key, val in rd.last_stats().items():
                self.total[key] = self.total.get(key, 0) + val
            return r
        return staticmethod(run)


def device_row(mesh, runs):
    ms, out, _ = time_device(mesh, runs)
    cnt = _Counting()

    class Box:
        subdivide = cnt.wrap(rd.subdivide_device)
        decimate = cnt.wrap(rd.decimate_device)
        remesh_botsch = cnt.wrap(rd.remesh_botsch_device)

    rd.triangle_remesh_device(mesh, round(0.75 * mesh.v_pos.shape[0]), 10, toolbox=Box)
    nf = mesh.t_pos_idx.shape[0]
    return {"ms": round(ms, 2), "us_per_face": round(ms * 1e3 / nf, 3), "faces_in": int(nf), "vertices_in": int(mesh.v_pos.shape[0]),
            "vertices_out": int(out.v_pos.shape[0]), "faces_out": int(out.t_pos_idx.shape[0]), "passes": cnt.total.get("passes", 0),
            "readbacks": cnt.total.get("readbacks", 0), "collapses": cnt.total.get("collapses", 0),
            "splits": cnt.total.get("splits", 0), "flips": cnt.total.get("flips", 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-full", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    mesh = full_mesh(dev)
    slab = slab_of(mesh)
    res = {"device": torch.cuda.get_device_name(0)}
    th, hout = time_host(slab)
    res["slab_host"] = {"ms": round(th, 1), "us_per_face": round(th * 1e3 / slab.t_pos_idx.shape[0], 2),
                        "vertices_out": int(hout.v_pos.shape[0]), "faces_out": int(hout.t_pos_idx.shape[0])}
    res["slab_device"] = device_row(slab, a.runs)
    res["slab_speedup"] = round(th / res["slab_device"]["ms"], 1)
    print("slab %d faces: host %.1f ms (%d vertices out), device %.2f ms (%d vertices out, %d passes, %d readbacks): %.1fx" % (
        slab.t_pos_idx.shape[0], th, hout.v_pos.shape[0], res["slab_device"]["ms"], res["slab_device"]["vertices_out"],
        res["slab_device"]["passes"], res["slab_device"]["readbacks"], res["slab_speedup"]), flush=True)
    res["full_device"] = device_row(mesh, a.runs)
    print("full %d faces: device %.2f ms (%.3f us/face, %d vertices out, %d passes, %d readbacks)" % (
        mesh.t_pos_idx.shape[0], res["full_device"]["ms"], res["full_device"]["us_per_face"], res["full_device"]["vertices_out"],
        res["full_device"]["passes"], res["full_device"]["readbacks"]), flush=True)
    if a.host_full:
        th, hout = time_host(mesh)
        res["full_host"] = {"ms": round(th, 1), "vertices_out": int(hout.v_pos.shape[0])}
    else:
        res["full_host_extrapolated_ms"] = round(res["slab_host"]["ms"] * mesh.t_pos_idx.shape[0] / slab.t_pos_idx.shape[0], 0)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
