"""Time the quadric-error simplifier (csrc/mesh_simplify.hip, ops.mesh_simplify) on the mesh it is meant for: extract_meshes at
256^3 of the full-size TSR with seeded weights, keep_components="largest", then simplify=0.1.  Beside it, to the same face
count: the device's shortest-edge decimation (sf3d/remesh_device.py decimate_device, mode 0) and the host's
(sculpt_mesh_decimate through sf3d/remesh.py; one run, it takes a while: --no-host leaves it out).
The seeded weights give a field that varies at the lattice pitch, so the largest component is small; the same three are
therefore also timed on the WHOLE mesh (every component, 1.68 M faces), which is the size a trained model's object has.

    python tools/time_simplify.py [--runs 5] [--warmup 1] [--ratio 0.1] [--no-host] [--out profiles/time_simplify.json]

Device times: wall clock around the call with a final torch.cuda.synchronize(), after warm-up calls, median over the runs with
the extremes beside it.  Per call: ms, rounds (topology rebuilds), host readbacks, faces and vertices reached.  No threshold is
set here."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _timing  # noqa: E402

MC_RES, THRESHOLD = 256, 25.0


def timed(fn, runs, warmup):
    """_timing.timed with the extremes only: a few runs of a long call have no quartiles worth reporting."""
    out, t = _timing.timed(fn, runs, warmup)
    return out, {k: t[k] for k in ("median_ms", "min_ms", "max_ms", "runs")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ratio", type=float, default=0.1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_simplify.json"))
    a = ap.parse_args()
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d import remesh as rm
    from sculptmate_amd.sf3d import remesh_device as rd

    dev = torch.device("cuda:0")
    model, code, mesh = _timing.seeded_mesh(dev, MC_RES, THRESHOLD)
    (v, f, _, _), keep = timed(lambda: ops.mesh_keep_components(mesh.vertices, mesh.faces, "largest"), a.runs, a.warmup)
    target = ops.simplify_target(a.ratio, f.shape[0])
    print("mesh: %d faces, largest component %d faces / %d vertices, target %d" % (mesh.faces.shape[0], f.shape[0], v.shape[0], target), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "ratio": a.ratio, "faces": int(mesh.faces.shape[0]),
              "kept_faces": int(f.shape[0]), "kept_vertices": int(v.shape[0]), "target": target, "keep_components": keep}

    def row(name, fn, runs=a.runs):
        (ov, of), t = timed(fn, runs, a.warmup)
        st = rd.last_stats()
        t.update(rounds=st["rounds"], readbacks=st["readbacks"], collapses=st["collapses"], faces_out=int(of.shape[0]),
                 vertices_out=int(ov.shape[0]), us_per_round=round(t["median_ms"] * 1e3 / max(st["rounds"], 1), 1))
        result[name] = t
        print("%s: %.1f ms (%.1f .. %.1f), %d rounds, %d readbacks, %d faces / %d vertices out" % (
            name, t["median_ms"], t["min_ms"], t["max_ms"], t["rounds"], t["readbacks"], t["faces_out"], t["vertices_out"]), flush=True)

    row("simplify", lambda: ops.mesh_simplify(v, f, a.ratio)[:2])
    row("decimate_device", lambda: rd.decimate_device(v, f, num_faces=target)[:2])
    with torch.no_grad():
        full = timed(lambda: model.extract_meshes([code], False, MC_RES, THRESHOLD, keep_components="largest", simplify=a.ratio),
                     a.runs, a.warmup)[1]
    result["extract_meshes_keep_largest_simplify"] = full
    print("extract_meshes(keep_components='largest', simplify=%g): %.1f ms" % (a.ratio, full["median_ms"]), flush=True)

    def host(name, v, f, target):
        t0 = time.perf_counter()
        vh, fh = v.cpu().numpy(), f.cpu().numpy()
        hv, hf, _, _ = rm.decimate(vh, fh, num_faces=target)
        back = torch.from_numpy(np.ascontiguousarray(hv, np.float32)).to(dev), torch.from_numpy(hf).to(dev)
        torch.cuda.synchronize()
        result[name] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "runs": 1, "faces_out": int(back[1].shape[0])}
        print("%s: %.0f ms, %d faces out" % (name, result[name]["ms"], back[1].shape[0]), flush=True)

    if not a.no_host:
        host("decimate_host_round_trip", v, f, target)
    wv, wf = mesh.vertices, mesh.faces
    wtarget = ops.simplify_target(a.ratio, wf.shape[0])
    result["whole_target"] = wtarget
    few = max(1, min(a.runs, 3))
    row("whole_simplify", lambda: ops.mesh_simplify(wv, wf, a.ratio)[:2], few)
    row("whole_decimate_device", lambda: rd.decimate_device(wv, wf, num_faces=wtarget)[:2], few)
    if not a.no_host:
        host("whole_decimate_host_round_trip", wv, wf, wtarget)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh_:
        json.dump(result, fh_, indent=1, sort_keys=True)
        fh_.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
