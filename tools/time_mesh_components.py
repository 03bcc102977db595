"""Time the connected components of a 256^3 mesh (csrc/mesh_components.hip) stage by stage, on four inputs:

  model     extract_meshes at 256^3 of the full-size TSR with seeded weights (the field varies at the lattice pitch: many
            components);
  spheres   marching cubes of a 256^3 analytic volume, one large sphere and six small ones: nearly every face adds to ONE
            component's counter (the contended case the wave / workgroup aggregation is there for);
  welded    the model mesh plus one degenerate face [root_i, root_i, root_0] per component: the same faces in the same order, the
            same size, but ONE component -- the contended case at the size of `model` (the spheres' mesh is a ninth of it, where
            the launches and the wait for the counts, not the faces, are most of the time);
  floor     one triangle: what the launches, the read-back and the allocations cost with nothing to do.

    python tools/time_mesh_components.py [--runs 21] [--warmup 3] [--out profiles/time_mesh_components.json]

Stages, each wall clock around the call with a final torch.cuda.synchronize(), after warm-up calls, median over the runs with
the quartiles beside it, and each timed a second time in the opposite order:
  label     sculpt_mesh_component_labels: init + union + flatten (and its wait for the error word)
  launch    sculpt_mesh_components_launch + _read under "largest": label + count + select + the scans' totals + the read-back;
            count + select + scans is reported as launch - label
  compact   sculpt_mesh_components_compact alone, on the workspace a launch left
  keep      ops.mesh_keep_components(v, f, "largest"): the two phases and the allocations between them
  report    ops.mesh_components: launch + the roots and counts
Where scipy imports, the host route on the same mesh beside them: device -> host, scipy.sparse.csgraph.connected_components,
numpy compaction of the largest component, host -> device.
What to look for: the inputs should cost about the same per face once the floor is taken off; `welded` several times slower than
`model` would mean that the counters' aggregation is not working.  No threshold is set here."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _timing import seeded_mesh, stats, timed  # noqa: E402

MC_RES, THRESHOLD = 256, 25.0
SPHERES = (((96.0, 96.0, 96.0), 57.2), ((200.0, 48.0, 48.0), 20.8), ((200.0, 120.0, 48.0), 16.4), ((200.0, 184.0, 48.0), 13.2),
           ((48.0, 208.0, 200.0), 18.4), ((120.0, 208.0, 200.0), 18.4), ((208.0, 208.0, 248.0), 25.6))


def sphere_volume(dev):
    g = torch.arange(MC_RES, dtype=torch.float32, device=dev)
    z, y, x = torch.meshgrid(g, g, g, indexing="ij")
    vol = None
    for (c0, c1, c2), r in SPHERES:
        t = r - torch.sqrt((z - c0) ** 2 + (y - c1) ** 2 + (x - c2) ** 2)
        vol = t if vol is None else torch.maximum(vol, t)
    return vol.contiguous()


def host_route(v, f):
    """What a caller does today: the mesh to the host, scipy's components, the largest one compacted in numpy, back."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components

    t = [time.perf_counter()]
    vh, fh = v.cpu().numpy(), f.cpu().numpy()
    t.append(time.perf_counter())
    a = np.concatenate([fh[:, 0], fh[:, 0]])
    b = np.concatenate([fh[:, 1], fh[:, 2]])
    _, ids = connected_components(sp.coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(len(vh), len(vh))), directed=False)
    t.append(time.perf_counter())
    best = np.bincount(ids[fh[:, 0]]).argmax()
    keep_v = ids == best
    keep_f = keep_v[fh[:, 0]]
    new_id = np.cumsum(keep_v) - 1
    v2, f2 = vh[keep_v], new_id[fh[keep_f]]
    t.append(time.perf_counter())
    out = torch.from_numpy(v2).to(v.device), torch.from_numpy(f2).to(v.device)
    torch.cuda.synchronize()
    t.append(time.perf_counter())
    return out, [(q - p) * 1e3 for p, q in zip(t, t[1:])]


def measure(name, v, f, runs, warmup, host=True):
    from sculptmate_amd import _lib, ops

    lib, nv, nf = _lib.lib, int(v.shape[0]), int(f.shape[0])
    i64 = int(f.dtype == torch.int64)
    ws = ops._workspace(("cc", f.device), lib.sculpt_mesh_components_workspace_bytes(nv, nf), f.device)
    labels = torch.empty(nv, dtype=torch.int32, device=f.device)
    counts = (ctypes.c_int64 * 5)()

    def label():
        _lib.check(lib.sculpt_mesh_component_labels(ops._ptr(f), i64, nf, nv, ops._ptr(labels), ops._ptr(ws), ops._stream()))

    def launch():
        _lib.check(lib.sculpt_mesh_components_launch(ops._ptr(f), i64, nf, nv, _lib.CC_KEEP_LARGEST, 0, 0.0, ops._ptr(ws), ops._stream()))
        _lib.check(lib.sculpt_mesh_components_read(ops._ptr(ws), counts))

    launch()
    comps, largest, knv, knf = int(counts[0]), int(counts[1]), int(counts[3]), int(counts[4])
    out_v = torch.empty((knv, 3), dtype=torch.float32, device=f.device)
    out_f = torch.empty((knf, 3), dtype=f.dtype, device=f.device)
    vi, fi = (torch.empty(n, dtype=torch.int64, device=f.device) for n in (knv, knf))

    def compact():
        _lib.check(lib.sculpt_mesh_components_compact(ops._ptr(v), ops._ptr(f), i64, nf, nv, ops._ptr(ws), ops._ptr(out_v), knv,
                                                      ops._ptr(out_f), knf, ops._ptr(vi), ops._ptr(fi), ops._stream()))

    def keep():
        return ops.mesh_keep_components(v, f, "largest")

    def report():
        return ops.mesh_components(f, nv)

    res = {"vertices": nv, "faces": nf, "index_type": str(f.dtype), "components": comps, "faces_of_the_largest": largest,
           "kept_vertices": knv, "kept_faces": knf, "workspace_bytes": int(lib.sculpt_mesh_components_workspace_bytes(nv, nf))}
    routes = [("label", label), ("launch", launch), ("compact", compact), ("keep", keep), ("report", report)]
    for key, fn in routes:
        res[key] = timed(fn, runs, warmup)[1]
    launch()   # (report ran under another rule: the workspace compact reads is a "largest" one again)
    for key, fn in reversed(routes):
        if key == "compact":
            launch()
        res[key + "_again"] = timed(fn, runs, warmup)[1]
    res["count_select_scans_ms"] = round(res["launch"]["median_ms"] - res["label"]["median_ms"], 4)
    res["launch_ns_per_face"] = round(res["launch"]["median_ms"] * 1e6 / nf, 4)
    res["keep_ns_per_face"] = round(res["keep"]["median_ms"] * 1e6 / nf, 4)
    try:
        if host:
            import scipy  # noqa: F401
    except ImportError:
        res["host_route"] = "scipy is not installed here: not measured"
    if host and "host_route" not in res:
        (hv, hf), _ = host_route(v, f)
        kv, kf = keep()[:2]
        res["host_route_gives_the_same_mesh"] = bool(torch.equal(hv, kv)) and bool(torch.equal(hf.to(kf.dtype), kf))
        for tag in ("host_route", "host_route_again"):
            for _ in range(warmup):
                host_route(v, f)
            parts = [host_route(v, f)[1] for _ in range(runs)]
            res[tag] = {"total": stats([sum(p) for p in parts]), "device_to_host": stats([p[0] for p in parts]),
                        "scipy_connected_components": stats([p[1] for p in parts]), "numpy_compaction": stats([p[2] for p in parts]),
                        "host_to_device": stats([p[3] for p in parts])}
    print("%s: %d faces, %d components (largest %d faces): label %.3f ms, launch %.3f ms (count+select+scans %.3f), compact %.3f ms, "
          "keep %.3f ms = %.3f ns/face" % (name, nf, comps, largest, res["label"]["median_ms"], res["launch"]["median_ms"],
                                           res["count_select_scans_ms"], res["compact"]["median_ms"], res["keep"]["median_ms"],
                                           res["keep_ns_per_face"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_mesh_components.json"))
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    from sculptmate_amd import ops

    dev = torch.device("cuda:0")
    model, code, mesh = seeded_mesh(dev, MC_RES, THRESHOLD)
    with torch.no_grad():
        extract = timed(lambda: model.extract_meshes([code], False, MC_RES, THRESHOLD), a.runs, a.warmup)[1]
        extract_kept = timed(lambda: model.extract_meshes([code], False, MC_RES, THRESHOLD, keep_components="largest"), a.runs, a.warmup)[1]
        extract_again = timed(lambda: model.extract_meshes([code], False, MC_RES, THRESHOLD), a.runs, a.warmup)[1]
    sv, sf = ops.marching_cubes(sphere_volume(dev), 0.0, reference_order=True)
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES,
              "extract_meshes": extract, "extract_meshes_keep_largest": extract_kept, "extract_meshes_again": extract_again,
              "model": measure("model", mesh.vertices, mesh.faces, a.runs, a.warmup),
              "spheres": measure("spheres", sv, sf, a.runs, a.warmup)}
    with torch.no_grad():
        roots = ops.mesh_components(mesh.faces, mesh.vertices.shape[0])["roots"].to(mesh.faces.dtype)
        weld = torch.stack([roots, roots, roots[:1].expand(roots.shape[0])], 1)
        welded = torch.cat([mesh.faces, weld]).contiguous()
        tri = torch.tensor([[0, 1, 2]], dtype=mesh.faces.dtype, device=dev)
    result["welded"] = measure("welded", mesh.vertices, welded, a.runs, a.warmup, host=False)
    result["floor"] = measure("floor", mesh.vertices[:3].contiguous(), tri, a.runs, a.warmup, host=False)
    for name in ("model", "spheres", "welded"):
        for stage in ("label", "launch", "keep"):
            over = result[name][stage]["median_ms"] - result["floor"][stage]["median_ms"]
            result[name][stage + "_above_floor_ns_per_face"] = round(over * 1e6 / result[name]["faces"], 4)
    result["welded_to_model_launch_above_floor"] = round(
        result["welded"]["launch_above_floor_ns_per_face"] / result["model"]["launch_above_floor_ns_per_face"], 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
