"""Time surface nets on the device (csrc/surface_nets.hip, ops.surface_nets) on the volume it is meant for: the 256^3 two-pass
("filtered") density grid of the full-size TSR with seeded weights, with and without the grid's sign planes.  Beside it, in the
same run on the same volume, ops.marching_cubes as extract_meshes calls it (the yard-stick), and the route a caller has without
the kernels: device -> host, the NumPy restatement tests/_snref.py, host -> device.  Also recorded: vertex and quad counts, border
and non-manifold edges, and the share of triangles whose smallest angle is below 10 degrees, for both extractors.

    python tools/time_surface_nets.py [--runs 21] [--warmup 3] [--no-host] [--out profiles/time_surface_nets.json]

Device times: wall clock around the call with a final torch.cuda.synchronize(), after warm-up calls; median and quartiles over
the runs.  No threshold is set here."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _timing import seeded_mesh, timed  # noqa: E402

MC_RES, THRESHOLD = 256, 25.0


def quality(vertices, faces, quads=None):
    import _snref

    v, f = vertices.cpu().numpy(), faces.cpu().numpy()
    angles = _snref.min_angles_deg(v, f)
    out = {"vertices": int(len(v)), "triangles": int(len(f)), "triangle_edges": _snref.edge_report(f),
           "min_angle_below_10_deg": round(float((angles < 10.0).mean()), 5), "median_min_angle_deg": round(float(np.median(angles)), 3)}
    if quads is not None:
        out["quads"] = int(len(quads))
        out["quad_edges"] = _snref.edge_report(quads.cpu().numpy())
    return out


def host_route(vol, kw):
    """device -> host -> tests/_snref.py -> device."""
    import _snref

    r = _snref.surface_nets(vol.cpu().numpy(), 0.0, kw["vert_div"], kw["vert_mul"], kw["vert_add"], index_dtype=np.int64)
    return tuple(torch.from_numpy(r[k]).to(vol.device) for k in ("verts", "quads", "faces"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_surface_nets.json"))
    a = ap.parse_args()
    from sculptmate_amd import ops

    dev = torch.device("cuda:0")
    model, code, mesh = seeded_mesh(dev, MC_RES, THRESHOLD)
    cfg, info, R = model.renderer.cfg, model.filter_info, MC_RES
    assert info["filtered"] >= 1 and info["margin"] is not None, "the seeded model's grid did not go through the filter"
    with torch.no_grad():
        vol, _ = ops.density_grid_filtered(code, model.decoder, R, info["margin"], coarse=info["coarse"], radius=cfg.radius,
                                           density_bias=cfg.density_bias, out_add=-THRESHOLD)
        signs = ops.filter_sign_planes(R, dev).clone()
    vol = vol.view(R, R, R).clone()
    kw = dict(vert_div=R - 1.0, vert_mul=2.0 * cfg.radius, vert_add=-cfg.radius)
    result = {"device": torch.cuda.get_device_name(0), "resolution": R, "threshold": THRESHOLD,
              "workspace_bytes": int(ops.lib.sculpt_surface_nets_workspace_bytes(R, R, R)),
              "mc_workspace_bytes": int(ops.lib.sculpt_mc_workspace_bytes(R, R, R))}

    (sv, sq, sf), result["surface_nets"] = timed(lambda: ops.surface_nets(vol, 0.0, faces_i64=True, **kw), a.runs, a.warmup)
    (pv, pq, pf), result["surface_nets_sign_planes"] = timed(lambda: ops.surface_nets(vol, 0.0, faces_i64=True, sign_planes=signs, **kw),
                                                             a.runs, a.warmup)
    assert torch.equal(sv.view(torch.int32), pv.view(torch.int32)) and torch.equal(sq, pq) and torch.equal(sf, pf)
    (mv, mf), result["marching_cubes"] = timed(lambda: ops.marching_cubes(vol, 0.0, reference_order=True, **kw), a.runs, a.warmup)
    (nv, nf), result["marching_cubes_sign_planes"] = timed(lambda: ops.marching_cubes(vol, 0.0, reference_order=True, sign_planes=signs, **kw),
                                                           a.runs, a.warmup)
    assert torch.equal(mv.view(torch.int32), nv.view(torch.int32)) and torch.equal(mf, nf)
    result["volume_is_extract_meshes"] = bool(torch.equal(mf, mesh.faces))   # the volume is the one extract_meshes saw
    for name in ("surface_nets", "surface_nets_sign_planes"):
        result[name + "_over_marching_cubes"] = round(result[name]["median_ms"] / result["marching_cubes" + name[len("surface_nets"):]]["median_ms"], 3)
    result["surface_nets_mesh"] = quality(sv, sf, sq)
    result["marching_cubes_mesh"] = quality(mv, mf)
    for name in ("surface_nets", "surface_nets_sign_planes", "marching_cubes", "marching_cubes_sign_planes"):
        r = result[name]
        print("%-28s %.3f ms (quartiles %.3f .. %.3f)" % (name, r["median_ms"], r["q1_ms"], r["q3_ms"]), flush=True)
    for name in ("surface_nets_mesh", "marching_cubes_mesh"):
        print(name, json.dumps(result[name], sort_keys=True), flush=True)
    with torch.no_grad():
        for iso in ("marching_cubes", "surface_nets"):
            result["extract_meshes_" + iso] = timed(lambda: model.extract_meshes([code], False, R, THRESHOLD, isosurface=iso),
                                                    max(1, min(a.runs, 7)), 2)[1]
    print("extract_meshes: marching cubes %.3f ms, surface nets %.3f ms" % (result["extract_meshes_marching_cubes"]["median_ms"],
                                                                         result["extract_meshes_surface_nets"]["median_ms"]), flush=True)
    if not a.no_host:
        (hv, hq, hf), result["host_round_trip"] = timed(lambda: host_route(vol, kw), 1, 0)
        same = torch.equal(hv.view(torch.int32), sv.view(torch.int32)) and torch.equal(hq, sq) and torch.equal(hf, sf)
        result["host_round_trip"]["same_bits_as_device"] = bool(same)
        print("host round trip: %.1f ms (same bits as the device: %s)" % (result["host_round_trip"]["median_ms"], same), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
