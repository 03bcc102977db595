"""Time the device Loop subdivision (csrc/mesh_subdivide.hip, ops.mesh_subdivide) on the mesh it is meant for: extract_meshes at
256^3 of the full-size TSR with seeded weights, reduced by simplify=0.1 -- the light, irregular cage that subdivision refines.
One and two levels, split into the topology constructions (the sorts) and the kernels (numbering, classification, the fused
mask launch).  Beside it the midpoint upsampling of the same levels (sf3d.remesh_device.subdivide_device: the same topology, one
kernel), and the route a caller has without the kernels: device -> host, the NumPy restatement tests/_loopref.py, host -> device.

    python tools/time_subdivide.py [--runs 7] [--warmup 2] [--no-host] [--out profiles/time_subdivide.json]

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

import torch  # noqa: E402

from _timing import seeded_mesh, timed  # noqa: E402

MC_RES, THRESHOLD, SIMPLIFY = 256, 25.0, 0.1


def host_route(v, f, levels):
    """device -> host -> tests/_loopref.py -> device."""
    import _loopref

    P, F, _ = _loopref.subdivide(v.cpu().numpy(), f.cpu().numpy(), levels)
    return torch.from_numpy(P).to(v.device), torch.from_numpy(F).to(v.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_subdivide.json"))
    a = ap.parse_args()
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d import remesh_device as rd

    dev = torch.device("cuda:0")
    model, code, mesh = seeded_mesh(dev, MC_RES, THRESHOLD)
    v, f = ops.mesh_simplify(mesh.vertices, mesh.faces, SIMPLIFY)[:2]
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "simplify": SIMPLIFY, "plain_faces": int(mesh.faces.shape[0]),
              "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "levels": {}}
    print("mesh: %d faces, simplify=%g: %d vertices, %d faces" % (mesh.faces.shape[0], SIMPLIFY, v.shape[0], f.shape[0]), flush=True)
    _, result["inputs_check"] = timed(lambda: rd._inputs(v, f, "time_subdivide"), a.runs, a.warmup)

    for levels in (1, 2):
        r = result["levels"][str(levels)] = {}
        (lv, lf, _), r["loop"] = timed(lambda: ops.mesh_subdivide(v, f, levels), a.runs, a.warmup)
        r["loop"]["readbacks"] = rd.last_stats()["readbacks"]
        (mv, mf), r["midpoint"] = timed(lambda: rd.subdivide_device(v, f, levels), a.runs, a.warmup)
        assert torch.equal(lf, mf.to(lf.dtype))
        r["loop_over_midpoint"] = round(r["loop"]["median_ms"] / r["midpoint"]["median_ms"], 3)
        r["vertices"], r["faces"] = int(lv.shape[0]), int(lf.shape[0])
        # the split, level by level on the level's own input
        P, F = rd._inputs(v, f, "time_subdivide")
        topo_ms = kernel_ms = 0.0
        for _ in range(levels):
            T, t = timed(lambda: rd._loop_topology(rd._Ctx(), F, P.shape[0]), a.runs, a.warmup)
            (P2, F2, _), k = timed(lambda: rd._loop_level(rd._Ctx(), T, P), a.runs, a.warmup)
            topo_ms, kernel_ms = topo_ms + t["median_ms"], kernel_ms + k["median_ms"]
            P, F = P2, F2
        assert torch.equal(P, lv) and torch.equal(F, lf.to(F.dtype))
        r["topology_ms"], r["kernels_ms"] = round(topo_ms, 4), round(kernel_ms, 4)
        print("%d level(s): loop %.3f ms (quartiles %.3f .. %.3f) = topology %.3f + kernels %.3f + input check; midpoint %.3f ms; "
              "ratio %.3f; %d faces" % (levels, r["loop"]["median_ms"], r["loop"]["q1_ms"], r["loop"]["q3_ms"], topo_ms, kernel_ms,
                                        r["midpoint"]["median_ms"], r["loop_over_midpoint"], r["faces"]), flush=True)
        with torch.no_grad():
            r["extract_meshes"] = timed(lambda: model.extract_meshes([code], False, MC_RES, THRESHOLD, simplify=SIMPLIFY, subdivide=levels),
                                        max(1, min(a.runs, 3)), 1)[1]
    with torch.no_grad():
        result["extract_meshes_simplify_only"] = timed(lambda: model.extract_meshes([code], False, MC_RES, THRESHOLD, simplify=SIMPLIFY),
                                                       max(1, min(a.runs, 3)), 1)[1]
    print("extract_meshes: simplify alone %.1f ms, + subdivide=1 %.1f ms, + subdivide=2 %.1f ms" % (
        result["extract_meshes_simplify_only"]["median_ms"], result["levels"]["1"]["extract_meshes"]["median_ms"],
        result["levels"]["2"]["extract_meshes"]["median_ms"]), flush=True)
    if not a.no_host:
        want = ops.mesh_subdivide(v, f, 1)
        (hv, hf), result["host_round_trip"] = timed(lambda: host_route(v, f, 1), 1, 0)
        same = torch.equal(hv.view(torch.int32), want[0].view(torch.int32)) and torch.equal(hf, want[1])
        result["host_round_trip"]["same_bits_as_device"] = bool(same)
        print("host round trip, one level: %.1f ms (same bits as the device: %s)" % (result["host_round_trip"]["median_ms"], same), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
