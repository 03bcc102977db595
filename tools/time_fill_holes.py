"""Time fill holes (csrc/mesh_holes.hip, ops.mesh_border_loops / ops.mesh_fill_holes) on the meshes it is meant for --
extract_meshes at 256^3 of the full-size TSR with seeded weights, and simplify=0.1 of it -- and record what it finds and what the
mesh report says before and after.

    python tools/time_fill_holes.py [--runs 5] [--warmup 1] [--out profiles/time_fill_holes.json]

Per mesh: the loop count, the histogram of the loop lengths, the pinched and open counts; for fill_holes = True, 4, 8, 16, 64 the
time of the whole call and its split into topology (the edge table, the border flags, the border count), loops (next, the
doubling rounds, the decision, the totals' readback) and fill (centroids, faces), on inputs that are already checked; the time of
the route device -> host -> NumPy -> device for fill_holes=True; and Mesh.report(self_intersections=True) before and after each
rule: border edges, watertight, volume, intersecting pairs.

Device times: wall clock around the call with a final torch.cuda.synchronize(), after warm-up calls; median and quartiles over
the runs.  No threshold is set here."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _timing import seeded_mesh, timed  # noqa: E402

MC_RES, THRESHOLD = 256, 25.0
RULES = (True, 4, 8, 16, 64)
REPORTED = ("faces", "border_edges", "nonmanifold_edges", "inconsistent_edges", "is_watertight", "is_winding_consistent", "euler",
            "volume", "self_intersections", "self_intersecting_faces")


def host_fill(vertices, faces):
    """The route a caller without the op would take: device -> host, the rule in NumPy (border edges by a sort, the loops by
    walking `next`, fp64 centroids -- not the device's fixed-point bits), the result back to the device."""
    dev = vertices.device
    v, f = vertices.cpu().numpy(), faces.cpu().numpy().astype(np.int64)
    start, end = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    key = np.minimum(start, end) * (len(v) + 1) + np.maximum(start, end)
    _, first, count = np.unique(key, return_index=True, return_counts=True)
    border = np.sort(first[count == 1])
    out, inn = np.bincount(start[border], minlength=len(v)), np.bincount(end[border], minlength=len(v))
    ok = (out == 1) & (inn == 1)
    blocked = ~(ok[start[border]] & ok[end[border]])
    start_of = np.full(len(v), -1, np.int64)
    start_of[start[border]] = np.arange(len(border))
    nxt = np.where(blocked, -1, start_of[end[border]])
    label = np.where(blocked, -1, -2)
    for i in range(len(border)):
        if label[i] != -2:
            continue
        path, cur = [], i
        while label[cur] == -2 and not (path and cur == i):
            path.append(cur)
            cur = nxt[cur]
        label[path] = min(path) if cur == i else label[cur]
    new_v, new_f = [], []
    centre = {}
    for x in np.unique(label[label >= 0]):
        members = np.nonzero(label == x)[0]
        if len(members) >= 4:
            centre[x] = len(v) + len(new_v)
            new_v.append(v[start[border[members]]].astype(np.float64).mean(0))
    for i in np.nonzero(label >= 0)[0]:
        a, b = start[border[i]], end[border[i]]
        if label[i] in centre:
            new_f.append((b, a, centre[label[i]]))
        elif label[i] == i:
            new_f.append((b, a, end[border[nxt[i]]]))
    vo = np.concatenate([v, np.asarray(new_v, np.float32).reshape(-1, 3)])
    fo = np.concatenate([f, np.asarray(new_f, np.int64).reshape(-1, 3)])
    return torch.from_numpy(vo).to(dev), torch.from_numpy(fo).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_fill_holes.json"))
    a = ap.parse_args()
    from sculptmate_amd import ops
    from sculptmate_amd.tsr.mesh import Mesh

    dev = torch.device("cuda:0")
    model, code, mesh = seeded_mesh(dev, MC_RES, THRESHOLD)
    meshes = {"extracted_256": mesh, "simplify_0.1": mesh.simplify(0.1)}
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "meshes": {}}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
            fh.write("\n")

    def reported(m):
        r = m.report(self_intersections=True)
        return {k: r[k] for k in REPORTED}

    for name, m in meshes.items():
        r = result["meshes"][name] = {"rules": {}}
        v, f = m.vertices, m.faces
        loops = m.border_loops()
        lengths = loops.pop("lengths")
        r["loops"] = dict(loops, longest=max(lengths, default=0),
                          length_histogram={str(n): lengths.count(n) for n in sorted(set(lengths))})
        r["report_before"] = reported(m)
        print("%s: %s; before: %s" % (name, json.dumps(loops), json.dumps(r["report_before"])), flush=True)
        save()
        P, F, _ = ops._holes_input(v, f, None, "time_fill_holes")
        for rule in RULES:
            q = r["rules"][str(rule)] = {}
            max_edges = ops.holes_rule(rule)
            s, q["topology"] = timed(lambda: ops._holes_topology(P, F), a.runs, a.warmup)
            s, q["loops"] = timed(lambda: ops._holes_loops(s, max_edges), a.runs, a.warmup)
            _, q["fill"] = timed(lambda: ops._holes_fill(s, P, F, None), a.runs, a.warmup)
            (fv, ff, _, info), q["call"] = timed(lambda: ops.mesh_fill_holes(v, f, rule), a.runs, a.warmup)
            q["info"] = info
            q["report_after"] = reported(Mesh(fv, ff))
            print("%s fill_holes=%s: topology %.2f ms, loops %.2f ms, fill %.2f ms, the call %.2f ms; %s; after: %s" % (
                name, rule, *(q[k]["median_ms"] for k in ("topology", "loops", "fill", "call")), json.dumps(info),
                json.dumps(q["report_after"])), flush=True)
            save()
        (hv, hf), r["host_route_true"] = timed(lambda: host_fill(v, f), a.runs, a.warmup)
        fv, ff = ops.mesh_fill_holes(v, f, True)[:2]
        assert torch.equal(hf, ff.long()) and torch.allclose(hv, fv, rtol=0, atol=1e-6), "the host route and the device disagree"
        print("%s: host route %.2f ms" % (name, r["host_route_true"]["median_ms"]), flush=True)
        save()
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
