"""Time the device Catmull-Clark subdivision (csrc/mesh_catmull.hip, ops.mesh_catmull_clark) on the two meshes it is meant for,
both from extract_meshes at 256^3 of the full-size TSR with seeded weights: the all-quad mesh of isosurface="surface_nets", and
the triangles that simplify=0.1 leaves of the marching cubes mesh.  One and two levels of each, split into the topology
constructions (the sorts), the numbering and classification, and the fused refine launch.  Beside it, in the same run, the
yardstick: ops.mesh_subdivide's Loop scheme on the same triangles with the same split; and the route a caller has without the
kernels: device -> host, the NumPy restatement tests/_catmullref.py, host -> device.

    python tools/time_catmull_clark.py [--runs 7] [--warmup 2] [--no-host] [--out profiles/time_catmull_clark.json]

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
    """device -> host -> tests/_catmullref.py -> device."""
    import _catmullref

    P, Q, T, _ = _catmullref.subdivide(v.cpu().numpy(), f.cpu().numpy(), levels)
    return tuple(torch.from_numpy(x).to(v.device) for x in (P, Q, T))


def catmull_split(rd, lib, check, v, f, levels, runs, warmup):
    """-> (topology ms, numbering + classify ms, refine ms) summed over the levels, each level on its own input."""
    p = rd._p
    P, F = v.to(torch.float32).contiguous(), f.to(torch.int32).contiguous()
    total = [0.0, 0.0, 0.0]
    for _ in range(levels):
        ctx = rd._Ctx()
        T, t = timed(lambda: rd._PolyTopo(rd._Ctx(), F, P.shape[0]), runs, warmup)
        nv, dev, s = P.shape[0], P.device, ctx.stream
        first = torch.empty(T.k * T.nf, dtype=torch.int32, device=dev)
        cls = torch.empty((nv, 4), dtype=torch.int32, device=dev)
        rows = torch.empty((nv, 4), dtype=torch.float32, device=dev)

        def number():
            check(lib.sculpt_catmull_first_halfedge(T.ref(), p(first), s))
            rank = torch.cumsum(first, 0, dtype=torch.int32)
            check(lib.sculpt_catmull_classify(T.ref(), p(P), p(cls), p(rows), s))
            return rank

        rank, c = timed(number, runs, warmup)
        n = nv + T.nf + T.ne
        Po = torch.empty((n, 3), dtype=torch.float32, device=dev)
        Qo = torch.empty((T.k * T.nf, 4), dtype=torch.int32, device=dev)
        To = torch.empty((2 * T.k * T.nf, 3), dtype=torch.int32, device=dev)
        _, r = timed(lambda: check(lib.sculpt_catmull_refine(T.ref(), p(cls), p(rows), p(rank), None, 0, p(Po), p(Qo), p(To), None, s)),
                     runs, warmup)
        for i, x in enumerate((t, c, r)):
            total[i] += x["median_ms"]
        P, F = Po, Qo
    return tuple(round(x, 4) for x in total), (P, F)


def loop_split(rd, lib, check, v, f, levels, runs, warmup):
    """The same split of the Loop route (sf3d.remesh_device._loop_level's calls)."""
    p = rd._p
    P, F = rd._inputs(v, f, "time_catmull_clark")
    total = [0.0, 0.0, 0.0]
    for _ in range(levels):
        ctx = rd._Ctx()
        T, t = timed(lambda: rd._loop_topology(rd._Ctx(), F, P.shape[0]), runs, warmup)
        nv, dev, s = P.shape[0], P.device, ctx.stream
        first = torch.empty(3 * T.nf, dtype=torch.int32, device=dev)
        cls = torch.empty((nv, 4), dtype=torch.int32, device=dev)
        rows = torch.empty((nv, 4), dtype=torch.float32, device=dev)

        def number():
            check(lib.sculpt_rmd_first_halfedge(T.ref(), p(first), s))
            rank = torch.cumsum(first, 0, dtype=torch.int32)
            check(lib.sculpt_subdiv_classify(T.ref(), p(P), p(cls), p(rows), s))
            return rank

        rank, c = timed(number, runs, warmup)
        Po = torch.empty((nv + T.ne, 3), dtype=torch.float32, device=dev)
        Fo = torch.empty((4 * T.nf, 3), dtype=torch.int32, device=dev)
        _, r = timed(lambda: check(lib.sculpt_subdiv_loop(T.ref(), p(cls), p(rows), p(rank), None, 0, p(Po), p(Fo), None, s)), runs, warmup)
        for i, x in enumerate((t, c, r)):
            total[i] += x["median_ms"]
        P, F = Po, Fo
    return tuple(round(x, 4) for x in total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_catmull_clark.json"))
    a = ap.parse_args()
    from sculptmate_amd import ops
    from sculptmate_amd._lib import check, lib
    from sculptmate_amd.sf3d import remesh_device as rd

    dev = torch.device("cuda:0")
    model, code, mesh = seeded_mesh(dev, MC_RES, THRESHOLD)
    with torch.no_grad():
        nets = model.extract_meshes([code], False, MC_RES, THRESHOLD, isosurface="surface_nets")[0]
    sv, sf = ops.mesh_simplify(mesh.vertices, mesh.faces, SIMPLIFY)[:2]
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "simplify": SIMPLIFY, "cages": {}}
    cages = {"surface_nets_quads": (nets.vertices, nets.quads), "simplified_triangles": (sv, sf)}
    for name, (v, f) in cages.items():
        c = result["cages"][name] = {"vertices": int(v.shape[0]), "faces": int(f.shape[0]), "corners": int(f.shape[1]), "levels": {}}
        print("%s: %d vertices, %d faces of %d corners" % (name, v.shape[0], f.shape[0], f.shape[1]), flush=True)
        for levels in (1, 2):
            r = c["levels"][str(levels)] = {}
            (gv, gq, gt, _), r["catmull_clark"] = timed(lambda: ops.mesh_catmull_clark(v, f, levels), a.runs, a.warmup)
            r["catmull_clark"]["readbacks"] = rd.last_stats()["readbacks"]
            r["vertices"], r["quads"] = int(gv.shape[0]), int(gq.shape[0])
            (r["topology_ms"], r["numbering_classify_ms"], r["refine_ms"]), (P, Q) = catmull_split(rd, lib, check, v, f, levels, a.runs, a.warmup)
            assert torch.equal(P, gv) and torch.equal(Q, gq.to(Q.dtype))
            line = "  %d level(s): catmull_clark %.3f ms (quartiles %.3f .. %.3f) = topology %.3f + numbering/classify %.3f + refine %.3f + input check; %d quads" % (
                levels, r["catmull_clark"]["median_ms"], r["catmull_clark"]["q1_ms"], r["catmull_clark"]["q3_ms"], r["topology_ms"],
                r["numbering_classify_ms"], r["refine_ms"], r["quads"])
            if f.shape[1] == 3:   # the yardstick: Loop on the same triangles
                (lv, lf, _), r["loop"] = timed(lambda: ops.mesh_subdivide(v, f, levels), a.runs, a.warmup)
                r["loop_topology_ms"], r["loop_numbering_classify_ms"], r["loop_mask_ms"] = loop_split(rd, lib, check, v, f, levels, a.runs, a.warmup)
                r["loop_faces"] = int(lf.shape[0])
                r["catmull_clark_over_loop"] = round(r["catmull_clark"]["median_ms"] / r["loop"]["median_ms"], 3)
                line += "; loop %.3f ms = topology %.3f + numbering/classify %.3f + masks %.3f, %d faces; ratio %.3f" % (
                    r["loop"]["median_ms"], r["loop_topology_ms"], r["loop_numbering_classify_ms"], r["loop_mask_ms"], r["loop_faces"],
                    r["catmull_clark_over_loop"])
            print(line, flush=True)
        if not a.no_host:
            want = ops.mesh_catmull_clark(v, f, 1)
            (hv, hq, ht), c["host_round_trip"] = timed(lambda: host_route(v, f, 1), 1, 0)
            same = (torch.equal(hv.view(torch.int32), want[0].view(torch.int32)) and torch.equal(hq.long(), want[1].long())
                    and torch.equal(ht.long(), want[2].long()))
            c["host_round_trip"]["same_bits_as_device"] = bool(same)
            print("  host round trip, one level: %.1f ms (same bits as the device: %s)" % (c["host_round_trip"]["median_ms"], same), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
