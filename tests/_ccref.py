"""numpy restatement of ops.mesh_components / ops.mesh_keep_components (csrc/mesh_components.hip): integer work, so every
comparison against it is equality.

Labels: min-propagation over the face edges (np.minimum.at) plus pointer jumping (lab = lab[lab]) until nothing changes ->
labels[v] = the smallest vertex index of v's component.  Counts by np.bincount.  Selection and stable compaction as the header
states them.  Nf == 0: the device code launches nothing and reports no component (none has a face); labels are arange(Nv)."""
import numpy as np


def labels(faces, n_vertices):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lab = np.arange(n_vertices, dtype=np.int64)
    if len(f) == 0:
        return lab
    a = np.concatenate([f[:, 0], f[:, 0]])
    b = np.concatenate([f[:, 1], f[:, 2]])
    while True:
        old = lab.copy()
        m = np.minimum(lab[a], lab[b])
        np.minimum.at(lab, a, m)
        np.minimum.at(lab, b, m)
        while True:   # pointer jumping
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        if np.array_equal(lab, old):
            return lab


def components(faces, n_vertices):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lab = labels(f, n_vertices)
    if len(f) == 0:
        e = np.zeros(0, np.int32)
        return {"labels": lab.astype(np.int32), "roots": e, "face_counts": e, "vertex_counts": e}
    roots = np.flatnonzero(lab == np.arange(n_vertices))
    fc = np.bincount(lab[f[:, 0]], minlength=n_vertices)[roots]
    vc = np.bincount(lab, minlength=n_vertices)[roots]
    return {"labels": lab.astype(np.int32), "roots": roots.astype(np.int32), "face_counts": fc.astype(np.int32),
            "vertex_counts": vc.astype(np.int32)}


def kept_roots(comp, keep):
    """The roots `keep` selects: "largest" (most faces, then the smallest root), an int (at least that many faces), a float x in
    (0, 1) ((double)count >= x * (double)largest count).  A component without faces is never kept."""
    roots, fc = comp["roots"].astype(np.int64), comp["face_counts"].astype(np.int64)
    if len(roots) == 0:
        return roots
    if isinstance(keep, str):
        assert keep == "largest"
        best = np.flatnonzero(fc == fc.max())[0]   # roots ascend: the first of the maxima has the smallest root
        sel = np.zeros(len(roots), bool)
        sel[best] = True
    elif isinstance(keep, (int, np.integer)) and not isinstance(keep, bool):
        sel = fc >= int(keep)
    else:
        sel = fc.astype(np.float64) >= np.float64(keep) * np.float64(fc.max())
    return roots[sel & (fc > 0)]


def keep_components(vertices, faces, keep):
    """-> (vertices', faces' re-indexed in faces' dtype, vertex_index i64, face_index i64): the input with rows deleted."""
    v = np.asarray(vertices)
    f = np.asarray(faces)
    comp = components(f, len(v))
    lab = comp["labels"].astype(np.int64)
    ok = np.zeros(len(v) + 1, bool)
    ok[kept_roots(comp, keep)] = True
    keep_v = ok[lab] if len(f) else np.zeros(len(v), bool)
    keep_f = keep_v[f[:, 0]] if len(f) else np.zeros(0, bool)
    vi = np.flatnonzero(keep_v).astype(np.int64)
    fi = np.flatnonzero(keep_f).astype(np.int64)
    new_id = np.full(len(v), -1, np.int64)
    new_id[vi] = np.arange(len(vi))
    return v[vi], new_id[f[fi].astype(np.int64)].astype(f.dtype).reshape(-1, 3), vi, fi


# ---------------------------------------------------------------------------------------------- fixtures (host and GPU tests)
def strip(n, order="asc", seed=0):
    """n triangles (i, i+1, i+2) over n + 2 vertices, renumbered: ascending, descending, or by a seeded permutation."""
    nv = n + 2
    i = np.arange(n, dtype=np.int64)
    f = np.stack([i, i + 1, i + 2], 1)
    p = {"asc": np.arange(nv), "desc": np.arange(nv)[::-1], "perm": np.random.default_rng(seed).permutation(nv)}[order]
    return p[f].astype(np.int32), nv


def shuffled(parts, seed, extra_vertices=0):
    """Disjoint pieces [(faces, nv), ...] -> one mesh with the faces and the vertex numbers shuffled by a seeded permutation."""
    rng = np.random.default_rng(seed)
    faces, base = [], 0
    for f, nv in parts:
        faces.append(np.asarray(f, np.int64) + base)
        base += nv
    nv = base + extra_vertices
    f = np.concatenate(faces)
    f = rng.permutation(nv)[f]
    return f[rng.permutation(len(f))].astype(np.int32), nv


def comb(seed=5):
    """300 strips of 1..300 triangles: all face counts distinct."""
    return shuffled([strip(n) for n in range(1, 301)], seed)


def dust(seed=6):
    """20 000 isolated triangles and one strip of 5 000: Nv = 65 002, 20 001 components."""
    return shuffled([(np.arange(60000).reshape(-1, 3), 60000), strip(5000)], seed)


def degenerate():
    """A strip of 6 with faces [a, a, b] and [a, a, a] inside it, a lone triangle, a lone degenerate face on its own vertex pair,
    and three vertices no face names (11, 14, 15)."""
    f = [[0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5], [4, 5, 6], [5, 6, 7], [3, 3, 6], [2, 2, 2], [8, 9, 10], [12, 12, 13]]
    return np.array(f, np.int32), 16


BLOBS = (   # (centre, radius) in voxels of a 64^3 lattice, gaps of many cells between them
    ((24.0, 24.0, 24.0), 14.3),                                                          # the large sphere
    ((50.0, 12.0, 12.0), 5.2), ((50.0, 30.0, 12.0), 4.1), ((50.0, 46.0, 12.0), 3.3),     # three smaller, different radii
    ((12.0, 52.0, 50.0), 4.6), ((30.0, 52.0, 50.0), 4.6),                                # two of equal radius
    ((52.0, 52.0, 62.0), 6.4),                                                           # crosses the border: an open component
)


def blob_volume(blobs=BLOBS, n=64):
    """max_i (r_i - |p - c_i|) in float32, every term rounded on its own (so a term is the same bits in any union)."""
    g = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    vol = None
    for (c0, c1, c2), r in blobs:
        d = np.sqrt((z - np.float32(c0)) ** 2 + (y - np.float32(c1)) ** 2 + (x - np.float32(c2)) ** 2, dtype=np.float32)
        t = (np.float32(r) - d).astype(np.float32)
        vol = t if vol is None else np.maximum(vol, t)
    return np.ascontiguousarray(vol, np.float32)
