"""The device remesher's kernels (csrc/remesh_device.hip, sculpt_rmd_* in include/sculpt_hip.h) stage by stage against the fp64
restatement of the host's rules in tests/_rmdref.py, through the C ABI and the `_Topo` / `_Grid` helpers of
sf3d/remesh_device.py, on regular and adversarial meshes.  Every output buffer is pre-filled with a sentinel that must survive
past the documented written range.  The last tests wrap the driver's steps (split sweep, collapse round, flip round,
relaxation) and check the mesh after every one of them."""
import ctypes

import numpy as np
import pytest
import torch

import _rmdref as R
from sculptmate_amd._lib import lib
from sculptmate_amd.sf3d import remesh_device as rd
from test_gpu_remesh_device import _isosurface
from test_remesh import edge_lengths, icosphere, open_sheet, torus

pytestmark = pytest.mark.gpu

G = 64  # guard elements past every written range
S32 = np.int32(-0x5A5A5A5B)  # 0xA5A5A5A5
S64 = np.int64(-0x5A5A5A5A5A5A5A5B)
S8 = 0xA5


# ---------------------------------------------------------------------------------------------------------------- meshes
def uv_sphere(ns=96, nr=6):
    """Both poles have valence ns."""
    v = [[0.0, 0.0, 1.0]]
    for i in range(1, nr):
        th = np.pi * i / nr
        v += [[np.sin(th) * np.cos(2 * np.pi * j / ns), np.sin(th) * np.sin(2 * np.pi * j / ns), np.cos(th)] for j in range(ns)]
    v.append([0.0, 0.0, -1.0])
    s = len(v) - 1
    ring = lambda i, j: 1 + (i - 1) * ns + j % ns  # noqa: E731
    f = [[0, ring(1, j), ring(1, j + 1)] for j in range(ns)]
    for i in range(1, nr - 1):
        for j in range(ns):
            a, b, c, d = ring(i, j), ring(i + 1, j), ring(i + 1, j + 1), ring(i, j + 1)
            f += [[a, b, c], [a, c, d]]
    f += [[s, ring(nr - 1, j + 1), ring(nr - 1, j)] for j in range(ns)]
    return np.array(v), np.array(f, np.int32)


def three_sheets():
    """Three strips that share the edge (0, 1)."""
    v = [[0, 0, 0], [1, 0, 0]]
    f = []
    for s, d in enumerate([(0, 1, 0), (0, -0.5, 0.8), (0, -0.5, -0.8)]):
        a, b = len(v), len(v) + 1
        v += [list(np.add([0, 0, 0], d)), list(np.add([1, 0, 0], d))]
        f += [[0, 1, b], [0, b, a]] if s != 1 else [[1, 0, a], [1, a, b]]
    return np.array(v, np.float64), np.array(f, np.int32)


def bowtie():
    """Two fans that meet in vertex 0 only."""
    v = [[0, 0, 0]] + [[np.cos(t), np.sin(t), 0.2] for t in np.linspace(0, 1.5, 4)] + [[np.cos(t), 0.2, np.sin(t)] for t in np.linspace(3, 4.5, 4)]
    f = [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 5, 6], [0, 6, 7], [0, 7, 8]]
    return np.array(v, np.float64), np.array(f, np.int32)


def reversed_patch():
    v, f = open_sheet(8, jitter=0.3, seed=3)
    f = f.copy()
    f[40] = f[40][::-1]
    return v, f


def duplicated_face():
    v, f = icosphere(1)
    return v, np.concatenate([f, f[:1]]).astype(np.int32)


def coincident():
    """Vertex 20 on top of vertex 21 (zero-area faces), vertex 30 on the segment 29 - 31."""
    v, f = open_sheet(8, jitter=0.2, seed=4)
    v = v.copy()
    v[20] = v[21]
    v[30] = 0.5 * (v[29] + v[31])
    return v, f


def unreferenced():
    v, f = icosphere(2)
    v = np.concatenate([v[:10], [[5, 5, 5], [6, 6, 6], [7, 7, 7]], v[10:], [[9, 9, 9]]])
    return v, np.where(f >= 10, f + 3, f).astype(np.int32)


def triangle_and_tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [3, 0, 0], [4, 0, 0], [3, 1, 0]], np.float64)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3], [4, 5, 6]], np.int32)
    return v, f


def flip_onto_an_edge():
    """A flat Delaunay patch plus one face (8, 10, 14) below it: the flip of (7, 12) would create the edge (8, 10), which that
    face already has; every other guard lets it through."""
    v = [[0.7739560604095459, 0.43887844681739807, 0.0], [0.8585979342460632, 0.6973680257797241, 0.0], [0.09417735040187836, 0.9756223559379578, 0.0],
         [0.7611396908760071, 0.7860643267631531, 0.0], [0.12811362743377686, 0.4503859281539917, 0.0], [0.3707980215549469, 0.926764965057373, 0.0],
         [0.6438651084899902, 0.822761595249176, 0.0], [0.44341421127319336, 0.2272387146949768, 0.0], [0.554584801197052, 0.06381725519895554, 0.0],
         [0.8276311755180359, 0.6316643953323364, 0.0], [0.7580877542495728, 0.35452595353126526, 0.0], [0.9706979990005493, 0.8931211233139038, 0.0],
         [0.7783834934234619, 0.1946387141942978, 0.0], [0.4667209982872009, 0.04380376636981964, 0.0], [0.6563363075256348, 0.2091716080904007, -1.0]]
    f = [[5, 11, 2], [5, 6, 11], [5, 4, 6], [4, 5, 2], [6, 3, 11], [9, 3, 6], [0, 9, 6], [12, 0, 10], [0, 12, 9], [3, 1, 11], [1, 3, 9],
         [1, 12, 11], [12, 1, 9], [0, 7, 10], [7, 4, 13], [4, 7, 6], [7, 0, 6], [8, 7, 13], [7, 12, 10], [7, 8, 12], [8, 10, 14]]
    return np.array(v, np.float64), np.array(f, np.int32)


def empty():
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64), np.zeros((0, 3), np.int32)


REGULAR = {
    "ico2": lambda: icosphere(2), "ico3": lambda: icosphere(3), "ico4": lambda: icosphere(4), "torus": lambda: torus(24, 12),
    "sheet": lambda: open_sheet(12, jitter=0.4), "iso0": lambda: _isosurface(0, 16), "iso1": lambda: _isosurface(1, 16),
    "iso2": lambda: _isosurface(2, 16),
}
ADVERSARIAL = {
    "pole96": uv_sphere, "three_sheets": three_sheets, "bowtie": bowtie, "reversed": reversed_patch, "duplicated": duplicated_face,
    "coincident": coincident, "unreferenced": unreferenced, "tri_tet": triangle_and_tetrahedron,
    "flip_onto_edge": flip_onto_an_edge, "empty": empty,
}
ALL = dict(REGULAR, **ADVERSARIAL)
_cache = {}


def mesh(name):
    if name not in _cache:
        v, f = ALL[name]()
        _cache[name] = (np.asarray(v, np.float32), np.asarray(f, np.int32).reshape(-1, 3))
    return _cache[name]


# --------------------------------------------------------------------------------------------------------------- helpers
def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def filled(n, dtype, value, cols=None):
    shape = (n + G,) if cols is None else (n + G, cols)
    return torch.full(shape, int(value) if dtype != torch.float32 else float("nan"), dtype=dtype, device="cuda")


def f32_sentinel(n, cols=3):
    t = torch.empty((n + G, cols), dtype=torch.float32, device="cuda")
    t.view(torch.int32).fill_(int(S32))
    return t


def h(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def guard_ok(t, n, value):
    a = h(t).reshape(t.shape[0], -1)[n:]
    return (a.view(np.int32) == np.int32(value)).all() if a.dtype == np.float32 else (a == value).all()


def as_u64(a):
    return np.asarray(a).astype(np.int64).view(np.uint64)


def dev(v, f):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda()


def topo_of(P, F):
    return rd._Topo(rd._Ctx(), F, P.shape[0])


def ulps(a, b):
    """Distance in fp32 ulps, element-wise."""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def mean_edge(v, f):
    return float(edge_lengths(np.asarray(v, np.float64), f).mean()) if len(f) else 1.0


# -------------------------------------------------------------------------------------------------------- 1. topology
@pytest.mark.parametrize("name", list(ALL))
def test_topology_kernels_match_np_unique(cuda, name):
    v, f = mesh(name)
    P, F = dev(v, f)
    nf, nv = len(f), len(v)
    nh = 3 * nf
    ref = R.topo(f, nv)
    keys = filled(nh, torch.int64, S64)
    assert lib.sculpt_rmd_halfedge_keys(_p(F), nf, _p(keys), _s()) == 0
    assert np.array_equal(h(keys)[:nh], ref["keys"]) and guard_ok(keys, nh, S64)
    skeys, sperm = torch.sort(keys[:nh], stable=True)
    head = filled(nh, torch.int32, S32)
    assert lib.sculpt_rmd_edge_heads(_p(skeys), nh, _p(head), _s()) == 0
    want_head = np.ones(nh, np.int32)
    want_head[1:] = ref["skeys"][1:] != ref["skeys"][:-1]
    assert np.array_equal(h(head)[:nh], want_head) and guard_ok(head, nh, S32)
    eid = torch.cumsum(head[:nh], 0, dtype=torch.int32)
    she, fe, es = filled(nh, torch.int32, S32), filled(nh, torch.int32, S32), filled(nh + 1, torch.int32, S32)
    assert lib.sculpt_rmd_edge_fill(_p(sperm), _p(eid), nh, _p(she), _p(fe), _p(es), _s()) == 0
    ne = ref["ne"]
    assert np.array_equal(h(she)[:nh], ref["she"]) and guard_ok(she, nh, S32)
    assert np.array_equal(h(fe)[:nh], ref["fe"]) and guard_ok(fe, nh, S32)
    if nh:
        assert np.array_equal(h(es)[:ne + 1], ref["es"]) and guard_ok(es, ne + 1, S32)
    # the whole _Topo
    T = topo_of(P, F)
    assert T.ne == ne
    assert np.array_equal(h(T.skeys), ref["skeys"]) and np.array_equal(h(T.she), ref["she"]) and np.array_equal(h(T.fe), ref["fe"])
    assert np.array_equal(h(T.es)[:ne + 1], ref["es"]), "es[ne] must be 3 nf"
    assert np.array_equal(h(T.vfs), ref["vfs"]) and np.array_equal(h(T.vfc), ref["vfc"])
    assert np.array_equal(h(T.bnd)[:nv], ref["bnd"][:nv]), np.nonzero(h(T.bnd)[:nv] != ref["bnd"][:nv])
    # the two flag passes alone, into zeroed ranges with a guard
    hv = torch.full((nv + G,), S8, dtype=torch.uint8, device=cuda)
    hv[:nv] = 0
    assert lib.sculpt_rmd_high_valence(T.ref(), _p(hv), _s()) == 0
    assert np.array_equal(h(hv)[:nv], ref["high_valence"][:nv]) and (h(hv)[nv:] == S8).all()
    bnd = torch.full((nv + G,), S8, dtype=torch.uint8, device=cuda)
    bnd[:nv] = 0
    assert lib.sculpt_rmd_boundary(T.ref(), _p(bnd), _s()) == 0
    assert np.array_equal(h(bnd)[:nv], ref["edge_bnd"][:nv]) and (h(bnd)[nv:] == S8).all()


@pytest.mark.parametrize("ns", [63, 64, 65, 96])
def test_high_valence_threshold(cuda, ns):
    """The poles of a closed UV sphere with ns segments have ns neighbours: a feature from 65 on, on both paths."""
    v, f = uv_sphere(ns)
    v = v.astype(np.float32)
    want = ns > 64
    bnd = h(topo_of(*dev(v, f)).bnd)
    assert bnd[0] == want and bnd[len(v) - 1] == want and bnd[1:-1].sum() == 0
    assert (R.topo(f, len(v))["bnd"][[0, len(v) - 1]] == want).all()
    assert (R.Mesh(v, f).bnd[[0, len(v) - 1]] == want).all() and not R.Mesh(v, f).bnd[1:-1].any()


def test_features_are_carried_through_passes(cuda):
    """A flag carried from the previous pass stays, whatever the valence is now (Mesh::build scans once); vertices past the
    carried range start unflagged; the edge boundary is recomputed on top."""
    v, f = uv_sphere(64)
    P, F = dev(v.astype(np.float32), f)
    nv = len(v)
    carry = torch.zeros(nv - 5, dtype=torch.uint8, device=cuda)
    carry[0] = 1
    carry[7] = 1
    bnd = h(rd._Topo(rd._Ctx(), F, nv, carry=carry).bnd)
    assert list(np.nonzero(bnd)[0]) == [0, 7]
    vs, fs = mesh("sheet")
    Ps, Fs = dev(vs, fs)
    carry = torch.ones(len(vs) + 10, dtype=torch.uint8, device=cuda)
    carry[:len(vs) // 2] = 0
    bnd = h(rd._Topo(rd._Ctx(), Fs, len(vs), carry=carry).bnd)
    want = R.topo(fs, len(vs))["edge_bnd"][:len(vs)].copy()
    want[len(vs) // 2:] = 1
    assert np.array_equal(bnd[:len(vs)], want)


# ------------------------------------------------------------------------------------------------ 2. and 4. collapses
def collapse_case(name, mode):
    v, f = mesh(name)
    he = mean_edge(v, f)
    return v, f, (1.1 * he, 1.6 * he) if mode == 1 else (0.0, 0.0)


def device_collapse_propose(T, P, mode, low, high):
    nv, ne = T.nv, T.ne
    claim = torch.full((max(nv, 1) + G,), -1, dtype=torch.int64, device="cuda")
    cand = filled(ne, torch.int64, S64)
    assert lib.sculpt_rmd_collapse_propose(T.ref(), _p(P), mode, low, high, _p(claim), _p(cand), _s()) == 0
    win = filled(ne, torch.int32, S32)
    assert lib.sculpt_rmd_collapse_select(T.ref(), _p(P), mode, _p(claim), _p(cand), _p(win), _s()) == 0
    return claim, cand, win


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(ALL))
def test_collapse_proposals_are_the_host_rule(cuda, name, mode):
    v, f, (low, high) = collapse_case(name, mode)
    P, F = dev(v, f)
    T = topo_of(P, F)
    claim, cand, win = device_collapse_propose(T, P, mode, low, high)
    ref_T, M, rcand, fp, nef, amb = R.collapse_proposals(v, f, mode, low, high)
    if name in REGULAR:
        assert not any(amb), "a regular mesh has a candidate within the sign-test margin"
    dcand = [int(x) for x in as_u64(h(cand)[:T.ne])]
    assert guard_ok(cand, T.ne, S64)
    bad = [e for e in range(T.ne) if dcand[e] != rcand[e] and not (amb[e] and dcand[e] in (R.NO_CLAIM, (rcand[e] if rcand[e] != R.NO_CLAIM else R.collapse_key(M, *R.edge_ends(ref_T, e), e))))]
    assert not bad, ("cand differs from the host rule", name, mode, [(e, R.edge_ends(ref_T, e), hex(dcand[e]), hex(rcand[e])) for e in bad[:8]])
    cl = R.claims(T.nv, dcand, fp)  # (the device's own verdict on ambiguous edges)
    dclaim = [int(x) for x in as_u64(h(claim))]
    assert dclaim[:T.nv] == cl[:T.nv], "claim[] is not the minimum key over the footprints"
    assert all(x == R.NO_CLAIM for x in dclaim[max(T.nv, 1):])
    assert list(h(win)[:T.ne]) == R.winners(cl, dcand, fp, nef) and guard_ok(win, T.ne, S32)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", [n for n in ALL if n != "empty"])
def test_collapse_round_is_sequential_application(cuda, name, mode):
    """The winners of a round, applied one after the other with the host's collapse() -- each still valid under the host rule
    when its turn comes -- in ascending and in descending edge order, give the device's faces (after compaction) and moved
    positions bit for bit."""
    v, f, (low, high) = collapse_case(name, mode)
    P, F = dev(v, f)
    T = topo_of(P, F)
    claim, cand, win = device_collapse_propose(T, P, mode, low, high)
    w = h(win)[:T.ne]
    dcand = [int(x) for x in as_u64(h(cand)[:T.ne])]
    ref_T = R.topo(f, len(v))
    alive = torch.ones(max(T.nf, 1), dtype=torch.uint8, device=cuda)
    assert lib.sculpt_rmd_collapse_apply(T.ref(), _p(P), _p(F), mode, _p(win), _p(alive), _s()) == 0
    Fo = rd._compact_faces(rd._Ctx(), F, alive[:T.nf], int(h(alive)[:T.nf].sum()))
    dF, dP = h(Fo), h(P)
    assert T.nf - len(dF) == int(w.sum())
    for order in (1, -1):
        M = R.Mesh(v, f, bnd=ref_T["bnd"][:len(v)].astype(bool))
        for e in np.nonzero(w)[0][::order]:
            a, b = R.edge_ends(ref_T, e)
            ok, u, vv, p, am = R.collapse_rule(M, a, b, mode, low, high)
            assert ok or am, ("a winner is no longer valid after other winners", name, e)
            assert R.collapse_key(M, u, vv, int(e)) == dcand[e]
            M.collapse(u, vv, p)
        assert np.array_equal(M.faces(), dF), (name, mode, order)
        assert np.array_equal(M.P.view(np.int32), dP.view(np.int32)), (name, mode, order)


# ---------------------------------------------------------------------------------------------------- 3. and 4. flips
@pytest.mark.parametrize("name", [n for n in ALL])
def test_flip_proposals_and_round(cuda, name):
    v, f = mesh(name)
    P, F = dev(v, f)
    T = topo_of(P, F)
    nv, ne = T.nv, T.ne
    claim = torch.full((max(nv, 1) + G,), -1, dtype=torch.int64, device=cuda)
    cand = filled(ne, torch.int64, S64)
    assert lib.sculpt_rmd_flip_propose(T.ref(), _p(P), _p(claim), _p(cand), _s()) == 0
    ref_T, M, rcand, fp, amb = R.flip_proposals(v, f)
    if name in REGULAR:
        assert not any(amb), "a regular mesh has a flip within the sign-test margin"
    dcand = [int(x) for x in as_u64(h(cand)[:ne])]
    assert guard_ok(cand, ne, S64)
    bad = [e for e in range(ne) if dcand[e] != rcand[e] and not amb[e]]
    assert not bad, ("flip cand differs from equalize_valences", name, [(e, R.edge_ends(ref_T, e), hex(dcand[e]), hex(rcand[e])) for e in bad[:8]])
    for e in range(ne):  # an ambiguous edge: no claim, or the key of the host rule's verdict without the guard
        if amb[e] and dcand[e] != rcand[e]:
            assert dcand[e] == R.NO_CLAIM or dcand[e] & 0xFFFFFFFF == e
    fp = [s if dcand[e] != R.NO_CLAIM else set() for e, s in enumerate(fp)]
    for e in range(ne):
        if amb[e] and dcand[e] != R.NO_CLAIM and not fp[e]:
            u, vv = R.edge_ends(ref_T, e)
            ef = M.edge_faces(u, vv)
            fp[e] = {u, vv} | {M.third(x, u, vv) for x in ef}
    cl = R.claims(nv, dcand, fp)
    dclaim = [int(x) for x in as_u64(h(claim))]
    assert dclaim[:nv] == cl[:nv] and all(x == R.NO_CLAIM for x in dclaim[max(nv, 1):])
    win = filled(ne, torch.int32, S32)
    assert lib.sculpt_rmd_flip_apply(T.ref(), _p(P), _p(claim), _p(cand), _p(F), _p(win), _s()) == 0
    w = h(win)[:ne]
    assert list(w) == R.winners(cl, dcand, fp, [1] * ne) and guard_ok(win, ne, S32)
    dF = h(F)
    for order in (1, -1):
        Mq = R.Mesh(v, f, bnd=ref_T["bnd"][:len(v)].astype(bool))
        for e in np.nonzero(w)[0][::order]:
            u, vv = R.edge_ends(ref_T, e)
            gain, quad, am = R.flip_rule(Mq, u, vv)
            assert gain is not None or am, ("a winning flip is no longer valid after other winners", name, e)
            assert Mq.flip(u, vv)
        assert np.array_equal(np.array(Mq.F, np.int64).reshape(-1, 3), dF), (name, order)


# --------------------------------------------------------------------------------------------------------------- 5. split
def split_case(name):
    v, f = mesh(name)
    return v, f, 0.9 * mean_edge(v, f)


def device_split(T, P, nv, high, vcap_less=0, fcap_less=0):
    ne, nf = T.ne, T.nf
    mark = filled(ne, torch.int32, S32)
    assert lib.sculpt_rmd_split_mark(T.ref(), _p(P), high, _p(mark), _s()) == 0
    mark_incl = torch.cumsum(mark[:ne], 0, dtype=torch.int32)
    cnt = filled(nf, torch.int32, S32)
    assert lib.sculpt_rmd_split_count(T.ref(), _p(mark), _p(cnt), _s()) == 0
    off_incl = torch.cumsum(cnt[:nf], 0, dtype=torch.int32)
    nsplit = int(h(mark_incl)[-1]) if ne else 0
    total = int(h(off_incl)[-1]) if nf else 0
    vcap, fcap = nv + nsplit - vcap_less, total - fcap_less
    Pb = f32_sentinel(nv + nsplit)
    Pb[:nv] = P
    Fo = filled(total, torch.int32, S32, cols=3)
    assert lib.sculpt_rmd_split_emit(T.ref(), _p(Pb), vcap, _p(mark), _p(mark_incl), _p(off_incl), fcap, _p(Fo), _s()) == 0
    return mark, cnt, h(off_incl), Pb, Fo, vcap, fcap


def _area_normal(V, F):
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    return np.cross(b - a, c - a)


@pytest.mark.parametrize("name", list(ALL))
def test_split_matches_the_templates(cuda, name):
    v, f, high = split_case(name)
    P, F = dev(v, f)
    nv = len(v)
    T = topo_of(P, F)
    mark, cnt, off, Pb, Fo, vcap, fcap = device_split(T, P, nv, high)
    ref_T, rmark, rcnt, rows, rFo, amb_f, amb_e = R.split_reference(v, f, high)
    if name in REGULAR:
        assert not amb_e.any()
    m = h(mark)[:T.ne]
    assert np.array_equal(m[~amb_e], rmark[~amb_e]) and guard_ok(mark, T.ne, S32)
    if amb_e.any() and not np.array_equal(m, rmark):
        pytest.skip("an edge length within rounding of `high` was marked otherwise; the marks above agree")  # not on REGULAR
    assert np.array_equal(h(cnt)[:T.nf], rcnt) and guard_ok(cnt, T.nf, S32)
    ns = len(rows)
    dP = h(Pb)
    assert np.array_equal(dP[:nv].view(np.int32), v.view(np.int32))
    assert np.array_equal(dP[nv:nv + ns].view(np.int32), rows.view(np.int32)), "new vertices are not the fp32 midpoints"
    assert guard_ok(Pb, nv + ns, S32)
    dF = h(Fo)
    n_out = len(rFo)
    assert guard_ok(Fo, n_out, S32)
    same = (dF[:n_out] == rFo).all(1)
    assert same[~amb_f].all(), ("children differ from the templates", name, np.nonzero(~same & ~amb_f)[0][:8])
    if name in ("sheet", "torus"):
        assert (rcnt == 3).sum() > 10, "the case must exercise the diagonal choice"
    out = dF[:n_out]
    Vn = np.concatenate([v, rows]).astype(np.float64)
    # conforming: with a manifold input, the output is manifold with the same Euler characteristic and boundary loops
    if name in REGULAR or name in ("pole96", "unreferenced", "tri_tet"):
        assert R.max_edge_faces(out) <= 2
        d = np.concatenate([out[:, [0, 1]], out[:, [1, 2]], out[:, [2, 0]]]).astype(np.int64)
        assert len(np.unique(d[:, 0] * (len(Vn) + 1) + d[:, 1])) == len(d)
        assert R.euler(len(np.unique(out)), out) == R.euler(len(np.unique(f)), f)
        assert R.boundary_loops(out) == R.boundary_loops(f)
    # orientation kept and area kept, per parent face
    parent = np.repeat(np.arange(len(f)), rcnt)
    n_par = _area_normal(v.astype(np.float64), f.astype(np.int64))
    n_out_ = _area_normal(Vn, out.astype(np.int64))
    a_par = np.linalg.norm(n_par, axis=1)
    a_sum = np.bincount(parent, np.linalg.norm(n_out_, axis=1), minlength=len(f))
    nz = a_par > 1e-6 * (np.abs(v).max() + 1) ** 2
    assert ((n_out_ * n_par[parent]).sum(1)[nz[parent]] > 0).all(), "a child turned over"
    assert np.allclose(a_sum[nz], a_par[nz], rtol=1e-5, atol=1e-6 * a_par.max(initial=0.0))  # fp32 midpoints
    assert abs(a_sum.sum() - a_par.sum()) <= 1e-5 * a_par.sum() + 1e-12


@pytest.mark.parametrize("name", ["ico3", "sheet", "iso1", "pole96"])
def test_split_writes_nothing_at_or_past_the_capacity(cuda, name):
    v, f, high = split_case(name)
    P, F = dev(v, f)
    nv = len(v)
    T = topo_of(P, F)
    _, rmark, rcnt, rows, rFo, amb_f, _ = R.split_reference(v, f, high)
    ns, total = len(rows), len(rFo)
    assert ns > 8 and total > len(f)
    mark, cnt, off, Pb, Fo, vcap, fcap = device_split(T, P, nv, high, vcap_less=ns // 2, fcap_less=total // 3)
    dP, dF = h(Pb), h(Fo)
    assert np.array_equal(dP[nv:vcap].view(np.int32), rows[:vcap - nv].view(np.int32))
    assert (dP[vcap:].view(np.int32) == S32).all(), "a vertex row written at or past vcap"
    assert (dF[fcap:] == S32).all(), "a face written at or past fcap"
    first = off - rcnt
    for fi in range(len(f)):
        blk = slice(first[fi], off[fi])
        if off[fi] <= fcap:
            assert (dF[blk] == rFo[blk]).all() or amb_f[blk].any()
        else:
            assert (dF[blk] == S32).all(), "a face block that does not fit whole was written in part"


# ---------------------------------------------------------------------------------------------- 6. grid and projection
def surfaces():
    s = {}
    vs, fs = icosphere(2)
    s["small_offset"] = (icosphere(3), (0.5 * vs + [0.6, 0.0, 0.0], fs))  # much of the relaxed sphere lies outside the grid
    vp, fp = open_sheet(9)
    vp = vp.copy()
    vp[:, 2] = 0.0
    vr, fr = open_sheet(12, jitter=0.5, seed=5)
    s["planar"] = ((vr, fr), (vp, fp))  # one grid layer
    s["one_face"] = (icosphere(2), (np.array([[0, 0, 0], [1.5, 0, 0.2], [0, 1.5, -0.2]]), np.array([[0, 1, 2]], np.int32)))
    n = 100
    xs = np.linspace(0, 10, n + 1)
    vstrip = np.concatenate([np.stack([xs, np.zeros_like(xs), 0.05 * np.sin(xs)], 1), np.stack([xs, 0.1 + 0 * xs, 0.05 * np.sin(xs)], 1)])
    fstrip = np.array([[i, i + 1, n + 2 + i] for i in range(n)] + [[i, n + 2 + i, n + 1 + i] for i in range(n)], np.int32)
    vr, fr = open_sheet(10, jitter=0.5, seed=6)
    vr = vr * [10.0, 0.3, 1.0] + [0, -0.1, 0.1]
    s["long_strip"] = ((vr, fr), (vstrip, fstrip))
    for name in ("ico3", "torus", "iso0", "pole96", "reversed", "coincident", "bowtie", "tri_tet"):
        vv, ff = mesh(name)
        rng = np.random.default_rng(len(name))
        s["self_" + name] = ((vv + rng.normal(0, 0.15 * mean_edge(vv, ff), vv.shape), ff), (vv, ff))
    return s


SURFACES = surfaces()


@pytest.mark.parametrize("case", list(SURFACES))
def test_grid_csr_is_the_host_grid(cuda, case):
    _, (gv, gf) = SURFACES[case]
    GP, GF = dev(gv, gf)
    g = rd._Grid(rd._Ctx(), GP, GF)
    lo, cell, n = R.grid_params(np.asarray(gv, np.float32), gf)
    assert list(g.params) == [lo[0], lo[1], lo[2], cell, n[0], n[1], n[2]]
    rcnt, pairs, items, start = R.grid_cells(np.asarray(gv, np.float32), gf, lo, cell, n)
    cnt = filled(len(gf), torch.int32, S32)
    assert lib.sculpt_rmd_grid_count(_p(GP), _p(GF), len(gf), g.params, _p(cnt), _s()) == 0
    assert np.array_equal(h(cnt)[:len(gf)], rcnt) and guard_ok(cnt, len(gf), S32)
    off = torch.cumsum(cnt[:len(gf)], 0, dtype=torch.int32)
    cellid, face = filled(len(pairs), torch.int32, S32), filled(len(pairs), torch.int32, S32)
    assert lib.sculpt_rmd_grid_fill(_p(GP), _p(GF), len(gf), g.params, _p(off), _p(cellid), _p(face), _s()) == 0
    assert np.array_equal(h(cellid)[:len(pairs)], pairs[:, 0]) and np.array_equal(h(face)[:len(pairs)], pairs[:, 1])
    assert guard_ok(cellid, len(pairs), S32) and guard_ok(face, len(pairs), S32)
    assert np.array_equal(h(g.items), items) and np.array_equal(h(g.start), start)
    if case == "planar":
        assert n[2] == 1


def device_relax(v, f, gv=None, gf=None):
    P, F = dev(v, f)
    T = topo_of(P, F)
    nv = len(v)
    Q = f32_sentinel(nv)
    undo = torch.full((rd._lib.rmd_undo_bytes(nv) + G,), S8, dtype=torch.uint8, device="cuda")
    if gf is None:
        assert lib.sculpt_rmd_relax(T.ref(), _p(P), None, None, 0, None, None, None, 0, _p(Q), _p(undo), _s()) == 0
    else:
        GP, GF = dev(gv, gf)
        g = rd._Grid(rd._Ctx(), GP, GF)
        assert lib.sculpt_rmd_relax(T.ref(), _p(P), _p(GP), _p(GF), len(gf), _p(g.items), _p(g.start), g.params, 1, _p(Q), _p(undo), _s()) == 0
    q = h(Q)
    assert guard_ok(Q, nv, S32) and (h(undo)[rd._lib.rmd_undo_bytes(nv):] == S8).all()
    return q[:nv]


def check_relax(v, f, q, gv=None, gf=None, regular=False):
    v = np.asarray(v, np.float32)
    if len(f):  # the promise: no face with nonzero area is turned over after the undo pass
        fb, fa = _area_normal(v.astype(np.float64), f.astype(np.int64)), _area_normal(q.astype(np.float64), f.astype(np.int64))
        bad = np.nonzero((np.abs(fb).sum(1) > 0) & ((fb * fa).sum(1) <= 0))[0]
        assert not len(bad), ("a face turned over after the relaxation", bad[:8])
    Qr, relaxed, pre, moved, undo, amb = R.relax(v, f, None if gf is None else np.asarray(gv, np.float32), gf)
    if regular:
        assert not amb.any()
    off = (ulps(q, Qr) > 1).any(1) & ~amb
    scale = float(np.abs(v).max()) + 1.0
    for u in np.nonzero(off)[0]:
        # equally close points of two triangles: the device's point is on the surface, as close as the reference's
        assert gf is not None and moved[u] and not undo[u], ("relaxed position differs", u, q[u], Qr[u], v[u])
        dq = R.closest_point(q[u].astype(np.float64), np.asarray(gv, np.float32), gf)[1]
        assert np.sqrt(dq) <= 1e-6 * scale, ("not on the surface", u)
        d_dev, d_ref = np.linalg.norm(q[u] - pre[u]), np.linalg.norm(Qr[u].astype(np.float64) - pre[u])
        assert abs(d_dev - d_ref) <= 1e-6 * scale, ("not a closest point", u, d_dev, d_ref)
    for u in np.nonzero(amb)[0]:
        assert (ulps(q[u], Qr[u]) <= 1).all() or np.array_equal(q[u], v[u]) or gf is not None


@pytest.mark.parametrize("name", list(ALL))
def test_relax_without_projection(cuda, name):
    v, f = mesh(name)
    if name != "empty":
        rng = np.random.default_rng(1)
        v = (v + rng.normal(0, 0.1 * mean_edge(v, f), v.shape)).astype(np.float32)
    check_relax(v, f, device_relax(v, f), regular=name in REGULAR)


@pytest.mark.parametrize("case", list(SURFACES))
def test_relax_with_projection(cuda, case):
    (v, f), (gv, gf) = SURFACES[case]
    v = np.asarray(v, np.float32)
    check_relax(v, f, device_relax(v, f, gv, gf), gv, gf, regular=case in ("small_offset", "planar", "one_face", "long_strip"))


def test_relax_centroid_is_over_distinct_neighbours(cuda):
    """One reversed face in a patch: the 'next corner' of every face around its vertices is not the set of their neighbours."""
    v, f = mesh("reversed")
    q = device_relax(v, f)
    Qr = R.relax(v, f)[0]
    touched = np.unique(f[40])
    assert (ulps(q[touched], Qr[touched]) <= 1).all(), (q[touched], Qr[touched])


# --------------------------------------------------------------------------------------------- 7. compaction and checks
@pytest.mark.parametrize("name", ["ico3", "unreferenced", "tri_tet", "empty"])
def test_compaction_kernels(cuda, name):
    v, f = mesh(name)
    P, F = dev(v, f)
    nf, nv = len(f), len(v)
    rng = np.random.default_rng(2)
    alive = (rng.uniform(size=max(nf, 1)) < 0.7).astype(np.uint8)
    incl = np.cumsum(alive[:nf]).astype(np.int32)
    kept = int(alive[:nf].sum())
    Fo = filled(kept, torch.int32, S32, cols=3)
    ta, ti = torch.from_numpy(alive).cuda(), torch.from_numpy(incl).cuda()
    assert lib.sculpt_rmd_compact_faces(_p(F), _p(ta), _p(ti), nf, _p(Fo), _s()) == 0
    assert np.array_equal(h(Fo)[:kept], f[alive[:nf] == 1]) and guard_ok(Fo, kept, S32)
    used = torch.zeros(nv + G, dtype=torch.int32, device=cuda)
    used[nv:] = int(S32)
    assert lib.sculpt_rmd_mark_used(_p(F), nf, _p(used), _s()) == 0
    ru = np.zeros(nv, np.int32)
    ru[np.unique(f)] = 1
    assert np.array_equal(h(used)[:nv], ru) and guard_ok(used, nv, S32)
    uincl = torch.cumsum(used[:nv], 0, dtype=torch.int32)
    n = int(ru.sum())
    Po = f32_sentinel(n)
    F2 = F.clone()
    assert lib.sculpt_rmd_compact_vertices(_p(P), _p(used), _p(uincl), nv, _p(Po), _p(F2), nf, _s()) == 0
    assert np.array_equal(h(Po)[:n].view(np.int32), v[ru == 1].view(np.int32)) and guard_ok(Po, n, S32)
    assert np.array_equal(h(F2), (np.cumsum(ru) - 1)[f])
    T = topo_of(P, F)
    first = filled(3 * nf, torch.int32, S32)
    assert lib.sculpt_rmd_first_halfedge(T.ref(), _p(first), _s()) == 0
    ref = R.topo(f, nv)
    rf = np.zeros(3 * nf, np.int32)
    rf[ref["she"][ref["es"][:-1]]] = 1
    assert np.array_equal(h(first)[:3 * nf], rf) and guard_ok(first, 3 * nf, S32)
    lens = filled(nf, torch.float64, 0)
    lens.view(torch.int64).fill_(int(S64))
    assert lib.sculpt_rmd_halfedge_lengths(_p(P), _p(F), nf, _p(lens), _s()) == 0
    vd = v.astype(np.float64)
    rl = sum(np.linalg.norm(vd[f[:, k]] - vd[f[:, (k + 1) % 3]], axis=1) for k in range(3))
    dl = h(lens)
    assert np.allclose(dl[:nf], rl, rtol=4e-16 * 4, atol=0) and (dl[nf:].view(np.int64) == S64).all()


def test_validate_status_bits(cuda):
    v, f = mesh("ico2")
    nv = len(v)

    def status(vv, ff):
        P, F = dev(vv, ff)
        st = torch.full((1,), int(S32), dtype=torch.int32, device=cuda)
        assert lib.sculpt_rmd_validate(_p(P), len(vv), _p(F), len(ff), _p(st), _s()) == 0
        return int(h(st)[0])

    assert status(v, f) == 0
    neg, top, rep = f.copy(), f.copy(), f.copy()
    neg[5, 1] = -1
    top[7, 2] = nv
    rep[9] = [rep[9, 0], rep[9, 0], rep[9, 2]]
    nanv, infv = v.copy(), v.copy()
    nanv[3, 1] = np.nan
    infv[nv - 1, 2] = -np.inf
    assert status(v, neg) == 1 and status(v, top) == 1 and status(v, rep) == 2
    assert status(nanv, f) == 4 and status(infv, f) == 4
    both = neg.copy()
    both[9] = rep[9]
    assert status(v, both) == 3 and status(nanv, both) == 7 and status(infv, top) == 5
    # more faces than vertices and the other way round: every element is looked at
    assert status(v[:3], np.concatenate([f[:0], [[0, 1, 2]] * 50]).astype(np.int32)) == 0
    assert status(v[:3], np.array([[0, 1, 2]] * 49 + [[0, 1, 3]], np.int32)) == 1
    big = np.concatenate([v, np.zeros((1000, 3))]).astype(np.float32)
    big[-1, 0] = np.nan
    assert status(big, f[:2]) == 4


# ------------------------------------------------------------------------------------------------ 8. whole-call invariants
def _faces_ok(F, nv, ctx):
    assert F.size == 0 or (F.min() >= 0 and F.max() < nv), ctx
    assert ((F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])).all(), ctx


def _directed_unique(F):
    d = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]).astype(np.int64)
    return len(np.unique(d[:, 0] * (int(F.max(initial=0)) + 2) + d[:, 1])) == len(d)


class Watch:
    """Wraps the driver's steps (monkeypatch): the original runs, then the mesh is checked."""

    def __init__(self, monkeypatch, v, f, botsch):
        self.ctx = None
        self.steps = {"split": 0, "collapse": 0, "flip": 0, "relax": 0}
        self.flipped = []
        f64 = np.asarray(f, np.int64)
        self.directed = _directed_unique(f64) if len(f) else True
        self.manifold_edges = R.max_edge_faces(f64) <= 2
        self.topo = (R.euler(len(np.unique(f64)), f64), R.boundary_loops(f64)) if self.manifold_edges and self.directed else None
        self.keep = np.nonzero(R.Mesh(v, f).bnd & np.isin(np.arange(len(v)), f64))[0] if botsch else np.zeros(0, np.int64)
        self.keep_pos = np.asarray(v, np.float32)[self.keep].copy()
        for name, fn in (("_split_sweep", self.split), ("_collapse_round", self.collapse), ("_flip_round", self.flip), ("_relax", self.relax)):
            monkeypatch.setattr(rd, name, fn(getattr(rd, name)))

    def check(self, F, P, what):
        F, P = h(F).astype(np.int64).reshape(-1, 3), h(P).reshape(-1, 3)
        ctx = (what, self.steps)
        _faces_ok(F, len(P), ctx)
        if self.directed:
            assert _directed_unique(F), ("a directed half-edge appears twice",) + ctx
        if self.manifold_edges:
            assert R.max_edge_faces(F) <= 2, ("an edge with more than two faces",) + ctx
        if self.topo is not None:
            assert (R.euler(len(np.unique(F)), F), R.boundary_loops(F)) == self.topo, ctx
        if len(self.keep):
            assert np.isin(self.keep, F).all(), ("a boundary vertex was removed",) + ctx
            assert np.array_equal(P[self.keep].view(np.int32), self.keep_pos.view(np.int32)), ("a boundary vertex moved",) + ctx

    def split(self, orig):
        def wrap(ctx, T, V, high):
            Fn, n = orig(ctx, T, V, high)
            self.steps["split"] += 1
            self.check(Fn, V.P[:V.nv], "split")
            return Fn, n
        return wrap

    def collapse(self, orig):
        def wrap(ctx, T, P, mode, low=0.0, high=0.0, target=None):
            Fn, n = orig(ctx, T, P, mode, low, high, target)
            self.steps["collapse"] += 1
            self.check(Fn, P[:T.nv], "collapse")
            return Fn, n
        return wrap

    def flip(self, orig):
        def wrap(ctx, T, P):
            n = orig(ctx, T, P)
            self.steps["flip"] += 1
            self.check(T.F, P[:T.nv], "flip")
            return n
        return wrap

    def relax(self, orig):
        def wrap(ctx, T, V, grid, project):
            before = h(V.P[:T.nv]).astype(np.float64)
            orig(ctx, T, V, grid, project)
            self.steps["relax"] += 1
            after = h(V.P[:T.nv]).astype(np.float64)
            F = h(T.F).astype(np.int64)
            nb, na = _area_normal(before, F), _area_normal(after, F)
            bad = np.nonzero((np.abs(nb).sum(1) > 0) & ((nb * na).sum(1) <= 0))[0]
            self.flipped += [(self.steps["relax"], int(x)) for x in bad]
            assert not len(bad), ("a face with nonzero area turned over in a relaxation", self.steps["relax"], bad[:8])
            self.check(T.F, V.P[:T.nv], "relax")
        return wrap


@pytest.mark.parametrize("name", [n for n in ALL if n != "empty"])
def test_invariants_after_every_step(cuda, monkeypatch, name):
    v, f = mesh(name)
    w = Watch(monkeypatch, v, f, botsch=True)
    rd.remesh_botsch_device(*dev(v, f), 10, None)  # the default iteration count: a pole's valence drops below 65 by the 4th
    if len(f) > 8:
        assert w.steps["split"] and w.steps["collapse"] and w.steps["relax"], w.steps
    monkeypatch.undo()
    w = Watch(monkeypatch, v, f, botsch=False)
    rd.decimate_device(*dev(v, f), face_ratio=0.3)
