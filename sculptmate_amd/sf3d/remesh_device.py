"""Triangle remeshing with the mesh in HBM: decimate / Botsch-Kobbelt / subdivide as HIP kernels (csrc/remesh_device.hip,
sculpt_rmd_* in include/sculpt_hip.h), with the contract of the host calls in sf3d/remesh.py:

    decimate_device(v, f, face_ratio=0.1, num_faces=None) -> (v, f, None, None)
    remesh_botsch_device(v, f, i=10, h=None, project=True) -> (v, f)
    subdivide_device(v, f, iters=1) -> (v, f)
    device_remesher(mesh, mode, vertex_count, remesh_steps=10) -> Mesh      the SF3D.remesher hook, opt-in
    simplify_device(v, f, target_faces) -> (v, f, vertex_index)             quadric-error collapse (ops.mesh_simplify)
    smooth_device(v, f, iterations, lam, mu) -> v                           Taubin lambda|mu smoothing (ops.mesh_smooth)
    loop_subdivide_device(v, f, levels, attributes=None) -> (v, f, attributes)   Loop subdivision (ops.mesh_subdivide)

v and f are HIP tensors (v any float dtype, f any integer dtype); results are float32 [n, 3] / int32 [m, 3] HIP tensors.  CPU
tensors are refused.  The rules are the host's (csrc/remesh_host.h); its sequential order becomes rounds of independent local
operations: every candidate claims its footprint, the winners of a round share no vertex.  Sorts and prefix sums are torch;
every per-element step is a kernel.  The output does not depend on scheduling: two runs give the same bits.  Not the host's
output vertex for vertex (a different order of operations): PARITY UNPINNED, like the host remesher's own.

What the host reads back per pass (a few integers: edge counts, round results, buffer totals) is counted in `last_stats()`.
"""
import ctypes
import math

import torch

from .. import _lib
from .._lib import SculptError, check, lib

SPLIT_SWEEPS = 16  # like the host: halving an edge longer than 2 high leaves halves that are still too long
COLLAPSE_ROUNDS = 8  # Botsch pass: rounds of independent collapses per iteration (stops early when a round collapses nothing)
FLIP_ROUNDS = 4
CAPACITY_GROWTH = 1.5  # first guess for the buffers a split sweep writes: 1.5 x the current mesh

_last = {}


def last_stats():
    """Counters of the last device call: passes (topology rebuilds), readbacks, split / collapse / flip counts, capacity retries."""
    return dict(_last)


class _Ctx:
    def __init__(self):
        self.stats = {"passes": 0, "readbacks": 0, "splits": 0, "collapses": 0, "flips": 0, "capacity_retries": 0, "rounds": 0}
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def read(self, *ts):
        """One device -> host copy of a few integer / float scalars."""
        self.stats["readbacks"] += 1
        if len(ts) == 1:
            return ts[0].reshape(-1)[:1].tolist()[0]
        return torch.stack([t.reshape(-1)[0].to(torch.float64) for t in ts]).tolist()

    def done(self):
        _last.clear()
        _last.update(self.stats)


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def _inputs(v, f, who, check_faces=True, allow_repeated=False):
    """allow_repeated: a face that names a vertex twice passes (a distance query can live with it; a topology pass cannot)."""
    for t, name in ((v, "v"), (f, "f")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise SculptError("%s: %s must be a CUDA/HIP tensor (no CPU fallback)" % (who, name))
    if v.dtype not in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
        raise SculptError("%s: v must be a float tensor, got %s" % (who, v.dtype))
    if f.dtype.is_floating_point or f.dtype == torch.bool:
        raise SculptError("%s: f must be an integer tensor, got %s" % (who, f.dtype))
    P = v.detach().reshape(-1, 3).to(torch.float32).clone().contiguous()  # owned: the passes write in place
    fl = f.detach().reshape(-1, 3)
    nv, nf = P.shape[0], fl.shape[0]
    if nv >= 1 << 31 or 3 * nf >= 1 << 31:
        raise SculptError("%s: mesh too large for int32 indices" % who)
    if nf and (int(fl.min()) < 0 or int(fl.max()) >= nv):  # before the int32 cast can wrap an index into range
        raise SculptError("%s: face index out of range" % who)
    F = fl.to(torch.int32).clone().contiguous()
    if check_faces and (nv or nf):
        status = torch.empty(1, dtype=torch.int32, device=P.device)
        check(lib.sculpt_rmd_validate(_p(P), nv, _p(F), nf, _p(status), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        s = int(status.item())
        if s & 1:
            raise SculptError("%s: face index out of range" % who)
        if s & 2 and not allow_repeated:
            raise SculptError("%s: degenerate face (repeated vertex index)" % who)
        if s & 4:
            raise SculptError("%s: non-finite vertex position" % who)
    return P, F


class _Topo:
    """Edge table, vertex -> corner CSR and boundary flags of the faces F (see csrc/remesh_device.hip).  `carry`: the previous
    pass's bnd (None: the first pass over an input, whose vertices with more than 64 neighbours become features).  Like the
    host's Mesh, a flag once set stays for the whole call: a high-valence vertex is a feature even after its valence drops."""

    def __init__(self, ctx, F, nv, carry=None):
        ctx.stats["passes"] += 1
        dev = F.device
        s = ctx.stream
        nf = F.shape[0]
        nh = 3 * nf
        self.F, self.nf, self.nv = F, nf, nv
        keys = torch.empty(nh, dtype=torch.int64, device=dev)
        check(lib.sculpt_rmd_halfedge_keys(_p(F), nf, _p(keys), s))
        self.skeys, sperm = torch.sort(keys, stable=True)
        head = torch.empty(nh, dtype=torch.int32, device=dev)
        check(lib.sculpt_rmd_edge_heads(_p(self.skeys), nh, _p(head), s))
        eid = torch.cumsum(head, 0, dtype=torch.int32)
        self.she = torch.empty(nh, dtype=torch.int32, device=dev)
        self.fe = torch.empty(nh, dtype=torch.int32, device=dev)
        self.es = torch.empty(nh + 1, dtype=torch.int32, device=dev) if nh else torch.zeros(1, dtype=torch.int32, device=dev)  # es[ne] = 3 nf
        check(lib.sculpt_rmd_edge_fill(_p(sperm), _p(eid), nh, _p(self.she), _p(self.fe), _p(self.es), s))
        self.ne = ctx.read(eid[-1:]) if nh else 0
        sv, vperm = torch.sort(F.reshape(-1), stable=True)
        self.vfc = vperm.to(torch.int32)
        self.vfs = torch.searchsorted(sv, torch.arange(nv + 1, dtype=torch.int32, device=dev), out_int32=True)
        self.bnd = torch.zeros(max(nv, 1), dtype=torch.uint8, device=dev)
        if carry is not None:
            n = min(nv, carry.shape[0])
            self.bnd[:n] = carry[:n]  # vertices a split added start at 0
        self.c = _lib.RmdTopo(F.data_ptr() if nf else 0, self.skeys.data_ptr() if nh else 0, self.she.data_ptr() if nh else 0,
                              self.es.data_ptr(), self.fe.data_ptr() if nh else 0, self.vfs.data_ptr(),
                              self.vfc.data_ptr() if nh else 0, self.bnd.data_ptr(), nf, nv, self.ne)
        if carry is None:
            check(lib.sculpt_rmd_high_valence(self.ref(), _p(self.bnd), s))
        check(lib.sculpt_rmd_boundary(self.ref(), _p(self.bnd), s))

    def ref(self):
        return ctypes.c_void_p(ctypes.addressof(self.c))


def _compact_faces(ctx, F, alive, nf_new):
    incl = torch.cumsum(alive, 0, dtype=torch.int32)
    Fo = torch.empty((nf_new, 3), dtype=torch.int32, device=F.device)
    check(lib.sculpt_rmd_compact_faces(_p(F), _p(alive), _p(incl), F.shape[0], _p(Fo), ctx.stream))
    return Fo


def _compact_vertices(ctx, P, nv, F, with_index=False):
    """Referenced vertices in index order; F is renumbered in place.  with_index: also the kept vertices' old indices (i64)."""
    used = torch.zeros(max(nv, 1), dtype=torch.int32, device=P.device)
    check(lib.sculpt_rmd_mark_used(_p(F), F.shape[0], _p(used), ctx.stream))
    incl = torch.cumsum(used, 0, dtype=torch.int32)
    n = ctx.read(incl[nv - 1:nv]) if nv else 0
    Po = torch.empty((n, 3), dtype=torch.float32, device=P.device)
    check(lib.sculpt_rmd_compact_vertices(_p(P), _p(used), _p(incl), nv, _p(Po), _p(F), F.shape[0], ctx.stream))
    if with_index:
        # old index of every kept vertex without another wait (n is known): row incl - 1 takes it, unused rows share a spare slot
        dest = torch.where(used[:nv] > 0, incl[:nv] - 1, n).long()
        index = torch.empty(n + 1, dtype=torch.int64, device=P.device)
        index.scatter_(0, dest, torch.arange(nv, dtype=torch.int64, device=P.device))
        return Po, index[:n]
    return Po


def _qem_propose(ctx, T, P, Q, target, claim, cand):
    """The quadric-error proposal of one round: every edge's key and target point, then the claims of the candidates under the
    round's cap -- the k-th smallest key, k = ceil((faces - target) / 2): a collapse removes at most two faces, so the k cheapest
    could reach the target on their own, and a dearer edge that is merely the cheapest of its neighbourhood waits.  The cap stays
    on the device.  Returns the targets [ne, 3]."""
    tgt = torch.empty((max(T.ne, 1), 3), dtype=torch.float32, device=P.device)
    check(lib.sculpt_rmd_qem_cost(T.ref(), _p(P), _p(Q), _p(cand), _p(tgt), ctx.stream))
    if T.ne == 0:
        return tgt
    k = max(1, min(T.ne, (T.nf - target + 1) // 2))
    # a key holds non-negative fp32 bits, so it orders the same signed; "no candidate" (~0 = -1) goes last
    keys = torch.where(cand[:T.ne] == -1, torch.iinfo(torch.int64).max, cand[:T.ne])
    cap = torch.sort(keys).values[k - 1:k].contiguous()  # (a sort: kthvalue selects a 1-D tensor with a single workgroup)
    check(lib.sculpt_rmd_qem_claim(T.ref(), _p(cand), _p(cap), _p(claim), ctx.stream))
    return tgt


def _collapse_round(ctx, T, P, mode, low=0.0, high=0.0, target=None, Q=None):
    """One round of independent collapses on T's faces; returns (new faces, collapses) -- (T.F, 0) if nothing collapsed.
    Q (quadrics fp64 [nv, 10]; mode 0, with a target): the quadric-error rule instead of the shortest edge (_qem_propose)."""
    dev = P.device
    claim = torch.full((max(T.nv, 1),), -1, dtype=torch.int64, device=dev)  # ~0: unclaimed
    cand = torch.empty(max(T.ne, 1), dtype=torch.int64, device=dev)
    win = torch.empty(max(T.ne, 1), dtype=torch.int32, device=dev)
    if Q is None:
        check(lib.sculpt_rmd_collapse_propose(T.ref(), _p(P), mode, float(low), float(high), _p(claim), _p(cand), ctx.stream))
    else:
        tgt = _qem_propose(ctx, T, P, Q, target, claim, cand)
    check(lib.sculpt_rmd_collapse_select(T.ref(), _p(P), mode, _p(claim), _p(cand), _p(win), ctx.stream))
    win = win[:T.ne]
    removed, n = ctx.read(win.sum(), (win > 0).sum())
    removed, n = int(removed), int(n)
    if n == 0:
        return T.F, 0
    if target is not None and T.nf - removed < target:
        # the last round of a decimation: keep the winners in priority order while more than `target` faces are left
        idx = torch.nonzero(win).squeeze(1)
        order = torch.argsort(cand[idx])
        rem = win[idx[order]].to(torch.int64)
        before = T.nf - (torch.cumsum(rem, 0) - rem)
        keep = before > target
        win[idx[order[~keep]]] = 0
        removed, n = ctx.read(rem[keep].sum(), keep.sum())
        removed, n = int(removed), int(n)
        if n == 0:
            return T.F, 0
    alive = torch.ones(T.nf, dtype=torch.uint8, device=dev)
    F = T.F
    if Q is None:
        check(lib.sculpt_rmd_collapse_apply(T.ref(), _p(P), _p(F), mode, _p(win), _p(alive), ctx.stream))
    else:
        check(lib.sculpt_rmd_qem_apply(T.ref(), _p(P), _p(F), _p(Q), _p(tgt), _p(win), _p(alive), ctx.stream))
    if mode == 0:
        # the kept end (the larger index) inherits the removed end's flag, as in Mesh::collapse; in mode 1 the removed end is
        # never flagged
        key = T.skeys[T.es[:T.ne][win > 0].long()]
        lo, hi = key >> 32, key & 0xFFFFFFFF
        T.bnd[hi] |= T.bnd[lo]
    ctx.stats["collapses"] += n
    return _compact_faces(ctx, F, alive, T.nf - removed), n


def _flip_round(ctx, T, P):
    dev = P.device
    claim = torch.full((max(T.nv, 1),), -1, dtype=torch.int64, device=dev)
    cand = torch.empty(max(T.ne, 1), dtype=torch.int64, device=dev)
    win = torch.empty(max(T.ne, 1), dtype=torch.int32, device=dev)
    check(lib.sculpt_rmd_flip_propose(T.ref(), _p(P), _p(claim), _p(cand), ctx.stream))
    check(lib.sculpt_rmd_flip_apply(T.ref(), _p(P), _p(claim), _p(cand), _p(T.F), _p(win), ctx.stream))
    n = int(ctx.read(win[:T.ne].sum()))
    ctx.stats["flips"] += n
    return n


class _VBuf:
    """Positions with spare rows for the vertices splits append."""

    def __init__(self, P):
        self.nv = P.shape[0]
        self.buf = torch.empty((max(int(self.nv * CAPACITY_GROWTH), self.nv + 64), 3), dtype=torch.float32, device=P.device)
        self.buf[:self.nv] = P

    @property
    def P(self):
        return self.buf

    def grow(self, need):
        nb = torch.empty((max(need, int(self.buf.shape[0] * CAPACITY_GROWTH)), 3), dtype=torch.float32, device=self.buf.device)
        nb[:self.nv] = self.buf[:self.nv]
        self.buf = nb


def _split_sweep(ctx, T, V, high):
    """Split every edge longer than `high` (one or two faces) at its midpoint; returns (new faces, splits).  The children go
    into buffers of a guessed size; the kernels write nothing past the capacity, and when the totals read back exceed it the
    emit runs again into buffers of the exact size."""
    dev = V.buf.device
    ne = max(T.ne, 1)
    mark = torch.zeros(ne, dtype=torch.int32, device=dev)
    check(lib.sculpt_rmd_split_mark(T.ref(), _p(V.P), float(high), _p(mark), ctx.stream))
    mark_incl = torch.cumsum(mark, 0, dtype=torch.int32)
    cnt = torch.empty(max(T.nf, 1), dtype=torch.int32, device=dev)
    check(lib.sculpt_rmd_split_count(T.ref(), _p(mark), _p(cnt), ctx.stream))
    off_incl = torch.cumsum(cnt[:T.nf], 0, dtype=torch.int32)
    fcap = max(int(T.nf * CAPACITY_GROWTH), 64)
    Fo = torch.empty((fcap, 3), dtype=torch.int32, device=dev)
    for attempt in range(2):
        check(lib.sculpt_rmd_split_emit(T.ref(), _p(V.P), V.buf.shape[0], _p(mark), _p(mark_incl), _p(off_incl), Fo.shape[0], _p(Fo),
                                        ctx.stream))
        if attempt:
            break
        nsplit, nf_new = (int(x) for x in ctx.read(mark_incl[T.ne - 1:], off_incl[T.nf - 1:]))
        if nsplit == 0:
            return T.F, 0
        if T.nv + nsplit <= V.buf.shape[0] and nf_new <= fcap:
            break
        ctx.stats["capacity_retries"] += 1
        if T.nv + nsplit > V.buf.shape[0]:
            V.grow(T.nv + nsplit)
        if nf_new > fcap:
            Fo = torch.empty((nf_new, 3), dtype=torch.int32, device=dev)
    V.nv = T.nv + nsplit
    ctx.stats["splits"] += nsplit
    return Fo[:nf_new], nsplit


class _Grid:
    """Uniform grid over the projection surface (remesh_host.h SurfaceGrid): cells about a triangle wide, at most ~4 per face."""

    def __init__(self, ctx, GP, GF):
        self.GP, self.GF = GP, GF
        dev = GP.device
        nf = GF.shape[0]
        if nf == 0:
            self.params = (ctypes.c_double * 7)(0, 0, 0, 1, 1, 1, 1)
            self.items = self.start = None
            self.amax = self.longest = 0.0
            self.bounds = None
            return
        pts = GP[GF.reshape(-1).long()].to(torch.float64)
        lo, hi = pts.min(0).values, pts.max(0).values
        b = ctx.read(lo[0:1], lo[1:2], lo[2:3], hi[0:1], hi[1:2], hi[2:3])
        lo3, ext = b[:3], [b[3 + k] - b[k] for k in range(3)]
        self.bounds = (lo3, ext)  # least corner and extent over the vertices the faces name (ops.mesh_sdf_grid)
        self.amax = max(abs(x) for x in b)  # the largest |coordinate| of the surface (ops.mesh_closest_points)
        self.longest = longest = max(ext)  # the longest side of the bounds (ops.mesh_occlusion's default offset)
        per_side = max(1.0, min(math.sqrt(nf / 2.0), (4.0 * nf) ** (1.0 / 3.0)))
        cell = longest / per_side if longest > 0 else 1.0
        n = [max(1, min(1024, int(math.floor(e / cell)) + 1)) for e in ext]
        self.params = (ctypes.c_double * 7)(lo3[0], lo3[1], lo3[2], cell, n[0], n[1], n[2])
        cnt = torch.empty(nf, dtype=torch.int32, device=dev)
        check(lib.sculpt_rmd_grid_count(_p(GP), _p(GF), nf, self.params, _p(cnt), ctx.stream))
        off = torch.cumsum(cnt, 0, dtype=torch.int32)
        total = int(ctx.read(off[-1:]))
        cellid = torch.empty(total, dtype=torch.int32, device=dev)
        face = torch.empty(total, dtype=torch.int32, device=dev)
        check(lib.sculpt_rmd_grid_fill(_p(GP), _p(GF), nf, self.params, _p(off), _p(cellid), _p(face), ctx.stream))
        sc, perm = torch.sort(cellid, stable=True)
        self.items = face[perm]
        nc = n[0] * n[1] * n[2]
        self.start = torch.searchsorted(sc, torch.arange(nc + 1, dtype=torch.int32, device=dev), out_int32=True)


def _relax(ctx, T, V, grid, project):
    Q = torch.empty_like(V.buf)
    undo = torch.empty(_lib.rmd_undo_bytes(T.nv), dtype=torch.uint8, device=V.buf.device)
    g = grid if project else None
    check(lib.sculpt_rmd_relax(T.ref(), _p(V.P), _p(g.GP) if g else None, _p(g.GF) if g else None, g.GF.shape[0] if g else 0,
                               _p(g.items) if g else None, _p(g.start) if g else None, g.params if g else None, 1 if project else 0,
                               _p(Q), _p(undo), ctx.stream))
    V.buf = Q


def _mean_halfedge_length(ctx, P, F):
    if F.shape[0] == 0:
        return 0.0
    lens = torch.empty(F.shape[0], dtype=torch.float64, device=P.device)
    check(lib.sculpt_rmd_halfedge_lengths(_p(P), _p(F), F.shape[0], _p(lens), ctx.stream))
    return float(ctx.read(lens.sum())) / (3.0 * F.shape[0])


# ---------------------------------------------------------------------------------------------------------------- public
def subdivide_device(v, f, iters=1):
    """gpytoolbox.subdivide(v, f, method='upsample', iters=...) on the device: the host's numbering (edge vertices after the
    old ones, in order of first appearance over the faces) and the host's face template."""
    iters = int(iters)
    if not 0 <= iters <= 12:
        raise SculptError("mesh_subdivide: iters=%d out of range" % iters)
    P, F = _inputs(v, f, "mesh_subdivide", check_faces=False)
    if F.shape[0] * 4.0 ** iters >= 1.5e9:
        raise SculptError("mesh_subdivide: %d faces x 4^%d does not fit int32 indices" % (F.shape[0], iters))
    ctx = _Ctx()
    for _ in range(iters):
        nv = P.shape[0]
        T = _Topo(ctx, F, nv)
        first = torch.empty(max(3 * T.nf, 1), dtype=torch.int32, device=P.device)
        check(lib.sculpt_rmd_first_halfedge(T.ref(), _p(first), ctx.stream))
        rank = torch.cumsum(first[:3 * T.nf], 0, dtype=torch.int32)
        Po = torch.empty((nv + T.ne, 3), dtype=torch.float32, device=P.device)
        Fo = torch.empty((4 * T.nf, 3), dtype=torch.int32, device=P.device)
        check(lib.sculpt_rmd_subdivide(T.ref(), _p(P), _p(rank), _p(Po), _p(Fo), ctx.stream))
        P, F = Po, Fo
    ctx.done()
    return P, F


LOOP_MAX_CHANNELS = 8  # csrc/mesh_subdivide.hip kMaxChannels


def _loop_topology(ctx, F, nv):
    """The topology of one Loop level.  A zero `carry`, as in _smooth_table: the kernels classify by the edges' face counts and
    never read bnd, so the scan for vertices of more than 64 neighbours is not run."""
    return _Topo(ctx, F, nv, carry=torch.zeros(max(nv, 1), dtype=torch.uint8, device=F.device))


def _loop_level(ctx, T, P, A=None):
    """One Loop level on the topology T of (P, T.F): the numbering (sculpt_rmd_first_halfedge, as subdivide_device), then the two
    launches of csrc/mesh_subdivide.hip -> (P' [nv + ne, 3], F' [4 nf, 3], A' or None); nothing is read back."""
    dev, s, nv = P.device, ctx.stream, T.nv
    first = torch.empty(3 * T.nf, dtype=torch.int32, device=dev)
    check(lib.sculpt_rmd_first_halfedge(T.ref(), _p(first), s))
    rank = torch.cumsum(first, 0, dtype=torch.int32)
    cls = torch.empty((nv, 4), dtype=torch.int32, device=dev)
    rows = torch.empty((nv, 4), dtype=torch.float32, device=dev)
    check(lib.sculpt_subdiv_classify(T.ref(), _p(P), _p(cls), _p(rows), s))
    Po = torch.empty((nv + T.ne, 3), dtype=torch.float32, device=dev)
    Fo = torch.empty((4 * T.nf, 3), dtype=torch.int32, device=dev)
    Ao = None if A is None else torch.empty((nv + T.ne, A.shape[1]), dtype=torch.float32, device=dev)
    check(lib.sculpt_subdiv_loop(T.ref(), _p(cls), _p(rows), _p(rank), _p(A), 0 if A is None else A.shape[1], _p(Po), _p(Fo), _p(Ao), s))
    return Po, Fo, Ao


def _attributes(attributes, nv, who):
    """attributes of a subdivision -> an owned f32 [nv, C] device tensor, 1 <= C <= LOOP_MAX_CHANNELS (None stays None)."""
    if attributes is None:
        return None
    a = attributes
    if not (isinstance(a, torch.Tensor) and a.is_cuda):
        raise SculptError("%s: attributes must be a CUDA/HIP tensor (no CPU fallback)" % who)
    if not a.dtype.is_floating_point or a.dim() != 2 or a.shape[0] != nv or not 1 <= a.shape[1] <= LOOP_MAX_CHANNELS:
        raise SculptError("%s: attributes must be float [%d, C] with 1 <= C <= %d (a row per vertex), got %s %s"
                          % (who, nv, LOOP_MAX_CHANNELS, a.dtype, tuple(a.shape)))
    return a.detach().to(torch.float32).clone().contiguous()


def loop_subdivide_device(v, f, levels, attributes=None):
    """`levels` levels of Loop subdivision (csrc/mesh_subdivide.hip; the contract is in include/sculpt_hip.h and
    ops.mesh_subdivide): the faces and the numbering of subdivide_device, the positions and the optional attributes (float
    [nv, C], C <= 8) by the scheme's masks, in fp64 rounded once.  -> (v f32 [n, 3], f int32 [m, 3], attributes f32 [n, C] or
    None), new tensors.  A face index out of range, a repeated index in a face and a non-finite position are a SculptError.  One
    topology construction per level, whose edge count is the level's one readback; no faces: copies."""
    levels = int(levels)
    if not 0 <= levels <= 12:
        raise SculptError("mesh_subdivide: levels=%d out of range" % levels)
    P, F = _inputs(v, f, "mesh_subdivide")
    A = _attributes(attributes, P.shape[0], "mesh_subdivide")
    if F.shape[0] * 4.0 ** levels >= 1.5e9:  # subdivide_device's bound
        raise SculptError("mesh_subdivide: %d faces x 4^%d does not fit int32 indices" % (F.shape[0], levels))
    ctx = _Ctx()
    if F.shape[0]:
        for _ in range(levels):
            P, F, A = _loop_level(ctx, _loop_topology(ctx, F, P.shape[0]), P, A)
    ctx.done()
    return P, F, A


class _PolyTopo:
    """Edge table and vertex -> corner CSR of the faces F [nf, k], k = 3 or 4 (sculpt_catmull_topo_t): _Topo's construction for
    k corners, without the boundary flags -- the Catmull-Clark kernels classify by the edges' face counts."""

    def __init__(self, ctx, F, nv):
        ctx.stats["passes"] += 1
        dev, s = F.device, ctx.stream
        nf, k = F.shape
        nh = k * nf
        self.F, self.nf, self.nv, self.k = F, nf, nv, k
        keys = torch.empty(nh, dtype=torch.int64, device=dev)
        check(lib.sculpt_catmull_halfedge_keys(_p(F), nf, k, _p(keys), s))
        self.skeys, sperm = torch.sort(keys, stable=True)
        head = torch.empty(nh, dtype=torch.int32, device=dev)
        check(lib.sculpt_rmd_edge_heads(_p(self.skeys), nh, _p(head), s))
        eid = torch.cumsum(head, 0, dtype=torch.int32)
        self.she = torch.empty(nh, dtype=torch.int32, device=dev)
        self.fe = torch.empty(nh, dtype=torch.int32, device=dev)
        self.es = torch.empty(nh + 1, dtype=torch.int32, device=dev)  # es[ne] = k nf
        check(lib.sculpt_rmd_edge_fill(_p(sperm), _p(eid), nh, _p(self.she), _p(self.fe), _p(self.es), s))
        self.ne = ctx.read(eid[-1:])
        sv, vperm = torch.sort(F.reshape(-1), stable=True)
        self.vfc = vperm.to(torch.int32)
        self.vfs = torch.searchsorted(sv, torch.arange(nv + 1, dtype=torch.int32, device=dev), out_int32=True)
        self.c = _lib.CatmullTopo(F.data_ptr(), self.skeys.data_ptr(), self.she.data_ptr(), self.es.data_ptr(), self.fe.data_ptr(),
                                  self.vfs.data_ptr(), self.vfc.data_ptr(), nf, nv, self.ne, k)

    def ref(self):
        return ctypes.c_void_p(ctypes.addressof(self.c))


def _catmull_level(ctx, T, P, A=None):
    """One Catmull-Clark level on the topology T of (P, T.F): the numbering, then the two launches of csrc/mesh_catmull.hip ->
    (P' [nv + nf + ne, 3], quads [k nf, 4], triangles [2 k nf, 3], A' or None); nothing is read back."""
    dev, s, nv = P.device, ctx.stream, T.nv
    first = torch.empty(T.k * T.nf, dtype=torch.int32, device=dev)
    check(lib.sculpt_catmull_first_halfedge(T.ref(), _p(first), s))
    rank = torch.cumsum(first, 0, dtype=torch.int32)
    cls = torch.empty((nv, 4), dtype=torch.int32, device=dev)
    rows = torch.empty((nv, 4), dtype=torch.float32, device=dev)
    check(lib.sculpt_catmull_classify(T.ref(), _p(P), _p(cls), _p(rows), s))
    n = nv + T.nf + T.ne
    Po = torch.empty((n, 3), dtype=torch.float32, device=dev)
    Qo = torch.empty((T.k * T.nf, 4), dtype=torch.int32, device=dev)
    To = torch.empty((2 * T.k * T.nf, 3), dtype=torch.int32, device=dev)
    Ao = None if A is None else torch.empty((n, A.shape[1]), dtype=torch.float32, device=dev)
    check(lib.sculpt_catmull_refine(T.ref(), _p(cls), _p(rows), _p(rank), _p(A), 0 if A is None else A.shape[1], _p(Po), _p(Qo), _p(To),
                                    _p(Ao), s))
    return Po, Qo, To, Ao


def catmull_clark_device(v, f, levels, attributes=None):
    """`levels` (1 .. 6) levels of Catmull-Clark subdivision (csrc/mesh_catmull.hip; the rule is in include/sculpt_hip.h, the
    contract in ops.mesh_catmull_clark).  f: [nf, 3] or [nf, 4]; only the first level can see triangles.  -> (v f32 [n, 3],
    quads int32 [m, 4], triangles int32 [2 m, 3], attributes f32 [n, C] or None), new tensors.  One topology construction per
    level, whose edge count is the level's one readback; before the first, the input check's status.  No faces: copies, and
    empty quads and triangles."""
    who = "mesh_catmull_clark"
    levels = int(levels)
    if not 1 <= levels <= 6:
        raise SculptError("%s: levels=%d out of range (1 .. 6)" % (who, levels))
    for t, name in ((v, "vertices"), (f, "faces")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise SculptError("%s: %s must be a CUDA/HIP tensor (no CPU fallback)" % (who, name))
    if not v.dtype.is_floating_point or v.dim() != 2 or v.shape[1] != 3:
        raise SculptError("%s: vertices must be float [Nv, 3], got %s %s" % (who, v.dtype, tuple(v.shape)))
    if f.dtype not in (torch.int32, torch.int64):
        raise SculptError("%s: faces must be int32 or int64, got %s" % (who, f.dtype))
    if f.dim() != 2 or f.shape[1] not in (3, 4):
        raise SculptError("%s: faces must be [Nf, 3] or [Nf, 4], got %s" % (who, tuple(f.shape)))
    P = v.detach().reshape(-1, 3).to(torch.float32).clone().contiguous()
    nv, (nf, k) = P.shape[0], f.shape
    if nv >= 1 << 31 or nf >= 1 << 27:
        raise SculptError("%s: mesh too large for int32 indices" % who)
    A = _attributes(attributes, nv, who)
    ctx = _Ctx()
    if nf and (int(f.min()) < 0 or int(f.max()) >= nv):  # before the int32 cast can wrap an index into range
        raise SculptError("%s: face index out of range" % who)
    F = f.detach().to(torch.int32).clone().contiguous()
    if nv or nf:
        status = torch.empty(1, dtype=torch.int32, device=P.device)
        check(lib.sculpt_catmull_validate(_p(P), nv, _p(F), nf, k, _p(status), ctx.stream))
        st = int(ctx.read(status))
        if st & 1:
            raise SculptError("%s: face index out of range" % who)
        if st & 2:
            raise SculptError("%s: degenerate face (repeated vertex index)" % who)
        if st & 4:
            raise SculptError("%s: non-finite vertex position" % who)
    # every level turns nq quads into 4 nq (the first: k nf); the last level's 4 x quads index entries must stay in int32
    if 4 * k * nf * 4 ** (levels - 1) >= 1 << 31:
        raise SculptError("%s: %d faces of %d corners x 4^%d does not fit int32 indices" % (who, nf, k, levels - 1))
    Q = torch.empty((0, 4), dtype=torch.int32, device=P.device)
    Tr = torch.empty((0, 3), dtype=torch.int32, device=P.device)
    if nf:
        for _ in range(levels):
            P, Q, Tr, A = _catmull_level(ctx, _PolyTopo(ctx, F, P.shape[0]), P, A)
            F = Q
    ctx.done()
    return P, Q, Tr, A


def _decimate(ctx, P, F, target):
    V = P
    T = None
    while F.shape[0] > target:
        T = _Topo(ctx, F, V.shape[0], carry=T.bnd if T is not None else None)
        ctx.stats["rounds"] += 1
        F, n = _collapse_round(ctx, T, V, 0, target=target)
        if n == 0:
            break
    V = _compact_vertices(ctx, V, V.shape[0], F)
    return V, F


def simplify_device(v, f, target_faces):
    """Quadric-error edge collapse (csrc/mesh_simplify.hip) down to at most `target_faces` faces, or to where a round collapses
    nothing: the rounds of _decimate with the quadric rule of _qem_propose.  -> (v f32 [n, 3], f int32 [m, 3], vertex_index i64
    [n]: the input vertex every output vertex descends from -- the kept end of its collapses).  The quadrics are built once, on
    the first topology; vertices keep their indices until the final compaction."""
    P, F = _inputs(v, f, "mesh_simplify")
    target = max(0, int(target_faces))
    ctx = _Ctx()
    nv = P.shape[0]
    T = Q = None
    while F.shape[0] > target:
        T = _Topo(ctx, F, nv, carry=T.bnd if T is not None else None)
        if Q is None:
            Q = torch.empty((max(nv, 1), 10), dtype=torch.float64, device=P.device)
            check(lib.sculpt_rmd_qem_quadrics(T.ref(), _p(P), _p(Q), ctx.stream))
        ctx.stats["rounds"] += 1
        F, n = _collapse_round(ctx, T, P, 0, target=target, Q=Q)
        if n == 0:
            break
    P, index = _compact_vertices(ctx, P, nv, F, with_index=True)
    ctx.done()
    return P, F, index


def _plain_topo(ctx, F, nv):
    """The topology of F with a zero `carry`: bnd[u] = 1 exactly where an edge at u does not have exactly two faces."""
    return _Topo(ctx, F, nv, carry=torch.zeros(max(nv, 1), dtype=torch.uint8, device=F.device))


def _smooth_table(ctx, F, nv, topo=None):
    """(start i32 [nv + 1], nb i32 [2 ne], fixed u8 [nv]) of the faces F: row u of the CSR holds the distinct neighbours of u in
    ascending order; fixed[u] = 1 where an edge at u does not have exactly two faces.  The topology gets a zero `carry`, so the
    remesher's more-than-64-neighbours feature rule is not applied: a high-valence vertex is smoothed like any other.  The
    directed keys of the unique edges are distinct, so their sorted order -- and with it the table -- is unique.  topo: a
    _plain_topo of F the caller has already (None: one is built)."""
    dev = F.device
    T = topo if topo is not None else _plain_topo(ctx, F, nv)
    keys = torch.empty(2 * T.ne, dtype=torch.int64, device=dev)
    check(lib.sculpt_smooth_edge_keys(T.ref(), _p(keys), ctx.stream))
    skeys = torch.sort(keys).values
    start = torch.searchsorted(skeys, torch.arange(nv + 1, dtype=torch.int64, device=dev) << 32, out_int32=True)
    nb = torch.empty(2 * T.ne, dtype=torch.int32, device=dev)
    check(lib.sculpt_smooth_neighbours(_p(skeys), 2 * T.ne, _p(nb), ctx.stream))
    return start, nb, T.bnd[:nv]


def _smooth_steps(ctx, P, table, n, lam, mu):
    """`n` iterations of the two half-steps on P [nv, 3] f32 -> a new tensor; every launch is queued, nothing is read back."""
    start, nb, fixed = table
    nv = P.shape[0]
    work = torch.empty((2, max(nv, 1), 4), dtype=torch.float32, device=P.device)
    out = torch.empty_like(P)
    check(lib.sculpt_smooth_taubin(_p(start), _p(nb), _p(fixed), nv, nb.shape[0], _p(P), int(n), float(lam), float(mu),
                                   _p(work[0]), _p(work[1]), _p(out), ctx.stream))
    ctx.stats["smooth_iterations"] = int(n)
    return out


def smooth_device(v, f, iterations, lam, mu):
    """Taubin's lambda|mu filter (csrc/mesh_smooth.hip): `iterations` times a half-step with lam, then one with mu (mu == 0: the
    first alone), every vertex towards (lam) or away from (mu) the centroid of its distinct neighbours; vertices on an edge
    without exactly two faces, and vertices no face names, stay.  -> v f32 [nv, 3], a new tensor; the faces are not touched.
    The host reads back what one topology construction reads (the edge count) and, before it, the input check's status."""
    P, F = _inputs(v, f, "mesh_smooth")
    ctx = _Ctx()
    if F.shape[0] and P.shape[0]:
        P = _smooth_steps(ctx, P, _smooth_table(ctx, F, P.shape[0]), iterations, lam, mu)
    ctx.done()
    return P


def _curvature_terms(ctx, T, P, outward):
    """(area, deficit, hint f64 [nv], valid u8 [nv]) of the topology T (a _plain_topo) over P f32 [nv, 3]: one pack and one gather."""
    nv, dev = P.shape[0], P.device
    area, deficit, hint = (torch.empty(nv, dtype=torch.float64, device=dev) for _ in range(3))
    valid = torch.empty(nv, dtype=torch.uint8, device=dev)
    work = torch.empty((max(nv, 1), 4), dtype=torch.float32, device=dev)
    check(lib.sculpt_curvature_terms(T.ref(), _p(P), float(outward), _p(work), _p(area), _p(deficit), _p(hint), _p(valid), ctx.stream))
    return area, deficit, hint, valid


def _curvature_ring(ctx, terms, start, nb, rounds):
    """`rounds` rounds of X'_u = X_u + the sum over the valid neighbours of u, on the three f64 channels of `terms` -> new terms."""
    area, deficit, hint, valid = terms
    nv, dev = area.shape[0], area.device
    out = tuple(torch.empty(nv, dtype=torch.float64, device=dev) for _ in range(3))
    work = torch.empty((2, max(nv, 1), 4), dtype=torch.float64, device=dev)
    check(lib.sculpt_curvature_ring(_p(start), _p(nb), _p(valid), nv, nb.shape[0], int(rounds), _p(area), _p(deficit), _p(hint),
                                    _p(work[0]), _p(work[1]), _p(out[0]), _p(out[1]), _p(out[2]), ctx.stream))
    ctx.stats["curvature_rounds"] = int(rounds)
    return out + (valid,)


def _curvature_finish(ctx, terms):
    area, deficit, hint, valid = terms
    nv, dev = area.shape[0], area.device
    mean, gauss = (torch.empty(nv, dtype=torch.float32, device=dev) for _ in range(2))
    check(lib.sculpt_curvature_finish(_p(area), _p(deficit), _p(hint), _p(valid), nv, _p(mean), _p(gauss), ctx.stream))
    return mean, gauss


def curvature_device(v, f, rings, outward, finish=True):
    """Discrete mean and Gaussian curvature per vertex (csrc/mesh_curvature.hip): the raw terms of every vertex from its corners,
    `rings` rounds of sums over the neighbour table, the two quotients.  finish=True -> (mean f32, gauss f32, valid u8), each
    [nv]; finish=False -> the terms after the rounds (area, deficit, hint f64 [nv], valid u8 [nv]).  Without faces: NaN / zeros
    and nothing is launched.  The host reads back what one topology construction reads (the edge count) and, before it, the input
    check's status; the neighbour table is built from that same topology, and only when rings > 0."""
    P, F = _inputs(v, f, "mesh_curvature")
    ctx = _Ctx()
    nv, dev = P.shape[0], P.device
    if F.shape[0] and nv:
        T = _plain_topo(ctx, F, nv)
        terms = _curvature_terms(ctx, T, P, outward)
        if rings:
            start, nb, _ = _smooth_table(ctx, F, nv, topo=T)
            terms = _curvature_ring(ctx, terms, start, nb, rings)
        out = _curvature_finish(ctx, terms) + (terms[3],) if finish else terms
    elif finish:
        out = (torch.full((nv,), math.nan, dtype=torch.float32, device=dev), torch.full((nv,), math.nan, dtype=torch.float32, device=dev),
               torch.zeros(nv, dtype=torch.uint8, device=dev))
    else:
        out = tuple(torch.zeros(nv, dtype=torch.float64, device=dev) for _ in range(3)) + (torch.zeros(nv, dtype=torch.uint8, device=dev),)
    ctx.done()
    return out


def decimate_device(v, f, face_ratio=0.1, num_faces=None):
    """gpytoolbox.decimate(v, f, face_ratio=..., num_faces=None) -> (v, f, None, None) on the device: rounds of independent
    shortest-edge collapses to the midpoint (each winner the shortest valid edge of its footprint), the host's link condition,
    until at most floor(face_ratio * F) faces are left or a round collapses nothing."""
    P, F = _inputs(v, f, "mesh_decimate")
    if num_faces is None:
        num_faces = int(math.floor(face_ratio * F.shape[0]))
    ctx = _Ctx()
    V, F = _decimate(ctx, P, F, max(0, int(num_faces)))
    ctx.done()
    return V, F, None, None


def remesh_botsch_device(v, f, i=10, h=None, project=True):
    """gpytoolbox.remesh_botsch(v, f, i, h) on the device; h None = the mean (half-)edge length of the input.  Per iteration:
    split sweeps (> 4/3 h), rounds of collapses (< 4/5 h), rounds of valence flips, one tangential relaxation projected onto
    the input surface."""
    i = int(i)
    if not 0 <= i <= 1000:
        raise SculptError("mesh_remesh_botsch: iters=%d out of range" % i)
    if h is not None and h != h:
        raise SculptError("mesh_remesh_botsch: h is NaN")
    P, F = _inputs(v, f, "mesh_remesh_botsch")
    ctx = _Ctx()
    if h is None or h <= 0:
        h = _mean_halfedge_length(ctx, P, F)
    if h > 0 and F.shape[0] > 0 and i > 0:
        high, low = 4.0 / 3.0 * h, 4.0 / 5.0 * h
        grid = _Grid(ctx, P.clone(), F.clone()) if project else None
        V = _VBuf(P)
        T = _Topo(ctx, F, V.nv)
        for _ in range(i):
            for _ in range(SPLIT_SWEEPS):
                Fn, n = _split_sweep(ctx, T, V, high)
                if n == 0:
                    break
                T = _Topo(ctx, Fn, V.nv, carry=T.bnd)
            for _ in range(COLLAPSE_ROUNDS):
                Fn, n = _collapse_round(ctx, T, V.P, 1, low, high)
                if n == 0:
                    break
                T = _Topo(ctx, Fn, V.nv, carry=T.bnd)
            for _ in range(FLIP_ROUNDS):
                if _flip_round(ctx, T, V.P) == 0:
                    break
                T = _Topo(ctx, T.F, V.nv, carry=T.bnd)  # the faces were rewritten in place
            _relax(ctx, T, V, grid, project)
        P, F = V.P[:V.nv], T.F
    P = _compact_vertices(ctx, P.contiguous(), P.shape[0], F)
    ctx.done()
    return P, F


class DeviceToolbox:
    """The three device calls under the names Mesh.triangle_remesh uses."""
    subdivide = staticmethod(subdivide_device)
    decimate = staticmethod(decimate_device)
    remesh_botsch = staticmethod(remesh_botsch_device)


def triangle_remesh_device(mesh, vertex_count=-1, remesh_steps: int = 10, toolbox=DeviceToolbox):
    """sf3d/remesh.py triangle_remesh (Mesh.triangle_remesh, mesh.py:175-237) statement for statement with the mesh in HBM:
    subdivide while the mesh has fewer vertices than asked for, decimate with face_ratio = budget / vertices, remesh at the
    decimated mesh's own mean edge length (no budget: at the input's)."""
    from .system import Mesh

    v, f = mesh.v_pos.detach(), mesh.t_pos_idx.detach()
    if vertex_count > 0:
        ratio = vertex_count / v.shape[0]
        if ratio > 1.0:
            v, f = toolbox.subdivide(v, f, iters=int(math.ceil(math.log(ratio) / math.log(2))))
            ratio = vertex_count / v.shape[0]
        v, f, _, _ = toolbox.decimate(v, f, face_ratio=ratio)
    v, f = toolbox.remesh_botsch(v, f, remesh_steps, None)
    return Mesh(v.to(mesh.v_pos.dtype).contiguous(), f.to(mesh.t_pos_idx.dtype).contiguous(), unwrapper=mesh.unwrapper)


def device_remesher(mesh, mode, vertex_count, remesh_steps: int = 10):
    """(Mesh, "triangle", target vertex count) -> Mesh, the mesh kept in HBM: the device twin of sf3d/remesh.py
    native_remesher.  Opt-in: `SF3D.remesher = device_remesher`."""
    if mode != "triangle":
        raise NotImplementedError("remesh=%r: only 'triangle' exists (the reference's quad path is commented out, "
                                  "mesh.py:152-171)" % mode)
    for t, name in ((mesh.v_pos, "v_pos"), (mesh.t_pos_idx, "t_pos_idx")):
        if not t.is_cuda:
            raise SculptError("device_remesher: mesh.%s must be a CUDA/HIP tensor (no CPU fallback)" % name)
    return triangle_remesh_device(mesh, vertex_count, remesh_steps)
