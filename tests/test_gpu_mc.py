"""HIP marching cubes vs the C oracle / scikit-image goldens: bit-exact vertices, faces and order (MI355X)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import capi

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(GOLDEN, "mc_skimage.npz"))
NAMES = sorted(k[:-4] for k in G.files if k.endswith("_vol"))


def _same(v, f, rv, rf):
    assert tuple(f.shape) == rf.shape and tuple(v.shape) == rv.shape, (f.shape, rf.shape, v.shape, rv.shape)
    assert np.array_equal(f.cpu().numpy(), rf)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), rv.view(np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_bit_exact_vs_skimage_golden(cuda, name):
    from sculptmate_amd import ops

    v, f = ops.marching_cubes(torch.from_numpy(G[name + "_vol"]).to(cuda), 0.0)
    assert f.dtype == torch.int32
    _same(v, f, G[name + "_verts"], G[name + "_faces"])


@pytest.mark.parametrize("shape,seed", [((2, 2, 2), 0), ((3, 2, 5), 1), ((17, 9, 33), 2), ((40, 41, 42), 3), ((64, 64, 64), 4)])
def test_noise_volumes_vs_oracle(cuda, shape, seed):
    """White noise hits every ambiguous Lewiner case and the centre vertex."""
    from sculptmate_amd import ops

    vol = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    rv, rf = capi.marching_cubes(vol, 0.0)
    v, f = ops.marching_cubes(torch.from_numpy(vol).to(cuda), 0.0)
    _same(v, f, rv, rf)


def test_integer_volume_with_exact_zeros_and_degenerate_saddles(cuda):
    from sculptmate_amd import ops

    vol = np.random.default_rng(7).integers(-2, 3, (20, 21, 19)).astype(np.float32)
    rv, rf = capi.marching_cubes(vol, 0.0)
    v, f = ops.marching_cubes(torch.from_numpy(vol).to(cuda), 0.0)
    _same(v, f, rv, rf)


def test_nonzero_level_and_classic_mode(cuda):
    from sculptmate_amd import ops

    vol = np.random.default_rng(8).standard_normal((15, 16, 17)).astype(np.float32)
    rv, rf = capi.marching_cubes(vol, 0.25)
    v, f = ops.marching_cubes(torch.from_numpy(vol).to(cuda), 0.25)
    _same(v, f, rv, rf)
    rv, rf = capi.marching_cubes(vol, 0.0, use_classic=True)
    v, f = ops.marching_cubes(torch.from_numpy(vol).to(cuda), 0.0, use_classic=True)
    _same(v, f, rv, rf)


def test_reference_order_output(cuda):
    """MarchingCubeHelper.forward + scale_tensor (isosurface.py:49-53, system.py:185-189)."""
    from sculptmate_amd import ops

    R = 24
    vol = G["density_vol"] if G["density_vol"].shape[0] == R else G["sphere_vol"]
    R = vol.shape[0]
    rv, rf = capi.reference_isosurface(-vol, R)
    rv = rv * np.float32(0.87 - (-0.87)) + np.float32(-0.87)
    v, f = ops.marching_cubes(torch.from_numpy(vol).to(cuda), 0.0, reference_order=True, vert_div=R - 1.0,
                              vert_mul=0.87 - (-0.87), vert_add=-0.87)
    assert f.dtype == torch.int64
    assert np.array_equal(f.cpu().numpy(), rf)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), rv.astype(np.float32).view(np.uint32))


def test_errors_like_skimage(cuda):
    from sculptmate_amd import ops

    with pytest.raises(ValueError):
        ops.marching_cubes(torch.ones(4, 4, 4, device=cuda), 0.0)
    vol = -torch.ones(3, 3, 3, device=cuda)
    vol[1, 1, 1] = 0.0
    with pytest.raises(RuntimeError):
        ops.marching_cubes(vol, 0.0)
    with pytest.raises(ops.SculptError):
        ops.marching_cubes(torch.ones(1, 4, 4, device=cuda), 0.0)


def _closed_manifold(f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    ue, cnt = np.unique(np.sort(e, 1), axis=0, return_counts=True)
    return (cnt == 2).all(), len(ue)


def test_full_size_256_properties_and_oracle(cuda):
    """BASELINE size: analytic blob field at 256^3 -- closed 2-manifold, Euler characteristic 2,
    and (the oracle finishes 256^3 in seconds) bit-exact against the oracle."""
    from sculptmate_amd import ops

    R = 256
    g = torch.linspace(-0.87, 0.87, R, device=cuda)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    dens = 25.0 * torch.exp(9.0 * (0.5 - torch.sqrt(x * x + 1.3 * y * y + 0.8 * z * z)))
    vol = (dens - 25.0).contiguous()
    v, f = ops.marching_cubes(vol, 0.0)
    fn = f.cpu().numpy()
    ok, ne = _closed_manifold(fn)
    assert ok
    assert len(v) - ne + len(fn) == 2
    rv, rf = capi.marching_cubes(vol.cpu().numpy(), 0.0)
    _same(v, f, rv, rf)
    # idempotent / deterministic
    v2, f2 = ops.marching_cubes(vol, 0.0)
    assert torch.equal(v, v2) and torch.equal(f, f2)


def test_dense_noisy_density_field_256_vs_oracle(cuda):
    """The bench-like case: a 256^3 density volume from the fused MLP kernel (random decoder, ~1.5 % of the
    voxels inside) -- a ~1 M vertex mesh with every Lewiner case -- bit-exact against the oracle."""
    from sculptmate_amd import ops, synth

    R = 256
    Ws, bs = synth.decoder_lists(synth.decoder_state(seed=71))
    mlp = ops.PackedMLP(Ws, bs, cuda)
    planes = torch.from_numpy(synth.triplane(seed=72, scale=2.0)).to(cuda)
    dens = ops.density_grid(planes, mlp, R)
    thr = float(dens.float().quantile(torch.tensor(0.985, device=cuda)) if dens.numel() < 2 ** 24 else
                torch.quantile(dens[:: 7].float(), 0.985))
    vol = (dens - thr).view(R, R, R).contiguous()
    v, f = ops.marching_cubes(vol, 0.0)
    assert len(v) > 200000
    rv, rf = capi.marching_cubes(vol.cpu().numpy(), 0.0)
    _same(v, f, rv, rf)


def test_nan_volume_is_reported(cuda):
    """fminf/fmaxf drop NaN, so the count pass looks for it explicitly (error 13) instead of meshing garbage."""
    import torch

    from sculptmate_amd import _lib, ops

    vol = torch.randn(12, 12, 12, device=cuda)
    vol[5, 6, 7] = float("nan")
    with pytest.raises(_lib.SculptError) as ei:
        ops.marching_cubes(vol, 0.0)
    assert ei.value.code == _lib.ERR_MC_NAN
    vol[5, 6, 7] = 0.5
    v, f = ops.marching_cubes(vol, 0.0)
    assert v.shape[0] > 0


def test_speculative_emit_equals_the_two_phase_path(cuda, monkeypatch):
    """ops.marching_cubes queues count and emit before it reads the counts back once it has seen a shape (buffers sized by the
    largest mesh so far + 25 %): the same vertices and faces as the count -> allocate -> emit path, whether the mesh fits the
    estimate, is far smaller, or does not fit (nothing written, exact path instead); the error cases keep their exceptions."""
    from sculptmate_amd import ops

    shape = (48, 50, 52)
    rng = np.random.default_rng(11)
    zz, yy, xx = np.meshgrid(*[np.linspace(-1, 1, n, dtype=np.float32) for n in shape], indexing="ij")
    small = (0.3 - np.sqrt(xx ** 2 + yy ** 2 + zz ** 2)).astype(np.float32)            # one small sphere
    medium = (0.7 - np.sqrt(xx ** 2 + yy ** 2 + zz ** 2)).astype(np.float32)
    noise = rng.standard_normal(shape).astype(np.float32)                                # far more surface than any estimate
    vols = [torch.from_numpy(v).to(cuda) for v in (medium, medium * 1.01, small, noise, noise, medium)]
    monkeypatch.setattr(ops, "_MC_SPECULATE", False)
    want = [ops.marching_cubes(v, 0.0, reference_order=True, vert_div=51.0) for v in vols]
    monkeypatch.setattr(ops, "_MC_SPECULATE", True)
    monkeypatch.setattr(ops, "_MC_CAPACITY", {})
    for i, v in enumerate(vols):
        gv, gf = ops.marching_cubes(v, 0.0, reference_order=True, vert_div=51.0)
        assert gf.dtype == torch.int64 and torch.equal(gv, want[i][0]) and torch.equal(gf, want[i][1]), i
        assert gv.is_contiguous() and gf.is_contiguous()
    (cap,) = ops._MC_CAPACITY.values()
    assert cap[0] >= want[3][0].shape[0] and cap[1] >= want[3][1].shape[0]              # grown by the overflowing call
    # error semantics on the speculative path (the shape has a capacity now)
    with pytest.raises(ValueError):
        ops.marching_cubes(torch.ones(shape, device=cuda), 0.0, reference_order=True, vert_div=51.0)
    e = -torch.ones(shape, device=cuda)
    e[1, 1, 1] = 0.0
    with pytest.raises(RuntimeError):
        ops.marching_cubes(e, 0.0, reference_order=True, vert_div=51.0)
    bad = vols[0].clone()
    bad[5, 5, 5] = float("nan")
    with pytest.raises(ops.SculptError):
        ops.marching_cubes(bad, 0.0, reference_order=True, vert_div=51.0)
    # and a good call afterwards is still right
    gv, gf = ops.marching_cubes(vols[0], 0.0, reference_order=True, vert_div=51.0)
    assert torch.equal(gv, want[0][0]) and torch.equal(gf, want[0][1])


def _planes_of(vol, level=0.0):
    """uint32 words along the last axis, bit i % 32 of word i / 32 = vol > level (bits past the row are zero), as int32 [n0*n1][words]."""
    n0, n1, n2 = vol.shape
    words = (n2 + 31) // 32
    bits = np.zeros((n0 * n1, words * 32), np.uint8)
    bits[:, :n2] = (vol.reshape(n0 * n1, n2) > np.float32(level))
    packed = np.packbits(bits.reshape(n0 * n1, words, 32), axis=-1, bitorder="little").view(np.uint32).reshape(n0 * n1, words)
    return torch.from_numpy(packed.view(np.int32))


@pytest.mark.parametrize("shape,seed", [((2, 2, 2), 0), ((17, 9, 33), 2), ((40, 41, 42), 3), ((64, 64, 64), 4), ((9, 10, 300), 5),
                                         ((12, 7, 513), 6)])
def test_count_phase_from_sign_planes_equals_the_plain_one(cuda, shape, seed, monkeypatch):
    """sculpt_mc_count_launch_signed: the cell signs come from caller-supplied planes and the volume is read only in bricks with an
    active cell -- same vertices, faces and order as the plain count phase (noise: every Lewiner case; rows longer than one
    256-cell segment; sizes that are not multiples of 32 / 64), with and without the speculative emit."""
    from sculptmate_amd import ops

    rng = np.random.default_rng(seed)
    vol = rng.standard_normal(shape).astype(np.float32)
    if min(shape) > 4:
        vol[2:4] = np.abs(vol[2:4]) + 1.0          # slabs without any sign change: bricks that never read the volume
    volt, planes = torch.from_numpy(vol).to(cuda), _planes_of(vol).to(cuda)
    for spec in (False, True, True):
        monkeypatch.setattr(ops, "_MC_SPECULATE", spec)
        v, f = ops.marching_cubes(volt, 0.0)
        sv, sf = ops.marching_cubes(volt, 0.0, sign_planes=planes)
        assert torch.equal(sv, v) and torch.equal(sf, f)
    rv, rf = capi.marching_cubes(vol, 0.0)
    _same(sv, sf, rv, rf)
    # integer values with exact zeros (value == level is "not above")
    ivol = rng.integers(-2, 3, shape).astype(np.float32)
    if (ivol > 0).any() and (ivol <= 0).any():
        it = torch.from_numpy(ivol).to(cuda)
        v, f = ops.marching_cubes(it, 0.0, reference_order=True, vert_div=3.0)
        sv, sf = ops.marching_cubes(it, 0.0, reference_order=True, vert_div=3.0, sign_planes=_planes_of(ivol).to(cuda))
        assert torch.equal(sv, v) and torch.equal(sf, f)


def test_sign_plane_count_keeps_the_error_semantics(cuda):
    from sculptmate_amd import ops

    shape = (20, 21, 70)
    ones = torch.ones(shape, device=cuda)
    with pytest.raises(ValueError):       # level below the data range: the planes say "no surface", the plain form names the error
        ops.marching_cubes(ones, 0.0, sign_planes=_planes_of(ones.cpu().numpy()).to(cuda))
    e = -torch.ones(shape, device=cuda)
    e[1, 1, 1] = 0.0
    with pytest.raises(RuntimeError):
        ops.marching_cubes(e, 0.0, sign_planes=_planes_of(e.cpu().numpy()).to(cuda))
    vol = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    bad = vol.copy()
    bad[5, 5, 5] = np.nan                 # inside the surface band of a noise volume: its brick is staged, the NaN is seen
    with pytest.raises(ops.SculptError):
        ops.marching_cubes(torch.from_numpy(bad).to(cuda), 0.0, sign_planes=_planes_of(bad).to(cuda))
    with pytest.raises(AssertionError):   # not in slab mode
        ops.marching_cubes(torch.from_numpy(vol).to(cuda), 0.0, slab=dict(axis0_offset=0), sign_planes=_planes_of(vol).to(cuda))


# ------------------------------------------------------------------------------------------------- the record pool (round 6)
def test_workspace_is_a_record_pool_and_overflow_is_reported_then_retried(cuda):
    """The workspace holds 8 bytes per ACTIVE cell in a pool of the caller's capacity.  With a pool of 1000 records a noise volume
    (every cell active) overflows: the count phase still returns the right totals, with SCULPT_ERR_MC_WORKSPACE and the number of
    active cells; a speculative emit after it writes nothing; ops.marching_cubes repeats the count with a larger workspace and
    returns the oracle's mesh."""
    import ctypes

    from sculptmate_amd import _lib, ops

    shape = (24, 25, 26)
    vol_np = np.random.default_rng(11).standard_normal(shape).astype(np.float32)
    rv, rf = capi.marching_cubes(vol_np, 0.0)
    vol = torch.from_numpy(vol_np).to(cuda)
    lib = _lib.lib
    small = lib.sculpt_mc_workspace_bytes_for(*shape, 1000)
    assert small < lib.sculpt_mc_workspace_bytes_for(*shape, 100000) and lib.sculpt_mc_workspace_bytes(*shape) == lib.sculpt_mc_workspace_bytes_for(*shape, 0)
    ws = torch.empty(small, dtype=torch.uint8, device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp, wp = ctypes.c_void_p(vol.data_ptr()), ctypes.c_void_p(ws.data_ptr())
    _lib.check(lib.sculpt_mc_count_launch_for(vp, None, 0, *shape, 0.0, 0, 1000, wp, st))
    verts = torch.full((rv.shape[0], 3), -7.0, dtype=torch.float32, device=cuda)
    faces = torch.full((rf.shape[0], 3), -7, dtype=torch.int32, device=cuda)
    _lib.check(lib.sculpt_mc_emit_capped(vp, *shape, 0.0, 0, wp, 1.0, 1.0, 0.0, 0, ctypes.c_void_p(verts.data_ptr()), rv.shape[0],
                                         ctypes.c_void_p(faces.data_ptr()), rf.shape[0], None, st))
    nv, nf, na = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    rc = lib.sculpt_mc_count_read_ex(*shape, 0.0, 0, wp, ctypes.byref(nv), ctypes.byref(nf), None, ctypes.byref(na), st)
    assert rc == _lib.ERR_MC_WORKSPACE and "record pool" in _lib.last_error()
    assert (nv.value, nf.value) == (rv.shape[0], rf.shape[0]) and 1000 < na.value <= 23 * 24 * 25
    assert bool((verts == -7.0).all()) and bool((faces == -7).all())          # the emit after an overflow wrote nothing
    # the same through a pool that holds them (a pool for every cell of the grid is never split: it cannot overflow)
    big = 23 * 24 * 25
    ws = torch.empty(lib.sculpt_mc_workspace_bytes_for(*shape, big), dtype=torch.uint8, device=cuda)
    wp = ctypes.c_void_p(ws.data_ptr())
    _lib.check(lib.sculpt_mc_count_launch_for(vp, None, 0, *shape, 0.0, 0, big, wp, st))
    _lib.check(lib.sculpt_mc_count_read_ex(*shape, 0.0, 0, wp, ctypes.byref(nv), ctypes.byref(nf), None, ctypes.byref(na), st))
    _lib.check(lib.sculpt_mc_emit(vp, *shape, 0.0, 0, wp, 1.0, 1.0, 0.0, 0, ctypes.c_void_p(verts.data_ptr()),
                                  ctypes.c_void_p(faces.data_ptr()), None, st))
    _same(verts, faces, rv, rf)
    # ops.marching_cubes: a pool that is too small for this shape, then the retry (and the capacity is remembered)
    key = (vol.device,) + shape
    ops._MC_REC_CAPACITY[key] = 500
    try:
        v, f = ops.marching_cubes(vol, 0.0)
        _same(v, f, rv, rf)
        assert ops._MC_REC_CAPACITY[key] >= na.value
        v, f = ops.marching_cubes(vol, 0.0)
        _same(v, f, rv, rf)
        # ... and in slab mode (sculpt_mc_count_read returns early there for an empty slab: the overflow must come first)
        ops._MC_REC_CAPACITY[key] = 500
        v, f, top, mm = ops.marching_cubes(vol, 0.0, slab=dict(axis0_offset=0, halo_low=False))
        _same(v, f, rv, rf)
    finally:
        ops._MC_REC_CAPACITY.pop(key, None)



# ------------------------------------------------------------------------------------------------- the record-pool protocol
# sculpt_hip.h: a count phase with more active cells than its pool is named for returns the right totals, SCULPT_ERR_MC_WORKSPACE
# and the number n of active cells; a count into sculpt_mc_workspace_bytes_for(.., n) with max_active_cells = n then succeeds --
# whatever the spread of the active cells over the pool's parts (one brick of 4 x 4 x 256 cells takes up to 4096 records at once).
def _lin(n):
    return np.linspace(-1.0, 1.0, n, dtype=np.float32)


def _sphere(n, r=0.6):
    z, y, x = np.meshgrid(_lin(n), _lin(n), _lin(n), indexing="ij")
    return (r - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


def _pool_volume(name):
    """Deterministic volumes: dense noise, sparse closed surfaces (few bricks hold all the records), ragged multi-segment rows."""
    if name.startswith("noise"):
        shape, seed = {"noise24": ((24, 25, 26), 11), "noise64": ((64, 64, 64), 4), "noise9x10x300": ((9, 10, 300), 5),
                       "noise40x3x520": ((40, 3, 520), 23), "noise66x37x700": ((66, 37, 700), 6)}[name]
        return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    if name == "sphere128":
        return _sphere(128)
    if name == "noisy_sphere128":
        return (_sphere(128) + np.float32(0.2) * np.random.default_rng(5).standard_normal((128,) * 3).astype(np.float32)).astype(np.float32)
    if name == "sphere256":
        return _sphere(256)
    if name == "cylinder":   # axis along the fastest axis: the surface crosses few bricks, each of them densely
        z, y = np.meshgrid(_lin(256), _lin(256), indexing="ij")
        return np.broadcast_to((0.6 - np.sqrt(z * z + y * y))[:, :, None], (256, 256, 64)).astype(np.float32)
    if name == "sphere9x10x300":
        z, y, x = np.meshgrid(_lin(9), _lin(10), _lin(300), indexing="ij")
        return (0.8 - np.sqrt(x * x + y * y + z * z)).astype(np.float32)
    raise KeyError(name)


class _Pool:
    """The count phase through the C ABI into a workspace named for a given number of records."""

    def __init__(self, cuda, vol_np):
        import ctypes

        from sculptmate_amd import _lib

        self.ct, self.L, self.lib = ctypes, _lib, _lib.lib
        self.cuda, self.shape = cuda, vol_np.shape
        self.vol = torch.from_numpy(np.ascontiguousarray(vol_np)).to(cuda)
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def count(self, cap, level=0.0, flags=0, planes=None):
        ct = self.ct
        ws = torch.empty(self.lib.sculpt_mc_workspace_bytes_for(*self.shape, cap), dtype=torch.uint8, device=self.cuda)
        sp, wpr = (ct.c_void_p(planes.data_ptr()), planes.stride(0)) if planes is not None else (None, 0)
        rflags = flags | (self.L.MC_SIGNED if planes is not None else 0)
        self.L.check(self.lib.sculpt_mc_count_launch_for(ct.c_void_p(self.vol.data_ptr()), sp, wpr, *self.shape, float(level), rflags,
                                                         cap, ct.c_void_p(ws.data_ptr()), self.st))
        nv, nf, na = ct.c_int64(), ct.c_int64(), ct.c_int64()
        rc = self.lib.sculpt_mc_count_read_ex(*self.shape, float(level), rflags, ct.c_void_p(ws.data_ptr()), ct.byref(nv), ct.byref(nf),
                                              None, ct.byref(na), self.st)
        return rc, (nv.value, nf.value, na.value), ws

    def emit(self, ws, counts, level=0.0, flags=0):
        ct = self.ct
        verts = torch.full((counts[0], 3), -7.0, dtype=torch.float32, device=self.cuda)
        faces = torch.full((counts[1], 3), -7, dtype=torch.int32, device=self.cuda)
        top = torch.full((2, self.shape[1], self.shape[2]), -7, dtype=torch.int32, device=self.cuda) if flags & self.L.MC_SLAB else None
        self.L.check(self.lib.sculpt_mc_emit(ct.c_void_p(self.vol.data_ptr()), *self.shape, float(level), flags, ct.c_void_p(ws.data_ptr()),
                                             1.0, 1.0, 0.0, 0, ct.c_void_p(verts.data_ptr()), ct.c_void_p(faces.data_ptr()),
                                             ct.c_void_p(top.data_ptr()) if top is not None else None, self.st))
        torch.cuda.synchronize()
        return verts, faces, top

    def protocol(self, first_cap, level=0.0, flags=0, planes=None):
        """The header's protocol: an overflowing count, then ONE count with max_active_cells = the active cells it reported, which
        must succeed with the same totals; then the emit.  Returns the totals of the first count, the mesh (and the top-plane map)."""
        rc, counts, _ = self.count(first_cap, level, flags, planes)
        assert rc == self.L.ERR_MC_WORKSPACE, (rc, counts, first_cap)
        assert "record pool" in self.L.last_error()
        n_active = counts[2]
        assert n_active > first_cap > 0 or first_cap == 0
        rc, again, ws = self.count(n_active, level, flags, planes)
        assert rc == 0, (rc, self.L.last_error(), n_active)
        assert again == counts, (again, counts)
        return counts, self.emit(ws, counts, level, flags)


POOL_VOLUMES = ["noise24", "noise64", "sphere128", "noisy_sphere128", "cylinder", "sphere256", "noise9x10x300", "noise40x3x520",
                "noise66x37x700", "sphere9x10x300"]


@pytest.mark.parametrize("name", POOL_VOLUMES)
def test_pool_protocol_of_the_header_through_the_c_abi(cuda, name):
    """Count with a small pool (SCULPT_ERR_MC_WORKSPACE, the oracle's totals, the active cells), count again into a workspace for
    exactly that many active cells (must succeed: the parts of the pool are loaded unevenly, so equal parts alone do not hold them),
    emit: the oracle's mesh bit for bit."""
    vol = _pool_volume(name)
    rv, rf = capi.marching_cubes(vol, 0.0)
    P = _Pool(cuda, vol)
    (nv, nf, na), (v, f, _) = P.protocol(256)
    assert (nv, nf) == (rv.shape[0], rf.shape[0])
    assert na <= np.prod(np.array(vol.shape) - 1)
    _same(v, f, rv, rf)


FORM_VOLUMES = ["noise24", "sphere128", "cylinder", "noise66x37x700"]


@pytest.mark.parametrize("name", FORM_VOLUMES)
@pytest.mark.parametrize("form", ["level", "classic", "sign_planes", "slab_halo_low"])
def test_pool_protocol_in_every_count_form(cuda, name, form):
    """The same protocol in every form of the count phase that fills the pool: a nonzero level and the classic tables against the
    oracle, the sign-plane count against the oracle (SCULPT_MC_SIGNED on the read), the slab flags against the same count into a
    pool for every cell of the grid (one part: it cannot overflow) -- vertices, faces and the top-plane map."""
    vol = _pool_volume(name)
    P = _Pool(cuda, vol)
    if form == "level":
        level = 0.1
        rv, rf = capi.marching_cubes(vol, level)
        (nv, nf, _), (v, f, _) = P.protocol(256, level=level)
    elif form == "classic":
        rv, rf = capi.marching_cubes(vol, 0.0, use_classic=True)
        flags = P.L.MC_USE_CLASSIC
        (nv, nf, _), (v, f, _) = P.protocol(256, flags=flags)
    elif form == "sign_planes":
        rv, rf = capi.marching_cubes(vol, 0.0)
        (nv, nf, _), (v, f, _) = P.protocol(256, planes=_planes_of(vol).to(cuda))
    else:
        flags = P.L.MC_SLAB | P.L.MC_SLAB_HALO_LOW
        ncells = int(np.prod(np.array(vol.shape) - 1))
        rc, want_counts, ws = P.count(ncells, flags=flags)
        assert rc == 0, P.L.last_error()
        wv, wf, wtop = P.emit(ws, want_counts, flags=flags)
        counts, (v, f, top) = P.protocol(256, flags=flags)
        assert counts == want_counts
        assert torch.equal(v, wv) and torch.equal(f, wf) and torch.equal(top, wtop)
        if name.startswith("noise"):          # a surface through plane 0: faces reference the previous slab's vertices
            assert bool((f < 0).any())
        return
    assert (nv, nf) == (rv.shape[0], rf.shape[0])
    _same(v, f, rv, rf)


def test_dense_field_overflows_the_default_pool_then_one_retry(cuda):
    """Noise at 64^3: nearly every cell is active, more than the default pool (max(ncells / 8, 65 536) records).  A count with
    max_active_cells = 0 (the default) overflows; the first retry with the reported number succeeds with the oracle's mesh."""
    shape = (64, 64, 64)
    vol = _pool_volume("noise64")
    rv, rf = capi.marching_cubes(vol, 0.0)
    P = _Pool(cuda, vol)
    assert P.lib.sculpt_mc_workspace_bytes_for(*shape, 0) == P.lib.sculpt_mc_workspace_bytes(*shape)
    (nv, nf, na), (v, f, _) = P.protocol(0)
    ncells = 63 ** 3
    assert na > max(ncells // 8, 65536)
    assert (nv, nf) == (rv.shape[0], rf.shape[0])
    _same(v, f, rv, rf)


class _CountingLib:
    """ops.lib with the calls of sculpt_mc_count_launch_for counted."""

    def __init__(self, lib):
        self._lib, self.count_launches = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "sculpt_mc_count_launch_for":
            return fn

        def counted(*args):
            self.count_launches += 1
            return fn(*args)

        return counted


@pytest.mark.parametrize("name", ["cylinder", "noisy_sphere128"])
@pytest.mark.parametrize("slab", [False, True])
def test_ops_marching_cubes_retries_exactly_once(cuda, monkeypatch, name, slab):
    """ops.marching_cubes with a remembered capacity far too small for the shape: one overflowing count, ONE retry, the oracle's
    mesh; the capacity it remembers holds the active cells (and is no smaller than the one that overflowed), so the next call of
    the shape counts once."""
    from sculptmate_amd import ops

    vol_np = _pool_volume(name)
    rv, rf = capi.marching_cubes(vol_np, 0.0)
    vol = torch.from_numpy(vol_np).to(cuda)
    n_active = _Pool(cuda, vol_np).count(int(np.prod(np.array(vol_np.shape) - 1)))[1][2]
    proxy = _CountingLib(ops.lib)
    monkeypatch.setattr(ops, "lib", proxy)
    key = (vol.device,) + tuple(vol_np.shape)
    small = 1000
    monkeypatch.setattr(ops, "_MC_REC_CAPACITY", {key: small})
    kw = dict(slab=dict(axis0_offset=0, halo_low=False)) if slab else {}
    for launches in (2, 1):
        proxy.count_launches = 0
        out = ops.marching_cubes(vol, 0.0, **kw)
        assert proxy.count_launches == launches
        _same(out[0], out[1], rv, rf)
        assert ops._MC_REC_CAPACITY[key] >= max(n_active, small)


def test_workspace_footprint(cuda):
    """<= 100 MB at 256^3 and <= 0.8 GB at 512^3 (the dense records + lattice-edge map took 403 MB / 3.2 GB)."""
    from sculptmate_amd import _lib

    assert _lib.lib.sculpt_mc_workspace_bytes(256, 256, 256) <= 100 * 2 ** 20
    assert _lib.lib.sculpt_mc_workspace_bytes(512, 512, 512) <= 0.8 * 2 ** 30


@pytest.mark.parametrize("shape,seed", [((6, 7, 300), 21), ((5, 300, 9), 22), ((40, 3, 520), 23), ((1100, 1100, 2), 24)])
def test_vertex_ids_across_row_segments_and_on_the_low_faces(cuda, shape, seed):
    """Vertex ids come from the OWNER cell's record (a neighbour at offset {0,-1}^3, found through the row's active mask): rows
    longer than one 256-cell segment (the owner may sit in the previous segment), thin volumes where every cell lies on a low
    face (the rank walk instead of the two record bits), noise (every Lewiner case).  The last shape has 1099 x 1099 one-cell
    rows: 1,207,801 row blocks in 1180 groups, so the scan of the group totals (mc_scan2_kernel) takes a second trip."""
    from sculptmate_amd import ops

    vol = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    rv, rf = capi.marching_cubes(vol, 0.0)
    v, f = ops.marching_cubes(torch.from_numpy(vol).to(cuda), 0.0)
    _same(v, f, rv, rf)
    rv, rf = capi.marching_cubes(vol, 0.0, use_classic=True)
    v, f = ops.marching_cubes(torch.from_numpy(vol).to(cuda), 0.0, use_classic=True)
    _same(v, f, rv, rf)


@pytest.mark.parametrize("tilt", [0.0, 0.013])
def test_surfaces_lying_flat_in_a_brick(cuda, tilt):
    """A plane across the long axis fills whole rows of cells: the emit pass then takes the brick through LDS one layer of rows
    (or one row) at a time instead of all at once; same mesh as the oracle's.  (White noise at 256^3 -- every cell active -- is
    test_dense_noisy_density_field_256_vs_oracle.)"""
    from sculptmate_amd import ops

    n0, n1, n2 = 11, 37, 300
    z, y, x = np.meshgrid(np.arange(n0), np.arange(n1), np.arange(n2), indexing="ij")
    vol = (z - 4.37 + tilt * x + 0.02 * np.sin(0.9 * y) + 0.4 * np.sin(0.05 * x) * (tilt > 0)).astype(np.float32)
    rv, rf = capi.marching_cubes(vol, 0.0)
    v, f = ops.marching_cubes(torch.from_numpy(vol).to(cuda), 0.0)
    _same(v, f, rv, rf)
    # two sheets, one directly above the other: two full layers of rows in the same bricks
    vol2 = np.minimum(vol, 3.1 - vol + 4.0).astype(np.float32)
    rv, rf = capi.marching_cubes(vol2, 0.0)
    v, f = ops.marching_cubes(torch.from_numpy(vol2).to(cuda), 0.0)
    _same(v, f, rv, rf)
