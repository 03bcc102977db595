"""Marching cubes' counts reach the host through a pinned slot and an event (csrc/mc.hip: ring_launch / ring_read): the host waits
for the counts, not for the stream, so the emit queued behind the count phase may still be running when ops.marching_cubes
returns.  Every path of ops.marching_cubes against the CPU oracle, bit for bit (MI355X)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import capi
from test_gpu_mc import _planes_of, _same

pytestmark = pytest.mark.gpu

SHAPES = [(24, 20, 33), (40, 40, 40)]   # n2 no multiple of 32; more than one brick of 4 x 4 rows; a call takes milliseconds
# The default record pool holds one record per 8 cells, at least 65 536, at most one per cell (mc.hip: default_rec_capacity):
# it can overflow only on a grid of more than 8 * 65 536 = 524 288 cells.  81 * 82 * 83 = 551 286 cells, pool 68 910 records;
# white noise makes nearly every cell active.
NOISY = (82, 83, 84)


def _grid(shape):
    return np.meshgrid(*[np.linspace(-1.0, 1.0, n, dtype=np.float32) for n in shape], indexing="ij")


def _smooth(shape, r, c=(0.0, 0.0, 0.0), squash=(1.0, 1.0, 1.0)):
    """A closed smooth surface: an ellipsoid of radius r around c."""
    z, y, x = _grid(shape)
    d = np.sqrt(squash[0] * (z - c[0]) ** 2 + squash[1] * (y - c[1]) ** 2 + squash[2] * (x - c[2]) ** 2)
    return (np.float32(r) - d).astype(np.float32)


_oracle = {}


def _case(cuda, name, shape):
    """(device volume, oracle vertices, oracle faces) of a named volume; computed once, never modified."""
    key = (name, shape)
    if key not in _oracle:
        if name == "noise":
            vol = np.random.default_rng(17).standard_normal(shape).astype(np.float32)
        else:
            vol = {"a": _smooth(shape, 0.62, (0.1, -0.05, 0.0), (1.0, 1.3, 0.8)), "b": _smooth(shape, 0.5, (-0.2, 0.1, 0.15)),
                   "small": _smooth(shape, 0.2), "large": _smooth(shape, 0.85, squash=(1.0, 0.9, 1.1))}[name]
        rv, rf = capi.marching_cubes(vol, 0.0)
        _oracle[key] = (torch.from_numpy(vol).to(cuda), rv, rf)
    return _oracle[key]


def _forget(cuda, shape):
    """ops.marching_cubes as on the first call of this shape: no speculative capacity, the default record pool."""
    from sculptmate_amd import ops

    for k in [k for k in ops._MC_CAPACITY if k[:4] == (cuda,) + tuple(shape)]:
        del ops._MC_CAPACITY[k]
    ops._MC_REC_CAPACITY.pop((cuda,) + tuple(shape), None)


def _capacity(cuda, shape, flags=0):
    from sculptmate_amd import ops

    return ops._MC_CAPACITY.get((cuda,) + tuple(shape) + (flags,))


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_emit_equals_speculative_emit_equals_oracle(cuda, shape):
    from sculptmate_amd import ops

    vol, rv, rf = _case(cuda, "a", shape)
    _forget(cuda, shape)
    assert _capacity(cuda, shape) is None
    v1, f1 = ops.marching_cubes(vol, 0.0)            # no capacity yet: count, read, exact emit
    cap = _capacity(cuda, shape)
    assert cap is not None and cap[0] >= rv.shape[0] and cap[1] >= rf.shape[0]
    v2, f2 = ops.marching_cubes(vol, 0.0)            # count + capped emit queued before the read
    assert v2._base is not None and v2._base.shape[0] == cap[0]   # (a view of the capacity-sized buffer: the speculative path)
    assert torch.equal(v1.view(torch.int32), v2.view(torch.int32)) and torch.equal(f1, f2)
    _same(v1, f1, rv, rf)
    _same(v2, f2, rv, rf)


@pytest.mark.parametrize("shape", SHAPES)
def test_speculative_miss_falls_back_to_the_exact_emit(cuda, shape):
    from sculptmate_amd import ops

    small, sv, sf = _case(cuda, "small", shape)
    large, lv, lf = _case(cuda, "large", shape)
    _forget(cuda, shape)
    v, f = ops.marching_cubes(small, 0.0)
    _same(v, f, sv, sf)
    cap = _capacity(cuda, shape)
    assert lv.shape[0] >= 2 * sv.shape[0] and lv.shape[0] > cap[0]    # the capped emit cannot hold it: it writes nothing
    v, f = ops.marching_cubes(large, 0.0)
    assert v._base is None                                              # exactly sized buffers: the fallback
    _same(v, f, lv, lf)
    v, f = ops.marching_cubes(small, 0.0)                               # and the small one again, now under a large capacity
    _same(v, f, sv, sf)


@pytest.mark.parametrize("shape", SHAPES)
def test_back_to_back_calls_keep_their_own_counts_and_outputs(cuda, shape):
    """Call 2 is queued while call 1's emit may still be running: call 1's views stay call 1's mesh, call 2's counts are its own."""
    from sculptmate_amd import ops

    a, av, af = _case(cuda, "a", shape)
    b, bv, bf = _case(cuda, "b", shape)
    assert av.shape != bv.shape
    ops.marching_cubes(a, 0.0), ops.marching_cubes(b, 0.0)             # capacities for both: the speculative path below
    torch.cuda.synchronize()
    v1, f1 = ops.marching_cubes(a, 0.0)
    v2, f2 = ops.marching_cubes(b, 0.0)
    assert (v1.shape[0], f1.shape[0]) == (av.shape[0], af.shape[0]) and (v2.shape[0], f2.shape[0]) == (bv.shape[0], bf.shape[0])
    _same(v1, f1, av, af)
    _same(v2, f2, bv, bf)


def test_two_shapes_alternating_over_eight_calls(cuda):
    from sculptmate_amd import ops

    cases = [_case(cuda, "a", SHAPES[0]), _case(cuda, "b", SHAPES[1])]
    for vol, _, _ in cases:
        ops.marching_cubes(vol, 0.0)
    got = [ops.marching_cubes(cases[i % 2][0], 0.0) for i in range(8)]   # nothing is read or synchronised in between
    for i, (v, f) in enumerate(got):
        _same(v, f, cases[i % 2][1], cases[i % 2][2])


@pytest.mark.parametrize("shape", SHAPES)
def test_on_a_non_default_stream(cuda, shape):
    from sculptmate_amd import ops

    a, av, af = _case(cuda, "a", shape)
    b, bv, bf = _case(cuda, "b", shape)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))      # the volumes and the shared workspace were last used there
    with torch.cuda.stream(s):
        _forget(cuda, shape)
        r = [ops.marching_cubes(a, 0.0), ops.marching_cubes(a, 0.0), ops.marching_cubes(b, 0.0)]   # exact, speculative, speculative
    torch.cuda.current_stream(cuda).wait_stream(s)
    _same(*r[0], av, af)
    _same(*r[1], av, af)
    _same(*r[2], bv, bf)


def test_pool_overflow_runs_the_second_count(cuda):
    from sculptmate_amd import ops

    vol, rv, rf = _case(cuda, "noise", NOISY)
    _forget(cuda, NOISY)
    key = (cuda,) + NOISY
    try:
        v, f = ops.marching_cubes(vol, 0.0)
        cells = (NOISY[0] - 1) * (NOISY[1] - 1) * (NOISY[2] - 1)
        assert cells // 8 > 65536                                   # the default pool is smaller than the grid ...
        assert ops._MC_REC_CAPACITY.get(key, 0) > cells // 8        # ... it overflowed, and the count ran again with room
        _same(v, f, rv, rf)
        v, f = ops.marching_cubes(vol, 0.0)                         # the remembered pool, the speculative emit
        _same(v, f, rv, rf)
    finally:
        ops._MC_REC_CAPACITY.pop(key, None)


def test_error_paths(cuda):
    from sculptmate_amd import _lib, ops

    shape = SHAPES[0]
    ones = torch.ones(shape, device=cuda)
    empty = -torch.ones(shape, device=cuda)
    empty[1, 1, 1] = 0.0
    for signed in (False, True):
        kw = (lambda t: dict(sign_planes=_planes_of(t.cpu().numpy()).to(cuda))) if signed else (lambda t: {})
        with pytest.raises(ValueError):       # level outside the data range
            ops.marching_cubes(ones, 0.0, **kw(ones))
        with pytest.raises(RuntimeError):     # no surface
            ops.marching_cubes(empty, 0.0, **kw(empty))
    bad = _case(cuda, "a", shape)[0].clone()
    bad[5, 5, 5] = float("nan")
    ws = torch.empty(_lib.lib.sculpt_mc_workspace_bytes(*shape), dtype=torch.uint8, device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nv, nf = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.lib.sculpt_mc_count_launch(ctypes.c_void_p(bad.data_ptr()), *shape, 0.0, 0, ctypes.c_void_p(ws.data_ptr()), st))
    rc = _lib.lib.sculpt_mc_count_read(*shape, 0.0, 0, ctypes.c_void_p(ws.data_ptr()), ctypes.byref(nv), ctypes.byref(nf), None, st)
    assert rc == _lib.ERR_MC_NAN
    with pytest.raises(ops.SculptError):
        ops.marching_cubes(bad, 0.0)
    a, av, af = _case(cuda, "a", shape)       # and a good call afterwards is still right
    _same(*ops.marching_cubes(a, 0.0), av, af)


def test_count_read_without_a_pending_launch_fails_at_once(cuda):
    from sculptmate_amd import _lib

    lib, shape = _lib.lib, SHAPES[0]
    vol, rv, rf = _case(cuda, "a", shape)
    ws = torch.empty(lib.sculpt_mc_workspace_bytes(*shape), dtype=torch.uint8, device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp, wp = ctypes.c_void_p(vol.data_ptr()), ctypes.c_void_p(ws.data_ptr())
    nv, nf, na = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    read = lambda: lib.sculpt_mc_count_read_ex(*shape, 0.0, 0, wp, ctypes.byref(nv), ctypes.byref(nf), None, ctypes.byref(na), st)
    assert read() == _lib.ERR_MC_NO_COUNT and "no count launch is pending" in _lib.last_error()   # never launched
    _lib.check(lib.sculpt_mc_count_launch(vp, *shape, 0.0, 0, wp, st))
    assert read() == 0 and (nv.value, nf.value) == (rv.shape[0], rf.shape[0]) and na.value > 0
    assert read() == _lib.ERR_MC_NO_COUNT                                                          # read already
    # a second launch before the read replaces the pending one: one read, the second's counts
    other, ov, of = _case(cuda, "b", shape)
    _lib.check(lib.sculpt_mc_count_launch(vp, *shape, 0.0, 0, wp, st))
    _lib.check(lib.sculpt_mc_count_launch(ctypes.c_void_p(other.data_ptr()), *shape, 0.0, 0, wp, st))
    assert read() == 0 and (nv.value, nf.value) == (ov.shape[0], of.shape[0])
    assert read() == _lib.ERR_MC_NO_COUNT
