"""The bookkeeping tail of the two-pass density grid (csrc/density_filter.hip): the header cleared by a launch of the call itself,
the dynamic-LDS attribute set once per kernel -- same signs, same mesh and the same statistics as before that change (MI355X).
The statistics are held against figures recorded from the commit before it, for the same seeds."""
import pytest
import torch

from test_gpu_density_filter import THR, _field, _margin, _same_mesh

pytestmark = pytest.mark.gpu

SEED = 31
SLAB = (7, 29)
FIELDS = ("n_marked", "n_refined", "n_cells", "n_audit", "n_mismatch")
# recorded at f93d0f1 (the parent of the change) with record() below: (R, coarse, slab) -> FIELDS
PARENT = {
    (40, 'fp16', False): (6146, 13795, 10604, 250, 0),
    (40, 'bf16', False): (33487, 34003, 10604, 142, 0),
    (64, 'fp16', False): (22762, 40312, 29420, 1146, 0),
    (64, 'bf16', False): (132706, 133872, 29420, 680, 0),
    (40, 'fp16', True): (3669, 7761, 5900, 134, 0),
    (40, 'bf16', True): (19901, 20121, 5900, 65, 0),
    (64, 'fp16', True): (7627, 13703, 9811, 369, 0),
    (64, 'bf16', True): (46929, 47329, 9811, 224, 0),
}

_cache = {}


def _setup(cuda, coarse):
    """(planes, mlp, margin) of the small synthetic decoder and scene code the filter tests use; once per coarse mode."""
    if coarse not in _cache:
        tri, mlp, _, _ = _field(cuda, SEED, inside=0.1)
        _cache[coarse] = (tri, mlp, _margin(tri, mlp, coarse)[0])
    return _cache[coarse]


def _filtered(cuda, R, coarse, slab):
    """One filtered call; (volume, statistics as a dict).  The statistics are cloned on the stream: the workspace is shared."""
    from sculptmate_amd import ops

    tri, mlp, margin = _setup(cuda, coarse)
    x0, x1 = SLAB if slab else (0, R)
    vol, st = ops.density_grid_filtered(tri, mlp, R, margin, out_add=-THR, coarse=coarse, x_begin=x0, x_end=x1)
    return vol, st.clone()


def record(cuda):
    """The PARENT table of whatever library is loaded (run once on the parent commit)."""
    from sculptmate_amd import ops

    out = {}
    for key in PARENT:
        s = ops.filter_stats(_filtered(cuda, *key)[1])
        out[key] = tuple(s[k] for k in FIELDS)
    return out


@pytest.mark.parametrize("coarse", ["fp16", "bf16"])
@pytest.mark.parametrize("R", [40, 64])
def test_signs_mesh_and_statistics_are_the_parents(cuda, R, coarse):
    from sculptmate_amd import ops

    tri, mlp, _ = _setup(cuda, coarse)
    full = ops.density_grid(tri, mlp, R, out_add=-THR, precision="bf16l3").clone()
    vol, st = _filtered(cuda, R, coarse, False)
    s = ops.filter_stats(st)
    assert int(((vol > 0) != (full > 0)).sum()) == 0, "a lattice point changed its side of the level"
    want = ops.marching_cubes(full.view(R, R, R), 0.0)
    assert want[0].shape[0] > 0
    assert _same_mesh(ops.marching_cubes(vol.view(R, R, R), 0.0), want)
    # ... and through the sign planes the call left behind (what TSR.extract_meshes does)
    assert _same_mesh(ops.marching_cubes(vol.view(R, R, R), 0.0, sign_planes=ops.filter_sign_planes(R, cuda)), want)
    assert s["n_points"] == R ** 3
    assert tuple(s[k] for k in FIELDS) == PARENT[(R, coarse, False)], s


@pytest.mark.parametrize("coarse", ["fp16", "bf16"])
@pytest.mark.parametrize("R", [40, 64])
def test_header_is_cleared_by_every_call(cuda, R, coarse):
    """Whole grid, a slab, the whole grid again: back to back on the same workspace, nothing read in between.  Every call's
    statistics are its own -- nothing is left over from the call before (each counter only ever grows inside a call)."""
    from sculptmate_amd import ops

    _filtered(cuda, R, coarse, False)          # (the workspace now has the whole grid's size: the three calls below share it)
    ws = ops._ws_cache[("dgf", cuda)].data_ptr()
    got = [_filtered(cuda, R, coarse, slab)[1] for slab in (False, True, False)]
    assert ops._ws_cache[("dgf", cuda)].data_ptr() == ws
    for slab, st in zip((False, True, False), got):
        s = ops.filter_stats(st)
        assert s["n_points"] == ((SLAB[1] - SLAB[0]) if slab else R) * R * R
        assert tuple(s[k] for k in FIELDS) == PARENT[(R, coarse, slab)], (slab, s)
        assert s["n_refined"] == s["n_first"] + s["n_second"] + s["n_audit"] and s["n_sign_fixed"] >= 0
