"""Mesh smoothing without a GPU: the validation of the public surface (ops.smooth_rule, ops.mesh_smooth, Mesh.smooth, the
`smooth` keyword through TSR and TripoGenerator), and the numpy restatement tests/_smoothref.py on its own -- against a dense
construction of the operator, its properties on a noisy sphere, and the fp32 form against the fp64 one.
tests/test_gpu_mesh_smooth.py then holds the device to the fp32 restatement bit for bit."""
import inspect

import numpy as np
import pytest
import torch

import _smoothref as ref

BAD_RULES = [True, False, "3", "x", 0, -1, 1001, 0.5, 3.0, None, (3, 0.5, -0.4), (3, 0.5, -0.5), (3, 0, -0.5), (3, 1.5, -1.0),
             (3, 0.5, -1.5), (3, 0.5, 0.2), (3, 0.5, float("nan")), (3, float("nan"), -0.9), (0, 0.5, -0.53), (1001, 0.5, -0.53),
             (True, 0.5, -0.53), (2.0, 0.5, -0.53), (3, "0.5", -0.53), (3, 0.5, True), (3, 0.5), (3, 0.5, -0.53, 1), (), [3, 0.5, -0.53]]


@pytest.mark.parametrize("rule", BAD_RULES, ids=repr)
def test_bad_rule_is_a_value_error_before_any_device_work(rule):
    from sculptmate_amd import ops
    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import Mesh

    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)   # CPU tensors: the rule is checked first
    with pytest.raises(ValueError):
        ops.smooth_rule(rule)
    with pytest.raises(ValueError):
        ops.mesh_smooth(v, f, rule)
    with pytest.raises(ValueError):
        Mesh(v, f).smooth(rule)
    if rule is not None:
        with pytest.raises(ValueError):
            TSR(SMALL_CFG).extract_meshes([], smooth=rule)


def test_good_rules():
    from sculptmate_amd import ops

    assert ops.smooth_rule(1) == (1, 0.5, -0.53) and ops.smooth_rule(1000) == (1000, 0.5, -0.53)
    assert ops.smooth_rule(np.int64(7)) == (7, 0.5, -0.53)
    assert ops.smooth_rule((3, 0.6, -0.7)) == (3, 0.6, -0.7)
    assert ops.smooth_rule((4, 0.5, 0)) == (4, 0.5, 0.0)             # plain Laplacian
    assert ops.smooth_rule((2, 0.75, -1)) == (2, 0.75, -1.0) and ops.smooth_rule((2, 1.0, 0.0)) == (2, 1.0, 0.0)   # both ends included
    assert ops.smooth_rule((np.int32(5), np.float32(0.25), np.float64(-0.5))) == (5, 0.25, -0.5)
    with pytest.raises(ValueError):
        ops.smooth_rule((2, 0.75, -1.0000001))


def test_cpu_tensors_are_refused():
    from sculptmate_amd import ops
    from sculptmate_amd.tsr.system import Mesh

    v, f = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for rule in (1, 10, (3, 0.6, -0.7)):     # no CPU fallback
        with pytest.raises(ops.SculptError):
            ops.mesh_smooth(v, f, rule)
        with pytest.raises(ops.SculptError):
            Mesh(v, f).smooth(rule)
    with pytest.raises(ops.SculptError):
        ops.mesh_smooth(v.numpy(), f.numpy(), 3)


def test_mesh_smooth_carries_colours_and_atlas_and_drops_the_normals(monkeypatch):
    from sculptmate_amd import ops
    from sculptmate_amd.tsr.system import Mesh

    P, F = ref.grid_patch()
    monkeypatch.setattr(ops, "mesh_smooth", lambda v, f, s: ref.taubin(v, f, *ops.smooth_rule(s)))
    rng = np.random.default_rng(5)
    col, nrm = (rng.random((len(P), 3)).astype(np.float32) for _ in range(2))
    uvs, tex = rng.random((3 * len(F), 2)).astype(np.float32), rng.random((4, 4, 3)).astype(np.float32)
    got = Mesh(P, F, col, uvs=uvs, texture=tex, vertex_normals=nrm).smooth(3)
    assert np.array_equal(got.vertices, ref.taubin(P, F, 3)) and not np.array_equal(got.vertices, P)
    assert got.faces is F and got.vertex_colors is col and got.uvs is uvs and got.texture is tex
    assert got.vertex_normals is None            # stale: the vertices moved
    plain = Mesh(P, F).smooth((2, 0.5, 0))
    assert plain.vertex_colors is None and plain.uvs is None and plain.texture is None and plain.vertex_normals is None


def test_the_keyword_is_carried_with_default_none():
    from sculptmate_amd import batch
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.tsr import TSR

    for name in ("extract_meshes", "extract_mesh", "run", "run_async", "run_batched", "run_pipelined"):
        p = inspect.signature(getattr(TSR, name)).parameters
        assert "smooth" in p and p["smooth"].default is None, name
    assert "smooth" not in inspect.signature(TSR.extract_mesh_sharded).parameters
    assert "Mesh.smooth" in TSR.extract_mesh_sharded.__doc__
    assert inspect.signature(batch.run_sharded).parameters["smooth"].default is None
    assert TripoGenerator(torch.device("cpu")).smooth is None


def test_the_generator_hands_its_attribute_to_extract_mesh():
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd._facade import STATUS_OK

    seen = {}

    class Model:
        def __call__(self, images, device=None):
            return ["code"]

        def extract_mesh(self, codes, **kw):
            seen.update(kw)
            return []

    g = TripoGenerator(torch.device("cpu"))
    g.model = Model()
    g.smooth = 5
    assert g.generate_mesh(object(), "name") == STATUS_OK
    assert seen["smooth"] == 5 and seen["simplify"] is None and seen["keep_components"] is None


# ------------------------------------------------------------------------------------------------------ the restatement
def test_tables_of_the_hand_meshes():
    P, F = ref.tetrahedron()
    start, nb = ref.neighbour_table(F, 4)
    assert start.tolist() == [0, 3, 6, 9, 12] and nb.tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2]
    assert start.dtype == nb.dtype == np.int32 and not ref.fixed_flags(F, 4).any()
    P, F = ref.grid_patch()
    start, nb = ref.neighbour_table(F, 25)
    assert np.array_equal(ref.fixed_flags(F, 25).astype(bool), ref.patch_border())
    assert nb[start[12]:start[13]].tolist() == [6, 7, 11, 13, 17, 18] and nb[start[0]:start[1]].tolist() == [1, 5, 6]
    P, F = ref.double_cone(70)
    start, nb = ref.neighbour_table(F, 72)
    assert np.diff(start).tolist() == [70, 70] + [4] * 70 and nb[:70].tolist() == list(range(2, 72))
    assert not ref.fixed_flags(F, 72).any()
    P, F = ref.two_components_and_an_orphan()
    start, nb = ref.neighbour_table(F, len(P))
    assert start[ref.ORPHAN] == start[ref.ORPHAN + 1] and not ref.fixed_flags(F, len(P)).any()
    P, F = ref.three_face_edge()
    assert ref.fixed_flags(F, 7).tolist() == [1, 0, 1, 0, 0, 0, 1]
    start, nb = ref.neighbour_table(np.zeros((0, 3), np.int32), 3)
    assert start.tolist() == [0, 0, 0, 0] and len(nb) == 0


def _dense(P, F, n, lam, mu):
    """Repeated application of I + k (D^-1 A - I), built densely, the rows of fixed and unreferenced vertices masked."""
    nv = len(P)
    A = np.zeros((nv, nv))
    for a, b, c in np.asarray(F):
        for u, v in ((a, b), (b, c), (c, a)):
            A[u, v] = A[v, u] = 1.0
    deg = A.sum(1)
    move = (deg > 0) & (ref.fixed_flags(F, nv) == 0)
    L = A / np.where(deg > 0, deg, 1.0)[:, None] - np.eye(nv)
    L[~move] = 0.0
    p = np.asarray(P, np.float64)
    for _ in range(n):
        for k in ((lam,) if mu == 0 else (lam, mu)):
            p = (np.eye(nv) + k * L) @ p
    return p


@pytest.mark.parametrize("mesh", ["octahedron", "grid_patch", "three_face_edge", "two_components_and_an_orphan"])
@pytest.mark.parametrize("rule", [(10, 0.5, -0.53), (3, 0.6, -0.7), (4, 0.5, 0)], ids=repr)
def test_fp64_restatement_is_the_dense_operator(mesh, rule):
    """Both are fp64 and differ only in the order of summation: 1e-14 relative."""
    P, F = getattr(ref, mesh)()
    got, want = ref.taubin(P, F, *rule, dtype=np.float64), _dense(P, F, *rule)
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    assert not np.array_equal(got, P)


@pytest.fixture(scope="module")
def sphere():
    return ref.noisy_icosphere(4, 0.01, 0)


def test_taubin_smooths_and_keeps_the_volume_and_laplacian_shrinks(sphere):
    P, F = sphere
    assert P.shape == (2562, 3) and F.shape == (5120, 3)
    rms0, vol0 = ref.radius_rms(P), ref.signed_volume(P, F)
    T = ref.taubin(P, F, 10, dtype=np.float64)
    L = ref.taubin(P, F, 10, 0.5, 0, dtype=np.float64)
    rms, vol, lvol = ref.radius_rms(T), ref.signed_volume(T, F), ref.signed_volume(L, F)
    print("rms %.4f -> %.4f, volume %.4f -> taubin %.4f (%+.2f %%), laplacian %.4f (%+.2f %%)" % (
        rms0, rms, vol0, vol, 100 * (vol - vol0) / vol0, lvol, 100 * (lvol - vol0) / vol0))
    assert rms <= 0.5 * rms0
    assert abs(vol - vol0) / vol0 <= 0.01
    assert (lvol - vol0) / vol0 <= -0.03          # so the inflate step is really applied in the other


def test_what_stays_put_keeps_its_bits():
    for dtype in (np.float32, np.float64):
        P, F = ref.grid_patch()
        Q = ref.taubin(P, F, 10, dtype=dtype)
        border = ref.patch_border()
        assert np.array_equal(Q[border], P[border].astype(dtype)) and (Q[~border] != P[~border]).any(1).all()
        P, F = ref.two_components_and_an_orphan()
        Q = ref.taubin(P, F, 10, dtype=dtype)
        assert np.array_equal(Q[ref.ORPHAN], P[ref.ORPHAN].astype(dtype))
        assert (np.delete(Q, ref.ORPHAN, 0) != np.delete(P, ref.ORPHAN, 0)).any(1).all()
        P, F = ref.three_face_edge()
        Q = ref.taubin(P, F, 10, dtype=dtype)
        assert np.array_equal(Q[[0, 2, 6]], P[[0, 2, 6]].astype(dtype)) and (Q[[1, 3, 4, 5]] != P[[1, 3, 4, 5]]).any(1).all()
        P, F = ref.double_cone(70)                  # 70 neighbours: no feature rule, the apexes move
        Q = ref.taubin(P, F, 1, dtype=dtype)
        assert (Q[:2] != P[:2]).any(1).all()


FP32_MEASURED = 3.75e-7   # max |fp32 - fp64| measured below (3.748e-07), about 3 ulp of 1.0


def test_fp32_restatement_against_fp64(sphere):
    """A property of the algorithm, not of the device: the fp32 iteration stays within a few ulp of the fp64 one (positions
    near 1.0, ulp 1.2e-7), because each half-step is a convex-like combination that does not amplify earlier rounding.
    Measured with this restatement on the noisy icosphere, 10 iterations: 3.748e-07 (about 3 ulp).  The bound is
    4 x that, the margin for other seeds and orders."""
    P, F = sphere
    a, b = ref.taubin(P, F, 10, dtype=np.float32), ref.taubin(P, F, 10, dtype=np.float64)
    assert a.dtype == np.float32
    diff = float(np.abs(a.astype(np.float64) - b).max())
    print("fp32 against fp64 after 10 iterations: max |difference| %.3e" % diff)
    assert diff <= 4 * FP32_MEASURED
