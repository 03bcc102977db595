"""tests/_gemmref.py shown to work before any GPU test leans on it (no GPU needed): a NumPy stand-in for the kernel -- bf16
operands, fp32 accumulation in 32-wide k-steps, the epilogues in fp32, the textbook erf -- passes check_every_element at
K = 64, 192 and 4096, and each of a list of planted defects, in ONE tile of a 12-tile launch, makes it fail."""
import math

import numpy as np
import pytest

import _gemmref as G

BM, BN = 128, 128          # the stand-in's tile: 300 x 512 outputs = 3 x 4 = 12 tiles, the last row of tiles ragged (44 rows)
M, N = 300, 512
LOW_VAR = slice(261, 300, 3)   # rows of the ragged last tile with variance ~1e-4 and |mean| ~ 3 sigma (eps = 1e-5: a 5 % effect)


def _bf16(x):
    """fp32 values rounded to bf16, as fp32."""
    return (G.bf16_rne_bits(x).astype(np.uint32) << 16).view(np.float32)


def _operands(K, epilogue, seed, ln=False, offset=0.0):
    rng = np.random.default_rng(seed)
    rows = 2 * N if epilogue == G.EPI_GEGLU else N
    h = rng.standard_normal((M, K)).astype(np.float32)
    if ln:
        h += 3.0 * rng.standard_normal((M, 1)).astype(np.float32)          # |mean| ~ 3 sigma
        n_low = len(range(M)[LOW_VAR])
        h[LOW_VAR] = (0.03 * np.sign(rng.standard_normal((n_low, 1))) + 0.01 * rng.standard_normal((n_low, K))).astype(np.float32)
    h += np.float32(offset)
    A = _bf16(h)
    W = _bf16((rng.standard_normal((rows, K)) / math.sqrt(K)).astype(np.float32))
    bias = rng.standard_normal(rows).astype(np.float32)
    res = (rng.standard_normal((M, N)) + offset).astype(np.float32)
    fold = None
    if ln:
        st, _, _ = G.slice_stats64(h)
        fold = {"stats": st.astype(np.float32), "colsum": W.astype(np.float64).sum(1).astype(np.float32), "eps": 1e-5}
    return A, W, bias, res, fold


def standin(A, W, bias, residual, epilogue, ln, outputs, n_split=None, stats=False, defect=None, tile=(1, 2)):
    """The kernel's arithmetic in NumPy fp32; `outputs` is a subset of {"f32", "bf16", "t"}.  -> dict of canvases.
    defect: one of DEFECTS, planted in tile `tile` = (row tile, column tile) only."""
    f = np.float32
    K = A.shape[1]
    rows_w = W.shape[0]
    mt, nt = tile
    r0, r1 = mt * BM, min(mt * BM + BM, M)
    c0, c1 = nt * BN, nt * BN + BN
    acc = np.zeros((M, rows_w), np.float32)
    for k0 in range(0, K, 32):
        step = A[:, k0:k0 + 32] @ W[:, k0:k0 + 32].T
        if defect == "drop_kstep" and k0 == 32:
            step[r1 - 1, c0:c1] = 0          # the last valid row of the (ragged) tile loses one k-step
        acc += step
    b = np.zeros(rows_w, np.float32) if bias is None else bias
    bt = np.broadcast_to(b, acc.shape).copy()
    if defect == "bias_quad":
        bt[r0:r1, c0 + 8:c0 + 12] = b[c0 + 12:c0 + 16]      # one 4-column quad takes its neighbour's bias
    if ln is not None:
        s = ln["stats"].astype(np.float32)[:, :M]
        mean = s[..., 0].mean(0, dtype=np.float32)
        m2 = (s[..., 1] + f(64) * (s[..., 0] - mean[None]) ** 2).sum(0, dtype=np.float32)
        var = m2 * f(1.0 / (64 * s.shape[0]))
        rstd = (f(1) / np.sqrt(var + f(ln["eps"]))).astype(np.float32)
        rs = np.broadcast_to(rstd[:, None], acc.shape).copy()
        if defect == "no_eps":
            rs[r0:r1, c0:c1] = (f(1) / np.sqrt(var))[r0:r1, None]
        pre = rs * (acc - mean[:, None] * ln["colsum"][None, :]) + bt
    else:
        pre = acc + bt
    if epilogue == G.EPI_GELU:
        out = G.gelu_as32(pre)
    elif epilogue == G.EPI_GEGLU:
        out = pre[:, :N] * G.gelu_as32(pre[:, N:])
    elif epilogue == G.EPI_RELU:
        out = np.maximum(pre, f(0))
    else:
        out = pre
    if residual is not None:
        out = out + residual
    out = out.astype(np.float32)
    split = n_split is not None and 0 < n_split < N
    nq = n_split if split else N
    got = {}
    if "f32" in outputs:
        got["out_f32"] = G.canvas("f32", M, nq)
        got["out_f32"][:M, :nq] = out[:, :nq]
        if defect == "row_past_m":
            got["out_f32"][M, c0:c1] = out[M - 1, c0:c1]
    bits = G.bf16_rne_bits(out)
    if defect == "bf16_trunc":
        bits[r0:r1, c0:c1] = (out[r0:r1, c0:c1].view(np.uint32) >> 16).astype(np.uint16)
    if "bf16" in outputs:
        got["out_bf16"] = G.canvas("bf16", M, nq)
        got["out_bf16"][:M, :nq] = bits[:, :nq]
    if "t" in outputs:
        lo = n_split if split else 0
        got["out_t"] = G.canvas("bf16", N - lo, M, pad_cols=(-M) % 64 + 8)
        got["out_t"][:N - lo, :M] = bits[:, lo:].T
        if defect == "t_shifted":
            n, m = max(c0, lo) + 5 - lo, r0 + 7
            got["out_t"][n, m + 1] = got["out_t"][n, m]      # one element lands one column to the right
    if stats:
        st, _, _ = G.slice_stats64(out)
        got["stats_out"] = np.full((N // 64 + 1, M + 5, 2), np.nan, np.float32)
        got["stats_out"][:N // 64, :M] = st.astype(np.float32)
        if defect == "stats_row_above":
            got["stats_out"][c0 // 64, r0 + 9] = got["stats_out"][c0 // 64, r0 + 8]
    return got


DEFECTS = ["drop_kstep", "bias_quad", "no_eps", "bf16_trunc", "t_shifted", "row_past_m", "stats_row_above"]
# what the checker has to say about each (a regular expression for its message), with an fp32 output in the launch and without
SAYS = {"drop_kstep": r"out_f32: 128 element\(s\) over the bound", "bias_quad": r"out_f32: \d+ element\(s\) over the bound",
        "no_eps": r"out_f32: \d+ element\(s\) over the bound", "bf16_trunc": r"out_bf16: \d+ element\(s\) are not round-to-nearest-even",
        "t_shifted": r"out_t: 1 element\(s\) differ from the token-major output", "row_past_m": r"out_f32: 128 element\(s\) OUTSIDE the 300 x 512 output",
        "stats_row_above": r"stats_out\.mean: .* x bound at row 137, slice 4 \(1 over\)"}
SAYS_BF16 = r"out_(bf16|t): \d+ element\(s\) outside rne\(ref -\+ bound\)"


def _launch(K, epilogue, ln, outputs, n_split=None, stats=False, residual=False, defect=None, tile=(1, 2), offset=0.0):
    A, W, bias, res, fold = _operands(K, epilogue, 1000 + K + epilogue, ln=ln, offset=offset)
    res = res if residual else None
    got = standin(A, W, bias, res, epilogue, fold, outputs, n_split=n_split, stats=stats, defect=defect, tile=tile)
    R = _reference(K, epilogue, ln, residual, offset)
    return G.check_every_element(R, M, N, n_split=n_split, tile=(BM, BN), label="standin K=%d epi=%d %s" % (K, epilogue, defect), **got)


_REFS = {}


def _reference(K, epilogue, ln, residual, offset=0.0):
    """One fp64 reference per operand set, shared by the clean run and the planted defects, never modified."""
    key = (K, epilogue, ln, residual, offset)
    if key not in _REFS:
        A, W, bias, res, fold = _operands(K, epilogue, 1000 + K + epilogue, ln=ln, offset=offset)
        _REFS[key] = G.reference(A, W, bias, res if residual else None, epilogue, fold)
    return _REFS[key]


@pytest.mark.parametrize("K", [64, 192, 4096])
@pytest.mark.parametrize("offset", [0.0, 20.0])
def test_standin_passes_plain_and_residual(K, offset):
    """fp32 + bf16 + transposed + statistics from one launch, with and without a common offset on the rows; the blocked fp32
    evaluation stays below 1e-7 of mag... asserted at 0.05 of the bound B = 5e-6 (2.5e-7 mag)."""
    w = _launch(K, G.EPI_NONE, False, {"f32", "bf16", "t"}, stats=True, residual=True, offset=offset)
    assert w["worst"] <= 1.0
    A, W, bias, res, _ = _operands(K, G.EPI_NONE, 1000 + K, offset=offset)
    got = standin(A, W, bias, res, G.EPI_NONE, None, {"f32"})
    R = _reference(K, G.EPI_NONE, False, True, offset)
    assert (np.abs(got["out_f32"][:M, :N] - R.ref) / R.mag).max() < 2.5e-7


@pytest.mark.parametrize("K", [64, 192, 4096])
@pytest.mark.parametrize("epilogue", [G.EPI_GELU, G.EPI_GEGLU, G.EPI_RELU])
def test_standin_passes_activations(K, epilogue):
    assert _launch(K, epilogue, False, {"f32", "bf16"})["worst"] <= 1.0


@pytest.mark.parametrize("K", [64, 192, 1024])     # the fold takes at most 16 slices
@pytest.mark.parametrize("epilogue", [G.EPI_NONE, G.EPI_GELU, G.EPI_GEGLU])
def test_standin_passes_layernorm_fold(K, epilogue):
    assert _launch(K, epilogue, True, {"f32", "bf16"})["worst"] <= 1.0


@pytest.mark.parametrize("K", [64, 192, 4096])
def test_standin_passes_bf16_only_split(K):
    """No fp32 output: Q | K token-major, V^T transposed, split on and off a tile boundary."""
    for n_split in (256, 336):
        assert _launch(K, G.EPI_NONE, False, {"bf16", "t"}, n_split=n_split)["worst"] <= 1.0


def test_dropped_kstep_moves_almost_every_element():
    """One dropped 32-wide k-step is more than B mag on > 99.7 % of the elements at every K up to 4096."""
    for K in (64, 192, 4096):
        A, W, bias, _, _ = _operands(K, G.EPI_NONE, 1000 + K)
        R = _reference(K, G.EPI_NONE, False, False)
        step = A[:, 32:64].astype(np.float64) @ W[:, 32:64].astype(np.float64).T
        assert (np.abs(step) > R.bound).mean() > 0.997, K


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("K", [64, 192, 4096])
def test_planted_defect_fails_the_checker(defect, K):
    """Each defect, in one tile of twelve, must be an AssertionError of check_every_element; the same launch without it passes
    (the cases above)."""
    ln = defect == "no_eps"
    if ln and K == 4096:
        K = 1024
    tile = (2, 1) if defect in ("drop_kstep", "no_eps", "row_past_m") else (1, 2)     # the ragged last row of tiles / an inner tile
    with pytest.raises(AssertionError, match=SAYS[defect]):
        _launch(K, G.EPI_NONE, ln, {"f32", "bf16", "t"}, stats=not ln, residual=not ln, defect=defect, tile=tile)


@pytest.mark.parametrize("defect", ["bf16_trunc", "t_shifted", "drop_kstep", "bias_quad"])
def test_planted_defect_fails_without_an_fp32_output(defect):
    """The interval form of the bf16 bound (no fp32 output to compare bits with) sees them too, token-major and transposed."""
    for n_split, tile in ((256, (1, 1)), (256, (1, 3)), (336, (2, 0))):
        if defect == "t_shifted" and tile[1] * BN < n_split:
            continue
        with pytest.raises(AssertionError, match=SAYS_BF16):
            _launch(192, G.EPI_NONE, False, {"bf16", "t"}, n_split=n_split, defect=defect, tile=tile)


def test_erf_constant_is_what_the_formula_measures():
    e, x = G.measure_e_erf()
    print("E_erf measured %.4g at x = %.4g" % (e, x))
    assert 0.9 * G.E_ERF < e <= G.E_ERF


def test_a_flat_2_to_minus_9_is_not_a_bound_of_a_correct_bf16_rounding():
    """Why the bf16 bound is the interval rne(ref -+ b) and not b + 2^-9 |ref|: round-to-nearest-even of EXACT values misses
    2^-9 |x| on about a quarter of them (half an ulp is 2^-8 |x| just above a power of two), and never misses half an ulp."""
    x = np.random.default_rng(5).standard_normal(200000)
    x = x.astype(np.float32).astype(np.float64)
    err = np.abs(G.bf16_bits_to_f64(G.bf16_rne_bits(x)) - x)
    assert 0.15 < (err > 2.0 ** -9 * np.abs(x)).mean() < 0.35
    assert (err <= G.bf16_half_ulp(x)).all() and (G.bf16_half_ulp(x) <= 2.0 ** -8 * np.abs(x)).all()


def test_bf16_helpers():
    import torch

    x = torch.randn(4096, generator=torch.Generator().manual_seed(3)) * 7
    x[:4] = torch.tensor([1.00390625, 1.01171875, -0.0, 3.3895314e38])     # two ties, -0, the largest finite bf16's neighbourhood
    want = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(G.bf16_rne_bits(x.numpy()), want)
    assert np.array_equal(G.bf16_bits_to_f64(want), x.to(torch.bfloat16).double().numpy())
    k = G.bf16_order_key(want)
    v = G.bf16_bits_to_f64(want)
    o = np.argsort(v, kind="stable")
    assert (np.diff(k[o]) >= 0).all()
