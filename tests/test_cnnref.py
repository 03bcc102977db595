"""The fp64 restatements of the conv-net blocks (tests/_cnnref.py) against torch's own operators, and the evidence that the
bounds of tests/test_gpu_u2net_layers.py have teeth: a convolution that is wrong in one tap, one K-step, one dilation or one
row tail breaks the bound that a correct fp32 convolution of the same operands keeps.  No GPU."""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

import _cnnref as R

BF = torch.bfloat16


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _operands(H, W, C, C_pad, N, g):
    act = torch.randn(H * W, C, generator=g).to(BF)
    w = torch.zeros(N, 9, C_pad)
    w[:, :, :C] = torch.randn(N, 9, C, generator=g) / math.sqrt(9 * C)
    return act, w.to(BF), torch.randn(N, generator=g)


def _torch_conv(act, w, bias, H, W, d, dtype):
    """F.conv2d on the same bf16 operands, computed in `dtype` -> [H*W, N]."""
    C = act.shape[1]
    x = act.to(dtype).view(1, H, W, C).permute(0, 3, 1, 2)
    k = w[:, :, :C].to(dtype).view(-1, 3, 3, C).permute(0, 3, 1, 2)
    return F.conv2d(x, k, bias.to(dtype), padding=d, dilation=d)[0].permute(1, 2, 0).reshape(H * W, -1)


# H, W, C, C_pad, N, dilation: odd sizes, a slice narrower than its padding, dilation larger than the image, one pixel
SMALL = [(5, 7, 8, 64, 16, 1), (9, 7, 24, 64, 8, 2), (5, 4, 64, 64, 8, 4), (5, 4, 16, 64, 8, 8), (3, 2, 8, 64, 4, 8),
         (1, 1, 8, 64, 4, 1), (1, 1, 8, 64, 4, 8), (13, 9, 72, 128, 8, 2)]


@pytest.mark.parametrize("H,W,C,C_pad,N,d", SMALL)
def test_conv3x3_ref_vs_conv2d(H, W, C, C_pad, N, d):
    """y against F.conv2d in fp64 (the sums differ only in their order: 1e-13 of S), S against F.conv2d of |a|, |w|, |bias|."""
    act, w, bias = _operands(H, W, C, C_pad, N, _gen("ref", H, W, C, N, d))
    y, S = R.conv3x3_ref(act, w, bias, H, W, d)
    assert y.dtype == torch.float64 and y.shape == (H * W, N) and S.shape == y.shape
    want = _torch_conv(act, w, bias, H, W, d, torch.float64)
    wantS = _torch_conv(act.abs(), w.abs(), bias.abs(), H, W, d, torch.float64)
    assert ((y - want).abs() <= 1e-13 * S).all() and ((S - wantS).abs() <= 1e-13 * S).all()
    assert (S >= y.abs()).all()
    if d >= max(H, W):   # every tap but the centre is outside the image: a 1x1 convolution with the centre weights
        centre = act.double() @ w[:, 4, :C].double().t() + bias.double()
        assert ((y - centre).abs() <= 1e-13 * S).all()


def test_conv3x3_ref_refuses_weights_in_the_padding_channels():
    act, w, bias = _operands(3, 3, 8, 64, 4, _gen("pad"))
    w[2, 5, 9] = 1.0
    with pytest.raises(AssertionError):
        R.conv3x3_ref(act, w, bias, 3, 3, 1)


@pytest.mark.parametrize("H,W,C", [(13, 9, 24), (9, 5, 8), (3, 2, 8), (1, 1, 8), (2, 1, 8), (320 // 32, 320 // 32, 16)])
def test_maxpool_ref_vs_max_pool2d(H, W, C):
    x = torch.randn(H * W, C, generator=_gen("pool", H, W, C)).to(BF)
    x[0, 0] = -float("inf")
    x[:, 1] = -x[:, 1].abs() - 100   # an out-of-image tap read as 0 would win here
    want = F.max_pool2d(x.double().view(1, H, W, C).permute(0, 3, 1, 2), 2, stride=2, ceil_mode=True)[0]
    got = R.maxpool_ref(x, H, W)
    assert torch.equal(got, want.permute(1, 2, 0).reshape(-1, C))
    assert torch.equal(got.to(BF).double(), got)   # the maximum of bf16 values is a bf16 value


def test_add_ref_is_one_fp32_add_away():
    g = _gen("add")
    a, b = torch.randn(1000, 8, generator=g).to(BF), (torch.randn(1000, 8, generator=g) * 7).to(BF)
    s = R.add_ref(a, b)
    assert torch.equal(s, a.double() + b.double())
    assert ((a.float() + b.float()).double() - s).abs().max() <= R.U * s.abs().max()


@pytest.mark.parametrize("h,w,H,W", [(10, 10, 20, 20), (13, 9, 31, 20), (5, 4, 9, 7), (3, 2, 5, 4), (2, 1, 3, 2), (1, 1, 2, 2),
                                     (1, 1, 1, 1), (4, 4, 4, 4)])
def test_upsample_ref_vs_interpolate(h, w, H, W):
    x = torch.randn(h * w, 8, generator=_gen("up", h, w, H, W)).to(BF)
    ref, amax = R.upsample_ref(x, h, w, H, W)
    want = F.interpolate(x.double().view(1, h, w, 8).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)[0]
    assert (ref - want.permute(1, 2, 0).reshape(H * W, 8)).abs().max() <= 1e-14 * x.double().abs().max()
    assert (amax >= ref.abs() * (1 - 1e-15)).all() and amax.max() <= x.double().abs().max()
    b = R.upsample_bound(ref, amax, h, w, H, W)
    assert (b >= R.UB * ref.abs()).all() and R.upsample_coef(10, 10, 20, 20) == 5.0 and R.upsample_coef(5, 4, 9, 7) == 7 + 6 * 9


def test_rne_bf16_bits_is_torchs_conversion():
    g = _gen("rne")
    x = torch.cat([torch.randn(100000, generator=g) * 3, torch.tensor([0.0, 1.00390625, 1.01171875, 1e-40, 3.3e38, 2.0 ** -133])])
    assert torch.equal(R.rne_bf16_bits(x), R.bf16_bits(x.to(BF)))


def test_bf16_unit_roundoff_is_two_to_the_minus_eight():
    """Round-to-nearest-even to bf16 errs by up to 2^-8 of the value (just below the midpoint of 1 and 1 + 2^-7), never more."""
    x = torch.tensor([1 + 2.0 ** -8 - 2.0 ** -20, 3.0 * (1 + 2.0 ** -8 - 2.0 ** -20)], dtype=torch.float64)
    err = ((x.float().to(BF).double() - x).abs() / x)
    assert err[0] > 2.0 ** -9 and R.UB == 2.0 ** -8
    g = _gen("ub")
    v = torch.cat([torch.randn(200000, generator=g).double() * 5, x])
    assert (((v.float().to(BF).double() - v).abs()) <= R.UB * v.abs()).all()


# ---------------------------------------------------------------------------------------------------------------------
# the bounds have teeth
# ---------------------------------------------------------------------------------------------------------------------
def _violates_elementwise(out, y, S, K_nz):
    return bool(((out - y).abs() > R.conv_bound_f32(S, K_nz)).any())


def _violates_norm(out, y, K_nz):
    return float((out - y).norm() / y.norm()) >= R.conv_norm_limit(K_nz)


def _violates_bf16(out, y, S, K_nz):
    got = out.clamp_min(0).float().to(BF).double()   # what a kernel computing `out` would store after ReLU
    return bool(((got - y.clamp_min(0)).abs() > R.conv_bound_bf16(y, S, K_nz)).any())


# a K = 9 * 1024 layer (stage5d's first convolution: 20 x 20, M % 128 = 16) and a K = 9 * 64 layer (10 x 10, M % 128 = 100)
@pytest.mark.parametrize("H,W,C,N,d", [(20, 20, 1024, 128, 2), (10, 10, 64, 128, 2)])
def test_conv_bounds_reject_a_subtly_wrong_convolution(H, W, C, N, d):
    """The correct result, evaluated in fp32 by F.conv2d, satisfies the elementwise bounds (fp32 and ReLU + bf16 form) and the
    norm condition; each mutation of the reference's own computation breaks the elementwise bounds at the elements it touches,
    in both forms, and leaves every other element inside them.
    (a) one tap of one border pixel read from inside the image instead of zero;  (b) one 64-channel K-step of one tap left out
    at one pixel;  (c) a dilation-d tap read at d - 1;  (d) the last M % 128 rows computed from the row above.
    (b) removes 64 of the K products of N sums: about sqrt(64 / K) of their size, 0.08 at K = 9216, where the elementwise bound
    is 0.03-0.04 (K u S, S ~ 0.64 sqrt(K)): it is caught elementwise at both depths, and by the norm condition too."""
    g = _gen("teeth", H, W, C, N, d)
    M, K_nz = H * W, 9 * C
    act, w, bias = _operands(H, W, C, C, N, g)
    y, S = R.conv3x3_ref(act, w, bias, H, W, d)
    good = _torch_conv(act, w, bias, H, W, d, torch.float32).double()
    assert not _violates_elementwise(good, y, S, K_nz) and not _violates_norm(good, y, K_nz) and not _violates_bf16(good, y, S, K_nz)
    a, wd = act.double().view(H, W, C), w.double()

    def check(name, mut, touched, norm_too=False):
        bad = (mut - y).abs() > R.conv_bound_f32(S, K_nz)
        assert bad.any(), name
        assert not bad[~touched].any(), name                     # the mutation is as local as it claims
        assert bad[touched].float().mean() > 0.25, name          # ... and a good share of the touched elements break it
        assert _violates_bf16(mut, y, S, K_nz), name
        if norm_too:
            assert _violates_norm(mut, y, K_nz), name

    rows = torch.zeros(M, dtype=torch.bool)
    # (a) pixel (0, 3): its tap (ky, kx) = (0, 1) lies d rows above the image; read the pixel itself instead
    p = 3
    mut = y.clone()
    mut[p] += a[0, 3] @ wd[:, 1].t()
    t = rows.clone()
    t[p] = True
    check("a", mut, t)
    # (b) pixel (H-1, W-1), tap (1, 0) (inside: d columns to the left), its last 64 channels left out
    p = M - 1
    mut = y.clone()
    mut[p] -= a[H - 1, W - 1 - d, C - 64:] @ wd[:, 3, C - 64:].t()
    t = rows.clone()
    t[p] = True
    check("b", mut, t, norm_too=True)
    # (c) tap (2, 2) of every pixel read at dilation d - 1
    mut = y - R.tap_rows(a, 2, 2, d) @ wd[:, 8].t() + R.tap_rows(a, 2, 2, d - 1) @ wd[:, 8].t()
    check("c", mut, ~rows, norm_too=True)
    # (d) the rows of the last, partial 128-row tile take the result of the row above them
    tail = M % 128
    assert tail != 0
    mut = y.clone()
    mut[M - tail:] = y[(torch.arange(M - tail, M) - 1).clamp_min(0)]   # (row 0, where there is none above, keeps its own)
    t = rows.clone()
    t[M - tail:] = True
    check("d", mut, t, norm_too=True)
