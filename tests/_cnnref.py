"""Plain fp64 statements of the channel-last bf16 conv-net blocks U^2-Net is built from (include/sculpt_hip.h:
sculpt_conv3x3_bf16, sculpt_maxpool2x2_ceil, sculpt_upsample_bilinear_bf16, sculpt_add_bf16), and the error bounds their
kernels are held to.  CPU only, torch / numpy only; tests/test_cnnref.py checks this file against torch's own operators and
shows that the bounds reject a subtly wrong convolution, tests/test_gpu_u2net_layers.py holds the HIP kernels to it.

Activations are [H*W][C] (pixel-major, the channels of a pixel contiguous), as the kernels see them.

The bounds (u = 2^-24, the unit roundoff of fp32; ub = 2^-8 that of bf16: 8 significant bits, so a number just above a
power of two 2^e lies up to half a spacing 2^(e-7) from its neighbours, 2^-8 of itself -- not 2^-9, which torch's own
conversion of 1 + 2^-8 - 2^-20 already exceeds, tests/test_cnnref.py):

* convolution, fp32 output.  A product of two bf16 numbers has 16 significant bits: exact in fp32.  The kernel therefore
  differs from the exact sum y of the K_nz = 9 C products and the bias only by the fp32 additions, in whatever order the MFMA
  tree and the K loop make them; for n terms summed in any order |err| <= (n - 1) u sum|terms| to first order.  With
  S = sum|a w| + |bias|:  |out - y| <= (K_nz + 2) u S  (conv_bound_f32).  Channels past C carry zero weights: exact zeros.
* the same in the Frobenius norm: rounding errors do not line up, the relative error grows like sqrt(K), and the project holds
  this arithmetic to ||out - y|| / ||y|| < 2e-6 sqrt(K_nz) everywhere (CONV_NORM_COEF).  The elementwise bound grows with K,
  this one with sqrt(K): it is the one that notices a 64-channel K-step missing from a K = 9216 sum at few pixels.
* convolution, ReLU, bf16 output.  ReLU is 1-Lipschitz, the store rounds once to nearest even.  With r = max(y, 0) and
  e = (K_nz + 2) u S:  |out - r| <= ub (|r| + e) + e  (conv_bound_bf16).
* bilinear upsampling: upsample_bound, derived there.
"""
import torch

U = 2.0 ** -24           # unit roundoff of fp32
UB = 2.0 ** -8           # unit roundoff of bf16 (8 significant bits: half of the spacing 2^-7)
CONV_NORM_COEF = 2e-6    # ||out - y|| / ||y|| < CONV_NORM_COEF * sqrt(K_nz)
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------
# 3x3 convolution
# ---------------------------------------------------------------------------------------------------------------------
def tap_rows(img, ky, kx, dilation):
    """img [H, W, C] -> [H*W, C]: for every output pixel (y, x) the input pixel (y + (ky-1) d, x + (kx-1) d), zero outside."""
    H, W, C = img.shape
    dy, dx = (ky - 1) * dilation, (kx - 1) * dilation
    out = torch.zeros_like(img)
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = img[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out.reshape(H * W, C)


def conv3x3_ref(act, w, bias, H, W, dilation):
    """Conv2d(3x3, padding = dilation, dilation) on the bf16 operands the kernel gets, in fp64.
    act [H*W, C] bf16; w [N, 9, C_pad] bf16 with k = (ky*3 + kx)*C_pad + c and C <= C_pad (U2Net._pack's order; the weights of
    channels C.. must be zero, the kernel multiplies them with whatever follows the slice); bias [N] fp32.
    -> (y, S), both [H*W, N] fp64: y = bias + sum a w, S = |bias| + sum |a w|."""
    assert act.dtype == BF and w.dtype == BF and act.shape[0] == H * W and w.shape[1] == 9
    C = act.shape[1]
    assert C <= w.shape[2] and not bool((w[:, :, C:] != 0).any()), "weights of the padding channels must be zero"
    a = act.double().view(H, W, C)
    wd = w[:, :, :C].double()
    y = bias.double()[None, :].repeat(H * W, 1)
    S = y.abs()
    for t in range(9):
        rows = tap_rows(a, t // 3, t % 3, dilation)
        y += rows @ wd[:, t].t()
        S += rows.abs() @ wd[:, t].abs().t()
    return y, S


def conv_bound_f32(S, K_nz):
    return (K_nz + 2) * U * S


def conv_bound_bf16(y, S, K_nz):
    e = conv_bound_f32(S, K_nz)
    return UB * (y.clamp_min(0) + e) + e


def conv_norm_limit(K_nz):
    return CONV_NORM_COEF * K_nz ** 0.5


def rne_bf16_bits(x):
    """fp32 tensor -> the bf16 bit patterns (int64, 0..65535) of round-to-nearest-even by the integer rule
    (u + 0x7fff + ((u >> 16) & 1)) >> 16.  Not for NaN."""
    u = x.detach().cpu().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def bf16_bits(x):
    return x.detach().cpu().contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


# ---------------------------------------------------------------------------------------------------------------------
# max-pool, add
# ---------------------------------------------------------------------------------------------------------------------
def maxpool_ref(act, H, W):
    """nn.MaxPool2d(2, stride=2, ceil_mode=True): [H*W, C] -> [ceil(H/2)*ceil(W/2), C] fp64.  A window that hangs over the
    edge takes the maximum of the pixels it has."""
    C = act.shape[1]
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    p = torch.full((2 * Ho, 2 * Wo, C), -float("inf"), dtype=torch.float64)
    p[:H, :W] = act.double().view(H, W, C)
    return p.view(Ho, 2, Wo, 2, C).amax(dim=(1, 3)).reshape(Ho * Wo, C)


def add_ref(a, b):
    return a.double() + b.double()


# ---------------------------------------------------------------------------------------------------------------------
# bilinear upsampling
# ---------------------------------------------------------------------------------------------------------------------
def _src(out_size, in_size):
    """F.interpolate(bilinear, align_corners=False): s = max(in/out (dst + 0.5) - 0.5, 0) -> (i0, i1, l1), in fp64."""
    dst = torch.arange(out_size, dtype=torch.float64)
    s = ((in_size / out_size) * (dst + 0.5) - 0.5).clamp_min(0)
    i0 = s.floor().long().clamp_max(in_size - 1)
    i1 = (i0 + 1).clamp_max(in_size - 1)
    return i0, i1, s - i0.double()


def upsample_ref(act, h, w, H, W):
    """F.interpolate(mode="bilinear", align_corners=False) of [h*w, C] to H x W, in fp64.
    -> (ref [H*W, C], amax [H*W, C]): amax = the largest magnitude among the four source pixels of each output element."""
    C = act.shape[1]
    a = act.double().view(h, w, C)
    y0, y1, ly = _src(H, h)
    x0, x1, lx = _src(W, w)
    ly, lx = ly[:, None, None], lx[None, :, None]
    p00, p01 = a[y0][:, x0], a[y0][:, x1]
    p10, p11 = a[y1][:, x0], a[y1][:, x1]
    ref = (1 - ly) * ((1 - lx) * p00 + lx * p01) + ly * ((1 - lx) * p10 + lx * p11)
    amax = torch.stack([p00.abs(), p01.abs(), p10.abs(), p11.abs()]).amax(0)
    return ref.reshape(H * W, C), amax.reshape(H * W, C)


def upsample_coef(h, w, H, W):
    """c of upsample_bound.  The kernel evaluates, in fp32, v = hy (hx a + lx b) + ly (hx c + lx d) and stores rne_bf16(v).
    With m = max(|a|, |b|, |c|, |d|) and exact weights the four products, the two inner sums, the two outer products and the
    last sum are at most four roundings deep on every path, over terms whose magnitudes are a convex combination of the four
    values: |v - ref| <= ((1 + u)^4 - 1) m < 5 u m.  (A fused multiply-add only removes roundings.)
    Exact 2x (H = 2h, W = 2w), the only case at 320 x 320: the scale 0.5, the products 0.5 (dst + 0.5), the source coordinates
    (multiples of 1/4) and the weights 0.25 / 0.75 / 0 / 1 are all exact in fp32: c = 5.
    Otherwise the coordinate s = scale (dst + 0.5) - 0.5 carries the rounding of the scale, of the product and of the
    subtraction, each relative to a quantity <= s + 0.5 <= the source size n: |ds| <= 3 u n; l = s - floor(s) is exact and
    1 - l rounds once more (<= u).  Bilinear interpolation with clamped ends is continuous and piecewise linear in s with slope
    <= |b - a| <= 2 m, so an s that crosses an integer changes nothing in this argument: the x direction adds (6 w + 1) u m,
    the y direction (6 h + 1) u m:  c = 5 + 2 + 6 (h + w)."""
    if H == 2 * h and W == 2 * w:
        return 5.0
    return 7.0 + 6.0 * (h + w)


def upsample_bound(ref, amax, h, w, H, W):
    """|out - ref| <= ub |ref| + (1 + ub) c u amax: one rounding to bf16 of v, |v - ref| <= c u amax (upsample_coef)."""
    return UB * ref.abs() + (1 + UB) * upsample_coef(h, w, H, W) * U * amax
