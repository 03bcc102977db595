"""The small kernels every image passes through, each against a plain restatement of its header contract (include/sculpt_hip.h).

Most of them copy, index, add or normalise: they are held to the bit, or to a bound derived from their arithmetic in the
docstring next to it (u = 2^-24, the unit roundoff of fp32).  Every test fills its output with a sentinel first and checks that
the sentinel survives outside the region the contract says is written."""
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U = 2.0 ** -24          # fp32 unit roundoff
FLT_MIN = 2.0 ** -126   # smallest normal fp32


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))   # seeded per case, the same in every process


def _bits(t):
    """Bit patterns of a tensor (NaN payloads, signed zeros and infinities compare exactly)."""
    t = t.detach().cpu().contiguous()
    return t.view({torch.float32: torch.int32, BF: torch.int16, torch.int16: torch.int16}[t.dtype])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


# ---------------------------------------------------------------------------------------------------------------------
# ViT front end: sculpt_vit_patchify, sculpt_vit_assemble
# ---------------------------------------------------------------------------------------------------------------------
def _patchify_ref(img, P, mean, std, ld):
    """(x - mean[c]) / std[c] in fp32, then the stride-P unfold: row = patch (row-major), column = c*P*P + py*P + px, columns
    3*P*P..ld-1 zero; the trailing S - (S//P)*P pixels are not read (a stride-P convolution ignores them)."""
    S = img.shape[0]
    n = S // P
    x = (img - torch.tensor(mean, dtype=torch.float32)) / torch.tensor(std, dtype=torch.float32)
    x = x[: n * P, : n * P].permute(2, 0, 1)                                         # [3][nP][nP]
    rows = x.reshape(3, n, P, n, P).permute(1, 3, 0, 2, 4).reshape(n * n, 3 * P * P)
    out = torch.zeros(n * n, ld)
    out[:, : 3 * P * P] = rows
    return out


def _norm_consts(which):
    from sculptmate_amd.sf3d.estimators import OPENAI_DATASET_MEAN, OPENAI_DATASET_STD
    from sculptmate_amd.sf3d.system import IMAGE_MEAN as D_MEAN, IMAGE_STD as D_STD
    from sculptmate_amd.tsr.spec import IMAGE_MEAN as T_MEAN, IMAGE_STD as T_STD

    return {"tsr": (T_MEAN, T_STD), "sf3d": (D_MEAN, D_STD), "clip": (OPENAI_DATASET_MEAN, OPENAI_DATASET_STD),
            "distinct": ((0.11, 0.52, 0.93), (0.17, 0.31, 0.67))}[which]


@pytest.mark.parametrize("S,P,ld,consts", [
    (512, 16, 768, "tsr"),        # TSR: 32 x 32 patches, K = 768 exactly
    (512, 14, 640, "sf3d"),       # SF3D DINOv2: 36 x 36 patches, 8 trailing pixels, K = 588 padded to patch_k = 640
    (224, 32, 3072, "clip"),      # CLIP ViT-B/32: 7 x 7 patches
    (37, 5, 80, "distinct"),      # ragged: 2 trailing pixels, 5 padding columns
    (1, 1, 4, "distinct"),        # smallest: one pixel, one padding column
])
def test_vit_patchify_vs_unfold(cuda, S, P, ld, consts):
    """Both outputs: the fp32 rows bit for bit (one IEEE subtract and one IEEE divide per element, as the reference), the bf16
    rows equal to torch's round-to-nearest-even cast of those fp32 rows.  Every channel has its own mean and std, so a channel
    mix-up shows.  The trailing pixels are NaN in the input, so reading them shows; the output starts as NaN, so an unwritten
    padding column shows; one extra row must stay NaN."""
    from sculptmate_amd import ops

    mean, std = _norm_consts(consts)
    g = _gen("patchify", S, P)
    img = torch.rand(S, S, 3, generator=g)
    n = S // P
    img[n * P:, :, :] = float("nan")
    img[:, n * P:, :] = float("nan")
    ref = _patchify_ref(img, P, mean, std, ld)
    assert torch.isfinite(ref).all()
    for dt in (torch.float32, BF):
        out = _nan((n * n + 1, ld), dt, cuda)
        ops.vit_patchify(img.to(cuda), P, mean, std, out[: n * n])
        want = ref if dt == torch.float32 else ref.to(BF)
        assert _same_bits(out[: n * n], want), (dt, float((out[: n * n].float().cpu() - want.float()).abs().nan_to_num(1e30).max()))
        assert torch.isnan(out[n * n:].float()).all(), "patchify wrote past its rows"


def test_vit_patchify_batched_row_slices(cuda):
    """TSR.image_tokens (tsr/system.py:437) patchifies B images into consecutive row slices of one buffer: each slice holds its
    own image's rows, bit for bit, and nothing past the last slice is written."""
    from sculptmate_amd import ops
    from sculptmate_amd.tsr.spec import IMAGE_MEAN, IMAGE_STD

    S, P, B = 512, 16, 3
    n2 = (S // P) ** 2
    g = _gen("patchify-batched")
    imgs = [torch.rand(S, S, 3, generator=g) for _ in range(B)]
    for dt in (BF, torch.float32):
        buf = _nan((B * n2 + 2, 3 * P * P), dt, cuda)
        for b, im in enumerate(imgs):
            ops.vit_patchify(im.to(cuda), P, IMAGE_MEAN, IMAGE_STD, buf[b * n2:(b + 1) * n2])
        for b, im in enumerate(imgs):
            want = _patchify_ref(im, P, IMAGE_MEAN, IMAGE_STD, 3 * P * P)
            assert _same_bits(buf[b * n2:(b + 1) * n2], want if dt == torch.float32 else want.to(BF)), (dt, b)
        assert torch.isnan(buf[B * n2:].float()).all()


@pytest.mark.parametrize("n_patches,hidden", [(1024, 768), (1296, 1024), (49, 768), (37, 200), (1, 1)])
def test_vit_assemble_bit_exact(cuda, n_patches, hidden):
    """tokens[0] = cls + pos[0], tokens[1+i] = patch_out[i] + pos[1+i]: one fp32 add per element, bit for bit.  Production:
    TSR (32^2 patches, 768), SF3D DINOv2 (36^2, 1024), CLIP (7^2, 768); then ragged and smallest.  The token buffer has a NaN
    tail (the batched TSR stream assembles into row slices of a taller buffer)."""
    from sculptmate_amd import ops

    g = _gen("assemble", n_patches, hidden)
    po, cls = torch.randn(n_patches, hidden, generator=g), torch.randn(hidden, generator=g)
    pos = torch.randn(n_patches + 1, hidden, generator=g)
    want = torch.cat([(cls + pos[0])[None], po + pos[1:]])
    tok = _nan((n_patches + 3, hidden), torch.float32, cuda)
    ops.vit_assemble(po.to(cuda), cls.to(cuda), pos.to(cuda), tok[: n_patches + 1])
    assert _same_bits(tok[: n_patches + 1], want)
    assert torch.isnan(tok[n_patches + 1:]).all()


# ---------------------------------------------------------------------------------------------------------------------
# statistics and norms: sculpt_row_slice_stats, sculpt_groupnorm_tokens, sculpt_transpose_add
# (sculpt_layernorm: test_gpu_transformer.py::test_layernorm)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,alloc_rows,cols,stats_ld", [(1025, 1025, 768, 1025), (1297, 1300, 1024, 1344), (50, 77, 256, 64),
                                                          (1, 2, 64, 3)])
def test_row_slice_stats_vs_fp64(cuda, rows, alloc_rows, cols, stats_ld):
    """(mean, M2) of every 64-column slice against fp64, and the bf16 copy against torch's cast.  Every row carries an offset of
    100 sigma, where a one-pass sum-of-squares form loses everything (its error ~ u 64 offset^2 ~ 0.04, against M2 ~ 64).
    Bounds: the mean is a fp32 sum of 64 terms, |err| <= 64 u mean|x| =: dm;  M2 = sum (x - mean_f)^2 = M2_exact + 64 dm^2 (the
    cross term cancels), and the squares plus the 64-term fma chain add <= 66 u M2.  `rows` < the rows of x and stats_ld > rows:
    the other rows and statistics stay untouched."""
    from sculptmate_amd import ops

    g = _gen("slice-stats", rows, cols)
    x = torch.randn(alloc_rows, cols, generator=g) + 100.0 * torch.sign(torch.randn(alloc_rows, 1, generator=g))
    stats = _nan((cols // 64, stats_ld, 2), torch.float32, cuda)
    xb = _nan((alloc_rows, cols), BF, cuda)
    ops.row_slice_stats(x.to(cuda), stats, xb, rows=rows)
    xs = x[:rows].double().view(rows, cols // 64, 64)
    m_ref = xs.mean(-1).t()                                        # [slice][row]
    m2_ref = ((xs - xs.mean(-1, keepdim=True)) ** 2).sum(-1).t()
    st = stats.cpu().double()
    dm = 64 * U * xs.abs().mean(-1).t()
    assert ((st[:, :rows, 0] - m_ref).abs() <= dm).all(), float(((st[:, :rows, 0] - m_ref).abs() / dm).max())
    tol2 = 66 * U * m2_ref + 64 * dm ** 2
    assert ((st[:, :rows, 1] - m2_ref).abs() <= tol2).all(), float(((st[:, :rows, 1] - m2_ref).abs() / tol2).max())
    assert torch.isnan(st[:, rows:]).all(), "statistics written past `rows`"
    assert _same_bits(xb[:rows], x[:rows].to(BF))
    assert torch.isnan(xb[rows:].float()).all(), "bf16 copy written past `rows`"


def _groupnorm_bound(x64, G, gamma, beta, depth):
    """|y - y_ref| per element of y = (x - mean) rstd gamma + beta with fp32 statistics from sums of depth `depth`: the mean is
    off by dm <= depth u mean|x|, which moves y by |gamma| dm / sigma; the variance (a sum of the same depth over deviations
    from the fp32 mean: + (depth + 4) u, + (dm / sigma)^2 <= 2 dm / sigma) and rsqrtf (<= 2 u) move rstd relatively, hence y by
    |gamma xhat| times that; the epilogue (x - mean) * rstd * gamma + beta rounds 4 times."""
    C, T = x64.shape
    xg = x64.view(G, -1)
    mean, var = xg.mean(1), xg.var(1, unbiased=False)
    sig = var.sqrt()
    dm = depth * U * xg.abs().mean(1)
    rel = (depth + 4) * U + 2 * dm / sig + 2 * U

    def per_c(v):
        return v.repeat_interleave(C // G)[:, None]

    xhat = (x64 - per_c(mean)) / per_c(sig)
    return (gamma.double()[:, None].abs() * (per_c(dm / sig) + xhat.abs() * (per_c(rel) + 4 * U))
            + beta.double()[:, None].abs() * 2 * U)


@pytest.mark.parametrize("C,T,G", [(1024, 3072, 32), (1024, 27648, 32), (96, 70, 3), (64, 100, 1), (1, 4, 1)])
def test_groupnorm_tokens_vs_fp64(cuda, C, T, G):
    """GroupNorm(G, C) over x [C][T] written transposed [T][C], both outputs, against fp64 F.group_norm.  Production: the TSR
    (1024 x 3*32^2) and SF3D (1024 x 3*96^2) triplane tokens, 32 groups; then a ragged T (a multiple of neither 4 nor 64: only
    the group size C/G*T has to be a multiple of 4), G = 1, and the smallest legal shape.  Bound: _groupnorm_bound at the depth
    of the statistics kernel's sums (a per-thread chain of ceil(group/4096) float4 steps, 3 adds in a step, a 6-level wave tree,
    16 partials); the bf16 output adds half a bf16 ulp, <= 2^-8 |y|."""
    from sculptmate_amd import ops

    g = _gen("groupnorm", C, T, G)
    x = torch.randn(C, T, generator=g) * 2 + 1.5 + torch.randn(C, 1, generator=g)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    x64 = x.double()
    ref = F.group_norm(x64[None], G, gamma.double(), beta.double(), 1e-6)[0]   # [C][T]
    depth = math.ceil(C // G * T / 4096) + 3 + 6 + 16
    tol = _groupnorm_bound(x64, G, gamma, beta, depth)
    xd, gd, bd = x.to(cuda), gamma.to(cuda), beta.to(cuda)
    for dt in (torch.float32, BF):
        y = _nan((T + 1, C), dt, cuda)
        st = _nan((2 * G + 1,), torch.float32, cuda)
        ops.groupnorm_tokens(xd, G, gd, bd, 1e-6, y[:T], st[: 2 * G])
        err = (y[:T].cpu().double().t() - ref).abs()
        lim = tol if dt == torch.float32 else tol + 2.0 ** -8 * ref.abs()
        assert (err <= lim).all(), (dt, float((err / lim).max()))
        assert torch.isnan(y[T:].float()).all() and torch.isnan(st[2 * G:]).all()


@pytest.mark.parametrize("T,C", [(3072, 1024), (70, 100), (1, 1)])
def test_transpose_add_bit_exact(cuda, T, C):
    """out[c][t] = x[t][c] + residual[c][t]: one fp32 add, bit for bit, at the TSR shape, at T and C that are not multiples of
    the 64 x 64 tile, and at 1 x 1; out has a NaN tail."""
    from sculptmate_amd import ops

    g = _gen("transpose-add", T, C)
    x, r = torch.randn(T, C, generator=g), torch.randn(C, T, generator=g)
    out = _nan((C * T + 5,), torch.float32, cuda)
    ops.transpose_add(x.to(cuda), r.to(cuda), out[: C * T].view(C, T))
    assert _same_bits(out[: C * T].view(C, T), x.t() + r)
    assert torch.isnan(out[C * T:]).all()


# ---------------------------------------------------------------------------------------------------------------------
# scatters: sculpt_upsample_scatter, sculpt_pixel_shuffle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,Co,ldg", [(32, 40, 160), (32, 40, 164), (5, 3, 17), (1, 1, 4)])
def test_upsample_scatter_bit_exact(cuda, S, Co, ldg):
    """ConvTranspose2d(k=2, s=2) from a given GEMM output g [3*S*S][ldg] (column co*4 + dy*2 + dx), no GEMM in between:
    planes[p][co][2h+dy][2w+dx] = g[p*S*S + h*S + w][co*4 + dy*2 + dx] + bias[co], one fp32 add, bit for bit.  Production: the
    TSR post-processor (S = 32, Co = 40) with ldg = 4*Co and wider; ragged; smallest.  Columns >= 4*Co of g are NaN, so reading
    them shows; the planes buffer has a NaN tail."""
    from sculptmate_amd import ops

    gen = _gen("scatter", S, Co, ldg)
    gm = torch.full((3 * S * S, ldg), float("nan"))
    gm[:, : 4 * Co] = torch.randn(3 * S * S, 4 * Co, generator=gen)
    bias = torch.randn(Co, generator=gen)
    want = torch.empty(3, Co, 2 * S, 2 * S)
    v = gm[:, : 4 * Co].reshape(3, S, S, Co, 2, 2)          # [p][h][w][co][dy][dx]
    for dy in range(2):
        for dx in range(2):
            want[:, :, dy::2, dx::2] = v[:, :, :, :, dy, dx].permute(0, 3, 1, 2) + bias[None, :, None, None]
    n = want.numel()
    out = _nan((n + 7,), torch.float32, cuda)
    ops.upsample_scatter(gm.to(cuda), bias.to(cuda), out[:n].view(want.shape), S, Co)
    assert _same_bits(out[:n].view(want.shape), want)
    assert torch.isnan(out[n:]).all()


@pytest.mark.parametrize("n,S,Co,r,ldg", [(3, 96, 40, 4, 640), (3, 96, 40, 4, 644), (2, 5, 3, 2, 13), (3, 7, 5, 1, 6),
                                          (1, 1, 1, 1, 1)])
def test_pixel_shuffle_bit_exact(cuda, n, S, Co, r, ldg):
    """nn.PixelShuffle(r) of g [n*S*S][ldg] (the last conv's channel-last output; column co*r*r + dy*r + dx), bit for bit.
    Production: SF3D's post-processor (3 planes of 96^2, Co = 40, r = 4) with ldg = Co*r*r and wider; ragged; r = 1; smallest.
    Columns >= Co*r*r are NaN; the planes buffer has a NaN tail."""
    from sculptmate_amd import ops

    gen = _gen("shuffle", n, S, Co, r, ldg)
    gm = torch.full((n * S * S, ldg), float("nan"))
    gm[:, : Co * r * r] = torch.randn(n * S * S, Co * r * r, generator=gen)
    chw = gm[:, : Co * r * r].reshape(n, S, S, Co * r * r).permute(0, 3, 1, 2)
    want = torch.nn.PixelShuffle(r)(chw).contiguous()
    m = want.numel()
    out = _nan((m + 3,), torch.float32, cuda)
    ops.pixel_shuffle(gm.to(cuda), out[:m].view(want.shape), n, S, Co, r)
    assert _same_bits(out[:m].view(want.shape), want)
    assert torch.isnan(out[m:]).all()


# ---------------------------------------------------------------------------------------------------------------------
# the cast and the im2col gathers: sculpt_cast_bf16, sculpt_im2col3x3, sculpt_im2col3x3_strided
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 255, 257, 1000003])
def test_cast_bf16_tail_and_specials(cuda, n):
    """fp32 -> bf16 at lengths that leave a partial block, or a single element: torch's .to(bfloat16) bits for every number
    (ties to even, denormals, infinities, the largest finite value rounding up), a NaN stays a NaN with its sign; y[n:] is
    untouched.  (Test_bf16_conversion_rounds_to_nearest_even_like_the_integer_rule covers a million bit patterns at one n.)"""
    from sculptmate_amd import ops

    g = _gen("cast", n)
    special = [0x3F808000, 0x3F818000, 0x00000001, 0x80008000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001,
               0x00018000, 0x80000000]
    u = torch.randint(0, 2 ** 32, (n,), generator=g, dtype=torch.int64)
    k = min(n, len(special))
    u[:k] = torch.tensor(special[:k], dtype=torch.int64)
    x = torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32).view(torch.float32)
    y = torch.full((n + 9,), 0x1234, dtype=torch.int16, device=cuda)
    ops.cast_bf16(x.to(cuda), y)
    got = y[:n].cpu()
    nan = torch.isnan(x)
    assert torch.equal(got[~nan], x.to(BF).view(torch.int16)[~nan])
    gn = got[nan].to(torch.int32) & 0xFFFF
    assert ((gn & 0x7FFF) > 0x7F80).all() and torch.equal(gn >> 15, (x[nan].view(torch.int32) < 0).to(torch.int32))
    assert (y[n:] == 0x1234).all()


def _im2col_ref(act, n, S, C, stride=1, pad=1, groups=1):
    """F.unfold of n separate images, or of ONE image whose channels are the `groups` maps side by side (channel g*C + c),
    reordered to k = (ky*3+kx)*channels + channel.  bf16 runs through as its bit patterns carried in fp32: exact."""
    raw = act.view(torch.int16).to(torch.float32) if act.dtype == BF else act
    if groups > 1:
        img = raw.view(groups, S, S, C).permute(0, 3, 1, 2).reshape(1, groups * C, S, S)
    else:
        img = raw.view(n, S, S, C).permute(0, 3, 1, 2)
    cols = F.unfold(img, 3, padding=pad, stride=stride)                   # [b][ch*9][L], index ch*9 + tap
    b, _, L = cols.shape
    ch = img.shape[1]
    out = cols.view(b, ch, 9, L).permute(0, 3, 2, 1).reshape(b * L, 9 * ch)
    return out.to(torch.int16).view(BF) if act.dtype == BF else out


@pytest.mark.parametrize("dt,n,S,C", [(BF, 3, 96, 64), (torch.float32, 3, 96, 64), (torch.float32, 3, 8, 1024), (BF, 2, 5, 8),
                                      (torch.float32, 4, 3, 4), (BF, 1, 1, 8), (torch.float32, 1, 1, 4)])
def test_im2col3x3_vs_unfold(cuda, dt, n, S, C):
    """3x3 / pad 1 im2col of n channel-last planes, bit for bit against F.unfold per plane: a tap across a plane's border reads
    zero, never the neighbouring plane.  SF3D post-processor planes (3 x 96^2; its full 1024 channels at a smaller S), ragged,
    and the smallest shape of each element size (one 16-byte chunk per pixel).  One extra output row must stay NaN."""
    from sculptmate_amd import ops

    g = _gen("im2col", n, S, C, dt)
    act = torch.randn(n * S * S, C, generator=g).to(dt)
    want = _im2col_ref(act, n, S, C)
    out = _nan((n * S * S + 1, 9 * C), dt, cuda)
    ops.im2col3x3(act.to(cuda), n, S, out[: n * S * S])
    assert _same_bits(out[: n * S * S], want)
    assert torch.isnan(out[n * S * S:].float()).all()


@pytest.mark.parametrize("dt,G,S,C,stride", [(BF, 3, 96, 1024, 2), (BF, 1, 47, 512, 2), (torch.float32, 2, 10, 4, 3),
                                             (BF, 2, 11, 16, 2), (BF, 1, 3, 8, 1), (torch.float32, 1, 3, 4, 2)])
def test_im2col3x3_strided_vs_unfold(cuda, dt, G, S, C, stride):
    """3x3 / padding 0 / stride s im2col over G channel-last maps treated as ONE image with G*C channels (channel g*C + c), bit
    for bit against F.unfold.  SF3D's global estimator (3 x 96^2 x 1024 -> 47^2, then 47^2 x 512 -> 23^2), strides that leave a
    remainder ((96-3) % 2, (10-3) % 3), and the smallest image (S = 3: one output pixel).  One extra row must stay NaN."""
    from sculptmate_amd import ops

    g = _gen("im2col-strided", G, S, C, stride, dt)
    act = torch.randn(G * S * S, C, generator=g).to(dt)
    want = _im2col_ref(act, 1, S, C, stride=stride, pad=0, groups=G)
    So = (S - 3) // stride + 1
    out = _nan((So * So + 1, 9 * G * C), dt, cuda)
    assert ops.im2col3x3_strided(act.to(cuda), G, S, stride, out[: So * So]) == So
    assert _same_bits(out[: So * So], want)
    assert torch.isnan(out[So * So:].float()).all()


# ---------------------------------------------------------------------------------------------------------------------
# sculpt_conv3x3_bf16 over planes (the SF3D post-processor's implicit-GEMM convolution)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S,C,N,relu,full", [(3, 96, 1024, 1024, True, False), (3, 96, 1024, 640, False, False),
                                               (3, 7, 64, 128, True, True), (1, 1, 64, 128, False, True)])
def test_conv3x3_planes_vs_fp32_conv(cuda, n, S, C, N, relu, full):
    """Conv2d(3x3, padding 1) of n planes against the same product on the same bf16 operands (in fp64, at least as exact as an
    fp32 F.conv2d), with and without ReLU.  Bounds as test_gemm_bias_residual_vs_fp32_reference derives them: the kernel differs
    from exact products of the bf16 inputs only by fp32 accumulation over K = 9C terms, relative error < 2e-6 sqrt(K); the bf16
    output adds its own rounding, < 4e-3.  The production shapes (SF3D's 3 x 96^2 planes, 1024 channels, N = 1024 with ReLU into
    bf16 / N = 640 into fp32) are checked on every pixel of every plane border plus 512 random pixels (the full product is
    261 GMAC); the small shapes on every pixel."""
    from sculptmate_amd import ops

    g = _gen("conv", n, S, C, N)
    K = 9 * C
    act = torch.randn(n * S * S, C, generator=g).to(BF)
    W2 = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF)
    bias = torch.randn(N, generator=g)
    if full:
        rows = torch.arange(n * S * S)
    else:
        yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
        border = ((yy == 0) | (yy == S - 1) | (xx == 0) | (xx == S - 1)).flatten().nonzero()[:, 0]
        rows = torch.cat([border + p * S * S for p in range(n)] + [torch.randint(0, n * S * S, (512,), generator=g)])
    # the im2col rows of the checked pixels (zero taps outside their plane), k = (ky*3+kx)*C + c as W2 is ordered
    pad = F.pad(act.float().view(n, S, S, C), (0, 0, 1, 1, 1, 1))
    p, y, x = rows // (S * S), (rows // S) % S, rows % S
    A = torch.stack([pad[p, y + ky, x + kx] for ky in range(3) for kx in range(3)], 1).reshape(len(rows), K)
    ref = A.double() @ W2.double().t() + bias.double()
    if relu:
        ref = ref.clamp_min(0)
    ad, wd, bd, rd = act.to(cuda), W2.to(cuda), bias.to(cuda), rows.to(cuda)
    if relu:
        outb = _nan((n * S * S, N), BF, cuda)
        ops.conv3x3_planes(ad, n, S, wd, bd, out_bf16=outb, relu=True)
        got = outb[rd].cpu().double()
        assert float((got - ref).norm() / ref.norm()) < 4e-3
    out = _nan((n * S * S, N), torch.float32, cuda)
    ops.conv3x3_planes(ad, n, S, wd, bd, out_f32=out, relu=relu)
    got = out[rd].cpu().double()
    rel, mx = float((got - ref).norm() / ref.norm()), float((got - ref).abs().max())
    assert rel < 2e-6 * math.sqrt(K) and mx < 1e-3, (rel, mx)


# ---------------------------------------------------------------------------------------------------------------------
# SF3D / estimator helpers: sculpt_normalize_rows3, sculpt_col_reduce_f32
# ---------------------------------------------------------------------------------------------------------------------
def test_normalize_rows3_vs_fp64(cuda):
    """F.normalize(x, dim=-1, eps=1e-7) against fp64 x / max(|x|, eps): ordinary rows, zero rows, rows below eps (divided by
    eps), rows whose squares underflow or overflow fp32 (|x| up to 3e38 per component, beyond FLT_MAX as a norm), denormals, and a
    row count that leaves a partial block.  Bound per element: the squared norm takes 3 roundings (1.5 u after the root), the
    root 0.5 u, the divide 0.5 u, eps rounded to fp32 < 0.5 u: |y - y_ref| <= 4 u |y_ref row|, plus one denormal ulp (2^-149).
    In place (the header permits it) gives the same bits."""
    from sculptmate_amd import ops

    g = _gen("normalize3")
    x = torch.randn(1000, 3, generator=g)
    x[10] = 0
    x[11] = torch.tensor([3e-8, -4e-8, 0.0])                # |x| = 5e-8 < eps
    x[12] = torch.tensor([1e-30, 0.0, -1e-30])              # squares underflow
    x[13] = torch.tensor([1e30, -1e30, 2e30])               # squares overflow
    x[14] = torch.tensor([3e19, 4e19, 0.0])                 # |x|^2 just past FLT_MAX
    x[15] = torch.tensor([3e38, 3e38, -3e38])               # |x| itself past FLT_MAX
    x[16] = torch.tensor([1e-45, 0.0, 0.0])                 # a denormal
    x[20:40] *= torch.exp2(torch.randint(-140, 127, (20, 1), generator=g).float())
    x = torch.nan_to_num(x, posinf=3e38, neginf=-3e38)
    x64 = x.double()
    ref = x64 / x64.norm(dim=1, keepdim=True).clamp_min(1e-7)
    y = ops.normalize_rows3(x.to(cuda)).cpu()
    tol = 4 * U * ref.norm(dim=1, keepdim=True) + 2.0 ** -149
    err = (y.double() - ref).abs()
    assert (err <= tol).all(), x[(err > tol).any(1)][:4]
    xi = x.to(cuda)
    ops.normalize_rows3(xi, out=xi)
    assert _same_bits(xi, y)


@pytest.mark.parametrize("rows,cols,ld", [(529, 512, 512), (224 * 224, 200, 208), (1, 70, 70), (3, 1, 4)])
def test_col_reduce_vs_amax_and_mean(cuda, rows, cols, ld):
    """out[c] = x[:rows, c].amax() / .mean() over fp32 x [*, ld].  Production: SF3D's global estimator pools 23^2 pixels of 512
    channels; then 224^2 rows, columns that are not a multiple of the 64-column block in a view with ld > cols, one row, one
    column.  The max is exact: bit for bit, and as amax for a column holding a NaN (NaN), an all -inf column (-inf) and a column
    of negative numbers.  The mean: four strided fp32 chains of rows/4 adds, three adds across them, one divide:
    |err| <= (rows/4 + 4) u mean|x| + u |mean|.  Rows past `rows` and columns past `cols` are NaN: reading them shows.  rows = 0
    is refused and writes nothing."""
    from sculptmate_amd import ops
    from sculptmate_amd._lib import SculptError

    g = _gen("col-reduce", rows, cols, ld)
    x = torch.randn(rows + 2, ld, generator=g) * 3 - 1
    x[rows:] = float("nan")
    x[:, cols:] = float("nan")
    if cols >= 3:
        x[:rows, 0] = -float("inf")
        x[rows // 2, 1] = float("nan")
        x[:rows, 2] = -x[:rows, 2].abs() - 1
    xd = x.to(cuda)[:, :cols]   # a [*, cols] view with row stride ld
    out = torch.full((cols + 5,), 12345.0, device=cuda)
    ops.col_reduce(xd, rows, out[:cols])
    got, want = out[:cols].cpu(), x[:rows, :cols].amax(0)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and _same_bits(got[~torch.isnan(want)], want[~torch.isnan(want)])
    assert (out[cols:] == 12345.0).all()
    xm = x.clone()
    if cols >= 3:
        xm[:rows, :2] = 1.0
    out.fill_(12345.0)
    ops.col_reduce(xm.to(cuda)[:, :cols], rows, out[:cols], mean=True)
    xs = xm[:rows, :cols].double()
    tol = (rows / 4 + 4) * U * xs.abs().mean(0) + U * xs.mean(0).abs()
    assert ((out[:cols].cpu().double() - xs.mean(0)).abs() <= tol).all()
    assert (out[cols:] == 12345.0).all()
    out.fill_(12345.0)
    with pytest.raises(SculptError):
        ops.col_reduce(xd, 0, out[:cols])
    assert (out == 12345.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# U^2-Net tail: sculpt_upsample_bilinear_f32, sculpt_fuse_sigmoid
# ---------------------------------------------------------------------------------------------------------------------
def _side_sizes(H, W):
    s = [(H, W)]
    for _ in range(5):
        s.append(((s[-1][0] + 1) // 2, (s[-1][1] + 1) // 2))   # MaxPool2d(2, ceil_mode=True)
    return s


@pytest.mark.parametrize("H,W", [(320, 320), (37, 53), (1, 1)])
def test_u2net_side_upsample_and_fuse_vs_fp64(cuda, H, W):
    """The six side outputs, each read from column 0 of an fp32 [h*w][128] conv output, upsampled with F.interpolate(bilinear,
    align_corners=False) to H x W, against fp64.  Sizes: U^2-Net's (320^2 and its halvings), an odd image whose halvings are
    odd or uneven, and 1 x 1.
    Bilinear bound: the source coordinate is formed in fp32 (scale h/H, a multiply, a subtract), <= 3 u h off, which moves a
    weight by as much; two directions, four products and sums: |err| <= u (12 max(h, w) + 8) max|in|.
    fuse_sigmoid on those maps: s = b + sum w_k m_k in fp32 (7 roundings of terms bounded by a = |b| + sum |w_k m_k|), expf and
    the reciprocal <= 4 u relative, sigma' = sigma (1 - sigma): |err| <= sigma (1 - sigma) (7 u a + 4 u) + 4 u sigma, plus
    FLT_MIN for results below the normal fp32 range (expf(-s) overflows for s < -88.7 and sigma becomes 0).  n = H*W does not
    fill the last block for the odd image; logits of +-30 and +-100 are planted."""
    from sculptmate_amd import ops

    g = _gen("u2net-tail", H, W)
    n = H * W
    maps = _nan((6, n + 3), torch.float32, cuda)
    for k, (h, w) in enumerate(_side_sizes(H, W)):
        side = torch.full((h * w, 128), float("nan"))
        side[:, 0] = torch.randn(h * w, generator=g) * 4
        ops.upsample_bilinear_f32(side.to(cuda), 128, h, w, maps[k], H, W)
        src = side[:, 0].double().view(1, 1, h, w)
        ref = F.interpolate(src, size=(H, W), mode="bilinear", align_corners=False).flatten()
        tol = U * (12 * max(h, w) + 8) * float(src.abs().max())
        err = float((maps[k, :n].cpu().double() - ref).abs().max())
        assert err <= tol, (k, h, w, err, tol)
        assert torch.isnan(maps[k, n:]).all()
    m = maps[:, :n].cpu()
    if n >= 4:   # plant large logits: +-30 (sigma within 1e-13 of 0 / 1) and +-100 (beyond the range of fp32 exp)
        m[:, :4] = 0
        m[0, :4] = torch.tensor([30.0, -30.0, 100.0, -100.0])
    wv = torch.tensor([1.0, 0.5, -0.25, 0.125, 0.75, -0.5])
    bias = 0.3
    out = _nan((n + 5,), torch.float32, cuda)
    ops.fuse_sigmoid(m.to(cuda), wv.to(cuda), bias, out[:n])
    b32 = float(np.float32(bias))
    terms = wv.double()[:, None] * m.double()
    s, a = b32 + terms.sum(0), abs(b32) + terms.abs().sum(0)
    sig = torch.sigmoid(s)
    tol = sig * (1 - sig) * (7 * U * a + 4 * U) + 4 * U * sig + FLT_MIN
    err = (out[:n].cpu().double() - sig).abs()
    assert (err <= tol).all(), float((err / tol).max())
    assert torch.isnan(out[n:]).all()
