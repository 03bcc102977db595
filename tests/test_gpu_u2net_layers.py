"""Every layer the 320 x 320 U^2-Net issues, each against the fp64 statement of its operation (tests/_cnnref.py), then every RSU
stage and the whole network against the oracle (oracle/u2net_ref.py).

The layer list is not written down here: U2Net.forward is walked with the entry points of sculptmate_amd.ops wrapped, and the
distinct argument tuples become the parametrised cases.  At collection time the walk runs on torch's "meta" device (shapes,
strides and offsets only: no memory, no kernel, no GPU); test_inventory_is_what_the_network_issues repeats it around a real
forward on the device and requires the same tuples, 118 convolutions among them.

Case ids: conv-<H>x<W>-c<C>@<offset>/<ld>-n<n_store>@<offset>/<ld> (or -f32/<stride>) -d<dilation>-bw<64|128>, bw being the
weight-tile width sculpt_conv3x3_bf16 picks on the 256 compute units of an MI355X ((N/128) ceil(M/128) < 1.5 CUs -> 64); the
tests compute the actual choice from the device and require that the network's cases reach both."""
import contextlib
import math
import time
import zlib

import numpy as np
import pytest
import torch

import _cnnref as R
from oracle import u2net_ref as O
from oracle.tsr_ref import _Q
from sculptmate_amd import synth
from sculptmate_amd.rembg import spec

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN_BF16 = 0x7FC0
WALKED = ((320, 320), (72, 56))     # the network's size, and one whose maps have odd sides (9, 5, 3 / 7): ceil mode, clamped ends


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _r(x, m):
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------------------
# the inventory: U2Net.forward with the ops wrapped
# ---------------------------------------------------------------------------------------------------------------------
def _slice(a):
    return (a.off, a.C, a.buf.shape[1])


@contextlib.contextmanager
def _recording(calls, call_through):
    """Wrap the ops U2Net calls; every call appends (kind, key) to `calls`.  call_through=False: nothing runs (meta walk)."""
    from sculptmate_amd import ops

    orig = {n: getattr(ops, n) for n in ("conv3x3_bf16", "maxpool2x2_ceil", "upsample_bilinear", "add_bf16",
                                         "upsample_bilinear_f32", "fuse_sigmoid")}

    def conv(x, W2, bias, out, n_store, dilation, relu, col=None, implicit=None):
        C_pad, N = W2.shape[1] // 9, W2.shape[0]
        o = ("bf16",) + _slice(out)[::2] + (int(n_store),) if isinstance(out, ops.Act) else ("f32", 0, out.stride(0), N)
        calls.append(("conv", (x.H, x.W) + _slice(x) + (C_pad,) + o + (N, int(dilation), bool(relu))))
        if call_through:
            orig["conv3x3_bf16"](x, W2, bias, out, n_store, dilation, relu, col, implicit)

    def pool(x, out):
        calls.append(("pool", (x.H, x.W) + _slice(x) + _slice(out)[::2]))
        if call_through:
            orig["maxpool2x2_ceil"](x, out)

    def up(x, out):
        calls.append(("up", (x.H, x.W) + _slice(x) + (out.H, out.W) + _slice(out)[::2]))
        if call_through:
            orig["upsample_bilinear"](x, out)

    def add(a, b, out):
        calls.append(("add", (a.H, a.W, a.C) + _slice(a)[::2] + _slice(b)[::2] + _slice(out)[::2]))
        if call_through:
            orig["add_bf16"](a, b, out)

    def passthrough(name):
        def f(*args):
            if call_through:
                orig[name](*args)
        return f

    new = {"conv3x3_bf16": conv, "maxpool2x2_ceil": pool, "upsample_bilinear": up, "add_bf16": add,
           "upsample_bilinear_f32": passthrough("upsample_bilinear_f32"), "fuse_sigmoid": passthrough("fuse_sigmoid")}
    for n, f in new.items():
        setattr(ops, n, f)
    try:
        yield
    finally:
        for n, f in orig.items():
            setattr(ops, n, f)


def _meta_walk():
    """{size: [(kind, key), ...]} of one forward per size in WALKED, on the meta device with all-zero parameters."""
    from sculptmate_amd.rembg.u2net import U2Net

    net = U2Net()
    net.load_state_dict({k: np.zeros(s, np.float32) for k, s in spec.param_spec().items()})
    net.device = torch.device("meta")    # U2Net.to() refuses anything but a HIP device: there is no CPU path to run
    net._prepare(net.device)
    out = {}
    for size in WALKED:
        calls = []
        with _recording(calls, call_through=False):
            net.forward(torch.empty((3,) + size, device="meta"))
        out[size] = calls
    return out


def _distinct(calls, kind):
    seen = []
    for k, key in calls:
        if k == kind and key not in seen:
            seen.append(key)
    return seen


_WALK = _meta_walk()
CONV_NET = _distinct(_WALK[(320, 320)], "conv")
POOLS = _distinct(_WALK[(320, 320)] + _WALK[(72, 56)], "pool")
UPS = _distinct(_WALK[(320, 320)] + _WALK[(72, 56)], "up")
ADDS = _distinct(_WALK[(320, 320)] + _WALK[(72, 56)], "add")

# shapes the network does not issue, on the kernel's edges.  Same tuple layout as the recorded ones:
# (H, W, off, C, ld, C_pad, "bf16", out off, out ld, n_store | "f32", 0, stride, N,   N, dilation, relu)
CONV_EXTRA = (
    # the 72 x 56 network's 9 x 7 and 5 x 4 maps: some, all and none of the dilated taps inside; a slice inside a wider row
    [(9, 7, 8, 24, 128, 64, "bf16", 16, 128, 40, 128, d, True) for d in (2, 4, 8)] +
    [(5, 4, 64, 128, 256, 128, "bf16", 0, 192, 128, 128, d, True) for d in (2, 4, 8)] +
    # one pixel; exactly one row tile, and one row more
    [(1, 1, 0, 64, 64, 64, "bf16", 0, 128, 128, 128, d, True) for d in (1, 8)] +
    [(16, 8, 0, 64, 128, 64, "bf16", 8, 136, 64, 128, 1, True), (43, 3, 0, 64, 128, 64, "bf16", 8, 136, 64, 128, 1, True),
     (43, 3, 8, 72, 136, 128, "f32", 0, 260, 256, 256, 1, False), (5, 4, 0, 8, 64, 64, "f32", 0, 132, 128, 128, 2, True)])


def _bw(key, cus=256):
    H, W, N = key[0], key[1], key[-3]
    return 64 if (N // 128) * ((H * W + 127) // 128) < cus * 3 // 2 else 128


def _conv_id(key):
    H, W, off, C, ld, _cp, kind, ooff, old, n_store, _N, d, relu = key
    o = "n%d@%d/%d" % (n_store, ooff, old) if kind == "bf16" else "f32/%d%s" % (old, "-relu" if relu else "")
    return "conv-%dx%d-c%d@%d/%d-%s-d%d-bw%d" % (H, W, C, off, ld, o, d, _bw(key))


def _explicit_subset(keys):
    """The first bf16 case of every (tile width, dilation) pair: both instantiations, every dilation."""
    first = {}
    for k in keys:
        if k[6] == "bf16":
            first.setdefault((_bw(k), k[-2]), k)
    return set(first.values())


EXPLICIT = _explicit_subset(CONV_NET)


def test_inventory_is_what_the_network_issues(cuda, net320):
    """The tuples the cases were made from at collection time are the ones a real forward on the device issues: 118 convolutions
    (112 REBNCONVs + 6 side convolutions), reaching both kernel instantiations on this device and dilations 1, 2, 4, 8; the
    ids are unique."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    for size in WALKED:
        assert net320["calls"][size] == _WALK[size]
    convs = [k for kind, k in net320["calls"][(320, 320)] if kind == "conv"]
    assert len(convs) == 118 and sum(1 for k in convs if k[6] == "f32") == 6
    assert {_bw(k, cus) for k in CONV_NET} == {64, 128} and {k[-2] for k in CONV_NET} == {1, 2, 4, 8}
    assert {(_bw(k, cus), k[-2]) for k in EXPLICIT} == {(_bw(k, cus), k[-2]) for k in CONV_NET if k[6] == "bf16"}
    ids = [_conv_id(k) for k in CONV_NET + CONV_EXTRA]
    assert len(set(ids)) == len(ids)
    print("distinct cases: conv %d (+%d extra, +2 at the switch), pool %d, upsample %d, add %d; explicit-path subset %d"
          % (len(CONV_NET), len(CONV_EXTRA), len(POOLS), len(UPS), len(ADDS), len(EXPLICIT)))


# ---------------------------------------------------------------------------------------------------------------------
# sculpt_conv3x3_bf16
# ---------------------------------------------------------------------------------------------------------------------
def _sentinel_bf16(rows, ld, dev):
    return torch.full((rows, ld), NAN_BF16, dtype=torch.int16, device=dev).view(BF)


def _untouched_bf16(buf, M, off, n):
    """Rows 0..M-1 outside columns [off, off + n) and every later row still hold the NaN pattern."""
    b = buf.view(torch.int16)
    return bool((b[:M, :off] == NAN_BF16).all() and (b[:M, off + n:] == NAN_BF16).all() and (b[M:] == NAN_BF16).all())


def _slice_input(g, M, off, C, ld, dev):
    """-> (act [M, C] bf16 on the host, buffer [M, ld] on the device with act at `off` and finite junk everywhere else)."""
    act = torch.randn(M, C, generator=g).to(BF)
    buf = (torch.randn(M, ld, generator=g) * 2 + 3).to(BF)
    buf[:, off:off + C] = act
    return act, buf.to(dev)


def _check_conv(cuda, key, explicit):
    """One sculpt_conv3x3_bf16 call shaped like `key`, on fresh random operands seeded from the key: activations N(0, 1) in a
    buffer of the recorded row stride with the slice at its offset and finite junk in every other channel (the implicit GEMM
    reads C_pad channels from the slice start and relies on zero weights past C), weights N(0, 1 / 9C) packed by U2Net._pack,
    bias N(0, 1).  Outputs start as NaN patterns with one extra row.

    Every pixel and every stored column of every case is checked (the largest reference is 102 400 x 64 sums of 576 products):
    * fp32 form (run for every case; it is the recorded call itself for the side convolutions):  |out - y| <= (K_nz + 2) u S,
      ||out - y|| / ||y|| < 2e-6 sqrt(K_nz); columns past the real output channels are exactly 0; [M, N] at the given stride is
      all that is written.
    * bf16 form with ReLU: |out - max(y, 0)| <= ub (|r| + e) + e, no NaN, nothing negative, nothing outside the slice written;
      and out == rne_bf16(max(fp32 form, 0)) bit for bit by the integer rule: the two forms of one shape always take the same
      kernel instantiation (the choice depends on M and N alone) and differ in the epilogue only.
    * `explicit`: the im2col + GEMM path on the same operands gives the same bits.  (Only for ReLU + bf16 cases: that GEMM has
      no k-split form, every tile shape accumulates a sum in the same order.  The plain fp32 GEMM may pick k-split pairs.)
    -> (largest |out - y| / ((K_nz + 2) u S) of the fp32 form, its norm ratio / limit)"""
    from sculptmate_amd import ops
    from sculptmate_amd.rembg.u2net import U2Net

    H, W, off, C, ld, C_pad, kind, ooff, old, n_store, N, d, relu = key
    M, K_nz = H * W, 9 * C
    co = n_store if kind == "bf16" else N - 56        # fp32 form: real output channels in both halves of the last 128 columns
    g = _gen("conv", key)
    act, buf = _slice_input(g, M, off, C, ld, cuda)
    w = torch.randn(co, C, 3, 3, generator=g) / math.sqrt(K_nz)
    b = torch.randn(co, generator=g)
    W2, b2, _ = U2Net._pack(w.numpy(), b.numpy(), cuda)
    assert W2.shape == (_r(co, 128), 9 * _r(C, 64)) and W2.shape[0] == N and W2.shape[1] == 9 * C_pad
    y, S = R.conv3x3_ref(act, W2.cpu().view(N, 9, C_pad)[:co], b2.cpu()[:co], H, W, d)
    x = ops.Act(buf, off, C, H, W)

    # fp32 form
    stride = old if kind == "f32" else N
    f32 = torch.full((M + 1, stride), float("nan"), device=cuda)
    ops.conv3x3_bf16(x, W2, b2, f32[:M], 0, d, relu if kind == "f32" else False)
    got = f32.cpu()
    assert torch.isnan(got[M:]).all() and torch.isnan(got[:M, N:]).all()
    assert not torch.isnan(got[:M, :N]).any() and (got[:M, co:N] == 0).all()
    pre = got[:M, :co].double()
    want = y.clamp_min(0) if (kind == "f32" and relu) else y
    err = (pre - want).abs()
    bound = R.conv_bound_f32(S, K_nz)
    ratio, nrm = float((err / bound).max()), float((pre - want).norm() / want.norm())
    print("CONV %-48s max|out-y|/((K+2)uS) = %.4f   norm ratio %.3e (limit %.3e)" % (_conv_id(key), ratio, nrm, R.conv_norm_limit(K_nz)))
    assert (err <= bound).all(), ratio
    assert nrm < R.conv_norm_limit(K_nz), nrm
    if kind == "f32":
        return ratio, nrm / R.conv_norm_limit(K_nz)

    # bf16 form with ReLU, into its slice
    assert relu
    obuf = _sentinel_bf16(M + 1, old, cuda)
    ops.conv3x3_bf16(x, W2, b2, ops.Act(obuf[:M], ooff, n_store, H, W), n_store, d, True)
    assert _untouched_bf16(obuf, M, ooff, n_store)
    outb = obuf[:M, ooff:ooff + n_store].cpu()
    out = outb.double()
    assert not torch.isnan(out).any() and (out >= 0).all()
    r = y.clamp_min(0)
    assert ((out - r).abs() <= R.conv_bound_bf16(y, S, K_nz)).all(), float(((out - r).abs() / R.conv_bound_bf16(y, S, K_nz)).max())
    assert torch.equal(R.bf16_bits(outb), R.rne_bf16_bits(got[:M, :co].clamp_min(0)))
    if explicit:
        col = torch.empty(M * 9 * C_pad, dtype=BF, device=cuda)
        obuf2 = _sentinel_bf16(M + 1, old, cuda)
        ops.conv3x3_bf16(x, W2, b2, ops.Act(obuf2[:M], ooff, n_store, H, W), n_store, d, True, col, implicit=False)
        assert torch.equal(obuf2.view(torch.int16), obuf.view(torch.int16))
    return ratio, nrm / R.conv_norm_limit(K_nz)


@pytest.mark.parametrize("key", CONV_NET, ids=_conv_id)
def test_conv_of_the_network_vs_fp64(cuda, key):
    """Each distinct convolution of the 320 x 320 forward: see _check_conv."""
    _check_conv(cuda, key, key in EXPLICIT)


@pytest.mark.parametrize("key", CONV_EXTRA, ids=_conv_id)
def test_conv_edge_shapes_vs_fp64(cuda, key):
    """Shapes the entry point accepts and the 320 x 320 network does not issue: H != W with dilation 2, 4, 8 on 9 x 7 and 5 x 4
    maps (some / all / none of the outer taps inside), a 1 x 1 map, M = 128 and 129, an fp32 output whose stride exceeds N, an
    fp32 output with ReLU.  Every bf16 case also runs the im2col + GEMM path."""
    _check_conv(cuda, key, True)


@pytest.mark.parametrize("side", ["below", "at"])
def test_conv_either_side_of_the_instantiation_switch(cuda, side):
    """N = 128 and 128-pixel-wide maps of 1.5 CUs - 1 and 1.5 CUs rows: the last shape on the 64-column form and the first on
    the 128-column form, from the device's own CU count."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    thr = cus * 3 // 2
    H = thr - 1 if side == "below" else thr
    key = (H, 128, 8, 8, 80, 64, "bf16", 8, 144, 128, 128, 1, True)
    assert _bw(key, cus) == (64 if side == "below" else 128)
    _check_conv(cuda, key, True)


# ---------------------------------------------------------------------------------------------------------------------
# sculpt_maxpool2x2_ceil, sculpt_add_bf16, sculpt_upsample_bilinear_bf16
# ---------------------------------------------------------------------------------------------------------------------
def _pool_id(k):
    H, W, off, C, ld, ooff, old = k
    return "pool-%dx%d-c%d@%d/%d-to@%d/%d" % (H, W, C, off, ld, ooff, old)


@pytest.mark.parametrize("key", POOLS, ids=_pool_id)
def test_maxpool_bit_exact(cuda, key):
    """MaxPool2d(2, 2, ceil_mode=True), every distinct call of the 320 x 320 and the 72 x 56 forward (odd sides: the last window
    hangs over the edge), bit for bit: the maximum of bf16 values is one of them.  A -inf is planted, and one channel holds
    values below -100 so that an out-of-image tap read as 0 instead of skipped would win.  No signed zeros (fmax does not order
    them).  Channels outside the output slice and one extra row keep their NaN patterns."""
    from sculptmate_amd import ops

    H, W, off, C, ld, ooff, old = key
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    g = _gen("pool", key)
    act = torch.randn(H * W, C, generator=g).to(BF)
    act[act == 0] = 1.0
    act[:, 1] = -act[:, 1].abs() - 100
    act[0, 0] = -float("inf")
    buf = (torch.randn(H * W, ld, generator=g) * 2 + 3).to(BF)
    buf[:, off:off + C] = act
    obuf = _sentinel_bf16(Ho * Wo + 1, old, cuda)
    ops.maxpool2x2_ceil(ops.Act(buf.to(cuda), off, C, H, W), ops.Act(obuf[:Ho * Wo], ooff, C, Ho, Wo))
    assert _untouched_bf16(obuf, Ho * Wo, ooff, C)
    assert torch.equal(R.bf16_bits(obuf[:Ho * Wo, ooff:ooff + C]), R.bf16_bits(R.maxpool_ref(act, H, W).to(BF)))


def _add_id(k):
    return "add-%dx%d-c%d-a@%d/%d-b@%d/%d-to@%d/%d" % k


@pytest.mark.parametrize("key", ADDS, ids=_add_id)
def test_add_bit_exact(cuda, key):
    """The RSU residual, every distinct call: one IEEE fp32 add and one round-to-nearest-even, (a.float() + b.float()).to(bf16)
    bit for bit (and within half a bf16 spacing of the fp64 sum); sentinels as above."""
    from sculptmate_amd import ops

    H, W, C, aoff, ald, boff, bld, ooff, old = key
    M = H * W
    g = _gen("add", key)
    a, abuf = _slice_input(g, M, aoff, C, ald, cuda)
    b, bbuf = _slice_input(g, M, boff, C, bld, cuda)
    b = (b.float() * 5).to(BF)
    bbuf[:, boff:boff + C] = b.to(cuda)
    obuf = _sentinel_bf16(M + 1, old, cuda)
    ops.add_bf16(ops.Act(abuf, aoff, C, H, W), ops.Act(bbuf, boff, C, H, W), ops.Act(obuf[:M], ooff, C, H, W))
    assert _untouched_bf16(obuf, M, ooff, C)
    got = obuf[:M, ooff:ooff + C].cpu()
    assert torch.equal(R.bf16_bits(got), R.bf16_bits((a.float() + b.float()).to(BF)))
    ref = R.add_ref(a, b)
    assert ((got.double() - ref).abs() <= R.UB * (1 + R.U) * ref.abs() + R.U * ref.abs()).all()


def _up_id(k):
    h, w, off, C, ld, H, W, ooff, old = k
    return "up-%dx%d-c%d@%d/%d-to-%dx%d@%d/%d" % (h, w, C, off, ld, H, W, ooff, old)


@pytest.mark.parametrize("key", UPS, ids=_up_id)
def test_upsample_vs_fp64(cuda, key):
    """F.interpolate(bilinear, align_corners=False), every distinct call of the two forwards (exact 2x at 320; 3 -> 5, 5 -> 9,
    4 -> 7 at 72 x 56, where the last source row / column is clamped), every element against fp64 within
    ub |ref| + (1 + ub) c u max(|a|, |b|, |c|, |d|), c from the kernel's expression (_cnnref.upsample_coef); sentinels as above."""
    from sculptmate_amd import ops

    h, w, off, C, ld, H, W, ooff, old = key
    g = _gen("up", key)
    act, buf = _slice_input(g, h * w, off, C, ld, cuda)
    obuf = _sentinel_bf16(H * W + 1, old, cuda)
    ops.upsample_bilinear(ops.Act(buf, off, C, h, w), ops.Act(obuf[:H * W], ooff, C, H, W))
    assert _untouched_bf16(obuf, H * W, ooff, C)
    got = obuf[:H * W, ooff:ooff + C].cpu().double()
    ref, amax = R.upsample_ref(act, h, w, H, W)
    err, bound = (got - ref).abs(), R.upsample_bound(ref, amax, h, w, H, W)
    assert not torch.isnan(got).any() and (err <= bound).all(), float((err / bound).max())


# ---------------------------------------------------------------------------------------------------------------------
# the RSU stages and the network at 320 x 320 against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _blob_image(n=320):
    """A smooth foreground on a smooth background, pre-processed as rembg/session.py does: a Gaussian blob (centre (0.5, 0.55)
    of the side, widths 0.22 / 0.3) over per-channel linear gradients, divided by its maximum, ImageNet mean / std."""
    from sculptmate_amd.rembg.session import MEAN, STD

    t = (torch.arange(n, dtype=torch.float64) + 0.5) / n
    yy, xx = torch.meshgrid(t, t, indexing="ij")
    blob = torch.exp(-0.5 * (((xx - 0.5) / 0.22) ** 2 + ((yy - 0.55) / 0.3) ** 2))
    bg = torch.stack([0.15 + 0.35 * xx, 0.45 - 0.3 * yy, 0.2 + 0.2 * (xx + yy) / 2])
    fg = torch.tensor([0.9, 0.65, 0.4], dtype=torch.float64)[:, None, None]
    img = bg * (1 - blob) + fg * blob
    img = img / img.max()
    mean, std = (torch.tensor(v, dtype=torch.float64)[:, None, None] for v in (MEAN, STD))
    return ((img - mean) / std).float()


def _oracle_at_320():
    """The oracle on the CPU, once: bf16 and fp32 forwards of the blob image, and for every stage the input the bf16 forward
    gave it, its bf16 output, and the fp32 oracle's output for that same input."""
    t0 = time.perf_counter()
    sd = synth.u2net_state(0)
    x = _blob_image()
    stages = {}
    orig = O.rsu

    def rec(sd_, name, kind, xin, Q):
        out = orig(sd_, name, kind, xin, Q)
        stages[name] = {"kind": kind, "x": xin.clone(), "bf16": out.clone()}
        return out

    O.rsu = rec
    try:
        d0_bf = O.u2net_forward(sd, x[None], bf16=True)[0, 0]
    finally:
        O.rsu = orig
    d0_32 = O.u2net_forward(sd, x[None])[0, 0]
    with torch.no_grad():
        for name, s in stages.items():
            s["fp32"] = orig(sd, name, s["kind"], s["x"], _Q(False))
    assert [s[0] for s in spec.STAGES] == list(stages)
    # the yardstick must be able to tell something: the bf16 oracle's own mask is within 1 % of the fp32 oracle's
    flips = int(((d0_bf > 0.5) != (d0_32 > 0.5)).sum())
    frac = float((d0_32 > 0.5).float().mean())
    assert flips <= 0.01 * d0_32.numel() and 0.05 < frac < 0.95, (flips, frac)
    print("oracle at 320: %.1f s; d0 fp32 in [%.3f, %.3f], %.1f %% above 0.5; bf16 vs fp32: max %.2e rms %.2e, %d mask pixels"
          % (time.perf_counter() - t0, float(d0_32.min()), float(d0_32.max()), 100 * frac, float((d0_bf - d0_32).abs().max()),
             float((d0_bf - d0_32).pow(2).mean().sqrt()), flips))
    return {"sd": sd, "x": x, "stages": stages, "d0_bf": d0_bf, "d0_32": d0_32, "flips": flips}


@pytest.fixture(scope="module")
def oracle320():
    return _oracle_at_320()


@pytest.fixture(scope="module")
def net320(cuda, oracle320):
    """The HIP network with the oracle's weights, after one recorded forward per walked size (320 x 320 last).  Keeps the Acts
    each stage was given, so that a stage can be run again on its own in exactly the buffers the network uses."""
    from sculptmate_amd.rembg.u2net import U2Net

    net = U2Net()
    net.load_state_dict(oracle320["sd"])
    net.to(cuda)
    acts, calls = {}, {}
    orig = net._rsu

    def rsu(name, kind, cin, mid, cout, x, out):
        acts[name] = (kind, cin, mid, cout, x, out)
        orig(name, kind, cin, mid, cout, x, out)

    net._rsu = rsu
    try:
        for size in WALKED[::-1]:
            calls[size] = []
            with _recording(calls[size], call_through=True):
                xin = oracle320["x"] if size == (320, 320) else torch.randn(3, *size, generator=_gen("walk", size))
                d0 = net.forward(xin.to(cuda)).cpu()
    finally:
        del net._rsu
    return {"net": net, "acts": acts, "calls": calls, "d0": d0}


@pytest.mark.parametrize("name", [s[0] for s in spec.STAGES])
def test_rsu_stage_vs_oracle(cuda, oracle320, net320, name):
    """One RSU block on its own: U2Net._rsu gets the input the bf16 oracle gave this stage, in the buffer slice the network
    uses for it, and its output is compared with the oracle's for that input.  Error does not compound across stages, so the
    failing id names the wrong stage.
    Up to 14 bf16-rounded layers deep, the tolerance cannot be derived; it is measured against the reference, not the kernels:
    e_ref = ||rsu_bf16(x) - rsu_fp32(x)|| / ||rsu_fp32(x)||, both from the oracle on the CPU.  Required:
    ||hip - rsu_fp32(x)|| / ||rsu_fp32(x)|| <= 2 e_ref  and  ||hip - rsu_bf16(x)|| <= 2 ||rsu_bf16(x) - rsu_fp32(x)||.
    Factor 2: the HIP stage and the bf16 oracle are two bf16 roundings of one fp32 function (another summation order flips
    single roundings, later layers amplify a flip), each may sit e_ref from fp32 on opposite sides; a structural error is of
    order 1."""
    s = oracle320["stages"][name]
    kind, cin, mid, cout, x, out = net320["acts"][name]
    xin = s["x"][0]                                              # [c, H, W], bf16-valued
    c, H, W = xin.shape
    assert (H, W) == (x.H, x.W) and c <= x.C and x.C - c < 8 and cout == out.C == s["fp32"].shape[1]
    x.buf[:, x.off:x.off + x.C] = 0
    x.buf[:, x.off:x.off + c] = xin.permute(1, 2, 0).reshape(H * W, c).to(BF).to(cuda)
    out.buf[:, out.off:out.off + out.C] = float("nan")
    net320["net"]._rsu(name, kind, cin, mid, cout, x, out)
    hip = out.buf[:, out.off:out.off + out.C].float().cpu().reshape(H, W, cout).permute(2, 0, 1).double()
    bf, f32 = s["bf16"][0].double(), s["fp32"][0].double()
    e_ref = float((bf - f32).norm() / f32.norm())
    e_hip = float((hip - f32).norm() / f32.norm())
    e_bf = float((hip - bf).norm() / (bf - f32).norm())
    print("STAGE %-8s %-5s %3dx%-3d  e_ref %.3e  hip-vs-fp32 / e_ref %.3f  |hip-bf16| / |bf16-fp32| %.3f" % (name, kind, H, W, e_ref, e_hip / e_ref, e_bf))
    assert not torch.isnan(hip).any()
    assert e_hip <= 2 * e_ref and e_bf <= 2, (e_ref, e_hip, e_bf)


def test_network_320_vs_oracle(cuda, oracle320, net320):
    """d0 of the blob image (a saturating, structured input; noise is the easy case) against the fp32 oracle, with the bf16
    oracle's own distance from it as the yardstick, recomputed here: max |hip - fp32| <= 2 max |bf16 - fp32|, the same in RMS,
    and the mask d0 > 0.5 differs from the fp32 oracle's in at most 2 x (the bf16 oracle's count) + 8 pixels.  The fixture
    asserts that the bf16 oracle's mask is itself within 1 % of the fp32 one, so that the input can tell something."""
    d0, bf, f32 = net320["d0"].double(), oracle320["d0_bf"].double(), oracle320["d0_32"].double()
    assert d0.shape == (320, 320) and not torch.isnan(d0).any()
    mx, mx_ref = float((d0 - f32).abs().max()), float((bf - f32).abs().max())
    rms, rms_ref = float((d0 - f32).pow(2).mean().sqrt()), float((bf - f32).pow(2).mean().sqrt())
    flips = int(((d0 > 0.5) != (f32 > 0.5)).sum())
    print("NETWORK 320: max %.3e (bf16 oracle %.3e)  rms %.3e (%.3e)  mask pixels %d (%d)" % (mx, mx_ref, rms, rms_ref, flips, oracle320["flips"]))
    assert mx <= 2 * mx_ref and rms <= 2 * rms_ref, (mx, mx_ref, rms, rms_ref)
    assert flips <= 2 * oracle320["flips"] + 8, (flips, oracle320["flips"])


def test_forward_is_reproducible_across_buffer_reuse(cuda, oracle320, net320):
    """The network keeps its activation buffers between calls: two forwards of one input give the same bits, they are the bits
    of the first forward ever made (whatever the stage tests left in the buffers since), and a forward at 72 x 56 in between
    changes nothing."""
    net, x = net320["net"], oracle320["x"].to(cuda)
    a = net.forward(x).cpu()
    b = net.forward(x).cpu()
    net.forward(torch.randn(3, 72, 56, generator=_gen("between")).to(cuda))
    c = net.forward(x).cpu()
    first = net320["d0"].view(torch.int32)
    assert torch.equal(a.view(torch.int32), first) and torch.equal(b.view(torch.int32), first) and torch.equal(c.view(torch.int32), first)
