"""The image-independent head of the TSR backbone (GroupNorm, proj_in, block 0's self-attention and cross-attention query
projection) is computed once per prepared model and cached: every forward must give the bits of a pass that computes it afresh,
the cache must follow the weights, and no forward may write it."""
import pytest
import torch

from sculptmate_amd import synth
from sculptmate_amd.tsr.spec import SMALL_CFG

pytestmark = pytest.mark.gpu


def _model(cuda, precision="bf16", sd=None):
    from sculptmate_amd.tsr import TSR

    m = TSR(SMALL_CFG, pos_embed_mode="size", precision=precision)
    m.load_state_dict(sd if sd is not None else synth.tsr_state(31, SMALL_CFG))
    m.to(cuda)
    return m


def _images(cuda, n=3):
    S = SMALL_CFG["cond_image_size"]
    return [torch.from_numpy(synth.composite_rgb(synth.image_rgba(seed=40 + i, size=S))).to(cuda) for i in range(n)]


def _uncached(m, im):
    """The pass as it was before the cache: the whole head through the blocks, every launch issued for this image."""
    ctx, _ = m.image_tokens(im)
    out, outb = m._backbone_tail(m._run_blocks(m._backbone_head(), ctx))
    return out.clone(), outb.clone()


@pytest.mark.parametrize("precision", ["bf16", "bf16l3", "fp16l2"])
def test_encode_image_equals_the_sequential_calls_and_the_uncached_pass(cuda, precision):
    m = _model(cuda, precision)
    imgs = _images(cuda)
    fresh = [_uncached(m, im) for im in imgs]
    want = []
    for im in imgs:
        ctx, _ = m.image_tokens(im)
        out, outb = m.backbone_tokens(ctx)
        want.append((out.clone(), outb.clone()))
    got = []
    for rep in range(3):
        for im in imgs:                       # no synchronisation between images or rounds
            out, outb = m.encode_image(im)
            got.append((out.clone(), outb.clone()))
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(want[k][0], fresh[k][0]) and torch.equal(want[k][1], fresh[k][1]), k
    for k, (o, ob) in enumerate(got):
        assert torch.isfinite(o).all()
        assert torch.equal(o, want[k % 3][0]) and torch.equal(ob, want[k % 3][1]), k


def test_stacked_pass_equals_the_single_passes(cuda):
    """bf16 mode: a stacked pass keeps the single-image tile forms (TSR.batch_exact), so each image gets the bits of its own pass --
    now from copies of the cached head instead of a head computed beside the tokenizer."""
    m = _model(cuda)
    imgs = _images(cuda)
    single = [m.encode_image(im)[0].clone() for im in imgs]
    out, _ = m.encode_images(imgs)
    T = out.shape[0] // 3
    for b in range(3):
        assert torch.equal(out[b * T:(b + 1) * T], single[b]), b


@pytest.mark.parametrize("precision", ["bf16", "bf16l3"])
def test_cache_follows_load_state_dict(cuda, precision):
    sd = synth.tsr_state(31, SMALL_CFG)
    m = _model(cuda, precision, sd)
    im = _images(cuda, 1)[0]
    before = m.encode_image(im)[0].clone()
    sd2 = dict(sd)
    key = "backbone.transformer_blocks.0.attn1.to_q.weight"
    sd2[key] = torch.as_tensor(sd[key]).clone() * 1.5
    m.load_state_dict(sd2)
    after = m.encode_image(im)[0].clone()
    fresh = _model(cuda, precision, sd2).encode_image(im)[0]
    assert torch.equal(after, fresh)
    assert not torch.equal(after, before)
    m.to(cuda)                                # .to() rebuilds the weights: the cache is rebuilt with them, same bits
    assert m._head0 is None
    assert torch.equal(m.encode_image(im)[0], fresh)


def test_no_forward_writes_the_cache(cuda):
    m = _model(cuda)
    imgs = _images(cuda)
    m.encode_image(imgs[0])
    hc = m._head0
    keep = {k: hc[k].clone() for k in ("h0", "hb0", "stats0", "q0")}
    for i in range(10):
        if i % 5 == 4:
            m.encode_images(imgs)
        else:
            m.encode_image(imgs[i % 3])
    torch.cuda.synchronize()
    assert m._head0 is hc
    for k, v in keep.items():
        assert torch.equal(hc[k], v), k
