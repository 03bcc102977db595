"""sculpt_vit_assemble_stats: the tokenizer's glue in front of layer 0 in one launch -- the assembled token rows, their bf16 copy
and the 64-column slice statistics must be the bits of sculpt_vit_assemble followed by sculpt_row_slice_stats."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("T,H", [(5, 64), (17, 128), (1025, 768)])
def test_fused_assemble_and_statistics_equal_the_two_kernels(cuda, T, H):
    from sculptmate_amd import ops

    g = torch.Generator().manual_seed(T * 1000 + H)
    n = T - 1
    po = (torch.randn(n, H, generator=g) + 3.0 * torch.randn(n, 1, generator=g)).to(cuda)   # a row offset: the mean term matters
    cls, pos = torch.randn(H, generator=g).to(cuda), torch.randn(T, H, generator=g).to(cuda)
    pad = 3                                                     # rows past the tokens in every output: never written
    tok0, hb0, st0 = _nan((T + pad, H), torch.float32, cuda), _nan((T + pad, H), BF, cuda), _nan((H // 64, T + pad, 2), torch.float32, cuda)
    ops.vit_assemble(po, cls, pos, tok0[:T])
    ops.row_slice_stats(tok0, st0, hb0, rows=T)
    tok1, hb1, st1 = _nan((T + pad, H), torch.float32, cuda), _nan((T + pad, H), BF, cuda), _nan((H // 64, T + pad, 2), torch.float32, cuda)
    ops.vit_assemble_stats(po, cls, pos, tok1[:T], st1, hb1)
    assert torch.isfinite(tok1[:T]).all() and torch.isfinite(st1[:, :T]).all() and torch.isfinite(hb1[:T].float()).all()
    assert torch.equal(_bits(tok1[:T]), _bits(tok0[:T]))
    assert torch.equal(_bits(hb1[:T]), _bits(hb0[:T]))
    assert torch.equal(_bits(st1[:, :T]), _bits(st0[:, :T]))
    assert torch.isnan(tok1[T:]).all() and torch.isnan(hb1[T:].float()).all() and torch.isnan(st1[:, T:]).all()
