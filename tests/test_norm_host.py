"""Host side of the fused GroupNorm front: on CPU tensors `group_norm_act` IS the stock composite, and the harness's CPU
forward (the path the CPU oracle runs through) does not go near it."""
import pytest
import torch
import torch.nn.functional as F

from diffusion_finetuning_amd import norm as dnorm
from tests.conftest import build_tiny_unet


@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("with_addend", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_tensors_get_the_stock_composite_exactly(act, with_addend, dtype):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 24, 6, 6, generator=g).to(dtype).requires_grad_(True)
    a = torch.randn(2, 24, generator=g).to(dtype).requires_grad_(True) if with_addend else None
    w, b = torch.randn(24, generator=g).to(dtype), torch.randn(24, generator=g).to(dtype)
    got = dnorm.group_norm_act(x, 4, w, b, 1e-5, act, a)
    h = x if a is None else x + a[:, :, None, None]
    h = F.group_norm(h, 4, w, b, 1e-5)
    want = F.silu(h) if act else h
    assert torch.equal(got, want)
    dy = torch.randn(got.shape, generator=g).to(dtype)
    ins = [x] + ([a] if with_addend else [])
    for u, v in zip(torch.autograd.grad(got, ins, dy), torch.autograd.grad(want, ins, dy)):
        assert torch.equal(u, v)


def test_harness_cpu_forward_is_the_stock_modules(monkeypatch):
    """The CPU forward of the harness blocks equals the stock module composition written out here, bit for bit, and never
    calls the fused front."""
    def boom(*a, **k):
        raise AssertionError("the CPU path must not reach group_norm_act")

    monkeypatch.setattr(dnorm, "group_norm_act", boom)
    unet = build_tiny_unet(1)
    blk = unet.down_blocks[0].resnets[0]
    g = torch.Generator().manual_seed(2)
    x, temb = torch.randn(2, 32, 8, 8, generator=g), torch.randn(2, 128, generator=g)
    h = blk.conv1(F.silu(blk.norm1(x)))
    h = h + blk.time_emb_proj(F.silu(temb))[:, :, None, None]
    h = blk.conv2(F.silu(blk.norm2(h)))
    assert torch.equal(blk(x, temb), x + h)

    tr = unet.down_blocks[0].attentions[0]
    ctx = torch.randn(2, 6, 32, generator=g)
    t = tr.proj_in(tr.norm(x)).permute(0, 2, 3, 1).reshape(2, 64, 32)
    for b in tr.transformer_blocks:
        t = b(t, ctx)
    assert torch.equal(tr(x, ctx), tr.proj_out(t.reshape(2, 8, 8, 32).permute(0, 3, 1, 2)) + x)

    out = unet(torch.randn(2, 4, 8, 8, generator=g), torch.tensor([3, 7]), ctx).sample
    assert out.shape == (2, 4, 8, 8) and torch.isfinite(out).all()


def test_unsupported_operands_are_told_apart_without_a_device():
    x = torch.randn(2, 16, 4, 4)
    w = torch.ones(16)
    assert dnorm._hip_layout(x, 4, w, w, None) is None  # CPU
    assert dnorm._hip_layout(x.half(), 4, w.half(), w.half(), None) is None  # still CPU
