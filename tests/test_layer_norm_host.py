"""Host side of the fused residual add + LayerNorm front (csrc/layer_norm.hip): on CPU tensors `add_layer_norm` / `layer_norm`
ARE the stock composite, the harness block's CPU forward does not go near them, and the C ABI refuses what the kernels do not
cover before anything is launched."""
import pytest
import torch
import torch.nn.functional as F

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import norm as dnorm


def _stock(x, delta, w, b, eps):
    h = x if delta is None else x + delta
    return h, F.layer_norm(h, (h.shape[-1],), w, b, eps)


# (with delta, which outputs get an upstream gradient); layer_norm has the one output
@pytest.mark.parametrize("with_delta,fed", [(True, "h"), (True, "y"), (True, "both"), (False, "y")])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_tensors_get_the_stock_composite_exactly(dtype, with_delta, fed):
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g).to(dtype)
    x, delta = rn(2, 5, 24).requires_grad_(True), (rn(2, 5, 24).requires_grad_(True) if with_delta else None)
    w, b = rn(24).requires_grad_(True), rn(24).requires_grad_(True)
    dh, dy = rn(2, 5, 24), rn(2, 5, 24)
    if with_delta:
        got = dnorm.add_layer_norm(x, delta, w, b, 1e-5)
    else:
        got = (x, dnorm.layer_norm(x, w, b, 1e-5))
    want = _stock(x, delta, w, b, 1e-5)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    ins = [x, w, b] + ([delta] if with_delta else [])
    pick = {"h": ([0], [dh]), "y": ([1], [dy]), "both": ([0, 1], [dh, dy])}[fed]
    grads = lambda outs: torch.autograd.grad([outs[i] for i in pick[0]], ins, pick[1], allow_unused=True)
    for u, v in zip(grads(got), grads(want)):
        assert (u is None and v is None) or torch.equal(u, v)


def test_unsupported_operands_are_told_apart_without_a_device():
    x, w = torch.randn(4, 16), torch.ones(16)
    assert not dnorm._hip_layer_norm(x, None, w, w)  # CPU
    assert not dnorm._hip_layer_norm(x.half(), x.half(), w.half(), w.half())  # still CPU


def test_harness_block_cpu_forward_is_the_three_stock_lines(monkeypatch):
    """The CPU forward of the harness's transformer block (the path the CPU oracle runs through) equals the three stock lines
    written out here, bit for bit, in fp32 and in bf16, and never calls the fused front."""
    from harness.unet import BasicTransformerBlock

    def boom(*a, **k):
        raise AssertionError("the CPU path must not reach the fused LayerNorm front")

    monkeypatch.setattr(dnorm, "layer_norm", boom)
    monkeypatch.setattr(dnorm, "add_layer_norm", boom)
    torch.manual_seed(3)
    blk = BasicTransformerBlock(32, 2, 16, 24)
    for dtype in (torch.float32, torch.bfloat16):
        blk = blk.to(dtype)
        g = torch.Generator().manual_seed(4)
        x, ctx = torch.randn(2, 10, 32, generator=g).to(dtype), torch.randn(2, 6, 24, generator=g).to(dtype)
        t = blk.attn1(blk.norm1(x)) + x
        t = blk.attn2(blk.norm2(t), ctx) + t
        t = blk.ff(blk.norm3(t)) + t
        assert torch.equal(blk(x, ctx), t)


# ------------------------------------------------------------------------------------------------ C ABI, without a device
BADARG, ALIGN, UNSUPPORTED = -1, -3, -5
P = 1 << 20  # a 16-byte-aligned stand-in for a device pointer: every call below is refused before anything reads it


def _fwd(x=P, delta=P, gamma=P, beta=P, h=P, y=P, mean=P, rstd=P, M=4, C=64, dtype=1):
    return nat.lib().add_layer_norm_fwd(x, delta, gamma, beta, h, y, mean, rstd, M, C, 1e-5, dtype, None)


def _bwd(dy=P, dh=P, h=P, gamma=P, mean=P, rstd=P, dx=P, M=4, C=64, dtype=1):
    return nat.lib().add_layer_norm_bwd(dy, dh, h, gamma, mean, rstd, dx, M, C, dtype, None)


def test_entry_points_tell_bad_arguments_from_unsupported_ones_before_any_launch():
    cmax = nat.lib().add_layer_norm_max_channels()
    assert cmax >= 2048 and cmax % 8 == 0
    for call in (_fwd, _bwd):
        assert call(C=0) == call(C=-8) == BADARG
        assert call(M=0) == call(M=-1) == BADARG
        assert call(dtype=7) == BADARG
        assert call(dtype=0) == UNSUPPORTED  # f32
        assert call(C=12) == UNSUPPORTED  # rows of 16-byte chunks
        assert call(C=cmax + 8) == UNSUPPORTED
        for dt in (1, 2):
            assert call(C=cmax, gamma=P + 2, dtype=dt) == call(C=8, gamma=P + 2, dtype=dt) == ALIGN  # both ends are covered
        assert call(M=1 << 40, gamma=P + 2) == ALIGN  # any M
    assert _fwd(x=None) == _fwd(y=None) == _bwd(dy=None) == BADARG
    assert _fwd(gamma=None) == _fwd(beta=None) == _fwd(mean=None) == _fwd(rstd=None) == BADARG
    assert _bwd(h=None) == _bwd(gamma=None) == _bwd(mean=None) == _bwd(rstd=None) == _bwd(dx=None) == BADARG
    assert _fwd(delta=P, h=None) == BADARG  # delta without h
    assert _fwd(delta=None, h=P) == BADARG  # h without delta
    for name in ("x", "delta", "gamma", "beta", "h", "y", "mean", "rstd"):
        assert _fwd(**{name: P + 2}) == ALIGN, name
    for name in ("dy", "dh", "h", "gamma", "mean", "rstd", "dx"):
        assert _bwd(**{name: P + 2}) == ALIGN, name
    assert _fwd(x=P + 8) == _bwd(dy=P + 8) == ALIGN
    # the nullable operands may be absent
    assert _fwd(delta=None, h=None, y=P + 2) == ALIGN and _bwd(dh=None, dx=P + 2) == ALIGN
    # the shape is judged before the pointers
    for call in (_fwd, _bwd):
        assert call(C=0, gamma=P + 2) == BADARG and call(dtype=7, gamma=P + 2) == BADARG
        assert call(C=12, gamma=P + 2) == call(dtype=0, gamma=P + 2) == call(C=cmax + 8, gamma=P + 2) == UNSUPPORTED
