"""Host side of the block-edge fronts: on CPU tensors each IS the stock composite and never touches the library, the harness's
CPU forward is bit-equal to the stock lines, and the `supported` queries and argument checks of the new entry points answer
without a device."""
import pytest
import torch
import torch.nn.functional as F

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import norm as dnorm


def _tokens(t):
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n, h * w, c)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_cpu_tensors_get_the_stock_composite_and_never_reach_the_library(monkeypatch, dtype):
    def boom(*a, **k):
        raise AssertionError("the CPU path must not reach the library")

    monkeypatch.setattr(nat, "lib", boom)
    torch.manual_seed(3)
    N, C, G, H, W = 2, 16, 4, 4, 6
    x, other = torch.randn(N, C, H, W).to(dtype), torch.randn(N, C, H, W).to(dtype)
    a, w, b = torch.randn(N, C).to(dtype), torch.randn(C).to(dtype), torch.randn(C).to(dtype)
    for act in (True, False):
        for add in (a, None):
            xs = x.clone().requires_grad_(True)
            xp, y = dnorm.group_norm_act_res(xs, G, w, b, 1e-5, act, add)
            h = F.group_norm(xs if add is None else xs + add[:, :, None, None], G, w, b, 1e-5)
            assert xp is xs and torch.equal(y, F.silu(h) if act else h)
    xp, tok = dnorm.group_norm_tokens(x, G, w, b, 1e-6)
    assert xp is x and torch.equal(tok, _tokens(F.group_norm(x, G, w, b, 1e-6)))
    assert not dnorm.group_norm_tokens_supported(x, G, w, b) and not dnorm.tokens_to_nchw_add_supported(tok, x)
    assert torch.equal(dnorm.tokens_to_nchw_add(tok, other), tok.view(N, H, W, C).permute(0, 3, 1, 2).contiguous() + other)
    v = lambda t: t[None, :, None, None]
    assert torch.equal(dnorm.residual_bias_add(x, other, w), other + (x + v(w)))
    assert torch.equal(dnorm.residual_bias_add(x, other, w, b), (other + v(b)) + (x + v(w)))
    # gradients flow through the composites like through the stock lines
    xs, ts = x.clone().requires_grad_(True), tok.clone().requires_grad_(True)
    xp, t = dnorm.group_norm_tokens(xs, G, w, b, 1e-6)
    out = dnorm.tokens_to_nchw_add(t + ts, xp)
    want = (_tokens(F.group_norm(xs, G, w, b, 1e-6)) + ts).view(N, H, W, C).permute(0, 3, 1, 2).contiguous() + xs
    for u, r in zip(torch.autograd.grad(out, [xs, ts], other), torch.autograd.grad(want, [xs, ts], other)):
        assert torch.equal(u, r)


def test_harness_cpu_forward_is_bit_equal_to_the_stock_lines(monkeypatch):
    import harness.unet as hu

    def boom(*a, **k):
        raise AssertionError("the CPU path must not reach the block-edge fronts")

    for name in ("group_norm_act_res", "group_norm_tokens", "tokens_to_nchw_add", "residual_bias_add"):
        monkeypatch.setattr(dnorm, name, boom)
    torch.manual_seed(4)
    temb = torch.randn(2, 128)
    for cin in (32, 64):
        blk = hu.ResnetBlock2D(cin, 64, 128, 8)
        x = torch.randn(2, cin, 6, 12)
        h = blk.conv1(F.silu(blk.norm1(x))) + blk.time_emb_proj(F.silu(temb))[:, :, None, None]
        h = blk.conv2(F.silu(blk.norm2(h)))
        assert torch.equal(blk(x, temb), (x if blk.conv_shortcut is None else blk.conv_shortcut(x)) + h)
    for linear in (False, True):
        tr = hu.Transformer2DModel(64, 2, 48, 8, linear)
        x, ctx = torch.randn(2, 64, 6, 12), torch.randn(2, 6, 48)
        b, c, hh, ww = x.shape
        t = tr.norm(x)
        if linear:
            t = tr.proj_in(t.permute(0, 2, 3, 1).reshape(b, hh * ww, c))
        else:
            t = tr.proj_in(t).permute(0, 2, 3, 1).reshape(b, hh * ww, c)
        t = tr.transformer_blocks[0](t, ctx)
        if linear:
            t = tr.proj_out(t).reshape(b, hh, ww, c).permute(0, 3, 1, 2).contiguous()
        else:
            t = tr.proj_out(t.reshape(b, hh, ww, c).permute(0, 3, 1, 2))
        assert torch.equal(tr(x, ctx), t + x)


def test_supported_queries_and_argument_checks_answer_without_a_device():
    lib = nat.lib()
    F16, BF16, F32 = nat.dtype_code(torch.float16), nat.dtype_code(torch.bfloat16), nat.dtype_code(torch.float32)
    # (N, C, HW): whole 16-byte chunks both ways for the re-layouts, along H·W for the sum
    for dt in (F16, BF16):
        assert lib.tokens_nchw_supported(2, 320, 64, dt) == 1 and lib.tokens_nchw_supported(3, 40, 24, dt) == 1
        assert lib.tokens_nchw_supported(1, 1280, 4096, dt) == 1
        assert lib.tokens_nchw_supported(2, 16, 9, dt) == 0 and lib.tokens_nchw_supported(2, 12, 16, dt) == 0
        assert lib.tokens_nchw_supported(65536, 8, 8, dt) == 0 and lib.tokens_nchw_supported(0, 8, 8, dt) == 0
        assert lib.residual_bias_add_supported(2, 12, 16, dt) == 1 and lib.residual_bias_add_supported(2, 16, 9, dt) == 0
    assert lib.tokens_nchw_supported(2, 320, 64, F32) == 0 and lib.residual_bias_add_supported(2, 320, 64, F32) == 0
    assert lib.tokens_nchw_supported(2, 320, 64, 7) == 0
    assert nat.tokens_nchw_supported(2, 320, 64, torch.float16) and not nat.tokens_nchw_supported(2, 320, 64, torch.float32)

    P, ODD = 4096, 4098  # stand-ins for device pointers: every status below is decided before anything is dereferenced
    E_BADARG, E_ALIGN, E_UNSUPPORTED = -1, -3, -5
    assert lib.residual_bias_add(None, P, P, None, P, 2, 16, 16, F16, None) == E_BADARG
    assert lib.residual_bias_add(P, P, None, None, P, 2, 16, 16, F16, None) == E_BADARG
    assert lib.residual_bias_add(P, P, P, None, P, 2, 16, 16, 7, None) == E_BADARG
    assert lib.residual_bias_add(P, P, P, None, P, 2, 16, 0, F16, None) == E_BADARG
    assert lib.residual_bias_add(P, P, P, None, P, 2, 16, 16, F32, None) == E_UNSUPPORTED
    assert lib.residual_bias_add(ODD, P, P, None, P, 2, 16, 12, F16, None) == E_UNSUPPORTED  # the shape before the pointers
    for args in ((ODD, P, P), (P, ODD, P), (P, P, ODD)):
        assert lib.residual_bias_add(args[0], args[1], P, ODD, args[2], 2, 16, 16, BF16, None) == E_ALIGN
    assert lib.tokens_to_nchw_add(None, P, P, 2, 16, 16, F16, None) == E_BADARG
    assert lib.tokens_to_nchw_add(P, None, None, 2, 16, 16, F16, None) == E_BADARG
    assert lib.tokens_to_nchw_add(P, P, P, 2, 12, 16, F16, None) == E_UNSUPPORTED
    assert lib.tokens_to_nchw_add(P, P, P, 2, 16, 16, F32, None) == E_UNSUPPORTED
    for args in ((ODD, P, P), (P, ODD, P), (P, None, ODD)):
        assert lib.tokens_to_nchw_add(*args, 2, 16, 16, F16, None) == E_ALIGN
    assert lib.nchw_to_tokens(None, P, 2, 16, 16, F16, None) == E_BADARG
    assert lib.nchw_to_tokens(P, P, 2, 16, 20, F16, None) == E_UNSUPPORTED
    assert lib.nchw_to_tokens(ODD, P, 2, 16, 16, F16, None) == E_ALIGN and lib.nchw_to_tokens(P, ODD, 2, 16, 16, BF16, None) == E_ALIGN

    bwd = lambda dy, dh, x, dx, ws, hw=16, dt=F16, act=1: lib.group_norm_act_bwd_res(dy, dh, x, None, P, P, P, P, dx, None, ws, 2, 16,
                                                                                   hw, 4, act, dt, None)
    assert bwd(None, P, P, P, P) == E_BADARG and bwd(P, P, P, P, P, act=2) == E_BADARG
    assert bwd(P, P, P, P, P, dt=F32) == E_UNSUPPORTED and bwd(P, ODD, P, P, P, hw=12) == E_UNSUPPORTED
    for args in ((ODD, P, P, P, P), (P, ODD, P, P, P), (P, None, ODD, P, P), (P, P, P, ODD, P), (P, P, P, P, ODD)):
        assert bwd(*args) == E_ALIGN
