"""Host side of the fused GroupNorm front: on CPU tensors `group_norm_act` IS the stock composite, and the harness's CPU
forward (the path the CPU oracle runs through) does not go near it."""
import pytest
import torch
import torch.nn.functional as F

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import norm as dnorm
from tests.conftest import build_tiny_unet
from tests.norm_cases import BIG_GROUP, NCHW_GEOMETRY, NHWC_GEOMETRY, SMALL_GROUPS


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


# ------------------------------------------------------------------------------------------------ C ABI, without a device
BADARG, ALIGN, UNSUPPORTED = -1, -3, -5
P = 1 << 20  # a 16-byte-aligned stand-in for a device pointer: every call below is refused before anything reads it


def _fwd(x=P, addend=P, y=P, ws=P, N=2, C=16, HW=8, G=4, act=1, cl=0, dtype=1):
    return nat.lib().group_norm_act_fwd(x, addend, P, P, y, P, P, ws, N, C, HW, G, 1e-5, act, cl, dtype, None)


def _bwd(dy=P, x=P, addend=P, dx=P, da=P, ws=P, N=2, C=16, HW=8, G=4, act=1, cl=0, dtype=1):
    return nat.lib().group_norm_act_bwd(dy, x, addend, P, P, P, P, dx, da, ws, N, C, HW, G, act, cl, dtype, None)


def test_entry_points_tell_bad_arguments_from_unsupported_ones_before_any_launch():
    for call in (_fwd, _bwd):
        assert call(C=18, G=4) == BADARG  # C % G ≠ 0
        assert call(act=2) == BADARG
        assert call(dtype=7) == BADARG
        assert call(x=None) == BADARG
        assert call(dtype=0) == UNSUPPORTED  # f32
        assert call(C=257 * 8, G=257, cl=0) == call(C=257 * 8, G=257, cl=1) == UNSUPPORTED  # kMaxGroups = 256
        assert call(HW=9) == UNSUPPORTED  # NCHW rows of 16-byte chunks
        assert call(C=12, cl=1) == UNSUPPORTED  # NHWC threads of 8 channels
        assert call(x=P + 2) == call(ws=P + 2) == call(x=P + 8) == ALIGN
    assert _fwd(y=P + 2) == _bwd(dy=P + 2) == _bwd(dx=P + 2) == ALIGN
    assert _bwd(addend=None, da=P) == BADARG  # an addend gradient without an addend
    assert _fwd(C=18, G=4, x=P + 2) == BADARG and _fwd(HW=9, x=P + 2) == UNSUPPORTED  # the shape is judged before the pointers


def test_workspace_bytes_is_zero_for_what_the_kernels_do_not_cover_and_grows_with_da():
    ws = nat.lib().group_norm_act_workspace_bytes
    for want_da in (0, 1):
        assert ws(2, 16, 9, 4, 0, want_da) == 0  # NCHW, H·W % 8 ≠ 0
        assert ws(2, 16, 1, 4, 0, want_da) == 0  # H·W = 1
        assert ws(2, 12, 16, 4, 1, want_da) == 0  # NHWC, C % 8 ≠ 0
        assert ws(1, 512, 8, 512, 0, want_da) == ws(1, 512, 8, 512, 1, want_da) == 0  # G = 512
        assert ws(1, 257 * 8, 8, 257, 1, want_da) == 0 and ws(1, 256 * 8, 8, 256, 1, want_da) > 0  # G = 257 / kMaxGroups
        assert ws(2, 18, 8, 4, 0, want_da) == 0  # C % G ≠ 0
        assert ws(65536, 8, 8, 1, 0, want_da) == 0  # more (n, group) slabs than a grid dimension holds
    for cl, shapes in ((0, NCHW_GEOMETRY + [BIG_GROUP, SMALL_GROUPS]), (1, NHWC_GEOMETRY + [BIG_GROUP, SMALL_GROUPS])):
        for N, C, G, H, W in shapes:
            no_da, with_da = ws(N, C, H * W, G, cl, 0), ws(N, C, H * W, G, cl, 1)
            assert 0 < no_da <= with_da and no_da % 16 == 0 and with_da % 16 == 0, (cl, N, C, G, H, W)
            # the forward's partials: one (mean, M2) pair per row in NCHW (3 floats a row are kept for the backward's sums),
            # at least one pair per (n, group) in NHWC
            assert no_da >= (N * C * 3 * 4 if not cl else N * G * 2 * 4)
            if cl:  # the per-channel partials of the addend gradient: three sums per channel and row block, at least one block
                assert with_da - no_da >= N * 3 * C * 4
