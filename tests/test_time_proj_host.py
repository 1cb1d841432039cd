"""Host side of the batched time-embedding projections (diffusion_finetuning_amd.time_proj, csrc/time_proj.hip): off the
kernel's envelope the front IS the stock lines and never touches the library, the `supported` query and the argument checks
answer without a device, and the harness computes the same bits whether a block is handed its addend or computes it."""
import ctypes

import torch
import torch.nn.functional as F

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import time_proj as tp


def _layers(dtype, E=24, widths=(5, 16, 7), seed=2):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g).to(dtype)
    layers = [(rn(c, E), rn(c), rn(c)) for c in widths]
    layers[1] = (layers[1][0], None, layers[1][2])
    layers[2] = (layers[2][0], layers[2][1], None)
    return rn(3, E), layers


def _stock(temb, layers):
    outs = []
    for w, b, cb in layers:
        h = F.linear(F.silu(temb), w, b)
        outs.append(h if cb is None else h + cb)
    return outs


def test_cpu_fp32_and_trainable_operands_get_the_stock_lines_and_never_reach_the_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("this path must not reach the library")

    monkeypatch.setattr(nat, "lib", boom)
    monkeypatch.setattr(nat, "time_proj_all", boom)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        temb, layers = _layers(dtype)
        assert not tp.time_projections_supported(temb, layers)
        for got, want in zip(tp.time_projections(temb, layers), _stock(temb, layers)):
            assert got.dtype == dtype and torch.equal(got, want)
    # a trainable weight keeps its gradient path: the stock lines, whose gradients are the stock ones
    temb, layers = _layers(torch.float32)
    w = layers[0][0].clone().requires_grad_(True)
    ts = temb.clone().requires_grad_(True)
    mine = [(w, layers[0][1], layers[0][2])] + layers[1:]
    outs = tp.time_projections(ts, mine)
    want = _stock(ts, mine)
    assert all(torch.equal(a, b) for a, b in zip(outs, want))
    dy = torch.ones_like(outs[0])
    for a, b in zip(torch.autograd.grad(outs[0], [w, ts], dy), torch.autograd.grad(want[0], [w, ts], dy)):
        assert torch.equal(a, b)
    assert tp.time_projections(temb, []) == []


def test_supported_query_and_argument_checks_answer_without_a_device():
    lib = nat.lib()
    F16, BF16, F32 = nat.dtype_code(torch.float16), nat.dtype_code(torch.bfloat16), nat.dtype_code(torch.float32)
    for dt in (F16, BF16):
        for N, E, ok in ((1, 8, 1), (4, 1280, 1), (16, 1288, 1), (3, 40, 1), (17, 1280, 0), (4, 12, 0), (0, 8, 0), (4, 0, 0)):
            assert lib.time_proj_supported(N, E, dt) == ok, (N, E, dt)
    assert lib.time_proj_supported(4, 1280, F32) == 0 and lib.time_proj_supported(4, 1280, 7) == 0
    assert nat.time_proj_supported(4, 1280, torch.float16) and not nat.time_proj_supported(4, 1280, torch.float32)

    P, ODD = 4096, 4098  # stand-ins for device pointers: every status below is decided before anything is dereferenced
    E_BADARG, E_ALIGN, E_UNSUPPORTED = -1, -3, -5
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    W, B, C = ptrs(P, P), ptrs(P, None), ints(5, 7)
    call = lambda t=P, W=W, b=B, cb=None, C=C, out=P, L=2, N=4, E=16, dt=F16: lib.time_proj_all(t, W, b, cb, C, out, L, N, E, dt, None)
    # 1. null pointers, non-positive sizes, unknown dtype
    assert call(t=None) == E_BADARG and call(W=None) == E_BADARG and call(C=None) == E_BADARG and call(out=None) == E_BADARG
    assert call(W=ptrs(P, None)) == E_BADARG and call(C=ints(5, 0)) == E_BADARG
    assert call(L=0) == E_BADARG and call(N=0) == E_BADARG and call(E=0) == E_BADARG and call(dt=7) == E_BADARG
    assert call(t=None, dt=F32) == E_BADARG and call(t=None, N=17) == E_BADARG  # a null pointer before the envelope
    # 2. the envelope, before the pointers' alignment
    assert call(dt=F32) == E_UNSUPPORTED and call(N=17) == E_UNSUPPORTED and call(E=12) == E_UNSUPPORTED
    assert call(t=ODD, N=17) == E_UNSUPPORTED and call(W=ptrs(ODD, P), E=12, dt=BF16) == E_UNSUPPORTED
    assert call(C=ints(2 ** 31 - 1, 7)) == E_UNSUPPORTED  # more rows than one launch numbers
    # 3. alignment of t and of every weight; biases and out only need their elements' alignment
    assert call(t=ODD) == E_ALIGN and call(W=ptrs(ODD, P)) == E_ALIGN and call(W=ptrs(P, ODD), dt=BF16) == E_ALIGN
    # the 34th layer's pointer is looked at too: a list longer than one launch's 32 layers is checked whole, before any launch
    many = [P] * 33 + [ODD]
    assert lib.time_proj_all(P, ptrs(*many), None, None, ints(*([3] * 34)), P, 34, 4, 16, F16, None) == E_ALIGN
    many[33] = None
    assert lib.time_proj_all(P, ptrs(*many), None, None, ints(*([3] * 34)), P, 34, 4, 16, F16, None) == E_BADARG


def test_harness_cpu_forward_is_bit_equal_with_and_without_the_addend_argument(monkeypatch):
    import harness.unet as hu

    torch.manual_seed(5)
    temb = torch.randn(2, 128)
    for cin in (32, 64):
        blk = hu.ResnetBlock2D(cin, 64, 128, 8)
        x = torch.randn(2, cin, 6, 12)
        w, b, cb = blk.time_addend_layer()
        assert w is blk.time_emb_proj.weight and b is blk.time_emb_proj.bias and cb is blk.conv1.bias
        (addend,) = tp.time_projections(temb, [(w, b, cb)])
        assert torch.equal(addend, blk.time_emb_proj(F.silu(temb)) + blk.conv1.bias)
        # the CPU keeps the stock lines, which take no addend: the argument changes nothing
        assert torch.equal(blk(x, temb, addend), blk(x, temb)) and torch.equal(blk(x, temb, None), blk(x, temb))
    blk.time_emb_proj = torch.nn.Sequential(blk.time_emb_proj)  # not the stock module: the block computes its own addend
    assert blk.time_addend_layer() is None

    # the whole model: the CPU forward asks for no batched projection and equals the per-block forward bit for bit
    torch.manual_seed(6)
    unet = hu.UNet2DConditionModel(hu.tiny_config(32, 32, 2)).requires_grad_(False)
    sample, ctx, t = torch.randn(2, 4, 8, 8), torch.randn(2, 6, 32), torch.tensor([3, 700])
    names = [n for n, m in unet.named_modules()]
    keys = list(unet.state_dict())
    want = unet(sample, t, ctx).sample

    def boom(*a, **k):
        raise AssertionError("the CPU forward must not ask for the batched projections")

    monkeypatch.setattr(hu, "_time_projections", boom)
    assert torch.equal(unet(sample, t, ctx).sample, want)
    monkeypatch.undo()
    # handing every block its addend by hand (what the GPU forward does) is the same forward on the CPU
    blocks = [*unet.down_blocks, unet.mid_block, *unet.up_blocks]
    temb = unet.time_embedding(unet.time_proj(t).to(sample.dtype))
    addends = unet._time_addends(temb, blocks)
    assert sum(len(v) for v in addends.values()) == sum(len(b.resnets) for b in blocks)
    assert all(a is not None and a.shape == (2, r.conv1.out_channels) for b in blocks for a, r in zip(addends[b], b.resnets))
    x = unet.conv_in(sample)
    skips = [x]
    for blk in unet.down_blocks:
        x, outs = blk(x, temb, ctx, addends[blk])
        skips += outs
    x = unet.mid_block(x, temb, ctx, addends[unet.mid_block])
    for blk in unet.up_blocks:
        x = blk(x, skips, temb, ctx, addends[blk])
    assert torch.equal(unet.conv_out(F.silu(unet.conv_norm_out(x))), want)
    assert [n for n, m in unet.named_modules()] == names and list(unet.state_dict()) == keys
