"""The fused GroupNorm (+ addend, + SiLU) kernels of csrc/norm.hip against float64 math on the same stored inputs.

Yardstick: the stock composite (`x + a` → F.group_norm → F.silu and its autograd, same dtype, on the GPU) measured against
the same float64 result.  The fused op's maximum and RMS error may exceed the stock path's by at most one unit in the last
place of the storage type at the output's magnitude — it rounds once where the stock form rounds two or three times, so it
should sit at or below it.  Every figure is printed before it is asserted."""
import math

import pytest
import torch
import torch.nn.functional as F

from diffusion_finetuning_amd.norm import _hip_layout, group_norm_act

pytestmark = pytest.mark.gpu

# (N, C, groups, H = W): the SD1.5 trunk (C/32 = 10 … 80 channels per group at 64 … 8), its batch-1 and batch-8 forms, the
# 96² / SD2.1 sizes of config 5, and the tiny parity model (8 groups of 4, 8, 12)
CASES = [
    (4, 320, 32, 64), (4, 640, 32, 64), (4, 960, 32, 64), (4, 640, 32, 32), (4, 1280, 32, 32), (4, 1920, 32, 32),
    (4, 1280, 32, 16), (4, 2560, 32, 16), (4, 1280, 32, 8), (4, 2560, 32, 8),
    (1, 320, 32, 32), (1, 1920, 32, 16), (8, 640, 32, 16), (8, 2560, 32, 8), (8, 320, 32, 64),
    (2, 320, 32, 96), (2, 960, 32, 48), (2, 1920, 32, 24), (2, 2560, 32, 12),
    (2, 32, 8, 8), (2, 64, 8, 16), (2, 96, 8, 8), (1, 96, 8, 12),
]
# (act, addend, eps): both eps of the model (resnets 1e-5 with SiLU, transformer entry 1e-6 without), each with and without addend
VARIANTS = [(True, True, 1e-5), (True, False, 1e-5), (False, False, 1e-6), (False, True, 1e-6), (True, True, 1e-6)]
EPS = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}


def _inputs(N, C, H, dtype, channels_last, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    x = (rn(N, C, H, H) * (0.5 + rn(1, C, 1, 1).abs()) + rn(1, C, 1, 1)).to(dtype)  # per-channel spread and offset
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    a = (0.5 * rn(N, C)).to(dtype)
    w, b = (1 + 0.2 * rn(C)).to(dtype), (0.2 * rn(C)).to(dtype)
    dy = rn(N, C, H, H).to(dtype)
    if channels_last:
        dy = dy.contiguous(memory_format=torch.channels_last)
    return x, a, w, b, dy


def _run(fn, x, a, dy):
    x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    ins = [x]
    if a is not None:
        a = a.detach().clone().requires_grad_(True)
        ins.append(a)
    y = fn(x, a)
    grads = torch.autograd.grad(y, ins, dy.to(y.dtype))
    return [y.detach()] + [t.detach() for t in grads]


def _composite(groups, w, b, eps, act):
    def fn(x, a):
        h = x if a is None else x + a[:, :, None, None]
        h = F.group_norm(h, groups, w, b, eps)
        return F.silu(h) if act else h
    return fn


def _ulp(ref, dtype):
    m = ref.abs().max().item()
    return EPS[dtype] * 2.0 ** math.floor(math.log2(m)) if m > 0 else 0.0


def _errs(t, ref):
    d = t.double() - ref
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-c%d-g%d-hw%d" % c)
def test_fused_norm_is_no_worse_than_stock_against_float64(case, channels_last, dtype):
    N, C, G, H = case
    for vi, (act, with_a, eps) in enumerate(VARIANTS):
        x, a, w, b, dy = _inputs(N, C, H, dtype, channels_last, 100 + vi)
        a = a if with_a else None
        assert _hip_layout(x, G, w, b, a) == int(channels_last)  # the HIP path is what is measured
        ref = _run(_composite(G, w.double(), b.double(), eps, act), x.double(), None if a is None else a.double(), dy.double())
        stock = _run(_composite(G, w, b, eps, act), x, a, dy)
        fused = _run(lambda xx, aa: group_norm_act(xx, G, w, b, eps, act, aa), x, a, dy)
        assert fused[0].stride() == x.stride() and fused[1].stride() == x.stride()
        for name, f, s, r in zip(("y", "dx", "da"), fused, stock, ref):
            (fmax, frms), (smax, srms), ulp = _errs(f, r), _errs(s, r), _ulp(r, dtype)
            print(f"{case} cl={int(channels_last)} {dtype} act={int(act)} a={int(with_a)} eps={eps:g} {name}: "
                  f"fused max {fmax:.3e} rms {frms:.3e} | stock max {smax:.3e} rms {srms:.3e} | ulp {ulp:.3e}")
            assert fmax <= smax + ulp, (name, act, with_a, eps, fmax, smax, ulp)
            assert frms <= srms + ulp, (name, act, with_a, eps, frms, srms, ulp)


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("case", [(4, 320, 32, 64), (4, 2560, 32, 8), (2, 96, 8, 8), (8, 640, 32, 16)],
                         ids=lambda c: "n%d-c%d-g%d-hw%d" % c)
def test_two_runs_are_bit_identical_and_a_graph_replay_equals_eager(case, channels_last):
    N, C, G, H = case
    x, a, w, b, dy = _inputs(N, C, H, torch.float16, channels_last, 7)
    fn = lambda xx, aa: group_norm_act(xx, G, w, b, 1e-5, True, aa)
    first, second = _run(fn, x, a, dy), _run(fn, x, a, dy)
    assert all(torch.equal(u, v) for u, v in zip(first, second))

    xs, as_ = x.clone(memory_format=torch.preserve_format).requires_grad_(True), a.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(fn(xs, as_), [xs, as_], dy)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = fn(xs, as_)
        dx, da = torch.autograd.grad(y, [xs, as_], dy)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(first, (y.detach(), dx, da)))


def test_addend_gradient_is_skipped_when_not_needed_and_trainable_gamma_takes_the_stock_path():
    N, C, G, H = 2, 320, 32, 16
    x, a, w, b, dy = _inputs(N, C, H, torch.float16, False, 9)
    # addend without requires_grad: same y and dx as with it
    xs = x.clone().requires_grad_(True)
    y = group_norm_act(xs, G, w, b, 1e-5, True, a)
    (dx,) = torch.autograd.grad(y, [xs], dy)
    full = _run(lambda xx, aa: group_norm_act(xx, G, w, b, 1e-5, True, aa), x, a, dy)
    assert torch.equal(y.detach(), full[0]) and torch.equal(dx, full[1])
    # γ requires grad → the stock composite, gradients of γ and β included
    wg, bg = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    assert _hip_layout(x, G, wg, bg, a) is None
    xs = x.clone().requires_grad_(True)
    got = group_norm_act(xs, G, wg, bg, 1e-5, True, a)
    want = F.silu(F.group_norm(xs + a[:, :, None, None], G, wg, bg, 1e-5))
    assert torch.equal(got, want)
    for u, v in zip(torch.autograd.grad(got, [xs, wg, bg], dy), torch.autograd.grad(want, [xs, wg, bg], dy)):
        assert torch.equal(u, v)
    # fp32 and odd strides keep the stock path too
    assert _hip_layout(x.float(), G, w.float(), b.float(), None) is None
    assert _hip_layout(x[:, :, ::2], G, w, b, None) is None
