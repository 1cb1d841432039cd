"""The block-edge passes of csrc/trunk_edges.hip and the `dh` operand of the NCHW GroupNorm backward (csrc/norm.hip) through
their fronts in diffusion_finetuning_amd.norm and through harness/unet.py.

Yardstick (tests/test_gpu_norm.py): float64 math on the same stored inputs is the reference, and the lines each front replaces,
run in the same dtype on the GPU, are the parent's composite.  The new path's maximum and RMS error may exceed the composite's
by at most one unit in the last place of the storage type at the output's magnitude.  Where a front only moves data, or adds
two stored values, its bits must equal the composite's.  Every figure is printed before it is asserted."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import norm as dnorm
from diffusion_finetuning_amd.norm import (group_norm_act, group_norm_act_res, group_norm_tokens, group_norm_tokens_supported,
                                           residual_bias_add, tokens_to_nchw_add, tokens_to_nchw_add_supported)

pytestmark = pytest.mark.gpu

# (N, C, groups, H, W)
RAGGED = [(2, 320, 32, 8, 8), (3, 40, 4, 2, 12), (2, 64, 8, 6, 12), (1, 1280, 32, 4, 4), (2, 96, 8, 16, 16)]
MODEL = [(1, 320, 32, 64, 64), (1, 640, 32, 32, 32), (1, 1280, 32, 16, 16), (1, 1280, 32, 8, 8)]
SHAPES = RAGGED + MODEL
UNSUPPORTED = [(2, 16, 4, 3, 3), (2, 12, 4, 4, 4)]
IDS = lambda s: "n%d-c%d-g%d-h%d-w%d" % s
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
EPS = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}
EPS_ENTRY, EPS_RESNET = 1e-6, 1e-5
E_ALIGN = -3


def _inputs(shape, dtype, seed):
    N, C, G, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    x = (rn(N, C, H, W) * (0.5 + rn(1, C, 1, 1).abs()) + rn(1, C, 1, 1)).to(dtype)  # per-channel spread and offset
    a = (0.5 * rn(N, C)).to(dtype)
    w, b = (1 + 0.2 * rn(C)).to(dtype), (0.2 * rn(C)).to(dtype)
    dy, dh = rn(N, C, H, W).to(dtype), rn(N, C, H, W).to(dtype)
    return x, a, w, b, dy, dh


def _to_tokens(t):
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n, h * w, c)


def _ulp(ref, dtype):
    m = ref.abs().max().item()
    return EPS[dtype] * 2.0 ** math.floor(math.log2(m)) if m > 0 else 0.0


def _errs(t, ref):
    d = t.double() - ref
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


def _yardstick(tag, new, stock, ref, dtype):
    (fmax, frms), (smax, srms), ulp = _errs(new, ref), _errs(stock, ref), _ulp(ref, dtype)
    print(f"{tag}: new max {fmax:.3e} rms {frms:.3e} | composite max {smax:.3e} rms {srms:.3e} | ulp {ulp:.3e}")
    assert fmax <= smax + ulp, (tag, fmax, smax, ulp)
    assert frms <= srms + ulp, (tag, frms, srms, ulp)


def _grads(fn, ins, gouts):
    """Outputs and input gradients of fn(*ins) -> tuple, with the upstream gradients gouts (None: that output gets none)."""
    ins = [None if t is None else t.detach().clone().requires_grad_(True) for t in ins]
    outs = fn(*ins)
    pairs = [(o, g) for o, g in zip(outs, gouts) if g is not None]
    grads = torch.autograd.grad([o for o, _ in pairs], [t for t in ins if t is not None], [g.to(o.dtype) for o, g in pairs])
    return [o.detach() for o in outs], list(grads)


def _entry_composite(G, w, b, eps):
    """The parent's transformer entry: x feeds the norm and the residual, autograd adds the two gradients (float64: stock math)."""
    def fn(x):
        h = F.group_norm(x, G, w, b, eps) if x.dtype == torch.float64 else group_norm_act(x, G, w, b, eps, False)
        return x.view_as(x), _to_tokens(h)
    return fn


def _res_composite(G, w, b, eps, act):
    """The parent's ResNet head: x feeds norm1 and the shortcut (float64: stock math)."""
    def fn(x, a=None):
        if x.dtype != torch.float64:
            return x.view_as(x), group_norm_act(x, G, w, b, eps, act, a)
        h = F.group_norm(x if a is None else x + a[:, :, None, None], G, w, b, eps)
        return x.view_as(x), (F.silu(h) if act else h)
    return fn


# ------------------------------------------------------------------------------------------------------ 1. bit equality
@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fronts_that_move_or_pass_data_equal_the_composite_bit_for_bit(shape, dtype):
    N, C, G, H, W = shape
    x, a, w, b, dy, dh = _inputs(shape, dtype, 11)
    assert group_norm_tokens_supported(x, G, w, b)
    # entry forward: the norm's bits in token layout, and x itself handed through
    xp, tok = group_norm_tokens(x, G, w, b, EPS_ENTRY)
    assert tok.shape == (N, H * W, C) and tok.is_contiguous()
    assert torch.equal(tok, _to_tokens(group_norm_act(x, G, w, b, EPS_ENTRY, False))) and xp.data_ptr() == x.data_ptr()
    # exit forward and backward
    t_in = _to_tokens(dh).contiguous()
    assert tokens_to_nchw_add_supported(t_in, x)
    (out,), (d_tok, d_res) = _grads(lambda t, r: (tokens_to_nchw_add(t, r),), [t_in, x], [dy])
    assert torch.equal(out, t_in.view(N, H, W, C).permute(0, 3, 1, 2).contiguous() + x)
    assert torch.equal(d_tok, _to_tokens(dy)) and d_tok.is_contiguous() and torch.equal(d_res, dy)
    # group_norm_act_res without a gradient into x_pass: group_norm_act's y and dx; the old entry point is unchanged
    for act, eps in ((True, EPS_RESNET), (False, EPS_ENTRY)):
        (_, y), (dx,) = _grads(lambda xx: group_norm_act_res(xx, G, w, b, eps, act), [x], [None, dy])
        (y0,), (dx0,) = _grads(lambda xx: (group_norm_act(xx, G, w, b, eps, act),), [x], [dy])
        assert torch.equal(y, y0) and torch.equal(dx, dx0), act
    # residual_bias_add hands the very dy to both branches
    hs, rs = x.clone().requires_grad_(True), dh.clone().requires_grad_(True)
    gh, gr = torch.autograd.grad(residual_bias_add(hs, rs, b, w), [hs, rs], dy)
    assert gh.data_ptr() == dy.data_ptr() and gr.data_ptr() == dy.data_ptr()


# --------------------------------------------------------------------------------------------------- 2. error yardstick
@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_entry_backward_is_no_worse_than_the_composite_against_float64(shape, dtype):
    N, C, G, H, W = shape
    x, a, w, b, dy, dh = _inputs(shape, dtype, 23)
    dtok = _to_tokens(dy).contiguous()
    for with_dh in (False, True):
        gouts = [dh if with_dh else None, dtok]
        _, (ref,) = _grads(_entry_composite(G, w.double(), b.double(), EPS_ENTRY), [x.double()],
                           [None if g is None else g.double() for g in gouts])
        _, (stock,) = _grads(_entry_composite(G, w, b, EPS_ENTRY), [x], gouts)
        _, (new,) = _grads(lambda xx: group_norm_tokens(xx, G, w, b, EPS_ENTRY), [x], gouts)
        assert new.is_contiguous()
        _yardstick(f"{shape} {dtype} entry dx dh={int(with_dh)}", new, stock, ref, dtype)


@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_norm_backward_with_dh_is_no_worse_than_the_composite_against_float64(shape, dtype):
    N, C, G, H, W = shape
    x, a, w, b, dy, dh = _inputs(shape, dtype, 37)
    for act in (True, False):
        for with_a in (True, False):
            ins = [x, a] if with_a else [x]
            _, ref = _grads(_res_composite(G, w.double(), b.double(), EPS_RESNET, act), [t.double() for t in ins],
                            [dh.double(), dy.double()])
            _, stock = _grads(_res_composite(G, w, b, EPS_RESNET, act), ins, [dh, dy])
            _, new = _grads(lambda *t: group_norm_act_res(t[0], G, w, b, EPS_RESNET, act, *t[1:]), ins, [dh, dy])
            for name, f, s, r in zip(("dx", "da"), new, stock, ref):
                _yardstick(f"{shape} {dtype} act={int(act)} a={int(with_a)} {name}", f, s, r, dtype)


@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_residual_bias_add_is_no_worse_than_the_composite_against_float64(shape, dtype):
    N, C, G, H, W = shape
    h, _, b1, b2, res, _ = _inputs(shape, dtype, 41)
    v = lambda t: t.double()[None, :, None, None]
    for two in (False, True):
        ref = res.double() + h.double() + v(b1) + (v(b2) if two else 0.0)
        # the parent's lines: each convolution's output with its bias rounded, then the sum of the two branches
        stock = (res + b2[None, :, None, None] if two else res) + (h + b1[None, :, None, None])
        new = residual_bias_add(h, res, b1, b2 if two else None)
        assert new.is_contiguous() and new.shape == h.shape
        _yardstick(f"{shape} {dtype} residual_bias_add biases={1 + int(two)}", new, stock, ref, dtype)


# ------------------------------------------------------------------------------------------------------------ 3. bounds
GUARD, SENTINEL = 4096, 0xA5


class _Guarded:
    """`nbytes` of device memory that start on a 16-byte boundary, between two guards of ≥ GUARD bytes; all filled with SENTINEL."""

    def __init__(self, nbytes, dtype, src=None):
        self.buf = torch.full((2 * GUARD + nbytes + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.lo = GUARD + (-(self.buf.data_ptr() + GUARD)) % 16
        self.hi = self.lo + nbytes
        self.t = self.buf[self.lo:self.hi].view(dtype)
        assert self.t.data_ptr() % 16 == 0 and self.lo >= GUARD and self.buf.numel() - self.hi >= GUARD
        if src is not None:
            self.t.copy_(src.reshape(-1))

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.hi:] == SENTINEL).all())


@DTYPES
@pytest.mark.parametrize("shape", RAGGED, ids=IDS)
def test_kernels_write_only_inside_their_tensors_and_the_workspace_formula_covers_them(shape, dtype):
    """The new C entry points called as _native calls them, every operand inside a larger sentinel-filled buffer and the
    workspace exactly group_norm_act_workspace_bytes long: the plain calls' bits, inputs unchanged, no guard byte changed."""
    N, C, G, H, W = shape
    HW, code, size = H * W, nat.dtype_code(dtype), 2
    x, a, w, b, dy, dh = _inputs(shape, dtype, 53)
    lib, stream, nb = nat.lib(), nat._stream(x), x.numel() * size
    G_ = lambda src=None, n=nb, dt=dtype: _Guarded(n, dt, src)
    tok = _to_tokens(dy).contiguous()
    gx, gdy, gdh, gtok = G_(x), G_(dy), G_(dh), G_(tok)
    ga, gw, gb = G_(a, N * C * size), G_(w, C * size), G_(b, C * size)
    outs = {k: G_() for k in ("sum1", "sum2", "nchw", "nchw_add", "tokens", "dx")}
    gda = G_(None, N * C * size)
    assert lib.residual_bias_add(gx.ptr(), gdh.ptr(), gw.ptr(), None, outs["sum1"].ptr(), N, C, HW, code, stream) == 0
    assert lib.residual_bias_add(gx.ptr(), gdh.ptr(), gw.ptr(), gb.ptr(), outs["sum2"].ptr(), N, C, HW, code, stream) == 0
    assert lib.tokens_to_nchw_add(gtok.ptr(), None, outs["nchw"].ptr(), N, C, HW, code, stream) == 0
    assert lib.tokens_to_nchw_add(gtok.ptr(), gx.ptr(), outs["nchw_add"].ptr(), N, C, HW, code, stream) == 0
    assert lib.nchw_to_tokens(gx.ptr(), outs["tokens"].ptr(), N, C, HW, code, stream) == 0
    y0, mean, rstd = nat.group_norm_act_fwd(x, a, w, b, G, EPS_RESNET, True, 0)
    ws = lib.group_norm_act_workspace_bytes(N, C, HW, G, 0, 1)
    assert ws > 0 and ws % 16 == 0
    gws = _Guarded(ws, torch.uint8)
    gmean, grstd = _Guarded(N * G * 4, torch.float32, mean), _Guarded(N * G * 4, torch.float32, rstd)
    assert lib.group_norm_act_bwd_res(gdy.ptr(), gdh.ptr(), gx.ptr(), ga.ptr(), gw.ptr(), gb.ptr(), gmean.ptr(), grstd.ptr(),
                                      outs["dx"].ptr(), gda.ptr(), gws.ptr(), N, C, HW, G, 1, code, stream) == 0
    torch.cuda.synchronize()
    dx0, da0 = nat.group_norm_act_bwd_res(dy, dh, x, a, w, b, mean, rstd, G, True, True)
    want = {"sum1": nat.residual_bias_add(x, dh, w, None), "sum2": nat.residual_bias_add(x, dh, w, b), "nchw": dy,
            "nchw_add": nat.tokens_to_nchw_add(tok, x, x.shape), "tokens": nat.nchw_to_tokens(x), "dx": dx0}
    assert torch.equal(want["nchw"], nat.tokens_to_nchw_add(tok, None, x.shape)) and torch.equal(want["tokens"], _to_tokens(x))
    for k, g in outs.items():
        assert torch.equal(g.t, want[k].reshape(-1)), k
    assert torch.equal(gda.t, da0.reshape(-1))
    for g, src in ((gx, x), (gdy, dy), (gdh, dh), (gtok, tok), (ga, a), (gw, w), (gb, b), (gmean, mean), (grstd, rstd)):
        assert torch.equal(g.t, src.reshape(-1))
    for name, g in list(outs.items()) + [("x", gx), ("dy", gdy), ("dh", gdh), ("tok", gtok), ("a", ga), ("gamma", gw),
                                         ("beta", gb), ("da", gda), ("mean", gmean), ("rstd", grstd), ("workspace", gws)]:
        assert g.guards_intact(), name


# ------------------------------------------------------------------------------------ 4. determinism and graph replay
def _chain(G, w, b):
    """A ResNet-shaped and a transformer-shaped use of all four fronts, one after the other."""
    def fn(x, a):
        xp, n = group_norm_act_res(x, G, w, b, EPS_RESNET, True, a)
        s = residual_bias_add(n, xp, b, w)
        res, tok = group_norm_tokens(s, G, w, b, EPS_ENTRY)
        return tokens_to_nchw_add(tok * 0.5, res)
    return fn


@pytest.mark.parametrize("shape", [(3, 40, 4, 2, 12), (2, 96, 8, 16, 16), (1, 320, 32, 64, 64)], ids=IDS)
def test_two_runs_are_bit_identical_and_a_graph_replay_equals_eager(shape):
    N, C, G, H, W = shape
    x, a, w, b, dy, _ = _inputs(shape, torch.float16, 7)
    fn = _chain(G, w, b)

    def run():
        xs, as_ = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
        y = fn(xs, as_)
        return [y.detach(), *torch.autograd.grad(y, [xs, as_], dy)]

    first, second = run(), run()
    assert all(torch.equal(u, v) for u, v in zip(first, second))

    xs, as_ = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
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


# ------------------------------------------------------------------------------------------------------------ 5. fronts
def _views(t):
    """t as every other column of a wider tensor, and as a dense tensor 2 bytes into its storage."""
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device="cuda")
    wide[..., ::2] = t
    store = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
    odd = store[1:1 + t.numel()].view(t.shape).copy_(t)
    assert not wide[..., ::2].is_contiguous() and odd.data_ptr() % 16 == 2
    return wide[..., ::2], odd


def test_a_gradient_into_one_output_only_and_strided_or_misaligned_gradients(monkeypatch):
    shape = (2, 64, 8, 6, 12)
    N, C, G, H, W = shape
    x, a, w, b, dy, dh = _inputs(shape, torch.bfloat16, 61)
    dtok = _to_tokens(dy).contiguous()
    calls = []
    real = nat.group_norm_act_bwd_res
    monkeypatch.setattr(nat, "group_norm_act_bwd_res", lambda *t: calls.append(1) or real(*t))
    for fn, gy in ((lambda xx: group_norm_act_res(xx, G, w, b, EPS_RESNET, True), dy),
                   (lambda xx: group_norm_tokens(xx, G, w, b, EPS_ENTRY), dtok)):
        xs = x.clone().requires_grad_(True)
        xp, y = fn(xs)
        (gx,) = torch.autograd.grad([xp], [xs], [dh], retain_graph=True)  # into x_pass only: no launch, the same tensor back
        assert not calls and gx.data_ptr() == dh.data_ptr()
        (gx,) = torch.autograd.grad([y], [xs], [gy], retain_graph=True)  # into y only
        assert len(calls) == 1
        calls.clear()
        want = _grads(fn, [x], [None, gy])[1][0]
        assert torch.equal(gx, want)
        # dh / dy as views give the bits of the dense aligned ones
        want = _grads(fn, [x], [dh, gy])[1][0]
        (sh, oh), (sy, oy) = _views(dh), _views(gy)
        assert torch.equal(_grads(fn, [x], [sh, oy])[1][0], want) and torch.equal(_grads(fn, [x], [oh, sy])[1][0], want)
        calls.clear()
    # the exit's dy likewise
    fn = lambda t, r: (tokens_to_nchw_add(t, r),)
    want = _grads(fn, [dtok, x], [dy])[1]
    for v in _views(dy):
        got = _grads(fn, [dtok, x], [v])[1]
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # without requires_grad nothing is recorded
    for out in (*group_norm_act_res(x, G, w, b, EPS_RESNET, True), *group_norm_tokens(x, G, w, b, EPS_ENTRY),
                tokens_to_nchw_add(dtok, x), residual_bias_add(x, dh, b, w)):
        assert not out.requires_grad and out.grad_fn is None


def _stock_fronts(x, a, w, b, G, tok, other):
    """What each front must return, bit for bit, for operands the kernels do not take."""
    N, C, H, W = x.shape
    gn = lambda eps, act, add=None: group_norm_act(x, G, w, b, eps, act, add)
    return [gn(EPS_RESNET, True, a), _to_tokens(gn(EPS_ENTRY, False)),
            tok.reshape(N, H, W, C).permute(0, 3, 1, 2).contiguous() + x,
            (other + b[None, :, None, None]) + (x + w[None, :, None, None])]


def test_operands_the_kernels_do_not_take_get_the_stock_composite_bit_for_bit(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a new kernel was reached")

    shape = (2, 64, 8, 6, 12)
    N, C, G, H, W = shape
    x, a, w, b, dy, dh = _inputs(shape, torch.float16, 67)
    tok = _to_tokens(dy).contiguous()
    store = torch.zeros(x.numel() + 8, dtype=x.dtype, device="cuda")
    x_odd = store[1:1 + x.numel()].view(x.shape).copy_(x)
    x_cl = x.contiguous(memory_format=torch.channels_last)
    # which fronts each case is outside of: 0 group_norm_act_res, 1 group_norm_tokens, 2 tokens_to_nchw_add, 3 residual_bias_add.
    # A channels-last x has no NCHW tensor beside it for the exit or the tail; C = 12 with H·W = 16 is outside the re-layouts only
    cases = [("2 bytes off", x_odd, w, b, G, dh, (0, 1, 2, 3)), ("channels-last", x_cl, w, b, G, dh, (0, 1))]
    for s, fronts in zip(UNSUPPORTED, ((0, 1, 2, 3), (1, 2))):
        xs, as_, ws_, bs_, dys, dhs = _inputs(s, torch.float16, 71)
        cases.append((str(s), xs, ws_, bs_, s[2], dhs, fronts))
    for tag, xx, ww, bb, gg, other, fronts in cases:
        aa = (0.5 * torch.randn(xx.shape[:2], device="cuda")).to(xx.dtype)
        tt = _to_tokens(other).contiguous()
        want = _stock_fronts(xx, aa, ww, bb, gg, tt, other)
        with monkeypatch.context() as mp:
            for name in ("group_norm_act_bwd_res", "residual_bias_add", "tokens_to_nchw_add", "nchw_to_tokens"):
                mp.setattr(nat, name, boom)
            got = {0: lambda: group_norm_act_res(xx, gg, ww, bb, EPS_RESNET, True, aa), 1: lambda: group_norm_tokens(xx, gg, ww, bb, EPS_ENTRY),
                   2: lambda: tokens_to_nchw_add(tt, xx), 3: lambda: residual_bias_add(xx, other, ww, bb)}
            for i in fronts:
                out = got[i]()
                if i < 2:
                    assert out[0] is xx, (tag, i)  # the composite hands x itself on
                    out = out[1]
                assert torch.equal(out, want[i]), (tag, i)
    # trainable γ or bias: the stock composite with their gradients; a trainable conv bias: the stock sum
    wg, bg = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    for p, q in ((wg, b), (w, bg)):
        xp, y = group_norm_act_res(x, G, p, q, EPS_RESNET, True)
        assert xp is x and torch.equal(y, F.silu(F.group_norm(x, G, p, q, EPS_RESNET))) and y.requires_grad
        xp, t = group_norm_tokens(x, G, p, q, EPS_ENTRY)
        assert xp is x and torch.equal(t, _to_tokens(F.group_norm(x, G, p, q, EPS_ENTRY))) and t.requires_grad
        s = residual_bias_add(x, dh, p, q)
        assert torch.equal(s, (dh + q[None, :, None, None]) + (x + p[None, :, None, None])) and s.requires_grad


def test_raw_entry_points_refuse_a_pointer_two_bytes_off_before_any_launch():
    shape = (2, 64, 8, 6, 12)
    N, C, G, H, W = shape
    x, a, w, b, dy, dh = _inputs(shape, torch.float16, 73)
    lib, code, HW, stream = nat.lib(), nat.dtype_code(torch.float16), H * W, nat._stream(x)
    out = torch.full_like(x, 7.0)
    p, o = (lambda t: t.data_ptr()), (lambda t: t.data_ptr() + 2)
    y, mean, rstd = nat.group_norm_act_fwd(x, a, w, b, G, EPS_RESNET, True, 0)
    ws = nat._norm_workspace(x, G, 0, True)
    sts = [lib.residual_bias_add(o(x), p(dh), p(w), p(b), p(out), N, C, HW, code, stream),
           lib.residual_bias_add(p(x), o(dh), p(w), p(b), p(out), N, C, HW, code, stream),
           lib.residual_bias_add(p(x), p(dh), p(w), p(b), o(out), N, C, HW, code, stream),
           lib.tokens_to_nchw_add(o(dy), p(x), p(out), N, C, HW, code, stream),
           lib.tokens_to_nchw_add(p(dy), o(x), p(out), N, C, HW, code, stream),
           lib.tokens_to_nchw_add(p(dy), None, o(out), N, C, HW, code, stream),
           lib.nchw_to_tokens(o(x), p(out), N, C, HW, code, stream),
           lib.nchw_to_tokens(p(x), o(out), N, C, HW, code, stream),
           lib.group_norm_act_bwd_res(p(dy), o(dh), p(x), p(a), p(w), p(b), p(mean), p(rstd), p(out), None, p(ws), N, C, HW, G, 1,
                                      code, stream),
           lib.group_norm_act_bwd_res(o(dy), p(dh), p(x), p(a), p(w), p(b), p(mean), p(rstd), p(out), None, p(ws), N, C, HW, G, 1,
                                      code, stream)]
    torch.cuda.synchronize()
    assert sts == [E_ALIGN] * len(sts), sts
    assert bool((out == 7.0).all())  # nothing was launched
    # shapes and dtypes are judged before the pointers
    assert lib.nchw_to_tokens(o(x), p(out), N, 12, HW, code, stream) == -5
    assert lib.residual_bias_add(o(x), p(dh), p(w), None, p(out), N, C, 9, code, stream) == -5
    assert lib.tokens_to_nchw_add(p(dy), None, p(out), N, C, HW, 0, stream) == -5


# ----------------------------------------------------------------------------------------------------------- 6. harness
def _spy_fronts(monkeypatch):
    counts = {"group_norm_act_res": 0, "group_norm_tokens": 0, "tokens_to_nchw_add": 0, "residual_bias_add": 0}

    def spy(name):
        real = getattr(dnorm, name)

        def call(*a, **k):
            counts[name] += 1
            return real(*a, **k)
        return call

    for name in counts:
        monkeypatch.setattr(dnorm, name, spy(name))
    return counts


def _module_yardstick(tag, mod, args, counts, want_counts, monkeypatch):
    """Output and input gradient of `mod` on the new path and with the fused paths switched off, both against a float64 copy
    of the module on the CPU."""
    import harness.unet as hu

    x = args[0]
    g = torch.Generator(device="cuda").manual_seed(5)
    dy = None

    def run(m, inputs):
        nonlocal dy
        xs = inputs[0].detach().clone().requires_grad_(True)
        out = m(xs, *inputs[1:])
        if dy is None:
            dy = torch.randn(out.shape, generator=g, device="cuda")
        (dx,) = torch.autograd.grad(out, [xs], dy.to(out.device, out.dtype))
        return out.detach(), dx

    for k in counts:
        counts[k] = 0
    new = run(mod, args)
    assert counts == want_counts, counts
    ref = run(copy.deepcopy(mod).double().cpu(), [t.double().cpu() for t in args])
    for k in counts:
        counts[k] = 0
    with monkeypatch.context() as mp:
        mp.setattr(hu, "_fused_norms", lambda t: False)
        off = run(mod, args)
    assert not any(counts.values()), counts
    for name, n, o, r in zip(("out", "dx"), new, off, ref):
        _yardstick(f"{tag} {name}", n.cpu(), o.cpu(), r, x.dtype)


def test_harness_blocks_go_through_the_fronts_on_16_bit_gpu_tensors(monkeypatch):
    import harness.unet as hu

    counts = _spy_fronts(monkeypatch)
    torch.manual_seed(31)
    temb = torch.randn(2, 128, device="cuda").half()
    for cin in (32, 64):  # with and without conv_shortcut
        blk = hu.ResnetBlock2D(cin, 64, 128, 8).cuda().half().requires_grad_(False)
        assert (blk.conv_shortcut is not None) == (cin != 64)
        x = torch.randn(2, cin, 6, 12, device="cuda").half()
        _module_yardstick(f"resnet {cin}->64", blk, [x, temb], counts,
                          {"group_norm_act_res": 1, "group_norm_tokens": 0, "tokens_to_nchw_add": 0, "residual_bias_add": 1},
                          monkeypatch)
    tr = hu.Transformer2DModel(64, 2, 48, 8, False).cuda().half().requires_grad_(False)
    x = torch.randn(2, 64, 6, 12, device="cuda").half()
    ctx = torch.randn(2, 6, 48, device="cuda").half()
    _module_yardstick("transformer", tr, [x, ctx], counts,
                      {"group_norm_act_res": 0, "group_norm_tokens": 1, "tokens_to_nchw_add": 1, "residual_bias_add": 0},
                      monkeypatch)
