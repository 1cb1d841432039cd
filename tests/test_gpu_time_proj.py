"""The batched time-embedding projections (csrc/time_proj.hip, diffusion_finetuning_amd.time_proj.time_projections) against
float64 on the same stored 16-bit inputs, at the kernel's lane, pass, row-group, layer-boundary and per-launch edges.

Per-element bound, in the form of tests/test_gpu_conv_small.py: with S = Σ_e |w|·|silu(t)| + |b| + |cb|,
    |out − ref| <= u·|ref| + 2·(E + 2)·2⁻²⁴·S + Σ_e |w|·δ(t) + tiny,
one output rounding (u = 2⁻¹¹ f16, 2⁻⁸ bf16), worst-case fp32 summation of E + 2 terms, and the error of the kernel's fp32 silu:
the kernel evaluates x · rcp(1 + exp2(−log2(e)·x)) with the 1-ulp hardware exp2 and rcp, so (header of csrc/time_proj.hip)
    δ(x) = (|x| + 3)·2⁻²³·|silu(x)| + 1e-30.
Yardstick (tests/test_gpu_trunk_edges.py): max and rms error no worse than the stock composite's
`F.linear(F.silu(t), w, b) + cb` on the same inputs, plus one ulp of the storage type at the output's magnitude.
Every figure is printed before it is asserted."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import time_proj as tp

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
EPS = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}

ES = (8, 40, 128, 1280, 1288)  # fewer chunks than lanes, a ragged lane pass, the tiny UNet's width, the real one, ragged past it
NS = (1, 2, 3, 4, 8, 16)
MIXED = [320, 320, 640, 5, 640, 1280, 33, 1280, 1280, 1280, 16, 1280, 1280, 1280, 1, 1280, 640, 640, 640, 320, 320, 320]
LISTS = {"one": [5], "boundary": [5, 32, 70], "mixed22": MIXED, "cap33": [3] * 33}


def _case(widths, N, E, dtype, seed, scale=1.5):
    """t [N, E] and per layer (w, b, cb); the projection's bias is missing in every third layer, the extra bias in every
    fourth, both in the twelfth."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    t = (scale * rn(N, E)).to(dtype)
    layers = []
    for i, c in enumerate(widths):
        w, b, cb = (rn(c, E) / math.sqrt(E)).to(dtype), (0.5 * rn(c)).to(dtype), (0.5 * rn(c)).to(dtype)
        layers.append((w, None if i % 3 == 2 else b, None if i % 4 == 3 else cb))
    return t, layers


def _stock(t, layers):
    outs = []
    for w, b, cb in layers:
        h = F.linear(F.silu(t), w, b)
        outs.append(h if cb is None else h + cb)
    return outs


def _ref64(t, layers):
    """Per layer (ref, bound without the output rounding) in float64."""
    x = t.double()
    s = x / (1 + torch.exp(-x))
    delta = (x.abs() + 3) * 2.0 ** -23 * s.abs() + 1e-30
    E = t.shape[1]
    out = []
    for w, b, cb in layers:
        w64 = w.double()
        ref, S = s @ w64.T, s.abs() @ w64.abs().T
        for v in (b, cb):
            if v is not None:
                ref, S = ref + v.double(), S + v.double().abs()
        out.append((ref, 2.0 * (E + 2) * 2.0 ** -24 * S + delta @ w64.abs().T))
    return out


def _check(tag, got, stock, refs, dtype):
    worst, sq_new, sq_old, mx_new, mx_old, mag, n = 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0
    for o, s, (ref, slack) in zip(got, stock, refs):
        assert o.shape == ref.shape and o.dtype == dtype
        err, old = (o.double() - ref).abs(), (s.double() - ref).abs()
        worst = max(worst, (err / (U[dtype] * ref.abs() + slack + TINY[dtype])).max().item())
        sq_new, sq_old, n = sq_new + err.pow(2).sum().item(), sq_old + old.pow(2).sum().item(), n + err.numel()
        mx_new, mx_old, mag = max(mx_new, err.max().item()), max(mx_old, old.max().item()), max(mag, ref.abs().max().item())
    ulp = EPS[dtype] * 2.0 ** math.floor(math.log2(mag)) if mag > 0 else 0.0
    rms_new, rms_old = math.sqrt(sq_new / n), math.sqrt(sq_old / n)
    print(f"{tag}: error/bound {worst:.3f} | new max {mx_new:.3e} rms {rms_new:.3e} | composite max {mx_old:.3e} rms {rms_old:.3e} "
          f"| ulp {ulp:.3e}")
    assert worst <= 1.0, (tag, "error / bound", worst)
    assert mx_new <= mx_old + ulp and rms_new <= rms_old + ulp, (tag, mx_new, mx_old, rms_new, rms_old, ulp)


def _spy(monkeypatch):
    calls = []
    real = nat.time_proj_all

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(nat, "time_proj_all", spy)
    return calls


def _captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs = fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph, outs


# first in the file: in the order pytest runs a file, the capture below is the first use of the kernel in the process
def test_a_call_captured_first_with_nothing_run_before_works():
    t, layers = _case(LISTS["cap33"] + [70], 4, 1288, torch.bfloat16, 1)
    assert tp.time_projections_supported(t, layers)
    graph, outs = _captured(lambda: tp.time_projections(t, layers))
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _check("captured first", outs, _stock(t, layers), _ref64(t, layers), torch.bfloat16)


@DTYPES
@pytest.mark.parametrize("E", ES)
def test_every_shape_and_layer_list_against_float64_and_the_composite(E, dtype, monkeypatch):
    calls = _spy(monkeypatch)
    for N in NS:
        for name, widths in LISTS.items():
            t, layers = _case(widths, N, E, dtype, 100 * N + E)
            outs = tp.time_projections(t, layers)
            base = outs[0].data_ptr()
            off = 0
            for o, c in zip(outs, widths):  # views of one allocation, layer l a dense [N, C_l] block behind the earlier ones
                assert o.shape == (N, c) and o.is_contiguous() and o.data_ptr() == base + 2 * off
                off += N * c
            _check(f"E={E} N={N} {name} {dtype}", outs, _stock(t, layers), _ref64(t, layers), dtype)
    assert len(calls) == len(NS) * len(LISTS)  # every case ran on the kernel


@DTYPES
def test_large_inputs_give_no_nan(dtype):
    N, E = 4, 128
    t, layers = _case([5, 32, 70], N, E, dtype, 9)
    t = torch.where(torch.arange(N * E, device=DEV).view(N, E) % 2 == 0, 30.0, -30.0).to(dtype)
    t[0, :8] = torch.tensor([-60.0, -88.0, -100.0, -300.0, 60.0, 100.0, 300.0, 0.0], device=DEV).to(dtype)
    outs = tp.time_projections(t, layers)
    assert all(torch.isfinite(o).all() for o in outs)
    _check(f"±30 {dtype}", outs, _stock(t, layers), _ref64(t, layers), dtype)


@DTYPES
def test_outside_the_envelope_the_stock_composite_runs_bit_for_bit(dtype, monkeypatch):
    calls = _spy(monkeypatch)
    for N, E in ((17, 128), (4, 12)):
        t, layers = _case([5, 32, 70], N, E, dtype, 4)
        assert not tp.time_projections_supported(t, layers)
        assert all(torch.equal(a, b) for a, b in zip(tp.time_projections(t, layers), _stock(t, layers)))
    t, layers = _case([5, 32, 70], 4, 128, dtype, 4)
    assert tp.time_projections_supported(t, layers)
    w0 = layers[0][0]
    for bad_t, bad_layers in ((t.clone().requires_grad_(True), layers),               # temb in the graph
                              (t, [(w0.clone().requires_grad_(True),) + layers[0][1:]] + layers[1:]),  # a trainable weight
                              (t, [(w0.float(),) + layers[0][1:]] + layers[1:]),     # another dtype
                              (t.t().contiguous().t(), layers),                      # not contiguous
                              (t, [(w0.cpu(),) + layers[0][1:]] + layers[1:])):      # another device
        assert not tp.time_projections_supported(bad_t, bad_layers)
    assert not calls
    ts = t.clone().requires_grad_(True)
    out = tp.time_projections(ts, layers)
    want = _stock(ts, layers)
    assert torch.equal(out[1], want[1])
    dy = torch.ones_like(out[1])
    assert torch.equal(torch.autograd.grad(out[1], ts, dy)[0], torch.autograd.grad(want[1], ts, dy)[0]) and not calls


@DTYPES
def test_two_calls_and_a_replayed_capture_give_the_same_bits(dtype):
    t, layers = _case(MIXED, 4, 1280, dtype, 6)
    a, b = tp.time_projections(t, layers), tp.time_projections(t, layers)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    graph, outs = _captured(lambda: tp.time_projections(t, layers))
    for o in outs:
        o.zero_()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(outs, a))


@DTYPES
@pytest.mark.parametrize("N,E,name", [(3, 40, "boundary"), (4, 1288, "cap33"), (16, 1280, "mixed22"), (1, 8, "one")])
def test_the_kernel_writes_only_inside_out(N, E, name, dtype):
    """out sits inside a canary-filled buffer, at an offset that is no multiple of 16 bytes; t, the weights and the biases sit in
    canary-filled buffers too.  Every canary is intact afterwards, the inputs are unchanged and every element of out is written."""
    widths = LISTS[name]
    t, layers = _case(widths, N, E, dtype, 8)
    pad, canary = 4096, torch.tensor(-1234.0, dtype=dtype).item()

    def framed(src=None, n=None, shift=0):
        n = src.numel() if n is None else n
        buf = torch.full((n + 2 * pad + shift,), canary, dtype=dtype, device=DEV)
        view = buf[pad + shift:pad + shift + n]
        if src is not None:
            view.copy_(src.flatten())
        return buf, view

    frames, ptr_rows = [], []
    tbuf, tv = framed(t)
    frames.append((tbuf, tv, t))
    for w, b, cb in layers:
        row = []
        for v in (w, b, cb):
            if v is None:
                row.append(None)
                continue
            buf, view = framed(v)
            frames.append((buf, view, v))
            row.append(view.data_ptr())
        ptr_rows.append(row)
    total = N * sum(widths)
    obuf, ov = framed(n=total, shift=3)
    L = len(widths)
    col = lambda j: (ctypes.c_void_p * L)(*[r[j] for r in ptr_rows])
    st = nat.lib().time_proj_all(tv.data_ptr(), col(0), col(1), col(2), (ctypes.c_int * L)(*widths), ov.data_ptr(), L, N, E,
                                 nat.dtype_code(dtype), nat._stream(t))
    assert st == 0
    torch.cuda.synchronize()
    for buf, view, src in frames:
        assert (buf[:pad] == canary).all() and (buf[-pad:] == canary).all() and torch.equal(view, src.flatten())
    assert (obuf[:pad + 3] == canary).all() and (obuf[-pad:] == canary).all() and not (ov == canary).any()
    want = torch.cat([o.flatten() for o in tp.time_projections(t, layers)])
    assert torch.equal(ov, want)


def test_tiny_unet_forward_with_the_batched_call_is_no_worse_than_with_per_block_projections(monkeypatch):
    import copy

    import harness.unet as hu

    torch.manual_seed(12)
    ref = hu.UNet2DConditionModel(hu.tiny_config(32, 32, 2)).requires_grad_(False)
    g = torch.Generator().manual_seed(13)
    sample, ctx, steps = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 6, 32, generator=g), torch.tensor([3, 700])
    unet = copy.deepcopy(ref).half().to(DEV)
    ref64 = copy.deepcopy(unet).cpu().double()  # float64 on the stored f16 weights
    s16, c16 = sample.half(), ctx.half()
    want = ref64(s16.double(), steps, c16.double()).sample

    calls = _spy(monkeypatch)
    new = unet(s16.to(DEV), steps.to(DEV), c16.to(DEV)).sample
    assert len(calls) == 1  # one batched call for every ResNet of the model
    monkeypatch.setattr(hu.UNet2DConditionModel, "_time_addends", staticmethod(lambda temb, blocks: {}))
    old = unet(s16.to(DEV), steps.to(DEV), c16.to(DEV)).sample
    assert len(calls) == 1
    (nmax, nrms), (omax, orms) = [((o.double().cpu() - want).abs().max().item(),
                                   (o.double().cpu() - want).pow(2).mean().sqrt().item()) for o in (new, old)]
    ulp = EPS[torch.float16] * 2.0 ** math.floor(math.log2(want.abs().max().item()))
    print(f"tiny UNet f16: batched max {nmax:.3e} rms {nrms:.3e} | per block max {omax:.3e} rms {orms:.3e} | ulp {ulp:.3e}")
    assert nmax <= omax + ulp and nrms <= orms + ulp
