"""The fused residual add + LayerNorm kernels (csrc/layer_norm.hip) against float64 math on the same stored inputs, at the
places a row-per-wave kernel can go wrong: fewer chunks than lanes, an exact lane multiple and either side of it, partial last
rounds, the widest row; rows that do not fill a workgroup or the last one.

Yardsticks (those of tests/test_gpu_norm_edges.py), every figure printed before it is asserted:
  h   bit-equal to the stock `x + delta` in the storage type;
  Y1  y and dx: maximum and RMS error ≤ the same-dtype stock composite's (`x + delta` → F.layer_norm, autograd, both upstream
      gradients fed in) + 1 ulp of the storage type at the reference's magnitude;
  Y2  the same against the stock composite run in fp32 on the upcast inputs and rounded once;
  Y3  the returned mean / rstd against float64 moments of the STORED h: |rstd/rstd₆₄ − 1| ≤ 2⁻¹³, |mean − mean₆₄|·rstd₆₄ ≤ 2⁻¹³.
The float64 reference of Y1 / Y2 is the composite on the upcast x, delta, γ, β, dy, dh (h not rounded), so with a delta the
error of y carries the rounding of h, which the kernels share bit for bit with the same-dtype stock composite and the fp32
composite of Y2 does not have: there y sits up to 0.83 ulp above the fp32 composite (measured, M = 1, C = 320, f16), inside
Y2's one ulp, and on the same-dtype stock composite's figure to three digits.

The constant row.  Its x̂ is zero, so y = β exactly and dx = rstd·(g − mean_c(g)) + dh with g = dy·γ: that is dh exactly where
g does not vary along the row (dy = 0, or γ = 1 with one dy value per row), which is what `test_constant_and_zero_rows_are_exact`
pins bit for bit; with a g that varies, dx is NOT dh in any correct LayerNorm backward, and such rows are held to Y1 / Y2
against float64 in `test_hard_rows` instead."""
import pytest
import torch
import torch.nn.functional as F

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import norm as dnorm
from diffusion_finetuning_amd.norm import _hip_layer_norm, add_layer_norm, layer_norm
from tests.test_gpu_norm import _errs, _ulp
from tests.test_gpu_norm_edges import SENTINEL, Y3_BOUND, _Guarded

pytestmark = pytest.mark.gpu

EPS = 1e-5
DTYPES = [torch.float16, torch.bfloat16]
CMAX = 2048
WIDTHS = [8, 32, 96, 320, 504, 512, 520, 640, 1280, CMAX]
ROWS = [1, 3, 63, 65, 257, 1025]


def _inputs(M, C, dtype, seed):
    """`_inputs` of test_gpu_norm.py for rows: per-channel spread and offset of order 1, γ = 1 + 0.2·n, β = 0.2·n, random dy, dh."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    x = (rn(M, C) * (0.5 + rn(1, C).abs()) + rn(1, C)).to(dtype)
    delta = (rn(M, C) * (0.5 + rn(1, C).abs()) + 0.5 * rn(1, C)).to(dtype)
    w, b = (1 + 0.2 * rn(C)).to(dtype), (0.2 * rn(C)).to(dtype)
    return x, delta, w, b, rn(M, C).to(dtype), rn(M, C).to(dtype)


def _stock(w, b, eps=EPS):
    def fn(x, delta):
        h = x if delta is None else x + delta
        return h, F.layer_norm(h, (h.shape[-1],), w, b, eps)
    return fn


def _fused(w, b, eps=EPS):
    def fn(x, delta):
        return (x, layer_norm(x, w, b, eps)) if delta is None else add_layer_norm(x, delta, w, b, eps)
    return fn


def _run(fn, x, delta, dy, dh):
    """[h, y, dx, ddelta] (without delta: [x, y, dx]); dh is fed into h where there is a delta."""
    x = x.detach().clone().requires_grad_(True)
    ins = [x]
    if delta is not None:
        delta = delta.detach().clone().requires_grad_(True)
        ins.append(delta)
    h, y = fn(x, delta)
    if delta is None:
        grads = torch.autograd.grad([y], ins, [dy.to(y.dtype)])
    else:
        grads = torch.autograd.grad([h, y], ins, [dh.to(h.dtype), dy.to(y.dtype)])
    return [h.detach(), y.detach()] + [t.detach() for t in grads]


def _check(tag, x, delta, w, b, dy, dh, bad, eps=EPS):
    """Bit equality of h, Y1 and Y2 on y and dx, Y3 on the statistics; appends every miss to `bad`.  Returns the fused results."""
    dtype = x.dtype
    assert _hip_layer_norm(x, delta, w, b), tag  # the HIP path is what is measured
    f64 = lambda t: None if t is None else t.double()
    f32 = lambda t: None if t is None else t.float()
    ref = _run(_stock(w.double(), b.double(), eps), f64(x), f64(delta), dy.double(), dh.double())
    stock = _run(_stock(w, b, eps), x, delta, dy, dh)
    stock32 = [t.to(dtype) for t in _run(_stock(w.float(), b.float(), eps), f32(x), f32(delta), dy.float(), dh.float())]
    fused = _run(_fused(w, b, eps), x, delta, dy, dh)
    if not torch.equal(fused[0], stock[0]):
        bad.append(("h", tag))
    if delta is not None and not torch.equal(fused[2], fused[3]):
        bad.append(("dx is not ddelta", tag))
    for name, i in (("y", 1), ("dx", 2)):
        f, s, s32, r = fused[i], stock[i], stock32[i], ref[i]
        assert f.shape == x.shape and f.is_contiguous() and torch.isfinite(f).all(), (tag, name)
        (fmax, frms), (smax, srms), (tmax, trms), ulp = _errs(f, r), _errs(s, r), _errs(s32, r), _ulp(r, dtype)
        print(f"{tag} {name}: fused max {fmax:.3e} rms {frms:.3e} | stock max {smax:.3e} rms {srms:.3e} | "
              f"fp32-stock max {tmax:.3e} rms {trms:.3e} | ulp {ulp:.3e}")
        if not (fmax <= smax + ulp and frms <= srms + ulp):
            bad.append(("Y1", tag, name, fmax, frms, smax, srms, ulp))
        if not (fmax <= tmax + ulp and frms <= trms + ulp):
            bad.append(("Y2", tag, name, fmax, frms, tmax, trms, ulp))
    _check_y3(tag, x, delta, w, b, bad, eps)
    return fused


def _check_y3(tag, x, delta, w, b, bad, eps=EPS):
    h, _, mean, rstd = nat.add_layer_norm_fwd(x, delta, w, b, eps)
    h64 = (x if delta is None else h).double()
    mean64 = h64.mean(-1)
    rstd64 = ((h64 - mean64[:, None]).pow(2).mean(-1) + eps).rsqrt()
    e_r = (rstd.double() / rstd64 - 1).abs().max().item()
    e_m = ((mean.double() - mean64).abs() * rstd64).max().item()
    print(f"{tag} stats: |rstd/rstd64 - 1| {e_r:.3e}  |mean - mean64|*rstd64 {e_m:.3e}  bound {Y3_BOUND:.3e}")
    if not (e_r <= Y3_BOUND and e_m <= Y3_BOUND):
        bad.append(("Y3", tag, e_r, e_m, Y3_BOUND))
    return mean, rstd


# ------------------------------------------------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize("C", WIDTHS, ids=lambda c: f"c{c}")
def test_fused_layer_norm_is_no_worse_than_stock_against_float64(C):
    assert nat.lib().add_layer_norm_max_channels() == CMAX
    bad = []
    for M in ROWS:
        for dtype in DTYPES:
            x, delta, w, b, dy, dh = _inputs(M, C, dtype, 1000 + C + M)
            for d in (delta, None):
                tag = f"M={M} C={C} {str(dtype)[6:]} delta={int(d is not None)}"
                _check(tag, x, d, w, b, dy, dh, bad)
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_model_sized_rows(dtype):
    bad = []
    x, delta, w, b, dy, dh = _inputs(16384, 320, dtype, 5)
    x, delta, dy, dh = (t.view(4, 4096, 320) for t in (x, delta, dy, dh))  # the harness hands [B, N, C] tensors over
    flat = lambda t: t.reshape(-1, 320)
    for d in (delta, None):
        _check(f"16384x320 {str(dtype)[6:]} delta={int(d is not None)}", flat(x), None if d is None else flat(d), w, b, flat(dy),
               flat(dh), bad)
    got = _run(_fused(w, b), x, delta, dy, dh)
    want = _run(_fused(w, b), flat(x), flat(delta), flat(dy), flat(dh))
    assert all(u.shape == x.shape and torch.equal(flat(u), v) for u, v in zip(got, want))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------- 2. hard statistics
def _hard_rows(C, dtype, seed):
    """Seven rows: offset 64 with spread 0.05, an outlier of 100 at the first / at the last channel, a constant row, a row of
    zeros, and two plain rows.  Values are rounded to `dtype` here, so what the kernels store is what float64 sees."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    x = rn(7, C)
    x[0] = 64 + 0.05 * x[0]
    x[1, 0] = 100.0
    x[2, -1] = 100.0
    x[3] = 1.25
    x[4] = 0.0
    return x.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("C", [320, 504, CMAX], ids=lambda c: f"c{c}")
def test_hard_rows(C, dtype):
    """Rows whose statistics are hard in fp32, with no delta and with a delta of zeros (h = x exactly on both paths): Y3 on
    mean / rstd, and Y1 / Y2 on y and dx with random dy and dh, the constant and the zero row included."""
    bad = []
    x = _hard_rows(C, dtype, 40 + C)
    _, _, w, b, dy, dh = _inputs(7, C, dtype, 41 + C)
    dy = dy / 16  # rstd = eps^-½ ≈ 316 on the constant rows: keeps dx there well inside f16
    for d in (torch.zeros_like(x), None):
        tag = f"hard C={C} {str(dtype)[6:]} delta={int(d is not None)}"
        h, y = _check(tag, x, d, w, b, dy, dh, bad)[:2]
        mean, rstd = _check_y3(tag, x, d, w, b, bad)
        for r in (3, 4):
            assert rstd[r].item() == pytest.approx(EPS ** -0.5, rel=2.0 ** -13) and mean[r].item() == x[r, 0].item()
            assert torch.equal(y[r], b), (tag, r)  # x̂ = 0 exactly
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_constant_and_zero_rows_are_exact(dtype):
    """A constant row and a row of zeros: rstd = 1/√eps, y = β exactly, and dx = dh exactly wherever g = dy·γ does not vary along
    the row — dy = 0 under a random γ, and one dy value per row under γ = 1."""
    M, C = 5, 504
    x, _, w, b, _, dh = _inputs(M, C, dtype, 77)
    x = (torch.tensor([1.25, 0.0, -3.0, 0.5, 64.0], device="cuda")[:, None].expand(M, C)).to(dtype).contiguous()
    zero = torch.zeros_like(x)
    row_dy = torch.tensor([0.5, -2.0, 1.0, 0.25, 3.0], device="cuda")[:, None].expand(M, C).to(dtype).contiguous()
    for gamma, dy in ((w, zero), (torch.ones_like(w), row_dy)):
        for d in (zero, None):
            h, y, dx = _run(_fused(gamma, b), x, d, dy, dh)[:3]
            _, _, mean, rstd = nat.add_layer_norm_fwd(x, d, gamma, b, EPS)
            print(f"{dtype} delta={int(d is not None)}: rstd {rstd.tolist()} mean {mean.tolist()}")
            assert torch.equal(h, x) and torch.equal(mean, x[:, 0].float())
            assert ((rstd.double() * EPS ** 0.5 - 1).abs() <= Y3_BOUND).all()
            assert torch.equal(y, b.expand(M, C))
            if d is None:  # no residual path: dx is the LayerNorm's own input gradient, exactly zero here
                assert not dx.any()
            else:
                assert torch.equal(dx, dh)


# -------------------------------------------------------------------------------------------------------------- 3. bounds
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("with_delta", [True, False], ids=["delta", "plain"])
@pytest.mark.parametrize("M,C", [(3, 504), (65, 8)])
def test_kernels_write_only_inside_their_tensors(M, C, with_delta, dtype):
    """The C entry points called as _native calls them, every operand inside a larger sentinel-filled buffer: the results equal
    the plain call's bit for bit, the inputs are unchanged and no guard byte changes."""
    x, delta, w, b, dy, dh = _inputs(M, C, dtype, 300)
    if not with_delta:
        delta = dh = None
    h0, y0, mean0, rstd0 = nat.add_layer_norm_fwd(x, delta, w, b, EPS)
    dx0 = nat.add_layer_norm_bwd(dy, dh, x if delta is None else h0, w, mean0, rstd0)
    lib, size, code, stream = nat.lib(), x.element_size(), nat.dtype_code(dtype), nat._stream(x)
    big = lambda src=None: _Guarded(M * C * size, dtype, src)
    gx, gdy, gw, gb = big(x), big(dy), _Guarded(C * size, dtype, w), _Guarded(C * size, dtype, b)
    gdelta, gdh = (big(delta), big(dh)) if with_delta else (None, None)
    gh, gy, gdx = big(), big(), big()
    gmean, grstd = _Guarded(M * 4, torch.float32), _Guarded(M * 4, torch.float32)
    p = lambda g: None if g is None else g.ptr()
    st = lib.add_layer_norm_fwd(gx.ptr(), p(gdelta), gw.ptr(), gb.ptr(), gh.ptr() if with_delta else None, gy.ptr(), gmean.ptr(),
                                grstd.ptr(), M, C, EPS, code, stream)
    assert st == 0
    st = lib.add_layer_norm_bwd(gdy.ptr(), p(gdh), (gh if with_delta else gx).ptr(), gw.ptr(), gmean.ptr(), grstd.ptr(), gdx.ptr(),
                                M, C, code, stream)
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(gy.t, y0.reshape(-1)) and torch.equal(gdx.t, dx0.reshape(-1))
    assert torch.equal(gmean.t, mean0) and torch.equal(grstd.t, rstd0)
    if with_delta:
        assert torch.equal(gh.t, h0.reshape(-1)) and torch.equal(gdelta.t, delta.reshape(-1)) and torch.equal(gdh.t, dh.reshape(-1))
    else:
        assert h0 is None and bool((gh.t.view(torch.uint8) == SENTINEL).all())  # no h is written without a delta
    assert torch.equal(gx.t, x.reshape(-1)) and torch.equal(gdy.t, dy.reshape(-1))
    assert torch.equal(gw.t, w) and torch.equal(gb.t, b)
    for name, g in (("x", gx), ("delta", gdelta), ("dy", gdy), ("dh", gdh), ("gamma", gw), ("beta", gb), ("h", gh), ("y", gy),
                    ("dx", gdx), ("mean", gmean), ("rstd", grstd)):
        assert g is None or g.guards_intact(), name


# ------------------------------------------------------------------------------------------------------- 4. repeatability
@pytest.mark.parametrize("M,C", [(1025, 320), (257, 1280), (65, CMAX), (3, 96)])
def test_two_runs_are_bit_identical_and_a_graph_replay_equals_eager(M, C):
    x, delta, w, b, dy, dh = _inputs(M, C, torch.float16, 7)
    fn = _fused(w, b)
    first, second = _run(fn, x, delta, dy, dh), _run(fn, x, delta, dy, dh)
    assert all(torch.equal(u, v) for u, v in zip(first, second))

    xs, ds = x.clone().requires_grad_(True), delta.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(list(fn(xs, ds)), [xs, ds], [dh, dy])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h, y = fn(xs, ds)
        dx, dd = torch.autograd.grad([h, y], [xs, ds], [dh, dy])
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(first, (h.detach(), y.detach(), dx, dd)))


# ----------------------------------------------------------------------------------------------------------- 5. the front
def test_what_the_kernels_do_not_take_gets_the_stock_composite():
    """A trainable γ, an fp32 tensor, a row-strided view and an x that starts 2 bytes into its storage each take the stock
    composite: results `torch.equal` to it, γ/β gradients included."""
    M, C = 33, 64
    x, delta, w, b, dy, dh = _inputs(M, C, torch.float16, 9)
    assert _hip_layer_norm(x, delta, w, b) and _hip_layer_norm(x, None, w, b)
    wide = torch.cat([x, x], dim=1)
    store = torch.zeros(M * C + 8, dtype=x.dtype, device="cuda")
    odd = store[1:1 + M * C].view(M, C).copy_(x)
    assert odd.data_ptr() % 16 == 2 and odd.is_contiguous()
    cases = {
        "trainable gamma": (x, delta, w.clone().requires_grad_(True), b.clone().requires_grad_(True), dy, dh),
        "fp32": tuple(t.float() for t in (x, delta, w, b, dy, dh)),
        "row-strided": (wide[:, :C], delta, w, b, dy, dh),
        "odd start": (odd, delta, w, b, dy, dh),
        "odd delta": (x, store[1:1 + M * C].view(M, C), w, b, dy, dh),
        "C % 8": tuple(t[..., :60].contiguous() for t in (x, delta, w, b, dy, dh)),
    }
    for name, (xx, dd, ww, bb, gy, gh) in cases.items():
        for d in (dd, None) if name != "odd delta" else (dd,):
            assert not _hip_layer_norm(xx, d, ww, bb), name
            ins = lambda: [xx.detach().requires_grad_(True)] + ([] if d is None else [d.detach().requires_grad_(True)])
            outs = []
            for fn in (_fused(ww, bb), _stock(ww, bb)):
                leaves = ins()
                assert leaves[0].stride() == xx.stride() and leaves[0].data_ptr() % 16 == xx.data_ptr() % 16
                h, y = fn(leaves[0], leaves[1] if d is not None else None)
                params = [ww, bb] if ww.requires_grad else []
                if d is None:
                    grads = torch.autograd.grad([y], leaves + params, [gy])
                else:
                    grads = torch.autograd.grad([h, y], leaves + params, [gh, gy])
                outs.append([h.detach(), y.detach(), *grads])
            assert len(outs[0]) == len(outs[1]) and all(torch.equal(u, v) for u, v in zip(*outs)), name


def test_a_strided_or_misaligned_dy_is_copied_once_and_h_only_gradients_pass_through(monkeypatch):
    M, C = 65, 320
    x, delta, w, b, dy, dh = _inputs(M, C, torch.bfloat16, 12)
    want = _run(_fused(w, b), x, delta, dy, dh)
    # dy and dh as views: every other column of a wider tensor, and a dense tensor 2 bytes into its storage
    wide = torch.zeros(M, 2 * C, dtype=dy.dtype, device="cuda")
    wide[:, ::2] = dy
    store = torch.zeros(M * C + 8, dtype=dh.dtype, device="cuda")
    odd = store[1:1 + M * C].view(M, C).copy_(dh)
    assert not wide[:, ::2].is_contiguous() and odd.data_ptr() % 16 == 2
    got = _run(_fused(w, b), x, delta, wide[:, ::2], odd)
    assert all(torch.equal(u, v) for u, v in zip(got, want))
    got = _run(_fused(w, b), x, delta, odd.copy_(dy), wide[:, ::2].copy_(dh))
    assert all(torch.equal(u, v) for u, v in zip(got, want))

    calls = []
    real = nat.add_layer_norm_bwd
    monkeypatch.setattr(nat, "add_layer_norm_bwd", lambda *a: calls.append(1) or real(*a))
    xs, ds = x.clone().requires_grad_(True), delta.clone().requires_grad_(True)
    h, y = add_layer_norm(xs, ds, w, b, EPS)
    gx, gd = torch.autograd.grad([h], [xs, ds], [dh], retain_graph=True)  # a gradient into h only: no launch
    assert not calls and torch.equal(gx, dh) and torch.equal(gd, dh)
    (gx,) = torch.autograd.grad([y], [xs], [dy], retain_graph=True)  # into y only, and only x asks
    assert len(calls) == 1
    y_only = _run(lambda a, c: (a + c, layer_norm(a + c, w, b, EPS)), x, delta, dy, torch.zeros_like(dh))
    assert torch.equal(gx, y_only[2])
    # without requires_grad nothing is recorded
    assert not add_layer_norm(x, delta, w, b, EPS)[1].requires_grad and not layer_norm(x, w, b, EPS).requires_grad


# ------------------------------------------------------------------------------------------------------------ 6. harness
def test_harness_block_goes_through_the_front_on_16_bit_gpu_tensors(monkeypatch):
    import harness.unet as hu

    torch.manual_seed(21)
    blk = hu.BasicTransformerBlock(64, 2, 32, 48).cuda().half()
    blk.requires_grad_(False)
    x = torch.randn(2, 40, 64, device="cuda").half().requires_grad_(True)
    ctx = torch.randn(2, 6, 48, device="cuda").half()
    counts = {"layer_norm": 0, "add_layer_norm": 0}

    def spy(name):
        real = getattr(dnorm, name)

        def call(*a, **k):
            counts[name] += 1
            return real(*a, **k)
        return call

    for name in counts:
        monkeypatch.setattr(dnorm, name, spy(name))
    out = blk(x, ctx)
    assert counts == {"layer_norm": 1, "add_layer_norm": 2}
    (dx,) = torch.autograd.grad(out, [x], torch.ones_like(out))

    counts.update(layer_norm=0, add_layer_norm=0)
    monkeypatch.setattr(hu, "_fused_norms", lambda t: False)
    ref = blk(x, ctx)
    assert counts == {"layer_norm": 0, "add_layer_norm": 0}
    (dref,) = torch.autograd.grad(ref, [x], torch.ones_like(ref))
    # the two forwards differ by the roundings the fused norms leave out: a few f16 ulps of the block's output
    print(f"block: |out - ref| max {(out - ref).abs().max().item():.3e} of {ref.abs().max().item():.3e}; "
          f"|dx - dref| max {(dx - dref).abs().max().item():.3e} of {dref.abs().max().item():.3e}")
    assert (out - ref).abs().max().item() <= 2.0 ** -7 * ref.abs().max().item()
    assert (dx - dref).abs().max().item() <= 2.0 ** -7 * dref.abs().max().item()
