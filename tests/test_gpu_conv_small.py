"""The packed-weight 3×3 convolution (csrc/conv_small.hip, diffusion_finetuning_amd/conv.py) against float64 at its tile, halo,
slice and image-grouping edges, its taps one by one, its determinism, its containment and its front's routing rules."""
import itertools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}

NS = (1, 3)
HWS = ((1, 1), (3, 5), (8, 8), (12, 12), (16, 16))
CINS = (32, 96, 160)
COUTS = (32, 160)


def _nat():
    from diffusion_finetuning_amd import _native as nat
    return nat


def _conv():
    from diffusion_finetuning_amd import conv
    return conv


def _positions(m0, MT, M, H, W):
    def q(m):
        img, r = divmod(m, H * W)
        h, w = divmod(r, W)
        return img * (H + 2) * (W + 2) + (h + 1) * (W + 2) + (w + 1)
    return q(min(m0 + MT, M) - 1) - q(m0) + 2 * (W + 3) + 1


def slices_folded(N, Cin, Cout, H, W, dtype):
    """S, the number of fp32 partials the second launch folds per element: the tiling rule of conv_small.hip restated, and
    checked against the workspace size the library reports (S · C_out · padded pixels · 4 bytes)."""
    M = N * H * W
    for MT, cap in ((128, 256), (64, 768)):
        mtiles = -(-M // MT)
        if max(_positions(t * MT, MT, M, H, W) for t in range(mtiles)) <= cap:
            break
    else:
        raise AssertionError("shape not covered")
    ntiles, chunks = -(-Cout // 128), Cin // 32
    want = max(1, 256 // (mtiles * ntiles))
    cps = -(-chunks // want)
    if chunks >= 4 and cps < 2:
        cps = 2
    S = -(-chunks // cps)
    nat = _nat()
    assert nat.lib().conv3x3_small_workspace_bytes(N, Cin, Cout, H, W, nat.dtype_code(dtype)) == S * Cout * mtiles * MT * 4
    return S


def _operands(N, Cin, Cout, H, W, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g).to(dtype)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)).to(dtype)
    b = torch.randn(Cout, generator=g).to(dtype)
    dy = torch.randn(N, Cout, H, W, generator=g).to(dtype)
    return x, w, b, dy


def _check_bound(got, ref64, absref64, terms, dtype, what):
    """|y − y64| ≤ u·|y64| + 2·terms·2⁻²⁴·(|x| ⊛ |w|) + tiny, per element."""
    err = (got.double().cpu() - ref64).abs()
    bound = U[dtype] * ref64.abs() + 2.0 * terms * 2.0 ** -24 * absref64 + TINY[dtype]
    worst = (err / bound).max().item()
    assert worst <= 1.0, (what, "error / bound", worst)


def _rel_l2(a, ref64):
    return ((a.double().cpu() - ref64).norm() / ref64.norm().clamp_min(1e-300)).item()


def _run_case(N, Cin, Cout, H, W, dtype, seed, record=None):
    conv = _conv()
    x, w, b, dy = _operands(N, Cin, Cout, H, W, dtype, seed)
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
    x64, w64, b64, dy64 = x.double(), w.double(), b.double(), dy.double()
    y64 = F.conv2d(x64, w64, None, padding=1)
    ya64 = F.conv2d(x64.abs(), w64.abs(), None, padding=1)
    S = slices_folded(N, Cin, Cout, H, W, dtype)
    what = (N, Cin, Cout, H, W, str(dtype))
    y = conv.conv3x3(xd, wd, None, route="hip")
    _check_bound(y, y64, ya64, 9 * Cin + S, dtype, what + ("fwd",))
    yb = conv.conv3x3(xd, wd, bd, route="hip")
    _check_bound(yb, y64 + b64[None, :, None, None], ya64 + b64.abs()[None, :, None, None], 9 * Cin + S + 1, dtype, what + ("fwd+bias",))
    xg = xd.clone().requires_grad_(True)
    conv.conv3x3(xg, wd, bd, route="hip").backward(dyd)
    dx64 = F.conv_transpose2d(dy64, w64, None, padding=1)
    dxa64 = F.conv_transpose2d(dy64.abs(), w64.abs(), None, padding=1)
    Sb = slices_folded(N, Cout, Cin, H, W, dtype)
    _check_bound(xg.grad, dx64, dxa64, 9 * Cout + Sb, dtype, what + ("bwd",))
    if record is not None:
        xs = xd.clone().requires_grad_(True)
        ys = F.conv2d(xs, wd, None, padding=1)
        ys.backward(dyd)
        record.append((what, _rel_l2(y, y64), _rel_l2(ys.detach(), y64), _rel_l2(xg.grad, dx64), _rel_l2(xs.grad, dx64)))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("N", NS)
def test_every_edge_shape_against_float64_both_directions(dtype, N):
    """Halo on every side, M off the MFMA tile, row pitches that are no power of two, one K-step, ragged N-tiles and K-slices,
    a ragged image grouping (N = 3): per-element bound from the one store rounding and worst-case fp32 summation."""
    record = []
    for seed, ((H, W), Cin, Cout) in enumerate(itertools.product(HWS, CINS, COUTS)):
        _run_case(N, Cin, Cout, H, W, dtype, seed, record if (Cin, Cout) == (160, 160) else None)
    for what, fy, sy, fdx, sdx in record:
        print(f"rel L2 vs float64 {what}: fwd hip {fy:.3e} stock {sy:.3e} | bwd hip {fdx:.3e} stock {sdx:.3e}")


# shapes that 128 pixels with their halo do not fit in 256 padded positions: the 64-pixel instantiation, three positions a thread.
# 40 images of 1×1 are 360 positions a tile; the 280-wide rows are 630 positions, 50 400 bytes of LDS: over the 48 KB that need the
# function attribute raised
SMALL_TILE_SHAPES = [(40, 96, 160, 1, 1), (1, 32, 160, 2, 280), (1, 160, 32, 3, 280), (26, 32, 32, 3, 5)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_the_64_pixel_instantiation_against_float64_both_directions(dtype):
    for seed, (N, Cin, Cout, H, W) in enumerate(SMALL_TILE_SHAPES):
        M = N * H * W
        assert max(_positions(t * 128, 128, M, H, W) for t in range(-(-M // 128))) > 256  # really the small-tile path
        _run_case(N, Cin, Cout, H, W, dtype, 50 + seed)


def test_real_slice_and_tile_counts_at_reduced_cost():
    """N = 1, 8×8, 2560→1280: the benchmark's ten channel tiles and 80 chunks in 20 K-slices (1280→2560 in the backward)."""
    record = []
    _run_case(1, 2560, 1280, 8, 8, torch.float16, 99, record)
    for what, fy, sy, fdx, sdx in record:
        print(f"rel L2 vs float64 {what}: fwd hip {fy:.3e} stock {sy:.3e} | bwd hip {fdx:.3e} stock {sdx:.3e}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_each_tap_and_each_border_pixel_by_itself(dtype):
    """A weight that is non-zero in ONE tap (with channel-dependent values) against every corner, edge and interior pixel lit
    alone: a flipped or shifted tap, or a wrong backward pack, fails by itself.  Values are small integers: exact in 16 bits."""
    conv = _conv()
    N, Cin, Cout, H, W = 2, 32, 64, 5, 6
    g = torch.Generator().manual_seed(5)
    pixels = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 2), (H - 1, 3), (2, 0), (3, W - 1), (2, 2)]
    for tap in range(9):
        w = torch.zeros(Cout, Cin, 3, 3)
        w[:, :, tap // 3, tap % 3] = torch.randint(-3, 4, (Cout, Cin), generator=g).float()
        wd = w.to(dtype).to(DEV)
        x = torch.zeros(len(pixels) * N, Cin, H, W)
        dy = torch.zeros(len(pixels) * N, Cout, H, W)
        for i, (h, ww) in enumerate(pixels):
            x[i * N:(i + 1) * N, :, h, ww] = torch.randint(-2, 3, (N, Cin), generator=g).float()
            dy[i * N:(i + 1) * N, :, h, ww] = torch.randint(-2, 3, (N, Cout), generator=g).float()
        xg = x.to(dtype).to(DEV).requires_grad_(True)
        y = conv.conv3x3(xg, wd, None, route="hip")
        y.backward(dy.to(dtype).to(DEV))
        assert torch.equal(y.detach().double().cpu(), F.conv2d(x.double(), w.double(), padding=1)), ("fwd tap", tap)
        assert torch.equal(xg.grad.double().cpu(), F.conv_transpose2d(dy.double(), w.double(), padding=1)), ("bwd tap", tap)


@pytest.mark.parametrize("shape", [(4, 160, 96, 8, 8), (3, 96, 160, 12, 12)])
def test_two_calls_and_a_replayed_capture_give_the_same_bits(shape):
    conv = _conv()
    N, Cin, Cout, H, W = shape
    x, w, b, dy = (t.to(DEV) for t in _operands(N, Cin, Cout, H, W, torch.float16, 3))
    nat = _nat()
    fwd, bwd = nat.conv3x3_small_pack(w, False), nat.conv3x3_small_pack(w, True)
    y1, y2 = nat.conv3x3_small(x, fwd, b, Cout), nat.conv3x3_small(x, fwd, b, Cout)
    d1, d2 = nat.conv3x3_small(dy, bwd, None, Cin), nat.conv3x3_small(dy, bwd, None, Cin)
    assert torch.equal(y1, y2) and torch.equal(d1, d2)
    xg = x.clone().requires_grad_(True)
    conv.conv3x3(xg, w, b, route="hip")  # packs made before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            yc = conv.conv3x3(xg, w, b, route="hip")
            dc, = torch.autograd.grad(yc, xg, dy)
    torch.cuda.current_stream().wait_stream(side)
    yc.detach().zero_(), dc.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yc.detach(), y1) and torch.equal(dc, d1)


@pytest.mark.parametrize("shape", [(3, 96, 160, 3, 5), (4, 160, 32, 8, 8), (1, 32, 160, 16, 16), (3, 32, 32, 1, 1),
                                   (40, 96, 160, 1, 1), (1, 32, 160, 2, 280)])  # the last two: 64-pixel tiles, the second over 48 KB of LDS
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_kernels_write_only_inside_y_and_the_workspace_formula_covers_what_they_touch(shape, dtype):
    """x, the pack, y and the workspace sit inside canary-filled buffers, the workspace exactly as large as
    conv3x3_small_workspace_bytes says: every canary is intact afterwards, and x and the pack are unchanged."""
    nat = _nat()
    N, Cin, Cout, H, W = shape
    x, w, b, _ = (t.to(DEV) for t in _operands(N, Cin, Cout, H, W, dtype, 7))
    code = nat.dtype_code(dtype)
    ws_bytes = int(nat.lib().conv3x3_small_workspace_bytes(N, Cin, Cout, H, W, code))
    assert ws_bytes > 0
    pad = 4096  # elements / floats of canary on either side (a multiple of 16 bytes)
    canary16 = torch.tensor(-1234.0, dtype=dtype).item()

    def framed(n, dt, fill):
        buf = torch.full((n + 2 * pad,), fill, dtype=dt, device=DEV)
        return buf, buf[pad:pad + n]

    xbuf, xv = framed(x.numel(), dtype, canary16)
    pbuf, pv = framed(w.numel(), dtype, canary16)
    ybuf, yv = framed(N * Cout * H * W, dtype, canary16)
    wbuf, wv = framed(ws_bytes // 4, torch.float32, -4321.0)
    xv.copy_(x.flatten())
    st = nat.lib().conv3x3_small_pack(w.data_ptr(), pv.data_ptr(), Cin, Cout, 0, code, nat._stream(x))
    assert st == 0
    packed = pv.clone()
    st = nat.lib().conv3x3_small(xv.data_ptr(), pv.data_ptr(), b.data_ptr(), yv.data_ptr(), wv.data_ptr(), ws_bytes, N, Cin, Cout,
                                 H, W, code, nat._stream(x))
    assert st == 0
    torch.cuda.synchronize()
    for name, buf, fill in (("x", xbuf, canary16), ("pack", pbuf, canary16), ("y", ybuf, canary16), ("workspace", wbuf, -4321.0)):
        assert (buf[:pad] == fill).all() and (buf[-pad:] == fill).all(), name
    assert torch.equal(xv, x.flatten()) and torch.equal(pv, packed)
    assert torch.equal(yv.view(N, Cout, H, W), nat.conv3x3_small(x, packed, b, Cout))
    # one byte less of workspace is refused before any launch
    assert nat.lib().conv3x3_small(xv.data_ptr(), pv.data_ptr(), None, yv.data_ptr(), wv.data_ptr(), ws_bytes - 1, N, Cin, Cout, H, W,
                                   code, nat._stream(x)) == -1


def _counting(monkeypatch):
    """Counts the calls that reach the HIP kernel."""
    nat = _nat()
    calls = []
    real = nat.conv3x3_small

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(nat, "conv3x3_small", spy)
    return calls


def test_front_routes_only_what_the_kernel_may_run(monkeypatch):
    conv = _conv()
    calls = _counting(monkeypatch)
    x, w, b, dy = (t.to(DEV) for t in _operands(2, 32, 64, 8, 8, torch.float16, 11))
    ref = F.conv2d(x, w, b, padding=1)

    def stock(xx, ww, bb=None):
        n = len(calls)
        out = conv.conv3x3(xx, ww, bb)  # "auto": never raises
        assert len(calls) == n
        return out

    # a trainable weight (or bias)
    wt = w.clone().requires_grad_(True)
    assert torch.equal(stock(x, wt, b), ref)
    with pytest.raises(RuntimeError):
        conv.conv3x3(x, wt, b, route="hip")
    with pytest.raises(RuntimeError):
        conv.conv3x3(x, w, b.clone().requires_grad_(True), route="hip")
    # a misaligned x (2 bytes into its storage) and a channels-last x
    flat = torch.zeros(x.numel() + 8, dtype=x.dtype, device=DEV)
    xm = flat[1:1 + x.numel()].view_as(x)
    xm.copy_(x)
    for bad in (xm, x.contiguous(memory_format=torch.channels_last)):
        with pytest.raises(RuntimeError):
            conv.conv3x3(bad, w, b, route="hip")
        stock(bad, w, b)
    # an fp32 x (and weight)
    with pytest.raises(RuntimeError):
        conv.conv3x3(x.float(), w.float(), b.float(), route="hip")
    stock(x.float(), w.float(), b.float())
    # the forced route does reach the kernel, and an unknown route is refused
    n = len(calls)
    conv.conv3x3(x, w, b, route="hip")
    assert len(calls) == n + 1
    with pytest.raises(ValueError):
        conv.conv3x3(x, w, b, route="fast")


def test_an_in_place_write_to_the_weight_is_seen_by_the_next_call():
    conv = _conv()
    x, w, b, _ = (t.to(DEV) for t in _operands(2, 32, 32, 8, 8, torch.float16, 12))
    y0 = conv.conv3x3(x, w, None, route="hip")
    w.mul_(2)
    y1 = conv.conv3x3(x, w, None, route="hip")
    assert torch.equal(y1, y0 * 2)  # doubling is exact in f16
    w.data = (w * 0.5).clone()  # reloaded into other memory
    assert torch.equal(conv.conv3x3(x, w, None, route="hip"), y0)


def test_capture_without_a_pack_runs_stock_and_with_a_prepack_runs_hip(monkeypatch):
    conv, nat = _conv(), _nat()
    calls = _counting(monkeypatch)
    x, _, _, _ = (t.to(DEV) for t in _operands(2, 32, 64, 8, 8, torch.float16, 13))
    layer = nn.Conv2d(32, 64, 3, padding=1).to(DEV).half().requires_grad_(False)
    assert conv.prepack_conv3x3(nn.Sequential(layer)) == 0  # the planner routes no 32→64 class ...
    monkeypatch.setattr(nat, "conv3x3_small_plan", lambda *a: True)  # ... so let it, to see what "auto" does with and without a pack
    monkeypatch.setattr(nat, "conv3x3_small_plan_channels", lambda *a: True)
    F.conv2d(x, layer.weight, layer.bias, padding=1)  # the stock call's own setup happens outside the capture
    torch.cuda.synchronize()

    def capture():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                y = conv.conv3x3(x, layer.weight, layer.bias)
        torch.cuda.current_stream().wait_stream(side)
        graph.replay()
        torch.cuda.synchronize()
        return y

    y_stock = capture()
    assert len(calls) == 0  # no pack, and none is made while capturing
    assert conv.prepack_conv3x3(nn.Sequential(layer)) == 1
    y_hip = capture()
    assert len(calls) == 1
    assert torch.equal(y_hip, conv.conv3x3(x, layer.weight, layer.bias, route="hip"))
    torch.testing.assert_close(y_hip, y_stock, rtol=2e-3, atol=2e-3)


def test_autograd_dx_is_the_direct_backward_call():
    conv, nat = _conv(), _nat()
    x, w, b, dy = (t.to(DEV) for t in _operands(3, 96, 160, 12, 12, torch.float16, 14))
    xg = x.clone().requires_grad_(True)
    conv.conv3x3(xg, w, b, route="hip").backward(dy)
    assert torch.equal(xg.grad, nat.conv3x3_small(dy, nat.conv3x3_small_pack(w, True), None, 96))
    # no input gradient wanted: the backward launches nothing
    assert not conv.conv3x3(x, w, b, route="hip").requires_grad


def _lora_grads(route, monkeypatch, seed=0):
    import diffusion_finetuning_amd as dfa
    from diffusion_finetuning_amd import trainer as tr
    from harness import unet as hu

    monkeypatch.setattr(hu, "CONV3X3_ROUTE", route)
    torch.manual_seed(seed)
    unet = hu.UNet2DConditionModel(hu.tiny_config(32, 32, 2))  # channels 32 and 64: every ResNet / upsampler conv is eligible
    unet.requires_grad_(False)
    unet = unet.to(DEV).half()
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for p in itertools.chain(*params):
            p.copy_((torch.randn(p.shape, generator=g) * 0.05).to(DEV))
    trainer = tr.LoraTrainer(unet, lr=1e-3, loss_scale=256.0)
    lat, noise = torch.randn(2, 4, 8, 8, generator=g).to(DEV), torch.randn(2, 4, 8, 8, generator=g).to(DEV)
    ts = torch.tensor([100, 700], device=DEV)
    ctx = torch.randn(2, 6, 32, generator=g).to(DEV)
    trainer.step(lat, noise, ts, ctx)
    torch.cuda.synchronize()
    return trainer.slab.grads[: trainer.slab.numel].double().cpu()


def test_one_training_step_with_every_conv_on_the_hip_kernel_matches_stock(monkeypatch):
    """LoRA gradients of one f16 step of the widened tiny UNet, every ResNet / upsampler conv forced to the HIP kernel, against
    the same step on stock convolutions.  Stock against stock is the baseline: its split-K path adds fp32 partials with atomics, in
    an order that changes from run to run, so two stock steps differ (1.2e-3 to 1.3e-3 relative L2 measured).  The HIP kernel
    differs from a stock run by that same reordering plus its own fixed order: the margin is 4 × the baseline of the same run
    (hip against stock measured 1.7e-3 to 1.9e-3, about 1.5 × the baseline)."""
    calls = _counting(monkeypatch)
    stock1 = _lora_grads("stock", monkeypatch)
    assert len(calls) == 0
    stock2 = _lora_grads("stock", monkeypatch)
    hip = _lora_grads("hip", monkeypatch)
    assert len(calls) >= 10  # forward and backward-data of the ResNets' and the upsampler's convs
    base = ((stock1 - stock2).norm() / stock1.norm()).item()
    diff = ((hip - stock1).norm() / stock1.norm()).item()
    print(f"LoRA gradient rel L2: hip vs stock {diff:.3e}, stock vs stock {base:.3e}")
    assert stock1.norm() > 0 and base > 0 and diff <= 4 * base, (diff, base)
