"""The many-pixel packed-weight 3×3 convolution (csrc/conv_large.hip, conv.conv3x3(route="large")) against float64 at its tile,
halo, row-pitch and image-grouping edges, in every instantiation, its taps one by one, its determinism, its containment and its
front's routing rules.  U, TINY and the per-element bound are those of tests/test_gpu_conv_small.py, restated here."""
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
HWS = ((1, 1), (3, 5), (5, 32), (3, 64), (2, 66))
CINS = (32, 96)
COUTS = (32, 160, 192, 352)  # of the 160-wide channel tile: below one, exactly one, ragged past one, ragged past two

VARIANTS = ((128, 384), (64, 192), (64, 384))  # (pixels per tile, padded positions its staging covers) of conv_large.hip's launcher


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


def variant(N, Cout, H, W):
    """The tiling rule of conv_large.hip restated: which instantiation a call of this shape runs on."""
    M = N * H * W
    ntiles = -(-Cout // 160)
    pmax = {MT: max(_positions(t * MT, MT, M, H, W) for t in range(-(-M // MT))) for MT in (128, 64)}
    fits = [pmax[MT] <= cap for MT, cap in VARIANTS]
    if fits[0] and -(-M // 128) * ntiles >= 256:
        return VARIANTS[0]
    if fits[1]:
        return VARIANTS[1]
    if fits[2]:
        return VARIANTS[2]
    assert fits[0], "shape not covered"
    return VARIANTS[0]


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


def _run_case(N, Cin, Cout, H, W, dtype, seed):
    """Both directions of one shape through route="large".  S = 1: the library reports no workspace, i.e. one slice."""
    conv, nat = _conv(), _nat()
    code = nat.dtype_code(dtype)
    assert nat.lib().conv3x3_large_workspace_bytes(N, Cin, Cout, H, W, code) == 0
    assert nat.lib().conv3x3_large_workspace_bytes(N, Cout, Cin, H, W, code) == 0
    S = 1
    x, w, b, dy = _operands(N, Cin, Cout, H, W, dtype, seed)
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
    x64, w64, b64, dy64 = x.double(), w.double(), b.double(), dy.double()
    y64 = F.conv2d(x64, w64, None, padding=1)
    ya64 = F.conv2d(x64.abs(), w64.abs(), None, padding=1)
    what = (N, Cin, Cout, H, W, str(dtype))
    y = conv.conv3x3(xd, wd, None, route="large")
    _check_bound(y, y64, ya64, 9 * Cin + S, dtype, what + ("fwd",))
    xg = xd.clone().requires_grad_(True)
    yb = conv.conv3x3(xg, wd, bd, route="large")
    _check_bound(yb.detach(), y64 + b64[None, :, None, None], ya64 + b64.abs()[None, :, None, None], 9 * Cin + S + 1, dtype,
                 what + ("fwd+bias",))
    yb.backward(dyd)
    dx64 = F.conv_transpose2d(dy64, w64, None, padding=1)
    dxa64 = F.conv_transpose2d(dy64.abs(), w64.abs(), None, padding=1)
    _check_bound(xg.grad, dx64, dxa64, 9 * Cout + S, dtype, what + ("bwd",))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("N", NS)
def test_every_edge_shape_against_float64_both_directions(dtype, N):
    """Halo on every side, the row pitches of the real levels and one that is no power of two, tiles that span rows, end in
    the middle of a row and straddle two images (N = 3), M off the pixel tile and off 16, one and three K-steps, channel
    tiles below one, exactly one, ragged past one and past two.  Both 64-pixel instantiations are reached."""
    seen = set()
    for seed, ((H, W), Cin, Cout) in enumerate(itertools.product(HWS, CINS, COUTS)):
        seen.add(variant(N, Cout, H, W))
        seen.add(variant(N, Cin, H, W))  # the backward call
        _run_case(N, Cin, Cout, H, W, dtype, seed)
    assert seen == {(64, 192), (64, 384)}


# shapes with at least 256 tiles of 128 pixels x 160 channels: the 128-pixel instantiation (forward of the first, backward of the
# second); their other direction has one channel tile, 128 tiles, and runs on 64-pixel tiles (the larger staging area: a 64-wide row)
BIG_TILE_SHAPES = [(4, 32, 192, 64, 64), (4, 192, 32, 64, 64)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", BIG_TILE_SHAPES)
def test_the_128_pixel_instantiation_against_float64_both_directions(shape, dtype):
    N, Cin, Cout, H, W = shape
    assert {variant(N, Cout, H, W), variant(N, Cin, H, W)} == {(128, 384), (64, 384)}
    _run_case(N, Cin, Cout, H, W, dtype, 70)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_a_long_k_loop_at_reduced_cost(dtype):
    """(1, 1920, 160, 4, 64) and its backward (1, 160, 1920, 4, 64): 60 chunks through one accumulator chain, 12 channel tiles."""
    _run_case(1, 1920, 160, 4, 64, dtype, 99)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 32, 64, 5, 6), (1, 32, 32, 3, 64)])
def test_each_tap_and_each_border_pixel_by_itself(shape, dtype):
    """A weight that is non-zero in ONE tap (with channel-dependent values) against every corner, edge and interior pixel lit
    alone: a flipped or shifted tap, or a wrong backward pack, fails by itself.  Values are small integers: exact in 16 bits."""
    conv = _conv()
    N, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(5)
    pixels = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 2), (H - 1, 3), (H // 2, 0), (H // 2, W - 1), (H // 2, 2)]
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
        y = conv.conv3x3(xg, wd, None, route="large")
        y.backward(dy.to(dtype).to(DEV))
        assert torch.equal(y.detach().double().cpu(), F.conv2d(x.double(), w.double(), padding=1)), ("fwd tap", tap)
        assert torch.equal(xg.grad.double().cpu(), F.conv_transpose2d(dy.double(), w.double(), padding=1)), ("bwd tap", tap)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(3, 96, 192, 5, 32), (3, 160, 96, 3, 64)])
def test_two_calls_and_a_replayed_capture_give_the_same_bits(shape, dtype):
    conv, nat = _conv(), _nat()
    N, Cin, Cout, H, W = shape
    x, w, b, dy = (t.to(DEV) for t in _operands(N, Cin, Cout, H, W, dtype, 3))
    fwd, bwd = nat.conv3x3_small_pack(w, False), nat.conv3x3_small_pack(w, True)
    y1, y2 = nat.conv3x3_large(x, fwd, b, Cout), nat.conv3x3_large(x, fwd, b, Cout)
    d1, d2 = nat.conv3x3_large(dy, bwd, None, Cin), nat.conv3x3_large(dy, bwd, None, Cin)
    assert torch.equal(y1, y2) and torch.equal(d1, d2)
    xg = x.clone().requires_grad_(True)
    conv.conv3x3(xg, w, b, route="large")  # packs made before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            yc = conv.conv3x3(xg, w, b, route="large")
            dc, = torch.autograd.grad(yc, xg, dy)
    torch.cuda.current_stream().wait_stream(side)
    yc.detach().zero_(), dc.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yc.detach(), y1) and torch.equal(dc, d1)


@pytest.mark.parametrize("shape", [(3, 96, 160, 3, 5), (1, 32, 192, 5, 32), (3, 32, 352, 3, 64), (3, 32, 32, 1, 1), (1, 96, 32, 2, 66),
                                   (4, 32, 192, 64, 64)])  # the last: 128-pixel tiles
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_the_kernel_writes_only_inside_y(shape, dtype):
    """x, the pack and y sit inside canary-filled buffers; no workspace is passed (the library asks for none): every canary is
    intact afterwards, and x and the pack are unchanged."""
    nat = _nat()
    N, Cin, Cout, H, W = shape
    x, w, b, _ = (t.to(DEV) for t in _operands(N, Cin, Cout, H, W, dtype, 7))
    code = nat.dtype_code(dtype)
    assert nat.lib().conv3x3_large_workspace_bytes(N, Cin, Cout, H, W, code) == 0
    pad = 4096
    canary16 = torch.tensor(-1234.0, dtype=dtype).item()

    def framed(n):
        buf = torch.full((n + 2 * pad,), canary16, dtype=dtype, device=DEV)
        return buf, buf[pad:pad + n]

    xbuf, xv = framed(x.numel())
    pbuf, pv = framed(w.numel())
    ybuf, yv = framed(N * Cout * H * W)
    xv.copy_(x.flatten())
    assert nat.lib().conv3x3_small_pack(w.data_ptr(), pv.data_ptr(), Cin, Cout, 0, code, nat._stream(x)) == 0
    packed = pv.clone()
    st = nat.lib().conv3x3_large(xv.data_ptr(), pv.data_ptr(), b.data_ptr(), yv.data_ptr(), None, 0, N, Cin, Cout, H, W, code,
                                 nat._stream(x))
    assert st == 0
    torch.cuda.synchronize()
    for name, buf in (("x", xbuf), ("pack", pbuf), ("y", ybuf)):
        assert (buf[:pad] == canary16).all() and (buf[-pad:] == canary16).all(), name
    assert torch.equal(xv, x.flatten()) and torch.equal(pv, packed)
    assert not (yv == canary16).any()  # every element of y was written
    assert torch.equal(yv.view(N, Cout, H, W), nat.conv3x3_large(x, packed, b, Cout))


def _counting(monkeypatch):
    """Counts the calls that reach the many-pixel kernel."""
    nat = _nat()
    calls = []
    real = nat.conv3x3_large

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(nat, "conv3x3_large", spy)
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
        conv.conv3x3(x, wt, b, route="large")
    with pytest.raises(RuntimeError):
        conv.conv3x3(x, w, b.clone().requires_grad_(True), route="large")
    # a misaligned x (2 bytes into its storage) and a channels-last x
    flat = torch.zeros(x.numel() + 8, dtype=x.dtype, device=DEV)
    xm = flat[1:1 + x.numel()].view_as(x)
    xm.copy_(x)
    for bad in (xm, x.contiguous(memory_format=torch.channels_last)):
        with pytest.raises(RuntimeError):
            conv.conv3x3(bad, w, b, route="large")
        assert torch.equal(stock(bad, w, b), F.conv2d(bad, w, b, padding=1))
    # an fp32 x (and weight)
    with pytest.raises(RuntimeError):
        conv.conv3x3(x.float(), w.float(), b.float(), route="large")
    assert torch.equal(stock(x.float(), w.float(), b.float()), F.conv2d(x.float(), w.float(), b.float(), padding=1))
    # channels that are no multiple of 32
    x48, w48 = torch.randn(2, 48, 8, 8, device=DEV).half(), torch.randn(64, 48, 3, 3, device=DEV).half()
    with pytest.raises(RuntimeError):
        conv.conv3x3(x48, w48, b, route="large")
    assert torch.equal(stock(x48, w48, b), F.conv2d(x48, w48, b, padding=1))
    # the forced route does reach the kernel, and an unknown route is refused
    n = len(calls)
    conv.conv3x3(x, w, b, route="large")
    assert len(calls) == n + 1
    with pytest.raises(ValueError):
        conv.conv3x3(x, w, b, route="fast")


def test_capture_without_a_pack_runs_stock_and_with_a_prepack_runs_the_kernel(monkeypatch):
    conv, nat = _conv(), _nat()
    calls = _counting(monkeypatch)
    x, _, _, _ = (t.to(DEV) for t in _operands(2, 32, 64, 8, 8, torch.float16, 13))
    layer = nn.Conv2d(32, 64, 3, padding=1).to(DEV).half().requires_grad_(False)
    assert conv.prepack_conv3x3(nn.Sequential(layer)) == 0  # no planner routes a 32→64 class ...
    monkeypatch.setattr(nat, "conv3x3_large_plan", lambda *a: True)  # ... so let the large one, to see "auto" with and without a pack
    monkeypatch.setattr(nat, "conv3x3_large_plan_channels", lambda *a: True)
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
    assert torch.equal(y_hip, conv.conv3x3(x, layer.weight, layer.bias, route="large"))
    torch.testing.assert_close(y_hip, y_stock, rtol=2e-3, atol=2e-3)


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


def test_one_training_step_with_every_conv_on_the_large_kernel_matches_stock(monkeypatch):
    """LoRA gradients of one f16 step of the widened tiny UNet, every ResNet / upsampler conv forced to the many-pixel kernel,
    against the same step on stock convolutions.  Stock against stock, measured in the same run, is the baseline; the margin is
    4 × that baseline, as for the small family.

    The baseline is the mean over the three pairs of three stock steps, two taken before the forced step and one after it, and
    the difference the mean over the same three.  One pair is not enough: with the stock library's per-user database empty,
    consecutive stock steps of one process were bit-identical (0.0 measured, three steps in a row), which made a one-pair
    baseline zero and this test fail by itself, while the first stock step of the process and a stock step taken after other
    work differed from those by 1.2e-3 to 1.3e-3 in every process (profiles/README.md has the table).  The forced step differed
    from the stock steps by 1.6e-3 to 2.0e-3, and two forced steps were bit-identical where the stock steps between them were."""
    calls = _counting(monkeypatch)
    stock = [_lora_grads("stock", monkeypatch), _lora_grads("stock", monkeypatch)]
    assert len(calls) == 0
    large = _lora_grads("large", monkeypatch)
    assert len(calls) >= 10  # forward and backward-data of the ResNets' and the upsampler's convs
    stock.append(_lora_grads("stock", monkeypatch))

    def rel(a, b):
        return ((a - b).norm() / b.norm()).item()

    pairs = [rel(stock[i], stock[j]) for i, j in itertools.combinations(range(3), 2)]
    diffs = [rel(large, s) for s in stock]
    base, diff = sum(pairs) / 3, sum(diffs) / 3
    print(f"LoRA gradient rel L2: large vs stock {diff:.3e} ({diffs}), stock vs stock {base:.3e} ({pairs})")
    assert all(s.norm() > 0 for s in stock) and base > 0 and diff <= 4 * base, (diff, base)
