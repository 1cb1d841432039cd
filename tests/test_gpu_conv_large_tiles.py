"""The pixel-heavy tiles of the many-pixel 3×3 convolution (csrc/conv_large.hip: 256 and 128 pixels × 80 channels, rows-form
staging with 16-byte loads) through `conv3x3_large_tile`, against float64 on the CPU: every row width at which the lane → unit
map takes another path (W = 8: one segment a row; 16: two; 32 and 64: segment bits above the channel pair), ragged channel
tiles, every start chunk of the rotated K loop, halo rows at the top, in the middle and at the bottom of an image, each tap
and border column by itself, the refusals, containment and determinism.  The per-element bound is that of
tests/test_gpu_conv_large.py::_check_bound, restated.

Channel counts: the pack (conv3x3_small_pack) takes multiples of 32 only, in both channel counts, because backward-data swaps
them; so where one 80-channel tile "exactly" or 2.2 of them were wanted (80, 176) the cases use 96 and 192: ragged past one and
past two tiles, with 160 as the count that fills its tiles exactly."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}
TILE_PIXELS = {1: 256, 2: 128}
UNSUPPORTED, BADARG = -5, -1

# ((N, C_in, C_out, H, W), tile)
CASES = [
    ((1, 64, 96, 32, 8), 1),    # one 256-pixel tile an image, C_out ragged past one 80-tile, two chunks
    ((1, 64, 96, 32, 8), 2),
    ((2, 64, 160, 32, 8), 1),   # two images, two full channel tiles
    ((2, 64, 160, 32, 8), 2),
    ((2, 32, 96, 16, 16), 1),   # W = 16: two segments a row
    ((2, 32, 96, 16, 16), 2),
    ((3, 96, 192, 16, 8), 2),   # three images = three tiles, three chunks: the rotated K start mt % chunks takes every value
    ((1, 32, 96, 48, 8), 2),    # three tiles in one image: halo rows above the image, inside it on both sides, below it
    ((1, 32, 96, 4, 32), 2),    # W = 32 and 64, the widths of the UNet's levels: segment bits above the channel pair
    ((1, 32, 96, 8, 32), 1),
    ((1, 32, 96, 2, 64), 2),
    ((2, 32, 96, 4, 64), 1),
]


def _nat():
    from diffusion_finetuning_amd import _native as nat
    return nat


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
    print(what, "error / bound", worst)
    assert worst <= 1.0, (what, "error / bound", worst)


_REFS = {}


def _reference(shape, dtype):
    """Operands and float64 results of one shape, computed once and shared (never modified)."""
    key = (shape, dtype)
    if key not in _REFS:
        N, Cin, Cout, H, W = shape
        x, w, b, dy = _operands(N, Cin, Cout, H, W, dtype, sum(shape))
        x64, w64, b64, dy64 = x.double(), w.double(), b.double(), dy.double()
        _REFS[key] = dict(
            x=x, w=w, b=b, dy=dy, b64=b64,
            y64=F.conv2d(x64, w64, None, padding=1), ya64=F.conv2d(x64.abs(), w64.abs(), None, padding=1),
            dx64=F.conv_transpose2d(dy64, w64, None, padding=1), dxa64=F.conv_transpose2d(dy64.abs(), w64.abs(), None, padding=1))
    return _REFS[key]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape,tile", CASES)
def test_rows_form_tiles_against_float64_both_directions(shape, tile, dtype):
    nat = _nat()
    N, Cin, Cout, H, W = shape
    assert (H * W) % TILE_PIXELS[tile] == 0 and TILE_PIXELS[tile] % W == 0 and W % 8 == 0
    r = _reference(shape, dtype)
    xd, wd, bd, dyd = (r[k].to(DEV) for k in ("x", "w", "b", "dy"))
    fwd, bwd = nat.conv3x3_small_pack(wd, False), nat.conv3x3_small_pack(wd, True)
    what = shape + (tile, str(dtype))
    y = nat.conv3x3_large_tile(xd, fwd, None, Cout, tile)
    _check_bound(y, r["y64"], r["ya64"], 9 * Cin + 1, dtype, what + ("fwd",))
    yb = nat.conv3x3_large_tile(xd, fwd, bd, Cout, tile)
    bias64 = r["b64"][None, :, None, None]
    _check_bound(yb, r["y64"] + bias64, r["ya64"] + bias64.abs(), 9 * Cin + 2, dtype, what + ("fwd+bias",))
    dx = nat.conv3x3_large_tile(dyd, bwd, None, Cin, tile)
    _check_bound(dx, r["dx64"], r["dxa64"], 9 * Cout + 1, dtype, what + ("bwd",))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape,tile", [((1, 32, 96, 16, 8), 2), ((1, 32, 96, 16, 16), 1)])
def test_each_tap_and_each_border_column_by_itself(shape, tile, dtype):
    """A weight that is non-zero in ONE tap (channel-dependent values) against single lit pixels in every corner, on every
    border and inside: a shifted tap, a padding column that is not zero or a wrong backward pack fails by itself.  Small
    integers: exact in 16 bits."""
    nat = _nat()
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
        y = nat.conv3x3_large_tile(x.to(dtype).to(DEV), nat.conv3x3_small_pack(wd, False), None, Cout, tile)
        dx = nat.conv3x3_large_tile(dy.to(dtype).to(DEV), nat.conv3x3_small_pack(wd, True), None, Cin, tile)
        assert torch.equal(y.double().cpu(), F.conv2d(x.double(), w.double(), padding=1)), ("fwd tap", tap)
        assert torch.equal(dx.double().cpu(), F.conv_transpose2d(dy.double(), w.double(), padding=1)), ("bwd tap", tap)


def _framed(n, dtype, canary, pad=4096):
    buf = torch.full((n + 2 * pad,), canary, dtype=dtype, device=DEV)
    return buf, buf[pad:pad + n]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_a_tile_whose_conditions_fail_is_refused_and_nothing_is_written(dtype):
    nat = _nat()
    code = nat.dtype_code(dtype)
    canary = torch.tensor(-1234.0, dtype=dtype).item()
    refused = [
        ((1, 32, 96, 64, 6), 1), ((1, 32, 96, 64, 6), 2),    # W = 6: no 16-byte segments (384 pixels)
        ((1, 32, 96, 20, 8), 2), ((1, 32, 96, 48, 8), 1),    # W = 8, H·W no multiple of the tile
        ((2, 32, 96, 24, 8), 2), ((2, 32, 96, 48, 8), 1),    # the second tile would straddle the two images
        ((1, 32, 96, 2, 128), 2),                            # one row fills the tile: two units a thread do not cover the halo
    ]
    for shape, tile in refused:
        N, Cin, Cout, H, W = shape
        x, w, b, _ = (t.to(DEV) for t in _operands(N, Cin, Cout, H, W, dtype, 1))
        pack = nat.conv3x3_small_pack(w, False)
        ybuf, yv = _framed(N * Cout * H * W, dtype, canary)
        st = nat.lib().conv3x3_large_tile(x.data_ptr(), pack.data_ptr(), b.data_ptr(), yv.data_ptr(), None, 0, N, Cin, Cout, H, W,
                                          code, tile, nat._stream(x))
        torch.cuda.synchronize()
        assert st == UNSUPPORTED, (shape, tile, st)
        assert (ybuf == canary).all(), (shape, tile)
        with pytest.raises(RuntimeError):
            nat.conv3x3_large_tile(x, pack, b, Cout, tile)
        # the same shape on the shape rule's tile runs
        assert nat.lib().conv3x3_large_tile(x.data_ptr(), pack.data_ptr(), b.data_ptr(), yv.data_ptr(), None, 0, N, Cin, Cout, H, W,
                                            code, 0, nat._stream(x)) == 0
        assert torch.equal(yv.view(N, Cout, H, W), nat.conv3x3_large(x, pack, b, Cout))
    x, w, b, _ = (t.to(DEV) for t in _operands(1, 32, 96, 16, 8, dtype, 1))
    pack = nat.conv3x3_small_pack(w, False)
    ybuf, yv = _framed(96 * 128, dtype, canary)
    for tile in (-1, 3):  # an unknown tile
        assert nat.lib().conv3x3_large_tile(x.data_ptr(), pack.data_ptr(), b.data_ptr(), yv.data_ptr(), None, 0, 1, 32, 96, 16, 8,
                                            code, tile, nat._stream(x)) == BADARG
    torch.cuda.synchronize()
    assert (ybuf == canary).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape,tile", [((1, 64, 96, 32, 8), 1), ((3, 96, 192, 16, 8), 2), ((1, 32, 96, 48, 8), 2), ((2, 32, 96, 4, 64), 1)])
def test_the_kernel_writes_only_inside_y(shape, tile, dtype):
    """x, the pack and y sit inside canary-filled buffers: every canary is intact afterwards, x and the pack are unchanged and
    every element of y was written."""
    nat = _nat()
    N, Cin, Cout, H, W = shape
    x, w, b, _ = (t.to(DEV) for t in _operands(N, Cin, Cout, H, W, dtype, 7))
    code = nat.dtype_code(dtype)
    canary = torch.tensor(-1234.0, dtype=dtype).item()
    xbuf, xv = _framed(x.numel(), dtype, canary)
    pbuf, pv = _framed(w.numel(), dtype, canary)
    ybuf, yv = _framed(N * Cout * H * W, dtype, canary)
    xv.copy_(x.flatten())
    assert nat.lib().conv3x3_small_pack(w.data_ptr(), pv.data_ptr(), Cin, Cout, 0, code, nat._stream(x)) == 0
    packed = pv.clone()
    st = nat.lib().conv3x3_large_tile(xv.data_ptr(), pv.data_ptr(), b.data_ptr(), yv.data_ptr(), None, 0, N, Cin, Cout, H, W, code,
                                      tile, nat._stream(x))
    assert st == 0
    torch.cuda.synchronize()
    pad = 4096
    for name, buf in (("x", xbuf), ("pack", pbuf), ("y", ybuf)):
        assert (buf[:pad] == canary).all() and (buf[-pad:] == canary).all(), name
    assert torch.equal(xv, x.flatten()) and torch.equal(pv, packed)
    assert not (yv == canary).any()
    assert torch.equal(yv.view(N, Cout, H, W), nat.conv3x3_large_tile(x, packed, b, Cout, tile))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape,tile", [((2, 64, 160, 32, 8), 1), ((3, 96, 192, 16, 8), 2)])
def test_two_calls_and_a_replayed_capture_give_the_same_bits(shape, tile, dtype):
    nat = _nat()
    N, Cin, Cout, H, W = shape
    x, w, b, dy = (t.to(DEV) for t in _operands(N, Cin, Cout, H, W, dtype, 3))
    fwd, bwd = nat.conv3x3_small_pack(w, False), nat.conv3x3_small_pack(w, True)
    y1, y2 = nat.conv3x3_large_tile(x, fwd, b, Cout, tile), nat.conv3x3_large_tile(x, fwd, b, Cout, tile)
    d1, d2 = nat.conv3x3_large_tile(dy, bwd, None, Cin, tile), nat.conv3x3_large_tile(dy, bwd, None, Cin, tile)
    assert torch.equal(y1, y2) and torch.equal(d1, d2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            yc = nat.conv3x3_large_tile(x, fwd, b, Cout, tile)
            dc = nat.conv3x3_large_tile(dy, bwd, None, Cin, tile)
    torch.cuda.current_stream().wait_stream(side)
    yc.zero_(), dc.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yc, y1) and torch.equal(dc, d1)
