"""The pipelined chunk loop of the few-pixel 3×3 convolution (csrc/conv_small.hip: two LDS stage buffers, one barrier a chunk,
the position and the rows form of the staging) through `conv3x3_small_form`, against float64 on the CPU: the prologue, the steady
state and the tail (1 to 5 chunks a workgroup, both buffer parities), ragged K-slices, the rows form's geometry (half-image and
whole-image tiles, a last tile of one image, halo rows inside and outside the image), the position form over many chunks, the
64-pixel instantiation, rows against position bit for bit, determinism and containment.

Every case is few channels × many tiles.  `geo` restates conv_geo and each case asserts the tile, chunk and slice counts it was
built for, so a shape that stops exercising its case fails here.  The per-element bound is that of
tests/test_gpu_conv_small.py::_check_bound, restated.

A case (N, Ci, Co, H, W) names the KERNEL's problem: Ci channels in, Co out.  Forward, the weight is [Co, Ci, 3, 3]; backward-data,
it is the weight [Ci, Co, 3, 3] of a layer Co → Ci, packed with backward = 1, the input is that layer's dy and the result its dx."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}
POSITION, ROWS = 0, 1
UNSUPPORTED, BADARG = -5, -1
DTYPES = [torch.float16, torch.bfloat16]
DIRECTIONS = ["fwd", "bwd"]


def _nat():
    from diffusion_finetuning_amd import _native as nat
    return nat


def _positions(m0, MT, M, H, W):
    def q(m):
        img, r = divmod(m, H * W)
        h, w = divmod(r, W)
        return img * (H + 2) * (W + 2) + (h + 1) * (W + 2) + (w + 1)
    return q(min(m0 + MT, M) - 1) - q(m0) + 2 * (W + 3) + 1


def geo(N, Ci, Co, H, W):
    """conv_geo and rows_units of csrc/conv_small.hip, restated."""
    M = N * H * W
    for MT, per in ((128, 1), (64, 3)):
        mtiles = -(-M // MT)
        pmax = max(_positions(t * MT, MT, M, H, W) for t in range(mtiles))
        if pmax <= per * 256:
            break
    else:
        raise AssertionError("shape not covered")
    ntiles, chunks = -(-Co // 128), Ci // 32
    want = max(1, 256 // (mtiles * ntiles))
    cps = -(-chunks // want)
    if chunks >= 4 and cps < 2:
        cps = 2
    S = -(-chunks // cps)
    HW = H * W
    if MT != 128 or W % 8 or 128 % W:
        rows = 0
    elif 128 % HW == 0:
        rows = 1
    else:
        rows = 2 if HW % 128 == 0 and 256 + 4 * W <= 512 else 0
    return dict(MT=MT, mtiles=mtiles, ntiles=ntiles, chunks=chunks, S=S, pmax=pmax, rows=rows,
                slice_chunks=[min(cps, chunks - s * cps) for s in range(S)], last_tile_pixels=M - (mtiles - 1) * MT)


def _check_bound(got, ref64, absref64, terms, dtype, what):
    """|y − y64| ≤ u·|y64| + 2·terms·2⁻²⁴·(|x| ⊛ |w|) + tiny, per element."""
    err = (got.double().cpu() - ref64).abs()
    bound = U[dtype] * ref64.abs() + 2.0 * terms * 2.0 ** -24 * absref64 + TINY[dtype]
    worst = (err / bound).max().item()
    print(what, "error / bound", worst)
    assert worst <= 1.0, (what, "error / bound", worst)


def _ref64(x, w, direction):
    """float64 result and the |x| ⊛ |w| of its bound, on the CPU."""
    x64, w64 = x.double(), w.double()
    if direction == "fwd":
        return F.conv2d(x64, w64, None, padding=1), F.conv2d(x64.abs(), w64.abs(), None, padding=1)
    return F.conv_transpose2d(x64, w64, None, padding=1), F.conv_transpose2d(x64.abs(), w64.abs(), None, padding=1)


_REFS = {}


def _reference(shape, dtype, direction):
    """Operands and float64 results of one case, computed once and shared (never modified)."""
    key = (shape, dtype, direction)
    if key not in _REFS:
        N, Ci, Co, H, W = shape
        g = torch.Generator().manual_seed(sum(shape) + (direction == "bwd"))
        x = torch.randn(N, Ci, H, W, generator=g).to(dtype)
        wshape = (Co, Ci, 3, 3) if direction == "fwd" else (Ci, Co, 3, 3)
        w = (torch.randn(wshape, generator=g) / (3.0 * Ci ** 0.5)).to(dtype)
        b = torch.randn(Co, generator=g).to(dtype)
        y64, ya64 = _ref64(x, w, direction)
        _REFS[key] = dict(x=x, w=w, b=b, y64=y64, ya64=ya64)
    return _REFS[key]


def _status(nat, x, pack, y, Co, form):
    """conv3x3_small_form's status for a device x [N, Ci, H, W] (y, workspace as the wrapper makes them)."""
    N, Ci, H, W = x.shape
    code = nat.dtype_code(x.dtype)
    nbytes = int(nat.lib().conv3x3_small_workspace_bytes(N, Ci, Co, H, W, code))
    ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=x.device)
    return nat.lib().conv3x3_small_form(x.data_ptr(), pack.data_ptr(), None, y.data_ptr(), ws.data_ptr(), nbytes, N, Ci, Co, H, W,
                                        code, form, nat._stream(x))


def _forms(shape):
    return (POSITION, ROWS) if geo(*shape)["rows"] else (POSITION,)


def _run_forms(shape, dtype, direction, x, w, b, y64, ya64):
    """Every form that covers the shape against float64, with and without the bias, and the forms against each other."""
    nat = _nat()
    N, Ci, Co, H, W = shape
    S = geo(*shape)["S"]
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    pack = nat.conv3x3_small_pack(wd, direction == "bwd")
    bias64 = b.double()[None, :, None, None]
    outs = []
    for form in _forms(shape):
        what = shape + (str(dtype), direction, "rows" if form else "position")
        y = nat.conv3x3_small_form(xd, pack, None, Co, form)
        _check_bound(y, y64, ya64, 9 * Ci + S, dtype, what)
        yb = nat.conv3x3_small_form(xd, pack, bd, Co, form)
        _check_bound(yb, y64 + bias64, ya64 + bias64.abs(), 9 * Ci + S + 1, dtype, what + ("bias",))
        outs.append((y, yb))
    for y, yb in outs[1:]:
        assert torch.equal(y, outs[0][0]) and torch.equal(yb, outs[0][1]), (shape, "rows and position differ")
    # what conv3x3_small itself runs is one of them
    assert torch.equal(nat.conv3x3_small(xd, pack, bd, Co), outs[0][1])
    return outs


def _run_case(shape, dtype, direction):
    r = _reference(shape, dtype, direction)
    return _run_forms(shape, dtype, direction, r["x"], r["w"], r["b"], r["y64"], r["ya64"])


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Ci", [32, 64, 96, 128, 160])
def test_one_to_five_chunks_a_workgroup_on_half_image_tiles(Ci, dtype, direction):
    """65 images of 16×16: 130 tiles that are the top and the bottom half of an image (one halo row real, one outside), one
    channel tile, ONE slice that runs all chunks: one chunk is prologue and tail alone, odd and even counts end in either buffer.
    A tile stages 180 positions: 76 threads of the position form have none."""
    shape = (65, Ci, 32, 16, 16)
    g = geo(*shape)
    assert (g["MT"], g["mtiles"], g["ntiles"], g["S"], g["slice_chunks"]) == (128, 130, 1, 1, [Ci // 32])
    assert g["pmax"] == 180 and 256 - g["pmax"] == 76 and g["rows"] == 2
    assert len(_run_case(shape, dtype, direction)) == 2


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,Ci,slices,last", [(130, 160, [2, 2, 1], 128), (130, 224, [3, 3, 1], 128), (131, 160, [2, 2, 1], 64)])
def test_ragged_last_slice_on_whole_image_tiles(N, Ci, slices, last, dtype, direction):
    """8×8 images, two to a tile (131 images: the last tile is a single image), three K-slices of which the last is short."""
    shape = (N, Ci, 64, 8, 8)
    g = geo(*shape)
    assert (g["MT"], g["mtiles"], g["ntiles"], g["slice_chunks"]) == (128, -(-N // 2), 1, slices)
    assert g["last_tile_pixels"] == last and g["pmax"] == 200 and g["rows"] == 1
    assert len(_run_case(shape, dtype, direction)) == 2


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_position_form_with_five_chunks_where_the_rows_form_is_refused(dtype, direction):
    """115 images of 12×12: 130 tiles that start anywhere in a row, five chunks in one slice; W % 8 != 0, so no rows form."""
    nat = _nat()
    shape = (115, 160, 32, 12, 12)
    g = geo(*shape)
    assert (g["MT"], g["mtiles"], g["ntiles"], g["slice_chunks"], g["rows"]) == (128, 130, 1, [5], 0)
    assert len(_run_case(shape, dtype, direction)) == 1
    x = torch.zeros(115, 160, 12, 12, dtype=dtype, device=DEV)
    pack = torch.zeros(160 * 32 * 9, dtype=dtype, device=DEV)
    y = torch.full((115, 32, 12, 12), 7.0, dtype=dtype, device=DEV)
    assert _status(nat, x, pack, y, 32, ROWS) == UNSUPPORTED
    assert _status(nat, x, pack, y, 32, 2) == BADARG and _status(nat, x, pack, y, 32, -1) == BADARG
    torch.cuda.synchronize()
    assert (y == 7.0).all()  # nothing was launched
    assert nat.conv3x3_small_form_choice(115, 160, 32, 12, 12, dtype) == POSITION
    assert nat.conv3x3_small_form_choice(115, 160, 32, 12, 12, torch.float32) == -1


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_64_pixel_instantiation_with_three_chunks_a_slice(dtype, direction):
    """One image of 20×280: 88 tiles of 64 pixels (three positions a thread, 2 × 60 KB of LDS), two slices of three chunks."""
    shape = (1, 192, 32, 20, 280)
    g = geo(*shape)
    assert (g["MT"], g["mtiles"], g["ntiles"], g["slice_chunks"], g["rows"]) == (64, 88, 1, [3, 3], 0)
    assert len(_run_case(shape, dtype, direction)) == 1


ROWS_SHAPES = [(3, 32, 64, 16, 16), (5, 32, 64, 8, 8)]  # half-image tiles; whole-image tiles with a last tile of one image


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ROWS_SHAPES)
def test_each_tap_and_each_border_row_and_column_by_itself(shape, dtype):
    """A weight that is non-zero in ONE tap (channel-dependent values) against single lit pixels in every corner, on every border,
    on the rows either side of the half-image cut and inside: a shifted tap, a border position that is not zero, a halo row that
    was not staged or a wrong backward pack fails by itself.  Small integers: exact in 16 bits."""
    nat = _nat()
    N, Ci, Co, H, W = shape
    assert geo(*shape)["rows"] and geo(N, Co, Ci, H, W)["rows"]
    g = torch.Generator().manual_seed(5)
    pixels = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 2), (H - 1, 3), (H // 2, 0), (H // 2 - 1, W - 1), (H // 2 - 1, 2),
              (H // 2, 5)]
    x = torch.zeros(N, Ci, H, W)
    dy = torch.zeros(N, Co, H, W)
    for n in range(N):  # every image has every lit pixel, with its own values
        for h, ww in pixels:
            x[n, :, h, ww] = torch.randint(-2, 3, (Ci,), generator=g).float()
            dy[n, :, h, ww] = torch.randint(-2, 3, (Co,), generator=g).float()
    xd, dyd = x.to(dtype).to(DEV), dy.to(dtype).to(DEV)
    for tap in range(9):
        w = torch.zeros(Co, Ci, 3, 3)
        w[:, :, tap // 3, tap % 3] = torch.randint(-3, 4, (Co, Ci), generator=g).float()
        wd = w.to(dtype).to(DEV)
        fwd, bwd = nat.conv3x3_small_pack(wd, False), nat.conv3x3_small_pack(wd, True)
        y64, dx64 = F.conv2d(x.double(), w.double(), padding=1), F.conv_transpose2d(dy.double(), w.double(), padding=1)
        for form in (POSITION, ROWS):
            assert torch.equal(nat.conv3x3_small_form(xd, fwd, None, Co, form).double().cpu(), y64), ("fwd tap", tap, form)
            assert torch.equal(nat.conv3x3_small_form(dyd, bwd, None, Ci, form).double().cpu(), dx64), ("bwd tap", tap, form)


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(5, 64, 32, 16, 16), (7, 64, 32, 8, 8)])
def test_large_border_pixels_and_a_zero_interior(shape, dtype, direction):
    """The outermost ring of every image is large (and differs from image to image), everything inside it is zero: a halo row or
    a border position staged from the neighbouring image, or left over from the other buffer, is an error far above the bound."""
    N, Ci, Co, H, W = shape
    g = torch.Generator().manual_seed(17 + (direction == "bwd"))
    x = torch.randn(N, Ci, H, W, generator=g) * 64.0
    x[:, :, 1:H - 1, 1:W - 1] = 0.0
    x = x.to(dtype)
    w = (torch.randn((Co, Ci, 3, 3) if direction == "fwd" else (Ci, Co, 3, 3), generator=g) / (3.0 * Ci ** 0.5)).to(dtype)
    b = torch.randn(Co, generator=g).to(dtype)
    y64, ya64 = _ref64(x, w, direction)
    assert len(_run_forms(shape, dtype, direction, x, w, b, y64, ya64)) == 2


@pytest.mark.parametrize("form", [POSITION, ROWS])
@pytest.mark.parametrize("shape", [(3, 96, 64, 16, 16), (5, 96, 64, 8, 8)])
def test_two_calls_and_a_replayed_capture_give_the_same_bits(shape, form):
    nat = _nat()
    N, Ci, Co, H, W = shape
    r = _reference(shape, torch.float16, "fwd")
    x, w, b = (r[k].to(DEV) for k in ("x", "w", "b"))
    pack = nat.conv3x3_small_pack(w, False)
    y1, y2 = nat.conv3x3_small_form(x, pack, b, Co, form), nat.conv3x3_small_form(x, pack, b, Co, form)
    assert torch.equal(y1, y2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            yc = nat.conv3x3_small_form(x, pack, b, Co, form)
    torch.cuda.current_stream().wait_stream(side)
    yc.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yc, y1)


@pytest.mark.parametrize("form", [POSITION, ROWS])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 96, 64, 16, 16), (5, 96, 64, 8, 8)])
def test_nothing_is_written_outside_y_and_the_workspace(shape, dtype, form):
    """x, the pack, y and the workspace sit inside canary-filled buffers, the workspace exactly as large as the library says: every
    canary is intact afterwards (the unconditional stage writes stay in LDS), x and the pack are unchanged."""
    nat = _nat()
    N, Ci, Co, H, W = shape
    r = _reference(shape, dtype, "fwd")
    x, w, b = (r[k].to(DEV) for k in ("x", "w", "b"))
    code = nat.dtype_code(dtype)
    ws_bytes = int(nat.lib().conv3x3_small_workspace_bytes(N, Ci, Co, H, W, code))
    assert ws_bytes > 0
    pad = 4096  # elements / floats of canary on either side (a multiple of 16 bytes)
    canary16 = torch.tensor(-1234.0, dtype=dtype).item()

    def framed(n, dt, fill):
        buf = torch.full((n + 2 * pad,), fill, dtype=dt, device=DEV)
        return buf, buf[pad:pad + n]

    xbuf, xv = framed(x.numel(), dtype, canary16)
    pbuf, pv = framed(w.numel(), dtype, canary16)
    ybuf, yv = framed(N * Co * H * W, dtype, canary16)
    wbuf, wv = framed(ws_bytes // 4, torch.float32, -4321.0)
    xv.copy_(x.flatten())
    pv.copy_(nat.conv3x3_small_pack(w, False))
    packed = pv.clone()
    st = nat.lib().conv3x3_small_form(xv.data_ptr(), pv.data_ptr(), b.data_ptr(), yv.data_ptr(), wv.data_ptr(), ws_bytes, N, Ci, Co,
                                      H, W, code, form, nat._stream(x))
    assert st == 0
    torch.cuda.synchronize()
    for name, buf, fill in (("x", xbuf, canary16), ("pack", pbuf, canary16), ("y", ybuf, canary16), ("workspace", wbuf, -4321.0)):
        assert (buf[:pad] == fill).all() and (buf[-pad:] == fill).all(), name
    assert torch.equal(xv, x.flatten()) and torch.equal(pv, packed)
    assert torch.equal(yv.view(N, Co, H, W), nat.conv3x3_small_form(x, packed, b, Co, 1 - form))
    assert nat.lib().conv3x3_small_form(xv.data_ptr(), pv.data_ptr(), None, yv.data_ptr(), wv.data_ptr(), ws_bytes - 1, N, Ci, Co, H, W,
                                        code, form, nat._stream(x)) == BADARG
