"""The fused GroupNorm kernels (csrc/norm.hip) where test_gpu_norm.py does not go: statistics that are hard in fp32, the
planners' and tails' corner geometry (tests/norm_cases.py), writes outside the tensors and the workspace, and the front's
promise that whatever the kernels do not take gets the stock composite.

Yardsticks, all against float64 math on the same stored inputs, every figure printed before it is asserted:
  Y1  fused max and RMS error ≤ the same-dtype stock composite's + 1 ulp of the storage type (the sibling module's yardstick);
  Y2  the same against the stock composite run in fp32 on the upcast inputs with its results rounded once to the storage type:
      both sides are then fp32 computations rounded once, and one storage ulp is 2¹³ (f16) / 2¹⁶ (bf16) fp32 ulps, out of reach
      of summation order or the fast exp / rcp;
  Y3  the kernels' own mean / rstd outputs: |rstd/rstd₆₄ − 1| ≤ 2⁻¹³ and |mean − mean₆₄| ≤ 2⁻¹³/rstd₆₄, an eighth of f16's
      relative spacing, so that the statistics cannot move an output by more than a quarter ulp."""
import pytest
import torch
import torch.nn.functional as F

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd.norm import _hip_layout, group_norm_act
from tests.norm_cases import BIG_GROUP, NCHW_GEOMETRY, NHWC_GEOMETRY, SMALL_GROUPS
from tests.test_gpu_norm import VARIANTS, _composite, _errs, _run, _ulp

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
LAYOUTS = pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
Y3_BOUND = 2.0 ** -13
_id = lambda c: "n%d-c%d-g%d-%dx%d" % c


def _to_layout(t, channels_last):
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t.contiguous()


def _inputs_hw(shape, dtype, channels_last, seed):
    """`_inputs` of the sibling module (per-channel spread and offset of order 1) for a non-square map."""
    N, C, _, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    x = _to_layout((rn(N, C, H, W) * (0.5 + rn(1, C, 1, 1).abs()) + rn(1, C, 1, 1)).to(dtype), channels_last)
    a = (0.5 * rn(N, C)).to(dtype)
    w, b = (1 + 0.2 * rn(C)).to(dtype), (0.2 * rn(C)).to(dtype)
    dy = _to_layout(rn(N, C, H, W).to(dtype), channels_last)
    return x, a, w, b, dy


def _same_strides(t, x):
    return all(st == sx for st, sx, n in zip(t.stride(), x.stride(), x.shape) if n > 1)


def _check_y1_y2(tag, x, a, w, b, dy, G, eps, act, channels_last, bad):
    """Runs the fused op, the stock composite in the storage type and in fp32, and float64; prints the figures and appends every
    miss of Y1 / Y2 to `bad`.  Returns the fused (y, dx[, da])."""
    dtype = x.dtype
    assert _hip_layout(x, G, w, b, a) == int(channels_last), tag  # the HIP path is what is measured
    f64 = lambda t: None if t is None else t.double()
    f32 = lambda t: None if t is None else t.float()
    ref = _run(_composite(G, w.double(), b.double(), eps, act), f64(x), f64(a), dy.double())
    stock = _run(_composite(G, w, b, eps, act), x, a, dy)
    stock32 = [t.to(dtype) for t in _run(_composite(G, w.float(), b.float(), eps, act), f32(x), f32(a), dy.float())]
    fused = _run(lambda xx, aa: group_norm_act(xx, G, w, b, eps, act, aa), x, a, dy)
    assert _same_strides(fused[0], x) and _same_strides(fused[1], x), tag
    for name, f, s, s32, r in zip(("y", "dx", "da"), fused, stock, stock32, ref):
        assert torch.isfinite(f).all(), (tag, name)
        (fmax, frms), (smax, srms), (tmax, trms), ulp = _errs(f, r), _errs(s, r), _errs(s32, r), _ulp(r, dtype)
        print(f"{tag} act={int(act)} a={int(a is not None)} eps={eps:g} {name}: fused max {fmax:.3e} rms {frms:.3e} | "
              f"stock max {smax:.3e} rms {srms:.3e} | fp32-stock max {tmax:.3e} rms {trms:.3e} | ulp {ulp:.3e}")
        if not (fmax <= smax + ulp and frms <= srms + ulp):
            bad.append(("Y1", tag, name, act, a is not None, eps, fmax, frms, smax, srms, ulp))
        if not (fmax <= tmax + ulp and frms <= trms + ulp):
            bad.append(("Y2", tag, name, act, a is not None, eps, fmax, frms, tmax, trms, ulp))
    return fused


def _check_y3(tag, x, a, w, b, G, eps, act, channels_last, bad):
    """mean / rstd as group_norm_act_fwd returns them against float64 moments of the stored x + a."""
    N, C = x.shape[:2]
    _, mean, rstd = nat.group_norm_act_fwd(x, a, w, b, G, eps, act, int(channels_last))
    h = x.double() if a is None else x.double() + a.double()[:, :, None, None]
    h = h.reshape(N, G, -1)
    mean64 = h.mean(-1)
    rstd64 = ((h - mean64[..., None]).pow(2).mean(-1) + eps).rsqrt()
    e_r = (rstd.double() / rstd64 - 1).abs().max().item()
    e_m = ((mean.double() - mean64).abs() * rstd64).max().item()
    print(f"{tag} act={int(act)} a={int(a is not None)} eps={eps:g} stats: |rstd/rstd64 - 1| {e_r:.3e}  "
          f"|mean - mean64|*rstd64 {e_m:.3e}  bound {Y3_BOUND:.3e}")
    if not (e_r <= Y3_BOUND and e_m <= Y3_BOUND):
        bad.append(("Y3", tag, act, a is not None, eps, e_r, e_m, Y3_BOUND))
    return mean, rstd


# ------------------------------------------------------------------------------------------------------ 1. hard statistics
def _first_of_group(t, G, value, c_off=0, h=0, w=0):
    cpg = t.shape[1] // G
    for g in range(G):
        t[:, g * cpg + c_off, h, w] = value


def _hard_case(kind, shape, dtype, channels_last, seed):
    """x, a, w, b, dy and the variants (act, with_a, eps) of one hard-statistics case."""
    N, C, G, H, W = shape
    x, a, w, b, dy = _inputs_hw(shape, dtype, channels_last, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1000)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    variants = VARIANTS
    name, *args = kind
    if name == "mean":  # x = m + σ·randn, σ still resolved by the storage type at m
        m, sigma = args
        x = m + sigma * rn(N, C, H, W)
    elif name in ("first", "other"):  # one element of every group far from the rest: at the group's first position, or not
        sigma, value = args
        x = sigma * rn(N, C, H, W)
        _first_of_group(x, G, value, *((0, 0, 0) if name == "first" else (1, 3, 5)))
    elif name == "addend":  # the addend of each group's first channel carries the outlier, x is plain
        sigma, value = args
        x = sigma * rn(N, C, H, W)
        a = a.clone()
        _first_of_group(a[:, :, None, None], G, value)
        variants = [v for v in VARIANTS if v[1]]
    elif name == "constant":  # zero variance: x + a is one constant per (n, group), exact in both 16-bit types
        k = (torch.arange(N * G, device="cuda").reshape(N, G, 1) % 13 - 6) / 4
        x = k.expand(N, G, C // G).reshape(N, C, 1, 1).expand(N, C, H, W).clone()
        a = ((torch.arange(N * G, device="cuda").reshape(N, G, 1) % 5 - 2) / 2).expand(N, G, C // G).reshape(N, C).to(dtype)
        dy = dy / 64  # rstd = eps^-½ is up to 1000 here: da ≈ rstd·Σ_hw dz would pass f16's largest number at 64×64
    elif name == "tiny":  # variance below eps
        sigma, eps = args
        x = sigma * rn(N, C, H, W)
        a = (sigma * rn(N, C)).to(dtype)
        variants = [(act, with_a, eps) for act, with_a, _ in VARIANTS[:4]]
    elif name == "saturated":  # |x̂γ+β| passes 88 (fp32 exp overflows) on both sides
        sign = lambda: torch.where(rn(C) < 0, -1.0, 1.0)
        w, b = (40 * sign()).to(dtype), (20 * sign()).to(dtype)
    else:
        raise AssertionError(kind)
    return _to_layout(x.to(dtype), channels_last), a, w, b, dy, variants


HARD_F16 = [("mean", 200, 0.5), ("mean", 1000, 2), ("mean", -3000, 4)]
HARD_BF16 = [("mean", 200, 4), ("mean", 1000, 16)]
HARD_BOTH = [("first", 0.02, 60), ("first", 0.02, 8), ("first", 0.2, 60), ("addend", 0.02, 60), ("other", 0.02, 60),
             ("constant",), ("tiny", 1e-3, 1e-5), ("saturated",)]
HARD = [(torch.float16, k) for k in HARD_F16 + HARD_BOTH] + [(torch.bfloat16, k) for k in HARD_BF16 + HARD_BOTH]


@LAYOUTS
@pytest.mark.parametrize("shape", [BIG_GROUP, SMALL_GROUPS], ids=_id)
@pytest.mark.parametrize("dtype,kind", HARD, ids=lambda v: str(v).replace("torch.", "") if isinstance(v, torch.dtype)
                         else "-".join(str(p) for p in v))
def test_hard_statistics_against_float64(dtype, kind, shape, channels_last):
    N, C, G, H, W = shape
    x, a, w, b, dy, variants = _hard_case(kind, shape, dtype, channels_last, 300)
    tag = f"{kind} {shape} cl={int(channels_last)} {dtype}"
    bad = []
    for act, with_a, eps in variants:
        aa = a if with_a else None
        fused = _check_y1_y2(tag, x, aa, w, b, dy, G, eps, act, channels_last, bad)
        mean, rstd = _check_y3(tag, x, aa, w, b, G, eps, act, channels_last, bad)
        if kind[0] == "constant":  # x̂ = 0: y = act(β) rounded once, rstd = eps^-½
            beta = b.float()[None, :, None, None].expand_as(x)
            want = (F.silu(beta) if act else beta).to(dtype)
            ulp = _ulp(want.double(), dtype)
            assert (fused[0].double() - want.double()).abs().max().item() <= ulp, tag
            assert ((rstd.double() * eps ** 0.5) - 1).abs().max().item() <= Y3_BOUND, tag
        if kind[0] == "saturated" and act:  # −0 / 0 where SiLU's limit is below every representable magnitude
            ref_y = F.silu(F.group_norm(x.double() if aa is None else x.double() + aa.double()[:, :, None, None], G,
                                        w.double(), b.double(), eps))
            gone = ref_y.abs() < (2.0 ** -26 if dtype == torch.float16 else 2.0 ** -152)  # half the smallest subnormal, halved
            print(f"{tag} a={int(with_a)}: {int(gone.sum())} outputs below the smallest subnormal, "
                  f"max |x̂γ+β| {F.group_norm(x.double(), G, w.double(), b.double(), eps).abs().max().item():.1f}")
            assert (fused[0][gone] == 0).all(), tag
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ 2. geometry
GEOMETRY = [(False, s) for s in NCHW_GEOMETRY] + [(True, s) for s in NHWC_GEOMETRY]
GEOMETRY_IDS = [("nhwc-" if cl else "nchw-") + _id(s) for cl, s in GEOMETRY]


@DTYPES
@pytest.mark.parametrize("channels_last,shape", GEOMETRY, ids=GEOMETRY_IDS)
def test_planner_and_tail_geometry_against_float64(channels_last, shape, dtype):
    G = shape[2]
    bad = []
    for vi, (act, with_a, eps) in enumerate(VARIANTS):
        x, a, w, b, dy = _inputs_hw(shape, dtype, channels_last, 500 + vi)
        a = a if with_a else None
        tag = f"{shape} cl={int(channels_last)} {dtype}"
        _check_y1_y2(tag, x, a, w, b, dy, G, eps, act, channels_last, bad)
        _check_y3(tag, x, a, w, b, G, eps, act, channels_last, bad)
    assert not bad, bad


# -------------------------------------------------------------------------------------------------------------- 3. bounds
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


def _memory_order(t, channels_last):
    return (t.permute(0, 2, 3, 1) if channels_last else t).reshape(-1)


@DTYPES
@pytest.mark.parametrize("want_da", [0, 1], ids=["no-da", "da"])
@pytest.mark.parametrize("channels_last,shape", GEOMETRY, ids=GEOMETRY_IDS)
def test_kernels_write_only_inside_their_tensors_and_the_workspace_formula_covers_them(channels_last, shape, want_da, dtype):
    """The C entry points called as _native calls them, every operand inside a larger sentinel-filled buffer and the workspace
    exactly group_norm_act_workspace_bytes(…, want_da) long: the results equal the plain call's bit for bit and no guard byte
    changes."""
    N, C, G, H, W = shape
    cl, HW, code, eps, act = int(channels_last), H * W, nat.dtype_code(dtype), 1e-5, 1
    x, a, w, b, dy = _inputs_hw(shape, dtype, channels_last, 700)
    y0, mean0, rstd0 = nat.group_norm_act_fwd(x, a, w, b, G, eps, True, cl)
    dx0, da0 = nat.group_norm_act_bwd(dy, x, a, w, b, mean0, rstd0, G, True, cl, bool(want_da))

    lib, size = nat.lib(), x.element_size()
    ws_fwd = lib.group_norm_act_workspace_bytes(N, C, HW, G, cl, 0)
    ws_bwd = lib.group_norm_act_workspace_bytes(N, C, HW, G, cl, want_da)
    assert ws_fwd > 0 and ws_bwd >= ws_fwd and ws_fwd % 16 == 0 and ws_bwd % 16 == 0
    gx, gdy = _Guarded(x.numel() * size, dtype, _memory_order(x, cl)), _Guarded(x.numel() * size, dtype, _memory_order(dy, cl))
    ga, gw, gb = _Guarded(N * C * size, dtype, a), _Guarded(C * size, dtype, w), _Guarded(C * size, dtype, b)
    gy, gdx, gda = _Guarded(x.numel() * size, dtype), _Guarded(x.numel() * size, dtype), _Guarded(N * C * size, dtype)
    gmean, grstd = _Guarded(N * G * 4, torch.float32), _Guarded(N * G * 4, torch.float32)
    gws_f, gws_b = _Guarded(ws_fwd, torch.uint8), _Guarded(ws_bwd, torch.uint8)
    stream = nat._stream(x)
    st = lib.group_norm_act_fwd(gx.ptr(), ga.ptr(), gw.ptr(), gb.ptr(), gy.ptr(), gmean.ptr(), grstd.ptr(), gws_f.ptr(), N, C, HW,
                                G, eps, act, cl, code, stream)
    assert st == 0
    st = lib.group_norm_act_bwd(gdy.ptr(), gx.ptr(), ga.ptr(), gw.ptr(), gb.ptr(), gmean.ptr(), grstd.ptr(), gdx.ptr(),
                                gda.ptr() if want_da else None, gws_b.ptr(), N, C, HW, G, act, cl, code, stream)
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(gy.t, _memory_order(y0, cl)) and torch.equal(gdx.t, _memory_order(dx0, cl))
    assert torch.equal(gmean.t, mean0.reshape(-1)) and torch.equal(grstd.t, rstd0.reshape(-1))
    if want_da:
        assert torch.equal(gda.t, da0.reshape(-1))
    else:
        assert da0 is None and bool((gda.t.view(torch.uint8) == SENTINEL).all())
    # inputs unchanged, every guard intact
    assert torch.equal(gx.t, _memory_order(x, cl)) and torch.equal(gdy.t, _memory_order(dy, cl)) and torch.equal(ga.t, a.reshape(-1))
    for name, g in (("x", gx), ("dy", gdy), ("a", ga), ("gamma", gw), ("beta", gb), ("y", gy), ("dx", gdx), ("da", gda),
                    ("mean", gmean), ("rstd", grstd), ("workspace fwd", gws_f), ("workspace bwd", gws_b)):
        assert g.guards_intact(), name


# ----------------------------------------------------------------------------------------------------------- 4. the front
FRONT_SHAPES = {False: (2, 66, 2, 8, 17), True: (2, 64, 4, 7, 143)}  # non-square, more than one apply block each


@LAYOUTS
def test_addend_gradient_skipped_gives_the_same_y_and_dx(channels_last):
    """needs_input_grad[1] false → da is a null pointer (the DA = false statistics template in NHWC): y and dx bit for bit."""
    shape = FRONT_SHAPES[channels_last]
    G = shape[2]
    x, a, w, b, dy = _inputs_hw(shape, torch.float16, channels_last, 9)
    xs = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    y = group_norm_act(xs, G, w, b, 1e-5, True, a)
    (dx,) = torch.autograd.grad(y, [xs], dy)
    full = _run(lambda xx, aa: group_norm_act(xx, G, w, b, 1e-5, True, aa), x, a, dy)
    assert torch.equal(y.detach(), full[0]) and torch.equal(dx, full[1])
    assert y.stride() == x.stride() and dx.stride() == x.stride()  # a non-square result keeps x's strides


@LAYOUTS
def test_strided_and_expanded_addends_equal_their_contiguous_copies(channels_last):
    shape = FRONT_SHAPES[channels_last]
    N, C, G = shape[:3]
    x, a, w, b, dy = _inputs_hw(shape, torch.float16, channels_last, 10)
    fn = lambda xx, aa: group_norm_act(xx, G, w, b, 1e-5, True, aa)
    big = torch.zeros(N, 2 * C, dtype=a.dtype, device="cuda")
    big[:, ::2] = a
    strided, expanded = big[:, ::2], a[:1, :].expand(N, C)
    assert not strided.is_contiguous() and not expanded.is_contiguous()
    for view in (strided, expanded):
        assert _hip_layout(x, G, w, b, view) == int(channels_last)
        got, want = _run(fn, x, view, dy), _run(fn, x, view.contiguous(), dy)
        assert len(got) == 3 and all(torch.equal(u, v) for u, v in zip(got, want))


@LAYOUTS
def test_dy_in_the_other_memory_format_gives_the_same_bits(channels_last):
    shape = FRONT_SHAPES[channels_last]
    G = shape[2]
    x, a, w, b, dy = _inputs_hw(shape, torch.float16, channels_last, 11)
    other = _to_layout(dy, not channels_last)
    assert other.stride() != dy.stride() and torch.equal(other, dy)
    fn = lambda xx, aa: group_norm_act(xx, G, w, b, 1e-5, True, aa)
    assert all(torch.equal(u, v) for u, v in zip(_run(fn, x, a, other), _run(fn, x, a, dy)))


def _offset_copy(t, channels_last):
    """A dense copy of t, same strides, that starts one element (2 bytes) into its storage."""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = flat[1:1 + t.numel()]
    view = view.view(t.shape[0], *t.shape[2:], t.shape[1]).permute(0, 3, 1, 2) if channels_last else view.view(t.shape)
    view.copy_(t)
    assert view.stride() == t.stride() and view.data_ptr() % 16 == 2 and torch.equal(view, t)
    return view


def _stock(x, G, w, b, eps, act, a):
    h = x if a is None else x + a[:, :, None, None]
    h = F.group_norm(h, G, w, b, eps)
    return F.silu(h) if act else h


UNSUPPORTED = [
    ("nchw-hw9", False, (2, 16, 4, 3, 3)),      # NCHW rows that are no multiple of 8 elements
    ("nhwc-c12", True, (2, 12, 4, 4, 4)),       # NHWC with C % 8 ≠ 0
    ("nchw-g512", False, (1, 512, 512, 2, 4)),  # more groups than kMaxGroups
    ("nhwc-g512", True, (1, 512, 512, 2, 4)),
    ("hw1", False, (2, 32, 4, 1, 1)),           # H·W = 1 (both layouts at once; counts as NCHW, whose rows need 8 elements)
]


@pytest.mark.parametrize("name,channels_last,shape", UNSUPPORTED, ids=[u[0] for u in UNSUPPORTED])
def test_shapes_the_kernels_do_not_cover_get_the_stock_composite(name, channels_last, shape):
    G = shape[2]
    x, a, w, b, dy = _inputs_hw(shape, torch.float16, channels_last, 12)
    assert _hip_layout(x, G, w, b, a) is None
    got = _run(lambda xx, aa: group_norm_act(xx, G, w, b, 1e-5, True, aa), x, a, dy)
    want = _run(lambda xx, aa: _stock(xx, G, w, b, 1e-5, True, aa), x, a, dy)
    assert len(got) == 3 and all(torch.equal(u, v) for u, v in zip(got, want))


@LAYOUTS
def test_x_that_starts_2_bytes_into_its_storage_gets_the_stock_composite(channels_last):
    shape = FRONT_SHAPES[channels_last]
    G = shape[2]
    x, a, w, b, dy = _inputs_hw(shape, torch.float16, channels_last, 13)
    assert _hip_layout(x, G, w, b, a) == int(channels_last)
    xo = _offset_copy(x, channels_last)
    assert _hip_layout(xo, G, w, b, a) is None

    def run(fn):
        xs, as_ = xo.detach().requires_grad_(True), a.detach().clone().requires_grad_(True)  # xo itself: a clone would realign it
        y = fn(xs, as_)
        return [y.detach()] + list(torch.autograd.grad(y, [xs, as_], dy))

    got = run(lambda xx, aa: group_norm_act(xx, G, w, b, 1e-5, True, aa))
    want = run(lambda xx, aa: _stock(xx, G, w, b, 1e-5, True, aa))
    assert all(torch.equal(u, v) for u, v in zip(got, want))


@LAYOUTS
def test_dy_that_starts_2_bytes_into_its_storage_is_realigned_not_refused(channels_last):
    """The forward has already taken the HIP path, so the backward copies such a dy once: same bits as with the aligned dy."""
    shape = FRONT_SHAPES[channels_last]
    G = shape[2]
    x, a, w, b, dy = _inputs_hw(shape, torch.float16, channels_last, 14)
    fn = lambda xx, aa: group_norm_act(xx, G, w, b, 1e-5, True, aa)
    want = _run(fn, x, a, dy)
    xs, as_ = x.clone(memory_format=torch.preserve_format).requires_grad_(True), a.clone().requires_grad_(True)
    y = fn(xs, as_)
    dx, da = torch.autograd.grad(y, [xs, as_], _offset_copy(dy, channels_last))
    assert torch.equal(y.detach(), want[0]) and torch.equal(dx, want[1]) and torch.equal(da, want[2])


def test_entry_points_refuse_a_misaligned_pointer_before_launching():
    """LORA_E_ALIGN for x, y, dy, dx or the workspace 2 bytes off, with everything else valid: the check comes before any launch."""
    N, C, G, H, W = 1, 16, 2, 2, 4
    x, a, w, b, dy = _inputs_hw((N, C, G, H, W), torch.float16, False, 15)
    y, mean, rstd = nat.group_norm_act_fwd(x, a, w, b, G, 1e-5, True, 0)
    dx, ws = torch.empty_like(x), torch.empty(1024, dtype=torch.uint8, device="cuda")
    lib, p = nat.lib(), lambda t: t.data_ptr()
    fwd = lambda xp, yp, wsp: lib.group_norm_act_fwd(xp, p(a), p(w), p(b), yp, p(mean), p(rstd), wsp, N, C, H * W, G, 1e-5, 1, 0, 1,
                                                     nat._stream(x))
    bwd = lambda dyp, xp, dxp, wsp: lib.group_norm_act_bwd(dyp, xp, p(a), p(w), p(b), p(mean), p(rstd), dxp, None, wsp, N, C,
                                                           H * W, G, 1, 0, 1, nat._stream(x))
    assert fwd(p(x) + 2, p(y), p(ws)) == fwd(p(x), p(y) + 2, p(ws)) == fwd(p(x), p(y), p(ws) + 2) == -3
    assert bwd(p(dy) + 2, p(x), p(dx), p(ws)) == bwd(p(dy), p(x) + 2, p(dx), p(ws)) == -3
    assert bwd(p(dy), p(x), p(dx) + 2, p(ws)) == bwd(p(dy), p(x), p(dx), p(ws) + 2) == -3
    assert fwd(p(x), p(y), p(ws)) == 0 and bwd(p(dy), p(x), p(dx), p(ws)) == 0
    torch.cuda.synchronize()
