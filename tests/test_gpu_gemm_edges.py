"""The fused LoRA GEMM (csrc/lora_gemm.hip) at its tile, ring, K-step and dispatch edges (MI355X).

Every class of tests/gemm_cases.py — each `launch_tile` instantiation a single-layer launch can reach, the fallback loop,
the shape-agnostic kernels and both split-K tiles — runs in every dtype it exists for, through the C ABI, against the
float64 oracle.  A shape (M, Kc, Nc) runs in both roles of the template:
  forward         layer K = Kc, N = Nc:   Y  = X·Wᵀ + b + s·(X·Aᵀ)·Bᵀ,  T = X·Aᵀ
  backward-input  layer N = Kc, K = Nc:   dX = dY·W + s·(dY·B)·A,       U = dY·B       (same Am and Bm: W = Bmᵀ)
and the skinny launch (U alone, `need_dx=False`) runs on both layers, checked against float64 itself.  The forward
layer's factor gradients come from lora_linear_bwd_params on the same operands (ragged K and N through lora_grad.hip).

Outputs are views into larger buffers whose bands (at least one 128-row tile on either side) hold a sentinel bit
pattern and must still hold it afterwards; the views start as NaN and must end without one.  Each launch runs under the
library's launch profiler, and the kernel kind it records must be the one the dispatch mirror predicts: the split-K kind
for split cases and no others, the 128-row and the 64-row kinds apart, no GEMM kind at all for the generic kernels.

Bounds are tests/test_gpu_parity.py's TOL (2e-5 / 1e-3 / 1e-2 relative L2 with the row and element bars of `assert_close`)
for Y, dX and the factor gradients; T and U, fp32 outputs, are held to 1e-3 on 16-bit inputs as
test_split_k_inside_the_gemm_launch holds them.  tests/test_gemm_coverage_host.py shows on the CPU that these bounds
reject an off-by-one row clamp, a missing rank-r term or bias at the last column tile, and a dropped partial K-step."""
import pytest
import torch

from diffusion_finetuning_amd import _native as nat
from oracle import lora_oracle as orc
from tests.gemm_cases import (CASES, DTYPES, ESIZE, GENERIC, SKINNY_CASES, SPLIT, class_of, make_factors, make_layer,
                              skinny_class_of, skinny_launch_class)
from tests.test_gpu_parity import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAME = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
BAND_ROWS = 128  # one full row tile of the tallest kernel on either side of every output

# names of the profiler kinds (csrc/prof.hip) the classes land on
KIND_128 = "lora_gemm_kernel<*, 128, 128|160, true>"
KIND_64 = "lora_gemm_kernel<*, 64, 64|128|160, true>"
KIND_SKINNY = "lora_gemm_kernel<*, 64, 64, false>"
KIND_SPLIT = "lora_gemm_kernel<*, 64|128, 128, true> split-K (in-launch combine)"

# (rank, bias, scale) per variant of a class: every class sees r = 16 and a rank below 4; a class with one shape runs it twice
CONFIGS = [(16, True, 0.7), (3, False, 0.7), (8, True, 0.0), (1, False, 0.7)]


def p_tol(dtype):
    return 1e-3 if dtype != torch.float32 else TOL[dtype]


def expected_kinds(key):
    if key[0] == GENERIC:
        return {}
    if key[0] == SPLIT:
        return {KIND_SPLIT: 1}
    return {KIND_128 if key[1] == 128 else KIND_64: 1}


def expected_skinny_kinds(key):
    return {} if key[0] == GENERIC else {KIND_SKINNY: 1}


def recorded(launch):
    """Kernel kinds the launch profiler records while `launch` runs: {kind name: launches}."""
    torch.cuda.synchronize()
    nat.prof_enable(8)
    try:
        launch()
        return {k: v["launches"] for k, v in nat.prof_collect().items()}
    finally:
        nat.prof_enable(0)


class Banded:
    """A [rows, cols] output inside a larger buffer: NaN where the kernel must write, a sentinel bit pattern in the bands."""

    def __init__(self, rows, cols, dtype):
        self.ints, self.sentinel = (torch.int32, 0x5A5A5A5A) if dtype == torch.float32 else (torch.int16, 0x5A5A)
        self.n = rows * cols
        self.pad = (BAND_ROWS * cols + 63) // 64 * 64  # (whole 16-byte chunks: the view starts 16-byte aligned)
        self.buf = torch.empty(2 * self.pad + (self.n + 63) // 64 * 64, dtype=dtype, device=DEV)
        self.buf.view(self.ints).fill_(self.sentinel)
        self.view = self.buf[self.pad:self.pad + self.n].view(rows, cols)
        self.view.fill_(float("nan"))
        assert self.view.data_ptr() % 16 == 0

    def check(self, what):
        raw = self.buf.view(self.ints)
        for name, band in (("before", raw[:self.pad]), ("after", raw[self.pad + self.n:])):
            assert torch.equal(band, torch.full_like(band, self.sentinel)), (what, "store into the band", name)
        assert not bool(torch.isnan(self.view).any()), (what, "element never written")
        return self.view


def off_by_one_element(t):
    """The same values at an address one element past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0
    return view


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def launch_fwd(x, w, b, down, up, packs, y, t, scale, ws=None):
    M, K = x.shape
    st = nat.lib().lora_linear_fwd_ws(_ptr(x), _ptr(w), _ptr(b), _ptr(down), _ptr(up), _ptr(packs[0]), _ptr(packs[1]), _ptr(y),
                                      _ptr(t), M, K, w.shape[0], down.shape[0], float(scale), nat.dtype_code(x.dtype),
                                      _ptr(ws), 0 if ws is None else ws.numel() * 4, nat._stream(x))
    assert st == 0, st


def launch_bwd(dy, wt, down, up, packs, dx, u, scale, ws=None):
    """dx None: the skinny launch (U alone)."""
    M, N = dy.shape
    r, K = down.shape
    st = nat.lib().lora_linear_bwd_input_ws(_ptr(dy), _ptr(wt), _ptr(down), _ptr(up), _ptr(packs[0]), _ptr(packs[1]),
                                            _ptr(dx), _ptr(u), M, K, N, r, float(scale), nat.dtype_code(dy.dtype), _ptr(ws),
                                            0 if ws is None else ws.numel() * 4, nat._stream(dy))
    assert st == 0, st


def workspace_for(M, Kc, Nc, dtype, key):
    """The split-K workspace the library asks for (zeroed, as its header must be): one exactly for the split classes."""
    nbytes = int(nat.lib().lora_gemm_workspace_bytes(M, Kc, Nc, nat.dtype_code(dtype)))
    assert (nbytes > 0) == (key[0] == SPLIT), (key, nbytes)
    return torch.zeros(nbytes // 4, dtype=torch.float32, device=DEV) if nbytes > 0 else None


def _params():
    out = []
    for esize, table in CASES.items():
        for key, shapes in table.items():
            runs = [(s, CONFIGS[i % len(CONFIGS)]) for i, s in enumerate(shapes)]
            if len(shapes) == 1:
                runs.append((shapes[0], CONFIGS[1]))
            assert any(c[0] == 16 for _, c in runs) and any(c[0] < 4 for _, c in runs)
            for dtype in DTYPES[esize]:
                for shape, cfg in runs:
                    tag = "%s-%s%dx%ds%d-%s%s-r%d" % (NAME[dtype], key[0], key[1], key[2], key[3], "x".join(map(str, shape[:3])),
                                                      "-offset" if len(shape) > 3 else "", cfg[0])
                    out.append(pytest.param(key, shape, dtype, cfg, id=tag))
    return out


@pytest.mark.parametrize("key,shape,dtype,cfg", _params())
def test_every_class_in_both_roles_inside_guard_bands(close, relerr, key, shape, dtype, cfg):
    (M, Kc, Nc), aligned = shape[:3], len(shape) < 4
    r, bias, scale = cfg
    tol, ptol, what = TOL[dtype], p_tol(dtype), (NAME[dtype], key, shape, cfg)
    assert class_of(shape, ESIZE[dtype]) == key
    # ---- forward role: layer K = Kc, N = Nc --------------------------------------------------------------------------------
    x, w, b, down, up, dy = make_layer(M, Kc, Nc, r, dtype, seed=M + Kc + Nc + r, bias=bias)
    y_ref = orc.lora_linear_forward(x.double(), w.double(), None if b is None else b.double(), down.double(), up.double(), scale)
    _, ga_ref, gb_ref = orc.lora_linear_backward(x.double(), w.double(), down.double(), up.double(), scale, dy.double())
    t_ref, u_ref = x.double() @ down.double().t(), dy.double() @ up.double()
    xa, wd, dyd, downd, upd = x.to(DEV), w.to(DEV), dy.to(DEV), down.to(DEV), up.to(DEV)
    xd = xa if aligned else off_by_one_element(xa)
    bd = None if b is None else b.to(DEV)
    packs = nat.lora_pack_factors(downd, upd, dtype)
    ws = workspace_for(M, Kc, Nc, dtype, key)
    Y, T = Banded(M, Nc, dtype), Banded(M, r, torch.float32)
    kinds = recorded(lambda: launch_fwd(xd, wd, bd, downd, upd, packs, Y.view, T.view, scale, ws))
    assert kinds == expected_kinds(key), (what, "forward", kinds)
    y, t = Y.check((what, "y")), T.check((what, "t"))
    print("rel L2 %s: y %.2e (bound %.0e)  t %.2e (bound %.0e)" % (what, relerr(y, y_ref), tol, relerr(t, t_ref), ptol))
    close(y, y_ref, tol, (what, "y"))
    close(t, t_ref, ptol, (what, "t"))
    if scale == 0.0:  # the rank-r term is off EXACTLY: bit for bit the launch whose up factor is zero
        Y0, T0 = Banded(M, Nc, dtype), Banded(M, r, torch.float32)
        zero = torch.zeros_like(upd)
        launch_fwd(xd, wd, bd, downd, zero, nat.lora_pack_factors(downd, zero, dtype), Y0.view, T0.view, 0.7, ws)
        assert torch.equal(Y0.check((what, "y, up = 0")), y) and torch.equal(T0.view, t), (what, "scale 0 is not the base product")
    # the skinny launch alone on this layer's dY (contraction Nc), against float64 — and the factor gradients from its U
    sk = skinny_launch_class(M, Nc, ESIZE[dtype])
    U = Banded(M, r, torch.float32)
    kinds = recorded(lambda: launch_bwd(dyd, None, downd, upd, packs, None, U.view, scale))
    assert kinds == expected_skinny_kinds(sk), (what, "skinny over Nc", sk, kinds)
    u = U.check((what, "u skinny"))
    close(u, u_ref, ptol, (what, "u skinny over Nc"))
    ga, gb = torch.zeros(r, Kc, device=DEV), torch.zeros(Nc, r, device=DEV)
    nat.lora_linear_bwd_params(dyd, xa, t.contiguous(), u.contiguous(), ga, gb, scale)
    close(ga, ga_ref, tol, (what, "grad A"))
    close(gb, gb_ref, tol, (what, "grad B"))
    if ws is not None:
        assert int(ws.view(torch.int32)[:1024].abs().max().item()) == 0, (what, "ticket header not left at zero")
        # the same call without a workspace runs unsplit and agrees to rounding; a repeated split launch is bit-identical
        Yu, Tu = Banded(M, Nc, dtype), Banded(M, r, torch.float32)
        kinds = recorded(lambda: launch_fwd(xd, wd, bd, downd, upd, packs, Yu.view, Tu.view, scale, None))
        assert kinds == expected_kinds(class_of(shape, ESIZE[dtype], workspace=False)), (what, "unsplit", kinds)
        close(y, Yu.check((what, "y unsplit")), tol, (what, "split vs unsplit y"))
        close(t, Tu.check((what, "t unsplit")), 1e-5, (what, "split vs unsplit t"))
        Y2, T2 = Banded(M, Nc, dtype), Banded(M, r, torch.float32)
        launch_fwd(xd, wd, bd, downd, upd, packs, Y2.view, T2.view, scale, ws)
        assert torch.equal(Y2.check((what, "y again")), y) and torch.equal(T2.check((what, "t again")), t), (what, "not repeatable")
        assert int(ws.view(torch.int32)[:1024].abs().max().item()) == 0, (what, "ticket header not left at zero")
    del Y, T, y_ref, ga_ref, gb_ref
    # ---- backward-input role: layer N = Kc, K = Nc, on the same Am (now dY) and Bm (now Wᵀ) -------------------------------
    down2, up2 = make_factors(Nc, Kc, r, dtype, seed=M + Kc + Nc + r + 1)  # A [r, K = Nc], B [N = Kc, r]
    # dX = dY·W + s·(dY·B)·A is the forward formula on (dY, Wᵀ, Bᵀ, Aᵀ): the template's identity (csrc/lora_gemm_kernel.h, top)
    dx_ref = orc.lora_linear_forward(x.double(), w.double(), None, up2.double().t(), down2.double().t(), scale)
    u2_ref = x.double() @ up2.double()
    down2d, up2d = down2.to(DEV), up2.to(DEV)
    packs2 = nat.lora_pack_factors(down2d, up2d, dtype)
    wt = nat.lora_cast_matrix(wd.t().contiguous(), dtype, True)  # W is [N, K] = Bmᵀ; the kernel wants Wᵀ = Bm
    assert torch.equal(wt, wd)
    DX, U2 = Banded(M, Nc, dtype), Banded(M, r, torch.float32)
    kinds = recorded(lambda: launch_bwd(xd, wt, down2d, up2d, packs2, DX.view, U2.view, scale, ws))
    assert kinds == expected_kinds(key), (what, "backward-input", kinds)
    dx, u2 = DX.check((what, "dx")), U2.check((what, "u"))
    print("rel L2 %s: dx %.2e (bound %.0e)  u %.2e (bound %.0e)" % (what, relerr(dx, dx_ref), tol, relerr(u2, u2_ref), ptol))
    close(dx, dx_ref, tol, (what, "dx"))
    close(u2, u2_ref, ptol, (what, "u"))
    if scale == 0.0:
        DX0, U0 = Banded(M, Nc, dtype), Banded(M, r, torch.float32)
        zero = torch.zeros_like(down2d)
        launch_bwd(xd, wt, zero, up2d, nat.lora_pack_factors(zero, up2d, dtype), DX0.view, U0.view, 0.7, ws)
        assert torch.equal(DX0.check((what, "dx, down = 0")), dx) and torch.equal(U0.view, u2), (what, "scale 0 is not the base product")
    if ws is not None:
        assert int(ws.view(torch.int32)[:1024].abs().max().item()) == 0, (what, "ticket header not left at zero")
        DXu, Uu = Banded(M, Nc, dtype), Banded(M, r, torch.float32)
        launch_bwd(xd, wt, down2d, up2d, packs2, DXu.view, Uu.view, scale, None)
        close(dx, DXu.check((what, "dx unsplit")), tol, (what, "split vs unsplit dx"))
        close(u2, Uu.check((what, "u unsplit")), 1e-5, (what, "split vs unsplit u"))
        DX2, U3 = Banded(M, Nc, dtype), Banded(M, r, torch.float32)
        launch_bwd(xd, wt, down2d, up2d, packs2, DX2.view, U3.view, scale, ws)
        assert torch.equal(DX2.check((what, "dx again")), dx) and torch.equal(U3.check((what, "u again")), u2), (what, "not repeatable")
    # the skinny launch alone on this layer (contraction Kc, the misaligned operand included)
    sk = skinny_launch_class(M, Kc, ESIZE[dtype], aligned)
    Us = Banded(M, r, torch.float32)
    kinds = recorded(lambda: launch_bwd(xd, None, down2d, up2d, packs2, None, Us.view, scale))
    assert kinds == expected_skinny_kinds(sk), (what, "skinny over Kc", sk, kinds)
    close(Us.check((what, "u skinny")), u2_ref, ptol, (what, "u skinny over Kc"))


def _skinny_params():
    out = []
    for esize, table in SKINNY_CASES.items():
        for key, shapes in table.items():
            for dtype in DTYPES[esize]:
                for i, shape in enumerate(shapes):
                    tag = "%s-%s-%s%s" % (NAME[dtype], key[0], "x".join(map(str, shape[:2])), "-offset" if len(shape) > 2 else "")
                    out.append(pytest.param(key, shape, dtype, (16, 3, 1)[i % 3], id=tag))
    return out


@pytest.mark.parametrize("key,shape,dtype,r", _skinny_params())
def test_skinny_launch_alone_against_float64(close, key, shape, dtype, r):
    """lora_linear_bwd_input(..., need_dx=False): U = dY·B from the !MAIN kernel, its fallback loop or the generic kernel,
    with one, two and four K-steps behind the three-stage ring — against float64, not against the main launch's U."""
    (M, N), aligned, K = shape[:2], len(shape) < 3, 24
    assert skinny_class_of(shape, ESIZE[dtype]) == key
    g = torch.Generator().manual_seed(M + N + r)
    dy = torch.randn(M, N, generator=g).to(dtype)
    down, up = make_factors(K, N, r, dtype, seed=M + N)
    u_ref = dy.double() @ up.double()
    dyd, downd, upd = dy.to(DEV), down.to(DEV), up.to(DEV)
    if not aligned:
        dyd = off_by_one_element(dyd)
    packs = nat.lora_pack_factors(downd, upd, dtype)
    U = Banded(M, r, torch.float32)
    kinds = recorded(lambda: launch_bwd(dyd, None, downd, upd, packs, None, U.view, 0.7))
    assert kinds == expected_skinny_kinds(key), (key, shape, kinds)
    close(U.check((key, shape, "u")), u_ref, p_tol(dtype), (NAME[dtype], key, shape, r))
    # the wrapper's own route gives the same bits
    dx, u = nat.lora_linear_bwd_input(dyd, None, downd, upd, 0.7, False, packs)
    assert dx is None and torch.equal(u, U.view)


ALL_DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CAST_SIZES = (1, 31, 32, 33, 65)  # around the kernel's 32×32 tile


@pytest.mark.parametrize("dst", ALL_DTYPES, ids=lambda d: "to_" + NAME[d])
@pytest.mark.parametrize("src", ALL_DTYPES, ids=lambda d: NAME[d])
def test_cast_matrix_at_ragged_edges(src, dst):
    """lora_cast_matrix makes every Wᵀ above: bit for bit `src.to(dst)` (transposed or not) inside a guard-banded destination."""
    g = torch.Generator().manual_seed(3)
    for rows in CAST_SIZES:
        for cols in CAST_SIZES:
            m = (torch.randn(rows, cols, generator=g) * 3).to(src).to(DEV)
            for transpose in (False, True):
                want = m.to(dst).t().contiguous() if transpose else m.to(dst)
                D = Banded(want.shape[0], want.shape[1], dst)
                st = nat.lib().lora_cast_matrix(m.data_ptr(), D.view.data_ptr(), rows, cols, nat.dtype_code(src),
                                                nat.dtype_code(dst), int(transpose), nat._stream(m))
                assert st == 0
                got = D.check((NAME[src], NAME[dst], rows, cols, transpose))
                ints = torch.int32 if dst == torch.float32 else torch.int16
                assert torch.equal(got.contiguous().view(ints), want.view(ints)), (NAME[src], NAME[dst], rows, cols, transpose)
