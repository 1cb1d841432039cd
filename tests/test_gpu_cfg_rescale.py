"""ddpm_cfg_rescale (csrc/cfg_rescale.hip) through the C-ABI on an MI355X: k against float64 on the storage-rounded inputs
(tests/zero_snr_reference.py), the scaled halves bit for bit against one fp32 multiplication by the kernel's own k, at the
layout edges — below one pack, around one workgroup's 1024 threads and its 4 register-held packs (4096 / 16384 elements), the
re-read path above them, both access widths — and the degenerate rows.

Tolerance on k: 1e-5 relative.  The kernel sums in fp32: a thread adds its elements in ascending order (n/1024 of them, 64 at
n = 65536), a 6-level butterfly joins a wave's lanes and a 4-level tree the 16 wave sums — a 10-level tree behind a serial chain
of at most 64 terms, worst case (n/1024 + 10)·2⁻²⁴ ≈ 4.4e-6 per sum; the bound is about twice that.  The element-by-element path
has the same shape (a thread's elements are then 1024 apart instead of 4-packs 4096 apart)."""
import itertools

import pytest
import torch

from diffusion_finetuning_amd import _native as nat
from tests import zero_snr_reference as zr

pytestmark = pytest.mark.gpu
DEV = "cuda"
K_TOL = 1e-5
PER_ROW = [1, 2, 3, 4, 255, 256, 1023, 1024, 1025, 4100, 16384, 65536]
DTYPES = [torch.float16, torch.bfloat16, torch.float32]


def _call(buf, B, per_row, g, phi, k_out=None, dtype=None):
    return nat.lib().ddpm_cfg_rescale(nat._ptr(buf), nat._ptr(k_out), B, per_row, float(g), float(phi),
                                      nat.dtype_code(buf.dtype if dtype is None else dtype), nat._stream(buf))


def _shifted(t):
    """The same values one element into a larger allocation: off every 4-element boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view


def _random_out(B, per_row, seed=0, mean=0.0):
    """[2B, per_row] fp32 on the host: both halves random, their difference varying within a row (noise plus a ramp)."""
    gen = torch.Generator().manual_seed(seed + 7 * B + per_row)
    u = mean + torch.randn(B, per_row, generator=gen)
    c = mean + 0.6 * (u - mean) + 0.8 * torch.randn(B, per_row, generator=gen) + torch.linspace(-0.5, 0.5, per_row)
    return torch.cat([u, c])


@pytest.fixture(scope="module")
def cases():
    """Inputs and float64 references, computed once: {(B, per_row, dtype, g, phi): (out fp32 host, k float64 [B])}."""
    made = {}
    for B, per_row, dtype in itertools.product((1, 3), PER_ROW, DTYPES):
        out = _random_out(B, per_row)
        for g, phi in itertools.product((1.5, 7.5), (0.7, 1.0)):
            k = zr.rescale_cfg(out, g, phi, dtype)[0] if per_row > 1 else torch.ones(B, dtype=torch.float64)
            made[(B, per_row, dtype, g, phi)] = (out, k)
    return made


def _check(out, k_ref, B, per_row, dtype, g, phi, shifted, what):
    stored = out.to(dtype).to(DEV)
    buf = _shifted(stored) if shifted else stored.clone()
    k_out = torch.full((B,), -3.0, device=DEV)
    assert _call(buf, B, per_row, g, phi, k_out) == 0
    k = k_out.cpu().double()
    # (relative to k; a row whose two stored conditional values coincide has σ_c = 0 and, at φ = 1, k = 0 exactly)
    err = float(((k - k_ref).abs() / k_ref.abs().clamp(min=1e-30)).max())
    print(f"\n[cfg rescale {what} {dtype} B {B} per_row {per_row} g {g} phi {phi} shifted {shifted}] k {k.tolist()} rel err {err:.3g}")
    assert bool(torch.isfinite(k).all()) and bool(((k - k_ref).abs() <= K_TOL * k_ref.abs()).all())
    # one fp32 multiplication by the kernel's own k, rounded to nearest even: bit for bit
    want = (stored.float() * k_out.repeat(2).view(2 * B, 1)).to(dtype)
    assert torch.equal(buf, want)
    return k_out.cpu(), buf.clone()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("per_row", PER_ROW)
def test_k_against_float64_and_the_halves_bit_for_bit(cases, per_row, dtype):
    for B, g, phi, shifted in itertools.product((1, 3), (1.5, 7.5), (0.7, 1.0), (False, True)):
        out, k_ref = cases[(B, per_row, dtype, g, phi)]
        k, _ = _check(out, k_ref, B, per_row, dtype, g, phi, shifted, "random")
        if per_row == 1:
            assert bool((k == 1.0).all())
        elif per_row >= 255:
            assert bool(((k - 1.0).abs() > 1e-3).all())  # the case checks something: guidance changed the row's deviation


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("per_row", [1023, 16384, 65536])
def test_rows_with_a_mean_far_above_their_deviation(per_row, dtype):
    """Row mean 100, standard deviation 1: E[x²] − E[x]² in fp32 keeps 3 digits of the variance here; the centred sums keep all."""
    for B, g, phi in ((3, 7.5, 0.7), (1, 1.5, 1.0)):
        out = _random_out(B, per_row, seed=5, mean=100.0)
        k_ref = zr.rescale_cfg(out, g, phi, dtype)[0]
        for shifted in (False, True):
            _check(out, k_ref, B, per_row, dtype, g, phi, shifted, "mean 100")


@pytest.mark.parametrize("per_row", [256, 1025, 16384, 65536])
def test_full_rescale_gives_the_guided_output_the_conditional_deviation(per_row):
    B, g = 3, 7.5
    out = _random_out(B, per_row, seed=2)
    buf = out.to(DEV)
    assert _call(buf, B, per_row, g, 1.0) == 0
    u, c = buf.cpu().double().chunk(2)
    got = (u + g * (c - u)).std(dim=1, unbiased=False)
    want = out[B:].double().std(dim=1, unbiased=False)
    assert float(((got - want).abs() / want).max()) <= 1e-5
    plain = (out[:B].double() + g * (out[B:].double() - out[:B].double())).std(dim=1, unbiased=False)
    assert float(((plain - want).abs() / want).min()) > 0.5  # (without the rescale guidance had inflated it)


@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_rows_keep_their_bits(dtype):
    g = 1.5
    rows = []
    for per_row in (37, 1024, 4100):
        flat = torch.full((2, per_row), 0.3)  # c == u == a constant no sum of which is exact
        alt = torch.arange(per_row) % 2 == 0
        c = torch.where(alt, torch.tensor(1.0), torch.tensor(3.0)).view(1, -1)
        u = torch.where(alt, torch.tensor(-1.0), torch.tensor(5.0)).view(1, -1)  # u + 1.5·(c − u) == 2 everywhere
        rows += [(per_row, flat), (per_row, torch.cat([u, c]))]
    rows.append((1, torch.tensor([[0.25], [-1.5]])))
    for (per_row, out), phi, shifted in itertools.product(rows, (0.7, 1.0), (False, True)):
        stored = out.to(dtype).to(DEV)
        buf = _shifted(stored) if shifted else stored.clone()
        k_out = torch.full((1,), -3.0, device=DEV)
        assert _call(buf, 1, per_row, g, phi, k_out) == 0
        assert float(k_out) == 1.0, (per_row, phi, shifted)
        assert torch.equal(buf.view(torch.int16 if dtype != torch.float32 else torch.int32),
                           stored.view(torch.int16 if dtype != torch.float32 else torch.int32))
        assert bool(torch.isfinite(buf.float()).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_rescale_is_exactly_one(dtype):
    for B, per_row in ((3, 1024), (2, 37)):
        stored = _random_out(B, per_row).to(dtype).to(DEV)
        buf, k_out = stored.clone(), torch.zeros(B, device=DEV)
        assert _call(buf, B, per_row, 7.5, 0.0, k_out) == 0
        assert bool((k_out == 1.0).all()) and torch.equal(buf, stored)


def test_run_to_run_rows_alone_and_without_k_out():
    g, phi = 7.5, 0.7
    for per_row, dtype in ((1024, torch.float16), (4100, torch.float32), (65536, torch.bfloat16)):
        B = 3
        stored = _random_out(B, per_row, seed=9).to(dtype).to(DEV)
        runs = []
        for _ in range(2):
            buf, k_out = stored.clone(), torch.zeros(B, device=DEV)
            assert _call(buf, B, per_row, g, phi, k_out) == 0
            runs.append((buf, k_out))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        for b in range(B):  # a row's result depends neither on B nor on the other rows
            alone, k_alone = torch.stack([stored[b], stored[B + b]]), torch.zeros(1, device=DEV)
            assert _call(alone, 1, per_row, g, phi, k_alone) == 0
            assert torch.equal(k_alone, runs[0][1][b:b + 1])
            assert torch.equal(alone[0], runs[0][0][b]) and torch.equal(alone[1], runs[0][0][B + b])
        silent = stored.clone()
        assert _call(silent, B, per_row, g, phi, None) == 0
        assert torch.equal(silent, runs[0][0])


def test_bad_arguments_are_refused_and_the_library_still_answers():
    buf = torch.zeros(4, 64, device=DEV, dtype=torch.float16)
    lib = nat.lib()
    good = [nat._ptr(buf), None, 2, 64, 7.5, 0.7, nat.dtype_code(torch.float16), nat._stream(buf)]
    for i, v in ((0, None), (2, 0), (2, -2), (3, 0), (3, -1), (6, 3), (6, -1), (5, -0.01), (5, 1.01), (5, float("nan")),
                 (4, float("inf")), (4, float("-inf")), (4, float("nan"))):
        bad = list(good)
        bad[i] = v
        assert lib.ddpm_cfg_rescale(*bad) == -1, (i, v)
    assert not buf.any() and lib.lora_version() == nat.ABI_VERSION
    assert lib.ddpm_cfg_rescale(*good) == 0


def test_the_wrapper_checks_what_the_step_wrapper_checks():
    import diffusion_finetuning_amd as dfa

    ts, coef = dfa.sampler_schedule("ddim", 4, True)
    st = nat.SampleState.alloc((2, 4, 8, 8), torch.float16, True, ts, coef, DEV)
    out = torch.randn(4, 4, 8, 8, device=DEV).half()
    with pytest.raises(ValueError, match="contiguous"):
        nat.ddpm_cfg_rescale(st, out.float(), 5.0, 0.7)
    with pytest.raises(ValueError, match="contiguous"):
        nat.ddpm_cfg_rescale(st, out[:, :, :, ::2], 5.0, 0.7)
    with pytest.raises(RuntimeError, match="HIP device"):
        nat.ddpm_cfg_rescale(st, out.cpu(), 5.0, 0.7)
    with pytest.raises(ValueError, match="k_out"):
        nat.ddpm_cfg_rescale(st, out, 5.0, 0.7, k_out=torch.zeros(3, device=DEV))
    single = nat.SampleState.alloc((2, 4, 8, 8), torch.float16, False, ts, coef, DEV)
    with pytest.raises(ValueError, match="no guidance rows"):
        nat.ddpm_cfg_rescale(single, out[:2].contiguous(), 5.0, 0.7)
    k, before = torch.zeros(2, device=DEV), out.clone()
    nat.ddpm_cfg_rescale(st, out, 5.0, 0.7, k_out=k)
    assert torch.equal(out, (before.float() * k.repeat(2).view(4, 1, 1, 1)).half()) and bool((k != 1.0).all())


def test_the_launch_is_capturable():
    B, per_row, g, phi = 3, 4100, 7.5, 0.7
    inputs = [_random_out(B, per_row, seed=s).half().to(DEV) for s in (1, 2)]
    eager = []
    for x in inputs:
        buf, k = x.clone(), torch.zeros(B, device=DEV)
        assert _call(buf, B, per_row, g, phi, k) == 0
        eager.append((buf, k))
    static, k_static = inputs[0].clone(), torch.zeros(B, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert _call(static, B, per_row, g, phi, k_static) == 0
    for x, (want, k_want) in zip(inputs, eager):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, want) and torch.equal(k_static, k_want)
