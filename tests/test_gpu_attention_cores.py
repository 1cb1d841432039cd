"""Every compiled attention kernel (csrc/attn_flash.hip, csrc/attn_ctx.hip) against float64 math on the same 16-bit
inputs, at the shapes where tiled kernels go wrong: each dispatch-table instantiation (tests/attention_cases.py), every
head width, the query / key counts around the tile and wave boundaries, the chunk partition of cross-attention, large
scores that exercise the online-softmax rescale, and non-default scales.

Every tensor is judged with `assert_close` (whole-tensor L2, every row, every element) at the bounds of the older core
tests: 2e-3 in f16, 1.2e-2 in bf16 — one output rounding of the dtype plus the 16-bit P (or dS) operand.  One exception,
flash dK at 1.5×: attn_flash_dkdv_kernel recomputes P from scores built on K·scale·log2 e rounded to 16 bits, while the
forward's LSE comes from Q·scale·log2 e rounded to 16 bits, so its P carries one more rounding than the forward's own.
Measured on the MI355X over the cases below, flash dK reached 1.14 (f16) and 1.22 (bf16) of the 1× element bar; cross-
attention dK, which scales in fp32, stays at 0.58, and every dQ at ≤ 0.80.  Where that defect grows past even 1.5× — scores
of 30–60, or scale 0.3 with wide heads in bf16 — the measured misses are strict xfails, so the fix shows.
A gradient that is identically zero in float64 (one key: softmax ≡ 1, dS ≡ 0) has no relative error; what a correct
kernel leaves there is the fp32 residue of dP − Δ, two length-d dot products equal in exact arithmetic, summed over the
query rows: ≤ 2.3e-6 measured over 50 rows, bounded at 2⁻¹⁶ (a kernel that loses Δ or the scale leaves O(0.1)).
Inputs carry B ≥ 2 so the rows past Tq / Tk of one batch are the next batch's real data: a kernel that reads past its own
rows picks up numbers, not zeros."""
import pytest
import torch

from diffusion_finetuning_amd.sandwich import (ctx_attention, ctx_attention_supported, flash_attention,
                                               flash_attention_supported)
from tests.attention_cases import INSTANTIATIONS, attention_reference, flash_keys

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
TOL = {torch.float16: 2e-3, torch.bfloat16: 1.2e-2}
FLASH_DK = 1.5  # flash dK only: the K-side prescale rounding of the dK/dV kernel (module docstring)
CORES = {"flash": (flash_attention, flash_attention_supported), "ctx": (ctx_attention, ctx_attention_supported)}
NAMES = ("o", "dq", "dk", "dv")
KEYS = sorted(INSTANTIATIONS, key=str)


def _inputs(shape, dtype, seed):
    B, Tq, Tk, H, d = shape
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, T, H * d, generator=g).to(dtype) for T in (Tq, Tk, Tk, Tq))  # q, k, v, dO


def _run(core, q, k, v, go, H, scale):
    fn, supported = CORES[core]
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    assert supported(qd, kd, H), (core, q.shape, k.shape, H)
    o = fn(qd, kd, vd, H, scale)
    grads = torch.autograd.grad(o, (qd, kd, vd), go.to(DEV))
    return [t.detach().cpu() for t in (o,) + grads]


def _reference(q, k, v, go, H, scale):
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    o = attention_reference(qr, kr, vr, H, scale)
    return [o.detach()] + list(torch.autograd.grad(o, (qr, kr, vr), go.double()))


def _check(close, core, q, k, v, go, H, scale=None, what=(), names=NAMES):
    """Kernel against float64 on the same inputs (the tensors in `names`); returns the kernel's (o, dq, dk, dv)."""
    got = _run(core, q, k, v, go, H, scale)
    for name, a, b in zip(NAMES, got, _reference(q, k, v, go, H, scale)):
        if name not in names:
            continue
        tag = (core, name, tuple(q.shape), tuple(k.shape), H, scale, str(q.dtype)) + tuple(what)
        if float(b.abs().max()) == 0.0:
            assert float(a.double().abs().max()) < 2.0 ** -16, tag  # (see the module docstring)
        else:
            close(a, b, TOL[q.dtype] * (FLASH_DK if (core, name) == ("flash", "dk") else 1.0), tag)
    return got


def _shape_case(close, core, shape, dtype, scale=None, seed=0, what=()):
    q, k, v, go = _inputs(shape, dtype, seed)
    return _check(close, core, q, k, v, go, shape[3], scale, what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", KEYS, ids=lambda k: "-".join(map(str, k)))
def test_every_instantiation_against_float64_and_bit_identical(close, key, dtype):
    """Each compiled kernel once at a shape that reaches it (the two earlier-untested families among them: flash
    forward with ONES at d = 56, 72, 88, 120, 152, and cross-attention with 97–128 keys); a second run must match the
    first bit for bit — outputs and all three gradients (every element has one owner; partials are summed in order)."""
    core = "flash" if key[0].startswith("flash") else "ctx"
    shape = INSTANTIATIONS[key]
    q, k, v, go = _inputs(shape, dtype, seed=KEYS.index(key))
    first = _check(close, core, q, k, v, go, shape[3], what=(key,))
    second = _run(core, q, k, v, go, shape[3], None)
    for name, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), (key, name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("core", ["flash", "ctx"])
def test_every_head_width(close, core, dtype):
    """d = 8 … 160 in steps of 8 — every width the planner accepts, so every amount of zero padding in the head-dim
    fragments — on a ragged two-batch shape (flash: a second, partial 64-key tile)."""
    Tq, Tk = (70, 83) if core == "flash" else (70, 45)
    for d in range(8, 161, 8):
        _shape_case(close, core, (2, Tq, Tk, 2, d), dtype, seed=d, what=("d", d))




FLASH_BUCKET_WIDTHS = [40, 64, 72, 96, 104, 160]  # one width per head-dim bucket of plan_flash (40: the ONES form)


def _flash_geometry(d):
    (_, _, _, rb, _), (_, _, _, rbq, nkw) = flash_keys(d)
    tqs = sorted({1, 64 * rb - 1, 64 * rb + 1, 64 * rbq - 1, 64 * rbq + 1})
    # dK/dV: 64·NKW keys per workgroup, 16·NKW per wave.  16·NKW − 1: one partial wave, three empty; 64·NKW + 1: a second
    # block with one key; 80·NKW + 3: a second block with one full wave, one of three keys and two empty waves
    tks = sorted({1, 16 * nkw - 1, 64 * nkw + 1, 80 * nkw + 3})
    return tqs, tks


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", FLASH_BUCKET_WIDTHS)
def test_flash_tile_edges(close, d, dtype):
    """Query counts one below / above the forward's (64·RB) and dQ's (64·RBQ) query blocks and a single query; key
    counts of one key, one partial dK/dV wave, one key past a dK/dV block, and a last block with empty waves; two
    non-default scales (0.3 and 1/d: the dK/dV kernel takes scale and scale·log2 e as separate arguments)."""
    tqs, tks = _flash_geometry(d)
    for Tq in tqs:
        _shape_case(close, "flash", (2, Tq, 70, 2, d), dtype, seed=Tq, what=("Tq", Tq))
    for Tk in tks:
        _shape_case(close, "flash", (2, 50, Tk, 2, d), dtype, seed=Tk, what=("Tk", Tk))
    _shape_case(close, "flash", (2, 90, 100, 2, d), dtype, scale=1.0 / d, seed=7)
    if dtype == torch.float16 or d <= 64:  # (bf16 at 0.3 with wider heads: test_flash_bf16_scale_0_3)
        _shape_case(close, "flash", (2, 90, 100, 2, d), dtype, scale=0.3, seed=7)


# Measured misses of flash in bf16 at scale 0.3, strict xfails: (d, tensor) -> what was measured
SCALE_0_3_MISSES = {
    (96, "dk"): "max_abs/rms 0.159 against 0.144",
    (96, "dv"): "max_abs/rms 0.108 against 0.096",
    (104, "dv"): "max_abs/rms 0.138 against 0.096",
    (160, "dq"): "worst row 0.056 against 0.048 (the forward / dQ Q-side rounding of the same scores)",
    (160, "dk"): "max_abs/rms 0.209 against 0.144",
    (160, "dv"): "max_abs/rms 0.151 against 0.096",
}


def _scale_0_3_params():
    for d in (w for w in FLASH_BUCKET_WIDTHS if w > 64):
        for name in NAMES:
            why = SCALE_0_3_MISSES.get((d, name))
            marks = [pytest.mark.xfail(reason=why, strict=True)] if why else []
            yield pytest.param(d, name, marks=marks, id=f"{d}-{name}")


@pytest.mark.parametrize("d,name", list(_scale_0_3_params()))
def test_flash_bf16_scale_0_3(close, d, name):
    """Scale 0.3 in bf16 for the buckets above 64: scores of std 0.3·√d ≥ 2.5, ≈ 10–14 at the top in the exp2 domain.
    There the dK/dV kernel's 16-bit rounding of K·scale·log2 e (bf16: 2⁻⁹ relative, per key) against the forward's of
    Q·scale·log2 e moves each recomputed P by 1–3 % — the precision defect of test_large_scores_against_float64 (at d = 160
    the forward / dQ's own Q-side rounding shows in dQ too), measured misses as strict xfails.  Cross-attention scales in fp32 and runs 0.3 in bf16 at every width (test_ctx_key_count_edges)."""
    q, k, v, go = _inputs((2, 90, 100, 2, d), torch.bfloat16, seed=7)
    _check(close, "flash", q, k, v, go, 2, 0.3, what=("scale", 0.3), names=(name,))


CTX_BUCKET_WIDTHS = [40, 64, 72, 96, 160]  # one width per DF of plan_ctx (160: the sliced wide-head backward)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", CTX_BUCKET_WIDTHS)
def test_ctx_key_count_edges(close, d, dtype):
    """1, 96, 97 and 128 keys (the NKF 6 / 8 boundary; wide heads stop at 96) and two non-default scales."""
    for Tk in (1, 96, 97, 128):
        if d > 96 and Tk > 96:
            assert not ctx_attention_supported(torch.empty(1, 1, 2 * d, device=DEV, dtype=dtype),
                                               torch.empty(1, Tk, 2 * d, device=DEV, dtype=dtype), 2)
            continue
        _shape_case(close, "ctx", (2, 100, Tk, 2, d), dtype, seed=Tk, what=("Tk", Tk))
    for scale in (0.3, 1.0 / d):
        _shape_case(close, "ctx", (2, 100, 77, 2, d), dtype, scale=scale, seed=9)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ctx_chunk_partition(close, dtype):
    """plan_ctx splits the query rows of a (batch, head) into `chunks` of `rq` rows to fill the GPU.  B·H ≥ 512 leaves
    one chunk (the ordered partial reduce of dK/dV then sums a single term); the others end in a ragged last chunk —
    1000 rows of one head: 16 chunks of 64, the last of 40; 128 heads: forward 4 chunks of 256, backward 2 of 512."""
    for shape in ((2, 130, 77, 256, 8), (1, 1000, 77, 1, 40), (2, 1000, 100, 64, 8), (1, 333, 50, 3, 160)):
        _shape_case(close, "ctx", shape, dtype, seed=shape[1], what=("chunks",))


def _large_score_inputs(core, placement, seed):
    """f16 inputs whose scores are ≈ 30–60 in magnitude: column 0 of each head carries q = ±320 and a per-key factor
    c_j = O(1), so with scale 1/8 the score is ±40·c_j plus an O(1) random part from the other 63 columns.  (The large
    part sits in Q: a large common offset in K would leave dQ = scale·Σ dS·k to cancel it through a 16-bit dS, which no
    16-bit kernel does — softmax is blind to the offset, the rounding of dS is not.)"""
    B, Tq, H, d = 2, 100, 2, 64
    Tk = 200 if core == "flash" else 90  # flash: tiles of 64 keys, the last one partial (192 … 199)
    g = torch.Generator().manual_seed(seed)
    q, k, v, go = (torch.randn(B, T, H, d, generator=g) for T in (Tq, Tk, Tk, Tq))
    u = torch.rand(B, Tk, H, generator=g)
    last = Tk - Tk % 64 if core == "flash" else Tk - 8  # the keys of the last (partial) tile
    q[..., 0] = 320.0
    if placement == "max_in_last_tile":  # every row's maximum arrives last and rescales all that was accumulated
        c = 0.8 + 0.15 * u
        c[:, last:] = 1.05 + 0.1 * u[:, last:]  # scores 32 … 38 before, 42 … 46 in the last tile
    elif placement == "max_in_first_tile":  # later tiles underflow to exact zeros in the exp2 of the kernels
        c = -1.25 - 0.25 * u
        c[:, :64] = 1.25 + 0.1 * u[:, :64]  # 50 … 54 against −50 … −60
    else:  # mixed signs: a row's q picks the largest or the most negative factors, anywhere in the sequence
        q[..., 0] *= torch.randint(0, 2, (B, Tq, H), generator=g).mul(2).sub(1)
        c = (0.75 + 0.75 * u) * torch.randint(0, 2, (B, Tk, H), generator=g).mul(2).sub(1)
    k[..., 0] = c
    return tuple(t.reshape(B, t.shape[1], H * d).half() for t in (q, k, v, go)), H


PLACEMENTS = ["max_in_last_tile", "max_in_first_tile", "mixed_signs"]
# Measured misses, each a strict xfail so that a fix shows: (core, placement, tensor) -> what was measured
LARGE_SCORE_MISSES = {
    ("flash", "max_in_last_tile", "dk"): "dK/dV prescale defect: rel 7.5e-3 against 3e-3",
    ("flash", "max_in_last_tile", "dv"): "dK/dV prescale defect: rel 9.3e-3 against 2e-3",
    ("flash", "max_in_first_tile", "dk"): "dK/dV prescale defect: rel 1.4e-2 against 3e-3",
    ("flash", "max_in_first_tile", "dv"): "dK/dV prescale defect: rel 1.5e-2 against 2e-3",
    ("flash", "mixed_signs", "dk"): "dK/dV prescale defect: rel 2.0e-2 against 3e-3",
    ("flash", "mixed_signs", "dv"): "dK/dV prescale defect: rel 2.2e-2 against 2e-3",
    # cross-attention (fp32 scale) meets the L2 and row bars (rel 3.2e-4); with a near one-hot softmax dK is heavy-tailed
    # and one element misses the element bar: 0.026 of rms against 0.016
    ("ctx", "mixed_signs", "dk"): "element bar of a one-hot dK: 0.026 of rms against 0.016",
}


def _large_score_params():
    for core in ("flash", "ctx"):
        for placement in PLACEMENTS:
            for name in NAMES:
                why = LARGE_SCORE_MISSES.get((core, placement, name))
                marks = [pytest.mark.xfail(reason=why, strict=True)] if why else []
                yield pytest.param(core, placement, name, marks=marks, id=f"{core}-{placement}-{name}")


@pytest.mark.parametrize("core,placement,name", list(_large_score_params()))
def test_large_scores_against_float64(close, core, placement, name):
    """Online softmax under f16 scores of 30–60 with random V: the running maximum found in the last, partial key tile;
    found in the first with every later probability an exact zero; and mixed signs.  Every tensor at the bounds of every
    other case.  The flash dK/dV kernel rounds K·scale·log2 e to 16 bits for its scores, while the forward's LSE (and the dQ
    kernel's scores) come from Q·scale·log2 e rounded to 16 bits: at scores of ≈ 40 (≈ 58 in the exp2 domain) the two
    roundings differ by ~1 % in each recomputed P.  That is a precision defect of attn_flash_dkdv_kernel, left in place
    here: its measured misses are strict xfails (LARGE_SCORE_MISSES), so the fix turns them into failures to remove."""
    (q, k, v, go), H = _large_score_inputs(core, placement, seed=len(placement))
    s = (q.double()[..., :64] @ k.double()[..., :64].transpose(1, 2)) / 8.0
    assert 30.0 <= float(s.abs().max()) <= 70.0  # (the inputs are what the docstring says)
    _check(close, core, q, k, v, go, H, what=(placement,), names=(name,))
