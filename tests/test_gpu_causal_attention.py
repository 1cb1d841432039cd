"""The causal attention kernels (csrc/attn_causal.hip) through the binding, against float64 math on the same 16-bit inputs:
every compiled instantiation (tests/causal_attention_cases.py), the token counts around the 16-row block, the NKF 6 / 8
bucket and the limits, dense operands and the column slices of one grouped [B·T, 3·H·d] buffer, causality itself (bit for
bit), batch·head counts at which a wave runs two query blocks, run-to-run reproducibility and the refusals.

Every tensor is judged with `close` (whole-tensor L2, every row, every element) at the bounds tests/test_gpu_attention_cores.py
applies to the attn_ctx kernels these were derived from — 2e-3 in f16, 1.2e-2 in bf16: one output rounding of the dtype plus the
16-bit P (or dS) operand.  A gradient that is identically zero in float64 (T = 1: softmax ≡ 1, dS ≡ 0) is bounded at 2⁻¹⁶ like
there.  B = 2, so the rows past T of batch 0 are batch 1's real data."""
import functools

import pytest
import torch

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd.sandwich import causal_attention, causal_attention_supported
from tests.causal_attention_cases import INSTANTIATIONS, causal_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
TOL = {torch.float16: 2e-3, torch.bfloat16: 1.2e-2}  # tests/test_gpu_attention_cores.py: TOL, as applied to "ctx"
NAMES = ("o", "dq", "dk", "dv")
KEYS = sorted(INSTANTIATIONS)
SENTINEL = 1234.0


@functools.lru_cache(maxsize=None)
def _case(shape, dtype, seed):
    """(q, k, v, dO) rounded to `dtype`, and the float64 (o, dq, dk, dv) on them — computed once per case, never modified."""
    B, T, H, d = shape
    g = torch.Generator().manual_seed(seed)
    q, k, v, go = (torch.randn(B, T, H * d, generator=g).to(dtype) for _ in range(4))
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    o = causal_reference(qr, kr, vr, H)
    ref = (o.detach(),) + tuple(torch.autograd.grad(o, (qr, kr, vr), go.double()))
    return (q, k, v, go), ref


def _run(q, k, v, go, H, scale, strided):
    """(o, dq, dk, dv) on the CPU.  strided: q | k | v are the column slices of one [B·T, 3·H·d] buffer and the gradients go
    into the slices of another, framed by sentinel columns and rows that must stay untouched."""
    B, T, HD = q.shape
    if not strided:
        qd, kd, vd = (t.to(DEV) for t in (q, k, v))
        o = nat.attn_causal_fwd(qd, kd, vd, H, scale)
        grads = nat.attn_causal_bwd(qd, kd, vd, go.to(DEV), H, scale)
        return [t.cpu() for t in (o,) + tuple(grads)]
    buf = torch.cat([q, k, v], dim=-1).to(DEV)  # [B, T, 3·HD]: what a grouped q/k/v projection writes
    qd, kd, vd = (buf[..., i * HD:(i + 1) * HD] for i in range(3))
    assert not qd.is_contiguous() and nat.shared_row_stride(qd, kd, vd) == 3 * HD
    o = nat.attn_causal_fwd(qd, kd, vd, H, scale)
    W = 3 * HD + 16  # 8 sentinel columns on either side of the three slices, one sentinel row after the last
    gbuf = torch.full((B * T + 1, W), SENTINEL, dtype=q.dtype, device=DEV)
    body = gbuf[: B * T].view(B, T, W)
    outs = tuple(body[..., 8 + i * HD: 8 + (i + 1) * HD] for i in range(3))
    nat.attn_causal_bwd(qd, kd, vd, go.to(DEV), H, scale, out=outs)
    g = gbuf.cpu()
    assert torch.all(g[:, :8] == SENTINEL) and torch.all(g[:, 8 + 3 * HD:] == SENTINEL) and torch.all(g[B * T] == SENTINEL)
    return [o.cpu()] + [t.cpu().contiguous() for t in outs]


def _check(close, shape, dtype, seed, strided=False, what=()):
    (q, k, v, go), ref = _case(shape, dtype, seed)
    H, d = shape[2], shape[3]
    got = _run(q, k, v, go, H, d ** -0.5, strided)
    for name, a, b in zip(NAMES, got, ref):
        tag = (name, shape, str(dtype), "strided" if strided else "dense") + tuple(what)
        err = ((a.double() - b).norm() / (b.norm() + 1e-30)).item()
        print(tag, "rel", err)
        if float(b.abs().max()) == 0.0:
            assert float(a.double().abs().max()) < 2.0 ** -16, tag  # (module docstring)
        else:
            close(a, b, TOL[dtype], tag)
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("key", KEYS, ids=lambda k: "-".join(map(str, k)))
def test_every_instantiation_against_float64(close, key, dtype):
    _check(close, INSTANTIATIONS[key], dtype, seed=KEYS.index(key), what=(key,))


# T = 1: a single key; 16 | 17: the block boundary; 77: the workload; 96 | 97: NKF 6 → 8; 128: the upper limit
EDGE_T = [1, 16, 17, 77, 96, 97, 128]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "grouped"])
@pytest.mark.parametrize("T", EDGE_T)
def test_token_count_edges(close, T, strided, dtype):
    _check(close, (2, T, 3, 64), dtype, seed=T, strided=strided, what=("T", T))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "grouped"])
@pytest.mark.parametrize("d", [8, 96])
def test_narrowest_and_widest_head(close, d, strided, dtype):
    _check(close, (2, 77, 3, d), dtype, seed=d, strided=strided, what=("d", d))


# plan_causal gives a workgroup rows 0–63 / 64–127 of a (batch, head) only while that adds workgroups the chip has room for:
# 2·B·H ≤ 512 forward, ≤ 256 backward.  Past that one workgroup owns all 128 rows and every wave runs its row loop TWICE
# (blocks t0 and t0 + 64): the prefetched Q / dO rows are handed over, the wave's Q / dO / P / dS tiles in LDS are rewritten
# behind the first block's transposing reads, the diagonal fragment moves, dK/dV accumulate over two blocks and the reduce
# kernel sums one partial.  B·H = 144: backward only; B·H = 264: both directions, at the workload's 77 tokens and at the limit.
TWO_BLOCK_SHAPES = [(12, 77, 12, 64), (22, 77, 12, 64), (22, 128, 12, 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "grouped"])
@pytest.mark.parametrize("shape", TWO_BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_two_blocks_per_wave(close, shape, strided, dtype):
    from tests.causal_attention_cases import causal_chunks

    B, T, H, d = shape
    assert causal_chunks(B, T, H, True) == (1, 128)  # (the shape reaches the path it is here for)
    assert causal_chunks(B, T, H, False) == ((1, 128) if B * H > 256 else (2, 64))
    _check(close, shape, dtype, seed=B + T, strided=strided, what=("two blocks per wave",))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", [(2, 77, 3, 64)] + TWO_BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_causality_bit_for_bit(shape, dtype):
    """O[:, :i0+1] does not move when the rows after i0 of Q, K and V change; dK[:, j0:] and dV[:, j0:] do not move when the
    rows before j0 of dO change (a key receives gradient only from the queries at or after it).  Also where a wave runs two
    blocks (TWO_BLOCK_SHAPES), with cuts inside the second block."""
    B, T, H, d = shape
    (q, k, v, go), _ = _case(shape, dtype, B + T if shape in TWO_BLOCK_SHAPES else 77)
    scale = d ** -0.5
    qd, kd, vd, gd = (t.to(DEV) for t in (q, k, v, go))
    o = nat.attn_causal_fwd(qd, kd, vd, H, scale)
    _, dk, dv = nat.attn_causal_bwd(qd, kd, vd, gd, H, scale)
    g = torch.Generator().manual_seed(5)
    for i0 in (0, 15, 16, 40, 63, 64, 70, 111):
        if i0 >= T - 1:
            continue
        q2, k2, v2 = (t.clone() for t in (qd, kd, vd))
        for t in (q2, k2, v2):
            t[:, i0 + 1:] = torch.randn(B, T - i0 - 1, H * d, generator=g).to(dtype).to(DEV)
        o2 = nat.attn_causal_fwd(q2, k2, v2, H, scale)
        assert torch.equal(o2[:, : i0 + 1], o[:, : i0 + 1]), i0
        assert not torch.equal(o2[:, i0 + 1:], o[:, i0 + 1:]), i0  # (the change was seen where it may be)
    for j0 in (16, 17, 64, 76, 127):
        if j0 >= T:
            continue
        g2 = gd.clone()
        g2[:, :j0] = torch.randn(B, j0, H * d, generator=g).to(dtype).to(DEV)
        _, dk2, dv2 = nat.attn_causal_bwd(qd, kd, vd, g2, H, scale)
        assert torch.equal(dk2[:, j0:], dk[:, j0:]) and torch.equal(dv2[:, j0:], dv[:, j0:]), j0
        assert not torch.equal(dv2[:, :j0], dv[:, :j0]), j0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_two_runs_are_bit_identical(dtype):
    for shape in ((2, 77, 3, 64), (2, 128, 3, 96), (22, 128, 12, 64)):
        (q, k, v, go), _ = _case(shape, dtype, shape[0] + shape[1] if shape[0] > 2 else shape[1])
        first = _run(q, k, v, go, shape[2], shape[3] ** -0.5, False)
        second = _run(q, k, v, go, shape[2], shape[3] ** -0.5, False)
        for name, a, b in zip(NAMES, first, second):
            assert torch.equal(a, b), (shape, name)


def test_unsupported_shapes_are_refused_before_any_launch():
    lib = nat.lib()
    f16 = nat.dtype_code(torch.float16)
    for B, T, H, d, dt in ((2, 77, 2, 104, torch.float16), (2, 129, 2, 64, torch.float16), (2, 77, 2, 64, torch.float32),
                           (2, 77, 2, 60, torch.bfloat16)):
        assert not nat.attn_causal_supported(B, T, H, d, dt)
        x = torch.zeros(B, T, H * d, dtype=dt, device=DEV)
        assert not causal_attention_supported(x, H)
        with pytest.raises(RuntimeError):
            causal_attention(x, x, x, H)
        code = nat.dtype_code(dt)
        o = torch.full_like(x, SENTINEL)
        st = lib.attn_causal_fwd_strided(x.data_ptr(), x.data_ptr(), x.data_ptr(), o.data_ptr(), H * d, B, T, H, d, 0.125,
                                         code, nat._stream(x))
        assert st == -1 and torch.all(o == SENTINEL)  # LORA_E_BADARG (-1), nothing written
        if dt != torch.float32:  # (the workspace size does not depend on the dtype)
            assert lib.attn_causal_bwd_workspace_bytes(B, T, H, d) == -1
        ws = torch.zeros(1 << 20, dtype=torch.float32, device=DEV)
        st = lib.attn_causal_bwd_strided(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), o.data_ptr(), o.data_ptr(),
                                         o.data_ptr(), ws.data_ptr(), H * d, H * d, B, T, H, d, 0.125, code, nat._stream(x))
        assert st == -1 and torch.all(o == SENTINEL)
    assert lib.attn_causal_supported(2, 77, 2, 64, f16) == 1
    with pytest.raises(RuntimeError):  # CPU tensors: no composite fallback in the front
        causal_attention(*(torch.zeros(1, 8, 64, dtype=torch.float16),) * 3, 1)
