"""The one-launch NCHW form of the fused GroupNorm (csrc/norm.hip: nchw_one_fwd_kernel / nchw_one_bwd_kernel, one workgroup of
1024 threads per (n, group) slab, 2, 5 or 8 chunks of 8 elements per thread forward and 2 or 5 backward) at its own edges, and
the two-launch form at the tails that the shapes of tests/norm_cases.py no longer reach now that the planner sends them to one
launch.  Every case first asks `group_norm_act_plan` which form it is about to run.

Yardsticks Y1 / Y2 / Y3 are those of test_gpu_norm_edges.py (float64 on the same stored inputs; fused error ≤ the stock
composite's in the storage type and in fp32, + 1 ulp; mean / rstd within 2⁻¹³), through that module's own helpers."""
import pytest
import torch
import torch.nn.functional as F

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import norm as dnorm
from diffusion_finetuning_amd.norm import group_norm_act_res, group_norm_tokens, group_norm_tokens_supported
from tests.norm_cases import SMALL_GROUPS
from tests.test_gpu_norm import VARIANTS, _errs, _ulp
from tests.test_gpu_norm_edges import (HARD, _check_y1_y2, _check_y3, _hard_case, _inputs_hw,
                                       test_kernels_write_only_inside_their_tensors_and_the_workspace_formula_covers_them as _guarded)

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
_id = lambda c: "n%d-c%d-g%d-%dx%d" % c
THREADS = 1024  # kOneThreads


def _plan(shape, backward):
    N, C, G, H, W = shape
    return nat.lib().group_norm_act_plan(N, C, H * W, G, 0, int(backward))


def _chunks(shape):
    N, C, G, H, W = shape
    return C // G * (H * W // 8)


def _planner_edge(backward):
    """(largest one-launch shape, smallest two-launch shape) for one sample of one group of 3 channels, from the query."""
    m = max(m for m in range(1, 4000) if nat.lib().group_norm_act_plan(1, 3, 8 * m, 1, 0, backward) == 1)
    return (1, 3, 1, 8, m), (1, 3, 1, 8, m + 1)


# (shape, variants or None for all five, what it is)
ALL, TWO = None, [VARIANTS[0], VARIANTS[2]]  # TWO: SiLU + addend, identity without: the larger tensors
ONE_LAUNCH = [
    ((1, 6, 3, 2, 4), ALL),         # 2 chunks in a slab, 1022 threads idle
    ((3, 6, 6, 5, 8), ALL),         # cpg = 1: da exactly 0
    ((1, 66, 2, 8, 17), ALL),       # 17 chunks per row: channel boundaries inside a wave's run of chunks
    ((2, 72, 1, 4, 4), ALL),        # cpg = 72 > 64
    ((1, 264, 1, 2, 4), ALL),       # cpg = 264 > 256: more channels than the da fold takes at once with 4 lanes each
    ((9, 64, 32, 4, 4), ALL),       # 288 workgroups, more than CUs
    ((1, 256, 128, 64, 128), TWO),  # 2 · 1024 chunks: the 2-chunk kernels full (128 slabs: the planner's middle class)
    ((1, 384, 128, 8, 683), TWO),   # 2 · 1024 + 1: the 5-chunk kernels with one chunk in their third pass
    ((1, 1280, 256, 64, 128), TWO),  # 5 · 1024 chunks: the 5-chunk kernels full (256 slabs), the backward's capacity
]
FWD_ONLY = [
    ((1, 768, 256, 8, 1707), TWO),  # 5 · 1024 + 1 chunks: forward 8-chunk kernel, backward on two launches
    ((1, 2048, 256, 64, 128), TWO),  # 8 · 1024 chunks: the forward's capacity
]


def _run_case(shape, variants, dtype, plans, seed):
    assert (_plan(shape, 0), _plan(shape, 1)) == plans, (shape, _chunks(shape))
    G, bad = shape[2], []
    for vi, (act, with_a, eps) in enumerate(variants or VARIANTS):
        x, a, w, b, dy = _inputs_hw(shape, dtype, False, seed + vi)
        a = a if with_a else None
        tag = f"{shape} plan={plans} {dtype}"
        fused = _check_y1_y2(tag, x, a, w, b, dy, G, eps, act, False, bad)
        _check_y3(tag, x, a, w, b, G, eps, act, False, bad)
        if with_a and shape[1] == G:  # one channel per group: dx sums to zero over it
            assert (fused[2] == 0).all(), tag
    assert not bad, bad


@DTYPES
@pytest.mark.parametrize("shape,variants", ONE_LAUNCH, ids=[_id(s) for s, _ in ONE_LAUNCH])
def test_one_launch_both_ways_at_the_kernels_edges_against_float64(shape, variants, dtype):
    _run_case(shape, variants, dtype, (1, 1), 900)


@DTYPES
@pytest.mark.parametrize("shape,variants", FWD_ONLY, ids=[_id(s) for s, _ in FWD_ONLY])
def test_one_launch_forward_with_a_two_launch_backward_against_float64(shape, variants, dtype):
    _run_case(shape, variants, dtype, (1, 2), 920)


@DTYPES
@pytest.mark.parametrize("backward", [0, 1], ids=["fwd-limit", "bwd-limit"])
def test_planner_edge_largest_one_launch_slab_and_smallest_two_launch_slab(backward, dtype):
    inside, outside = _planner_edge(backward)
    print(f"planner edge, backward={backward}: {_chunks(inside)} chunks on one launch, {_chunks(outside)} on two")
    assert _plan(inside, backward) == 1 and _plan(outside, backward) == 2
    for shape in (inside, outside):
        _run_case(shape, TWO, dtype, (_plan(shape, 0), _plan(shape, 1)), 940)


# ---------------------------------------------------------------------------------------------------------- hard statistics
# SMALL_GROUPS is on one launch; BIG_GROUP (32768 chunks) is not, and the nearest one-launch shape of one sample is the backward's
# limit at fewer than 128 slabs: one group of 1280 chunks = 10 240 elements
NEAR_BIG = (1, 20, 1, 16, 32)
HARD_KINDS = [(d, k) for d, k in HARD if k[0] in ("mean", "first", "other", "addend", "constant", "tiny", "saturated")]


@pytest.mark.parametrize("shape", [NEAR_BIG, SMALL_GROUPS], ids=_id)
@pytest.mark.parametrize("dtype,kind", HARD_KINDS, ids=lambda v: str(v).replace("torch.", "") if isinstance(v, torch.dtype)
                         else "-".join(str(p) for p in v))
def test_hard_statistics_on_one_launch_against_float64(dtype, kind, shape):
    assert (_plan(shape, 0), _plan(shape, 1)) == (1, 1)
    G = shape[2]
    x, a, w, b, dy, variants = _hard_case(kind, shape, dtype, False, 300)
    tag, bad = f"{kind} {shape} one launch {dtype}", []
    for act, with_a, eps in variants:
        aa = a if with_a else None
        fused = _check_y1_y2(tag, x, aa, w, b, dy, G, eps, act, False, bad)
        _, rstd = _check_y3(tag, x, aa, w, b, G, eps, act, False, bad)
        if kind[0] == "constant":  # x̂ = 0: y = act(β) rounded once, rstd = eps^-½
            beta = b.float()[None, :, None, None].expand_as(x)
            want = (F.silu(beta) if act else beta).to(dtype)
            assert (fused[0].double() - want.double()).abs().max().item() <= _ulp(want.double(), dtype), tag
            assert ((rstd.double() * eps ** 0.5) - 1).abs().max().item() <= 2.0 ** -13, tag
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------- dh
RES_SHAPE = (2, 64, 8, 8, 16)  # 128 chunks per slab, C % 8 == 0 and H·W % 8 == 0 for the token front


def _dh_case(front, dtype, seed=40):
    """Fused (dx[, da]) of the front with dh joined, the same from the stock lines in `dtype`, and float64."""
    N, C, G, H, W = RES_SHAPE
    x, a, w, b, dy = _inputs_hw(RES_SHAPE, dtype, False, seed)
    dh = torch.randn(x.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed + 1)).to(dtype)
    tok = front == "tokens"
    eps, a = (1e-6, None) if tok else (1e-5, a)
    to_tok = lambda t: t.permute(0, 2, 3, 1).reshape(N, H * W, C)
    dout = to_tok(dy).contiguous() if tok else dy

    def stock(cast):
        xs = cast(x).detach().requires_grad_(True)
        as_ = None if a is None else cast(a).detach().requires_grad_(True)
        h = xs if as_ is None else xs + as_[:, :, None, None]
        y = F.group_norm(h, G, cast(w), cast(b), eps)
        y = to_tok(y) if tok else F.silu(y)
        g = torch.autograd.grad([xs * 1, y], [xs] + ([] if as_ is None else [as_]), [cast(dh), cast(dout)])
        return list(g)

    xs = x.detach().clone().requires_grad_(True)
    as_ = None if a is None else a.detach().clone().requires_grad_(True)
    if tok:
        assert group_norm_tokens_supported(xs, G, w, b)
        xp, y = group_norm_tokens(xs, G, w, b, eps)
    else:
        xp, y = group_norm_act_res(xs, G, w, b, eps, True, as_)
    fused = list(torch.autograd.grad([xp, y], [xs] + ([] if as_ is None else [as_]), [dh, dout], retain_graph=True))
    return fused, stock(lambda t: t), stock(lambda t: t.double()), (xs, xp, y, dh)


@DTYPES
@pytest.mark.parametrize("front", ["res", "tokens"])
def test_dh_joins_dx_before_its_one_rounding_on_a_one_launch_shape(front, dtype, monkeypatch):
    assert (_plan(RES_SHAPE, 0), _plan(RES_SHAPE, 1)) == (1, 1)
    fused, stock, ref, (xs, xp, y, dh) = _dh_case(front, dtype)
    for name, f, s, r in zip(("dx", "da"), fused, stock, ref):
        (fmax, frms), (smax, srms), ulp = _errs(f, r), _errs(s, r), _ulp(r, dtype)
        print(f"{front} {dtype} {name}: fused max {fmax:.3e} rms {frms:.3e} | stock max {smax:.3e} rms {srms:.3e} | ulp {ulp:.3e}")
        assert fmax <= smax + ulp and frms <= srms + ulp, (front, name)
    # dy absent: dh passes through as dx, no launch
    calls, real = [], nat.group_norm_act_bwd_res
    monkeypatch.setattr(nat, "group_norm_act_bwd_res", lambda *t: calls.append(1) or real(*t))
    (dx,) = torch.autograd.grad([xp], [xs], [dh], retain_graph=True)
    assert torch.equal(dx, dh) and not calls


# ---------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("shape", [(4, 1280, 32, 8, 8), (8, 320, 32, 64, 64)], ids=["floor-5KB", "80KB-slab"])
def test_two_runs_are_bit_identical_and_a_graph_replay_equals_eager(shape):
    assert (_plan(shape, 0), _plan(shape, 1)) == (1, 1)
    G = shape[2]
    x, a, w, b, dy = _inputs_hw(shape, torch.float16, False, 60)
    dh = dy.flip(0).contiguous()

    def run():
        y, mean, rstd = nat.group_norm_act_fwd(x, a, w, b, G, 1e-5, True, 0)
        dx, da = nat.group_norm_act_bwd_res(dy, dh, x, a, w, b, mean, rstd, G, True, True)
        return y, mean, rstd, dx, da

    first, second = run(), run()
    assert all(torch.equal(u, v) for u, v in zip(first, second))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(captured, first))


# ----------------------------------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("want_da", [0, 1], ids=["no-da", "da"])
@pytest.mark.parametrize("shape", [(3, 40, 4, 4, 10), (1, 384, 128, 8, 683)], ids=_id)
def test_one_launch_kernels_write_only_inside_their_tensors(shape, want_da):
    """test_gpu_norm_edges' guarded-buffer check (sentinel guards around every operand, the workspace exactly as long as the
    formula says, results equal to the plain call's) on two one-launch shapes: 50 chunks, and 2049 with a lone chunk in pass 3."""
    assert (_plan(shape, 0), _plan(shape, 1)) == (1, 1)
    _guarded(False, shape, want_da, torch.float16)


# ------------------------------------------------------------------------------------------- the two-launch form's tails
# above the planner's limit for fewer than 128 slabs (1920 chunks forward, 1280 backward), so still on two launches
TWO_LAUNCH_TAILS = [
    (1, 2, 1, 64, 256),    # 2 rows: the statistics workgroup has 2 of its 4 waves past the end; 4096 chunks
    (1, 3, 3, 128, 128),   # cpg = 1: a group is one row, the fold has a single partial; 3 rows; 2048 chunks a slab
    (1, 6, 2, 8, 683),     # 2049 chunks → 5 slices of 410: every boundary in mid-row (683 chunks a row), 410 % 256 ≠ 0
    (1, 72, 1, 16, 32),    # cpg = 72 > 64: the fold's lane loop has a remainder pass of 8 lanes; 4608 chunks → 9 slices
]


@DTYPES
@pytest.mark.parametrize("shape", TWO_LAUNCH_TAILS, ids=_id)
def test_two_launch_form_keeps_its_tail_coverage_against_float64(shape, dtype):
    _run_case(shape, ALL, dtype, (2, 2), 960)
