"""CPU-only guards for the attention-core tests (tests/test_gpu_attention_cores.py):

1. the instantiation table of tests/attention_cases.py names exactly the dispatch-table kernels of csrc/attn_flash.hip
   and csrc/attn_ctx.hip, and the planners select every one of them — a kernel added there without a test shape, or one
   that no plan selects, fails here;
2. the three-part check `assert_close` rejects the plausible attention-kernel bugs it is meant to catch, at the f16 and
   bf16 bounds of the GPU tests."""
import os
import re

import pytest
import torch

from tests.attention_cases import (CTX_BWD, CTX_FWD, FLASH_BWD, FLASH_FWD, INSTANTIATIONS, attention_reference, ctx_keys,
                                   flash_keys, key_of)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffusion_finetuning_amd", "csrc")


def _dispatch_lines(name, macro):
    """Argument tuples of every use of `macro(...)` in the dispatch function of csrc/<name> (not its #define)."""
    with open(os.path.join(CSRC, name)) as f:
        src = f.read()
    uses = re.findall(r"(?<!#define )\b%s\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*(?:,\s*(\d+)\s*)?\)" % macro, src)
    return [tuple(int(x) for x in u if x) for u in uses]


def compiled_instantiations():
    keys = set()
    for ks, df, rb in _dispatch_lines("attn_flash.hip", "FLASH_CASE"):
        keys |= {(FLASH_FWD, ks, df, rb, False), (FLASH_FWD, ks, df, rb, True)}  # launch_flash_fwd builds both forms
    keys |= {(FLASH_BWD,) + c for c in _dispatch_lines("attn_flash.hip", "FLASH_BCASE")}
    for c in _dispatch_lines("attn_ctx.hip", "CTX_CASE"):
        keys |= {(CTX_FWD,) + c, (CTX_BWD,) + c}
    keys |= {(CTX_FWD,) + c for c in _dispatch_lines("attn_ctx.hip", "CTX_FWD_ONLY")}
    keys |= {(CTX_BWD,) + c for c in _dispatch_lines("attn_ctx.hip", "CTX_BWD_ONLY")}
    return keys


def test_dispatch_tables_hold_only_the_planned_cases():
    flash = _dispatch_lines("attn_flash.hip", "FLASH_CASE")
    assert len(flash) == 6 and len(_dispatch_lines("attn_flash.hip", "FLASH_BCASE")) == 6
    assert len(_dispatch_lines("attn_ctx.hip", "CTX_CASE")) == 8
    assert _dispatch_lines("attn_ctx.hip", "CTX_FWD_ONLY") == [(5, 10, 6)]
    assert _dispatch_lines("attn_ctx.hip", "CTX_BWD_ONLY") == [(5, 5, 6)]
    # every forward bucket has exactly one ONES width, 16·(DF − 1) + 8
    for ks, df, rb in flash:
        ones = [d for d in range(8, 161, 8) if d % 16 == 8 and d // 16 == df - 1]
        assert ones == [16 * (df - 1) + 8]


def test_every_compiled_instantiation_has_a_test_shape():
    compiled = compiled_instantiations()
    assert set(INSTANTIATIONS) == compiled, (
        "untested", compiled - set(INSTANTIATIONS), "not compiled", set(INSTANTIATIONS) - compiled)


def test_table_shapes_reach_their_instantiations_and_the_plan_reaches_nothing_else():
    for key, shape in INSTANTIATIONS.items():
        assert key_of(key[0], shape) == key, (key, shape)
    # the planner mirrors select only table entries, over everything *_supported accepts
    reach = set()
    for d in range(8, 161, 8):
        reach |= set(flash_keys(d))
        for Tk in range(1, 129):
            keys = ctx_keys(Tk, d)
            if keys is not None:
                reach |= set(keys)
    assert reach == set(INSTANTIATIONS)


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_planner_mirrors_match_the_knob_free_cpp_planners():
    """flash_keys / ctx_keys copy plan_flash, launch_flash_fwd and plan_ctx; pin them to the C++ they copy, so a change of
    a bucket there (and with it the kernel a table shape lands on) fails here instead of going unnoticed."""
    src = _source("attn_flash.hip")
    body = src[src.index("bool plan_flash("):src.index("template <int KS, int DF> constexpr int flash_fwd_lds")]
    fields = r"\{\s*pl->ks = (\d+); pl->df = (\d+); pl->rb = (\d+); pl->rb_dq = (\d+); pl->nkw = (\d+); \}"
    buckets = [(int(m[0]),) + tuple(int(x) for x in m[1:])
               for m in re.findall(r"if \(d <= (\d+)\) " + fields, body)]
    last = re.search(r"else " + fields, body)
    assert len(buckets) == 5 and last, body
    buckets.append((160,) + tuple(int(x) for x in last.groups()))
    lo = 8
    for top, ks, df, rb, rbq, nkw in buckets:
        for d in range(lo, top + 1, 8):
            fwd, bwd = flash_keys(d)
            assert fwd[1:4] == (ks, df, rb) and bwd[1:] == (ks, df, rbq, nkw), (d, fwd, bwd)
        lo = top + 8
    assert "(a.d % 16) == 8 && a.d / 16 == DF - 1" in src  # the ONES condition of launch_flash_fwd
    ctx = _source("attn_ctx.hip")
    plan = ctx[ctx.index("bool plan_ctx("):ctx.index("template <int KS, int DF, int NKF> constexpr int fwd_lds")]
    for line in ("d > 160 || Tk > 128) return false;", "if (d > 96 && Tk > 96) return false;", "if (d <= 96) {",
                 "pl->ks = d <= 64 ? 2 : 3;", "pl->df = (d + 15) / 16;", "if (pl->df < 3) pl->df = 3;", "pl->ks = 5;",
                 "pl->df = backward ? 5 : 10;", "pl->nkf = Tk <= 96 ? 6 : 8;"):
        assert line in plan, line


# ---- sensitivity of assert_close ---------------------------------------------------------------------------------------

TOLS = {"f16": 2e-3, "bf16": 1.2e-2}  # the bounds of tests/test_gpu_attention_cores.py
DK_WIDEST = 1.5  # that file judges flash dK at 1.5× (its FLASH_DK): bug (b) must be caught there too
B, TQ, TK, H, D = 2, 300, 33, 4, 40


@pytest.fixture(scope="module")
def reference():
    """A correct f16 kernel, as far as the check can tell: float64 attention and its dK on a ragged shape, rounded to f16."""
    g = torch.Generator().manual_seed(0)
    q, k, v, go = (torch.randn(B, T, H * D, generator=g).half().double() for T in (TQ, TK, TK, TQ))
    k.requires_grad_(True)
    o = attention_reference(q, k, v, H)
    (dk,) = torch.autograd.grad(o, (k,), go)
    return q, k.detach(), v, o.detach(), dk


DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def test_assert_close_accepts_a_correctly_rounded_result(close, reference):
    q, k, v, o, dk = reference
    for dt, tol in TOLS.items():
        close(o.to(DT[dt]), o, tol)
        close(dk.to(DT[dt]), dk, tol)


# What the older whole-tensor-only bar (rel_err < tol) says about the same three bugs at this shape (measured):
#   (a) one query row without its last key: rel 3.3e-3 (f16) / 3.7e-3 (bf16) — passes the bf16 bar, caught at f16;
#       assert_close rejects it at both by the row (7.4e-2) and element (0.38) bars.  (With 77 keys the same bug moves
#       its row by only 1 %, which the bf16 row bar, 4.8e-2, does not see; the f16 one does.)
#   (b) one key's dK row zeroed in one head: rel 6.2e-2 over dK's 264 head-rows — caught here, but the whole-tensor
#       ratio falls as 1/√rows: past ~7,000 head-rows (e.g. 4096 keys × 4 heads) it passes bf16.
#   (c) one output row taken from the neighbouring batch: rel 6.3e-2 over 2,400 head-rows — caught here; passes bf16
#       past ~66,000 head-rows.
# The row and element bars of assert_close do not depend on the tensor's size.
OLD_BAR_PASSES = {"a": {"bf16"}, "b": set(), "c": set()}


def _bug_a(q, k, v, o):
    """Query row 37 of batch 0, head 1 misses the last key (a ragged-tile mask one key too short)."""
    bad = o.clone()
    t, h, sl = 37, 1, slice(1 * D, 2 * D)
    qh, kh, vh = q[0, t, sl], k[0, : TK - 1, sl], v[0, : TK - 1, sl]
    bad[0, t, sl] = torch.softmax(kh @ qh * D ** -0.5, dim=0) @ vh
    return bad


def test_assert_close_rejects_injected_attention_bugs(close, relerr, reference):
    q, k, v, o, dk = reference
    bugs = {"a": (_bug_a(q, k, v, o), o)}
    bad = dk.clone()
    bad[1, TK - 1, 2 * D: 3 * D] = 0.0  # (b) the last key's dK row of batch 1, head 2 never written (zeroed)
    bugs["b"] = (bad, dk)
    bad = o.clone()
    bad[0, TQ - 1] = o[1, TQ - 1]  # (c) the last query row of batch 0 read from batch 1
    bugs["c"] = (bad, o)
    for name, (bad, want) in bugs.items():
        for dt, tol in TOLS.items():
            got = bad.to(DT[dt])
            with pytest.raises(AssertionError):
                close(got, want, tol * (DK_WIDEST if name == "b" else 1.0))
            assert (relerr(got, want) < tol) == (dt in OLD_BAR_PASSES[name]), (name, dt, relerr(got, want))
