"""Per-row gates of the fused forward at operator level (MI355X): `lora_linear_fwd_rows` / `lora_linear_geglu_fwd_rows`.

    Y[m,:] = X[m,:]·Wᵀ + b + Σ_j (s · G[m div rps, j]) · P[m,j] · B[:,j]          (csrc/lora_gemm.hip, RS kernels)

Shapes: tests/row_scale_cases.py — the smallest shape of every single-layer class of tests/gemm_cases.py (ring classes of
both row-tile heights, fallback, generic, both split tiles), M a multiple of 77, every dtype the class admits, ranks 1 / 4 / 16
(20 on the generic class), rows-per-sample 1, 77 and M; and the gated `proj` launch at K = 64, F = 64, M = 154.

 (a) a uniform table IS the scalar launch, bit for bit: table ≡ g at scale 1, and table ≡ 1 at scale g, against today's entry
     at scale g.  The kernels form (s·G) in fp32 first and multiply it into P, so both are the scalar launch's arithmetic.
 (b) a closed gate IS scale 0, bit for bit, and in the same launch every open sample's rows are (a)'s rows for its value —
     any row → sample slip at a tile or fragment boundary shows.
 (c) slot selection: four rank-4 adapters stacked to rank 16, one-hot tables, random sample → adapter assignment, against the
     float64 restatement of W x + b + B_k A_k x on the compute-dtype operands.  Bound: 2 × the max-abs error of TODAY's entry
     running adapter k alone at rank 4 on the same rows against the same float64 values (the stacked operand changes the order
     of the 32 products inside the one extra MFMA step and nothing else).  Both figures are printed.
 (d) the `_rows` entries' own LORA_E_BADARG cases launch nothing and write nothing.
Every output lies inside the guard bands of tests/test_gpu_gemm_edges.py; P must be the un-gated launch's P exactly.

Measured on MI355X for (c), max-abs error against float64, worst class per dtype: f16 9.768e-04 for today's rank-4 entry and
9.768e-04 for the gated rank-16 stack, bf16 7.812e-03 and 7.812e-03, f32 1.767e-06 and 1.767e-06 — in every class the two
figures are EQUAL: the closed slots contribute exact zeros and the open slots' products land in the same MFMA step.
"""
import pytest
import torch

from diffusion_finetuning_amd import _native as nat
from tests.gemm_cases import ESIZE, GENERIC, SPLIT, make_layer
from tests.row_scale_cases import (GEGLU_SHAPE, NAME, RPS, case_id, mixed_table, one_hot_table, operator_cases,
                                   sample_counts)
from tests.test_gpu_gemm_edges import Banded, launch_fwd, off_by_one_element, workspace_for

pytestmark = pytest.mark.gpu
DEV = "cuda"
G1, G2 = 0.7, -1.25  # gate values (neither a power of two)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def launch_rows(x, w, b, down, up, packs, y, t, scale, table, n_samples, ld, ws=None):
    """The raw entry; returns its status."""
    M, K = x.shape
    return nat.lib().lora_linear_fwd_rows(_ptr(x), _ptr(w), _ptr(b), _ptr(down), _ptr(up), _ptr(packs[0]), _ptr(packs[1]),
                                          _ptr(y), _ptr(t), M, K, w.shape[0], down.shape[0], float(scale), _ptr(table),
                                          n_samples, ld, nat.dtype_code(x.dtype), _ptr(ws),
                                          0 if ws is None else ws.numel() * 4, nat._stream(x))


class Layer:
    """Device operands of one case (+ the split-K workspace its class wants)."""

    def __init__(self, key, shape, dtype, r, seed=0):
        (M, Kc, Nc), aligned = shape[:3], len(shape) < 4
        x, w, b, down, up, _ = make_layer(M, Kc, Nc, r, dtype, seed=M + Kc + Nc + r + seed)
        self.host = (x, w, b, down, up)
        self.M, self.K, self.N, self.r, self.dtype = M, Kc, Nc, r, dtype
        xa = x.to(DEV)
        self.x = xa if aligned else off_by_one_element(xa)
        self.w, self.b, self.down, self.up = w.to(DEV), b.to(DEV), down.to(DEV), up.to(DEV)
        self.packs = nat.lora_pack_factors(self.down, self.up, dtype)
        self.ws = workspace_for(M, Kc, Nc, dtype, key)

    def today(self, scale, what, down=None, up=None, packs=None):
        """(Y, T) of the entry without gates."""
        down, up = (self.down, self.up) if down is None else (down, up)
        Y, T = Banded(self.M, self.N, self.dtype), Banded(self.M, down.shape[0], torch.float32)
        launch_fwd(self.x, self.w, self.b, down, up, self.packs if packs is None else packs, Y.view, T.view, scale, self.ws)
        return Y.check((what, "y")), T.check((what, "t"))

    def gated(self, scale, table, what):
        table = table.to(DEV).contiguous()
        Y, T = Banded(self.M, self.N, self.dtype), Banded(self.M, self.r, torch.float32)
        st = launch_rows(self.x, self.w, self.b, self.down, self.up, self.packs, Y.view, T.view, scale, table, table.shape[0],
                         table.stride(0), self.ws)
        assert st == 0, (what, st)
        if self.ws is not None:
            assert int(self.ws.view(torch.int32)[:1024].abs().max().item()) == 0, (what, "ticket header not left at zero")
        return Y.check((what, "y")), T.check((what, "t"))


def _params():
    return [pytest.param(*c, id=case_id(*c)) for c in operator_cases()]


@pytest.mark.parametrize("key,shape,dtype,r", _params())
def test_uniform_table_is_the_scalar_launch_exactly(key, shape, dtype, r):
    """(a).  On the MFMA forms the gated factor (s·G) is formed first and multiplied into P, the scalar launch's own arithmetic.
    The shape-agnostic kernels (the `generic` class, and r = 20 anywhere) scale the SUM when ungated, s·(Σ_j P_j·Q_j); their gated
    form is that arithmetic at slot 0's factor plus the other slots' deviations from it, Σ_j ((f_j − f_0)·P_j)·Q_j, every one an
    exact zero under equal gates — so the identity holds there bit for bit as well."""
    what = (NAME[dtype], key, shape, r)
    L = Layer(key, shape, dtype, r)
    y_ref, t_ref = L.today(G1, (what, "today", G1))
    assert bool((y_ref != L.today(0.0, (what, "today", 0.0))[0]).any()), (what, "the rank-r term does not show in this case")
    R = r + 3  # (a table wider than the rank: ld_scale > r)
    misses = []
    for n in sample_counts(L.M):
        for scale, fill in ((1.0, G1), (G1, 1.0)):
            y, t = L.gated(scale, torch.full((n, R), fill), (what, "uniform", n, scale))
            assert torch.equal(t, t_ref), (what, "P is not the un-gated P", n, scale)
            if not torch.equal(y, y_ref):
                misses.append((n, scale, int((y != y_ref).sum()), float((y.double() - y_ref.double()).abs().max())))
    print("uniform table vs scalar launch %s: %s" % (what, ["n_samples %d scale %.1f: %d elements differ, max abs %.3e" % m
                                                           for m in misses] or "bit-identical"))
    assert not misses, (what, misses)


@pytest.mark.parametrize("key,shape,dtype,r", _params())
def test_closed_gates_are_scale_zero_and_open_samples_keep_their_value(key, shape, dtype, r):
    """(b): one launch with closed and open samples side by side.  Closed samples' rows are today's entry at scale 0, exactly;
    open samples' rows are (a)'s output — the uniform-table launch — for their value, exactly (and, on the MFMA forms, today's
    entry at that scale)."""
    what = (NAME[dtype], key, shape, r)
    L = Layer(key, shape, dtype, r)
    R = r + 3
    y_zero, t_ref = L.today(0.0, (what, "today", 0.0))
    for n in sample_counts(L.M)[:2]:
        uniform = {g: L.gated(1.0, torch.full((n, R), g), (what, "uniform", n, g))[0] for g in (G1, G2)}
        table, which = mixed_table(n, R, (G1, G2), seed=r)
        y, t = L.gated(1.0, table, (what, "mixed", n))
        assert torch.equal(t, t_ref), (what, "P is not the un-gated P", n)
        row_which = which.repeat_interleave(L.M // n).to(DEV)
        for v, want in ((-1, y_zero), (0, uniform[G1]), (1, uniform[G2])):
            rows = row_which == v
            if not bool(rows.any()):  # (two samples: one closed, one open)
                assert n < 4 and v >= 0
                continue
            assert torch.equal(y[rows], want[rows]), (what, "samples of kind", v, "rows per sample", L.M // n)
        if key[0] != GENERIC and r <= 16:  # the MFMA forms: (a) holds, so the open samples are today's entry too
            for v, g in ((0, G1), (1, G2)):
                rows = row_which == v
                if bool(rows.any()):
                    assert torch.equal(y[rows], L.today(g, (what, "today", g))[0][rows]), (what, "vs today at", g, L.M // n)


def _stack_params():
    return [pytest.param(k, s, d, id=case_id(k, s, d, 16)) for k, s, d, r in operator_cases() if r == 16]


ERRORS = {}  # dtype name -> worst (today's error, gated error) over the classes, printed by the last case


@pytest.mark.parametrize("key,shape,dtype", _stack_params())
def test_one_hot_tables_select_one_stacked_adapter_per_sample(key, shape, dtype):
    what = (NAME[dtype], key, shape)
    K_AD, r = 4, 4
    L = Layer(key, shape, dtype, K_AD * r)  # the stacked layer: rank 16, adapter k in slots [4k, 4k + 4)
    x, w, b, down, up = L.host
    n = L.M // RPS
    g = torch.Generator().manual_seed(L.M + n)
    assign = torch.randint(0, K_AD, (n,), generator=g)
    assign[:K_AD] = torch.arange(K_AD)[:n]  # every adapter is used where there are enough samples
    slots = [slice(k * r, (k + 1) * r) for k in range(K_AD)]
    # float64 restatement, and TODAY's entry running adapter k alone at rank 4, composed per sample
    base = x.double() @ w.double().t() + b.double()
    p64 = x.double() @ down.double().t()
    ref = torch.empty(L.M, L.N, dtype=torch.float64)
    today = torch.empty(L.M, L.N, dtype=dtype, device=DEV)
    row_k = assign.repeat_interleave(RPS)
    for k in range(K_AD):
        rows = row_k == k
        if not bool(rows.any()):
            continue
        ref[rows] = base[rows] + p64[rows][:, slots[k]] @ up.double()[:, slots[k]].t()
        dk, uk = L.down[slots[k]].contiguous(), L.up[:, slots[k]].contiguous()
        yk, _ = L.today(1.0, (what, "adapter", k), dk, uk, nat.lora_pack_factors(dk, uk, dtype))
        today[rows.to(DEV)] = yk[rows.to(DEV)]
    y, t = L.gated(1.0, one_hot_table(assign, slots, K_AD * r), (what, "one-hot"))
    _, t_plain = L.today(1.0, (what, "stacked, no gates"))
    assert torch.equal(t, t_plain), (what, "P is not the un-gated P")
    e_today = float((today.double().cpu() - ref).abs().max())
    e_gated = float((y.double().cpu() - ref).abs().max())
    print("max abs error vs float64 %s: today's rank-4 entry %.3e, gated rank-16 stack %.3e (bound %.3e)" % (
        what, e_today, e_gated, 2 * e_today))
    worst = ERRORS.setdefault(NAME[dtype], [0.0, 0.0])
    worst[0], worst[1] = max(worst[0], e_today), max(worst[1], e_gated)
    print("worst so far per dtype (today, gated):", {k: ("%.3e" % v[0], "%.3e" % v[1]) for k, v in ERRORS.items()})
    assert e_gated <= 2 * e_today, (what, e_gated, e_today)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("r", [1, 4, 16])
def test_gated_proj_launch_honours_the_table(dtype, r):
    """The GEGLU-gated instantiation (`lora_linear_geglu_fwd_rows`): (a), (b) and — at r = 16 — (c) on out = h·gelu(g)
    and on the [h | g] tile it leaves when asked."""
    M, K, F = GEGLU_SHAPE
    what = (NAME[dtype], "geglu", GEGLU_SHAPE, r)
    x, w, b, down, up, _ = make_layer(M, K, 2 * F, r, dtype, seed=M + K + F + r)
    xd, wd, bd, downd, upd = x.to(DEV), w.to(DEV), b.to(DEV), down.to(DEV), up.to(DEV)
    packs = nat.lora_pack_factors(downd, upd, dtype)
    scalar = {}
    for g in (G1, G2, 0.0, 1.0):
        res = nat.lora_linear_geglu_fwd(xd, wd, bd, r, g, packs, True)
        assert res is not None, (what, "the smallest supported shape is not supported")
        scalar[g] = res
    out_ref, y_ref, t_ref = scalar[G1]
    assert bool((out_ref != scalar[0.0][0]).any())
    R = r + 1
    for n in sample_counts(M):
        for scale, fill in ((1.0, G1), (G1, 1.0)):
            for want_y in (True, False):
                res = nat.lora_linear_geglu_fwd_rows(xd, wd, bd, r, scale, torch.full((n, R), fill, device=DEV), packs, want_y)
                assert res is not None
                out, y, t = res
                assert torch.equal(out, out_ref) and torch.equal(t, t_ref), (what, "uniform", n, scale, want_y)
                assert (y is None and not want_y) or torch.equal(y, y_ref), (what, "uniform y", n, scale)
        if n == 1:
            continue
        table, which = mixed_table(n, R, (G1, G2), seed=r)
        out, y, t = nat.lora_linear_geglu_fwd_rows(xd, wd, bd, r, 1.0, table.to(DEV), packs, True)
        row_which = which.repeat_interleave(M // n).to(DEV)
        for v, g in ((-1, 0.0), (0, G1), (1, G2)):
            rows = row_which == v
            if not bool(rows.any()):
                assert n < 4 and v >= 0
                continue
            assert torch.equal(out[rows], scalar[g][0][rows]) and torch.equal(y[rows], scalar[g][1][rows]), (what, "gate", g, n)
        assert torch.equal(t, t_ref)
    if r == 16:  # (c): y = [h | g] against float64 with the bound of the ungated classes; out follows from y exactly
        slots = [slice(4 * k, 4 * k + 4) for k in range(4)]
        assign = torch.tensor([2, 1])
        ref = torch.empty(M, 2 * F, dtype=torch.float64)
        today = torch.empty(M, 2 * F, dtype=dtype, device=DEV)
        base = x.double() @ w.double().t() + b.double()
        for i, k in enumerate(assign.tolist()):
            rows = slice(i * RPS, (i + 1) * RPS)
            ref[rows] = base[rows] + (x.double()[rows] @ down.double()[slots[k]].t()) @ up.double()[:, slots[k]].t()
            dk, uk = downd[slots[k]].contiguous(), upd[:, slots[k]].contiguous()
            today[rows] = nat.lora_linear_geglu_fwd(xd, wd, bd, 4, 1.0, nat.lora_pack_factors(dk, uk, dtype), True)[1][rows]
        out, y, t = nat.lora_linear_geglu_fwd_rows(xd, wd, bd, r, 1.0, one_hot_table(assign, slots, 16).to(DEV), packs, True)
        e_today, e_gated = float((today.double().cpu() - ref).abs().max()), float((y.double().cpu() - ref).abs().max())
        print("max abs error vs float64 %s: today's rank-4 entry %.3e, gated rank-16 stack %.3e" % (what, e_today, e_gated))
        assert e_gated <= 2 * e_today, (what, e_gated, e_today)
        assert torch.equal(out, nat.geglu_gate_fwd(y)) and torch.equal(t, scalar[1.0][2])


def test_bad_calls_return_badarg_and_write_nothing():
    M, K, N, r, dtype = 154, 64, 128, 4, torch.float16
    x, w, b, down, up, _ = make_layer(M, K, N, r, dtype, seed=5)
    xd, wd, bd, downd, upd = x.to(DEV), w.to(DEV), b.to(DEV), down.to(DEV), up.to(DEV)
    packs = nat.lora_pack_factors(downd, upd, dtype)
    table = torch.ones(2, r, device=DEV)
    y = torch.full((M, N), 3.0, dtype=dtype, device=DEV)
    out = torch.full((M, N // 2), 3.0, dtype=dtype, device=DEV)
    t = torch.full((M, r), 3.0, device=DEV)
    bad = [("n_samples < 1", table, 0, r), ("n_samples < 1", table, -2, r), ("M % n_samples", table, 4, r),
           ("ld_scale < r", table, 2, r - 1), ("null table", None, 2, r)]
    for why, tab, n, ld in bad:
        st = launch_rows(xd, wd, bd, downd, upd, packs, y, t, 1.0, tab, n, ld)
        assert st == -1, (why, st)
        st = nat.lib().lora_linear_geglu_fwd_rows(_ptr(xd), _ptr(wd), _ptr(bd), _ptr(packs[0]), _ptr(packs[1]), _ptr(y),
                                                  _ptr(out), _ptr(t), M, K, N, r, 1.0, _ptr(tab), n, ld, nat.dtype_code(dtype),
                                                  nat._stream(xd))
        assert st == -1, (why, "geglu", st)
    torch.cuda.synchronize()
    for buf in (y, out, t):
        assert torch.equal(buf, torch.full_like(buf, 3.0))
    # the envelope of the gated entry is the ungated entry's: fp32 has no fused gate kernel
    xf, wf, bf = xd.float(), wd.float(), bd.float()
    pf = nat.lora_pack_factors(downd, upd, torch.float32)
    assert nat.lora_linear_geglu_fwd_rows(xf, wf, bf, r, 1.0, table, pf, True) is None
    # the wrappers refuse a table that does not fit before anything is launched
    for tab in (torch.ones(4, r, device=DEV), torch.ones(2, r - 1, device=DEV), torch.ones(2, r, device=DEV).double(),
                torch.ones(2, r)):
        with pytest.raises((ValueError, RuntimeError)):
            nat.lora_linear_fwd_rows(xd, wd, bd, downd, upd, 1.0, tab, packs)
    assert ESIZE[dtype] == 2 and GENERIC and SPLIT
