"""`lora_prodigy_moments` + `lora_prodigy_apply` (csrc/prodigy.hip) through the C ABI on the device, against the float64
restatement and the bounds of tests/prodigy_cases.py: every class of the launch grid, ranges that end inside a vector, every
branch of the scalar step, the options, the overflow rule, the EMA form, run-to-run bits and a 60-step trajectory."""
import math

import pytest
import torch

from diffusion_finetuning_amd import _native as nat
from tests import ema_cases as ec
from tests import prodigy_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda"


def run_kernels(p, p0, g, m, v, s, st, cfg, t=1, norm_sq=0.0, flagged=False, shadow=None, ema=(0.0, 0), mutant=None):
    """One step through the two launches; the signature of prodigy_cases.step_f32 (so `trajectory` can drive it).  Returns the
    buffers on the host, "state" (d, d_max, numerator, d_hat, denom), all eight "scalars" and the "shadow"."""
    assert mutant is None
    n = p.numel()
    h = pc._hp(cfg, n)
    p, p0, g, m, v, s = (x.detach().float().reshape(-1).clone().to(DEV) for x in (p, p0, g, m, v, s))
    norm = torch.tensor([norm_sq, 1.0 if flagged else 0.0, float(t), 0.0], dtype=torch.float32, device=DEV)
    sc = torch.tensor([st["d"], st["d_max"], st["numerator"], 0, 0, 0, 0, 0], dtype=torch.float32, device=DEV)
    sh = None if shadow is None else shadow.clone().to(DEV)
    nat.lora_prodigy_moments(p, p0, g, m, v, s, h["ends"], cfg["lr"], norm, sc, cfg["mul"], cfg["max_norm"], cfg["beta1"],
                             cfg["beta2"], cfg["beta3"], cfg["d0"], cfg["d_coef"], cfg["growth_rate"], cfg["bias_correction"],
                             cfg["safeguard"])
    nat.lora_prodigy_apply(p, m, v, sh, h["ends"], cfg["lr"], cfg["wd"], norm, sc, cfg["beta1"], cfg["beta2"], cfg["eps"],
                           cfg["bias_correction"], ema[0], ema[1])
    sc = sc.cpu()
    wrote = float(sc[3]) != 0.0  # d_prev: the launch ran its scalar step
    return {"p": p.cpu(), "m": m.cpu(), "v": v.cpu(), "s": s.cpu(), "scalars": sc, "shadow": None if sh is None else sh.cpu(),
            "state": {"d": float(sc[0]), "d_max": float(sc[1]), "numerator": float(sc[2]),
                      "d_hat": float(sc[4]) if wrote else None, "denom": float(sc[5]) if wrote else None}}


def _check(ins, st, cfg, t=1, clip=False):
    n = ins[0].numel()
    norm_sq = pc.norm_sq_of(ins[2], cfg) if clip else 0.0
    ref = pc.reference(*ins, st, cfg, t, norm_sq)
    got = run_kernels(*ins, st, cfg, t, norm_sq)
    w = pc.worst(got, ref, pc.bounds(ref, n, clip))
    print(n, ref["state"]["branch"], {k: float("%.3g" % x) for k, x in w.items()})
    assert max(w.values()) <= 1.0, (n, ref["state"]["branch"], w)
    assert got["state"]["d"] >= st["d"] and float(got["scalars"][3]) == st["d"]
    return ref, got


@pytest.mark.parametrize("n", pc.ALL_SIZES)
def test_grid_edges(n):
    ins = pc.inputs(n)
    for cfg, st, t, clip in pc.GRID_CONFIGS:
        ref, got = _check(ins, st, cfg, t, clip)
        assert {"d", "numerator", "denom"} <= {k for k, x in got["state"].items() if x is not None}
    # (tests/test_prodigy_host.py shows, for every config, the share of both sums planted in each range a wrong bound would drop)


@pytest.mark.parametrize("case", range(len(pc.RANGE_CASES)))
def test_ranges_end_inside_a_vector(case):
    ends, lr, wd = pc.RANGE_CASES[case]
    n = pc.RANGE_N
    ins = pc.inputs(n, plant=False)
    for e in ends[:-1]:  # (a live gradient either side of every boundary)
        ins[2][e - 1], ins[2][e] = 0.37, -0.21
    cfg = pc.config(ends=ends, lr=lr, wd=wd, growth_rate=1.02)
    ref, got = _check(ins, pc.MID_RUN, cfg, 7)
    bnd = pc.bounds(ref, n, False)
    # the elements either side of every boundary take their own range's values: with the boundaries moved by one they would not
    moved = pc.reference(*ins, pc.MID_RUN, pc.config(ends=tuple(e + 1 for e in ends[:-1]) + (n,), lr=lr, wd=wd, growth_rate=1.02), 7)
    for e in ends[:-1]:
        for key in ("p", "s"):
            assert abs(float(moved[key][e] - ref[key][e])) > 4 * float(bnd[key][e]), (e, key)  # (the check can tell)
            for i in (e - 1, e):
                assert abs(float(got[key][i]) - float(ref[key][i])) <= float(bnd[key][i]), (e, i, key)


def test_branches_of_the_scalar_step():
    n = 1027
    ins = pc.inputs(n)
    # the first growth from d == d0 is not rate-limited
    cfg = pc.config(growth_rate=1.02)
    ref, got = _check(ins, pc.state(), cfg, 1)
    assert ref["state"]["branch"] == "first growth" and got["state"]["d"] > 2 * pc.f32(cfg["d0"])
    # later growth is
    ref, got = _check(ins, pc.MID_RUN, cfg, 7)
    assert ref["state"]["branch"] == "rate-limited" and got["state"]["d_max"] > 2 * got["state"]["d"]
    assert abs(got["state"]["d"] / pc.MID_RUN["d"] - pc.f32(1.02)) < 1e-6
    # without a limit d jumps to d_max
    ref, got = _check(ins, pc.MID_RUN, pc.config(), 7)
    assert ref["state"]["branch"] == "d_max" and got["state"]["d"] == got["state"]["d_max"] > pc.MID_RUN["d_max"]
    # d_hat < d: d and d_max keep their bits
    low, level = pc.inputs(n, s_scale=30.0), pc.LEVEL
    ref, got = _check(low, level, pc.config(), 7)
    assert ref["state"]["branch"] == "d_hat below d" and 0 < got["state"]["d_hat"] < level["d"]
    assert got["state"]["d"] == level["d"] and got["state"]["d_max"] == level["d_max"]
    assert got["state"]["numerator"] != level["numerator"]
    # denom == 0 (no gradient, no s): the scalars keep their bits and p moves by weight decay alone
    p, p0, g, m, v, s = (x.clone() for x in ins)
    g.zero_(), s.zero_(), m.zero_()
    cfg = pc.config(wd=(0.1,), lr=(0.5,))
    ref, got = _check((p, p0, g, m, v, s), pc.MID_RUN, cfg, 7)
    assert ref["state"]["branch"] == "denom == 0" and got["state"]["denom"] == 0.0
    assert [got["state"][k] for k in ("d", "d_max", "numerator")] == [pc.MID_RUN[k] for k in ("d", "d_max", "numerator")]
    assert not ec.same_bits(got["p"], p) and float((got["p"].double() - ref["p"]).abs().max()) <= 8 * pc.U * float(p.abs().max())
    assert ec.same_bits(got["v"], pc.step_f32(p, p0, g, m, v, s, pc.MID_RUN, cfg, 7)["v"])
    # every γ = 0: s and the numerator decay, d stays, p keeps its bits
    cfg = pc.config(lr=(0.0,), wd=(0.1,))
    ref, got = _check(ins, pc.MID_RUN, cfg, 7)
    assert ref["state"]["branch"] == "all lr zero" and got["state"]["d"] == pc.MID_RUN["d"]
    assert got["state"]["d_max"] == pc.MID_RUN["d_max"] and ec.same_bits(got["p"], ins[0])
    assert abs(got["state"]["numerator"] / (pc.f32(cfg["beta3"]) * pc.MID_RUN["numerator"]) - 1) < 1e-6


@pytest.mark.parametrize("t", (1, 2, 1000))
def test_bias_correction_follows_the_device_counter(t):
    ins = pc.inputs(1027)
    on, off = pc.config(bias_correction=True, wd=(0.1,)), pc.config(wd=(0.1,))
    ref_on, got_on = _check(ins, pc.MID_RUN, on, t)
    ref_off, got_off = _check(ins, pc.MID_RUN, off, t)
    bnd = pc.bounds(ref_on, 1027, False)
    assert float(((ref_on["p"] - ref_off["p"]).abs() / bnd["p"]).max()) > 100  # (the option shows at every t)
    assert not ec.same_bits(got_on["p"], got_off["p"]) and ec.same_bits(got_on["m"], got_off["m"])


def test_safeguard_warmup():
    ins = pc.inputs(1027)
    on, off = pc.config(safeguard=True, lr=(0.5,)), pc.config(lr=(0.5,))
    ref_on, got_on = _check(ins, pc.MID_RUN, on, 7)
    ref_off, got_off = _check(ins, pc.MID_RUN, off, 7)
    bnd = pc.bounds(ref_on, 1027, False)
    assert float(((ref_on["s"] - ref_off["s"]).abs() / bnd["s"]).max()) > 100
    assert not ec.same_bits(got_on["s"], got_off["s"]) and ec.same_bits(got_on["m"], got_off["m"])
    # at γ·bc = 1 the two forms are the same arithmetic
    same = run_kernels(*ins, pc.MID_RUN, pc.config(safeguard=True), 7)
    plain = run_kernels(*ins, pc.MID_RUN, pc.config(), 7)
    assert all(ec.same_bits(same[k], plain[k]) for k in ("p", "m", "v", "s", "scalars"))


@pytest.mark.parametrize("n", (3, 1027, pc.OVER_THE_CAP))
def test_an_overflowed_step_changes_nothing(n):
    ins = pc.inputs(n)
    shadow = ec.ema_inputs(n)[4]
    got = run_kernels(*ins, pc.MID_RUN, pc.config(wd=(0.1,)), 7, flagged=True, shadow=shadow, ema=(ec.MAX_DECAY, 0))
    for key, before in zip(("p", "m", "v", "s"), (ins[0], ins[3], ins[4], ins[5])):
        assert ec.same_bits(got[key], before), key
    assert ec.same_bits(got["shadow"], shadow)
    assert got["scalars"].tolist() == [pc.MID_RUN["d"], pc.MID_RUN["d_max"], pc.MID_RUN["numerator"], 0, 0, 0, 0, 0]
    plain = run_kernels(*ins, pc.MID_RUN, pc.config(wd=(0.1,)), 7, flagged=True)
    assert ec.same_bits(plain["p"], ins[0]) and ec.same_bits(plain["s"], ins[5])


@pytest.mark.parametrize("n", (3, 5, 1027, 257 * 1024 + 1))
@pytest.mark.parametrize("t,after", ((1, 0), (3, 0), (11, 0), (6, 5), (200000, 0)))
def test_ema_form(n, t, after):
    ins = pc.inputs(n)
    shadow = ec.ema_inputs(n)[4]
    cfg = pc.config(wd=(0.1,), bias_correction=True)
    plain = run_kernels(*ins, pc.MID_RUN, cfg, t)
    with_ema = run_kernels(*ins, pc.MID_RUN, cfg, t, shadow=shadow, ema=(ec.MAX_DECAY, after))
    assert all(ec.same_bits(plain[k], with_ema[k]) for k in ("p", "m", "v", "s", "scalars"))
    assert ec.same_bits(with_ema["shadow"], ec.ema_emulate(shadow, with_ema["p"], ec.omd_at(t, ec.MAX_DECAY, after)))
    assert not ec.same_bits(with_ema["shadow"], shadow)


def test_two_runs_agree_bit_for_bit():
    ins = pc.inputs(pc.OVER_THE_CAP)
    cfg = pc.config(growth_rate=1.02, wd=(0.1,))
    a, b = (run_kernels(*ins, pc.MID_RUN, cfg, 7) for _ in range(2))
    assert all(ec.same_bits(a[k], b[k]) for k in ("p", "m", "v", "s", "scalars"))
    assert a["state"]["d"] > pc.MID_RUN["d"]


def test_trajectory_on_the_quadratic():
    ref_ds, ref_p, ref_loss = pc.trajectory(pc.reference, torch.float64)
    ds, p, loss = pc.trajectory(run_kernels, torch.float32)
    d_rel, p_abs = pc.trajectory_deviation(ds, p, ref_ds, ref_p)
    print(f"d relative deviation {d_rel:.3g} (allowed {4 * pc.TRAJ_D_REL:.3g}), p absolute deviation {p_abs:.3g} "
          f"(allowed {4 * pc.TRAJ_P_ABS:.3g}); d: {ds[0]:.3g} -> {ds[-1]:.3g}, loss {loss[0]:.3g} -> {loss[-1]:.3g}")
    assert all(b >= a for a, b in zip(ds, ds[1:])) and ds[-1] > 1000 * ds[0] and math.isfinite(loss[-1])
    assert d_rel <= 4 * pc.TRAJ_D_REL and p_abs <= 4 * pc.TRAJ_P_ABS, (d_rel, p_abs)
