"""sampling.sigma_schedule on the CPU: the collapsed tables against the stateful float64 samplers of tests/sigma_reference.py
over whole runs, the DDIM identity that ties the sigma-space restatement to `sampler_schedule`, the tables' structure, the
validation errors and the rows an image-to-image run starts at."""
import math

import numpy as np
import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import sampling as smp
from tests import sigma_reference as sr

METHODS = ("euler", "euler_a", "heun")
SAMPLER_NAME = {"euler": "k_euler", "euler_a": "euler_a", "heun": "heun"}  # LatentSampler's: "euler" stays an unknown method there
STEPS = (1, 2, 3, 10, 50)
SAMPLER_NAME_INVERSE = {v: k for k, v in SAMPLER_NAME.items()}
PUSH, SAVE, USE_SAVED = 1, 2, 4


def _apply(coef, plan, i, x, o, z, xs, hist):
    """Iteration i of the collapsed form, in the table's own precision; (x', xs, hist)."""
    p, q, a, c0, c1, s = (float(c) for c in coef[i, :6])
    flags = int(plan[i, 4])
    h = p * x + q * o
    base = xs if flags & USE_SAVED else x
    new = a * base + c0 * h
    if c1 != 0.0:
        new = new + c1 * hist
    if s != 0.0:
        new = new + s * z
    return new, (x if flags & SAVE else xs), (h if flags & PUSH else hist)


@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("v", [False, True])
@pytest.mark.parametrize("S", STEPS)
@pytest.mark.parametrize("method", METHODS)
def test_collapsed_tables_follow_the_stateful_samplers(method, S, v, karras):
    ts, sigmas, coef, plan = dfa.sigma_schedule(method, S, v, karras_sigmas=karras, coef_dtype=torch.float64)
    ref = sr.make(method, S, v, karras)
    n_it = 2 * S - 1 if method == "heun" else S
    assert ts.dtype == sigmas.dtype == coef.dtype == torch.float64 and plan.dtype == torch.int32
    assert tuple(ts.shape) == (n_it,) and tuple(sigmas.shape) == (S + 1,) and tuple(coef.shape) == (n_it, 8)
    assert tuple(plan.shape) == (n_it, 5)
    np.testing.assert_allclose(sigmas.numpy(), np.array(ref.sigmas), rtol=1e-12, atol=0)
    g = torch.Generator().manual_seed(S * 8 + v * 2 + karras)
    x = ref.start(torch.randn(2, 33, generator=g, dtype=torch.float64))
    got, xs, hist, worst = x.clone(), None, None, 0.0
    for i in range(n_it):
        assert not ref.done
        assert abs(float(ts[i]) - ref.model_timestep) <= 1e-9 * max(1.0, ref.model_timestep)  # (log-σ interpolation: 1e-12 of σ)
        assert abs(float(coef[i, 7]) - ref.model_sigma) <= 1e-12 * ref.model_sigma
        o, z = torch.randn(2, 33, generator=g, dtype=torch.float64), torch.randn(2, 33, generator=g, dtype=torch.float64)
        assert abs(float(coef[i, 5]) - ref.noise_scale) <= 1e-12 * max(1.0, ref.noise_scale)
        x = ref.step(x, o, z)
        got, xs, hist = _apply(coef, plan, i, got, o, z, xs, hist)
        err = float((got - x).abs().max() / x.abs().max())
        worst = max(worst, err)
        assert err <= 1e-12, (i, err)
        n_want = 1.0 if ref.done else 1.0 / math.sqrt(ref.model_sigma ** 2 + 1.0)  # c_in of the NEXT evaluation
        assert abs(float(coef[i, 6]) - n_want) <= 1e-12
    assert ref.done
    print(f"\n[{method} S {S} v {v} karras {karras}] worst relative difference {worst:.3g}")
    # the fp32 table is the float64 one rounded once
    ts32, sig32, coef32, plan32 = dfa.sigma_schedule(method, S, v, karras_sigmas=karras)
    assert coef32.dtype == torch.float32 and torch.equal(coef32, coef.float()) and torch.equal(plan32, plan)
    assert torch.equal(ts32, ts) and torch.equal(sig32, sigmas) and ts32.dtype == torch.float64


@pytest.mark.parametrize("v", [False, True])
@pytest.mark.parametrize("S", [10, 50])
@pytest.mark.parametrize("method,eta", [("euler", 0.0), ("euler_a", 1.0)])
def test_on_a_shared_integer_grid_euler_is_ddim(method, eta, S, v):
    """For the state y = c_in(σ)·x the sigma step is y' = (n·(a + c0·p)/n_prev)·y + (n·c0·q)·o + (n·s)·z: DDIM's (a, b, σ) at
    η = 0 for euler and at η = 1 for euler_a, to one fp32 rounding of the existing table's entry."""
    ddim_ts, ddim = dfa.sampler_schedule("ddim", S, v, eta)
    ts, sigmas, coef, _ = dfa.sigma_schedule(method, S, v, timesteps=ddim_ts.tolist(), coef_dtype=torch.float64)
    assert ts.tolist() == [float(t) for t in ddim_ts]
    ratio, worst, checked = 1000 // S, 0.0, 0
    for i in range(S):
        if int(ddim_ts[i]) - ratio < 0:
            continue
        p, q, a, c0, _, s = (float(c) for c in coef[i, :6])
        n_prev, n = (1.0 / math.sqrt(float(sg) ** 2 + 1.0) for sg in (sigmas[i], sigmas[i + 1]))
        for mine, theirs in zip((n * (a + c0 * p) / n_prev, n * c0 * q, n * s), ddim[i].tolist()):
            worst = max(worst, abs(mine - theirs) / max(1.0, abs(theirs)))
            assert abs(mine - theirs) <= 2.0 ** -24 * max(1.0, abs(theirs)), (i, mine, theirs)
        checked += 1
    print(f"\n[{method} == ddim eta {eta} S {S} v {v}] {checked} steps, worst |Δ|/max(1, |coef|) {worst:.3g}")
    assert checked == S - 1


@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("S", STEPS)
def test_structure(S, karras):
    table = sr.sigma_table()
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    acp = np.cumprod(1.0 - betas)
    sigma_max = math.sqrt((1.0 - acp[999]) / acp[999])
    assert abs(sigma_max - 14.6146) < 1e-4 and abs(float(table[-1]) - sigma_max) <= 1e-12 * sigma_max
    for method in METHODS:
        for v in (False, True):
            ts, sigmas, coef, plan = dfa.sigma_schedule(method, S, v, karras_sigmas=karras, coef_dtype=torch.float64)
            assert float(ts[0]) == 999.0 and abs(float(sigmas[0]) - sigma_max) <= 1e-12 * sigma_max and float(sigmas[-1]) == 0.0
            assert bool((sigmas[:-1].diff() < 0).all()) and bool((ts.diff() <= 0).all())
            assert float(coef[-1, 6]) == 1.0 and float(coef[-1, 5]) == 0.0
            assert not plan[:, :4].any()
            flags = plan[:, 4].tolist()
            if method == "heun":
                assert flags == [SAVE | PUSH, USE_SAVED] * (S - 1) + [0]
                assert ts.tolist()[1::2] == ts.tolist()[2::2]  # stage B and the next stage A see the same timestep
                used = torch.tensor([bool(f & USE_SAVED) for f in flags])
                assert bool((coef[used, 4] != 0.0).all()) and bool((coef[~used, 4] == 0.0).all())
            else:
                assert flags == [0] * S and bool((coef[:, 4] == 0.0).all())
            if method != "euler_a":
                assert bool((coef[:, 5] == 0.0).all())
            else:
                assert bool((coef[:-1, 5] > 0.0).all())
            if not v:
                assert bool((coef[:, 0] == 0.0).all()) and bool((coef[:, 1] == 1.0).all())
            # the reference's own walk: timestep and σ of every evaluation
            for row, (t, sg, _, _) in zip(coef, sr.walk(method, S, v, karras)):
                assert abs(float(row[7]) - sg) <= 1e-12 * sg


def test_default_grid_is_fractional_linspace():
    ts, sigmas, _, _ = dfa.sigma_schedule("euler", 50, False)
    assert ts.tolist() == np.linspace(0, 999, 50)[::-1].tolist()
    assert abs(float(ts[1]) - 978.6122448979592) < 1e-9 and float(ts[-1]) == 0.0
    table = sr.sigma_table()
    assert abs(float(sigmas[1]) - (table[978] + (float(ts[1]) - 978) * (table[979] - table[978]))) < 1e-12


def test_validation_errors():
    with pytest.raises(ValueError, match="unknown sigma-space sampling method"):
        dfa.sigma_schedule("ddim", 10, False)
    for bad in (0, -1, 1001):
        with pytest.raises(ValueError, match="num_inference_steps"):
            dfa.sigma_schedule("euler", bad, False)
    with pytest.raises(ValueError, match="coef_dtype"):
        dfa.sigma_schedule("euler", 10, False, coef_dtype=torch.float16)
    with pytest.raises(ValueError, match="exclude"):
        dfa.sigma_schedule("euler", 3, False, karras_sigmas=True, timesteps=[900, 500, 1])
    for grid in ([1, 500, 900], [900, 500, 500], [1000, 500, 1], [900, 500, -1], [900.0, float("nan"), 1.0]):
        with pytest.raises(ValueError, match="strictly descending"):
            dfa.sigma_schedule("heun", 3, False, timesteps=grid)
    with pytest.raises(ValueError, match="must hold num_inference_steps"):
        dfa.sigma_schedule("heun", 3, False, timesteps=[900, 1])


class _Unet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(4, 4, 1)


def test_sampler_arguments_are_checked_before_anything_is_allocated():
    with pytest.raises(ValueError, match="eta must be 0"):
        dfa.LatentSampler(_Unet(), method="euler_a", eta=1.0)
    with pytest.raises(ValueError, match="karras_sigmas belongs"):
        dfa.LatentSampler(_Unet(), method="ddim", karras_sigmas=True)
    with pytest.raises(ValueError, match="unknown sampling method"):
        dfa.LatentSampler(_Unet(), method="euler_b")
    with pytest.raises(ValueError, match="unknown sampling method"):  # as before: plain Euler is "k_euler" on the sampler
        dfa.LatentSampler(_Unet(), method="euler")
    assert smp.SAMPLER_SIGMA_METHODS == SAMPLER_NAME_INVERSE
    s = dfa.LatentSampler(_Unet(), num_inference_steps=25, method="heun", karras_sigmas=True)
    assert s.num_model_evaluations == 49 and s.timesteps.dtype == torch.float64 and tuple(s.sigmas.shape) == (26,)
    assert s._schedule_args[-1] is True and s.latents is None
    assert dfa.LatentSampler(_Unet(), method="ddim").sigmas is None
    a = dfa.LatentSampler(_Unet(), num_inference_steps=4, method="k_euler")._fingerprint([])
    b = dfa.LatentSampler(_Unet(), num_inference_steps=4, method="k_euler", karras_sigmas=True)._fingerprint([])
    assert a[0] != b[0]  # the Karras flag is part of what a recording bakes in


@pytest.mark.parametrize("method", METHODS)
def test_partial_rows(method):
    S = 8
    sampler = dfa.LatentSampler(_Unet(), num_inference_steps=S, method=SAMPLER_NAME[method])
    n_full = sampler.num_model_evaluations
    for strength, n in ((0.75, 6), (0.5, 4), (0.13, 1), (1.0, 8)):
        got_n, k0 = dfa.partial_start(S, strength)
        assert (got_n, k0) == (n, S - n)
        row, n_it, ts, coef, plan = sampler._run_tables(k0)
        assert row == (2 * k0 if method == "heun" else k0) and n_it == (2 * n - 1 if method == "heun" else n)
        assert row + n_it == n_full and ts is sampler.timesteps and coef is sampler.coef and plan is sampler.plan
        # the tail rows are the fresh sub-run: it begins at a stage that reads neither xs nor H, at σ_{k0}
        assert float(coef[row, 4]) == 0.0 and not int(plan[row, 4]) & USE_SAVED
        assert abs(float(coef[row, 7]) - float(sampler.sigmas[k0])) <= 1e-6 * float(sampler.sigmas[k0])
    with pytest.raises(ValueError, match="leaves no step"):
        dfa.partial_start(S, 0.1)
    keep = smp.sigma_keep_schedule(sampler.coef)
    assert keep.dtype == torch.float32 and tuple(keep.shape) == (n_full, 2) and keep[-1].tolist() == [1.0, 0.0]
    assert torch.equal(keep[:-1, 1], sampler.coef[1:, 7]) and bool((keep[:, 0] == 1.0).all())


def test_sigma_state_checks_its_buffers():
    ts, _, coef, plan = dfa.sigma_schedule("heun", 3, False)
    x, m_in, cur = torch.zeros(2, 4, 8, 8), torch.zeros(4, 4, 8, 8), torch.zeros(2, dtype=torch.int32)
    t = torch.zeros(4)
    ok = (x, x.clone(), x.clone(), m_in, t, cur, ts.float(), coef, plan, True)

    def swapped(i, value):
        args = list(ok)
        args[i] = value
        return args

    for i, value, match in ((1, torch.zeros(2, 4, 8, 4), "disagree"), (2, torch.zeros(4, 2, 4, 8, 8), "disagree"),
                            (4, torch.zeros(4, dtype=torch.int64), "fp32"), (6, ts, "fp32"), (7, coef[:, :7].contiguous(), "fp32"),
                            (8, plan.long(), "fp32"), (3, torch.zeros(4, 4, 8, 16)[..., ::2], "disagree|contiguous")):
        with pytest.raises(ValueError, match=match):
            nat.SigmaState(*swapped(i, value))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.SigmaState(*ok)
    lib = nat.lib()
    assert lib.ddpm_sample_sigma(*([None] * 14), 1, 4, 4, 1, 0, 0, 1.0, 0, None) == -1
    assert lib.ddpm_sample_sigma_init(*([None] * 7), 1, 4, 1, 0, 0.0, 1.0, 1.0, 0, 0, 0, 0, None) == -1
