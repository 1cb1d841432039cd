"""Host side of the latent sampler: `sampler_schedule`'s collapsed (a, b, σ) against the uncollapsed float64 step of
tests/sampling_reference.py, the argument validation of the three C entries without a launch, and LatentSampler's argument errors.
(That header, exports and bindings agree is tests/test_native_abi.py's business.)"""
import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import sampling
from tests import sampling_reference as ref

CASES = [("ddpm", 0.0), ("ddim", 0.0), ("ddim", 1.0)]
STEPS = (1, 4, 50, 1000)


def test_public_names():
    assert dfa.LatentSampler is sampling.LatentSampler and dfa.sampler_schedule is sampling.sampler_schedule
    assert {"ddpm_sample_init", "ddpm_sample_step", "ddpm_sample_advance"} <= set(nat.SIGNATURES)


@pytest.mark.parametrize("v_prediction", [False, True])
@pytest.mark.parametrize("S", STEPS)
@pytest.mark.parametrize("method,eta", CASES)
def test_schedule_equals_the_uncollapsed_step(method, eta, S, v_prediction):
    ts, coef = dfa.sampler_schedule(method, S, v_prediction, eta)
    assert ts.dtype == torch.int64 and tuple(ts.shape) == (S,) and coef.dtype == torch.float32 and tuple(coef.shape) == (S, 3)
    assert ts.tolist() == ref.timesteps(method, S)
    assert all(a > b for a, b in zip(ts.tolist(), ts.tolist()[1:])) and 0 <= int(ts.min()) and int(ts.max()) < 1000
    g = torch.Generator().manual_seed(S * 7 + int(v_prediction))
    x, o, z = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(3))
    worst = 0.0
    for i in (range(S) if S <= 50 else list(range(0, S, 37)) + [S - 1]):
        a, b, sg = (float(c) for c in coef[i].double())
        want = ref.step(method, S, i, x, o, z, v_prediction, eta)
        got = a * x + b * o + sg * z
        # (a, b, σ) are single fp32 roundings of float64 values: 6e-8 each on terms no larger than |a·x| + |b·o| + |σ·z| —
        # judged element by element against that sum, and as a whole against the reference's norm
        scale = (a * x).abs() + (b * o).abs() + (sg * z).abs()
        worst = max(worst, float(((got - want).abs() / scale).max()), float((got - want).norm() / want.norm()))
        assert abs(sg - ref.sigma(method, S, i, eta)) <= 1e-6 * max(sg, 1e-30) or sg == ref.sigma(method, S, i, eta) == 0.0
    assert worst <= 1e-6, worst
    if method == "ddpm":
        assert float(coef[-1, 2]) == 0.0 and (S == 1 or bool((coef[:-1, 2] > 0).all()))
    elif eta == 0.0:
        assert bool((coef[:, 2] == 0).all())
    else:  # (at t = 0 — S = 1000, where the offset has no room — ᾱ_p = ᾱ[0] = ᾱ_t: that last σ is 0)
        assert bool((coef[:-1, 2] > 0).all()) and float(coef[-1, 2]) >= 0.0


@pytest.mark.parametrize("method,eta", CASES)
def test_a_single_step_takes_the_branch_below_timestep_zero(method, eta):
    """S = 1: t_prev = t − 1000 < 0, so ᾱ_p is 1 (ddpm: the step returns x0 itself) or ᾱ[0] (ddim)."""
    ts, coef = dfa.sampler_schedule(method, 1, False, eta)
    acp = ref.alphas_cumprod()
    t = int(ts[0])
    assert t == (0 if method == "ddpm" else 1)
    a, b, _ = (float(c) for c in coef[0].double())
    s, q = float(acp[t].sqrt()), float((1 - acp[t]).sqrt())
    if method == "ddpm":  # x' = x0 = (x − q·o)/s
        assert a == pytest.approx(1 / s, rel=1e-6) and b == pytest.approx(-q / s, rel=1e-6)
    elif eta == 0.0:  # x' = √ᾱ_0·x0 + √(1−ᾱ_0)·o
        s0, q0 = float(acp[0].sqrt()), float((1 - acp[0]).sqrt())
        assert a == pytest.approx(s0 / s, rel=1e-6) and b == pytest.approx(q0 - s0 * q / s, rel=1e-5, abs=1e-9)


def test_schedule_rejects_bad_arguments():
    for args in (("plms", 50, False), ("ddpm", 0, False), ("ddpm", 1001, False), ("ddim", 50, False, -0.1),
                 ("ddim", 50, False, float("nan"))):
        with pytest.raises(ValueError):
            dfa.sampler_schedule(*args)


def test_c_entries_reject_bad_arguments_without_a_launch():
    lib = nat.lib()
    one = 16  # a non-null address: never dereferenced, the checks return first
    # ddpm_sample_init(x, model_in, t_model, cursor, timesteps, B, per_row, S, cfg, seed, dtype, stream)
    args = [one, one, one, one, one, 2, 16, 4, 1, 7, 1, None]
    assert len(args) == len(nat.SIGNATURES["ddpm_sample_init"][1])
    for i in range(5):
        bad = list(args)
        bad[i] = None
        assert lib.ddpm_sample_init(*bad) == -1, i
    for i, v in ((5, 0), (5, -1), (6, 0), (7, 0), (7, -2), (10, 3), (10, -1)):  # B, per_row, S < 1; dtype
        bad = list(args)
        bad[i] = v
        assert lib.ddpm_sample_init(*bad) == -1, (i, v)
    # ddpm_sample_step(x, model_out, model_in, t_model, cursor, timesteps, coef, z_out, B, per_row, S, cfg, guidance, dtype, stream)
    args = [one, one, one, one, one, one, one, None, 2, 16, 4, 1, 5.0, 2, None]
    assert len(args) == len(nat.SIGNATURES["ddpm_sample_step"][1])
    for i in range(7):
        bad = list(args)
        bad[i] = None
        assert lib.ddpm_sample_step(*bad) == -1, i
    for i, v in ((8, 0), (9, 0), (9, -5), (10, 0), (13, 3), (13, -1)):
        bad = list(args)
        bad[i] = v
        assert lib.ddpm_sample_step(*bad) == -1, (i, v)
    # ddpm_sample_advance(cursor, S, stream)
    assert lib.ddpm_sample_advance(None, 4, None) == -1 and lib.ddpm_sample_advance(one, 0, None) == -1


def test_bindings_refuse_host_tensors_and_buffers_that_disagree():
    ts, coef = dfa.sampler_schedule("ddpm", 4, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.SampleState.alloc((2, 4, 8, 8), torch.float16, True, ts, coef, "cpu")
    x, t = torch.zeros(2, 4, 8, 8), torch.zeros(4, dtype=torch.int64)
    cur = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="disagree"):  # guidance wants 2B model-input rows
        nat.SampleState(x, torch.zeros(2, 4, 8, 8), t[:2], cur, ts, coef, True)
    with pytest.raises(ValueError, match="coef fp32"):
        nat.SampleState(x, torch.zeros(4, 4, 8, 8), t, cur, ts, coef[:, :2].contiguous(), True)


class _Unet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(4, 4, 1)


def test_latent_sampler_rejects_bad_arguments():
    unet = _Unet()
    for kw in ({"method": "euler"}, {"num_inference_steps": 0}, {"num_inference_steps": 1001}, {"method": "ddim", "eta": -1.0}):
        with pytest.raises(ValueError):
            dfa.LatentSampler(unet, **kw)
    s = dfa.LatentSampler(unet, num_inference_steps=4)
    assert s.timesteps.tolist() == [750, 500, 250, 0] and s.latents is None and s.step() is False
    ehs = torch.zeros(2, 6, 32)
    with pytest.raises(ValueError, match="does not match"):
        s.begin(ehs, torch.zeros(3, 6, 32), seed=1)
    with pytest.raises(ValueError, match=r"\[B, L, D\]"):
        s.begin(ehs[0], seed=1)
    with pytest.raises(ValueError, match="latent_shape"):
        s.begin(ehs, seed=1, latent_shape=(4, 8))
    with pytest.raises(ValueError, match="seed"):
        s.begin(ehs, seed=None)
    with pytest.raises(TypeError):
        s.begin(ehs)  # the seed is required
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.begin(ehs, seed=1)
    assert unet.training  # untouched by the refused calls
