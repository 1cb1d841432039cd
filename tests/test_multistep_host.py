"""Host side of the multistep sampling methods: `multistep_schedule`'s collapsed tables against the stateful float64 PLMS and
DPM-Solver++(2M) of tests/multistep_reference.py over whole runs, a cross-check of both against the DDIM schedule the project
already pins, the invariants of the ring's plan, and argument validation without a launch."""
import pytest
import torch

import diffusion_finetuning_amd as dfa
import lora_diffusion
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import sampling
from tests import multistep_reference as ref
from tests import sampling_reference as sr

METHODS = ("plms", "dpmpp_2m")
STEPS = (1, 2, 3, 4, 5, 20, 50)


def test_public_names():
    assert dfa.multistep_schedule is sampling.multistep_schedule is lora_diffusion.multistep_schedule
    assert "ddpm_sample_multistep" in nat.SIGNATURES and issubclass(nat.MultistepState, nat.SampleState)
    assert (sampling.PUSH, sampling.SAVE, sampling.USE_SAVED) == (ref.PUSH, ref.SAVE, ref.USE_SAVED)


@pytest.mark.parametrize("v_prediction", [False, True])
@pytest.mark.parametrize("S", STEPS)
@pytest.mark.parametrize("method", METHODS)
def test_tables_reproduce_the_stateful_reference_over_a_whole_run(method, S, v_prediction):
    """Every iteration is judged from the reference's own previous state, saved sample and history: the ring is filled with
    what the reference appended to its list, so no error is carried.  (p, q, a, c_k) are single fp32 roundings of float64
    values, 6e-8 each, on terms no larger than their absolute sum: 1e-6 of that sum, element by element."""
    ts, coef, plan = dfa.multistep_schedule(method, S, v_prediction)
    n_it = ref.evaluations(method, S)
    assert ts.dtype == torch.int64 and tuple(ts.shape) == (n_it,)
    assert coef.dtype == torch.float32 and tuple(coef.shape) == (n_it, 7)
    assert plan.dtype == torch.int32 and tuple(plan.shape) == (n_it, 5)
    solver = ref.SOLVERS[method](S, v_prediction)
    assert ts.tolist() == solver.timesteps
    g = torch.Generator().manual_seed(S * 11 + int(v_prediction))
    x = torch.randn(64, generator=g, dtype=torch.float64)
    xs, ring, worst = None, {}, 0.0
    for i in range(n_it):
        o = torch.randn(64, generator=g, dtype=torch.float64)
        got, _, terms = ref.apply_tables(coef[i].double(), plan[i], x, o, xs, ring)
        want = solver.step(x, o)
        worst = max(worst, float(((got - want).abs() / terms).max()))
        flags = int(plan[i, 4])
        if flags & ref.SAVE:
            xs = x
            assert torch.equal(solver.cur_sample, x)
        if method == "plms":  # the plan pushes exactly the outputs the reference keeps
            assert bool(flags & ref.PUSH) == (solver.history[-1] is o)
        if flags & ref.PUSH:
            ring[int(plan[i, 0])] = solver.history[-1]  # the reference's own entry: o for plms, its x0 for dpmpp_2m
        x = want
    assert worst <= 1e-6, worst


@pytest.mark.parametrize("S", STEPS)
@pytest.mark.parametrize("method", METHODS)
def test_constant_prediction_ends_where_ddim_ends(method, S):
    """Independent of the restated solvers: φ is algebraically DDIM's η = 0 step and every Adams–Bashforth weight set sums to
    1, so plms with a constant output e ends where `sampler_schedule("ddim", S, η = 0)` ends on the same grid; dpmpp_2m's
    step with a constant data prediction is DDIM's too (σ_t/σ_s·x + α_t(1 − e^{−h})·x0 with ε = (x − α_s·x0)/σ_s).  Float64
    on both sides: the unrounded multistep coefficients against the DDIM recurrence written out here."""
    ts, coef, plan = dfa.multistep_schedule(method, S, False, coef_dtype=torch.float64)
    assert coef.dtype == torch.float64
    ddim_ts, _ = dfa.sampler_schedule("ddim", S, False, 0.0)
    assert sorted(set(ts.tolist()), reverse=True) == ddim_ts.tolist()
    acp, ratio = sr.alphas_cumprod(), 1000 // S
    g = torch.Generator().manual_seed(S)
    x_T, const = (torch.randn(32, generator=g, dtype=torch.float64) for _ in range(2))
    # DDIM, η = 0, float64, with a constant ε (plms) or a constant x0 (dpmpp_2m)
    want = x_T.clone()
    for t in ddim_ts.tolist():
        ab_t, ab_p = acp[t], acp[t - ratio] if t - ratio >= 0 else acp[0]
        if method == "plms":
            x0, eps = (want - (1 - ab_t).sqrt() * const) / ab_t.sqrt(), const
        else:
            x0, eps = const, (want - ab_t.sqrt() * const) / (1 - ab_t).sqrt()
        want = ab_p.sqrt() * x0 + (1 - ab_p).sqrt() * eps
    # the tables, with history that is the constant
    x, xs = x_T.clone(), None
    for i in range(ts.shape[0]):
        p, q, a, c0, c1, c2, c3 = (float(c) for c in coef[i])
        flags = int(plan[i, 4])
        base = xs if flags & ref.USE_SAVED else x
        if flags & ref.SAVE:
            xs = x
        x = a * base + (c0 + c1 + c2 + c3) * const  # (h = the constant: o for plms, p·x + q·o = x0 for dpmpp_2m)
    assert float((x - want).abs().max()) <= 1e-9 * float(want.abs().max())
    # the same through the DDIM schedule the project's own tests pin (fp32 coefficients: to their rounding) — plms only, whose
    # constant is the model output itself
    if method == "plms":
        _, ddim_coef = dfa.sampler_schedule("ddim", S, False, 0.0)
        y = x_T.clone()
        for a, b, _ in ddim_coef.double().tolist():
            y = a * y + b * const
        # (2·S roundings of 6e-8, each carried to the end by a product of a's no larger than √(ᾱ_0/ᾱ_T) < 15)
        assert float((x - y).abs().max()) <= 2 * S * 6e-8 * 15 * float(want.abs().max())


@pytest.mark.parametrize("v_prediction", [False, True])
@pytest.mark.parametrize("S", STEPS + (6, 9, 1000))
@pytest.mark.parametrize("method", METHODS)
def test_plan_invariants(method, S, v_prediction):
    ts, coef, plan = dfa.multistep_schedule(method, S, v_prediction)
    n_it = ts.shape[0]
    assert n_it == (S + 1 if method == "plms" and S >= 2 else S)
    assert bool(torch.isfinite(coef).all())
    t = ts.tolist()
    assert all(a >= b for a, b in zip(t, t[1:])) and 0 <= min(t) and max(t) < 1000
    repeats = [i for i in range(1, n_it) if t[i] == t[i - 1]]
    assert repeats == ([2] if method == "plms" and S >= 2 else [])
    flags = plan[:, 4].tolist()
    assert all(0 <= f < 8 for f in flags) and bool(((plan[:, :4] >= 0) & (plan[:, :4] < 4)).all())
    if method == "plms":
        assert flags[0] == ref.PUSH | ref.SAVE
        if S >= 2:
            assert flags[1] == ref.USE_SAVED  # the saved state, no push
            assert all(f == ref.PUSH for f in flags[2:])
        assert bool((coef[:, 0] == 0).all()) and bool((coef[:, 1] == 1).all())  # history is the raw guided output
    else:
        assert all(f == ref.PUSH for f in flags)
    pushed_slots = [int(plan[i, 0]) for i in range(n_it) if flags[i] & ref.PUSH]
    assert pushed_slots == [k % 4 for k in range(len(pushed_slots))]  # cycles through all four: S >= 6 wraps
    if S >= 6:
        assert set(pushed_slots) == {0, 1, 2, 3} and len(pushed_slots) > 4
    solver = ref.SOLVERS[method]
    for i in range(n_it):
        slots = ref.ring_slots(plan, i)
        before = solver.pushes_before(i)
        for k in (1, 2, 3):
            c = float(coef[i, 3 + k])
            if k > before:
                assert c == 0.0, (i, k)  # absent history: exactly 0
            if c != 0.0:
                assert slots[k - 1] is not None and int(plan[i, k]) == slots[k - 1], (i, k)  # pushed earlier, still there
        if flags[i] & ref.USE_SAVED:
            assert any(f & ref.SAVE for f in flags[:i])  # saved earlier
        assert float(coef[i, 2]) != 0.0 and (float(coef[i, 3]) != 0.0 or S == 1000)  # (S = T: the last transfer is t = 0 → 0)
    order = [int((coef[i, 3:] != 0).sum()) for i in range(n_it)]
    if method == "plms":
        want = [1, 2] + [min(j + 1, 4) for j in range(1, S)] if S >= 2 else [1]
    else:
        want = [1] + [2] * (S - 2) + ([1] if S < 15 else [2]) * (S > 1)
    keep = n_it - 1 if S == 1000 else n_it  # (S = T: the last transfer, t = 0 → 0, is the identity)
    assert order[:keep] == want[:keep]


def test_schedule_rejects_bad_arguments():
    for args in (("ddpm", 50, False), ("euler", 50, False), ("plms", 0, False), ("plms", 1001, False), ("dpmpp_2m", -1, False)):
        with pytest.raises(ValueError):
            dfa.multistep_schedule(*args)
    with pytest.raises(ValueError):
        dfa.sampler_schedule("plms", 50, False)  # the one-step schedule keeps to its two methods
    with pytest.raises(ValueError):
        dfa.sampler_schedule("dpmpp_2m", 20, False)
    ts, coef, _ = dfa.multistep_schedule("dpmpp_2m", 1000, False)  # no room for the offset: the last step starts at t = 0
    assert int(ts[-1]) == 0 and coef[-1].tolist() == [coef[-1, 0], coef[-1, 1], 1.0, 0.0, 0.0, 0.0, 0.0]


def test_c_entry_rejects_bad_arguments_without_a_launch():
    lib = nat.lib()
    one = 16  # a non-null address: never dereferenced, the checks return first
    # ddpm_sample_multistep(x, xs, hist, model_out, model_in, t_model, cursor, timesteps, coef, plan, B, per_row, I, cfg,
    #                       guidance, dtype, stream)
    args = [one] * 10 + [2, 16, 4, 1, 5.0, 1, None]
    assert len(args) == len(nat.SIGNATURES["ddpm_sample_multistep"][1])
    for i in range(10):
        bad = list(args)
        bad[i] = None
        assert lib.ddpm_sample_multistep(*bad) == -1, i
    for i, v in ((10, 0), (10, -1), (11, 0), (11, -5), (12, 0), (12, -2), (15, 3), (15, -1)):  # B, per_row, I < 1; dtype
        bad = list(args)
        bad[i] = v
        assert lib.ddpm_sample_multistep(*bad) == -1, (i, v)


def test_bindings_refuse_host_tensors_and_buffers_that_disagree():
    ts, coef, plan = dfa.multistep_schedule("plms", 4, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.MultistepState.alloc((2, 4, 8, 8), torch.float16, True, ts, coef, plan, "cpu")
    x, t, cur = torch.zeros(2, 4, 8, 8), torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    hist, m_in = torch.zeros(4, 2, 4, 8, 8), torch.zeros(4, 4, 8, 8)
    with pytest.raises(ValueError, match="disagree"):  # three history slots
        nat.MultistepState(x, x.clone(), hist[:3], m_in, t, cur, ts, coef, plan, True)
    with pytest.raises(ValueError, match="disagree"):  # guidance wants 2B model-input rows
        nat.MultistepState(x, x.clone(), hist, m_in[:2], t[:2], cur, ts, coef, plan, True)
    with pytest.raises(ValueError, match=r"coef fp32 \[I, 7\]"):
        nat.MultistepState(x, x.clone(), hist, m_in, t, cur, ts, coef[:, :3].contiguous(), plan, True)
    with pytest.raises(ValueError, match="plan int32"):
        nat.MultistepState(x, x.clone(), hist, m_in, t, cur, ts, coef, plan.long(), True)
    with pytest.raises(ValueError, match="contiguous"):
        nat.MultistepState(x, x.clone(), hist, m_in, t, cur, ts, coef, plan.t().contiguous().t(), True)


class _Unet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(4, 4, 1)


def test_latent_sampler_takes_the_multistep_methods():
    unet = _Unet()
    for kw in ({"method": "plms", "eta": 0.5}, {"method": "dpmpp_2m", "eta": 1.0}, {"method": "euler"}, {"method": "pndm"},
               {"method": "plms", "num_inference_steps": 0}, {"method": "dpmpp_2m", "num_inference_steps": 1001}):
        with pytest.raises(ValueError):
            dfa.LatentSampler(unet, **kw)
    s = dfa.LatentSampler(unet, num_inference_steps=4, method="plms")
    assert s.num_inference_steps == 4 and s.num_model_evaluations == 5 and s.timesteps.tolist() == [751, 501, 501, 251, 1]
    assert s.latents is None and s.step() is False
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.begin(torch.zeros(2, 6, 32), seed=1)
    d = dfa.LatentSampler(unet, num_inference_steps=20, method="dpmpp_2m")
    assert d.num_model_evaluations == 20 and d.timesteps.tolist() == sr.timesteps("ddim", 20)
    assert dfa.LatentSampler(unet, num_inference_steps=4).num_model_evaluations == 4  # the one-step methods: I = S
    assert unet.training
