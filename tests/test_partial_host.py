"""Host side of image-to-image sampling: `multistep_schedule(first_step=k)` against the stateful float64 solvers started fresh
on grid[k:] (tests/partial_reference.py) over whole runs, the tail placement's plan invariants, the strength → (n, k0) mapping,
the keep-mask table against float64, every refusal of `LatentSampler.begin` before anything is written, and LORA_E_BADARG of the
three new entries without a launch."""
import math

import pytest
import torch

import diffusion_finetuning_amd as dfa
import lora_diffusion
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import sampling
from tests import multistep_reference as mr
from tests import partial_reference as ref
from tests import sampling_reference as sr

METHODS = ("plms", "dpmpp_2m")
STEPS = (2, 3, 7, 20)


def test_public_names():
    for name in ("partial_start", "keep_schedule"):
        assert getattr(dfa, name) is getattr(sampling, name) is getattr(lora_diffusion, name)
    for name in ("ddpm_sample_init_from", "ddpm_sample_step_keep", "ddpm_sample_multistep_keep"):
        assert name in nat.SIGNATURES and callable(getattr(nat, name))
    for prop in ("run_evaluations", "run_timesteps"):
        assert isinstance(getattr(dfa.LatentSampler, prop), property)


@pytest.mark.parametrize("v_prediction", [False, True])
@pytest.mark.parametrize("S", STEPS)
@pytest.mark.parametrize("method", METHODS)
def test_first_step_tables_reproduce_a_fresh_solver_on_the_sub_grid(method, S, v_prediction):
    """Every first step k of the grid, n = S − k = 1 and 2 included; judged as tests/test_multistep_host.py judges the full
    run: each iteration from the reference's own previous state and history, 1e-6 of Σ|terms| for the fp32 rounding of the
    coefficients."""
    for k in range(S):
        n = S - k
        ts, coef, plan = dfa.multistep_schedule(method, S, v_prediction, first_step=k)
        n_it = n + 1 if method == "plms" and n >= 2 else n
        assert tuple(ts.shape) == (n_it,) and tuple(coef.shape) == (n_it, 7) and tuple(plan.shape) == (n_it, 5)
        solver = ref.fresh_solver(method, S, v_prediction, k)
        assert ts.tolist() == solver.timesteps == ref.run_timesteps(method, S, k)
        g = torch.Generator().manual_seed(S * 101 + k * 2 + int(v_prediction))
        x = torch.randn(64, generator=g, dtype=torch.float64)
        xs, ring, worst = None, {}, 0.0
        for i in range(n_it):
            o = torch.randn(64, generator=g, dtype=torch.float64)
            got, _, terms = mr.apply_tables(coef[i].double(), plan[i], x, o, xs, ring)  # (a slot never pushed: KeyError)
            want = solver.step(x, o)
            worst = max(worst, float(((got - want).abs() / terms).max()))
            flags = int(plan[i, 4])
            if flags & mr.SAVE:
                xs = x
            if flags & mr.PUSH:
                ring[int(plan[i, 0])] = solver.history[-1]
            x = want
        assert worst <= 1e-6, (k, worst)
        # the order of every iteration: dpmpp_2m's first is first order, its last when the FULL S is below 15
        order = [int((coef[i, 3:] != 0).sum()) for i in range(n_it)]
        if method == "dpmpp_2m":
            assert order == ([1] + [2] * (n - 2) + ([1] if S < 15 else [2]) * (n > 1))
        else:
            assert order == ([1, 2] + [min(j + 1, 4) for j in range(1, n)] if n >= 2 else [1])


@pytest.mark.parametrize("S", STEPS + (1, 50))
@pytest.mark.parametrize("method", METHODS)
def test_first_step_zero_is_the_full_run_bit_for_bit(method, S):
    for v in (False, True):
        full = dfa.multistep_schedule(method, S, v)
        zero = dfa.multistep_schedule(method, S, v, first_step=0)
        assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(full, zero))
    for bad in (-1, S, S + 3):
        with pytest.raises(ValueError, match="first_step"):
            dfa.multistep_schedule(method, S, False, first_step=bad)


class _Unet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(4, 4, 1)


@pytest.mark.parametrize("S", STEPS)
@pytest.mark.parametrize("method", METHODS)
def test_tail_placement_keeps_absent_history_at_exactly_zero(method, S):
    """The sampler's full-size tables of a run begun at grid step k0: the sub-run in rows [I − I', I), cursor from I − I'.
    Replaying the pushes FROM THE START ROW, a term whose history does not exist has coefficient exactly 0, every other names
    a slot pushed within the run and still there; USE_SAVED only after a SAVE within the run."""
    sampler = dfa.LatentSampler(_Unet(), num_inference_steps=S, method=method)
    n_full = sampler.num_model_evaluations
    for k0 in range(S):
        row, n_it, ts, coef, plan = sampler._run_tables(k0)
        sub = dfa.multistep_schedule(method, S, False, first_step=k0)
        assert n_it == sub[0].shape[0] and row == n_full - n_it and row >= 0
        assert tuple(ts.shape) == (n_full,) and tuple(coef.shape) == (n_full, 7) and tuple(plan.shape) == (n_full, 5)
        assert all(torch.equal(full[row:], part) for full, part in zip((ts, coef, plan), sub))
        run_plan, run_coef = plan[row:], coef[row:]
        for i in range(n_it):
            slots = mr.ring_slots(run_plan, i)  # pushes of the run alone
            before = mr.SOLVERS[method].pushes_before(i)
            for k in (1, 2, 3):
                c = float(run_coef[i, 3 + k])
                if k > before:
                    assert c == 0.0, (k0, i, k)
                if c != 0.0:
                    assert slots[k - 1] is not None and int(run_plan[i, k]) == slots[k - 1], (k0, i, k)
            if int(run_plan[i, 4]) & mr.USE_SAVED:
                assert any(int(f) & mr.SAVE for f in run_plan[:i, 4])
    assert torch.equal(sampler.timesteps, dfa.multistep_schedule(method, S, False)[0])  # the sampler's own tables: untouched


def test_strength_maps_to_steps_run_and_first_step():
    for S, strength, want in ((50, 0.75, (37, 13)), (50, 1.0, (50, 0)), (20, 0.3, (6, 14)), (7, 0.3, (2, 5)), (7, 0.75, (5, 2)),
                              (7, 1.0, (7, 0)), (3, 0.34, (1, 2)), (1, 1.0, (1, 0)), (1000, 0.001, (1, 999))):
        assert dfa.partial_start(S, strength) == want == ref.steps_run(S, strength)
    for S in (1, 2, 7, 20, 50):
        for strength in (0.05, 0.2, 0.3, 0.5, 0.75, 0.99, 1.0):
            want = ref.steps_run(S, strength)
            if want is None:
                with pytest.raises(ValueError, match=rf"num_inference_steps = {S} at strength = {strength}"):
                    dfa.partial_start(S, strength)
            else:
                assert dfa.partial_start(S, strength) == want
    for bad in (0.0, -0.5, 1.0001, 2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="strength"):
            dfa.partial_start(50, bad)


@pytest.mark.parametrize("method,S", [("ddpm", 7), ("ddim", 20), ("plms", 7), ("plms", 2), ("dpmpp_2m", 20), ("ddpm", 1)])
def test_keep_schedule_against_float64(method, S):
    for k0 in range(S):
        ts = ref.run_timesteps(method, S, k0)
        table = dfa.keep_schedule(torch.tensor(ts))
        assert table.dtype == torch.float32 and tuple(table.shape) == (len(ts), 2)
        want = torch.tensor(ref.keep_pairs(ts), dtype=torch.float64)
        assert torch.equal(table, want.float())  # float64 rounded once
        assert table[-1].tolist() == [1.0, 0.0]
        sq = table.double() ** 2
        assert float((sq.sum(dim=1) - 1).abs().max()) <= 4e-7  # k² + n² = 1 to two fp32 roundings


def test_begin_refuses_bad_image_to_image_arguments_before_writing_anything():
    unet = _Unet()
    s = dfa.LatentSampler(unet, num_inference_steps=4)
    ehs, init = torch.zeros(2, 6, 32), torch.zeros(2, 4, 8, 8)
    mask = torch.ones(2, 1, 8, 8)
    refusals = [
        (dict(init_latents=init), "strength"),  # required with init
        (dict(strength=0.5), "init_latents"),
        (dict(keep_mask=mask), "init_latents"),  # a mask without init
        (dict(keep_mask=mask, strength=1.0), "init_latents"),
        (dict(init_latents=init, strength=0.0), "strength"),
        (dict(init_latents=init, strength=-0.1), "strength"),
        (dict(init_latents=init, strength=1.5), "strength"),
        (dict(init_latents=init, strength=float("nan")), "strength"),
        (dict(init_latents=init, strength=float("inf")), "strength"),
        (dict(init_latents=init, strength=0.2), "num_inference_steps = 4"),  # n == 0
        (dict(init_latents=init[:1], strength=0.5), "init_latents"),  # batch
        (dict(init_latents=init[0], strength=0.5), "init_latents"),  # rank
        (dict(init_latents=init.double(), strength=0.5), "init_latents"),  # dtype
        (dict(init_latents=init.half(), strength=0.5), "init_latents"),  # (the compute dtype here is fp32)
        (dict(init_latents=init, strength=0.5, keep_mask=mask[:1]), "keep_mask"),
        (dict(init_latents=init, strength=0.5, keep_mask=torch.ones(2, 4, 8, 8)), "keep_mask"),
        (dict(init_latents=init, strength=0.5, keep_mask=torch.ones(2, 1, 8, 4)), "keep_mask"),
        (dict(init_latents=init, strength=0.5, keep_mask=mask.half()), "keep_mask"),
        (dict(init_latents=init, strength=0.5, keep_mask=mask.bool()), "keep_mask"),
    ]
    for kw, match in refusals:
        with pytest.raises(ValueError, match=match):
            s.begin(ehs, seed=1, **kw)
        with pytest.raises(ValueError, match=match):
            s.sample(ehs, seed=1, **kw)
    assert s.state is None and s.latents is None and s.step() is False and s.run_evaluations == 4 and unet.training
    assert s.run_timesteps.tolist() == s.timesteps.tolist()
    # host tensors are refused as elsewhere — behind every ValueError
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.begin(ehs, seed=1, init_latents=init, strength=0.5, keep_mask=mask)
    assert s.state is None


def test_state_buffers_refuse_what_does_not_fit():
    ts, coef = dfa.sampler_schedule("ddpm", 4, False)
    x, t, cur, m_in = torch.zeros(2, 4, 8, 8), torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(4, 4, 8, 8)
    mask, kc = torch.zeros(2, 1, 8, 8), torch.zeros(4, 2)
    with pytest.raises(ValueError, match="init"):
        nat.SampleState(x, m_in, t, cur, ts, coef, True, init=torch.zeros(2, 4, 8, 4))
    with pytest.raises(ValueError, match="init"):
        nat.SampleState(x, m_in, t, cur, ts, coef, True, init=x.half())
    with pytest.raises(ValueError, match="needs init"):
        nat.SampleState(x, m_in, t, cur, ts, coef, True, mask=mask, keep_coef=kc)
    with pytest.raises(ValueError, match="needs init"):
        nat.SampleState(x, m_in, t, cur, ts, coef, True, init=x.clone(), mask=mask)
    with pytest.raises(ValueError, match="mask"):
        nat.SampleState(x, m_in, t, cur, ts, coef, True, init=x.clone(), mask=torch.zeros(2, 1, 8, 5), keep_coef=kc)
    with pytest.raises(ValueError, match="mask"):
        nat.SampleState(x, m_in, t, cur, ts, coef, True, init=x.clone(), mask=torch.zeros(3, 1, 8, 8), keep_coef=kc)
    with pytest.raises(ValueError, match="keep_coef"):
        nat.SampleState(x, m_in, t, cur, ts, coef, True, init=x.clone(), mask=mask, keep_coef=torch.zeros(3, 2))
    with pytest.raises(ValueError, match="needs init"):
        nat.SampleState.alloc((2, 4, 8, 8), torch.float16, True, ts, coef, "cpu", with_mask=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.SampleState.alloc((2, 4, 8, 8), torch.float16, True, ts, coef, "cpu", with_init=True, with_mask=True)


def test_c_entries_reject_bad_arguments_without_a_launch():
    lib = nat.lib()
    one = 16  # a non-null address: never dereferenced, the checks return first
    # ddpm_sample_init_from(x, model_in, t_model, cursor, timesteps, init, eps_out, B, per_row, S, start, k, n, cfg, seed, dtype,
    #                       stream)
    args = [one] * 7 + [2, 16, 4, 1, 0.5, 0.5, 1, 7, 1, None]
    assert len(args) == len(nat.SIGNATURES["ddpm_sample_init_from"][1])
    for i in range(6):  # (eps_out, argument 6, is optional)
        bad = list(args)
        bad[i] = None
        assert lib.ddpm_sample_init_from(*bad) == -1, i
    for i, v in ((7, 0), (7, -1), (8, 0), (8, -5), (9, 0), (9, -2), (10, -1), (10, 4), (10, 9), (15, 3), (15, -1)):
        bad = list(args)  # B, per_row, S < 1; start outside [0, S); dtype
        bad[i] = v
        assert lib.ddpm_sample_init_from(*bad) == -1, (i, v)
    # ddpm_sample_step_keep(x, model_out, model_in, t_model, cursor, timesteps, coef, z_out, mask, init, keep_coef, B, per_row,
    #                       hw, S, cfg, guidance, dtype, stream)
    args = [one] * 11 + [2, 16, 4, 4, 1, 5.0, 1, None]
    assert len(args) == len(nat.SIGNATURES["ddpm_sample_step_keep"][1])
    for i in (0, 1, 2, 3, 4, 5, 6, 8, 9, 10):  # (z_out, argument 7, is optional)
        bad = list(args)
        bad[i] = None
        assert lib.ddpm_sample_step_keep(*bad) == -1, i
    for i, v in ((11, 0), (11, -1), (12, 0), (12, -4), (13, 0), (13, -4), (13, 3), (13, 32), (14, 0), (14, -2), (17, 3), (17, -1)):
        bad = list(args)  # B, per_row, hw < 1; per_row % hw != 0; S < 1; dtype
        bad[i] = v
        assert lib.ddpm_sample_step_keep(*bad) == -1, (i, v)
    # ddpm_sample_multistep_keep(x, xs, hist, model_out, model_in, t_model, cursor, timesteps, coef, plan, mask, init, keep_coef,
    #                            B, per_row, hw, I, cfg, guidance, dtype, stream)
    args = [one] * 13 + [2, 16, 4, 4, 1, 5.0, 1, None]
    assert len(args) == len(nat.SIGNATURES["ddpm_sample_multistep_keep"][1])
    for i in range(13):
        bad = list(args)
        bad[i] = None
        assert lib.ddpm_sample_multistep_keep(*bad) == -1, i
    for i, v in ((13, 0), (13, -1), (14, 0), (14, -4), (15, 0), (15, -4), (15, 3), (15, 32), (16, 0), (16, -2), (19, 3), (19, -1)):
        bad = list(args)
        bad[i] = v
        assert lib.ddpm_sample_multistep_keep(*bad) == -1, (i, v)
    assert math.isfinite(lib.lora_version())  # (the library is still there: nothing was launched)
