"""Host side of the training-objective extensions: `step.min_snr_weights` against a float64 formula written here, the trainers'
argument rules for snr_gamma / timestep_weights / noise_offset, the LORA_E_BADARG paths of the three C entries without a launch,
and the routing of step.noise_prologue / step.loss_backward.  (That header, exports and bindings agree is
tests/test_native_abi.py's business.)"""
import math

import numpy as np
import pytest
import torch

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import inversion as inv
from diffusion_finetuning_amd import step as stp
from diffusion_finetuning_amd import trainer as tr
from tests import objective_reference as ref


def test_the_three_entries_are_declared_and_bound():
    names = {"ddpm_mse_weighted_fwd_bwd", "ddpm_noise_prologue_offset", "ddpm_posterior_prologue_offset"}
    assert names <= set(nat.SIGNATURES)
    lib = nat.lib()
    assert all(hasattr(lib, n) for n in names)


@pytest.mark.parametrize("v_prediction", [False, True])
@pytest.mark.parametrize("gamma", [5.0, 1.0, 1e6])
def test_min_snr_weights_against_a_float64_formula(gamma, v_prediction):
    acp = tr.ddpm_alphas_cumprod()
    got = stp.min_snr_weights(acp, gamma, v_prediction)
    assert got.dtype == torch.float32 and got.shape == (1000,) and got.device.type == "cpu"
    want = ref.min_snr(acp, gamma, v_prediction)
    assert torch.equal(got, want.float())  # computed in float64, rounded once
    snr = acp.double() / (1.0 - acp.double())
    if gamma > float(snr.max()):  # γ above the largest SNR: nothing is capped
        assert gamma == 1e6
        if v_prediction:
            assert torch.equal(got, (snr / (snr + 1.0)).float())
        else:
            assert bool((got == 1.0).all())
    else:
        assert float(got.min()) < 1.0 and float(got.max()) <= 1.0
        capped = snr > gamma
        assert bool(capped.any()) and bool((~capped).any())
        if not v_prediction:
            assert bool((got[~capped] == 1.0).all()) and bool((got[capped] < 1.0).all())


def test_min_snr_weights_at_zero_and_full_snr_and_refused_arguments():
    acp = torch.tensor([1.0, 0.75, 0.5, 0.0])  # SNR = inf, 3, 1, 0 (zero-terminal-SNR schedule)
    eps_w = stp.min_snr_weights(acp, 2.0, False)
    assert eps_w.tolist() == [0.0, np.float32(2.0 / 3.0), 1.0, 1.0]  # SNR == 0: the limit 1, not 0/0
    v_w = stp.min_snr_weights(acp, 2.0, True)
    assert v_w.tolist() == [0.0, 0.5, 0.5, 0.0]
    assert bool(torch.isfinite(eps_w).all()) and bool(torch.isfinite(v_w).all())
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="snr_gamma"):
            stp.min_snr_weights(acp, bad)
    with pytest.raises(ValueError, match="alphas_cumprod"):
        stp.min_snr_weights(torch.tensor([0.5, 1.5]), 5.0)


def _constructors():
    from tests.test_inversion_host import _tiny_models

    unet, te = _tiny_models()
    return [lambda **kw: tr.LoraTrainer(unet, **kw), lambda **kw: inv.InversionTrainer(unet, te, [3], **kw)]


def test_trainers_refuse_inconsistent_objective_arguments():
    """All of it is checked on the host before anything is built: no device is needed to be told."""
    ones = torch.ones(1000)
    for make in _constructors():
        with pytest.raises(ValueError, match="mutually exclusive"):
            make(snr_gamma=5.0, timestep_weights=ones)
        with pytest.raises(ValueError, match="999 entries, the schedule has 1000"):
            make(timestep_weights=torch.ones(999))
        for bad in (-ones, torch.full((1000,), float("nan")), torch.cat([ones[:999], torch.tensor([float("inf")])])):
            with pytest.raises(ValueError, match="finite and non-negative"):
                make(timestep_weights=bad)
        for bad in (ones.double(), ones.reshape(10, 100), [1.0] * 1000):
            with pytest.raises(ValueError, match=r"fp32 \[T\] tensor"):
                make(timestep_weights=bad)
        for bad in (0.0, -2.0, float("nan")):
            with pytest.raises(ValueError, match="snr_gamma must be a finite positive"):
                make(snr_gamma=bad)
        with pytest.raises(ValueError, match="noise_offset must be finite"):
            make(noise_offset=float("inf"))
    # well-formed arguments pass these checks: the constructors go on to what they need next
    with pytest.raises(ValueError, match="No lora injected"):
        _constructors()[0](snr_gamma=5.0, noise_offset=0.1)
    with pytest.raises(RuntimeError, match="must be on the HIP device"):
        _constructors()[1](timestep_weights=ones, noise_offset=0.1)


def test_noise_offset_with_the_callers_noise_is_refused_by_both_trainers():
    lat = noise = torch.zeros(2, 4, 8, 8)
    ts, ehs, ids = torch.zeros(2, dtype=torch.int64), torch.zeros(2, 6, 32), torch.zeros(2, 5, dtype=torch.int64)
    lora = tr.LoraTrainer.__new__(tr.LoraTrainer)  # step()'s argument checks alone (no device)
    lora.text_encoder, lora.token_table, lora.noise_offset = None, None, 0.1
    fake_inv = inv.InversionTrainer.__new__(inv.InversionTrainer)
    fake_inv.module, fake_inv.noise_offset = object(), 0.1
    for call in (lambda **kw: lora.step(encoder_hidden_states=ehs, **kw), lambda **kw: fake_inv.step(input_ids=ids, **kw)):
        with pytest.raises(ValueError, match="add the offset to it yourself"):
            call(latents=lat, noise=noise, timesteps=ts)
    stp.check_noise_offset(0.0, noise)  # no offset: the caller's noise is fine
    stp.check_noise_offset(0.1, None)  # device draw: the offset is the kernel's


def test_c_entries_reject_bad_arguments_without_a_launch():
    lib = nat.lib()
    one = 16  # a non-null address: never dereferenced, the checks return first
    # ddpm_mse_weighted_fwd_bwd(pred, target, mask, t, weights, n_weights, n_inst, n_prior, per_row, hw, prior_weight,
    #                           grad_scale, loss_out, dpred, workspace, dtype, stream)
    args = [one, one, None, one, one, 1000, 2, 0, 64, 16, 1.0, 1.0, one, None, one, 0, None]
    for i in (0, 1, 3, 4, 12, 14):  # null pred / target / t / weights / loss_out / workspace
        bad = list(args)
        bad[i] = None
        assert lib.ddpm_mse_weighted_fwd_bwd(*bad) == -1, i
    for i, v in ((5, 0), (5, -1), (6, 0), (7, -1), (8, 0), (9, 0), (9, 5)):  # n_weights, n_inst, n_prior, per_row, hw; per_row % hw
        bad = list(args)
        bad[i] = v
        assert lib.ddpm_mse_weighted_fwd_bwd(*bad) == -1, (i, v)
    # ddpm_noise_prologue_offset(x0, sqrt_acp, sqrt_1macp, noisy, target, eps_out, t_out, B, per_row, n_timesteps, seed, step,
    #                            v_prediction, dtype, hw, noise_offset, xi_out, stream)
    args = [one, one, one, one, None, None, None, 2, 64, 1000, 1, 2, 0, 0, 16, 0.1, None, None]
    for i in (0, 1, 2, 3):
        bad = list(args)
        bad[i] = None
        assert lib.ddpm_noise_prologue_offset(*bad) == -1, i
    for i, v in ((7, 0), (8, 0), (9, 0), (13, 3), (14, 0), (14, 5), (14, -16), (15, float("nan")), (15, float("inf"))):
        bad = list(args)  # B, per_row, T < 1; dtype; hw < 1, per_row % hw != 0; a non-finite offset
        bad[i] = v
        assert lib.ddpm_noise_prologue_offset(*bad) == -1, (i, v)
    # ddpm_posterior_prologue_offset(moments, moments_dtype, sqrt_acp, sqrt_1macp, noisy, target, x0_out, z_out, eps_out, t_out,
    #                                B, per_row, n_timesteps, scale, seed, step, v_prediction, dtype, hw, noise_offset, xi_out, stream)
    args = [one, 0, one, one, one, None, None, None, None, None, 2, 64, 1000, 0.18215, 1, 2, 0, 0, 16, 0.1, None, None]
    for i in (0, 2, 3, 4):
        bad = list(args)
        bad[i] = None
        assert lib.ddpm_posterior_prologue_offset(*bad) == -1, i
    for i, v in ((10, 0), (11, 0), (12, 0), (1, 3), (17, 7), (18, 0), (18, 5), (19, float("nan"))):
        bad = list(args)
        bad[i] = v
        assert lib.ddpm_posterior_prologue_offset(*bad) == -1, (i, v)


def test_bindings_refuse_host_tensors_and_malformed_tables():
    sa = torch.ones(1000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.ddpm_noise_prologue_offset(torch.zeros(2, 4, 4, 4), sa, sa, torch.float32, 1, 0, False, noise_offset=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.ddpm_posterior_prologue_offset(torch.zeros(2, 8, 4, 4), sa, sa, torch.float32, 1, 0, False, noise_offset=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.ddpm_mse_weighted_fwd_bwd(torch.zeros(2, 4, 4, 4), torch.zeros(2, 4, 4, 4), None, torch.zeros(2, dtype=torch.int64),
                                      sa, 2, 0, 1.0, 1.0)
    with pytest.raises(ValueError, match=r"\[B, C, h, w\]"):
        nat._channel_plane((2, 64))
    assert nat._channel_plane((3, 4, 5, 7)) == 35


def test_noising_defaults_and_the_routing_of_prologue_and_loss(monkeypatch):
    """Knobs off: the plain entries get the arguments they always got.  Knobs on: the `_offset` / weighted entries, with the
    offset and the table; the caller's noise never reaches an `_offset` entry."""
    nz = stp.Noising(torch.ones(4), torch.zeros(4), torch.float16, True, 1000)
    assert nz.noise_offset == 0.0 and nz.loss_weights is None and nz.scale == 0.18215
    calls = []

    def spy(name, result):
        def f(*a, **kw):
            calls.append((name, a, kw))
            return result
        return f

    for name in ("ddpm_noise_prologue", "ddpm_posterior_prologue", "ddpm_noise_prologue_offset",
                 "ddpm_posterior_prologue_offset"):
        monkeypatch.setattr(nat, name, spy(name, ("noisy", "target", "t")))
    monkeypatch.setattr(nat, "ddpm_add_noise", spy("ddpm_add_noise", ("noisy", "target")))
    lat, m = torch.zeros(2, 4, 3, 3), torch.zeros(2, 8, 3, 3)
    off = nz._replace(noise_offset=0.25)
    stp.noise_prologue(nz, lat, None, None, 7, 3)
    stp.noise_prologue(nz, None, None, None, 7, 3, moments=m)
    stp.noise_prologue(off, lat, None, None, 7, 3)
    stp.noise_prologue(off, None, None, None, 7, 3, moments=m)
    stp.noise_prologue(off, lat, lat, torch.zeros(2, dtype=torch.int64), None, 3)
    assert [c[0] for c in calls] == ["ddpm_noise_prologue", "ddpm_posterior_prologue", "ddpm_noise_prologue_offset",
                                     "ddpm_posterior_prologue_offset", "ddpm_add_noise"]
    assert calls[0][1][3:] == (torch.float16, 7, 3, True, 1000) and calls[1][1][3:] == (torch.float16, 7, 3, True, 1000, 0.18215)
    assert calls[2][1][3:] == (torch.float16, 7, 3, True, 1000, 0.25)
    assert calls[3][1][3:] == (torch.float16, 7, 3, True, 1000, 0.18215, 0.25)

    del calls[:]

    class Pred:
        shape = (2, 4, 3, 3)

        def is_contiguous(self):
            return True

        def backward(self, g):
            calls.append(("backward", g))

    monkeypatch.setattr(nat, "ddpm_mse_fwd_bwd", spy("plain", ("loss", "dpred")))
    monkeypatch.setattr(nat, "ddpm_mse_weighted_fwd_bwd", spy("weighted", ("wloss", "wdpred")))
    pred, ts, table = Pred(), torch.tensor([1, 2]), torch.ones(5)
    assert stp.loss_backward(pred, "target", None, 2, 0, 1.0, 8.0, ts, None) == "loss"
    assert stp.loss_backward(pred, "target", None, 2, 0, 1.0, 8.0) == "loss"
    assert stp.loss_backward(pred, "target", None, 1, 1, 0.5, 8.0, ts, table) == "wloss"
    assert [c[0] for c in calls] == ["plain", "backward", "plain", "backward", "weighted", "backward"]
    assert calls[0][1] == (pred, "target", None, 2, 0, 1.0, 8.0) and calls[5][1] == "wdpred"
    assert calls[4][1][:5] == (pred, "target", None, ts, table) and calls[4][1][5:] == (1, 1, 0.5, 8.0)


def test_config_and_identity_helpers():
    w = torch.linspace(0, 1, 1000)
    assert stp.table_digest(None) is None and stp.table_identity(None) is None
    d = stp.table_digest(w)
    assert isinstance(d, str) and len(d) == 16 and d == stp.table_digest(w.clone()) and d != stp.table_digest(w * 2)
    cfg = stp.objective_config(5.0, None, 0.1)
    assert cfg == {"snr_gamma": 5.0, "timestep_weights": None, "noise_offset": 0.1}
    with pytest.warns(UserWarning, match="snr_gamma: checkpoint 5.0, trainer 1.0"):
        stp.warn_config_differences("T", cfg, stp.objective_config(1.0, None, 0.1))
    before = stp.table_identity(w)
    w.mul_(2)
    assert stp.table_identity(w) != before  # an in-place edit of the table asks for a new recording
    assert stp.objective_table(None, None, None, False, "cpu") is None
    own = stp.objective_table(None, w, None, False, "cpu")
    assert torch.equal(own, w) and own.data_ptr() != w.data_ptr()  # the trainer's copy: the caller's tensor is left alone
    assert math.isclose(float(stp.objective_table(5.0, None, tr.ddpm_alphas_cumprod(), False, "cpu")[0]),
                        5.0 / float(tr.ddpm_alphas_cumprod()[0].double() / (1 - tr.ddpm_alphas_cumprod()[0].double())), rel_tol=1e-6)
