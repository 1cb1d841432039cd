"""Host side of the posterior draw (ddpm_posterior_prologue / ddpm_posterior_sample) and of LoraTrainer's gradient accumulation:
argument validation of the two C entries without a launch, the trainers' argument errors, and the independence of the new
Philox stream on the CPU helper.  (That header, exports and bindings agree is tests/test_native_abi.py's business.)"""
import numpy as np
import pytest
import torch

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import inversion as inv
from diffusion_finetuning_amd import step as stp
from diffusion_finetuning_amd import trainer as tr
from tests import posterior_cases as pc


def test_the_two_entries_are_declared_and_bound():
    assert {"ddpm_posterior_prologue", "ddpm_posterior_sample"} <= set(nat.SIGNATURES)
    lib = nat.lib()
    assert hasattr(lib, "ddpm_posterior_prologue") and hasattr(lib, "ddpm_posterior_sample")


def test_c_entries_reject_bad_arguments_without_a_launch():
    lib = nat.lib()
    one = 16  # a non-null address: never dereferenced, the checks return first
    # ddpm_posterior_prologue(moments, moments_dtype, sqrt_acp, sqrt_1macp, noisy, target, x0_out, z_out, eps_out, t_out, B,
    #                         per_row, n_timesteps, scale, seed, step, v_prediction, dtype, stream)
    args = [one, 0, one, one, one, None, None, None, None, None, 2, 16, 1000, 0.18215, 1, 2, 0, 0, None]
    for i in (0, 2, 3, 4):  # null moments / tables / noisy
        bad = list(args)
        bad[i] = None
        assert lib.ddpm_posterior_prologue(*bad) == -1, i
    for i, v in ((10, 0), (10, -3), (11, 0), (12, 0), (1, 3), (1, -1), (17, 3), (17, 7)):  # B, per_row, T < 1; dtypes
        bad = list(args)
        bad[i] = v
        assert lib.ddpm_posterior_prologue(*bad) == -1, (i, v)
    # ddpm_posterior_sample(moments, moments_dtype, z, x0, B, per_row, scale, stream)
    args = [one, 2, one, one, 2, 16, 0.18215, None]
    for i in (0, 2, 3):
        bad = list(args)
        bad[i] = None
        assert lib.ddpm_posterior_sample(*bad) == -1, i
    for i, v in ((4, 0), (5, 0), (1, 3)):
        bad = list(args)
        bad[i] = v
        assert lib.ddpm_posterior_sample(*bad) == -1, (i, v)


def test_bindings_refuse_host_tensors_and_moments_that_are_not_mean_logvar_rows():
    sa = torch.ones(1000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.ddpm_posterior_prologue(torch.zeros(2, 8, 4, 4), sa, sa, torch.float32, 1, 0, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.ddpm_posterior_sample(torch.zeros(2, 8, 4, 4), torch.zeros(2, 4, 4, 4))
    with pytest.raises(ValueError, match=r"contiguous \[B, 2C"):
        nat._moments_rows(torch.zeros(2, 7, 4, 4))
    with pytest.raises(ValueError, match=r"contiguous \[B, 2C"):
        nat._moments_rows(torch.zeros(2, 4, 4, 8).transpose(1, 3))
    assert nat._moments_rows(torch.zeros(3, 8, 5, 6)) == (3, 120, (3, 4, 5, 6))


def _bare_lora_trainer():
    t = tr.LoraTrainer.__new__(tr.LoraTrainer)  # step()'s argument checks alone (no device)
    t.sqrt_acp = t.sqrt_1macp = torch.ones(1000)
    t.dtype, t.v_prediction, t.text_encoder, t.token_table = torch.float32, False, None, None
    return t


def test_trainers_refuse_inconsistent_latents_moments_and_noise():
    lat, m = torch.zeros(2, 4, 8, 8), torch.zeros(2, 8, 8, 8)
    noise, ts, ehs = torch.zeros(2, 4, 8, 8), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 6, 32)
    fake_inv = inv.InversionTrainer.__new__(inv.InversionTrainer)
    fake_inv.module = object()
    ids = torch.zeros(2, 5, dtype=torch.int64)
    calls = [lambda **kw: _bare_lora_trainer().step(encoder_hidden_states=ehs, **kw),
             lambda **kw: fake_inv.step(input_ids=ids, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="exactly one of latents and moments"):
            call(latents=lat, moments=m, seed=1)
        with pytest.raises(ValueError, match="exactly one of latents and moments"):
            call(seed=1)
        with pytest.raises(ValueError, match="or a seed for the on-device draw"):
            call(moments=m)
        with pytest.raises(ValueError, match="posterior_noise as well"):
            call(moments=m, noise=noise, timesteps=ts)
        with pytest.raises(ValueError, match="posterior_noise goes with moments"):
            call(latents=lat, noise=noise, timesteps=ts, posterior_noise=noise)
        with pytest.raises(ValueError, match="posterior_noise goes with moments"):
            call(moments=m, seed=3, posterior_noise=noise)
        with pytest.raises(ValueError, match="both noise and timesteps"):
            call(moments=m, noise=noise, posterior_noise=noise, seed=1)


def test_gradient_accumulation_argument_checks(monkeypatch):
    with pytest.raises(ValueError, match="gradient_accumulation_steps must be >= 1"):
        tr.LoraTrainer(None, gradient_accumulation_steps=0)
    with pytest.raises(ValueError, match="gradient_accumulation_steps must be >= 1"):
        tr.LoraTrainer(None, gradient_accumulation_steps=-2)
    # the script's refusal (train_lora_dreambooth.py:496-507): text encoder trains + accumulation + more than one process
    from tests.test_inversion_host import _tiny_models

    unet, te = _tiny_models()  # the token table trains: that alone makes the text encoder a trained model
    monkeypatch.setattr(tr.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(tr.dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="gradient accumulation is not supported while the text encoder trains"):
        tr.LoraTrainer(unet, te, gradient_accumulation_steps=2)
    # neither of the three alone is refused for that reason (the constructor goes on to look for LoRA layers)
    for kw, world in ((dict(gradient_accumulation_steps=1), 2), (dict(gradient_accumulation_steps=2), 1)):
        monkeypatch.setattr(tr.dist, "get_world_size", lambda group=None, w=world: w)
        with pytest.raises(ValueError, match="No lora injected"):
            tr.LoraTrainer(unet, te, **kw)


def test_the_noise_key_differs_between_the_micro_batches_of_a_window_and_is_the_step_count_without_accumulation():
    class Opt:
        step_count = 0

    t = tr.LoraTrainer.__new__(tr.LoraTrainer)
    t.opt = Opt()
    keys = []
    for n in (1, 4):
        t.accum = n
        for count in range(3):
            t.opt.step_count = count
            for t._micro in range(n):
                keys.append((n, t._noise_key()))
    assert [k for n, k in keys if n == 1] == [0, 1, 2]
    assert [k for n, k in keys if n == 4] == list(range(12))


def test_noising_keeps_its_positional_fields_and_defaults_the_latent_scale():
    nz = stp.Noising(torch.ones(4), torch.zeros(4), torch.float16, True, 1000)
    assert nz.scale == 0.18215 and nz.n_timesteps == 1000 and nz[:5] == (nz.sqrt_acp, nz.sqrt_1macp, torch.float16, True, 1000)


def test_posterior_stream_is_independent_of_the_noise_and_timestep_streams():
    """Equal counters (g, g>>32, ·, 0) and key: the words of stream 2 differ from those of streams 0 and 1 in every group, and
    the helper's stream-0 normals are the oracle's eps — the mapping is the one `step_randomness` applies."""
    from oracle import philox

    n, seed, step = 5 * 1024, 77, 3
    w0, w1, w2 = (np.stack(pc.group_words(n, seed, step, s)) for s in (0, 1, 2))
    assert w2.shape == (4, n // 4)
    assert not (w2 == w0).all(axis=0).any() and not (w2 == w1).all(axis=0).any()
    assert (w2 == w0).mean() < 1e-3 and (w2 == w1).mean() < 1e-3  # single words coincide at the 2^-32 rate only
    eps, _ = philox.step_randomness(5, 1024, 1000, seed, step)
    assert np.array_equal(pc.stream_normals(5, 1024, seed, step, stream=0), eps)
    z = pc.stream_normals(5, 1024, seed, step)
    assert abs(float(z.mean())) < 0.05 and abs(float(z.std()) - 1.0) < 0.05
    assert abs(float(np.corrcoef(z.reshape(-1), eps.reshape(-1))[0, 1])) < 0.05  # 5120 samples: σ of r is 0.014
    # ragged tail: the last group is cut, not padded
    assert np.array_equal(pc.stream_normals(3, 37, seed, step).reshape(-1), pc.stream_normals(1, 112, seed, step).reshape(-1)[:111])


def test_float64_formula_of_the_helper_clamps_like_torch():
    m = torch.zeros(1, 2, 1, 4)
    m[0, 1, 0] = torch.tensor([-40.0, -30.0, 20.0, 25.0])
    z = torch.ones(1, 1, 1, 4)
    x0 = pc.posterior_x0(m, z, scale=1.0).reshape(-1)
    want = torch.tensor([np.exp(-15.0), np.exp(-15.0), np.exp(10.0), np.exp(10.0)], dtype=torch.float64)
    assert torch.allclose(x0, want, rtol=1e-15)
    assert pc.storage_ulp(torch.tensor([1.0, 1.5, 2.0, 1e-30]).double(), torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24]


def test_step_recorder_gives_a_moments_fed_step_buffers_of_its_own(monkeypatch):
    """The recorder's bookkeeping for the two moments-fed modes, the device part and the three native calls stood in for on
    host tensors: caller-drawn — static (moments, posterior noise) next to (noise, timesteps), posterior_sample + add_noise
    inside the recorded body; device-drawn — the draw stays outside and fills (noisy, target, timesteps); a latents-fed step
    keeps the three buffers it always had."""
    from tests.test_trainer_host import _FakeCapture

    calls = []

    def sample(moments, z, scale):
        calls.append("posterior_sample")
        return pc.posterior_x0(moments, z, scale).float()

    def add_noise(x0, eps, t, sa, sb, dtype, v):
        calls.append("add_noise")
        return (x0 + eps).to(dtype), eps.to(dtype)

    def prologue(moments, sa, sb, dtype, seed, step, v, n_timesteps, scale):
        calls.append(("posterior_prologue", seed, step, scale))
        shape = nat._moments_rows(moments)[2]
        return torch.full(shape, 1.0, dtype=dtype), torch.full(shape, 2.0, dtype=dtype), torch.arange(shape[0])

    monkeypatch.setattr(nat, "ddpm_posterior_sample", sample)
    monkeypatch.setattr(nat, "ddpm_add_noise", add_noise)
    monkeypatch.setattr(nat, "ddpm_posterior_prologue", prologue)
    nz = stp.Noising(torch.ones(1000), torch.zeros(1000), torch.bfloat16, False, 1000, 0.5)
    m = torch.randn(2, 8, 3, 3).half()
    pz, noise, ts, ids = torch.randn(2, 4, 3, 3), torch.randn(2, 4, 3, 3), torch.tensor([5, 900]), torch.arange(10).reshape(2, 5)
    class Capture(_FakeCapture):  # the recorder's own `_run` in place of the device part
        def _capture(self, body, before_capture):
            before_capture()
            self.loss = self._run(body)
            return self

    rec = Capture("FakeTrainer", [])
    body = lambda noisy, target, timesteps, cond, mask: noisy.float().sum()
    # caller-drawn
    assert rec.load("k-sampled", "fp", nz, None, noise, ts, None, 0, ids, None, None, m, pz)
    assert rec.inputs[0] is None and torch.equal(rec.inputs[1], noise) and torch.equal(rec.inputs[2], ts)
    assert torch.equal(rec.moments[0], m) and rec.moments[0].dtype == torch.float16 and rec.moments[0] is not m
    assert torch.equal(rec.moments[1], pz) and calls == []
    assert rec.record(body) and calls == ["posterior_sample", "add_noise"]
    want = (pc.posterior_x0(m, pz, 0.5).float() + noise).to(torch.bfloat16).float().sum()
    assert torch.equal(rec.loss, want)
    assert not rec.load("k-sampled", "fp", nz, None, noise + 1, ts, None, 0, ids, None, None, m * 2, pz)  # replayed: copies only
    assert torch.equal(rec.moments[0], m * 2) and torch.equal(rec.inputs[1], noise + 1)
    # device-drawn: another key, the draw outside the recording
    del calls[:]
    assert rec.load("k-drawn", "fp", nz, None, None, None, 7, 12, ids, None, None, m, None)
    assert calls == [("posterior_prologue", 7, 12, 0.5)] and rec.drawn and rec.moments is None
    assert [b.dtype for b in rec.inputs] == [torch.bfloat16, torch.bfloat16, torch.int64] and rec.inputs[0].shape == (2, 4, 3, 3)
    assert rec.record(body) and len(calls) == 1 and float(rec.loss) == 2 * 4 * 9
    # latents-fed after it
    lat = torch.randn(2, 4, 3, 3)
    assert rec.load("k-latents", "fp", nz, lat, noise, ts, None, 0, ids, None, None)
    assert rec.moments is None and len(rec.inputs) == 3 and torch.equal(rec.inputs[0], lat)
