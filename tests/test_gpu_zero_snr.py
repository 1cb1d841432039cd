"""Zero-terminal-SNR sampling and training on an MI355X: LatentSampler on the trailing grid with the rescaled table and the
guidance rescale — step by step against the float64 restatement of tests/zero_snr_reference.py, replayed against host-launched —
and both trainers on the rescaled noise tables.

The step-by-step bound: `state_bound` (tests/sampling_reference.py) of the step itself, plus |b_i| times what the rescale adds
to the guided output the step consumes — 1e-5·max|o'| for k (the kernel's tolerance, tests/test_gpu_cfg_rescale.py) and
(2g − 1)·2⁻²⁴·max|k·out| for the storage rounding of the two scaled halves (half an fp32 ulp each, carried through
u' + g·(c' − u') with weights |1 − g| and g)."""
import gc
import warnings

import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import trainer as tr
from diffusion_finetuning_amd.inversion import InversionTrainer
from tests import zero_snr_reference as zr
from tests.sampling_reference import alphas_cumprod
from tests.test_gpu_checkpoint import _assert_same, _deterministic_stock_kernels, _feed, _lora_trainer, _snap, _steps
from tests.test_gpu_sampling import _conditioning, _harness_unet

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE, S, B, G, PHI = (4, 8, 8), 4, 2, 5.0, 0.7
ZERO = dict(method="ddim", v_prediction=True, timestep_spacing="trailing", zero_terminal_snr=True)


@pytest.fixture(autouse=True)
def _collect_garbage_first():
    """A recording left in a reference cycle by an earlier test must not be destroyed in the middle of another capture."""
    gc.collect()


@pytest.fixture
def repeatable_stock_kernels():
    """tests/test_gpu_checkpoint.py's fixture of the same name: two trainers are compared bit for bit."""
    before = _deterministic_stock_kernels()
    yield
    _deterministic_stock_kernels(False, before)


class _Out:
    def __init__(self, sample):
        self.sample = sample


class GainDenoiser(torch.nn.Module):
    """out = (w + 0.3·mean(context))·x + c[t], fp32: the conditional output minus the unconditional one is a multiple of x, so
    it varies over the row and guidance changes the row's standard deviation (a context-dependent OFFSET would give k ≡ 1)."""

    def __init__(self, w=0.9):
        super().__init__()
        self.w = torch.nn.Parameter(torch.full((1, 1, 1, 1), float(w)), requires_grad=False)  # (4-d: names the compute dtype)
        self.register_buffer("c", torch.linspace(-0.5, 0.5, 1000))

    def forward(self, x, t, ctx):
        return _Out((self.w + 0.3 * ctx.mean(dim=(1, 2)).view(-1, 1, 1, 1)) * x + self.c[t].view(-1, 1, 1, 1))


def _gain_conditioning():
    gen = torch.Generator().manual_seed(3)
    return (torch.randn(B, 6, 32, generator=gen) + 0.5).to(DEV), (torch.randn(B, 6, 32, generator=gen) - 0.5).to(DEV)


@pytest.mark.parametrize("capture", [True, False])
def test_trailing_zero_snr_rescaled_run_step_by_step(capture):
    """After each step the expected state follows from the sampler's PREVIOUS state by the test's own forward of the same model
    on the same input, the rescale, guidance and the uncollapsed update in float64: nothing is compared across a model call."""
    model = GainDenoiser().to(DEV)
    cond, neg = _gain_conditioning()
    sampler = dfa.LatentSampler(model, num_inference_steps=S, guidance_scale=G, guidance_rescale=PHI, capture_graph=capture, **ZERO)
    sampler.begin(cond, neg, seed=5, latent_shape=SHAPE)
    assert sampler.replaying == capture
    acp = zr.rescaled_alphas_cumprod(alphas_cumprod())
    grid = zr.trailing_grid(S)
    assert grid == [999, 749, 499, 249] and sampler.timesteps.tolist() == grid
    st = sampler.state
    assert st.t_model.cpu().tolist() == [999] * (2 * B)  # the first forward runs at T − 1
    ks = []
    for i in range(S):
        x_prev, in_prev, t_prev = st.x.cpu().double(), st.model_in.clone(), st.t_model.clone()
        assert t_prev.cpu().tolist() == [grid[i]] * (2 * B)
        with torch.no_grad():
            out = model(in_prev, t_prev, sampler.conditioning).sample.cpu()
        sampler.step()
        k, scaled = zr.rescale_cfg(out, G, PHI, torch.float32)
        o = zr.guided(scaled, G, True)
        want = zr.step("ddim", acp, grid, i, x_prev, o, torch.zeros_like(x_prev), True)
        b_i = abs(float(sampler.coef[i, 1]))
        bound = zr.state_bound(want, 0.0) + b_i * (1e-5 * float(o.abs().max()) + (2 * G - 1) * 2.0 ** -24 * float(scaled.abs().max()))
        err = float((st.x.cpu().double() - want).abs().max())
        plain = zr.step("ddim", acp, grid, i, x_prev, zr.guided(out, G, True), torch.zeros_like(x_prev), True)
        print(f"\n[zero-SNR chain capture {capture} step {i} t {grid[i]}] k {k.tolist()} err {err:.3g} (bound {bound:.3g}); "
              f"without the rescale {float((plain - want).abs().max()):.3g}")
        assert err <= bound
        assert float((plain - want).abs().max()) > 100 * bound  # the rescale is what is being checked
        ks.append(k)
    assert bool(((torch.stack(ks) - 1.0).abs() > 1e-2).all())
    assert sampler.step() is False and st.cursor.cpu().tolist() == [S, 5]


@pytest.fixture(scope="module")
def harness():
    return (_harness_unet(), *_conditioning())


@pytest.mark.parametrize("kw", [ZERO, dict(method="plms"), dict(method="euler_a")], ids=["ddim-zero-snr", "plms", "euler_a"])
def test_replayed_equals_host_launched_with_the_rescale(harness, kw):
    unet, cond, neg = harness
    run = lambda s, seed=5: s.sample(cond, neg, seed=seed, latent_shape=SHAPE).cpu()  # noqa: E731
    host = dfa.LatentSampler(unet, num_inference_steps=S, guidance_rescale=PHI, capture_graph=False, **kw)
    want = run(host)
    sampler = dfa.LatentSampler(unet, num_inference_steps=S, guidance_rescale=PHI, **kw)
    first = run(sampler)
    assert sampler.replaying and not host.replaying and bool(torch.isfinite(first).all())
    assert torch.equal(first, want)
    other, again = run(sampler, 6), run(sampler)  # the same recording: the seed lives in device memory
    assert sampler.replaying and torch.equal(again, first) and not torch.equal(other, first)
    none = run(dfa.LatentSampler(unet, num_inference_steps=S, guidance_rescale=0.0, **kw))
    assert torch.equal(none, run(dfa.LatentSampler(unet, num_inference_steps=S, **kw)))  # 0: the sampler as it was
    assert not torch.equal(none, first)


def test_a_single_pass_launches_nothing():
    model = GainDenoiser().to(DEV)
    cond, neg = _gain_conditioning()
    runs = []
    for phi in (PHI, 0.0):
        sampler = dfa.LatentSampler(model, num_inference_steps=S, guidance_scale=1.0, guidance_rescale=phi, **ZERO)
        runs.append(sampler.sample(cond, neg, seed=5, latent_shape=SHAPE).cpu())
        assert sampler.replaying and not sampler.state.cfg and sampler.state.model_in.shape[0] == B
    assert torch.equal(runs[0], runs[1])
    guided = [dfa.LatentSampler(model, num_inference_steps=S, guidance_scale=G, guidance_rescale=phi, **ZERO)
              .sample(cond, neg, seed=5, latent_shape=SHAPE).cpu() for phi in (PHI, 0.0)]
    assert not torch.equal(guided[0], guided[1])  # (on the same model a guided run does show the rescale)


def test_full_strength_image_to_image_starts_from_the_seeds_noise():
    model = GainDenoiser().to(DEV)
    cond, neg = _gain_conditioning()
    init = torch.randn(B, *SHAPE, generator=torch.Generator().manual_seed(2)).to(DEV) * 3.0
    sampler = dfa.LatentSampler(model, num_inference_steps=S, guidance_scale=G, **ZERO)
    sampler.begin(cond, neg, seed=5, latent_shape=SHAPE)
    x_T = sampler.latents.clone()
    sampler.begin(cond, neg, seed=5, init_latents=init, strength=1.0)
    assert sampler.run_timesteps.tolist() == [999, 749, 499, 249]
    assert torch.equal(sampler.latents, x_T)  # 0·init + 1·ε
    plain = dfa.LatentSampler(model, num_inference_steps=S, guidance_scale=G, method="ddim", v_prediction=True,
                              timestep_spacing="trailing")
    plain.begin(cond, neg, seed=5, init_latents=init, strength=1.0)
    assert not torch.equal(plain.latents, x_T)  # (the plain table keeps √ᾱ[999] ≈ 0.068 of the image)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_add_noise_at_the_last_timestep_is_pure_noise(dtype):
    gen = torch.Generator().manual_seed(1)
    x0, eps = torch.randn(3, 4, 8, 8, generator=gen).to(DEV), torch.randn(3, 4, 8, 8, generator=gen).to(DEV)
    t = torch.tensor([999, 999, 500], dtype=torch.int64, device=DEV)
    sa, sb = tr.ddpm_tables(device=DEV, zero_terminal_snr=True)
    noisy, target = nat.ddpm_add_noise(x0, eps, t, sa, sb, dtype, True)
    assert torch.equal(noisy[:2], eps[:2].to(dtype)) and torch.equal(target[:2], (-x0[:2]).to(dtype))
    assert not torch.equal(noisy[2], eps[2].to(dtype))
    sa, sb = tr.ddpm_tables(device=DEV)
    noisy, _ = nat.ddpm_add_noise(x0, eps, t, sa, sb, dtype, True)
    assert not torch.equal(noisy[:2], eps[:2].to(dtype))  # (the plain table leaves signal in)


def test_lora_trainer_on_the_rescaled_tables(tmp_path, repeatable_stock_kernels):
    kw = dict(v_prediction=True, zero_terminal_snr=True, snr_gamma=5.0)
    plain, _ = _lora_trainer(v_prediction=True, snr_gamma=5.0)
    sa, sb = tr.ddpm_tables()
    assert torch.equal(plain.sqrt_acp.cpu(), sa) and torch.equal(plain.sqrt_1macp.cpu(), sb)  # the flag off: today's tables
    assert plain._config()["zero_terminal_snr"] is False
    ends = {}
    for graph in (False, True):
        trainer, _ = _lora_trainer(capture_graph=graph, **kw)
        assert float(trainer.sqrt_acp[-1]) == 0.0 and float(trainer.sqrt_1macp[-1]) == 1.0 and float(trainer.loss_weights[-1]) == 0.0
        assert torch.equal(trainer.sqrt_acp.cpu(), tr.ddpm_tables(zero_terminal_snr=True)[0])
        assert trainer._config()["zero_terminal_snr"] is True
        losses = _steps(trainer, _feed, 0, 1)
        assert (trainer._graph is not None) == graph and bool(torch.isfinite(losses[0]))
        ends[graph] = (trainer.slab.params.clone(), losses[0])
    assert torch.equal(ends[True][0], ends[False][0]) and torch.equal(ends[True][1], ends[False][1])
    plain_loss = _steps(plain, _feed, 0, 1)[0]
    assert not torch.equal(plain_loss, ends[False][1])  # the tables are read
    # two steps, a save and a third against a load into a fresh trainer of the same flags and one step
    straight, _ = _lora_trainer(**kw)
    _steps(straight, _feed, 0, 2)
    path = tmp_path / "zero_snr.safetensors"
    straight.save_checkpoint(path)
    want_loss = _steps(straight, _feed, 2, 3)
    resumed, _ = _lora_trainer(warm_seed=12, **kw)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        resumed.load_checkpoint(path)
    assert not [w for w in caught if "other arguments" in str(w.message)]
    got_loss = _steps(resumed, _feed, 2, 3)
    assert torch.equal(got_loss[0], want_loss[0])
    _assert_same(_snap(resumed), _snap(straight), "2 + save + 1 against load + 1")
    with pytest.warns(UserWarning, match="zero_terminal_snr: checkpoint True, trainer False"):
        plain.load_checkpoint(path)
    assert float(plain.sqrt_acp[-1]) != 0.0  # nothing is restored from the file
    # a file from before the argument existed reads as False
    sd = straight.state_dict()
    del sd["meta"]["config"]["zero_terminal_snr"]
    with pytest.warns(UserWarning, match="zero_terminal_snr: checkpoint False, trainer True"):
        resumed.load_state_dict(sd)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        other, _ = _lora_trainer(v_prediction=True, snr_gamma=5.0)
        other.load_state_dict(sd)
    assert not [w for w in caught if "other arguments" in str(w.message)]
    with pytest.raises(ValueError, match="needs v_prediction=True"):
        _lora_trainer(zero_terminal_snr=True)


def test_inversion_trainer_on_the_rescaled_tables():
    from tests.test_inversion_host import _tiny_models

    gen = torch.Generator().manual_seed(4)
    lat = (torch.randn(2, 4, 8, 8, generator=gen) * 0.18215).to(DEV)
    ids = torch.randint(3, 50, (2, 8), generator=gen)
    ids[:, 2] = 55
    losses = []
    for flag in (False, True):
        unet, te = _tiny_models()
        trainer = InversionTrainer(unet.to(DEV), te.to(DEV), [55], accum_iter=1, v_prediction=True, zero_terminal_snr=flag)
        assert trainer._config()["zero_terminal_snr"] is flag and (float(trainer.sqrt_acp[-1]) == 0.0) == flag
        if not flag:
            assert torch.equal(trainer.sqrt_acp.cpu(), tr.ddpm_tables()[0]) and torch.equal(trainer.sqrt_1macp.cpu(), tr.ddpm_tables()[1])
        losses.append(float(trainer.step(lat, input_ids=ids.to(DEV), seed=3)))
        assert bool(torch.isfinite(te.get_input_embeddings().weight[55]).all())
        sd = trainer.state_dict()
        del sd["meta"]["config"]["zero_terminal_snr"]
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            trainer.load_state_dict(sd)  # a file without the key loads, and reads as False
        assert bool([w for w in caught if "zero_terminal_snr: checkpoint False, trainer True" in str(w.message)]) == flag
        trainer.close()
    assert all(l == l and abs(l) < float("inf") for l in losses) and losses[0] != losses[1]
    unet, te = _tiny_models()
    with pytest.raises(ValueError, match="needs v_prediction=True"):
        InversionTrainer(unet.to(DEV), te.to(DEV), [55], zero_terminal_snr=True)
