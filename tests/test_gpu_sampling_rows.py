"""Per-sample LoRA gates and shared noise in the latent sampler (MI355X): `LatentSampler(..., lora_scales=, shared_noise=)`.

 (e) per-sample independence through the whole UNet forward: sample b of a run with gates (s0, s1, s2) is sample b of the run
     with the uniform gates (s_b, s_b, s_b), bit for bit in f16; one-hot gates over three stacked rank-4 adapters against the
     model patched with adapter b alone (fp32, the routes differ in rank: FP32_TOL of tests/test_gpu_sampling.py);
 (f) a uniform table against `tune_lora_scale` (fp32, FP32_TOL);
 (g) one recording serves every table: the captured graph is the same object across runs, replayed ≡ host-launched (f16,
     torch.equal), nothing stays installed and the groups come back;
 (h) shared noise at kernel level: every sample's x_T, variance draw and keep-mask re-noise is the B = 1 state's, with
     per_row a multiple of 4 and ragged (37); without it the draws are today's;
 (i) the notebook's sweep end to end: gates [0, 0.7, 1.0], shared noise, img2img at strength 0.75, 4-step PLMS.
"""
import itertools

import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd.ops import ROW_SCALES
from tests import sampling_reference as ref
from tests.conftest import build_tiny_unet, rel_err
from diffusion_finetuning_amd import trainer as tr
from diffusion_finetuning_amd.attention import set_use_hip_attention
from tests.test_gpu_sampling import FP32_TOL, S_UNET, SHAPE, _conditioning, _harness_unet, _same, _set_cursor, _warm

pytestmark = pytest.mark.gpu
DEV = "cuda"
B3 = 3


@pytest.fixture(autouse=True)
def _collect_garbage_first():
    """A recording left in a reference cycle by an earlier test must not be destroyed in the middle of another capture."""
    import gc

    gc.collect()


@pytest.fixture(scope="module")
def f16_unet():
    return _harness_unet(torch.float16)


def _no_table_left(unet):
    return not any(ROW_SCALES in m.__dict__ for m in unet.modules())


@pytest.fixture
def deterministic_convs():
    """At 6 rows MIOpen's default pick for one of the harness UNet's stock convolutions (up_blocks.0.upsamplers.0.conv) is not
    run-to-run deterministic — two no-table runs of the unchanged sampler differ by 2e-3 there, at 4 rows they are bit-identical —
    so a bit-for-bit comparison at B = 3 asks PyTorch for deterministic convolution algorithms, and puts the flag back."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def test_each_sample_follows_its_own_gate_through_the_unet(f16_unet, deterministic_convs):
    """(e), first regime: f16, guidance on (6 rows), a per-sample [B] table on the plainly injected model."""
    unet = f16_unet
    cond, neg = _conditioning(B3)
    scales = (0.0, 0.7, 1.3)
    sampler = dfa.LatentSampler(unet, num_inference_steps=S_UNET)
    mixed = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE, lora_scales=torch.tensor(scales, device=DEV)).cpu()
    assert sampler.replaying and _no_table_left(unet)
    for b, s in enumerate(scales):
        uniform = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE, lora_scales=torch.full((B3,), s, device=DEV)).cpu()
        assert torch.equal(uniform[b], mixed[b]), (b, s, rel_err(uniform[b], mixed[b]))
    # the gates act: the run without LoRA (all gates closed) differs from the run with all gates open
    closed = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE, lora_scales=[0.0, 0.0, 0.0]).cpu()
    opened = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE, lora_scales=[1.0, 1.0, 1.0]).cpu()
    assert not torch.equal(closed, opened) and torch.equal(closed[0], mixed[0])


def _adapters(n, seed=21):
    """n rank-4 adapters for the tiny UNet as positional [up0, down0, ...] lists (fp32, CPU)."""
    probe = build_tiny_unet(seed=5)
    dfa.inject_trainable_lora(probe, r=4)
    shapes = [(up.weight.shape, down.weight.shape) for up, down in dfa.extract_lora_ups_down(probe)]
    g = torch.Generator().manual_seed(seed)
    return [list(itertools.chain(*[(torch.randn(u, generator=g) * 0.05, torch.randn(d, generator=g) / 4) for u, d in shapes]))
            for _ in range(n)]


def test_one_hot_gates_pick_one_stacked_checkpoint_per_sample():
    """(e), second regime: fp32, three rank-4 adapters stacked to rank 12, one-hot [B, 12] tables, against the model patched
    with adapter b alone under a table of ones."""
    lists = _adapters(3)
    cond, neg = _conditioning(B3)
    stacked = build_tiny_unet(seed=5).to(DEV)
    slots = dfa.monkeypatch_stack_lora(stacked, lists)
    assert [(s.start, s.stop) for s in slots] == [(0, 4), (4, 8), (8, 12)]
    table = torch.zeros(B3, 12, device=DEV)
    assign = (2, 0, 1)
    for b, k in enumerate(assign):
        table[b, slots[k]] = 1.0
    sampler = dfa.LatentSampler(stacked, num_inference_steps=S_UNET)
    mixed = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE, lora_scales=table).cpu()
    assert _no_table_left(stacked)
    for b, k in enumerate(assign):
        alone = build_tiny_unet(seed=5).to(DEV)
        dfa.monkeypatch_or_replace_lora(alone, list(lists[k]), r=4)
        one = dfa.LatentSampler(alone, num_inference_steps=S_UNET)
        want = one.sample(cond, neg, seed=5, latent_shape=SHAPE, lora_scales=torch.ones(B3, 4, device=DEV)).cpu()
        assert _same(mixed[b], want[b], torch.float32, f"sample {b}: stacked + one-hot vs adapter {k} alone")
        other = want[(b + 1) % B3]
        assert rel_err(mixed[b], other) > 10 * FP32_TOL  # (the comparison can tell the samples apart)
    with pytest.raises(ValueError, match="rank"):
        sampler.sample(cond, neg, seed=5, latent_shape=SHAPE, lora_scales=torch.ones(B3, 11, device=DEV))
    assert _no_table_left(stacked)


def test_uniform_table_against_tune_lora_scale():
    """(f): fp32, a table filled with s against `tune_lora_scale(unet, s)` without a table."""
    unet = _harness_unet(torch.float32)
    cond, neg = _conditioning(B3)
    s = 0.7
    sampler = dfa.LatentSampler(unet, num_inference_steps=S_UNET)
    gated = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE, lora_scales=torch.full((B3,), s, device=DEV)).cpu()
    dfa.tune_lora_scale(unet, s)
    scalar = dfa.LatentSampler(unet, num_inference_steps=S_UNET).sample(cond, neg, seed=5, latent_shape=SHAPE).cpu()
    dfa.tune_lora_scale(unet, 1.0)
    assert _same(gated, scalar, torch.float32, "uniform table vs tune_lora_scale")
    plain = dfa.LatentSampler(unet, num_inference_steps=S_UNET).sample(cond, neg, seed=5, latent_shape=SHAPE).cpu()
    assert rel_err(gated, plain) > 10 * FP32_TOL  # (s = 0.7 is not s = 1)


def test_one_recording_serves_every_table(f16_unet):
    """(g)"""
    unet = f16_unet
    cond, neg = _conditioning(2)
    tables = [torch.tensor([0.2, 1.0], device=DEV), torch.tensor([1.5, 0.0], device=DEV),
              torch.tensor([[1.0, 0.0, 0.5, 0.0], [0.0, 2.0, 0.0, 1.0]], device=DEV)]
    sampler = dfa.LatentSampler(unet, num_inference_steps=S_UNET, capture_graph=True)
    host = dfa.LatentSampler(unet, num_inference_steps=S_UNET, capture_graph=False)
    graphs, outs = [], []
    for t in tables:
        outs.append(sampler.sample(cond, neg, seed=5, latent_shape=SHAPE, lora_scales=t).cpu())
        assert sampler.replaying
        graphs.append(sampler._recorder.graph)
        assert torch.equal(outs[-1], host.sample(cond, neg, seed=5, latent_shape=SHAPE, lora_scales=t).cpu())
        assert _no_table_left(unet)
    assert graphs[0] is not None and graphs[1] is graphs[0] and graphs[2] is graphs[0]
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])


def test_groups_stand_aside_for_a_table_and_come_back():
    """(g), the grouped launches: an f16 model with fp32 factors (the drop-in q/k/v and context-K/V groups of the attention
    switch are usable there) samples with a table on the per-layer route and afterwards exactly as before."""
    unet = build_tiny_unet(seed=5).to(DEV).half()
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    _warm(list(itertools.chain(*params)), 11, 0.05)
    for layer in tr.lora_layers(unet):
        layer.lora_down.float()
        layer.lora_up.float()
    assert set_use_hip_attention(unet, True) > 0
    cond, neg = _conditioning(2)
    groups = [m.__dict__["_dfa_qkv"] for m in unet.modules() if m.__dict__.get("_dfa_qkv") is not None]
    assert groups
    x = torch.zeros(2, 4, groups[0].K, dtype=torch.float16, device=DEV)
    sampler = dfa.LatentSampler(unet, num_inference_steps=S_UNET)
    before = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE).cpu()
    with torch.no_grad():
        assert groups[0].usable(x, torch.float16)
    gated = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE, lora_scales=[1.0, 0.0]).cpu()
    assert _no_table_left(unet) and not torch.equal(gated[1], before[1])
    print("\n[groups] sample 0 under a gate of 1.0 (per-layer launches) vs no table (grouped launches): rel err %.3g" %
          rel_err(gated[0], before[0]))
    assert rel_err(gated[0], before[0]) < 2e-2  # (f16 through four forwards on two routes: the bar of the single-pass comparison)
    with torch.no_grad():
        assert groups[0].usable(x, torch.float16)
        with dfa.lora_row_scales(unet, torch.ones(2, 4, device=DEV)):
            assert not groups[0].usable(x, torch.float16) and not _no_table_left(unet)
        assert groups[0].usable(x, torch.float16) and _no_table_left(unet)
    assert torch.equal(sampler.sample(cond, neg, seed=5, latent_shape=SHAPE).cpu(), before)


def _sample_state(B, per_row, shared, hw=None, multistep=False, S=4):
    """A state on the device with every sample holding the SAME data (so equal draws give equal results), zeros as model
    output; with `hw` a keep mask and init."""
    g = torch.Generator().manual_seed(3)
    rep = lambda t: t.repeat(B, *([1] * (t.dim() - 1))).contiguous().to(DEV)  # noqa: E731
    x = rep(torch.randn(1, per_row, generator=g))
    init = rep(torch.randn(1, per_row, generator=g)) if hw else None
    mask = rep(torch.rand(1, hw, generator=g)) if hw else None
    zeros = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    if multistep:
        ts, coef, plan = dfa.multistep_schedule("dpmpp_2m", S, False)
        keep = dfa.keep_schedule(ts).to(DEV) if hw else None
        st = nat.MultistepState(x, zeros(B, per_row), zeros(4, B, per_row), zeros(B, per_row), zeros(B, dt=torch.int64),
                                zeros(2, dt=torch.int32), ts.to(DEV), coef.to(DEV), plan.to(DEV), False, init, mask, keep)
    else:
        ts, coef = dfa.sampler_schedule("ddpm", S, False)
        keep = dfa.keep_schedule(ts).to(DEV) if hw else None
        st = nat.SampleState(x, zeros(B, per_row), zeros(B, dt=torch.int64), zeros(2, dt=torch.int32), ts.to(DEV), coef.to(DEV),
                             False, init, mask, keep)
    st.shared_noise = shared
    return st


@pytest.mark.parametrize("per_row,hw", [(256, 64), (37, 37)], ids=["quads", "ragged"])
def test_shared_noise_gives_every_sample_the_draws_of_the_single_run(per_row, hw):
    """(h).  Ragged: per_row = 37 is no multiple of the 4-element Philox group — element j of a sample still takes lane j mod 4
    of counter j div 4, so samples 1 and 2 start inside a group of the batch."""
    seed, step = 41, 1
    out1, out3 = torch.zeros(1, per_row, device=DEV), torch.zeros(B3, per_row, device=DEV)
    # x_T
    one, three, plain = _sample_state(1, per_row, True), _sample_state(B3, per_row, True), _sample_state(B3, per_row, False)
    today = _sample_state(B3, per_row, False)
    del today.shared_noise  # the state made the existing way: the class default
    for st in (one, three, plain, today):
        nat.ddpm_sample_init(st, seed)
    oracle = ref.init_normals(1, per_row, seed)
    assert float((one.x.cpu() - oracle).abs().max()) <= ref.Z_TOL
    single = _sample_state(1, per_row, False)
    nat.ddpm_sample_init(single, seed)
    assert torch.equal(one.x, single.x)  # B = 1: shared and plain are the same draw
    for b in range(B3):
        assert torch.equal(three.x[b], one.x[0]) and torch.equal(three.model_in[b], one.model_in[0]), ("x_T", b)
    assert torch.equal(plain.x, today.x) and not torch.equal(plain.x[1], plain.x[0])
    assert float((plain.x.cpu() - ref.init_normals(B3, per_row, seed)).abs().max()) <= ref.Z_TOL
    # the variance draw of a step (σ != 0 at step 1 of 4)
    z = {}
    for name, st, out in (("one", one, out1), ("three", three, out3), ("plain", plain, out3), ("today", today, out3)):
        _set_cursor(st, step, seed)
        z[name] = torch.full_like(st.x, 7.0)
        nat.ddpm_sample_step(st, out, 1.0, z_out=z[name])
    assert float((z["one"].cpu() - ref.step_normals(1, per_row, seed, step)).abs().max()) <= ref.Z_TOL
    for b in range(B3):
        assert torch.equal(z["three"][b], z["one"][0]), ("z", b)
    assert torch.equal(z["plain"], z["today"]) and torch.equal(plain.x, today.x) and not torch.equal(z["plain"][1], z["plain"][0])
    # the start noise of an image-to-image run, and the keep blend that regenerates it (step and multistep forms)
    for multistep in (False, True):
        one, three = _sample_state(1, per_row, True, hw, multistep), _sample_state(B3, per_row, True, hw, multistep)
        plain, today = _sample_state(B3, per_row, False, hw, multistep), _sample_state(B3, per_row, False, hw, multistep)
        del today.shared_noise
        eps = {}
        for name, st in (("one", one), ("three", three), ("plain", plain), ("today", today)):
            eps[name] = torch.full_like(st.x, 7.0)
            nat.ddpm_sample_init_from(st, seed, step, 0.8, 0.6, eps_out=eps[name])
        for b in range(B3):
            assert torch.equal(eps["three"][b], eps["one"][0]) and torch.equal(three.x[b], one.x[0]), ("eps", multistep, b)
        assert torch.equal(eps["one"], single.x) and torch.equal(eps["plain"], eps["today"])
        for st, out in ((one, out1), (three, out3), (plain, out3), (today, out3)):
            if multistep:
                nat.ddpm_sample_multistep_keep(st, out, 1.0)
            else:
                nat.ddpm_sample_step_keep(st, out, 1.0)
        for b in range(B3):
            assert torch.equal(three.x[b], one.x[0]), ("keep blend", multistep, b)
        assert torch.equal(plain.x, today.x) and not torch.equal(plain.x[1], plain.x[0])


def test_scale_sweep_at_equal_seed_in_one_batch():
    """(i): the reference's img2img recipe — strength 0.75, one sample per tune_lora_scale value at equal seed — as one batch."""
    unet = _harness_unet(torch.float32)
    cond1, neg1 = _conditioning(1)
    cond, neg = cond1.repeat(B3, 1, 1), neg1.repeat(B3, 1, 1)
    g = torch.Generator().manual_seed(9)
    init1 = torch.randn(1, *SHAPE, generator=g).to(DEV)
    kw = dict(seed=5, strength=0.75)
    sweep = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method="plms")
    batch = sweep.sample(cond, neg, init_latents=init1.repeat(B3, 1, 1, 1), lora_scales=[0.0, 0.7, 1.0], shared_noise=True,
                         **kw).cpu()
    assert not torch.equal(batch[0], batch[1]) and not torch.equal(batch[1], batch[2]) and not torch.equal(batch[0], batch[2])
    assert rel_err(batch[0], batch[2]) > 10 * FP32_TOL
    dfa.tune_lora_scale(unet, 0.0)
    alone = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method="plms").sample(cond1, neg1, init_latents=init1, **kw).cpu()
    dfa.tune_lora_scale(unet, 1.0)
    assert _same(batch[0], alone[0], torch.float32, "sample 0 of the sweep vs tune_lora_scale(unet, 0.0) at B = 1")
    last = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method="plms").sample(cond1, neg1, init_latents=init1, **kw).cpu()
    assert _same(batch[2], last[0], torch.float32, "sample 2 of the sweep vs scale 1.0 at B = 1")
