"""ddpm_posterior_prologue / ddpm_posterior_sample — the latents drawn from the VAE's moments inside the step prologue
(train_lora_dreambooth.py:818-821, cli_lora_pti.py:180-184) — against the Philox oracle and the float64 formula
(tests/posterior_cases.py), at the layout edges, and through both trainers, host-launched and recorded."""
import itertools
import json

import numpy as np
import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import trainer as tr
from diffusion_finetuning_amd.inversion import InversionTrainer
from oracle import lora_oracle as orc
from oracle import philox
from tests import posterior_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = 0.18215


@pytest.fixture(autouse=True)
def _collect_garbage_first():
    """A recording left in a reference cycle by an earlier test must not be destroyed in the middle of another capture."""
    import gc

    gc.collect()


def _moments(shape, seed, dtype=torch.float32):
    """VAE-like moments: means of order one, log-variances around −3 ± 2."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(shape, generator=g)
    c = shape[1] // 2
    m[:, c:] = m[:, c:] * 2.0 - 3.0
    return m.to(dtype)


@pytest.fixture(scope="module")
def tables():
    return tr.ddpm_tables(device=DEV), orc.ddpm_alphas_cumprod()


@pytest.fixture(scope="module")
def draw(tables):
    """The issue's draw case, launched once: B=5, [5,8,16,16] moments, seed 77, step 3, fp32 out, ε-target."""
    (sa, sb), _ = tables
    m = _moments((5, 8, 16, 16), 0)
    out = nat.ddpm_posterior_prologue(m.to(DEV), sa, sb, torch.float32, 77, 3, False, want_draw=True)
    return m, tuple(o.cpu() for o in out)


def test_draw_matches_the_philox_oracle_and_the_existing_prologue(draw, tables):
    (sa, sb), _ = tables
    m, (noisy, target, t, x0, z, eps) = draw
    eps_ref, t_ref = philox.step_randomness(5, 4 * 16 * 16, 1000, 77, 3)
    z_ref = pc.stream_normals(5, 4 * 16 * 16, 77, 3)
    assert np.array_equal(t.numpy(), t_ref)  # integer stream: bit-exact
    d_eps = float((eps.reshape(5, -1) - torch.from_numpy(eps_ref)).abs().max())
    d_z = float((z.reshape(5, -1) - torch.from_numpy(z_ref)).abs().max())
    print(f"\n[posterior draw] |eps - oracle| {d_eps:.3g}  |z - oracle| {d_z:.3g}")
    assert d_eps < 2e-5 and d_z < 2e-5  # libm vs GPU logf/sincosf
    assert not torch.equal(z, eps)
    # eps and t are the existing entry's, bit for bit, whatever x0 it is given
    for x0_any in (x0, torch.zeros_like(x0)):
        _, _, t_old, eps_old = nat.ddpm_noise_prologue(x0_any.to(DEV), sa, sb, torch.float32, 77, 3, False, want_draw=True)
        assert torch.equal(t_old.cpu(), t) and torch.equal(eps_old.cpu(), eps)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("m_dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_formula_against_float64_from_the_kernels_own_draw(tables, relerr, m_dtype, out_dtype):
    """x0, noisy and both targets from the launch's own z_out / eps_out / t_out, so no libm difference enters: fp32 outputs
    within 1e-5 relative, 16-bit outputs within one unit in the last place of the storage type at the float64 value."""
    (sa, sb), acp = tables
    m = _moments((5, 8, 16, 16), 1, m_dtype)
    for v in (False, True):
        noisy, target, t, x0, z, eps = (o.cpu() for o in nat.ddpm_posterior_prologue(m.to(DEV), sa, sb, out_dtype, 77, 3, v,
                                                                                      want_draw=True))
        assert noisy.dtype == target.dtype == out_dtype and x0.dtype == torch.float32 and x0.shape == (5, 4, 16, 16)
        # the very bits ddpm_add_noise makes of this draw: what lets a moments-fed step stand in for a latents-fed one
        again = nat.ddpm_add_noise(x0.to(DEV), eps.to(DEV), t.to(DEV), sa, sb, out_dtype, v)
        assert torch.equal(again[0].cpu(), noisy) and torch.equal(again[1].cpu(), target)
        x0_ref = pc.posterior_x0(m, z, SCALE)
        noisy_ref, target_ref = pc.noisy_and_target(x0_ref, eps, t, acp, v)
        errs = relerr(x0, x0_ref), relerr(noisy, noisy_ref), relerr(target, target_ref)
        print(f"\n[posterior formula m={m_dtype} out={out_dtype} v={v}] x0 {errs[0]:.3g} noisy {errs[1]:.3g} target {errs[2]:.3g}")
        assert errs[0] < 1e-5
        if out_dtype == torch.float32:
            assert errs[1] < 1e-5 and errs[2] < 1e-5
        else:
            for got, ref in ((noisy, noisy_ref), (target, target_ref)):
                off = ((got.double() - ref).abs() / pc.storage_ulp(ref, out_dtype)).max().item()
                assert off <= 1.0, off


def _check_against_own_draw(m, out, acp, v, relerr, scale=SCALE):
    noisy, target, t, x0, z, eps = (None if o is None else o.cpu() for o in out)
    x0_ref = pc.posterior_x0(m, z, scale)
    noisy_ref, target_ref = pc.noisy_and_target(x0_ref, eps, t, acp, v)
    assert torch.isfinite(x0).all()
    assert relerr(x0, x0_ref) < 1e-5 and relerr(noisy, noisy_ref) < 1e-5
    if target is not None:
        assert relerr(target, target_ref) < 1e-5
    return x0, x0_ref


def test_edges_ragged_rows_unaligned_pointer_clamps_smallest_shape_and_no_target(tables, relerr):
    (sa, sb), acp = tables
    # B=3, per_row=37: 111 elements — groups straddle rows, the last one is ragged, the element-by-element path
    m = _moments((3, 2, 37), 2)
    out = nat.ddpm_posterior_prologue(m.to(DEV), sa, sb, torch.float32, 5, 9, True, want_draw=True)
    _check_against_own_draw(m, out, acp, True, relerr)
    eps_ref, t_ref = philox.step_randomness(3, 37, 1000, 5, 9)
    assert np.array_equal(out[2].cpu().numpy(), t_ref)
    assert float((out[5].cpu().reshape(3, 37) - torch.from_numpy(eps_ref)).abs().max()) < 2e-5
    assert float((out[4].cpu().reshape(3, 37) - torch.from_numpy(pc.stream_normals(3, 37, 5, 9))).abs().max()) < 2e-5
    # a moments pointer one element off the allocation: per_row % 4 == 0, yet the unaligned path — same bits as the aligned one
    for dtype in (torch.float32, torch.bfloat16):
        m = _moments((2, 8, 4, 4), 3, dtype)
        flat = torch.zeros(m.numel() + 1, dtype=dtype, device=DEV)
        flat[1:].copy_(m.reshape(-1))
        shifted = flat[1:].view(m.shape)
        assert shifted.data_ptr() % (4 * m.element_size()) != 0 and shifted.is_contiguous()
        off = nat.ddpm_posterior_prologue(shifted, sa, sb, torch.float32, 5, 9, False, want_draw=True)
        on = nat.ddpm_posterior_prologue(m.to(DEV), sa, sb, torch.float32, 5, 9, False, want_draw=True)
        _check_against_own_draw(m, off, acp, False, relerr)
        assert all(torch.equal(a, b) for a, b in zip(off, on))
        z = off[4]
        assert torch.equal(nat.ddpm_posterior_sample(shifted, z, SCALE), nat.ddpm_posterior_sample(m.to(DEV), z, SCALE))
    # both clamps, in the first and the last element of a row, on both paths (per_row 64: 4-element accesses; 37: scalar)
    for shape in ((2, 2, 64), (2, 2, 37)):
        m = _moments(shape, 4)
        m[0, 1, 0], m[0, 1, -1], m[1, 1, 0], m[1, 1, -1] = -40.0, 25.0, 20.0, -30.0
        m[0, 0, 0] = 0.0  # (no mean in front of the tiny std of the lower clamp)
        out = nat.ddpm_posterior_prologue(m.to(DEV), sa, sb, torch.float32, 8, 1, False, want_draw=True)
        x0, x0_ref = _check_against_own_draw(m, out, acp, False, relerr)
        pick = (torch.tensor([0, 0, 1, 1]), torch.tensor([0, 0, 0, 0]), torch.tensor([0, -1, 0, -1]))
        assert torch.allclose(x0[pick].double(), x0_ref[pick], rtol=1e-5, atol=0.0)
        unclamped = (m[:, :1].double() + torch.exp(0.5 * m[:, 1:].double()) * out[4].cpu().double()) * SCALE
        assert ((unclamped[pick][:2] - x0_ref[pick][:2]).abs() > 0.5 * x0_ref[pick][:2].abs()).all()  # −40 and 25 WERE clamped
    # the smallest shape, and no target
    m = _moments((1, 2, 4), 5)
    out = nat.ddpm_posterior_prologue(m.to(DEV), sa, sb, torch.float32, 1, 0, False, want_draw=True, want_target=False)
    assert out[1] is None
    _check_against_own_draw(m, out, acp, False, relerr)


def test_caller_drawn_form_against_the_torch_composite_and_add_noise(tables, relerr):
    (sa, sb), acp = tables
    g = torch.Generator().manual_seed(6)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        m = _moments((2, 8, 8, 8), 6, dtype)
        z = torch.randn(2, 4, 8, 8, generator=g)
        x0 = nat.ddpm_posterior_sample(m.to(DEV), z.to(DEV), SCALE)
        assert x0.dtype == torch.float32 and x0.shape == (2, 4, 8, 8)
        assert relerr(x0, pc.posterior_x0(m, z, SCALE)) < 1e-5
    m = _moments((2, 8, 37), 7)  # the scalar path
    z = torch.randn(2, 4, 37, generator=g)
    assert relerr(nat.ddpm_posterior_sample(m.to(DEV), z.to(DEV), 0.5), pc.posterior_x0(m, z, 0.5)) < 1e-5
    # the step's caller-drawn route (posterior_sample, then add_noise) is ddpm_add_noise on that very x0, bit for bit
    from diffusion_finetuning_amd import step as stp

    m = _moments((2, 8, 8, 8), 6, torch.bfloat16).to(DEV)
    z, eps = torch.randn(2, 4, 8, 8, generator=g).to(DEV), torch.randn(2, 4, 8, 8, generator=g).to(DEV)
    t = torch.tensor([3, 998], device=DEV)
    x0 = nat.ddpm_posterior_sample(m, z, SCALE)
    for v in (False, True):
        nz = stp.Noising(sa, sb, torch.float32, v, 1000)
        noisy, target, t_back = stp.noise_prologue(nz, None, eps, t, None, None, moments=m, posterior_noise=z)
        want = nat.ddpm_add_noise(x0, eps, t, sa, sb, torch.float32, v)
        assert torch.equal(noisy, want[0]) and torch.equal(target, want[1]) and t_back is t
        want_noisy, want_target = pc.noisy_and_target(x0, eps, t, acp, v)
        assert relerr(noisy, want_noisy) < 1e-6 and relerr(target, want_target) < 1e-6


def test_two_launches_are_bit_identical_and_the_step_changes_the_draw(tables):
    (sa, sb), _ = tables
    m = _moments((5, 8, 16, 16), 8, torch.float16).to(DEV)
    a = nat.ddpm_posterior_prologue(m, sa, sb, torch.float16, 1, 2, True, want_draw=True)
    b = nat.ddpm_posterior_prologue(m, sa, sb, torch.float16, 1, 2, True, want_draw=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = nat.ddpm_posterior_prologue(m, sa, sb, torch.float16, 1, 3, True, want_draw=True)
    assert not torch.equal(a[4], c[4]) and not torch.equal(a[5], c[5])
    d = nat.ddpm_posterior_prologue(m, sa, sb, torch.float16, 2, 2, True, want_draw=True)
    assert not torch.equal(a[4], d[4])


# -- through the trainers ------------------------------------------------------------------------------------------------
@pytest.fixture
def repeatable_stock_kernels():
    """The stock fp32 kernels under the tiny models do not repeat bit for bit by default on this stack (profiles/README.md,
    "Repeatability of the fp32 inversion step"): two runs of the SAME latents-fed trainer already differ in the last bits, so a
    bit-for-bit comparison of two trainers says nothing.  With torch's deterministic algorithms they repeat, and the comparison
    is about the step's inputs alone."""
    before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
              torch.backends.cudnn.deterministic)
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic = True
    yield
    torch.use_deterministic_algorithms(before[0], warn_only=before[1])
    torch.backends.cudnn.deterministic = before[2]


def _warm(params, seed, std):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i, p in enumerate(params):
            if i % 2 == 0:
                p.copy_(torch.randn(p.shape, generator=g).to(p.device) * std)


def _lora_trainer(tiny_unet_factory, dtype=torch.float32, **kw):
    unet = tiny_unet_factory(seed=5).to(DEV).to(dtype)
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    _warm(list(itertools.chain(*params)), 11, 0.02)
    return tr.LoraTrainer(unet, lr=1e-3, **kw), unet


@pytest.mark.parametrize("graph", [False, True])
def test_lora_trainer_fed_with_moments_leaves_the_bits_of_the_step_fed_with_the_draw(tiny_unet_factory, relerr, graph,
                                                                                     repeatable_stock_kernels):
    """step(moments=m, seed=s) against step(latents=x0_out, noise=eps_out, timesteps=t_out) of a direct prologue call with the
    same key; then the caller-drawn form against latents from ddpm_posterior_sample; then a latents-fed step re-records."""
    sa, sb = tr.ddpm_tables(device=DEV)
    batches = [(_moments((2, 8, 8, 8), 20 + s).to(DEV), orc.synthetic_batch(s, 2, 8, 6, 32)[3].to(DEV)) for s in range(3)]
    a, unet_a = _lora_trainer(tiny_unet_factory, capture_graph=graph)
    b, unet_b = _lora_trainer(tiny_unet_factory, capture_graph=graph)
    for s, (m, ctx) in enumerate(batches):
        la = a.step(moments=m, seed=41, encoder_hidden_states=ctx)
        _, _, t, x0, _, eps = nat.ddpm_posterior_prologue(m, sa, sb, torch.float32, 41, s, False, want_draw=True)
        lb = b.step(latents=x0, noise=eps, timesteps=t, encoder_hidden_states=ctx)
        assert torch.equal(la, lb), (s, la, lb)
    state_a, state_b = tr.flat_lora_state(unet_a), tr.flat_lora_state(unet_b)
    print(f"\n[moments-fed LoraTrainer graph={graph}] against the latents-fed one: {relerr(state_a, state_b):.3g}")
    assert torch.equal(state_a, state_b)
    assert (a._graph is not None) == graph == (b._graph is not None)
    # caller-drawn: posterior_noise + noise + timesteps
    g = torch.Generator().manual_seed(3)
    m, ctx = batches[0]
    pz, noise, ts = torch.randn(2, 4, 8, 8, generator=g).to(DEV), torch.randn(2, 4, 8, 8, generator=g).to(DEV), torch.tensor([7, 900], device=DEV)
    key_before = a._recorder.key
    la = a.step(moments=m, noise=noise, timesteps=ts, posterior_noise=pz, encoder_hidden_states=ctx)
    lb = b.step(latents=nat.ddpm_posterior_sample(m, pz), noise=noise, timesteps=ts, encoder_hidden_states=ctx)
    assert torch.equal(la, lb) and torch.equal(tr.flat_lora_state(unet_a), tr.flat_lora_state(unet_b))
    if graph:
        assert a._graph is not None and a._recorder.key != key_before and a._recorder.moments is not None
        assert "moments" in a._recorder.key and torch.float32 in a._recorder.key and "moments" not in b._recorder.key
        # a latents-fed step after a moments-fed one: recorded anew, never a replay of the moments recording
        old = a._recorder.graph
        a.step(latents=nat.ddpm_posterior_sample(m, pz), noise=noise, timesteps=ts, encoder_hidden_states=ctx)
        assert a._graph is not None and a._recorder.graph is not old and a._recorder.key == b._recorder.key
        assert a._recorder.moments is None and len(a._recorder.inputs) == 3 and a._recorder.inputs[0] is not None
        # moments of another dtype: another recording
        a.step(moments=m.half(), seed=41, encoder_hidden_states=ctx)
        k16 = a._recorder.key
        a.step(moments=m, seed=41, encoder_hidden_states=ctx)
        assert k16 != a._recorder.key and torch.float16 in k16


@pytest.mark.parametrize("graph", [False, True])
def test_inversion_trainer_fed_with_moments_leaves_the_bits_of_the_step_fed_with_the_draw(golden_pti, graph, repeatable_stock_kernels):
    from tests.test_oracle_golden import build_pti_models

    t, meta = golden_pti
    cfg = json.loads(meta["cfg"])
    ph = [cfg["vocab"] - 3, cfg["vocab"] - 8]
    sa, sb = tr.ddpm_tables(device=DEV)
    tables = []
    for fed in ("moments", "latents"):
        unet, te = build_pti_models(t, cfg, DEV, torch.float32)
        orc.freeze_all_but_token_embeddings(te)
        trainer = InversionTrainer(unet, te, ph, lr=5e-3, weight_decay=1e-2, lr_scheduler="linear", max_train_steps=8,
                                   accum_iter=2, capture_graph=graph)
        for s in range(3):
            m = _moments((cfg["batch"], 8, cfg["latent_hw"], cfg["latent_hw"]), 30 + s).to(DEV)
            ids = t["ids"][s % t["ids"].shape[0]].clone()
            ids[:, 1] = ph[0]
            ids[0, 2] = ph[1]
            if fed == "moments":
                trainer.step(moments=m, input_ids=ids.to(DEV), seed=17)
            else:
                _, _, ts, x0, _, eps = nat.ddpm_posterior_prologue(m, sa, sb, torch.float32, 17, s, False, want_draw=True)
                trainer.step(x0, eps, ts, input_ids=ids.to(DEV))
        assert (trainer._graph is not None) == graph
        tables.append(te.get_input_embeddings().weight.detach().clone())
    assert torch.equal(tables[0], tables[1])
    assert not torch.equal(tables[0][ph].cpu(), t["table.init"][ph])
