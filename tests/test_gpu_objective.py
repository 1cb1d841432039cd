"""Min-SNR / per-timestep loss weights and offset noise on the device: ddpm_mse_weighted_fwd_bwd against float64 autograd
and against ddpm_mse_fwd_bwd bit for bit, the two `_offset` prologues against the Philox oracle and against their plain forms,
and both trainers with the knobs on — host-launched against recorded, against the unweighted trainer, against the float64
loss of their own prediction, and across a checkpoint (tests/objective_reference.py holds the CPU side)."""
import gc
import itertools
import math
import warnings

import numpy as np
import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import step as stp
from diffusion_finetuning_amd import trainer as tr
from diffusion_finetuning_amd.inversion import InversionTrainer
from oracle import lora_oracle as orc
from tests import objective_reference as ref
from tests.conftest import build_tiny_unet, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 1000
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# loss and dpred against float64: the bounds of test_losses_against_reference_golden (f32, f16).  That test has no bf16 case,
# and one rounding of dpred to bf16 cannot meet the f16 figure, so the bf16 dpred bound is 2 × the error of the UNWEIGHTED kernel
# (ddpm_mse_fwd_bwd against float64) on the same inputs, measured in the same run and printed next to the weighted error
# (the figures seen on an MI355X are below).  The loss is accumulated in fp32 from the stored values whatever
# the dtype, so bf16 takes the 16-bit loss bound of that test.
DPRED_TOL = {torch.float32: 2e-6, torch.float16: 1e-3}
LOSS_TOL = {torch.float32: 2e-6, torch.float16: 2e-6 * 50, torch.bfloat16: 2e-6 * 50}
# Measured on an MI355X over the 18 bf16 cases: unweighted kernel 1.53e-3 – 1.81e-3 (so bounds of 3.06e-3 – 3.62e-3), weighted
# kernel 1.51e-3 – 1.79e-3; the largest weighted / unweighted ratio of a case is 1.17.
GRAD_SCALE = 64.0  # (keeps the f16 gradient of a 1/(n·C·h·w) mean out of the subnormals)


@pytest.fixture(autouse=True)
def _collect_garbage_first():
    """A recording left in a reference cycle by an earlier test must not be destroyed in the middle of another capture."""
    gc.collect()


@pytest.fixture
def repeatable_stock_kernels():
    """The stock fp32 kernels under the tiny UNet repeat bit for bit only with torch's deterministic algorithms (see
    tests/test_gpu_checkpoint.py): what a bit-for-bit comparison of two trainers needs."""
    before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
              torch.backends.cudnn.deterministic)
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic = True
    yield
    torch.use_deterministic_algorithms(before[0], warn_only=before[1])
    torch.backends.cudnn.deterministic = before[2]


# -- the weighted loss kernel -------------------------------------------------------------------------------------------------
SHAPES = {"vector": (4, 8, 8), "scalar": (3, 5, 7), "misaligned": (4, 8, 8)}


def _on_device(x, dtype, misaligned):
    """`x` on the device in `dtype`; `misaligned`: a contiguous view that starts 4 bytes off a 16-byte boundary."""
    x = x.to(dtype)
    if not misaligned:
        return x.to(DEV)
    lead = 4 // x.element_size()
    buf = torch.zeros(x.numel() + 16, dtype=dtype, device=DEV)
    view = buf[lead:lead + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    return view


def _loss_case(rows, kind, masked, dtype, seed=0):
    n_inst, n_prior = rows
    n = n_inst + n_prior
    C, h, w = SHAPES[kind]
    g = torch.Generator().manual_seed(seed)
    pred = _on_device(torch.randn(n, C, h, w, generator=g), dtype, kind == "misaligned")
    target = _on_device(torch.randn(n, C, h, w, generator=g), dtype, False)
    mask = None
    if masked:  # what lora_mask_prepare leaves: positive, mean 1
        m = torch.rand(n, 1, h, w, generator=g) + 0.05
        mask = (m / m.mean()).to(DEV)
    t = torch.tensor([0, T - 1, 500, 17, 250][:n], dtype=torch.int64)
    table = torch.rand(T, generator=g) + 0.5  # distinct weights for the timesteps in use …
    table[500] = 0.0                          # … one of them exactly 0
    return pred, target, mask, t.to(DEV), table.to(DEV), n_inst, n_prior


@pytest.fixture(scope="module")
def loss_references():
    """float64 (loss, dpred) per case, computed once and shared."""
    cache = {}

    def get(rows, kind, masked, dtype, case):
        key = (rows, kind, masked, dtype)
        if key not in cache:
            pred, target, mask, t, table, n_inst, n_prior = case
            cache[key] = ref.weighted_loss(pred, target, mask, t, table, n_inst, n_prior, 0.7, GRAD_SCALE)
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", list(SHAPES))
@pytest.mark.parametrize("rows", [(3, 0), (3, 2), (2, 2)])
def test_weighted_loss_against_float64(rows, kind, masked, dtype, loss_references):
    case = _loss_case(rows, kind, masked, dtype)
    pred, target, mask, t, table, n_inst, n_prior = case
    loss, dpred = nat.ddpm_mse_weighted_fwd_bwd(pred, target, mask, t, table, n_inst, n_prior, 0.7, GRAD_SCALE)
    want_loss, want_dpred = loss_references(rows, kind, masked, dtype, case)
    assert loss.dtype == torch.float32 and dpred.dtype == dtype and dpred.shape == pred.shape
    loss_err = abs(loss.item() - want_loss.item()) / max(1.0, abs(want_loss.item()))
    dpred_err = rel_err(dpred.float(), want_dpred)
    print(f"\n[weighted loss {rows} {kind} mask={masked} {dtype}] loss err {loss_err:.3g} dpred relerr {dpred_err:.3g}")
    assert loss_err < LOSS_TOL[dtype]
    if dtype in DPRED_TOL:
        assert dpred_err < DPRED_TOL[dtype]
    else:  # bf16: twice what the unweighted kernel leaves on the same prediction, target and mask
        _, plain = nat.ddpm_mse_fwd_bwd(pred, target, mask, n_inst, n_prior, 0.7, GRAD_SCALE)
        _, want_plain = ref.weighted_loss(pred, target, mask, t, torch.ones(T), n_inst, n_prior, 0.7, GRAD_SCALE)
        plain_err = rel_err(plain.float(), want_plain)
        print(f"    unweighted kernel on the same inputs: dpred relerr {plain_err:.3g}; bound {2 * plain_err:.3g}")
        assert 0.0 < plain_err < 2 ** -8  # (itself no worse than one rounding to bf16 per element)
        assert dpred_err <= 2 * plain_err
    row = 2  # t = 500: weight exactly 0 — no gradient, whatever the row holds
    assert float(dpred[row].float().abs().max()) == 0.0
    again, _ = nat.ddpm_mse_weighted_fwd_bwd(pred, target, mask, t, table, n_inst, n_prior, 0.7, GRAD_SCALE)
    assert torch.equal(again, loss)  # the fold is ordered: launches repeat


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", list(SHAPES))
def test_a_table_of_ones_leaves_the_bits_of_the_unweighted_kernel(kind, masked, dtype):
    pred, target, mask, t, _, n_inst, n_prior = _loss_case((3, 2), kind, masked, dtype, seed=1)
    ones = torch.ones(T, device=DEV)
    loss_w, dpred_w = nat.ddpm_mse_weighted_fwd_bwd(pred, target, mask, t, ones, n_inst, n_prior, 0.7, GRAD_SCALE)
    loss_p, dpred_p = nat.ddpm_mse_fwd_bwd(pred, target, mask, n_inst, n_prior, 0.7, GRAD_SCALE)
    assert torch.equal(loss_w, loss_p) and math.isfinite(loss_p.item()) and loss_p.item() > 0.0
    assert torch.equal(dpred_w, dpred_p)
    loss_only, none = nat.ddpm_mse_weighted_fwd_bwd(pred, target, mask, t, ones, n_inst, n_prior, 0.7, GRAD_SCALE, want_grad=False)
    assert none is None and torch.equal(loss_only, loss_p)


@pytest.mark.parametrize("kind", ["vector", "scalar"])
@pytest.mark.parametrize("bad", [T, -1, 2 ** 40])
def test_a_timestep_outside_the_table_poisons_its_row_only(kind, bad):
    pred, target, mask, t, table, n_inst, n_prior = _loss_case((3, 2), kind, True, torch.float32, seed=2)
    loss, dpred = nat.ddpm_mse_weighted_fwd_bwd(pred, target, mask, t, table, n_inst, n_prior, 0.7, GRAD_SCALE)
    assert math.isfinite(loss.item())
    t_bad = t.clone()
    t_bad[1] = bad
    loss_bad, dpred_bad = nat.ddpm_mse_weighted_fwd_bwd(pred, target, mask, t_bad, table, n_inst, n_prior, 0.7, GRAD_SCALE)
    assert math.isnan(loss_bad.item())
    others = [0, 2, 3, 4]
    assert bool(torch.isfinite(dpred_bad[others]).all()) and torch.equal(dpred_bad[others], dpred[others])
    assert bool(torch.isnan(dpred_bad[1]).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,guard", [("vector", 8), ("scalar", 1), ("vector", 1)])
def test_weighted_loss_writes_nothing_outside_dpred(kind, guard, dtype):
    """dpred is a slice of a larger buffer: the elements in front of and behind it keep their sentinel (guard 8 keeps the
    16-byte vector stores, guard 1 forces element stores)."""
    pred, target, mask, t, table, n_inst, n_prior = _loss_case((3, 2), kind, False, dtype, seed=3)
    n = pred.numel()
    buf = torch.full((n + 2 * guard,), 7.0, dtype=dtype, device=DEV)
    dpred = buf[guard:guard + n]
    loss = torch.empty(1, device=DEV)
    ws = nat._workspace(pred.device, int(nat.lib().lora_mse_workspace_bytes()), "mse")
    rc = nat.lib().ddpm_mse_weighted_fwd_bwd(nat._ptr(pred), nat._ptr(target), None, nat._ptr(t), nat._ptr(table), T, n_inst,
                                             n_prior, pred[0].numel(), pred.shape[-1] * pred.shape[-2], 0.7, GRAD_SCALE,
                                             nat._ptr(loss), nat._ptr(dpred), nat._ptr(ws), nat.dtype_code(dtype),
                                             nat._stream(pred))
    assert rc == 0
    _, want = nat.ddpm_mse_weighted_fwd_bwd(pred, target, None, t, table, n_inst, n_prior, 0.7, GRAD_SCALE)
    assert torch.equal(dpred.view(pred.shape), want)
    assert bool((buf[:guard] == 7.0).all()) and bool((buf[guard + n:] == 7.0).all())


# -- the offset prologues -----------------------------------------------------------------------------------------------------
# hw % 4 == 0; vector path with groups straddling channels; element path; rows shorter than a Philox group (a group of four
# elements enters a new row more than once: per_row 3, and per_row 2 with one element per channel)
OFFSET_SHAPES = [(4, 8, 8), (4, 3, 2), (3, 5, 7), (1, 1, 3), (2, 1, 1)]
B, SEED, STEP, OFFSET = 3, 77, 3, 0.1


def _tables():
    return tr.ddpm_tables(device=DEV), orc.ddpm_alphas_cumprod()


def _latents(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, *shape, generator=g) * 0.18215


def _moments(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    C, h, w = shape
    return torch.cat([torch.randn(B, C, h, w, generator=g), torch.randn(B, C, h, w, generator=g) * 2.0 - 3.0], dim=1)


def _check_offset_outputs(shape, v, t, t_plain, eps, eps_plain, xi, x0, noisy, target, acp, relerr=rel_err):
    C = shape[0]
    xi_ref = torch.from_numpy(ref.offset_normals(B, C, SEED, STEP))
    assert xi.shape == (B, C)
    assert float((xi.cpu() - xi_ref).abs().max()) < 2e-5  # libm vs GPU logf/sincosf (test_noise_prologue_matches_philox_oracle)
    assert torch.equal(t, t_plain)  # integer stream: untouched
    # eps' = fmaf(offset, ξ[b, c], eps): one rounding of the exact value, per element with the element's own channel
    exact = eps_plain.double().cpu() + float(np.float32(OFFSET)) * xi.double().cpu()[:, :, None, None]
    ulps = ((eps.double().cpu() - exact).abs() / ref.f32_ulp(exact)).max().item()
    assert ulps <= 1.0, ulps
    assert not torch.equal(eps, eps_plain)
    tt = t.cpu()
    assert relerr(noisy, orc.add_noise(x0.cpu(), eps.cpu(), tt, acp)) < 1e-5
    assert relerr(target, orc.get_velocity(x0.cpu(), eps.cpu(), tt, acp) if v else eps.cpu()) < 1e-5


@pytest.mark.parametrize("v", [False, True])
@pytest.mark.parametrize("shape", OFFSET_SHAPES)
def test_noise_prologue_offset_against_the_philox_oracle_and_the_plain_entry(shape, v):
    (sa, sb), acp = _tables()
    x0 = _latents(shape).to(DEV)
    _, _, t_plain, eps_plain = nat.ddpm_noise_prologue(x0, sa, sb, torch.float32, SEED, STEP, v, want_draw=True)
    noisy, target, t, eps, xi = nat.ddpm_noise_prologue_offset(x0, sa, sb, torch.float32, SEED, STEP, v, noise_offset=OFFSET,
                                                               want_draw=True)
    _check_offset_outputs(shape, v, t, t_plain, eps, eps_plain, xi, x0, noisy, target, acp)


@pytest.mark.parametrize("v", [False, True])
@pytest.mark.parametrize("shape", OFFSET_SHAPES)
def test_posterior_prologue_offset_against_the_philox_oracle_and_the_plain_entry(shape, v):
    (sa, sb), acp = _tables()
    m = _moments(shape).to(DEV)
    plain = nat.ddpm_posterior_prologue(m, sa, sb, torch.float32, SEED, STEP, v, want_draw=True)
    noisy, target, t, x0, z, eps, xi = nat.ddpm_posterior_prologue_offset(m, sa, sb, torch.float32, SEED, STEP, v,
                                                                          noise_offset=OFFSET, want_draw=True)
    assert torch.equal(x0, plain[3]) and torch.equal(z, plain[4])  # the latents' draw is not the offset's business
    _check_offset_outputs(shape, v, t, plain[2], eps, plain[5], xi, x0, noisy, target, acp)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("v", [False, True])
@pytest.mark.parametrize("shape", OFFSET_SHAPES)
def test_offset_zero_leaves_the_bits_of_the_plain_entries(shape, v, dtype):
    (sa, sb), _ = _tables()
    x0 = _latents(shape, 1).to(DEV)
    plain = nat.ddpm_noise_prologue(x0, sa, sb, dtype, SEED, STEP, v, want_draw=True)
    zero = nat.ddpm_noise_prologue_offset(x0, sa, sb, dtype, SEED, STEP, v, noise_offset=0.0, want_draw=True)
    for got, want in zip(zero[:4], plain):
        assert torch.equal(got, want)
    m = _moments(shape, 1).to(DEV).to(dtype)  # (the moments in the compute dtype, as a cache would hold them)
    plain = nat.ddpm_posterior_prologue(m, sa, sb, dtype, SEED, STEP, v, want_draw=True)
    zero = nat.ddpm_posterior_prologue_offset(m, sa, sb, dtype, SEED, STEP, v, noise_offset=0.0, want_draw=True)
    for got, want in zip(zero[:6], plain):
        assert torch.equal(got, want)
    # and the draw-less call (no eps_out / xi_out) gives the same noisy / target / t as the one that copies the draw out
    off = nat.ddpm_noise_prologue_offset(x0, sa, sb, dtype, SEED, STEP, v, noise_offset=OFFSET, want_draw=True)
    bare = nat.ddpm_noise_prologue_offset(x0, sa, sb, dtype, SEED, STEP, v, noise_offset=OFFSET)
    assert all(torch.equal(a, b) for a, b in zip(bare, off[:3]))


# -- the trainers -------------------------------------------------------------------------------------------------------------
def _warm(params, seed, std=0.02):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i, p in enumerate(params):
            if i % 2 == 0:
                p.copy_(torch.randn(p.shape, generator=g).to(p.device) * std)


def _lora_trainer(warm_seed=11, **kw):
    unet = build_tiny_unet(seed=5).to(DEV)
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    _warm(list(itertools.chain(*params)), warm_seed)
    return tr.LoraTrainer(unet, lr=1e-3, **kw), unet


def _feed(s, rows=2):
    lat, _, _, ctx = orc.synthetic_batch(s, rows, 8, 6, 32)
    return dict(latents=lat.to(DEV), seed=41, encoder_hidden_states=ctx.to(DEV))


def test_recorded_steps_with_both_knobs_leave_the_bits_of_host_launched_ones(repeatable_stock_kernels):
    """snr_gamma = 5, noise_offset = 0.1, windows of two micro-batches, three optimizer steps: the recorded step reads the
    weight table through its address and the timesteps from the static buffer the offset draw filled."""
    def run(graph):
        trainer, unet = _lora_trainer(snr_gamma=5.0, noise_offset=0.1, gradient_accumulation_steps=2, capture_graph=graph)
        losses = [trainer.step(**_feed(s)).detach().clone().reshape(()) for s in range(6)]
        assert trainer.opt.step_count == 3
        assert (trainer._graph is not None) == graph  # the recording really exists (no silent host-launched fall-back)
        return tr.flat_lora_state(unet).clone(), torch.stack(losses).cpu()

    state, losses = run(False)
    state_rec, losses_rec = run(True)
    assert bool(torch.isfinite(losses).all())
    assert torch.equal(losses_rec, losses), (losses_rec - losses).abs().max().item()
    assert torch.equal(state_rec, state), (state_rec - state).abs().max().item()
    plain, _ = _lora_trainer(gradient_accumulation_steps=2)
    assert not torch.equal(torch.stack([plain.step(**_feed(s)).detach().reshape(()) for s in range(2)]).cpu(), losses[:2])


def test_timestep_weights_of_one_half_halve_loss_and_gradient_slab_bit_for_bit(repeatable_stock_kernels):
    """fp32, loss scale 1, clipping off: a constant weight of 0.5 is an exact power-of-two scaling of the row coefficients,
    hence of dpred, of everything backward computes from it, and of the loss."""
    lat, noise, ts, ctx = (x.to(DEV) for x in orc.synthetic_batch(0, 2, 8, 6, 32))
    out = []
    for weights in (None, torch.full((T,), 0.5)):
        trainer, _ = _lora_trainer(timestep_weights=weights, loss_scale=1.0, max_grad_norm=0.0)
        loss = trainer.step(lat, noise, ts, ctx)
        out.append((loss.detach().clone(), trainer.slab.grads.clone()))
    (loss_plain, grads_plain), (loss_half, grads_half) = out
    assert float(grads_plain.abs().max()) > 0.0 and math.isfinite(loss_plain.item())
    assert torch.equal(loss_half, 0.5 * loss_plain)
    assert torch.equal(grads_half, 0.5 * grads_plain)


@pytest.mark.parametrize("mode", ["plain", "prior+mask"])
@pytest.mark.parametrize("v_prediction", [False, True])
def test_snr_gamma_with_the_callers_noise_and_timesteps_against_float64(mode, v_prediction):
    """The loss returned equals the float64 weighted loss of the trainer's OWN prediction, re-obtained under no_grad from the
    same inputs before the step.  Bound: the fp32 loss kernel's 2e-6 is for equal predictions; the prediction here comes from
    another launch sequence of the fp32 UNet than the training forward, which the project's host-launched-against-recorded
    check allows 2e-5 on the loss (test_hipgraph_step_matches_eager_step) — that bound is used."""
    rows = 4 if mode != "plain" else 2
    lat, noise, _, ctx = (x.to(DEV) for x in orc.synthetic_batch(3, rows, 8, 6, 32))
    ts = torch.tensor([10, 600, 100, 900][:rows], dtype=torch.int64, device=DEV)  # SNR above and below γ
    raw = None
    if mode != "plain":
        raw = (torch.rand(rows, 1, 64, 64, generator=torch.Generator().manual_seed(9)) > 0.6).float().to(DEV)
    trainer, unet = _lora_trainer(snr_gamma=5.0, v_prediction=v_prediction)
    table = stp.min_snr_weights(tr.ddpm_alphas_cumprod(), 5.0, v_prediction)
    assert torch.equal(trainer.loss_weights.cpu(), table) and trainer.loss_weights.is_cuda
    noisy, target = nat.ddpm_add_noise(lat, noise, ts, trainer.sqrt_acp, trainer.sqrt_1macp, torch.float32, v_prediction)
    with torch.no_grad():
        pred = unet(noisy, ts, ctx).sample
    m = nat.lora_mask_prepare(raw, 8, 8) if raw is not None else None
    n_inst, n_prior = (rows // 2, rows // 2) if mode != "plain" else (rows, 0)
    want, _ = ref.weighted_loss(pred, target, m, ts, table, n_inst, n_prior, 0.7)
    unweighted, _ = ref.weighted_loss(pred, target, m, ts, torch.ones(T), n_inst, n_prior, 0.7)
    loss = trainer.step(lat, noise, ts, ctx, with_prior_preservation=mode != "plain", prior_loss_weight=0.7, mask=raw)
    err = abs(loss.item() - want.item()) / abs(want.item())
    print(f"\n[snr_gamma, caller's noise, {mode}, v={v_prediction}] loss {loss.item():.6g} float64 {want.item():.6g} err {err:.3g}")
    assert err < 2e-5
    assert abs(unweighted.item() - want.item()) / abs(want.item()) > 1e-3  # the weights matter at these timesteps


@pytest.mark.parametrize("graph", [False, True])
def test_a_checkpoint_after_step_two_continues_the_weighted_offset_run_bit_for_bit(tmp_path, graph, repeatable_stock_kernels):
    kw = dict(snr_gamma=5.0, noise_offset=0.1, capture_graph=graph)
    straight, _ = _lora_trainer(**kw)
    want = [straight.step(**_feed(s)).detach().clone().reshape(()) for s in range(4)]
    first, _ = _lora_trainer(**kw)
    for s in range(2):
        first.step(**_feed(s))
    path = tmp_path / "objective.safetensors"
    first.save_checkpoint(path)
    resumed, _ = _lora_trainer(warm_seed=99, **kw)  # (other factors: whatever the load does not restore shows)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        resumed.load_checkpoint(path)
    assert not [w for w in caught if "other arguments" in str(w.message)]  # same arguments: nothing to report
    got = [resumed.step(**_feed(s)).detach().clone().reshape(()) for s in range(2, 4)]
    assert (resumed._graph is not None) == graph
    for s, (a, b) in enumerate(zip(got, want[2:]), start=2):
        assert torch.equal(a, b), (s, a.item(), b.item())
    assert torch.equal(resumed.slab.params, straight.slab.params)
    assert torch.equal(resumed.opt.exp_avg, straight.opt.exp_avg) and torch.equal(resumed.opt.exp_avg_sq, straight.opt.exp_avg_sq)
    other, _ = _lora_trainer(snr_gamma=1.0, noise_offset=0.1)
    with pytest.warns(UserWarning, match="snr_gamma: checkpoint 5.0, trainer 1.0"):
        other.load_checkpoint(path)
    cfg = first.state_dict()["meta"]["config"]
    assert (cfg["snr_gamma"], cfg["timestep_weights"], cfg["noise_offset"]) == (5.0, None, 0.1)
    assert first.state_dict()["meta"]["format_version"] == 1


def test_inversion_step_with_both_knobs_is_finite_and_differs_from_the_plain_step():
    from tests.test_inversion_host import _tiny_models

    g = torch.Generator().manual_seed(4)
    lat = (torch.randn(2, 4, 8, 8, generator=g) * 0.18215).to(DEV)
    ids = torch.randint(3, 50, (2, 8), generator=g)
    ids[:, 2] = 55
    losses = []
    for kw in ({}, dict(snr_gamma=5.0, noise_offset=0.1), dict(snr_gamma=5.0, noise_offset=0.1, capture_graph=True)):
        unet, te = _tiny_models()
        trainer = InversionTrainer(unet.to(DEV), te.to(DEV), [55], accum_iter=1, **kw)
        losses.append(trainer.step(lat, input_ids=ids.to(DEV), seed=3).detach().clone().reshape(()))
        assert (trainer._graph is not None) == bool(kw.get("capture_graph"))
        assert bool(torch.isfinite(te.get_input_embeddings().weight[55]).all())  # (the step's AdamW moved a finite row)
        trainer.close()
    plain, knobs, knobs_recorded = (float(l) for l in losses)
    assert all(math.isfinite(l) for l in (plain, knobs, knobs_recorded))
    assert knobs != plain and abs(knobs_recorded - knobs) <= 2e-5 * abs(knobs)
