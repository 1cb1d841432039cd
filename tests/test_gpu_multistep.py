"""The multistep sampling methods on the device: ddpm_sample_multistep against the stateful float64 PLMS / DPM-Solver++(2M) of
tests/multistep_reference.py at the layout edges and at every order of the history, the 4-element against the element-by-element
path, a warm-up over NaN-filled history, the out-of-range cursor, whole chains with a linear stand-in denoiser, and LatentSampler
with method="plms" on the harness UNet — replayed against host-launched and next to a recording LoraTrainer.

Every iteration is judged from the DEVICE's own previous state, saved state and ring, read back exactly into float64: no error
is carried from one iteration to the next.  The bound (`_judge`): x' takes fewer than twenty fp32 roundings of 6e-8 each, on
partial sums no larger than Σ|terms| = |a·base| + |c0|·(|p·x| + |q·o|) + Σ|c_k·H[s_k]| with |q|·(|u| + g·|c − u|) standing for
|q·o| (guidance is computed in fp32 too): 1e-5 of that sum's maximum — the ×10 margin of sampling_reference.state_bound, taken
over the term sum and not the result, because PLMS's weights cancel.  The pushed slot h = p·x + q·o likewise against
|p·x| + |q·o|.  The model input is the kernel's fp32 state cast once, bit for bit."""
import itertools

import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import trainer as tr
from oracle import lora_oracle as orc
from tests import multistep_reference as ref
from tests import sampling_reference as sr
from tests import test_gpu_sampling as tgs
from tests.conftest import build_tiny_unet

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 256), (3, 37), (2, 4 * 8 * 8)]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# (method, S, iteration): plms at every order and one wrapped push (S = 8: I = 9, iteration 6 pushes slot 1 a second time);
# dpmpp_2m's first, a middle and the last (second order at S = 20, the lower-order final at S = 5)
S_PLMS, S_DPM = 8, 20
ITERATIONS = [("plms", S_PLMS, i) for i in (0, 1, 2, 3, 6)] + [("dpmpp_2m", S_DPM, i) for i in (0, 10, 19)] + [("dpmpp_2m", 5, 4)]
GUIDANCE = 5.0


@pytest.fixture(autouse=True)
def _collect_garbage_first():
    """A recording left in a reference cycle by an earlier test must not be destroyed in the middle of another capture."""
    import gc

    gc.collect()


def _state(B, per_row, dtype, cfg, method, S, v, shifted=False, data_seed=0, poison=False):
    """A MultistepState whose x, xs, ring and model output hold random data (NaN in xs and the ring: `poison`); (state, model
    output on the device)."""
    ts, coef, plan = dfa.multistep_schedule(method, S, v)
    g = torch.Generator().manual_seed(data_seed)
    rows = 2 * B if cfg else B
    x, xs, hist = torch.randn(B, per_row, generator=g), torch.randn(B, per_row, generator=g), torch.randn(4, B, per_row, generator=g)
    out = torch.randn(rows, per_row, generator=g).to(dtype)
    if poison:
        xs.fill_(float("nan"))
        hist.fill_(float("nan"))
    place = (lambda t: tgs._shifted(t.to(DEV))) if shifted else (lambda t: t.to(DEV))
    st = nat.MultistepState(place(x), place(xs), place(hist), place(torch.zeros(rows, per_row, dtype=dtype)),
                            place(torch.zeros(rows, dtype=torch.int64)), place(torch.zeros(2, dtype=torch.int32)), place(ts),
                            place(coef), place(plan), cfg)
    return st, place(out)


def _snapshot(st):
    return {"x": st.x.cpu(), "xs": st.xs.cpu(), "hist": st.hist.cpu(), "model_in": st.model_in.cpu(), "t_model": st.t_model.cpu()}


def _judge(before, st, out, method, S, v, i, cfg, dtype, what, guidance=GUIDANCE):
    """The state after iteration i against the reference resumed from `before` (the device's buffers before the launch) and the
    model output `out`: x', the pushed slot and xs within bound / bit for bit, every other slot untouched, the next model input
    and timestep tensor.  Returns the measured error of x'."""
    x, xs, hist = before["x"].double(), before["xs"].double(), before["hist"].double()
    _, coef, plan = dfa.multistep_schedule(method, S, v, coef_dtype=torch.float64)  # (magnitudes of the bound only)
    n_it, flags, w = plan.shape[0], int(plan[i, 4]), int(plan[i, 0])
    solver = ref.SOLVERS[method](S, v)
    slots = ref.ring_slots(plan, i)
    known = min(solver.pushes_before(i), 3)
    assert all(slots[k - 1] is not None for k in range(1, known + 1))
    solver.resume(i, [hist[slots[k - 1]] for k in range(known, 0, -1)], saved=xs if flags & ref.USE_SAVED else None)
    o = sr.guided(out.cpu(), guidance, cfg)
    want = solver.step(x, o)
    # Σ|terms|
    outd = out.cpu().double()
    o_abs = outd[:x.shape[0]].abs() + guidance * (outd[x.shape[0]:] - outd[:x.shape[0]]).abs() if cfg else outd.abs()
    p, q, a, c0 = (float(c) for c in coef[i, :4])
    h_terms = (p * x).abs() + abs(q) * o_abs
    terms = (a * (xs if flags & ref.USE_SAVED else x)).abs() + abs(c0) * h_terms
    for k in (1, 2, 3):
        if float(coef[i, 3 + k]) != 0.0:
            terms = terms + (float(coef[i, 3 + k]) * hist[int(plan[i, k])]).abs()
    bound = 1e-5 * float(terms.max())
    after = _snapshot(st)
    err = float((after["x"].double() - want).abs().max())
    print(f"\n[{what} {method} S {S} v {v} i {i} {dtype} cfg {cfg} {tuple(x.shape)}] state err {err:.3g} (bound {bound:.3g})", end="")
    assert bool(torch.isfinite(after["x"]).all()) and err <= bound
    for slot in range(4):
        if flags & ref.PUSH and slot == w:
            h_want = o if method == "plms" else solver.history[-1]
            h_err, h_bound = float((after["hist"][slot].double() - h_want).abs().max()), 1e-5 * float(h_terms.max())
            print(f"  pushed slot {slot} err {h_err:.3g} (bound {h_bound:.3g})", end="")
            assert h_err <= h_bound
        else:
            assert torch.equal(tgs._bits(after["hist"][slot]), tgs._bits(before["hist"][slot])), slot
    # xs: the state BEFORE the update where the plan saves it, else untouched — bit for bit
    assert torch.equal(tgs._bits(after["xs"]), tgs._bits(before["x"] if flags & ref.SAVE else before["xs"]))
    B = x.shape[0]
    assert torch.equal(after["model_in"][:B], after["x"].to(dtype))  # the state cast once
    sr.check_model_input(st.model_in, want, dtype, cfg, slack=bound)  # (both halves bit-identical under guidance)
    assert after["t_model"].tolist() == [solver.timesteps[min(i + 1, n_it - 1)]] * (2 * B if cfg else B)
    return err


def _one_step(B, per_row, dtype, cfg, method, S, v, i, shifted=False, seed=41):
    st, out = _state(B, per_row, dtype, cfg, method, S, v, shifted=shifted)
    tgs._set_cursor(st, i, seed)
    before = _snapshot(st)
    nat.ddpm_sample_multistep(st, out, GUIDANCE)
    return st, out, before


@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,per_row", SHAPES)
def test_step_against_float64(B, per_row, dtype, cfg):
    for (method, S, i), v in itertools.product(ITERATIONS, (False, True)):
        st, out, before = _one_step(B, per_row, dtype, cfg, method, S, v, i)
        _judge(before, st, out, method, S, v, i, cfg, dtype, "multistep step")
        assert st.cursor.cpu().tolist() == [i, 41]  # the step does not move its cursor
        if method == "plms" and i == 1:  # the repeated timestep: iteration 1 leaves its own for iteration 2
            assert st.t_model.cpu().tolist()[0] == ref.Plms(S, v).timesteps[1]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_step_with_every_operand_one_element_off_alignment(dtype):
    """The element-by-element path on a shape the 4-element path would take: the same bits in x, the ring, xs and the model
    input — and within bound of the reference."""
    B, per_row = 2, 256
    for method, S, i in (("plms", S_PLMS, 0), ("plms", S_PLMS, 1), ("plms", S_PLMS, 6), ("dpmpp_2m", S_DPM, 10)):
        sh, out, before = _one_step(B, per_row, dtype, True, method, S, False, i, shifted=True)
        assert sh.x.data_ptr() % 16 != 0 and sh.xs.data_ptr() % 16 != 0 and sh.hist.data_ptr() % 16 != 0
        assert sh.model_in.data_ptr() % 8 != 0 and out.data_ptr() % 8 != 0
        _judge(before, sh, out, method, S, False, i, True, dtype, "multistep off alignment")
        al, _, _ = _one_step(B, per_row, dtype, True, method, S, False, i)
        a, b = _snapshot(sh), _snapshot(al)
        assert all(torch.equal(tgs._bits(a[k]), tgs._bits(b[k])) for k in a), [k for k in a if not torch.equal(a[k], b[k])]


@pytest.mark.parametrize("method,S", [("plms", S_PLMS), ("dpmpp_2m", S_DPM)])
@pytest.mark.parametrize("B,per_row,shifted", [(2, 256, False), (3, 37, False), (2, 256, True)])
def test_warm_up_over_poisoned_history(method, S, B, per_row, shifted):
    """xs and every history slot hold NaN before iteration 0: a coefficient of exactly 0 keeps them unread, so the state stays
    finite and within bound through iteration 5 (plms: every order, the first wrapped push)."""
    st, _ = _state(B, per_row, torch.float16, True, method, S, False, shifted=shifted, poison=True)
    tgs._set_cursor(st, 0, 3)
    g = torch.Generator().manual_seed(17)
    for i in range(6):
        out = torch.randn(2 * B, per_row, generator=g).half().to(DEV)
        if shifted:
            out = tgs._shifted(out)
        before = _snapshot(st)
        nat.ddpm_sample_multistep(st, out, GUIDANCE)
        nat.ddpm_sample_advance(st)
        _judge(before, st, out, method, S, False, i, True, torch.float16, "poisoned warm-up")
        assert st.cursor.cpu().tolist()[0] == i + 1


@pytest.mark.parametrize("shifted", [False, True])
def test_a_launch_with_the_cursor_out_of_range_changes_nothing(shifted):
    n_it = S_PLMS + 1
    for cursor in (n_it, n_it + 3, -1):
        st, out = _state(3, 37, torch.bfloat16, True, "plms", S_PLMS, False, shifted=shifted)
        st.model_in.fill_(3.0)
        st.t_model.fill_(-5)
        tgs._set_cursor(st, cursor, 9)
        before = _snapshot(st)
        nat.ddpm_sample_multistep(st, out, GUIDANCE)
        nat.ddpm_sample_advance(st)
        after = _snapshot(st)
        assert all(torch.equal(tgs._bits(after[k]), tgs._bits(before[k])) for k in before)
        assert st.cursor.cpu().tolist()[0] == cursor


# -- whole chains ----------------------------------------------------------------------------------------------------------------
class _Out:
    def __init__(self, sample):
        self.sample = sample


class LinearDenoiser(torch.nn.Module):
    """out = w·x + c[t] + 0.1·mean(context), fp32: depends on the state, the timestep and the conditioning row."""

    def __init__(self, w):
        super().__init__()
        self.w = torch.nn.Parameter(torch.full((1, 1, 1, 1), float(w)), requires_grad=False)  # (4-d: names the compute dtype)
        self.register_buffer("c", torch.linspace(-0.5, 0.5, 1000))

    def forward(self, x, t, ctx):
        return _Out(self.w * x + self.c[t].view(-1, 1, 1, 1) + 0.1 * ctx.mean(dim=(1, 2)).view(-1, 1, 1, 1))


def _flat(snapshot, B):
    return {k: (v.reshape(4, B, -1) if k == "hist" else v.reshape(v.shape[0], -1) if v.dim() > 1 else v) for k, v in snapshot.items()}


@pytest.mark.parametrize("method,S", [("plms", 6), ("dpmpp_2m", 5)])  # plms: I = 7, all four orders and one ring wrap
@pytest.mark.parametrize("capture", [True, False])
def test_chain_with_a_linear_denoiser(capture, method, S):
    """After each iteration the expected state follows from the sampler's PREVIOUS state, saved state and ring by the test's
    own forward of the same module on the same input: nothing is compared across iterations."""
    B, shape, seed = 2, (4, 8, 8), 123
    n_it = ref.evaluations(method, S)
    model = LinearDenoiser(0.9).to(DEV)
    gen = torch.Generator().manual_seed(3)
    cond, neg = torch.randn(B, 6, 32, generator=gen), torch.randn(B, 6, 32, generator=gen)
    sampler = dfa.LatentSampler(model, num_inference_steps=S, guidance_scale=GUIDANCE, method=method, capture_graph=capture)
    assert sampler.num_inference_steps == S and sampler.num_model_evaluations == n_it == sampler.timesteps.shape[0]
    sampler.begin(cond.to(DEV), neg.to(DEV), seed=seed, latent_shape=shape)
    assert sampler.replaying == capture
    st = sampler.state
    assert isinstance(st, nat.MultistepState) and st.cursor.cpu().tolist() == [0, seed]
    assert float((st.x.cpu().reshape(B, -1) - sr.init_normals(B, 256, seed)).abs().max()) <= sr.Z_TOL  # the oracle's x_T
    more = True
    for i in range(n_it):
        assert more
        before = _flat(_snapshot(st), B)
        with torch.no_grad():
            out = model(st.model_in.clone(), st.t_model.clone(), sampler.conditioning).sample.reshape(2 * B, -1)
        more = sampler.step()
        flat = nat.MultistepState(st.x.view(B, -1), st.xs.view(B, -1), st.hist.view(4, B, -1), st.model_in.view(2 * B, -1),
                                  st.t_model, st.cursor, st.timesteps, st.coef, st.plan, True)
        _judge(before, flat, out, method, S, False, i, True, torch.float32, f"linear chain capture {capture}")
        assert st.cursor.cpu().tolist() == [i + 1, seed]
    assert more is False and st.cursor.cpu().tolist() == [n_it, seed]
    before = _snapshot(st)
    assert sampler.step() is False  # a further step launches nothing
    after = _snapshot(st)
    assert all(torch.equal(tgs._bits(after[k]), tgs._bits(before[k])) for k in before) and st.cursor.cpu().tolist() == [n_it, seed]


# -- on the harness UNet -----------------------------------------------------------------------------------------------------------
SHAPE, S_UNET = (4, 8, 8), 4


def test_plms_on_the_harness_unet_replayed_equals_host_launched():
    """f16, 4 UNet rows (the forward is run-to-run deterministic there): one recording serves all I = S + 1 iterations and
    every seed."""
    unet = tgs._harness_unet()
    cond, neg = tgs._conditioning()
    host = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method="plms", capture_graph=False)
    want = host.sample(cond, neg, seed=5, latent_shape=SHAPE).cpu()
    assert not host.replaying
    sampler = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method="plms")
    seen = []
    first = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE, callback=lambda i, t, x: seen.append((i, t))).cpu()
    timesteps = ref.Plms(S_UNET, False).timesteps
    assert len(timesteps) == S_UNET + 1 == sampler.num_model_evaluations and timesteps[1] == timesteps[2]
    assert sampler.replaying and seen == list(enumerate(timesteps))
    assert first.dtype == torch.float32 and tuple(first.shape) == (2, *SHAPE) and bool(torch.isfinite(first).all())
    assert torch.equal(first, want)
    other = sampler.sample(cond, neg, seed=6, latent_shape=SHAPE).cpu()  # the same recording: the seed lives in device memory
    again = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE).cpu()
    assert torch.equal(again, first) and not torch.equal(other, first)
    ddpm = dfa.LatentSampler(unet, num_inference_steps=S_UNET, capture_graph=False).sample(cond, neg, seed=5, latent_shape=SHAPE)
    assert not torch.equal(ddpm.cpu(), first)  # another method from the same x_T


def _train(sample_after=None):
    unet = build_tiny_unet(seed=5).to(DEV).to(torch.float16)
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    tgs._warm(list(itertools.chain(*params)), 11, 0.02)
    trainer = tr.LoraTrainer(unet, lr=1e-3, capture_graph=True)
    cond, neg = tgs._conditioning()
    sampler = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method="plms")
    losses = []
    for k in range(4):
        losses.append(trainer.step(*(x.to(DEV) for x in orc.synthetic_batch(k, 4, 8, 6, 32))))
        if sample_after is not None and k + 1 in sample_after:
            tensors, host = tgs._trainer_buffers(trainer)
            before = {name: tgs._bits(t).clone() for name, t in tensors.items()}
            sample = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE)
            assert sampler.replaying and unet.training and bool(torch.isfinite(sample).all())
            tensors, host_after = tgs._trainer_buffers(trainer)  # sample() wrote nothing the trainer owns, bit for bit
            assert host_after == host and all(torch.equal(before[name], tgs._bits(t)) for name, t in tensors.items())
    assert trainer._graph is not None
    return tr.flat_lora_state(unet).cpu(), torch.stack(losses).reshape(-1).cpu()


def test_plms_sampling_between_steps_leaves_a_recording_trainer_alone():
    """Two recorded 4-step runs of the f16 tiny UNet on 4-row batches, one of which samples with plms after steps 2 and 4: the
    final LoRA state and the losses are bit-identical, and every buffer and counter the trainer owns is the same before and
    after each sample()."""
    plain_state, plain_losses = _train()
    state, losses = _train(sample_after=(2, 4))
    assert bool(torch.isfinite(state).all()) and torch.equal(state, plain_state) and torch.equal(losses, plain_losses)
