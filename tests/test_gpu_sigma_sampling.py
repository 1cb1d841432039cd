"""The sigma-space sampler on the device: ddpm_sample_sigma / ddpm_sample_sigma_init against the stateful float64 samplers of
tests/sigma_reference.py and the Philox oracle at the layout edges, whole chains with a linear stand-in denoiser that takes
fractional timesteps, keep mask / image-to-image / shared noise on it, and LatentSampler("k_euler" / "euler_a" / "heun") on the
harness UNet — replayed against host-launched, after LoRA edits, under per-sample gates.

The per-step bound is the project's `sampling_reference.state_bound` with the step's noise scale s in place of σ: 1e-5 of the
largest reference value plus s·2e-5 for the libm-against-device difference of z.  The model input is the kernel's own fp32
state times n, rounded once in fp32 and cast once — asserted bit for bit from the device's state."""
import itertools
import math

import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import trainer as tr
from tests import sampling_reference as ref
from tests import sigma_reference as sr
from tests.conftest import rel_err
from tests.test_gpu_sampling import FP32_TOL, S_UNET, SHAPE, _conditioning, _harness_unet, _same, _set_cursor, _shifted

pytestmark = pytest.mark.gpu
DEV = "cuda"
S_STEP = 50
SHAPES = [(1, 256), (3, 37), (2, 4 * 8 * 8)]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
METHODS = ("euler", "euler_a", "heun")  # sigma_schedule's and the reference's names
SAMPLER_NAME = {"euler": "k_euler", "euler_a": "euler_a", "heun": "heun"}  # LatentSampler's: "euler" stays an unknown method there
SEED = 41
# (method, v-prediction, iteration): first, middle and last; for Heun a stage B (odd) and a stage A (even) in the middle
CASES = [(m, v, i) for m, v in (("euler_a", False), ("euler_a", True), ("euler", False), ("euler", True))
         for i in (0, S_STEP // 2, S_STEP - 1)] + \
        [("heun", v, i) for v in (False, True) for i in (0, S_STEP - 1, S_STEP, 2 * S_STEP - 2)]


@pytest.fixture(autouse=True)
def _collect_garbage_first():
    """A recording left in a reference cycle by an earlier test must not be destroyed in the middle of another capture."""
    import gc

    gc.collect()


def _place(shifted):
    return (lambda t: _shifted(t.to(DEV))) if shifted else (lambda t: t.to(DEV))


def _state(B, per_row, dtype, cfg, method, v, i, S=S_STEP, shifted=False, karras=False, hw=None):
    """A SigmaState at iteration i on random data.  Before a Heun stage B `xs` and `hist` hold known data, before every other
    iteration NaN (they are uninitialised memory there).  (state, model_out, host copies: x, out, xs, hist, tables)."""
    ts, sigmas, coef, plan = dfa.sigma_schedule(method, S, v, karras_sigmas=karras)
    g = torch.Generator().manual_seed(7 * i + B)
    rows = 2 * B if cfg else B
    scale = max(1.0, float(coef[i, 7]))
    x = torch.randn(B, per_row, generator=g) * scale
    out = torch.randn(rows, per_row, generator=g).to(dtype)
    stage_b = bool(int(plan[i, 4]) & 4)
    xs = torch.randn(B, per_row, generator=g) * scale if stage_b else torch.full((B, per_row), float("nan"))
    hist = torch.randn(B, per_row, generator=g) if stage_b else torch.full((B, per_row), float("nan"))
    place = _place(shifted)
    init = mask = keep = None
    if hw:
        init, mask = torch.randn(B, per_row, generator=g), torch.rand(B, hw, generator=g)
        keep = dfa.sampling.sigma_keep_schedule(coef)
    st = nat.SigmaState(place(x), place(xs), place(hist), place(torch.zeros(rows, per_row, dtype=dtype)),
                        place(torch.full((rows,), -5.0)), place(torch.zeros(2, dtype=torch.int32)), place(ts.float()),
                        place(coef), place(plan), cfg, None if init is None else place(init),
                        None if mask is None else place(mask), None if keep is None else place(keep))
    _set_cursor(st, i, SEED)
    return st, place(out), dict(x=x, out=out, xs=xs, hist=hist, ts=ts, coef=coef, plan=plan, init=init, mask=mask, keep=keep)


def _reference_at(method, v, i, host, S=S_STEP, karras=False):
    """The stateful float64 sampler positioned at iteration i, a Heun stage B with the known saved sample and derivative."""
    smp = sr.make(method, S, v, karras)
    if method == "heun":
        smp.i = i // 2
        if i % 2 == 1:
            smp.sample, smp.d1 = host["xs"].double(), host["hist"].double()
    else:
        smp.i = i
    return smp


def _one_step(B, per_row, dtype, cfg, method, v, i, shifted=False, guidance=5.0):
    st, out_dev, host = _state(B, per_row, dtype, cfg, method, v, i, shifted=shifted)
    z_out = torch.full((B, per_row), 7.0, device=DEV)
    if shifted:
        z_out = _shifted(z_out)
    nat.ddpm_sample_sigma(st, out_dev, guidance, z_out=z_out)
    return st, z_out.cpu(), host


@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,per_row", SHAPES)
def test_step_against_float64(B, per_row, dtype, cfg):
    for method, v, i in CASES:
        st, z, host = _one_step(B, per_row, dtype, cfg, method, v, i)
        coef, plan, ts = host["coef"], host["plan"], host["ts"]
        n_it, flags, s = ts.shape[0], int(plan[i, 4]), float(coef[i, 5])
        smp = _reference_at(method, v, i, host)
        assert abs(smp.model_sigma - float(coef[i, 7])) <= 1e-6 * smp.model_sigma and bool(flags & 4) == (method == "heun" and i % 2 == 1)
        z_ref = ref.step_normals(B, per_row, SEED, i) if s != 0.0 else torch.zeros(B, per_row)
        d_z = float((z - z_ref).abs().max())
        o = ref.guided(host["out"], 5.0, cfg)
        d_ref = smp.to_d(host["x"].double(), o, smp.model_sigma)
        want = smp.step(host["x"], o, z_ref)
        got = st.x.cpu()
        err, bound = float((got.double() - want).abs().max()), ref.state_bound(want, s)
        print(f"\n[sigma step {method} v {v} i {i} flags {flags} {dtype} cfg {cfg} {B}x{per_row}] |z - oracle| {d_z:.3g}  "
              f"state err {err:.3g} (bound {bound:.3g})")
        assert bool(torch.isfinite(got).all())  # NaN in xs / H before their first use never reaches the state
        assert d_z <= ref.Z_TOL and (s != 0.0 or not z.any())
        assert err <= bound
        n32 = coef[i, 6]  # fp32
        assert torch.equal(st.model_in.cpu()[:B], (got * n32).to(dtype))  # fp32(n·x) cast once
        if cfg:
            assert torch.equal(st.model_in.cpu()[B:], st.model_in.cpu()[:B])
        t_next = ts.float()[min(i + 1, n_it - 1)]
        assert st.t_model.dtype == torch.float32 and torch.equal(st.t_model.cpu(), t_next.expand(2 * B if cfg else B))
        assert st.cursor.cpu().tolist() == [i, SEED]  # the step does not move its cursor
        # SAVE / PUSH: the state before the update and this iteration's d; otherwise xs / H are left as they were
        xs, hist = st.xs.cpu(), st.hist.cpu()
        if flags & 2:
            assert torch.equal(xs, host["x"])
        else:
            assert torch.equal(xs.view(torch.int32), host["xs"].view(torch.int32))
        if flags & 1:
            assert float((hist.double() - d_ref).abs().max()) <= ref.state_bound(d_ref, 0.0)
        else:
            assert torch.equal(hist.view(torch.int32), host["hist"].view(torch.int32))
    assert float(ts[1]) != round(float(ts[1]))  # the grid under test is fractional


def test_step_with_every_operand_one_element_off_alignment():
    """The element-by-element path on a shape the 4-element path would take: same draw and same state, bit for bit."""
    B, per_row = 2, 256
    for dtype, (method, v, i) in itertools.product((torch.float16, torch.float32),
                                                   (("euler_a", False, S_STEP // 2), ("heun", True, S_STEP - 1), ("heun", False, 0))):
        st, z, host = _one_step(B, per_row, dtype, True, method, v, i, shifted=True)
        assert st.x.data_ptr() % 16 != 0 and st.model_in.data_ptr() % 8 != 0 and st.hist.data_ptr() % 16 != 0
        al, z_al, _ = _one_step(B, per_row, dtype, True, method, v, i)
        assert al.x.data_ptr() % 16 == 0
        assert torch.equal(z, z_al) and torch.equal(st.x.cpu(), al.x.cpu()) and torch.equal(st.model_in.cpu(), al.model_in.cpu())
        assert torch.equal(st.t_model.cpu(), al.t_model.cpu())
        for a, b in ((st.xs, al.xs), (st.hist, al.hist)):
            assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))
        assert bool(torch.isfinite(st.x).all())


@pytest.mark.parametrize("B,per_row,hw,dtype,cfg,shifted", [(3, 37, 37, torch.float16, True, False), (2, 256, 64, torch.float32, False, False),
                                                             (2, 256, 64, torch.bfloat16, True, True), (2, 24, 6, torch.float32, True, False)])
def test_keep_blend_on_the_sigma_step(B, per_row, hw, dtype, cfg, shifted):
    """The keep instantiation: x = fp32(m·y) + fp32((1−m)·x'), y = fp32(init) + fp32(σ_next·ε), on the plain entry's own x' —
    bit for bit from the device's own results (the plain launch, the start draw)."""
    for method, v, i in (("euler_a", False, 3), ("heun", True, S_STEP - 1), ("heun", False, 2 * S_STEP - 2)):
        st, out_dev, host = _state(B, per_row, dtype, cfg, method, v, i, hw=hw, shifted=shifted)
        plain, out_plain, _ = _state(B, per_row, dtype, cfg, method, v, i)
        nat.ddpm_sample_sigma(plain, out_plain, 5.0)
        eps = torch.empty(B, per_row, device=DEV)
        scratch, _, _ = _state(B, per_row, dtype, cfg, method, v, i)
        nat.ddpm_sample_sigma_init(scratch, SEED, 0, 0.0, 1.0, 1.0, eps_out=eps)
        assert float((eps.cpu() - ref.init_normals(B, per_row, SEED)).abs().max()) <= ref.Z_TOL
        nat.ddpm_sample_sigma(st, out_dev, 5.0, keep=True)
        k, nn = host["keep"][i]
        m = host["mask"].view(B, 1, hw).expand(B, per_row // hw, hw).reshape(B, per_row)
        y = host["init"] * k + eps.cpu() * nn
        want = m * y + (1.0 - m) * plain.x.cpu()
        assert torch.equal(st.x.cpu(), want)
        assert torch.equal(st.model_in.cpu()[:B], (want * host["coef"][i, 6]).to(dtype))
        assert float(nn) == (0.0 if i == host["ts"].shape[0] - 1 else float(host["coef"][i + 1, 7]))


@pytest.mark.parametrize("B,per_row,dtype,cfg,shifted", [(3, 37, torch.float16, True, False), (2, 256, torch.bfloat16, False, False),
                                                          (2, 256, torch.float32, True, True)])
def test_init(B, per_row, dtype, cfg, shifted):
    rows = 2 * B if cfg else B
    for method, start in (("euler_a", 1), ("heun", 2)):
        st, _, host = _state(B, per_row, dtype, cfg, method, False, 0, S=4, shifted=shifted, hw=per_row)
        ts, sigmas = host["ts"], dfa.sigma_schedule(method, 4, False)[1]
        # text-to-image: x_T = σ₀·z
        s0 = float(sigmas[0])
        c_in = 1.0 / math.sqrt(s0 * s0 + 1.0)
        nat.ddpm_sample_sigma_init(st, 77, 0, 0.0, s0, c_in)
        x = st.x.cpu()
        d = float((x.double() - s0 * ref.init_normals(B, per_row, 77).double()).abs().max())
        print(f"\n[sigma init {method} {B}x{per_row} {dtype}] |x_T - σ₀·oracle| {d:.3g} (bound {ref.Z_TOL * s0:.3g})")
        assert d <= ref.Z_TOL * s0
        assert torch.equal(st.model_in.cpu(), (x * torch.tensor(c_in, dtype=torch.float32)).to(dtype).repeat(rows // B, 1))
        assert torch.equal(st.t_model.cpu(), ts.float()[0].expand(rows)) and st.cursor.cpu().tolist() == [0, 77]
        # from an image at a start row: x = fp32(init) + fp32(σ·ε)
        sg = float(sigmas[1])
        assert abs(sg - float(host["coef"][start, 7])) <= 1e-6 * sg
        c_in = 1.0 / math.sqrt(sg * sg + 1.0)
        eps = torch.full((B, per_row), 7.0, device=DEV)
        if shifted:
            eps = _shifted(eps)
        nat.ddpm_sample_sigma_init(st, 78, start, 1.0, sg, c_in, from_init=True, eps_out=eps)
        x = st.x.cpu()
        assert float((eps.cpu() - ref.init_normals(B, per_row, 78)).abs().max()) <= ref.Z_TOL
        assert torch.equal(x, host["init"] + eps.cpu() * torch.tensor(sg, dtype=torch.float32))
        want = host["init"].double() + sg * ref.init_normals(B, per_row, 78).double()
        assert float((x.double() - want).abs().max()) <= ref.Z_TOL * sg
        assert torch.equal(st.model_in.cpu(), (x * torch.tensor(c_in, dtype=torch.float32)).to(dtype).repeat(rows // B, 1))
        assert torch.equal(st.t_model.cpu(), ts.float()[start].expand(rows)) and st.cursor.cpu().tolist() == [start, 78]
        if not shifted:  # the draw again, on the other access path
            sh, _, _ = _state(B, per_row, dtype, cfg, method, False, 0, S=4, shifted=True, hw=per_row)
            sh.init.copy_(st.init)
            nat.ddpm_sample_sigma_init(sh, 78, start, 1.0, sg, c_in, from_init=True)
            assert torch.equal(sh.x.cpu(), x) and torch.equal(sh.model_in.cpu(), st.model_in.cpu())


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("shifted", [False, True])
def test_a_launch_past_the_last_iteration_changes_nothing(shifted, keep):
    n_it = 2 * S_STEP - 1
    for cursor in (n_it, n_it + 3, -1):
        st, out_dev, host = _state(3, 37, torch.bfloat16, True, "heun", False, 1, shifted=shifted, hw=37 if keep else None)
        st.model_in.fill_(3.0)
        _set_cursor(st, cursor, 9)
        z_out = torch.full((3, 37), 7.0, device=DEV)
        nat.ddpm_sample_sigma(st, out_dev, 5.0, z_out=z_out, keep=keep)
        nat.ddpm_sample_advance(st)
        assert torch.equal(st.x.cpu(), host["x"]) and torch.equal(st.xs.cpu(), host["xs"]) and torch.equal(st.hist.cpu(), host["hist"])
        assert bool((st.model_in == 3.0).all()) and bool((st.t_model == -5.0).all())
        assert bool((z_out == 7.0).all()) and st.cursor.cpu().tolist()[0] == cursor


# -- whole chains ----------------------------------------------------------------------------------------------------------------
class _Out:
    def __init__(self, sample):
        self.sample = sample


class FractionalLinearDenoiser(torch.nn.Module):
    """out = w·x_in + (t/999 − 0.5) + 0.1·mean(context), fp32, t a FLOAT timestep: a denoiser whose chain a float64 loop follows
    exactly.  (tests/test_gpu_sampling.LinearDenoiser indexes a table by integer timestep.)"""

    def __init__(self, w):
        super().__init__()
        self.w = torch.nn.Parameter(torch.full((1, 1, 1, 1), float(w)), requires_grad=False)  # (4-d: names the compute dtype)

    def forward(self, x, t, ctx):
        assert t.dtype == torch.float32
        return _Out(self.w * x + (t / 999.0 - 0.5).view(-1, 1, 1, 1) + 0.1 * ctx.mean(dim=(1, 2)).view(-1, 1, 1, 1))


W, G = 0.9, 5.0


def _guided_reference_output(smp, x, cond, neg):
    """The guided output of the linear denoiser in float64, from the reference sampler's own σ and timestep."""
    x_in = smp.model_input(x)
    o_u, o_c = (W * x_in + (smp.model_timestep / 999.0 - 0.5) + 0.1 * m.double().mean(dim=(1, 2)).view(-1, 1, 1, 1) for m in (neg, cond))
    return o_u + G * (o_c - o_u)


def _slopes(method, S, v, karras):
    """From the float64 reference alone: the slope of every STEP's new state in the state it starts from — the map is affine, so
    two evaluations (from 0 and from 1) give it; a Heun step is its two model evaluations, the last one its single one."""
    zero_ctx = torch.zeros(1, 1, 1)
    smps = [sr.make(method, S, v, karras) for _ in range(2)]
    out = []
    while not smps[0].done:
        xs = [torch.zeros(1, 1, 1, 1, dtype=torch.float64), torch.ones(1, 1, 1, 1, dtype=torch.float64)]
        step = smps[0].i
        while smps[0].i == step:  # (one evaluation, or Heun's two)
            xs = [s.step(x, _guided_reference_output(s, x, zero_ctx, zero_ctx), torch.zeros_like(x)) for s, x in zip(smps, xs)]
        out.append(abs(float(xs[1] - xs[0])))
    assert len(out) == S
    return out


def test_no_step_of_the_linear_chain_amplifies():
    """The precondition of the running bound below, from the float64 reference alone."""
    worst = max(max(_slopes(m, S, v, k)) for m in METHODS for v in (False, True) for k in (False, True) for S in (4, 5))
    print(f"\n[linear chain] largest slope of a step in the state {worst:.4g}")
    assert worst <= 1.0


@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_chain_with_a_linear_denoiser_against_float64(method, karras, capture):
    S, B, shape, seed = 4, 2, (4, 8, 8), 123
    assert max(_slopes(method, S, False, karras)) <= 1.0  # no iteration amplifies an earlier iteration's error
    model = FractionalLinearDenoiser(W).to(DEV)
    gen = torch.Generator().manual_seed(3)
    cond, neg = torch.randn(B, 6, 32, generator=gen), torch.randn(B, 6, 32, generator=gen)
    sampler = dfa.LatentSampler(model, num_inference_steps=S, guidance_scale=G, method=SAMPLER_NAME[method], karras_sigmas=karras, capture_graph=capture)
    sampler.begin(cond.to(DEV), neg.to(DEV), seed=seed, latent_shape=shape)
    assert sampler.replaying == capture and sampler.timesteps.dtype == torch.float64
    smp = sr.make(method, S, False, karras)
    n_it = sampler.num_model_evaluations
    assert n_it == (2 * S - 1 if method == "heun" else S) and sampler.run_evaluations == n_it
    x = sampler.latents.cpu().double()  # the chain starts from the sampler's own x_T …
    start = smp.start(ref.init_normals(B, 256, seed).reshape(x.shape))
    assert float((x - start).abs().max()) <= ref.Z_TOL * smp.sigmas[0]  # … which is σ₀ times the oracle's draw
    bound, more = 0.0, True
    for i in range(n_it):
        assert more and not smp.done
        assert abs(float(sampler.run_timesteps[i]) - smp.model_timestep) <= 1e-9 * max(1.0, smp.model_timestep)
        s = smp.noise_scale
        z = ref.step_normals(B, 256, seed, i).reshape(x.shape)
        x = smp.step(x, _guided_reference_output(smp, x, cond, neg), z)
        bound += ref.state_bound(x, s)
        more = sampler.step()
        err = float((sampler.latents.cpu().double() - x).abs().max())
        print(f"\n[sigma linear chain {method} karras {karras} capture {capture} iteration {i}] err {err:.3g} (bound {bound:.3g})")
        assert err <= bound
    assert smp.done and more is False and sampler.step() is False and sampler.state.cursor.cpu().tolist() == [n_it, seed]


def _checkerboard(B, h, w):
    yy, xx, bb = torch.arange(h).view(1, 1, h, 1), torch.arange(w).view(1, 1, 1, w), torch.arange(B).view(B, 1, 1, 1)
    return ((yy + xx + bb) % 2).float()


def _states_of_a_run(sampler, cond, neg, **kw):
    sampler.begin(cond, neg, **kw)
    states = [sampler.latents.cpu().clone()]
    while True:
        more = sampler.step()
        states.append(sampler.latents.cpu().clone())
        if not more:
            return states


@pytest.mark.parametrize("method", METHODS)
def test_keep_mask_and_image_to_image_on_the_linear_denoiser(method):
    S, B, shape = 4, 2, (4, 8, 8)
    model = FractionalLinearDenoiser(W).to(DEV)
    gen = torch.Generator().manual_seed(3)
    cond, neg = torch.randn(B, 6, 32, generator=gen).to(DEV), torch.randn(B, 6, 32, generator=gen).to(DEV)
    init, mask = torch.randn(B, *shape, generator=gen), _checkerboard(B, 8, 8)
    masked = dfa.LatentSampler(model, num_inference_steps=S, guidance_scale=G, method=SAMPLER_NAME[method])
    plain = dfa.LatentSampler(model, num_inference_steps=S, guidance_scale=G, method=SAMPLER_NAME[method])
    full = plain.timesteps
    graphs = []
    for strength, seed in ((0.75, 11), (0.5, 11), (0.75, 12)):
        n, k0 = dfa.partial_start(S, strength)
        kw = dict(seed=seed, init_latents=init.to(DEV), strength=strength)
        held = _states_of_a_run(masked, cond, neg, keep_mask=mask.to(DEV), **kw)
        assert masked.replaying
        graphs.append(masked._recorder.graph)
        free = _states_of_a_run(plain, cond, neg, **kw)
        n_it = 2 * n - 1 if method == "heun" else n
        for smp_ in (masked, plain):  # a partial run is the TAIL of the full run
            assert smp_.run_evaluations == n_it == len(free) - 1 and torch.equal(smp_.run_timesteps, full[full.shape[0] - n_it:])
            assert smp_.state.cursor.cpu().tolist() == [smp_.num_model_evaluations, seed]
        # the start state: init + σ_{k0}·ε
        sg = float(plain.sigmas[k0])
        want = init.double() + sg * ref.init_normals(B, 256, seed).reshape(init.shape).double()
        assert float((free[0].double() - want).abs().max()) <= ref.Z_TOL * sg and torch.equal(free[0], held[0])
        keep, resample = (mask == 1).expand_as(init), (mask == 0).expand_as(init)
        assert torch.equal(held[-1][keep], init[keep])  # held: the start image, bit for bit
        for a, b in zip(held, free):  # resampled: every iteration's state is the unmasked run's, bit for bit
            assert torch.equal(a[resample], b[resample])
        assert not torch.equal(held[-1][keep], free[-1][keep])
    assert graphs[0] is not None and all(g is graphs[0] for g in graphs)  # one recording: two strengths, two seeds


def test_shared_noise_gives_every_sample_the_single_run():
    S, shape = 4, (4, 8, 8)
    model = FractionalLinearDenoiser(W).to(DEV)
    gen = torch.Generator().manual_seed(3)
    cond1, neg1 = torch.randn(1, 6, 32, generator=gen).to(DEV), torch.randn(1, 6, 32, generator=gen).to(DEV)
    sampler = dfa.LatentSampler(model, num_inference_steps=S, guidance_scale=G, method="euler_a")
    one = sampler.sample(cond1, neg1, seed=9, latent_shape=shape).cpu()
    three = sampler.sample(cond1.repeat(3, 1, 1), neg1.repeat(3, 1, 1), seed=9, latent_shape=shape, shared_noise=True).cpu()
    own = sampler.sample(cond1.repeat(3, 1, 1), neg1.repeat(3, 1, 1), seed=9, latent_shape=shape).cpu()
    for b in range(3):
        assert torch.equal(three[b], one[0]), b
    assert torch.equal(own[0], one[0]) and not torch.equal(own[1], one[0])  # without it: the batch's own stream


# -- on the harness UNet -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def f16_unet():
    return _harness_unet()


@pytest.mark.parametrize("method", METHODS)
def test_harness_unet_replayed_equals_host_launched(f16_unet, method):
    """f16, LoRA r = 4, HIP attention on, 4 UNet rows (the forward is run-to-run deterministic there)."""
    unet = f16_unet
    cond, neg = _conditioning()
    host = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method=SAMPLER_NAME[method], capture_graph=False)
    sampler = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method=SAMPLER_NAME[method])
    seen = []
    first = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE, callback=lambda i, t, x: seen.append((i, t))).cpu()
    assert sampler.replaying and not host.replaying
    assert seen == list(enumerate(sampler.timesteps.tolist())) and all(type(t) is float for _, t in seen)
    assert len(seen) == (2 * S_UNET - 1 if method == "heun" else S_UNET)
    assert first.dtype == torch.float32 and tuple(first.shape) == (2, *SHAPE) and bool(torch.isfinite(first).all())
    assert torch.equal(first, host.sample(cond, neg, seed=5, latent_shape=SHAPE).cpu())
    graph = sampler._recorder.graph
    other = sampler.sample(cond, neg, seed=6, latent_shape=SHAPE).cpu()  # the same recording: the seed lives in device memory
    assert sampler._recorder.graph is graph and not torch.equal(other, first)
    assert torch.equal(sampler.sample(cond, neg, seed=5, latent_shape=SHAPE).cpu(), first)
    layer = tr.lora_layers(unet)[3]
    with torch.no_grad():
        layer.lora_up.weight.mul_(-2.0)
    try:
        edited = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE).cpu()  # an in-place edit alone
        assert sampler.replaying and not torch.equal(edited, first)
        assert torch.equal(edited, host.sample(cond, neg, seed=5, latent_shape=SHAPE).cpu())
    finally:
        with torch.no_grad():
            layer.lora_up.weight.mul_(-0.5)


def test_a_closed_gate_is_the_model_without_its_lora():
    """`lora_scales=[0.0, 1.0]`: sample 0 against the run with the LoRA switched off (tune_lora_scale 0.0), sample 1 against the
    plain run — fp32, to the tolerance tests/test_gpu_sampling_rows.py holds the same comparison to."""
    unet = _harness_unet(torch.float32)
    cond, neg = _conditioning()
    kw = dict(seed=5, latent_shape=SHAPE)
    gated = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method="euler_a").sample(cond, neg, lora_scales=[0.0, 1.0], **kw).cpu()
    with_lora = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method="euler_a").sample(cond, neg, **kw).cpu()
    dfa.tune_lora_scale(unet, 0.0)
    without = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method="euler_a").sample(cond, neg, **kw).cpu()
    dfa.tune_lora_scale(unet, 1.0)
    assert _same(gated[0], without[0], torch.float32, "sample 0 under a gate of 0 vs tune_lora_scale(unet, 0.0)")
    assert _same(gated[1], with_lora[1], torch.float32, "sample 1 under a gate of 1 vs no table")
    assert rel_err(gated[0], with_lora[0]) > 10 * FP32_TOL  # (the LoRA matters)
