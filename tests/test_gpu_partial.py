"""Image-to-image sampling on the device: ddpm_sample_init_from, ddpm_sample_step_keep and ddpm_sample_multistep_keep against
the float64 restatement of tests/partial_reference.py at the layout edges, whole partial runs with a linear stand-in denoiser —
host-launched and replayed — and LatentSampler(init_latents=, strength=, keep_mask=) on the harness UNet.

Every iteration is judged from the DEVICE's own previous state (and saved state and ring), read back exactly into float64: no
error is carried from one iteration to the next.  Bounds are the project's own: `sampling_reference.state_bound` for the one-step
methods (1e-5 of the largest reference value plus σ·Z_TOL), 1e-5 of max Σ|terms| for the multistep methods (tests/
test_gpu_multistep.py: PLMS's weights cancel), the 1e-5 taken over the blend's operands too (x', y: three more fp32 roundings
inside the same ×10 margin), plus Z_TOL times the coefficient of ε in the quantity under test: n for the start state, n_j for a
blended state (the oracle's ε against the device's logf / sincosf).  Where m == 0 and m == 1 the standard is bit equality."""
import functools
import itertools

import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import trainer as tr
from tests import multistep_reference as mr
from tests import partial_reference as ref
from tests import sampling_reference as sr
from tests import test_gpu_multistep as tgm
from tests import test_gpu_sampling as tgs

pytestmark = pytest.mark.gpu
DEV = "cuda"
# element path; 4-element path; per_row % 4 == 0 but hw % 4 != 0 (groups straddle channels); several workgroups
SHAPES = [(1, 1, 3, 5), (3, 4, 8, 8), (2, 4, 2, 3), (2, 4, 32, 32)]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
MASKS = ("zeros", "ones", "checkerboard", "ramp")
GUIDANCE, SEED = 5.0, 41
S_ONE, S_PLMS, S_DPM = 50, 8, 20
# (method, S, η, v-prediction, iteration): a middle and the last row of the one-step methods; plms's warm-up pair, a wrapped
# push and its last row; dpmpp_2m's first, a middle and its last row
ONE_STEP = [(m, S_ONE, eta, v, i) for (m, eta, v) in (("ddpm", 0.0, False), ("ddim", 0.5, True)) for i in (S_ONE // 2, S_ONE - 1)]
MULTISTEP = [("plms", S_PLMS, 0.0, False, i) for i in (0, 1, 6, S_PLMS)] + [("dpmpp_2m", S_DPM, 0.0, True, i) for i in (0, 10, S_DPM - 1)]


@pytest.fixture(autouse=True)
def _collect_garbage_first():
    """A recording left in a reference cycle by an earlier test must not be destroyed in the middle of another capture."""
    import gc

    gc.collect()


def _mask(kind, B, h, w):
    if kind == "zeros":
        return torch.zeros(B, 1, h, w)
    if kind == "ones":
        return torch.ones(B, 1, h, w)
    if kind == "checkerboard":
        yy, xx, bb = torch.arange(h).view(1, 1, h, 1), torch.arange(w).view(1, 1, 1, w), torch.arange(B).view(B, 1, 1, 1)
        return ((yy + xx + bb) % 2).float()
    return torch.linspace(0.0, 1.0, B * h * w).view(B, 1, h, w).flip(0).contiguous()  # soft ramp, 0 and 1 at its ends


@functools.lru_cache(maxsize=None)
def _device_eps(B, per_row, seed):
    """The device's own x_T draw (ddpm_sample_init) for (B, per_row, seed), on the host: what the kernels regenerate."""
    ts, coef = dfa.sampler_schedule("ddpm", 2, False)
    st = nat.SampleState.alloc((B, per_row), torch.float32, False, ts, coef, DEV)
    nat.ddpm_sample_init(st, seed)
    return st.x.cpu()


def _tables(method, S, v, eta, k0=0):
    """(timesteps, coef, plan or None, keep_coef, first row, run length) as full-size host tables: a multistep run begun at grid
    step k0 in the tail rows, built here from the public schedules."""
    if method in ("ddpm", "ddim"):
        ts, coef = dfa.sampler_schedule(method, S, v, eta)
        keep = torch.zeros(S, 2)
        keep[k0:] = dfa.keep_schedule(ts[k0:])
        return ts, coef, None, keep, k0, S - k0
    ts, coef, plan = (t.clone() for t in dfa.multistep_schedule(method, S, v))
    sub = dfa.multistep_schedule(method, S, v, first_step=k0)
    row = ts.shape[0] - sub[0].shape[0]
    for full, part in zip((ts, coef, plan), sub):
        full[row:] = part
    keep = torch.zeros(ts.shape[0], 2)
    keep[row:] = dfa.keep_schedule(sub[0])
    return ts, coef, plan, keep, row, int(sub[0].shape[0])


def _make_state(shape, dtype, cfg, method, S, v, eta, mask, init, x, xs=None, hist=None, k0=0, shifted=False, keep="all"):
    B = shape[0]
    rows = 2 * B if cfg else B
    ts, coef, plan, keep_tab, row, n_it = _tables(method, S, v, eta, k0)
    place = (lambda t: tgs._shifted(t.to(DEV))) if shifted else (lambda t: t.to(DEV).clone())
    common = (place(torch.zeros(rows, *shape[1:], dtype=dtype)), place(torch.zeros(rows, dtype=torch.int64)),
              place(torch.zeros(2, dtype=torch.int32)), place(ts), place(coef))
    extra = {"all": lambda: dict(init=place(init), mask=place(mask), keep_coef=place(keep_tab)), "init": lambda: dict(init=place(init)),
             None: dict}[keep]()
    if plan is None:
        return nat.SampleState(place(x), *common, cfg, **extra), row, n_it
    return nat.MultistepState(place(x), place(xs), place(hist), *common, place(plan), cfg, **extra), row, n_it


def _snapshot(st):
    snap = {"x": st.x.cpu(), "model_in": st.model_in.cpu(), "t_model": st.t_model.cpu()}
    if isinstance(st, nat.MultistepState):
        snap.update(xs=st.xs.cpu(), hist=st.hist.cpu())
    return snap


def _same_bits(a, b):
    return all(torch.equal(tgs._bits(a[k]), tgs._bits(b[k])) for k in a)


def _unblended(before, out, method, S, v, eta, cfg, k0, i, row, seed, guidance=GUIDANCE):
    """(x' in float64, its bound without the 1e-5 factor's other operand, σ) of run iteration i from the device's buffers
    `before`: the uncollapsed one-step update with the oracle's z, or the stateful solver begun at grid step k0 and resumed."""
    x = before["x"].double()
    B = x.shape[0]
    o = sr.guided(out.cpu().reshape(-1, *x.shape[1:]), guidance, cfg)
    if method in ("ddpm", "ddim"):
        sg = sr.sigma(method, S, k0 + i, eta)
        z = sr.step_normals(B, x[0].numel(), seed, k0 + i).reshape(x.shape) if sg != 0.0 else torch.zeros_like(x)
        want = sr.step(method, S, k0 + i, x, o, z, v, eta)
        return want, float(want.abs().max()), sg
    xs, hist = before["xs"].double(), before["hist"].double()
    _, coef, plan = dfa.multistep_schedule(method, S, v, coef_dtype=torch.float64, first_step=k0)  # (magnitudes of the bound only)
    flags = int(plan[i, 4])
    solver = ref.fresh_solver(method, S, v, k0)
    slots = mr.ring_slots(plan, i)
    known = min(solver.pushes_before(i), 3)
    assert all(slots[k - 1] is not None for k in range(1, known + 1))
    solver.resume(i, [hist[slots[k - 1]] for k in range(known, 0, -1)], saved=xs if flags & mr.USE_SAVED else None)
    want = solver.step(x, o)
    outd = out.cpu().double().reshape(-1, *x.shape[1:])
    o_abs = outd[:B].abs() + guidance * (outd[B:] - outd[:B]).abs() if cfg else outd.abs()
    p, q, a, c0 = (float(c) for c in coef[i, :4])
    terms = (a * (xs if flags & mr.USE_SAVED else x)).abs() + abs(c0) * ((p * x).abs() + abs(q) * o_abs)
    for k in (1, 2, 3):
        if float(coef[i, 3 + k]) != 0.0:
            terms = terms + (float(coef[i, 3 + k]) * hist[int(plan[i, k])]).abs()
    return want, float(terms.max()), 0.0


def _judge(before, after, out, method, S, v, eta, cfg, dtype, k0, i, row, seed, mask, init, keep_row, what):
    """The state after run iteration i (table row `row` + i) against float64, from the device's buffers before the launch.
    `mask` None: the unmasked entry.  Returns the measured error."""
    want, scale, sg = _unblended(before, out, method, S, v, eta, cfg, k0, i, row, seed)
    B, per_row = want.shape[0], want[0].numel()
    bound = 1e-5 * scale + sg * sr.Z_TOL
    if mask is not None:
        pair = ref.keep_pairs(ref.run_timesteps(method, S, k0))[i]
        eps = sr.init_normals(B, per_row, seed).reshape(want.shape)
        y = pair[0] * init.double() + pair[1] * eps
        want = ref.blend(mask, init, eps, pair, want)
        bound = 1e-5 * max(scale, float(y.abs().max())) + (sg + pair[1]) * sr.Z_TOL
        # where the mask is exactly 1 / exactly 0: bit equality with the fp32 host value / the caller checks the unmasked twin
        k32, n32 = keep_row[0], keep_row[1]
        held = (k32 * init) + (n32 * _device_eps(B, per_row, seed).reshape(init.shape))  # two products, one sum, fp32
        ones = (mask == 1).expand_as(init)
        assert torch.equal(after["x"][ones], held[ones])
        if keep_row.tolist() == [1.0, 0.0]:
            assert torch.equal(after["x"][ones], init[ones])  # the last row: the original, exactly
    err = float((after["x"].double() - want).abs().max())
    print(f"\n[{what} {method} S {S} k0 {k0} i {i} v {v} {dtype} cfg {cfg} {tuple(want.shape)}] err {err:.3g} (bound {bound:.3g})", end="")
    assert bool(torch.isfinite(after["x"]).all()) and err <= bound
    assert torch.equal(after["model_in"][:B], after["x"].to(dtype))  # the BLENDED state cast once
    if cfg:
        assert torch.equal(after["model_in"][:B], after["model_in"][B:])
    sr.check_model_input(after["model_in"], want, dtype, cfg, slack=bound)
    ts = ref.run_timesteps(method, S, k0)
    assert after["t_model"].tolist() == [ts[min(i + 1, len(ts) - 1)]] * (2 * B if cfg else B)
    return err


def _data(shape, dtype, cfg, data_seed=0):
    g = torch.Generator().manual_seed(data_seed)
    B = shape[0]
    rows = 2 * B if cfg else B
    x, xs, init = (torch.randn(shape, generator=g) for _ in range(3))
    hist = torch.randn(4, *shape, generator=g)
    out = torch.randn(rows, *shape[1:], generator=g).to(dtype)
    return x, xs, hist, init, out


def _launch(st, out, z_out=None):
    keep = st.mask is not None
    if isinstance(st, nat.MultistepState):
        (nat.ddpm_sample_multistep_keep if keep else nat.ddpm_sample_multistep)(st, out, GUIDANCE)
    else:
        (nat.ddpm_sample_step_keep if keep else nat.ddpm_sample_step)(st, out, GUIDANCE, z_out=z_out)


# -- the start state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_init_from_against_float64(shape, dtype, cfg):
    B, per_row, S, seed = shape[0], shape[1] * shape[2] * shape[3], 8, 77
    x, _, _, init, _ = _data(shape, dtype, cfg)
    x_T = _device_eps(B, per_row, seed).reshape(shape)
    assert float((x_T - sr.init_normals(B, per_row, seed).reshape(shape)).abs().max()) <= sr.Z_TOL
    for shifted, start in itertools.product((False, True), (0, S // 2, S - 1)):
        st, _, _ = _make_state(shape, dtype, cfg, "ddim", S, False, 0.0, None, init, x, shifted=shifted, keep="init")
        t0 = ref.run_timesteps("ddim", S, 0)[start]
        k, n = ref.noise_pair(t0)
        eps_out = torch.full(shape, 7.0, device=DEV)
        eps_out = tgs._shifted(eps_out) if shifted else eps_out
        nat.ddpm_sample_init_from(st, seed, start, k, n, eps_out=eps_out)
        got = st.x.cpu()
        assert torch.equal(eps_out.cpu(), x_T)  # the text-to-image run's noise, bit for bit: any dtype, alignment, guidance
        want = ref.noised(init, sr.init_normals(B, per_row, seed).reshape(shape), t0)
        err, bound = float((got.double() - want).abs().max()), sr.state_bound(want, n)
        print(f"\n[init_from {shape} {dtype} cfg {cfg} shifted {shifted} start {start}] err {err:.3g} (bound {bound:.3g})", end="")
        assert err <= bound
        k32, n32 = torch.tensor(k).float(), torch.tensor(n).float()
        assert torch.equal(got, (k32 * init) + (n32 * x_T))  # each product rounded on its own, the sum once: no fma
        rows = 2 * B if cfg else B
        assert torch.equal(st.model_in.cpu(), got.to(dtype).repeat(rows // B, 1, 1, 1))
        sr.check_model_input(st.model_in, want, dtype, cfg, slack=bound)
        assert st.t_model.cpu().tolist() == [t0] * rows and st.cursor.cpu().tolist() == [start, seed]
    st.init.fill_(0.0)  # a zero image at the last start: the state is n·ε alone
    nat.ddpm_sample_init_from(st, seed + 1, S - 1, k, n)
    assert torch.equal(st.x.cpu(), n32 * _device_eps(B, per_row, seed + 1).reshape(shape)) and st.cursor.cpu().tolist() == [S - 1, seed + 1]


# -- one keep step ---------------------------------------------------------------------------------------------------------------
def _keep_steps(shape, dtype, cfg, cases, shifted=False):
    """Every (method, iteration) of `cases` with every mask, next to the unmasked entry on the same inputs.  Returns the
    snapshots, keyed, for a caller that compares two access paths."""
    B, h, w = shape[0], shape[2], shape[3]
    x, xs, hist, init, out = _data(shape, dtype, cfg)
    results = {}
    for method, S, eta, v, i in cases:
        multistep = method in mr.SOLVERS
        plain, _, _ = _make_state(shape, dtype, cfg, method, S, v, eta, None, init, x, xs, hist, shifted=shifted, keep=None)
        out_dev = tgs._shifted(out.to(DEV)) if shifted else out.to(DEV)
        tgs._set_cursor(plain, i, SEED)
        before = _snapshot(plain)
        z_plain = None if multistep else torch.full(shape, 7.0, device=DEV)
        _launch(plain, out_dev, z_plain)
        unmasked = _snapshot(plain)
        _judge(before, unmasked, out, method, S, v, eta, cfg, dtype, 0, i, 0, SEED, None, None, None, "unmasked twin")
        for kind in MASKS:
            mask = _mask(kind, B, h, w)
            st, _, _ = _make_state(shape, dtype, cfg, method, S, v, eta, mask, init, x, xs, hist, shifted=shifted)
            tgs._set_cursor(st, i, SEED)
            z_out = None if multistep else torch.full(shape, 7.0, device=DEV)
            _launch(st, out_dev, z_out)
            after = _snapshot(st)
            _judge(before, after, out, method, S, v, eta, cfg, dtype, 0, i, 0, SEED, mask, init, st.keep_coef.cpu()[i], f"keep {kind}")
            zeros = (mask == 0).expand_as(x)
            assert torch.equal(tgs._bits(after["x"][zeros]), tgs._bits(unmasked["x"][zeros]))  # resampled: the unmasked bits
            assert torch.equal(after["t_model"], unmasked["t_model"]) and st.cursor.cpu().tolist() == [i, SEED]
            if multistep:  # SAVE and PUSH read the state before the update, as without a mask
                assert torch.equal(tgs._bits(after["xs"]), tgs._bits(unmasked["xs"]))
                assert torch.equal(tgs._bits(after["hist"]), tgs._bits(unmasked["hist"]))
            else:
                assert torch.equal(z_out.cpu(), z_plain.cpu())
            if kind == "zeros":
                assert _same_bits(after, unmasked)
            results[(method, i, kind)] = after
    return results


@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_keep_step_of_the_one_step_methods(shape, dtype, cfg):
    _keep_steps(shape, dtype, cfg, ONE_STEP)


@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_keep_step_of_the_multistep_methods(shape, dtype, cfg):
    _keep_steps(shape, dtype, cfg, MULTISTEP)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_keep_step_with_every_operand_one_element_off_alignment(dtype):
    """The element-by-element path — mask index per element — on a shape the 4-element path takes: the same bits everywhere."""
    shape = (3, 4, 8, 8)
    cases = ONE_STEP[:1] + ONE_STEP[-1:] + MULTISTEP[:2] + MULTISTEP[-2:]
    aligned = _keep_steps(shape, dtype, True, cases)
    shifted = _keep_steps(shape, dtype, True, cases, shifted=True)
    assert aligned.keys() == shifted.keys() and all(_same_bits(aligned[k], shifted[k]) for k in aligned)


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("method,S", [("ddpm", S_ONE), ("plms", S_PLMS)])
def test_a_keep_launch_with_the_cursor_out_of_range_changes_nothing(method, S, shifted):
    shape = (3, 4, 2, 3)
    x, xs, hist, init, out = _data(shape, torch.bfloat16, True)
    for cursor in (None, 3, -1):
        st, _, n_it = _make_state(shape, torch.bfloat16, True, method, S, False, 0.0, _mask("checkerboard", 3, 2, 3), init, x, xs, hist,
                                  shifted=shifted)
        cursor = st.S if cursor is None else st.S + cursor if cursor > 0 else cursor
        st.model_in.fill_(3.0)
        st.t_model.fill_(-5)
        tgs._set_cursor(st, cursor, 9)
        before = _snapshot(st)
        z_out = None if method == "plms" else torch.full(shape, 7.0, device=DEV)
        _launch(st, tgs._shifted(out.to(DEV)) if shifted else out.to(DEV), z_out)
        nat.ddpm_sample_advance(st)
        assert _same_bits(_snapshot(st), before) and st.cursor.cpu().tolist()[0] == cursor
        assert z_out is None or bool((z_out == 7.0).all())


@pytest.mark.parametrize("method,S,k0", [("plms", S_PLMS, 3), ("plms", S_PLMS, S_PLMS - 2), ("dpmpp_2m", S_DPM, 15), ("dpmpp_2m", 7, 4)])
@pytest.mark.parametrize("shape,shifted", [((2, 4, 8, 8), False), ((3, 4, 2, 3), False), ((2, 4, 8, 8), True)])
def test_partial_run_warms_up_over_poisoned_history(method, S, k0, shape, shifted):
    """A run begun at grid step k0 in the tail rows, xs and every history slot NaN before it: the sub-run's own warm-up keeps
    them unread — every iteration finite and within bound of the solver started fresh on grid[k0:], under a soft mask."""
    B, dtype = shape[0], torch.float16
    x, xs, hist, init, _ = _data(shape, dtype, True)
    xs.fill_(float("nan"))
    hist.fill_(float("nan"))
    mask = _mask("ramp", B, shape[2], shape[3])
    st, row, n_it = _make_state(shape, dtype, True, method, S, False, 0.0, mask, init, x, xs, hist, k0=k0, shifted=shifted)
    n = S - k0
    assert n_it == (n + 1 if method == "plms" and n >= 2 else n) and row == st.S - n_it
    t0 = ref.run_timesteps(method, S, k0)[0]
    nat.ddpm_sample_init_from(st, 3, row, *ref.noise_pair(t0))
    assert st.cursor.cpu().tolist() == [row, 3] and st.t_model.cpu().tolist() == [t0] * (2 * B)
    g = torch.Generator().manual_seed(17)
    for i in range(n_it):
        out = torch.randn(2 * B, *shape[1:], generator=g).half()
        before = _snapshot(st)
        _launch(st, tgs._shifted(out.to(DEV)) if shifted else out.to(DEV))
        nat.ddpm_sample_advance(st)
        _judge(before, _snapshot(st), out, method, S, False, 0.0, True, dtype, k0, i, row, 3, mask, init, st.keep_coef.cpu()[row + i],
               "poisoned partial warm-up")
        assert st.cursor.cpu().tolist()[0] == row + i + 1
    assert st.cursor.cpu().tolist()[0] == st.S  # the run ends where the full run ends


# -- whole runs ------------------------------------------------------------------------------------------------------------------
STRENGTHS = (0.3, 0.75, 1.0)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("S", [7, 20])
@pytest.mark.parametrize("method", ["ddpm", "ddim", "plms", "dpmpp_2m"])
def test_whole_runs_with_a_linear_denoiser(method, S, capture, masked):
    """One sampler, every strength in turn (replayed: the same recording).  After each iteration the expected state follows
    from the sampler's PREVIOUS buffers by the test's own forward of the same module on the same input."""
    B, shape, eta = 2, (4, 8, 8), (0.5 if method == "ddim" else 0.0)
    model = tgm.LinearDenoiser(0.9).to(DEV)
    gen = torch.Generator().manual_seed(3)
    cond, neg = torch.randn(B, 6, 32, generator=gen).to(DEV), torch.randn(B, 6, 32, generator=gen).to(DEV)
    sampler = dfa.LatentSampler(model, num_inference_steps=S, guidance_scale=GUIDANCE, method=method, eta=eta, capture_graph=capture)
    graph = None
    for k, strength in enumerate(STRENGTHS):
        seed = 100 + k
        init = torch.randn(B, *shape, generator=gen)
        mask = _mask(("ramp", "checkerboard", "ones")[k], B, 8, 8) if masked else None
        n, k0 = ref.steps_run(S, strength)
        sampler.begin(cond, neg, seed=seed, init_latents=init.to(DEV), strength=strength, keep_mask=None if mask is None else mask.to(DEV))
        assert sampler.replaying == capture
        if capture:
            graph = graph or sampler._recorder.graph
            assert sampler._recorder.graph is graph  # strength, init, mask values and seed: one recording
        ts = ref.run_timesteps(method, S, k0)
        assert sampler.run_evaluations == len(ts) and sampler.run_timesteps.tolist() == ts
        assert sampler.num_model_evaluations == (mr.evaluations(method, S) if method in mr.SOLVERS else S)
        st = sampler.state
        row = st.S - len(ts)
        assert st.cursor.cpu().tolist() == [row, seed] and (st.mask is not None) == masked
        start = ref.noised(init, sr.init_normals(B, 256, seed).reshape(init.shape), ts[0])
        assert float((st.x.cpu().double() - start).abs().max()) <= sr.state_bound(start, ref.noise_pair(ts[0])[1])
        more = True
        for i in range(len(ts)):
            assert more
            before = _snapshot(st)
            with torch.no_grad():
                out = model(st.model_in.clone(), st.t_model.clone(), sampler.conditioning).sample
            more = sampler.step()
            _judge(before, _snapshot(st), out, method, S, False, eta, True, torch.float32, k0, i, row, seed, mask, init,
                   None if mask is None else st.keep_coef.cpu()[row + i], f"linear run strength {strength} capture {capture}")
            assert st.cursor.cpu().tolist() == [row + i + 1, seed]
        assert more is False and sampler.step() is False and st.cursor.cpu().tolist() == [st.S, seed]
        if masked and k == 2:  # everything held: the start image comes back exactly
            assert torch.equal(sampler.latents.cpu(), init)


# -- on the harness UNet -----------------------------------------------------------------------------------------------------------
SHAPE, S_UNET = (4, 8, 8), 4


def _img2img_inputs(seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, *SHAPE, generator=g).to(DEV), _mask("checkerboard", 2, 8, 8).to(DEV)


@pytest.mark.parametrize("method", ["plms", "ddpm"])
def test_harness_unet_replayed_equals_host_launched_and_one_recording_serves(method):
    """f16, 4 UNet rows (the forward is run-to-run deterministic there)."""
    unet = tgs._harness_unet()
    cond, neg = tgs._conditioning()
    init, mask = _img2img_inputs()
    host = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method=method, capture_graph=False)
    sampler = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method=method)
    seen = []
    first = sampler.sample(cond, neg, seed=5, init_latents=init, strength=0.75, keep_mask=mask,
                           callback=lambda i, t, x: seen.append((i, t))).cpu()
    ts = ref.run_timesteps(method, S_UNET, 1)
    assert sampler.replaying and not host.replaying and seen == list(enumerate(ts)) and sampler.run_evaluations == len(ts)
    assert torch.equal(first, host.sample(cond, neg, seed=5, init_latents=init, strength=0.75, keep_mask=mask).cpu())
    held = (mask == 1).expand_as(init).cpu()
    assert torch.equal(first[held], init.cpu()[held]) and not torch.equal(first[~held], init.cpu()[~held])
    graph = sampler._recorder.graph
    # strength, init values, mask values, seed: the same graph object, replayed — each equal to the host-launched run
    other_init, other_mask = _img2img_inputs(seed=22)[0], _mask("ramp", 2, 8, 8).to(DEV)
    for kw in (dict(seed=5, init_latents=init, strength=0.5, keep_mask=mask), dict(seed=5, init_latents=other_init, strength=1.0, keep_mask=mask),
               dict(seed=5, init_latents=init, strength=0.75, keep_mask=other_mask), dict(seed=6, init_latents=init, strength=0.75, keep_mask=mask)):
        got = sampler.sample(cond, neg, **kw).cpu()
        assert sampler.replaying and sampler._recorder.graph is graph
        assert torch.equal(got, host.sample(cond, neg, **kw).cpu()) and not torch.equal(got, first)
    assert torch.equal(sampler.sample(cond, neg, seed=5, init_latents=init, strength=0.75, keep_mask=mask).cpu(), first)
    # a new recording only when the presence of init or mask toggles
    unmasked = sampler.sample(cond, neg, seed=5, init_latents=init, strength=0.75).cpu()
    assert sampler.replaying and sampler._recorder.graph is not graph and sampler.state.mask is None
    assert torch.equal(unmasked, host.sample(cond, neg, seed=5, init_latents=init, strength=0.75).cpu()) and not torch.equal(unmasked, first)
    graph = sampler._recorder.graph
    sampler.sample(cond, neg, seed=7, init_latents=other_init, strength=0.5)
    assert sampler._recorder.graph is graph
    # text-to-image after image-to-image on the same sampler: the bits of a fresh sampler
    plain = sampler.sample(cond, neg, seed=5, latent_shape=SHAPE).cpu()
    assert sampler._recorder.graph is not graph and sampler.run_evaluations == sampler.num_model_evaluations
    assert torch.equal(plain, dfa.LatentSampler(unet, num_inference_steps=S_UNET, method=method).sample(cond, neg, seed=5, latent_shape=SHAPE).cpu())
    # strength 1.0 keeps the image's contribution √ᾱ[t_0]·init: not the text-to-image run
    assert not torch.equal(sampler.sample(cond, neg, seed=5, init_latents=init, strength=1.0).cpu(), plain)


def test_lora_changes_show_in_the_next_image_to_image_sample():
    """The notebook's comparison: the same seed and start image under tune_lora_scale 0.0 / 0.7 / 1.0."""
    unet = tgs._harness_unet()
    cond, neg = tgs._conditioning()
    init, _ = _img2img_inputs()
    sampler = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method="plms")
    kw = dict(seed=5, init_latents=init, strength=0.75)
    samples = []
    for scale in (0.0, 0.7, 1.0):
        dfa.tune_lora_scale(unet, scale)
        samples.append(sampler.sample(cond, neg, **kw).cpu())
        fresh = dfa.LatentSampler(unet, num_inference_steps=S_UNET, method="plms", capture_graph=False)
        assert sampler.replaying and torch.equal(samples[-1], fresh.sample(cond, neg, **kw).cpu())
    assert not torch.equal(samples[0], samples[1]) and not torch.equal(samples[1], samples[2])
    graph = sampler._recorder.graph
    with torch.no_grad():
        tr.lora_layers(unet)[3].lora_up.weight.mul_(-2.0)  # an in-place edit alone: the same recording, another sample
    edited = sampler.sample(cond, neg, **kw).cpu()
    assert sampler._recorder.graph is graph and not torch.equal(edited, samples[2])
    assert torch.equal(edited, dfa.LatentSampler(unet, num_inference_steps=S_UNET, method="plms", capture_graph=False).sample(cond, neg, **kw).cpu())
