"""CPU side of the sampler tests: one denoising step in the UNCOLLAPSED x0 / ε form, float64 — what diffusers' DDPMScheduler
(ancestral, variance fixed_small) and DDIMScheduler compute for SD's config (scaled_linear betas, clip_sample=False, leading
spacing), restated from their published definitions; diffusers is not part of the reference tree.  The product collapses each
step to x' = a·x + b·o + σ·z (sampling.sampler_schedule); nothing here shares code with it.  Also the Philox normals of the
sampler's two streams and classifier-free guidance as lora_diffusion/utils.py:112-163 asks the pipeline for it."""
import numpy as np
import torch

from tests import posterior_cases as pc

INIT_STREAM, NOISE_STREAM = 3, 4  # eps: 0, timesteps: 1, posterior z: 2
Z_TOL = 2e-5  # libm against the device's logf / sincosf: the bound of tests/test_gpu_posterior.py


def alphas_cumprod(T=1000, beta_start=0.00085, beta_end=0.012):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def timesteps(method, S, T=1000):
    ratio = T // S
    offset = 1 if method == "ddim" and (S - 1) * ratio + 1 <= T - 1 else 0  # steps_offset where the table has room for it
    return [(S - 1 - i) * ratio + offset for i in range(S)]


def sigma(method, S, i, eta=0.0, T=1000):
    acp = alphas_cumprod(T)
    t = timesteps(method, S, T)[i]
    t_prev = t - T // S
    ab_t = acp[t]
    if method == "ddpm":
        if i == S - 1:
            return 0.0
        ab_p = acp[t_prev] if t_prev >= 0 else torch.tensor(1.0, dtype=torch.float64)
        return float(torch.clamp((1 - ab_p) / (1 - ab_t) * (1 - ab_t / ab_p), min=1e-20).sqrt())
    ab_p = acp[t_prev] if t_prev >= 0 else acp[0]
    return float(eta * ((1 - ab_p) / (1 - ab_t)).sqrt() * (1 - ab_t / ab_p).sqrt())


def step(method, S, i, x, o, z, v_prediction, eta=0.0, T=1000):
    """x' (float64) of denoising step i from the state x, the (guided) model output o and the noise z."""
    x, o, z = x.double(), o.double(), z.double()
    acp = alphas_cumprod(T)
    t = timesteps(method, S, T)[i]
    t_prev = t - T // S
    ab_t = acp[t]
    s, q = ab_t.sqrt(), (1 - ab_t).sqrt()
    if v_prediction:
        x0, eps = s * x - q * o, q * x + s * o
    else:
        x0, eps = (x - q * o) / s, o
    sg = sigma(method, S, i, eta, T)
    if method == "ddpm":
        ab_p = acp[t_prev] if t_prev >= 0 else torch.tensor(1.0, dtype=torch.float64)
        alpha_c = ab_t / ab_p
        beta_c = 1 - alpha_c
        mean = (ab_p.sqrt() * beta_c / (1 - ab_t)) * x0 + (alpha_c.sqrt() * (1 - ab_p) / (1 - ab_t)) * x
        return mean + sg * z
    ab_p = acp[t_prev] if t_prev >= 0 else acp[0]
    return ab_p.sqrt() * x0 + (1 - ab_p - sg ** 2).sqrt() * eps + sg * z


def guided(out, guidance, cfg):
    """o from the model output: rows [uncond | cond] under guidance."""
    out = out.double()
    if not cfg:
        return out
    u, c = out.chunk(2, dim=0)
    return u + guidance * (c - u)


def init_normals(B, per_row, seed):
    return torch.from_numpy(pc.stream_normals(B, per_row, seed, 0, stream=INIT_STREAM))


def step_normals(B, per_row, seed, i):
    return torch.from_numpy(pc.stream_normals(B, per_row, seed, i, stream=NOISE_STREAM))


def state_bound(ref, sg):
    """The per-step bound on the fp32 state: 1e-5 relative (to the largest reference value: a handful of fp32 roundings of
    terms no larger than that, each 6e-8) plus σ times the bound on z."""
    return 1e-5 * float(ref.abs().max()) + sg * Z_TOL


def check_model_input(model_in, ref_state, dtype, cfg, slack=0.0):
    """Within one unit in the last place of `dtype` of the rounded reference state — plus `slack`, the bound on the fp32 state
    it is cast from; both halves bit-identical under guidance."""
    got = model_in.detach().cpu()
    if cfg:
        lo, hi = got.chunk(2, dim=0)
        assert torch.equal(lo, hi)
        got = lo
    want = ref_state.reshape(got.shape).to(dtype).double()
    ulp = pc.storage_ulp(ref_state.reshape(got.shape).double(), dtype)
    assert bool(((got.double() - want).abs() <= ulp + slack).all()), float(((got.double() - want).abs() / (ulp + slack)).max())
