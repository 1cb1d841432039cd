"""CPU side of the posterior-draw tests: the Philox stream-2 normals of ddpm_posterior_prologue, built from the oracle's
Philox4x32-10 with the mapping `oracle.philox.step_randomness` applies to stream 0, and the float64 statement of

    x0 = (mean + exp(0.5·clamp(logvar, −30, 20))·z)·scale ;  noisy = √ᾱ_t·x0 + √(1−ᾱ_t)·eps ;  target = eps | velocity

(`vae.encode(pixels).latent_dist.sample() * 0.18215`, train_lora_dreambooth.py:818-821, followed by :824-853).  diffusers'
DiagonalGaussianDistribution is not part of the reference tree: the formula is restated from its published definition."""
import numpy as np
import torch

from oracle import philox

POSTERIOR_STREAM = 2  # eps: 0, timesteps: 1


def group_words(n, seed, step, stream):
    """The four Philox words of every element group g < ceil(n/4): counter (g, g>>32, stream, 0), key (seed, step)."""
    groups = (n + 3) // 4
    g = np.arange(groups, dtype=np.uint64)
    return philox.philox4x32_10((g & np.uint64(0xFFFFFFFF)).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32),
                                np.full(groups, stream, np.uint32), np.zeros(groups, np.uint32), seed & 0xFFFFFFFF,
                                step & 0xFFFFFFFF)


def stream_normals(batch, per_row, seed, step, stream=POSTERIOR_STREAM):
    """[batch, per_row] float32 normals of `stream`: Box–Muller on the two word pairs, u = (x + 0.5)·2^-32, in float32 like
    step_randomness (stream 0 reproduces its eps)."""
    n = batch * per_row
    r0, r1, r2, r3 = group_words(n, seed, step, stream)
    rad0 = np.sqrt(np.float32(-2.0) * np.log(philox._u01(r0))).astype(np.float32)
    rad1 = np.sqrt(np.float32(-2.0) * np.log(philox._u01(r2))).astype(np.float32)
    a0 = np.float32(6.283185307179586) * philox._u01(r1)
    a1 = np.float32(6.283185307179586) * philox._u01(r3)
    z = np.stack([rad0 * np.cos(a0), rad0 * np.sin(a0), rad1 * np.cos(a1), rad1 * np.sin(a1)], axis=1).astype(np.float32)
    return z.reshape(-1)[:n].reshape(batch, per_row)


def posterior_x0(moments, z, scale=0.18215):
    """float64 latents from moments [B, 2C, ...] (any dtype: read as stored) and z shaped like the latents — torch's own
    chunk / clamp / exp / mul / add / mul, the composite the kernels replace."""
    mean, logvar = torch.chunk(moments.double().cpu(), 2, dim=1)
    std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
    return (mean + std * z.double().cpu().reshape(mean.shape)) * scale


def noisy_and_target(x0, eps, t, acp, v_prediction):
    """float64 add_noise / target of the DDPM definitions from float64 ᾱ (`acp` [T])."""
    x0, eps = x0.double().cpu(), eps.double().cpu().reshape(x0.shape)
    shape = (-1,) + (1,) * (x0.dim() - 1)
    a = acp.double()[t.cpu()].sqrt().reshape(shape)
    s = (1.0 - acp.double()[t.cpu()]).sqrt().reshape(shape)
    return a * x0 + s * eps, (a * eps - s * x0) if v_prediction else eps


def storage_ulp(ref, dtype):
    """Spacing of `dtype`'s representable numbers at each float64 value of `ref` (subnormal spacing below the smallest
    normal)."""
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}[dtype]
    exp = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, exp - mant)
