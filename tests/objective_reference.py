"""CPU references of the training-objective extensions (Min-SNR-γ loss weights, offset noise): the weighted DDPM loss in
float64 with torch autograd, the Min-SNR formula in float64, and the offset normals ξ built from the oracle's Philox4x32-10
(imported, not modified) with the Box–Muller mapping `oracle.philox.step_randomness` applies to stream 0.

    loss = (1/n_inst) Σ_b w_b·mean_chw((m·p − m·t)²) + prior_weight·(1/n_prior) Σ_b w_b·mean_chw(…),   w_b = weights[t_b]
    ξ[b, c]: counter (j, j>>32, 3, 0) with j = b·C + c, key (seed, step);  ξ = sqrt(−2·ln u(r0))·cos(2π·u(r1))

There is no reference file to cite: both are extensions beyond the reference (Hang et al. 2023; Guttenberg 2023)."""
import numpy as np
import torch

from oracle import philox

OFFSET_STREAM = 3  # eps: 0, timesteps: 1, posterior z: 2


def weighted_loss(pred, target, mask, t, weights, n_inst, n_prior, prior_weight, grad_scale=1.0):
    """(loss, dpred·grad_scale) in float64.  pred / target [rows, C, h, w] (read as stored), mask [rows, 1, h, w] normalised or
    None, t int64 [rows], weights [T]."""
    p = pred.detach().double().cpu().requires_grad_(True)
    q = target.detach().double().cpu()
    w = weights.detach().double().cpu()[t.cpu()]
    a, b = (p, q) if mask is None else (p * mask.double().cpu(), q * mask.double().cpu())
    per_row = ((a - b) ** 2).reshape(p.shape[0], -1).mean(dim=1) * w
    loss = per_row[:n_inst].sum() / n_inst
    if n_prior:
        loss = loss + prior_weight * per_row[n_inst:].sum() / n_prior
    (grad,) = torch.autograd.grad(loss, p)
    return loss.detach(), grad * grad_scale


def min_snr(acp, gamma, v_prediction):
    """The Min-SNR-γ weights in float64 from ᾱ [T], written element by element."""
    out = []
    for a in acp.double().tolist():
        if a == 0.0:
            out.append(0.0 if v_prediction else 1.0)  # SNR = 0: min(0, γ)/(0 + 1) = 0; the ε form's limit is 1
            continue
        snr = a / (1.0 - a)
        out.append(min(snr, gamma) / (snr + 1.0) if v_prediction else min(snr, gamma) / snr)
    return torch.tensor(out, dtype=torch.float64)


def offset_normals(batch, channels, seed, step):
    """ξ [batch, channels] float32."""
    j = np.arange(batch * channels, dtype=np.uint64)
    n = j.size
    r0, r1, _, _ = philox.philox4x32_10((j & np.uint64(0xFFFFFFFF)).astype(np.uint32), (j >> np.uint64(32)).astype(np.uint32),
                                        np.full(n, OFFSET_STREAM, np.uint32), np.zeros(n, np.uint32), seed & 0xFFFFFFFF,
                                        step & 0xFFFFFFFF)
    rad = np.sqrt(np.float32(-2.0) * np.log(philox._u01(r0))).astype(np.float32)
    xi = (rad * np.cos(np.float32(6.283185307179586) * philox._u01(r1))).astype(np.float32)
    return xi.reshape(batch, channels)


def f32_ulp(ref):
    """Spacing of fp32 numbers at each float64 value of `ref`."""
    exp = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, exp - 23)
