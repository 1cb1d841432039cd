"""`lora_distill` — lora_diffusion/cli_svd.py: a fully fine-tuned model → rank-r LoRA factors of `tuned − base`.

The reference runs one full `torch.linalg.svd` per target linear (192 on SD1.5: 144 UNet + 48 CLIP-L layers).  Here every
layer is solved at once by batched block subspace iteration with Rayleigh–Ritz in HIP kernels (csrc/distill.hip for ranks
1–16, csrc/distill_wide.hip for ranks 17–64; DESIGN.md "svd_distill"): the difference D = float(T(W1 − W0)) is formed on load and never stored, each phase is one launch
for all layers, converged layers leave the launch table.

Contract (cli_svd.py:29-111): up = U_r·diag(S_r) [N, r], down = Vh_r [r, K], both clamped to [−hi, hi] with
hi = torch.quantile(cat(up.flatten(), down.flatten()), clamp_quantile) (linear interpolation, per layer, signed values).
An SVD fixes each singular pair (u_i, v_i) only up to a common sign and the clamp is not sign-invariant, so this module
fixes one: **the largest-magnitude entry of each `down` row is positive, ties going to the lowest index.**

Deviations from the reference, stated: the `.pt` lists `svd_distill` saves hold CPU fp32 tensors (the reference saves
device tensors), so `torch.load(..., weights_only=True)` works on any machine; `distill_lora` (the whole-model solver
with `clamp_quantile=None` to skip the clamp and an optional info dict) is an extension the reference does not have.
"""
import argparse
import warnings
from typing import List

import torch
import torch.nn as nn

from . import _native as nat
from .core import _find_modules
from .formats import _text_lora_path, _ti_lora_path  # noqa: F401  (cli_svd.py exports them)

UNET_TARGETS = ["CrossAttention", "Attention", "GEGLU"]  # cli_svd.py:47-48
TEXT_TARGETS = ["CLIPAttention"]  # cli_svd.py:50

_ALIGN = 256
_STATE_ITERS, _STATE_RES, _STATE_LAM = 4, 8, 64  # per-layer workspace header (csrc/distill.hip, csrc/distill_wide.hip)


def extract_linear_weights(model, target_replace_module) -> List[torch.Tensor]:
    """The weights of the nn.Linear children of `target_replace_module` classes, in _find_modules order (cli_svd.py:19-26):
    the order weight_apply_lora and monkeypatch_lora consume factor lists in."""
    return [child.weight for _, _, child in _find_modules(model, target_replace_module, search_class=[nn.Linear])]


def _layer_names(model, target_replace_module) -> List[str]:
    return [f"{type(holder).__name__}.{name}" for holder, name, _ in
            _find_modules(model, target_replace_module, search_class=[nn.Linear])]


def distill_lora(tuned, base, target_replace_module, rank: int = 4, clamp_quantile=0.99, *, tol: float = 1e-5,
                 max_iters: int = 200, seed: int = 0, check_every: int = 4, return_info: bool = False):
    """Rank-`rank` factors (1 <= rank <= 64) of tuned − base for every target linear: the flat list [up0, down0, up1,
    down1, …] of fp32 device tensors (views of one slab), as cli_svd.py:66-107 builds per model.  Ranks up to 16 run on the
    width-32 kernels, ranks 17–64 on the wide ones (block width 48, 64 or 80); planning, iteration and polling are the same.

    `clamp_quantile=None` skips the clamp (extension).  A layer is done when max_{i<=r} ‖Dᵀu_i − σ_i v_i‖ / σ_1 <= tol;
    layers still above it after `max_iters` iterations are reported with a RuntimeWarning and in info["unconverged"].
    With return_info, also returns {"iters": [per layer], "residual": [...], "sigma": [[σ_1..σ_r] per layer],
    "launches": kernel launches issued, "unconverged": [layer indices]}."""
    w1s = [w.detach() for w in extract_linear_weights(tuned, target_replace_module)]
    w0s = [w.detach() for w in extract_linear_weights(base, target_replace_module)]
    names = _layer_names(base, target_replace_module)
    if len(w1s) != len(w0s):
        raise ValueError(f"distill_lora: tuned model has {len(w1s)} target linears, base model {len(w0s)}")
    if not w0s:
        return ([], {"iters": [], "residual": [], "sigma": [], "launches": 0, "unconverged": []}) if return_info else []
    for i, (a, b) in enumerate(zip(w1s, w0s)):
        if a.shape != b.shape or a.dtype != b.dtype:
            raise ValueError(f"distill_lora: layer {i} ({names[i]}): tuned {tuple(a.shape)} {a.dtype} vs base "
                             f"{tuple(b.shape)} {b.dtype}")
    dtype = w0s[0].dtype
    if any(w.dtype != dtype for w in w0s):
        raise ValueError("distill_lora: all target weights must share one dtype")
    nat.dtype_code(dtype)
    if clamp_quantile is not None and not 0.0 <= float(clamp_quantile) <= 1.0:
        raise ValueError(f"distill_lora: clamp_quantile must be in [0, 1], got {clamp_quantile}")
    r = int(rank)
    if r > nat.DISTILL_MAX_RANK:
        raise ValueError(f"distill_lora: rank {r} > {nat.DISTILL_MAX_RANK} is not supported")
    if max_iters < 1:
        raise ValueError("distill_lora: max_iters must be >= 1")

    kern = nat.DistillKernels(r)
    plan = _plan(w1s, w0s, kern)
    device, rows, ws, out, full, flag_idx = (plan[k] for k in ("device", "rows", "ws", "out", "table", "flag_idx"))
    ws_off, out_off, L = plan["ws_off"], plan["out_off"], len(rows)
    min_nk = min(min(row[2], row[3]) for row in rows)

    launches = 0
    kern.start(full, L, min_nk, int(seed), ws)
    launches += 1
    active = list(range(L))
    table = full
    for it in range(max_iters):
        last = it == max_iters - 1
        n = len(active)
        max_n = max(rows[i][2] for i in active)
        max_k = max(rows[i][3] for i in active)
        kern.diff(table, n, max_n, False, dtype, ws)
        kern.rayleigh_ritz(table, n, 1, tol, False, ws)
        kern.diff(table, n, max_k, True, dtype, ws)
        kern.rayleigh_ritz(table, n, 2, tol, last, ws)
        launches += 4
        if last or (it + 1) % check_every == 0:
            flags = ws.view(torch.int32)[flag_idx].cpu()
            active = [i for i in active if int(flags[i]) == 0]
            if not active:
                break
            table = full[torch.tensor(active, device=device)]
    kern.finalize(full, L, clamp_quantile, ws, out)
    launches += 1

    flags = ws.view(torch.int32)[flag_idx].cpu().tolist()
    bad = [i for i in range(L) if flags[i] == 3]
    if bad:
        raise ValueError(f"distill_lora: non-finite values in layer {bad[0]} ({names[bad[0]]})"
                         + (f" and {len(bad) - 1} more" if len(bad) > 1 else ""))
    unconverged = [i for i in range(L) if flags[i] == 2]
    if unconverged:
        warnings.warn(f"distill_lora: {len(unconverged)} layer(s) did not reach tol={tol} in {max_iters} iterations "
                      f"(first: {unconverged[0]} {names[unconverged[0]]})", RuntimeWarning)

    loras = []
    for i, row in enumerate(rows):
        N, K = row[2], row[3]
        o = out_off[i]
        loras.append(out[o:o + N * r].view(N, r))
        loras.append(out[o + N * r:o + r * (N + K)].view(r, K))
    if not return_info:
        return loras
    head = torch.stack([ws[o:o + _STATE_LAM + 8 * r] for o in ws_off]).cpu()
    info = {
        "iters": head[:, _STATE_ITERS:_STATE_ITERS + 4].contiguous().view(torch.int32).flatten().tolist(),
        "residual": head[:, _STATE_RES:_STATE_RES + 8].contiguous().view(torch.float64).flatten().tolist(),
        "sigma": head[:, _STATE_LAM:].contiguous().view(torch.float64).sqrt().tolist(),
        "launches": launches,
        "unconverged": unconverged,
    }
    return loras, info


def _plan(w1s, w0s, kern):
    """Device copies of the weights, the layer table, the workspace slab and the output slab of one distill_lora call on the
    kernel set `kern` (nat.DistillKernels)."""
    r = kern.r
    device = nat.staging_device(*w1s, *w0s)
    w1s = [w.to(device).contiguous() for w in w1s]
    w0s = [w.to(device).contiguous() for w in w0s]
    rows, ws_off, out_off, ws_total, out_total = [], [], [], 0, 0
    for i, (a, b) in enumerate(zip(w1s, w0s)):
        N, K = b.shape
        ws_off.append(ws_total)
        out_off.append(out_total)
        rows.append([a.data_ptr(), b.data_ptr(), N, K, ws_total, out_total, i, 0])
        ws_total += (kern.workspace_bytes(N, K) + _ALIGN - 1) // _ALIGN * _ALIGN
        out_total += r * (N + K)
    return {
        "device": device, "rows": rows, "ws_off": ws_off, "out_off": out_off, "weights": (w1s, w0s),
        "ws": torch.zeros(ws_total, dtype=torch.uint8, device=device),
        "out": torch.empty(out_total, dtype=torch.float32, device=device),
        "table": torch.tensor(rows, dtype=torch.int64).to(device),
        "flag_idx": torch.tensor(ws_off, dtype=torch.int64, device=device) // 4,
    }


def _load_pipeline(path: str, device):
    try:
        from diffusers import StableDiffusionPipeline
    except ImportError as e:
        raise ImportError("svd_distill: loading a model from a path or hub id needs `diffusers`; pass a loaded pipeline "
                          "(any object with .unet and .text_encoder) instead") from e
    return StableDiffusionPipeline.from_pretrained(path, torch_dtype=torch.float16).to(device)  # cli_svd.py:37-44


def svd_distill(
    target_model,
    base_model,
    rank: int = 4,
    clamp_quantile: float = 0.99,
    device: str = "cuda:0",
    save_path: str = "svd_distill.pt",
):
    """cli_svd.py:29-111.  Models are pipelines (objects with .unet and .text_encoder) or paths loaded with diffusers in
    fp16 as the reference does.  The UNet list goes to `save_path`, the text-encoder list to _text_lora_path(save_path),
    as CPU fp32 tensors (the reference saves device tensors)."""
    dev = torch.device(device)
    pipe_base = _load_pipeline(base_model, dev) if isinstance(base_model, str) else base_model
    pipe_tuned = _load_pipeline(target_model, dev) if isinstance(target_model, str) else target_model
    text_path = _text_lora_path(save_path)
    with torch.cuda.device(dev):
        unet = distill_lora(pipe_tuned.unet, pipe_base.unet, UNET_TARGETS, rank, clamp_quantile)
        clip = distill_lora(pipe_tuned.text_encoder, pipe_base.text_encoder, TEXT_TARGETS, rank, clamp_quantile)
    torch.save([t.cpu() for t in unet], save_path)
    torch.save([t.cpu() for t in clip], text_path)


def main(argv=None):
    """`lora_distill` (cli_svd.py:114-115): fire when it is installed, else argparse with the same flag names."""
    try:
        import fire
    except ImportError:
        fire = None
    if fire is not None and argv is None:
        fire.Fire(svd_distill)
        return
    p = argparse.ArgumentParser(prog="lora_distill", description=svd_distill.__doc__)
    p.add_argument("target_model", nargs="?")
    p.add_argument("base_model", nargs="?")
    p.add_argument("--target_model", "--target-model", dest="target_model_flag")
    p.add_argument("--base_model", "--base-model", dest="base_model_flag")
    p.add_argument("--rank", type=int, default=4)
    p.add_argument("--clamp_quantile", "--clamp-quantile", type=float, default=0.99)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--save_path", "--save-path", default="svd_distill.pt")
    a = p.parse_args(argv)
    target, base = a.target_model_flag or a.target_model, a.base_model_flag or a.base_model
    if target is None or base is None:
        p.error("target_model and base_model are required")
    svd_distill(target, base, rank=a.rank, clamp_quantile=a.clamp_quantile, device=a.device, save_path=a.save_path)
