"""What `trainer.LoraTrainer` and `inversion.InversionTrainer` share of a training step: the DDPM noise prologue, the masked
loss with its backward pass, and the recording of a step into a hipGraph.  Nothing here knows which trainer is calling."""
import hashlib
import math
import warnings
from typing import NamedTuple, Optional

import torch
import torch.distributed as dist

from . import _native as nat


def compute_dtype(unet) -> torch.dtype:
    """The dtype a step computes in: that of the UNet's conv weights."""
    return next(p for p in unet.parameters() if p.dim() == 4).dtype


class Noising(NamedTuple):
    sqrt_acp: torch.Tensor
    sqrt_1macp: torch.Tensor
    dtype: torch.dtype  # of the noisy latents and the target
    v_prediction: bool
    n_timesteps: int  # a device draw takes its timesteps from [0, n_timesteps)
    scale: float = 0.18215  # of latents drawn from VAE moments (train_lora_dreambooth.py:821)
    noise_offset: float = 0.0  # of a device draw: eps + noise_offset·ξ[b, c] (ddpm_*_prologue_offset)
    loss_weights: Optional[torch.Tensor] = None  # device fp32 [T]: row b's loss is weighted by loss_weights[t_b]


def noise_prologue(nz: Noising, latents, noise, timesteps, seed, step_key, moments=None, posterior_noise=None):
    """(noisy, target, timesteps): from the caller's `noise` and `timesteps`, or — `noise` None — drawn on the device in the
    same launch, Philox keyed by (seed, step_key), timesteps uniform; with `nz.noise_offset` non-zero that draw is the
    `_offset` entry's.  `moments` [B,2C,h,w] instead of `latents`: the latents are drawn from them, `latent_dist.sample() *
    scale` — in that same launch, or from the caller's `posterior_noise` in a launch of its own in front of add_noise."""
    if moments is not None:
        if noise is None:
            if nz.noise_offset != 0.0:
                return nat.ddpm_posterior_prologue_offset(moments, nz.sqrt_acp, nz.sqrt_1macp, nz.dtype, seed, step_key,
                                                          nz.v_prediction, nz.n_timesteps, nz.scale, nz.noise_offset)
            return nat.ddpm_posterior_prologue(moments, nz.sqrt_acp, nz.sqrt_1macp, nz.dtype, seed, step_key, nz.v_prediction,
                                               nz.n_timesteps, nz.scale)
        latents = nat.ddpm_posterior_sample(moments, posterior_noise, nz.scale)
    if noise is None:
        if nz.noise_offset != 0.0:
            return nat.ddpm_noise_prologue_offset(latents, nz.sqrt_acp, nz.sqrt_1macp, nz.dtype, seed, step_key,
                                                  nz.v_prediction, nz.n_timesteps, nz.noise_offset)
        return nat.ddpm_noise_prologue(latents, nz.sqrt_acp, nz.sqrt_1macp, nz.dtype, seed, step_key, nz.v_prediction,
                                       nz.n_timesteps)
    noisy, target = nat.ddpm_add_noise(latents, noise, timesteps, nz.sqrt_acp, nz.sqrt_1macp, nz.dtype, nz.v_prediction)
    return noisy, target, timesteps


def zero_terminal_snr(alphas_cumprod) -> torch.Tensor:
    """ᾱ' float64 [T] on the CPU: the schedule rescaled so that its last timestep carries no signal (Lin et al., "Common
    Diffusion Noise Schedules and Sample Steps are Flawed", WACV 2024, Algorithm 1), in float64 throughout:
        s = √ᾱ;   s' = (s − s[T−1])·s[0]/(s[0] − s[T−1]);   ᾱ' = s'².
    ᾱ'[T−1] is exactly 0, ᾱ'[0] is ᾱ[0] to rounding, and a strictly decreasing table stays one.  diffusers'
    `rescale_zero_terminal_snr` goes on from ᾱ' to fp32 betas and a second cumprod; this form does not, so the last bits
    differ from its table.  ValueError for an empty table, a table of one entry, values outside [0, 1] and a table that is not
    strictly decreasing."""
    acp = torch.as_tensor(alphas_cumprod).detach().to("cpu", torch.float64).reshape(-1)
    if acp.numel() < 2:
        raise ValueError(f"alphas_cumprod must hold at least two timesteps; got {acp.numel()}")
    if bool(((acp < 0.0) | (acp > 1.0) | acp.isnan()).any()):
        raise ValueError("alphas_cumprod must be a table of values in [0, 1]")
    if not bool((acp[1:] < acp[:-1]).all()):
        raise ValueError("alphas_cumprod must be strictly decreasing")
    s = acp.sqrt()
    s = (s - s[-1]) * s[0] / (s[0] - s[-1])
    return s * s


def check_zero_terminal_snr(zero_terminal_snr: bool, v_prediction: bool) -> bool:
    """The trainers' rule for the flag: ε-prediction has nothing to learn at SNR 0 (the input is the target), and the ε-form of
    Min-SNR divides by it."""
    if zero_terminal_snr and not v_prediction:
        raise ValueError("zero_terminal_snr=True needs v_prediction=True: at zero SNR the noisy input IS the noise, so "
                         "ε-prediction learns nothing there")
    return bool(zero_terminal_snr)


def min_snr_weights(alphas_cumprod, gamma: float, v_prediction: bool = False) -> torch.Tensor:
    """The Min-SNR-γ loss weights per timestep (Hang et al. 2023), fp32 [T] on the CPU, computed in float64 from ᾱ_t:
    SNR = ᾱ/(1 − ᾱ); ε-prediction min(SNR, γ)/SNR — where SNR == 0 (a zero-terminal-SNR schedule) the weight is 1, the limit;
    v-prediction min(SNR, γ)/(SNR + 1)."""
    gamma = float(gamma)
    if not (math.isfinite(gamma) and gamma > 0.0):
        raise ValueError(f"snr_gamma must be a finite positive number; got {gamma!r}")
    acp = torch.as_tensor(alphas_cumprod).detach().to("cpu", torch.float64).reshape(-1)
    if not acp.numel() or bool(((acp < 0.0) | (acp > 1.0) | acp.isnan()).any()):
        raise ValueError("alphas_cumprod must be a non-empty table of values in [0, 1]")
    with_signal = acp > 0.0
    snr = acp / (1.0 - acp)  # (ᾱ == 1: SNR = inf, and γ/inf = 0 in both forms)
    capped = snr.clamp(max=gamma)
    if v_prediction:
        w = capped / (snr + 1.0)
    else:
        w = torch.where(with_signal, capped / torch.where(with_signal, snr, torch.ones_like(snr)), torch.ones_like(snr))
    return w.to(torch.float32)


def check_objective(snr_gamma, timestep_weights, noise_offset, n_timesteps: int):
    """The trainers' rules for their three objective arguments, on the host, before anything is built."""
    if snr_gamma is not None and timestep_weights is not None:
        raise ValueError("snr_gamma and timestep_weights are mutually exclusive: the first builds the table the second hands in")
    if snr_gamma is not None and not (math.isfinite(float(snr_gamma)) and float(snr_gamma) > 0.0):
        raise ValueError(f"snr_gamma must be a finite positive number; got {snr_gamma!r}")
    if timestep_weights is not None:
        w = timestep_weights
        if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 1:
            raise ValueError("timestep_weights must be an fp32 [T] tensor")
        if w.numel() != n_timesteps:
            raise ValueError(f"timestep_weights has {w.numel()} entries, the schedule has {n_timesteps} timesteps")
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
            raise ValueError("timestep_weights must be finite and non-negative")
    if not math.isfinite(float(noise_offset)):
        raise ValueError(f"noise_offset must be finite; got {noise_offset!r}")


def objective_table(snr_gamma, timestep_weights, alphas_cumprod, v_prediction: bool, device):
    """The device table of a trainer's loss weights — built once; a recorded step reads it through its address — or None."""
    if snr_gamma is not None:
        return min_snr_weights(alphas_cumprod, snr_gamma, v_prediction).to(device)
    if timestep_weights is not None:
        return timestep_weights.detach().to(device, copy=True).contiguous()
    return None


def table_digest(timestep_weights):
    """What a checkpoint's config records of the caller's table: a short digest of its fp32 bytes, None without one."""
    if timestep_weights is None:
        return None
    raw = timestep_weights.detach().to("cpu", torch.float32).contiguous().numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()[:16]


def objective_config(snr_gamma, timestep_weights_digest, noise_offset) -> dict:
    """The three objective arguments as a trainer's `_config()` records them."""
    return {"snr_gamma": None if snr_gamma is None else float(snr_gamma), "timestep_weights": timestep_weights_digest,
            "noise_offset": float(noise_offset)}


def table_identity(table):
    """What a recording bakes in of the loss-weight table: its address and version."""
    return None if table is None else (table.data_ptr(), table._version)


def check_noise_offset(noise_offset: float, noise):
    """The offset belongs to the device draw: the caller's noise cannot take it."""
    if noise_offset != 0.0 and noise is not None:
        raise ValueError("noise_offset applies to noise drawn on the device (pass a seed); with your own `noise`, add the "
                         "offset to it yourself: noise + noise_offset * randn(B, C, 1, 1)")


def latents_like(latents, moments):
    """What stands for the latents where only their shape and device are asked: themselves, or the mean half of the moments."""
    return latents if moments is None else moments[:, : moments.shape[1] // 2]


def check_noise_inputs(latents, moments, noise, timesteps, posterior_noise, seed):
    """The argument rules both trainers share for a step's latents and noise."""
    if (latents is None) == (moments is None):
        raise ValueError("pass exactly one of latents and moments")
    if (noise is None) != (timesteps is None):
        raise ValueError("pass both noise and timesteps, or neither (and a seed)")
    if noise is None and seed is None:
        raise ValueError("pass noise and timesteps, or a seed for the on-device draw")
    if moments is not None and noise is not None and posterior_noise is None:
        raise ValueError("moments with the caller's noise and timesteps need the caller's posterior_noise as well")
    if posterior_noise is not None and (moments is None or noise is None):
        raise ValueError("posterior_noise goes with moments and the caller's noise and timesteps")


def raw_mask(mask, like):
    """The raw mask of cli_lora_pti.py:222-247 as `lora_mask_prepare` reads it: fp32 [rows,1,8h,8w], contiguous, on the device
    of `like` (the latents or the prediction, [rows,C,h,w]).  None stays None."""
    if mask is None:
        return None
    return mask.to(like.device).reshape(like.shape[0], 1, like.shape[2] * 8, like.shape[3] * 8).float().contiguous()


def loss_backward(pred, target, raw, n_inst, n_prior, prior_weight, grad_scale, timesteps=None, loss_weights=None):
    """Fused (masked) MSE of the prediction and the backward pass from it, the gradient scaled by `grad_scale`.  With a
    `loss_weights` table (device fp32 [T]) row b is weighted by loss_weights[timesteps[b]], looked up inside the loss kernel.
    Returns the unscaled loss."""
    m = nat.lora_mask_prepare(raw, pred.shape[2], pred.shape[3]) if raw is not None else None
    pred_c = pred if pred.is_contiguous() else pred.contiguous()
    if loss_weights is not None:
        loss, dpred = nat.ddpm_mse_weighted_fwd_bwd(pred_c, target, m, timesteps, loss_weights, n_inst, n_prior, prior_weight,
                                                    grad_scale)
    else:
        loss, dpred = nat.ddpm_mse_fwd_bwd(pred_c, target, m, n_inst, n_prior, prior_weight, grad_scale)
    pred_c.backward(dpred)
    return loss


# -- EMA of the trained weights: the host's one statement of the decay `lora_adamw_ema_step` computes on the device -----------
def _f32(x: float) -> float:
    """The double that equals x rounded to fp32: what a float argument of the C ABI holds."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def check_ema(ema_decay, ema_update_after_step):
    """`LoraTrainer`'s rules for its two EMA arguments, on the host, before anything is built."""
    if ema_decay is not None and not (0.0 < float(ema_decay) < 1.0 and 0.0 < _f32(ema_decay) < 1.0):
        raise ValueError(f"ema_decay must lie strictly between 0 and 1 (None: no EMA); got {ema_decay!r}")
    after = ema_update_after_step
    if not isinstance(after, int) or isinstance(after, bool) or after < 0:
        raise ValueError(f"ema_update_after_step must be a non-negative integer; got {after!r}")


def ema_decay_at(applied_step: int, max_decay: float, update_after: int = 0) -> float:
    """The EMA decay d of the optimizer step whose 1-based APPLIED index is `applied_step` (skipped steps do not count), in
    double: diffusers' EMAModel.get_decay with use_ema_warmup=False, restated from its published definition —
        n = max(0, applied_step − update_after − 1) ;  d = 0 if n <= 0 else min(max_decay, (1 + n)/(10 + n))
    with `max_decay` rounded to fp32 first, as the kernel receives it.  d = 0 on the first counted step: the update
    s − 1·(s − p) then moves the average onto the parameters."""
    n = max(0, int(applied_step) - int(update_after) - 1)
    if n <= 0:
        return 0.0
    return min(_f32(max_decay), (1.0 + n) / (10.0 + n))


def ema_one_minus_decay_at(applied_step: int, max_decay: float, update_after: int = 0) -> float:
    """omd = fp32(1 − d) of `ema_decay_at`, as a double: the factor of the update s ← s − omd·(s − p)."""
    return _f32(1.0 - ema_decay_at(applied_step, max_decay, update_after))


# -- Prodigy: the host's rules for the options `lora_prodigy_moments` takes ------------------------------------------------------
OPTIMIZERS = ("adamw", "prodigy")


def check_prodigy(optimizer, d0=1e-6, d_coef=1.0, growth_rate=math.inf, use_bias_correction=False, safeguard_warmup=False,
                  betas=(0.9, 0.999)):
    """`LoraTrainer`'s rules for `optimizer` and its Prodigy options, on the host, before anything is built (the options are
    checked whichever optimizer is chosen: a typo does not wait for the switch).  Returns beta3 = sqrt(beta2)."""
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer must be one of {OPTIMIZERS}; got {optimizer!r}")
    for name, value in (("prodigy_d0", d0), ("prodigy_d_coef", d_coef)):
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or not _f32(value) > 0.0:
            raise ValueError(f"{name} must be a positive finite number (also after rounding to fp32); got {value!r}")
    if isinstance(growth_rate, bool) or not isinstance(growth_rate, (int, float)) or not growth_rate >= 1.0:
        raise ValueError(f"prodigy_growth_rate must be >= 1 (inf: no limit); got {growth_rate!r}")
    for name, value in (("prodigy_use_bias_correction", use_bias_correction), ("prodigy_safeguard_warmup", safeguard_warmup)):
        if not isinstance(value, bool):
            raise ValueError(f"{name} must be True or False; got {value!r}")
    if optimizer == "prodigy" and not all(0.0 <= _f32(b) < 1.0 for b in betas):
        raise ValueError(f"Prodigy needs betas in [0, 1); got {betas!r}")
    return math.sqrt(_f32(betas[1])) if 0.0 <= _f32(betas[1]) < 1.0 else None


def check_max_weight_norm(max_weight_norm):
    """`LoraTrainer`'s rule for `max_weight_norm`, on the host, before anything is built: None (no constraint) or a positive
    finite number that is still positive and finite as the fp32 value the kernel receives.  Returns it as a float, or None."""
    if max_weight_norm is None:
        return None
    v = max_weight_norm
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 0.0 \
            or not (math.isfinite(_f32(v)) and _f32(v) > 0.0):
        raise ValueError(f"max_weight_norm must be a positive finite number (None: no constraint); got {max_weight_norm!r}")
    return float(v)


# -- checkpoints: what the two trainers share of validating one before anything is written ---------------------------------
CHECKPOINT_VERSION = 1


def check_checkpoint_header(sd, kind: str) -> dict:
    """The metadata of a trainer's `state_dict()` after the checks that come first: it is one, of a version this code reads
    (a newer one is refused), written by a trainer of `kind`."""
    meta = sd.get("meta") if isinstance(sd, dict) else None
    if not isinstance(meta, dict) or not isinstance(sd.get("tensors"), dict):
        raise ValueError("not a trainer checkpoint: expected {'meta': {...}, 'tensors': {...}}")
    version = meta.get("format_version")
    if not isinstance(version, int) or isinstance(version, bool) or version < 1:
        raise ValueError(f"checkpoint format version {version!r} is not a version number")
    if version > CHECKPOINT_VERSION:
        raise ValueError(f"checkpoint format version {version} is newer than this code reads ({CHECKPOINT_VERSION})")
    if meta.get("kind") != kind:
        raise ValueError(f"checkpoint of a {meta.get('kind')!r}, not of a {kind!r}")
    return meta


def layout_difference(saved, own):
    """None when the two layout signatures agree, else one sentence naming the FIRST difference.  A signature: {"models":
    per model the ordered list of [module name, in_features, out_features, rank], "dense": the dense tails' shapes}."""
    s_models, o_models = saved.get("models", []), own.get("models", [])
    for m, (s_layers, o_layers) in enumerate(zip(s_models, o_models)):
        for i, (s, o) in enumerate(zip(s_layers, o_layers)):
            if list(s) != list(o):
                what = lambda l: f"{l[0]} (in {l[1]}, out {l[2]}, rank {l[3]})"
                return f"model {m}, LoRA layer {i}: the checkpoint has {what(s)}, the trainer {what(o)}"
        if len(s_layers) != len(o_layers):
            longer, who = (s_layers, "checkpoint") if len(s_layers) > len(o_layers) else (o_layers, "trainer")
            i = min(len(s_layers), len(o_layers))
            return (f"model {m}: the checkpoint has {len(s_layers)} LoRA layers, the trainer {len(o_layers)}; the first one only "
                    f"the {who} has is layer {i}, {longer[i][0]}")
    if len(s_models) != len(o_models):
        return f"the checkpoint holds LoRA layers of {len(s_models)} model(s), the trainer of {len(o_models)}"
    s_dense, o_dense = [list(d) for d in saved.get("dense", [])], [list(d) for d in own.get("dense", [])]
    if s_dense != o_dense:
        return f"dense parameters: the checkpoint has shapes {s_dense}, the trainer {o_dense}"
    return None


def check_checkpoint_tensors(tensors, expected):
    """`expected`: {name: (shape, dtype)}.  Every one is there with that shape and dtype, nothing else is, and every
    floating-point one is finite."""
    for name, (shape, dtype) in expected.items():
        t = tensors.get(name)
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"checkpoint tensor {name!r} is missing")
        if tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            raise ValueError(f"checkpoint tensor {name!r}: {tuple(t.shape)} {t.dtype}, expected {tuple(shape)} {dtype}")
        if t.is_floating_point() and not bool(torch.isfinite(t).all()):
            raise ValueError(f"checkpoint tensor {name!r} holds a non-finite value")
    extra = sorted(set(tensors) - set(expected))
    if extra:
        raise ValueError(f"checkpoint tensor {extra[0]!r} is not part of this trainer's state")


def check_checkpoint_optimizer(meta, owner: str, optimizer: str, options=None):
    """The file was written under the optimizer this trainer runs ("adamw" where the header is silent) — AdamW's and Prodigy's
    states do not convert — and, under Prodigy, with the same d0: the kernel's `d == d0` test is an exact fp32 comparison, so
    another d0 would silently change which step takes the first, unlimited growth.  The other options are the caller's and go
    through `warn_config_differences`."""
    saved = meta.get("optimizer", "adamw")
    if saved != optimizer:
        raise ValueError(f"{owner}: the checkpoint was written under optimizer={saved!r}, this trainer runs {optimizer!r} — "
                         "their states do not convert")
    if optimizer == "prodigy":
        recorded = meta.get("prodigy")
        d0 = recorded.get("d0") if isinstance(recorded, dict) else None
        if isinstance(d0, bool) or not isinstance(d0, (int, float)) or _f32(d0) != _f32(options["d0"]):
            raise ValueError(f"{owner}: the checkpoint was written with prodigy_d0={d0!r}, this trainer has "
                             f"prodigy_d0={options['d0']!r} — the estimate's first growth is decided by d == d0; build the "
                             "trainer with the file's value")


def check_checkpoint_counters(meta, names):
    """The integer scalars `names` of the metadata, each a non-negative int."""
    for name in names:
        v = meta.get(name)
        if not isinstance(v, int) or isinstance(v, bool) or v < 0:
            raise ValueError(f"checkpoint scalar {name!r} is {v!r}, expected a non-negative integer")
    return [meta[name] for name in names]


def warn_config_differences(owner: str, saved, own):
    """Constructor arguments are the caller's and are not restored: one warning lists those the file records differently.  A
    file from before `zero_terminal_snr` or `max_weight_norm` existed was written without it."""
    saved = {"zero_terminal_snr": False, "max_weight_norm": None, **(saved or {})}
    diff =[f"{k}: checkpoint {saved[k]!r}, trainer {own[k]!r}" for k in own if k in (saved or {}) and saved[k] != own[k]]
    if diff:
        warnings.warn(f"{owner}.load_state_dict: the checkpoint was written with other arguments, which are NOT restored — "
                      + "; ".join(diff))


class StepRecorder:
    """At most one step recorded into a hipGraph, with the static buffers its kernels read.  Per step: `load` (True: the step
    must be recorded), then `record` if need be, then `replay`.  `graph` is None exactly when nothing is recorded."""

    def __init__(self, owner: str):
        self.owner = owner  # names the trainer in the fall-back warning
        self.drop()

    def drop(self):
        self.graph = self.key = self.fp = self.nz = self.drawn = self.inputs = self.cond = self.mask = None
        self.moments = None  # moments-fed with the caller's noise: static (moments, posterior noise) the recording reads
        self.loss = None  # the loss tensor every replay writes
        self.held = None  # what `record`'s `keep` returned: alive as long as the recording is

    def load(self, key, fp, nz: Noising, latents, noise, timesteps, seed, step_key, cond, cond_dtype, mask, moments=None,
             posterior_noise=None) -> bool:
        """Copies one step's inputs into the static buffers (host-launched).  `key`: the shapes and modes of the step; `fp`:
        whatever else a recording bakes in (scalars passed as kernel arguments, addresses of frozen operands).  When either
        differs from the recording's, that recording is dropped and the buffers of this step's mode are allocated first (`cond`:
        hidden states, kept in `cond_dtype`, or token ids); the caller then has to `record`: True.  `moments` in place of
        `latents` (the key has to tell the two apart, and the moments' dtype): with the caller's noise they and the
        `posterior_noise` get static buffers of their own, which the recording's first launch reads."""
        fresh = self.graph is None or self.key != key or self.fp != fp
        sampled = moments is not None and noise is not None
        if moments is not None:
            latents = latents_like(None, moments)  # (shape and device; never read)
        if fresh:
            self.drop()  # the old recording (and the operand buffers it pins) goes before a new one is made
            self.key, self.fp, self.nz, self.drawn = key, fp, nz, noise is None
            dt = nz.dtype if self.drawn else torch.float32
            new = lambda: torch.empty(latents.shape, dtype=dt, device=latents.device)
            self.inputs = (None if sampled else new(), new(),
                           torch.empty(latents.shape[0], dtype=torch.int64, device=latents.device))
            if sampled:
                self.moments = (torch.empty_like(moments), new())
            self.cond = torch.empty_like(cond, dtype=cond_dtype, device=latents.device)
            if mask is not None:
                self.mask = torch.empty_like(raw_mask(mask, latents))
        # `inputs`: (latents, noise, timesteps) of the caller — or, the draw being a launch outside the recording, its results
        # (noisy, target, timesteps)
        values = (latents, noise, timesteps)
        if self.drawn:
            values = noise_prologue(nz, latents, None, None, seed, step_key, moments=moments)
        for buffer, value in zip(self.inputs, values):
            if buffer is not None:
                buffer.copy_(value)
        if sampled:
            self.moments[0].copy_(moments)
            self.moments[1].copy_(posterior_noise)
        self.cond.copy_(cond)  # (hidden states: casts to the compute dtype)
        if mask is not None:
            self.mask.copy_(raw_mask(mask, latents))
        return fresh

    def _run(self, body):
        """body(noisy, target, timesteps, cond, raw mask) on the static buffers: add_noise on the caller's noise is the first
        launch of the recording — behind posterior_sample where the step is fed with moments."""
        if self.drawn:
            noised = self.inputs
        else:
            moments, posterior_noise = self.moments or (None, None)
            noised = noise_prologue(self.nz, *self.inputs, None, None, moments=moments, posterior_noise=posterior_noise)
        return body(*noised, self.cond, self.mask)

    def _capture(self, body, before_capture):
        # warm up on a side stream (solver searches, lazy initialisation, allocator), then record
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._run(body)
        torch.cuda.current_stream().wait_stream(side)
        before_capture()
        graph = torch.cuda.CUDAGraph()
        # With a process group alive, its watchdog thread polls HIP events every now and then; under the default
        # "global" capture mode such a call from ANOTHER thread invalidates the recording (a race that shows up
        # in a few percent of the captures).  "thread_local" keeps the check for this thread only.
        mode = "thread_local" if (dist.is_available() and dist.is_initialized()) else "global"
        with torch.cuda.graph(graph, capture_error_mode=mode):
            self.loss = self._run(body)
        return graph

    def record(self, body, before_capture=lambda: None, keep=lambda: None, undo=lambda: None) -> bool:
        """Records `body` — it gets the static buffers (`_run`), reads nothing else that changes from step to step, and returns
        the loss tensor — after two warm-up passes.  `before_capture()` runs between the warm-up and the capture; `keep()`
        after a successful capture, and what it returns (`held`) lives as long as the recording; `undo()` at the end, captured
        or not: it takes back what the warm-up passes and the capture left behind outside this object.  False when the capture
        failed: a warning, nothing is recorded, and the caller launches from the host from then on."""
        try:
            self.graph = self._capture(body, before_capture)
            self.held = keep()
        except Exception as exc:
            warnings.warn(f"{self.owner}: hipGraph capture failed ({exc!r}); continuing with host-launched steps")
            self.drop()
            return False
        finally:
            undo()
        return True

    def replay(self):
        self.graph.replay()
