"""What `trainer.LoraTrainer` and `inversion.InversionTrainer` share of a training step: the DDPM noise prologue, the masked
loss with its backward pass, and the recording of a step into a hipGraph.  Nothing here knows which trainer is calling."""
import warnings
from typing import NamedTuple

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


def noise_prologue(nz: Noising, latents, noise, timesteps, seed, step_key):
    """(noisy, target, timesteps): from the caller's `noise` and `timesteps`, or — `noise` None — drawn on the device in the
    same launch, Philox keyed by (seed, step_key), timesteps uniform."""
    if noise is None:
        return nat.ddpm_noise_prologue(latents, nz.sqrt_acp, nz.sqrt_1macp, nz.dtype, seed, step_key, nz.v_prediction,
                                       nz.n_timesteps)
    noisy, target = nat.ddpm_add_noise(latents, noise, timesteps, nz.sqrt_acp, nz.sqrt_1macp, nz.dtype, nz.v_prediction)
    return noisy, target, timesteps


def raw_mask(mask, like):
    """The raw mask of cli_lora_pti.py:222-247 as `lora_mask_prepare` reads it: fp32 [rows,1,8h,8w], contiguous, on the device
    of `like` (the latents or the prediction, [rows,C,h,w]).  None stays None."""
    if mask is None:
        return None
    return mask.to(like.device).reshape(like.shape[0], 1, like.shape[2] * 8, like.shape[3] * 8).float().contiguous()


def loss_backward(pred, target, raw, n_inst, n_prior, prior_weight, grad_scale):
    """Fused (masked) MSE of the prediction and the backward pass from it, the gradient scaled by `grad_scale`.  Returns the
    unscaled loss."""
    m = nat.lora_mask_prepare(raw, pred.shape[2], pred.shape[3]) if raw is not None else None
    pred_c = pred if pred.is_contiguous() else pred.contiguous()
    loss, dpred = nat.ddpm_mse_fwd_bwd(pred_c, target, m, n_inst, n_prior, prior_weight, grad_scale)
    pred_c.backward(dpred)
    return loss


class StepRecorder:
    """At most one step recorded into a hipGraph, with the static buffers its kernels read.  Per step: `load` (True: the step
    must be recorded), then `record` if need be, then `replay`.  `graph` is None exactly when nothing is recorded."""

    def __init__(self, owner: str):
        self.owner = owner  # names the trainer in the fall-back warning
        self.drop()

    def drop(self):
        self.graph = self.key = self.fp = self.nz = self.drawn = self.inputs = self.cond = self.mask = None
        self.loss = None  # the loss tensor every replay writes
        self.held = None  # what `record`'s `keep` returned: alive as long as the recording is

    def load(self, key, fp, nz: Noising, latents, noise, timesteps, seed, step_key, cond, cond_dtype, mask) -> bool:
        """Copies one step's inputs into the static buffers (host-launched).  `key`: the shapes and modes of the step; `fp`:
        whatever else a recording bakes in (scalars passed as kernel arguments, addresses of frozen operands).  When either
        differs from the recording's, that recording is dropped and the buffers of this step's mode are allocated first (`cond`:
        hidden states, kept in `cond_dtype`, or token ids); the caller then has to `record`: True."""
        fresh = self.graph is None or self.key != key or self.fp != fp
        if fresh:
            self.drop()  # the old recording (and the operand buffers it pins) goes before a new one is made
            self.key, self.fp, self.nz, self.drawn = key, fp, nz, noise is None
            dt = nz.dtype if self.drawn else torch.float32
            self.inputs = (torch.empty_like(latents, dtype=dt), torch.empty_like(latents, dtype=dt),
                           torch.empty(latents.shape[0], dtype=torch.int64, device=latents.device))
            self.cond = torch.empty_like(cond, dtype=cond_dtype, device=latents.device)
            if mask is not None:
                self.mask = torch.empty_like(raw_mask(mask, latents))
        # `inputs`: (latents, noise, timesteps) of the caller — or, the draw being a launch outside the recording, its results
        # (noisy, target, timesteps)
        values = (latents, noise, timesteps)
        if self.drawn:
            values = noise_prologue(nz, latents, None, None, seed, step_key)
        for buffer, value in zip(self.inputs, values):
            buffer.copy_(value)
        self.cond.copy_(cond)  # (hidden states: casts to the compute dtype)
        if mask is not None:
            self.mask.copy_(raw_mask(mask, latents))
        return fresh

    def _run(self, body):
        """body(noisy, target, timesteps, cond, raw mask) on the static buffers: add_noise on the caller's noise is the first
        launch of the recording."""
        noised = self.inputs if self.drawn else noise_prologue(self.nz, *self.inputs, None, None)
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
