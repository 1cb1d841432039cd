"""Step harness for the textual-inversion phase of PTI: placeholder rows of the token table, no LoRA.

Reproduces train_inversion of lora_diffusion/cli_lora_pti.py (:290-346), the first phase of `train()` (:651-687), one call of
`InversionTrainer.step` per loop iteration (a "micro-step" g = 0, 1, …):

    lr_scheduler.step()                                      → lr_g = lr·λ(g + 1)                      (:293)
    loss = loss_step(...) / accum_iter ; loss.backward()     → fp32, t ~ U[0, 1000·t_multiplier)       (:295-307, :170-247)
    if g % accum_iter == 0: optimizer.step(); zero_grad()    → AdamW, no clipping                      (:311-313)
        clip_ti_decay: w ← normalize(w)·(‖w‖ + λd·(0.4 − ‖w‖)), λd = min(1, 100·lr_g)                  (:318-336)
        every other row ← orig_embeds_params                                                           (:344-346)

Because of the restore, only the P placeholder rows ever differ from the initial table, and AdamW's weight decay and moments
only matter on those rows.  So the update runs on those rows alone (DESIGN.md §"Textual inversion"): `ti_rows_grad` sums
their gradient rows into a [P, D] buffer in a fixed order (the [V, D] table gradient is never formed), `ti_rows_adamw_decay`
applies AdamW and the renormalisation to the P rows of the module's own table; the other rows are never written, so they stay
bit-identical to the initial table with no 200-MB clone and no dense moments.

After `close()` the same text encoder goes to `trainer.LoraTrainer` for perform_tuning (cli_lora_pti.py:693-753): its
TokenTable starts from the module's weight, which holds the learned rows.
"""
import functools
from typing import List, Optional, Sequence

import torch
import torch.nn as nn

from . import _native as nat
from . import step as stp
from .formats import load_checkpoint_file, save_checkpoint_file
from .trainer import NUM_TRAIN_TIMESTEPS, ddpm_alphas_cumprod, ddpm_tables, lr_lambda

TARGET_NORM = 0.4  # clip_ti_decay's target row norm (cli_lora_pti.py:333)


def optimizer_steps_at(micro_step: int, accum_iter: int) -> bool:
    """train_inversion steps the optimizer when `global_step % accum_iter == 0` (:311): at g = 0, accum_iter, 2·accum_iter, …
    The first step therefore sees ONE micro-batch's gradient, every later one `accum_iter` of them."""
    return micro_step % accum_iter == 0


def decay_lambda(lr: float) -> float:
    """λd of clip_ti_decay: min(1, 100·lr_scheduler.get_last_lr()[0]) (:327)."""
    return min(1.0, 100.0 * float(lr))


class _PlaceholderRowsFn(torch.autograd.Function):
    """rows = table[ids] through the HIP gather; backward sums the incoming rows of the placeholder tokens into the trainer's
    [P, D] gradient buffer (ti_rows_grad, always accumulating).  The table's `.grad` is never produced."""

    @staticmethod
    def forward(ctx, ids, weight, trainer, out_dtype):
        ctx.trainer, ctx.ids = trainer, ids
        return nat.embed_rows_fwd(weight.detach(), ids, out_dtype)

    @staticmethod
    def backward(ctx, d_rows):
        t = ctx.trainer
        rows = d_rows.reshape(-1, t.D)
        ids = ctx.ids.reshape(-1)
        nat.ti_rows_grad(rows if rows.is_contiguous() else rows.contiguous(), ids if ids.is_contiguous() else ids.contiguous(),
                         t.slot_ids, t.grad, accumulate=True)
        return None, None, None, None


class InversionTrainer:
    """One object per process, single GPU (train_inversion runs on "cuda:0", cli_lora_pti.py:539).  `step()` is one micro-step
    and returns the reference's `loss` (already divided by `accum_iter`) as a device tensor."""

    def __init__(self, unet: nn.Module, text_encoder: nn.Module, placeholder_token_ids: Sequence[int], lr: float = 5e-4,
                 weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, lr_scheduler: str = "linear",
                 lr_warmup_steps: int = 0, max_train_steps: Optional[int] = 1000, accum_iter: int = 4,
                 clip_ti_decay: bool = True, v_prediction: bool = False, capture_graph: bool = False, process_group=None,
                 snr_gamma: Optional[float] = None, timestep_weights: Optional[torch.Tensor] = None,
                 noise_offset: float = 0.0, zero_terminal_snr: bool = False):
        """Arguments are train()'s for this phase: `lr` = ti_lr, `weight_decay` = weight_decay_ti, `lr_scheduler` /
        `lr_warmup_steps` / `max_train_steps` = lr_scheduler, lr_warmup_steps, max_train_steps_ti (:659-664), `accum_iter` =
        gradient_accumulation_steps (:518,670).  The optimizer is AdamW(betas, eps) over the token table (:651-657).
        Compute dtype: the UNet's conv weights.  fp32 is the reference's (mixed_precision=False, :685) and the parity route;
        bf16 is an opt-in deviation from it; f16 is refused — the reference's phase has no loss scaler.
        capture_graph: record noise → text encoder → UNet → loss → backward → ti_rows_grad once and replay it; the optimizer
        launch and the zeroing of the gradient buffer stay outside the recording.
        `snr_gamma`, `timestep_weights`, `noise_offset`: LoraTrainer's — Min-SNR-γ or the caller's per-timestep loss weights,
        looked up inside the loss kernel, and offset noise in the device draw; extensions beyond the reference.
        `zero_terminal_snr`: LoraTrainer's — the tables of the schedule rescaled to zero SNR at T − 1; needs `v_prediction`."""
        self.zero_terminal_snr = stp.check_zero_terminal_snr(zero_terminal_snr, v_prediction)
        stp.check_objective(snr_gamma, timestep_weights, noise_offset, NUM_TRAIN_TIMESTEPS)
        if process_group is not None:
            raise ValueError("InversionTrainer is single-process, as train_inversion is (cli_lora_pti.py:539)")
        trainable = [n for n, p in unet.named_parameters() if p.requires_grad]
        if trainable:
            raise ValueError(f"the UNet must be frozen during textual inversion (cli_lora_pti.py:638-647); trainable: {trainable[:3]}")
        if not hasattr(text_encoder, "get_input_embeddings"):
            raise ValueError("the text encoder has no get_input_embeddings()")
        emb = text_encoder.get_input_embeddings()
        table = emb.weight
        others = [n for n, p in text_encoder.named_parameters() if p.requires_grad and p is not table]
        if others:
            raise ValueError(f"only the token table may train in this phase (cli_lora_pti.py:638-647); also trainable: {others[:3]}")
        if not table.requires_grad:
            raise ValueError("the token table must have requires_grad: it is the optimizer's parameter (cli_lora_pti.py:651-657)")
        if table.dtype != torch.float32:
            raise ValueError(f"the token table must be fp32 (got {table.dtype})")
        V, D = table.shape
        ids = [int(i) for i in placeholder_token_ids]
        if not 1 <= len(ids) <= nat.TI_MAX_ROWS:
            raise ValueError(f"between 1 and {nat.TI_MAX_ROWS} placeholder ids (got {len(ids)})")
        if any(i < 0 or i >= V for i in ids):
            raise ValueError(f"placeholder ids out of range for the {V}-row token table: {ids}")
        if len(set(ids)) != len(ids):
            raise ValueError(f"placeholder ids repeat: {ids}")
        self.dtype = stp.compute_dtype(unet)
        if self.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"compute dtype {self.dtype}: fp32 (the reference's) or bf16 only — the reference's inversion "
                             "phase has no loss scaler for f16")
        if int(accum_iter) < 1:
            raise ValueError("accum_iter must be >= 1")
        if not table.is_cuda:
            raise RuntimeError("InversionTrainer: the models must be on the HIP device")
        self.unet, self.text_encoder, self.module = unet, text_encoder, emb
        self.placeholder_token_ids = ids
        self.V, self.D, self.P = V, D, len(ids)
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), tuple(betas), float(eps)
        self.lr_lambda = lr_lambda(lr_scheduler, lr_warmup_steps, max_train_steps, lr_init=lr)
        self._scheduler_args = (str(lr_scheduler), int(lr_warmup_steps), None if max_train_steps is None else int(max_train_steps))
        self.accum_iter, self.clip_ti_decay = int(accum_iter), bool(clip_ti_decay)
        self.v_prediction, self.capture_graph = bool(v_prediction), bool(capture_graph)
        self.device = table.device
        self.te_dtype = next((p.dtype for p in text_encoder.parameters() if p is not table), torch.float32)
        self.slot_ids = torch.tensor(ids, dtype=torch.int64, device=self.device)
        self.grad = torch.zeros(self.P, D, dtype=torch.float32, device=self.device)
        self.exp_avg = torch.zeros_like(self.grad)
        self.exp_avg_sq = torch.zeros_like(self.grad)
        self.sqrt_acp, self.sqrt_1macp = ddpm_tables(device=self.device, zero_terminal_snr=self.zero_terminal_snr)
        self.snr_gamma = None if snr_gamma is None else float(snr_gamma)
        self.noise_offset = float(noise_offset)
        self.loss_weights = stp.objective_table(snr_gamma, timestep_weights,
                                                ddpm_alphas_cumprod(zero_terminal_snr=self.zero_terminal_snr), self.v_prediction,
                                                self.device)
        self._timestep_weights_digest = stp.table_digest(timestep_weights)
        self.global_step = 0      # micro-steps taken (train_inversion's global_step)
        self.optimizer_steps = 0  # AdamW steps taken (its bias-correction count)
        self.scheduler_epoch = 0  # LambdaLR.last_epoch
        self._recorder = stp.StepRecorder("InversionTrainer")
        self._prev_forward = emb.__dict__.get("forward")
        emb.forward = functools.partial(self._embed_forward, emb)  # (instance attribute: the class is untouched)

    # -- the token table -------------------------------------------------------------------------------
    def _embed_forward(self, module, input_ids):
        if not module.weight.requires_grad or not torch.is_grad_enabled():
            return nat.embed_rows_fwd(module.weight.detach(), input_ids, self.te_dtype)
        return _PlaceholderRowsFn.apply(input_ids, module.weight, self, self.te_dtype)

    def close(self):
        """Gives the embedding module its own forward back (the learned rows stay in its weight)."""
        if self.module is None:
            return
        self.module.__dict__.pop("forward", None)
        if self._prev_forward is not None:
            self.module.forward = self._prev_forward
        self.module = None
        self._recorder.drop()

    def get_last_lr(self) -> List[float]:
        """`lr_scheduler.get_last_lr()`: the rate of the last micro-step."""
        return [self.lr * float(self.lr_lambda(self.scheduler_epoch))]

    # -- checkpoint and resume -------------------------------------------------------------------------
    def _config(self) -> dict:
        """The constructor arguments a checkpoint records (and a load compares, never restores)."""
        name, warmup, max_steps = self._scheduler_args
        return {"lr": self.lr, "weight_decay": self.weight_decay, "betas": [float(b) for b in self.betas], "eps": self.eps,
                "accum_iter": self.accum_iter, "lr_scheduler": name, "lr_warmup_steps": warmup, "max_train_steps": max_steps,
                "clip_ti_decay": self.clip_ti_decay, "v_prediction": self.v_prediction,
                "zero_terminal_snr": self.zero_terminal_snr, "compute_dtype": str(self.dtype).replace("torch.", ""),
                **stp.objective_config(self.snr_gamma, self._timestep_weights_digest, self.noise_offset)}

    def state_dict(self) -> dict:
        """{"meta", "tensors"} like LoraTrainer's: the P placeholder rows of the table, the [P, D] gradient buffer — so a save
        is allowed at ANY micro-step, train_inversion counts `save_steps` in micro-steps — both moments, and the three
        counters (micro-steps: it keys the device draw; AdamW steps; scheduler epoch).  Every other row of the table is the
        initial one and is not stored.  Raises after `close()`."""
        if self.module is None:
            raise RuntimeError("InversionTrainer.state_dict after close()")
        tensors = {"rows": self.module.weight.data[self.slot_ids].cpu(), "grad": self.grad.cpu(),
                   "exp_avg": self.exp_avg.cpu(), "exp_avg_sq": self.exp_avg_sq.cpu()}
        meta = {"format_version": stp.CHECKPOINT_VERSION, "kind": "InversionTrainer", "global_step": self.global_step,
                "optimizer_steps": self.optimizer_steps, "scheduler_epoch": self.scheduler_epoch,
                "placeholder_token_ids": list(self.placeholder_token_ids), "compute_dtype": str(self.dtype).replace("torch.", ""),
                "world_size": 1, "layout": {"models": [], "dense": [[self.V, self.D]]}, "config": self._config()}
        return {"meta": meta, "tensors": tensors}

    def load_state_dict(self, sd: dict):
        """Continue from a `state_dict()`.  All or nothing: version, kind, the placeholder ids (they must be this trainer's, in
        this order), the table's shape, every tensor's shape, dtype and finiteness are checked first; a mismatch raises
        ValueError and leaves the trainer as it was.  The rows are written into the module's own table and the buffers in
        place, so a live recording is replayed by the next `step()`."""
        if self.module is None:
            raise RuntimeError("InversionTrainer.load_state_dict after close()")
        meta = stp.check_checkpoint_header(sd, "InversionTrainer")
        if meta.get("placeholder_token_ids") != list(self.placeholder_token_ids):
            raise ValueError(f"InversionTrainer: the checkpoint's placeholder ids {meta.get('placeholder_token_ids')} are not "
                             f"this trainer's {list(self.placeholder_token_ids)}")
        diff = stp.layout_difference(meta.get("layout") or {}, {"models": [], "dense": [[self.V, self.D]]})
        if diff is not None:
            raise ValueError(f"InversionTrainer: the checkpoint does not fit this trainer — {diff}")
        counters = stp.check_checkpoint_counters(meta, ("global_step", "optimizer_steps", "scheduler_epoch"))
        shape = ((self.P, self.D), torch.float32)
        tensors = sd["tensors"]
        stp.check_checkpoint_tensors(tensors, {"rows": shape, "grad": shape, "exp_avg": shape, "exp_avg_sq": shape})
        stp.warn_config_differences("InversionTrainer", meta.get("config"), self._config())
        # -- validated: from here on nothing raises --
        self.module.weight.data.index_copy_(0, self.slot_ids, tensors["rows"].to(self.device))
        self.grad.copy_(tensors["grad"])
        self.exp_avg.copy_(tensors["exp_avg"])
        self.exp_avg_sq.copy_(tensors["exp_avg_sq"])
        self.global_step, self.optimizer_steps, self.scheduler_epoch = counters

    def save_checkpoint(self, path):
        """`state_dict()` as one safetensors file, written under a temporary name and moved into place."""
        sd = self.state_dict()
        save_checkpoint_file(path, sd["tensors"], sd["meta"])

    def load_checkpoint(self, path):
        self.load_state_dict(load_checkpoint_file(path))

    # -- one micro-step ------------------------------------------------------------------------------
    def step(self, latents=None, noise=None, timesteps=None, *, input_ids, mask=None, seed: Optional[int] = None,
             t_multiplier: float = 1.0, moments=None, posterior_noise=None, latent_scale: float = 0.18215):
        """latents fp32 [B,4,h,w] on the device; input_ids int64 [B, L].  Noise: pass `noise` and `timesteps` (the caller drew
        them, as loss_step does, :186-195) or neither and a `seed` — the device draw is then keyed by (seed, micro-step), so the
        micro-batches of one accumulation window get different noise.  `mask`: raw [B,1,8h,8w] mask (:222-247).
        `moments` [B,8,h,w] (the VAE encoder's mean | logvar) in place of `latents`: the micro-step draws the latents itself,
        `latent_dist.sample() * latent_scale` (:180-184) — in the launch of the device draw, or from the caller's
        `posterior_noise` (fp32, shaped like the latents) where the caller passes `noise` and `timesteps`."""
        if self.module is None:
            raise RuntimeError("InversionTrainer.step after close()")
        stp.check_noise_inputs(latents, moments, noise, timesteps, posterior_noise, seed)
        stp.check_noise_offset(self.noise_offset, noise)
        if input_ids.device.type == "cpu" and input_ids.numel():
            if int(input_ids.min()) < 0 or int(input_ids.max()) >= self.V:
                raise IndexError(f"token id out of range for the {self.V}-row embedding table")
        ids = input_ids.to(self.device, torch.int64)
        nz = stp.Noising(self.sqrt_acp, self.sqrt_1macp, self.dtype, self.v_prediction,
                         max(1, int(self.sqrt_acp.numel() * float(t_multiplier))), float(latent_scale), self.noise_offset,
                         self.loss_weights)
        self._drawn_from = (moments, posterior_noise)
        g = self.global_step
        self.scheduler_epoch += 1  # lr_scheduler.step() comes first (:293)
        lr_g = self.lr * float(self.lr_lambda(self.scheduler_epoch))
        if self.capture_graph:
            loss = self._step_graph(latents, noise, timesteps, ids, mask, seed, g, nz)
        else:
            loss = self._step_eager(latents, noise, timesteps, ids, mask, seed, g, nz)
        if optimizer_steps_at(g, self.accum_iter):
            self.optimizer_steps += 1
            nat.ti_rows_adamw_decay(self.module.weight.data, self.slot_ids, self.grad, self.exp_avg, self.exp_avg_sq, 1.0, lr_g,
                                    self.betas[0], self.betas[1], self.eps, self.weight_decay, self.optimizer_steps,
                                    decay_lambda(lr_g) if self.clip_ti_decay else -1.0, TARGET_NORM)
            self.grad.zero_()
        self.global_step += 1
        return loss

    def _forward_backward(self, noisy, target, timesteps, ids, raw_mask):
        """text encoder → UNet → fused MSE (gradient scaled by 1/accum_iter) → backward, which ends in ti_rows_grad.
        Returns the unscaled loss."""
        ehs = self.text_encoder(ids)[0].to(self.dtype)
        pred = self.unet(noisy, timesteps, ehs).sample
        return stp.loss_backward(pred, target, raw_mask, pred.shape[0], 0, 1.0, 1.0 / self.accum_iter, timesteps,
                                 self.loss_weights)

    def _step_eager(self, latents, noise, timesteps, ids, mask, seed, g, nz):
        moments, posterior_noise = self._drawn_from
        noisy, target, t = stp.noise_prologue(nz, latents, noise, timesteps, seed, g, moments, posterior_noise)
        loss = self._forward_backward(noisy, target, t, ids, stp.raw_mask(mask, stp.latents_like(latents, moments)))
        return loss / self.accum_iter

    # -- the same micro-step replayed from a hipGraph ---------------------------------------------------
    @property
    def _graph(self):
        """The live recording; None exactly when there is none."""
        return self._recorder if self._recorder.graph is not None else None

    def _fingerprint(self):
        """What a recording bakes in besides the shapes: scalars passed as kernel arguments and the address of the table the
        gather reads."""
        return (self.v_prediction, self.accum_iter, self.module.weight.data_ptr(), self.noise_offset,
                stp.table_identity(self.loss_weights))

    def _step_graph(self, latents, noise, timesteps, ids, mask, seed, g, nz):
        moments, posterior_noise = self._drawn_from
        key = (tuple(stp.latents_like(latents, moments).shape), tuple(ids.shape), noise is None, mask is not None)
        if moments is not None:
            key += ("moments", moments.dtype, float(nz.scale))
        rec = self._recorder
        if rec.load(key, self._fingerprint(), nz, latents, noise, timesteps, seed, g, ids, None, mask, moments, posterior_noise):
            saved = self.grad.clone()  # the warm-up passes accumulate into the buffer: what the window holds so far is kept
            if not rec.record(self._forward_backward, undo=lambda: self.grad.copy_(saved)):
                self.capture_graph = False  # keep training: host-launched micro-steps from here on
                return self._step_eager(latents, noise, timesteps, ids, mask, seed, g, nz)
        rec.replay()
        return rec.loss / self.accum_iter
