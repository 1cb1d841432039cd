"""Max-norm constraint on the learned update ΔW = scale·up·down of every LoRA layer (csrc/max_norm.hip, one launch per model):
the per-layer Frobenius norms, and the factors of a layer above a bound scaled back onto it — what the kohya trainers call
`--scale_weight_norms` ("Max-norm constraint").  `LayerNorms` is the launch with its device buffers, used by
`LoraTrainer(max_weight_norm=...)` on its slab; `lora_weight_norms` / `clamp_lora_norms_` serve any injected model.
"""
import math

import torch

from . import _native as nat
from .core import DEFAULT_TARGET_REPLACE, LoraInjectedLinear, _find_modules


class LayerNorms:
    """The device table of `lora_max_norm` over one flat fp32 buffer, with the buffers a launch writes: `stats` [n_layers, 2]
    (norm before the scaling, factor applied) and `counters` (int32 [1]: layers scaled, summed over launches)."""

    def __init__(self, params: torch.Tensor, rows):
        """rows: [(up_off, down_off, K, N, r, scale), ...], element offsets from params.data_ptr()."""
        self.params = params
        self.table = nat.max_norm_table(rows, params.device)
        self.n_layers = len(rows)
        self.max_r = max(int(row[4]) for row in rows)
        self.stats = torch.zeros((self.n_layers, 2), dtype=torch.float32, device=params.device)
        self.counters = torch.zeros(1, dtype=torch.int32, device=params.device)

    @classmethod
    def of_slab(cls, slab) -> "LayerNorms":
        """Every LoRA layer of a `LoraSlab`, at its offsets in `slab.params`, with the `scale` the layer has NOW."""
        rows = []
        for i, layer in enumerate(slab.layers):
            r, K = layer.lora_down.weight.shape
            rows.append((slab.offsets[2 * i][0], slab.offsets[2 * i + 1][0], K, layer.lora_up.weight.shape[0], r, layer.scale))
        return cls(slab.params, rows)

    def launch(self, max_norm: float = math.inf) -> None:
        """One launch, no host sync: `stats` of every layer, and every layer above `max_norm` scaled onto it (inf: none)."""
        nat.lora_max_norm(self.params, self.table, self.max_r, max_norm, self.stats, self.counters)


def _injected_layers(model, target_replace_module):
    layers = [m for _, _, m in _find_modules(model, target_replace_module, search_class=[LoraInjectedLinear])]
    if not layers:
        raise ValueError("No lora injected.")
    return layers


@torch.no_grad()
def _run_on_model(model, target_replace_module, max_norm: float):
    layers = _injected_layers(model, target_replace_module)
    factors = [w for l in layers for w in (l.lora_up.weight, l.lora_down.weight)]
    if any(not w.is_cuda for w in factors):
        raise RuntimeError("lora_weight_norms / clamp_lora_norms_: the model must be on the HIP device — the norms come from a "
                           "HIP kernel and there is no CPU fallback")
    shapes = [(l.lora_down.weight.shape[1], l.lora_up.weight.shape[0], l.lora_down.weight.shape[0], l.scale) for l in layers]
    in_place = all(w.dtype == torch.float32 and w.is_contiguous() and w.device == factors[0].device for w in factors)
    if in_place:
        # fp32 factors (a LoraSlab's views, or separate allocations) are read and scaled where they are: the table addresses
        # them relative to the lowest one
        anchor = min(factors, key=lambda w: w.data_ptr())
        base = anchor.data_ptr()
        offs = [(w.data_ptr() - base) // 4 for w in factors]
        flat = anchor.data.view(-1)
    else:
        # factors held in a 16-bit dtype: measured (and scaled) as an fp32 copy; a scaled layer is rounded back into its dtype
        flat = torch.cat([w.detach().to(factors[0].device, torch.float32).reshape(-1) for w in factors])
        offs, at = [], 0
        for w in factors:
            offs.append(at)
            at += w.numel()
    rows = [(offs[2 * i], offs[2 * i + 1], K, N, r, scale) for i, (K, N, r, scale) in enumerate(shapes)]
    norms = LayerNorms(flat, rows)
    norms.launch(max_norm)
    if in_place and math.isfinite(max_norm):
        for w in factors:  # the kernel wrote behind autograd's back: what caches key on a factor's version must see an update
            torch.autograd.graph.increment_version(w)
    if not in_place and math.isfinite(max_norm):
        for i in (norms.stats[:, 1] != 1.0).nonzero().reshape(-1).tolist():
            for w, off in ((factors[2 * i], offs[2 * i]), (factors[2 * i + 1], offs[2 * i + 1])):
                w.data.copy_(flat[off:off + w.numel()].view(w.shape))
    return norms.stats[:, 0].clone(), norms.stats[:, 1].clone()


def lora_weight_norms(model, target_replace_module=DEFAULT_TARGET_REPLACE) -> torch.Tensor:
    """‖scale·up·down‖_F of every LoraInjectedLinear of `model`, in enumeration order (the `.pt` order): fp32 [n_layers] on the
    model's device, from one HIP launch that reads each factor once and forms no [N,K] product.  Nothing is written.  A model
    that is not on the HIP device raises RuntimeError; ValueError when nothing is injected."""
    return _run_on_model(model, target_replace_module, math.inf)[0]


def clamp_lora_norms_(model, max_norm: float, target_replace_module=DEFAULT_TARGET_REPLACE):
    """In place: every layer whose ‖scale·up·down‖_F exceeds `max_norm` (positive, finite) has BOTH factors multiplied by
    sqrt(max_norm/norm), so its update lands on the bound; a layer inside the bound is not written.  Returns (norms before,
    factors applied), fp32 [n_layers] each.  The packed operands of a drop-in model follow at its next forward, as after any
    parameter update; a model that a `LoraTrainer` owns is re-packed by the trainer's next step (or `trainer.slab.repack()`) —
    during training use `LoraTrainer(max_weight_norm=...)` instead.  Errors as `lora_weight_norms`."""
    from .step import check_max_weight_norm

    if max_norm is None:
        raise ValueError("clamp_lora_norms_ needs a bound; lora_weight_norms measures only")
    return _run_on_model(model, target_replace_module, check_max_weight_norm(max_norm))
