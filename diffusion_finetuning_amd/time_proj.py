"""Front of the batched time-embedding projections (csrc/time_proj.hip): what every ResNet block adds to its hidden state,
`time_emb_proj(silu(temb)) + conv1.bias`, for all blocks of a UNet in one launch.

The branch depends on nothing in the trunk and its weights are frozen, so a model computes it once at the top of its forward
and hands each block its [N, C_l] addend.  The HIP path is taken only where it is what the kernel covers: a contiguous 16-bit
CUDA `temb` that needs no gradient, frozen contiguous weights and biases of that dtype on that device, N <= 16 and E % 8 == 0.
Everything else (the CPU, fp32, a trainable projection, fp32 modules under autocast) gets, per layer, exactly the stock lines
`F.linear(F.silu(temb), w, b) + extra_bias` and never touches the library."""
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _native as nat

Layer = Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]  # (weight [C, E], bias [C] | None, extra_bias [C] | None)


def _frozen_dense(t, like, shape) -> bool:
    return (t.dtype == like.dtype and t.device == like.device and tuple(t.shape) == shape and t.is_contiguous()
            and not t.requires_grad)


def time_projections_supported(temb: torch.Tensor, layers: Sequence[Layer]) -> bool:
    """Whether `time_projections` runs these on the HIP kernel (no launch)."""
    if not (temb.is_cuda and temb.dim() == 2 and temb.dtype in (torch.float16, torch.bfloat16) and temb.is_contiguous()
            and temb.numel() > 0 and len(layers) > 0):
        return False
    if temb.requires_grad and torch.is_grad_enabled():
        return False
    N, E = temb.shape
    for w, b, cb in layers:
        if w.dim() != 2 or w.shape[0] < 1 or not _frozen_dense(w, temb, (w.shape[0], E)) or w.data_ptr() % 16:
            return False
        for v in (b, cb):
            if v is not None and not _frozen_dense(v, temb, (w.shape[0],)):
                return False
    return temb.data_ptr() % 16 == 0 and nat.time_proj_supported(N, E, temb.dtype)


def time_projections(temb: torch.Tensor, layers: Sequence[Layer]) -> List[torch.Tensor]:
    """[silu(temb) @ w.T + bias + extra_bias for (w, bias, extra_bias) in layers], each [N, C_l]; on the HIP path views of one
    allocation, fp32 sums with one rounding."""
    if time_projections_supported(temb, layers):
        return nat.time_proj_all(temb, [w for w, _, _ in layers], [b for _, b, _ in layers], [cb for _, _, cb in layers])
    outs = []
    for w, b, cb in layers:
        h = F.linear(F.silu(temb), w, b)
        outs.append(h if cb is None else h + cb)
    return outs
