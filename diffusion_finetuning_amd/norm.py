"""Autograd front of the fused GroupNorm (+ per-(n,c) addend, + SiLU) of the UNet's convolution trunk (csrc/norm.hip).

The HIP path takes f16 / bf16 tensors on the HIP device that are NCHW-contiguous or channels-last, start on a 16-byte boundary
and whose γ/β are frozen; everything else (CPU, fp32, other strides, an x at an odd offset into its storage, trainable γ/β,
shapes the kernels do not cover) gets the stock composite `F.silu(F.group_norm(x + addend[:, :, None, None]))`, which is what
the caller would have written.  In the backward the forward's choice is already made: a `dy` in the other memory format, or
one that does not start on a 16-byte boundary, is copied once into x's layout and the kernels run on the copy."""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _native as nat


class _GroupNormActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, addend, weight, bias, groups, eps, act, layout):
        y, mean, rstd = nat.group_norm_act_fwd(x, addend, weight, bias, groups, eps, act, layout)
        # x is saved, not the normalised tensor: the backward recomputes it (and SiLU') from x, mean and rstd
        ctx.save_for_backward(x, addend, weight, bias, mean, rstd)
        ctx.groups, ctx.act, ctx.layout = groups, act, layout
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, addend, weight, bias, mean, rstd = ctx.saved_tensors
        fmt = torch.channels_last if ctx.layout else torch.contiguous_format
        dy = dy.contiguous(memory_format=fmt)
        if dy.data_ptr() % 16:  # dense but at an odd offset into its storage: the kernels read 16-byte chunks
            dy = dy.clone(memory_format=fmt)
        want_da = addend is not None and ctx.needs_input_grad[1]
        dx, da = nat.group_norm_act_bwd(dy, x, addend, weight, bias, mean, rstd, ctx.groups, ctx.act, ctx.layout, want_da)
        return (dx if ctx.needs_input_grad[0] else None), da, None, None, None, None, None, None


def _hip_layout(x, groups, weight, bias, addend):
    """The layout code of the HIP path for these operands, or None when they get the stock composite."""
    if not x.is_cuda or x.dtype not in (torch.float16, torch.bfloat16) or weight is None or bias is None:
        return None
    if torch.is_grad_enabled() and (weight.requires_grad or bias.requires_grad):
        return None  # the kernels produce no γ/β gradients
    for p in (weight, bias):
        if p.dtype != x.dtype or p.dim() != 1 or p.shape[0] != x.shape[1] or not p.is_contiguous():
            return None
    if addend is not None and (addend.dtype != x.dtype or addend.shape != x.shape[:2]):
        return None
    layout = nat.group_norm_act_layout(x)
    return layout if nat.group_norm_act_supported(x, groups, layout) else None


def group_norm_act(x: torch.Tensor, groups: int, weight, bias, eps: float, act: bool, addend=None) -> torch.Tensor:
    """act(GroupNorm(x + addend[:, :, None, None])) for x [N,C,H,W]; `act` True = SiLU, False = identity; `addend` [N,C] or
    None.  The result has x's memory layout.  One statistics and one apply kernel each way on the HIP path."""
    layout = _hip_layout(x, groups, weight, bias, addend)
    if layout is None:
        h = x if addend is None else x + addend[:, :, None, None]
        h = F.group_norm(h, groups, weight, bias, eps)
        return F.silu(h) if act else h
    if addend is not None and not addend.is_contiguous():
        addend = addend.contiguous()
    return _GroupNormActFn.apply(x, addend, weight, bias, int(groups), float(eps), bool(act), layout)
