"""Autograd fronts of the fused norms: GroupNorm (+ per-(n,c) addend, + SiLU) of the UNet's convolution trunk (csrc/norm.hip)
and residual add + LayerNorm of its transformer blocks (csrc/layer_norm.hip, second half of this file).

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


# ------------------------------------------------------------------------------------ residual add + LayerNorm (layer_norm.hip)
class _AddLayerNormFn(torch.autograd.Function):
    """(h, y) = (x + delta, LayerNorm(h)) with delta, or y = LayerNorm(x) without: one launch each way."""

    @staticmethod
    def forward(ctx, x, delta, weight, bias, eps):
        # a missing dh or dy arrives as None, never as a tensor of zeros that a kernel would have to read
        ctx.set_materialize_grads(False)
        h, y, mean, rstd = nat.add_layer_norm_fwd(x, delta, weight, bias, eps)
        # h (x where there is no delta) is saved, not the normalised tensor: the backward recomputes it from h, mean and rstd
        ctx.save_for_backward(x if delta is None else h, weight, mean, rstd)
        return y if delta is None else (h, y)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        dh, dy = grads if len(grads) == 2 else (None, grads[0])
        if dy is None:  # only the residual path carries a gradient: it passes through, no launch
            dx = dh
        else:
            h, weight, mean, rstd = ctx.saved_tensors
            dy, dh = _dense16(dy), _dense16(dh)
            dx = nat.add_layer_norm_bwd(dy, dh, h, weight, mean, rstd)
        return (dx if ctx.needs_input_grad[0] else None), (dx if ctx.needs_input_grad[1] else None), None, None, None


def _dense16(g):
    """An upstream gradient as the kernels read it: dense rows from a 16-byte boundary, copied once when it is not."""
    if g is None:
        return None
    g = g.contiguous()
    return g.clone() if g.data_ptr() % 16 else g


def _hip_layer_norm(x, delta, weight, bias):
    """Whether these operands take the HIP path; everything else gets the stock composite."""
    if not x.is_cuda or x.dtype not in (torch.float16, torch.bfloat16) or weight is None or bias is None:
        return False
    if torch.is_grad_enabled() and (weight.requires_grad or bias.requires_grad):
        return False  # the kernels produce no γ/β gradients
    for p in (weight, bias):
        if p.dtype != x.dtype or p.shape != x.shape[-1:] or not p.is_contiguous() or p.data_ptr() % 16:
            return False
    if delta is not None and (delta.dtype != x.dtype or delta.shape != x.shape or not nat.add_layer_norm_supported(delta)):
        return False
    return nat.add_layer_norm_supported(x)


def add_layer_norm(x: torch.Tensor, delta: torch.Tensor, weight, bias, eps: float):
    """(h, y) with h = x + delta and y = LayerNorm(h) over the last dimension: the residual sum and the normalised tensor the
    next sublayer reads, in one pass each way on the HIP path (the backward joins the gradient of h into dx)."""
    if not _hip_layer_norm(x, delta, weight, bias):
        h = x + delta
        return h, F.layer_norm(h, (h.shape[-1],), weight, bias, eps)
    return _AddLayerNormFn.apply(x, delta, weight, bias, float(eps))


def layer_norm(x: torch.Tensor, weight, bias, eps: float) -> torch.Tensor:
    """LayerNorm(x) over the last dimension; the same kernels without the add."""
    if not _hip_layer_norm(x, None, weight, bias):
        return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)
    return _AddLayerNormFn.apply(x, None, weight, bias, float(eps))
