"""Autograd fronts of the fused norms: GroupNorm (+ per-(n,c) addend, + SiLU) of the UNet's convolution trunk (csrc/norm.hip),
the passes at the edges of its blocks that only move or add activations (csrc/trunk_edges.hip, middle of this file), and
residual add + LayerNorm of its transformer blocks (csrc/layer_norm.hip, last part of this file).

The HIP path takes f16 / bf16 tensors on the HIP device that are NCHW-contiguous or channels-last, start on a 16-byte boundary
and whose γ/β are frozen; everything else (CPU, fp32, other strides, an x at an odd offset into its storage, trainable γ/β,
shapes the kernels do not cover) gets the stock composite `F.silu(F.group_norm(x + addend[:, :, None, None]))`, which is what
the caller would have written.  In the backward the forward's choice is already made: a `dy` in the other memory format, or
one that does not start on a 16-byte boundary, is copied once into x's layout and the kernels run on the copy.

The block-edge fronts follow the same rule, each with the stock lines it replaces as its other path:
  * `group_norm_act_res` / `group_norm_tokens` hand x through next to the normalised tensor, so that the gradient of whatever
    else reads x (a ResNet's shortcut, a transformer's exit residual) comes back to the norm's backward as `dh` and is added
    into dx before its one rounding, instead of in an accumulation kernel of autograd's;
  * `group_norm_tokens` / `tokens_to_nchw_add` re-lay [N,C,H,W] ↔ [N, H·W, C] through an LDS tile, the second with the residual
    added on the way;
  * `residual_bias_add` sums a ResNet block's two branches and the biases of their last convolutions in one pass."""
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
    None.  The result has x's memory layout.  On the HIP path one statistics and one apply kernel each way, or a single kernel
    where an NCHW (n, group) slab fits one workgroup's registers (`_native.lib().group_norm_act_plan` tells which)."""
    layout = _hip_layout(x, groups, weight, bias, addend)
    if layout is None:
        h = x if addend is None else x + addend[:, :, None, None]
        h = F.group_norm(h, groups, weight, bias, eps)
        return F.silu(h) if act else h
    if addend is not None and not addend.is_contiguous():
        addend = addend.contiguous()
    return _GroupNormActFn.apply(x, addend, weight, bias, int(groups), float(eps), bool(act), layout)


# ------------------------------------------------------------------------------------ block edges (norm.hip, trunk_edges.hip)
def _norm_res_backward(ctx, dh, dy):
    """Input gradients of a norm whose x was handed through: GroupNorm's dx with dh joined in one launch, or dh alone."""
    x, addend, weight, bias, mean, rstd = ctx.saved_tensors
    want_da = addend is not None and ctx.needs_input_grad[1]
    dx, da = nat.group_norm_act_bwd_res(_dense16(dy), _dense16(dh), x, addend, weight, bias, mean, rstd, ctx.groups, ctx.act,
                                        want_da)
    return dx, da


class _GroupNormActResFn(torch.autograd.Function):
    """(x, y) with y = act(GroupNorm(x + addend)) for an NCHW-contiguous x: the gradient of the x handed through joins dx."""

    @staticmethod
    def forward(ctx, x, addend, weight, bias, groups, eps, act):
        ctx.set_materialize_grads(False)  # a missing dh or dy arrives as None, never as zeros a kernel would have to read
        y, mean, rstd = nat.group_norm_act_fwd(x, addend, weight, bias, groups, eps, act, 0)
        ctx.save_for_backward(x, addend, weight, bias, mean, rstd)
        ctx.groups, ctx.act = groups, act
        return x, y

    @staticmethod
    @once_differentiable
    def backward(ctx, dh, dy):
        if dy is None:  # only the path around the norm carries a gradient: it passes through, no launch
            dx, da = dh, None
        else:
            dx, da = _norm_res_backward(ctx, dh, dy)
        return (dx if ctx.needs_input_grad[0] else None), da, None, None, None, None, None


def group_norm_act_res(x: torch.Tensor, groups: int, weight, bias, eps: float, act: bool, addend=None):
    """(x_pass, y): y = `group_norm_act(x, ...)` and x_pass is x handed through for whatever else reads it.  On the HIP path
    with an NCHW-contiguous x the gradient of x_pass is added into the norm's dx inside its apply kernel; every other case
    (channels-last included) returns (x, group_norm_act(x, ...))."""
    if _hip_layout(x, groups, weight, bias, addend) != 0:
        return x, group_norm_act(x, groups, weight, bias, eps, act, addend)
    if addend is not None and not addend.is_contiguous():
        addend = addend.contiguous()
    return _GroupNormActResFn.apply(x, addend, weight, bias, int(groups), float(eps), bool(act))


class _GroupNormTokensFn(torch.autograd.Function):
    """(x, tokens): identity-activation GroupNorm of an NCHW x, re-laid out as [N, H·W, C] through the LDS tile of
    trunk_edges.hip; the backward brings the token-layout gradient back through the same tile and joins dh."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps):
        ctx.set_materialize_grads(False)
        y, mean, rstd = nat.group_norm_act_fwd(x, None, weight, bias, groups, eps, False, 0)
        ctx.save_for_backward(x, None, weight, bias, mean, rstd)
        ctx.groups, ctx.act = groups, False
        return x, nat.nchw_to_tokens(y)

    @staticmethod
    @once_differentiable
    def backward(ctx, dh, dtok):
        if dtok is None:
            dx = dh
        else:
            dy = nat.tokens_to_nchw_add(_dense16(dtok), None, ctx.saved_tensors[0].shape)
            dx, _ = _norm_res_backward(ctx, dh, dy)
        return (dx if ctx.needs_input_grad[0] else None), None, None, None, None


def group_norm_tokens_supported(x, groups: int, weight, bias) -> bool:
    """Whether `group_norm_tokens` takes the HIP path for these operands (no launch)."""
    if x.dim() != 4 or _hip_layout(x, groups, weight, bias, None) != 0:
        return False
    N, C, H, W = x.shape
    return nat.tokens_nchw_supported(N, C, H * W, x.dtype)


def group_norm_tokens(x: torch.Tensor, groups: int, weight, bias, eps: float):
    """(x_pass, tokens): tokens [N, H·W, C] = GroupNorm(x) in token layout, the bits of `group_norm_act(x, ..., act=False)`
    permuted, and x_pass as in `group_norm_act_res`.  Needs an NCHW-contiguous x with C % 8 == 0 and H·W % 8 == 0 on the HIP
    path; everything else gets `group_norm_act` and the permuted reshape."""
    if not group_norm_tokens_supported(x, groups, weight, bias):
        n, c, h, w = x.shape
        return x, group_norm_act(x, groups, weight, bias, eps, False).permute(0, 2, 3, 1).reshape(n, h * w, c)
    return _GroupNormTokensFn.apply(x, weight, bias, int(groups), float(eps))


class _TokensToNchwAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tok, res):
        ctx.set_materialize_grads(False)
        return nat.tokens_to_nchw_add(tok, res, res.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        if dy is None:
            return None, None
        d_tok = nat.nchw_to_tokens(_dense16(dy)) if ctx.needs_input_grad[0] else None
        return d_tok, (dy if ctx.needs_input_grad[1] else None)  # the residual's gradient is dy itself, no launch


def tokens_to_nchw_add_supported(tok, res) -> bool:
    """Whether `tokens_to_nchw_add` takes the HIP path: dense 16-bit tok [N, H·W, C] and NCHW res from 16-byte boundaries."""
    if res.dim() != 4 or not tok.is_cuda or not res.is_cuda or tok.dtype != res.dtype:
        return False
    N, C, H, W = res.shape
    if tok.shape != (N, H * W, C) or tok.numel() == 0:
        return False
    if not (tok.is_contiguous() and res.is_contiguous()) or tok.data_ptr() % 16 or res.data_ptr() % 16:
        return False
    return nat.tokens_nchw_supported(N, C, H * W, tok.dtype)


def tokens_to_nchw_add(tok: torch.Tensor, res: torch.Tensor) -> torch.Tensor:
    """res + tok re-laid out: out[n,c,h,w] = res[n,c,h,w] + tok[n, h·W + w, c], one pass each way on the HIP path (the backward
    hands dy to res as it is and re-lays it out for tok)."""
    if not tokens_to_nchw_add_supported(tok, res):
        n, c, h, w = res.shape
        return tok.reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous() + res
    return _TokensToNchwAddFn.apply(tok, res)


class _ResidualBiasAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, res, b1, b2):
        ctx.set_materialize_grads(False)
        return nat.residual_bias_add(h, res, b1, b2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):  # both branches get dy itself, no launch
        return (dy if ctx.needs_input_grad[0] else None), (dy if ctx.needs_input_grad[1] else None), None, None


def residual_bias_add(h: torch.Tensor, res: torch.Tensor, b1, b2=None) -> torch.Tensor:
    """res + h + b1[None, :, None, None] (+ b2 likewise): a ResNet block's two branches and the biases their last convolutions
    were run without, in one pass on the HIP path (frozen biases, NCHW-contiguous 16-bit h and res, H·W % 8 == 0)."""
    hip = h.is_cuda and res.is_cuda and b1 is not None and nat.residual_bias_add_supported(h, res, b1, b2)
    if hip and torch.is_grad_enabled() and (b1.requires_grad or (b2 is not None and b2.requires_grad)):
        hip = False  # the kernel produces no bias gradients
    if not hip:
        h = h if b1 is None else h + b1[None, :, None, None]
        return (res if b2 is None else res + b2[None, :, None, None]) + h
    return _ResidualBiasAddFn.apply(h, res, b1, b2)


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
