"""Autograd front of the packed-weight 3×3 convolutions (csrc/conv_small.hip, csrc/conv_large.hip).

`conv3x3(x, weight, bias)` is `F.conv2d(x, weight, bias, padding=1)`.  Where the weight is frozen and 16-bit, the stock call
re-lays the same filter bytes (and the activation, to channels-last and back) on every call; there a HIP kernel runs on a
pack of the weight made once, forward and backward-data, reading and writing NCHW: the small family where the pixels are few
and the filters wide (the UNet's 8×8 and 16×16 levels), the large family where the pixels are many (32×32 and 64×64).  One
pack per weight and direction feeds both.  A call takes a HIP path only when weight and bias need no gradient, the dtypes
match, x is NCHW-contiguous from a 16-byte boundary, the shape is covered and a planner of the library (`conv3x3_small_plan`
first, then `conv3x3_large_plan`, both set from measurement) routes the class; everything else is the stock line.  Forward
and backward-data are planned each for its own class, so under "auto" they may run on different families.

Packs are cached per weight tensor in a weak map and validated by (data_ptr, _version, dtype, device): a weight that was moved,
reloaded or written in place is packed again on its next use.  Nothing is packed while the stream is capturing: a call that
finds no valid pack during capture takes the stock path, so `prepack_conv3x3(model)` before recording (LoraTrainer does it at
construction for a model that declares `conv3x3_front = True`, i.e. whose forward calls this front) is what puts the routed
layers of a recorded step on the HIP path."""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable
from torch.utils.weak import WeakIdKeyDictionary

from . import _native as nat

ROUTES = ("auto", "hip", "large", "stock")

_FAMILY = {"hip": "small", "large": "large"}

_packs = WeakIdKeyDictionary()  # weight tensor (by identity) -> (key, forward pack, backward pack)


def _key(weight):
    return (weight.data_ptr(), weight._version, weight.dtype, weight.device)


def _get_packs(weight):
    """(forward pack, backward pack) of `weight`, made now unless the stream is capturing (then None when there is none)."""
    entry = _packs.get(weight)
    key = _key(weight)
    if entry is not None and entry[0] == key:
        return entry[1], entry[2]
    if torch.cuda.is_current_stream_capturing():
        return None
    w = weight.detach()
    entry = (key, nat.conv3x3_small_pack(w, False), nat.conv3x3_small_pack(w, True))
    _packs[weight] = entry
    return entry[1], entry[2]


def _weight_eligible(weight, bias) -> bool:
    if not weight.is_cuda or weight.dtype not in (torch.float16, torch.bfloat16) or weight.dim() != 4:
        return False
    if tuple(weight.shape[2:]) != (3, 3) or weight.shape[0] % 32 or weight.shape[1] % 32 or not weight.is_contiguous():
        return False
    if weight.data_ptr() % 16 or weight.requires_grad:
        return False
    if bias is not None and (bias.requires_grad or bias.dtype != weight.dtype or bias.device != weight.device or
                             bias.shape != weight.shape[:1] or not bias.is_contiguous()):
        return False
    return True


def _supported(x, weight, bias, family="small") -> bool:
    if not _weight_eligible(weight, bias):
        return False
    if x.dim() != 4 or x.dtype != weight.dtype or x.device != weight.device or x.shape[1] != weight.shape[1]:
        return False
    if x.numel() == 0 or not x.is_contiguous() or x.data_ptr() % 16:
        return False
    N, Cin, H, W = x.shape
    Cout = weight.shape[0]
    # the backward-data call is the same kernel with the channel roles swapped: both must be covered
    covers = nat.conv3x3_small_supported if family == "small" else nat.conv3x3_large_supported
    return covers(N, Cin, Cout, H, W, x.dtype) and covers(N, Cout, Cin, H, W, x.dtype)


def _run(family, x, pack, bias, Cout):
    return (nat.conv3x3_small if family == "small" else nat.conv3x3_large)(x, pack, bias, Cout)


def _auto_family(pixels, Cin, Cout, dtype):
    """The family the planners give a class: the small family's planner is asked first.  None: stock."""
    if nat.conv3x3_small_plan(pixels, Cin, Cout, dtype):
        return "small"
    if nat.conv3x3_large_plan(pixels, Cin, Cout, dtype):
        return "large"
    return None


class _Conv3x3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, fwd_pack, bwd_pack, fwd_family, bwd_family):
        ctx.bwd_pack = bwd_pack
        ctx.bwd_family = bwd_family
        ctx.cin = x.shape[1]
        return _run(fwd_family, x, fwd_pack, bias, weight.shape[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        dy = dy.contiguous()
        if dy.data_ptr() % 16:
            dy = dy.clone()
        return (_run(ctx.bwd_family, dy, ctx.bwd_pack, None, ctx.cin),) + (None,) * 6


def conv3x3(x: torch.Tensor, weight: torch.Tensor, bias=None, route: str = "auto") -> torch.Tensor:
    """F.conv2d(x, weight, bias, padding=1) for a 3×3 weight.  route: "auto" (the planners decide, each direction for its own
    class), "hip" (force the small-image kernel) or "large" (force the many-pixel kernel), which raise where the kernel cannot
    run, or "stock"."""
    if route not in ROUTES:
        raise ValueError(f"conv3x3: route must be one of {ROUTES}, got {route!r}")
    if route != "stock":
        fwd = bwd = None
        if route == "auto":
            # a class and its backward form are routed together, but not necessarily to the same family; the planners are
            # table look-ups and are asked first, the shape envelope once per family that they name
            if x.dim() == 4 and weight.dim() == 4 and x.is_cuda:
                N, Cin, H, W = x.shape
                fwd = _auto_family(N * H * W, Cin, weight.shape[0], x.dtype)
                bwd = _auto_family(N * H * W, weight.shape[0], Cin, x.dtype) if fwd is not None else None
                if bwd is None or not all(_supported(x, weight, bias, f) for f in {fwd, bwd}):
                    fwd = bwd = None
        elif _supported(x, weight, bias, _FAMILY[route]):
            fwd = bwd = _FAMILY[route]
        packs = _get_packs(weight) if fwd is not None else None
        if packs is not None:
            return _Conv3x3Fn.apply(x, weight, bias, packs[0], packs[1], fwd, bwd)
        if route != "auto":
            raise RuntimeError(f"conv3x3(route={route!r}): the HIP kernel does not cover this call (needs a frozen 16-bit 3×3 "
                               "weight with channel counts that are multiples of 32, an NCHW-contiguous x of the same dtype "
                               "from a 16-byte boundary, and a pack made before stream capture)")
    return F.conv2d(x, weight, bias, padding=1)


def prepack_conv3x3(module: nn.Module, route: str = "auto") -> int:
    """Packs the weight of every nn.Conv2d under `module` that `conv3x3` could route (3×3, stride 1, padding 1, frozen, 16-bit,
    on the device, and under "auto" a class either family's planner routes at some pixel count; "hip" and "large" pack whatever
    the kernels cover),
    so that a step recorded afterwards finds its packs.  Returns the number of weights packed (or found packed)."""
    if route not in ROUTES:
        raise ValueError(f"prepack_conv3x3: route must be one of {ROUTES}, got {route!r}")
    if route == "stock":
        return 0
    n = 0
    for m in module.modules():
        if type(m) is not nn.Conv2d or m.kernel_size != (3, 3) or m.stride != (1, 1) or m.padding != (1, 1):
            continue
        if m.dilation != (1, 1) or m.groups != 1 or not _weight_eligible(m.weight, m.bias):
            continue
        if route == "auto" and not (nat.conv3x3_small_plan_channels(m.weight.shape[1], m.weight.shape[0], m.weight.dtype) or
                                    nat.conv3x3_large_plan_channels(m.weight.shape[1], m.weight.shape[0], m.weight.dtype)):
            continue
        if _get_packs(m.weight) is not None:
            n += 1
    return n


def packed_bytes() -> int:
    """Bytes the cached packs hold (both directions)."""
    return sum(e[1].numel() * e[1].element_size() + e[2].numel() * e[2].element_size() for e in _packs.values())
