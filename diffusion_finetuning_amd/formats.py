"""LoRA file formats of the `lora_diffusion` API (reference: lora_diffusion/lora.py:12-29, 201-407, 603-610).

Host-side I/O only, byte-compatible with the reference: `.pt` = flat python list [up0, down0, ...] of fp16 CPU
tensors; safetensors = tensors `{name}:{i}:up|down` + metadata `{name}` (JSON list of target classes) and
`{name}:{i}:rank`, textual-inversion embeddings stored under their token with metadata EMBED_FLAG.
"""
import json
import os
from itertools import groupby
from typing import Dict, List, Set, Tuple

import torch
import torch.nn as nn

from .core import DEFAULT_TARGET_REPLACE, EMBED_FLAG, extract_lora_ups_down

try:
    from safetensors.torch import safe_open
    from safetensors.torch import save_file as safe_save

    safetensors_available = True
except ImportError:  # reference: lora.py:12-29
    from .safe_open import safe_open

    def safe_save(tensors, filename, metadata=None):
        raise EnvironmentError(
            "Saving safetensors requires the safetensors library. Please install with pip or similar."
        )

    safetensors_available = False


def stack_lora_lists(lists):
    """K positional `[up0, down0, up1, …]` lists (one per adapter: what a `.pt` file or `parse_safeloras` holds) → one list of
    the same form whose layer i carries ALL adapters side by side along the rank,
        up_i = [up_i⁰ | up_i¹ | …]  [N, Σr],      down_i = [down_i⁰; down_i¹; …]  [Σr, K]
    so that up_i·diag(g)·down_i = Σ_k g_k·up_iᵏ·down_iᵏ for gates g constant on each adapter's slots.  Returns
    (stacked, slots): slots[k] is the `slice` of rank slots adapter k owns (they partition [0, Σr)).  The adapters may differ in
    rank, but each has ONE rank for all its layers; all lists have equal length and, per layer, equal feature sizes — anything
    else is a ValueError naming the layer index.  Pure tensor code (runs on the CPU); the inputs are left alone."""
    lists = [list(l) for l in lists]
    if not lists:
        raise ValueError("stack_lora_lists: no adapters given")
    n = len(lists[0])
    for k, l in enumerate(lists):
        if len(l) != n or n % 2 != 0 or n == 0:
            raise ValueError(f"stack_lora_lists: adapter {k} has {len(l)} tensors, adapter 0 has {n} "
                             "(equal, even, non-zero lengths are required: [up0, down0, up1, ...])")
    ranks = [int(l[1].shape[0]) for l in lists]
    stacked = []
    for i in range(n // 2):
        ups, downs = [l[2 * i] for l in lists], [l[2 * i + 1] for l in lists]
        for k, (u, d) in enumerate(zip(ups, downs)):
            if u.dim() != 2 or d.dim() != 2 or u.shape[1] != ranks[k] or d.shape[0] != ranks[k]:
                raise ValueError(f"stack_lora_lists: layer {i} of adapter {k} has up {tuple(u.shape)} / down {tuple(d.shape)}; "
                                 f"the adapter's rank is {ranks[k]} (one rank per adapter)")
            if u.shape[0] != ups[0].shape[0] or d.shape[1] != downs[0].shape[1]:
                raise ValueError(f"stack_lora_lists: layer {i} of adapter {k} is {d.shape[1]} -> {u.shape[0]} features, "
                                 f"adapter 0 has {downs[0].shape[1]} -> {ups[0].shape[0]}")
        like = ups[0]
        stacked.append(torch.cat([u.detach().to(like.device, like.dtype) for u in ups], dim=1))
        stacked.append(torch.cat([d.detach().to(like.device, like.dtype) for d in downs], dim=0))
    slots, at = [], 0
    for r in ranks:
        slots.append(slice(at, at + r))
        at += r
    return stacked, slots


def save_lora_weight(model, path="./lora.pt", target_replace_module=DEFAULT_TARGET_REPLACE):
    """`.pt`: flat python list [up0, down0, up1, ...] of fp16 CPU tensors (lora.py:201-213)."""
    flat = []
    for up, down in extract_lora_ups_down(model, target_replace_module=target_replace_module):
        flat += [up.weight.to("cpu").to(torch.float16), down.weight.to("cpu").to(torch.float16)]
    torch.save(flat, path)


def save_lora_as_json(model, path="./lora.json"):
    """Nested-list JSON dump of [up0, down0, ...] (lora.py:216-225)."""
    flat = []
    for up, down in extract_lora_ups_down(model):
        flat += [up.weight.detach().cpu().numpy().tolist(), down.weight.detach().cpu().numpy().tolist()]
    with open(path, "w") as f:
        json.dump(flat, f)


def save_safeloras_with_embeds(
    modelmap: Dict[str, Tuple[nn.Module, Set[str]]] = {},
    embeds: Dict[str, torch.Tensor] = {},
    outpath="./lora.safetensors",
):
    """One safetensors file for several models: tensors `{name}:{i}:up|down`, metadata `{name}` = JSON list of
    target classes and `{name}:{i}:rank`; TI embeddings stored under their token with metadata EMBED_FLAG
    (lora.py:228-258)."""
    tensors, meta = {}, {}
    for name, (model, targets) in modelmap.items():
        meta[name] = json.dumps(list(targets))
        for i, (up, down) in enumerate(extract_lora_ups_down(model, targets)):
            meta[f"{name}:{i}:rank"] = str(down.out_features)
            tensors[f"{name}:{i}:up"] = up.weight
            tensors[f"{name}:{i}:down"] = down.weight
    for token, tensor in (embeds or {}).items():  # save_all passes None when save_ti is off
        meta[token] = EMBED_FLAG
        tensors[token] = tensor
    print(f"Saving weights to {outpath}")
    safe_save(tensors, outpath, meta)


def save_safeloras(modelmap: Dict[str, Tuple[nn.Module, Set[str]]] = {}, outpath="./lora.safetensors"):
    return save_safeloras_with_embeds(modelmap=modelmap, outpath=outpath)


def convert_loras_to_safeloras_with_embeds(
    modelmap: Dict[str, Tuple[str, Set[str], int]] = {},
    embeds: Dict[str, torch.Tensor] = {},
    outpath="./lora.safetensors",
):
    """`.pt` lists → one safetensors file; modelmap values are (path, targets, rank) (lora.py:268-302)."""
    tensors, meta = {}, {}
    for name, (path, targets, rank) in modelmap.items():
        meta[name] = json.dumps(list(targets))
        for pos, weight in enumerate(torch.load(path, map_location="cpu", weights_only=True)):
            idx, kind = divmod(pos, 2)
            if kind == 0:
                meta[f"{name}:{idx}:rank"] = str(rank)
                tensors[f"{name}:{idx}:up"] = weight
            else:
                tensors[f"{name}:{idx}:down"] = weight
    for token, tensor in embeds.items():
        meta[token] = EMBED_FLAG
        tensors[token] = tensor
    print(f"Saving weights to {outpath}")
    safe_save(tensors, outpath, meta)


def convert_loras_to_safeloras(modelmap: Dict[str, Tuple[str, Set[str], int]] = {}, outpath="./lora.safetensors"):
    convert_loras_to_safeloras_with_embeds(modelmap=modelmap, outpath=outpath)


def parse_safeloras(safeloras) -> Dict[str, Tuple[List[nn.parameter.Parameter], List[int], List[str]]]:
    """Opened safetensors → {name: ([up0, down0, ...] Parameters, ranks, target classes)}; embeddings are
    skipped; a tensor group without metadata raises ValueError (lora.py:313-371)."""
    meta = safeloras.metadata()
    owner = lambda key: key.split(":")[0]
    keys = sorted(safeloras.keys(), key=owner)
    out = {}
    for name, group in groupby(keys, owner):
        info = meta.get(name)
        if not info:
            raise ValueError(f"Tensor {name} has no metadata - is this a Lora safetensor?")
        if info == EMBED_FLAG:
            continue
        group = list(group)
        ranks = [4] * (len(group) // 2)
        weights = [None] * len(group)
        for key in group:
            _, idx, direction = key.split(":")
            idx = int(idx)
            ranks[idx] = int(meta[f"{name}:{idx}:rank"])
            weights[2 * idx + (direction == "down")] = nn.parameter.Parameter(safeloras.get_tensor(key))
        out[name] = (weights, ranks, json.loads(info))
    return out


def parse_safeloras_embeds(safeloras) -> Dict[str, torch.Tensor]:
    """{token: tensor} for every entry flagged EMBED_FLAG (lora.py:374-392)."""
    meta = safeloras.metadata()
    return {k: safeloras.get_tensor(k) for k in safeloras.keys() if meta.get(k) == EMBED_FLAG}


def load_safeloras(path, device="cpu"):
    return parse_safeloras(safe_open(path, framework="pt", device=device))


def load_safeloras_embeds(path, device="cpu"):
    return parse_safeloras_embeds(safe_open(path, framework="pt", device=device))


def load_safeloras_both(path, device="cpu"):
    handle = safe_open(path, framework="pt", device=device)
    return parse_safeloras(handle), parse_safeloras_embeds(handle)


def lerp_lora_lists(l1: List[torch.Tensor], l2: List[torch.Tensor], alpha: float = 0.5) -> List[torch.Tensor]:
    """LoRA ⊕ LoRA of `lora_add --mode lpl` (lora_diffusion/cli_lora_add.py:44-60) on two positional
    `[up0, down0, up1, ...]` lists: every tensor of `l1` becomes alpha·l1 + (1-alpha)·l2 IN PLACE (`.data` is
    replaced, dtype and device kept, op-by-op rounding as the reference) and the list of merged tensors is returned,
    ready for `torch.save`.  One HIP launch per dtype over the concatenated lists (host tensors are staged through
    the device).  A trailing unpaired tensor is dropped, like the reference's pair zip."""
    from . import _native as nat

    n = 2 * min(len(l1) // 2, len(l2) // 2)
    if n == 0:
        return []
    for x1, x2 in zip(l1[:n], l2[:n]):
        if x1.shape != x2.shape:
            raise RuntimeError(f"lerp_lora_lists: LoRA tensors differ in shape: {tuple(x1.shape)} vs {tuple(x2.shape)}")
    device = nat.staging_device(*l1[:n])
    for dtype in {t.dtype for t in l1[:n]}:
        idx = [i for i in range(n) if l1[i].dtype == dtype]
        a = torch.cat([l1[i].detach().to(device).reshape(-1) for i in idx])
        b = torch.cat([l2[i].detach().to(device, dtype).reshape(-1) for i in idx])
        nat.lora_lerp_(a, b, alpha)
        off = 0
        for i in idx:
            k = l1[i].numel()
            l1[i].data = a[off:off + k].view(l1[i].shape).to(l1[i].device, copy=True)
            off += k
    return list(l1[:n])


CHECKPOINT_KEY = "checkpoint"  # the metadata entry that holds a trainer checkpoint's scalars and layout signature (one JSON string)


def save_checkpoint_file(path, tensors: Dict[str, torch.Tensor], meta: dict):
    """A trainer checkpoint (`LoraTrainer.save_checkpoint`, `InversionTrainer.save_checkpoint`): one safetensors file, the
    tensors as given (CPU), `meta` as one JSON string under CHECKPOINT_KEY.  Written to a temporary name in the target
    directory and moved into place, so that a file already at `path` is whole at every moment, and left as it was when the
    write fails."""
    path = os.fspath(path)
    tmp = os.path.join(os.path.dirname(path) or ".", f".{os.path.basename(path)}.{os.getpid()}.tmp")
    try:
        safe_save({k: v.contiguous() for k, v in tensors.items()}, tmp, {CHECKPOINT_KEY: json.dumps(meta)})
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def load_checkpoint_file(path) -> dict:
    """{"meta": …, "tensors": {name: CPU tensor}} of a file `save_checkpoint_file` wrote — what the trainers' `state_dict()`
    returns.  ValueError when the file holds no checkpoint."""
    handle = safe_open(os.fspath(path), framework="pt", device="cpu")
    raw = (handle.metadata() or {}).get(CHECKPOINT_KEY)
    if raw is None:
        raise ValueError(f"{path}: no trainer checkpoint in this file (metadata entry {CHECKPOINT_KEY!r} is missing)")
    try:
        meta = json.loads(raw)
    except json.JSONDecodeError as exc:
        raise ValueError(f"{path}: the checkpoint's metadata is not JSON ({exc})") from None
    return {"meta": meta, "tensors": {k: handle.get_tensor(k) for k in handle.keys()}}


def _derived_path(path: str, tag: str) -> str:
    assert path.endswith(".pt"), "Only .pt files are supported"
    return ".".join(path.split(".")[:-1] + [tag, "pt"])


def _text_lora_path(path: str) -> str:  # lora.py:603-605
    return _derived_path(path, "text_encoder")


def _ti_lora_path(path: str) -> str:  # lora.py:608-610
    return _derived_path(path, "ti")
