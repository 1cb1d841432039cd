"""Per-sample LoRA gates, the parts that need no GPU: `stack_lora_lists` against float64, every ValueError of the module level
and that nothing stays installed after one, the inference-only RuntimeError, the sampler's argument checks, the header's new
entries, and the case table of tests/row_scale_cases.py."""
import os
import re

import pytest
import torch
import torch.nn as nn

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd.ops import ROW_SCALES
from tests import row_scale_cases as rc
from tests.conftest import build_tiny_unet
from tests.gemm_cases import CASES, ESIZE, class_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = [(24, 16), (8, 24), (40, 40)]  # (N, K) per layer


def _adapter(rank, seed, layers=LAYERS):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n, k in layers:
        out += [torch.randn(n, rank, generator=g, dtype=torch.float64), torch.randn(rank, k, generator=g, dtype=torch.float64)]
    return out


@pytest.mark.parametrize("ranks", [(4,), (4, 4), (4, 4, 4, 4), (2, 6)], ids=lambda r: "ranks" + "_".join(map(str, r)))
def test_stack_lora_lists_against_float64(ranks):
    """B_stack·diag(g)·A_stack·x == Σ_k g_k·B_k·A_k·x: the same sums in float64, so the bound is float64 rounding."""
    lists = [_adapter(r, 10 + k) for k, r in enumerate(ranks)]
    kept = [[t.clone() for t in l] for l in lists]
    stacked, slots = dfa.stack_lora_lists(lists)
    assert len(stacked) == len(lists[0])
    # the slots partition [0, Σr) in adapter order
    assert slots[0].start == 0 and slots[-1].stop == sum(ranks)
    assert all(a.stop == b.start for a, b in zip(slots, slots[1:]))
    assert [s.stop - s.start for s in slots] == list(ranks)
    g = torch.Generator().manual_seed(1)
    gates = torch.randn(len(ranks), generator=g, dtype=torch.float64)
    diag = torch.zeros(sum(ranks), dtype=torch.float64)
    for k, s in enumerate(slots):
        diag[s] = gates[k]
    for i, (n, kf) in enumerate(LAYERS):
        up, down = stacked[2 * i], stacked[2 * i + 1]
        assert tuple(up.shape) == (n, sum(ranks)) and tuple(down.shape) == (sum(ranks), kf)
        x = torch.randn(kf, 5, generator=g, dtype=torch.float64)
        got = up @ (diag[:, None] * (down @ x))
        want = sum(gates[k] * (lists[k][2 * i] @ (lists[k][2 * i + 1] @ x)) for k in range(len(ranks)))
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12 * float(want.abs().max()))
    assert all(torch.equal(a, b) for l, m in zip(lists, kept) for a, b in zip(l, m))  # the inputs are left alone


def test_stack_lora_lists_errors_name_the_layer():
    a, b = _adapter(4, 1), _adapter(4, 2)
    with pytest.raises(ValueError, match="adapter 1 has 4 tensors"):
        dfa.stack_lora_lists([a, b[:4]])
    with pytest.raises(ValueError):
        dfa.stack_lora_lists([])
    with pytest.raises(ValueError, match="layer 1 .*features"):
        dfa.stack_lora_lists([a, _adapter(4, 2, [(24, 16), (8, 32), (40, 40)])])
    mixed = _adapter(4, 3)
    mixed[4], mixed[5] = _adapter(2, 3)[4], _adapter(2, 3)[5]  # layer 2 of this adapter has another rank
    with pytest.raises(ValueError, match="layer 2 of adapter 1 .*one rank per adapter"):
        dfa.stack_lora_lists([a, mixed])


class Attention(nn.Module):  # (the class NAME is a LoRA target)
    def __init__(self):
        super().__init__()
        self.to_q = nn.Linear(32, 48, bias=False)
        self.to_out = nn.Linear(48, 32)


def _injected(ranks=(4, 4)):
    model = nn.Sequential(Attention(), Attention())
    model.requires_grad_(False)
    dfa.monkeypatch_or_replace_lora(model, _flat_for(model, max(ranks)), r=max(ranks))
    layers = [m for m in model.modules() if type(m).__name__ == "LoraInjectedLinear"]
    return model, layers


def _flat_for(model, r):
    out = []
    for m in model.modules():
        if isinstance(m, nn.Linear):
            out += [torch.zeros(m.out_features, r), torch.zeros(r, m.in_features)]
    return out


def _installed(layers):
    return [l.__dict__.get(ROW_SCALES) for l in layers]


def test_set_lora_row_scales_installs_clears_and_refuses_whole():
    model, layers = _injected()
    assert len(layers) == 4
    table = torch.ones(3, 4)
    dfa.set_lora_row_scales(model, table)
    assert all(t is table for t in _installed(layers))
    dfa.set_lora_row_scales(model, None)
    assert _installed(layers) == [None] * 4
    # the last layer gets a larger rank: a table too narrow for it is refused before ANY layer is touched
    dfa.monkeypatch_or_replace_lora(model[1], _flat_for(nn.Sequential(*[l.linear for l in layers[2:]]), 6), r=6)
    layers = [m for m in model.modules() if type(m).__name__ == "LoraInjectedLinear"]
    assert [l.lora_down.weight.shape[0] for l in layers] == [4, 4, 6, 6]
    with pytest.raises(ValueError, match="rank 6"):
        dfa.set_lora_row_scales(model, torch.ones(3, 5))
    assert _installed(layers) == [None] * 4
    for bad in (torch.ones(3, 6).double(), torch.ones(6), torch.ones(0, 6), [[1.0] * 6], torch.ones(3, 12)[:, ::2]):
        with pytest.raises(ValueError):
            dfa.set_lora_row_scales(model, bad)
        assert _installed(layers) == [None] * 4
    # a refused table leaves the installed one in place; the context manager restores what was there
    first = torch.ones(3, 6)
    dfa.set_lora_row_scales(model, first)
    with pytest.raises(ValueError):
        dfa.set_lora_row_scales(model, torch.ones(3, 5))
    assert all(t is first for t in _installed(layers))
    second = torch.zeros(2, 8)
    with dfa.lora_row_scales(model, second) as t:
        assert t is second and all(x is second for x in _installed(layers))
    assert all(t is first for t in _installed(layers))
    with pytest.raises(ValueError):
        with dfa.lora_row_scales(model, torch.ones(3, 5)):
            raise AssertionError("entered with a refused table")
    assert all(t is first for t in _installed(layers))
    dfa.set_lora_row_scales(model, None)
    assert _installed(layers) == [None] * 4


def test_a_forward_under_grad_mode_raises_while_a_table_is_installed():
    model, layers = _injected()
    x = torch.randn(3, 5, 32)
    dfa.set_lora_row_scales(model, torch.ones(3, 4))
    with pytest.raises(RuntimeError, match="inference-only"):
        layers[0](x)
    with torch.no_grad():  # without grad the call gets as far as the device check (no CPU fallback), not further
        with pytest.raises(RuntimeError, match="HIP device"):
            layers[0](x)
    dfa.set_lora_row_scales(model, None)
    with pytest.raises(RuntimeError, match="HIP device"):
        layers[0](x)


def test_monkeypatch_stack_lora_wraps_with_the_total_rank():
    model = nn.Sequential(Attention())
    model.requires_grad_(False)
    shapes = [(48, 32), (32, 48)]
    lists = [_adapter(4, 1, shapes), _adapter(2, 2, shapes), _adapter(12, 3, shapes)]
    slots = dfa.monkeypatch_stack_lora(model, [[t.float() for t in l] for l in lists])
    assert [(s.start, s.stop) for s in slots] == [(0, 4), (4, 6), (6, 18)]
    layers = [m for m in model.modules() if type(m).__name__ == "LoraInjectedLinear"]
    assert [tuple(l.lora_down.weight.shape) for l in layers] == [(18, 32), (18, 48)]  # above 16: allowed (generic kernels)
    assert torch.equal(layers[0].lora_up.weight[:, slots[1]], lists[1][0].float())
    assert "generic" in dfa.monkeypatch_stack_lora.__doc__ or "shape-agnostic" in dfa.monkeypatch_stack_lora.__doc__
    import lora_diffusion.lora as alias

    for name in ("set_lora_row_scales", "lora_row_scales", "stack_lora_lists", "monkeypatch_stack_lora"):
        assert getattr(alias, name) is getattr(dfa, name)


def test_sampler_checks_its_gates_before_any_device_work():
    unet = build_tiny_unet(seed=5)
    dfa.inject_trainable_lora(unet, r=4)
    sampler = dfa.LatentSampler(unet, num_inference_steps=4)
    cond = torch.zeros(3, 6, 32)
    kw = dict(seed=1, latent_shape=(4, 8, 8))
    with pytest.raises(ValueError, match="lora_scales.*B = 3"):
        sampler.begin(cond, cond, lora_scales=torch.ones(2), **kw)
    with pytest.raises(ValueError, match="lora_scales.*B = 3"):
        sampler.begin(cond, cond, lora_scales=[1.0, 0.5], **kw)
    with pytest.raises(ValueError, match="lora_scales.*B = 3"):
        sampler.begin(cond, cond, lora_scales=torch.ones(3, 4, 1), **kw)
    with pytest.raises(ValueError, match="lora_scales must be float32"):
        sampler.begin(cond, cond, lora_scales=torch.ones(3, dtype=torch.float16), **kw)
    with pytest.raises(ValueError, match="lora_scales must live on the HIP device"):
        sampler.begin(cond, cond, lora_scales=torch.ones(3, 4), **kw)
    with pytest.raises(ValueError, match="lora_scales"):
        sampler.begin(cond, cond, lora_scales="abc", **kw)
    assert sampler.state is None and not any(ROW_SCALES in m.__dict__ for m in unet.modules())


def test_header_declares_the_new_entries():
    header = open(os.path.join(ROOT, "include", "lora_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    rows = re.search(r"int lora_linear_fwd_rows\(([^)]*)\)", flat).group(1)
    assert re.search(r"float scale, const float\* row_scale, int n_samples, int ld_scale, int dtype, void\* workspace ?, "
                     r"int64_t ws_bytes, void\* stream$", rows), rows
    geglu = re.search(r"int lora_linear_geglu_fwd_rows\(([^)]*)\)", flat).group(1)
    assert re.search(r"float scale, const float\* row_scale, int n_samples, int ld_scale, int dtype, void\* stream$", geglu), geglu
    for ref_lines in ("lora.py:49-50", "lora.py:597-600", "utils.py:191-211"):
        assert ref_lines in header
    # every existing signature is as it was: the entries the new ones mirror
    assert "int lora_linear_fwd_ws(const void* X, const void* W, const void* bias , const float* A, const float* B, " in flat
    for name in ("lora_linear_fwd_rows", "lora_linear_geglu_fwd_rows", "ddpm_sample_init_shared", "ddpm_sample_step_shared",
                 "ddpm_sample_init_from_shared", "ddpm_sample_step_keep_shared", "ddpm_sample_multistep_keep_shared"):
        assert name in nat.SIGNATURES and re.search(r"\bint %s\(" % name, flat), name
    assert len(nat.SIGNATURES["lora_linear_fwd_rows"][1]) == len(nat.SIGNATURES["lora_linear_fwd_ws"][1]) + 3
    assert len(nat.SIGNATURES["lora_linear_geglu_fwd_rows"][1]) == len(nat.SIGNATURES["lora_linear_geglu_fwd"][1]) + 3
    for name in ("ddpm_sample_init", "ddpm_sample_step", "ddpm_sample_init_from", "ddpm_sample_step_keep",
                 "ddpm_sample_multistep_keep"):
        assert nat.SIGNATURES[name + "_shared"] == nat.SIGNATURES[name]


def test_case_table_keeps_every_class_at_a_multiple_of_77_rows():
    cases = rc.operator_cases()
    classes = {(ESIZE[d], k[:4]) for k, _, d, _ in cases}
    assert classes == {(e, k[:4]) for e, table in CASES.items() for k in table}
    for key, shape, dtype, r in cases:
        assert shape[0] % rc.RPS == 0 and class_of(shape, ESIZE[dtype]) == key
        assert r <= min(shape[1], shape[2]) and rc.sample_counts(shape[0]) == (shape[0], shape[0] // 77, 1)
        # 77 rows per sample put a boundary strictly inside a 16-row fragment, a 64-row and a 128-row tile
        assert rc.RPS % 16 and rc.RPS % 64 and rc.RPS % 128 and shape[0] >= 2 * rc.RPS
    assert {r for k, _, _, r in cases if k[0] == "generic"} == {1, 4, 16, 20}
    table, which = rc.mixed_table(6, 5, (0.7, -1.25), seed=1)
    assert table.shape == (6, 5) and set(which.tolist()) == {-1, 0, 1} and not table[which == -1].any()
    assert bool((table[which == 0] == 0.7).all()) and bool((table[which == 1] == -1.25).all())
