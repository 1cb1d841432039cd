"""CPU-only checks of the fp32 attention core's fronts (csrc/attn_f32.hip, sandwich.f32_attention, the fp32 keyword of
attention.set_use_hip_attention): nothing here needs a GPU, and nothing may reach a kernel."""
import inspect
import os
import re

import pytest
import torch

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import attention
from diffusion_finetuning_amd.sandwich import f32_attention, f32_attention_supported
from tests.attention_f32_cases import INSTANTIATIONS, OPERATOR_SHAPES, df_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source():
    with open(os.path.join(ROOT, "diffusion_finetuning_amd", "csrc", "attn_f32.hip")) as f:
        return f.read()


def test_every_compiled_instantiation_has_a_test_shape():
    src = _source()
    compiled = {int(x) for x in re.findall(r"(?<!#define )\bF32_CASE\(\s*(\d+)\s*\)", src)}
    assert compiled and set(INSTANTIATIONS) == compiled
    for df, shape in INSTANTIATIONS.items():
        assert df_of(shape[4]) == df and shape in [s[:5] for s in OPERATOR_SHAPES]
    assert {df_of(d) for d in range(8, 161, 8)} == compiled  # the plan reaches every one of them and nothing else
    plan = src[src.index("int plan_f32("):src.index("template <int DF> constexpr int f32_lds")]
    for top, df in ((32, 2), (48, 3), (64, 4), (96, 6), (128, 8)):
        assert f"if (d <= {top}) return {df};" in plan
    assert "return 10;" in plan and "d < 8 || (d % 8) != 0 || d > 160" in plan


def test_envelope_is_decided_on_the_host():
    lib = nat.lib()
    assert lib.attn_f32_supported(1, 1, 1, 1, 8) == 1 and lib.attn_f32_supported(2, 9216, 77, 5, 160) == 1
    for d in (0, 4, 12, 168, 164):
        assert lib.attn_f32_supported(1, 16, 16, 1, d) == 0
    assert lib.attn_f32_supported(1, 0, 16, 1, 64) == 0 and lib.attn_f32_supported(1, 16, 0, 1, 64) == 0
    # bad arguments are refused before any HIP call
    assert lib.attn_f32_fwd(None, None, None, None, None, 1, 16, 16, 1, 64, 0.125, None) == -1
    assert lib.attn_f32_bwd(*([None] * 10), 1, 16, 16, 1, 64, 0.125, None) == -1
    assert lib.attn_f32_bwd_workspace_bytes(2, 100, 3) == 2 * 100 * 3 * 4 and lib.attn_f32_bwd_workspace_bytes(0, 1, 1) == -1


def test_f32_attention_refuses_cpu_tensors():
    q = torch.randn(1, 5, 16)
    assert not f32_attention_supported(q, q, 1)
    with pytest.raises(RuntimeError):
        f32_attention(q, q, q, 1)
    with pytest.raises(RuntimeError):
        nat.attn_f32_fwd(q, q, q, 1, 0.25)


def test_fp32_keyword_defaults_to_off_and_the_reference_named_hook_never_sets_it():
    assert inspect.signature(attention.set_use_hip_attention).parameters["fp32"].default is False
    assert list(inspect.signature(attention.set_use_memory_efficient_attention_xformers).parameters) == ["module", "valid"]
    from harness.unet import BasicTransformerBlock

    blk = BasicTransformerBlock(32, 2, 16, 24)
    attention.set_use_hip_attention(blk, True)
    assert attention._FP32 not in blk.attn1.__dict__
    assert attention.set_use_hip_attention(blk, True, fp32=True) == 0  # idempotent: nothing new installed, the flag set
    assert blk.attn1.__dict__[attention._FP32] and blk.attn2.__dict__[attention._FP32]
    attention.set_use_memory_efficient_attention_xformers(blk, True)
    assert attention._FP32 not in blk.attn1.__dict__
    attention.set_use_hip_attention(blk, True, fp32=True)
    assert attention.set_use_hip_attention(blk, False) == 2
    assert attention._FP32 not in blk.attn1.__dict__ and "forward" not in blk.attn1.__dict__


def test_a_switched_fp32_block_on_the_cpu_is_handed_back_bit_identically():
    from harness.unet import BasicTransformerBlock

    torch.manual_seed(0)
    blk = BasicTransformerBlock(32, 2, 16, 24)
    x, ctx = torch.randn(2, 10, 32), torch.randn(2, 7, 24)
    want = blk(x, ctx)
    assert attention.set_use_hip_attention(blk, True, fp32=True) == 2
    assert torch.equal(blk(x, ctx), want)
    attention.set_use_hip_attention(blk, False)
    assert torch.equal(blk(x, ctx), want)


def test_product_still_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "diffusion_finetuning_amd")
    for name in ("attention.py", "sandwich.py", "_native.py"):
        src = open(os.path.join(pkg, name)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), name
