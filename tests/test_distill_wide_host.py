"""svd_distill at ranks 17–64 without a GPU: the lora_distill_wide_* entries in header / library / bindings, their argument
codes (each returned before any launch), the workspace query, and the Python rank limit.  The shapes and planted
spectra are those of the GPU file, shared through tests/distill_wide_cases.py."""
import ctypes
import inspect
import os

import pytest
import torch
import torch.nn as nn

from diffusion_finetuning_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["lora_distill_wide_width", "lora_distill_wide_workspace_bytes", "lora_distill_wide_start",
           "lora_distill_wide_diff", "lora_distill_wide_rayleigh_ritz", "lora_distill_wide_finalize"]
FAKE = 256  # a non-null "pointer" that is never dereferenced: every call below returns before a launch


def test_wide_entries_are_declared_exported_and_bound_version_unchanged():
    header = open(os.path.join(ROOT, "include", "lora_hip.h")).read()
    handle = ctypes.CDLL(nat.library_path())
    for name in ENTRIES:
        assert f" {name}(" in header and hasattr(handle, name) and name in nat.SIGNATURES, name
    assert "cli_svd.py:71-77" in header  # the slice U[:, :rank] the wide entries restate
    assert nat.lib().lora_version() == nat.ABI_VERSION == 9


def test_width_follows_the_rank():
    lib = nat.lib()
    for r in range(1, 65):
        w = lib.lora_distill_wide_width(r)
        assert w in (48, 64, 80) and w >= r + 16 and w % 16 == 0 and w <= 128, (r, w)
        assert nat.distill_width(r) == (32 if r <= 16 else w)
    assert [lib.lora_distill_wide_width(r) for r in (17, 32, 33, 48, 49, 64)] == [48, 48, 64, 64, 80, 80]
    assert lib.lora_distill_wide_width(0) == -2 and lib.lora_distill_wide_width(65) == -5


def test_argument_codes_need_no_gpu():
    lib = nat.lib()
    # -1: null or unknown arguments
    assert lib.lora_distill_wide_start(None, 1, 320, 32, 0, FAKE, None) == -1
    assert lib.lora_distill_wide_start(FAKE, 1, 320, 32, 0, None, None) == -1
    assert lib.lora_distill_wide_start(FAKE, 0, 320, 32, 0, FAKE, None) == -1
    assert lib.lora_distill_wide_diff(None, 1, 64, 0, 1, 32, FAKE, None) == -1
    assert lib.lora_distill_wide_diff(FAKE, 1, 64, 0, 7, 32, FAKE, None) == -1      # unknown dtype
    assert lib.lora_distill_wide_diff(FAKE, 70000, 64, 0, 1, 32, FAKE, None) == -1  # more layers than grid.y holds
    assert lib.lora_distill_wide_rayleigh_ritz(FAKE, 1, 3, 32, 1e-5, 0, FAKE, None) == -1  # unknown side
    assert lib.lora_distill_wide_rayleigh_ritz(FAKE, 1, 1, 32, 1e-5, 0, None, None) == -1
    assert lib.lora_distill_wide_finalize(FAKE, 1, 32, 0.5, 1, FAKE, None, None) == -1
    assert lib.lora_distill_wide_finalize(FAKE, 1, 32, 1.5, 1, FAKE, FAKE, None) == -1     # q outside [0, 1]
    # -2: r < 1 or r > min(N, K)
    assert lib.lora_distill_wide_start(FAKE, 1, 320, 0, 0, FAKE, None) == -2
    assert lib.lora_distill_wide_start(FAKE, 1, 31, 32, 0, FAKE, None) == -2
    assert lib.lora_distill_wide_diff(FAKE, 1, 64, 0, 1, 0, FAKE, None) == -2
    assert lib.lora_distill_wide_rayleigh_ritz(FAKE, 1, 1, 0, 1e-5, 0, FAKE, None) == -2
    assert lib.lora_distill_wide_finalize(FAKE, 1, 0, 0.5, 1, FAKE, FAKE, None) == -2
    # -5: r > 64
    assert lib.lora_distill_wide_start(FAKE, 1, 320, 65, 0, FAKE, None) == -5
    assert lib.lora_distill_wide_start(FAKE, 1, 8, 65, 0, FAKE, None) == -5  # also when min(N, K) is below it
    assert lib.lora_distill_wide_diff(FAKE, 1, 64, 1, 1, 65, FAKE, None) == -5
    assert lib.lora_distill_wide_rayleigh_ritz(FAKE, 1, 2, 65, 1e-5, 0, FAKE, None) == -5
    assert lib.lora_distill_wide_finalize(FAKE, 1, 65, 0.5, 0, FAKE, FAKE, None) == -5
    # the width-32 entries answer as before
    assert lib.lora_distill_start(FAKE, 1, 320, 17, 0, FAKE, None) == -5
    assert lib.lora_distill_rayleigh_ritz(FAKE, 1, 1, 17, 1e-5, 0, FAKE, None) == -5


def test_workspace_query():
    lib = nat.lib()
    for r in (17, 32, 48, 64):
        assert lib.lora_distill_wide_workspace_bytes(0, 8, r) == 0
        assert lib.lora_distill_wide_workspace_bytes(8, 0, r) == 0
    assert lib.lora_distill_wide_workspace_bytes(320, 768, 0) == 0
    assert lib.lora_distill_wide_workspace_bytes(320, 768, 65) == 0
    last = lib.lora_distill_workspace_bytes(320, 768)
    for r in (17, 32, 33, 48, 49, 64):  # widths 48, 48, 64, 64, 80, 80
        w = lib.lora_distill_wide_width(r)
        b = lib.lora_distill_wide_workspace_bytes(320, 768, r)
        assert b % 256 == 0 and b >= last, (r, b, last)
        assert b >= 4 * w * (320 + 2 * 768) + 8 * w * w + 8 * w  # the three blocks, Ũ and λ
        assert nat.distill_workspace_bytes(320, 768, r) == b
        last = b
    assert nat.distill_workspace_bytes(320, 768, 16) == lib.lora_distill_workspace_bytes(320, 768)


class CrossAttention(nn.Module):
    def __init__(self):
        super().__init__()
        self.to_q = nn.Linear(80, 72, bias=False)


def test_rank_above_64_is_refused_by_name_on_cpu_models():
    from diffusion_finetuning_amd.distill import distill_lora

    with pytest.raises(ValueError, match="64"):
        distill_lora(CrossAttention(), CrossAttention(), ["CrossAttention"], rank=65)


def test_svd_distill_signature_is_unchanged():
    from lora_diffusion.cli_svd import svd_distill

    params = inspect.signature(svd_distill).parameters
    assert [(p.name, p.default) for p in params.values()] == [  # cli_svd.py:29-36
        ("target_model", inspect.Parameter.empty), ("base_model", inspect.Parameter.empty), ("rank", 4),
        ("clamp_quantile", 0.99), ("device", "cuda:0"), ("save_path", "svd_distill.pt")]


def test_planted_fixture_satisfies_the_factor_test_precondition():
    """The factor-wise GPU test compares vector i within 2·res/gap_i and refuses bounds above 1e-2.  At res = tol = 1e-5 the
    float64 spectra of the rounded planted differences must leave every bound under that, or the GPU test could only fail."""
    from tests.distill_wide_cases import CASES, neighbour_gaps, planted_pairs, reference_svds

    for dtype in (torch.float32, torch.float16):
        for r, shapes in CASES.items():
            for (_, S, _) in reference_svds(r, dtype):
                gap = neighbour_gaps(S, r)
                assert (2 * 1e-5 / gap).max() <= 1e-2, (dtype, r, gap.min())
            assert len(planted_pairs(r, dtype)) == len(shapes)
