"""lora_distill's API surface without a GPU: the `lora_diffusion.cli_svd` alias, svd_distill's signature against the
reference's, output naming, the C entries in header / library / bindings, argument checks before any HIP call."""
import inspect
import os

import pytest

from diffusion_finetuning_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["lora_distill_workspace_bytes", "lora_distill_start", "lora_distill_diff", "lora_distill_rayleigh_ritz",
           "lora_distill_finalize", "lora_quantile_clamp"]


def test_cli_svd_alias_exports_the_reference_names():
    import lora_diffusion.cli_svd as cli

    for name in ("svd_distill", "extract_linear_weights", "_text_lora_path", "_ti_lora_path", "main"):
        assert callable(getattr(cli, name)), name
    import diffusion_finetuning_amd as dfa

    assert dfa.svd_distill is cli.svd_distill and callable(dfa.distill_lora)


def test_svd_distill_signature_matches_the_reference():
    from lora_diffusion.cli_svd import svd_distill

    params = inspect.signature(svd_distill).parameters
    # cli_svd.py:29-36
    assert [(p.name, p.default) for p in params.values()] == [
        ("target_model", inspect.Parameter.empty), ("base_model", inspect.Parameter.empty), ("rank", 4),
        ("clamp_quantile", 0.99), ("device", "cuda:0"), ("save_path", "svd_distill.pt")]


def test_output_paths():
    from lora_diffusion.cli_svd import _text_lora_path, _ti_lora_path

    assert _text_lora_path("svd_distill.pt") == "svd_distill.text_encoder.pt"
    assert _text_lora_path("out/a.b.pt") == "out/a.b.text_encoder.pt"
    assert _ti_lora_path("x.pt") == "x.ti.pt"
    with pytest.raises(AssertionError):
        _text_lora_path("x.safetensors")


def test_a_path_without_diffusers_is_a_clear_import_error(tmp_path):
    try:
        import diffusers  # noqa: F401
        pytest.skip("diffusers is installed")
    except ImportError:
        pass
    from lora_diffusion.cli_svd import svd_distill

    with pytest.raises(ImportError, match="diffusers"):
        svd_distill("some/tuned", "some/base", save_path=str(tmp_path / "o.pt"))


def test_extract_linear_weights_follows_find_modules_order():
    import torch.nn as nn

    from lora_diffusion.cli_svd import extract_linear_weights

    class CLIPAttention(nn.Module):
        def __init__(self):
            super().__init__()
            self.k_proj, self.v_proj = nn.Linear(4, 6), nn.Linear(4, 5)

    m = nn.Sequential(CLIPAttention(), nn.Linear(3, 3), CLIPAttention())
    ws = extract_linear_weights(m, ["CLIPAttention"])
    assert [tuple(w.shape) for w in ws] == [(6, 4), (5, 4), (6, 4), (5, 4)]
    assert ws[0] is m[0].k_proj.weight


def test_entries_are_declared_exported_and_bound_abi_unchanged():
    import ctypes

    header = open(os.path.join(ROOT, "include", "lora_hip.h")).read()
    handle = ctypes.CDLL(nat.library_path())
    for name in ENTRIES:
        assert f" {name}(" in header and hasattr(handle, name) and name in nat.SIGNATURES, name
    assert "cli_svd.py" in header
    assert nat.lib().lora_version() == nat.ABI_VERSION == 9


def test_argument_checks_need_no_gpu():
    lib = nat.lib()
    assert lib.lora_distill_workspace_bytes(320, 768) >= 4 * 32 * (320 + 2 * 768)
    assert lib.lora_distill_workspace_bytes(320, 768) % 256 == 0
    assert lib.lora_distill_workspace_bytes(0, 8) == 0
    fake = 256  # never dereferenced: every check below fails before a launch
    assert lib.lora_distill_start(None, 1, 8, 4, 0, fake, None) == -1
    assert lib.lora_distill_start(fake, 1, 8, 0, 0, fake, None) == -2     # r < 1
    assert lib.lora_distill_start(fake, 1, 3, 4, 0, fake, None) == -2     # r > min(N, K)
    assert lib.lora_distill_start(fake, 1, 320, 17, 0, fake, None) == -5  # r > 16
    assert lib.lora_distill_diff(fake, 1, 64, 0, 7, fake, None) == -1     # unknown dtype
    assert lib.lora_distill_rayleigh_ritz(fake, 1, 3, 4, 1e-5, 0, fake, None) == -1
    assert lib.lora_distill_rayleigh_ritz(fake, 1, 1, 17, 1e-5, 0, fake, None) == -5
    assert lib.lora_distill_finalize(fake, 1, 4, 1.5, 1, fake, fake, None) == -1
    assert lib.lora_distill_finalize(fake, 1, 0, 0.5, 1, fake, fake, None) == -2
    assert lib.lora_quantile_clamp(None, 4, 0.5, None, None) == -1
    assert lib.lora_quantile_clamp(fake, 4, -0.1, None, None) == -1


def test_torch_quantile_arithmetic_the_kernel_restates():
    """The kernel computes rank = fp32(q)·(n−1) in fp32, below = trunc, w = rank − below, and torch's lerp with one fused
    multiply-add per branch; restated here in float64-exact steps and checked against CPU torch."""
    import numpy as np
    import torch

    g = torch.Generator().manual_seed(0)

    def restated(x, q):
        s = torch.sort(x).values.numpy()
        rank = np.float32(np.float32(q) * np.float32(len(s) - 1))
        lo, hi = int(rank), int(np.ceil(rank))
        w = np.float32(rank - np.float32(lo))
        a, b = s[lo], s[hi]
        d = np.float32(b - a)
        if abs(w) < 0.5:
            return np.float32(np.float64(w) * np.float64(d) + np.float64(a))
        return np.float32(np.float64(b) - np.float64(d) * np.float64(np.float32(1) - w))

    for t in range(400):
        n = int(torch.randint(1, 20000, (), generator=g))
        x = torch.randn(n, generator=g) * 0.1
        q = [0.5, 0.9, 0.99, 1.0][t % 4] if t % 2 else float(torch.rand((), generator=g))
        assert np.float32(torch.quantile(x, q).item()) == restated(x, q), (n, q)
