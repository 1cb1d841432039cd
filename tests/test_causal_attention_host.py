"""CPU-only guards for the causal attention core (csrc/attn_causal.hip) and its switch:

(a) the table of tests/causal_attention_cases.py names exactly the `CAUSAL_CASE` instantiations, and the planner mirror
    reaches every one of them and nothing else;
(b) `set_use_hip_attention` recognises transformers' CLIPAttention, is idempotent, restores the class forward, and on the
    CPU hands every call back (bit-identical output);
(c) the float64 causal reference of the GPU tests is torch's own causal attention, and the three-bar `close` check at the
    GPU tests' bounds rejects the bug those tests exist for: a row that attends one key past its diagonal."""
import os
import re

import pytest
import torch

from tests.causal_attention_cases import INSTANTIATIONS, causal_chunks, causal_key, causal_reference

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffusion_finetuning_amd", "csrc")
TOLS = {torch.float16: 2e-3, torch.bfloat16: 1.2e-2}  # the attn_ctx bounds of tests/test_gpu_attention_cores.py


def _source():
    with open(os.path.join(CSRC, "attn_causal.hip")) as f:
        return f.read()


def test_table_is_the_dispatch_table_and_the_plan_reaches_all_of_it_and_nothing_else():
    uses = re.findall(r"(?<!#define )\bCAUSAL_CASE\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)", _source())
    compiled = [tuple(int(x) for x in u) for u in uses]
    assert len(compiled) == len(set(compiled)) == 8
    assert set(INSTANTIATIONS) == set(compiled)
    for key, (B, T, H, d) in INSTANTIATIONS.items():
        assert causal_key(T, d) == key, (key, T, d)
    reach = {causal_key(T, d) for T in range(1, 129) for d in range(8, 97, 8)}
    assert reach == set(INSTANTIATIONS)
    for T, d in ((77, 104), (77, 160), (129, 64), (0, 64), (77, 60), (77, 0)):
        assert causal_key(T, d) is None, (T, d)


def test_planner_mirror_matches_plan_causal():
    """causal_key / causal_chunks copy plan_causal: pin them to the C++ they copy.  Chunks of 64 or 128 rows put every wave's
    16-row blocks at multiples of 16 — what lets a block's diagonal be one whole key fragment."""
    src = _source()
    plan = src[src.index("bool plan_causal("):src.index("template <int KS, int DF, int NKF> constexpr int causal_fwd_lds")]
    for line in ("T > 128 || H < 1 || d < 8 || (d % 8) != 0 || d > 96) return false;", "pl->ks = d <= 64 ? 2 : 3;",
                 "pl->df = (d + 15) / 16;", "if (pl->df < 3) pl->df = 3;", "pl->nkf = T <= 96 ? 6 : 8;",
                 "pl->rq = (T > 64 && 2 * bh <= (backward ? 256 : 512)) ? 64 : 128;", "return (pl->rq % 64) == 0;"):
        assert line in plan, line
    assert causal_chunks(4, 77, 12, False) == (2, 64) and causal_chunks(4, 77, 12, True) == (2, 64)
    assert causal_chunks(2, 64, 2, False) == (1, 128) and causal_chunks(16, 128, 16, True) == (1, 128)
    assert causal_chunks(16, 128, 16, False) == (2, 64)


def _tiny_clip(dtype=torch.float32, impl=None):
    from transformers import CLIPTextConfig, CLIPTextModel

    torch.manual_seed(0)
    cfg = CLIPTextConfig(vocab_size=99, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                         num_attention_heads=2, max_position_embeddings=77, bos_token_id=1, eos_token_id=2, pad_token_id=0)
    if impl is not None:
        cfg._attn_implementation = impl
    return CLIPTextModel(cfg).to(dtype).eval()


def test_switch_recognises_clip_attention_and_hands_cpu_calls_back():
    from diffusion_finetuning_amd.attention import set_use_hip_attention

    te = _tiny_clip()
    mods = [m for m in te.modules() if m.__class__.__name__ == "CLIPAttention"]
    assert len(mods) == 2
    ids = torch.randint(0, 99, (2, 77), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = te(ids)[0]
    assert set_use_hip_attention(te, True) == len(mods)
    assert all("forward" in m.__dict__ for m in mods)
    assert set_use_hip_attention(te, True) == 0  # idempotent
    with torch.no_grad():
        got = te(ids)[0]
        padded = te(ids, attention_mask=torch.ones_like(ids))[0]
    assert torch.equal(got, want)  # CPU tensors: every call is handed back to the module's own forward
    assert torch.equal(padded, want)
    assert set_use_hip_attention(te, False) == len(mods)
    assert all("forward" not in m.__dict__ for m in mods)
    assert set_use_hip_attention(te, False) == 0
    with torch.no_grad():
        assert torch.equal(te(ids)[0], want)


def test_switch_restores_a_forward_installed_before_it():
    from diffusion_finetuning_amd.attention import set_use_hip_attention

    te = _tiny_clip()
    m = next(m for m in te.modules() if m.__class__.__name__ == "CLIPAttention")
    mine = lambda *a, **k: type(m).forward(m, *a, **k)  # noqa: E731
    m.forward = mine
    assert set_use_hip_attention(te, True) == 2
    assert set_use_hip_attention(te, False) == 2
    assert m.__dict__["forward"] is mine


def test_front_raises_on_cpu_tensors_and_unsupported_shapes():
    from diffusion_finetuning_amd.sandwich import causal_attention, causal_attention_supported

    q = torch.zeros(1, 8, 64, dtype=torch.float16)
    assert not causal_attention_supported(q, 1)
    with pytest.raises(RuntimeError):
        causal_attention(q, q, q, 1)


def test_shared_row_stride_ignores_the_strides_of_size_one_dimensions():
    """PyTorch leaves the stride of a size-1 dimension arbitrary: a contiguous [1, T, W] or [B, 1, W] tensor must not be
    refused for it, and slices of one buffer still report the buffer's row stride."""
    from diffusion_finetuning_amd._native import shared_row_stride

    x = torch.zeros(2, 5, 24)
    assert shared_row_stride(x, x, x) == 24
    q, k, v = (x[..., i * 8:(i + 1) * 8] for i in range(3))
    assert shared_row_stride(q, k, v) == 24 and shared_row_stride(q, k, torch.zeros(2, 5, 8)) is None
    assert shared_row_stride(x.transpose(0, 1), x, x) is None and shared_row_stride(x[..., ::2], x, x) is None
    one_batch = torch.zeros(5, 8).as_strided((1, 5, 8), (999, 8, 1))
    assert one_batch.is_contiguous() and shared_row_stride(one_batch, one_batch, one_batch) == 8
    one_row = torch.zeros(2, 8).as_strided((2, 1, 8), (8, 999, 1))
    assert one_row.is_contiguous() and shared_row_stride(one_row, one_row, one_row) == 8
    single = torch.zeros(8).as_strided((1, 1, 8), (77, 999, 1))
    assert shared_row_stride(single, single, single) == 8
    qs = torch.zeros(2, 24)[:, :8].unsqueeze(1)  # [2, 1, 8] slices of a [2, 24] buffer
    assert shared_row_stride(qs, qs, qs) == 24


def test_a_handed_back_call_is_logged_once_with_its_reason(caplog):
    import logging

    from diffusion_finetuning_amd import attention

    te = _tiny_clip()
    attention._CLIP_LOGGED.clear()
    attention.set_use_hip_attention(te, True)
    ids = torch.randint(0, 99, (1, 77), generator=torch.Generator().manual_seed(1))
    with caplog.at_level(logging.DEBUG, logger=attention.__name__), torch.no_grad():
        te(ids)
        te(ids)
    notes = [r.getMessage() for r in caplog.records if "handed back" in r.getMessage()]
    assert len(notes) == 1 and "HIP device" in notes[0], notes


# ---- the reference and the sensitivity of the check -------------------------------------------------------------------------

B, T, H, D = 2, 77, 3, 64


@pytest.fixture(scope="module")
def reference():
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, T, H * D, generator=g).half().double() for _ in range(3))
    return q, k, v, causal_reference(q, k, v, H)


def test_reference_is_torch_causal_attention_in_float64(reference):
    q, k, v, o = reference
    qh, kh, vh = (t.view(B, T, H, D).transpose(1, 2) for t in (q, k, v))
    want = torch.nn.functional.scaled_dot_product_attention(qh, kh, vh, is_causal=True)
    assert (o - want.transpose(1, 2).reshape(B, T, H * D)).abs().max().item() < 1e-12
    assert torch.equal(o[:, 0], v[:, 0])  # row 0 sees one key


def test_close_rejects_a_row_that_attends_one_key_past_its_diagonal(close, reference):
    """Row 37 of batch 0, head 1 also sees key 38 (a diagonal mask off by one): rejected at the f16 and the bf16 bound; the
    correctly rounded result passes both."""
    q, k, v, o = reference
    t, sl = 37, slice(1 * D, 2 * D)
    bad = o.clone()
    qh, kh, vh = q[0, t, sl], k[0, : t + 2, sl], v[0, : t + 2, sl]
    bad[0, t, sl] = torch.softmax(kh @ qh * D ** -0.5, dim=0) @ vh
    for dt, tol in TOLS.items():
        close(o.to(dt), o, tol)
        with pytest.raises(AssertionError):
            close(bad.to(dt), o, tol)
