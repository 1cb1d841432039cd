"""Which compiled causal attention kernels exist (csrc/attn_causal.hip), and one shape that reaches each of them.

No GPU and no library: tests/test_gpu_causal_attention.py runs every entry against float64 math;
tests/test_causal_attention_host.py checks on the CPU that the keys are exactly the `CAUSAL_CASE` uses of the dispatch
function and that `plan_causal` selects every one of them and nothing else — the companion of tests/attention_cases.py.

Keys name the kernels' template arguments (the element type aside — every entry runs in f16 and bf16, forward and backward):
  (KS, DF, NKF)    attn_causal_fwd_kernel and attn_causal_bwd_kernel (+ attn_ctx_reduce_kernel)
Values are (B, T, H, d) shapes.
"""
import torch

INSTANTIATIONS = {
    # DF = max(3, ⌈d/16⌉), KS = 2 up to d = 64 and 3 up to 96; NKF = 6 up to 96 tokens, 8 up to 128
    (2, 3, 6): (2, 77, 2, 40),
    (2, 4, 6): (2, 77, 2, 64),
    (3, 5, 6): (2, 77, 2, 72),
    (3, 6, 6): (2, 77, 2, 88),
    (2, 3, 8): (2, 110, 2, 24),
    (2, 4, 8): (2, 110, 2, 56),
    (3, 5, 8): (2, 110, 2, 80),
    (3, 6, 8): (2, 110, 2, 96),
}


def causal_key(T, d):
    """The instantiation plan_causal picks, or None where attn_causal_supported refuses."""
    if not (1 <= T <= 128 and 8 <= d <= 96 and d % 8 == 0):
        return None
    return (2 if d <= 64 else 3), max(3, (d + 15) // 16), (6 if T <= 96 else 8)


def causal_chunks(B, T, H, backward):
    """(chunks, rows per chunk) of plan_causal: two workgroups per (batch, head) while the chip has room for them."""
    rq = 64 if T > 64 and 2 * B * H <= (256 if backward else 512) else 128
    return (T + rq - 1) // rq, rq


def causal_reference(q, k, v, heads, scale=None):
    """softmax(mask(QKᵀ·scale))V per head in float64 on [B, T, H·d] tensors, mask = −inf for key j > query i (the math of
    transformers' CLIPAttention core under `is_causal=True`; scale defaults to 1/√d)."""
    B, T, HD = q.shape
    d = HD // heads
    scale = d ** -0.5 if scale is None else scale
    qh, kh, vh = (t.double().view(B, T, heads, d).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * scale
    above = torch.ones(T, T, dtype=torch.bool).triu(1)
    p = s.masked_fill(above, float("-inf")).softmax(dim=-1)
    return (p @ vh).transpose(1, 2).reshape(B, T, HD)
