"""Which compiled attention kernels exist, and one shape that reaches each of them under the shipped plan.

No GPU and no library: tests/test_gpu_attention_cores.py runs every entry against float64 math;
tests/test_attention_coverage_host.py checks on the CPU that the keys are exactly the dispatch-table instantiations of
csrc/attn_flash.hip and csrc/attn_ctx.hip, and that `plan_flash` / `plan_ctx` select every one of them, so a new
instantiation with no test shape, or one no plan selects, fails the CPU suite.

Keys name the kernel's template arguments (the element type aside — every entry runs in f16 and bf16):
  ("flash_fwd", KS, DF, RB, ONES)   attn_flash_fwd_kernel
  ("flash_bwd", KS, DF, RBQ, NKW)   attn_flash_dq_kernel<KS, DF, RBQ> + attn_flash_dkdv_kernel<KS, DF, NKW, …>
  ("ctx_fwd", KS, DF, NKF)          attn_ctx_fwd_kernel
  ("ctx_bwd", KS, DF, NKF)          attn_ctx_bwd_kernel (+ attn_ctx_reduce_kernel)
Values are (B, Tq, Tk, H, d) shapes.
"""

FLASH_FWD, FLASH_BWD, CTX_FWD, CTX_BWD = "flash_fwd", "flash_bwd", "ctx_fwd", "ctx_bwd"

INSTANTIATIONS = {
    # flash forward: ONES is the one width per bucket with d % 16 == 8 and d / 16 == DF - 1 (Σp read from column d)
    (FLASH_FWD, 2, 3, 4, False): (2, 200, 130, 2, 48),
    (FLASH_FWD, 2, 3, 4, True): (2, 200, 130, 2, 40),
    (FLASH_FWD, 2, 4, 4, False): (2, 300, 150, 2, 64),
    (FLASH_FWD, 2, 4, 4, True): (2, 300, 150, 2, 56),
    (FLASH_FWD, 3, 5, 2, False): (2, 150, 200, 2, 80),
    (FLASH_FWD, 3, 5, 2, True): (2, 150, 200, 2, 72),
    (FLASH_FWD, 3, 6, 2, False): (2, 150, 200, 2, 96),
    (FLASH_FWD, 3, 6, 2, True): (2, 150, 200, 2, 88),
    (FLASH_FWD, 4, 8, 2, False): (2, 140, 170, 2, 112),
    (FLASH_FWD, 4, 8, 2, True): (2, 140, 170, 2, 120),
    (FLASH_FWD, 5, 10, 1, False): (2, 100, 140, 2, 136),
    (FLASH_FWD, 5, 10, 1, True): (2, 100, 140, 2, 152),
    # flash backward (dQ and dK/dV)
    (FLASH_BWD, 2, 3, 2, 4): (2, 200, 300, 2, 32),
    (FLASH_BWD, 2, 4, 2, 2): (2, 140, 150, 2, 56),
    (FLASH_BWD, 3, 5, 2, 2): (2, 140, 150, 2, 72),
    (FLASH_BWD, 3, 6, 2, 2): (2, 140, 150, 2, 88),
    (FLASH_BWD, 4, 8, 1, 1): (2, 70, 90, 2, 104),
    (FLASH_BWD, 5, 10, 1, 1): (2, 70, 90, 2, 144),
    # cross-attention: DF = max(3, ⌈d/16⌉) up to d = 96 (the whole head in one workgroup both ways), NKF = 6 up to 96 keys,
    # 8 up to 128; heads of 104 … 160 (≤ 96 keys) run forward whole (DF 10) and backward in two slices of DF 5
    (CTX_FWD, 2, 3, 6): (2, 100, 77, 2, 24),
    (CTX_FWD, 2, 4, 6): (2, 100, 77, 2, 56),
    (CTX_FWD, 3, 5, 6): (2, 100, 77, 2, 72),
    (CTX_FWD, 3, 6, 6): (2, 100, 77, 2, 88),
    (CTX_FWD, 2, 3, 8): (2, 100, 110, 2, 40),
    (CTX_FWD, 2, 4, 8): (2, 100, 110, 2, 64),
    (CTX_FWD, 3, 5, 8): (2, 100, 110, 2, 80),
    (CTX_FWD, 3, 6, 8): (2, 100, 110, 2, 96),
    (CTX_FWD, 5, 10, 6): (2, 100, 77, 2, 120),
    (CTX_BWD, 2, 3, 6): (2, 90, 50, 2, 48),
    (CTX_BWD, 2, 4, 6): (2, 90, 50, 2, 64),
    (CTX_BWD, 3, 5, 6): (2, 90, 50, 2, 80),
    (CTX_BWD, 3, 6, 6): (2, 90, 50, 2, 96),
    (CTX_BWD, 2, 3, 8): (2, 90, 128, 2, 8),
    (CTX_BWD, 2, 4, 8): (2, 90, 128, 2, 56),
    (CTX_BWD, 3, 5, 8): (2, 90, 128, 2, 72),
    (CTX_BWD, 3, 6, 8): (2, 90, 128, 2, 88),
    (CTX_BWD, 5, 5, 6): (2, 90, 96, 2, 160),
}

def flash_keys(d):
    """(forward key, backward key) that plan_flash / launch_flash_fwd pick for head dim d (8 … 160, d % 8 == 0)."""
    if d <= 48:
        ks, df, rb, rbq, nkw = 2, 3, 4, 2, 4
    elif d <= 64:
        ks, df, rb, rbq, nkw = 2, 4, 4, 2, 2
    elif d <= 80:
        ks, df, rb, rbq, nkw = 3, 5, 2, 2, 2
    elif d <= 96:
        ks, df, rb, rbq, nkw = 3, 6, 2, 2, 2
    elif d <= 128:
        ks, df, rb, rbq, nkw = 4, 8, 2, 1, 1
    else:
        ks, df, rb, rbq, nkw = 5, 10, 1, 1, 1
    ones = d % 16 == 8 and d // 16 == df - 1
    return (FLASH_FWD, ks, df, rb, ones), (FLASH_BWD, ks, df, rbq, nkw)


def ctx_keys(Tk, d):
    """(forward key, backward key) that plan_ctx picks, or None where attn_ctx_supported refuses."""
    if not (1 <= Tk <= 128 and 8 <= d <= 160 and d % 8 == 0) or (d > 96 and Tk > 96):
        return None
    nkf = 6 if Tk <= 96 else 8
    if d <= 96:
        ks, df = (2 if d <= 64 else 3), max(3, (d + 15) // 16)
        return (CTX_FWD, ks, df, nkf), (CTX_BWD, ks, df, nkf)
    return (CTX_FWD, 5, 10, nkf), (CTX_BWD, 5, 5, nkf)


def key_of(key_kind, shape):
    """The instantiation a table shape reaches, by the mirrors above."""
    B, Tq, Tk, H, d = shape
    fwd, bwd = ctx_keys(Tk, d) if key_kind.startswith("ctx") else flash_keys(d)
    return fwd if key_kind.endswith("fwd") else bwd


def attention_reference(q, k, v, heads, scale=None):
    """softmax(QKᵀ·scale)V per head in float64 on [B, T, H·d] tensors (the math of diffusers CrossAttention's core; scale
    defaults to 1/√d)."""
    B, Tq, HD = q.shape
    d = HD // heads
    scale = d ** -0.5 if scale is None else scale
    qh, kh, vh = (t.double().view(B, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    p = (qh @ kh.transpose(-1, -2) * scale).softmax(dim=-1)
    return (p @ vh).transpose(1, 2).reshape(B, Tq, HD)
