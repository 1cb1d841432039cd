"""Shapes, inputs and the float64 restatement for the max-norm constraint on LoRA updates: `lora_max_norm`
(csrc/max_norm.hip), `lora_weight_norms` / `clamp_lora_norms_` and `LoraTrainer(max_weight_norm=...)`.  Plain data and CPU
torch; tests/test_max_norm_host.py checks the restatement itself, tests/test_gpu_max_norm*.py run the kernel against it.

The restatement takes the norm from the explicit product scale·up@down in float64 — NOT from the two Gram matrices the
kernel uses — so a comparison also checks the identity ‖up·down‖_F² = Σ_ij (down·downᵀ)_ij·(upᵀ·up)_ij the kernel rests on.

Inputs are small integers from an integer hash times a power of two, so every product the kernel forms is exact in fp32 up
to the sums' roundings and the inputs are the same on every host.  Every shape comes in three regimes against ONE bound
(`BOUND`, a launch has one): "below" (norm in [BOUND/8, BOUND/4)), "above" (norm in (2·BOUND, 4·BOUND]) — the raw layer
moved there by a power of two on `up`, which keeps every entry exact — and "on": a rank-one update of small integers whose
norm is exactly BOUND as an fp32 integer."""
import functools
import math

import torch

U = 2.0 ** -24  # unit roundoff of fp32

# (r, K, N).  (1,5,3) directly followed by (4,7,9): lengths below one wave, a second layer that starts 8 elements in;
# (4,1280,10240): the longest sums of SD1.5; 16: the last packed rank; 17: r4 = 20, a padded tile; 64: the largest rank
SHAPES = ((1, 5, 3), (4, 7, 9), (4, 320, 320), (4, 1280, 10240), (16, 64, 64), (17, 40, 24), (64, 96, 80))
REGIMES = ("below", "above", "on")
BOUND = 36.0
SCALES = {"below": 0.75, "above": 1.5, "on": 2.0}


def hashed(n, seed):
    """n integers in [-7, 7] from a multiplicative hash of the index (int64 arithmetic: the same on every host)."""
    i = torch.arange(n, dtype=torch.int64)
    h = (i * 2654435761 + seed * 40503 + 12345) & 0xFFFFFFFF
    return ((h >> 7) % 15 - 7).to(torch.float32)


def product_norm(up, down, scale):
    """‖scale·up@down‖_F in float64 from the explicit product."""
    delta = float(scale) * (up.double() @ down.double())
    return math.sqrt(float((delta * delta).sum()))


@functools.lru_cache(maxsize=None)
def layer(r, K, N, regime):
    """(up [N,r], down [r,K]) fp32 and the layer's scale for one shape and regime."""
    seed = 1000 * r + 10 * K + N
    scale = SCALES[regime]
    down = hashed(r * K, seed).view(r, K) * 2.0 ** -3
    if regime == "on":
        # up = u·e0ᵀ, so up@down = u ⊗ down[0]: ‖·‖_F = ‖u‖·‖down[0]‖ = 3·6, times scale 2 = 36 = BOUND exactly.  The other
        # rows of down are hashed values that meet zero columns of up.
        up = torch.zeros(N, r)
        up[:3, 0] = torch.tensor([2.0, 1.0, 2.0])
        down[0] = 0.0
        down[0, :3] = torch.tensor([2.0, 4.0, 4.0])
        assert product_norm(up, down, scale) == BOUND
        return up, down, scale
    up = hashed(N * r, seed + 7).view(N, r) * 2.0 ** -4
    norm = product_norm(up, down, scale)
    assert norm > 0.0
    lo = BOUND / 8 if regime == "below" else 2 * BOUND  # move the norm into [lo, 2·lo) by a power of two
    up = up * 2.0 ** math.ceil(math.log2(lo / norm))
    norm = product_norm(up, down, scale)
    assert (BOUND / 8 <= norm < BOUND / 2) if regime == "below" else (2 * BOUND <= norm <= 4 * BOUND), (r, K, N, regime, norm)
    return up, down, scale


def reference(up, down, scale, max_norm):
    """(norm, factor, up·factor, down·factor) in float64 on the fp32 inputs: norm from the explicit product;
    factor = sqrt(max_norm/norm) above the bound, else 1."""
    norm = product_norm(up, down, scale)
    factor = math.sqrt(float(max_norm) / norm) if norm > float(max_norm) else 1.0
    return norm, factor, up.double() * factor, down.double() * factor


def gram_norm_squared(up, down, scale):
    """scale²·Σ_ij (down·downᵀ)_ij·(upᵀ·up)_ij in float64: the kernel's route."""
    u, d = up.double(), down.double()
    return float(scale) ** 2 * float(((d @ d.T) * (u.T @ u)).sum())


def abs_sum(up, down, scale):
    """S = scale²·Σ_ij (|down|·|down|ᵀ)_ij·(|up|ᵀ·|up|)_ij: what every rounding of the kernel's sums is relative to."""
    u, d = up.double().abs(), down.double().abs()
    return float(scale) ** 2 * float(((d @ d.T) * (u.T @ u)).sum())


def norm_squared_bound(up, down, scale):
    """|n²_gpu − n²_ref| ≤ (max(K,N) + r² + 4)·2⁻²⁴·S for ANY order of the fp32 sums: at most max(K,N) roundings per Gram entry
    (first order: each enters the product once per factor it belongs to, and the longer sum dominates), r² terms of the
    contraction, and a few roundings of the scalar tail (the fp32 scale, the square root, the fp32 result)."""
    r, K = down.shape
    N = up.shape[0]
    return (max(K, N) + r * r + 4) * U * abs_sum(up, down, scale)


def table_layers():
    """Every shape in every regime, regime-major: (1,5,3) is directly followed by (4,7,9) three times."""
    return [(r, K, N, regime) for regime in REGIMES for (r, K, N) in SHAPES]


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))
