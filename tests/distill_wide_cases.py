"""Cases of the wide (rank 17–64) svd_distill tests, shared by the host and the GPU file: the smallest shapes at which each
block width can go wrong, planted differences with a known spectrum, and their float64 SVDs (computed once per rank and dtype,
on the rounded difference T(W1 − W0) the reference decomposes, cli_svd.py:59-71)."""
import functools

import torch

# rank → layers of ONE distill_lora call.  Every call mixes sizes, so workgroups past a layer's rows take the early exit.
#   (96, 80)   @17: first wide rank, min(N, K) just above W = 48
#   (160, 136) @32: N and K not multiples of the 64-row tile
#   (144, 200) @48, (128, 320) @64: widths 64 and 80
#   (64, 96)   @64: r = min(N, K), so W = 80 > min(N, K) and the surplus columns must carry λ = 0
#   (40, 520)  @24: a very flat layer, W = 48 > N
CASES = {
    17: [(96, 80), (160, 136), (40, 520)],
    24: [(40, 520), (96, 80), (144, 200)],
    32: [(160, 136), (144, 200), (40, 520)],
    48: [(144, 200), (128, 320), (64, 96)],
    64: [(128, 320), (64, 96), (160, 136)],
}


def planted(N, K, r, dtype, gen):
    """W0 and W1 = W0 + Q1·diag(σ)·Q2ᵀ with σ_i = 1 − i/(2r) for i < r — every gap among the leading r values is 1/(2r) —
    and a tail 0.05·0.9^j below them."""
    n = min(N, K)
    q1, _ = torch.linalg.qr(torch.randn(N, n, generator=gen, dtype=torch.float64))
    q2, _ = torch.linalg.qr(torch.randn(K, n, generator=gen, dtype=torch.float64))
    sig = torch.cat([1 - torch.arange(r, dtype=torch.float64) / (2 * r),
                     0.05 * 0.9 ** torch.arange(n - r, dtype=torch.float64)])
    w0 = (torch.randn(N, K, generator=gen) * 0.05).to(dtype)
    w1 = (w0.double() + (q1 * sig) @ q2.T).to(dtype)
    return w0, w1


def rounded_diff(w1, w0):
    return (w1.cpu() - w0.cpu()).double()  # the reference's subtraction in the weights' dtype (cli_svd.py:59-63)


@functools.lru_cache(maxsize=None)
def planted_pairs(r, dtype):
    gen = torch.Generator().manual_seed(1000 + r)
    return tuple(planted(n, k, r, dtype, gen) for n, k in CASES[r])


@functools.lru_cache(maxsize=None)
def reference_svds(r, dtype):
    """(U, S, Vh) in float64 of each layer's rounded difference; shared by the tests and never modified."""
    return tuple(torch.linalg.svd(rounded_diff(w1, w0), full_matrices=False) for w0, w1 in planted_pairs(r, dtype))


def sign_convention(up, down):
    """The project's sign convention: the largest-|.| entry of each down row positive, first index on ties."""
    idx = down.abs().argmax(dim=1)
    s = torch.where(down.gather(1, idx[:, None])[:, 0] < 0, -1.0, 1.0).to(down.dtype)
    return up * s, down * s[:, None]


def neighbour_gaps(S, r):
    """Distance of each of the leading r singular values to its nearest neighbour, relative to σ_1; past the last singular
    value of a layer with r = min(N, K) the neighbour is the zero of the null space."""
    S = torch.cat([S, S.new_zeros(1)])
    below = S[:r] - S[1:r + 1]
    above = torch.cat([S[:1], S[:r - 1] - S[1:r]])
    return torch.minimum(below, above) / S[0]
