"""`lora_distill` (lora_diffusion/cli_svd.py:29-111) at ranks 17–64 on the wide HIP kernels of csrc/distill_wide.hip, against the
reference's own arithmetic restated as tests/test_gpu_distill.py restates it: torch.linalg.svd in float64 on the CPU, on the
rounded difference T(W1 − W0), then U_r·diag(S_r), Vh_r, the sign convention and torch.quantile / clamp.  Shapes:
tests/distill_wide_cases.py."""
import copy
import warnings

import pytest
import torch
import torch.nn as nn

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd.distill import distill_lora
from tests.distill_wide_cases import CASES, neighbour_gaps, planted_pairs, reference_svds, rounded_diff, sign_convention

pytestmark = pytest.mark.gpu
DEV = "cuda"
TARGETS = ["CrossAttention"]


class CrossAttention(nn.Module):
    """A target container (matched by class name, as _find_modules does) holding the given linears."""

    def __init__(self, shapes, dtype):
        super().__init__()
        self.lins = nn.ModuleList([nn.Linear(k, n, bias=False, dtype=dtype) for n, k in shapes])


def _model(weights):
    m = CrossAttention([tuple(w.shape) for w in weights], weights[0].dtype)
    with torch.no_grad():
        for lin, w in zip(m.lins, weights):
            lin.weight.copy_(w)
    return m.to(DEV)


def _models(pairs):
    return _model([p[0] for p in pairs]), _model([p[1] for p in pairs])


def _quiet():
    w = warnings.catch_warnings()
    w.__enter__()
    warnings.simplefilter("ignore", RuntimeWarning)  # flat spectra need not converge; the bound is what counts
    return w


def _eckart_young(d, up, down, r):
    """‖D − up·down‖_F against (1 + 1e-4)·tail + 2e-6·‖D‖_F (the bound of tests/test_gpu_distill.py: the same convergence
    criterion, plus the fp32 arithmetic of the factors)."""
    S = torch.linalg.svdvals(d)
    bound = (1 + 1e-4) * S[r:].square().sum().sqrt().item() + 2e-6 * d.norm().item()
    err = (d - up.double().cpu() @ down.double().cpu()).norm().item()
    return err, bound


def test_rank_32_is_no_longer_refused():
    base, tuned = _models(planted_pairs(32, torch.float16))
    got = distill_lora(tuned, base, TARGETS, rank=32)
    assert len(got) == 2 * len(CASES[32])
    for i, (n, k) in enumerate(CASES[32]):
        assert got[2 * i].shape == (n, 32) and got[2 * i + 1].shape == (32, k)
        assert got[2 * i].dtype == got[2 * i + 1].dtype == torch.float32 and got[2 * i].is_cuda


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("r", sorted(CASES))
def test_singular_values_and_optimality_on_planted_spectra(r, dtype):
    pairs, svds = planted_pairs(r, dtype), reference_svds(r, dtype)
    base, tuned = _models(pairs)
    got, info = distill_lora(tuned, base, TARGETS, rank=r, clamp_quantile=None, return_info=True)
    assert not info["unconverged"], info
    assert all(len(s) == r for s in info["sigma"])
    for i, ((w0, w1), (_, S, _)) in enumerate(zip(pairs, svds)):
        sig = torch.tensor(info["sigma"][i], dtype=torch.float64)
        rel = ((sig - S[:r]).abs() / S[:r]).max().item()
        err, bound = _eckart_young(rounded_diff(w1, w0), got[2 * i], got[2 * i + 1], r)
        print(f"r={r} {dtype} layer {i} {tuple(w0.shape)}: sigma rel {rel:.2e}, EY err {err:.6e} bound {bound:.6e}, "
              f"iters {info['iters'][i]}, res {info['residual'][i]:.2e}")
        assert rel <= 1e-4, (i, r, sig, S[:r])
        assert err <= bound, (i, r, err, bound)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("r", sorted(CASES))
def test_factors_match_the_float64_svd_within_the_davis_kahan_bound(r, dtype):
    """Vector i is fixed by the SVD up to an angle of about res/gap_i (Davis–Kahan), res the solver's final residual relative to
    σ_1 and gap_i the distance of σ_i to its neighbours relative to σ_1; it is compared within max(1e-3, 2·res/gap_i) of the
    factor's largest entry.  A bound above 1e-2 would compare nothing, and fails."""
    pairs, svds = planted_pairs(r, dtype), reference_svds(r, dtype)
    base, tuned = _models(pairs)
    got, info = distill_lora(tuned, base, TARGETS, rank=r, clamp_quantile=None, return_info=True)
    for i, (U, S, Vh) in enumerate(svds):
        gap = neighbour_gaps(S, r)
        tol = torch.clamp(2 * info["residual"][i] / gap, min=1e-3)
        assert tol.max() <= 1e-2, (i, r, info["residual"][i], gap.min())
        up, down = sign_convention(U[:, :r] * S[:r], Vh[:r])
        up_g, down_g = got[2 * i].double().cpu(), got[2 * i + 1].double().cpu()
        e_up = (up_g - up).abs().max(dim=0).values / up.abs().max()
        e_down = (down_g - down).abs().max(dim=1).values / down.abs().max()
        print(f"r={r} {dtype} layer {i}: worst up {(e_up / tol).max():.3f} down {(e_down / tol).max():.3f} of the tolerance "
              f"(tol max {tol.max():.2e})")
        assert (e_up <= tol).all() and (e_down <= tol).all(), (i, r, (e_up / tol).max(), (e_down / tol).max())


@pytest.mark.parametrize("r", sorted(CASES))
def test_down_rows_are_orthonormal(r):
    """‖down·downᵀ − I‖_max ≤ W·2⁻²²: the fp32 rounding of a W-term dot product of unit vectors, on the rows not dropped."""
    base, tuned = _models(planted_pairs(r, torch.float32))
    got, info = distill_lora(tuned, base, TARGETS, rank=r, clamp_quantile=None, return_info=True)
    W = nat.distill_width(r)
    for i in range(len(CASES[r])):
        keep = torch.tensor(info["sigma"][i]) > 0
        assert keep.all()  # the planted layers have min(N, K) >= r non-zero singular values
        down = got[2 * i + 1].double().cpu()[keep]
        dev = (down @ down.T - torch.eye(len(down), dtype=torch.float64)).abs().max().item()
        print(f"r={r} layer {i}: orthonormality {dev:.3e} (bound {W * 2.0 ** -22:.3e})")
        assert dev <= W * 2.0 ** -22, (i, r, dev)


def _degenerate_layers(r, gen):
    """After tests/test_gpu_distill.py: flat (Gaussian), exactly rank 20 (below r), 28 repeated singular values, zero, and a
    Gaussian layer with min(N, K) < W.  The rank-20 difference is A·Bᵀ/128 of small integers on a 2⁻⁷ grid, so W0 + D and
    T(W1 − W0) = D are exact in every dtype."""
    out = []
    w0 = torch.randn(160, 136, generator=gen) * 0.05
    out.append((w0, w0 + torch.randn(160, 136, generator=gen) * 1e-2))
    a = torch.randint(-1, 2, (144, 20), generator=gen).double()
    b = torch.randint(-3, 4, (200, 20), generator=gen).double()
    w0 = torch.randint(-64, 65, (144, 200), generator=gen).double() / 128
    out.append((w0.float(), (w0 + a @ b.T / 128).float()))
    q1, _ = torch.linalg.qr(torch.randn(128, 28, generator=gen))
    q2, _ = torch.linalg.qr(torch.randn(128, 28, generator=gen))
    w0 = torch.randn(128, 128, generator=gen) * 0.05
    out.append((w0, w0 + q1 @ q2.T * 0.5))
    w0 = torch.randn(96, 112, generator=gen) * 0.05
    out.append((w0, w0.clone()))
    n, k = (40, 520) if r == 24 else (64, 96)  # W = 48 resp. 80
    w0 = torch.randn(n, k, generator=gen) * 0.05
    out.append((w0, w0 + torch.randn(n, k, generator=gen) * 1e-2))
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("r", [24, 64])
def test_eckart_young_on_degenerate_spectra(r, dtype):
    gen = torch.Generator().manual_seed(11 + r)
    pairs = [(a.to(dtype), b.to(dtype)) for a, b in _degenerate_layers(r, gen)]
    assert min(min(a.shape) for a, _ in pairs) < nat.distill_width(r)
    base, tuned = _models(pairs)
    w = _quiet()
    try:
        got, info = distill_lora(tuned, base, TARGETS, rank=r, clamp_quantile=None, return_info=True)  # flag 3 would raise
    finally:
        w.__exit__(None, None, None)
    for i, (w0, w1) in enumerate(pairs):
        d = rounded_diff(w1, w0)
        assert torch.isfinite(got[2 * i]).all() and torch.isfinite(got[2 * i + 1]).all()
        err, bound = _eckart_young(d, got[2 * i], got[2 * i + 1], r)
        print(f"r={r} {dtype} layer {i}: EY err {err:.6e} bound {bound:.6e}, iters {info['iters'][i]}, "
              f"res {info['residual'][i]:.2e}")
        assert err <= bound, (i, r, err, bound)
    assert not got[6].any() and not got[7].any() and not any(info["sigma"][3])  # zero layer → zero factors
    # exactly rank 20 in every dtype: the directions above it hold only the fp32 rounding of the diff-GEMM, far below the
    # drop threshold 1e-6·σ_1, so the mask must deliver σ_j = 0 exactly, and zero `up` columns and `down` rows with it
    d = rounded_diff(pairs[1][1], pairs[1][0])
    assert torch.linalg.matrix_rank(d) == 20
    sig = torch.tensor(info["sigma"][1], dtype=torch.float64)
    print(f"r={r} {dtype} rank-20 layer: sigma above the rank {sig[20:].max():.3e}")
    assert (sig[20:] == 0).all(), sig[20:]
    assert not got[2][:, 20:].any() and not got[3][20:].any()
    assert ((sig[:20] - torch.linalg.svdvals(d)[:20]).abs() / sig[:20]).max() <= 1e-4


def test_clamp_parity_with_torch_quantile():
    base, tuned = _models(planted_pairs(32, torch.float16))
    plain = distill_lora(tuned, base, TARGETS, rank=32, clamp_quantile=None)
    for q in (0.5, 0.99, 1.0):
        got = distill_lora(tuned, base, TARGETS, rank=32, clamp_quantile=q)
        for i in range(len(CASES[32])):
            up, down = plain[2 * i].cpu(), plain[2 * i + 1].cpu()
            hi = torch.quantile(torch.cat([up.flatten(), down.flatten()]), q)  # cli_svd.py:79-84
            assert torch.equal(got[2 * i].cpu(), up.clamp(-hi, hi)), (q, i)
            assert torch.equal(got[2 * i + 1].cpu(), down.clamp(-hi, hi)), (q, i)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_merge_round_trip_at_rank_48(dtype):
    pairs = planted_pairs(48, dtype)
    base, tuned = _models(pairs)
    got = distill_lora(tuned, base, TARGETS, rank=48, clamp_quantile=None)
    merged = copy.deepcopy(base)
    dfa.weight_apply_lora(merged, [t.clone() for t in got], TARGETS, alpha=1.0)
    eps = torch.finfo(dtype).eps
    for i, (lin_m, lin_t) in enumerate(zip(merged.lins, tuned.lins)):
        d = rounded_diff(pairs[i][1], pairs[i][0])
        err = (d - got[2 * i].double().cpu() @ got[2 * i + 1].double().cpu()).norm().item()
        res = (lin_t.weight.double() - lin_m.weight.double()).norm().item()
        assert abs(res - err) <= eps * lin_t.weight.double().norm().item(), (i, res, err)


def test_runs_are_bit_identical_and_launches_do_not_grow_with_layers():
    pairs = planted_pairs(32, torch.float16)
    base, tuned = _models(pairs)
    a = distill_lora(tuned, base, TARGETS, rank=32)
    b = distill_lora(tuned, base, TARGETS, rank=32)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    counts = []
    for copies in (1, 2):
        m0, m1 = _models(pairs * copies)
        w = _quiet()
        try:
            _, info = distill_lora(m1, m0, TARGETS, rank=32, tol=0.0, max_iters=3, return_info=True)
        finally:
            w.__exit__(None, None, None)
        assert info["iters"] == [3] * (len(pairs) * copies)
        counts.append(info["launches"])
    assert counts[0] == counts[1] == 1 + 4 * 3 + 1


def test_non_finite_weights_and_the_iteration_cap_are_reported():
    pairs = [(a.clone(), b.clone()) for a, b in planted_pairs(32, torch.float32)]
    base, tuned = _models(pairs)
    with pytest.warns(RuntimeWarning, match="did not reach"):
        _, info = distill_lora(tuned, base, TARGETS, rank=32, tol=0.0, max_iters=2, return_info=True)
    assert info["unconverged"] == [0, 1, 2] and info["iters"] == [2, 2, 2]  # flag 2 on every layer, and the call returned
    pairs[1][1][3, 5] = float("nan")
    base, tuned = _models(pairs)
    with pytest.raises(ValueError, match=r"layer 1 \(ModuleList\.1\)"):
        distill_lora(tuned, base, TARGETS, rank=32)
