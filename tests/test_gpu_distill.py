"""`lora_distill` (lora_diffusion/cli_svd.py:29-111) on the HIP kernels of csrc/distill.hip: the quantile clamp against CPU
torch bit for bit, the factors against a float64 SVD of the same rounded difference (sign convention and clamp applied to the
expectation), the Eckart–Young bound on degenerate spectra, the reference's shipped artefact recovered, the whole
svd_distill at SD1.5 / CLIP-L size, determinism and one launch count whatever the layer count."""
import copy
import os

import pytest
import torch
import torch.nn as nn

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd.distill import distill_lora, svd_distill

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARTEFACT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example_loras",
                        "analog_svd_distill.text_encoder.pt")
# every distinct (N, K) of the SD1.5 UNet targets and the CLIP-L attention projections
SD15_CLIP_SHAPES = [(320, 320), (320, 768), (640, 640), (640, 768), (1280, 1280), (1280, 768), (2560, 320), (5120, 640),
                    (10240, 1280), (768, 768)]
TEST2_SHAPES = [(320, 320), (2560, 320), (640, 768), (1280, 1280), (10240, 1280)]


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


def _sign_and_clamp(up, down, q):
    """The project's sign convention (largest-|.| entry of each down row positive, first index on ties), then the
    reference's quantile clamp (cli_svd.py:79-84) — applied to a float64 expectation."""
    idx = down.abs().argmax(dim=1)
    s = torch.where(down.gather(1, idx[:, None])[:, 0] < 0, -1.0, 1.0).to(down.dtype)
    up, down = up * s, down * s[:, None]
    if q is not None:
        hi = torch.quantile(torch.cat([up.flatten(), down.flatten()]), q)
        up, down = up.clamp(-hi, hi), down.clamp(-hi, hi)
    return up, down


def _planted(N, K, dtype, gen):
    """W0 and W1 = W0 + Q1·diag(σ)·Q2ᵀ with σ_i = 30·0.8^i (i < 40): relative gaps of 20 % far above the rounding of W1."""
    n_sig = min(N, K, 40)
    q1, _ = torch.linalg.qr(torch.randn(N, n_sig, generator=gen, dtype=torch.float64))
    q2, _ = torch.linalg.qr(torch.randn(K, n_sig, generator=gen, dtype=torch.float64))
    sig = 30 * 0.8 ** torch.arange(n_sig, dtype=torch.float64)
    d = (q1 * sig) @ q2.T
    w0 = torch.randn(N, K, generator=gen) * 0.05
    w1 = (w0.double() + d).to(dtype)
    return w0.to(dtype), w1


def _rounded_diff(w1, w0):
    return (w1.cpu() - w0.cpu()).double()  # the reference's subtraction in the weights' dtype (cli_svd.py:59-63)


@pytest.mark.parametrize("q", [0.5, 0.9, 0.99, 1.0])
def test_quantile_clamp_is_bit_identical_to_cpu_torch(q):
    g = torch.Generator().manual_seed(1)
    sizes = sorted({r * (n + k) for n, k in SD15_CLIP_SHAPES for r in (1, 4, 16)}) + [1, 2, 3, 7]
    for i, n in enumerate(sizes):
        x = torch.randn(n, generator=g) * 0.1
        if i % 3 == 1:
            x = (x * 64).round() / 64  # many ties
        if i % 7 == 2:
            x = torch.full((n,), -0.25)  # all equal
        hi = torch.quantile(x, q)
        want = x.clamp(-hi, hi)
        xd = x.to(DEV)
        hid = torch.empty(1, device=DEV)
        nat.quantile_clamp_(xd, q, hid)
        assert torch.equal(hid.cpu()[0], hi), (n, q, hid.item(), hi.item())
        assert torch.equal(xd.cpu(), want), (n, q)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_factors_match_a_float64_svd_on_planted_spectra(dtype):
    gen = torch.Generator().manual_seed(7)
    pairs = [_planted(n, k, dtype, gen) for n, k in TEST2_SHAPES]
    base, tuned = _model([p[0] for p in pairs]), _model([p[1] for p in pairs])
    svds = []
    for w0, w1 in pairs:
        d = _rounded_diff(w1, w0)
        U, S, Vh = torch.linalg.svd(d, full_matrices=False)
        svds.append((U, S, Vh))
    for r in (1, 4, 16):
        for _, S, _ in svds:
            gaps = (S[:r] - S[1:r + 1]) / S[:r]
            assert gaps.min() >= 1e-2  # precondition of the comparison
        got, info = distill_lora(tuned, base, ["CrossAttention"], rank=r, clamp_quantile=0.99, return_info=True)
        assert not info["unconverged"], info
        for i, (U, S, Vh) in enumerate(svds):
            up, down = _sign_and_clamp(U[:, :r] * S[:r], Vh[:r], 0.99)
            up_g, down_g = got[2 * i].double().cpu(), got[2 * i + 1].double().cpu()
            torch.testing.assert_close(up_g, up, rtol=1e-3, atol=1e-3 * up.abs().max().item())
            torch.testing.assert_close(down_g, down, rtol=1e-3, atol=1e-3 * down.abs().max().item())
            sig = torch.tensor(info["sigma"][i], dtype=torch.float64)
            assert ((sig - S[:r]).abs() / S[:r]).max() <= 1e-4, (i, r, sig, S[:r])


def _degenerate_layers(gen):
    """Flat (Gaussian), exactly rank 2, repeated singular values, zero, and a tiny 20×24 layer (block width 20)."""
    out = []
    w0 = torch.randn(640, 768, generator=gen) * 0.05
    out.append((w0, w0 + torch.randn(640, 768, generator=gen) * 1e-2))
    w0 = torch.randn(1280, 320, generator=gen) * 0.05
    out.append((w0, w0 + torch.randn(1280, 2, generator=gen) @ torch.randn(2, 320, generator=gen) * 1e-2))
    q1, _ = torch.linalg.qr(torch.randn(320, 8, generator=gen))
    q2, _ = torch.linalg.qr(torch.randn(320, 8, generator=gen))
    w0 = torch.randn(320, 320, generator=gen) * 0.05
    out.append((w0, w0 + q1 @ q2.T * 0.5))
    w0 = torch.randn(768, 768, generator=gen) * 0.05
    out.append((w0, w0.clone()))
    w0 = torch.randn(20, 24, generator=gen) * 0.05
    out.append((w0, w0 + torch.randn(20, 24, generator=gen) * 1e-2))
    return out


def _eckart_young(d, up, down, r, slack=1e-4):
    S = torch.linalg.svdvals(d)
    bound = (1 + slack) * S[r:].square().sum().sqrt().item()
    err = (d - up.double().cpu() @ down.double().cpu()).norm().item()
    return err, bound


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_eckart_young_on_degenerate_spectra_and_the_merge_reproduces_it(dtype):
    gen = torch.Generator().manual_seed(11)
    pairs = [(a.to(dtype), b.to(dtype)) for a, b in _degenerate_layers(gen)]
    base, tuned = _model([p[0] for p in pairs]), _model([p[1] for p in pairs])
    for r in (1, 4, 16):
        with _no_check():
            got = distill_lora(tuned, base, ["CrossAttention"], rank=r, clamp_quantile=None)
        for i, (w0, w1) in enumerate(pairs):
            d = _rounded_diff(w1, w0)
            err, bound = _eckart_young(d, got[2 * i], got[2 * i + 1], r)
            # plus the fp32 arithmetic of the factors on an exactly low-rank D, whose tail is the rounding of W1 alone
            assert err <= bound + 2e-6 * d.norm().item(), (i, r, err, bound)
            if i == 3:
                assert not got[2 * i].any() and not got[2 * i + 1].any()  # zero layer → zero factors
        merged = copy.deepcopy(base)
        dfa.weight_apply_lora(merged, [t.clone() for t in got], ["CrossAttention"], alpha=1.0)
        eps = torch.finfo(dtype).eps
        for i, (lin_m, lin_t) in enumerate(zip(merged.lins, tuned.lins)):
            d = _rounded_diff(pairs[i][1], pairs[i][0])
            err = (d - got[2 * i].double().cpu() @ got[2 * i + 1].double().cpu()).norm().item()
            res = (lin_t.weight.double() - lin_m.weight.double()).norm().item()
            assert abs(res - err) <= eps * lin_t.weight.double().norm().item(), (i, r, res, err)


class _no_check:
    def __enter__(self):
        import warnings
        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter("ignore", RuntimeWarning)  # flat spectra need not converge; the bound is what counts

    def __exit__(self, *a):
        self._w.__exit__(*a)


def _clip_l(dtype):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.CLIPTextConfig(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12)
    with torch.device("meta"):
        te = transformers.CLIPTextModel(cfg)
    return te.to_empty(device=DEV).to(dtype)


def test_shipped_artefact_is_recovered_and_rank_is_checked():
    lst = torch.load(ARTEFACT, map_location="cpu", weights_only=True)
    base = _clip_l(torch.float32)
    gen = torch.Generator().manual_seed(3)
    lins = dfa.extract_linear_weights(base, dfa.TEXT_ENCODER_DEFAULT_TARGET_REPLACE)
    assert len(lins) == 48
    with torch.no_grad():
        for w in lins:
            w.copy_(torch.randn(w.shape, generator=gen) * 0.02)
    tuned = copy.deepcopy(base)
    with torch.no_grad():
        for i, w in enumerate(dfa.extract_linear_weights(tuned, dfa.TEXT_ENCODER_DEFAULT_TARGET_REPLACE)):
            w.add_((lst[2 * i] @ lst[2 * i + 1]).to(DEV))
    got = distill_lora(tuned, base, ["CLIPAttention"], rank=4, clamp_quantile=None)
    for i in range(48):
        want = (lst[2 * i] @ lst[2 * i + 1]).double()
        prod = (got[2 * i] @ got[2 * i + 1]).double().cpu()
        assert (prod - want).norm() / want.norm() <= 1e-4, i
    with pytest.raises(ValueError):
        small = _model([torch.zeros(8, 3)])
        distill_lora(small, _model([torch.ones(8, 3)]), ["CrossAttention"], rank=4)


def _exact_lowrank(w, gen, rank=8):
    """W0 and D = A·Bᵀ on a 2⁻⁷ grid: W0 + D is exact in fp16, D = T(W1 − W0) exactly, σ(D) from an 8×8 problem."""
    N, K = w.shape
    a = torch.randint(-1, 2, (N, rank), generator=gen).double()
    b = torch.randint(-3, 4, (K, rank), generator=gen).double()
    w0 = torch.randint(-64, 65, (N, K), generator=gen).double() / 128
    return w0, (a, b)


def _tail_from_factors(a, b, r):
    m = (a.T @ a) @ (b.T @ b)
    lam = torch.linalg.eigvals(m).real.clamp_min(0).sort(descending=True).values / 128 ** 2
    return lam[r:].sum().sqrt().item()


def test_svd_distill_full_size_unet_and_text_encoder(tmp_path):
    from harness.unet import UNet2DConditionModel, sd15_config

    class Pipe:
        pass

    gen = torch.Generator().manual_seed(21)
    pipes, truth = [Pipe(), Pipe()], {"unet": [], "te": []}
    with torch.device("meta"):
        u = UNet2DConditionModel(sd15_config())
    pipes[0].unet = u.to_empty(device=DEV).half()
    pipes[0].text_encoder = _clip_l(torch.float16)
    pipes[1].unet = copy.deepcopy(pipes[0].unet)
    pipes[1].text_encoder = copy.deepcopy(pipes[0].text_encoder)
    for key, targets in (("unet", dfa.DEFAULT_TARGET_REPLACE), ("te", dfa.TEXT_ENCODER_DEFAULT_TARGET_REPLACE)):
        attr = "unet" if key == "unet" else "text_encoder"
        ws0 = dfa.extract_linear_weights(getattr(pipes[0], attr), ["CrossAttention", "Attention", "GEGLU"] if key == "unet"
                                         else ["CLIPAttention"])
        ws1 = dfa.extract_linear_weights(getattr(pipes[1], attr), ["CrossAttention", "Attention", "GEGLU"] if key == "unet"
                                         else ["CLIPAttention"])
        with torch.no_grad():
            for w0, w1 in zip(ws0, ws1):
                base, (a, b) = _exact_lowrank(w0, gen)
                w0.copy_(base.to(w0.dtype))
                w1.copy_((base + (a @ b.T) / 128).to(w1.dtype))
                truth[key].append((a, b))
    assert len(truth["unet"]) == 144 and len(truth["te"]) == 48
    save = str(tmp_path / "distilled.pt")
    with _no_check():
        svd_distill(pipes[1], pipes[0], rank=4, clamp_quantile=None, device="cuda:0", save_path=save)
    for path, key, attr, targets in ((save, "unet", "unet", dfa.DEFAULT_TARGET_REPLACE),
                                     (str(tmp_path / "distilled.text_encoder.pt"), "te", "text_encoder",
                                      dfa.TEXT_ENCODER_DEFAULT_TARGET_REPLACE)):
        lst = torch.load(path, weights_only=True)
        assert all(t.device.type == "cpu" and t.dtype == torch.float32 for t in lst)
        assert len(lst) == 2 * len(truth[key])
        for i, (a, b) in enumerate(truth[key]):
            d = (a @ b.T) / 128
            err = (d - lst[2 * i].double() @ lst[2 * i + 1].double()).norm().item()
            assert err <= (1 + 1e-4) * _tail_from_factors(a, b, 4) + 1e-6 * d.norm().item(), (key, i)
        model = getattr(pipes[0], attr)
        want = [t.clone() for t in lst]
        dfa.monkeypatch_or_replace_lora(model, lst, targets, r=4)
        got = dfa.extract_lora_ups_down(model, targets)
        assert len(got) == len(truth[key])
        # installed in the model's dtype, as the reference's monkeypatch does
        assert all(torch.equal(u.weight.cpu(), want[2 * i].to(u.weight.dtype)) and
                   torch.equal(dn.weight.cpu(), want[2 * i + 1].to(dn.weight.dtype)) for i, (u, dn) in enumerate(got))


def test_runs_are_bit_identical_and_launches_do_not_grow_with_layers():
    gen = torch.Generator().manual_seed(5)
    pairs = [_planted(n, k, torch.float16, gen) for n, k in TEST2_SHAPES[:3]]
    base, tuned = _model([p[0] for p in pairs]), _model([p[1] for p in pairs])
    a = distill_lora(tuned, base, ["CrossAttention"], rank=4)
    b = distill_lora(tuned, base, ["CrossAttention"], rank=4)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    counts = []
    for n_layers in (9, 144):
        shapes = [(320, 320)] * n_layers
        ps = [(torch.randn(s, generator=gen).half(), torch.randn(s, generator=gen).half()) for s in shapes]
        m0, m1 = _model([p[0] for p in ps]), _model([p[1] for p in ps])
        with _no_check():
            _, info = distill_lora(m1, m0, ["CrossAttention"], rank=4, tol=0.0, max_iters=3, return_info=True)
        assert info["iters"] == [3] * n_layers
        counts.append(info["launches"])
    assert counts[0] == counts[1] == 1 + 4 * 3 + 1
