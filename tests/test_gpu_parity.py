"""Parity tests proper (MI355X): every HIP entry point, called through the C-ABI, against the reference's golden
vectors and against the CPU oracle on seeded inputs.

Tolerances (north_star: outputs within 1e-3 relative of the fp32 CPU reference):
  f32 path  : 2e-5 relative L2 (exact-f32 MFMA, only the summation order differs)
  f16 path  : 1e-3 relative L2 on golden inputs that are exactly fp16-representable (output rounding 2^-11)
  bf16 path : 1e-2 (8-bit mantissa output rounding)
"""
import itertools
import json

import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import trainer as tr
from oracle import lora_oracle as orc
from tests.attention_cases import attention_reference as _attention_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float32: 2e-5, torch.float16: 1e-3, torch.bfloat16: 1e-2}


def _bf16_safe(t, dtype):
    # golden inputs are fp16-representable; for bf16 compare against the oracle on the re-rounded inputs
    return t.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_operator_against_reference_golden(golden_operator, relerr, close, dtype):
    t, meta = golden_operator
    for c in [k for k in meta if k.startswith("c")]:
        cfg = json.loads(meta[c])
        s = cfg["scale"]
        x = t[f"{c}.x"].to(DEV).to(dtype).reshape(-1, cfg["K"])
        w = t[f"{c}.w"].to(DEV).to(dtype)
        dy = t[f"{c}.dy"].to(DEV).to(dtype).reshape(-1, cfg["N"])
        b = t[f"{c}.b"].to(DEV).to(dtype) if cfg["bias"] else None
        down, up = t[f"{c}.down"].to(DEV), t[f"{c}.up"].to(DEV)
        if dtype == torch.bfloat16:  # inputs re-rounded to bf16: expected values from the oracle on those inputs
            xf, wf, dyf = x.float().cpu(), w.float().cpu(), dy.float().cpu()
            dn, upc = down.bfloat16().float().cpu(), up.bfloat16().float().cpu()
            y_ref = orc.lora_linear_forward(xf, wf, None if b is None else b.float().cpu(), dn, upc, s)
            dx_ref, gd_ref, gu_ref = orc.lora_linear_backward(xf, wf, dn, upc, s, dyf)
        else:
            y_ref, dx_ref = t[f"{c}.y"].reshape(-1, cfg["N"]), t[f"{c}.dx"].reshape(-1, cfg["K"])
            gd_ref, gu_ref = t[f"{c}.g_down"], t[f"{c}.g_up"]
        y, T = nat.lora_linear_fwd(x, w, b, down, up, s)
        wt = nat.lora_cast_matrix(w, dtype, True)
        dx, U = nat.lora_linear_bwd_input(dy, wt, down, up, s, True)
        ga, gb = torch.zeros_like(down), torch.zeros_like(up)
        nat.lora_linear_bwd_params(dy, x, T, U, ga, gb, s)
        tol = TOL[dtype]
        close(y, y_ref, tol, (c, "y"))
        close(dx, dx_ref, tol, (c, "dx"))
        close(ga, gd_ref, tol, (c, "g_down"))
        close(gb, gu_ref, tol, (c, "g_up"))
        # no-input-grad variant (attn2 to_k/to_v): same U, no dX
        dx_none, U2 = nat.lora_linear_bwd_input(dy, None, down, up, s, False)
        assert dx_none is None and relerr(U2, U) < 1e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_operator_against_reference_golden_matrix(golden_operator_matrix, relerr, close, dtype):
    """SURVEY §8(c)'s operator matrix, produced by the REFERENCE's module (oracle/make_golden.py::gen_operator_matrix): the 12
    SD1.5 layer kinds × r ∈ {1,4,8,16} × scale ∈ {1,0.7} — 96 cases through the C-ABI.  The fixture keeps two full rows of Y
    and dX and 16 seeded projections of each output (the wide outputs would be 24 MB); inputs are integer-hash operands, exact
    in fp16.  bf16 re-rounds the inputs, so its expected values come from the float64 oracle on the re-rounded inputs (which
    test_oracle_golden.py pins on the same fixture)."""
    from oracle import synthetic as syn
    from tests.test_oracle_golden import matrix_digest

    t, meta = golden_operator_matrix
    tol = TOL[dtype]
    for tag, K, N, bias, M, r, s, seed in syn.matrix_cases():
        x, w, b, dy, down, up = syn.matrix_inputs(K, N, bias, M, r, seed)
        xd, wd, dyd = x.to(DEV).to(dtype), w.to(DEV).to(dtype), dy.to(DEV).to(dtype)
        bd = None if b is None else b.to(DEV).to(dtype)
        y, T = nat.lora_linear_fwd(xd, wd, bd, down.to(DEV), up.to(DEV), s)
        dx, U = nat.lora_linear_bwd_input(dyd, nat.lora_cast_matrix(wd, dtype, True), down.to(DEV), up.to(DEV), s, True)
        ga, gb = torch.zeros(r, K, device=DEV), torch.zeros(N, r, device=DEV)
        nat.lora_linear_bwd_params(dyd, xd, T, U, ga, gb, s)
        got = matrix_digest(y, dx, ga, gb, K, N, seed)
        if dtype == torch.bfloat16:
            xf, wf, dyf = xd.double().cpu(), wd.double().cpu(), dyd.double().cpu()
            dn, upc = down.bfloat16().double(), up.bfloat16().double()
            y_ref = orc.lora_linear_forward(xf, wf, None if bd is None else bd.double().cpu(), dn, upc, s)
            want = matrix_digest(y_ref, *orc.lora_linear_backward(xf, wf, dn, upc, s, dyf), K, N, seed)
        else:
            want = {k: t[f"{tag}.{k}"].double() for k in got}
        for k in got:
            if k.endswith("rows"):
                close(got[k], want[k], tol, (tag, k))
            else:  # a projection sums K or N rounding errors with random signs: the relative error of the sum is no larger
                assert relerr(got[k], want[k]) < tol, (tag, k, relerr(got[k], want[k]))


SD_SHAPES = [  # (M, K, N, bias): the distinct LoRA GEMMs of SD1.5 at 512² / B=4, M reduced where huge
    (2048, 320, 320, True), (1024, 320, 2560, True), (308, 768, 320, False), (1024, 640, 640, False),
    (512, 640, 5120, True), (308, 768, 640, False), (1024, 1280, 1280, True), (256, 1280, 10240, True),
    (308, 768, 1280, False), (77, 768, 320, False), (144, 1024, 1280, False),
    # cfg-3: CLIP-L attention projections at B=4 (77·4 rows); cfg-5: SD2.1-768 (96² latents, 1024-wide context);
    # long contractions on small grids (the deep-ring path); ragged row counts
    (308, 768, 768, True), (9216, 320, 320, False), (2304, 640, 640, True), (2304, 1024, 640, False),
    (576, 1280, 1280, True), (256, 1280, 1280, False), (1024, 10240, 1280, False), (333, 320, 960, False),
    (2304, 1024, 1280, False), (77, 1024, 1280, False),
    # every tile class of the ring kernel: 64×128 two-stage (128..255-tile grids), 128×160 with a ragged last row tile and
    # six column tiles, 128×128 at >= 256 tiles
    (4096, 640, 640, True), (8200, 320, 960, False), (4096, 320, 1280, True),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("r", [1, 4, 8, 16])
def test_operator_against_oracle_sd_shapes(relerr, close, dtype, r):
    g = torch.Generator().manual_seed(100 + r)
    # r = 1 and r = 8 run every other shape — plus, always, the CLIP-L projection (308,768,768): cfg-3 trains it at r = 8
    shapes = SD_SHAPES if r in (4, 16) else sorted(set(SD_SHAPES[::2]) | {(308, 768, 768, True)}, key=SD_SHAPES.index)
    for (M, K, N, bias) in shapes:
        x = torch.randn(M, K, generator=g).to(dtype)
        w = ((torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5).to(dtype)
        b = (torch.randn(N, generator=g) * 0.1).to(dtype) if bias else None
        down = (torch.randn(r, K, generator=g) / r).to(dtype).float()
        up = (torch.randn(N, r, generator=g) * 0.05).to(dtype).float()
        dy = torch.randn(M, N, generator=g).to(dtype)
        s = 0.7
        y_ref = orc.lora_linear_forward(x.double(), w.double(), None if b is None else b.double(), down.double(), up.double(), s)
        dx_ref, gd_ref, gu_ref = orc.lora_linear_backward(x.double(), w.double(), down.double(), up.double(), s, dy.double())
        xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
        y, T = nat.lora_linear_fwd(xd, wd, None if b is None else b.to(DEV), down.to(DEV), up.to(DEV), s)
        dx, U = nat.lora_linear_bwd_input(dyd, wd.t().contiguous(), down.to(DEV), up.to(DEV), s, True)
        ga, gb = torch.zeros(r, K, device=DEV), torch.zeros(N, r, device=DEV)
        nat.lora_linear_bwd_params(dyd, xd, T, U, ga, gb, s)
        tol = TOL[dtype]
        for name, got, ref in (("y", y, y_ref), ("dx", dx, dx_ref), ("ga", ga, gd_ref), ("gb", gb, gu_ref)):
            close(got, ref, tol, (M, K, N, r, name))


FULL_SIZE_SHAPES = [  # (M, K, N, bias) at the row counts the BASELINE configs REALLY run: config 2 (batch 4 at 64² latents) and
    # config 4 (4 instance + 4 class rows per GPU, train_lora_dreambooth.py:698-702: every M doubles)
    (16384, 320, 320, True), (32768, 320, 320, False),
    # GEGLU.proj: its forward also runs gated; its dX is the split-K kind (M×2560→320, M×5120→640, M×10240→1280)
    (16384, 320, 2560, True), (32768, 320, 2560, True),
    (4096, 640, 5120, True), (8192, 640, 5120, True),
    (1024, 1280, 10240, True), (2048, 1280, 10240, True),
    (8192, 640, 640, False), (2048, 1280, 1280, True),
]


@pytest.mark.parametrize("shape", FULL_SIZE_SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_operator_at_the_row_counts_the_configs_run(close, shape):
    """The strict per-operator check (relative L2 1e-3, every row 4e-3, every element 8e-3 of the rms) at FULL size, f16, rank 4,
    against the float64 oracle (lora.py:49-50 and its autograd): forward, the gated forward of `proj`, dX (split over K inside
    the launch for the long contractions), ∇A, ∇B.  The sweep above reduces M where it is huge; a tile map, a split plan or a
    row-block count that only goes wrong at 16 384 or 32 768 rows would pass there."""
    M, K, N, bias = shape
    r, s, dtype = 4, 0.7, torch.float16
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = ((torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5).to(dtype)
    b = (torch.randn(N, generator=g) * 0.1).to(dtype) if bias else None
    down = (torch.randn(r, K, generator=g) / r).to(dtype).float()
    up = (torch.randn(N, r, generator=g) * 0.05).to(dtype).float()
    dy = torch.randn(M, N, generator=g).to(dtype)
    y_ref = orc.lora_linear_forward(x.double(), w.double(), None if b is None else b.double(), down.double(), up.double(), s)
    dx_ref, gd_ref, gu_ref = orc.lora_linear_backward(x.double(), w.double(), down.double(), up.double(), s, dy.double())
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    bd = None if b is None else b.to(DEV)
    packs = nat.lora_pack_factors(down.to(DEV), up.to(DEV), dtype)
    y, T = nat.lora_linear_fwd(xd, wd, bd, down.to(DEV), up.to(DEV), s, packs)
    dx, U = nat.lora_linear_bwd_input(dyd, wd.t().contiguous(), down.to(DEV), up.to(DEV), s, True, packs)
    ga, gb = torch.zeros(r, K, device=DEV), torch.zeros(N, r, device=DEV)
    nat.lora_linear_bwd_params(dyd, xd, T, U, ga, gb, s)
    for name, got, ref in (("y", y, y_ref), ("dx", dx, dx_ref), ("ga", ga, gd_ref), ("gb", gb, gu_ref)):
        close(got, ref, TOL[dtype], (shape, name))
    if N >= 8 * K:  # the `proj` layers: the same forward with the gate in its epilogue (what a training step launches)
        res = nat.lora_linear_geglu_fwd(xd, wd, bd, r, s, packs, True)
        assert res is not None
        out, yg, Tg = res
        assert torch.equal(yg, y) and torch.equal(Tg, T)  # same contraction, same rounding: the strict check above covers it
        h, gt = yg.double().cpu().chunk(2, dim=-1)
        ref = h * torch.nn.functional.gelu(gt)
        err = (out.double().cpu() - ref).abs()
        # one rounding of the product (2^-11 relative) on top of the gate function's own error (≤ 1.5e-7 absolute on erf)
        assert bool((err <= 1.0e-3 * ref.abs() + 1e-5 * ref.pow(2).mean().sqrt()).all()), (shape, float(err.max()))
        out2, y2, _ = nat.lora_linear_geglu_fwd(xd, wd, bd, r, s, packs, False)
        assert y2 is None and torch.equal(out2, out)


def test_edge_cases_empty_and_single_row(relerr):
    K, N, r = 32, 48, 4
    w = torch.randn(N, K, device=DEV)
    a, b = torch.randn(r, K, device=DEV), torch.randn(N, r, device=DEV)
    y, T = nat.lora_linear_fwd(torch.empty(0, K, device=DEV), w, None, a, b, 1.0)
    assert y.shape == (0, N) and T.shape == (0, r)
    x1 = torch.randn(1, K, device=DEV)
    y1, _ = nat.lora_linear_fwd(x1, w, None, a, b, 1.0)
    assert relerr(y1, orc.lora_linear_forward(x1.cpu(), w.cpu(), None, a.cpu(), b.cpu(), 1.0)) < 2e-5
    with pytest.raises(ValueError):  # rank > min(K, N): same class of error as the reference (lora.py:36-39)
        nat.lora_linear_fwd(x1, w, None, torch.randn(40, K, device=DEV), torch.randn(N, 40, device=DEV), 1.0)
    # scale = 0 switches the LoRA branch off exactly
    y0, _ = nat.lora_linear_fwd(x1, w, None, a, b, 0.0)
    assert relerr(y0, x1.cpu() @ w.cpu().t()) < 2e-5


@pytest.mark.parametrize("mode", ["fp32", "autocast_fp16", "half_model"])
def test_module_autograd_matches_oracle_module(relerr, mode):
    """LoraInjectedLinear as the trainers use it: nn.Module forward + loss.backward(), incl. autocast."""
    torch.manual_seed(0)
    K, N, r = 64, 96, 4
    ref = orc.LoraInjectedLinear(K, N, True, r)
    with torch.no_grad():
        ref.lora_up.weight.normal_(0, 0.05)
        for p in ref.parameters():
            p.copy_(p.half().float())
    ref.scale = 0.7
    ref.linear.requires_grad_(False)
    mod = dfa.LoraInjectedLinear(K, N, True, r)
    mod.load_state_dict(ref.state_dict())
    mod.scale = 0.7
    mod.linear.requires_grad_(False)
    mod.to(DEV)
    x = torch.randn(2, 50, K).half().float()
    xr = x.clone().requires_grad_(True)
    xg = x.to(DEV).requires_grad_(True)
    dy = torch.randn(2, 50, N).half().float()
    ref(xr).backward(dy)
    if mode == "fp32":
        y = mod(xg)
        assert y.dtype == torch.float32
        y.backward(dy.to(DEV))
        tol = 2e-5
    elif mode == "autocast_fp16":
        with torch.autocast("cuda", dtype=torch.float16):
            y = mod(xg)
        assert y.dtype == torch.float16  # like F.linear under autocast
        y.backward(dy.to(DEV).half())
        tol = 1e-3
    else:
        mod.half()
        xg = x.to(DEV).half().requires_grad_(True)
        y = mod(xg)
        y.backward(dy.to(DEV).half())
        tol = 1e-3
    assert relerr(y.float(), ref(xr).detach()) < tol
    assert relerr(xg.grad.float(), xr.grad) < tol
    assert relerr(mod.lora_down.weight.grad.float(), ref.lora_down.weight.grad) < tol
    assert relerr(mod.lora_up.weight.grad.float(), ref.lora_up.weight.grad) < tol
    assert mod.linear.weight.grad is None and mod.lora_down.weight.grad.dtype == mod.lora_down.weight.dtype
    # grads accumulate across backward calls like any autograd leaf
    before = mod.lora_up.weight.grad.clone()
    (mod(xg.detach()).float() * dy.to(DEV)).sum().backward()
    assert relerr(mod.lora_up.weight.grad.float(), 2 * before.float()) < 2e-3


def test_weight_cache_invalidation(relerr):
    mod = dfa.LoraInjectedLinear(32, 32, False, 2).to(DEV)
    with torch.no_grad():
        mod.lora_up.weight.normal_()
    x = torch.randn(4, 32, device=DEV, requires_grad=True)
    with torch.autocast("cuda", dtype=torch.float16):
        y1 = mod(x)
        with torch.no_grad():
            mod.linear.weight.mul_(2.0)  # in-place edit bumps the version counter
        y2 = mod(x)
    base = x.detach() @ (mod.linear.weight.detach() / 2).t()
    assert relerr((y2 - y1).float(), base) < 2e-3


def test_losses_against_reference_golden(golden_losses, relerr):
    t, meta = golden_losses
    w = float(meta["prior_loss_weight"])
    for dtype, tol in ((torch.float32, 2e-6), (torch.float16, 1e-3)):
        for tag, kw in (("plain", {}), ("prior", dict(with_prior_preservation=True, prior_loss_weight=w)),
                        ("masked", dict(mask=t["masked.raw_mask"]))):
            pred = t[f"{tag}.pred"].to(DEV).to(dtype).requires_grad_(True)
            loss = dfa.ddpm_mse_loss(pred, t[f"{tag}.target"].to(DEV).to(dtype), **kw)
            assert loss.dtype == torch.float32 and loss.dim() == 0
            loss.backward()
            assert abs(loss.item() - t[f"{tag}.loss"].item()) < 2e-6 * max(1.0, abs(t[f"{tag}.loss"].item())) * (1 if dtype == torch.float32 else 50)
            assert relerr(pred.grad.float(), t[f"{tag}.dpred"]) < tol, (tag, dtype)
    m = nat.lora_mask_prepare(t["masked.raw_mask"].reshape(2, 1, 64, 64).to(DEV), 8, 8)
    assert relerr(m, t["masked.mask"]) < 1e-6
    # deterministic: two launches give bit-identical loss
    p = torch.randn(8, 4, 64, 64, device=DEV, dtype=torch.float16)
    q = torch.randn_like(p)
    l1, _ = nat.ddpm_mse_fwd_bwd(p, q, None, 8, 0, 1.0, 1.0)
    l2, _ = nat.ddpm_mse_fwd_bwd(p, q, None, 8, 0, 1.0, 1.0)
    assert torch.equal(l1, l2)
    assert abs(l1.item() - orc.mse_loss(p.cpu(), q.cpu()).item()) < 1e-5


def test_merge_against_reference_golden(golden_merge, relerr):
    t, _ = golden_merge

    class CrossAttention(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.to_q = torch.nn.Linear(48, 64, bias=False)
            self.to_out = torch.nn.ModuleList([torch.nn.Linear(64, 48)])

    for alpha in (0.5, 1.0, 1.2):
        for dt, tag in ((torch.float32, "f32"), (torch.float16, "f16")):
            m = CrossAttention()
            with torch.no_grad():
                m.to_q.weight.copy_(t["w_q"])
                m.to_out[0].weight.copy_(t["w_o"])
            m = m.to(dt).to(DEV)
            old = m.to_q.weight
            loras = [t["up0"].clone(), t["down0"].clone(), t["up1"].clone(), t["down1"].clone()]
            dfa.weight_apply_lora(m, loras, alpha=alpha)
            assert loras == [] and m.to_q.weight is not old and isinstance(m.to_q.weight, torch.nn.Parameter)
            assert m.to_q.weight.dtype == dt
            # fp32: fma-vs-mul/add ordering only; fp16: op-by-op rounding emulated → at most 1 ulp apart
            tol = 1e-6 if dt == torch.float32 else 1e-3
            assert relerr(m.to_q.weight.float(), t[f"merged_q.{tag}.a{alpha}"]) < tol
            assert relerr(m.to_out[0].weight.float(), t[f"merged_o.{tag}.a{alpha}"]) < tol


def test_merge_of_a_cpu_resident_model_like_lora_add_upl(golden_merge):
    """The reference's `lora_add` moves the pipeline to the CPU before merging (cli_lora_add.py:74-78, 92-96):
    `weight_apply_lora` must take host-resident weights (staged through the HIP device, merged by the same kernel) and
    hand back Parameters on the CPU, bit-identical to the device-resident merge; `loras` is consumed either way."""
    t, meta = golden_merge
    for dt in (torch.float32, torch.float16):
        results = []
        for where in ("cpu", DEV):
            m = torch.nn.Module()
            m.blk = type("CrossAttention", (torch.nn.Module,), {})()
            m.blk.to_q = torch.nn.Linear(t["w_q"].shape[1], t["w_q"].shape[0], bias=False)
            m.blk.to_out = torch.nn.ModuleList([torch.nn.Linear(t["w_o"].shape[1], t["w_o"].shape[0])])
            with torch.no_grad():
                m.blk.to_q.weight.copy_(t["w_q"])
                m.blk.to_out[0].weight.copy_(t["w_o"])
            m = m.to(dt).to(where)
            loras = [t["up0"].clone(), t["down0"].clone(), t["up1"].clone(), t["down1"].clone()]
            dfa.weight_apply_lora(m, loras, alpha=0.5)
            assert loras == []
            assert m.blk.to_q.weight.device.type == torch.device(where).type and m.blk.to_q.weight.dtype == dt
            results.append((m.blk.to_q.weight.detach().cpu(), m.blk.to_out[0].weight.detach().cpu()))
        assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


def test_lerp_lora_lists_is_lora_add_lpl():
    """`lerp_lora_lists` = the LoRA ⊕ LoRA interpolation of cli_lora_add.py:44-60, op-by-op in the tensors' dtype
    (fp16 lists as `save_lora_weight` writes them).  fp32: bit-identical to the reference's torch expression on the CPU.
    fp16: within one ulp OF THE LARGEST TERM against torch's own CPU half arithmetic, which is not the same on every host
    (one rounding of a product apart is more than an ulp of the SUM where the two terms cancel).  The kernel itself is
    float-product-then-round bit for bit on any host: tests/test_gpu_optim_edges.py::test_lerp_is_the_emulation_bit_for_bit."""
    g = torch.Generator().manual_seed(12)
    shapes = [(320, 4), (4, 320), (640, 4), (4, 768), (1280, 1), (1, 1280)]
    for dtype in (torch.float16, torch.float32):
        for alpha in (0.5, 0.3, 1.0):
            l1 = [(torch.randn(s, generator=g) * 0.1).to(dtype) for s in shapes]
            l2 = [(torch.randn(s, generator=g) * 0.1).to(dtype) for s in shapes]
            want = [alpha * a + (1 - alpha) * b for a, b in zip(l1, l2)]  # the reference's expression, CPU torch
            big = [torch.maximum((alpha * a.float()).abs(), ((1 - alpha) * b.float()).abs()) for a, b in zip(l1, l2)]
            exact = [float(torch.tensor(alpha, dtype=torch.float32)) * a.double()
                     + float(torch.tensor(1 - alpha, dtype=torch.float32)) * b.double() for a, b in zip(l1, l2)]
            keep = list(l1)
            out = dfa.lerp_lora_lists(l1, l2, alpha)
            assert len(out) == len(shapes) and all(o is k for o, k in zip(out, keep))  # merged IN PLACE (x1.data = ...)
            for o, w, t, x in zip(out, want, big, exact):
                assert o.device.type == "cpu" and o.dtype == dtype
                if dtype == torch.float32:
                    assert torch.equal(o, w)
                else:
                    # one half-precision ulp of the largest of {term 1, term 2, sum}
                    ulp = torch.maximum(torch.maximum(w.float().abs(), t), torch.tensor(6.1e-5)) * 2.0 ** -10
                    # the arithmetic itself, host-independent: three roundings (two products, one sum) around the exact value
                    assert ((o.double() - x).abs() <= 1.5 * ulp.double()).all()
                    # and torch's CPU half arithmetic on this host (some round the scalar to half first): a few ulps
                    assert ((o.float() - w.float()).abs() <= 3 * ulp).all()
    assert dfa.lerp_lora_lists([], [], 0.5) == []
    with pytest.raises(RuntimeError, match="shape"):
        dfa.lerp_lora_lists([torch.zeros(4, 2), torch.zeros(2, 4)], [torch.zeros(4, 3), torch.zeros(3, 4)], 0.5)


def test_merge_equals_scaled_forward(relerr):
    """Ties a6 to a2: linear with W' = W + α·B·A equals the LoRA forward at scale α (merged UNet weights at α)."""
    torch.manual_seed(1)
    mod = dfa.LoraInjectedLinear(320, 320, True, 4).to(DEV)
    with torch.no_grad():
        mod.lora_up.weight.normal_(0, 0.05)
    mod.scale = 1.2
    x = torch.randn(512, 320, device=DEV)
    y_lora = mod(x)
    holder = torch.nn.Module()
    holder.blk = type("CrossAttention", (torch.nn.Module,), {})()
    holder.blk.to_q = torch.nn.Linear(320, 320).to(DEV)
    holder.blk.to_q.load_state_dict(mod.linear.state_dict())
    dfa.weight_apply_lora(holder, [mod.lora_up.weight.detach().clone(), mod.lora_down.weight.detach().clone()], alpha=1.2)
    y_merged = torch.nn.functional.linear(x, holder.blk.to_q.weight, holder.blk.to_q.bias)
    assert relerr(y_lora, y_merged.cpu()) < 2e-5


def test_clip_adamw_against_oracle(relerr):
    g = torch.Generator().manual_seed(3)
    n = 10007
    p0 = torch.randn(n, generator=g)
    for max_norm, gm in ((1.0, 1.0), (1e9, 0.5), (0.0, 1.0)):
        p_ref, m_ref, v_ref = p0.clone(), torch.zeros(n), torch.zeros(n)
        p = p0.to(DEV).clone()
        m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        norm = torch.zeros(4, device=DEV)
        for step in range(1, 4):
            grad = torch.randn(n, generator=g) * (3.0 if step == 1 else 0.01)
            gref = grad * gm
            total = gref.norm()
            if max_norm > 0:
                orc.clip_grad_norm([gref], max_norm)
            orc.adamw_step(p_ref, gref, m_ref, v_ref, step, 1e-3)
            gd = grad.to(DEV)
            nat.lora_grad_sqnorm(gd, gm, norm)
            nat.lora_adamw_step(p, gd, m, v, norm, gm, max_norm, 1e-3, 0.9, 0.999, 1e-8, 1e-2, step)
            assert abs(norm[0].sqrt().item() - total.item()) / total.item() < 1e-5 and norm[1].item() == 0.0
        assert relerr(p, p_ref) < 1e-6 and relerr(m, m_ref) < 1e-5 and relerr(v, v_ref) < 1e-4  # fp32 rounding order only
    # overflow → the whole step is skipped
    bad = torch.randn(n, device=DEV)
    bad[17] = float("inf")
    before = p.clone()
    nat.lora_grad_sqnorm(bad, 1.0, norm)
    nat.lora_adamw_step(p, bad, m, v, norm, 1.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 5)
    assert norm[1].item() == 1.0 and torch.equal(p, before)


def test_overflow_skip_follows_gradscaler_and_torch_adamw(relerr):
    """GradScaler semantics end to end on the device: an overflowed step leaves parameters, moments AND the step
    count alone (torch's scaler does not call optimizer.step()), so after [ok, inf, ok, nan, ok] the state equals
    torch.optim.AdamW stepped three times — bias corrections come from the device counter norm[2] (step = 0)."""
    g = torch.Generator().manual_seed(8)
    n, lr, scale = 4099, 1e-3, 1024.0
    p0 = torch.randn(n, generator=g)
    p_ref = torch.nn.Parameter(p0.clone())
    ref = torch.optim.AdamW([p_ref], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    p, m, v = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    norm = torch.zeros(4, device=DEV)
    for kind in ("ok", "inf", "ok", "nan", "ok"):
        grad = torch.randn(n, generator=g)
        scaled = (grad * scale).to(DEV)  # what backward leaves in the slab: loss-scaled gradients
        if kind != "ok":
            scaled[123] = float(kind)
        else:
            p_ref.grad = grad.clone()
            torch.nn.utils.clip_grad_norm_([p_ref], 1.0)
            ref.step()
        nat.lora_grad_sqnorm(scaled, 1.0 / scale, norm)
        nat.lora_adamw_step(p, scaled, m, v, norm, 1.0 / scale, 1.0, lr, 0.9, 0.999, 1e-8, 1e-2, 0)
        assert (norm[1].item() != 0.0) == (kind != "ok")
    assert norm[2].item() == 3.0 and norm[3].item() == 2.0
    assert int(ref.state[p_ref]["step"]) == 3
    assert relerr(p, p_ref.detach()) < 1e-6
    assert relerr(m, ref.state[p_ref]["exp_avg"]) < 1e-5 and relerr(v, ref.state[p_ref]["exp_avg_sq"]) < 1e-4


def test_trainer_backs_the_loss_scale_off_after_an_overflow(tiny_unet_factory):
    """fp16 trainer: a step whose gradients overflow is skipped, reported once, and the loss scale is halved for the
    following steps (picked up without a host sync, so at most two steps late)."""
    import warnings

    unet = tiny_unet_factory(seed=3).to(DEV).half()
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    _warm(list(itertools.chain(*params)), 11, 0.02)
    trainer = tr.LoraTrainer(unet, lr=1e-3, loss_scale=2.0 ** 30)  # absurd scale: the first steps must overflow
    before = tr.flat_lora_state(unet).clone()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for step in range(40):
            lat, noise, ts, ctx = orc.synthetic_batch(step, 2, 8, 6, 32)
            trainer.step(lat.to(DEV), noise.to(DEV), ts.to(DEV), ctx.to(DEV))
            torch.cuda.synchronize()
    assert trainer.opt.skipped_steps() >= 1 and trainer.opt.applied_steps() >= 1
    assert trainer.opt.skipped_steps() + trainer.opt.applied_steps() == 40 == trainer.opt.step_count
    assert trainer.loss_scale < 2.0 ** 30 and any("loss scale" in str(x.message) for x in w)
    assert not torch.equal(tr.flat_lora_state(unet), before) and torch.isfinite(tr.flat_lora_state(unet)).all()


def test_add_noise_against_oracle(relerr):
    g = torch.Generator().manual_seed(4)
    x0, eps = torch.randn(4, 4, 16, 16, generator=g), torch.randn(4, 4, 16, 16, generator=g)
    t = torch.tensor([0, 17, 500, 999])
    acp = orc.ddpm_alphas_cumprod()
    sa, sb = tr.ddpm_tables(device=DEV)
    for v in (False, True):
        noisy, target = nat.ddpm_add_noise(x0.to(DEV), eps.to(DEV), t.to(DEV), sa, sb, torch.float32, v)
        assert relerr(noisy, orc.add_noise(x0, eps, t, acp)) < 1e-6
        assert relerr(target, orc.get_velocity(x0, eps, t, acp) if v else eps) < 1e-6


def _warm(params, seed, std):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i, p in enumerate(params):
            if i % 2 == 0:
                p.copy_(torch.randn(p.shape, generator=g).to(p.device) * std)


@pytest.mark.parametrize("tag", ["plain", "prior"])
def test_trajectory_fused_trainer_vs_reference(golden_trajectory, tiny_unet_factory, relerr, tag):
    """Row H through the product's own step harness (slab + fused loss + fused clip/AdamW), fp32."""
    t, meta = golden_trajectory
    cfg = json.loads(meta[tag])
    unet = tiny_unet_factory(seed=cfg["unet_seed"]).to(DEV)
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    plist = list(itertools.chain(*params))
    _warm(plist, cfg["warm_seed"], cfg["warm_std"])
    assert relerr(tr.flat_lora_state(unet), t[f"{tag}.init"]) == 0.0
    trainer = tr.LoraTrainer(unet, lr=cfg["lr"])
    losses = []
    for step in range(cfg["steps"]):
        latents, noise, ts, ctx = orc.synthetic_batch(step, cfg["batch"], cfg["latent_hw"], cfg["ctx_len"], cfg["ctx_dim"])
        loss = trainer.step(latents.to(DEV), noise.to(DEV), ts.to(DEV), ctx.to(DEV), with_prior_preservation=cfg["with_prior"])
        losses.append(loss.item())
    assert relerr(torch.tensor(losses), t[f"{tag}.losses"]) < 1e-4
    assert relerr(tr.flat_lora_state(unet), t[f"{tag}.final"]) < 1e-3  # north_star: output LoRA within 1e-3


def test_trajectory_drop_in_with_torch_optimizer(golden_trajectory, tiny_unet_factory, relerr):
    """The same 10 steps written the way train_lora_dreambooth.py writes them: inject_trainable_lora →
    itertools.chain → torch.optim.AdamW → clip_grad_norm_ — only the operator and the loss are ours."""
    t, meta = golden_trajectory
    cfg = json.loads(meta["plain"])
    unet = tiny_unet_factory(seed=cfg["unet_seed"]).to(DEV)
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    plist = list(itertools.chain(*params))
    _warm(plist, cfg["warm_seed"], cfg["warm_std"])
    opt = torch.optim.AdamW(plist, lr=cfg["lr"], betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    acp = orc.ddpm_alphas_cumprod()
    for step in range(cfg["steps"]):
        latents, noise, ts, ctx = orc.synthetic_batch(step, cfg["batch"], cfg["latent_hw"], cfg["ctx_len"], cfg["ctx_dim"])
        noisy = orc.add_noise(latents, noise, ts, acp).to(DEV)
        pred = unet(noisy, ts.to(DEV), ctx.to(DEV)).sample
        loss = dfa.ddpm_mse_loss(pred, noise.to(DEV))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(unet.parameters(), 1.0)
        opt.step()
        opt.zero_grad()
    assert relerr(tr.flat_lora_state(unet), t["plain.final"]) < 1e-3


def test_fp16_training_tracks_fp32_reference(golden_trajectory, tiny_unet_factory, relerr):
    """cfg-2 numerics in miniature: fp16 storage/compute, fp32 master LoRA, static loss scale."""
    t, meta = golden_trajectory
    cfg = json.loads(meta["plain"])
    unet = tiny_unet_factory(seed=cfg["unet_seed"]).half().to(DEV)
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    plist = list(itertools.chain(*params))
    trainer = tr.LoraTrainer(unet, lr=cfg["lr"])
    assert trainer.slab.params.dtype == torch.float32 and plist[0].dtype == torch.float32  # masters are fp32
    _warm(plist, cfg["warm_seed"], cfg["warm_std"])
    for step in range(cfg["steps"]):
        latents, noise, ts, ctx = orc.synthetic_batch(step, cfg["batch"], cfg["latent_hw"], cfg["ctx_len"], cfg["ctx_dim"])
        trainer.step(latents.to(DEV), noise.to(DEV), ts.to(DEV), ctx.to(DEV))
    assert not trainer.opt.overflowed()
    # the LoRA *update* (final - init) agrees with the fp32 reference to a few percent in fp16
    upd = tr.flat_lora_state(unet).cpu() - t["plain.init"]
    upd_ref = t["plain.final"] - t["plain.init"]
    assert relerr(upd, upd_ref) < 0.1
    assert relerr(tr.flat_lora_state(unet), t["plain.final"]) < 5e-3


def test_saved_lora_roundtrip_after_training(tiny_unet_factory, tmp_path, relerr):
    unet = tiny_unet_factory().to(DEV)
    dfa.inject_trainable_lora(unet, r=4)
    trainer = tr.LoraTrainer(unet, lr=1e-3)
    latents, noise, ts, ctx = orc.synthetic_batch(0, 2, 8, 6, 32)
    trainer.step(latents.to(DEV), noise.to(DEV), ts.to(DEV), ctx.to(DEV))
    path = str(tmp_path / "out.safetensors")
    dfa.save_safeloras({"unet": (unet, dfa.DEFAULT_TARGET_REPLACE)}, path)
    weights, ranks, _ = dfa.load_safeloras(path)["unet"]
    assert relerr(torch.cat([w.detach().reshape(-1) for w in weights]), tr.flat_lora_state(unet)) == 0.0
    fresh = tiny_unet_factory().to(DEV)
    dfa.monkeypatch_or_replace_lora(fresh, weights, r=ranks)
    x = (torch.randn(2, 4, 8, 8, device=DEV), torch.tensor([5, 9], device=DEV), torch.randn(2, 6, 32, device=DEV))
    with torch.no_grad():
        assert relerr(fresh(*x).sample, unet(*x).sample) < 1e-5


def test_full_size_properties_cfg2():
    """BASELINE config-2 sizes (M=16384, 320→320 and 320→2560, fp16): size-independent properties."""
    torch.manual_seed(0)
    for (M, K, N) in ((16384, 320, 320), (16384, 320, 2560), (4096, 640, 640)):
        x = torch.randn(M, K, device=DEV, dtype=torch.float16)
        w = (torch.randn(N, K, device=DEV) / K ** 0.5).half()
        a = torch.randn(4, K, device=DEV) / 4
        b = torch.randn(N, 4, device=DEV) * 0.05
        y0, T = nat.lora_linear_fwd(x, w, None, a, b, 0.0)
        y1, _ = nat.lora_linear_fwd(x, w, None, a, b, 1.0)
        y2, _ = nat.lora_linear_fwd(x, w, None, a, b, 2.0)
        # (1) linear in the LoRA scale
        d1, d2 = (y1.float() - y0.float()), (y2.float() - y0.float())
        assert ((d2 - 2 * d1).norm() / d2.norm()).item() < 2e-2
        # (2) scale 0 is the plain base GEMM (hipBLASLt via torch as an independent implementation)
        ref = torch.nn.functional.linear(x, w)
        assert ((y0.float() - ref.float()).norm() / ref.float().norm()).item() < 1e-3
        # (3) T is X·Aᵀ; the row-permutation property: permuting rows of X permutes rows of Y and T
        perm = torch.randperm(M, device=DEV)
        yp, Tp = nat.lora_linear_fwd(x[perm].contiguous(), w, None, a, b, 1.0)
        assert torch.equal(yp, y1[perm]) and torch.equal(Tp, T[perm])
        # (4) gradient sums are additive over row blocks (what the DP all-reduce relies on)
        dy = torch.randn(M, N, device=DEV, dtype=torch.float16)
        U = torch.randn(M, 4, device=DEV)
        ga, gb = torch.zeros(4, K, device=DEV), torch.zeros(N, 4, device=DEV)
        nat.lora_linear_bwd_params(dy, x, T, U, ga, gb, 1.0)
        ga2, gb2 = torch.zeros(4, K, device=DEV), torch.zeros(N, 4, device=DEV)
        h = M // 2
        nat.lora_linear_bwd_params(dy[:h], x[:h], T[:h], U[:h], ga2, gb2, 1.0)
        nat.lora_linear_bwd_params(dy[h:], x[h:], T[h:], U[h:], ga2, gb2, 1.0)
        assert ((ga - ga2).norm() / ga.norm()).item() < 1e-5 and ((gb - gb2).norm() / gb.norm()).item() < 1e-5


def test_rccl_bucketed_exchange_single_rank(golden_trajectory, tiny_unet_factory, relerr):
    """The multi-GPU code path (broadcast, early [up|mid] bucket launched from the mid-block backward hook, RCCL
    all-reduce of slab ranges, partial-sum folding per range) on ONE GPU: a 1-rank NCCL(=RCCL) group must reproduce
    the reference trajectory exactly like the plain path does."""
    import os
    import torch.distributed as dist

    t, meta = golden_trajectory
    cfg = json.loads(meta["plain"])
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        unet = tiny_unet_factory(seed=cfg["unet_seed"]).to(DEV)
        params, _ = dfa.inject_trainable_lora(unet, r=4)
        _warm(list(itertools.chain(*params)), cfg["warm_seed"], cfg["warm_std"])
        trainer = tr.LoraTrainer(unet, lr=cfg["lr"], always_reduce=True, group_projections=False)
        assert trainer.exchange.active and trainer.exchange.early_range is not None
        a, b = trainer.exchange.early_range
        assert 0 < a < b == trainer.slab.numel  # [down | up | mid]: the early bucket is the tail
        for step in range(cfg["steps"]):
            latents, noise, ts, ctx = orc.synthetic_batch(step, cfg["batch"], cfg["latent_hw"], cfg["ctx_len"], cfg["ctx_dim"])
            trainer.step(latents.to(DEV), noise.to(DEV), ts.to(DEV), ctx.to(DEV))
        assert relerr(tr.flat_lora_state(unet), t["plain.final"]) < 1e-3
    finally:
        dist.destroy_process_group()


def test_hipgraph_step_matches_eager_step(golden_trajectory, tiny_unet_factory, relerr):
    """capture_graph=True records forward+backward once and replays it: same LoRA trajectory as launching every
    kernel from the host — for the explicit-noise step, for the on-device draw, and under a (1-rank) RCCL group whose
    watchdog thread is alive during the capture.  The explicit-noise run also lands on the reference trajectory."""
    import os
    import torch.distributed as dist

    t, meta = golden_trajectory
    cfg = json.loads(meta["plain"])

    def run(graph, seeded, reduce=False):
        unet = tiny_unet_factory(seed=cfg["unet_seed"]).to(DEV)
        params, _ = dfa.inject_trainable_lora(unet, r=4)
        _warm(list(itertools.chain(*params)), cfg["warm_seed"], cfg["warm_std"])
        trainer = tr.LoraTrainer(unet, lr=cfg["lr"], capture_graph=graph, always_reduce=reduce)
        losses = []
        for step in range(cfg["steps"]):
            lat, noise, ts, ctx = orc.synthetic_batch(step, cfg["batch"], cfg["latent_hw"], cfg["ctx_len"], cfg["ctx_dim"])
            if seeded:
                losses.append(trainer.step(lat.to(DEV), None, None, ctx.to(DEV), seed=77))
            else:
                losses.append(trainer.step(lat.to(DEV), noise.to(DEV), ts.to(DEV), ctx.to(DEV)))
        assert (trainer._graph is not None) == graph  # the capture really happened (no silent eager fallback)
        return tr.flat_lora_state(unet), torch.stack(losses)

    for seeded in (False, True):
        want, lw = run(False, seeded)
        got, lg = run(True, seeded)
        assert relerr(got, want) < 2e-5 and relerr(lg, lw) < 2e-5, (seeded, relerr(got, want), relerr(lg, lw))
        if not seeded:
            assert relerr(got, t["plain.final"]) < 1e-3
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29631")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        want, _ = run(False, False, reduce=True)
        got, _ = run(True, False, reduce=True)
        assert relerr(got, want) < 2e-5
    finally:
        dist.destroy_process_group()


def test_hipgraph_step_at_full_size_with_idle_gaps(relerr):
    """SD1.5-sized f16 model, device idle between steps (a host sync after each): the replayed loss and the LoRA state
    track the eagerly launched step.  Regression test for a captured hipMemsetAsync node that was not ordered before
    the kernel after it when the graph started on an idle queue (the loss came out as a partial sum); the reduction
    workspaces are now zeroed by a kernel."""
    from harness.unet import UNet2DConditionModel, sd15_config

    def run(graph):
        torch.manual_seed(0)
        with torch.device(DEV):
            unet = UNet2DConditionModel(sd15_config())
        unet = unet.half()
        unet.requires_grad_(False)
        dfa.inject_trainable_lora(unet, r=4)
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for up, _ in dfa.extract_lora_ups_down(unet):
                up.weight.copy_((torch.randn(up.weight.shape, generator=g) * 0.01).to(DEV))
        trainer = tr.LoraTrainer(unet, lr=1e-4, capture_graph=graph)
        losses = []
        for step in range(4):
            lat, noise, ts, ctx = orc.synthetic_batch(step, 2, 64, 77, 768)
            losses.append(trainer.step(lat.to(DEV), noise.to(DEV), ts.to(DEV), ctx.to(DEV)))
            torch.cuda.synchronize()
        assert (trainer._graph is not None) == graph
        return tr.flat_lora_state(unet), torch.stack(losses).cpu()

    want, lw = run(False)
    got, lg = run(True)
    assert (lw > 0.5).all() and relerr(lg, lw) < 1e-3, (lg, lw)
    assert relerr(got, want) < 1e-3


def test_pack_factors_and_partial_reduce_entry_points(relerr):
    """lora_pack_factors(_batched), lora_linear_bwd_params (row-block partials) and lora_reduce_partials."""
    g = torch.Generator().manual_seed(21)
    K, N, r, M = 96, 160, 5, 300
    a = torch.randn(r, K, generator=g).to(DEV)
    b = torch.randn(N, r, generator=g).to(DEV)
    for dt in (torch.float16, torch.float32):
        apack, bpack = nat.lora_pack_factors(a, b, dt)
        assert apack.shape == (32 * K,) and bpack.shape == (32 * N,) and apack.dtype == dt
        a16, at16 = apack[: 16 * K].view(16, K), apack[16 * K:].view(K, 16)
        bt16, b16 = bpack[: 16 * N].view(16, N), bpack[16 * N:].view(N, 16)
        assert torch.equal(a16[:r], a.to(dt)) and torch.equal(bt16[:r], b.t().to(dt))
        assert torch.equal(at16, a16.t()) and torch.equal(b16, bt16.t())
        assert float(a16[r:].abs().max()) == 0.0 and float(bt16[r:].abs().max()) == 0.0
    # batched form over a slab laid out [up(B) | down(A)] like the trainer's
    params = torch.cat([b.reshape(-1), a.reshape(-1)]).contiguous()
    table = torch.tensor([[N * r, 0, K, N, r, 0, 32 * K, 0]], dtype=torch.int64, device=DEV)
    packed = torch.empty(32 * (K + N), dtype=torch.float16, device=DEV)
    nat.lora_pack_factors_batched(table, 1, max(K, N), params, packed)
    ap, bp = nat.lora_pack_factors(a, b, torch.float16)
    assert torch.equal(packed[: 32 * K], ap) and torch.equal(packed[32 * K:], bp)
    # partial sums: any block count gives the same gradients after the ordered fold; folds are deterministic
    x = torch.randn(M, K, generator=g).to(DEV).half()
    dy = torch.randn(M, N, generator=g).to(DEV).half()
    t = torch.randn(M, r, generator=g).to(DEV)
    u = torch.randn(M, r, generator=g).to(DEV)
    ref_gb = (dy.double().t() @ t.double()).cpu()
    ref_ga = (u.double().t() @ x.double()).cpu()
    size = r * (K + N)
    stride = (size + 3) // 4 * 4
    outs = []
    for nb in (1, 3, 7, 64):
        ws = torch.full((nb, stride), float("nan"), device=DEV)  # every block must be fully written
        nat.lora_linear_bwd_params_partial(dy, x, t, u, ws[0], ws[0, r * K:], stride, nb, 1.0)
        out = torch.ones(stride, device=DEV)
        nat.lora_reduce_partials(ws, stride, nb, out, size, True)   # accumulate onto ones
        ga, gb = out[: r * K].view(r, K) - 1, out[r * K: size].view(N, r) - 1
        assert relerr(ga, ref_ga) < 1e-5 and relerr(gb, ref_gb) < 1e-5, nb
        out2 = torch.empty(stride, device=DEV)
        nat.lora_reduce_partials(ws, stride, nb, out2, size, False)
        out3 = torch.empty(stride, device=DEV)
        nat.lora_reduce_partials(ws, stride, nb, out3, size, False)
        assert torch.equal(out2[:size], out3[:size])
        outs.append(out2[:size].clone())
    # empty batch: partials are written as zeros
    ws = torch.full((2, stride), float("nan"), device=DEV)
    nat.lora_linear_bwd_params_partial(dy[:0], x[:0], t[:0], u[:0], ws[0], ws[0, r * K:], stride, 2, 1.0)
    assert float(ws[:, :size].abs().max()) == 0.0


def test_hot_path_kernels_are_deterministic():
    """No float atomics anywhere on the path: repeated launches on the same inputs are bit-identical (the stock PyTorch
    convolution/attention backward kernels around them are not, so this is asserted per kernel, not per step).  The
    shapes cover the unsplit ring kernel and the split-K launches (1280-wide projections at 1024 / 256 rows, the GEGLU
    `proj` backward): there the tile's LAST ARRIVER adds the K-slices — in index order whoever it is, so the result may
    not depend on the arrival order, which differs from launch to launch."""
    g = torch.Generator().manual_seed(8)
    for (M, K, N, r) in ((4096, 640, 640, 4), (1024, 1280, 1280, 4), (256, 1280, 1280, 16), (1024, 10240, 1280, 4),
                         (1000, 1280, 3840, 12)):
        x = torch.randn(M, K, generator=g).to(DEV).half()
        w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV).half()
        a, b = (torch.randn(r, K, generator=g) / r).to(DEV), (torch.randn(N, r, generator=g) * 0.05).to(DEV)
        dy = torch.randn(M, N, generator=g).to(DEV).half()
        wt = w.t().contiguous()
        runs = []
        for _ in range(4):
            y, t = nat.lora_linear_fwd(x, w, None, a, b, 1.0)
            dx, u = nat.lora_linear_bwd_input(dy, wt, a, b, 1.0, True)
            ga, gb = torch.zeros(r, K, device=DEV), torch.zeros(N, r, device=DEV)
            nat.lora_linear_bwd_params(dy, x, t, u, ga, gb, 1.0)
            p = torch.randn(M * 16, generator=torch.Generator().manual_seed(1)).to(DEV)
            norm = torch.zeros(4, device=DEV)
            nat.lora_grad_sqnorm(p, 1.0, norm)
            runs.append((y, t, dx, u, ga, gb, norm.clone()))
        for other in runs[1:]:
            for first, again in zip(runs[0], other):
                assert torch.equal(first, again), (M, K, N)


def test_split_k_inside_the_gemm_launch(close):
    """Contractions on grids too small for the chip are cut into K-slices INSIDE one launch (last-arriver reduction,
    csrc/lora_gemm.hip): against float64 on the shapes the plan splits, with bias, ragged row counts and every rank class;
    the workspace's ticket header must be zero again afterwards (the next launch relies on it), and the same call without
    a workspace (unsplit) must agree to rounding."""
    g = torch.Generator().manual_seed(21)
    split_seen = 0
    for (M, K, N, r, bias) in ((1024, 3840, 1280, 12, True), (256, 3840, 1280, 8, False), (1000, 5120, 1280, 16, True),
                               (1024, 10240, 1280, 4, False), (200, 5120, 640, 1, True), (77, 10240, 320, 4, False),
                               (1024, 1280, 1280, 4, True)):
        x = torch.randn(M, K, generator=g).half()
        w = ((torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5).half()
        bvec = (torch.randn(N, generator=g) * 0.1).half() if bias else None
        down = (torch.randn(r, K, generator=g) / r).half().float()
        up = (torch.randn(N, r, generator=g) * 0.05).half().float()
        s = 0.7
        y_ref = orc.lora_linear_forward(x.double(), w.double(), None if bvec is None else bvec.double(), down.double(),
                                        up.double(), s)
        t_ref = x.double() @ down.double().t()
        xd, wd = x.to(DEV), w.to(DEV)
        bd = None if bvec is None else bvec.to(DEV)
        nbytes = nat.lib().lora_gemm_workspace_bytes(M, K, N, nat.dtype_code(torch.float16))
        split_seen += int(nbytes > 0)
        y, T = nat.lora_linear_fwd(xd, wd, bd, down.to(DEV), up.to(DEV), s)
        close(y, y_ref, 2e-3, (M, K, N, r, "y"))
        close(T, t_ref, 1e-3, (M, K, N, r, "t"))
        if nbytes > 0:
            ws = next(iter(nat._splitk_ws.values()))
            header = ws.view(torch.int32)[: 1024]
            assert int(header.abs().max().item()) == 0, "ticket header not left at zero"
            # the unsplit launch of the same problem (no workspace handed over)
            packs = nat.lora_pack_factors(down.to(DEV), up.to(DEV), torch.float16)
            y0 = torch.empty_like(y)
            t0 = torch.empty_like(T)
            st = nat.lib().lora_linear_fwd(xd.data_ptr(), wd.data_ptr(), 0 if bd is None else bd.data_ptr(),
                                           down.to(DEV).data_ptr(), up.to(DEV).data_ptr(), packs[0].data_ptr(),
                                           packs[1].data_ptr(), y0.data_ptr(), t0.data_ptr(), M, K, N, r, s,
                                           nat.dtype_code(torch.float16), nat._stream(xd))
            assert st == 0
            close(y, y0, 1e-3, (M, K, N, r, "split vs unsplit"))
            close(T, t0, 1e-5, (M, K, N, r, "split vs unsplit T"))
    assert split_seen >= 5, "the plan no longer splits the shapes this test was written for"


def test_cfg3_text_encoder_lora_rank8(relerr):
    """BASELINE config 3: LoRA rank 8 on the CLIP text encoder (target class CLIPAttention, lora.py:54).  The
    transformers CLIP forward is the caller; only the four projections per layer run on the HIP path."""
    from transformers import CLIPTextConfig, CLIPTextModel

    cfg = CLIPTextConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                         vocab_size=100, max_position_embeddings=16, bos_token_id=1, eos_token_id=2, pad_token_id=0)
    torch.manual_seed(0)
    ref = CLIPTextModel(cfg)
    ref.requires_grad_(False)
    gpu = CLIPTextModel(cfg)
    gpu.load_state_dict(ref.state_dict())
    gpu.requires_grad_(False)
    gpu.to(DEV)
    ref_params, ref_names = orc.inject(ref, orc.TEXT_ENCODER_TARGETS, r=8)
    params, names = dfa.inject_trainable_lora(gpu, dfa.TEXT_ENCODER_DEFAULT_TARGET_REPLACE, r=8)
    plist = list(itertools.chain(*params))
    assert names == ref_names and len(plist) == len(ref_params) == 2 * 4 * 2
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p_ref, p in zip(ref_params, plist):
            p_ref.copy_(torch.randn(p_ref.shape, generator=g) * 0.05)
            p.copy_(p_ref.to(DEV))
    ids = torch.randint(3, 100, (3, 16), generator=g)
    wgt = torch.randn(3, 16, 64, generator=g)
    out_ref = ref(ids)[0]
    (out_ref * wgt).sum().backward()
    out = gpu(ids.to(DEV))[0]
    (out * wgt.to(DEV)).sum().backward()
    assert relerr(out, out_ref.detach()) < 1e-4
    for p_ref, p in zip(ref_params, plist):
        assert relerr(p.grad, p_ref.grad) < 1e-3


def test_cfg5_sd21_shape_rank16_v_prediction(relerr):
    """BASELINE config 5 in miniature: SD2.x-style UNet (linear proj_in/out), rank 16, v-prediction target."""
    from harness.unet import UNet2DConditionModel, UNetConfig

    cfg = UNetConfig(block_out_channels=(32, 64), down_attention=(True, False), layers_per_block=1, num_heads=(2, 2),
                     cross_attention_dim=48, norm_groups=8, linear_projection=True, name="tiny-sd21")

    def make():
        torch.manual_seed(9)
        m = UNet2DConditionModel(cfg)
        m.requires_grad_(False)
        return m

    ref = make()
    ref_params, _ = orc.inject(ref, r=16)
    unet = make().to(DEV)
    params, _ = dfa.inject_trainable_lora(unet, r=16)
    plist = list(itertools.chain(*params))
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for i, (p_ref, p) in enumerate(zip(ref_params, plist)):
            if i % 2 == 0:
                p_ref.copy_(torch.randn(p_ref.shape, generator=g) * 0.02)
            p.copy_(p_ref.to(DEV))
    ref_losses = orc.train_steps(ref, ref_params, 3, 2, 8, 5, 48, lr=1e-3, v_prediction=True)
    trainer = tr.LoraTrainer(unet, lr=1e-3, v_prediction=True)
    losses = []
    for step in range(3):
        latents, noise, ts, ctx = orc.synthetic_batch(step, 2, 8, 5, 48)
        losses.append(trainer.step(latents.to(DEV), noise.to(DEV), ts.to(DEV), ctx.to(DEV)).item())
    assert relerr(torch.tensor(losses), torch.tensor(ref_losses)) < 1e-4
    assert relerr(tr.flat_lora_state(unet), orc.flat_params(ref_params)) < 1e-3


def test_rank_above_16_uses_generic_kernels(relerr):
    """Ranks the fused tiles do not cover (r > 16) stay on the HIP device (shape-agnostic kernels)."""
    g = torch.Generator().manual_seed(5)
    M, K, N, r = 70, 48, 40, 20
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / 7
    a, b = torch.randn(r, K, generator=g) / r, torch.randn(N, r, generator=g) * 0.05
    dy = torch.randn(M, N, generator=g)
    y_ref = orc.lora_linear_forward(x, w, None, a, b, 0.9)
    dx_ref, ga_ref, gb_ref = orc.lora_linear_backward(x, w, a, b, 0.9, dy)
    y, t = nat.lora_linear_fwd(x.to(DEV), w.to(DEV), None, a.to(DEV), b.to(DEV), 0.9)
    dx, u = nat.lora_linear_bwd_input(dy.to(DEV), w.t().contiguous().to(DEV), a.to(DEV), b.to(DEV), 0.9, True)
    ga, gb = torch.zeros(r, K, device=DEV), torch.zeros(N, r, device=DEV)
    nat.lora_linear_bwd_params(dy.to(DEV), x.to(DEV), t, u, ga, gb, 0.9)
    for got, want in ((y, y_ref), (dx, dx_ref), (ga, ga_ref), (gb, gb_ref)):
        assert relerr(got, want) < 2e-5


def test_noise_prologue_matches_philox_oracle(relerr):
    """f-3: on-device draw (Philox4x32-10 + Box–Muller) + add_noise/target in one launch vs the numpy oracle."""
    import numpy as np

    from oracle import philox

    acp = orc.ddpm_alphas_cumprod()
    sa, sb = tr.ddpm_tables(device=DEV)
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn(5, 4, 16, 16, generator=g) * 0.18215
    for v in (False, True):
        noisy, target, t, eps = nat.ddpm_noise_prologue(x0.to(DEV), sa, sb, torch.float32, 77, 3, v, want_draw=True)
        eps_ref, t_ref = philox.step_randomness(5, 4 * 16 * 16, 1000, 77, 3)
        assert np.array_equal(t.cpu().numpy(), t_ref)  # integer stream: bit-exact
        eps_ref = torch.from_numpy(eps_ref).reshape(x0.shape)
        assert float((eps.cpu() - eps_ref).abs().max()) < 2e-5  # libm vs GPU logf/sincosf
        tt = torch.from_numpy(t_ref)
        assert relerr(noisy, orc.add_noise(x0, eps_ref, tt, acp)) < 1e-5
        assert relerr(target, orc.get_velocity(x0, eps_ref, tt, acp) if v else eps_ref) < 1e-5
    # same (seed, step) → same draw; the trainer's seeded step runs end to end
    a = nat.ddpm_noise_prologue(x0.to(DEV), sa, sb, torch.float16, 1, 2, False)
    b = nat.ddpm_noise_prologue(x0.to(DEV), sa, sb, torch.float16, 1, 2, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    from tests.conftest import build_tiny_unet

    unet = build_tiny_unet().to(DEV)
    dfa.inject_trainable_lora(unet, r=4)
    trainer = tr.LoraTrainer(unet, lr=1e-3)
    lat, _, _, ctx = orc.synthetic_batch(0, 2, 8, 6, 32)
    l0 = trainer.step(lat.to(DEV), None, None, ctx.to(DEV), seed=5)
    assert torch.isfinite(l0).all()


@pytest.mark.parametrize("mode", ["ehs", "ids", "ids-graph"])
def test_cfg3_unet_plus_text_encoder_training_step(relerr, tiny_unet_factory, mode):
    """BASELINE config 3 end to end (--train_text_encoder, train_lora_dreambooth.py:608-621,659-676): UNet LoRA r=4 and
    CLIP LoRA r=8 in ONE slab with two learning rates; attn2 to_k/to_v now need dX (the text encoder trains).
    `ehs`: the caller runs the text encoder and hands over its output; `ids`: the step runs it (train_lora_dreambooth.py:840);
    `ids-graph`: that step recorded into a hipGraph and replayed — the recording must really exist."""
    from transformers import CLIPTextConfig, CLIPTextModel

    ccfg = CLIPTextConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2,
                          vocab_size=50, max_position_embeddings=8, bos_token_id=1, eos_token_id=2, pad_token_id=0)

    def make():
        torch.manual_seed(4)
        te = CLIPTextModel(ccfg)
        te.requires_grad_(False)
        return tiny_unet_factory(seed=6), te

    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, 50, (2, 8), generator=g)
    lr_u, lr_t = 1e-3, 3e-4
    # reference loop on the CPU (oracle pieces, two param groups)
    ref_unet, ref_te = make()
    pu, _ = orc.inject(ref_unet, r=4)
    pt, _ = orc.inject(ref_te, orc.TEXT_ENCODER_TARGETS, r=8)
    unet, te = make()
    unet.to(DEV), te.to(DEV)
    gu, _ = dfa.inject_trainable_lora(unet, r=4)
    gt, _ = dfa.inject_trainable_lora(te, dfa.TEXT_ENCODER_DEFAULT_TARGET_REPLACE, r=8)
    plist = list(itertools.chain(*gu)) + list(itertools.chain(*gt))
    with torch.no_grad():
        for i, (p_ref, p) in enumerate(zip(pu + pt, plist)):
            if i % 2 == 0:
                p_ref.copy_(torch.randn(p_ref.shape, generator=g) * 0.02)
            p.copy_(p_ref.to(DEV))
    acp = orc.ddpm_alphas_cumprod()
    params = pu + pt
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    trainer = tr.LoraTrainer(unet, te, lr=lr_u, lr_text=lr_t, capture_graph=mode == "ids-graph")
    assert trainer.slab.model_ranges[1][0] == trainer.slab.model_ranges[0][1] > 0
    for step in range(3):
        latents, noise, ts, _ = orc.synthetic_batch(step, 2, 8, 6, 32)
        for p in params:
            p.grad = None
        ehs = ref_te(ids)[0]
        pred = ref_unet(orc.add_noise(latents, noise, ts, acp), ts, ehs).sample
        orc.mse_loss(pred, noise).backward()
        grads = [p.grad for p in params]
        orc.clip_grad_norm(grads, 1.0)
        with torch.no_grad():
            for i, (p, gr, mm, vv) in enumerate(zip(params, grads, m, v)):
                orc.adamw_step(p, gr, mm, vv, step + 1, lr_u if i < len(pu) else lr_t)
        if mode == "ehs":
            trainer.step(latents.to(DEV), noise.to(DEV), ts.to(DEV), te(ids.to(DEV))[0])
        else:
            trainer.step(latents.to(DEV), noise.to(DEV), ts.to(DEV), input_ids=ids.to(DEV))
    assert (trainer._graph is not None) == (mode == "ids-graph")
    n_u = sum(p.numel() for p in pu)
    got = trainer.slab.params[: trainer.slab.numel].cpu()
    want = orc.flat_params(params)
    assert relerr(got[:n_u], want[:n_u]) < 1e-3 and relerr(got[n_u:], want[n_u:]) < 1e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_sandwich_ops_geglu_and_head_layouts(relerr, dtype):
    """f-4 (first part): GEGLU gate and head split/merge kernels vs the stock PyTorch composites they replace."""
    from diffusion_finetuning_amd.sandwich import geglu_gate, merge_heads, split_heads

    g = torch.Generator().manual_seed(12)
    y = torch.randn(3, 50, 2 * 64, generator=g)
    dout = torch.randn(3, 50, 64, generator=g)
    yr = y.double().requires_grad_(True)
    h, gate = yr.chunk(2, dim=-1)
    (h * torch.nn.functional.gelu(gate)).backward(dout.double())
    yg = y.to(DEV).to(dtype).requires_grad_(True)
    out = geglu_gate(yg)
    out.backward(dout.to(DEV).to(dtype))
    tol = 1e-6 if dtype == torch.float32 else 2e-3
    hh, gg = y.to(dtype).double().chunk(2, dim=-1)
    assert relerr(out, hh * torch.nn.functional.gelu(gg)) < tol
    yq = y.to(dtype).double().requires_grad_(True)
    h2, g2 = yq.chunk(2, dim=-1)
    (h2 * torch.nn.functional.gelu(g2)).backward(dout.to(dtype).double())
    assert relerr(yg.grad, yq.grad) < tol
    # heads: split pads with zeros, merge drops the padding; each is the other's adjoint
    B, N, H, d, D = 2, 37, 8, 40, 64
    x = torch.randn(B, N, H * d, generator=g).to(dtype)
    xs = x.to(DEV).requires_grad_(True)
    s4 = split_heads(xs, H, D)
    ref4 = torch.nn.functional.pad(x.view(B, N, H, d).transpose(1, 2), (0, D - d))
    assert torch.equal(s4.cpu(), ref4)
    back = merge_heads(s4, d)
    assert torch.equal(back.cpu(), x)
    w = torch.randn(B, H, N, D, generator=g).to(dtype)
    s4.backward(w.to(DEV))
    assert torch.equal(xs.grad.cpu(), w[..., :d].transpose(1, 2).reshape(B, N, H * d))
    # the attention core returns [B,H,N,D] as a transposed VIEW of [B,N,H,D]: merged in place, no contiguous() copy
    t = torch.randn(B, N, H, D, generator=g).to(dtype)
    view = t.to(DEV).transpose(1, 2)
    assert not view.is_contiguous()
    assert torch.equal(merge_heads(view, d).cpu(), t[..., :d].reshape(B, N, H * d))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_ctx_attention_core_against_float64_reference(close, dtype):
    """f-4 (second part): the short-context attention kernels (forward, dQ/dK/dV) on cross-attention shapes — the SD
    ones (77 text tokens; heads of 40 and 80), ragged query counts, 1 … 128 keys, every head-dim bucket — against
    float64 math on the same 16-bit inputs.  Tolerance: one output rounding of the dtype plus the 16-bit P·V operand."""
    from diffusion_finetuning_amd.sandwich import ctx_attention, ctx_attention_supported

    tol = 2e-3 if dtype == torch.float16 else 1.2e-2
    g = torch.Generator().manual_seed(21)
    shapes = [(2, 64, 77, 2, 40), (1, 100, 77, 3, 40), (2, 256, 77, 8, 80), (1, 50, 5, 1, 8), (2, 130, 96, 2, 64),
              (1, 77, 128, 2, 96), (1, 16, 1, 1, 16), (1, 333, 100, 4, 48), (4, 1024, 77, 8, 80), (2, 4096, 77, 8, 40),
              (4, 256, 77, 8, 160), (2, 64, 77, 8, 160), (1, 70, 90, 2, 104)]
    for (B, Tq, Tk, H, d) in shapes:
        q = torch.randn(B, Tq, H * d, generator=g).to(dtype)
        k = torch.randn(B, Tk, H * d, generator=g).to(dtype)
        v = torch.randn(B, Tk, H * d, generator=g).to(dtype)
        go = torch.randn(B, Tq, H * d, generator=g).to(dtype)
        qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
        want = _attention_reference(qr, kr, vr, H)
        want.backward(go.double())
        qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
        assert ctx_attention_supported(qd, kd, H)
        got = ctx_attention(qd, kd, vd, H)
        got.backward(go.to(DEV))
        for name, a, b in (("o", got, want), ("dq", qd.grad, qr.grad), ("dk", kd.grad, kr.grad), ("dv", vd.grad, vr.grad)):
            close(a, b, tol, (name, (B, Tq, Tk, H, d)))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_flash_attention_core_against_float64_reference(close, dtype):
    """f-4 (third part): the long-context attention kernels (online softmax over 64-key tiles; forward, dQ, dK, dV) on the
    SD self-attention shapes (4096 tokens × heads of 40, 1024 × 80, 256 × 160), ragged query/key counts, cross shapes with
    more than 128 keys and every head-dim bucket — against float64 math on the same 16-bit inputs."""
    from diffusion_finetuning_amd.sandwich import flash_attention, flash_attention_supported

    tol = 2e-3 if dtype == torch.float16 else 1.2e-2
    g = torch.Generator().manual_seed(31)
    shapes = [(1, 64, 64, 1, 40), (2, 200, 130, 2, 40), (1, 256, 256, 2, 64), (2, 1024, 1024, 4, 80), (1, 256, 256, 8, 160),
              (1, 70, 300, 2, 96), (1, 100, 77, 2, 128), (1, 1, 1, 1, 8), (1, 333, 65, 3, 48), (1, 4096, 4096, 4, 40)]
    for (B, Tq, Tk, H, d) in shapes:
        q = torch.randn(B, Tq, H * d, generator=g).to(dtype)
        k = torch.randn(B, Tk, H * d, generator=g).to(dtype)
        v = torch.randn(B, Tk, H * d, generator=g).to(dtype)
        go = torch.randn(B, Tq, H * d, generator=g).to(dtype)
        qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
        want = _attention_reference(qr, kr, vr, H)
        want.backward(go.double())
        qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
        assert flash_attention_supported(qd, kd, H)
        got = flash_attention(qd, kd, vd, H)
        got.backward(go.to(DEV))
        for name, a, b in (("o", got, want), ("dq", qd.grad, qr.grad), ("dk", kd.grad, kr.grad), ("dv", vd.grad, vr.grad)):
            # (a gradient that is EXACTLY zero in float64 — one key: softmax ≡ 1, dS ≡ 0 — has no relative error; the kernels
            #  form dP − Δ inside the MFMA chain since round 4 and may leave the smallest f16 subnormal there: absolute bound)
            #  — ONLY then: any reference that is not identically zero keeps the relative check, however small it is)
            if float(b.abs().max()) == 0.0:
                assert float(a.double().cpu().abs().max()) < 1e-6, (name, (B, Tq, Tk, H, d), float(a.abs().max()))
            else:
                close(a, b, tol, (name, (B, Tq, Tk, H, d)))
    # inference form (no gradient requested): no log-sum-exp buffer, same output
    with torch.no_grad():
        assert torch.equal(flash_attention(qd, kd, vd, H), got)


def test_flash_attention_is_deterministic_and_bounded():
    from diffusion_finetuning_amd.sandwich import flash_attention, flash_attention_supported

    g = torch.Generator().manual_seed(32)
    q = torch.randn(2, 1024, 640, generator=g).half().to(DEV).requires_grad_(True)
    k = torch.randn(2, 1024, 640, generator=g).half().to(DEV).requires_grad_(True)
    v = torch.randn(2, 1024, 640, generator=g).half().to(DEV).requires_grad_(True)
    go = torch.randn(2, 1024, 640, generator=g).half().to(DEV)
    runs = []
    for _ in range(2):
        o = flash_attention(q, k, v, 8)
        runs.append((o.detach().clone(),) + tuple(t.clone() for t in torch.autograd.grad(o, (q, k, v), go)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)  # every output element has one owner: bit-identical from run to run
    assert not flash_attention_supported(q.float(), k.float(), 8)
    assert not flash_attention_supported(q, k, 2)  # head dim 320
    # large scores: the running maximum keeps exp2 in range (no inf/nan), rows still sum to one
    big = (torch.randn(1, 128, 64, generator=g) * 30).half().to(DEV)
    ones = torch.ones(1, 128, 64, dtype=torch.float16, device=DEV)
    out = flash_attention(big, big, ones, 1)
    assert torch.isfinite(out).all() and (out - 1).abs().max() < 2e-3


def test_ctx_attention_is_deterministic_and_rejects_what_it_does_not_cover():
    from diffusion_finetuning_amd.sandwich import ctx_attention, ctx_attention_supported

    g = torch.Generator().manual_seed(22)
    q = torch.randn(2, 4096, 320, generator=g).half().to(DEV).requires_grad_(True)
    k = torch.randn(2, 77, 320, generator=g).half().to(DEV).requires_grad_(True)
    v = torch.randn(2, 77, 320, generator=g).half().to(DEV).requires_grad_(True)
    go = torch.randn(2, 4096, 320, generator=g).half().to(DEV)
    runs = []
    for _ in range(2):
        o = ctx_attention(q, k, v, 8)
        runs.append((o.detach().clone(),) + tuple(t.clone() for t in torch.autograd.grad(o, (q, k, v), go)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)  # ordered partial sums: bit-identical dK/dV from run to run
    # outside the kernel's envelope the caller must keep its generic attention: fp32, long contexts, wide heads
    assert not ctx_attention_supported(q.float(), k.float(), 8)
    assert not ctx_attention_supported(q, torch.zeros(2, 129, 320, device=DEV, dtype=torch.float16), 8)
    assert not ctx_attention_supported(q, k, 1)  # head dim 320
    with pytest.raises(RuntimeError):
        nat.attn_ctx_fwd(q.detach().float(), k.detach().float(), v.detach().float(), 8, 0.1)


def test_attention_hook_routes_cross_attention_through_the_hip_core(relerr):
    """`set_use_memory_efficient_attention_xformers(model, True)` — the reference's own switch
    (lora_diffusion/xformers_utils.py:41-70) — sends both attentions of a transformer block through the HIP cores
    (self-attention: flash_attention, cross-attention: ctx_attention); output and LoRA gradients agree with the un-hooked
    block; `False` undoes it."""
    import harness.unet as hu
    from diffusion_finetuning_amd import attention, sandwich
    from lora_diffusion.xformers_utils import set_use_memory_efficient_attention_xformers as hook

    torch.manual_seed(5)
    blk = hu.BasicTransformerBlock(320, 8, 40, 768).to(DEV).half()
    blk.requires_grad_(False)
    params, _ = dfa.inject_trainable_lora(blk, r=4)
    plist = list(itertools.chain(*params))
    with torch.no_grad():
        for i, p in enumerate(plist):
            if i % 2 == 1:
                p.copy_(torch.randn_like(p) * 0.02)
    x = torch.randn(2, 256, 320, device=DEV).half()
    ctx = torch.randn(2, 77, 768, device=DEV).half()

    def run():
        for p in plist:
            p.grad = None
        out = blk(x, ctx)
        out.float().pow(2).sum().mul(1e-2).backward()
        return out, [p.grad.clone() for p in plist]

    ref, ref_grads = run()
    calls = []
    real, real_flash = attention.ctx_attention, attention.flash_attention
    attention.ctx_attention = lambda *a, **kw: (calls.append("ctx"), real(*a, **kw))[1]
    attention.flash_attention = lambda *a, **kw: (calls.append("flash"), real_flash(*a, **kw))[1]
    try:
        hook(blk, True)
        hook(blk, True)  # idempotent
        out, grads = run()
    finally:
        attention.ctx_attention, attention.flash_attention = real, real_flash
    assert calls == ["flash", "ctx"]  # attn1: 256 keys → tiled kernel; attn2: 77 text tokens → single-tile kernel
    assert relerr(out, ref) < 2e-3
    for a, b in zip(grads, ref_grads):
        assert relerr(a, b) < 2e-2
    hook(blk, False)
    assert all("forward" not in m.__dict__ for m in blk.modules())
    out2, _ = run()
    assert torch.equal(out2, ref)
    # the GEGLU switch: the feed-forward gate rides in the `proj` LoRA kernel's epilogue (one launch, tests/test_gpu_geglu.py)
    # and agrees with the stock chunk·gelu composite
    calls.clear()
    real_gate = nat.lora_linear_geglu_fwd
    nat.lora_linear_geglu_fwd = lambda *a, **kw: (calls.append(1), real_gate(*a, **kw))[1]
    try:
        assert attention.set_use_hip_geglu(blk, True) == 1
        out3, grads3 = run()
    finally:
        nat.lora_linear_geglu_fwd = real_gate
        attention.set_use_hip_geglu(blk, False)
    assert len(calls) == 1 and relerr(out3, ref) < 2e-3
    for a, b in zip(grads3, ref_grads):
        assert relerr(a, b) < 2e-2


def test_attention_hook_under_autocast_checkpointing_and_odd_inputs(relerr):
    """The hooked block the way the reference trainers drive it: fp32 module under fp16 autocast
    (train_lora_dreambooth.py:489-494 mixed_precision), activation checkpointing (:627-630), a non-contiguous query
    tensor, a keyword `encoder_hidden_states=` call, and a masked call that must go back to the module's own forward."""
    import harness.unet as hu
    from torch.utils.checkpoint import checkpoint

    from diffusion_finetuning_amd import attention

    torch.manual_seed(9)
    blk = hu.BasicTransformerBlock(320, 8, 40, 768).to(DEV)
    blk.requires_grad_(False)
    params, _ = dfa.inject_trainable_lora(blk, r=4)
    plist = list(itertools.chain(*params))
    with torch.no_grad():
        for i, p in enumerate(plist):
            if i % 2 == 1:
                p.copy_(torch.randn_like(p) * 0.02)
    xw = torch.randn(2, 200, 640, device=DEV)
    x = xw[..., ::2]  # non-contiguous [2,200,320]
    ctx = torch.randn(2, 77, 768, device=DEV)

    def run(use_ckpt):
        for p in plist:
            p.grad = None
        xin = x.clone().requires_grad_(True) if use_ckpt else x
        with torch.autocast("cuda", dtype=torch.float16):
            out = checkpoint(blk, xin, ctx, use_reentrant=False) if use_ckpt else blk(xin, ctx)
        out.float().pow(2).sum().mul(1e-2).backward()
        return out, [p.grad.clone() for p in plist]

    ref, ref_grads = run(False)
    calls = []
    real = attention.ctx_attention
    attention.ctx_attention = lambda *a, **kw: (calls.append(a[0].dtype), real(*a, **kw))[1]
    original_attn2 = blk.attn2.forward
    try:
        assert attention.set_use_hip_attention(blk, True) == 2
        out, grads = run(False)
        n_plain = len(calls)
        out_c, grads_c = run(True)
        # keyword form of the newer diffusers signature (the harness class itself only knows `context`)
        h16 = x.half().contiguous()
        c16 = ctx.half()
        blk16 = blk.attn2.half()
        kw = blk16(h16, encoder_hidden_states=c16)
        pos = blk16(h16, c16)
        assert torch.equal(kw, pos) and len(calls) == 5
        # a mask is outside the kernel's envelope: the call must reach the module's own forward, arguments intact
        seen = {}
        blk16.__dict__[attention._ORIG] = lambda hs, *a, **k: seen.update(args=a, kwargs=k) or hs
        assert blk16(h16, c16, attention_mask=torch.ones(2, 200, 77, device=DEV)) is h16
        assert len(seen["args"]) == 1 and "attention_mask" in seen["kwargs"] and len(calls) == 5
        blk.attn2.float()
    finally:
        attention.ctx_attention = real
        blk.attn2.__dict__[attention._ORIG] = original_attn2
        attention.set_use_hip_attention(blk, False)
    assert n_plain == 1 and calls[0] == torch.float16  # autocast dtype reached the kernel
    assert calls[:3] == [torch.float16] * 3  # checkpointing re-ran the forward once more in backward
    assert relerr(out, ref) < 3e-3 and relerr(out_c, ref) < 3e-3
    for a, b, c in zip(grads, grads_c, ref_grads):
        assert relerr(a, c) < 3e-2 and relerr(b, c) < 3e-2


def test_drop_in_under_ddp_autocast_and_checkpointing(golden_trajectory, tiny_unet_factory, relerr):
    """What `accelerate` does around the reference trainer (train_lora_dreambooth.py:489-494,627-630,744-757): the
    model wrapped in torch DistributedDataParallel (1-rank RCCL group), fp16 autocast with a GradScaler, and
    gradient checkpointing (the fused forward is re-entered from the autograd thread).  The LoRA gradients must reach
    the DDP reducer through ordinary autograd and the run must track the fp32 reference trajectory."""
    import os

    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    from torch.utils.checkpoint import checkpoint

    t, meta = golden_trajectory
    cfg = json.loads(meta["plain"])
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29534")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        unet = tiny_unet_factory(seed=cfg["unet_seed"]).to(DEV)
        params, _ = dfa.inject_trainable_lora(unet, r=4)
        plist = list(itertools.chain(*params))
        _warm(plist, cfg["warm_seed"], cfg["warm_std"])
        # gradient checkpointing on every transformer block, as diffusers' enable_gradient_checkpointing does
        for m in unet.modules():
            if type(m).__name__ == "BasicTransformerBlock":
                inner = m.forward
                m.forward = (lambda f: lambda x, ctx: checkpoint(f, x, ctx, use_reentrant=False))(inner)
        ddp = DDP(unet, device_ids=[0])
        opt = torch.optim.AdamW(plist, lr=cfg["lr"], betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
        acp = orc.ddpm_alphas_cumprod()
        for step in range(cfg["steps"]):
            latents, noise, ts, ctx = orc.synthetic_batch(step, cfg["batch"], cfg["latent_hw"], cfg["ctx_len"], cfg["ctx_dim"])
            noisy = orc.add_noise(latents, noise, ts, acp).to(DEV)
            with torch.autocast("cuda", dtype=torch.float16):
                pred = ddp(noisy, ts.to(DEV), ctx.to(DEV)).sample
            loss = dfa.ddpm_mse_loss(pred, noise.to(DEV))
            scaler.scale(loss).backward()
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(ddp.parameters(), 1.0)
            scaler.step(opt)
            scaler.update()
            opt.zero_grad()
        assert all(p.dtype == torch.float32 for p in plist)  # masters stay fp32 under autocast
        upd = tr.flat_lora_state(unet).cpu() - t["plain.init"]
        assert relerr(upd, t["plain.final"] - t["plain.init"]) < 0.1  # fp16 autocast vs the fp32 reference
        assert relerr(tr.flat_lora_state(unet), t["plain.final"]) < 5e-3
    finally:
        dist.destroy_process_group()


def test_cfg1_full_size_sd15_fp32_trajectory_vs_cpu_oracle(relerr):
    """BASELINE config 1 at full size: SD1.5-shaped UNet (859.5 M parameters), LoRA rank 4, batch 1, 256² (32×32
    latents), fp32 — the reference's own CPU-runnable case.  The GPU path (fused kernels, slab, fused clip+AdamW) must
    land within 1e-3 relative of the CPU oracle's LoRA state on identical seeds and inputs (north_star)."""
    import bench
    from harness.unet import UNet2DConditionModel, sd15_config

    steps = 10  # BASELINE.json configs[0]: "10 steps on CPU reference path" (also bench.py's cpu_baseline.cfg1 workload)
    n_threads = bench.usable_cpus()
    torch.set_num_threads(n_threads)

    def make(device):
        torch.manual_seed(0)
        with torch.device(device):
            m = UNet2DConditionModel(sd15_config())
        m.requires_grad_(False)
        return m

    ref = make("cpu")
    ref_params, _ = orc.inject(ref, r=4)
    g = torch.Generator().manual_seed(1)
    warm = [torch.randn(p.shape, generator=g) * 0.01 if i % 2 == 0 else None for i, p in enumerate(ref_params)]
    with torch.no_grad():
        for p, w in zip(ref_params, warm):
            if w is not None:
                p.copy_(w)
    init_state = orc.flat_params(ref_params).clone()
    ref_losses = orc.train_steps(ref, ref_params, steps, 1, 32, 77, 768, lr=1e-4)
    want = orc.flat_params(ref_params)
    state = {k: v for k, v in ref.state_dict().items() if "lora_" not in k}
    del ref

    unet = make("cpu")
    unet.load_state_dict({k.replace(".linear.", "."): v for k, v in state.items()})  # same frozen weights, bit for bit
    unet.to(DEV)
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    plist = list(itertools.chain(*params))
    with torch.no_grad():
        for i, (p, rp) in enumerate(zip(plist, torch.split(init_state, [q.numel() for q in plist]))):
            p.copy_(rp.view(p.shape).to(DEV))
    trainer = tr.LoraTrainer(unet, lr=1e-4)
    assert trainer.slab.numel == 1246464
    losses = []
    for step in range(steps):
        latents, noise, ts, ctx = orc.synthetic_batch(step, 1, 32, 77, 768)
        losses.append(trainer.step(latents.to(DEV), noise.to(DEV), ts.to(DEV), ctx.to(DEV)).item())
    got = tr.flat_lora_state(unet).cpu()
    assert relerr(torch.tensor(losses), torch.tensor(ref_losses)) < 1e-3
    assert relerr(got, want) < 1e-3
    assert relerr(got - init_state, want - init_state) < 2e-2  # the 4-step UPDATE itself, not just the state


def test_masked_step_recorded_into_a_hipgraph(tiny_unet_factory, relerr):
    """cli_lora_pti.py:222-247 masked loss inside the recorded step (the raw mask is a static input like the latents): the
    replayed trajectory is the host-launched one, and both follow the CPU oracle's masked loop."""
    def run(graph):
        unet = tiny_unet_factory(seed=5).to(DEV)
        params, _ = dfa.inject_trainable_lora(unet, r=4)
        _warm(list(itertools.chain(*params)), 11, 0.02)
        trainer = tr.LoraTrainer(unet, lr=1e-3, capture_graph=graph)
        losses = []
        for step in range(4):
            lat, noise, ts, ctx = orc.synthetic_batch(step, 2, 8, 6, 32)
            g = torch.Generator().manual_seed(50 + step)
            mask = (torch.rand(2, 1, 64, 64, generator=g) > 0.4).float()
            losses.append(trainer.step(lat.to(DEV), noise.to(DEV), ts.to(DEV), ctx.to(DEV), mask=mask))
        assert (trainer._graph is not None) == graph
        return tr.flat_lora_state(unet).cpu(), torch.stack(losses).reshape(-1).cpu()

    want, lw = run(False)
    got, lg = run(True)
    assert relerr(got, want) < 2e-5 and relerr(lg, lw) < 2e-5, (relerr(got, want), relerr(lg, lw))
    # the CPU oracle's masked loop
    ref = tiny_unet_factory(seed=5)
    ref_params, _ = orc.inject(ref, r=4)
    _warm(ref_params, 11, 0.02)
    acp = orc.ddpm_alphas_cumprod()
    m = [torch.zeros_like(p) for p in ref_params]
    v = [torch.zeros_like(p) for p in ref_params]
    ref_losses = []
    for step in range(4):
        lat, noise, ts, ctx = orc.synthetic_batch(step, 2, 8, 6, 32)
        g = torch.Generator().manual_seed(50 + step)
        mask = (torch.rand(2, 1, 64, 64, generator=g) > 0.4).float()
        for p in ref_params:
            p.grad = None
        pred = ref(orc.add_noise(lat, noise, ts, acp), ts, ctx).sample
        loss = orc.masked_mse_loss(pred, noise, mask)
        loss.backward()
        ref_losses.append(loss.item())
        grads = [p.grad for p in ref_params]
        orc.clip_grad_norm(grads, 1.0)
        with torch.no_grad():
            for p, gr, mm, vv in zip(ref_params, grads, m, v):
                orc.adamw_step(p, gr, mm, vv, step + 1, 1e-3)
    assert relerr(lg, torch.tensor(ref_losses)) < 1e-3 and relerr(got, orc.flat_params(ref_params)) < 1e-3


def test_drop_in_backward_defers_factor_gradients_into_one_batched_launch(tiny_unet_factory, relerr, monkeypatch):
    """An unchanged trainer's `loss.backward()` (no LoraSlab): the per-layer factor-gradient launches are deferred and go
    out as ONE lora_grad_batched call when the autograd engine finishes the pass (ops._AutoSink); `.grad` of every LoRA
    Parameter must equal what the per-layer launches produce (DFA_DEFER_GRADS=0), accumulate over two backward passes, and
    survive optimizer.zero_grad(set_to_none=True)."""
    unet = tiny_unet_factory(seed=2).to(DEV)
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    plist = list(itertools.chain(*params))
    _warm(plist, 5, 0.02)
    lat, noise, ts, ctx = orc.synthetic_batch(0, 2, 8, 6, 32)
    calls = []
    real = nat.lora_grad_batched_array
    monkeypatch.setattr(nat, "lora_grad_batched_array", lambda arr, n, dt, dev: (calls.append(n), real(arr, n, dt, dev))[1])

    def backward():
        pred = unet(lat.to(DEV), ts.to(DEV), ctx.to(DEV)).sample
        dfa.ddpm_mse_loss(pred, noise.to(DEV)).backward()

    packs = {"items": 0, "per_layer": 0}
    real_items, real_one = nat.lora_pack_items, nat.lora_pack_factors
    monkeypatch.setattr(nat, "lora_pack_items", lambda *a, **k: (packs.__setitem__("items", packs["items"] + 1), real_items(*a, **k))[1])
    monkeypatch.setattr(nat, "lora_pack_factors", lambda *a, **k: (packs.__setitem__("per_layer", packs["per_layer"] + 1), real_one(*a, **k))[1])
    backward()
    n_layers = len(plist) // 2
    assert calls == [2 * n_layers]  # every layer's two reductions in one call
    # ... and the packed compute-dtype factors of all layers come from ONE launch per parameter update (ops.PackRegistry):
    # none for a second pass over unchanged factors, one again after an optimizer-style in-place update
    assert packs == {"items": 1, "per_layer": 0}, packs
    deferred = [p.grad.clone() for p in plist]
    backward()  # accumulation into existing .grad
    assert packs == {"items": 1, "per_layer": 0}, packs
    for p, g in zip(plist, deferred):
        assert relerr(p.grad, 2 * g) < 1e-5
    with torch.no_grad():
        plist[0].mul_(1.0)  # an in-place update bumps the version: the next forward repacks (everything, once)
    for p in plist:
        p.grad = None
    backward()
    assert packs == {"items": 2, "per_layer": 0}, packs
    for p, g in zip(plist, deferred):
        assert relerr(p.grad, g) < 1e-5
    for p in plist:
        p.grad = None
    monkeypatch.setenv("DFA_DEFER_GRADS", "0")
    del calls[:]
    backward()
    assert calls == []  # per-layer launches
    for p, g in zip(plist, deferred):
        assert relerr(p.grad, g) < 1e-5, relerr(p.grad, g)


def test_drop_in_sink_plan_survives_a_layer_called_twice_and_a_frozen_factor(relerr, monkeypatch):
    """The drop-in sink keeps ONE plan per recurring backward pass (ops._SinkPlan: problem arrays, result layout grouped by
    Parameter shape, fold table) and only rewrites the operand pointers each step.  Cases a plan must not get wrong: the same
    layer applied twice in one pass (the same problem object twice: two slots, the second hand-over accumulates), layers of
    different shapes and row counts interleaved, a factor the caller froze (its .grad stays None), a second pass on new
    activations (the plan is re-used), and a pass of a different composition afterwards (a new plan)."""
    from diffusion_finetuning_amd import ops

    torch.manual_seed(3)
    a = dfa.LoraInjectedLinear(64, 128, bias=True, r=4).to(DEV)
    b = dfa.LoraInjectedLinear(128, 64, bias=False, r=8).to(DEV)
    for m in (a, b):
        m.linear.requires_grad_(False)
        with torch.no_grad():
            m.lora_up.weight.normal_(0, 0.05)
    b.lora_down.weight.requires_grad_(False)
    plist = [a.lora_down.weight, a.lora_up.weight, b.lora_down.weight, b.lora_up.weight]

    def backward(x1, x2, both=True):
        h = b(a(x1).half()) if both else a(x1)
        (h.float().square().mean() + a(x2).float().square().mean() * 0.5).backward()

    def grads():
        out = [None if p.grad is None else p.grad.clone() for p in plist]
        for p in plist:
            p.grad = None
        return out

    xs = [torch.randn(96, 64, device=DEV, dtype=torch.float16, requires_grad=True) for _ in range(2)]
    ys = [torch.randn(96, 64, device=DEV, dtype=torch.float16, requires_grad=True) for _ in range(2)]
    with torch.autocast("cuda", dtype=torch.float16):
        backward(xs[0], xs[1])
        sink = ops._auto_sinks[torch.device(DEV, torch.cuda.current_device())]
        n_plans = len(sink.plans)
        first = grads()
        backward(ys[0], ys[1])
        assert len(sink.plans) == n_plans  # same pass, new activations: the plan was re-used
        second = grads()
        backward(xs[0], xs[1], both=False)
        assert len(sink.plans) == n_plans + 1
        third = grads()
        monkeypatch.setenv("DFA_DEFER_GRADS", "0")
        backward(xs[0], xs[1])
        want_first = grads()
        backward(ys[0], ys[1])
        want_second = grads()
        backward(xs[0], xs[1], both=False)
        want_third = grads()
    for got, want in ((first, want_first), (second, want_second), (third, want_third)):
        assert got[2] is None and want[2] is None  # the frozen factor
        for g, w in zip(got, want):
            if w is None:
                assert g is None
            else:
                assert g.shape == w.shape and relerr(g, w) < 1e-5, relerr(g, w)
    assert third[3] is None  # (b took no part in the third pass)


def test_seeded_step_draws_timesteps_below_t_multiplier(tiny_unet_factory, monkeypatch):
    """cli_lora_pti.py:176,190-195: the PTI loop draws timesteps on [0, int(1000·t_mutliplier)).  The seeded step hands that
    bound to the prologue kernel — host-launched and recorded steps alike — and the draw respects it."""
    seen = []
    real = nat.ddpm_noise_prologue

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((a[7] if len(a) > 7 else kw.get("n_timesteps", 1000), int(out[2].max().item())))
        return out

    monkeypatch.setattr(nat, "ddpm_noise_prologue", spy)
    for graph in (False, True):
        unet = tiny_unet_factory(seed=1).to(DEV)
        dfa.inject_trainable_lora(unet, r=4)
        trainer = tr.LoraTrainer(unet, lr=1e-3, capture_graph=graph)
        lat, _, _, ctx = orc.synthetic_batch(0, 4, 8, 6, 32)
        del seen[:]
        for _ in range(3):
            assert torch.isfinite(trainer.step(lat.to(DEV), None, None, ctx.to(DEV), seed=9, t_multiplier=0.05)).all()
        assert seen and all(n == 50 and tmax < 50 for n, tmax in seen), seen
        trainer.step(lat.to(DEV), None, None, ctx.to(DEV), seed=9)
        assert seen[-1][0] == 1000


def test_autograd_grad_callers_get_gradients_with_deferral_off(tiny_unet_factory, relerr, monkeypatch):
    """`torch.autograd.grad(loss, lora_params)` is not a `.backward()`: the drop-in sink defers the factor gradients to the end
    of a backward PASS and hands them to `.grad`, so such a caller sees None for them (ops._AutoSink docstring).  The documented
    switch — DFA_DEFER_GRADS=0 — restores per-layer launches that RETURN the gradients: they must equal the deferred ones."""
    unet = tiny_unet_factory(seed=2).to(DEV)
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    plist = list(itertools.chain(*params))
    _warm(plist, 5, 0.02)
    lat, noise, ts, ctx = orc.synthetic_batch(0, 2, 8, 6, 32)

    def loss():
        return dfa.ddpm_mse_loss(unet(lat.to(DEV), ts.to(DEV), ctx.to(DEV)).sample, noise.to(DEV))

    loss().backward()
    deferred = [p.grad.clone() for p in plist]
    for p in plist:
        p.grad = None
    monkeypatch.setenv("DFA_DEFER_GRADS", "0")
    grads = torch.autograd.grad(loss(), plist)
    assert all(p.grad is None for p in plist)
    for g, d in zip(grads, deferred):
        assert relerr(g, d) < 1e-5, relerr(g, d)
