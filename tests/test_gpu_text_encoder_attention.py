"""The attention switch on the text encoder: transformers' CLIPAttention running its causal core through
csrc/attn_causal.hip (attention._hip_clip_forward → sandwich.causal_attention).

1. a LoRA-injected CLIP text model, switched and un-switched, against the same model in float64 on the CPU;
2. the core is really used for the text tower's own call, and every call outside its envelope is handed back bit for bit;
3. under a LoraTrainer (host-launched and recorded into a hipGraph, grouped projections on and off) the switched run
   follows the un-switched one, and the grouped q/k/v launch of groups.shared_projection survives the switch."""
import itertools

import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import trainer as tr
from diffusion_finetuning_amd.attention import set_use_hip_attention, set_use_memory_efficient_attention_xformers
from oracle import lora_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNEL_TOL = {torch.float16: 2e-3, torch.bfloat16: 1.2e-2}  # the kernel-level bounds of tests/test_gpu_causal_attention.py


def _clip(hidden, heads, positions=77, impl=None, seed=4):
    from transformers import CLIPTextConfig, CLIPTextModel

    cfg = CLIPTextConfig(hidden_size=hidden, intermediate_size=2 * hidden, num_hidden_layers=2, num_attention_heads=heads,
                         vocab_size=60, max_position_embeddings=positions, bos_token_id=1, eos_token_id=2, pad_token_id=0)
    if impl is not None:
        cfg._attn_implementation = impl
    torch.manual_seed(seed)
    te = CLIPTextModel(cfg)
    te.requires_grad_(False)
    return te.eval()


def _ids(positions=77, seed=3):
    return torch.randint(3, 60, (2, positions), generator=torch.Generator().manual_seed(seed))


def _count_core_calls(monkeypatch):
    calls = []
    real = nat.attn_causal_fwd
    monkeypatch.setattr(nat, "attn_causal_fwd", lambda *a, **k: (calls.append(tuple(a[0].shape)), real(*a, **k))[1])
    return calls


def _relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_switched_text_encoder_against_float64(dtype):
    """Hidden 128, 2 layers, 2 heads of 64, 77 positions, LoRA r = 4 on CLIPAttention.  `te(ids)[0]` and the LoRA factor
    gradients of the stock and of the switched model, each against the SAME model (weights rounded to `dtype`) in float64 on
    the CPU.  The switched error may be at most twice the stock error — two correct 16-bit evaluations round in different
    places — and need never be below the kernel-level bound of the dtype."""
    ids = _ids()
    base = _clip(128, 2).to(dtype)
    state = {k: v.clone() for k, v in base.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    go = torch.randn(2, 77, 128, generator=g)

    ref = _clip(128, 2).double()
    ref.load_state_dict({k: v.double() for k, v in state.items()})
    rparams, _ = orc.inject(ref, orc.TEXT_ENCODER_TARGETS, r=4)
    factors = [(torch.randn(p.shape, generator=g) * 0.05) for p in rparams]
    with torch.no_grad():
        for p, f in zip(rparams, factors):
            p.copy_(f.double())
    out_ref = ref(ids)[0]
    (out_ref * go.double()).sum().backward()
    grad_ref = torch.cat([p.grad.reshape(-1) for p in rparams])
    out_ref = out_ref.detach()

    def run(switched):
        te = _clip(128, 2).to(dtype)
        te.load_state_dict(state)
        te = te.to(DEV)
        params, _ = dfa.inject_trainable_lora(te, dfa.TEXT_ENCODER_DEFAULT_TARGET_REPLACE, r=4)
        plist = list(itertools.chain(*params))
        assert len(plist) == len(rparams)
        with torch.no_grad():
            for p, f in zip(plist, factors):
                p.copy_(f.to(DEV))
        if switched:
            assert set_use_hip_attention(te, True) == 2
        out = te(ids.to(DEV))[0]
        (out.float() * go.to(DEV)).sum().backward()
        grad = torch.cat([p.grad.reshape(-1) for p in plist])
        return _relerr(out.detach(), out_ref), _relerr(grad, grad_ref)

    stock_o, stock_g = run(False)
    hip_o, hip_g = run(True)
    print(f"{dtype}: output rel err stock {stock_o:.3e} switched {hip_o:.3e}; "
          f"LoRA gradient rel err stock {stock_g:.3e} switched {hip_g:.3e}")
    tol = KERNEL_TOL[dtype]
    assert stock_o < 10 * tol and stock_g < 10 * tol  # (the float64 model is the same model)
    assert hip_o <= max(2 * stock_o, tol), (hip_o, stock_o)
    assert hip_g <= max(2 * stock_g, tol), (hip_g, stock_g)


def test_core_is_used_and_everything_else_is_handed_back(monkeypatch):
    ids = _ids().to(DEV)
    calls = _count_core_calls(monkeypatch)

    def pair(dtype, impl=None):
        te = _clip(128, 2, impl=impl).to(dtype).to(DEV)
        return te

    # the text tower's own call: one core launch per layer per forward
    te = pair(torch.float16)
    with torch.no_grad():
        want = te(ids)[0]
        assert not calls
        assert set_use_hip_attention(te, True) == 2
        got = te(ids)[0]
        assert calls == [(2, 77, 128)] * 2
        assert _relerr(got, want) < 2e-3
        # a padding mask: handed back, bit for bit
        del calls[:]
        mask = torch.ones_like(ids)
        mask[:, 60:] = 0
        padded = te(ids, attention_mask=mask)[0]
        assert not calls
        set_use_hip_attention(te, False)
        assert torch.equal(padded, te(ids, attention_mask=mask)[0])
        # fp32 model
        te32 = pair(torch.float32)
        want32 = te32(ids)[0]
        assert set_use_hip_attention(te32, True) == 2
        assert torch.equal(te32(ids)[0], want32) and not calls
        # the eager implementation passes its 4-D mask tensor
        tee = pair(torch.float16, impl="eager")
        wante = tee(ids)[0]
        assert set_use_hip_attention(tee, True) == 2
        assert torch.equal(tee(ids)[0], wante) and not calls
        # attention dropout while training: handed back (drawn from the same generator state → the same output)
        ted = pair(torch.float16)
        for m in ted.modules():
            if m.__class__.__name__ == "CLIPAttention":
                m.dropout = 0.5
        ted.train()
        assert set_use_hip_attention(ted, True) == 2
        ted(ids)
        assert not calls
        ted.eval()
        ted(ids)
        assert len(calls) == 2


def _tiny64(seed=6):
    from harness.unet import UNet2DConditionModel, tiny_config

    torch.manual_seed(seed)
    unet = UNet2DConditionModel(tiny_config(64, 64, 2))  # widths 64/128, context 64 (tests/test_gpu_groups.py)
    unet.requires_grad_(False)
    return unet


def _warm(params, seed=11, std=0.02):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i, p in enumerate(params):
            if i % 2 == 0:
                p.copy_((torch.randn(p.shape, generator=g) * std).to(p.device))


@pytest.mark.parametrize("r", [4, 8])
@pytest.mark.parametrize("grouped", [True, False], ids=["groups", "no_groups"])
def test_trainer_follows_the_unswitched_run(relerr, monkeypatch, grouped, r):
    """tests/test_gpu_groups.py::test_clip_attention_projections_share_one_launch's tiny UNet + CLIP with 77 positions: 3
    steps with `input_ids`, the switch flipped on the text encoder before the LoraTrainer is built.  Losses and the LoRA slab
    follow the un-switched run within that test's bound (2e-3), host-launched and recorded; under groups the grouped CLIP
    launches per step are the un-switched count (the projections are still called as modules on one tensor)."""
    ids = _ids()

    def train(switched, graph=False):
        te = _clip(64, 2)
        unet = _tiny64()
        unet, te = unet.to(DEV).half(), te.to(DEV).half()
        gu, _ = dfa.inject_trainable_lora(unet, r=4)
        gt, _ = dfa.inject_trainable_lora(te, dfa.TEXT_ENCODER_DEFAULT_TARGET_REPLACE, r=r)
        _warm(list(itertools.chain(*gu)) + list(itertools.chain(*gt)))
        set_use_memory_efficient_attention_xformers(unet, True)
        if switched:
            assert set_use_hip_attention(te, True) == 2
        trainer = tr.LoraTrainer(unet, te, lr=1e-3, lr_text=3e-4, group_projections=grouped, capture_graph=graph)
        packed, parts = [], []
        real_p, real_q = nat.lora_gemm_packed, nat.lora_gemm_parts
        monkeypatch.setattr(nat, "lora_gemm_packed", lambda *a, **k: (packed.append((a[11], a[12], a[13])), real_p(*a, **k))[1])
        monkeypatch.setattr(nat, "lora_gemm_parts", lambda *a, **k: (parts.append(1), real_q(*a, **k))[1])
        core = _count_core_calls(monkeypatch)
        losses = []
        for step in range(3):
            lat, noise, ts, _ = orc.synthetic_batch(step, 2, 8, 8, 64)
            losses.append(trainer.step(lat.to(DEV), noise.to(DEV), ts.to(DEV), input_ids=ids.to(DEV)))
        monkeypatch.undo()
        clip_packed = [c for c in packed if c[0] == 2 * 77 and 192 in (c[1], c[2])]  # M = 2·77 tokens, 64 ↔ 3·64
        return (trainer, trainer.slab.params[: trainer.slab.numel].cpu(), torch.stack(losses).reshape(-1).cpu(),
                len(clip_packed), len(parts), len(core))

    _, want, lw, packed_w, parts_w, core_w = train(False)
    t_s, got, ls, packed_s, parts_s, core_s = train(True)
    assert core_w == 0 and core_s == 3 * 2  # 3 steps × 2 CLIP layers
    assert torch.isfinite(ls).all()
    assert relerr(ls, lw) < 2e-3 and relerr(got, want) < 2e-3, (relerr(ls, lw), relerr(got, want))
    assert (packed_s, parts_s) == (packed_w, parts_w)  # the grouped launches per step did not change
    if grouped:
        assert len([g for g in t_s.slab.qkv_groups if g.layers[0].linear.bias is not None]) == 2
        assert packed_s == (3 * 2 * 2 if r == 4 else 0)  # r = 8: the wide group goes through lora_gemm_parts
    t_r, got_r, lr_, _, _, core_r = train(True, graph=True)
    assert t_r._graph is not None and core_r >= 2  # recorded once (plus any host-launched warm-up), then replayed
    assert relerr(lr_, lw) < 2e-3 and relerr(got_r, want) < 2e-3, (relerr(lr_, lw), relerr(got_r, want))
