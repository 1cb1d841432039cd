"""`LoraTrainer(optimizer="prodigy")` on an MI355X: every step against the float64 restatement of tests/prodigy_cases.py on the
gradient slab the step itself produced, the routes, accumulation, skipped steps, checkpoints, EMA, refusals, and the untouched
default.  The tiny UNet, the feed and the repeatability fixture are tests/test_gpu_checkpoint.py's.

Not covered here: data parallelism.  The two-ranks-on-one-GPU launcher of tests/test_gpu_dp.py builds its AdamW trainer inside
the worker it spawns and takes no optimizer argument, so it cannot serve without an edit."""
import gc
import itertools
import json
import math
import warnings

import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import formats as fmt
from diffusion_finetuning_amd import trainer as tr
from diffusion_finetuning_amd.attention import set_use_memory_efficient_attention_xformers
from oracle import lora_oracle as orc
from tests import ema_cases as ec
from tests import prodigy_cases as pc
from tests.conftest import build_tiny_unet
from tests.test_gpu_checkpoint import _deterministic_stock_kernels, _feed, _lora_trainer, _pti_feed, _steps, _warm

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _collect_garbage_first():
    """A recording left in a reference cycle by an earlier test must not be destroyed in the middle of another capture."""
    gc.collect()


@pytest.fixture
def repeatable_stock_kernels():
    """tests/test_gpu_checkpoint.py's fixture of the same name: two trainers are compared bit for bit."""
    before = _deterministic_stock_kernels()
    yield
    _deterministic_stock_kernels(False, before)


def _trainer(warm_seed=11, dtype=torch.float32, lr=1.0, **kw):
    """tests/test_gpu_checkpoint.py's `_lora_trainer` under Prodigy at its normal lr = 1."""
    unet = build_tiny_unet(seed=5).to(DEV).to(dtype)
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    _warm(list(itertools.chain(*params)), warm_seed)
    return tr.LoraTrainer(unet, lr=lr, optimizer="prodigy", **kw), unet


def snap(trainer):
    """The optimizer's whole state on the host: (p, m, v, s, p0, the 8 scalars, norm, shadow | None)."""
    n, opt = trainer.slab.numel, trainer.opt
    return {"p": trainer.slab.params[:n].cpu(), "m": opt.exp_avg[:n].cpu(), "v": opt.exp_avg_sq[:n].cpu(), "s": opt.s.cpu(),
            "p0": opt.p0.cpu(), "scalars": opt.scalars.cpu(), "norm": opt.norm.cpu(),
            "shadow": opt.shadow[:n].cpu() if opt.ema_decay is not None else None}


def same(a, b, keys=("p", "m", "v", "s", "p0", "scalars", "norm")):
    return all(ec.same_bits(a[k], b[k]) for k in keys)


def run(trainer, feed, first, last):
    out = []
    for s in range(first, last):
        _steps(trainer, feed, s, s + 1)
        out.append(snap(trainer))
    return out


def _state(sn):
    d, d_max, numerator = sn["scalars"][:3].tolist()
    return {"d": d, "d_max": d_max, "numerator": numerator}


def _parity(trainer, feed, steps, cfg):
    """Every step: the slab after it against `reference` applied to the state before it and the step's own gradient slab."""
    n = trainer.slab.numel
    before, ds = snap(trainer), []
    assert ec.same_bits(before["p0"], before["p"]) and _state(before) == pc.state(cfg["d0"])
    for k in range(steps):
        _steps(trainer, feed, k, k + 1)
        after = snap(trainer)
        g = trainer.slab.grads[:n].cpu()
        t, norm_sq = int(after["norm"][2]), float(after["norm"][0])
        assert t == k + 1 and float(after["norm"][1]) == 0.0
        ref = pc.reference(before["p"], before["p0"], g, before["m"], before["v"], before["s"], _state(before), cfg, t, norm_sq)
        got = dict(after, state=dict(_state(after), d_hat=float(after["scalars"][4]), denom=float(after["scalars"][5])))
        w = pc.worst(got, ref, pc.bounds(ref, n, True))  # (the norm is the launch's own fp32 value: an input, kg = 8)
        print(k, ref["state"]["branch"], f"d = {got['state']['d']:.4g}", {x: float("%.3g" % y) for x, y in w.items()})
        assert max(w.values()) <= 1.0, (k, w)
        assert ec.same_bits(after["p0"], before["p0"]) and float(after["scalars"][3]) == _state(before)["d"]
        ds.append(got["state"]["d"])
        before = after
    return ds


def test_every_step_is_the_restatement_on_the_steps_own_gradient():
    trainer, _ = _trainer()
    assert isinstance(trainer.opt, tr.FusedProdigy) and trainer.opt.ends == [trainer.slab.numel]
    cfg = pc.config(max_norm=1.0, wd=(1e-2,), lr=(1.0,))
    ds = _parity(trainer, _feed, 8, cfg)
    assert ds[-1] > 2 * pc.f32(cfg["d0"]) and all(b >= a for a, b in zip(ds, ds[1:]))
    assert trainer.opt.d() == ds[-1] and trainer.opt.d_history_entry()["applied_steps"] == 8
    assert trainer.opt.d_history_entry()["d"] == ds[-1] and trainer.get_last_lr() == [1.0]


def test_the_options_and_the_schedule_reach_the_kernels():
    kw = dict(prodigy_d0=1e-5, prodigy_d_coef=2.0, prodigy_growth_rate=1.5, prodigy_use_bias_correction=True,
              prodigy_safeguard_warmup=True, weight_decay=0.1, lr_scheduler="linear", max_train_steps=12)
    trainer, _ = _trainer(lr=0.5, **kw)
    n, before = trainer.slab.numel, snap(trainer)
    ds = []
    for k in range(5):
        cfg = pc.config(max_norm=1.0, wd=(0.1,), lr=(0.5 * float(trainer.lr_lambda(k)),), d0=1e-5, d_coef=2.0, growth_rate=1.5,
                        bias_correction=True, safeguard=True)
        assert trainer.lr_lambda(k) == pytest.approx(1 - k / 12)
        _steps(trainer, _feed, k, k + 1)
        after = snap(trainer)
        ref = pc.reference(before["p"], before["p0"], trainer.slab.grads[:n].cpu(), before["m"], before["v"], before["s"],
                           _state(before), cfg, k + 1, float(after["norm"][0]))
        got = dict(after, state=_state(after))
        w = pc.worst(got, ref, pc.bounds(ref, n, True))
        assert max(w.values()) <= 1.0, (k, w)
        ds.append(got["state"]["d"])
        before = after
    d0 = pc.f32(1e-5)  # (the first growth, from d == d0, is not rate-limited; every later one is)
    assert ds[0] >= d0 and all(a <= b <= (b if a == d0 else a * 1.5 * (1 + 1e-6)) for a, b in zip(ds, ds[1:]))


def test_a_lora_text_encoder_is_a_second_range_with_lr_text(golden_pti):
    from tests.test_oracle_golden import build_pti_models

    t, meta = golden_pti
    cfg_g = json.loads(meta["cfg"])
    unet, te = build_pti_models(t, cfg_g, DEV, torch.float32)
    te.requires_grad_(False)
    gu, _ = dfa.inject_trainable_lora(unet, r=4)
    gt, _ = dfa.inject_trainable_lora(te, dfa.TEXT_ENCODER_DEFAULT_TARGET_REPLACE, r=4)
    _warm(list(itertools.chain(*gu)) + list(itertools.chain(*gt)), 11)
    set_use_memory_efficient_attention_xformers(unet, True)
    trainer = tr.LoraTrainer(unet, te, lr=1.0, lr_text=0.25, weight_decay=1e-2, optimizer="prodigy")
    ends = [r[1] for r in trainer.slab.model_ranges]
    assert trainer.token_table is None and trainer.opt.ends == ends and len(ends) == 2 and ends[1] == trainer.slab.numel
    cfg = pc.config(max_norm=1.0, ends=tuple(ends), lr=(1.0, 0.25), wd=(1e-2, 1e-2))
    ds = _parity(trainer, _pti_feed(t, cfg_g), 4, cfg)
    assert ds[-1] > pc.f32(cfg["d0"]) and trainer.get_last_lr() == [1.0, 0.25]


def test_recorded_and_host_launched_runs_end_with_the_same_bits(repeatable_stock_kernels):
    ends = []
    for graph in (False, True):
        trainer, _ = _trainer(capture_graph=graph)
        ends.append(run(trainer, _feed, 0, 5)[-1])
        assert (trainer._graph is not None) == graph
    assert same(ends[0], ends[1]) and ends[0]["scalars"][0] > pc.f32(1e-6)


def test_one_prodigy_step_per_accumulation_window(repeatable_stock_kernels):
    trainer, _ = _trainer(gradient_accumulation_steps=2)
    last = snap(trainer)
    for k, sn in enumerate(run(trainer, _feed, 0, 8)):
        if k % 2 == 0:  # inside a window: nothing of the optimizer moved
            assert same(sn, last) and int(sn["norm"][2]) == k // 2
        else:
            assert int(sn["norm"][2]) == k // 2 + 1 and not ec.same_bits(sn["s"], last["s"])
            assert float(sn["scalars"][3]) == float(last["scalars"][0])  # d_prev: the launch ran, once
        last = sn
    assert trainer.opt.applied_steps() == 4 and trainer.opt.d() > pc.f32(1e-6)


def test_a_step_the_loss_scaler_skips_leaves_s_the_scalars_and_the_count_alone(repeatable_stock_kernels):
    """loss_scale=2**30 on the f16 tiny UNet: the first steps overflow (tests/test_gpu_checkpoint.py's recipe)."""
    N = 40
    feed = lambda s: {**_feed(s), "seed": 7}  # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the trainer reports the first skipped step)
        trainer, _ = _trainer(dtype=torch.float16, loss_scale=2.0 ** 30)
        last, skipped, applied = snap(trainer), 0, 0
        for k, sn in enumerate(run(trainer, feed, 0, N)):
            if int(sn["norm"][2]) == int(last["norm"][2]):
                skipped += 1
                assert same(sn, last, ("p", "m", "v", "s", "p0", "scalars")) and int(sn["norm"][3]) == int(last["norm"][3]) + 1
            else:
                applied += 1
                assert int(sn["norm"][2]) == int(last["norm"][2]) + 1 and not ec.same_bits(sn["s"], last["s"])
            last = sn
    print(f"\n[prodigy under overflow] {skipped} skipped, {applied} applied of {N}")
    assert skipped >= 3 and applied >= 3 and trainer.opt.applied_steps() == applied and trainer.opt.skipped_steps() == skipped


def test_save_and_load_mid_run_leave_the_bits_of_the_uninterrupted_run(tmp_path, repeatable_stock_kernels):
    kw = dict(prodigy_growth_rate=2.0, ema_decay=0.5)
    keys = ("p", "m", "v", "s", "p0", "scalars", "norm", "shadow")
    straight, _ = _trainer(**kw)
    want = run(straight, _feed, 0, 12)  # (d leaves d0 at the fifth step: the save at 6 of 12 has an estimate under way)
    first, _ = _trainer(**kw)
    run(first, _feed, 0, 6)
    path = tmp_path / "prodigy.safetensors"
    first.save_checkpoint(path)
    sd = fmt.load_checkpoint_file(path)
    n = first.slab.numel
    assert sd["meta"]["optimizer"] == "prodigy" and sd["meta"]["prodigy"] == first.opt.options()
    assert sd["meta"]["prodigy"]["growth_rate"] == 2.0 and sd["meta"]["config"]["optimizer"] == "prodigy"
    assert ec.same_bits(sd["tensors"]["lora.prodigy.s"], want[5]["s"]) and ec.same_bits(sd["tensors"]["lora.prodigy.p0"], want[5]["p0"])
    assert sd["tensors"]["lora.prodigy.s"].shape == (n,) and ec.same_bits(sd["tensors"]["opt.prodigy"], want[5]["scalars"][:3])
    assert float(sd["tensors"]["opt.prodigy"][0]) > pc.f32(1e-6)  # (the estimate was under way at the save)
    fresh, _ = _trainer(warm_seed=12, **kw)  # other factors: its p0 differs until the load
    assert not ec.same_bits(snap(fresh)["p0"], want[5]["p0"])
    addresses = (fresh.opt.s.data_ptr(), fresh.opt.p0.data_ptr(), fresh.opt.scalars.data_ptr())
    fresh.load_checkpoint(path)
    assert addresses == (fresh.opt.s.data_ptr(), fresh.opt.p0.data_ptr(), fresh.opt.scalars.data_ptr())
    assert same(snap(fresh), want[5], ("p", "m", "v", "s", "p0", "shadow")) and ec.same_bits(snap(fresh)["scalars"][:3], want[5]["scalars"][:3])
    got = run(fresh, _feed, 6, 12)
    for k in range(6):
        assert same(got[k], want[6 + k], keys), k


def test_a_save_inside_the_overflow_phase_continues_exactly(tmp_path, repeatable_stock_kernels):
    N, K = 40, 2  # (the first steps under loss_scale 2**30 overflow: step 2 is inside that phase)
    feed = lambda s: {**_feed(s), "seed": 7}  # noqa: E731
    kw = dict(dtype=torch.float16, loss_scale=2.0 ** 30)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        straight, _ = _trainer(**kw)
        want = run(straight, feed, 0, N)
        assert int(want[K - 1]["norm"][2]) == 0 and straight.opt.applied_steps() >= 3, "the save was not inside the overflow phase"
        first, _ = _trainer(**kw)
        run(first, feed, 0, K)
        first.save_checkpoint(tmp_path / "overflow.safetensors")
        fresh, _ = _trainer(warm_seed=12, **kw)
        fresh.load_checkpoint(tmp_path / "overflow.safetensors")
        got = run(fresh, feed, K, N)
    assert [int(g["norm"][2]) for g in got] == [int(w["norm"][2]) for w in want[K:]]
    assert same(got[-1], want[-1])


def _everything(trainer):
    sn = snap(trainer) if trainer.optimizer == "prodigy" else None
    n = trainer.slab.numel
    out = [trainer.slab.params[:n].cpu(), trainer.opt.exp_avg[:n].cpu(), trainer.opt.exp_avg_sq[:n].cpu(), trainer.opt.norm.cpu()]
    if sn is not None:
        out += [sn["s"], sn["p0"], sn["scalars"]]
    return out, (trainer.opt.step_count, trainer.scheduler_epoch, trainer._micro)


def test_adamw_and_prodigy_files_are_refused_by_the_other_kind(tmp_path):
    prodigy, _ = _trainer()
    adamw, _ = _lora_trainer()
    run(prodigy, _feed, 0, 2)
    _steps(adamw, _feed, 0, 2)
    prodigy.save_checkpoint(tmp_path / "prodigy.safetensors")
    adamw.save_checkpoint(tmp_path / "adamw.safetensors")
    saved = fmt.load_checkpoint_file(tmp_path / "adamw.safetensors")
    assert "optimizer" not in saved["meta"] and not any("prodigy" in k for k in saved["tensors"])
    for target, path in ((_trainer(warm_seed=12)[0], "adamw.safetensors"), (_lora_trainer(warm_seed=12)[0], "prodigy.safetensors")):
        before, host = _everything(target)
        with pytest.raises(ValueError, match="optimizer="):
            target.load_checkpoint(tmp_path / path)
        after, host_after = _everything(target)
        assert host_after == host and all(ec.same_bits(a, b) for a, b in zip(after, before)), "a refused load wrote"
    # a file whose header is silent about the optimizer but whose tensors are the other kind's is refused by the tensor check
    sd = prodigy.state_dict()
    del sd["meta"]["optimizer"]
    target = _lora_trainer(warm_seed=12)[0]
    before, host = _everything(target)
    with pytest.raises(ValueError, match="lora.prodigy"):
        target.load_state_dict(sd)
    assert all(ec.same_bits(a, b) for a, b in zip(_everything(target)[0], before))
    sd = adamw.state_dict()
    target = _trainer(warm_seed=12)[0]
    sd["meta"]["optimizer"], sd["meta"]["prodigy"] = "prodigy", target.opt.options()
    before, host = _everything(target)
    with pytest.raises(ValueError, match="lora.prodigy"):
        target.load_state_dict(sd)
    assert all(ec.same_bits(a, b) for a, b in zip(_everything(target)[0], before))
    # a Prodigy file written with another d0 is refused too (the first growth hangs on d == d0); other options only warn
    target = _trainer(warm_seed=12, prodigy_d0=1e-5)[0]
    before, host = _everything(target)
    with pytest.raises(ValueError, match="prodigy_d0"):
        target.load_checkpoint(tmp_path / "prodigy.safetensors")
    assert _everything(target)[1] == host and all(ec.same_bits(a, b) for a, b in zip(_everything(target)[0], before))
    target = _trainer(warm_seed=12, prodigy_growth_rate=1.5)[0]
    with pytest.warns(UserWarning, match="prodigy_growth_rate"):
        target.load_checkpoint(tmp_path / "prodigy.safetensors")
    assert ec.same_bits(snap(target)["s"], snap(prodigy)["s"])


def test_with_ema_the_parameters_are_those_without_and_ema_weights_works(repeatable_stock_kernels):
    plain, _ = _trainer()
    want = run(plain, _feed, 0, 5)
    trainer, unet = _trainer(ema_decay=0.5)
    shadow = snap(trainer)["shadow"]
    assert ec.same_bits(shadow, snap(trainer)["p"])
    for k, sn in enumerate(run(trainer, _feed, 0, 5)):
        assert same(sn, want[k]), (k, "the state differs from a trainer without EMA")
        shadow = ec.ema_emulate(shadow, sn["p"], ec.omd_at(k + 1, 0.5, 0))
        assert ec.same_bits(sn["shadow"], shadow), (k, int((ec.bits(sn["shadow"]) != ec.bits(shadow)).sum()))
    live = snap(trainer)
    with trainer.ema_weights():
        assert ec.same_bits(tr.flat_lora_state(unet).cpu(), live["shadow"]) and ec.same_bits(snap(trainer)["shadow"], live["p"])
        with pytest.raises(RuntimeError, match="ema_weights"):
            trainer.step(**_feed(5))
    assert same(snap(trainer), live) and ec.same_bits(snap(trainer)["shadow"], live["shadow"])
    assert "lora.ema" in trainer.state_dict()["tensors"]


def test_refusals_at_construction(golden_pti):
    for kw in (dict(prodigy_d0=0.0), dict(prodigy_d0=-1e-6), dict(prodigy_d0=math.inf), dict(prodigy_d_coef=0.0),
               dict(prodigy_growth_rate=0.99), dict(prodigy_growth_rate=math.nan), dict(prodigy_use_bias_correction=1),
               dict(prodigy_safeguard_warmup="yes"), dict(betas=(0.9, 1.0))):
        with pytest.raises(ValueError, match="prodigy|Prodigy"):
            _trainer(**kw)
    with pytest.raises(ValueError, match="optimizer"):
        _lora_trainer(optimizer="adam")
    with pytest.raises(ValueError, match="prodigy_d0"):
        _lora_trainer(prodigy_d0=0.0)  # (checked whichever optimizer runs)
    from tests.test_oracle_golden import build_pti_models

    t, meta = golden_pti
    unet, te = build_pti_models(t, json.loads(meta["cfg"]), DEV, torch.float32)
    orc.freeze_all_but_token_embeddings(te)
    dfa.inject_trainable_lora(unet, r=4)
    with pytest.raises(ValueError, match="token table"):
        tr.LoraTrainer(unet, te, lr=1.0, optimizer="prodigy")


def test_the_default_is_adamw_untouched(monkeypatch):
    trainer, _ = _lora_trainer()
    explicit, _ = _lora_trainer(optimizer="adamw")
    for t in (trainer, explicit):
        _steps(t, _feed, 0, 1)
        assert t.optimizer == "adamw" and type(t.opt) is tr.FusedClipAdamW
        assert not any(hasattr(t.opt, name) for name in ("s", "p0", "scalars", "ends", "d0"))
        sd = t.state_dict()
        assert sorted(sd["tensors"]) == ["lora.exp_avg", "lora.exp_avg_sq", "lora.params", "opt.norm"]
        assert "optimizer" not in sd["meta"] and "prodigy" not in sd["meta"]
        assert not any("prodigy" in k or k == "optimizer" for k in sd["meta"]["config"])
    calls = []
    for name in ("lora_grad_sqnorm", "lora_adamw_step", "lora_adamw_ema_step", "lora_prodigy_moments", "lora_prodigy_apply"):
        real = getattr(tr.nat, name)
        monkeypatch.setattr(tr.nat, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    _steps(trainer, _feed, 1, 2)
    assert calls == ["lora_grad_sqnorm", "lora_adamw_step"]
    del calls[:]
    prodigy, _ = _trainer()
    _steps(prodigy, _feed, 0, 1)
    assert calls == ["lora_grad_sqnorm", "lora_prodigy_moments", "lora_prodigy_apply"]
