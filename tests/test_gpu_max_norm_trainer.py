"""`LoraTrainer(max_weight_norm=...)` on an MI355X: the projection after every optimizer step, on every route, with both
optimizers, the EMA, a checkpoint, a trainable token table, and the untouched default.

The tiny UNet, the feed and the repeatability fixture are tests/test_gpu_checkpoint.py's; the restatement and the derived
bound are tests/max_norm_cases.py's.  Two trainers are compared BIT FOR BIT."""
import gc
import itertools
import json
import math
import warnings

import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import trainer as tr
from diffusion_finetuning_amd.attention import set_use_memory_efficient_attention_xformers
from diffusion_finetuning_amd.max_norm import LayerNorms
from oracle import lora_oracle as orc
from tests import ema_cases as ec
from tests import max_norm_cases as mc
from tests.conftest import build_tiny_unet
from tests.test_gpu_checkpoint import _deterministic_stock_kernels, _feed, _pti_feed, _steps, _warm

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = mc.U


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


def _trainer(warm_seed=11, lr=1e-2, **kw):
    """tests/test_gpu_checkpoint.py's `_lora_trainer` at a learning rate that moves the norms within a few steps."""
    unet = build_tiny_unet(seed=5).to(DEV)
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    _warm(list(itertools.chain(*params)), warm_seed)
    return tr.LoraTrainer(unet, lr=lr, **kw), unet


def lora(trainer):
    return trainer.slab.params[: trainer.slab.numel].cpu()


def host_layers(trainer):
    return [(l.lora_up.weight.detach().float().cpu().clone(), l.lora_down.weight.detach().float().cpu().clone(), l.scale)
            for l in trainer.slab.layers]


def measured(trainer):
    """The norms of the slab as it is now, from a table of the test's own."""
    norms = LayerNorms.of_slab(trainer.slab)
    norms.launch()
    return norms.stats[:, 0].cpu()


def state(trainer):
    n, opt = trainer.slab.numel, trainer.opt
    out = {"p": trainer.slab.params.cpu(), "m": opt.exp_avg[:n].cpu(), "v": opt.exp_avg_sq[:n].cpu(), "norm": opt.norm.cpu()}
    if opt.ema_decay is not None:
        out["shadow"] = opt.shadow[:n].cpu()
    if trainer.optimizer == "prodigy":
        out.update(s=opt.s.cpu(), p0=opt.p0.cpu(), scalars=opt.scalars.cpu())
    return out


def same_state(a, b):
    return a.keys() == b.keys() and all(ec.same_bits(a[k], b[k]) for k in a)


@pytest.fixture(scope="module")
def free_run():
    """Six steps WITHOUT the knob: the norms after every step (measured on the spot) — where the bounds below come from."""
    before = _deterministic_stock_kernels()
    try:
        trainer, _ = _trainer()
        assert trainer.max_weight_norm is None and trainer._clamp is None
        norms, losses = [], []
        for s in range(6):
            losses += _steps(trainer, _feed, s, s + 1)
            n, f = trainer.weight_norms()
            assert bool((f == 1.0).all())
            norms.append(n)
        return {"norms": norms, "losses": losses, "state": state(trainer), "layers": host_layers(trainer)}
    finally:
        _deterministic_stock_kernels(False, before)


def middle_bound(free_run):
    """A bound that some layers cross within the six steps and others never reach: the median of the last norms."""
    last = free_run["norms"][-1]
    return f32(float(last.sort().values[last.numel() // 2]) * 0.999)


def f32(x):
    """x rounded to fp32, as a double: a bound the kernel receives exactly."""
    return float(torch.tensor(x, dtype=torch.float32))


@pytest.fixture(scope="module")
def start_bound():
    """A bound that half the layers exceed from the first step on, under either optimizer: the median of the norms every
    trainer of this file starts from."""
    trainer, _ = _trainer()
    first = measured(trainer)
    return f32(float(first.sort().values[first.numel() // 2]) * 0.999)


# -- 1. the clamp holds ----------------------------------------------------------------------------------------------------------
def test_every_layer_stays_on_or_inside_the_bound_after_every_step(free_run, repeatable_stock_kernels):
    bound = middle_bound(free_run)
    trainer, _ = _trainer(max_weight_norm=bound)
    ever_scaled = torch.zeros(len(trainer.slab.layers), dtype=torch.bool)
    for s in range(6):
        _steps(trainer, _feed, s, s + 1)
        norms, factors = trainer.weight_norms()
        stats = trainer.max_norm_stats()
        scaled = factors != 1.0
        assert stats["keys_scaled"] == int(scaled.sum())
        assert bool((norms[scaled] >= bound).all()) and bool((norms[~scaled] <= bound).all())
        ever_scaled |= scaled
        again = measured(trainer)
        for l, (up, down, scale) in enumerate(host_layers(trainer)):
            limit = (bound * (1 + 4 * U)) ** 2 + mc.norm_squared_bound(up, down, scale)
            assert float(again[l]) ** 2 <= limit, (s, l, float(again[l]), bound)
            if scaled[l]:  # a scaled layer lands ON the bound; its factor is the restatement's for the norm the launch reported
                assert float(again[l]) >= bound * (1 - 1e-5), (s, l, float(again[l]))
                assert abs(float(factors[l]) - math.sqrt(bound / float(norms[l]))) <= 2 * U
        assert stats["max_norm"] <= bound * (1 + 1e-6) and 0.0 < stats["mean_norm"] <= stats["max_norm"]
    print(f"\n[clamp holds] bound {bound:.6g}: {int(ever_scaled.sum())} of {ever_scaled.numel()} layers were scaled at some step")
    assert 0 < int(ever_scaled.sum()) < ever_scaled.numel(), "both populations must be non-empty"


# -- 2. inert above every norm ---------------------------------------------------------------------------------------------------
def test_a_bound_above_every_norm_leaves_the_bits_of_a_trainer_without_the_knob(free_run, repeatable_stock_kernels):
    trainer, _ = _trainer(max_weight_norm=1e6)
    losses = _steps(trainer, _feed, 0, 6)
    assert same_state(state(trainer), free_run["state"])
    assert all(torch.equal(a, b) for a, b in zip(losses, free_run["losses"]))
    norms, factors = trainer.weight_norms()
    assert bool((factors == 1.0).all()) and ec.same_bits(norms, free_run["norms"][-1])
    assert trainer.max_norm_stats()["keys_scaled"] == 0 and int(trainer._clamp.counters.cpu()[0]) == 0


# -- 3. the routes ---------------------------------------------------------------------------------------------------------------
def _prodigy_trainer(**kw):
    return _trainer(lr=1.0, optimizer="prodigy", **kw)


ROUTE_CASES = {
    "adamw": (_trainer, {}, 4),
    "accumulation": (_trainer, {"gradient_accumulation_steps": 2}, 6),
    "prodigy": (_prodigy_trainer, {"prodigy_d0": 1e-4}, 5),
    "ema": (_trainer, {"ema_decay": 0.99}, 4),
}


@pytest.mark.parametrize("name", list(ROUTE_CASES))
def test_host_launched_and_replayed_routes_end_with_the_same_bits(name, start_bound, repeatable_stock_kernels):
    build, kw, steps = ROUTE_CASES[name]
    bound = start_bound
    ends, scaled = [], []
    for graph in (False, True):
        trainer, _ = build(max_weight_norm=bound, capture_graph=graph, **kw)
        start = lora(trainer)
        pre, post = [], []  # the slab as the optimizer left it before each projection, and after it
        clamp = trainer._clamp_norms

        def recording_clamp(clamp=clamp, trainer=trainer, pre=pre, post=post):
            pre.append(lora(trainer))
            clamp()
            post.append(lora(trainer))

        trainer._clamp_norms = recording_clamp
        shadow = trainer.opt.shadow[: trainer.slab.numel].cpu() if name == "ema" else None
        losses = _steps(trainer, _feed, 0, steps)
        assert (trainer._graph is not None) == graph
        assert len(pre) == (steps // 2 if name == "accumulation" else steps)  # once per OPTIMIZER step
        ends.append((state(trainer), losses))
        scaled.append(int(trainer._clamp.counters.cpu()[0]))
        if name == "ema":  # the average is taken inside the optimizer launch: of the values BEFORE the projection
            for k, p in enumerate(pre):
                shadow = ec.ema_emulate(shadow, p, ec.omd_at(k + 1, 0.99, 0))
            assert ec.same_bits(trainer.opt.shadow[: trainer.slab.numel].cpu(), shadow)
            assert any(not ec.same_bits(a, b) for a, b in zip(pre, post))  # (projections did move what was averaged)
        assert ec.same_bits(post[-1], lora(trainer))
        if name == "prodigy":
            assert ec.same_bits(trainer.opt.p0.cpu(), start)  # p0 is not rescaled
    assert scaled[0] == scaled[1] > 0, scaled
    assert same_state(ends[0][0], ends[1][0])
    assert all(torch.equal(a, b) for a, b in zip(ends[0][1], ends[1][1]))


# -- 4. checkpoint ---------------------------------------------------------------------------------------------------------------
def test_save_and_load_mid_run_leave_the_bits_of_the_uninterrupted_run(tmp_path, start_bound, repeatable_stock_kernels):
    bound = start_bound
    straight, _ = _trainer(max_weight_norm=bound)
    want_losses = _steps(straight, _feed, 0, 6)
    assert int(straight._clamp.counters.cpu()[0]) > 0
    first, _ = _trainer(max_weight_norm=bound)
    _steps(first, _feed, 0, 3)
    path = tmp_path / "step3.safetensors"
    first.save_checkpoint(path)
    second, _ = _trainer(warm_seed=12, max_weight_norm=bound)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        second.load_checkpoint(path)
    assert not [x for x in w if "NOT restored" in str(x.message)]
    got_losses = _steps(second, _feed, 3, 6)
    assert same_state(state(second), state(straight))
    assert all(torch.equal(a, b) for a, b in zip(got_losses, want_losses[3:]))
    assert all(ec.same_bits(a, b) for a, b in zip(second.weight_norms(), straight.weight_norms()))

    other, _ = _trainer(max_weight_norm=2 * bound)  # another bound: one warning, naming the key; nothing restored
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        other.load_checkpoint(path)
    text = [str(x.message) for x in w if "NOT restored" in str(x.message)]
    assert len(text) == 1 and "max_weight_norm" in text[0] and other.max_weight_norm == 2 * bound


def test_files_of_a_trainer_without_the_knob_load_and_a_file_without_the_key_reads_as_none(tmp_path, start_bound):
    plain, _ = _trainer()
    _steps(plain, _feed, 0, 1)
    path = tmp_path / "plain.safetensors"
    plain.save_checkpoint(path)
    knob, _ = _trainer(warm_seed=12, max_weight_norm=start_bound)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        knob.load_checkpoint(path)
    text = [str(x.message) for x in w if "NOT restored" in str(x.message)]
    assert len(text) == 1 and "max_weight_norm: checkpoint None" in text[0]
    assert ec.same_bits(lora(knob), lora(plain))
    _steps(knob, _feed, 1, 2)  # and it trains on, with the projection
    sd = plain.state_dict()
    assert sd["meta"]["config"].pop("max_weight_norm") is None  # a file from before the knob existed
    fresh, _ = _trainer(warm_seed=12)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        fresh.load_state_dict(sd)
    assert not [x for x in w if "NOT restored" in str(x.message)]


# -- 5. the token table ----------------------------------------------------------------------------------------------------------
def _pti_trainer(t, cfg, **kw):
    """tests/test_gpu_checkpoint.py's `_pti_trainer` with the trainer's keywords open."""
    from tests.test_oracle_golden import build_pti_models

    unet, te = build_pti_models(t, cfg, DEV, torch.float32)
    orc.freeze_all_but_token_embeddings(te)
    gu, _ = dfa.inject_trainable_lora(unet, r=4)
    gt, _ = dfa.inject_trainable_lora(te, dfa.TEXT_ENCODER_DEFAULT_TARGET_REPLACE, r=4)
    _warm(list(itertools.chain(*gu)) + list(itertools.chain(*gt)), 11)
    set_use_memory_efficient_attention_xformers(unet, True)
    trainer = tr.LoraTrainer(unet, te, lr=1e-3, lr_text=3e-4, lr_embed=5e-3, weight_decay=1e-2, weight_decay_embed=1e-3,
                             v_prediction=True, lr_scheduler="linear", max_train_steps=6, scheduler_steps_first=True, **kw)
    assert trainer.token_table is not None and len(trainer.slab.models) == 2
    return trainer


def test_the_token_table_and_the_padding_are_never_written(golden_pti, repeatable_stock_kernels):
    t, meta = golden_pti
    cfg = json.loads(meta["cfg"])
    feed = _pti_feed(t, cfg)
    plain = _pti_trainer(t, cfg)
    _steps(plain, feed, 0, 3)
    inert = _pti_trainer(t, cfg, max_weight_norm=1e6)
    _steps(inert, feed, 0, 3)
    assert inert._clamp.n_layers == len(inert.slab.layers) > len(tr.lora_layers(inert.unet))  # both models' layers
    assert int(inert._clamp.counters.cpu()[0]) == 0
    assert ec.same_bits(inert.slab.params.cpu(), plain.slab.params.cpu())  # no layer scaled: the whole slab, tail included
    # scaling active: a bound under every norm, applied by the trainer's own method on the slab as it is
    norms, _ = inert.weight_norms()
    numel, stride = inert.slab.numel, inert.slab.stride
    before = inert.slab.params.cpu()
    inert.max_weight_norm = float(norms[norms > 0].min()) * 0.5
    inert._clamp_norms()
    after = inert.slab.params.cpu()
    _, factors = inert.weight_norms()
    assert int((factors != 1.0).sum()) == int((norms > 0).sum()) > 0
    assert not ec.same_bits(after[:numel], before[:numel])
    assert ec.same_bits(after[numel:], before[numel:]) and after[stride:].numel() == inert.token_table.V * inert.token_table.D
    a, b = inert.token_table.range
    assert ec.same_bits(after[a:b], plain.slab.params[a:b].cpu())


# -- 6. the default --------------------------------------------------------------------------------------------------------------
def test_without_the_knob_nothing_is_allocated_and_the_norms_are_measured_on_demand():
    trainer, unet = _trainer()
    assert trainer.max_weight_norm is None and trainer._clamp is None and trainer._config()["max_weight_norm"] is None
    _steps(trainer, _feed, 0, 1)
    assert trainer._clamp is None
    norms, factors = trainer.weight_norms()
    assert trainer._clamp is None and bool((factors == 1.0).all()) and norms.shape == (len(trainer.slab.layers),)
    assert ec.same_bits(norms, dfa.lora_weight_norms(unet).cpu())  # the helper reads the slab's views where they are
    for l, (up, down, scale) in enumerate(host_layers(trainer)):
        ref = mc.product_norm(up, down, scale)
        assert abs(float(norms[l]) ** 2 - ref * ref) <= mc.norm_squared_bound(up, down, scale), (l, float(norms[l]), ref)
    assert trainer.max_norm_stats()["keys_scaled"] == 0


@pytest.mark.parametrize("value", [0, -1.0, math.inf, math.nan, "1"])
def test_a_bad_bound_raises_at_construction(value):
    unet = build_tiny_unet(seed=5).to(DEV)
    dfa.inject_trainable_lora(unet, r=4)
    with pytest.raises(ValueError, match="max_weight_norm"):
        tr.LoraTrainer(unet, max_weight_norm=value)
