"""Checkpoint / resume of LoraTrainer and InversionTrainer.  The yardstick everywhere is THE UNINTERRUPTED RUN: N steps
straight against k steps, save_checkpoint, load_checkpoint into a fresh trainer — built around a fresh model whose factors were
warmed with another seed, so that whatever is not restored shows — and N − k steps.  Everything is compared with torch.equal:
the kernels are reduction-ordered and the noise is keyed by (seed, step), so a continuation leaves the bits of the run that was
never stopped."""
import gc
import itertools
import json
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import formats as fmt
from diffusion_finetuning_amd import step as stp
from diffusion_finetuning_amd import trainer as tr
from diffusion_finetuning_amd.attention import set_use_memory_efficient_attention_xformers
from diffusion_finetuning_amd.inversion import InversionTrainer
from oracle import lora_oracle as orc
from tests.conftest import build_tiny_unet

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _collect_garbage_first():
    """A recording left in a reference cycle by an earlier test must not be destroyed in the middle of another capture."""
    gc.collect()


def _deterministic_stock_kernels(on=True, before=None):
    if on:
        before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
                  torch.backends.cudnn.deterministic)
        torch.use_deterministic_algorithms(True, warn_only=True)
        torch.backends.cudnn.deterministic = True
        return before
    torch.use_deterministic_algorithms(before[0], warn_only=before[1])
    torch.backends.cudnn.deterministic = before[2]


@pytest.fixture
def repeatable_stock_kernels():
    """The stock fp32 kernels under the tiny models do not repeat bit for bit by default on this stack (profiles/README.md,
    "Repeatability of the fp32 inversion step"): two runs of the SAME trainer already differ in the last bits, so a
    bit-for-bit comparison of two trainers says nothing.  With torch's deterministic algorithms they repeat."""
    before = _deterministic_stock_kernels()
    yield
    _deterministic_stock_kernels(False, before)


def _warm(params, seed, std=0.02):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i, p in enumerate(params):
            if i % 2 == 0:
                p.copy_(torch.randn(p.shape, generator=g).to(p.device) * std)


def _lora_trainer(warm_seed=11, dtype=torch.float32, rank=4, **kw):
    unet = build_tiny_unet(seed=5).to(DEV).to(dtype)
    params, _ = dfa.inject_trainable_lora(unet, r=rank)
    _warm(list(itertools.chain(*params)), warm_seed)
    return tr.LoraTrainer(unet, lr=1e-3, **kw), unet


def _feed(s):
    """Step s of the tiny shapes: 8×8 latents, batch 2; noise and timesteps are drawn on the device from the seed."""
    lat, _, _, ctx = orc.synthetic_batch(s, 2, 8, 6, 32)
    return dict(latents=lat.to(DEV), seed=41, encoder_hidden_states=ctx.to(DEV))


def _steps(trainer, feed, first, last):
    return [trainer.step(**feed(s)).detach().clone().reshape(()) for s in range(first, last)]


def _snap(trainer):
    """Everything a continuation must reproduce, and everything a refused load must leave alone."""
    tt = trainer.token_table
    return {"lora": [tr.flat_lora_state(m).clone() for m in trainer.slab.models],
            "params": trainer.slab.params.clone(), "exp_avg": trainer.opt.exp_avg.clone(),
            "exp_avg_sq": trainer.opt.exp_avg_sq.clone(), "norm": trainer.opt.norm[2:4].clone(),
            "active": None if tt is None else tt.active.clone(),
            "scalars": (trainer.opt.step_count, trainer.scheduler_epoch, trainer._micro, trainer.get_last_lr(),
                        trainer.loss_scale, json.dumps(trainer.scaler.state_dict()))}


def _assert_same(got, want, what):
    assert got["scalars"] == want["scalars"], (what, got["scalars"], want["scalars"])
    for key in ("params", "exp_avg", "exp_avg_sq", "norm"):
        assert torch.equal(got[key], want[key]), (what, key, (got[key] != want[key]).sum().item())
    for i, (a, b) in enumerate(zip(got["lora"], want["lora"])):
        assert torch.equal(a, b), (what, "flat_lora_state", i)
    assert (got["active"] is None) == (want["active"] is None)
    if got["active"] is not None:
        assert torch.equal(got["active"], want["active"]), (what, "active")


def _assert_losses(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), (what, i, a.item(), b.item())


# -- 1. fp32, linear schedule, device-drawn noise: 6 steps against 3 + 3 ------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_three_steps_save_load_three_steps_leave_the_bits_of_six_steps(tmp_path, graph, repeatable_stock_kernels):
    kw = dict(lr_scheduler="linear", max_train_steps=6, capture_graph=graph)
    straight, _ = _lora_trainer(**kw)
    want_losses = _steps(straight, _feed, 0, 6)
    want = _snap(straight)
    # first of all: the stack repeats.  If it does not, nothing below can be laid at the checkpoint's door.
    again, _ = _lora_trainer(**kw)
    again_losses = _steps(again, _feed, 0, 6)
    same = all(torch.equal(a, b) for a, b in zip(again_losses, want_losses)) and torch.equal(again.slab.params, straight.slab.params)
    assert same, "two UNINTERRUPTED runs of the same trainer differ bit for bit: the stack does not repeat, not the checkpoint"
    _assert_same(_snap(again), want, "second uninterrupted run")
    first, _ = _lora_trainer(**kw)
    _assert_losses(_steps(first, _feed, 0, 3), want_losses[:3], "before the save")
    path = tmp_path / "step3.safetensors"
    first.save_checkpoint(path)
    assert os.listdir(tmp_path) == ["step3.safetensors"]
    fresh, _ = _lora_trainer(warm_seed=12, **kw)
    assert not torch.equal(fresh.slab.params, first.slab.params)
    fresh.load_checkpoint(path)
    _assert_same(_snap(fresh), _snap(first), "right after the load")
    assert fresh.opt.step_count == 3 and fresh.scheduler_epoch == 3 and fresh.opt.applied_steps() == 3
    _assert_losses(_steps(fresh, _feed, 3, 6), want_losses[3:], "after the load")
    _assert_same(_snap(fresh), want, "3 + 3 against 6")
    assert fresh.get_last_lr() == straight.get_last_lr() == [0.0] and fresh.loss_scale == straight.loss_scale == 1.0
    assert (fresh._graph is not None) == graph == (straight._graph is not None)
    meta = fmt.load_checkpoint_file(path)["meta"]
    assert meta["kind"] == "LoraTrainer" and meta["step_count"] == 3 and meta["scheduler_epoch"] == 3
    assert meta["compute_dtype"] == "float32" and meta["world_size"] == 1 and meta["config"]["lr_scheduler"] == "linear"
    assert len(meta["layout"]["models"][0]) == len(first.slab.layers) and meta["layout"]["models"][0][0][3] == 4


def test_a_load_warns_about_other_constructor_arguments_and_restores_none_of_them(tmp_path):
    import warnings

    saver, _ = _lora_trainer(lr_scheduler="linear", max_train_steps=6)
    _steps(saver, _feed, 0, 1)
    saver.save_checkpoint(tmp_path / "a.safetensors")
    other, _ = _lora_trainer(warm_seed=12, lr_scheduler="constant", max_grad_norm=0.5)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        other.load_checkpoint(tmp_path / "a.safetensors")
    text = [str(x.message) for x in w if "NOT restored" in str(x.message)]
    assert len(text) == 1 and "lr_scheduler" in text[0] and "max_grad_norm" in text[0] and "betas" not in text[0]
    assert other.opt.max_grad_norm == 0.5 and other.get_last_lr() == [1e-3] and other.opt.step_count == 1
    assert torch.equal(other.slab.params, saver.slab.params)


# -- 2. fp16 under an absurd loss scale: the scale history with two flags in flight ----------------------------------------
def test_fp16_loss_scale_history_with_two_flags_in_flight_continues_exactly(tmp_path, repeatable_stock_kernels):
    """loss_scale=2**30 makes the first steps overflow; the scale is halved step after step (each flag two steps late) until a
    step comes out clean.  The save is placed from the UNINTERRUPTED run's own history: right after its first clean step j, so
    the two flags in flight are (overflow of j − 1, clean j) and the scale is halved once more after the save."""
    import warnings

    N = 40
    feed = lambda s: {**_feed(s), "seed": 7}
    kw = dict(dtype=torch.float16, loss_scale=2.0 ** 30)

    def run(trainer, first, last, scales, skipped, losses):
        for s in range(first, last):
            losses += _steps(trainer, feed, s, s + 1)
            scales.append(trainer.loss_scale)
            skipped.append(trainer.opt.skipped_steps())

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the trainer reports the first skipped step)
        straight, _ = _lora_trainer(**kw)
        scales, skipped, losses = [], [], []
        run(straight, 0, N, scales, skipped, losses)
        flags = [float(b != a) for a, b in zip([0] + skipped, skipped)]
        assert 0.0 in flags, f"no clean step in {N}: {scales}"
        k = flags.index(0.0) + 1
        print(f"\n[fp16 resume] first clean step {k - 1}, scale history {scales[:k + 4]}, skipped {skipped[-1]} of {N}")
        assert 3 <= k <= N - 3 and scales[k - 1] < 2.0 ** 30 and any(s != scales[k - 1] for s in scales[k:]), (k, scales)
        saver, _ = _lora_trainer(**kw)
        s_scales, s_skipped, s_losses = [], [], []
        run(saver, 0, k, s_scales, s_skipped, s_losses)
        path = tmp_path / "fp16.safetensors"
        saver.save_checkpoint(path)
        scaler = fmt.load_checkpoint_file(path)["meta"]["scaler"]
        assert scaler["inflight"] == flags[k - 2:k] == [1.0, 0.0] and scaler["scale"] == scales[k - 1] and scaler["initial"] == 2.0 ** 30
        fresh, _ = _lora_trainer(warm_seed=12, **kw)
        fresh.load_checkpoint(path)
        r_scales, r_skipped, r_losses = list(s_scales), list(s_skipped), list(s_losses)
        run(fresh, k, N, r_scales, r_skipped, r_losses)
        run(saver, k, N, s_scales, s_skipped, s_losses)  # the trainer that saved runs on: the save consumed nothing
    for who, trainer, got in (("resumed", fresh, (r_scales, r_skipped, r_losses)), ("saver", saver, (s_scales, s_skipped, s_losses))):
        assert got[0] == scales, (who, got[0], scales)
        assert got[1] == skipped, (who, got[1], skipped)
        _assert_losses(got[2], losses, who)
        assert trainer.opt.applied_steps() == straight.opt.applied_steps() >= 1
        assert trainer.opt.skipped_steps() == straight.opt.skipped_steps() >= 3
        _assert_same(_snap(trainer), _snap(straight), who)


# -- 3. text-encoder LoRA + a trainable token table ----------------------------------------------------------------------
def _pti_trainer(t, cfg, warm_seed=11, graph=False):
    from tests.test_oracle_golden import build_pti_models

    unet, te = build_pti_models(t, cfg, DEV, torch.float32)
    orc.freeze_all_but_token_embeddings(te)
    gu, _ = dfa.inject_trainable_lora(unet, r=4)
    gt, _ = dfa.inject_trainable_lora(te, dfa.TEXT_ENCODER_DEFAULT_TARGET_REPLACE, r=4)
    _warm(list(itertools.chain(*gu)) + list(itertools.chain(*gt)), warm_seed)
    set_use_memory_efficient_attention_xformers(unet, True)
    trainer = tr.LoraTrainer(unet, te, lr=1e-3, lr_text=3e-4, lr_embed=5e-3, weight_decay=1e-2, weight_decay_embed=1e-3,
                             v_prediction=True, capture_graph=graph, lr_scheduler="linear", max_train_steps=6,
                             scheduler_steps_first=True)
    assert trainer.token_table is not None and len(trainer.slab.models) == 2 and len(trainer.opt.groups) == 3
    return trainer


def _pti_feed(t, cfg):
    def feed(s):
        lat = orc.synthetic_batch(s, cfg["batch"], cfg["latent_hw"], cfg["ctx_len"], cfg["hidden"])[0]
        return dict(latents=lat.to(DEV), seed=23, input_ids=t["ids"][s % t["ids"].shape[0]].to(DEV),
                    t_multiplier=cfg["t_multiplier"])
    return feed


@pytest.mark.parametrize("graph", [False, True])
def test_token_table_and_text_encoder_lora_continue_exactly_from_a_compact_file(tmp_path, golden_pti, graph,
                                                                                repeatable_stock_kernels):
    t, meta = golden_pti
    cfg = json.loads(meta["cfg"])
    feed = _pti_feed(t, cfg)
    straight = _pti_trainer(t, cfg, graph=graph)
    want_losses = _steps(straight, feed, 0, 6)
    first = _pti_trainer(t, cfg, graph=graph)
    _assert_losses(_steps(first, feed, 0, 3), want_losses[:3], "before the save")
    path = tmp_path / "pti.safetensors"
    first.save_checkpoint(path)
    # the file holds moment rows for the rows that ever had a gradient, and for no other
    tensors = fmt.load_checkpoint_file(path)["tensors"]
    tt = first.token_table
    rows = tt.active.cpu().nonzero().reshape(-1)
    assert 0 < rows.numel() < tt.V
    assert torch.equal(tensors["dense.0.rows"], rows) and torch.equal(tensors["dense.0.active"], tt.active.cpu())
    assert tensors["dense.0.exp_avg.rows"].shape == tensors["dense.0.exp_avg_sq.rows"].shape == (rows.numel(), tt.D)
    assert "dense.0.exp_avg" not in tensors and "dense.0.exp_avg_sq" not in tensors
    assert tensors["dense.0.param"].shape == (tt.V, tt.D) and tensors["lora.params"].numel() == first.slab.numel
    a, b = tt.range
    assert torch.equal(tensors["dense.0.exp_avg_sq.rows"], first.opt.exp_avg_sq[a:b].view(tt.V, tt.D)[rows.to(DEV)].cpu())
    fresh = _pti_trainer(t, cfg, warm_seed=12, graph=graph)
    rows_group = fresh.opt.groups[-1]["rows"]
    fresh.load_checkpoint(path)
    assert fresh.opt.groups[-1]["rows"] is rows_group and rows_group[2] is fresh.token_table.active  # written in place
    _assert_same(_snap(fresh), _snap(first), "right after the load")
    _assert_losses(_steps(fresh, feed, 3, 6), want_losses[3:], "after the load")
    _assert_same(_snap(fresh), _snap(straight), "3 + 3 against 6")
    assert (fresh._graph is not None) == graph


def test_a_moment_outside_the_active_rows_makes_the_save_dense_and_loads_to_the_same_bits(tmp_path, golden_pti,
                                                                                         repeatable_stock_kernels):
    t, meta = golden_pti
    cfg = json.loads(meta["cfg"])
    feed = _pti_feed(t, cfg)
    first = _pti_trainer(t, cfg)
    _steps(first, feed, 0, 3)
    tt = first.token_table
    a, b = tt.range
    idle = int((tt.active == 0).nonzero()[0])
    first.opt.exp_avg[a:b].view(tt.V, tt.D)[idle, 1] = 0.25  # by hand: no kernel leaves a moment on a row without a gradient
    path = tmp_path / "dense.safetensors"
    first.save_checkpoint(path)
    tensors = fmt.load_checkpoint_file(path)["tensors"]
    assert "dense.0.rows" not in tensors and "dense.0.exp_avg.rows" not in tensors
    assert tensors["dense.0.exp_avg"].shape == tensors["dense.0.exp_avg_sq"].shape == (tt.V, tt.D)
    assert tensors["dense.0.exp_avg"][idle, 1] == 0.25
    fresh = _pti_trainer(t, cfg, warm_seed=12)
    fresh.load_checkpoint(path)
    _assert_same(_snap(fresh), _snap(first), "right after the load")
    _assert_losses(_steps(fresh, feed, 3, 6), _steps(first, feed, 3, 6), "after the load")
    _assert_same(_snap(fresh), _snap(first), "both run on")
    assert fresh.opt.exp_avg[a:b].view(tt.V, tt.D)[idle, 1] == 0.25


# -- 4. gradient accumulation: no save inside a window ------------------------------------------------------------------
def test_a_save_inside_an_accumulation_window_is_refused_and_one_at_its_boundary_continues_exactly(tmp_path,
                                                                                                   repeatable_stock_kernels):
    kw = dict(gradient_accumulation_steps=2, lr_scheduler="linear", max_train_steps=3)
    straight, _ = _lora_trainer(**kw)
    want_losses = _steps(straight, _feed, 0, 6)  # three windows of two micro-batches
    first, _ = _lora_trainer(**kw)
    path = tmp_path / "window.safetensors"
    path.write_bytes(b"what was there before")
    losses = _steps(first, _feed, 0, 1)
    assert first._micro == 1
    with pytest.raises(RuntimeError, match="accumulation window"):
        first.save_checkpoint(path)
    with pytest.raises(RuntimeError, match="accumulation window"):
        first.state_dict()
    assert path.read_bytes() == b"what was there before" and os.listdir(tmp_path) == ["window.safetensors"]
    losses += _steps(first, _feed, 1, 2)
    assert first._micro == 0 and first.opt.step_count == 1
    first.save_checkpoint(path)
    _assert_losses(losses, want_losses[:2], "before the save")
    fresh, _ = _lora_trainer(warm_seed=12, **kw)
    fresh.load_checkpoint(path)
    _assert_losses(_steps(fresh, _feed, 2, 6), want_losses[2:], "after the load")
    _assert_same(_snap(fresh), _snap(straight), "1 + 2 windows against 3")
    assert fresh.opt.step_count == 3 == fresh.scheduler_epoch


# -- 5. InversionTrainer: a save at any micro-step -------------------------------------------------------------------------
def _inversion_trainer(t, cfg, graph, nudge=0.0):
    from tests.test_oracle_golden import build_pti_models

    ph = [cfg["vocab"] - 3, cfg["vocab"] - 8]
    unet, te = build_pti_models(t, cfg, DEV, torch.float32)
    orc.freeze_all_but_token_embeddings(te)
    if nudge:  # a fresh model whose placeholder rows start somewhere else: rows that are not restored show
        with torch.no_grad():
            te.get_input_embeddings().weight[ph] += nudge
    trainer = InversionTrainer(unet, te, ph, lr=5e-3, weight_decay=1e-2, lr_scheduler="linear", max_train_steps=8, accum_iter=2,
                               capture_graph=graph)
    return trainer, te, ph


def _inversion_snap(trainer, te):
    return {"table": te.get_input_embeddings().weight.detach().clone(), "grad": trainer.grad.clone(),
            "exp_avg": trainer.exp_avg.clone(), "exp_avg_sq": trainer.exp_avg_sq.clone(),
            "scalars": (trainer.global_step, trainer.optimizer_steps, trainer.scheduler_epoch, trainer.get_last_lr())}


def _assert_same_inversion(got, want, what):
    assert got["scalars"] == want["scalars"], (what, got["scalars"], want["scalars"])
    for key in ("table", "grad", "exp_avg", "exp_avg_sq"):
        assert torch.equal(got[key], want[key]), (what, key)


@pytest.mark.parametrize("graph", [False, True])
def test_inversion_saved_inside_a_window_resumes_in_a_fresh_trainer(tmp_path, golden_pti, graph, repeatable_stock_kernels):
    """accum_iter = 2: AdamW steps at micro-steps 0, 2, 4.  Saved after micro-step 1 (and, second round, after the third
    micro-step taken, g = 2): after micro-step 1 the [P, D] gradient buffer holds half a window, which the file carries."""
    t, meta = golden_pti
    cfg = json.loads(meta["cfg"])
    ph = [cfg["vocab"] - 3, cfg["vocab"] - 8]

    def feed(s):
        lat = orc.synthetic_batch(s, cfg["batch"], cfg["latent_hw"], cfg["ctx_len"], cfg["hidden"])[0]
        ids = t["ids"][s % t["ids"].shape[0]].clone()
        ids[:, 1] = ph[0]
        ids[0, 2] = ph[1]
        return dict(latents=lat.to(DEV), seed=17, input_ids=ids.to(DEV))

    straight, te_straight, _ = _inversion_trainer(t, cfg, graph)
    want_losses = _steps(straight, feed, 0, 6)
    want = _inversion_snap(straight, te_straight)
    assert not torch.equal(want["table"][ph].cpu(), t["table.init"][ph])
    for k in (2, 3):
        first, te_first, _ = _inversion_trainer(t, cfg, graph)
        _assert_losses(_steps(first, feed, 0, k), want_losses[:k], "before the save")
        path = tmp_path / f"inversion{k}.safetensors"
        first.save_checkpoint(path)
        sd = fmt.load_checkpoint_file(path)
        assert bool(sd["tensors"]["grad"].abs().max() > 0) == (k == 2)  # half a window is in the buffer after micro-step 1
        assert sd["meta"]["global_step"] == k and sd["meta"]["placeholder_token_ids"] == ph
        assert set(sd["tensors"]) == {"rows", "grad", "exp_avg", "exp_avg_sq"} and sd["tensors"]["rows"].shape == (2, cfg["hidden"])
        fresh, te_fresh, _ = _inversion_trainer(t, cfg, graph, nudge=0.05)
        fresh.load_checkpoint(path)
        _assert_same_inversion(_inversion_snap(fresh, te_fresh), _inversion_snap(first, te_first), "right after the load")
        _assert_losses(_steps(fresh, feed, k, 6), want_losses[k:], f"after the load at {k}")
        _assert_same_inversion(_inversion_snap(fresh, te_fresh), want, f"{k} + {6 - k} against 6")
        assert (fresh._graph is not None) == graph
        # other placeholder ids: refused, nothing written
        other = InversionTrainer(first.unet, te_first, [ph[0]], accum_iter=2) if k == 3 else None
        if other is not None:
            before = _inversion_snap(other, te_first)
            with pytest.raises(ValueError, match="placeholder ids"):
                other.load_checkpoint(path)
            _assert_same_inversion(_inversion_snap(other, te_first), before, "refused load")
            other.close()
        first.close()
        with pytest.raises(RuntimeError, match="after close"):
            first.save_checkpoint(tmp_path / "closed.safetensors")
        assert not os.path.exists(tmp_path / "closed.safetensors")
        fresh.close()
    straight.close()


# -- 6. rollback in a live trainer that holds a recording --------------------------------------------------------------------
def test_rollback_in_a_live_trainer_replays_its_recording(tmp_path, repeatable_stock_kernels):
    trainer, _ = _lora_trainer(lr_scheduler="linear", max_train_steps=6, capture_graph=True)
    _steps(trainer, _feed, 0, 2)
    graph = trainer._recorder.graph
    assert graph is not None
    path = tmp_path / "step2.safetensors"
    trainer.save_checkpoint(path)
    at_save = _snap(trainer)
    losses = _steps(trainer, _feed, 2, 4)
    after = _snap(trainer)
    assert trainer._recorder.graph is graph and not torch.equal(after["params"], at_save["params"])
    views = [(p.data_ptr(), p.grad.data_ptr()) for l in trainer.slab.layers for p in (l.lora_up.weight, l.lora_down.weight)]
    trainer.load_checkpoint(path)
    _assert_same(_snap(trainer), at_save, "rolled back")
    assert views == [(p.data_ptr(), p.grad.data_ptr()) for l in trainer.slab.layers for p in (l.lora_up.weight, l.lora_down.weight)]
    assert trainer._recorder.graph is graph
    _assert_losses(_steps(trainer, _feed, 2, 4), losses, "steps 3-4 once more")
    _assert_same(_snap(trainer), after, "steps 3-4 once more")
    assert trainer._recorder.graph is graph  # fp32: the scale is constant, nothing asked for a new recording


# -- 7. refusals: ValueError, and the trainer is bit for bit what it was -------------------------------------------------
@pytest.fixture(scope="module")
def rank4_file(tmp_path_factory):
    trainer, _ = _lora_trainer()
    _steps(trainer, _feed, 0, 1)
    path = tmp_path_factory.mktemp("refusals") / "rank4.safetensors"
    trainer.save_checkpoint(path)
    return path


def _edited(src, dst, edit):
    sd = fmt.load_checkpoint_file(src)
    edit(sd)
    fmt.save_checkpoint_file(dst, sd["tensors"], sd["meta"])
    return dst


def _poison(sd):
    sd["tensors"]["lora.exp_avg"][5] = float("nan")


def _newer(sd):
    sd["meta"]["format_version"] += 1


@pytest.mark.parametrize("case", ["rank4_into_rank8", "inversion_into_lora", "newer_version", "nan_in_exp_avg"])
def test_a_refused_load_raises_value_error_and_leaves_the_trainer_as_it_was(tmp_path, rank4_file, golden_pti, case):
    trainer, _ = _lora_trainer(warm_seed=12, rank=8 if case == "rank4_into_rank8" else 4, lr_scheduler="linear", max_train_steps=6)
    _steps(trainer, _feed, 0, 2)  # a state of its own: moments, counters, epoch
    path, match = rank4_file, None
    if case == "rank4_into_rank8":
        name = next(n for n, m in trainer.unet.named_modules() if m is trainer.slab.layers[0])
        match = f"layer 0.*{name}.*rank 4.*rank 8"
    elif case == "inversion_into_lora":
        t, meta = golden_pti
        inversion, _, _ = _inversion_trainer(t, json.loads(meta["cfg"]), False)
        path = tmp_path / "inversion.safetensors"
        inversion.save_checkpoint(path)
        inversion.close()
        match = "InversionTrainer"
    elif case == "newer_version":
        path, match = _edited(rank4_file, tmp_path / "newer.safetensors", _newer), "newer"
        assert fmt.load_checkpoint_file(path)["meta"]["format_version"] == stp.CHECKPOINT_VERSION + 1
    else:
        path, match = _edited(rank4_file, tmp_path / "nan.safetensors", _poison), "lora.exp_avg.*non-finite"
    before = _snap(trainer)
    with pytest.raises(ValueError, match=match):
        trainer.load_checkpoint(path)
    _assert_same(_snap(trainer), before, case)
    if case != "rank4_into_rank8":  # and the file it was derived from does load
        trainer.load_checkpoint(rank4_file)
        assert trainer.opt.step_count == 1


# -- 8. two data-parallel ranks on one GPU over gloo -------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_dp(rank, world, port, path, out):
    """Per rank, in one process group: 4 uninterrupted steps; then 2 steps, rank 0 saves, a barrier, BOTH ranks load into a
    fresh trainer and run 2 more."""
    torch.set_num_threads(2)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _deterministic_stock_kernels()
    dev = torch.device("cuda", 0)

    def trainer(warm_seed):
        unet = build_tiny_unet(seed=3).to(dev)
        params, _ = dfa.inject_trainable_lora(unet, r=4)
        _warm(list(itertools.chain(*params)), warm_seed + rank)  # ranks start different: rank 0's factors are broadcast
        return tr.LoraTrainer(unet, lr=1e-3, group_projections=False, lr_scheduler="linear", max_train_steps=4)

    def steps(tn, first, last):
        losses = []
        for s in range(first, last):
            lat, _, _, ctx = orc.synthetic_batch(s, 2 * world, 8, 6, 32)
            sl = slice(rank * 2, (rank + 1) * 2)
            losses.append(tn.step(latents=lat[sl].to(dev), seed=41, encoder_hidden_states=ctx[sl].to(dev)).item())
        return losses

    def state(tn):
        n = tn.slab.numel
        return (tn.slab.params[:n].cpu().numpy().copy(), tn.opt.exp_avg[:n].cpu().numpy().copy(),
                tn.opt.exp_avg_sq[:n].cpu().numpy().copy(), tn.opt.norm[2:4].cpu().numpy().copy(),
                (tn.opt.step_count, tn.scheduler_epoch, tn.get_last_lr(), tn.loss_scale))

    straight = trainer(11)
    assert straight.exchange.active and straight.world == 2
    straight_losses = steps(straight, 0, 4)
    first = trainer(11)
    losses = steps(first, 0, 2)
    if rank == 0:  # the caller decides which rank writes
        first.save_checkpoint(path)
    dist.barrier()
    fresh = trainer(21)
    fresh.load_checkpoint(path)  # every rank, the same file; no collective inside
    losses += steps(fresh, 2, 4)
    gathered = [None] * world
    dist.all_gather_object(gathered, (state(straight), straight_losses, state(fresh), losses))
    if rank == 0:
        out.put(gathered)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_resume_from_the_file_rank_zero_wrote(tmp_path):
    import numpy as np

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_run_dp, args=(r, 2, port, str(tmp_path / "dp.safetensors"), q)) for r in range(2)]
    for p in procs:
        p.start()
    gathered = q.get(timeout=300)
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    (straight0, straight_losses0, fresh0, losses0), (straight1, straight_losses1, fresh1, losses1) = gathered

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]

    assert same(straight0, straight1), "the replicas of the uninterrupted run differ: not the checkpoint's doing"
    assert same(fresh0, fresh1)                                          # the two ranks agree with each other
    assert same(fresh0, straight0) and same(fresh1, straight1)            # and with the uninterrupted 2-rank run
    assert losses0 == straight_losses0 and losses1 == straight_losses1    # each rank's own losses, bit for bit
    assert fresh0[4][0] == 4 and fresh0[4][1] == 4
