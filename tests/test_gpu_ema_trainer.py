"""`LoraTrainer(ema_decay=...)` on an MI355X: the average kept inside the AdamW launch, its checkpoint, and `ema_weights()`.

The tiny UNet, the feed and the repeatability fixture are tests/test_gpu_checkpoint.py's.  The shadow is compared BIT FOR BIT
with tests/ema_cases.py's fp32 emulation applied to the parameter snapshots the run itself produced, the decay from
`step.ema_decay_at` at the index `applied_steps()` gives; the parameters with a trainer without EMA at equal seed."""
import gc
import itertools
import json
import warnings

import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import formats as fmt
from diffusion_finetuning_amd import trainer as tr
from diffusion_finetuning_amd.attention import set_use_memory_efficient_attention_xformers
from oracle import lora_oracle as orc
from tests import ema_cases as ec
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


def lora(trainer):
    """The LoRA region of the slab, on the host."""
    return trainer.slab.params[: trainer.slab.numel].cpu()


def shadow(trainer):
    return trainer.opt.shadow[: trainer.slab.numel].cpu()


def run(trainer, feed, first, last):
    """Steps [first, last): (params, shadow | None, applied steps) after each."""
    out = []
    for s in range(first, last):
        _steps(trainer, feed, s, s + 1)
        out.append((lora(trainer), shadow(trainer) if trainer.opt.ema_decay is not None else None, trainer.opt.applied_steps()))
    return out


def moments(trainer):
    n = trainer.slab.numel
    return trainer.opt.exp_avg[:n].cpu(), trainer.opt.exp_avg_sq[:n].cpu(), trainer.opt.norm.cpu()


# -- 1. the trajectory ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay,after", [(0.9999, 0), (0.5, 0), (0.9999, 2)])
def test_params_as_without_ema_and_shadow_is_the_emulation_step_by_step(decay, after, repeatable_stock_kernels):
    N = 5
    plain, _ = _lora_trainer()
    want = run(plain, _feed, 0, N)
    trainer, _ = _lora_trainer(ema_decay=decay, ema_update_after_step=after)
    s = shadow(trainer)
    assert ec.same_bits(s, lora(trainer)) and trainer.opt.shadow.data_ptr() != trainer.slab.params.data_ptr()
    got = run(trainer, _feed, 0, N)
    for k in range(N):
        assert ec.same_bits(got[k][0], want[k][0]), (k, "the parameters differ from a trainer without EMA")
        assert got[k][2] == k + 1
        s = ec.ema_emulate(s, got[k][0], ec.omd_at(k + 1, decay, after))
        differ = int((ec.bits(got[k][1]) != ec.bits(s)).sum())
        assert differ == 0, (decay, after, k, "shadow elements off the emulation", differ)
    assert not ec.same_bits(got[-1][1], got[-1][0]) and not ec.same_bits(got[-1][1], got[0][1])  # an average, and it moves
    for a, b in zip(moments(trainer), moments(plain)):
        assert ec.same_bits(a, b)


# -- 2. skipped steps ------------------------------------------------------------------------------------------------------------
def test_skipped_steps_leave_the_shadow_alone_and_the_decay_follows_the_applied_count(repeatable_stock_kernels):
    """loss_scale=2**30 on the f16 tiny UNet: the first steps overflow (tests/test_gpu_checkpoint.py's recipe)."""
    N, decay = 40, 0.5
    feed = lambda s: {**_feed(s), "seed": 7}  # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the trainer reports the first skipped step)
        trainer, _ = _lora_trainer(dtype=torch.float16, loss_scale=2.0 ** 30, ema_decay=decay)
        s = shadow(trainer)
        p = lora(trainer)
        applied, skipped_seen, applied_seen = 0, 0, 0
        for k, (p_k, s_k, t_k) in enumerate(run(trainer, feed, 0, N)):
            if t_k == applied:  # skipped: neither the parameters nor the shadow moved
                skipped_seen += 1
                assert ec.same_bits(p_k, p) and ec.same_bits(s_k, s), (k, "a skipped step wrote")
            else:
                assert t_k == applied + 1
                applied, applied_seen = t_k, applied_seen + 1
                s = ec.ema_emulate(s, p_k, ec.omd_at(t_k, decay, 0))
                assert ec.same_bits(s_k, s), (k, t_k, int((ec.bits(s_k) != ec.bits(s)).sum()))
            p = p_k
    print(f"\n[ema under overflow] {skipped_seen} skipped, {applied_seen} applied of {N}")
    assert skipped_seen >= 3 and applied_seen >= 3 and trainer.opt.skipped_steps() == skipped_seen


# -- 3. accumulation, recorded against host-launched -----------------------------------------------------------------------------
def test_one_shadow_update_per_accumulation_window(repeatable_stock_kernels):
    decay = 0.5
    trainer, _ = _lora_trainer(gradient_accumulation_steps=2, ema_decay=decay)
    s = shadow(trainer)
    for k, (p_k, s_k, t_k) in enumerate(run(trainer, _feed, 0, 6)):
        if k % 2 == 0:  # inside a window: nothing moved
            assert t_k == k // 2 and ec.same_bits(s_k, s)
        else:
            assert t_k == k // 2 + 1
            s = ec.ema_emulate(s, p_k, ec.omd_at(t_k, decay, 0))
            assert ec.same_bits(s_k, s), (k, t_k)
    assert trainer.opt.applied_steps() == 3


def test_recorded_and_host_launched_runs_end_with_the_same_shadow(repeatable_stock_kernels):
    ends = []
    for graph in (False, True):
        trainer, _ = _lora_trainer(ema_decay=0.5, capture_graph=graph)
        ends.append(run(trainer, _feed, 0, 4)[-1])
        assert (trainer._graph is not None) == graph
    assert ec.same_bits(ends[0][0], ends[1][0]) and ec.same_bits(ends[0][1], ends[1][1])


# -- 4. checkpoint ----------------------------------------------------------------------------------------------------------------
def test_save_and_load_mid_run_leave_the_bits_of_the_uninterrupted_run(tmp_path, repeatable_stock_kernels):
    kw = dict(ema_decay=0.9999, ema_update_after_step=1)
    straight, _ = _lora_trainer(**kw)
    want = run(straight, _feed, 0, 6)
    first, _ = _lora_trainer(**kw)
    run(first, _feed, 0, 3)
    path = tmp_path / "ema.safetensors"
    first.save_checkpoint(path)
    sd = fmt.load_checkpoint_file(path)
    assert ec.same_bits(sd["tensors"]["lora.ema"], want[2][1]) and sd["tensors"]["lora.ema"].shape == (first.slab.numel,)
    assert sd["meta"]["config"]["ema_decay"] == 0.9999 and sd["meta"]["config"]["ema_update_after_step"] == 1
    assert sd["meta"]["format_version"] == 1
    fresh, _ = _lora_trainer(warm_seed=12, **kw)
    address = fresh.opt.shadow.data_ptr()
    fresh.load_checkpoint(path)
    assert fresh.opt.shadow.data_ptr() == address and ec.same_bits(shadow(fresh), want[2][1])
    got = run(fresh, _feed, 3, 6)
    for k in range(3):
        assert ec.same_bits(got[k][0], want[3 + k][0]) and ec.same_bits(got[k][1], want[3 + k][1]), k
    for a, b in zip(moments(fresh), moments(straight)):
        assert ec.same_bits(a, b)


def test_a_save_inside_the_overflow_phase_continues_exactly(tmp_path, repeatable_stock_kernels):
    N, K = 40, 2  # (the first steps under loss_scale 2**30 overflow: step 2 is inside that phase)
    feed = lambda s: {**_feed(s), "seed": 7}  # noqa: E731
    kw = dict(dtype=torch.float16, loss_scale=2.0 ** 30, ema_decay=0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        straight, _ = _lora_trainer(**kw)
        want = run(straight, feed, 0, N)
        assert want[K - 1][2] == 0 and straight.opt.applied_steps() >= 3, "the save was not inside the overflow phase"
        first, _ = _lora_trainer(**kw)
        run(first, feed, 0, K)
        first.save_checkpoint(tmp_path / "overflow.safetensors")
        fresh, _ = _lora_trainer(warm_seed=12, **kw)
        fresh.load_checkpoint(tmp_path / "overflow.safetensors")
        got = run(fresh, feed, K, N)
    assert [g[2] for g in got] == [w[2] for w in want[K:]]
    assert ec.same_bits(got[-1][0], want[-1][0]) and ec.same_bits(got[-1][1], want[-1][1])
    for a, b in zip(moments(fresh), moments(straight)):
        assert ec.same_bits(a, b)


def _everything(trainer):
    out = [lora(trainer), *moments(trainer)]
    if trainer.opt.ema_decay is not None:
        out.append(shadow(trainer))
    return out, (trainer.opt.step_count, trainer.scheduler_epoch, trainer._micro)


def test_files_with_and_without_the_average_are_refused_by_the_other_kind(tmp_path):
    with_ema, _ = _lora_trainer(ema_decay=0.5)
    without, _ = _lora_trainer()
    run(with_ema, _feed, 0, 2)
    run(without, _feed, 0, 2)
    with_ema.save_checkpoint(tmp_path / "with.safetensors")
    without.save_checkpoint(tmp_path / "without.safetensors")
    assert "lora.ema" not in fmt.load_checkpoint_file(tmp_path / "without.safetensors")["tensors"]
    for target, path, word in ((_lora_trainer(warm_seed=12, ema_decay=0.5)[0], "without.safetensors", "missing"),
                               (_lora_trainer(warm_seed=12)[0], "with.safetensors", "not part of")):
        before, host = _everything(target)
        with pytest.raises(ValueError, match="'lora.ema'") as e:
            target.load_checkpoint(tmp_path / path)
        assert word in str(e.value)
        after, host_after = _everything(target)
        assert host_after == host and all(ec.same_bits(a, b) for a, b in zip(after, before)), "a refused load wrote"


# -- 5. ema_weights() ------------------------------------------------------------------------------------------------------------
def _conditioning(B=2, seed=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 6, 32, generator=g).to(DEV), torch.randn(B, 6, 32, generator=g).to(DEV)


def _model_with_factors(flat, dtype):
    """A separately injected copy of the tiny UNet whose LoRA factors are `flat` ([up0, down0, up1, …], the slab's order)."""
    unet = build_tiny_unet(seed=5).to(DEV).to(dtype)
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    off = 0
    with torch.no_grad():
        for layer in tr.lora_layers(unet):
            for w in (layer.lora_up.weight, layer.lora_down.weight):
                w.copy_(flat[off:off + w.numel()].view(w.shape).to(DEV))
                off += w.numel()
    assert off == flat.numel()
    return unet


def test_inside_the_block_everything_reads_the_average_and_afterwards_the_run_goes_on_exactly(tmp_path):
    """f16 and 4 rows (2 samples under guidance): the tiny UNet's forward and the recorded step are run-to-run deterministic
    there (tests/test_gpu_sampling.py)."""
    dtype, kw = torch.float16, dict(dtype=torch.float16, ema_decay=0.5, capture_graph=True)
    feed = lambda s: {k: (torch.cat([v, v + 0.25]) if torch.is_tensor(v) else v) for k, v in _feed(s).items()}  # noqa: E731
    straight, _ = _lora_trainer(**kw)
    want = run(straight, feed, 0, 6)
    trainer, unet = _lora_trainer(**kw)
    run(trainer, feed, 0, 3)
    live, avg = lora(trainer), shadow(trainer)
    assert not ec.same_bits(live, avg)
    cond, neg = _conditioning()
    sampler = dfa.LatentSampler(unet, num_inference_steps=4)
    live_sample = sampler.sample(cond, neg, seed=5, latent_shape=(4, 8, 8)).cpu()
    recording = sampler._recorder.graph
    assert recording is not None
    packed_live = trainer.slab.packed.clone()
    addresses = (trainer.slab.params.data_ptr(), trainer.opt.shadow.data_ptr(), trainer.slab.packed.data_ptr(),
                 [p.data_ptr() for l in trainer.slab.layers for p in (l.lora_up.weight, l.lora_down.weight)])
    with trainer.ema_weights() as inside:
        assert inside is trainer
        # the Parameters and the packed factors hold the shadow's values; the shadow buffer holds the live ones
        assert ec.same_bits(tr.flat_lora_state(unet).cpu(), avg) and ec.same_bits(lora(trainer), avg)
        assert ec.same_bits(shadow(trainer), live)
        assert not torch.equal(trainer.slab.packed, packed_live)
        other = tr.LoraTrainer(_model_with_factors(avg, dtype), lr=1e-3)  # (its slab packs the same factors)
        assert torch.equal(other.slab.packed, trainer.slab.packed)
        ema_sample = sampler.sample(cond, neg, seed=5, latent_shape=(4, 8, 8)).cpu()
        assert sampler._recorder.graph is recording, "the sampler recorded again"
        copy = _model_with_factors(avg, dtype)
        copy_sample = dfa.LatentSampler(copy, num_inference_steps=4).sample(cond, neg, seed=5, latent_shape=(4, 8, 8)).cpu()
        assert torch.equal(ema_sample, copy_sample), float((ema_sample - copy_sample).abs().max())
        assert not torch.equal(ema_sample, live_sample)
        dfa.save_lora_weight(unet, str(tmp_path / "ema.pt"))
        with pytest.raises(RuntimeError, match="ema_weights"):
            trainer.step(**feed(3))
        with pytest.raises(RuntimeError, match="ema_weights"):
            trainer.state_dict()
        with pytest.raises(RuntimeError, match="ema_weights"):
            trainer.load_state_dict({})
        with pytest.raises(RuntimeError, match="ema_weights"):
            with trainer.ema_weights():
                pass
        assert ec.same_bits(lora(trainer), avg)  # (the refused calls changed nothing: still inside)
    saved = torch.cat([t.reshape(-1) for t in torch.load(str(tmp_path / "ema.pt"), weights_only=True)])
    assert saved.dtype == torch.float16 and torch.equal(saved, avg.to(torch.float16))
    assert not torch.equal(saved, live.to(torch.float16))
    after = (trainer.slab.params.data_ptr(), trainer.opt.shadow.data_ptr(), trainer.slab.packed.data_ptr(),
             [p.data_ptr() for l in trainer.slab.layers for p in (l.lora_up.weight, l.lora_down.weight)])
    assert after == addresses
    assert ec.same_bits(lora(trainer), live) and ec.same_bits(shadow(trainer), avg) and torch.equal(trainer.slab.packed, packed_live)
    assert torch.equal(sampler.sample(cond, neg, seed=5, latent_shape=(4, 8, 8)).cpu(), live_sample)
    assert sampler._recorder.graph is recording
    # an exception raised inside the block leaves the live bits restored as well
    with pytest.raises(KeyError, match="from inside"):
        with trainer.ema_weights():
            assert ec.same_bits(lora(trainer), avg)
            raise KeyError("from inside")
    assert ec.same_bits(lora(trainer), live) and ec.same_bits(shadow(trainer), avg) and torch.equal(trainer.slab.packed, packed_live)
    trainer.state_dict()  # (allowed again)
    graph = trainer._graph.graph
    got = run(trainer, feed, 3, 6)
    assert trainer._graph.graph is graph, "the trainer recorded again"
    for k in range(3):
        assert ec.same_bits(got[k][0], want[3 + k][0]) and ec.same_bits(got[k][1], want[3 + k][1]), k


def test_entering_inside_an_accumulation_window_or_without_ema_raises():
    trainer, _ = _lora_trainer(gradient_accumulation_steps=2, ema_decay=0.5)
    run(trainer, _feed, 0, 1)
    before = lora(trainer)
    with pytest.raises(RuntimeError, match="accumulation window"):
        with trainer.ema_weights():
            pass
    assert ec.same_bits(lora(trainer), before) and not trainer._ema_active
    plain, _ = _lora_trainer()
    with pytest.raises(RuntimeError, match="ema_decay"):
        with plain.ema_weights():
            pass


def test_bad_arguments_raise_at_construction():
    for kw in (dict(ema_decay=0.0), dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=0.5, ema_update_after_step=-1)):
        with pytest.raises(ValueError, match="ema_"):
            _lora_trainer(**kw)


# -- 6. a trainable token table is not averaged -------------------------------------------------------------------------------
def _pti_ema_trainer(t, cfg):
    """tests/test_gpu_checkpoint.py's `_pti_trainer` (UNet and text-encoder LoRA, a trainable token table) with an average."""
    from tests.test_oracle_golden import build_pti_models

    unet, te = build_pti_models(t, cfg, DEV, torch.float32)
    orc.freeze_all_but_token_embeddings(te)
    gu, _ = dfa.inject_trainable_lora(unet, r=4)
    gt, _ = dfa.inject_trainable_lora(te, dfa.TEXT_ENCODER_DEFAULT_TARGET_REPLACE, r=4)
    _warm(list(itertools.chain(*gu)) + list(itertools.chain(*gt)), 11)
    set_use_memory_efficient_attention_xformers(unet, True)
    trainer = tr.LoraTrainer(unet, te, lr=1e-3, lr_text=3e-4, lr_embed=5e-3, v_prediction=True, ema_decay=0.5)
    assert trainer.token_table is not None and len(trainer.slab.models) == 2 and len(trainer.opt.groups) == 3
    return trainer


def test_a_token_table_keeps_its_live_values_inside_the_block(golden_pti):
    t, meta = golden_pti
    cfg = json.loads(meta["cfg"])
    trainer = _pti_ema_trainer(t, cfg)
    _steps(trainer, _pti_feed(t, cfg), 0, 3)
    tt = trainer.token_table
    a, b = tt.range
    table = trainer.slab.params[a:b].clone()
    emb = trainer.text_encoder.get_input_embeddings().weight
    assert trainer.opt.shadow.numel() == trainer.slab.stride < trainer.slab.total  # the average covers the LoRA region only
    assert "lora.ema" in trainer.state_dict()["tensors"]
    live, avg = lora(trainer), shadow(trainer)
    with trainer.ema_weights():
        assert ec.same_bits(lora(trainer), avg)  # both models' LoRA factors are averaged
        assert torch.equal(trainer.slab.params[a:b], table) and torch.equal(emb.detach().reshape(-1), table)
    assert torch.equal(trainer.slab.params[a:b], table) and ec.same_bits(lora(trainer), live)


# -- 7. off ------------------------------------------------------------------------------------------------------------------------
def test_without_ema_decay_there_is_no_buffer_and_no_tensor():
    trainer, _ = _lora_trainer()
    run(trainer, _feed, 0, 1)
    assert not hasattr(trainer.opt, "shadow") and trainer.opt.ema_decay is None
    sd = trainer.state_dict()
    assert "lora.ema" not in sd["tensors"] and sd["meta"]["config"]["ema_decay"] is None
    assert sorted(sd["tensors"]) == ["lora.exp_avg", "lora.exp_avg_sq", "lora.params", "opt.norm"]
