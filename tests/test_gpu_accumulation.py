"""LoraTrainer(gradient_accumulation_steps=n) — train_lora_dreambooth.py:310,490,878-893: n micro-batches summed into the slab,
one exchange / clip + AdamW / scheduler step per window — against plain steps on the concatenated batches, against a CPU loop of
the oracle's modules with torch.optim.AdamW, host-launched and recorded, under two data-parallel ranks and under fp16 overflow."""
import itertools
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import trainer as tr
from oracle import lora_oracle as orc
from tests.conftest import build_tiny_unet

pytestmark = pytest.mark.gpu
DEV = "cuda"
WINDOWS, N, ROWS = 3, 2, 2  # three windows of two micro-batches of two rows


@pytest.fixture(autouse=True)
def _collect_garbage_first():
    """A recording left in a reference cycle by an earlier test must not be destroyed in the middle of another capture."""
    import gc

    gc.collect()


def _warm(params, seed, std):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i, p in enumerate(params):
            if i % 2 == 0:
                p.copy_(torch.randn(p.shape, generator=g).to(p.device) * std)


def _trainer(dtype=torch.float32, **kw):
    unet = build_tiny_unet(seed=5).to(DEV).to(dtype)
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    _warm(list(itertools.chain(*params)), 11, 0.02)
    return tr.LoraTrainer(unet, lr=1e-3, **kw), unet


def _window(w, device=DEV):
    """The 4-row batch of window `w`; micro-batch k is its rows [2k, 2k + 2)."""
    return tuple(x.to(device) for x in orc.synthetic_batch(w, N * ROWS, 8, 6, 32))


def _run_accumulated(graph=False, counts=None):
    trainer, unet = _trainer(gradient_accumulation_steps=N, capture_graph=graph)
    zeroed = []
    zero = trainer.slab.zero_grad
    trainer.slab.zero_grad = lambda: (zeroed.append(trainer._micro), zero())[1]
    losses = []
    for w in range(WINDOWS):
        lat, noise, ts, ctx = _window(w)
        for k in range(N):
            sl = slice(k * ROWS, (k + 1) * ROWS)
            zeroed_before = len(zeroed)
            losses.append(trainer.step(lat[sl], noise[sl], ts[sl], ctx[sl]))
            assert trainer.opt.step_count == w + (k == N - 1)  # one optimizer step per window, at its last micro-batch
            if k == 0:
                assert trainer._micro == 1 and float(trainer.slab.grads.abs().max()) > 0.0
                first = trainer.slab.grads.clone()
            elif w > 0 or not graph:  # (recording a window's step zeroes once more, after the warm-up passes: `undo`)
                assert len(zeroed) == zeroed_before  # the slab is not zeroed between the micro-batches of a window
        assert trainer._micro == 0 and not torch.equal(trainer.slab.grads, first)  # the second micro-batch was added on top
    if counts is not None:
        counts.append((trainer.opt.step_count, trainer.opt.applied_steps(), trainer.scheduler_epoch))
    assert (trainer._graph is not None) == graph
    return tr.flat_lora_state(unet).clone(), torch.stack(losses).reshape(-1).cpu()


@pytest.fixture(scope="module")
def accumulated():
    counts = []
    state, losses = _run_accumulated(counts=counts)
    assert counts == [(WINDOWS, WINDOWS, WINDOWS)]
    return state, losses


def test_windows_of_two_micro_batches_equal_plain_steps_on_the_concatenated_batches(accumulated, relerr):
    state, losses = accumulated
    trainer, unet = _trainer()
    plain = [trainer.step(*_window(w)) for w in range(WINDOWS)]
    err = relerr(state, tr.flat_lora_state(unet))
    # the loss of a 4-row batch is the mean of its two micro-batches' (undivided) losses
    loss_err = relerr(losses.reshape(WINDOWS, N).mean(dim=1), torch.stack(plain).reshape(-1))
    print(f"\n[accumulation vs plain 4-row steps] state {err:.3g} losses {loss_err:.3g}")
    assert err < 1e-3 and loss_err < 1e-3


def test_windows_equal_a_cpu_loop_stepping_adamw_every_second_backward(accumulated, relerr):
    """accelerate's loop written out: loss / n, backward, and at every n-th micro-batch clip_grad_norm_ + AdamW.step +
    zero_grad (train_lora_dreambooth.py:877-893) over the oracle's injected modules, fp32 on the CPU."""
    state, losses = accumulated
    ref = build_tiny_unet(seed=5)
    params, _ = orc.inject(ref, r=4)
    _warm(params, 11, 0.02)
    opt = torch.optim.AdamW(params, lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    acp = orc.ddpm_alphas_cumprod()
    ref_losses = []
    for w in range(WINDOWS):
        lat, noise, ts, ctx = _window(w, "cpu")
        for k in range(N):
            sl = slice(k * ROWS, (k + 1) * ROWS)
            loss = orc.mse_loss(ref(orc.add_noise(lat[sl], noise[sl], ts[sl], acp), ts[sl], ctx[sl]).sample, noise[sl])
            ref_losses.append(loss.item())
            (loss / N).backward()
            if k == N - 1:
                torch.nn.utils.clip_grad_norm_(params, 1.0)
                opt.step()
                opt.zero_grad()
    err, loss_err = relerr(state, orc.flat_params(params)), relerr(losses, torch.tensor(ref_losses))
    print(f"\n[accumulation vs CPU AdamW loop] state {err:.3g} losses {loss_err:.3g}")
    assert err < 1e-3 and loss_err < 1e-3


def test_recorded_windows_equal_host_launched_ones(accumulated, relerr):
    """One recording serves every micro-batch of every window.  Bit for bit whenever two host-launched runs coincide (the stock
    torch kernels of the UNet are then run-to-run deterministic), within 1e-6 always."""
    state, losses = accumulated
    again, losses_again = _run_accumulated()
    recorded, losses_rec = _run_accumulated(graph=True)
    repeats = torch.equal(state, again) and torch.equal(losses, losses_again)
    print(f"\n[accumulation recorded] host-launched run-to-run bit-identical: {repeats}; recorded vs host-launched state "
          f"{relerr(recorded, state):.3g} losses {relerr(losses_rec, losses):.3g}")
    assert relerr(recorded, state) < 1e-6 and relerr(losses_rec, losses) < 1e-6
    if repeats:
        assert torch.equal(recorded, state) and torch.equal(losses_rec, losses)


@pytest.mark.parametrize("graph", [False, True])
def test_device_draw_differs_between_the_micro_batches_of_a_window(monkeypatch, graph):
    seen = []
    real = nat.ddpm_noise_prologue

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((a[5], out[0].clone(), out[2].clone()))
        return out

    monkeypatch.setattr(nat, "ddpm_noise_prologue", spy)
    trainer, _ = _trainer(gradient_accumulation_steps=N, capture_graph=graph)
    lat, _, _, ctx = _window(0)
    for _ in range(2 * N):  # the same latents every time: only the key tells the draws apart
        trainer.step(lat[:ROWS], None, None, ctx[:ROWS], seed=9)
    assert [k for k, _, _ in seen] == [0, 1, 2, 3]  # optimizer step · n + micro-batch
    for (_, noisy_a, _), (_, noisy_b, _) in itertools.combinations(seen, 2):
        assert not torch.equal(noisy_a, noisy_b)
    sa, sb = tr.ddpm_tables(device=DEV)
    for k, noisy, t in seen:
        want = real(lat[:ROWS], sa, sb, torch.float32, 9, k, False)
        assert torch.equal(noisy, want[0]) and torch.equal(t, want[2])


def test_an_inf_in_one_micro_batch_skips_the_window_in_fp16():
    trainer, unet = _trainer(torch.float16, gradient_accumulation_steps=N, loss_scale=256.0)
    for w in range(2):
        lat, noise, ts, ctx = _window(w)
        if w == 1:
            lat = lat.clone()
            lat[0, 0, 0, 0] = float("inf")  # in the window's FIRST micro-batch: the sum carries it to the window's one norm
            before = tr.flat_lora_state(unet).clone()
        for k in range(N):
            sl = slice(k * ROWS, (k + 1) * ROWS)
            trainer.step(lat[sl], noise[sl], ts[sl], ctx[sl])
    assert trainer.opt.step_count == 2 and trainer.opt.applied_steps() == 1 and trainer.opt.skipped_steps() == 1
    assert torch.equal(tr.flat_lora_state(unet), before) and torch.isfinite(before).all()


def _rank(rank, world, port, out):
    torch.set_num_threads(2)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    reduces = []
    real = dist.all_reduce
    tr.dist.all_reduce = lambda *a, **kw: (reduces.append(1), real(*a, **kw))[1]
    trainer, unet = _trainer(gradient_accumulation_steps=N)
    assert trainer.exchange.active
    per_exchange = 1 if trainer.exchange.early_range is None else 2  # (an early [up|mid] bucket goes ahead of the rest)
    after = []
    for w in range(WINDOWS):
        lat, noise, ts, ctx = _window(w)
        for k in range(N):  # rank r takes row r of every micro-batch
            i = k * ROWS + rank
            trainer.step(lat[i:i + 1], noise[i:i + 1], ts[i:i + 1], ctx[i:i + 1])
            after.append(len(reduces))
    state = trainer.slab.params[: trainer.slab.numel].cpu()
    gathered = [torch.zeros_like(state) for _ in range(world)]
    dist.all_gather(gathered, state)
    assert all(torch.equal(gathered[0], g_) for g_ in gathered)
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        out.put((state.numpy().copy(), after, per_exchange))


def test_two_ranks_exchange_once_per_window(accumulated):
    from tests.test_gpu_dp import _free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    state, after, per_exchange = q.get(timeout=300)
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    # nothing crosses the ranks inside a window; its last micro-batch exchanges the slab once
    assert after == [per_exchange * (i // N) for i in range(1, WINDOWS * N + 1)], (after, per_exchange)
    # 2 ranks × 2 micro-batches × 1 row see the rows of the single-process windows (2 micro-batches × 2 rows)
    one = accumulated[0].cpu()
    err = ((torch.from_numpy(state) - one).norm() / one.norm()).item()
    assert err < 1e-4, err
