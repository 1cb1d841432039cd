"""BASELINE config 5's first half — train_inversion of cli_lora_pti.py (:290-346): the placeholder rows of the token table
train alone, UNet and the rest of the encoder frozen, AdamW + clip_ti_decay + restore of every other row.  The two C entries
against float64 / torch.optim.AdamW on the full table; InversionTrainer's trajectory against a CPU fp32 restatement of the
loop (tests/inversion_reference.py); the recorded micro-step against the host-launched one; the hand-over to LoraTrainer; one
accumulation window at full size against the stock-torch loop on the same GPU."""
import itertools
import json

import pytest
import torch
import torch.nn.functional as F

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import trainer as tr
from diffusion_finetuning_amd.inversion import InversionTrainer
from oracle import lora_oracle as orc
from tests.inversion_reference import config5_batches, config5_models, reference_inversion
from tests.test_oracle_golden import build_pti_models

pytestmark = pytest.mark.gpu
DEV = "cuda"
# learned rows, their update and the loss history against the fp32 restatement: 2x the worst measured on an MI355X over the
# tiny and the full-size cases over two runs (rows 3.5e-7, update 6.8e-7, losses 1.3e-7), far under the project's 1e-3 bar
ROWS_TOL, MOVE_TOL, LOSS_TOL = 7e-7, 1.36e-6, 2.6e-7


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_ti_rows_grad_sums_the_placeholder_rows_in_a_fixed_order(dtype):
    """grad[s] = Σ dE[p] over the positions of slot s's token — float64 index_add restricted to the placeholder ids; zero for
    an absent placeholder; accumulate adds on top; a second run is bit-identical."""
    g = torch.Generator().manual_seed(5)
    V, D, n = 300, 1000, 3 * 77  # D not a multiple of the 256-column chunk
    ids = torch.randint(0, V, (n,), generator=g)
    ids[10:20] = 17     # a placeholder in ten positions
    ids[100] = 250      # and one in a single position
    ids[ids == 33] = 34  # 33: a placeholder that does not occur
    slots = torch.tensor([250, 33, 17])
    dE = torch.randn(n, D, generator=g).to(dtype)
    full = torch.zeros(V, D, dtype=torch.float64).index_add_(0, ids, dE.double())
    want = full[slots]
    grad = torch.full((3, D), 7.0, device=DEV)
    nat.ti_rows_grad(dE.to(DEV), ids.to(DEV), slots.to(DEV), grad, accumulate=False)
    got = grad.double().cpu()
    assert (got - want).abs().max() <= 1e-5 * want.abs().max()
    assert torch.equal(grad[1], torch.zeros(D, device=DEV))  # absent placeholder: written as zero
    again = torch.full((3, D), -1.0, device=DEV)
    nat.ti_rows_grad(dE.to(DEV), ids.to(DEV), slots.to(DEV), again, accumulate=False)
    assert torch.equal(again, grad)
    nat.ti_rows_grad(dE.to(DEV), ids.to(DEV), slots.to(DEV), again, accumulate=True)
    assert (again.double().cpu() - 2 * want).abs().max() <= 2e-5 * want.abs().max()


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
@pytest.mark.parametrize("lr,decay", [(3e-3, False), (3e-3, True), (2e-2, True)])  # λd = 0.3 and λd = 1
def test_ti_rows_adamw_decay_matches_full_table_adamw_decay_and_restore(weight_decay, lr, decay):
    """Four optimizer steps: the kernel on the P placeholder rows against torch.optim.AdamW over the FULL table on the CPU,
    then the reference's clip_ti_decay and restore (:311-346) written out — the placeholder rows within 2e-6, every other row
    torch.equal to the initial table."""
    g = torch.Generator().manual_seed(9)
    V, D = 400, 1024
    slots = [301, 7, 55]
    init = torch.randn(V, D, generator=g) * 0.05
    ref = torch.nn.Parameter(init.clone())
    opt = torch.optim.AdamW([ref], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    upd = torch.zeros(V, dtype=torch.bool)
    upd[slots] = True
    table = init.clone().to(DEV)
    slot_ids = torch.tensor(slots, device=DEV)
    m, v = torch.zeros(3, D, device=DEV), torch.zeros(3, D, device=DEV)
    lam = min(1.0, 100 * lr)
    for step in range(1, 5):
        dense = torch.randn(V, D, generator=g) * 1e-2  # every row has a gradient: the restore is what keeps them still
        ref.grad = dense.clone()
        opt.step()
        with torch.no_grad():
            if decay:
                pre = ref[upd, :].norm(dim=-1, keepdim=True)
                ref[upd] = F.normalize(ref[upd, :], dim=-1) * (pre + lam * (0.4 - pre))
            ref[~upd] = init[~upd]
        nat.ti_rows_adamw_decay(table, slot_ids, dense[slots].to(DEV), m, v, 1.0, lr, 0.9, 0.999, 1e-8, weight_decay, step,
                                lam if decay else -1.0)
        got = table.cpu()
        err = (got[slots] - ref.detach()[slots]).abs().max().item()
        assert err <= 2e-6 * ref.detach()[slots].abs().max().item(), (step, err)
        assert torch.equal(got[~upd], init[~upd])
        if decay and lam == 1.0:  # λd = 1: every placeholder row is put at norm 0.4
            assert torch.allclose(got[slots].norm(dim=-1), torch.full((3,), 0.4), rtol=1e-6)


def _placeholder_ids(cfg):
    return [cfg["vocab"] - 3, cfg["vocab"] - 8]


def _tiny_batches(t, cfg, n, device, mask):
    ph = _placeholder_ids(cfg)
    out = []
    for s in range(n):
        lat, noise, ts, _ = orc.synthetic_batch(s, cfg["batch"], cfg["latent_hw"], cfg["ctx_len"], cfg["hidden"], t_max=1000)
        ids = t["ids"][s % t["ids"].shape[0]].clone()
        ids[:, 1] = ph[0]
        if s % 3 != 2:  # the second placeholder is absent from every third micro-batch
            ids[0, 2] = ids[1, 3] = ph[1]
        mk = None
        if mask:
            gm = torch.Generator().manual_seed(500 + s)
            hw = cfg["latent_hw"] * 8
            mk = (torch.rand(cfg["batch"], 1, hw, hw, generator=gm) > 0.6).float()
        out.append((lat.to(device), noise.to(device), ts.to(device), ids.to(device), None if mk is None else mk.to(device)))
    return out


SCHED = dict(name="linear", warmup=0, total=16)
TINY_LR, ACCUM, MICRO = 5e-3, 4, 13


def _tiny_run(t, cfg, v_prediction, mask, graph=False, seed=None):
    unet, te = build_pti_models(t, cfg, DEV, torch.float32)
    orc.freeze_all_but_token_embeddings(te)
    trainer = InversionTrainer(unet, te, _placeholder_ids(cfg), lr=TINY_LR, weight_decay=1e-2, lr_scheduler=SCHED["name"],
                               lr_warmup_steps=SCHED["warmup"], max_train_steps=SCHED["total"], accum_iter=ACCUM,
                               v_prediction=v_prediction, capture_graph=graph)
    losses = []
    for lat, noise, ts, ids, mk in _tiny_batches(t, cfg, MICRO, DEV, mask):
        if seed is None:
            losses.append(trainer.step(lat, noise, ts, input_ids=ids, mask=mk))
        else:
            losses.append(trainer.step(lat, input_ids=ids, mask=mk, seed=seed))
    return trainer, unet, te, torch.stack(losses).reshape(-1).cpu()


@pytest.mark.parametrize("v_prediction", [False, True])
@pytest.mark.parametrize("mask", [False, True])
def test_inversion_trajectory_matches_the_reference_loop(golden_pti, relerr, v_prediction, mask):
    """13 micro-steps, accum_iter 4 (optimizer steps at 0, 4, 8, 12), linear schedule, clip_ti_decay on, weight decay 1e-2:
    learned rows and loss history against the CPU fp32 restatement of :290-346 (full-table AdamW + restore); every other
    row bit-identical to the initial table."""
    t, meta = golden_pti
    cfg = json.loads(meta["cfg"])
    ph = _placeholder_ids(cfg)
    trainer, unet, te, losses = _tiny_run(t, cfg, v_prediction, mask)
    assert trainer.global_step == MICRO and trainer.optimizer_steps == 4
    lam = tr.lr_lambda(SCHED["name"], SCHED["warmup"], SCHED["total"], lr_init=TINY_LR)
    assert trainer.get_last_lr() == [TINY_LR * lam(MICRO)]
    table = te.get_input_embeddings().weight.detach().cpu()

    cu, cte = build_pti_models(t, cfg, "cpu", torch.float32)
    orc.freeze_all_but_token_embeddings(cte)
    acp, s1 = tr.ddpm_tables()
    cpu_batches = [tuple(None if x is None else x.cpu() for x in b) for b in _tiny_batches(t, cfg, MICRO, DEV, mask)]
    ref_losses, lrs = reference_inversion(cu, cte, ph, cpu_batches, TINY_LR, 1e-2, ACCUM, lam, True, v_prediction, acp, s1)
    assert lrs == [TINY_LR * lam(g + 1) for g in range(MICRO)]
    ref = cte.get_input_embeddings().weight.detach()
    init = t["table.init"]
    rows_err, loss_err = relerr(table[ph], ref[ph]), relerr(losses, ref_losses)
    move_err = relerr(table[ph] - init[ph], ref[ph] - init[ph])
    print(f"\n[inversion tiny v={v_prediction} mask={mask}] rows {rows_err:.3g} update {move_err:.3g} losses {loss_err:.3g}")
    assert rows_err < ROWS_TOL and loss_err < LOSS_TOL and move_err < MOVE_TOL
    assert (table[ph] - init[ph]).abs().max() > 1e-3  # the rows did move
    others = torch.ones(cfg["vocab"], dtype=torch.bool)
    others[ph] = False
    assert torch.equal(table[others], init[others])
    assert te.get_input_embeddings().weight.grad is None  # no dense table gradient was ever formed


@pytest.mark.parametrize("seed", [None, 1234])
def test_recorded_micro_step_matches_the_host_launched_one(golden_pti, relerr, seed):
    """capture_graph: forward, backward and ti_rows_grad replayed from one recording (the optimizer launch and the zeroing of
    the buffer outside it).  The recorded trajectory equals the host-launched one bit for bit whenever two host-launched runs do
    (the stock torch UNet / encoder kernels are then run-to-run deterministic), and within 1e-6 always; with a seed the device
    draw is keyed by the micro-step."""
    t, meta = golden_pti
    cfg = json.loads(meta["cfg"])
    _, _, te_e, loss_e = _tiny_run(t, cfg, True, True, graph=False, seed=seed)
    _, _, te_e2, loss_e2 = _tiny_run(t, cfg, True, True, graph=False, seed=seed)
    tr_g, _, te_g, loss_g = _tiny_run(t, cfg, True, True, graph=True, seed=seed)
    assert tr_g._graph is not None and tr_g.capture_graph
    w_e, w_e2, w_g = (te.get_input_embeddings().weight.detach() for te in (te_e, te_e2, te_g))
    eager_repeats = torch.equal(loss_e, loss_e2) and torch.equal(w_e, w_e2)
    print(f"\n[inversion recorded seed={seed}] eager run-to-run bit-identical: {eager_repeats}; recorded vs eager losses "
          f"{relerr(loss_g, loss_e):.3g} table {relerr(w_g, w_e):.3g}, bit-identical: {torch.equal(loss_g, loss_e) and torch.equal(w_g, w_e)}")
    assert relerr(loss_g, loss_e) < 1e-6 and relerr(w_g, w_e) < 1e-6
    if eager_repeats:
        assert torch.equal(loss_g, loss_e) and torch.equal(w_g, w_e)
    if seed is not None:  # two micro-steps on the same batch with a table that cannot move (lr 0, no decay): different draws
        unet, te = build_pti_models(t, cfg, DEV, torch.float32)
        orc.freeze_all_but_token_embeddings(te)
        still = InversionTrainer(unet, te, _placeholder_ids(cfg), lr=0.0, lr_scheduler="constant", clip_ti_decay=False)
        lat, _, _, ids, _ = _tiny_batches(t, cfg, 1, DEV, False)[0]
        a, b = still.step(lat, input_ids=ids, seed=seed), still.step(lat, input_ids=ids, seed=seed)
        assert not torch.equal(a, b)


def test_handover_to_the_tuning_phase(golden_pti, tmp_path):
    """close() gives the embedding its own forward back; save_all(save_lora=False) writes the learned rows (:687-690);
    LoraTrainer with continue_inversion starts from them and runs a step (perform_tuning, :693-753)."""
    t, meta = golden_pti
    cfg = json.loads(meta["cfg"])
    ph = _placeholder_ids(cfg)
    trainer, unet, te, _ = _tiny_run(t, cfg, True, False)
    emb = te.get_input_embeddings()
    assert "forward" in emb.__dict__
    trainer.close()
    assert "forward" not in emb.__dict__
    learned = emb.weight.detach().clone()
    ids = t["ids"][0].to(DEV)
    with torch.no_grad():
        assert torch.equal(emb(ids), F.embedding(ids, learned))  # the module's own forward again
    path = str(tmp_path / "ti.safetensors")
    dfa.save_all(unet, te, ph, ["<s1>", "<s2>"], path, save_lora=False)
    from safetensors import safe_open

    with safe_open(path, "pt") as f:
        for tok, i in zip(["<s1>", "<s2>"], ph):
            assert torch.equal(f.get_tensor(tok), learned[i].cpu())
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    plist = list(itertools.chain(*params))
    with torch.no_grad():
        for p, v in zip(plist, torch.split(t["lora.init"], [q.numel() for q in plist])):
            p.copy_(v.view(p.shape).to(DEV))
    lt = tr.LoraTrainer(unet, te, lr=cfg["lr_unet"], lr_embed=cfg["lr_embed"], weight_decay=cfg["weight_decay"],
                        v_prediction=True)
    assert lt.token_table is not None and torch.equal(emb.weight.detach(), learned)  # starts from the learned rows
    lat, noise, ts, _ = orc.synthetic_batch(0, cfg["batch"], cfg["latent_hw"], cfg["ctx_len"], cfg["hidden"], t_max=800)
    loss = lt.step(lat.to(DEV), noise.to(DEV), ts.to(DEV), input_ids=ids)
    assert torch.isfinite(loss).all()
    assert not torch.equal(emb.weight.detach()[ph], learned[ph])  # continue_inversion trains the rows further


def test_full_size_window_against_the_stock_loop():
    """Config 5 shape (SD2.1-768 harness UNet, OpenCLIP-H-shaped encoder, 96² latents, batch 1, fp32): one accumulation window
    (5 micro-steps) against the stock-torch loop on the same GPU — rows and losses within the bounds, every other row
    bit-identical, and the peak allocation at least two table sizes below the stock loop's."""
    ph = [49400, 320]
    unet, te = config5_models(DEV)
    batches = config5_batches(5, DEV, ph)
    emb = te.get_input_embeddings()
    init = emb.weight.detach().clone()
    table_bytes = init.numel() * 4
    acp, s1 = tr.ddpm_tables(device=DEV)
    lam = tr.lr_lambda("linear", 0, 1000, lr_init=5e-4)

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ref_losses, _ = reference_inversion(unet, te, ph, batches, 5e-4, 0.0, 4, lam, True, False, acp, s1)
    torch.cuda.synchronize()
    ref_peak = torch.cuda.max_memory_allocated() - base
    ref_rows = emb.weight.detach()[ph].clone()
    with torch.no_grad():
        emb.weight.copy_(init)

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    trainer = InversionTrainer(unet, te, ph)
    losses = torch.stack([trainer.step(lat, noise, ts, input_ids=ids) for lat, noise, ts, ids, _ in batches]).reshape(-1)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    trainer.close()
    table = emb.weight.detach()
    rows_err = tr_rel(table[ph], ref_rows)
    move_err = tr_rel(table[ph] - init[ph], ref_rows - init[ph])
    loss_err = tr_rel(losses, ref_losses)
    print(f"\n[inversion full size] rows {rows_err:.3g} update {move_err:.3g} losses {loss_err:.3g} "
          f"peak {peak / 2**20:.0f} MiB vs stock {ref_peak / 2**20:.0f} MiB (table {table_bytes / 2**20:.0f} MiB)")
    assert rows_err < ROWS_TOL and loss_err < LOSS_TOL and move_err < MOVE_TOL
    others = torch.ones(init.shape[0], dtype=torch.bool, device=DEV)
    others[ph] = False
    assert torch.equal(table[others], init[others])
    assert peak + 2 * table_bytes <= ref_peak


def tr_rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()
