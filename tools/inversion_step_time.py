"""ms per micro-step and peak allocation of train_inversion (cli_lora_pti.py:290-346) at BASELINE config 5's shape — SD2.1-768
harness UNet, OpenCLIP-H-shaped encoder with its 49408 x 1024 fp32 table, 96² latents, batch 1, fp32 (mixed_precision=False,
:685) — for three runs on the same device:
  eager     InversionTrainer, host-launched micro-steps
  recorded  InversionTrainer(capture_graph=True)
  stock     the reference loop restated in stock torch (tests/inversion_reference.py): AdamW over the whole table + clone restore
Each run: `--warmup` micro-steps, then `--steps` timed ones (whole accumulation windows by default: 4 micro-steps each, the
optimizer at every 4th).  Peak = torch.cuda.max_memory_allocated() over the run minus what was allocated before it (the models).
Prints one JSON line.

`--fp32-attention` flips the UNet's attention onto the fp32 HIP core (attention.set_use_hip_attention(unet, True, fp32=True),
csrc/attn_f32.hip) before the trainers are built — all three runs then share the switched UNet; `--runs` restricts the runs
(a kernel trace of one route: `--runs eager`).

    python tools/inversion_step_time.py [--steps 16] [--warmup 4] [--fp32-attention] [--runs eager,recorded,stock]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffusion_finetuning_amd import trainer as tr  # noqa: E402
from diffusion_finetuning_amd.inversion import InversionTrainer  # noqa: E402
from tests.inversion_reference import config5_batches, config5_models, reference_inversion  # noqa: E402

PLACEHOLDERS = [49400, 320]


def timed(run_steps, n_warm, n_timed):
    """run_steps(k, on_step) runs k micro-steps; returns (ms per timed micro-step, peak bytes above the starting allocation)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    marks = {}

    def on_step(g):
        if g == n_warm - 1 or g == n_warm + n_timed - 1:
            torch.cuda.synchronize()
            marks[g] = time.perf_counter()

    run_steps(n_warm + n_timed, on_step)
    torch.cuda.synchronize()
    ms = (marks[n_warm + n_timed - 1] - marks[n_warm - 1]) * 1e3 / n_timed
    return ms, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--fp32-attention", action="store_true", help="run the UNet's fp32 attention on the HIP fp32 core")
    ap.add_argument("--runs", default="eager,recorded,stock", help="comma-separated subset of eager, recorded, stock")
    args = ap.parse_args()
    runs = [r for r in args.runs.split(",") if r]
    dev = "cuda"
    unet, te = config5_models(dev)
    if args.fp32_attention:
        from diffusion_finetuning_amd.attention import set_use_hip_attention

        set_use_hip_attention(unet, True, fp32=True)
    emb = te.get_input_embeddings()
    init = emb.weight.detach().clone()
    n = args.warmup + args.steps
    batches = config5_batches(n, dev, PLACEHOLDERS)
    acp, s1 = tr.ddpm_tables(device=dev)
    out = {"shape": "config 5: SD2.1-768 UNet, OpenCLIP-H encoder, 49408x1024 table, 96x96 latents, batch 1, fp32",
           "accum_iter": 4, "warmup": args.warmup, "steps": args.steps, "table_MiB": init.numel() * 4 / 2**20,
           "fp32_attention": bool(args.fp32_attention)}

    for name, graph in (("eager", False), ("recorded", True)):
        if name not in runs:
            continue
        with torch.no_grad():
            emb.weight.copy_(init)
        trainer = InversionTrainer(unet, te, PLACEHOLDERS, capture_graph=graph)

        def run(k, on_step, trainer=trainer):
            for g, (lat, noise, ts, ids, _) in enumerate(batches[:k]):
                trainer.step(lat, noise, ts, input_ids=ids)
                on_step(g)

        ms, peak = timed(run, args.warmup, args.steps)
        trainer.close()
        del trainer
        out[name] = {"ms_per_micro_step": round(ms, 3), "peak_MiB": round(peak / 2**20, 1)}

    with torch.no_grad():
        emb.weight.copy_(init)
    lam = tr.lr_lambda("linear", 0, 1000, lr_init=5e-4)

    def run_stock(k, on_step):
        reference_inversion(unet, te, PLACEHOLDERS, batches[:k], 5e-4, 0.0, 4, lam, True, False, acp, s1, on_step=on_step)

    if "stock" in runs:
        ms, peak = timed(run_stock, args.warmup, args.steps)
        out["stock"] = {"ms_per_micro_step": round(ms, 3), "peak_MiB": round(peak / 2**20, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
