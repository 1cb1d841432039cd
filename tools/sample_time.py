"""Time of one 50-step sample at SD1.5 shape — batch 4 with classifier-free guidance (8 UNet rows), 64×64 latents, f16 — on
three routes through the same UNet (harness SD1.5 topology, random weights, LoRA rank 4 injected, HIP attention and GEGLU on):

  replayed      LatentSampler(capture_graph=True): one recorded iteration (forward, ddpm_sample_step, advance) replayed 50 times
  host          LatentSampler(capture_graph=False): the same launches issued from the host
  stock         the loop a diffusers pipeline runs around the forward, written out in torch ops: torch.randn, cat of the doubled
                input, cast, chunk, guidance, the same linear update with host scalars, randn for the variance noise

The parent commit has no sampler, so the stock loop is the baseline.  All three routes run in ONE process, alternating, --reps
times after one untimed round (recording, solver searches, allocator); each sample ends in a device synchronise and is timed with
a host clock.  Prints one readable line per repetition, the medians, and one JSON line.

    python tools/sample_time.py [--reps 5] [--steps 50] [--batch 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import diffusion_finetuning_amd as dfa  # noqa: E402
from diffusion_finetuning_amd.attention import set_use_hip_attention, set_use_hip_geglu  # noqa: E402


def build_unet():
    from harness.unet import UNet2DConditionModel, sd15_config

    torch.manual_seed(0)
    cfg = sd15_config()
    unet = UNet2DConditionModel(cfg).requires_grad_(False).half().to("cuda")
    params, _ = dfa.inject_trainable_lora(unet, r=4)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for group in params[::2]:  # the lora_up factors: non-zero, as after training
            for p in group:
                p.copy_((torch.randn(p.shape, generator=g) * 0.02).to(p.device, p.dtype))
    set_use_hip_attention(unet, True)
    set_use_hip_geglu(unet, True)
    return unet.eval(), cfg.cross_attention_dim


def stock_loop(unet, cond, neg, steps, guidance, latent_shape, timesteps, coef, gen):
    """What the pipeline does per step (pipeline __call__ + scheduler.step), with this library's forward."""
    B = cond.shape[0]
    ctx = torch.cat([neg, cond]).half()
    x = torch.randn((B, *latent_shape), generator=gen, device="cuda", dtype=torch.float32)
    with torch.no_grad():
        for i in range(steps):
            t = timesteps[i]
            a, b, sigma = coef[i]
            model_in = torch.cat([x] * 2).half()
            out = unet(model_in, t.expand(2 * B), ctx).sample
            u, c = out.float().chunk(2)
            o = u + guidance * (c - u)
            x = a * x + b * o
            if sigma != 0.0:
                x = x + sigma * torch.randn(x.shape, generator=gen, device="cuda", dtype=torch.float32)
    return x


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    unet, ctx_dim = build_unet()
    shape = (4, 64, 64)
    g = torch.Generator().manual_seed(2)
    cond = torch.randn(a.batch, 77, ctx_dim, generator=g).to("cuda")
    neg = torch.randn(a.batch, 77, ctx_dim, generator=g).to("cuda")
    guidance = 5.0
    replayed = dfa.LatentSampler(unet, a.steps, guidance)
    host = dfa.LatentSampler(unet, a.steps, guidance, capture_graph=False)
    ts, coef = dfa.sampler_schedule("ddpm", a.steps, False)
    ts_dev, coef_host = ts.to("cuda"), [tuple(float(v) for v in row) for row in coef]
    gen = torch.Generator(device="cuda").manual_seed(3)
    routes = {
        "replayed": lambda: replayed.sample(cond, neg, seed=7, latent_shape=shape),
        "host": lambda: host.sample(cond, neg, seed=7, latent_shape=shape),
        "stock": lambda: stock_loop(unet, cond, neg, a.steps, guidance, shape, ts_dev, coef_host, gen),
    }
    first = {name: timed(fn) for name, fn in routes.items()}  # untimed round: recording, solver searches, allocator
    assert replayed.replaying, "the recording failed: the replayed route would measure host launches"
    same = bool(torch.equal(first["replayed"][1], first["host"][1]))
    print(f"first (untimed) round, ms: " + ", ".join(f"{k} {v[0]:.1f}" for k, v in first.items()) +
          f"; replayed == host-launched bit for bit: {same}", flush=True)
    times = {name: [] for name in routes}
    for rep in range(a.reps):
        for name, fn in routes.items():
            times[name].append(timed(fn)[0])
        print(f"rep {rep}: " + ", ".join(f"{k} {times[k][-1]:.1f} ms" for k in routes), flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    print("medians: " + ", ".join(f"{k} {v:.1f} ms ({v / a.steps:.2f} ms/step)" for k, v in med.items()), flush=True)
    print(json.dumps({"gpu": torch.cuda.get_device_name(0), "unet": "sd15", "batch": a.batch,
                      "rows": 2 * a.batch, "steps": a.steps, "dtype": "f16", "guidance": guidance, "reps": a.reps,
                      "median_ms": med, "all_ms": times, "first_round_ms": {k: v[0] for k, v in first.items()},
                      "replayed_equals_host": same, "stock_over_replayed": med["stock"] / med["replayed"],
                      "host_over_replayed": med["host"] / med["replayed"]}), flush=True)


if __name__ == "__main__":
    main()
