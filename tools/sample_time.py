"""Time of one sample (50 DDPM steps unless --method / --steps say otherwise) at SD1.5 shape — batch 4 with classifier-free
guidance (8 UNet rows), 64×64 latents, f16 — on three routes through the same UNet (harness SD1.5 topology, random weights,
LoRA rank 4 injected, HIP attention and GEGLU on):

  replayed      LatentSampler(capture_graph=True): one recorded iteration (forward, ddpm_sample_step, advance) replayed 50 times
  host          LatentSampler(capture_graph=False): the same launches issued from the host
  stock         the loop a diffusers pipeline runs around the forward, written out in torch ops: torch.randn, cat of the doubled
                input, cast, chunk, guidance, the same linear update with host scalars, randn for the variance noise

The stock loop is the baseline.  All three routes run in ONE process, alternating, --reps
times after one untimed round (recording, solver searches, allocator); each sample ends in a device synchronise and is timed with
a host clock.  Prints one readable line per repetition, the medians, and one JSON line.

--method and --steps take one value or several, paired in order ("ddpm" / "ddim" / "plms" / "dpmpp_2m"): every pair is a
configuration with its own three routes, and all of them alternate in the same process — so a replayed PLMS or DPM-Solver++(2M)
iteration (ddpm_sample_multistep) is timed next to a replayed DDPM iteration (ddpm_sample_step).  The multistep methods run
num_model_evaluations iterations (plms: steps + 1); their stock route keeps the history in a Python list of tensors, as a
diffusers scheduler does.  One readable line per repetition and configuration, medians and one JSON line per configuration.

"k_euler" / "euler_a" / "heun" (and --karras for their Karras sigma grid) time ddpm_sample_sigma the same way: heun runs
2·steps − 1 iterations; their stock route scales the model input, keeps the saved sample and derivative in Python variables and
passes fractional timesteps, as a k-diffusion sampler does.

--strength S adds an image-to-image route per configuration — `img2img`: a replayed LatentSampler begun from a random start
image at that strength, min(int(steps·S), steps) grid steps — and --keep-mask a second one, `img2img+mask`, with a keep mask of
8×8 blocks (ddpm_sample_*_keep).  They alternate with the full run's routes in the same process; every route is reported per
iteration of ITS run (a partial run has fewer), with the spread (min – max) of its repetitions.

--sweep K compares the two ways to sample K members of a `tune_lora_scale` sweep (scales 0 … 1, equal seed, one prompt) — the
reference's `visualize_progress` / img2img comparison loops:
  sequential       one member after the other on ONE LatentSampler: `tune_lora_scale(unet, s_k)`, then a B = 1 sample (2 UNet
                   rows).  The change of scale drops the recording, so every member pays its warm-up passes and a capture again
  sequential host  the same with capture_graph=False: no recording to lose, every launch issued from the host
  batched          ONE sample of K rows per pass (2K with guidance) with `lora_scales=` (the per-row gates of the fused forward)
                   and `shared_noise=True`, replayed — the recording survives every change of the table
in one process, alternating, medians and spreads over --reps; the first (untimed) round also prints how far member k of the
batch is from member k sampled alone.  --batch is not read in this mode.

--guidance-rescale PHI adds the route `rescaled` per configuration: the replayed route with `guidance_rescale=PHI`, that is
ddpm_cfg_rescale in front of every step launch inside the recording — timed next to the plain `replayed` route, alternating in
the same process.  --spacing trailing and --zero-terminal-snr add, for ddpm / ddim, the route `scheduled`: a replayed sampler on
that spacing and table (v-prediction with the zero-terminal-SNR table; with PHI too if given) — other host tables, the same
launches.  --routes NAME … times a subset of a configuration's routes.

    python tools/sample_time.py [--reps 5] [--steps 50] [--batch 4]
    python tools/sample_time.py --batch 1 --reps 7 --guidance-rescale 0.7 --spacing trailing --zero-terminal-snr \
        --routes replayed rescaled scheduled
    python tools/sample_time.py --sweep 4 --method ddpm plms --steps 50 50
    python tools/sample_time.py --batch 1 --method ddpm plms dpmpp_2m --steps 50 50 20
    python tools/sample_time.py --batch 1 --method plms --steps 50 --strength 0.75 --keep-mask
    python tools/sample_time.py --batch 1 --method ddpm euler_a heun --steps 50 50 25
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


def stock_multistep_loop(unet, cond, neg, guidance, latent_shape, timesteps, coef, plan, gen):
    """The same loop around a multistep scheduler: earlier outputs in a list of tensors, the saved sample, host scalars."""
    B = cond.shape[0]
    ctx = torch.cat([neg, cond]).half()
    x = torch.randn((B, *latent_shape), generator=gen, device="cuda", dtype=torch.float32)
    ring, saved = [None] * 4, None
    with torch.no_grad():
        for i in range(len(coef)):
            p, q, a, *c = coef[i]
            w, s1, s2, s3, flags = plan[i]
            model_in = torch.cat([x] * 2).half()
            out = unet(model_in, timesteps[i].expand(2 * B), ctx).sample
            u, cc = out.float().chunk(2)
            o = u + guidance * (cc - u)
            h = q * o if p == 0.0 else p * x + q * o
            nxt = a * (saved if flags & dfa.sampling.USE_SAVED else x) + c[0] * h
            for ck, sk in zip(c[1:], (s1, s2, s3)):
                if ck != 0.0:
                    nxt = nxt + ck * ring[sk]
            if flags & dfa.sampling.SAVE:
                saved = x
            if flags & dfa.sampling.PUSH:
                ring[w] = h
            x = nxt
    return x


def stock_sigma_loop(unet, cond, neg, guidance, latent_shape, timesteps, sigma0, coef, plan, gen):
    """The loop around a sigma-space sampler: the scaled model input, fractional timesteps, the saved sample and derivative in
    Python variables, randn for the ancestral noise, host scalars."""
    B = cond.shape[0]
    ctx = torch.cat([neg, cond]).half()
    x = sigma0 * torch.randn((B, *latent_shape), generator=gen, device="cuda", dtype=torch.float32)
    c_in, saved, d1 = 1.0 / (sigma0 * sigma0 + 1.0) ** 0.5, None, None
    with torch.no_grad():
        for i in range(len(coef)):
            p, q, a, c0, c1, s, n, _ = coef[i]
            flags = plan[i][4]
            model_in = torch.cat([x * c_in] * 2).half()
            out = unet(model_in, timesteps[i].expand(2 * B), ctx).sample
            u, cc = out.float().chunk(2)
            o = u + guidance * (cc - u)
            h = q * o if p == 0.0 else p * x + q * o
            nxt = a * (saved if flags & dfa.sampling.USE_SAVED else x) + c0 * h
            if c1 != 0.0:
                nxt = nxt + c1 * d1
            if s != 0.0:
                nxt = nxt + s * torch.randn(x.shape, generator=gen, device="cuda", dtype=torch.float32)
            if flags & dfa.sampling.SAVE:
                saved = x
            if flags & dfa.sampling.PUSH:
                d1 = h
            x, c_in = nxt, n
    return x


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def routes_for(unet, method, steps, guidance, cond, neg, shape, gen, strength=None, keep_mask=False, karras=False, rescale=None,
               spacing="leading", zero_snr=False):
    """(replayed sampler, {route: callable}, {route: iterations of its run}) of one configuration."""
    kw = dict(karras_sigmas=True) if karras and method in dfa.sampling.SAMPLER_SIGMA_METHODS else {}
    replayed = dfa.LatentSampler(unet, steps, guidance, method=method, **kw)
    host = dfa.LatentSampler(unet, steps, guidance, method=method, capture_graph=False, **kw)
    if method in dfa.sampling.SAMPLER_SIGMA_METHODS:
        ts, sigmas, coef, plan = dfa.sigma_schedule(dfa.sampling.SAMPLER_SIGMA_METHODS[method], steps, False, **kw)
        ts_dev, coef_host, plan_host = ts.float().to("cuda"), [tuple(float(v) for v in row) for row in coef], plan.tolist()
        stock = lambda: stock_sigma_loop(unet, cond, neg, guidance, shape, ts_dev, float(sigmas[0]), coef_host, plan_host, gen)  # noqa: E731
    elif method in dfa.sampling.MULTISTEP_METHODS:
        ts, coef, plan = dfa.multistep_schedule(method, steps, False)
        ts_dev, coef_host, plan_host = ts.to("cuda"), [tuple(float(v) for v in row) for row in coef], plan.tolist()
        stock = lambda: stock_multistep_loop(unet, cond, neg, guidance, shape, ts_dev, coef_host, plan_host, gen)  # noqa: E731
    else:
        ts, coef = dfa.sampler_schedule(method, steps, False)
        ts_dev, coef_host = ts.to("cuda"), [tuple(float(v) for v in row) for row in coef]
        stock = lambda: stock_loop(unet, cond, neg, steps, guidance, shape, ts_dev, coef_host, gen)  # noqa: E731
    routes = {
        "replayed": lambda: replayed.sample(cond, neg, seed=7, latent_shape=shape),
        "host": lambda: host.sample(cond, neg, seed=7, latent_shape=shape),
        "stock": stock,
    }
    extra = {}
    if rescale is not None:  # the plain replayed route plus ddpm_cfg_rescale in front of every step launch
        extra["rescaled"] = dfa.LatentSampler(unet, steps, guidance, method=method, guidance_rescale=rescale, **kw)
    if (spacing != "leading" or zero_snr) and method in dfa.sampling.METHODS:  # other host tables, the same launches
        extra["scheduled"] = dfa.LatentSampler(unet, steps, guidance, method=method, timestep_spacing=spacing,
                                               zero_terminal_snr=zero_snr, v_prediction=zero_snr, guidance_rescale=rescale or 0.0)
    for name, sampler in extra.items():
        routes[name] = lambda sampler=sampler: sampler.sample(cond, neg, seed=7, latent_shape=shape)
        sampler.begin(cond, neg, seed=7, latent_shape=shape)  # (records)
        assert sampler.replaying, f"the recording failed: the {name} route would measure host launches"
    iterations = {name: replayed.num_model_evaluations for name in routes}
    if strength is not None:
        g = torch.Generator().manual_seed(4)
        init = torch.randn(cond.shape[0], *shape, generator=g).to("cuda")
        yy, xx = torch.arange(shape[1]).view(-1, 1) // 8, torch.arange(shape[2]).view(1, -1) // 8
        mask = ((yy + xx) % 2).float().expand(cond.shape[0], 1, -1, -1).contiguous().to("cuda")
        for name, m in (("img2img", None),) + ((("img2img+mask", mask),) if keep_mask else ()):
            sampler = dfa.LatentSampler(unet, steps, guidance, method=method, **kw)  # (a sampler each: the recording depends on the mask)
            routes[name] = lambda sampler=sampler, m=m: sampler.sample(cond, neg, seed=7, init_latents=init, strength=strength,
                                                                       keep_mask=m)
            sampler.begin(cond, neg, seed=7, init_latents=init, strength=strength, keep_mask=m)  # (records; counts the run)
            assert sampler.replaying, "the recording failed: the image-to-image route would measure host launches"
            iterations[name] = sampler.run_evaluations
    return replayed, routes, iterations


def sweep(a):
    """--sweep K: K members one after another against one batched run (module docstring)."""
    K = a.sweep
    unet, ctx_dim = build_unet()
    shape, guidance = (4, 64, 64), 5.0
    g = torch.Generator().manual_seed(2)
    cond1, neg1 = torch.randn(1, 77, ctx_dim, generator=g).to("cuda"), torch.randn(1, 77, ctx_dim, generator=g).to("cuda")
    cond, neg = cond1.repeat(K, 1, 1), neg1.repeat(K, 1, 1)
    scales = [k / max(K - 1, 1) for k in range(K)]
    table = torch.tensor(scales, device="cuda")

    def members(sampler):
        out = []
        for s_k in scales:
            dfa.tune_lora_scale(unet, s_k)
            out.append(sampler.sample(cond1, neg1, seed=7, latent_shape=shape))
        dfa.tune_lora_scale(unet, 1.0)
        return torch.cat(out)

    configs = {}
    for method, steps in zip(a.method, a.steps):
        seq = dfa.LatentSampler(unet, steps, guidance, method=method)
        seq_host = dfa.LatentSampler(unet, steps, guidance, method=method, capture_graph=False)
        batched = dfa.LatentSampler(unet, steps, guidance, method=method)
        routes = {
            "sequential": lambda seq=seq: members(seq),
            "sequential host": lambda seq_host=seq_host: members(seq_host),
            "batched": lambda batched=batched: batched.sample(cond, neg, seed=7, latent_shape=shape, lora_scales=table,
                                                              shared_noise=True),
        }
        configs[f"{method} {steps}"] = (method, steps, batched, routes)
    first = {}
    for label, (_, _, batched, routes) in configs.items():  # untimed round: recording, solver searches, allocator
        first[label] = {name: timed(fn) for name, fn in routes.items()}
        assert batched.replaying, "the recording failed: the batched route would measure host launches"
        graph = batched._recorder.graph
        alone, both = first[label]["sequential host"][1].double(), first[label]["batched"][1].double()
        rel = [float((both[k] - alone[k]).norm() / alone[k].norm()) for k in range(K)]
        print(f"[sweep {K}, {label}] first (untimed) round, ms: " + ", ".join(f"{k} {v[0]:.1f}" for k, v in first[label].items()) +
              "; member k of the batch vs member k alone, rel L2: " + ", ".join(f"{r:.2e}" for r in rel), flush=True)
        configs[label] = configs[label] + (graph,)
    times = {label: {name: [] for name in cfg[3]} for label, cfg in configs.items()}
    for rep in range(a.reps):
        for label, (_, _, _, routes, _) in configs.items():
            for name, fn in routes.items():
                times[label][name].append(timed(fn)[0])
            print(f"[sweep {K}, {label}] rep {rep}: " + ", ".join(f"{k} {times[label][k][-1]:.1f} ms" for k in routes), flush=True)
    for label, (method, steps, batched, _, graph) in configs.items():
        assert batched._recorder.graph is graph, "the batched route recorded again"
        med = {k: statistics.median(v) for k, v in times[label].items()}
        print(f"[sweep {K}, {label}] medians: " + ", ".join(f"{k} {v:.1f} ms (spread {min(times[label][k]):.1f} – "
                                                           f"{max(times[label][k]):.1f})" for k, v in med.items()) +
              f"; sequential / batched = {med['sequential'] / med['batched']:.2f}, sequential host / batched = "
              f"{med['sequential host'] / med['batched']:.2f}", flush=True)
        print(json.dumps({"gpu": torch.cuda.get_device_name(0), "unet": "sd15", "sweep": K, "scales": scales, "method": method,
                          "steps": steps, "iterations": batched.num_model_evaluations, "dtype": "f16", "guidance": guidance,
                          "rows_sequential": 2, "rows_batched": 2 * K, "reps": a.reps, "median_ms": med, "all_ms": times[label],
                          "first_round_ms": {k: v[0] for k, v in first[label].items()},
                          "sequential_over_batched": med["sequential"] / med["batched"],
                          "sequential_host_over_batched": med["sequential host"] / med["batched"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, nargs="+", default=[50])
    ap.add_argument("--method", nargs="+", default=["ddpm"], choices=dfa.sampling.METHODS + dfa.sampling.MULTISTEP_METHODS +
                    tuple(dfa.sampling.SAMPLER_SIGMA_METHODS))
    ap.add_argument("--karras", action="store_true", help="the Karras sigma grid for k_euler / euler_a / heun")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--strength", type=float, default=None, help="add a replayed image-to-image route at this strength")
    ap.add_argument("--keep-mask", action="store_true", help="with --strength: add the route with a keep mask too")
    ap.add_argument("--guidance-rescale", type=float, default=None, metavar="PHI",
                    help="add the route `rescaled`: the replayed route with guidance_rescale=PHI (ddpm_cfg_rescale per iteration)")
    ap.add_argument("--spacing", default="leading", choices=dfa.sampling.SPACINGS,
                    help="with ddpm / ddim: add the route `scheduled` on this timestep spacing")
    ap.add_argument("--zero-terminal-snr", action="store_true",
                    help="with ddpm / ddim: the route `scheduled` on the zero-terminal-SNR table (v-prediction)")
    ap.add_argument("--routes", nargs="+", default=None, help="time these routes only (default: all of the configuration)")
    ap.add_argument("--sweep", type=int, default=None, metavar="K",
                    help="K members of a tune_lora_scale sweep one after another against one batched run (lora_scales=)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if len(a.steps) == 1:
        a.steps = a.steps * len(a.method)
    if len(a.steps) != len(a.method):
        ap.error("--steps takes one value, or one per --method")
    if a.keep_mask and a.strength is None:
        ap.error("--keep-mask needs --strength")
    if a.sweep is not None:
        if a.sweep < 2 or a.strength is not None:
            ap.error("--sweep takes K >= 2 and no --strength")
        return sweep(a)
    if a.karras and not any(m in dfa.sampling.SAMPLER_SIGMA_METHODS for m in a.method):
        ap.error("--karras needs one of " + " / ".join(dfa.sampling.SAMPLER_SIGMA_METHODS))
    unet, ctx_dim = build_unet()
    shape = (4, 64, 64)
    g = torch.Generator().manual_seed(2)
    cond = torch.randn(a.batch, 77, ctx_dim, generator=g).to("cuda")
    neg = torch.randn(a.batch, 77, ctx_dim, generator=g).to("cuda")
    guidance = 5.0
    gen = torch.Generator(device="cuda").manual_seed(3)
    configs = {}
    for method, steps in zip(a.method, a.steps):
        replayed, routes, its = routes_for(unet, method, steps, guidance, cond, neg, shape, gen, a.strength, a.keep_mask, a.karras,
                                           a.guidance_rescale, a.spacing, a.zero_terminal_snr)
        if a.routes:
            unknown = [r for r in a.routes if r not in routes]
            if unknown:
                ap.error(f"--routes: {unknown} not among {list(routes)} of {method}")
            routes = {name: routes[name] for name in a.routes}
        configs[f"{method} {steps}"] = (method, steps, replayed, routes, its)
    first, same = {}, {}
    for label, (_, _, replayed, routes, _) in configs.items():  # untimed round: recording, solver searches, allocator
        first[label] = {name: timed(fn) for name, fn in routes.items()}
        assert replayed.replaying or "replayed" not in routes, "the recording failed: the replayed route would measure host launches"
        same[label] = bool(torch.equal(first[label]["replayed"][1], first[label]["host"][1])) if {"replayed", "host"} <= set(routes) \
            else None
        print(f"[{label}] first (untimed) round, ms: " + ", ".join(f"{k} {v[0]:.1f}" for k, v in first[label].items()) +
              f"; replayed == host-launched bit for bit: {same[label]}", flush=True)
    times = {label: {name: [] for name in cfg[3]} for label, cfg in configs.items()}
    for rep in range(a.reps):
        for label, (_, _, _, routes, _) in configs.items():
            for name, fn in routes.items():
                times[label][name].append(timed(fn)[0])
            print(f"[{label}] rep {rep}: " + ", ".join(f"{k} {times[label][k][-1]:.1f} ms" for k in routes), flush=True)
    for label, (method, steps, _, _, its) in configs.items():
        med = {k: statistics.median(v) for k, v in times[label].items()}
        print(f"[{label}] medians: " + ", ".join(f"{k} {v:.1f} ms over {its[k]} iterations = {v / its[k]:.3f} ms/iteration "
                                                 f"(spread {min(times[label][k]) / its[k]:.3f} – {max(times[label][k]) / its[k]:.3f})"
                                                 for k, v in med.items()), flush=True)
        n_it = its["replayed"]
        ratio = lambda x, y: med[x] / med[y] if x in med and y in med else None  # noqa: E731
        print(json.dumps({"gpu": torch.cuda.get_device_name(0), "unet": "sd15", "batch": a.batch, "rows": 2 * a.batch,
                          "method": method, "steps": steps, "iterations": n_it, "route_iterations": its, "strength": a.strength,
                          "karras": bool(a.karras and method in dfa.sampling.SAMPLER_SIGMA_METHODS),
                          "guidance_rescale": a.guidance_rescale, "spacing": a.spacing, "zero_terminal_snr": a.zero_terminal_snr,
                          "dtype": "f16", "guidance": guidance,
                          "reps": a.reps, "median_ms": med, "all_ms": times[label],
                          "ms_per_iteration": {k: v / its[k] for k, v in med.items()},
                          "first_round_ms": {k: v[0] for k, v in first[label].items()}, "replayed_equals_host": same[label],
                          "stock_over_replayed": ratio("stock", "replayed"), "host_over_replayed": ratio("host", "replayed"),
                          "rescaled_over_replayed": ratio("rescaled", "replayed")}), flush=True)


if __name__ == "__main__":
    main()
