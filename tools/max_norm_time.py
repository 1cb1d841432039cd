"""What the max-norm constraint on the LoRA updates costs (LoraTrainer(max_weight_norm=...): lora_max_norm), on the slab of the
SD1.5 UNet — 144 layers — at rank 4 (1 246 464 fp32 elements) and at rank 64.  Modelled on tools/ema_time.py, whose `--step`
process and whose `spread` / `--bench-pairs` (tools/objective_time.py) it reuses.

Default: the launch alone, in ONE process, alternating, --reps repetitions after an untimed round.  Every buffer is allocated
once and the C entries are called directly; --launches launches of one case are recorded into a hipGraph, and a repetition times
--replays replays of it between two device events — no host work between the launches — and reports the device time per launch:

  adamw              lora_adamw_step on the same slab (rank 4 only: the launch the projection follows)
  none over          no layer above the bound: every layer is read once, nothing is written but the 2 stats per layer
  half over          every second layer above the bound: those are read twice and written once
  all over           every layer above the bound

A scaled layer lands ON the bound, so a second launch with the same bound would find nothing to do.  The recorded launches
therefore take a falling sequence of bounds, bound_k = 0.97^k — every launch of a replay finds the "over" layers (norm 10 at the
start of a replay, then bound_{k-1}) above its own bound, the "under" layers (norm 1e-4) never — and each replay starts with one
device copy of the slab from a saved image (1/--launches of the timed work).

--step / --pairs N / --bench-pairs N --parent-root DIR: tools/ema_time.py's protocol with `max_weight_norm` as the knob — one
process per measurement of the replayed headline step (bench.py config 2), the parent checkout, this tree with the knob off and
with it on, alternating; and bench.py itself in the parent checkout and in this tree.

    python tools/max_norm_time.py [--reps 7] [--launches 200] [--replays 20]
    python tools/max_norm_time.py --step [--max-weight-norm 1.0] [--root DIR]
    python tools/max_norm_time.py --pairs 5 --parent-root DIR
    python tools/max_norm_time.py --bench-pairs 5 --parent-root DIR
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from objective_time import STEP_TIMEOUT_S, bench_pairs, spread  # noqa: E402

HBM_BYTES_PER_US = 6.29e6  # measured float4 copy rate of the MI355X: 6.29 TB/s
BOUND_RATIO = 0.97


def sd15_layers():
    """[(K, N)] of the 144 LoRA targets of the SD1.5 UNet, in enumeration order (no weights are allocated)."""
    import torch

    sys.path.insert(0, ROOT)
    import diffusion_finetuning_amd as dfa
    from harness.unet import UNet2DConditionModel, sd15_config

    with torch.device("meta"):
        unet = UNet2DConditionModel(sd15_config())
    return [(m.in_features, m.out_features) for _, _, m in dfa._find_modules(unet, dfa.DEFAULT_TARGET_REPLACE)]


def build_slab(layers, r, over, gen):
    """(host slab, table rows): layer l is [up | down]; its norm is 10 where over(l), else 1e-4 (exactly enough: the factors are
    rescaled from a float64 product norm)."""
    import torch

    rows, parts, at = [], [], 0
    for l, (K, N) in enumerate(layers):
        up = torch.randn(N, r, generator=gen) * 0.02
        down = torch.randn(r, K, generator=gen) / r
        gram = (down.double() @ down.double().T) * (up.double().T @ up.double())  # ‖up·down‖_F² without the [N,K] product
        norm = math.sqrt(float(gram.sum()))
        up = up * ((10.0 if over(l) else 1e-4) / norm)
        rows.append((at, at + N * r, K, N, r, 1.0))
        parts += [up.reshape(-1), down.reshape(-1)]
        at += r * (K + N)
    return torch.cat(parts), rows


def kernels(a):
    import torch

    sys.path.insert(0, ROOT)
    from diffusion_finetuning_amd import _native as nat

    dev = "cuda"
    layers = sd15_layers()
    lib, P = nat.lib(), nat._ptr
    results = {}
    for r in (4, 64):
        gen = torch.Generator().manual_seed(r)
        cases = {"none over": lambda l: False, "half over": lambda l: l % 2 == 0, "all over": lambda l: True}
        n = r * sum(K + N for K, N in layers)
        live = torch.empty(n, device=dev)
        stats = torch.zeros(2 * len(layers), device=dev)
        counters = torch.zeros(1, dtype=torch.int32, device=dev)
        images, table = {}, None
        for name, over in cases.items():
            host, rows = build_slab(layers, r, over, gen)
            images[name] = host.to(dev)
            table = nat.max_norm_table(rows, dev)  # (the layout is the same for the three cases)
        assert live.numel() == images["all over"].numel() and (r != 4 or n == 1246464)

        def stream():
            return nat._stream(live)  # (the current stream: the capture's while a graph is recorded)

        def clamp(bound):
            return lib.lora_max_norm(P(live), P(table), len(layers), r, bound, P(stats), P(counters), stream())

        entries = {}
        if r == 4:
            grad = torch.randn(n, generator=gen).mul_(1e-3).to(dev)
            m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            norm = torch.tensor([1.0, 0.0, 1000.0, 0.0], device=dev)  # a clean step, 1000 applied so far
            hyper = (1.0, 1.0, 1e-4, 0.9, 0.999, 1e-8, 1e-2, 0)
            entries["adamw"] = (images["none over"], lambda k: lib.lora_adamw_step(P(live), P(grad), P(m), P(v), n, P(norm), *hyper,
                                                                                  stream()))
        for name in cases:
            entries[name] = (images[name], lambda k: clamp(BOUND_RATIO ** k))
        graphs = {}
        for name, (image, fn) in entries.items():
            live.copy_(image)
            assert fn(0) == 0, name
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                live.copy_(image)
                for k in range(a.launches):
                    fn(k)
        # what a replay of each case scales: counted once, outside the timed windows
        scaled = {}
        for name in cases:
            counters.zero_()
            graphs[name].replay()
            torch.cuda.synchronize()
            scaled[name] = int(counters.cpu()[0]) / a.launches
            assert bool(torch.isfinite(live).all()), name
        want = {"none over": 0, "half over": (len(layers) + 1) // 2, "all over": len(layers)}
        assert scaled == {k: float(x) for k, x in want.items()}, (scaled, want)

        def per_launch_us(graph):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(a.replays):
                graph.replay()
            end.record()
            end.synchronize()
            return 1e3 * start.elapsed_time(end) / (a.launches * a.replays)

        for graph in graphs.values():  # untimed round
            per_launch_us(graph)
        times = {name: [] for name in entries}
        for rep in range(a.reps):
            for name, graph in graphs.items():
                times[name].append(per_launch_us(graph))
            print(f"rank {r}, rep {rep}: " + ", ".join(f"{k} {v[-1]:.2f} us" for k, v in times.items()), flush=True)
        med = {k: statistics.median(v) for k, v in times.items()}
        one_read = 4 * n / HBM_BYTES_PER_US
        print(f"rank {r}: medians, device us per launch over {n} elements in {len(layers)} layers (replayed graphs of {a.launches} "
              f"launches, {a.replays} replays a repetition): " + "; ".join(f"{k} {spread(v)}" for k, v in times.items()), flush=True)
        print(f"rank {r}: layers scaled per launch {scaled}; one read of the slab at 6.29 TB/s = {one_read:.2f} us; ratio to it: "
              + ", ".join(f"{k} {med[k] / one_read:.2f}" for k in cases)
              + ("; ratio to the AdamW launch: " + ", ".join(f"{k} {med[k] / med['adamw']:.2f}" for k in cases) if r == 4 else ""),
              flush=True)
        results[f"rank {r}"] = {"elements": n, "layers": len(layers), "median_us": med, "all_us": times, "scaled_per_launch": scaled,
                                "one_read_at_hbm_us": one_read}
    print(json.dumps({"gpu": torch.cuda.get_device_name(0), "launches": a.launches, "replays": a.replays, "reps": a.reps,
                      **results}), flush=True)


def step(a):
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch

    import bench  # the headline configuration's model and batches, from the checkout under test
    from diffusion_finetuning_amd.trainer import LoraTrainer

    assert os.path.abspath(bench.__file__).startswith(root), bench.__file__
    cfg = bench.CONFIGS[2]
    unet = bench.build_unet("cuda", torch.float16, cfg["rank"], cfg["unet"])
    knobs = {} if a.max_weight_norm is None else {"max_weight_norm": a.max_weight_norm}
    trainer = LoraTrainer(unet, None, lr=1e-4, capture_graph=True, v_prediction=cfg["v_prediction"], **knobs)
    data = bench.synthetic_steps(1, cfg["batch"], cfg["latent"], 0, 1, "cuda", cfg["ctx_len"], cfg["ctx_dim"])

    def run_step():
        lat, _, _, cond = data[0]
        return trainer.step(lat, None, None, seed=1000, encoder_hidden_states=cond)

    trainer.capture_graph = False
    run_step()  # priming, host-launched: solver searches and lazy initialisation
    trainer.capture_graph = True
    run_step()  # records
    assert trainer._graph is not None, "the recording failed: the run would measure host launches"
    for _ in range(a.warmup):
        run_step()
    times = []
    for _ in range(a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = run_step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    assert trainer._graph is not None
    logged = trainer.max_norm_stats() if knobs else None
    print(json.dumps({"root": root, "knobs": knobs, "slab": int(trainer.slab.numel), "steps": a.steps,
                      "median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "loss": float(loss),
                      "max_norm_stats": logged}), flush=True)


def pairs(a):
    variants = {"parent": ["--root", os.path.abspath(a.parent_root)], "knob off": [],
                "knob on": ["--max-weight-norm", str(a.max_weight_norm if a.max_weight_norm is not None else 0.05)]}
    medians = {name: [] for name in variants}
    for rnd in range(a.pairs):
        for name, extra in variants.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--step", "--steps", str(a.steps), "--warmup", str(a.warmup), *extra]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
            if out.returncode != 0:  # nothing more is started on the device after a process that failed
                sys.exit(f"[round {rnd}, {name}] exit status {out.returncode}\n{out.stderr[-2000:]}")
            line = json.loads(out.stdout.strip().splitlines()[-1])
            medians[name].append(line["median_ms"])
            print(f"round {rnd}, {name}: median {line['median_ms']:.3f} ms/step (min {line['min_ms']:.3f}, max {line['max_ms']:.3f}) "
                  f"over {line['steps']} replayed steps, loss {line['loss']:.5f}, {line['max_norm_stats']}", flush=True)
    print("median of the process medians, ms/step: " + "; ".join(f"{k} {spread(v)}" for k, v in medians.items()), flush=True)
    print(json.dumps({"rounds": a.pairs, "steps_per_process": a.steps, "process_median_ms": medians,
                      "median_ms": {k: statistics.median(v) for k, v in medians.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200, help="launches of a case in one recorded graph")
    ap.add_argument("--replays", type=int, default=20, help="replays of that graph per repetition")
    ap.add_argument("--step", action="store_true", help="one process: the replayed headline step")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-weight-norm", type=float, default=None)
    ap.add_argument("--root", default=ROOT, help="with --step: the checkout whose package and bench.py are imported")
    ap.add_argument("--pairs", type=int, default=None, metavar="N", help="N rounds of parent / knob off / knob on processes")
    ap.add_argument("--bench-pairs", type=int, default=None, metavar="N", help="N rounds of bench.py: parent checkout / this tree")
    ap.add_argument("--parent-root", default=None)
    a = ap.parse_args()
    if a.bench_pairs is not None:
        if a.bench_pairs < 5 or a.parent_root is None:
            ap.error("--bench-pairs takes N >= 5 and needs --parent-root")
        return bench_pairs(a)
    if a.pairs is not None:
        if a.pairs < 5 or a.parent_root is None:
            ap.error("--pairs takes N >= 5 and needs --parent-root")
        return pairs(a)
    if a.step:
        return step(a)
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    kernels(a)


if __name__ == "__main__":
    main()
