"""What the EMA of the LoRA weights costs (LoraTrainer(ema_decay=...): lora_adamw_ema_step), at the SD1.5 rank-4 slab size —
1 246 464 fp32 elements.  Modelled on tools/objective_time.py, whose `spread` and `--bench-pairs` it reuses.

Default: the optimizer launch alone, in ONE process, alternating, --reps repetitions after an untimed round.  Every buffer is
allocated once and the C entries are called directly; --launches launches of one case are recorded into a hipGraph, and a
repetition times --replays replays of it between two device events — no host work between the launches — and reports the
device time per optimizer step:

  adamw              lora_adamw_step
  adamw + ema        lora_adamw_ema_step                   (one launch: 4 reads + 3 writes become 5 reads + 4 writes per element)
  adamw, torch ema   lora_adamw_step, then the average as three torch ops on the slab, diffusers' EMAModel.step:
                     tmp = s − p ; tmp *= omd ; s −= tmp   (what fusing avoids: three more launches, 7 more passes; omd is a host
                     number here, which a real run could only have by reading the device's step counter every step)

--step: ONE process runs the replayed LoraTrainer step of the headline configuration (bench.py config 2: SD1.5 UNet, LoRA rank
4, batch 4, device-drawn noise, hipGraph) --steps times after priming, recording and --warmup steps, each step ended by a
device synchronise and timed with a host clock; prints one JSON line.  --ema-decay switches the average on; --root DIR imports
the package (and bench.py's model builder) from another checkout, e.g. the parent commit's with its library built in place.

--pairs N --parent-root DIR: N rounds; every round starts three fresh `--step` processes one after the other — the parent
checkout, this tree with EMA off, this tree with ema_decay 0.9999 — so the three alternate.  Prints every process's median,
then per variant the median of the process medians with their spread (min – max).  The spread of the parent's processes is
the yardstick: EMA off must overlap it.

--bench-pairs N --parent-root DIR: objective_time.py's — `bench.py --gpus 1 --steps 20 --warmup 5` in the parent checkout and
in this tree, a process each, alternating.

    python tools/ema_time.py [--reps 7] [--launches 200] [--replays 20]
    python tools/ema_time.py --step [--ema-decay 0.9999] [--root DIR]
    python tools/ema_time.py --pairs 5 --parent-root DIR
    python tools/ema_time.py --bench-pairs 5 --parent-root DIR
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from objective_time import STEP_TIMEOUT_S, bench_pairs, spread  # noqa: E402

SLAB = 1246464  # LoRA elements of the SD1.5 UNet at rank 4 (bench.py config 2)


def kernels(a):
    import torch

    sys.path.insert(0, ROOT)
    from diffusion_finetuning_amd import _native as nat
    from diffusion_finetuning_amd import step as stp

    dev, n = "cuda", SLAB
    g = torch.Generator().manual_seed(0)
    p, s = (torch.randn(n, generator=g).mul_(0.02).to(dev) for _ in range(2))
    grad = torch.randn(n, generator=g).mul_(1e-3).to(dev)
    m, v, tmp = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.empty(n, device=dev)
    norm = torch.tensor([1.0, 0.0, 1000.0, 0.0], device=dev)  # a clean step, 1000 applied so far
    omd = stp.ema_one_minus_decay_at(1000, 0.9999, 0)
    lib, P = nat.lib(), nat._ptr
    hyper = (1.0, 1.0, 1e-4, 0.9, 0.999, 1e-8, 1e-2, 0)

    def stream():
        return nat._stream(p)  # (the current stream: the capture's while a graph is recorded)

    def adamw():
        return lib.lora_adamw_step(P(p), P(grad), P(m), P(v), n, P(norm), *hyper, stream())

    def adamw_ema():
        return lib.lora_adamw_ema_step(P(p), P(grad), P(m), P(v), P(s), n, P(norm), *hyper, 0.9999, 0, stream())

    def adamw_torch_ema():
        st = adamw()
        torch.sub(s, p, out=tmp)
        tmp.mul_(omd)
        s.sub_(tmp)
        return st

    entries = {"adamw": adamw, "adamw + ema": adamw_ema, "adamw, torch ema": adamw_torch_ema}
    graphs = {}
    for name, fn in entries.items():  # --launches steps of one case recorded once: replays issue them with no host in between
        assert fn() == 0, name
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(a.launches):
                fn()

    def per_step_us(graph):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(a.replays):
            graph.replay()
        end.record()
        end.synchronize()
        return 1e3 * start.elapsed_time(end) / (a.launches * a.replays)

    for graph in graphs.values():  # untimed round
        per_step_us(graph)
    times = {name: [] for name in entries}
    for rep in range(a.reps):
        for name, graph in graphs.items():
            times[name].append(per_step_us(graph))
        print(f"rep {rep}: " + ", ".join(f"{k} {v[-1]:.2f} us" for k, v in times.items()), flush=True)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(s).all())
    print(f"medians, device us per optimizer step over {n} elements (replayed graphs of {a.launches} steps, {a.replays} replays a "
          "repetition): " + "; ".join(f"{k} {spread(v)}" for k, v in times.items()), flush=True)
    print(json.dumps({"gpu": torch.cuda.get_device_name(0), "elements": n, "launches": a.launches, "replays": a.replays,
                      "reps": a.reps, "median_us": {k: statistics.median(v) for k, v in times.items()}, "all_us": times}),
          flush=True)


def step(a):
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch

    import bench  # the headline configuration's model and batches, from the checkout under test
    from diffusion_finetuning_amd.trainer import LoraTrainer

    assert os.path.abspath(bench.__file__).startswith(root), bench.__file__
    cfg = bench.CONFIGS[2]
    unet = bench.build_unet("cuda", torch.float16, cfg["rank"], cfg["unet"])
    knobs = {} if a.ema_decay is None else {"ema_decay": a.ema_decay}
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
    print(json.dumps({"root": root, "knobs": knobs, "slab": int(trainer.slab.numel), "steps": a.steps,
                      "median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "loss": float(loss)}),
          flush=True)


def pairs(a):
    variants = {"parent": ["--root", os.path.abspath(a.parent_root)], "ema off": [], "ema on": ["--ema-decay", "0.9999"]}
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
                  f"over {line['steps']} replayed steps, loss {line['loss']:.5f}", flush=True)
    print("median of the process medians, ms/step: " + "; ".join(f"{k} {spread(v)}" for k, v in medians.items()), flush=True)
    print(json.dumps({"rounds": a.pairs, "steps_per_process": a.steps, "process_median_ms": medians,
                      "median_ms": {k: statistics.median(v) for k, v in medians.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200, help="optimizer steps of a case in one recorded graph")
    ap.add_argument("--replays", type=int, default=20, help="replays of that graph per repetition")
    ap.add_argument("--step", action="store_true", help="one process: the replayed headline step")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ema-decay", type=float, default=None)
    ap.add_argument("--root", default=ROOT, help="with --step: the checkout whose package and bench.py are imported")
    ap.add_argument("--pairs", type=int, default=None, metavar="N", help="N rounds of parent / ema off / ema on processes")
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
