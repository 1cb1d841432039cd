"""What the training-objective knobs cost (snr_gamma / timestep_weights: ddpm_mse_weighted_fwd_bwd; noise_offset: the
`_offset` prologues), at the headline shape — 4 rows of 4×64×64 latents, f16.

Default: the kernels alone, in ONE process, alternating, --reps repetitions after an untimed round.  Every output is allocated
once and the C entries are called directly; --launches launches of one entry are recorded into a hipGraph, and a repetition
times --replays replays of it between two device events — no host work between the launches, the way a recorded step runs
them — and reports the device time per launch:

  loss               ddpm_mse_fwd_bwd                      loss weighted        ddpm_mse_weighted_fwd_bwd (Min-SNR γ = 5 table)
  noise              ddpm_noise_prologue                   noise offset         ddpm_noise_prologue_offset (0.1)
  posterior          ddpm_posterior_prologue               posterior offset     ddpm_posterior_prologue_offset (0.1)

--step: ONE process runs the replayed LoraTrainer step of the headline configuration (bench.py config 2: SD1.5 UNet, LoRA rank
4, batch 4, device-drawn noise, hipGraph) --steps times after priming, recording and --warmup steps, each step ended by a
device synchronise and timed with a host clock; prints one JSON line.  (MIOpen stays in immediate mode — bench.py's shipped
find-db is not loaded — for every variant alike: the convolutions are not what is compared.)  --snr-gamma / --noise-offset switch the knobs on;
--root DIR imports the package (and bench.py's model builder) from another checkout, e.g. the parent commit's with its library
built in place.

--pairs N --parent-root DIR: the comparison across processes.  N rounds; every round starts three fresh `--step` processes one
after the other — the parent checkout, this tree with the knobs off, this tree with both knobs on — so the three alternate.
Prints every process's median, then per variant the median of the process medians with their spread (min – max), and one JSON
line.  The spread of the parent's processes is the yardstick the other two are read against.

    python tools/objective_time.py [--reps 7] [--launches 200] [--replays 20]
    python tools/objective_time.py --step [--snr-gamma 5 --noise-offset 0.1] [--root DIR]
    python tools/objective_time.py --pairs 5 --parent-root DIR
    python tools/objective_time.py --bench-pairs 5 --parent-root DIR

--bench-pairs N --parent-root DIR: `bench.py --gpus 1 --steps 20 --warmup 5` in the parent checkout and in this tree, a process
each, alternating, N rounds; prints every run's line, then medians and spreads.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 240  # one --step process: model build, priming, recording and a few dozen 30-ms steps


def spread(values):
    return f"{statistics.median(values):.4g} (spread {min(values):.4g} – {max(values):.4g})"


def kernels(a):
    import torch

    sys.path.insert(0, ROOT)
    from diffusion_finetuning_amd import _native as nat
    from diffusion_finetuning_amd import step as stp
    from diffusion_finetuning_amd import trainer as tr

    dev, dtype, shape = "cuda", torch.float16, (4, 4, 64, 64)
    B, per_row, hw, code = shape[0], shape[1] * shape[2] * shape[3], shape[2] * shape[3], nat.dtype_code(dtype)
    g = torch.Generator().manual_seed(0)
    pred, target = (torch.randn(shape, generator=g).to(dev, dtype) for _ in range(2))
    x0 = (torch.randn(shape, generator=g) * 0.18215).to(dev)
    moments = torch.cat([torch.randn(shape, generator=g), torch.randn(shape, generator=g) - 3.0], dim=1).to(dev, dtype)
    t = torch.tensor([10, 400, 700, 999], device=dev)
    table = stp.min_snr_weights(tr.ddpm_alphas_cumprod(), 5.0).to(dev)
    sa, sb = tr.ddpm_tables(device=dev)
    # every output allocated once: a timed launch is the C entry alone
    loss, dpred = torch.empty(1, device=dev), torch.empty_like(pred)
    ws = torch.empty(int(nat.lib().lora_mse_workspace_bytes()), dtype=torch.uint8, device=dev)
    noisy, tgt, t_out = torch.empty_like(pred), torch.empty_like(pred), torch.empty(B, dtype=torch.int64, device=dev)
    lib, P = nat.lib(), nat._ptr
    mdt = nat.dtype_code(moments.dtype)

    def stream():
        return nat._stream(pred)  # (the current stream: the capture's while a graph is recorded)

    entries = {
        "loss": lambda: lib.ddpm_mse_fwd_bwd(P(pred), P(target), None, 4, 0, per_row, hw, 1.0, 1024.0, P(loss), P(dpred), P(ws),
                                             code, stream()),
        "loss weighted": lambda: lib.ddpm_mse_weighted_fwd_bwd(P(pred), P(target), None, P(t), P(table), table.numel(), 4, 0,
                                                               per_row, hw, 1.0, 1024.0, P(loss), P(dpred), P(ws), code, stream()),
        "noise": lambda: lib.ddpm_noise_prologue(P(x0), P(sa), P(sb), P(noisy), P(tgt), None, P(t_out), B, per_row, 1000, 1000, 3,
                                                 0, code, stream()),
        "noise offset": lambda: lib.ddpm_noise_prologue_offset(P(x0), P(sa), P(sb), P(noisy), P(tgt), None, P(t_out), B, per_row,
                                                               1000, 1000, 3, 0, code, hw, 0.1, None, stream()),
        "posterior": lambda: lib.ddpm_posterior_prologue(P(moments), mdt, P(sa), P(sb), P(noisy), P(tgt), None, None, None,
                                                         P(t_out), B, per_row, 1000, 0.18215, 1000, 3, 0, code, stream()),
        "posterior offset": lambda: lib.ddpm_posterior_prologue_offset(P(moments), mdt, P(sa), P(sb), P(noisy), P(tgt), None, None,
                                                                       None, P(t_out), B, per_row, 1000, 0.18215, 1000, 3, 0,
                                                                       code, hw, 0.1, None, stream()),
    }
    graphs = {}
    for name, fn in entries.items():  # --launches launches of one entry recorded once: replays issue them with no host in between
        assert fn() == 0, name
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(a.launches):
                fn()

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
        print(f"rep {rep}: " + ", ".join(f"{k} {v[-1]:.2f} us" for k, v in times.items()), flush=True)
    print(f"medians, device us per launch of the entry (replayed graphs of {a.launches} launches, {a.replays} replays a repetition; the "
          "loss entries are two kernels, ticket zeroing + loss): " + "; ".join(f"{k} {spread(v)}" for k, v in times.items()), flush=True)
    print(json.dumps({"gpu": torch.cuda.get_device_name(0), "shape": list(shape), "dtype": "f16", "launches": a.launches,
                      "replays": a.replays, "reps": a.reps, "median_us": {k: statistics.median(v) for k, v in times.items()},
                      "all_us": times}), flush=True)


def step(a):
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch

    import bench  # the headline configuration's model and batches, from the checkout under test
    from diffusion_finetuning_amd.trainer import LoraTrainer

    assert os.path.abspath(bench.__file__).startswith(root), bench.__file__
    cfg = bench.CONFIGS[2]
    unet = bench.build_unet("cuda", torch.float16, cfg["rank"], cfg["unet"])
    knobs = {}
    if a.snr_gamma is not None:
        knobs["snr_gamma"] = a.snr_gamma
    if a.noise_offset:
        knobs["noise_offset"] = a.noise_offset
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
    print(json.dumps({"root": root, "knobs": knobs, "steps": a.steps, "median_ms": statistics.median(times), "min_ms": min(times),
                      "max_ms": max(times), "loss": float(loss)}), flush=True)


def pairs(a):
    variants = {"parent": ["--root", os.path.abspath(a.parent_root)], "knobs off": [],
                "knobs on": ["--snr-gamma", "5", "--noise-offset", "0.1"]}
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


def bench_pairs(a):
    """bench.py of the parent checkout and of this tree, a process each, alternating."""
    roots = {"parent": os.path.abspath(a.parent_root), "this tree": ROOT}
    values = {name: [] for name in roots}
    for rnd in range(a.bench_pairs):
        for name, root in roots.items():
            cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]
            out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
            if out.returncode != 0:  # nothing more is started on the device after a process that failed
                sys.exit(f"[round {rnd}, {name}] exit status {out.returncode}\n{out.stderr[-2000:]}")
            line = json.loads(out.stdout.strip().splitlines()[-1])
            values[name].append(line["value"])
            print(f"round {rnd}, {name}: {line['value']:.2f} images/s, {line['ms_per_step']:.3f} ms/step, hipgraph "
                  f"{line['config']['hipgraph']}", flush=True)
    print("bench.py --gpus 1 --steps 20 --warmup 5, images/s: " + "; ".join(f"{k} {spread(v)}" for k, v in values.items()), flush=True)
    print(json.dumps({"rounds": a.bench_pairs, "images_per_s": values,
                      "median": {k: statistics.median(v) for k, v in values.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200, help="launches of an entry in one recorded graph")
    ap.add_argument("--replays", type=int, default=20, help="replays of that graph per repetition")
    ap.add_argument("--step", action="store_true", help="one process: the replayed headline step")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--snr-gamma", type=float, default=None)
    ap.add_argument("--noise-offset", type=float, default=0.0)
    ap.add_argument("--root", default=ROOT, help="with --step: the checkout whose package and bench.py are imported")
    ap.add_argument("--pairs", type=int, default=None, metavar="N", help="N rounds of parent / knobs off / knobs on processes")
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
