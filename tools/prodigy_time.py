"""What a Prodigy step costs next to AdamW's (LoraTrainer(optimizer="prodigy"): lora_prodigy_moments + lora_prodigy_apply), at the
SD1.5 rank-4 slab size — 1 246 464 fp32 elements.  Modelled on tools/ema_time.py; `spread` and `--bench-pairs` are
tools/objective_time.py's.

Default: the optimizer step alone, in ONE process, alternating, --reps repetitions after an untimed round.  Every buffer is
allocated once and the C entries are called directly; --launches steps of one route are recorded into a hipGraph, and a
repetition times --replays replays of it between two device events — no host work between the launches, d stays on the device —
and reports the device time per optimizer step:

  adamw           lora_grad_sqnorm, lora_adamw_step                         (7 slab-sized streams behind the norm's one)
  prodigy         lora_grad_sqnorm, lora_prodigy_moments, lora_prodigy_apply  (9 + 4 streams; d, d_max, numerator in device memory)
  prodigy, torch  lora_grad_sqnorm, then the same step as torch ops on the slab with d, d_max and the numerator as 0-dim
                  device tensors (what a framework optimizer does for ONE flat tensor without a host sync; a stock one walks
                  288 tensors and keeps d on the host).  The overflow skip is not reproduced: torch cannot skip without a sync.

growth_rate = 1 and γ = 1e-3 keep the replayed state finite over the ~30 000 identical steps of a run: d makes its one free
jump from d0 and holds; every branch of the scalar step still runs.

--step: ONE process runs the replayed LoraTrainer step of the headline configuration (bench.py config 2) --steps times after
priming, recording and --warmup steps, as tools/ema_time.py does; --optimizer prodigy switches (lr 1.0); --root DIR imports the
package and bench.py from another checkout, e.g. the parent commit's with its library built in place.

--pairs N --parent-root DIR: N rounds of three fresh `--step` processes — the parent checkout, this tree with AdamW, this tree
with Prodigy — alternating.  The spread of the parent's processes is the yardstick: this tree with AdamW must overlap it.

--bench-pairs N --parent-root DIR: objective_time.py's — `bench.py --gpus 1 --steps 20 --warmup 5` in the parent checkout and
in this tree, a process each, alternating.

    python tools/prodigy_time.py [--reps 7] [--launches 200] [--replays 20]
    python tools/prodigy_time.py --step [--optimizer prodigy] [--root DIR]
    python tools/prodigy_time.py --pairs 5 --parent-root DIR
    python tools/prodigy_time.py --bench-pairs 5 --parent-root DIR
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

SLAB = 1246464  # LoRA elements of the SD1.5 UNet at rank 4 (bench.py config 2)


def kernels(a):
    import torch

    sys.path.insert(0, ROOT)
    from diffusion_finetuning_amd import _native as nat

    dev, n = "cuda", SLAB
    gen = torch.Generator().manual_seed(0)
    lib, P = nat.lib(), nat._ptr
    grad = torch.randn(n, generator=gen).mul_(1e-3).to(dev)
    init = torch.randn(n, generator=gen).mul_(0.02).to(dev)
    b1, b2, eps, wd, lr, d0, max_norm = 0.9, 0.999, 1e-8, 1e-2, 1e-3, 1e-6, 1.0
    b3 = math.sqrt(b2)
    ws_norm = torch.empty(int(lib.lora_sqnorm_workspace_bytes()), dtype=torch.uint8, device=dev)
    ws_prodigy = torch.empty(int(lib.lora_prodigy_workspace_bytes()), dtype=torch.uint8, device=dev)
    ends, lrs, wds = nat.prodigy_ranges([n], [lr], [wd])

    def state():
        return {"p": init.clone(), "m": torch.zeros(n, device=dev), "v": torch.zeros(n, device=dev),
                "norm": torch.tensor([0.0, 0.0, 1000.0, 0.0], device=dev)}  # 1000 applied steps so far

    A, K, T = state(), state(), state()
    for st in (K, T):
        st.update(s=torch.zeros(n, device=dev), p0=init.clone())
    K["scalars"] = torch.tensor([d0, d0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=dev)
    T.update(d=torch.tensor(d0, device=dev), d_max=torch.tensor(d0, device=dev), numerator=torch.tensor(0.0, device=dev),
             g=torch.empty(n, device=dev), tmp=torch.empty(n, device=dev))

    def stream():
        return nat._stream(grad)  # (the current stream: the capture's while a graph is recorded)

    def norm_of(st):
        return lib.lora_grad_sqnorm(P(grad), n, 1.0, P(st["norm"]), P(ws_norm), stream())

    def adamw():
        return norm_of(A) or lib.lora_adamw_step(P(A["p"]), P(grad), P(A["m"]), P(A["v"]), n, P(A["norm"]), 1.0, max_norm, 1e-4, b1, b2,
                                                 eps, wd, 0, stream())

    def prodigy():
        return (norm_of(K)
                or lib.lora_prodigy_moments(P(K["p"]), P(K["p0"]), P(grad), P(K["m"]), P(K["v"]), P(K["s"]), n, ends, lrs, 1, P(K["norm"]),
                                            P(K["scalars"]), P(ws_prodigy), 1.0, max_norm, b1, b2, b3, d0, 1.0, 1.0, 0, 0, stream())
                or lib.lora_prodigy_apply(P(K["p"]), P(K["m"]), P(K["v"]), None, n, ends, lrs, wds, 1, P(K["norm"]), P(K["scalars"]), b1,
                                          b2, eps, 0, 0.0, 0, stream()))

    def prodigy_torch():
        status = norm_of(T)
        p, p0, m, v, s, g, tmp, d = T["p"], T["p0"], T["m"], T["v"], T["s"], T["g"], T["tmp"], T["d"]
        clip = torch.clamp(max_norm / (T["norm"][0].sqrt() + 1e-6), max=1.0)
        torch.mul(grad, clip, out=g)
        dlr, ratio = d * lr, d / d0
        torch.sub(p0, p, out=tmp)
        tmp.mul_(g)
        sum_num = tmp.sum() * (ratio * dlr)
        m.mul_(b1).addcmul_(g, d * (1 - b1))
        torch.mul(g, g, out=tmp)
        v.mul_(b2).addcmul_(tmp, d * d * (1 - b2))
        s.mul_(b3).addcmul_(g, ratio * dlr)
        denom = s.abs().sum()
        numerator = T["numerator"] * b3 + sum_num
        d_hat = numerator / denom
        d_new = torch.where(d == d0, torch.maximum(d, d_hat), d)
        d_max = torch.maximum(T["d_max"], d_hat)
        d_new = torch.minimum(d_max, d_new * 1.0)
        torch.sqrt(v, out=tmp)
        tmp.add_(d_new * eps)
        torch.div(m, tmp, out=tmp)
        p.mul_(1 - wd * dlr).addcmul_(tmp, -dlr)
        T["numerator"].copy_(numerator)
        T["d_max"].copy_(d_max)
        d.copy_(d_new)
        return status

    entries = {"adamw": adamw, "prodigy": prodigy, "prodigy, torch": prodigy_torch}
    graphs = {}
    for name, fn in entries.items():  # --launches steps of one route recorded once: replays issue them with no host in between
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
    assert all(bool(torch.isfinite(st["p"]).all()) for st in (A, K, T))
    d_kernel, d_torch = float(K["scalars"][0]), float(T["d"])
    assert d_kernel > d0 and abs(d_kernel / d_torch - 1) < 1e-3, (d_kernel, d_torch)  # (the two routes ran the same algorithm)
    print(f"d after the run: kernels {d_kernel:.6g}, torch ops {d_torch:.6g}", flush=True)
    print(f"medians, device us per optimizer step (norm included) over {n} elements (replayed graphs of {a.launches} steps, "
          f"{a.replays} replays a repetition): " + "; ".join(f"{k} {spread(v)}" for k, v in times.items()), flush=True)
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
    knobs = {"lr": 1e-4} if a.optimizer == "adamw" else {"lr": 1.0, "optimizer": a.optimizer}
    trainer = LoraTrainer(unet, None, capture_graph=True, v_prediction=cfg["v_prediction"], **knobs)
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
    variants = {"parent": ["--root", os.path.abspath(a.parent_root)], "adamw": [], "prodigy": ["--optimizer", "prodigy"]}
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
    ap.add_argument("--launches", type=int, default=200, help="optimizer steps of a route in one recorded graph")
    ap.add_argument("--replays", type=int, default=20, help="replays of that graph per repetition")
    ap.add_argument("--step", action="store_true", help="one process: the replayed headline step")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--optimizer", default="adamw", choices=("adamw", "prodigy"))
    ap.add_argument("--root", default=ROOT, help="with --step: the checkout whose package and bench.py are imported")
    ap.add_argument("--pairs", type=int, default=None, metavar="N", help="N rounds of parent / adamw / prodigy processes")
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
