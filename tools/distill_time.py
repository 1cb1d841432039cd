"""Time of svd_distill (lora_diffusion/cli_svd.py:29-111) on the HIP kernels against the reference's per-layer
torch.linalg.svd loop, at full size: the SD1.5 harness UNet's 144 target linears and a CLIP-L-shaped encoder's 48, fp16.
No fine-tuned checkpoints exist offline, so tuned = base + a synthetic difference per layer,
    D = G1·diag(σ)·G2ᵀ + floor·G3   (G Gaussian, scaled to near-orthonormal columns; σ_i = s·i^-p for i <= 64)
with p cycling over the three spectrum families 0.3, 0.5, 1.0 layer by layer and a noise floor of 1e-3·σ_1/√max(N,K).
Reports, as one JSON line and a readable table:
  - end-to-end time of distill_lora per model (UNet, text encoder) and the kernel launches issued;
  - per-phase time of one iteration over all layers (diff-GEMM Y = D·V, Z = Dᵀ·U, both Rayleigh–Ritz sides, finalize),
    each the median of --reps event-timed launches;
  - the iteration histogram per spectrum family;
  - achieved bandwidth of each diff-GEMM pass (both models' target weights read once) against 8 TB/s;
  - the yardstick: the reference's loop (fp16 subtraction, .float(), torch.linalg.svd, quantile, clamp per layer) on the same GPU.

    python tools/distill_time.py [--rank 4] [--reps 5] [--no-yardstick]

--rank takes 1..64: ranks up to 16 time the width-32 kernels, ranks 17–64 the wide ones (the JSON line carries the width).
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffusion_finetuning_amd import _native as nat  # noqa: E402
from diffusion_finetuning_amd import distill as dl  # noqa: E402

FAMILIES = (0.3, 0.5, 1.0)
HBM_TBS = 8.0


def sd15_unet_targets():
    from harness.unet import UNet2DConditionModel, sd15_config

    with torch.device("meta"):
        u = UNet2DConditionModel(sd15_config())
    return [tuple(w.shape) for w in dl.extract_linear_weights(u, dl.UNET_TARGETS)]


def clip_l_targets():
    return [(768, 768)] * 48  # 12 layers × q/k/v/out_proj


def synth(shapes, gen_seed, dev):
    g = torch.Generator(device=dev).manual_seed(gen_seed)
    w0s, w1s, fams = [], [], []
    for i, (N, K) in enumerate(shapes):
        p = FAMILIES[i % len(FAMILIES)]
        k = 64
        sig = (torch.arange(1, k + 1, device=dev, dtype=torch.float32) ** -p) * 0.5
        g1 = torch.randn(N, k, generator=g, device=dev) / N ** 0.5
        g2 = torch.randn(K, k, generator=g, device=dev) / K ** 0.5
        d = (g1 * sig) @ g2.T + torch.randn(N, K, generator=g, device=dev) * (1e-3 * 0.5 / max(N, K) ** 0.5)
        w0 = (torch.randn(N, K, generator=g, device=dev) * 0.02).half()
        w0s.append(w0)
        w1s.append((w0.float() + d).half())
        fams.append(p)
    return w0s, w1s, fams


class Holder(torch.nn.Module):
    def __init__(self, ws):
        super().__init__()
        self.lins = torch.nn.ModuleList()
        for w in ws:
            lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=False, device="meta")
            lin.weight = torch.nn.Parameter(w, requires_grad=False)
            self.lins.append(lin)


def model(ws):
    m = torch.nn.Module()
    m.attn = type("CrossAttention", (Holder,), {})(ws)
    return m


def event_ms(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def phases(w1s, w0s, r, reps):
    kern = nat.DistillKernels(r)
    plan = dl._plan(w1s, w0s, kern)
    t, ws, L, rows = plan["table"], plan["ws"], len(plan["rows"]), plan["rows"]
    max_n, max_k = max(x[2] for x in rows), max(x[3] for x in rows)
    min_nk = min(min(x[2], x[3]) for x in rows)
    res = {
        "start": event_ms(lambda: kern.start(t, L, min_nk, 0, ws), reps),
        "diff_Y=DV": event_ms(lambda: kern.diff(t, L, max_n, False, torch.float16, ws), reps),
        "rr_left": event_ms(lambda: kern.rayleigh_ritz(t, L, 1, 0.0, False, ws), reps),
        "diff_Z=DtU": event_ms(lambda: kern.diff(t, L, max_k, True, torch.float16, ws), reps),
        "rr_right": event_ms(lambda: kern.rayleigh_ritz(t, L, 2, 0.0, False, ws), reps),
        "finalize": event_ms(lambda: kern.finalize(t, L, 0.99, ws, plan["out"]), reps),
    }
    nbytes = sum(2 * 2 * x[2] * x[3] for x in rows)
    bw = {k: nbytes / (res[k] * 1e-3) / 1e12 for k in ("diff_Y=DV", "diff_Z=DtU")}
    return res, bw, nbytes


def yardstick(w1s, w0s, r, q=0.99):
    """The reference's loop body (cli_svd.py:66-85) timed once per distinct shape after one warm-up call, times the number of
    layers of that shape (the full loop over 144 UNet layers with full_matrices SVDs would take minutes)."""
    def body(a, b):
        mat = (a - b).float()
        U, S, Vh = torch.linalg.svd(mat)
        U = U[:, :r] @ torch.diag(S[:r])
        Vh = Vh[:r, :]
        hi = torch.quantile(torch.cat([U.flatten(), Vh.flatten()]), q)
        return U.clamp(-hi, hi), Vh.clamp(-hi, hi)

    first = {}
    for i, w in enumerate(w0s):
        first.setdefault(tuple(w.shape), i)
    total, per_shape = 0.0, {}
    with torch.no_grad():
        for shape, i in first.items():
            body(w1s[i], w0s[i])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            body(w1s[i], w0s[i])
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            n = sum(1 for w in w0s if tuple(w.shape) == shape)
            per_shape[f"{shape[0]}x{shape[1]}"] = {"ms": ms, "layers": n}
            total += ms * n
    return total, per_shape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"rank": a.rank, "width": nat.distill_width(a.rank), "gpu": torch.cuda.get_device_name(0)}
    for name, shapes, seed in (("unet", sd15_unet_targets(), 1), ("text_encoder", clip_l_targets(), 2)):
        w0s, w1s, fams = synth(shapes, seed, dev)
        base, tuned = model(w0s), model(w1s)
        dl.distill_lora(tuned, base, ["CrossAttention"], rank=a.rank)  # warm-up (module load, allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        import warnings
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            _, info = dl.distill_lora(tuned, base, ["CrossAttention"], rank=a.rank, return_info=True)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        hist = {str(p): dict(sorted(collections.Counter(it for it, f in zip(info["iters"], fams) if f == p).items()))
                for p in FAMILIES}
        ph, bw, nbytes = phases(w1s, w0s, a.rank, a.reps)
        rec = {"layers": len(shapes), "distill_ms": total, "launches": info["launches"], "iters_by_family": hist,
               "unconverged": len(info["unconverged"]), "warnings": len(caught), "phase_ms": ph,
               "diff_pass_bytes": nbytes, "diff_pass_TBs": bw, "diff_pass_frac_of_8TBs": {k: v / HBM_TBS for k, v in bw.items()},
               "max_residual": max(info["residual"])}
        if not a.no_yardstick:
            rec["yardstick_svd_loop_ms"], rec["yardstick_per_shape"] = yardstick(w1s, w0s, a.rank)
        out[name] = rec
        del base, tuned, w0s, w1s
        torch.cuda.empty_cache()
    for name in ("unet", "text_encoder"):
        r = out[name]
        print(f"{name}: {r['layers']} layers, distill {r['distill_ms']:.1f} ms ({r['launches']} launches), "
              f"yardstick {r.get('yardstick_svd_loop_ms', float('nan')):.1f} ms; iterations by family {r['iters_by_family']}; "
              f"phases (ms) {json.dumps({k: round(v, 3) for k, v in r['phase_ms'].items()})}; diff passes "
              f"{json.dumps({k: round(v, 2) for k, v in r['diff_pass_TBs'].items()})} TB/s", flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
