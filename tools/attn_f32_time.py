"""µs per launch of the fp32 attention core (csrc/attn_f32.hip) per shape class, next to the stock fp32 composite the harness
UNet runs (harness.unet._attention_core: SDPA on padded [B,H,T,D] tensors) on the same tensors, and the achieved TF against
the 155 TF f32 matrix peak.  Forward, dQ and dK/dV come from the library's launch profiler (event pairs on the dispatches);
the stock forward / backward from event pairs around the calls.  Prints one JSON line per shape.

    python tools/attn_f32_time.py [--iters 10]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffusion_finetuning_amd import _native as nat  # noqa: E402
from diffusion_finetuning_amd.sandwich import f32_attention  # noqa: E402
from harness.unet import _attention_core  # noqa: E402

SHAPES = [(1, 9216, 9216, 5, 64), (1, 2304, 2304, 10, 64), (1, 9216, 77, 5, 64), (1, 1024, 1024, 8, 40)]
PEAK_TF = 155.0


def _events(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    for B, Tq, Tk, H, d in SHAPES:
        g = torch.Generator().manual_seed(0)
        q, k, v, go = (torch.randn(B, T, H * d, generator=g).cuda().requires_grad_(r)
                       for T, r in ((Tq, True), (Tk, True), (Tk, True), (Tq, False)))
        out = {"shape": [B, Tq, Tk, H, d]}
        for name, fn in (("core", lambda: f32_attention(q, k, v, H)), ("stock", lambda: _attention_core(q, k, v, H))):
            o = fn()
            out[name + "_fwd_us"] = round(_events(fn, args.iters), 1)
            out[name + "_bwd_us"] = round(_events(lambda: torch.autograd.grad(o, (q, k, v), go, retain_graph=True), args.iters), 1)
        nat.prof_enable(4096)
        for _ in range(args.iters):
            torch.autograd.grad(f32_attention(q, k, v, H), (q, k, v), go)
        torch.cuda.synchronize()
        prof = nat.prof_collect()
        nat.prof_enable(0)
        flop = 4.0 * B * H * Tq * Tk * d  # forward: two products
        for kind, mult in (("attn_flash_fwd_kernel", 1.0), ("attn_flash_dq_kernel", 1.5), ("attn_flash_dkdv_kernel", 2.0)):
            hit = [v_ for k_, v_ in prof.items() if k_ == kind]
            if hit:
                us = hit[0]["ms"] * 1e3 / hit[0]["launches"]
                tag = kind[len("attn_flash_"):-len("_kernel")]  # the fp32 core reports under the long-context core's kinds
                out[tag + "_us"] = round(us, 1)
                out[tag + "_TF"] = round(flop * mult / us / 1e6, 1)
                out[tag + "_of_peak"] = round(flop * mult / us / 1e6 / PEAK_TF, 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
