"""Same-process A/B of the text encoder's attention: transformers' stock CLIPAttention path (view/transpose ×3, SDPA,
reshape().contiguous()) against the causal HIP core behind `set_use_hip_attention` (csrc/attn_causal.hip).

Builds bench.build_text_encoder for both kinds the benchmark trains through —
  clip-l-lora    CLIP-L shape, LoRA r = 8 on the CLIPAttention projections, batch 4 (BASELINE config 3)
  openclip-h-ti  OpenCLIP-H shape, frozen but for its token table, batch 1 (BASELINE config 5)
— and times forward + backward of `text_encoder(ids)[0]` with the switch off and on, alternating the two settings in one
process on one device (N alternations after a warm-up of both: 6 rounds of 50 passes per setting — a shorter one left the
first alternations on unsettled clocks), each sample the mean of `--iters` passes between two device
events.  Reports the median, min and max of the per-alternation samples and the median of the paired ratios.

    python tools/text_attention_ab.py [--alternations 7] [--iters 20] [--dtype f16]
    python tools/text_attention_ab.py --once off|on --kind clip-l-lora     # a few passes of ONE setting, for a kernel trace
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from diffusion_finetuning_amd.attention import set_use_hip_attention  # noqa: E402

KINDS = {"clip-l-lora": 4, "openclip-h-ti": 1}  # kind → batch


def build(kind, dtype):
    te = bench.build_text_encoder("cuda", dtype, 8, kind=kind)
    g = torch.Generator().manual_seed(1000)
    ids = torch.randint(2, 49000, (KINDS[kind], 77), generator=g)
    ids[:, 0], ids[:, 24:] = 49406, 49407  # caption-shaped, as bench.synthetic_steps
    go = torch.randn(KINDS[kind], 77, te.config.hidden_size, generator=g).to(dtype)
    return te, ids.cuda(), go.cuda()


def one_pass(te, ids, go):
    out = te(ids)[0]
    out.backward(go)
    for p in te.parameters():
        p.grad = None


def timed(te, ids, go, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        one_pass(te, ids, go)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6, help="warm-up rounds per model: 50 passes of each setting per round")
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16"])
    ap.add_argument("--once", choices=["off", "on"])
    ap.add_argument("--kind", default="clip-l-lora", choices=sorted(KINDS))
    args = ap.parse_args()
    dtype = torch.float16 if args.dtype == "f16" else torch.bfloat16
    if args.once:
        te, ids, go = build(args.kind, dtype)
        layers = set_use_hip_attention(te, args.once == "on")
        for _ in range(3):
            one_pass(te, ids, go)
        torch.cuda.synchronize()
        print(f"{args.kind} switch {args.once} ({layers} CLIPAttention modules switched): 3 forward+backward passes")
        return
    print(f"device {torch.cuda.get_device_name(0)}, {args.dtype}, {args.alternations} alternations × {args.iters} passes after {args.warmup} × 2 × 50 warm-up passes, "
          "ms per forward+backward of text_encoder(ids)[0]")
    for kind in KINDS:
        te, ids, go = build(kind, dtype)
        for on in (False, True) * args.warmup:  # warm-up of both settings, long enough for the clocks to settle
            set_use_hip_attention(te, on)
            timed(te, ids, go, 50)
        off, hip = [], []
        for _ in range(args.alternations):
            set_use_hip_attention(te, False)
            off.append(timed(te, ids, go, args.iters))
            set_use_hip_attention(te, True)
            hip.append(timed(te, ids, go, args.iters))
        set_use_hip_attention(te, False)
        ratios = [h / o for h, o in zip(hip, off)]
        for name, xs in (("stock", off), ("hip  ", hip)):
            print(f"{kind:14s} batch {KINDS[kind]} {name}: median {statistics.median(xs):.3f}  min {min(xs):.3f}  "
                  f"max {max(xs):.3f}  samples {' '.join(f'{x:.3f}' for x in xs)}")
        print(f"{kind:14s} hip / stock, paired: median {statistics.median(ratios):.3f}  min {min(ratios):.3f}  "
              f"max {max(ratios):.3f}")
        del te


if __name__ == "__main__":
    main()
