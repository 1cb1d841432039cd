"""Dev tool: times the batched time-embedding projections (csrc/time_proj.hip) against the 66 launches they replace, inside a
replayed graph, at the headline's shape: N = 4, E = 1280, the 22 ResNets of the SD1.5 UNet (20 160 output rows, 51.6 MB of f16
weights).

The weights must not sit in a cache from one call to the next, as in the training step, where a whole UNet pass lies between two
uses: the graph holds SETS calls, each on its own copy of all weights (SETS × 51.6 MB, above the 256 MB of last-level cache), so
every call streams its weights from HBM.  The two forms are replayed alternately, REPS times each; the figures are medians, per
call: µs, and the effective bandwidth of the weight stream.

    python tools/time_proj_time.py
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from diffusion_finetuning_amd import time_proj as tp

N, E, SETS, REPS = 4, 1280, 8, 15
WIDTHS = [320, 320, 640, 640, 1280, 1280, 1280, 1280, 1280, 1280] + [1280] * 6 + [640] * 3 + [320] * 3  # down, mid, up


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def replay_us(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / SETS


def main():
    print(f"# {torch.cuda.get_device_name(0)}  N={N} E={E} layers={len(WIDTHS)} rows={sum(WIDTHS)} sets={SETS} reps={REPS}", flush=True)
    for dtype in (torch.float16, torch.bfloat16):
        gen = torch.Generator(device="cuda").manual_seed(1)
        rn = lambda *s: torch.randn(*s, generator=gen, device="cuda")
        temb = rn(N, E).to(dtype)
        sets = [[((rn(c, E) / E ** 0.5).to(dtype), rn(c).to(dtype), rn(c).to(dtype)) for c in WIDTHS] for _ in range(SETS)]
        assert tp.time_projections_supported(temb, sets[0])
        batched = lambda: [tp.time_projections(temb, layers) for layers in sets]
        stock = lambda: [[F.linear(F.silu(temb), w, b) + cb for w, b, cb in layers] for layers in sets]
        (gb, kb), (gs, ks) = graph_of(batched), graph_of(stock)
        tb, ts = [], []
        for _ in range(REPS):
            tb.append(replay_us(gb))
            ts.append(replay_us(gs))
        mb, ms = statistics.median(tb), statistics.median(ts)
        mbytes = sum(WIDTHS) * E * 2 / 1e6
        print(f"{str(dtype)[6:]}: batched {mb:.2f} us/call ({mbytes / mb:.2f} TB/s over {mbytes:.1f} MB, min {min(tb):.2f} max {max(tb):.2f})"
              f" | 66 stock launches {ms:.2f} us/call (min {min(ts):.2f} max {max(ts):.2f}) | ratio {ms / mb:.1f}", flush=True)


if __name__ == "__main__":
    main()
