"""Per-class timing of the UNet's frozen 3×3 stride-1 convolutions with many pixels: stock F.conv2d against both HIP families.

    python tools/conv_large_sweep.py [--configs 4x64] [--min-pixels 4096] [--max-pixels 16384] [--calls 32] [--replays 20] [--out FILE]
                                     [--only PIXELSxCINxCOUT,...] [--large-only]

The method is that of tools/conv_small_sweep.py (whose docstring explains it): for every eligible (pixels, C_in, C_out) of the
given workloads, µs per call of each side, forward and backward-data, f16, inside a replayed graph of `--calls` calls going
round about `--weight-mb` MB of distinct filters, the median of `--replays` replays; the stock side with
`torch.backends.cudnn.benchmark` on and the shipped find-db, so its figure covers all of its launches.  `small` is
csrc/conv_small.hip, `large` csrc/conv_large.hip, both on the same packs.  A class belongs in `conv3x3_large_plan` only if the
large kernel beats the stock call in BOTH directions (`wins`); `plan` says what the two planners do now.

`large` is the channel-heavy tile the shape rule gives (`conv3x3_large_tile(..., 0)`), `t256` and `t128` the pixel-heavy tiles
256 × 80 and 128 × 80 (tiles 1 and 2; `nan` where a tile's conditions fail).  `±` is the largest spread (max − min of the
replays) among the large columns of that direction.  `tile` names the pixel-heavy tile that is faster than `large` in BOTH
directions by more than that spread (the faster of the two if both are; 0: none): what the measured table of
csrc/conv_large.hip may hold.  `now` is the tile `conv3x3_large` runs at present, forward/backward
(`conv3x3_large_tile_choice`).  `--only` restricts the classes, `--large-only` skips the stock
and small columns (diagnostic builds of the large kernel)."""
import argparse
import faulthandler
import glob
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    from conv_small_sweep import unet_classes

    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4x64", help="batch x latent size of the workloads to cover")
    ap.add_argument("--min-pixels", type=int, default=4096)
    ap.add_argument("--max-pixels", type=int, default=16384)
    ap.add_argument("--calls", type=int, default=32)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--weight-mb", type=int, default=600, help="distinct filter bytes a graph cycles through (0: one filter)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="comma-separated PIXELSxCINxCOUT classes to time (default: all)")
    ap.add_argument("--large-only", action="store_true", help="time only the large kernel's columns")
    args = ap.parse_args()
    faulthandler.enable()

    db = tempfile.mkdtemp(prefix="dfa_miopen_db_")
    for f in glob.glob(os.path.join(ROOT, "harness", "miopen_db", "*.txt")):
        shutil.copy(f, db)
    os.environ.setdefault("MIOPEN_USER_DB_PATH", db)

    import torch
    import torch.nn.functional as F

    from diffusion_finetuning_amd import _native as nat

    torch.backends.cudnn.benchmark = True
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        """µs per call of fn inside a replayed graph of args.calls calls."""
        for i in range(2):
            fn(i)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                for i in range(args.calls):
                    fn(i)
        torch.cuda.current_stream().wait_stream(side)
        graph.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.replays):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / args.calls)
        ts.sort()
        return ts[len(ts) // 2], ts[-1] - ts[0]

    cases = set()
    for batch, latent in (tuple(int(v) for v in c.split("x")) for c in args.configs.split(",")):
        for level, cin, cout in unet_classes():
            side = latent >> level
            if args.min_pixels <= batch * side * side <= args.max_pixels:
                cases.add((batch, side, cin, cout))
    say(f"# conv_large sweep: f16, graph of {args.calls} calls over ~{args.weight_mb} MB of distinct filters, median of "
        f"{args.replays} replays, µs per call")
    say(f"# {'N':>2} {'HxW':>7} {'pixels':>6} {'C_in':>5} {'C_out':>5} | {'fwd stock':>9} {'small':>8} {'large':>8} {'t256':>8} "
        f"{'t128':>8} {'±':>5} | {'bwd stock':>9} {'small':>8} {'large':>8} {'t256':>8} {'t128':>8} {'±':>5} | wins plan  | tile now")
    only = {tuple(int(v) for v in c.split("x")) for c in args.only.split(",") if c}
    nan = (float("nan"), 0.0)
    for batch, side, cin, cout in sorted(cases, key=lambda c: (c[0] * c[1] * c[1], c[2], c[3], c[0])):
        if not (nat.conv3x3_large_supported(batch, cin, cout, side, side, torch.float16) and
                nat.conv3x3_large_supported(batch, cout, cin, side, side, torch.float16)):
            continue
        pixels = batch * side * side
        if only and (pixels, cin, cout) not in only:
            continue
        x = torch.randn(batch, cin, side, side, device=dev, dtype=torch.float16)
        dy = torch.randn(batch, cout, side, side, device=dev, dtype=torch.float16)
        nw = max(1, min(args.calls, (args.weight_mb << 20) // (cin * cout * 18)))
        ws = [torch.randn(cout, cin, 3, 3, device=dev, dtype=torch.float16) * 0.01 for _ in range(nw)]
        fwd = [nat.conv3x3_small_pack(w, False) for w in ws]
        bwd = [nat.conv3x3_small_pack(w, True) for w in ws]
        stock = not args.large_only
        t_fs = timed(lambda i: F.conv2d(x, ws[i % nw], None, padding=1))[0] if stock else nan[0]
        t_bs = timed(lambda i: torch.ops.aten.convolution_backward(dy, x, ws[i % nw], None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                                   [True, False, False]))[0] if stock else nan[0]
        small = stock and nat.conv3x3_small_supported(batch, cin, cout, side, side, torch.float16) and \
            nat.conv3x3_small_supported(batch, cout, cin, side, side, torch.float16)
        t_fh = timed(lambda i: nat.conv3x3_small(x, fwd[i % nw], None, cout))[0] if small else nan[0]
        t_bh = timed(lambda i: nat.conv3x3_small(dy, bwd[i % nw], None, cin))[0] if small else nan[0]

        def tile_ok(tile):
            mt = {1: 256, 2: 128}[tile]
            return side % 8 == 0 and mt % side == 0 and (side * side) % mt == 0 and 2 * side <= mt

        t_f = [timed(lambda i, t=t: nat.conv3x3_large_tile(x, fwd[i % nw], None, cout, t)) if t == 0 or tile_ok(t) else nan
               for t in range(3)]
        t_b = [timed(lambda i, t=t: nat.conv3x3_large_tile(dy, bwd[i % nw], None, cin, t)) if t == 0 or tile_ok(t) else nan
               for t in range(3)]
        sp_f, sp_b = max(v[1] for v in t_f), max(v[1] for v in t_b)
        (t_fl, _), (t_bl, _) = t_f[0], t_b[0]
        wins = t_fl < t_fs and t_bl < t_bs
        plan = "small" if nat.conv3x3_small_plan(pixels, cin, cout, torch.float16) else \
            "large" if nat.conv3x3_large_plan(pixels, cin, cout, torch.float16) else "stock"
        better = [t for t in (1, 2) if t_fl - t_f[t][0] > sp_f and t_bl - t_b[t][0] > sp_b]  # (nan compares false)
        tile = min(better, key=lambda t: t_f[t][0] + t_b[t][0]) if better else 0
        now = "/".join(str(nat.conv3x3_large_tile_choice(batch, a, b, side, side, torch.float16)) for a, b in ((cin, cout), (cout, cin)))
        say(f"  {batch:>2} {side:>3}x{side:<3} {pixels:>6} {cin:>5} {cout:>5} | {t_fs:>9.1f} {t_fh:>8.1f} {t_fl:>8.1f} {t_f[1][0]:>8.1f} "
            f"{t_f[2][0]:>8.1f} {sp_f:>5.1f} | {t_bs:>9.1f} {t_bh:>8.1f} {t_bl:>8.1f} {t_b[1][0]:>8.1f} {t_b[2][0]:>8.1f} {sp_b:>5.1f} | "
            f"{'yes' if wins else 'no':>4} {plan:<5} | {tile:>4} {now:>3}")
        del x, dy, ws, fwd, bwd
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    shutil.rmtree(db, ignore_errors=True)


if __name__ == "__main__":
    main()
