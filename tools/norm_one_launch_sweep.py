"""Dev tool: times the NCHW GroupNorm entry points per size class inside a replayed graph, the regime of the training step.

The planner of csrc/norm.hip chooses the form from the shape, so the two forms are compared as two dev builds of the library on
the same box, one process each (NORM_ONE_FORCE: 1 = one launch wherever the registers allow, 0 = two launches everywhere):
    python -m diffusion_finetuning_amd.build_native --variant one -DNORM_ONE_FORCE=1
    python -m diffusion_finetuning_amd.build_native --variant two -DNORM_ONE_FORCE=0
    DFA_LIB_PATH=.../lib/liblora_hip_one.so python tools/norm_one_launch_sweep.py
    DFA_LIB_PATH=.../lib/liblora_hip_two.so python tools/norm_one_launch_sweep.py
Without DFA_LIB_PATH it times the library as shipped, planner included.
Each figure is the best of 5 replays of a graph of 40 identical calls, divided by 40 (µs per call, launch floor included).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffusion_finetuning_amd import _native as nat

CALLS, REPLAYS, G = 40, 5, 32
# (C, H): the sd15 sites at 64² latents, the 96² ones of config 5, and the register capacity's edge (C/G·H²/8 = 8192 chunks)
SITES = [(1280, 8), (2560, 8), (640, 16), (1280, 16), (320, 32), (1920, 16), (640, 32), (2560, 16), (960, 32), (320, 64),
         (1280, 32), (1920, 32), (2048, 32), (640, 64), (320, 48), (640, 48), (960, 48), (1280, 24), (320, 96)]


def timed(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    best = 1e9
    for _ in range(REPLAYS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / CALLS)
    return best


def main():
    lib = nat.lib()
    print(f"# {torch.cuda.get_device_name(0)}  lib={os.path.basename(nat.library_path())}", flush=True)
    print("# N C H slab_KB slabs | plan_fwd  identity silu silu+addend (us) | plan_bwd  identity+dh silu+dh silu+addend+da (us)", flush=True)
    for N in (1, 4, 8):
        for C, H in SITES:
            HW, dt = H * H, torch.float16
            x = torch.randn(N, C, H, H, device="cuda").to(dt)
            dy, dh, y, dx = torch.randn_like(x), torch.randn_like(x), torch.empty_like(x), torch.empty_like(x)
            a, da = torch.randn(N, C, device="cuda").to(dt), torch.empty(N, C, device="cuda", dtype=dt)
            w, b = torch.ones(C, device="cuda", dtype=dt), torch.zeros(C, device="cuda", dtype=dt)
            mean, rstd = (torch.empty(N, G, device="cuda") for _ in range(2))
            ws = torch.empty(lib.group_norm_act_workspace_bytes(N, C, HW, G, 0, 1), dtype=torch.uint8, device="cuda")
            p, code = (lambda t: t.data_ptr()), nat.dtype_code(dt)

            def fwd(act, add):
                assert lib.group_norm_act_fwd(p(x), p(a) if add else None, p(w), p(b), p(y), p(mean), p(rstd), p(ws), N, C, HW, G,
                                              1e-5, act, 0, code, nat._stream(x)) == 0

            def bwd(act, res, add):
                assert lib.group_norm_act_bwd_res(p(dy), p(dh) if res else None, p(x), p(a) if add else None, p(w), p(b), p(mean),
                                                  p(rstd), p(dx), p(da) if add else None, p(ws), N, C, HW, G, act, code,
                                                  nat._stream(x)) == 0

            # the variants of the UNet: transformer entry (identity; dh in the backward), ResNet norm1 (SiLU; dh), norm2 (SiLU, addend; da)
            t = [timed(lambda: fwd(0, False)), timed(lambda: fwd(1, False)), timed(lambda: fwd(1, True)),
                 timed(lambda: bwd(0, True, False)), timed(lambda: bwd(1, True, False)), timed(lambda: bwd(1, False, True))]
            print(f"{N} {C} {H} {C // G * HW * 2 / 1024:.0f} {N * G} | {lib.group_norm_act_plan(N, C, HW, G, 0, 0)} {t[0]:.2f} "
                  f"{t[1]:.2f} {t[2]:.2f} | {lib.group_norm_act_plan(N, C, HW, G, 0, 1)} {t[3]:.2f} {t[4]:.2f} {t[5]:.2f}", flush=True)


if __name__ == "__main__":
    main()
