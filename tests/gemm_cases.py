"""Which fused-GEMM kernels a single-layer launch can reach, and the smallest shapes that reach each of them.

No GPU and no library: tests/test_gpu_gemm_edges.py runs every entry against float64 math inside guard bands;
tests/test_gemm_coverage_host.py checks on the CPU that the keys are exactly the `launch_tile` instantiations that
`launch_pipe` / `launch_typed` of csrc/lora_gemm.hip hand out for a single-layer launch, that the mirrors below send
every table shape to its key, and that the mirrors still copy the C++ they were written from.

A key is (path, BM, BN, STG, S):
  path  "ring"      lora_gemm_kernel<T, BM, BN, true, STG>           the LDS-DMA ring (contraction a whole number of K-steps)
        "fallback"  lora_gemm_kernel<T, 64, 64, true, 0>             the register-staged loop (ragged contraction)
        "generic"   lora_skinny_generic_kernel + lora_gemm_generic_kernel   (sizes or pointers that are not 16-byte whole)
        "split"     lora_gemm_kernel<T, BM, 128, true, STG, …, SPLITK>     the contraction cut into S slices inside the launch
  S     the slice count of the table's shape (1 unless split).  A CLASS is key[:4]: the slice count is a launch parameter,
        not an instantiation, so the coverage checks compare classes.
A shape is (M, Kc, Nc) of C[M,Nc] = Am[M,Kc]·Bm[Nc,Kc]ᵀ, or (M, Kc, Nc, False) when Am is handed over one element off a
16-byte boundary.  CASES[esize][key] lists the variants of a class, the smallest first; every ring and split class has a
ragged last row tile, and a ragged last column tile where its dispatch rule admits one (64×128 behind three stages wants
Nc % 128 == 0, the 160-wide tiles want Nc % 160 == 0).  Grouped launches, equal parts, the GEGLU gate and the part-wise
backward stay out: tests/test_gpu_groups.py and tests/test_gpu_geglu.py own those.
"""
import torch

RING, FALLBACK, GENERIC, SPLIT = "ring", "fallback", "generic", "split"
ROW_BYTES = 128       # kRowBytes (csrc/lora_gemm_kernel.h): one K-step of one tile row
TICKET_BYTES = 4096   # LORA_GEMM_WS_TICKET_BYTES
ESIZE = {torch.float32: 4, torch.float16: 2, torch.bfloat16: 2}
DTYPES = {2: (torch.float16, torch.bfloat16), 4: (torch.float32,)}


def plan_splitk(M, Kc, Nc, esize):
    """(S, bm) of plan_splitk() in csrc/lora_gemm.hip."""
    off = (1, 128)
    nk = (Kc * esize + ROW_BYTES - 1) // ROW_BYTES
    tiles128 = ((M + 127) // 128) * ((Nc + 127) // 128)
    tiles64 = ((M + 63) // 64) * ((Nc + 127) // 128)
    if (Nc & 7) != 0 or (Kc * esize) % ROW_BYTES != 0 or tiles128 >= 192:
        return off
    if nk < 48:
        return off
    bm = 64 if tiles128 <= 96 else 128
    if tiles128 >= 64 and nk >= 128:
        bm = 128
    tiles = tiles64 if bm == 64 else tiles128
    if tiles > TICKET_BYTES // 4:
        return off
    S = min((480 + tiles // 2) // tiles, 8)
    while S > 1 and nk // S < 10:
        S -= 1
    while S > 1 and (S - 1) * ((nk + S - 1) // S) >= nk:
        S -= 1
    return S, bm


def gate_tile_width(tiles_m, cols):
    """gate_tile_width(tiles_m, cols, gated=false): the round-count model of the ungated launches."""
    if cols % 160 != 0:
        return 128
    t128, t160 = tiles_m * (cols // 128), tiles_m * (cols // 160)
    c128, c160 = float((t128 + 511) // 512), 1.25 * float((t160 + 511) // 512)
    return 160 if c160 < c128 else 128


def gemm_launch_class(M, Kc, Nc, esize, aligned=True, workspace=True):
    """Key of the MAIN launch of a single layer (rank <= 16, packed factors given): the `fast` condition and the
    workspace condition of launch_typed, plan_splitk, and launch_pipe<T, true> with n_parts == 0 and no tile_part."""
    vec, bk = 16 // esize, ROW_BYTES // esize
    if not (aligned and Kc % vec == 0 and Nc % vec == 0):
        return (GENERIC, 0, 0, 0, 1)
    if Kc % bk != 0:
        return (FALLBACK, 64, 64, 0, 1)
    if workspace:  # (the wrapper sizes it with lora_gemm_workspace_bytes, i.e. for this very plan)
        S, bm = plan_splitk(M, Kc, Nc, esize)
        if S > 1:
            return (SPLIT, 64, 128, 3, S) if bm == 64 else (SPLIT, 128, 128, 2, S)
    tiles128 = ((M + 127) // 128) * ((Nc + 127) // 128)
    tiles64 = ((M + 63) // 64) * ((Nc + 63) // 64)
    padded = (Nc + 127) // 128 * 128
    big = tiles128 >= 128 and (padded - Nc) * 4 <= Nc
    if esize == 2:
        tiles160 = ((M + 127) // 128) * (Nc // 160)
        w160 = Nc % 160 == 0 and Nc % 128 != 0 and tiles160 >= 128
        if w160 and tiles160 < 384:
            return (RING, 64, 160, 2, 1)
        if w160:
            return (RING, 128, 160, 2, 1)
        if big and tiles128 < 256:
            return (RING, 64, 128, 2, 1)
        if not big and tiles128 >= 64 and Nc % 128 == 0:
            return (RING, 64, 128, 3, 1)
        if big and tiles128 >= 256 and gate_tile_width((M + 127) // 128, Nc) == 160:
            return (RING, 128, 160, 2, 1)
    if big:
        return (RING, 128, 128, 2, 1)
    deep = tiles64 < 512
    nk = (Kc * esize + ROW_BYTES - 1) // ROW_BYTES
    ring = 3 if deep else 2
    if deep and nk >= 8:
        ring = 4
    return (RING, 64, 64, ring, 1)


def skinny_launch_class(M, Kc, esize, aligned=True):
    """Key of the skinny launch (P = Am·Fᵀ alone: lora_linear_bwd_input without dX): launch_pipe<T, false>, the
    fallback loop, or the generic kernel.  No output width enters the choice."""
    vec, bk = 16 // esize, ROW_BYTES // esize
    if not (aligned and Kc % vec == 0):
        return (GENERIC, 0, 0, 0, 1)
    return (RING, 64, 64, 3, 1) if Kc % bk == 0 else (FALLBACK, 64, 64, 0, 1)


CASES = {
    2: {
        # 64×64: three stages with one, two and three K-steps (the prologue issues two: the last step is also the first),
        # four stages from eight K-steps on, two stages once 512 tiles overlap each other (too much padding for `big`)
        (RING, 64, 64, 3, 1): ((65, 64, 72), (65, 128, 72), (65, 192, 72)),
        (RING, 64, 64, 4, 1): ((65, 512, 72), (65, 576, 72)),
        (RING, 64, 64, 2, 1): ((16330, 64, 72),),
        (RING, 64, 128, 3, 1): ((2000, 128, 512),),
        (RING, 64, 128, 2, 1): ((2000, 128, 1000),),    # `big` with 24 padding columns in the last column tile
        (RING, 128, 128, 2, 1): ((4000, 128, 1000),),
        (RING, 64, 160, 2, 1): ((8100, 128, 320),),
        (RING, 128, 160, 2, 1): ((8100, 128, 960), (13100, 64, 640)),  # by width, and by the round-count rule
        (FALLBACK, 64, 64, 0, 1): ((130, 40, 200), (130, 72, 200), (130, 136, 200)),
        (GENERIC, 0, 0, 0, 1): ((70, 50, 72), (70, 64, 50), (70, 64, 72, False)),
        (SPLIT, 64, 128, 3, 5): ((100, 3392, 136),),    # 53 K-steps: slices of 11, 11, 11, 11, 9
        (SPLIT, 128, 128, 2, 4): ((1600, 3136, 1000),),  # 49 K-steps: slices of 13, 13, 13, 10
    },
    4: {  # f32 never enters launch_pipe's sizeof(T) == 2 block: no 160-wide tile, no unsplit 64×128
        (RING, 64, 64, 3, 1): ((65, 32, 68), (65, 64, 68), (65, 96, 68)),
        (RING, 64, 64, 4, 1): ((65, 256, 68), (65, 288, 68)),
        (RING, 64, 64, 2, 1): ((16330, 32, 68),),
        (RING, 128, 128, 2, 1): ((2000, 32, 1000), (2000, 64, 1000)),
        (FALLBACK, 64, 64, 0, 1): ((130, 36, 200), (130, 44, 200), (130, 68, 200)),
        (GENERIC, 0, 0, 0, 1): ((70, 50, 72), (70, 64, 50), (70, 64, 72, False)),
        (SPLIT, 64, 128, 3, 5): ((100, 1696, 136),),
        (SPLIT, 128, 128, 2, 4): ((1600, 1568, 1000),),
    },
}

# (M, Kc[, aligned]) of the skinny launch; the ring is three stages deep whatever the contraction: one, two and four K-steps
SKINNY_CASES = {
    2: {
        (RING, 64, 64, 3, 1): ((65, 64), (130, 128), (65, 256)),
        (FALLBACK, 64, 64, 0, 1): ((130, 40), (65, 136)),
        (GENERIC, 0, 0, 0, 1): ((70, 50), (70, 64, False)),
    },
    4: {
        (RING, 64, 64, 3, 1): ((65, 32), (130, 64), (65, 128)),
        (FALLBACK, 64, 64, 0, 1): ((130, 36), (65, 68)),
        (GENERIC, 0, 0, 0, 1): ((70, 50), (70, 64, False)),
    },
}


def class_of(shape, esize, workspace=True):
    return gemm_launch_class(shape[0], shape[1], shape[2], esize, aligned=len(shape) < 4 or shape[3], workspace=workspace)


def skinny_class_of(shape, esize):
    return skinny_launch_class(shape[0], shape[1], esize, aligned=len(shape) < 3 or shape[2])


def make_layer(M, K, N, r, dtype, seed, bias=True):
    """Operands of one LoRA layer as tests/test_gpu_parity.py's SD-shape sweep draws them, rounded to `dtype` FIRST so the
    reference sees what the kernel sees: x [M,K], w [N,K], b [N] | None, down [r,K] and up [N,r] (fp32 masters holding
    `dtype` values), dy [M,N]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = ((torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5).to(dtype)
    b = (torch.randn(N, generator=g) * 0.1).to(dtype)
    down = (torch.randn(r, K, generator=g) / r).to(dtype).float()
    up = (torch.randn(N, r, generator=g) * 0.05).to(dtype).float()
    dy = torch.randn(M, N, generator=g).to(dtype)
    return x, w, (b if bias else None), down, up, dy


def make_factors(K, N, r, dtype, seed):
    """down [r,K] and up [N,r] alone, drawn and rounded as make_layer draws them."""
    g = torch.Generator().manual_seed(seed)
    down = (torch.randn(r, K, generator=g) / r).to(dtype).float()
    up = (torch.randn(N, r, generator=g) * 0.05).to(dtype).float()
    return down, up
