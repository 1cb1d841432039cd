"""Case tables, launch mirrors, input builders, float64 references and derived bounds for csrc/optim.hip: the squared-norm
reduction, clip + AdamW (dense and row-aware), the weight merge and the LoRA (+) LoRA interpolation.  Plain data and CPU
torch; tests/test_optim_host.py pins it to the C++ and shows what the bounds reject, tests/test_gpu_optim_edges.py runs it.

u = 2^-24 is the unit roundoff of fp32: one correctly rounded +, -, x or fma has relative error <= u.  sqrtf and / are
counted as 2u (one ulp), whatever the build gives them.  All bounds are first order in u; k and L are rounded UP to whole
numbers, which covers the second-order terms (k·u < 1e-5).

Squared norm (`sqnorm_bound`): every summand (g·mul)² is non-negative, so the relative error of the sum is at most u times
the number of roundings on the longest path from a summand to the result:
    L = 2                      a = g·mul is rounded once and squared
      + 4·iters + tail         the thread's fma chain: 4 per grid-stride iteration, one more for a tail element (block 0)
      + 8                      block_sum_256: 6 butterfly adds in the wave, 2 adds across the 4 waves
      + rounds                 the last block's chain over the partials, ceil(blocks/256) adds per thread
      + 8                      block_sum_256 again
and |norm[0] − Σ(g·mul)²| <= L·u/(1 − L·u) · Σ(g·mul)².

AdamW (`adamw_bounds`), for the operations of adamw_element (csrc/common.h) and of adamw_kernel before it.  The gradient the
element sees, g' = g·(grad_mul·clip), has relative error kg·u:
    no clipping   kg = 1       grad_mul·1 is exact, g·gm rounds once
    clipping      kg = ceil(L/2) + 8:   norm[0] carries L·u, halved by the square root; sqrtf 2; + 1e-6f 1; the fp32 1e-6f
                  against the reference's double 1e-6 at most 1; max_norm/(…) 2; grad_mul·clip 1; g·gm 1
  m' = m + (g' − m)·c1,  c1 = 1 − β1 exact (Sterbenz):  g' − m rounds once, ·c1 once, the sum once, and g' brings kg·u·c1·|g'|:
        |Δm| <= (3 + kg)·u·Mm,                     Mm = |m| + c1·(|g'| + |m|)          (>= |m'|: m' itself may cancel)
  v' = β2·v + (c2·g')·g',  c2 = 1 − β2 exact:  two products on the right and 2·kg·u from g'², one on the left, the sum:
        |Δv| <= (3 + 2·kg)·u·Mv,                   Mv = β2·v + c2·g'²                  (= v', no cancellation)
  p' = p·decay − (lr/bc1)·(m'/denom),  denom = sqrtf(v')/bc2_sqrt + eps:
        denom:   (3 + 2kg)/2 from v', sqrtf 2, bc2_sqrt (a double rounded to fp32) 1, the division 2, + eps 1
        m'/denom 2, lr/bc1 = 1 + 2, the product 1:  the Adam term has (kv/2 + 12)·u of its own size plus Δm carried through
        p·decay: decay = 1 − lr·wd is 2u off (lr·wd <= 0.01), the product 1; the final subtraction 1 on |p'| <= both terms
        |Δp| <= (17.5 + 2·kg)·u·Mp, rounded up,    Mp = |p|·decay + (lr/bc1)·Mm/denom
  A compiler that contracts a product and a sum into an fma removes a rounding; the bounds hold either way.
Each bound gets the smallest normal fp32 number added, so that no test pins how denormal results are handled.

Merge (`merge_emulate`): every step after the fp32 accumulation is a correctly rounded cast, product or sum, restated here
op by op; the accumulation d = Σ_j b_j·a_j (r fmas in sequence) is within e = r·u/(1 − r·u)·Σ|b_j||a_j| of the exact
product.  Every later step is monotone non-decreasing in d (alpha >= 0), so the kernel's result lies between the emulation
run at d − e and at d + e — and equals the one at d unless d is within e of a point where a cast changes.

Lerp (`lerp_emulate`): three IEEE single operations with explicit casts; bit for bit on any host."""
import math

import torch

from oracle import lora_oracle as orc

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126  # smallest normal fp32

# ---- the launch grids of csrc/optim.hip (pinned to its text by tests/test_optim_host.py) ------------------------------
THREADS = 256
SQNORM_MAX_BLOCKS = 1024    # kMaxBlocks
SQNORM_VEC = 4              # float4 loads: nvec = n >> 2, the n % 4 tail on block 0
ADAMW_MAX_BLOCKS = 2048
LERP_MAX_BLOCKS = 2048
ROWS_MAX_BLOCKS = 4096      # one block per row
MERGE_MAX_BLOCKS = 4096
BATCHED_ELEMS_PER_BLOCK = 1024
BATCHED_MAX_BLOCKS = 1024

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NAME = {F32: "f32", F16: "f16", BF16: "bf16"}


def _cdiv(a, b):
    return (a + b - 1) // b


def f32(x):
    """The double that equals x rounded to fp32: what a float argument of the C ABI holds."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def sqnorm_launch(n):
    """lora_grad_sqnorm's grid and the loop counts of grad_sqnorm_kernel."""
    nvec, tail = n // SQNORM_VEC, n % SQNORM_VEC
    blocks = min(max(_cdiv(nvec, THREADS), 1), SQNORM_MAX_BLOCKS)
    stride = blocks * THREADS
    return {"blocks": blocks, "nvec": nvec, "tail": tail,
            "iters": _cdiv(nvec, stride),                           # of the busiest thread
            "threads_in_last_iter": nvec - (_cdiv(nvec, stride) - 1) * stride if nvec else 0,
            "rounds": _cdiv(blocks, THREADS)}                       # the last block's loop over the partials


def sqnorm_class(n):
    lay = sqnorm_launch(n)
    if lay["nvec"] == 0:
        return "tail only"
    if lay["iters"] > 1:
        return "over the cap"
    if lay["blocks"] == SQNORM_MAX_BLOCKS:
        return "at the cap"
    if lay["rounds"] > 1:
        return "partials loop twice"
    if lay["blocks"] > 1:
        return "two blocks"
    return "one block + tail" if lay["tail"] else "one vector"


def adamw_blocks(n):
    return min(_cdiv(n, THREADS), ADAMW_MAX_BLOCKS)


def lerp_blocks(n):
    return min(_cdiv(n, THREADS), LERP_MAX_BLOCKS)


def stream_class(n, cap):
    """Class of an elementwise grid-stride launch of ceil(n/256) blocks capped at `cap` (adamw_kernel, lerp_kernel)."""
    if n > cap * THREADS:
        return "over the cap"
    if n == cap * THREADS:
        return "at the cap"
    if n > THREADS:
        return "two blocks"
    if n == THREADS:
        return "full block"
    return "one thread" if n == 1 else "partial block"


def rows_launch(V, D):
    """lora_adamw_rows' grid and the paths of adamw_rows_kernel a [V, D] table takes."""
    vec = D % 4 == 0
    return {"blocks": min(V, ROWS_MAX_BLOCKS), "row_stride": V > ROWS_MAX_BLOCKS, "vec": vec,
            "idle_cols": (D // 4 if vec else D) < THREADS,          # inactive rows: lanes with no column
            "col_stride_inactive": (D // 4 if vec else D) > THREADS,
            "col_stride_active": D > THREADS}


def merge_blocks(elems):
    return min(_cdiv(elems, THREADS), MERGE_MAX_BLOCKS)


def batched_blocks(max_elems):
    return min(_cdiv(max_elems, BATCHED_ELEMS_PER_BLOCK), BATCHED_MAX_BLOCKS)


# ---- size tables: the smallest n of each class ---------------------------------------------------------------------------
SQNORM_SIZES = {
    "tail only": (1, 2, 3),
    "one vector": (4,),
    "one block + tail": (1027,),                     # 256 vectors and 3 tail elements
    "two blocks": (1028,),
    "partials loop twice": (257 * 1024,),            # 257 blocks: thread 0 of the last arriver adds two partials
    "at the cap": (1024 * 1024,),                    # 1024 blocks, every thread exactly one vector
    "over the cap": (1024 * 1024 + 1024 + 3,),       # block 0 alone takes a second iteration; 3 tail elements
}
ADAMW_SIZES = {
    "one thread": (1,), "partial block": (255,), "full block": (256,), "two blocks": (257,),
    "at the cap": (ADAMW_MAX_BLOCKS * THREADS,), "over the cap": (ADAMW_MAX_BLOCKS * THREADS + 257,),
}
LERP_SIZES = {
    "one thread": (1,), "partial block": (255,), "two blocks": (257,), "over the cap": (LERP_MAX_BLOCKS * THREADS + 3,),
}
LERP_ALPHAS = (0.5, 0.3, 1.0, 0.0)
DTYPES = (F32, F16, BF16)

ROWS_V = (1, 300, 4097)
ROWS_D = (1, 3, 4, 6, 64, 260, 1028, 1030)
ROWS_SHAPES = tuple((V, D) for V in ROWS_V for D in ROWS_D if V * D <= 300 * 1030 and (V <= 300 or D <= 64))
ROWS_PATTERNS = ("none", "all", "first", "last", "alternating")

# (N, K, r, W dtype, factor dtype)
MERGE_GRID = tuple((37, 53, 4, wd, fd) for wd in DTYPES for fd in DTYPES)
MERGE_TABLE = (                                      # one batched launch: blockIdx.y = layer
    (8, 8, 8, F32, F32),                             # r = min(K, N); all but one block of the launch idle
    (37, 53, 1, F16, F16),
    (64, 48, 16, BF16, F32),
    (130, 70, 64, F32, BF16),
    (1031, 1021, 4, F16, F32),                       # > 4096·256 elements: both kernels stride
    (53, 37, 4, BF16, BF16),
)
MERGE_ALPHA = 0.7
# pairs (W dtype, factor dtype) whose product rounding must show in the merged weight (f16 factors in an f16 weight cannot:
# rounding to f16 twice is rounding once)
FACTOR_ROUNDING_SHOWS = ((F32, F16), (F32, BF16), (F16, BF16))

# ---- hyper-parameter samples ---------------------------------------------------------------------------------------------
BETA1, BETA2, EPS = f32(0.9), f32(0.999), f32(1e-8)
BOUNDARY = "boundary"  # max_norm = the gradient's own norm rounded to fp32: within 2^-24 of the clip decision
ADAMW_CONFIGS = (
    {"lr": 1e-4, "wd": 1e-2, "mul": 1.0, "max_norm": 1.0, "step": 1},
    {"lr": 1e-1, "wd": 0.1, "mul": 1.0 / 1024, "max_norm": 0.0, "step": 1000},
    {"lr": 1e-1, "wd": 0.0, "mul": 1.0, "max_norm": 1e9, "step": 7},
    {"lr": 1e-4, "wd": 0.1, "mul": 1.0 / 1024, "max_norm": BOUNDARY, "step": 10000},
    {"lr": 1e-1, "wd": 0.1, "mul": 1.0 / 1024, "max_norm": 1.0, "step": 2},
)
BIAS_STEPS = (1, 2, 7, 100, 1000, 10000)


# ---- input builders ------------------------------------------------------------------------------------------------------
def _log_uniform(n, lo, hi, gen):
    e = torch.rand(n, generator=gen, dtype=torch.float64) * (math.log10(hi) - math.log10(lo)) + math.log10(lo)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    return (sign * 10.0 ** e).float()


def sqnorm_ranges(n):
    """{name: element indices} of the parts of the gradient a wrong loop bound would drop."""
    lay = sqnorm_launch(n)
    blocks, nvec = lay["blocks"], lay["nvec"]
    vec = torch.arange(nvec, dtype=torch.int64)
    out = {}
    if lay["tail"]:
        out["tail"] = torch.arange(4 * nvec, n)
    if blocks > 1:
        last = vec[(vec // THREADS) % blocks == blocks - 1]
        out["last block"] = (last[:, None] * 4 + torch.arange(4)).reshape(-1)
    if lay["iters"] > 1:
        second = vec[vec >= blocks * THREADS]
        out["second iteration"] = (second[:, None] * 4 + torch.arange(4)).reshape(-1)
    return out


def sqnorm_inputs(n, seed=0):
    """A gradient whose magnitudes span 1e-12 … 1e4, with one element of every range of `sqnorm_ranges` (every tail element)
    raised to the root of the rest's square sum: each range then holds at least a tenth of the total."""
    gen = torch.Generator().manual_seed(1000 + seed + n)
    g = _log_uniform(n, 1e-12, 10.0, gen)
    ranges = sqnorm_ranges(n)
    planted = []
    for name, idx in ranges.items():
        planted += idx.tolist() if name == "tail" else [int(idx[idx.numel() // 2])]
    if n > 64:
        g[16], g[8] = 1e4, 1e-12
    keep = torch.ones(n, dtype=torch.bool)
    keep[planted] = False
    root = float(g[keep].double().pow(2).sum().sqrt()) if bool(keep.any()) else 1.0
    for j, i in enumerate(planted):
        g[i] = root * (-1.0 if j % 2 else 1.0)
    return g


def sqnorm_reference(g, mul):
    return float((g.double() * f32(mul)).pow(2).sum())


def sqnorm_mass(g, mul):
    """{range: its share of Σ(g·mul)²}."""
    sq = (g.double() * f32(mul)).pow(2)
    total = float(sq.sum())
    return {name: float(sq[idx].sum()) / total for name, idx in sqnorm_ranges(g.numel()).items()}


def adamw_inputs(n, seed=0):
    """(p, g, m, v) fp32 [n] with, by index mod 8: 1 → g = 0 under live moments; 2 → p near 1e4 and an update far below
    its ulp; 3 → a never-touched element (g = m = v = 0); 4 → first gradient ever, tiny (the eps-dominated denominator);
    the rest → g over 1e-12 … 1e4 with moments of that size, as after many steps.  The last element is an ordinary one."""
    gen = torch.Generator().manual_seed(2000 + seed + n)
    i = torch.arange(n)
    g = _log_uniform(n, 1e-12, 1e4, gen)
    p = torch.randn(n, generator=gen)
    m = 0.3 * g.abs() * torch.randn(n, generator=gen)
    v = (g.abs() * (0.5 + torch.rand(n, generator=gen))) ** 2
    k = i % 8
    g[k == 1] = 0.0
    sel = k == 2
    p[sel] = 1e4 * (1 + 1e-3 * torch.randn(int(sel.sum()), generator=gen))
    g[sel], m[sel], v[sel] = 1e-10, -1e-10, 1.0
    sel = k == 3
    g[sel], m[sel], v[sel] = 0.0, 0.0, 0.0
    sel = k == 4
    g[sel] = _log_uniform(int(sel.sum()), 1e-12, 1e-9, gen)
    m[sel], v[sel] = 0.0, 0.0
    if n > 64:
        g[16], g[8] = 1e4, 1e-12
    p[-1], g[-1], m[-1], v[-1] = -0.8, 0.37, 0.01, 0.04
    return p, g, m, v


def rows_active(V, pattern):
    a = torch.zeros(V, dtype=torch.uint8)
    if pattern == "all":
        a[:] = 1
    elif pattern == "first":
        a[0] = 1
    elif pattern == "last":
        a[-1] = 1
    elif pattern == "alternating":
        a[::2] = 1
    else:
        assert pattern == "none"
    return a


def rows_inputs(V, D, pattern, seed=0):
    """(p, g, m, v [V, D], active [V]): adamw_inputs with g = m = v = 0 on the rows that never had a gradient."""
    p, g, m, v = (t.view(V, D) for t in adamw_inputs(V * D, seed))
    active = rows_active(V, pattern)
    off = active == 0
    g[off], m[off], v[off] = 0.0, 0.0, 0.0
    return p, g, m, v, active


def resolve_max_norm(cfg, g):
    """The config's max_norm as the fp32 value handed to the kernel."""
    if cfg["max_norm"] == BOUNDARY:
        return f32(math.sqrt(sqnorm_reference(g, cfg["mul"])))
    return f32(cfg["max_norm"])


# ---- float64 references --------------------------------------------------------------------------------------------------
def adamw_reference(p, g, m, v, cfg, max_norm, step, clip=True):
    """clip_grad_norm_ + torch.optim.AdamW in float64 on the stored fp32 values (hyper-parameters as the fp32 the C ABI
    passes).  clip False: the null-norm route.  Returns (p', m', v', clip coefficient)."""
    gd = g.double().reshape(-1) * f32(cfg["mul"])
    coef = 1.0
    if clip and max_norm > 0:
        total = orc.clip_grad_norm([gd], max_norm)  # (scales gd in place)
        coef = min(max_norm / (float(total) + 1e-6), 1.0)
    pd, md, vd = p.double().reshape(-1).clone(), m.double().reshape(-1).clone(), v.double().reshape(-1).clone()
    orc.adamw_step(pd, gd, md, vd, step, f32(cfg["lr"]), BETA1, BETA2, EPS, f32(cfg["wd"]))
    return pd.view(p.shape), md.view(p.shape), vd.view(p.shape), coef


def sqnorm_chain(n):
    lay = sqnorm_launch(n)
    return 2 + 4 * lay["iters"] + (1 if lay["tail"] else 0) + 8 + lay["rounds"] + 8


def sqnorm_bound(n):
    L = sqnorm_chain(n)
    return L * U / (1 - L * U)


def grad_k(n, clipping):
    return math.ceil(sqnorm_chain(n) / 2) + 8 if clipping else 1


def adamw_k(n, clipping):
    """(k_m, k_v, k_p) of the module docstring."""
    kg = grad_k(n, clipping)
    return 3 + kg, 3 + 2 * kg, math.ceil(17.5 + 2 * kg)


def adamw_bounds(p, g, m, v, cfg, coef, step, clipping):
    """Elementwise (bound_p, bound_m, bound_v) in float64 around `adamw_reference`."""
    km, kv, kp = adamw_k(g.numel(), clipping)
    lr, wd = f32(cfg["lr"]), f32(cfg["wd"])
    ga = (g.double() * f32(cfg["mul"]) * coef).abs()
    c1, c2 = 1 - BETA1, 1 - BETA2
    Mm = m.double().abs() + c1 * (ga + m.double().abs())
    Mv = BETA2 * v.double() + c2 * ga * ga
    denom = Mv.sqrt() / math.sqrt(1 - BETA2 ** step) + EPS
    Mp = p.double().abs() * (1 - lr * wd) + lr / (1 - BETA1 ** step) * Mm / denom
    return kp * U * Mp + FLT_MIN, km * U * Mm + FLT_MIN, kv * U * Mv + FLT_MIN


def worst_ratio(got, ref, bound):
    """max |got − ref| / bound (inf for a non-finite result): <= 1 is inside the bound."""
    got = got.detach().double().cpu().reshape(-1)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref.reshape(-1)).abs() / bound.reshape(-1)).max())


# ---- fp32 restatements (self-checks of the bounds; the mutants of tests/test_optim_host.py) --------------------------------
def _fma(a, b, c):
    """fp32 fma of fp32 tensors: the product is exact in float64; the sum is rounded to float64 and then to fp32 (a double
    rounding that differs from the fused result in about one case in 2^29 — far inside what the bounds allow)."""
    return (a.double() * b.double() + c.double()).float()


def _block_sum_256(v):
    """block_sum_256 of csrc/optim.hip on [blocks, 256]: the xor butterfly of wave_sum, then (w0 + w1) + (w2 + w3)."""
    w = v.reshape(-1, 4, 64)
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lane ^ off]
    s = w[:, :, 0]
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def sqnorm_f32(g, mul, mutant=None):
    """grad_sqnorm_kernel's sum in its own order, in fp32.  mutant: "skip last tail element", "skip second iteration",
    "drop a partial"."""
    n = g.numel()
    lay = sqnorm_launch(n)
    blocks, nvec, iters = lay["blocks"], lay["nvec"], lay["iters"]
    a = g.float() * torch.tensor(mul, dtype=torch.float32)
    local = torch.zeros(blocks, THREADS)
    if iters:
        body = torch.zeros(iters * blocks * THREADS * 4)
        body[:4 * nvec] = a[:4 * nvec]
        body = body.view(iters, blocks, THREADS, 4)
        for it in range(1 if mutant == "skip second iteration" else iters):
            for c in range(4):
                local = _fma(body[it, :, :, c], body[it, :, :, c], local)
    tail = a[4 * nvec:]
    if mutant == "skip last tail element":
        tail = tail[:-1]
    if tail.numel():
        local[0, :tail.numel()] = _fma(tail, tail, local[0, :tail.numel()])
    partials = _block_sum_256(local)
    if mutant == "drop a partial":
        partials[blocks - 1] = 0.0
    padded = torch.zeros(lay["rounds"] * THREADS)
    padded[:blocks] = partials
    t = torch.zeros(THREADS)
    for row in padded.view(lay["rounds"], THREADS):
        t = t + row
    return float(_block_sum_256(t[None])[0])


ADAMW_MUTANTS = ("eps inside the square root", "bias correction 2 without its root", "weight decay after the Adam term",
                 "clip coefficient not applied", "grad_mul applied twice", "last element skipped")


def adamw_f32(p, g, m, v, cfg, max_norm, step, norm_sq=None, mutant=None):
    """adamw_kernel + adamw_element in fp32, operation by operation without contraction.  norm_sq: norm[0] as an fp32
    value (None: the null-norm route)."""
    t = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    clip = t(1.0)
    if norm_sq is not None and max_norm > 0 and mutant != "clip coefficient not applied":
        c = t(max_norm) / (torch.sqrt(t(norm_sq)) + t(1e-6))
        clip = c if float(c) < 1.0 else t(1.0)
    beta1, beta2, eps, lr = t(BETA1), t(BETA2), t(EPS), t(cfg["lr"])
    bc1 = t(1.0 - BETA1 ** step)
    bc2_sqrt = t(math.sqrt(1.0 - BETA2 ** step))
    if mutant == "bias correction 2 without its root":
        bc2_sqrt = t(1.0 - BETA2 ** step)
    gm = t(cfg["mul"]) * clip
    if mutant == "grad_mul applied twice":
        gm = gm * t(cfg["mul"])
    step_size = lr / bc1
    decay = t(1.0) - lr * t(cfg["wd"])
    p0, m0, v0 = p.float(), m.float(), v.float()
    gg = g.float() * gm
    after = mutant == "weight decay after the Adam term"
    pn = p0 if after else p0 * decay
    mn = m0 + (gg - m0) * (t(1.0) - beta1)
    vn = beta2 * v0 + (t(1.0) - beta2) * gg * gg
    if mutant == "eps inside the square root":
        denom = torch.sqrt(vn / (bc2_sqrt * bc2_sqrt) + eps)
    else:
        denom = torch.sqrt(vn) / bc2_sqrt + eps
    pn = pn - step_size * (mn / denom)
    if after:
        pn = pn * decay
    if mutant == "last element skipped":
        pn, mn, vn = pn.clone(), mn.clone(), vn.clone()
        pn.view(-1)[-1], mn.view(-1)[-1], vn.view(-1)[-1] = p0.view(-1)[-1], m0.view(-1)[-1], v0.view(-1)[-1]
    return pn, mn, vn


# ---- merge ---------------------------------------------------------------------------------------------------------------
def merge_inputs(N, K, r, wdtype, fdtype, seed=0):
    """(W [N, K] in wdtype, A [r, K], B [N, r]: fp32 copies of factors held in fdtype).  B·A is several times W, so the
    rounding of the product to fdtype moves the merged weight."""
    gen = torch.Generator().manual_seed(3000 + seed + 7 * N + K + 31 * r)
    w = (torch.randn(N, K, generator=gen) * 0.05).to(wdtype)
    a = (torch.randn(r, K, generator=gen) * 0.5).to(fdtype).float()
    b = (torch.randn(N, r, generator=gen) * 0.5).to(fdtype).float()
    return w, a, b


def merge_emulate(w, a, b, alpha, fdtype, shift=0):
    """The merge op by op at d + shift·e.  Returns (merged W in w's dtype, e)."""
    T, r = w.dtype, a.shape[0]
    exact = b.double() @ a.double()
    e = r * U / (1 - r * U) * (b.double().abs() @ a.double().abs())
    d = (exact + shift * e).float()                     # the fp32 accumulator
    if fdtype != F32:
        d = d.to(fdtype).float()                        # the product as the reference forms it, in the factors' dtype
    dt = d.to(T)                                        # .type(W.dtype)
    upd = (torch.tensor(alpha, dtype=torch.float32) * dt.float()).to(T)
    return (w.float() + upd.float()).to(T), e


def merge_verdict(got, w, a, b, alpha, fdtype):
    """(elements outside [emulation at d − e, emulation at d + e], elements that differ from the emulation at d)."""
    got = got.detach().cpu()
    lo, hi, mid = (merge_emulate(w, a, b, alpha, fdtype, s)[0].double() for s in (-1, 1, 0))
    assert bool((lo <= hi).all())  # (monotone in d for alpha >= 0)
    g = got.double()
    outside = int(((g < lo) | (g > hi) | ~torch.isfinite(g)).sum())
    return outside, int((g != mid).sum())


# ---- lerp ----------------------------------------------------------------------------------------------------------------
def lerp_inputs(n, dtype, seed=0):
    """(x1, x2): LoRA-sized values with large and small magnitudes mixed in, and x2 = −x1 on every 11th element."""
    gen = torch.Generator().manual_seed(4000 + seed + n)
    x1, x2 = torch.randn(n, generator=gen) * 0.1, torch.randn(n, generator=gen) * 0.1
    i = torch.arange(n)
    x1[i % 7 == 3] *= 1e3
    x2[i % 5 == 2] *= 1e-3
    x1, x2 = x1.to(dtype), x2.to(dtype)
    x2[i % 11 == 5] = -x1[i % 11 == 5]
    return x1, x2


def lerp_emulate(x1, x2, alpha):
    """T( T(a·x1) + T(b·x2) ) with a = f32(alpha), b = f32(1 − alpha), every product and the sum in IEEE single."""
    T = x1.dtype
    a, b = torch.tensor(alpha, dtype=torch.float32), torch.tensor(1 - alpha, dtype=torch.float32)
    p = (a * x1.float()).to(T)
    q = (b * x2.float()).to(T)
    return (p.float() + q.float()).to(T)
