"""Case tables, the launch mirror, input builders, the float64 and fp32 restatements and derived bounds for csrc/prodigy.hip
(`lora_prodigy_moments`, `lora_prodigy_apply`) and `LoraTrainer(optimizer="prodigy")`.  Plain data and CPU torch;
tests/test_prodigy_host.py pins it to the C++ and shows what the bounds reject, tests/test_gpu_prodigy.py and
tests/test_gpu_prodigy_trainer.py run it.

The yardstick is `reference`: the algorithm of K. Mishchenko, A. Defazio, "Prodigy: An Expeditiously Adaptive Parameter-Free
Learner" (arXiv:2306.06101) restated in float64 from its published definition — the `prodigyopt` package is in no tree this
project can read, parity with it is unpinned.  One applied step, g the gradient after grad_mul and the clip
coefficient, t the 1-based count of applied steps, per range j of the slab γ_j = lr_j·λ:
    bc = sqrt(1 − β2^t)/(1 − β1^t) if use_bias_correction else 1 ;  dlr_j = d·γ_j·bc
    num_i = (d/d0)·dlr_j·g_i·(p0_i − p_i) ;  m_i = β1·m_i + d·(1 − β1)·g_i ;  v_i = β2·v_i + d²·(1 − β2)·g_i²
    s_i = β3·s_i + (d/d0)·(d if safeguard_warmup else dlr_j)·g_i ;  den_i = |s_i| (the new s)
    denom = Σ den_i ;  unless denom == 0:  numerator = β3·numerator + Σ num_i  and, if any γ_j > 0:
        d_hat = d_coef·numerator/denom ;  d_new = max(d, d_hat) if d == d0 else d ;  d_max = max(d_max, d_hat)
        d_new = min(d_max, d_new·growth_rate)
    p_i = p_i·(1 − wd_j·dlr_j) − dlr_j·m_i/(sqrt(v_i) + d_new·eps) ;  d ← d_new
dlr uses the OLD d throughout, only the eps term sees d_new; d never decreases.  A step whose overflow flag is set changes nothing.

Bounds, to first order in u = 2^-24 (one correctly rounded +, −, × or fma has relative error <= u; sqrtf and / count 2u; k and
L are whole numbers rounded UP, which covers the second-order terms).  The kernels form every coefficient (c_num = (d/d0)·dlr,
c_m = d·(1 − β1), c_v = d²·(1 − β2), c_s = (d/d0)·(d or dlr), dlr itself) in double from fp32 arguments and round it ONCE: 1u each.
  g' = g·(grad_mul·clip) has relative error kg·u:  kg = 1 without clipping; with clipping the norm is an fp32 INPUT here (the
       tests hand `norm[0]` over), so kg = 8: sqrtf 2, + 1e-6f 1, max_norm/(…) 2, grad_mul·clip 1, g·gm 1, rounded up.  The trainer
       tests read the norm lora_grad_sqnorm left in `norm[0]` back and hand that fp32 value to `reference`: an input again,
       kg = 8 (`bounds(…, kg=…)` takes another count for a caller that compares against a norm of its own).
  m' = β1·m + c_m·g':   left product 1, right: c_m 1, product 1, kg; the sum 1:        |Δm| <= (kg + 3)·u·Mm,  Mm = β1|m| + c_m|g'|
  s' likewise:                                                                       |Δs| <= (kg + 3)·u·Ms,  Ms = β3|s| + c_s|g'|
  v' = β2·v + (c_v·g')·g':  c_v 1, two products, 2·kg, the sum 1:                      |Δv| <= (2kg + 4)·u·Mv, Mv = β2·v + c_v·g'² = v'
  num_i = (c_num·g')·(p0 − p):  the difference 1, c_num 1, two products 2, kg:         |Δnum_i| <= (kg + 4)·u·|num_i|
  Σ num (signed summands): every fp32 addition on the way adds u times a partial sum of magnitudes <= Σ|num_i|; the longest
       chain of additions is  C = 4·iters + tail (the thread's) + 8 (block_sum_256) + 1 (the fold over the block partials runs
       in double: rounded up to one):      |Δ Σnum| <= L·u·Σ|num_i|,  L = kg + 4 + C
       the stored numerator β3·numerator + Σnum is rounded to fp32 once more:  + u·(β3|numerator| + Σ|num_i|)
  denom = Σ|s'_i| (non-negative summands, each within (kg + 3)·u·Ms_i of its value: s' itself may cancel):
       |Δdenom| <= u·((kg + 3)·ΣMs_i + (C + 1)·Σ|s'_i|)                               (+ 1: the fp32 store)
  d_hat = d_coef·numerator/denom in double:  |Δd_hat| <= d_coef·(|Δnumerator|/denom + |numerator|·|Δdenom|/denom²) + u·|d_hat|
  d_new, d_max follow through max and min, which are 1-Lipschitz; d_new·growth_rate scales a deviation by growth_rate where the
       jump from d == d0 is rate-limited:  |Δd_new| <= (growth_rate if finite and d == d0 else 1)·|Δd_hat| + u·|d_new|
  p' = p·decay − dlr·(m'/(sqrtf(v') + d_new·eps)):   decay = 1 − wd·dlr: dlr 1, product 1, difference 1, p·decay 1, the final
       difference 1:  5·u·|p|·(decay + wd·dlr).  The denominator D = sqrtf(v') + eps_d:  v' brings (2kg + 4)/2, sqrtf 2, eps_d =
       d_new·eps 1 and d_new's own deviation and fp32 store, the sum 1; v' may have lost a denormal amount, which the root
       turns into at most sqrt(FLT_MIN).  The quotient 2, dlr 1, the product 1, and m' carries (kg + 3)·u·Mm:
       |Δp| <= 5u·|p|(decay + wd·dlr) + dlr·Mm/D·((2kg + 16)·u + (|Δd_new|/d_new)·eps_d/D + sqrt(FLT_MIN)/D)
Each bound gets FLT_MIN added, so that no test pins how denormal results are handled; the builders keep |g| in 1e-6 … 1e2
(or exactly 0) so that no product of the update underflows.  A compiler that contracts a product and a sum into an fma removes
a rounding; the bounds hold either way.

Trajectory (`trajectory`, the 2048-element noisy quadratic: p0 = 0, target std 0.05, gradient p − target + noise of std 0.01,
lr = 1, no decay, 60 steps, the gradient computed from the run's own parameters): the fp32 restatement `step_f32` deviates from
the float64 one by  TRAJ_D_REL = 7.2e-8  in d (largest relative deviation over the 60 steps) and  TRAJ_P_ABS = 1.4e-7  in the
final p (largest absolute deviation), measured with `trajectory_deviation()` on the CPU (tests/test_prodigy_host.py repeats the
measurement and holds it to these figures).  The kernels are allowed 4 times that: contraction and reduction order differ,
nothing else should."""
import math

import torch

from tests import optim_cases as oc

U, FLT_MIN, f32 = oc.U, oc.FLT_MIN, oc.f32

# ---- the launch grids of csrc/prodigy.hip (pinned to its text by tests/test_prodigy_host.py) ---------------------------------
THREADS = 256
MAX_BLOCKS = 1024      # kMaxBlocks: both kernels
VEC = 4                # float4 body: nvec = n >> 2, the n % 4 tail on block 0
MAX_RANGES = 4         # kMaxRanges
WORKSPACE_BYTES = 16 + 2 * MAX_BLOCKS * 4
SCALARS = 8            # d, d_max, numerator, d_prev, d_hat, denom, 0, 0
ONE_EM6 = f32(1e-6)    # the kernel's 1e-6f

TRAJ_D_REL = 7.2e-8
TRAJ_P_ABS = 1.4e-7
TRAJ_STEPS, TRAJ_N = 60, 2048


def launch(n):
    """The grid of both entries and the loop counts of their kernels."""
    nvec, tail = n // VEC, n % VEC
    blocks = min(max(oc._cdiv(nvec, THREADS), 1), MAX_BLOCKS)
    stride = blocks * THREADS
    return {"blocks": blocks, "nvec": nvec, "tail": tail, "iters": oc._cdiv(nvec, stride),
            "rounds": oc._cdiv(blocks, THREADS)}  # the last arriver's loop over the partials


def size_class(n):
    lay = launch(n)
    if lay["nvec"] == 0:
        return "tail only"
    if lay["iters"] > 1:
        return "over the cap"
    if lay["blocks"] == MAX_BLOCKS:
        return "at the cap"
    if lay["rounds"] > 1:
        return "partials loop twice"
    if lay["blocks"] > 1:
        return "two blocks"
    if lay["tail"]:
        return "body + tail"
    if lay["nvec"] == 1:
        return "one vector"
    return "full block" if lay["nvec"] == THREADS else "partial block"


SIZES = {
    "tail only": (1, 3),
    "one vector": (4,),
    "partial block": (1020,),                        # 255 vectors
    "full block": (1024,),
    "body + tail": (1027,),                          # 256 vectors and 3 tail elements
    "two blocks": (1028,),
    "partials loop twice": (257 * 1024,),            # 257 blocks: thread 0 of the last arriver adds two partials
    "at the cap": (1024 * 1024,),
    "over the cap": (1024 * 1024 + 1024 + 3,),       # block 0 alone takes a second iteration; 3 tail elements
}
ALL_SIZES = tuple(n for sizes in SIZES.values() for n in sizes)
OVER_THE_CAP = SIZES["over the cap"][0]

RANGE_N = 1540
RANGE_CASES = (                                      # (ends, lr, wd): no end a multiple of 4 or 256 but the last
    ((5, RANGE_N), (1.0, 0.25), (0.0, 0.1)),
    ((261, RANGE_N), (0.5, 1.0), (0.1, 0.01)),
    ((1027, RANGE_N), (1.0, 0.0), (0.01, 0.1)),      # a frozen second range: γ = 0 there, not everywhere
    ((5, 261, 1027, RANGE_N), (1.0, 0.25, 0.5, 0.125), (0.0, 0.1, 0.01, 0.05)),
)


def config(**kw):
    """The options of one step; hyper-parameters are rounded to fp32 where they are used, as the C ABI passes them."""
    cfg = {"beta1": 0.9, "beta2": 0.999, "beta3": None, "eps": 1e-8, "d0": 1e-6, "d_coef": 1.0, "growth_rate": math.inf,
           "bias_correction": False, "safeguard": False, "mul": 1.0, "max_norm": 0.0, "ends": None, "lr": (1.0,), "wd": (0.0,)}
    cfg.update(kw)
    if cfg["beta3"] is None:
        cfg["beta3"] = math.sqrt(f32(cfg["beta2"]))
    return cfg


def _hp(cfg, n):
    h = {k: f32(cfg[k]) for k in ("beta1", "beta2", "beta3", "eps", "d0", "d_coef", "mul", "max_norm")}
    h["growth_rate"] = f32(cfg["growth_rate"]) if math.isfinite(cfg["growth_rate"]) else math.inf
    h["ends"] = tuple(cfg["ends"]) if cfg["ends"] is not None else (n,)
    h["lr"], h["wd"] = [f32(x) for x in cfg["lr"]], [f32(x) for x in cfg["wd"]]
    assert len(h["ends"]) == len(h["lr"]) == len(h["wd"]) and h["ends"][-1] == n
    return h


def range_index(n, ends):
    """The range of every element: j with ends[j − 1] <= i < ends[j]."""
    return torch.bucketize(torch.arange(n), torch.tensor(list(ends)), right=True)


def state(d=1e-6, d_max=None, numerator=0.0):
    """The three scalars as fp32 values."""
    return {"d": f32(d), "d_max": f32(d if d_max is None else d_max), "numerator": f32(numerator)}


MID_RUN = state(3e-4, 5e-4, 2.5e-3)  # d has left d0, d_max is ahead of it, the numerator has history
LEVEL = state(3e-4, 3e-4, 2.5e-3)    # d == d_max: a d_hat below d then leaves both alone (with d_max ahead, d rises to it)

# (options, scalars, applied-step count, clipping) every size of the grid is run at
GRID_CONFIGS = (
    (config(), MID_RUN, 7, False),
    (config(max_norm=1.0, mul=1.0 / 1024, bias_correction=True, growth_rate=1.02, wd=(0.1,)), MID_RUN, 2, True),
    (config(growth_rate=1.02, wd=(0.1,), lr=(0.5,)), state(), 1, False),
)


def norm_sq_of(g, cfg):
    """Σ(g·mul)² as the fp32 value a test hands over in norm[0]."""
    return f32(float((g.double() * f32(cfg["mul"])).pow(2).sum()))


# ---- the scalar step ------------------------------------------------------------------------------------------------------------
def scalar_step(st, sum_num, denom, h, mutant=None):
    """d → d_new in double.  Returns the new state (unrounded) with "d_hat", "denom" and "branch"."""
    d, d_max, numerator = st["d"], st["d_max"], st["numerator"]
    out = {"d": d, "d_max": d_max, "numerator": numerator, "d_hat": None, "denom": denom, "branch": "denom == 0"}
    if not denom > 0:
        return out
    out["numerator"] = numerator = (1.0 if mutant == "numerator not decayed by beta3" else h["beta3"]) * numerator + sum_num
    out["branch"] = "all lr zero"
    if not any(x > 0 for x in h["lr"]):
        return out
    d_hat = h["d_coef"] * numerator / denom
    d_new = d
    if d == h["d0"] and mutant != "first growth rate-limited":
        d_new = max(d, d_hat)
    d_max = max(d_max, d_hat)
    grown = d_new * h["growth_rate"]
    out["branch"] = ("first growth" if d == h["d0"] and d_hat > d else "d_hat below d" if d_hat < d else
                     "rate-limited" if grown < d_max else "d_max")
    out.update(d=min(d_max, grown), d_max=d_max, d_hat=d_hat)
    return out


def _clip(h, norm_sq):
    if h["max_norm"] > 0:
        return min(h["max_norm"] / (math.sqrt(norm_sq) + ONE_EM6), 1.0)
    return 1.0


def _bc(h, cfg, t):
    return math.sqrt(1.0 - h["beta2"] ** t) / (1.0 - h["beta1"] ** t) if cfg["bias_correction"] else 1.0


# ---- float64 ----------------------------------------------------------------------------------------------------------------------
def reference(p, p0, g, m, v, s, st, cfg, t=1, norm_sq=0.0, flagged=False):
    """One step in float64 on the stored values.  Returns {"p", "m", "v", "s" (float64 tensors), "state" (scalar_step's
    result), and what `bounds` needs}."""
    n = p.numel()
    h = _hp(cfg, n)
    p, p0, m, v, s = (x.double().reshape(-1) for x in (p, p0, m, v, s))
    if flagged:
        return {"p": p, "m": m, "v": v, "s": s, "state": dict(st, d_hat=None, denom=None, branch="overflow")}
    gd = g.double().reshape(-1) * (h["mul"] * _clip(h, norm_sq))
    j = range_index(n, h["ends"])
    lr, wd = torch.tensor(h["lr"], dtype=torch.float64)[j], torch.tensor(h["wd"], dtype=torch.float64)[j]
    d, b1, b2, b3 = st["d"], h["beta1"], h["beta2"], h["beta3"]
    dlr = d * lr * _bc(h, cfg, t)
    ratio = d / h["d0"]
    c_s = ratio * (torch.full_like(dlr, d) if cfg["safeguard"] else dlr)
    num = ratio * dlr * gd * (p0 - p)
    m2 = b1 * m + d * (1 - b1) * gd
    v2 = b2 * v + d * d * (1 - b2) * gd * gd
    s2 = b3 * s + c_s * gd
    new = scalar_step(st, float(num.sum()), float(s2.abs().sum()), h)
    D = v2.sqrt() + new["d"] * h["eps"]
    p2 = p * (1 - wd * dlr) - dlr * m2 / D
    return {"p": p2, "m": m2, "v": v2, "s": s2, "state": new, "num": num, "dlr": dlr, "wd": wd, "D": D,
            "Mm": b1 * m.abs() + d * (1 - b1) * gd.abs(), "Ms": b3 * s.abs() + c_s * gd.abs(), "p_old": p, "h": h, "old": dict(st)}


def sum_chain(n):
    """C of the module docstring."""
    lay = launch(n)
    return 4 * lay["iters"] + (1 if lay["tail"] else 0) + 8 + 1


def bounds(ref, n, clipping, kg=None):
    """{"p", "m", "v", "s": elementwise; "numerator", "denom", "d", "d_max", "d_hat": scalars} around `reference`."""
    if kg is None:
        kg = 8 if clipping else 1
    h, new, old = ref["h"], ref["state"], ref["old"]
    C = sum_chain(n)
    out = {"m": (kg + 3) * U * ref["Mm"] + FLT_MIN, "s": (kg + 3) * U * ref["Ms"] + FLT_MIN,
           "v": (2 * kg + 4) * U * ref["v"] + FLT_MIN}
    sum_abs = float(ref["num"].abs().sum())
    d_sum = (kg + 4 + C) * U * sum_abs
    denom = float(ref["s"].abs().sum())
    out["denom"] = U * ((kg + 3) * float(ref["Ms"].sum()) + (C + 1) * denom) + FLT_MIN
    out["numerator"] = d_sum + U * (h["beta3"] * abs(old["numerator"]) + sum_abs) + FLT_MIN
    d_dev = 0.0
    if new["d_hat"] is not None:
        d_hat = new["d_hat"]
        hat_dev = h["d_coef"] * (d_sum / denom + abs(new["numerator"]) * out["denom"] / denom ** 2) + U * abs(d_hat)
        limited = math.isfinite(h["growth_rate"]) and old["d"] == h["d0"]
        d_dev = (h["growth_rate"] if limited else 1.0) * hat_dev
        out["d_hat"] = hat_dev + FLT_MIN
    out["d"] = out["d_max"] = d_dev + U * abs(new["d"]) + FLT_MIN
    eps_d = new["d"] * h["eps"]
    D, dlr = ref["D"], ref["dlr"]
    decay_mag = (1 - ref["wd"] * dlr).abs() + ref["wd"] * dlr
    rel = (2 * kg + 16) * U + (out["d"] / new["d"]) * eps_d / D + math.sqrt(FLT_MIN) / D
    out["p"] = 5 * U * ref["p_old"].abs() * decay_mag + dlr * ref["Mm"] / D * rel + FLT_MIN
    return out


def worst(got, ref, bnd):
    """{name: max |got − ref| / bound} over p, m, v, s and the scalars; got: {"p", "m", "v", "s": tensors, "state": the three
    scalars and optionally "denom", "d_hat"}.  <= 1 is inside."""
    out = {k: oc.worst_ratio(got[k], ref[k], bnd[k]) for k in ("p", "m", "v", "s")}
    for k in ("d", "d_max", "numerator", "denom", "d_hat"):
        if k in got["state"] and got["state"][k] is not None and ref["state"].get(k) is not None and k in bnd:
            x = float(got["state"][k])
            out[k] = abs(x - ref["state"][k]) / bnd[k] if math.isfinite(x) else math.inf
    return out


# ---- fp32, operation by operation in the kernels' order --------------------------------------------------------------------------
MUTANTS = ("dlr from d_new", "den from the old s", "first growth rate-limited", "numerator not decayed by beta3",
           "weight decay with lr instead of dlr", "last element skipped")


def _thread_sums(x, n):
    """The fp32 per-block sums of the per-element values x in the launch's order: thread chains, then block_sum_256."""
    lay = launch(n)
    blocks, nvec, iters = lay["blocks"], lay["nvec"], lay["iters"]
    local = torch.zeros(blocks, THREADS)
    if iters:
        body = torch.zeros(iters * blocks * THREADS * VEC)
        body[:VEC * nvec] = x[:VEC * nvec]
        body = body.view(iters, blocks, THREADS, VEC)
        for it in range(iters):
            for c in range(VEC):
                local = local + body[it, :, :, c]
    tail = x[VEC * nvec:]
    if tail.numel():
        local[0, :tail.numel()] = local[0, :tail.numel()] + tail
    return oc._block_sum_256(local)


def _fold(partials, n):
    """The last arriver's double sum over the fp32 block partials: thread k adds partials k, k + 256, …, then one butterfly."""
    lay = launch(n)
    padded = torch.zeros(lay["rounds"] * THREADS, dtype=torch.float64)
    padded[:lay["blocks"]] = partials.double()
    t = torch.zeros(THREADS, dtype=torch.float64)
    for row in padded.view(lay["rounds"], THREADS):
        t = t + row
    return float(oc._block_sum_256(t[None])[0])


def step_f32(p, p0, g, m, v, s, st, cfg, t=1, norm_sq=0.0, flagged=False, mutant=None):
    """`lora_prodigy_moments` + `lora_prodigy_apply` in fp32 without contraction, the scalar step in double on the fp32
    scalars and its results rounded to fp32, as the kernels store them.  Returns {"p", "m", "v", "s", "state"}."""
    T = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    n = p.numel()
    h = _hp(cfg, n)
    p, p0, m, v, s = (x.float().reshape(-1) for x in (p, p0, m, v, s))
    if flagged:
        return {"p": p, "m": m, "v": v, "s": s, "state": dict(st, d_hat=None, denom=None)}
    clip = T(1.0)
    if h["max_norm"] > 0:
        c = T(h["max_norm"]) / (torch.sqrt(T(norm_sq)) + T(1e-6))
        clip = c if float(c) < 1.0 else T(1.0)
    gg = g.float().reshape(-1) * (T(h["mul"]) * clip)
    j = range_index(n, h["ends"])
    d, b1, b2, b3 = st["d"], h["beta1"], h["beta2"], h["beta3"]
    bc, ratio = _bc(h, cfg, t), st["d"] / h["d0"]
    dlr64 = [d * lr * bc for lr in h["lr"]]
    c_num = torch.tensor([ratio * x for x in dlr64], dtype=torch.float64).float()[j]
    c_s = torch.tensor([ratio * (d if cfg["safeguard"] else x) for x in dlr64], dtype=torch.float64).float()[j]
    c_m, c_v = T(d * (1.0 - b1)), T(d * d * (1.0 - b2))
    num = (c_num * gg) * (p0 - p)
    m2 = T(b1) * m + c_m * gg
    v2 = T(b2) * v + (c_v * gg) * gg
    s2 = T(b3) * s + c_s * gg
    den = (s if mutant == "den from the old s" else s2).abs()
    if mutant == "last element skipped":
        num, den = num.clone(), den.clone()
        num[-1], den[-1] = 0.0, 0.0
    new = scalar_step(st, _fold(_thread_sums(num, n), n), _fold(_thread_sums(den, n), n), h, mutant)
    new = {k: (f32(x) if isinstance(x, float) else x) for k, x in new.items()}
    d_for_lr = new["d"] if mutant == "dlr from d_new" else d
    dlr = torch.tensor([d_for_lr * lr * bc for lr in h["lr"]], dtype=torch.float64).float()
    wd = torch.tensor(h["wd"], dtype=torch.float32)
    lr32 = torch.tensor(h["lr"], dtype=torch.float32)
    decay = (T(1.0) - wd * (lr32 if mutant == "weight decay with lr instead of dlr" else dlr))[j]
    dlr = dlr[j]
    eps_d = T(new["d"]) * T(h["eps"])
    p2 = p * decay - dlr * (m2 / (torch.sqrt(v2) + eps_d))
    if mutant == "last element skipped":
        p2, m2, v2, s2 = p2.clone(), m2.clone(), v2.clone(), s2.clone()
        p2[-1], m2[-1], v2[-1], s2[-1] = p[-1], m[-1], v[-1], s[-1]
    return {"p": p2, "m": m2, "v": v2, "s": s2, "state": new}


# ---- input builders ----------------------------------------------------------------------------------------------------------------
def inputs(n, seed=0, plant=True, s_scale=1e-2):
    """(p, p0, g, m, v, s) fp32 [n].  |g| log-uniform over 1e-6 … 1e2 with moments of that size, as after many steps (s of size
    s_scale·|g|: 30 gives a denominator so large that d_hat falls below d); by index
    mod 8: 1 → g = 0 under live state; 3 → a never-touched element (g = m = v = s = 0, p = p0).  plant: one element of every
    range of `optim_cases.sqnorm_ranges` (the grid is the same; every tail element) gets g = Σ|g| of the rest and p0 − p such
    that its |num_i| equals Σ|num_i| of the rest, signs alternating: each range then holds a tenth of Σ|num_i| at least and
    more than that of Σ|s_i|."""
    gen = torch.Generator().manual_seed(6000 + seed + n)
    i = torch.arange(n)
    g = oc._log_uniform(n, 1e-6, 1e2, gen)
    p0 = 0.1 * torch.randn(n, generator=gen)
    # g·(p0 − p) > 0 on three elements in four: Σ num_i is positive and d_hat lies well above MID_RUN's d and d_max
    toward = torch.where(torch.rand(n, generator=gen) < 0.75, 1.0, -1.0) * torch.sign(g)
    p = p0 - 0.02 * torch.randn(n, generator=gen).abs() * toward
    m = 3e-4 * 0.3 * g.abs() * torch.randn(n, generator=gen)
    v = (3e-4 * g.abs() * (0.5 + torch.rand(n, generator=gen))) ** 2
    s = s_scale * g.abs() * torch.randn(n, generator=gen)
    k = i % 8
    g[k == 1] = 0.0
    sel = k == 3
    g[sel], m[sel], v[sel], s[sel] = 0.0, 0.0, 0.0, 0.0
    p[sel] = p0[sel]
    if n > 1:
        p[-1], p0[-1], g[-1], m[-1], v[-1], s[-1] = -0.8, -0.5, 0.37, 1e-5, 4e-9, -2.0
    if plant:
        planted = planted_elements(n)
        keep = torch.ones(n, dtype=torch.bool)
        keep[planted] = False
        if planted and bool(keep.any()):
            sum_g = float(g[keep].double().abs().sum())
            sum_gd = float((g[keep].double() * (p0[keep] - p[keep]).double()).abs().sum())
            for q, idx in enumerate(planted):
                g[idx] = sum_g
                p[idx] = p0[idx] - (sum_gd / sum_g) * (-1.0 if q % 2 else 1.0)
    return p, p0, g, m, v, s


def planted_elements(n):
    out = []
    for name, idx in oc.sqnorm_ranges(n).items():
        out += idx.tolist() if name == "tail" else [int(idx[idx.numel() // 2])]
    return out


def shares(ref, n):
    """{range: (its share of Σ|num_i|, its share of Σ|s_i|)}."""
    num, den = ref["num"].abs(), ref["s"].abs()
    return {name: (float(num[idx].sum() / num.sum()), float(den[idx].sum() / den.sum()))
            for name, idx in oc.sqnorm_ranges(n).items()}


# ---- the trajectory ------------------------------------------------------------------------------------------------------------------
def quadratic(seed=0, steps=TRAJ_STEPS, n=TRAJ_N):
    """(target [n], noise [steps, n]) fp32 from a seeded CPU generator: the gradient at p is p − target + noise[k]."""
    gen = torch.Generator().manual_seed(7000 + seed)
    return 0.05 * torch.randn(n, generator=gen), 0.01 * torch.randn(steps, n, generator=gen)


def trajectory(step_fn, dtype, cfg=None, steps=TRAJ_STEPS, seed=0, n=TRAJ_N):
    """`steps` steps from p0 = 0 with `step_fn` (reference or step_f32), state carried in `dtype`; the scalars stay as the
    step returns them (unrounded under `reference`).  Returns (d after every step, final p, loss 0.5·|p − target|² per step)."""
    cfg = cfg or config()
    target, noise = quadratic(seed, steps, n)
    p = torch.zeros(n, dtype=dtype)
    p0, m, v, s = p.clone(), p.clone(), p.clone(), p.clone()
    st, ds, losses = state(cfg["d0"]), [], []
    for k in range(steps):
        g = (p - target.to(dtype)) + noise[k].to(dtype)
        out = step_fn(p, p0, g, m, v, s, st, cfg, t=k + 1)
        p, m, v, s = (out[x].to(dtype) for x in ("p", "m", "v", "s"))
        st = {x: out["state"][x] for x in ("d", "d_max", "numerator")}
        ds.append(st["d"])
        losses.append(float(0.5 * (p.double() - target.double()).pow(2).sum()))
    return ds, p, losses


def trajectory_deviation(ds, p, ref_ds, ref_p):
    """(largest relative deviation of d over the steps, largest absolute deviation of the final p)."""
    return (max(abs(a - b) / b for a, b in zip(ds, ref_ds)), float((p.double().cpu() - ref_p.double()).abs().max()))
