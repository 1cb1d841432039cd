"""CPU-only guards for the Prodigy tests (tests/test_gpu_prodigy.py, tests/test_gpu_prodigy_trainer.py):

1. the launch mirror of tests/prodigy_cases.py and the arithmetic it restates are pinned to the text of csrc/prodigy.hip;
2. every size class is hit, and the builders put a tenth of Σ|num_i| in every range a wrong loop bound would drop;
3. both entry points return the status include/lora_hip.h documents for a bad argument, before any launch (fake pointers:
   nothing here reaches a device), and `step.check_prodigy` raises on each bad option;
4. at exactly the bounds the GPU files use, the checker accepts the fp32 restatement of the kernels and rejects six plausible bugs;
5. the float64 restatement has the properties the algorithm promises: d never decreases, growth_rate caps its rise, the
   safeguard form is the plain one at γ·bc = 1 and another one at γ = 0.5; and the fp32 trajectory deviates from it by the
   figures the case file records."""
import ctypes
import math
import os
import re

import pytest
import torch

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import build_native as bn
from diffusion_finetuning_amd import step as stp
from tests import optim_cases as oc
from tests import prodigy_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "diffusion_finetuning_amd", "csrc", "prodigy.hip")


def _source():
    with open(SRC) as f:
        return f.read()


def _kernel(src, name):
    i = src.index("void %s(" % name)
    return src[i:src.index("\n}\n", i)]


def test_the_mirror_matches_the_source():
    src = _source()
    assert "prodigy.hip" in bn.SOURCES
    assert int(re.search(r"constexpr int kMaxBlocks = (\d+);", src)[1]) == pc.MAX_BLOCKS
    assert int(re.search(r"constexpr int kMaxRanges = (\d+);", src)[1]) == pc.MAX_RANGES == nat.PRODIGY_MAX_RANGES
    assert set(re.findall(r"__launch_bounds__\((\d+)\)", src)) == {str(pc.THREADS)}
    assert len(re.findall(r"dim3\(256\)", src)) == src.count("hipLaunchKernelGGL(") == 3  # every launch: 256 threads
    m = re.search(r"int64_t blocks = \(n / (\d+) \+ (\d+)\) / (\d+);", src)
    assert m and (int(m[1]), int(m[2]) + 1, int(m[3])) == (pc.VEC, pc.THREADS, pc.THREADS)
    assert "if (blocks > kMaxBlocks) blocks = kMaxBlocks;" in src and "if (blocks < 1) blocks = 1;" in src
    assert src.count("dim3((unsigned)stream_blocks(n))") + src.count("const dim3 grid((unsigned)stream_blocks(n));") == 2
    assert "return 16 + 2 * kMaxBlocks * 4;" in src and nat.lib().lora_prodigy_workspace_bytes() == pc.WORKSPACE_BYTES
    for name in ("prodigy_moments_kernel", "prodigy_apply_kernel"):
        k = _kernel(src, name)
        for line in ("const int64_t nvec = a.n >> 2;",
                     "for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {",
                     "if (blockIdx.x == 0) {", "for (int64_t i = (nvec << 2) + threadIdx.x; i < a.n; i += 256) {",
                     "if (a.norm_in[1] != 0.f) return;"):
            assert line in k, (name, line)
    k = _kernel(src, "prodigy_moments_kernel")
    for line in ("for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) {", "a.partials[kMaxBlocks + blockIdx.x] = bden;",
                 "tn += (double)a.partials[i];"):
        assert line in k, line
    # the hand-off: stores drained, released at agent scope, drained again, THEN the ticket; the last arriver acquires
    order = [k.index(x) for x in ("a.partials[blockIdx.x] = bnum;", '__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");',
                                  "__hip_atomic_fetch_add(a.ticket", '__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");')]
    assert order == sorted(order) and k.count('asm volatile("s_waitcnt vmcnt(0)" ::: "memory");') == 3
    assert "lora_zero_ticket(workspace, st)" in src and "hipMemset" not in src and "atomicAdd" not in src
    # the grid is the squared-norm launch's: optim_cases.sqnorm_ranges names the ranges a wrong loop bound would drop
    assert (pc.THREADS, pc.MAX_BLOCKS, pc.VEC) == (oc.THREADS, oc.SQNORM_MAX_BLOCKS, oc.SQNORM_VEC)
    for n in pc.ALL_SIZES + (pc.RANGE_N, pc.TRAJ_N, 1246464):
        mine, theirs = pc.launch(n), oc.sqnorm_launch(n)
        assert all(mine[key] == theirs[key] for key in mine), n


def test_restated_arithmetic_matches_the_source():
    """step_f32 restates these lines; a change to them must come with a change to the restatement."""
    src = _source()
    for line in ("num += (c_num * g) * (p0 - p);", "m = beta1 * m + c_m * g;", "v = beta2 * v + (c_v * g) * g;",
                 "s = beta3 * s + c_s * g;", "den += fabsf(s);",
                 "const float q = m / (sqrtf(v) + eps_d);", "p = fmaf(-dlr, q, rounded_f32(p * decay));",
                 "const float c = a.max_norm / (sqrtf(a.norm_in[0]) + 1e-6f);", "clip = c < 1.f ? c : 1.f;",
                 "const float gm = a.grad_mul * clip;", "const double ratio = d / (double)a.d0;",
                 "const float c_m = (float)(d * (1.0 - (double)a.beta1));",
                 "const float c_v = (float)(d * d * (1.0 - (double)a.beta2));",
                 "const double dlr = d * (double)a.r.lr[j] * bc;", "c_num[j] = (float)(ratio * dlr);",
                 "c_s[j] = (float)(ratio * (a.safeguard ? d : dlr));",
                 "dlr[j] = (float)(d_prev * (double)a.r.lr[j] * bc);", "decay[j] = fmaf(-a.r.wd[j], dlr[j], 1.f);",
                 "const float eps_d = a.scalars[0] * a.eps;",
                 "return sqrt(1.0 - pow((double)beta2, t)) / (1.0 - pow((double)beta1, t));",
                 "const double numerator = (double)a.beta3 * (double)a.scalars[2] + tn;",
                 "const double d_hat = (double)a.d_coef * numerator / td;", "if (d_f == a.d0) d_new = d_hat > d ? d_hat : d;",
                 "if (d_hat > d_max) d_max = d_hat;", "const double grown = d_new * (double)a.growth_rate;",
                 "d_new = d_max < grown ? d_max : grown;", "if (td > 0.0) {", "a.scalars[3] = d_f;"):
        assert line in src, line
    k = _kernel(src, "prodigy_moments_kernel")
    assert k.index("a.scalars[3] = d_f;") < k.index("a.scalars[0] = (float)d_new;")  # d_prev = d before d = d_new
    assert "template <bool kEma>" in src and src.count("if constexpr (kEma)") == 3


def test_every_size_class_is_hit_and_every_range_is_planted():
    for name, sizes in pc.SIZES.items():
        for n in sizes:
            assert pc.size_class(n) == name, (n, pc.size_class(n))
    assert set(pc.SIZES) == {"tail only", "one vector", "partial block", "full block", "body + tail", "two blocks",
                             "partials loop twice", "at the cap", "over the cap"}
    lay = {n: pc.launch(n) for n in pc.ALL_SIZES}
    assert (lay[1027]["nvec"], lay[1027]["tail"], lay[1027]["blocks"]) == (256, 3, 1) and lay[1028]["blocks"] == 2
    assert (lay[257 * 1024]["blocks"], lay[257 * 1024]["rounds"]) == (257, 2)
    assert (lay[1024 * 1024]["blocks"], lay[1024 * 1024]["iters"]) == (1024, 1)
    over = lay[pc.OVER_THE_CAP]
    assert (over["blocks"], over["iters"], over["tail"]) == (1024, 2, 3) and max(pc.ALL_SIZES) * 4 * 7 < 32 << 20
    for ends, lr, wd in pc.RANGE_CASES:
        assert ends[-1] == pc.RANGE_N and all(e % 4 and e % 256 for e in ends[:-1]) and len(set(lr)) == len(lr) == len(ends)
        assert len(set(wd)) == len(wd)
    assert {len(c[0]) for c in pc.RANGE_CASES} == {2, 4} and {e for c in pc.RANGE_CASES for e in c[0][:-1]} == {5, 261, 1027}
    for n in pc.ALL_SIZES:
        ins = pc.inputs(n)
        assert all(torch.equal(a, b) for a, b in zip(ins, pc.inputs(n))) and all(bool(torch.isfinite(x).all()) for x in ins)
        g = ins[2]
        assert float(g[g != 0].abs().min()) >= 1e-6 and bool((ins[4] >= 0).all())
        for cfg, st, t, clip in pc.GRID_CONFIGS:
            ref = pc.reference(*ins, st, cfg, t, pc.norm_sq_of(g, cfg) if clip else 0.0)
            bnd = pc.bounds(ref, n, clip)
            for name, (num_share, den_share) in pc.shares(ref, n).items():
                assert num_share >= 0.1, (n, name, num_share)
                if n < 4:  # (nothing to weigh a lone tail against: it is the whole input)
                    continue
                # a dropped range moves both sums by far more than their bounds
                assert num_share * float(ref["num"].abs().sum()) > 100 * bnd["numerator"], (n, name)
                if not clip and st is pc.MID_RUN:  # (clipped to norm 1, or at d = d0, the planted gradient does not outweigh the old s)
                    assert den_share * ref["state"]["denom"] > 100 * bnd["denom"], (n, name)
    assert set(oc.sqnorm_ranges(pc.OVER_THE_CAP)) == {"tail", "last block", "second iteration"}
    # the three states keep d_hat away from the d == d0 equality and the denominator away from zero
    branches = {pc.reference(*pc.inputs(1027), st, cfg, t)["state"]["branch"] for cfg, st, t, _ in pc.GRID_CONFIGS}
    assert branches == {"d_max", "d_hat below d", "first growth"}, branches  # (clipped to norm 1, d_hat stays small)


# ---- argument validation: no launch ---------------------------------------------------------------------------------------------
OK, OK2, ODD = 0x10000, 0x20000, 0x10004  # fake device pointers: 16-byte aligned, and 4 bytes past a 16-byte boundary
BADARG, ALIGN = -1, -3


def _ranges(ends, lrs, wds):
    return nat.prodigy_ranges(ends, lrs, wds)


def _moments(lib, ptrs=None, n=8, ranges=((8,), (1.0,)), n_ranges=None, hp=(1.0, 1.0, 0.9, 0.999, 0.9995, 1e-6, 1.0, math.inf),
             scalars=OK2, norm=OK2, ws=OK2):
    e, l, _ = _ranges(ranges[0], ranges[1], None)
    ptrs = [OK] * 6 if ptrs is None else ptrs
    return lib.lora_prodigy_moments(*ptrs, n, e, l, len(ranges[0]) if n_ranges is None else n_ranges, norm, scalars, ws, *hp, 0, 0,
                                    None)


def _apply(lib, ptrs=None, shadow=None, n=8, ranges=((8,), (1.0,), (0.0,)), n_ranges=None, hp=(0.9, 0.999, 1e-8), ema=(0.0, 0),
           scalars=OK2, norm=OK2):
    e, l, w = _ranges(*ranges)
    ptrs = [OK] * 3 if ptrs is None else ptrs
    return lib.lora_prodigy_apply(*ptrs, shadow, n, e, l, w, len(ranges[0]) if n_ranges is None else n_ranges, norm, scalars, *hp,
                                  0, *ema, None)


def test_bad_arguments_return_their_status_before_any_launch():
    lib = nat.lib()
    with open(os.path.join(ROOT, "include", "lora_hip.h")) as f:
        h = f.read()
    for name in ("lora_prodigy_moments", "lora_prodigy_apply", "lora_prodigy_workspace_bytes"):
        assert re.search(r"\b%s\(" % name, h) and name in nat.SIGNATURES
    assert lib.lora_version() == 9
    for null in range(6):
        ptrs = [OK] * 6
        ptrs[null] = None
        assert _moments(lib, ptrs) == BADARG, null
    assert _moments(lib, scalars=None) == BADARG and _moments(lib, norm=None) == BADARG and _moments(lib, ws=None) == BADARG
    assert lib.lora_prodigy_moments(*[OK] * 6, 8, None, None, 1, OK2, OK2, OK2, 1.0, 1.0, 0.9, 0.999, 0.9995, 1e-6, 1.0, 2.0, 0, 0,
                                    None) == BADARG
    assert _moments(lib, n=0) == BADARG and _moments(lib, n=-8) == BADARG
    assert _moments(lib, n_ranges=0) == BADARG and _moments(lib, n_ranges=5) == BADARG and _moments(lib, n_ranges=-1) == BADARG
    for ends in ((7,), (9,), (4, 4, 8), (6, 4, 8), (0, 8), (4, 8, 8)):  # not ending at n, not increasing, an empty range
        assert _moments(lib, ranges=(ends, (1.0,) * len(ends))) == BADARG, ends
    assert _moments(lib, ranges=((4, 8), (1.0, -1.0))) == BADARG and _moments(lib, ranges=((8,), (math.nan,))) == BADARG
    good = (1.0, 1.0, 0.9, 0.999, 0.9995, 1e-6, 1.0, math.inf)
    for i, bad in ((2, 1.0), (2, -0.1), (3, 1.0), (3, 1.5), (4, 1.0), (4, -1e-3), (5, 0.0), (5, -1e-6), (5, math.nan), (6, 0.0),
                   (6, -1.0), (7, 0.99), (7, 0.0), (7, math.nan), (7, -math.inf)):
        hp = list(good)
        hp[i] = bad
        assert _moments(lib, hp=tuple(hp)) == BADARG, (i, bad)
    for odd in range(6):
        ptrs = [OK] * 6
        ptrs[odd] = ODD
        assert _moments(lib, ptrs) == ALIGN, odd
    assert _moments(lib, ws=ODD) == ALIGN
    ptrs = [ODD] + [OK] * 5
    assert _moments(lib, ptrs, n=0) == BADARG and _moments(lib, ptrs, hp=good[:7] + (0.5,)) == BADARG  # (bad arguments first)

    for null in range(3):
        ptrs = [OK] * 3
        ptrs[null] = None
        assert _apply(lib, ptrs) == BADARG, null
    assert _apply(lib, scalars=None) == BADARG and _apply(lib, norm=None) == BADARG and _apply(lib, n=0) == BADARG
    assert lib.lora_prodigy_apply(OK, OK, OK, None, 8, None, None, None, 1, OK2, OK2, 0.9, 0.999, 1e-8, 0, 0.0, 0, None) == BADARG
    assert _apply(lib, n_ranges=0) == BADARG and _apply(lib, n_ranges=5) == BADARG
    for ends in ((7,), (9,), (4, 4, 8), (6, 4, 8), (0, 8)):
        assert _apply(lib, ranges=(ends, (1.0,) * len(ends), (0.0,) * len(ends))) == BADARG, ends
    assert _apply(lib, ranges=((4, 8), (1.0, 1.0), (0.0, -0.1))) == BADARG
    assert _apply(lib, ranges=((4, 8), (1.0, -1.0), (0.0, 0.0))) == BADARG
    for hp in ((1.0, 0.999, 1e-8), (0.9, 1.0, 1e-8), (-0.1, 0.999, 1e-8), (0.9, 0.999, -1e-8), (0.9, 0.999, math.nan)):
        assert _apply(lib, hp=hp) == BADARG, hp
    for ema in ((1.5, 0), (-0.1, 0), (0.5, -1), (math.nan, 0)):
        assert _apply(lib, shadow=OK, ema=ema) == BADARG, ema
    for odd in range(3):
        ptrs = [OK] * 3
        ptrs[odd] = ODD
        assert _apply(lib, ptrs) == ALIGN, odd
    assert _apply(lib, shadow=ODD) == ALIGN
    assert _apply(lib, [ODD, OK, OK], n=0) == BADARG


def test_check_prodigy_raises_on_each_bad_option():
    assert stp.check_prodigy("adamw") == stp.check_prodigy("prodigy") == math.sqrt(pc.f32(0.999))
    assert stp.check_prodigy("prodigy", 1e-6, 1.0, math.inf, False, False) and stp.check_prodigy("prodigy", 1e-3, 2, 1, True, True)
    with pytest.raises(ValueError, match="optimizer"):
        stp.check_prodigy("sgd")
    for kw in (dict(d0=0.0), dict(d0=-1e-6), dict(d0=math.inf), dict(d0=math.nan), dict(d0=1e-60), dict(d0=True), dict(d0="1e-6"),
               dict(d_coef=0.0), dict(d_coef=-1.0), dict(d_coef=math.inf), dict(growth_rate=0.999), dict(growth_rate=math.nan),
               dict(growth_rate=-math.inf), dict(growth_rate=None), dict(use_bias_correction=1), dict(safeguard_warmup=None),
               dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)), dict(betas=(-0.1, 0.999))):
        with pytest.raises(ValueError, match="prodigy|Prodigy"):
            stp.check_prodigy("prodigy", **kw)
    stp.check_prodigy("adamw", betas=(0.9, 1.0))  # (AdamW's betas are not Prodigy's business)


# ---- what the bounds accept and reject ------------------------------------------------------------------------------------------
def _verdict(ins, st, cfg, t, clip=False, mutant=None):
    n = ins[0].numel()
    norm_sq = pc.norm_sq_of(ins[2], cfg) if clip else 0.0
    ref = pc.reference(*ins, st, cfg, t, norm_sq)
    return pc.worst(pc.step_f32(*ins, st, cfg, t, norm_sq, mutant=mutant), ref, pc.bounds(ref, n, clip)), ref


@pytest.mark.parametrize("n", pc.ALL_SIZES)
def test_bounds_accept_the_fp32_restatement(n):
    ins = pc.inputs(n)
    for cfg, st, t, clip in pc.GRID_CONFIGS:
        w, ref = _verdict(ins, st, cfg, t, clip)
        assert max(w.values()) <= 1.0 and {"p", "m", "v", "s", "d", "d_max", "numerator", "denom", "d_hat"} <= set(w), (n, w)


def test_bounds_accept_the_ranges_the_branches_and_the_options():
    for ends, lr, wd in pc.RANGE_CASES:
        w, _ = _verdict(pc.inputs(pc.RANGE_N, plant=False), pc.MID_RUN, pc.config(ends=ends, lr=lr, wd=wd, growth_rate=1.02), 7)
        assert max(w.values()) <= 1.0, (ends, w)
    ins = pc.inputs(1027)
    seen = set()
    for cfg, st, use in ((pc.config(), pc.LEVEL, pc.inputs(1027, s_scale=30.0)), (pc.config(lr=(0.0,), wd=(0.1,)), pc.MID_RUN, ins),
                         (pc.config(safeguard=True, lr=(0.5,)), pc.MID_RUN, ins)):
        w, ref = _verdict(use, st, cfg, 7)
        seen.add(ref["state"]["branch"])
        assert max(w.values()) <= 1.0, (ref["state"]["branch"], w)
    quiet = [x.clone() for x in ins]
    for i in (2, 3, 5):
        quiet[i].zero_()
    w, ref = _verdict(quiet, pc.MID_RUN, pc.config(wd=(0.1,), lr=(0.5,)), 7)
    seen.add(ref["state"]["branch"])
    assert max(w.values()) <= 1.0 and ref["state"]["d"] == pc.MID_RUN["d"] and ref["state"]["numerator"] == pc.MID_RUN["numerator"]
    assert seen == {"d_hat below d", "all lr zero", "d_max", "denom == 0"}
    for t in (1, 2, 1000):
        w, _ = _verdict(ins, pc.MID_RUN, pc.config(bias_correction=True, wd=(0.1,)), t)
        assert max(w.values()) <= 1.0, (t, w)


MUTANT_CASE = {  # (options, scalars) at which each bug shows; the numerator is set to Σ|num_i| where its decay is the bug
    "dlr from d_new": (pc.config(wd=(0.1,)), pc.MID_RUN),
    "den from the old s": (pc.config(), pc.MID_RUN),
    "first growth rate-limited": (pc.config(growth_rate=1.02), pc.state()),
    "numerator not decayed by beta3": (pc.config(), "numerator = sum |num|"),
    "weight decay with lr instead of dlr": (pc.config(wd=(0.1,), lr=(0.5,)), pc.MID_RUN),
    "last element skipped": (pc.config(), pc.MID_RUN),
}


@pytest.mark.parametrize("mutant", pc.MUTANTS)
def test_bounds_reject_planted_bugs(mutant):
    assert set(MUTANT_CASE) == set(pc.MUTANTS) and len(pc.MUTANTS) == 6
    cfg, st = MUTANT_CASE[mutant]
    for n in (1027, 1028, pc.OVER_THE_CAP):
        ins = pc.inputs(n)
        st_n = st
        if isinstance(st, str):
            st_n = pc.state(3e-4, 5e-4, float(pc.reference(*ins, pc.MID_RUN, cfg, 7)["num"].abs().sum()))
        good, _ = _verdict(ins, st_n, cfg, 7)
        bad, _ = _verdict(ins, st_n, cfg, 7, mutant=mutant)
        assert max(good.values()) <= 1.0 < max(bad.values()), (mutant, n, bad)
    if mutant == "last element skipped":  # an unwritten last element shows at every size
        for n in pc.ALL_SIZES:
            bad, _ = _verdict(pc.inputs(n), pc.MID_RUN, pc.config(), 7, mutant=mutant)
            assert max(bad.values()) > 1.0, n


def test_chain_lengths_are_what_the_docstring_derives():
    assert [pc.sum_chain(n) for n in (1, 4, 1027, 1028, 257 * 1024, 1024 * 1024, pc.OVER_THE_CAP)] == [10, 13, 14, 13, 13, 13, 18]


# ---- the algorithm's own properties -------------------------------------------------------------------------------------------------
def test_d_is_monotone_the_growth_rate_caps_it_and_the_safeguard_form():
    ds, p, loss = pc.trajectory(pc.reference, torch.float64, steps=300)
    d0 = pc.f32(1e-6)
    assert ds[0] == d0 and all(b >= a for a, b in zip(ds, ds[1:])) and 0.005 < ds[-1] < 0.05
    assert loss[-1] < loss[0] / 20  # (the gradient noise of std 0.01 sets the floor)
    capped, _, _ = pc.trajectory(pc.reference, torch.float64, pc.config(growth_rate=1.02), steps=300)
    rate = pc.f32(1.02)
    assert all(b <= a * rate * (1 + 1e-12) for a, b in zip(capped, capped[1:]) if a != d0)
    assert any(b > a * rate * 1.5 for a, b in zip(ds, ds[1:]) if a != d0) and capped[-1] < ds[-1]
    assert sum(abs(b / a - rate) < 1e-9 for a, b in zip(capped, capped[1:])) > 100  # the cap is what holds d back
    # safeguard_warmup: s takes d where the plain form takes dlr = d·γ·bc — the same number at γ·bc = 1
    same, ps, _ = pc.trajectory(pc.reference, torch.float64, pc.config(safeguard=True))
    plain, pp, _ = pc.trajectory(pc.reference, torch.float64)
    assert same == plain and torch.equal(ps, pp)
    half_on, _, _ = pc.trajectory(pc.reference, torch.float64, pc.config(safeguard=True, lr=(0.5,)))
    half_off, _, _ = pc.trajectory(pc.reference, torch.float64, pc.config(lr=(0.5,)))
    assert half_on != half_off and all(b >= a for a, b in zip(half_on, half_on[1:]))


def test_the_fp32_trajectory_deviates_by_the_recorded_figures():
    ref_ds, ref_p, _ = pc.trajectory(pc.reference, torch.float64)
    ds, p, _ = pc.trajectory(pc.step_f32, torch.float32)
    d_rel, p_abs = pc.trajectory_deviation(ds, p, ref_ds, ref_p)
    print(f"fp32 restatement against float64 over {pc.TRAJ_STEPS} steps: d {d_rel:.3g} relative, p {p_abs:.3g} absolute")
    assert pc.TRAJ_D_REL / 1.1 <= d_rel <= pc.TRAJ_D_REL and pc.TRAJ_P_ABS / 1.1 <= p_abs <= pc.TRAJ_P_ABS
    assert ds[-1] > 1000 * ds[0] and all(b >= a for a, b in zip(ds, ds[1:]))
