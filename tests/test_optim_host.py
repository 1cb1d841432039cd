"""CPU-only guards for the optimizer / merge / lerp edge tests (tests/test_gpu_optim_edges.py):

1. the grid constants and launch mirrors of tests/optim_cases.py are pinned to the text of csrc/optim.hip — a cap changed
   there fails here instead of moving a case out of its class;
2. every class the tables name is hit by an entry, as the mirrors compute it, and the hard-value builders put what they
   promise where they promise it;
3. at exactly the bounds the GPU file uses, the checker accepts an fp32 restatement of the kernels in their own operation
   order and rejects eight plausible bugs;
4. every entry point of optim.hip returns the status include/lora_hip.h documents for a bad argument, before any launch
   (fake pointers: nothing here reaches a device)."""
import os
import re

import pytest
import torch

from diffusion_finetuning_amd import _native as nat
from tests import optim_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "diffusion_finetuning_amd", "csrc", "optim.hip")


def _source():
    with open(SRC) as f:
        return f.read()


def _entry(src, name):
    """The text of the extern "C" entry point `name`, up to the next one."""
    i = src.index('extern "C" int %s(' % name)
    j = src.find('extern "C"', i + 1)
    return src[i:j if j > 0 else len(src)]


def _kernel(src, name):
    i = src.index("void %s(" % name)
    return src[i:src.index("\n}\n", i)]


def _int(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


def test_grid_constants_match_the_source():
    src = _source()
    assert _int(r"constexpr int kMaxBlocks = (\d+);", src) == oc.SQNORM_MAX_BLOCKS
    assert set(re.findall(r"__launch_bounds__\((\d+)\)", src)) == {str(oc.THREADS)}
    assert len(re.findall(r"dim3\(256\)", src)) == src.count("hipLaunchKernelGGL(")  # every launch: 256 threads

    sq = _entry(src, "lora_grad_sqnorm")
    m = re.search(r"int64_t blocks = \(n / (\d+) \+ (\d+)\) / (\d+);", sq)
    assert m and (int(m[1]), int(m[2]) + 1, int(m[3])) == (oc.SQNORM_VEC, oc.THREADS, oc.THREADS)
    assert "if (blocks > kMaxBlocks) blocks = kMaxBlocks;" in sq and "if (blocks < 1) blocks = 1;" in sq
    k = _kernel(src, "grad_sqnorm_kernel")
    for line in ("const int64_t nvec = n >> 2;",
                 "for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {",
                 "if (blockIdx.x == 0) {",
                 "for (int64_t i = (nvec << 2) + threadIdx.x; i < n; i += 256) {",
                 "for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) {"):
        assert line in k, line
    assert "16 + 2 * kMaxBlocks * 4" in src  # the workspace: ticket header, partials, flags

    for name, cap in (("lora_adamw_step", oc.ADAMW_MAX_BLOCKS), ("lora_lerp", oc.LERP_MAX_BLOCKS)):
        body = _entry(src, name)
        m = re.search(r"int64_t blocks = \(n \+ (\d+)\) / (\d+);\s*if \(blocks > (\d+)\) blocks = (\d+);", body)
        assert m and [int(x) for x in m.groups()] == [oc.THREADS - 1, oc.THREADS, cap, cap], name
    for name in ("adamw_kernel", "lerp_kernel"):
        assert re.search(r"for \(int64_t i = \(int64_t\)blockIdx\.x \* 256 \+ threadIdx\.x; i < (a\.)?n; "
                         r"i \+= \(int64_t\)gridDim\.x \* 256\)", _kernel(src, name)), name

    rows = _entry(src, "lora_adamw_rows")
    m = re.search(r"const int64_t blocks = V < (\d+) \? V : (\d+);", rows)
    assert m and int(m[1]) == int(m[2]) == oc.ROWS_MAX_BLOCKS
    k = _kernel(src, "adamw_rows_kernel")
    for line in ("for (int64_t row = blockIdx.x; row < V; row += gridDim.x) {", "if ((D & 3) == 0) {",
                 "for (int c = threadIdx.x; c < D / 4; c += 256) {",
                 "for (int c = threadIdx.x; c < D; c += 256) a.p[base + c] = a.p[base + c] * decay;",
                 "for (int c = threadIdx.x; c < D; c += 256) {"):
        assert line in k, line

    merge = _entry(src, "lora_merge_weight")
    m = re.search(r"int64_t blocks = \(\(int64_t\)N \* K \+ (\d+)\) / (\d+);\s*if \(blocks > (\d+)\) blocks = (\d+);", merge)
    assert m and [int(x) for x in m.groups()] == [oc.THREADS - 1, oc.THREADS, oc.MERGE_MAX_BLOCKS, oc.MERGE_MAX_BLOCKS]
    batched = _entry(src, "lora_merge_weight_batched")
    m = re.search(r"int64_t blocks = \(max_elems \+ (\d+)\) / (\d+);.*\n\s*if \(blocks > (\d+)\) blocks = (\d+);", batched)
    assert m and [int(x) for x in m.groups()] == [oc.BATCHED_ELEMS_PER_BLOCK - 1, oc.BATCHED_ELEMS_PER_BLOCK,
                                                  oc.BATCHED_MAX_BLOCKS, oc.BATCHED_MAX_BLOCKS]
    assert "dim3((unsigned)blocks, (unsigned)n_layers)" in batched
    stride = "for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {"
    assert stride in _kernel(src, "merge_kernel") and stride in _kernel(src, "merge_rows")


def test_restated_arithmetic_matches_the_source():
    """adamw_f32 and merge_emulate restate these lines; a change to them must come with a change to the restatement."""
    src = _source()
    with open(os.path.join(os.path.dirname(SRC), "common.h")) as f:
        common = f.read()
    for line in ("p = p * decay;", "m = m + (g - m) * (1.f - beta1);", "v = beta2 * v + (1.f - beta2) * g * g;",
                 "const float denom = sqrtf(v) / bc2_sqrt + eps;", "p = p - step_size * (m / denom);"):
        assert line in common, line
    for name in ("adamw_kernel", "adamw_rows_kernel"):
        k = _kernel(src, name)
        for line in ("const float c = a.max_norm / (sqrtf(a.norm_in[0]) + 1e-6f);", "clip = c < 1.f ? c : 1.f;",
                     "const float gm = a.grad_mul * clip;", "const float step_size = a.lr / bc1;",
                     "const float decay = 1.f - a.lr * a.wd;", "const float g = a.g[i] * gm;"):
            assert line in k, (name, line)
    for name in ("merge_kernel", "merge_rows"):
        k = _kernel(src, name)
        for line in ("for (int j = 0; j < r; ++j) d = fmaf(B[(int64_t)n * r + j], A[(int64_t)j * K + k], d);",
                     "if (factor_dtype == LORA_F16) d = to_f32<half_t>(from_f32<half_t>(d));",
                     "if (factor_dtype == LORA_BF16) d = to_f32<bf16_t>(from_f32<bf16_t>(d));",
                     "const T dt = from_f32<T>(rounded_f32(d));",
                     "const T upd = from_f32<T>(rounded_f32(alpha * to_f32<T>(dt)));",
                     "W[i] = from_f32<T>(to_f32<T>(W[i]) + to_f32<T>(upd));"):
            assert line in k, (name, line)
    k = _kernel(src, "lerp_kernel")
    for line in ("const T p = from_f32<T>(rounded_f32(a * to_f32<T>(x1[i])));",
                 "const T q = from_f32<T>(rounded_f32(b * to_f32<T>(x2[i])));",
                 "x1[i] = from_f32<T>(to_f32<T>(p) + to_f32<T>(q));"):
        assert line in k, line
    assert 'asm("" : "+v"(x));' in common  # rounded_f32: the product is an fp32 register before anything consumes it


def test_every_size_class_is_hit():
    for n_class, sizes in oc.SQNORM_SIZES.items():
        for n in sizes:
            assert oc.sqnorm_class(n) == n_class, (n, oc.sqnorm_class(n))
    lay = {n: oc.sqnorm_launch(n) for sizes in oc.SQNORM_SIZES.values() for n in sizes}
    assert all(lay[n]["nvec"] == 0 and lay[n]["tail"] == n and lay[n]["blocks"] == 1 for n in (1, 2, 3))
    assert (lay[4]["nvec"], lay[4]["tail"], lay[4]["blocks"]) == (1, 0, 1)
    assert (lay[1027]["nvec"], lay[1027]["tail"], lay[1027]["blocks"]) == (256, 3, 1)
    assert (lay[1028]["blocks"], lay[1028]["threads_in_last_iter"]) == (2, 257)
    assert (lay[257 * 1024]["blocks"], lay[257 * 1024]["rounds"], lay[257 * 1024]["iters"]) == (257, 2, 1)
    at = lay[1024 * 1024]
    assert (at["blocks"], at["iters"], at["threads_in_last_iter"], at["tail"]) == (1024, 1, 1024 * 256, 0)
    over = lay[1024 * 1024 + 1024 + 3]
    assert (over["blocks"], over["iters"], over["threads_in_last_iter"], over["tail"]) == (1024, 2, 256, 3)

    for table, cap, blocks in ((oc.ADAMW_SIZES, oc.ADAMW_MAX_BLOCKS, oc.adamw_blocks),
                               (oc.LERP_SIZES, oc.LERP_MAX_BLOCKS, oc.lerp_blocks)):
        for n_class, sizes in table.items():
            for n in sizes:
                assert oc.stream_class(n, cap) == n_class, (n, n_class)
                assert blocks(n) == min((n + 255) // 256, cap)
        assert any(n > cap * 256 and n % 256 for sizes in table.values() for n in sizes)  # a ragged second iteration
    assert set(oc.ADAMW_SIZES) == {"one thread", "partial block", "full block", "two blocks", "at the cap", "over the cap"}
    assert {n for s in oc.LERP_SIZES.values() for n in s} == {1, 255, 257, 2048 * 256 + 3}
    assert set(oc.LERP_ALPHAS) == {0.5, 0.3, 1.0, 0.0}

    shapes = set(oc.ROWS_SHAPES)
    assert {V for V, _ in shapes} == {1, 300, 4097} and {D for _, D in shapes} == {1, 3, 4, 6, 64, 260, 1028, 1030}
    lays = {s: oc.rows_launch(*s) for s in shapes}
    assert any(l["row_stride"] for l in lays.values()) and oc.rows_launch(4097, 4)["blocks"] == 4096
    assert not lays[(300, 3)]["vec"] and not lays[(300, 1)]["vec"]                       # scalar, below 4 columns
    assert not lays[(300, 6)]["vec"] and 6 % 4 == 2
    assert all(lays[(300, D)]["vec"] and lays[(300, D)]["idle_cols"] for D in (4, 64, 260))   # D/4 < 256
    assert lays[(300, 1028)]["vec"] and lays[(300, 1028)]["col_stride_inactive"] and 1028 // 4 == 257
    assert not lays[(300, 1030)]["vec"] and lays[(300, 1030)]["col_stride_inactive"]     # scalar path past 256 columns
    assert lays[(300, 260)]["col_stride_active"] and not lays[(300, 260)]["col_stride_inactive"]
    assert max(V * D for V, D in shapes) * 4 < 4 << 20
    assert set(oc.ROWS_PATTERNS) == {"none", "all", "first", "last", "alternating"}
    for V in oc.ROWS_V:
        assert {int(oc.rows_active(V, p).sum()) for p in oc.ROWS_PATTERNS} >= {0, V, 1, (V + 1) // 2}

    assert {(w, f) for _, _, _, w, f in oc.MERGE_GRID} == {(w, f) for w in oc.DTYPES for f in oc.DTYPES}
    assert all(N % 4 and K % 4 for N, K, *_ in oc.MERGE_GRID)
    cases = oc.MERGE_GRID + oc.MERGE_TABLE
    assert {r for _, _, r, _, _ in cases} >= {1, 4, 16, 64} and any(r == min(N, K) for N, K, r, _, _ in cases)
    assert all(1 <= r <= min(N, K) for N, K, r, _, _ in cases)
    big = max(N * K for N, K, *_ in oc.MERGE_TABLE)
    assert big > oc.MERGE_MAX_BLOCKS * 256 and oc.merge_blocks(big) == oc.MERGE_MAX_BLOCKS       # the single kernel strides
    assert oc.batched_blocks(big) == oc.BATCHED_MAX_BLOCKS and big > oc.BATCHED_MAX_BLOCKS * 256  # so does the batched one
    assert len(oc.MERGE_TABLE) >= 5 and {w for *_, w, _ in oc.MERGE_TABLE} == set(oc.DTYPES)
    assert len({f for *_, f in oc.MERGE_TABLE}) >= 2 and min(N * K for N, K, *_ in oc.MERGE_TABLE) == 64
    assert oc.batched_blocks(big) * 256 > 64                                                     # idle blocks on the 8x8 layer


def test_builders_hold_the_hard_values():
    for sizes in oc.SQNORM_SIZES.values():
        for n in sizes:
            g = oc.sqnorm_inputs(n)
            assert g.dtype == torch.float32 and bool(torch.isfinite(g).all()) and torch.equal(g, oc.sqnorm_inputs(n))
            if n > 64:
                assert float(g.abs().min()) <= 1e-12 and float(g.abs().max()) >= 1e4
            for mul in (1.0, 1.0 / 1024):
                mass = oc.sqnorm_mass(g, mul)
                assert set(mass) == set(oc.sqnorm_ranges(n)) and all(share >= 1e-3 for share in mass.values()), (n, mass)
                assert oc.sqnorm_bound(n) < 1e-5  # a dropped range moves the sum by 100 times the tolerance at least
    assert set(oc.sqnorm_ranges(1024 * 1024 + 1024 + 3)) == {"tail", "last block", "second iteration"}
    assert set(oc.sqnorm_ranges(257 * 1024)) == {"last block"} and set(oc.sqnorm_ranges(1027)) == {"tail"}
    p, g, m, v = oc.adamw_inputs(2048 * 256 + 257)
    assert float(g.abs().max()) == 1e4 and float(g[g != 0].abs().min()) <= 1e-12
    assert bool(((g == 0) & (m != 0) & (v != 0)).any()) and bool(((g == 0) & (m == 0) & (v == 0)).any())
    assert bool(((p.abs() > 9e3) & (g.abs() < 1e-9)).any()) and bool(((g != 0) & (v == 0)).any())
    assert bool((v >= 0).all()) and p.numel() * 4 < 4 << 20
    assert {c["wd"] for c in oc.ADAMW_CONFIGS} == {0.0, 1e-2, 0.1} and {c["lr"] for c in oc.ADAMW_CONFIGS} == {1e-4, 1e-1}
    assert {c["mul"] for c in oc.ADAMW_CONFIGS} == {1.0, 1.0 / 1024}
    assert {c["max_norm"] for c in oc.ADAMW_CONFIGS} == {0.0, 1.0, 1e9, oc.BOUNDARY}
    cfg = next(c for c in oc.ADAMW_CONFIGS if c["max_norm"] == oc.BOUNDARY)
    norm = oc.sqnorm_reference(g, cfg["mul"]) ** 0.5
    assert abs(oc.resolve_max_norm(cfg, g) - norm) <= 1e-6 * norm
    for V, D in ((300, 6), (1, 4)):
        for pattern in oc.ROWS_PATTERNS:
            p, g, m, v, active = oc.rows_inputs(V, D, pattern)
            off = active == 0
            assert not bool(g[off].any()) and not bool(m[off].any()) and not bool(v[off].any())


# ---- sensitivity of the bounds ---------------------------------------------------------------------------------------------
ALL_SQNORM = [n for sizes in oc.SQNORM_SIZES.values() for n in sizes]
ALL_ADAMW = [n for sizes in oc.ADAMW_SIZES.values() for n in sizes]


def _sq_err(n, mul, mutant=None):
    g = oc.sqnorm_inputs(n)
    ref = oc.sqnorm_reference(g, mul)
    return abs(oc.sqnorm_f32(g, mul, mutant) - ref) / ref


@pytest.mark.parametrize("n", ALL_SQNORM)
def test_sqnorm_bound_accepts_the_fp32_reduction_tree(n):
    for mul in (1.0, 1.0 / 1024):
        assert _sq_err(n, mul) <= oc.sqnorm_bound(n), (n, mul, _sq_err(n, mul), oc.sqnorm_bound(n))


def test_sqnorm_bound_rejects_dropped_ranges():
    over, two_rounds = 1024 * 1024 + 1024 + 3, 257 * 1024
    for n, mutant in ((1, "skip last tail element"), (3, "skip last tail element"), (1027, "skip last tail element"),
                      (over, "skip last tail element"), (over, "skip second iteration"), (two_rounds, "drop a partial"),
                      (over, "drop a partial"), (1028, "drop a partial")):
        for mul in (1.0, 1.0 / 1024):
            assert _sq_err(n, mul, mutant) > 100 * oc.sqnorm_bound(n), (n, mutant, mul)


def _adamw_verdict(n, cfg, mutant=None):
    """Worst |error| / bound over p, m, v of the fp32 restatement (with its own fp32 norm) against float64."""
    p, g, m, v = oc.adamw_inputs(n)
    max_norm = oc.resolve_max_norm(cfg, g)
    clipping = max_norm > 0
    ref_p, ref_m, ref_v, coef = oc.adamw_reference(p, g, m, v, cfg, max_norm, cfg["step"])
    bounds = oc.adamw_bounds(p, g, m, v, cfg, coef, cfg["step"], clipping)
    got = oc.adamw_f32(p, g, m, v, cfg, max_norm, cfg["step"], oc.sqnorm_f32(g, cfg["mul"]), mutant)
    return max(oc.worst_ratio(x, r, b) for x, r, b in zip(got, (ref_p, ref_m, ref_v), bounds))


@pytest.mark.parametrize("n", ALL_ADAMW)
def test_adamw_bounds_accept_the_fp32_update(n):
    for cfg in oc.ADAMW_CONFIGS:
        worst = _adamw_verdict(n, cfg)
        assert worst <= 1.0, (n, cfg, worst)
    # the null-norm route
    p, g, m, v = oc.adamw_inputs(n)
    cfg = oc.ADAMW_CONFIGS[1]
    ref = oc.adamw_reference(p, g, m, v, cfg, 1.0, 3, clip=False)
    bounds = oc.adamw_bounds(p, g, m, v, cfg, 1.0, 3, False)
    got = oc.adamw_f32(p, g, m, v, cfg, 1.0, 3, None)
    assert max(oc.worst_ratio(x, r, b) for x, r, b in zip(got, ref[:3], bounds)) <= 1.0


MUTANT_CONFIG = {  # the sampled configuration at which each bug shows
    "eps inside the square root": 0, "bias correction 2 without its root": 0, "weight decay after the Adam term": 1,
    "clip coefficient not applied": 4, "grad_mul applied twice": 1, "last element skipped": 1,
}


@pytest.mark.parametrize("mutant", oc.ADAMW_MUTANTS)
def test_adamw_bounds_reject_planted_bugs(mutant):
    assert set(MUTANT_CONFIG) == set(oc.ADAMW_MUTANTS) and len(oc.ADAMW_MUTANTS) == 6
    cfg = oc.ADAMW_CONFIGS[MUTANT_CONFIG[mutant]]
    for n in (257, 2048 * 256 + 257):
        assert _adamw_verdict(n, cfg) <= 1.0 < _adamw_verdict(n, cfg, mutant), (mutant, n)
    if mutant == "last element skipped":  # an unwritten last element shows at every size and configuration
        for n in ALL_ADAMW:
            for cfg in oc.ADAMW_CONFIGS:
                assert _adamw_verdict(n, cfg, mutant) > 1.0, (n, cfg)


def test_k_and_l_are_what_the_docstring_derives():
    assert [oc.sqnorm_chain(n) for n in (1, 4, 1027, 1028, 257 * 1024, 1024 * 1024, 1024 * 1024 + 1027)] == \
        [20, 23, 24, 23, 24, 26, 31]
    assert oc.adamw_k(1, False) == (4, 5, 20)
    assert oc.grad_k(257, True) == 20 and oc.adamw_k(257, True) == (23, 43, 58)
    assert oc.adamw_k(2048 * 256 + 257, True)[2] == 58 + 2 * (oc.grad_k(2048 * 256 + 257, True) - 20)


def test_merge_and_lerp_emulations():
    # factor-dtype rounding moves the merged weight where it can
    for wd, fd in oc.FACTOR_ROUNDING_SHOWS:
        w, a, b = oc.merge_inputs(37, 53, 4, wd, fd)
        held, _ = oc.merge_emulate(w, a, b, oc.MERGE_ALPHA, fd)
        plain, _ = oc.merge_emulate(w, a, b, oc.MERGE_ALPHA, oc.F32)
        assert int((held != plain).sum()) > w.numel() // 4, (wd, fd)
    # the emulation is the reference's expression where that is exact on the CPU: fp32 weights, fp32 factors
    w, a, b = oc.merge_inputs(37, 53, 4, oc.F32, oc.F32)
    got, e = oc.merge_emulate(w, a, b, oc.MERGE_ALPHA, oc.F32)
    want = w.double() + oc.f32(oc.MERGE_ALPHA) * (b.double() @ a.double())
    assert float((got.double() - want).abs().max()) < 4 * oc.U * float(want.abs().max()) and float(e.max()) < 1e-5
    assert oc.merge_verdict(got, w, a, b, oc.MERGE_ALPHA, oc.F32) == (0, 0)
    bad = got.clone()
    bad[-1, -1] = w[-1, -1]                             # an element the merge never reached
    assert oc.merge_verdict(bad, w, a, b, oc.MERGE_ALPHA, oc.F32)[0] == 1
    # lerp: fp32 is torch's own expression bit for bit; alpha = 1 and 0 return the operands
    for dtype in oc.DTYPES:
        x1, x2 = oc.lerp_inputs(257, dtype)
        assert torch.equal(oc.lerp_emulate(x1, x2, 1.0), x1) and torch.equal(oc.lerp_emulate(x1, x2, 0.0), x2)
        assert bool((x2[5::11] == -x1[5::11]).all())
    x1, x2 = oc.lerp_inputs(257, oc.F32)
    assert torch.equal(oc.lerp_emulate(x1, x2, 0.3), 0.3 * x1 + (1 - 0.3) * x2)


# ---- argument validation: no launch ----------------------------------------------------------------------------------------
OK, OK2, ODD = 0x10000, 0x20000, 0x10004  # fake device pointers: 16-byte aligned, and 4 bytes past a 16-byte boundary
HP = (1.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-2)  # grad_mul, max_norm, lr, beta1, beta2, eps, weight_decay


def test_status_codes_are_the_header_ones():
    with open(os.path.join(ROOT, "include", "lora_hip.h")) as f:
        h = f.read()
    for name, code in (("LORA_OK", 0), ("LORA_E_BADARG", -1), ("LORA_E_RANK", -2), ("LORA_E_ALIGN", -3)):
        assert re.search(r"\b%s = %d\b" % (name, code), h), name
    assert "LORA_E_ALIGN when D % 4 == 0 and `param` is not 16-byte aligned" in h


def test_argument_validation_of_the_optimizer_entries():
    lib = nat.lib()
    BADARG, RANK, ALIGN = -1, -2, -3
    sq = lib.lora_grad_sqnorm
    assert sq(None, 8, 1.0, OK, OK2, None) == BADARG and sq(OK, 8, 1.0, None, OK2, None) == BADARG
    assert sq(OK, 8, 1.0, OK2, None, None) == BADARG
    assert sq(OK, 0, 1.0, OK2, OK2, None) == BADARG and sq(OK, -4, 1.0, OK2, OK2, None) == BADARG
    assert sq(ODD, 8, 1.0, OK2, OK2, None) == ALIGN and sq(OK, 8, 1.0, OK2, ODD, None) == ALIGN

    step = lib.lora_adamw_step
    assert step(OK, OK, OK, OK, 8, OK2, *HP, -1, None) == BADARG
    assert step(OK, OK, OK, OK, 8, None, *HP, 0, None) == BADARG   # step 0 reads the device counter of a norm it was not given
    assert step(OK, OK, OK, OK, 0, OK2, *HP, 1, None) == BADARG
    for null in range(4):
        ptrs = [OK] * 4
        ptrs[null] = None
        assert step(*ptrs, 8, OK2, *HP, 1, None) == BADARG

    rows = lib.lora_adamw_rows
    assert rows(OK, OK, OK, OK, OK2, 4, 8, OK2, *HP, -1, None) == BADARG
    assert rows(OK, OK, OK, OK, OK2, 4, 8, None, *HP, 0, None) == BADARG
    assert rows(OK, OK, OK, OK, OK2, 0, 8, OK2, *HP, 1, None) == BADARG
    assert rows(OK, OK, OK, OK, OK2, 4, 0, OK2, *HP, 1, None) == BADARG
    assert rows(OK, OK, OK, OK, None, 4, 8, OK2, *HP, 1, None) == BADARG
    # rows of whole 16-byte chunks take the float4 path: a table off a 16-byte boundary is refused, with or without a norm
    for D in (4, 8, 1028):
        assert rows(ODD, OK, OK, OK, OK2, 4, D, OK2, *HP, 1, None) == ALIGN
        assert rows(ODD, OK, OK, OK, OK2, 4, D, None, *HP, 1, None) == ALIGN
        assert rows(OK + 8, OK, OK, OK, OK2, 4, D, OK2, *HP, 0, None) == ALIGN
    assert rows(ODD, OK, OK, OK, OK2, 4, 8, OK2, *HP, -1, None) == BADARG  # (bad arguments are named first)
    assert rows(ODD, OK, OK, OK, None, 4, 6, OK2, *HP, 1, None) == BADARG


def test_argument_validation_of_merge_lerp_and_cast():
    lib = nat.lib()
    BADARG, RANK = -1, -2
    merge = lib.lora_merge_weight
    assert merge(OK, OK, OK, 8, 6, 0, 1.0, 0, 0, None) == RANK and merge(OK, OK, OK, 8, 6, -1, 1.0, 0, 0, None) == RANK
    assert merge(OK, OK, OK, 8, 6, 7, 1.0, 0, 0, None) == RANK and merge(OK, OK, OK, 6, 8, 7, 1.0, 1, 0, None) == RANK
    assert merge(OK, OK, OK, 8, 6, 4, 1.0, 3, 0, None) == BADARG and merge(OK, OK, OK, 8, 6, 4, 1.0, -1, 0, None) == BADARG
    assert merge(None, OK, OK, 8, 6, 4, 1.0, 0, 0, None) == BADARG and merge(OK, OK, OK, 0, 6, 4, 1.0, 0, 0, None) == BADARG
    batched = lib.lora_merge_weight_batched
    assert batched(None, 3, 64, 1.0, None) == BADARG and batched(OK, 0, 64, 1.0, None) == BADARG
    assert batched(OK, 3, 0, 1.0, None) == BADARG
    lerp = lib.lora_lerp
    assert lerp(OK, OK2, 0, 0.5, 0.5, 0, None) == BADARG and lerp(OK, OK2, -1, 0.5, 0.5, 1, None) == BADARG
    assert lerp(OK, OK2, 8, 0.5, 0.5, 3, None) == BADARG and lerp(None, OK2, 8, 0.5, 0.5, 0, None) == BADARG
    cast = lib.lora_cast_matrix
    assert cast(OK, OK2, 0, 8, 0, 1, 0, None) == BADARG and cast(OK, OK2, 8, 0, 0, 1, 1, None) == BADARG
    assert cast(OK, OK2, 8, 8, 5, 1, 0, None) == BADARG and cast(OK, OK2, 8, 8, 0, 5, 0, None) == BADARG
