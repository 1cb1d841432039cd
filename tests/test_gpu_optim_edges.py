"""The kernels of csrc/optim.hip at their grid and layout edges (MI355X): the squared-norm reduction, clip + AdamW over the
slab and over a row-structured table, the weight merge (single and batched) and the LoRA (+) LoRA interpolation.

Sizes, inputs, float64 references and the derived bounds are tests/optim_cases.py's (its docstring holds the derivations);
tests/test_optim_host.py shows on the CPU that those bounds accept the kernels' arithmetic in fp32 and reject eight planted
bugs.  Every tensor a kernel writes — p, m, v, W, x1 and the 4-float norm — is a view between sentinel bands (`Banded` of
tests/test_gpu_gemm_edges.py) that must be intact after each launch; every read-only operand is compared bit for bit with a
copy afterwards.

Bias corrections from the host's `step` and from the device counter norm[2] (`step = 0`) are the same double expression
evaluated by two math libraries; test_bias_corrections_from_host_step_and_device_counter_agree holds them to bit equality
(on an MI355X p, m and v are 0 ulps apart at every t of BIAS_STEPS).

What these tests caught when first run: the merge and the lerp were not op by op.  hipcc folded alpha·d into an fma with
the add for fp32 weights (28 % of a 37x53 layer's elements off the emulation once 16-bit factors pin d), and for fp16 folded
a product and its cast into one instruction that rounds the exact product once (1.5 – 2.5 % of the elements one ulp off at
alpha = 0.3 / 0.7, where 0.3·x and 0.7·x land on fp16 rounding ties after the fp32 rounding).  csrc/common.h's rounded_f32
now keeps each product an fp32 value first; test_lerp_is_the_emulation_bit_for_bit[f16-*] and the 16-bit rows of
test_merge_single_layer_against_the_emulation are the cases that show it."""
import functools

import pytest
import torch

from diffusion_finetuning_amd import _native as nat
from tests import optim_cases as oc
from tests.test_gpu_gemm_edges import Banded, off_by_one_element

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL_SQNORM = [n for sizes in oc.SQNORM_SIZES.values() for n in sizes]
ALL_ADAMW = [n for sizes in oc.ADAMW_SIZES.values() for n in sizes]
ALL_LERP = [n for sizes in oc.LERP_SIZES.values() for n in sizes]
TWO_ROUNDS, OVER_CAP = 257 * 1024, 1024 * 1024 + 1024 + 3


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a).cpu(), bits(b).cpu())


def held(t):
    """`t`'s values in a device view between sentinel bands."""
    t2 = t.reshape(t.shape[0], -1) if t.dim() > 1 else t.reshape(-1, 1)
    b = Banded(t2.shape[0], t2.shape[1], t.dtype)
    b.view.copy_(t2.to(DEV))
    return b


def bands_intact(b, what):
    """Banded.check without its NaN test (a flagged reduction leaves a non-finite norm[0] behind)."""
    raw = b.buf.view(b.ints)
    for name, band in (("before", raw[:b.pad]), ("after", raw[b.pad + b.n:])):
        assert torch.equal(band, torch.full_like(band, b.sentinel)), (what, "store into the band", name)
    return b.view


class Frozen:
    """A read-only operand on the device and the bits it must still hold afterwards."""

    def __init__(self, t):
        self.t = t.to(DEV).contiguous()
        self.copy = self.t.clone()

    def check(self, what):
        flat = self.t.view(torch.uint8) if self.t.dtype == torch.uint8 else bits(self.t)
        assert torch.equal(flat, self.copy.view(flat.dtype)), (what, "read-only operand changed")


def new_norm(values=(0.0, 0.0, 0.0, 0.0)):
    return held(torch.tensor(values, dtype=torch.float32))


# ---- lora_grad_sqnorm ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ALL_SQNORM)
def test_sqnorm_every_size_against_float64(n):
    g = oc.sqnorm_inputs(n)
    G = Frozen(g)
    for mul in (1.0, 1.0 / 1024):
        ref, bound = oc.sqnorm_reference(g, mul), oc.sqnorm_bound(n)
        N = new_norm()
        seen = []
        for call in range(3):
            nat.lora_grad_sqnorm(G.t, mul, N.view)
            out = N.check((n, mul, "norm")).reshape(-1).cpu()
            err = abs(float(out[0]) - ref) / ref
            if call == 0:
                print("sqnorm n=%d mul=%g: rel err %.2e (bound %.2e, L=%d)" % (n, mul, err, bound, oc.sqnorm_chain(n)))
            assert err <= bound, (n, mul, err, bound)
            # finite input: no flag, one more applied step, no skipped one
            assert out[1:].tolist() == [0.0, float(call + 1), 0.0], (n, mul, out)
            seen.append(out[:1])
        assert same_bits(seen[0], seen[1]) and same_bits(seen[0], seen[2]), (n, mul, "not repeatable", seen)
    G.check((n, "g"))


def test_sqnorm_flags_one_non_finite_element_wherever_it_sits():
    n = OVER_CAP
    lay, ranges = oc.sqnorm_launch(n), oc.sqnorm_ranges(n)
    nvec, blocks = lay["nvec"], lay["blocks"]
    where = {"element 0": 0, "last vector element": 4 * nvec - 1,
             "last block": 4 * ((blocks - 1) * 256 + 5) + 2, "second iteration": 4 * (blocks * 256 + 17) + 1}
    where.update({"tail %d" % k: 4 * nvec + k for k in range(lay["tail"])})
    assert lay["tail"] == 3 and all(where["tail %d" % k] in ranges["tail"].tolist() for k in range(3))
    assert where["last block"] in ranges["last block"].tolist() and where["last block"] < 4 * blocks * 256
    assert where["second iteration"] in ranges["second iteration"].tolist() and max(where.values()) == n - 1
    g = oc.sqnorm_inputs(n)
    work, N = g.to(DEV), new_norm()
    skipped = 0
    for value in (float("inf"), float("nan")):
        for name, i in where.items():
            keep = work[i].clone()
            work[i] = value
            nat.lora_grad_sqnorm(work, 1.0, N.view)
            out = bands_intact(N, (name, value)).reshape(-1).cpu()
            skipped += 1
            assert out[1:].tolist() == [1.0, 0.0, float(skipped)], (name, value, out)
            work[i] = keep
    assert skipped == 14
    nat.lora_grad_sqnorm(work, 1.0, N.view)  # the restored gradient: the flag clears, the applied counter starts
    out = N.check("clean").reshape(-1).cpu()
    ref = oc.sqnorm_reference(g, 1.0)
    assert abs(float(out[0]) - ref) / ref <= oc.sqnorm_bound(n) and out[1:].tolist() == [0.0, 1.0, 14.0], out


def test_sqnorm_flags_overflow_of_finite_gradients():
    n = 1027
    N = new_norm()

    def run(value, mul):
        nat.lora_grad_sqnorm(torch.full((n,), value, device=DEV), mul, N.view)
        return bands_intact(N, (value, mul)).reshape(-1).cpu()

    assert run(3e19, 1.0)[1:].tolist() == [1.0, 0.0, 1.0]          # every square is past fp32's largest number
    assert run(1e19, 1.0)[1:].tolist() == [1.0, 0.0, 2.0]          # every square is finite, their sum is not
    assert run(1e30, 1e10)[1:].tolist() == [1.0, 0.0, 3.0]         # the product with grad_mul overflows
    mul = 2.0 ** -40                                               # the loss scale's inverse rescues the first gradient
    out = run(3e19, mul)
    ref = oc.sqnorm_reference(torch.full((n,), 3e19), mul)
    assert out[1:].tolist() == [0.0, 1.0, 3.0] and abs(float(out[0]) - ref) / ref <= oc.sqnorm_bound(n), out
    assert not bool(torch.isnan(N.view).any())


def test_sqnorm_back_to_back_through_one_workspace():
    """257 blocks, then 2 blocks (255 stale partials stay behind in the workspace), then 257 again, with no host
    synchronisation in between."""
    g1, g2 = oc.sqnorm_inputs(TWO_ROUNDS), oc.sqnorm_inputs(1028, seed=1)
    G1, G2 = Frozen(g1), Frozen(g2)
    norms = [new_norm(), new_norm(), new_norm()]
    for G, N in zip((G1, G2, G1), norms):
        nat.lora_grad_sqnorm(G.t, 1.0, N.view)
    outs = [N.check("norm").reshape(-1).cpu() for N in norms]
    for out, g in zip(outs, (g1, g2, g1)):
        ref = oc.sqnorm_reference(g, 1.0)
        assert abs(float(out[0]) - ref) / ref <= oc.sqnorm_bound(g.numel()) and out[1:].tolist() == [0.0, 1.0, 0.0], out
    assert same_bits(outs[0], outs[2])
    G1.check("g1")
    G2.check("g2")


# ---- lora_adamw_step -------------------------------------------------------------------------------------------------------
def step_args(cfg, max_norm, step):
    return (cfg["mul"], max_norm, cfg["lr"], oc.BETA1, oc.BETA2, oc.EPS, cfg["wd"], step)


def assert_within(got, ref, bounds, what):
    ratios = [oc.worst_ratio(x, r, b) for x, r, b in zip(got, ref, bounds)]
    print("adamw %s: worst |err|/bound  p %.3f  m %.3f  v %.3f" % (what, *ratios))
    assert max(ratios) <= 1.0, (what, "p, m, v error / bound", ratios)


@pytest.mark.parametrize("ci", range(len(oc.ADAMW_CONFIGS)))
@pytest.mark.parametrize("n", ALL_ADAMW)
def test_adamw_step_elementwise_against_float64(n, ci):
    cfg = oc.ADAMW_CONFIGS[ci]
    p, g, m, v = oc.adamw_inputs(n)
    max_norm, step = oc.resolve_max_norm(cfg, g), cfg["step"]
    ref = oc.adamw_reference(p, g, m, v, cfg, max_norm, step)
    bounds = oc.adamw_bounds(p, g, m, v, cfg, ref[3], step, max_norm > 0)
    G, P, M, V, N = Frozen(g), held(p), held(m), held(v), new_norm()
    nat.lora_grad_sqnorm(G.t, cfg["mul"], N.view)
    norm = N.check("norm").clone()
    assert float(norm[1]) == 0.0
    nat.lora_adamw_step(P.view, G.t, M.view, V.view, N.view, *step_args(cfg, max_norm, step))
    what = (n, ci, oc.adamw_k(n, max_norm > 0))
    got = [B.check((what, name)).reshape(-1) for B, name in ((P, "p"), (M, "m"), (V, "v"))]
    assert_within(got, ref[:3], bounds, what)
    assert same_bits(N.check("norm after the step"), norm), (what, "the step wrote the norm")
    G.check((what, "g"))


@pytest.mark.parametrize("n", [257, ALL_ADAMW[-1]])
def test_adamw_step_without_a_norm(n):
    """norm_in null, step >= 1: no clip whatever max_norm says, no skip."""
    cfg = oc.ADAMW_CONFIGS[1]
    p, g, m, v = oc.adamw_inputs(n)
    ref = oc.adamw_reference(p, g, m, v, cfg, 1.0, 3, clip=False)
    bounds = oc.adamw_bounds(p, g, m, v, cfg, 1.0, 3, False)
    G, P, M, V = Frozen(g), held(p), held(m), held(v)
    nat.lora_adamw_step(P.view, G.t, M.view, V.view, None, *step_args(cfg, 1.0, 3))
    got = [B.check((n, name)).reshape(-1) for B, name in ((P, "p"), (M, "m"), (V, "v"))]
    assert_within(got, ref[:3], bounds, (n, "null norm"))
    G.check((n, "g"))


@pytest.mark.parametrize("n", [257, ALL_ADAMW[-1]])
def test_adamw_step_after_an_overflow_moves_nothing(n):
    cfg = oc.ADAMW_CONFIGS[0]
    p, g, m, v = oc.adamw_inputs(n)
    g[n // 2] = float("inf")
    G, P, M, V, N = Frozen(g), held(p), held(m), held(v), new_norm()
    nat.lora_grad_sqnorm(G.t, 1.0, N.view)
    assert bands_intact(N, "norm").reshape(-1)[1:].tolist() == [1.0, 0.0, 1.0]
    for step in (1, 0):  # the host's step count and the device's
        nat.lora_adamw_step(P.view, G.t, M.view, V.view, N.view, *step_args(cfg, 1.0, step))
        for B, t, name in ((P, p, "p"), (M, m, "m"), (V, v, "v")):
            assert same_bits(B.check((n, name)).reshape(-1), t), (n, step, name, "moved by a skipped step")


def ulps_apart(a, b):
    return int((bits(a).cpu().long() - bits(b).cpu().long()).abs().max())


@pytest.mark.parametrize("t", oc.BIAS_STEPS)
def test_bias_corrections_from_host_step_and_device_counter_agree(t):
    """`step = t` (bias corrections in double on the host) against `step = 0` with norm[2] = t (the same expression in
    double on the device) from identical state: the same bits, and both inside the float64 bounds."""
    n = 4099
    cfg = dict(oc.ADAMW_CONFIGS[4], step=t)
    p, g, m, v = oc.adamw_inputs(n)
    ref = oc.adamw_reference(p, g, m, v, cfg, 1.0, t)
    bounds = oc.adamw_bounds(p, g, m, v, cfg, ref[3], t, True)
    G = Frozen(g)
    results = []
    for step, counter in ((t, 0.0), (0, float(t - 1))):
        P, M, V, N = held(p), held(m), held(v), new_norm((0.0, 0.0, counter, 0.0))
        nat.lora_grad_sqnorm(G.t, cfg["mul"], N.view)
        assert N.check("norm").reshape(-1)[1:].tolist() == [0.0, counter + 1.0, 0.0]
        nat.lora_adamw_step(P.view, G.t, M.view, V.view, N.view, *step_args(cfg, 1.0, step))
        got = [B.check((t, step, name)).reshape(-1) for B, name in ((P, "p"), (M, "m"), (V, "v"))]
        assert_within(got, ref[:3], bounds, (t, "host step" if step else "device counter"))
        results.append(got)
    apart = [ulps_apart(a, b) for a, b in zip(*results)]
    print("t=%d: host-step and device-counter results differ by at most %s ulps (p, m, v)" % (t, apart))
    assert apart == [0, 0, 0], (t, "ulps apart (p, m, v)", apart)


# ---- lora_adamw_rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,D", oc.ROWS_SHAPES)
def test_adamw_rows_is_the_dense_update(V, D):
    for pi, pattern in enumerate(oc.ROWS_PATTERNS):
        cfg = oc.ADAMW_CONFIGS[(pi + V + D) % len(oc.ADAMW_CONFIGS)]
        what = (V, D, pattern)
        p, g, m, v, active = oc.rows_inputs(V, D, pattern)
        max_norm, step = oc.resolve_max_norm(cfg, g), cfg["step"]
        ref = oc.adamw_reference(p, g, m, v, cfg, max_norm, step)
        bounds = oc.adamw_bounds(p, g, m, v, cfg, ref[3], step, max_norm > 0)
        G, A, N = Frozen(g), Frozen(active), new_norm()
        nat.lora_grad_sqnorm(G.t.view(-1), cfg["mul"], N.view)
        norm = N.check("norm").clone()
        args = step_args(cfg, max_norm, step)
        dense = [t.reshape(-1).to(DEV) for t in (p, m, v)]
        nat.lora_adamw_step(dense[0], G.t.view(-1), dense[1], dense[2], N.view, *args)
        P, M, Vb = held(p), held(m), held(v)
        nat.lora_adamw_rows(P.view, G.t, M.view, Vb.view, A.t, N.view, *args)
        got = [B.check((what, name)) for B, name in ((P, "p"), (M, "m"), (Vb, "v"))]
        for x, d, name in zip(got, dense, "pmv"):
            assert same_bits(x.reshape(-1), d), (what, name, "row kernel and dense kernel differ")
        assert_within(got, ref[:3], bounds, what)
        # rows that never had a gradient: whatever their g, m and v hold is neither read into p nor written
        off = (active == 0).to(DEV)
        if bool(off.any()):
            g2, m2, v2 = g.clone(), m.clone(), v.clone()
            g2[active == 0], m2[active == 0], v2[active == 0] = -3.25, 123.456, 7.5
            G2, P2, M2, V2 = Frozen(g2), held(p), held(m2), held(v2)
            nat.lora_adamw_rows(P2.view, G2.t, M2.view, V2.view, A.t, N.view, *args)
            assert same_bits(P2.check((what, "p")), got[0]), (what, "p depends on an inactive row's g, m or v")
            for B, t, x, name in ((M2, m2, got[1], "m"), (V2, v2, got[2], "v")):
                after = B.check((what, name))
                assert same_bits(after[off], t.to(DEV)[off]), (what, name, "inactive rows written")
                assert same_bits(after[~off], x[~off]), (what, name, "active rows differ")
            G2.check((what, "g2"))
        assert same_bits(N.check("norm after the steps"), norm)
        G.check((what, "g"))
        A.check((what, "active"))


def test_adamw_rows_scalar_path_takes_a_table_off_a_16_byte_boundary():
    """D % 4 != 0 rows are read element by element: 4-byte alignment is enough, and the alignment check does not refuse it."""
    V, D, cfg = 5, 3, oc.ADAMW_CONFIGS[1]
    p, g, m, v, active = oc.rows_inputs(V, D, "alternating")
    args = step_args(cfg, 0.0, 3)
    dense = [t.reshape(-1).to(DEV) for t in (p, m, v)]
    gd, ad = g.to(DEV), active.to(DEV)
    nat.lora_adamw_step(dense[0], gd.view(-1), dense[1], dense[2], None, *args)
    shifted = [off_by_one_element(t.to(DEV)) for t in (p, m, v)]
    nat.lora_adamw_rows(shifted[0], gd, shifted[1], shifted[2], ad, None, *args)
    for x, d in zip(shifted, dense):
        assert same_bits(x.reshape(-1), d)


# ---- merge -----------------------------------------------------------------------------------------------------------------
def case_id(case):
    N, K, r, wd, fd = case
    return "%dx%d-r%d-%s-factors_%s" % (N, K, r, oc.NAME[wd], oc.NAME[fd])


@functools.lru_cache(maxsize=None)
def merged_single(case):
    """(inputs, the single-layer kernel's result on the CPU) of a case, computed once."""
    N, K, r, wd, fd = case
    w, a, b = oc.merge_inputs(N, K, r, wd, fd)
    W, A, B = held(w), Frozen(a), Frozen(b)
    nat.lora_merge_weight(W.view, A.t, B.t, oc.MERGE_ALPHA, fd)
    out = W.check((case_id(case), "W")).cpu()
    A.check((case_id(case), "A"))
    B.check((case_id(case), "B"))
    return (w, a, b), out


def assert_merged(got, inputs, fd, what):
    outside, off_centre = oc.merge_verdict(got, *inputs, oc.MERGE_ALPHA, fd)
    print("merge %s: %d of %d elements differ from the emulation at d, %d outside [d - e, d + e]"
          % (what, off_centre, got.numel(), outside))
    assert outside == 0, (what, "outside the emulation at d -/+ e", outside, "differing from the emulation at d", off_centre)


@pytest.mark.parametrize("case", oc.MERGE_GRID + oc.MERGE_TABLE, ids=case_id)
def test_merge_single_layer_against_the_emulation(case):
    inputs, out = merged_single(case)
    assert_merged(out, inputs, case[4], case_id(case))


@pytest.mark.parametrize("wd,fd", oc.FACTOR_ROUNDING_SHOWS, ids=lambda d: oc.NAME[d])
def test_merge_rounds_the_product_to_the_factor_dtype(wd, fd):
    w, a, b = oc.merge_inputs(37, 53, 4, wd, fd)
    outs = {}
    for held_in in (fd, oc.F32):
        W = held(w)
        nat.lora_merge_weight(W.view, a.to(DEV), b.to(DEV), oc.MERGE_ALPHA, held_in)
        outs[held_in] = W.check((oc.NAME[wd], oc.NAME[held_in])).cpu()
        assert_merged(outs[held_in], (w, a, b), held_in, (oc.NAME[wd], oc.NAME[held_in]))
    moved = int((bits(outs[fd]) != bits(outs[oc.F32])).sum())
    assert moved > w.numel() // 4, (oc.NAME[wd], oc.NAME[fd], "factor-dtype rounding moved only", moved)


def test_merge_batched_is_the_single_kernel_on_every_layer():
    singles = [merged_single(case) for case in oc.MERGE_TABLE]
    Ws = [held(inputs[0]) for inputs, _ in singles]
    As = [Frozen(inputs[1]) for inputs, _ in singles]
    Bs = [Frozen(inputs[2]) for inputs, _ in singles]
    nat.lora_merge_weight_batched([(W.view, A.t, B.t, case[4]) for W, A, B, case in zip(Ws, As, Bs, oc.MERGE_TABLE)],
                                  oc.MERGE_ALPHA)
    for W, A, B, case, (inputs, single) in zip(Ws, As, Bs, oc.MERGE_TABLE, singles):
        out = W.check((case_id(case), "batched W")).cpu()
        assert same_bits(out, single), (case_id(case), "batched and single kernels differ",
                                        int((bits(out) != bits(single)).sum()))
        assert_merged(out, inputs, case[4], case_id(case) + " batched")
        A.check(case_id(case))
        B.check(case_id(case))


# ---- lerp ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ALL_LERP)
@pytest.mark.parametrize("dtype", oc.DTYPES, ids=lambda d: oc.NAME[d])
def test_lerp_is_the_emulation_bit_for_bit(dtype, n):
    x1, x2 = oc.lerp_inputs(n, dtype)
    X2 = Frozen(x2)
    for alpha in oc.LERP_ALPHAS:
        X1 = held(x1)
        nat.lora_lerp_(X1.view, X2.t, alpha)
        got, want = X1.check((oc.NAME[dtype], n, alpha)).reshape(-1).cpu(), oc.lerp_emulate(x1, x2, alpha)
        assert same_bits(got, want), (oc.NAME[dtype], n, alpha, int((bits(got) != bits(want)).sum()), "elements differ")
    X2.check((oc.NAME[dtype], n))
