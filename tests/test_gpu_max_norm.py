"""`lora_max_norm` (csrc/max_norm.hip) on an MI355X through the C-ABI, against the float64 restatement of
tests/max_norm_cases.py, and the two public helpers on the tiny UNet.

Layout of every buffer here: a guard of an ODD number of sentinel elements (so `params` itself is only 4-byte aligned and
most layers start off a 16-byte boundary), the layers as [up | down] with 3 sentinel elements between them, a guard behind.
Whatever the kernel must not touch — guards, padding, layers inside the bound — is compared BIT FOR BIT with what was sent."""
import math

import pytest
import torch

import diffusion_finetuning_amd as dfa
from diffusion_finetuning_amd import _native as nat
from tests import max_norm_cases as mc
from tests.conftest import build_tiny_unet

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 253
PAD = 3
SENTINEL = -1234.5
U = mc.U


class Slab:
    """Host image of a test slab: `buf` with guards, `rows` for the table (offsets from buf[GUARD]), `spans` [(a, b)] of each
    layer inside buf."""

    def __init__(self, layers):
        """layers: [(up, down, scale)]"""
        total = 2 * GUARD + sum(u.numel() + d.numel() + PAD for u, d, _ in layers)
        self.buf = torch.full((total,), SENTINEL, dtype=torch.float32)
        self.rows, self.spans, self.layers = [], [], layers
        at = GUARD
        for up, down, scale in layers:
            (N, r), K = up.shape, down.shape[1]
            self.buf[at:at + N * r] = up.reshape(-1)
            self.buf[at + N * r:at + N * r + r * K] = down.reshape(-1)
            self.rows.append((at - GUARD, at - GUARD + N * r, K, N, r, scale))
            self.spans.append((at, at + N * r + r * K))
            at += N * r + r * K + PAD
        self.max_r = max(row[4] for row in self.rows)

    def run(self, max_norm, dev=None, counters=None):
        """One launch on a device copy of `buf` (or on `dev`, a buffer of an earlier launch): (device buffer, stats on the host)."""
        dev = self.buf.to(DEV) if dev is None else dev
        table = nat.max_norm_table(self.rows, DEV)
        stats = torch.full((len(self.rows), 2), math.nan, dtype=torch.float32, device=DEV)
        nat.lora_max_norm(dev[GUARD:], table, self.max_r, max_norm, stats, counters)
        torch.cuda.synchronize()
        return dev, stats.cpu()

    def outside(self, image):
        """The elements of a buffer image that belong to no layer."""
        keep = torch.ones(image.numel(), dtype=torch.bool)
        for a, b in self.spans:
            keep[a:b] = False
        return image[keep]


def check_layers(slab, before, after, stats, max_norm, what):
    """The three write rules, layer by layer and around them; returns the number of layers scaled."""
    scaled = 0
    for l, ((a, b), (up, down, scale)) in enumerate(zip(slab.spans, slab.layers)):
        norm_ref, factor_ref, _, _ = mc.reference(up, down, scale, max_norm)
        norm, factor = float(stats[l, 0]), float(stats[l, 1])
        if factor_ref == 1.0:
            assert factor == 1.0, (what, l, "a layer inside the bound got a factor", norm, norm_ref, factor)
            assert mc.same_bits(after[a:b], before[a:b]), (what, l, "a layer inside the bound was written")
        else:
            assert factor != 1.0 and 0.0 < factor < 1.0, (what, l, norm, norm_ref, factor)
            want = before[a:b] * torch.tensor(factor, dtype=torch.float32)  # one fp32 multiply per element
            differ = int((mc.bits(after[a:b]) != mc.bits(want)).sum())
            assert differ == 0, (what, l, "elements that are not before·factor", differ)
            scaled += 1
    assert mc.same_bits(slab.outside(after), slab.outside(before)), (what, "guards or padding were written")
    assert bool((slab.outside(after) == SENTINEL).all())
    return scaled


def check_accuracy(slab, stats, max_norm, what):
    """The reported norm and factor against the restatement, within the derived bound of max_norm_cases.norm_squared_bound."""
    for l, (up, down, scale) in enumerate(slab.layers):
        norm_ref, factor_ref, _, _ = mc.reference(up, down, scale, max_norm)
        bound = mc.norm_squared_bound(up, down, scale)
        norm, factor = float(stats[l, 0]), float(stats[l, 1])
        err = abs(norm * norm - norm_ref * norm_ref)
        print(f"[{what}] layer {l} r,K,N={down.shape[0]},{down.shape[1]},{up.shape[0]}: norm {norm!r} ref {norm_ref!r} "
              f"|Δn²| {err:.3e} bound {bound:.3e} factor {factor!r} ref {factor_ref!r}")
        assert err <= bound, (what, l, norm, norm_ref, err, bound)
        if factor_ref != 1.0:
            rel = abs(factor - factor_ref) / factor_ref
            assert rel <= bound / (2 * norm_ref * norm_ref) + U, (what, l, factor, factor_ref, rel)


def case_layers(cases):
    return [mc.layer(*c) for c in cases]


@pytest.fixture(scope="module")
def table_run():
    """Every shape in every regime in ONE table, clamped once at BOUND, then measured again with max_norm = inf."""
    slab = Slab(case_layers(mc.table_layers()))
    counters = torch.zeros(1, dtype=torch.int32, device=DEV)
    dev, stats = slab.run(mc.BOUND, counters=counters)
    after = dev.cpu()
    dev2, stats_after = slab.run(math.inf, dev=dev.clone(), counters=counters)
    return slab, after, stats, stats_after, dev2.cpu(), int(counters.cpu()[0])


# -- 1. what is written ----------------------------------------------------------------------------------------------------------
def test_one_table_of_every_case_writes_only_the_layers_above_the_bound(table_run):
    slab, after, stats, _, _, count = table_run
    scaled = check_layers(slab, slab.buf, after, stats, mc.BOUND, "table")
    assert scaled == len(mc.SHAPES)  # the "above" regime, and nothing of "below" or "on"
    assert count == scaled  # the measuring launch that followed added nothing
    for l, case in enumerate(mc.table_layers()):
        if case[3] == "on":
            assert float(stats[l, 0]) == mc.BOUND and float(stats[l, 1]) == 1.0, (case, stats[l])


@pytest.mark.parametrize("case", mc.table_layers(), ids=lambda c: "r{}-K{}-N{}-{}".format(*c))
def test_each_case_alone(case):
    slab = Slab(case_layers([case]))
    dev, stats = slab.run(mc.BOUND)
    scaled = check_layers(slab, slab.buf, dev.cpu(), stats, mc.BOUND, "alone")
    assert scaled == (1 if case[3] == "above" else 0)
    check_accuracy(slab, stats, mc.BOUND, "alone")


# -- 2. accuracy -----------------------------------------------------------------------------------------------------------------
def test_reported_norms_and_factors_are_within_the_derived_bound(table_run):
    slab, _, stats, _, _, _ = table_run
    check_accuracy(slab, stats, mc.BOUND, "table")


def test_a_clamped_layer_measures_at_most_the_bound_afterwards(table_run):
    slab, after, stats, stats_after, after2, _ = table_run
    assert mc.same_bits(after2, after)  # max_norm = inf wrote nothing but stats
    assert bool((stats_after[:, 1] == 1.0).all())
    for l, ((a, b), (up, down, scale)) in enumerate(zip(slab.spans, slab.layers)):
        (N, r), K = up.shape, down.shape[1]
        up2, down2 = after[a:a + N * r].view(N, r), after[a + N * r:b].view(r, K)
        bound = mc.norm_squared_bound(up2, down2, scale)  # of the factors as they are now
        norm = float(stats_after[l, 0])
        limit = (mc.BOUND * (1 + 4 * U)) ** 2 + bound
        print(f"[after] layer {l}: norm {norm!r} norm² − BOUND² {norm * norm - mc.BOUND ** 2:.3e} bound {bound:.3e}")
        assert norm * norm <= limit, (l, norm, bound)
        if float(stats[l, 1]) != 1.0:  # and a scaled layer lands ON the bound, not somewhere below it
            assert norm * norm >= (mc.BOUND * (1 - 4 * U)) ** 2 - bound, (l, norm)
        else:
            assert norm == float(stats[l, 0])


# -- 3. corner inputs ------------------------------------------------------------------------------------------------------------
def test_zero_up_has_norm_zero_factor_one_and_keeps_its_bits():
    layers = []
    for r, K, N in mc.SHAPES:
        up, down, scale = mc.layer(r, K, N, "above")
        layers.append((torch.zeros_like(up), down, scale))
    slab = Slab(layers)
    dev, stats = slab.run(1e-3)
    after = dev.cpu()
    assert torch.equal(stats, torch.tensor([[0.0, 1.0]] * len(layers)))
    assert mc.same_bits(after, slab.buf) and bool(torch.isfinite(after).all())


def test_infinite_bound_measures_only():
    slab = Slab(case_layers([(r, K, N, "above") for r, K, N in mc.SHAPES]))
    counters = torch.zeros(1, dtype=torch.int32, device=DEV)
    dev, stats = slab.run(math.inf, counters=counters)
    assert mc.same_bits(dev.cpu(), slab.buf) and int(counters.cpu()[0]) == 0
    assert bool((stats[:, 1] == 1.0).all()) and bool((stats[:, 0] >= 2 * mc.BOUND * (1 - 1e-3)).all())
    check_accuracy(slab, stats, math.inf, "inf")


def test_counter_counts_the_scaled_layers_and_accumulates_over_launches():
    cases = [(4, 7, 9, "above"), (1, 5, 3, "below"), (17, 40, 24, "above"), (4, 7, 9, "on"), (16, 64, 64, "above")]
    slab = Slab(case_layers(cases))
    counters = torch.zeros(1, dtype=torch.int32, device=DEV)
    _, stats = slab.run(mc.BOUND, counters=counters)
    assert int((stats[:, 1] != 1.0).sum()) == 3 and int(counters.cpu()[0]) == 3
    _, stats = slab.run(mc.BOUND, counters=counters)  # a fresh copy of the same inputs: three more
    assert int(counters.cpu()[0]) == 6
    dev, _ = slab.run(mc.BOUND)  # no counter: the launch works without one
    assert not mc.same_bits(dev.cpu(), slab.buf)


# -- 4. grid edge and determinism ------------------------------------------------------------------------------------------------
def grid_edge_slab():
    """300 layers of (4, 8, 8) — more layers than compute units — every third one far above the bound of the rest."""
    raw = []
    for l in range(300):
        up = mc.hashed(32, 31 * l + 1).view(8, 4) * 2.0 ** -4
        down = mc.hashed(32, 31 * l + 2).view(4, 8) * 2.0 ** -3
        up[0, 0] = up[0, 0] + 1.0  # (no layer is all zero)
        down[0, 0] = down[0, 0] + 1.0
        raw.append((up, down, 1.0))
    bound = 2.0 * max(mc.product_norm(*x) for x in raw)
    layers = []
    for l, (up, down, scale) in enumerate(raw):
        if l % 3 == 0:
            up = up * 2.0 ** math.ceil(math.log2(4 * bound / mc.product_norm(up, down, scale)))
        layers.append((up, down, scale))
    return Slab(layers), bound


def test_three_hundred_layers_every_third_above_the_bound():
    slab, bound = grid_edge_slab()
    counters = torch.zeros(1, dtype=torch.int32, device=DEV)
    dev, stats = slab.run(bound, counters=counters)
    scaled = check_layers(slab, slab.buf, dev.cpu(), stats, bound, "300")
    assert scaled == 100 and int(counters.cpu()[0]) == 100
    assert [bool(f != 1.0) for f in stats[:, 1]] == [l % 3 == 0 for l in range(300)]
    check_accuracy(slab, stats, bound, "300")


def test_two_launches_from_equal_inputs_give_equal_bits(table_run):
    slab, after, stats, _, _, _ = table_run
    dev, stats2 = slab.run(mc.BOUND)
    assert mc.same_bits(dev.cpu(), after) and mc.same_bits(stats2, stats)


# -- 5. the public helpers -------------------------------------------------------------------------------------------------------
def warmed_unet(dtype=torch.float32, rank=4):
    unet = build_tiny_unet(seed=5).to(DEV).to(dtype)
    dfa.inject_trainable_lora(unet, r=rank)
    layers = [m for m in unet.modules() if isinstance(m, dfa.LoraInjectedLinear)]
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for i, l in enumerate(layers):
            l.lora_up.weight.copy_((torch.randn(l.lora_up.weight.shape, generator=g) * 0.02 * (1 + i % 5)).to(DEV))
        layers[1].scale = 0.5  # the table takes each layer's own scale
    return unet, layers


def host_factors(layers):
    return [(l.lora_up.weight.detach().float().cpu().clone(), l.lora_down.weight.detach().float().cpu().clone(), l.scale)
            for l in layers]


def test_helpers_on_the_tiny_unet_equal_the_restatement():
    unet, layers = warmed_unet()
    before = host_factors(layers)
    norms = dfa.lora_weight_norms(unet).cpu()
    assert norms.shape == (len(layers),) and all(mc.same_bits(a[0], b[0]) and mc.same_bits(a[1], b[1])
                                                 for a, b in zip(host_factors(layers), before))
    refs = [mc.product_norm(*x) for x in before]
    for l, x in enumerate(before):
        assert abs(float(norms[l]) ** 2 - refs[l] ** 2) <= mc.norm_squared_bound(*x), (l, float(norms[l]), refs[l])
    m = float(torch.tensor(sorted(refs)[len(refs) // 2] * 1.0001, dtype=torch.float32))  # about half the layers are above
    got_norms, factors = (t.cpu() for t in dfa.clamp_lora_norms_(unet, m))
    assert mc.same_bits(got_norms, norms)
    after = host_factors(layers)
    n_scaled = 0
    for l, (x, y) in enumerate(zip(before, after)):
        f = float(factors[l])
        if refs[l] > m * (1 + 1e-5):
            f_ref = math.sqrt(m / refs[l])
            assert abs(f - f_ref) / f_ref <= mc.norm_squared_bound(*x) / (2 * refs[l] ** 2) + U, (l, f, f_ref)
        if f == 1.0:
            assert mc.same_bits(y[0], x[0]) and mc.same_bits(y[1], x[1]), l
        else:
            n_scaled += 1
            ft = torch.tensor(f, dtype=torch.float32)
            assert mc.same_bits(y[0], x[0] * ft) and mc.same_bits(y[1], x[1] * ft), l
    assert 0 < n_scaled < len(layers)
    again = dfa.lora_weight_norms(unet).cpu()
    for l, y in enumerate(after):
        assert float(again[l]) ** 2 <= (m * (1 + 4 * U)) ** 2 + mc.norm_squared_bound(*y), (l, float(again[l]), m)


def test_helpers_on_half_precision_factors_measure_an_fp32_copy_and_round_a_scaled_layer_back():
    unet, layers = warmed_unet(torch.float16)
    before = host_factors(layers)
    norms = dfa.lora_weight_norms(unet).cpu()
    refs = [mc.product_norm(*x) for x in before]
    for l, x in enumerate(before):  # fp16 values are fp32 values: the same bound
        assert abs(float(norms[l]) ** 2 - refs[l] ** 2) <= mc.norm_squared_bound(*x), (l, float(norms[l]), refs[l])
    m = float(torch.tensor(sorted(refs)[len(refs) // 2] * 1.0001, dtype=torch.float32))
    _, factors = dfa.clamp_lora_norms_(unet, m)
    assert layers[0].lora_up.weight.dtype == torch.float16 and 0 < int((factors != 1.0).sum()) < len(layers)
    # every element of both factors is rounded to fp16 once (2⁻¹¹ relative each): the product moves by at most 2·2⁻¹¹ + O(2⁻²²)
    after = [mc.product_norm(*x) for x in host_factors(layers)]
    for l, n in enumerate(after):
        assert (n <= m * (1 + 4 * 2.0 ** -11)) if float(factors[l]) != 1.0 else (n == refs[l]), (l, n, m)


def test_a_host_model_raises_as_the_slab_does():
    unet = build_tiny_unet(seed=5)
    dfa.inject_trainable_lora(unet, r=4)
    with pytest.raises(RuntimeError, match="HIP device"):
        dfa.lora_weight_norms(unet)
    with pytest.raises(RuntimeError, match="HIP device"):
        dfa.clamp_lora_norms_(unet, 1.0)
