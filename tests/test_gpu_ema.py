"""`lora_adamw_ema_step` and `lora_slab_swap` (csrc/optim.hip) on an MI355X, kernel level through `_native`.

Sizes, inputs and the fp32 emulation are tests/ema_cases.py's; tests/test_ema_host.py shows on the CPU that the emulation's bits
differ from a contracted (fma) update and from four planted bugs.  Every comparison here is bit for bit:
  p, m, v  against `lora_adamw_step` on the same inputs and the same norm — the fused launch must not change AdamW;
  shadow   against s − omd·(s − p) in CPU fp32 on the p the GPU produced, omd from `step.ema_one_minus_decay_at`.
Every written buffer is a view between sentinel bands (`Banded` of tests/test_gpu_gemm_edges.py); the gradient and the norm
are compared with copies afterwards."""
import pytest
import torch

from diffusion_finetuning_amd import _native as nat
from tests import ema_cases as ec
from tests import optim_cases as oc
from tests.test_gpu_gemm_edges import Banded, off_by_one_element

pytestmark = pytest.mark.gpu
DEV = "cuda"


def held(t):
    """`t`'s values in a device view between sentinel bands."""
    b = Banded(t.numel(), 1, t.dtype)
    b.view.copy_(t.reshape(-1, 1).to(DEV))
    return b


def flat(b, what):
    return b.check(what).reshape(-1)


def step_args(max_norm=1.0, step=0):
    cfg = ec.CFG
    return (cfg["mul"], max_norm, cfg["lr"], oc.BETA1, oc.BETA2, oc.EPS, cfg["wd"], step)


def counted_norm(g_dev, t):
    """The 4-float norm after the norm launch of applied step t (the counter is planted at t − 1 first)."""
    N = held(torch.tensor([0.0, 0.0, float(t - 1), 0.0]))
    nat.lora_grad_sqnorm(g_dev, ec.CFG["mul"], N.view.reshape(-1))
    out = flat(N, "norm")
    assert out[1:].tolist() == [0.0, float(t), 0.0], out
    return N


def run_pair(n, t, max_decay, update_after, off_by_one=False, step=0):
    """One `lora_adamw_step` and one `lora_adamw_ema_step` from identical state, every operand of the second between sentinel
    bands — or, `off_by_one`, at an address one element past a 16-byte boundary.  Returns what the assertions need."""
    p, g, m, v, s = ec.ema_inputs(n)
    g_dev = g.to(DEV)
    N = counted_norm(g_dev, t)  # (the norm launch reads a 16-byte-aligned gradient)
    G = off_by_one_element(g_dev) if off_by_one else g_dev
    g_copy = G.clone()
    norm = N.view.reshape(-1)
    norm_copy = norm.clone()
    ref = [x.to(DEV).clone() for x in (p, m, v)]
    nat.lora_adamw_step(ref[0], G, ref[1], ref[2], norm, *step_args(step=step))
    if off_by_one:
        bands = None
        views = [off_by_one_element(x.to(DEV)) for x in (p, m, v, s)]
        assert all(x.data_ptr() % 16 == 4 for x in views + [G])
    else:
        bands = [held(x) for x in (p, m, v, s)]
        views = [b.view.reshape(-1) for b in bands]
    nat.lora_adamw_ema_step(views[0], G, views[1], views[2], views[3], norm, *step_args(step=step), max_decay, update_after)
    torch.cuda.synchronize()
    what = (n, t, max_decay, update_after, "off by one" if off_by_one else "aligned")
    if bands is not None:
        for b, name in zip(bands, "pmvs"):
            b.check((what, name))
    for got, want, name in zip(views[:3], ref, "pmv"):
        assert ec.same_bits(got, want), (what, name, "differs from lora_adamw_step",
                                         int((ec.bits(got) != ec.bits(want)).sum()))
    assert ec.same_bits(G, g_copy), (what, "g changed")
    assert ec.same_bits(flat(N, "norm"), norm_copy), (what, "the step wrote the norm")
    return p, s, views[0].cpu(), views[3].cpu(), what


@pytest.mark.parametrize("n", ec.EMA_SIZES)
def test_every_size_adamw_bits_unchanged_and_shadow_is_the_emulation(n):
    md, ua = ec.MAX_DECAY, 0
    for t in (3, 11):  # two ramp steps: omd = 0.75 (two mantissa bits) and 9/20 (a full mantissa)
        p_old, s, p_new, s_new, what = run_pair(n, t, md, ua)
        want = ec.ema_emulate(s, p_new, ec.omd_at(t, md, ua))
        differ = int((ec.bits(s_new) != ec.bits(want)).sum())
        assert differ == 0, (what, "shadow differs from the emulation in", differ, "of", n)
        if n >= 255:  # the step moved things: neither the old shadow nor a copy of p
            assert not ec.same_bits(s_new, s) and not ec.same_bits(s_new, p_new) and not ec.same_bits(p_new, p_old)
            assert not ec.same_bits(s_new, ec.ema_emulate_fma(s, p_new, ec.omd_at(t, md, ua))), (what, "a contracted update")


@pytest.mark.parametrize("n", ec.OFF_BY_ONE_SIZES)
def test_views_that_are_only_four_byte_aligned(n):
    t, md, ua = 11, ec.MAX_DECAY, 0
    _, s, p_new, s_new, what = run_pair(n, t, md, ua, off_by_one=True)
    want = ec.ema_emulate(s, p_new, ec.omd_at(t, md, ua))
    assert ec.same_bits(s_new, want), (what, int((ec.bits(s_new) != ec.bits(want)).sum()))


@pytest.mark.parametrize("t,md,ua", ec.COUNTER_CASES)
def test_decay_follows_the_device_counter(t, md, ua):
    """omd is the host statement's, seen through the shadow's bits — also when the bias corrections come from a host step."""
    n = 4099
    for step in (0, t):
        p_old, s, p_new, s_new, what = run_pair(n, t, md, ua, step=step)
        omd = ec.omd_at(t, md, ua)
        want = ec.ema_emulate(s, p_new, omd)
        differ = int((ec.bits(s_new) != ec.bits(want)).sum())
        print("t=%d max_decay=%g update_after=%d: omd %.9g, %d of %d shadow elements off" % (t, md, ua, float(omd), differ, n))
        assert differ == 0, (what, step, differ)
        for wrong_t in (t - 1, t + 1):  # the neighbours' decay would show, wherever it is another number
            other = ec.omd_at(wrong_t, md, ua)
            if float(other) != float(omd):
                assert not ec.same_bits(s_new, ec.ema_emulate(s, p_new, other)), (what, wrong_t)


@pytest.mark.parametrize("n", [257, ec.EMA_SIZES[-1]])
def test_a_flagged_step_writes_nothing(n):
    p, g, m, v, s = ec.ema_inputs(n)
    g[n // 2] = float("inf")
    G = g.to(DEV)
    N = held(torch.tensor([0.0, 0.0, 4.0, 0.0]))
    norm = N.view.reshape(-1)
    nat.lora_grad_sqnorm(G, 1.0, norm)
    assert norm[1:].tolist() == [1.0, 4.0, 1.0]
    bands = [held(x) for x in (p, m, v, s)]
    views = [b.view.reshape(-1) for b in bands]
    for step in (0, 5):
        nat.lora_adamw_ema_step(views[0], G, views[1], views[2], views[3], norm, *step_args(step=step), ec.MAX_DECAY, 0)
        for b, x, name in zip(bands, (p, m, v, s), "pmvs"):
            assert ec.same_bits(flat(b, (n, name)), x), (n, step, name, "moved by a skipped step")


@pytest.mark.parametrize("n", ec.EMA_SIZES)
def test_swap_exchanges_the_bits_and_twice_is_the_identity(n):
    gen = torch.Generator().manual_seed(6000 + n)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    a[0], b[-1] = float("nan"), float("-inf")  # bits, not values: a payload travels as it is
    a_bits = ec.bits(a).clone()
    layouts = [("aligned", None)]
    if n in ec.OFF_BY_ONE_SIZES:
        layouts += [("a off by one", 0), ("b off by one", 1), ("both off by one", 2)]
    for name, which in layouts:
        if which is None:
            A, B = held(a), held(b)
            va, vb = A.view.reshape(-1), B.view.reshape(-1)
        else:
            va = off_by_one_element(a.to(DEV)) if which in (0, 2) else a.to(DEV)
            vb = off_by_one_element(b.to(DEV)) if which in (1, 2) else b.to(DEV)
        nat.lora_slab_swap(va, vb)
        assert torch.equal(ec.bits(va), ec.bits(b)) and torch.equal(ec.bits(vb), a_bits), (n, name, "once")
        nat.lora_slab_swap(va, vb)
        assert torch.equal(ec.bits(va), a_bits) and torch.equal(ec.bits(vb), ec.bits(b)), (n, name, "twice")
        if which is None:
            for band in (A, B):  # (Banded.check minus its NaN test: a NaN is part of the payload)
                raw = band.buf.view(band.ints)
                for part in (raw[:band.pad], raw[band.pad + band.n:]):
                    assert torch.equal(part, torch.full_like(part, band.sentinel)), (n, "store into a band")


def test_swap_refuses_one_buffer_and_overlapping_ranges_without_a_launch():
    buf = torch.arange(64, dtype=torch.float32, device=DEV)
    keep = buf.clone()
    torch.cuda.synchronize()
    for a, b in ((buf[:32], buf[:32]), (buf[:32], buf[31:63]), (buf[31:63], buf[:32]), (buf[:32], buf[1:33])):
        with pytest.raises(RuntimeError, match="lora_slab_swap"):
            nat.lora_slab_swap(a, b)
    with pytest.raises(ValueError):
        nat.lora_slab_swap(buf[:32], buf[32:63])  # (two lengths)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)
    nat.lora_slab_swap(buf[:32], buf[32:])  # ranges that touch are two buffers
    assert torch.equal(buf[:32], keep[32:]) and torch.equal(buf[32:], keep[:32])
