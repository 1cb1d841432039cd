"""CPU-only guards for the EMA tests (tests/test_gpu_ema.py, tests/test_gpu_ema_trainer.py):

1. `step.ema_decay_at` — the one host statement of the decay `lora_adamw_ema_step` computes on the device — against values
   worked out by hand, the first step at which the cap 0.9999 binds among them;
2. on the inputs the GPU tests use, the fp32 emulation s − omd·(s − p) differs in its BITS from a fused-multiply-add
   evaluation and from four planted bugs, so a bit comparison with it tells them apart;
3. the two new entry points return the header's argument-error status before any launch (fake pointers: nothing here
   reaches a device), the kernel's text states the update through `ema_element`, and the trainer refuses bad arguments."""
import ctypes
import os

import pytest
import torch

from diffusion_finetuning_amd import _native as nat
from diffusion_finetuning_amd import step as stp
from tests import ema_cases as ec
from tests import optim_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusion_finetuning_amd", "csrc")


def test_decay_against_hand_values():
    c = oc.f32(0.9999)
    assert c != 0.9999 and abs(c - 0.9999) < 1e-7                      # max_decay is the fp32 the kernel receives
    assert stp.ema_decay_at(1, 0.9999, 0) == 0.0                       # first counted step: n = 0
    assert stp.ema_decay_at(2, 0.9999, 0) == 2.0 / 11.0                # n = 1
    assert stp.ema_decay_at(3, 0.9999, 0) == 3.0 / 12.0
    for t in range(0, 7):
        assert stp.ema_decay_at(t, 0.9999, 5) == 0.0, t                # update_after = 5: t <= 6 → n <= 0
    assert stp.ema_decay_at(7, 0.9999, 5) == 2.0 / 11.0
    # the cap: (1 + n)/(10 + n) > c  ⇔  n > (10c − 1)/(1 − c) = 89975.07…: n = 89976 is the first, t = n + 1
    bound = (10 * c - 1) / (1 - c)
    assert 89975 < bound < 89976 and ec.FIRST_CAPPED_T == 89977
    assert stp.ema_decay_at(89976, 0.9999, 0) == 89976.0 / 89985.0 < c  # n = 89975: still on the ramp
    assert stp.ema_decay_at(89977, 0.9999, 0) == c                     # capped
    assert 89977.0 / 89986.0 > c
    assert stp.ema_decay_at(200000, 0.9999, 0) == c                    # and beyond
    assert stp.ema_decay_at(89977 + 5, 0.9999, 5) == c                 # the cap moves with update_after
    assert stp.ema_decay_at(10, 0.5, 0) == 0.5 and 10.0 / 19.0 > 0.5   # a small cap binds early (the GPU cases)
    assert stp.ema_decay_at(9, 0.5, 0) == 0.5 == 9.0 / 18.0


def test_one_minus_decay_is_rounded_to_fp32_once():
    for t, md, ua in ec.COUNTER_CASES:
        d = stp.ema_decay_at(t, md, ua)
        omd = stp.ema_one_minus_decay_at(t, md, ua)
        assert omd == oc.f32(1.0 - d) and float(ec.omd_at(t, md, ua)) == omd, (t, md, ua)
    assert stp.ema_one_minus_decay_at(1, 0.9999, 0) == 1.0
    assert stp.ema_one_minus_decay_at(200000, 0.9999, 0) == oc.f32(1.0 - oc.f32(0.9999))
    # 1 − fp32(0.9999) in double, then to fp32 — not fp32(1) − fp32(0.9999) in fp32, and not fp32(1 − 0.9999)
    assert stp.ema_one_minus_decay_at(200000, 0.9999, 0) != oc.f32(1.0 - 0.9999)


def test_counter_cases_cover_what_the_issue_names():
    cases = set(ec.COUNTER_CASES)
    assert {(t, ec.MAX_DECAY, 0) for t in (1, 2, 3, 10, 11)} <= cases
    assert (5, ec.MAX_DECAY, 5) in cases and (6, ec.MAX_DECAY, 5) in cases       # update_after and update_after + 1
    assert any(stp.ema_decay_at(t, md, ua) == oc.f32(md) for t, md, ua in cases)  # a capped t
    assert any(t >= ec.FIRST_CAPPED_T and md == ec.MAX_DECAY for t, md, ua in cases)
    assert {1, 3, 5, 257 * 1024, 1024 * 1024 + 1024 + 3} <= set(ec.EMA_SIZES)
    assert {n for sizes in oc.ADAMW_SIZES.values() for n in sizes} <= set(ec.EMA_SIZES)
    assert set(ec.OFF_BY_ONE_SIZES) <= set(ec.EMA_SIZES) and any(n % 4 for n in ec.OFF_BY_ONE_SIZES)


def _stepped(n):
    """(p_old, p_new, s): the chosen inputs and the parameters after one AdamW step in fp32 (optim_cases.adamw_f32)."""
    p, g, m, v, s = ec.ema_inputs(n)
    norm_sq = oc.sqnorm_f32(g, ec.CFG["mul"])
    p_new = oc.adamw_f32(p, g, m, v, ec.CFG, 1.0, 3, norm_sq=norm_sq)[0]
    return p, p_new, s


@pytest.mark.parametrize("n", [255, 4099])
def test_the_emulation_differs_from_a_fused_multiply_add(n):
    _, p_new, s = _stepped(n)
    for t, md, ua in ((2, ec.MAX_DECAY, 0), (3, ec.MAX_DECAY, 0), (11, ec.MAX_DECAY, 0), (7, ec.MAX_DECAY, 5)):  # ramp steps
        omd = ec.omd_at(t, md, ua)
        a, b = ec.ema_emulate(s, p_new, omd), ec.ema_emulate_fma(s, p_new, omd)
        differ = int((ec.bits(a) != ec.bits(b)).sum())
        print("n=%d t=%d: op-by-op and fma evaluations differ in %d of %d elements" % (n, t, differ, n))
        assert differ >= n // 20, (n, t, differ)
        assert float((a - b).abs().max()) <= 2.0 ** -22 * float(s.abs().max())  # (and by rounding only)
    # omd = 1 (d = 0): the product is exact, the two evaluations agree — and neither is a plain copy of p for every element
    one = ec.omd_at(1)
    assert ec.same_bits(ec.ema_emulate(s, p_new, one), ec.ema_emulate_fma(s, p_new, one))


@pytest.mark.parametrize("mutant", ec.EMA_MUTANTS)
def test_the_emulation_rejects_planted_bugs(mutant):
    n = 4099
    p_old, p_new, s = _stepped(n)
    assert int((ec.bits(p_old) != ec.bits(p_new)).sum()) > n // 2  # the step moves the parameters
    # where each bug shows: any ramp step; a flagged step; any step; a capped step
    t, flagged = {"decay from t - 1": (3, False), "update on a flagged step": (3, True),
                  "p_old instead of p_new": (3, False), "cap ignored": (200000, False)}[mutant]
    good = ec.ema_step_emulate(s, p_old, p_new, t, flagged)
    bad = ec.ema_step_emulate(s, p_old, p_new, t, flagged, mutant=mutant)
    differ = int((ec.bits(good) != ec.bits(bad)).sum())
    assert differ > n // 2, (mutant, differ)
    if flagged:
        assert ec.same_bits(good, s)


def test_entry_points_reject_bad_arguments_before_any_launch():
    lib = nat.lib()
    P = ctypes.c_void_p
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    at = lambda i: P(a + 4 * i)  # noqa: E731
    hyper = (1.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-2)
    good = [at(0), at(8), at(16), at(24), at(32), 8, at(40)]
    for i in (0, 1, 2, 3, 4, 6):   # every pointer, the norm included: the average always follows the device counter
        args = list(good)
        args[i] = None
        assert lib.lora_adamw_ema_step(*args, *hyper, 0, 0.9999, 0, None) == -1, i
    bad_n = list(good)
    bad_n[5] = 0
    assert lib.lora_adamw_ema_step(*bad_n, *hyper, 0, 0.9999, 0, None) == -1
    assert lib.lora_adamw_ema_step(*good, *hyper, -1, 0.9999, 0, None) == -1
    assert lib.lora_adamw_ema_step(*good, *hyper, 0, 1.5, 0, None) == -1
    assert lib.lora_adamw_ema_step(*good, *hyper, 0, -0.1, 0, None) == -1
    assert lib.lora_adamw_ema_step(*good, *hyper, 0, float("nan"), 0, None) == -1
    assert lib.lora_adamw_ema_step(*good, *hyper, 0, 0.9999, -1, None) == -1
    # swap: null, n < 1, the same buffer, ranges that overlap from either side; touching ranges are two buffers
    assert lib.lora_slab_swap(None, at(0), 8, None) == -1 and lib.lora_slab_swap(at(0), None, 8, None) == -1
    assert lib.lora_slab_swap(at(0), at(32), 0, None) == -1
    assert lib.lora_slab_swap(at(0), at(0), 8, None) == -1
    assert lib.lora_slab_swap(at(0), at(7), 8, None) == -1 and lib.lora_slab_swap(at(7), at(0), 8, None) == -1
    assert lib.lora_slab_swap(at(0), at(1), 8, None) == -1


def test_the_kernel_states_the_update_through_ema_element():
    with open(os.path.join(CSRC, "common.h")) as f:
        common = f.read()
    assert "s = s - rounded_f32(omd * (s - p));" in common
    with open(os.path.join(CSRC, "optim.hip")) as f:
        src = f.read()
    i = src.index("void adamw_ema_kernel(")
    k = src[i:src.index("\n}\n", i)]
    for line in ("if (a.norm_in[1] != 0.f) return;", "adamw_element(p, m, v, g, decay, step_size, a.beta1, a.beta2, bc2_sqrt, a.eps);",
                 "ema_element(s, p, omd);", "const double n_ema = t - (double)ema_update_after - 1.0;",
                 "d = (1.0 + n_ema) / (10.0 + n_ema);", "const float omd = (float)(1.0 - d);",
                 "for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256)"):
        assert line in k, line
    assert k.index("adamw_element(") < k.index("ema_element(") < k.index("a.p[i] = p;")
    assert k.index("if (a.norm_in[1] != 0.f) return;") < k.index("for (")


def test_trainer_argument_rules():
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan"), 1.0 - 1e-12):  # (the last one rounds to 1 in fp32)
        with pytest.raises(ValueError, match="ema_decay"):
            stp.check_ema(bad, 0)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="ema_update_after_step"):
            stp.check_ema(0.999, bad)
    stp.check_ema(None, 0)
    stp.check_ema(0.9999, 10)
