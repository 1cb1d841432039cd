"""Sizes, inputs and the fp32 emulation for the EMA of the LoRA weights: `lora_adamw_ema_step`, `lora_slab_swap`
(csrc/optim.hip) and `LoraTrainer(ema_decay=...)`.  Plain data and CPU torch; tests/test_ema_host.py shows what the emulation
tells apart, tests/test_gpu_ema.py and tests/test_gpu_ema_trainer.py run it.

The shadow update is three IEEE single operations,  s − omd·(s − p):  a difference, a product, a difference, each rounded to
fp32 — what three torch ops on fp32 CPU tensors give, bit for bit on any host.  A kernel that contracts the product and the
last difference into one fma rounds once less and differs in a large share of the elements (`ema_emulate_fma`), so the GPU
tests compare BITS and need no tolerance.  omd is `step.ema_one_minus_decay_at`: the one host statement of the decay."""
import torch

from diffusion_finetuning_amd import step as stp
from tests import optim_cases as oc

# every class of the AdamW launch (the EMA kernel keeps its grid), plus: below one float4 (1, 3), one past it (5), a grid of
# more than one round of blocks at an odd count (257 blocks' worth), and over the 2048-block cap with a ragged end
EMA_SIZES = tuple(sorted({n for sizes in oc.ADAMW_SIZES.values() for n in sizes} | {1, 3, 5, 257 * 1024, 1024 * 1024 + 1024 + 3}))
OFF_BY_ONE_SIZES = (5, 257, 1024 * 1024 + 1024 + 3)   # also run through a view that is only 4-byte aligned

MAX_DECAY = 0.9999
# (t, max_decay, update_after): the device counter after the norm launch.  d = 0 at t <= update_after + 1; the ramp; the cap
COUNTER_CASES = (
    (1, MAX_DECAY, 0), (2, MAX_DECAY, 0), (3, MAX_DECAY, 0), (10, MAX_DECAY, 0), (11, MAX_DECAY, 0),
    (5, MAX_DECAY, 5), (6, MAX_DECAY, 5), (7, MAX_DECAY, 5),     # t = update_after, update_after + 1 (both d = 0), + 2 (2/11)
    (10, 0.5, 0), (11, 0.5, 0),                                  # (1 + n)/(10 + n) = 10/19, 11/20 > 0.5: capped
    (200000, MAX_DECAY, 0),                                      # far past the first capped t of 0.9999 (89977)
)
FIRST_CAPPED_T = 89977  # smallest t with (1 + n)/(10 + n) > fp32(0.9999), n = t − 1: n > (10c − 1)/(1 − c) = 89975.07…

CFG = oc.ADAMW_CONFIGS[4]  # lr 0.1, wd 0.1, mul 1/1024, max_norm 1: the parameters move by far more than an ulp


def omd_at(t, max_decay=MAX_DECAY, update_after=0):
    """fp32 scalar tensor 1 − d of applied step t."""
    return torch.tensor(stp.ema_one_minus_decay_at(t, max_decay, update_after), dtype=torch.float32)


def ema_inputs(n, seed=0):
    """(p, g, m, v, s) fp32 [n]: optim_cases.adamw_inputs and a shadow of the parameters' size on the other side of zero —
    omd·(s − p) is then larger than s on the ramp steps, so how the product is rounded decides the last bit of the result
    in a large share of the elements (a shadow close to p would hide a contracted product behind the final rounding)."""
    p, g, m, v = oc.adamw_inputs(n, seed)
    gen = torch.Generator().manual_seed(5000 + seed + n)
    s = -0.7 * p * (1.0 + 0.3 * torch.randn(n, generator=gen)) + 1e-3 * torch.randn(n, generator=gen)
    return p, g, m, v, s.float()


def ema_emulate(s, p_new, omd):
    """s − omd·(s − p_new), op by op in fp32."""
    s, p_new = s.detach().float().cpu(), p_new.detach().float().cpu()
    return s - omd * (s - p_new)


def ema_emulate_fma(s, p_new, omd):
    """The same with the product and the last difference fused: fma(−omd, s − p_new, s).  The product of two fp32 values is
    exact in float64; the sum is rounded to float64 and then to fp32."""
    s, p_new = s.detach().float().cpu(), p_new.detach().float().cpu()
    return (s.double() - omd.double() * (s - p_new).double()).float()


EMA_MUTANTS = ("decay from t - 1", "update on a flagged step", "p_old instead of p_new", "cap ignored")


def ema_step_emulate(s, p_old, p_new, t, flagged, max_decay=MAX_DECAY, update_after=0, mutant=None):
    """The shadow after one `lora_adamw_ema_step` whose norm holds the applied count t (this step included) and the overflow
    flag `flagged`; p_old / p_new are the parameters before and after the AdamW update."""
    if flagged and mutant != "update on a flagged step":
        return s.detach().float().cpu().clone()
    if mutant == "decay from t - 1":
        t = t - 1
    omd = omd_at(t, 1.0 if mutant == "cap ignored" else max_decay, update_after)
    return ema_emulate(s, p_old if mutant == "p_old instead of p_new" else p_new, omd)


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))
