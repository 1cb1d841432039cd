"""CPU side of the multistep sampler tests: PLMS (PNDM with skip_prk_steps, Liu et al. 2022, as SD's pipeline runs it) and
DPM-Solver++(2M) (Lu et al. 2022, Algorithm 2, midpoint form), float64 and STATEFUL — explicit lists of earlier model outputs /
data predictions and the saved sample, a counter, one `step(x, o)` per model evaluation — as the schedulers are written, not
collapsed into coefficient tables.  diffusers is not part of the reference tree: both are restated from the published
definitions.  The product collapses every iteration to x' = a·base + c0·(p·x + q·o) + Σ c_k·H[s_k]
(sampling.multistep_schedule); nothing here shares code with it.  ᾱ, the grid, guidance and the Philox x_T are
tests/sampling_reference.py's."""
import torch

from tests import sampling_reference as sr

PUSH, SAVE, USE_SAVED = 1, 2, 4  # the plan's flag bits, as include/lora_hip.h documents them


class Plms:
    """`ets`: the model outputs kept, oldest first (at most four); `cur_sample`: the sample saved by the first call for the
    second, which repeats the first transfer with the averaged output.  `counter` counts model evaluations."""

    def __init__(self, S, v_prediction, T=1000):
        self.S, self.v, self.ratio, self.acp = S, v_prediction, T // S, sr.alphas_cumprod(T)
        grid = sr.timesteps("ddim", S, T)  # descending, steps_offset where the table has room
        self.timesteps = grid[:1] + grid[1:2] + grid[1:]  # the second one twice (S = 1: the only one once)
        self.ets, self.cur_sample, self.counter = [], None, 0

    def _acp(self, t):
        return self.acp[t] if t >= 0 else self.acp[0]  # set_alpha_to_one = False

    def transfer(self, x, e, t, t_prev):
        ab_t, ab_p = self._acp(t), self._acp(t_prev)
        if self.v:  # converted AFTER the combination, with the sample the transfer starts from
            e = ab_t.sqrt() * e + (1 - ab_t).sqrt() * x
        sample_coeff = (ab_p / ab_t).sqrt()
        denom = ab_t * (1 - ab_p).sqrt() + (ab_t * (1 - ab_t) * ab_p).sqrt()
        return sample_coeff * x - (ab_p - ab_t) * e / denom

    def step(self, x, o):
        x, o = x.double(), o.double()
        t = self.timesteps[self.counter]
        t_prev = t - self.ratio
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(o)
        else:  # the corrected first step: from the first timestep again
            t_prev = t
            t = t + self.ratio
        if len(self.ets) == 1 and self.counter == 0:
            e = o
            self.cur_sample = x
        elif len(self.ets) == 1 and self.counter == 1:
            e = (o + self.ets[-1]) / 2
            x = self.cur_sample
            self.cur_sample = None
        elif len(self.ets) == 2:
            e = (3 * self.ets[-1] - self.ets[-2]) / 2
        elif len(self.ets) == 3:
            e = (23 * self.ets[-1] - 16 * self.ets[-2] + 5 * self.ets[-3]) / 12
        else:
            e = (55 * self.ets[-1] - 59 * self.ets[-2] + 37 * self.ets[-3] - 9 * self.ets[-4]) / 24
        self.counter += 1
        return self.transfer(x, e, t, t_prev)

    @property
    def history(self):
        return self.ets

    def resume(self, counter, history, saved=None):
        """Put the solver before model evaluation `counter` with the given kept outputs (oldest first) and saved sample."""
        self.counter, self.ets, self.cur_sample = counter, [h.double() for h in history], saved

    @staticmethod
    def pushes_before(i):
        """How many outputs have been kept before model evaluation i (the second evaluation's is not kept)."""
        return 0 if i == 0 else max(1, i - 1)


class Dpmpp2M:
    """`x0s`: the data predictions so far, oldest first; `counter` counts steps."""

    def __init__(self, S, v_prediction, T=1000):
        self.S, self.v, self.ratio, self.acp = S, v_prediction, T // S, sr.alphas_cumprod(T)
        self.timesteps = sr.timesteps("ddim", S, T)
        self.x0s, self.counter = [], 0

    def _asl(self, t):
        ab = self.acp[t] if t >= 0 else self.acp[0]
        alpha, sigma = ab.sqrt(), (1 - ab).sqrt()
        return alpha, sigma, torch.log(alpha / sigma)

    def step(self, x, o):
        x, o = x.double(), o.double()
        s = self.timesteps[self.counter]
        a_s, s_s, l_s = self._asl(s)
        a_t, s_t, l_t = self._asl(s - self.ratio)
        x0 = a_s * x - s_s * o if self.v else (x - s_s * o) / a_s
        self.x0s = self.x0s[-1:]
        self.x0s.append(x0)
        h = l_t - l_s
        first_order = self.counter == 0 or (self.counter == self.S - 1 and self.S < 15)  # lower-order final
        if first_order:
            d = self.x0s[-1]
        else:
            h_prev = l_s - self._asl(self.timesteps[self.counter - 1])[2]
            r = h_prev / h
            d = (1 + 1 / (2 * r)) * self.x0s[-1] - (1 / (2 * r)) * self.x0s[-2]
        self.counter += 1
        return (s_t / s_s) * x - a_t * (torch.exp(-h) - 1) * d

    @property
    def history(self):
        return self.x0s

    def resume(self, counter, history, saved=None):
        self.counter, self.x0s = counter, [h.double() for h in history]

    @staticmethod
    def pushes_before(i):
        return i


SOLVERS = {"plms": Plms, "dpmpp_2m": Dpmpp2M}


def evaluations(method, S):
    return S + 1 if method == "plms" and S >= 2 else S


def ring_slots(plan, i):
    """Which slot holds the k-th last push (k = 1, 2, 3) BEFORE iteration i, by replaying the pushes of plan[:i] — None where
    there is no such push or a later push has taken its slot."""
    pushes = [int(row[0]) for row in plan[:i].tolist() if row[4] & PUSH]
    slots = []
    for k in (1, 2, 3):
        if k > len(pushes):
            slots.append(None)
            continue
        slot = pushes[-k]
        slots.append(None if slot in pushes[len(pushes) - k + 1:] else slot)
    return slots


def apply_tables(coef_row, plan_row, x, o, xs, ring):
    """The contract of ddpm_sample_multistep in float64: (x', h, Σ|terms|) from the state x, the guided output o, the saved
    state and the ring (a mapping slot → tensor).  A coefficient of exactly 0 reads nothing; a slot that was never pushed is a
    KeyError."""
    p, q, a, c0, c1, c2, c3 = (float(c) for c in coef_row)
    _, s1, s2, s3, flags = (int(v) for v in plan_row)
    h = p * x + q * o
    acc, terms = torch.zeros_like(x), torch.zeros_like(x)
    if a != 0.0:
        base = xs if flags & USE_SAVED else x
        acc, terms = acc + a * base, terms + (a * base).abs()
    if c0 != 0.0:
        acc, terms = acc + c0 * h, terms + (c0 * p * x).abs() + (c0 * q * o).abs()
    for c, s in ((c1, s1), (c2, s2), (c3, s3)):
        if c != 0.0:
            acc, terms = acc + c * ring[s], terms + (c * ring[s]).abs()
    return acc, h, terms
