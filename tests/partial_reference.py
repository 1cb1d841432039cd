"""CPU side of the image-to-image sampler tests, float64: the strength → (n, k0) mapping, the noised start state, the keep-mask
blend and its (k, n) pairs, and the stateful PLMS / DPM-Solver++(2M) of tests/multistep_reference.py started FRESH on the
sub-grid grid[k0:] — empty history, warm-up there, the lower-order-final rule keyed on the full step count.  diffusers' img2img /
inpaint pipelines are not part of the reference tree: restated from their published behaviour.  Nothing here shares code with
the product (sampling.partial_start / keep_schedule / multistep_schedule(first_step=...)); ᾱ, the grids, the one-step update
and the Philox normals are tests/sampling_reference.py's."""
import math

import torch

from tests import multistep_reference as mr
from tests import sampling_reference as sr


def steps_run(S, strength):
    """(n, k0): grid steps run and the first one; None where no step is left."""
    n = min(int(S * strength), S)
    return (n, S - n) if n > 0 else None


def noise_pair(t, T=1000):
    """(√ᾱ[t], √(1−ᾱ[t])) as Python floats (float64)."""
    ab = float(sr.alphas_cumprod(T)[t])
    return math.sqrt(ab), math.sqrt(1.0 - ab)


def noised(init, eps, t):
    k, n = noise_pair(t)
    return k * init.double() + n * eps.double()


def keep_pairs(timesteps):
    """(k_j, n_j) per evaluation of a run with these model timesteps: the noise level of the NEXT evaluation, (1, 0) last."""
    return [noise_pair(timesteps[j + 1]) if j + 1 < len(timesteps) else (1.0, 0.0) for j in range(len(timesteps))]


def blend(mask, init, eps, pair, x_new):
    """m·y + (1 − m)·x' with y = k·init + n·ε; `mask` broadcasts against the state."""
    m = mask.double()
    return m * (pair[0] * init.double() + pair[1] * eps.double()) + (1.0 - m) * x_new.double()


class PartialDpmpp2M(mr.Dpmpp2M):
    """DPM-Solver++(2M) over grid[k0:] with no history: the first step there is first order, the LAST one is when the full S is
    below 15."""

    def __init__(self, S, v_prediction, k0):
        super().__init__(S, v_prediction)
        self.timesteps = self.timesteps[k0:]

    def step(self, x, o):
        x, o = x.double(), o.double()
        s = self.timesteps[self.counter]
        a_s, s_s, l_s = self._asl(s)
        a_t, s_t, l_t = self._asl(s - self.ratio)
        x0 = a_s * x - s_s * o if self.v else (x - s_s * o) / a_s
        self.x0s = self.x0s[-1:]
        self.x0s.append(x0)
        h = l_t - l_s
        if self.counter == 0 or (self.counter == len(self.timesteps) - 1 and self.S < 15):
            d = self.x0s[-1]
        else:
            r = (l_s - self._asl(self.timesteps[self.counter - 1])[2]) / h
            d = (1 + 1 / (2 * r)) * self.x0s[-1] - (1 / (2 * r)) * self.x0s[-2]
        self.counter += 1
        return (s_t / s_s) * x - a_t * (torch.exp(-h) - 1) * d


def fresh_solver(method, S, v_prediction, k0):
    """The stateful solver of a run begun at grid step k0."""
    if method == "dpmpp_2m":
        return PartialDpmpp2M(S, v_prediction, k0)
    solver = mr.Plms(S, v_prediction)
    grid = sr.timesteps("ddim", S)[k0:]
    solver.timesteps = grid[:1] + grid[1:2] + grid[1:]  # the second one twice (one step left: the only one once)
    return solver


def run_timesteps(method, S, k0):
    """The model timestep of every evaluation of the run begun at grid step k0."""
    if method in ("ddpm", "ddim"):
        return sr.timesteps(method, S)[k0:]
    return fresh_solver(method, S, False, k0).timesteps


class Chain:
    """A whole run in float64: `state` after `start(init, eps)`, then `step(o, z)` per evaluation — the method's own update,
    then the blend where a mask is given.  `i` counts the run's evaluations; the one-step methods key their tables and their
    noise by the ABSOLUTE index k0 + i."""

    def __init__(self, method, S, k0, v_prediction=False, eta=0.0, mask=None):
        self.method, self.S, self.k0, self.v, self.eta, self.mask = method, S, k0, v_prediction, eta, mask
        self.timesteps = run_timesteps(method, S, k0)
        self.pairs = keep_pairs(self.timesteps)
        self.solver = fresh_solver(method, S, v_prediction, k0) if method in mr.SOLVERS else None
        self.i = 0

    def start(self, init, eps):
        self.init, self.eps = init.double(), eps.double()
        self.x = noised(init, eps, self.timesteps[0])
        return self.x

    def sigma(self):
        return sr.sigma(self.method, self.S, self.k0 + self.i, self.eta) if self.solver is None else 0.0

    def step(self, o, z=None):
        if self.solver is None:
            z = torch.zeros_like(self.x) if z is None else z
            x_new = sr.step(self.method, self.S, self.k0 + self.i, self.x, o, z, self.v, self.eta)
        else:
            x_new = self.solver.step(self.x, o)
        if self.mask is not None:
            x_new = blend(self.mask, self.init, self.eps, self.pairs[self.i], x_new)
        self.x, self.i = x_new, self.i + 1
        return x_new
