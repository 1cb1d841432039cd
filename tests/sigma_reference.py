"""CPU side of the sigma-space sampler tests: k-diffusion's Euler, Euler-ancestral and Heun samplers (Karras et al. 2022,
Algorithm 1 for Heun; sample_euler / sample_euler_ancestral / sample_heun as published) as STATEFUL float64 classes, written
the way the samplers are written — `denoised`, `d`, `sigma_up` / `sigma_down`, a saved sample and a saved derivative, one
`step(x, o, z)` per model evaluation.  k-diffusion and diffusers are not part of the reference tree: restated from the paper and
the published code's behaviour.  The product collapses every iteration to coefficients (sampling.sigma_schedule); nothing here
shares code with it, the sigma grid included."""
import math

import numpy as np
import torch

T = 1000
RHO = 7.0


def sigma_table(beta_start=0.00085, beta_end=0.012):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float64) ** 2
    acp = torch.cumprod(1.0 - betas, dim=0)
    return ((1.0 - acp) / acp).sqrt().numpy()


def _interp(t, table):
    """The table at a fractional row, by hand: the two neighbours weighted by the fraction."""
    lo = min(int(math.floor(t)), T - 2)
    w = t - lo
    return (1.0 - w) * table[lo] + w * table[lo + 1]


def _sigma_to_t(sigma, table):
    """k-diffusion's DiscreteSchedule.sigma_to_t (quantize=False): linear in log σ between the two rows around it."""
    log_sigma, logs = math.log(sigma), np.log(table)
    low = int(np.clip(np.cumsum(log_sigma - logs >= 0).argmax(), 0, T - 2))
    w = (logs[low] - log_sigma) / (logs[low] - logs[low + 1])
    w = min(max(w, 0.0), 1.0)
    return (1.0 - w) * low + w * (low + 1)


def grid(S, karras=False, timesteps=None):
    """(timesteps [S], sigmas [S + 1]) float64 lists: the scheduler's grid, σ_S = 0."""
    table = sigma_table()
    if karras:
        lo, hi = table[0] ** (1 / RHO), table[-1] ** (1 / RHO)
        sig = [float((hi + (i / (S - 1) if S > 1 else 0.0) * (lo - hi)) ** RHO) for i in range(S)]
        ts = [_sigma_to_t(s, table) for s in sig]
    else:
        if timesteps is None:
            timesteps = [float(T - 1)] if S == 1 else [float(T - 1) * (S - 1 - i) / (S - 1) for i in range(S)]
        ts = [float(t) for t in timesteps]
        sig = [float(_interp(t, table)) for t in ts]
    return ts, sig + [0.0]


class _Sampler:
    """`step(x, o, z)`: the state after one model evaluation `o` at `model_sigma` / `model_timestep`, the model having seen
    `model_input(x)`.  `done` once the run is over."""

    def __init__(self, S, v_prediction, karras=False, timesteps=None):
        self.ts, self.sigmas = grid(S, karras, timesteps)
        self.S, self.v, self.i = S, bool(v_prediction), 0

    def denoised(self, x, o, sigma):
        if self.v:
            return x / (sigma ** 2 + 1.0) - o * sigma / math.sqrt(sigma ** 2 + 1.0)
        return x - sigma * o

    def to_d(self, x, o, sigma):
        return (x - self.denoised(x, o, sigma)) / sigma

    @property
    def done(self):
        return self.i >= self.S

    @property
    def model_sigma(self):
        return self.sigmas[self.i]

    @property
    def model_timestep(self):
        return self.ts[self.i]

    def model_input(self, x):
        return x / math.sqrt(self.model_sigma ** 2 + 1.0)

    def start(self, z):
        return self.sigmas[0] * z.double()


class Euler(_Sampler):
    noise_scale = 0.0

    def step(self, x, o, z=None):
        x, o = x.double(), o.double()
        sigma, sigma_next = self.sigmas[self.i], self.sigmas[self.i + 1]
        d = self.to_d(x, o, sigma)
        self.i += 1
        return x + d * (sigma_next - sigma)


class EulerAncestral(_Sampler):
    def ancestral(self):
        s, n = self.sigmas[self.i], self.sigmas[self.i + 1]
        up = math.sqrt(n ** 2 * (s ** 2 - n ** 2) / s ** 2)
        return math.sqrt(n ** 2 - up ** 2), up

    @property
    def noise_scale(self):
        return self.ancestral()[1]

    def step(self, x, o, z):
        x, o = x.double(), o.double()
        sigma = self.sigmas[self.i]
        sigma_down, sigma_up = self.ancestral()
        d = self.to_d(x, o, sigma)
        x = x + d * (sigma_down - sigma)
        if sigma_up > 0.0:
            x = x + z.double() * sigma_up
        self.i += 1
        return x


class Heun(_Sampler):
    """Two model evaluations per step with σ' > 0: the second on the Euler-predicted state at σ'."""
    noise_scale = 0.0

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.sample = self.d1 = None  # saved between the two evaluations of a step

    @property
    def second(self):
        return self.sample is not None

    @property
    def model_sigma(self):
        return self.sigmas[self.i + 1] if self.second else self.sigmas[self.i]

    @property
    def model_timestep(self):
        return self.ts[self.i + 1] if self.second else self.ts[self.i]

    def step(self, x, o, z=None):
        x, o = x.double(), o.double()
        sigma, sigma_next = self.sigmas[self.i], self.sigmas[self.i + 1]
        dt = sigma_next - sigma
        if not self.second:
            d = self.to_d(x, o, sigma)
            if sigma_next == 0.0:  # the last step: Euler
                self.i += 1
                return x + d * dt
            self.sample, self.d1 = x, d
            return x + d * dt
        d_2 = self.to_d(x, o, sigma_next)
        d_prime = (self.d1 + d_2) / 2.0
        x = self.sample + d_prime * dt
        self.sample = self.d1 = None
        self.i += 1
        return x


SAMPLERS = {"euler": Euler, "euler_a": EulerAncestral, "heun": Heun}


def make(method, S, v_prediction, karras=False, timesteps=None):
    return SAMPLERS[method](S, v_prediction, karras, timesteps)


def walk(method, S, v_prediction, karras=False):
    """[(timestep, σ of the evaluation, noise scale, σ of the next evaluation or None)] per iteration of a run: the reference's
    own bookkeeping, stepped with dummy data."""
    smp, rows, x = make(method, S, v_prediction, karras), [], torch.zeros(1, dtype=torch.float64)
    while not smp.done:
        rows.append([smp.model_timestep, smp.model_sigma, smp.noise_scale, None])
        x = smp.step(x, x, x)
        if not smp.done:
            rows[-1][3] = smp.model_sigma
    return rows
