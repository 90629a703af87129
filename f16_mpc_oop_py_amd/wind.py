"""Steady wind and sampled gusts for the rollouts (include/f16_hip.h: f16_rollout_wind, f16_rollout_lqr_wind, f16_gust_sample).

`GustModel` is what F16Batch.rollout_schedule / rollout_LQR take as `gusts=` for in-kernel generation: the coefficients of the
first-order Gauss-Markov process per body axis, the seed, and -- per batch it has flown with -- the generator's state and row counter,
so that consecutive calls continue one sequence.  `gust_coefficients` restates f16_gust_coeffs_host and `gust_reference` the sampler
in numpy (on mppi.philox4x32_10): documentation and the tests' reference, like mppi.sample_reference; the product never calls them.
"""
import ctypes

import numpy as np

from . import cabi
from . import lib as _lib
from .mppi import philox4x32_10

GUST_COUNTER_WORD = 0xFFFFFFFF        # counter word 2 of a gust row: a value MPPI's sample index (< 256) never takes


def gust_coefficients(sigma, length, v0, dt_row):
    """a = exp(-v0 dt_row / L), b = sigma sqrt(1 - a^2) per body axis: the exact discretisation of the first-order Dryden form at the
    frozen airspeed v0 over the row period dt_row -- the stationary standard deviation is sigma whatever the row period.
    sigma, length: scalars or three values (ft/s, ft) -> (a [3], b [3])."""
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (3,))
    L = np.broadcast_to(np.asarray(length, dtype=np.float64), (3,))
    if not (np.all(np.isfinite(sg)) and np.all(sg >= 0) and np.all(np.isfinite(L)) and np.all(L > 0) and 0 < v0 < np.inf and 0 < dt_row < np.inf):
        raise ValueError("sigma must be finite and >= 0; length, v0 and dt_row finite and > 0")
    a = np.exp(-(float(v0) * float(dt_row)) / L)
    return a, sg * np.sqrt(1.0 - a * a)


def gust_coefficients_host(sigma, length, v0, dt_row):
    """The same through the library's host function f16_gust_coeffs_host (no GPU, no context)."""
    d3 = ctypes.c_double * 3
    sg, L = d3(*np.broadcast_to(np.asarray(sigma, dtype=np.float64), (3,))), d3(*np.broadcast_to(np.asarray(length, dtype=np.float64), (3,)))
    a, b = d3(), d3()
    lib = cabi.declare(ctypes.CDLL(_lib.build()))
    rc = lib.f16_gust_coeffs_host(sg, L, float(v0), float(dt_row), a, b)
    if rc != 0:
        raise _lib.F16HipError(f"libf16hip error {rc}: {lib.f16_last_error().decode()}")
    return np.array(a), np.array(b)


def gust_normals(seed, row0, nrows, aircraft):
    """The three standard normals of gust rows row0 .. row0 + nrows - 1 of `aircraft` aircraft, [nrows, aircraft, 3]: f16_mppi_sample's
    rule (U_i = (r_i + 0.5) 2^-32; Box-Muller on (U0, U1) -> cos, sin and on (U2, U3) -> cos) from the Philox counter
    (row, 0, 0xFFFFFFFF, aircraft), key = the two halves of the seed."""
    seed = int(seed)
    r, a = np.meshgrid((np.arange(nrows, dtype=np.uint64) + np.uint64(int(row0))) & np.uint64(0xffffffff), np.arange(aircraft, dtype=np.uint64),
                       indexing="ij")
    ctr = np.stack([r, np.zeros_like(r), np.full_like(r, GUST_COUNTER_WORD), a], -1)
    w = philox4x32_10(ctr, np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], dtype=np.uint64))
    U = (w.astype(np.float64) + 0.5) * 2.0 ** -32
    ra, rb = np.sqrt(-2.0 * np.log(U[..., 0])), np.sqrt(-2.0 * np.log(U[..., 2]))
    return np.stack([ra * np.cos(2.0 * np.pi * U[..., 1]), ra * np.sin(2.0 * np.pi * U[..., 1]), rb * np.cos(2.0 * np.pi * U[..., 3])], -1)


def gust_reference(a, b, state, seed, row0, nrows):
    """f16_gust_sample restated: g(r) = (a * g(r-1)) + (b * n(r)) per axis, each operation rounded on its own.  a, b: [3] or [B, 3];
    state [B, 3]: the row before row0 (zeros for a fresh sequence) -> (rows [nrows, B, 3], the last row [B, 3])."""
    g = np.array(state, dtype=np.float64)
    if g.ndim != 2 or g.shape[1] != 3:
        raise ValueError(f"state must be [B, 3], not {g.shape}")
    a, b = np.broadcast_to(np.asarray(a, dtype=np.float64), g.shape), np.broadcast_to(np.asarray(b, dtype=np.float64), g.shape)
    n = gust_normals(seed, row0, nrows, len(g))
    out = np.zeros((nrows,) + g.shape)
    for r in range(nrows):
        g = (a * g) + (b * n[r])
        out[r] = g
    return out, g


class GustModel:
    """First-order Gauss-Markov gusts per body axis, generated inside the rollout kernels: sigma (ft/s) and length (ft), scalars or
    three values (x forward, y right, z down), at the frozen nominal airspeed v0 (ft/s); a new row every `every` steps.  The object
    keeps ONE sequence per (batch size, dt, device) it has flown with -- the generator's state [3, B] and the row counter -- so
    consecutive rollouts of a batch continue that batch's sequence, and two batches that alternate on one model do not disturb each
    other (a call whose step count is not a multiple of `every` ends inside a row; the next call starts a new one).  `row` is the
    counter of the sequence used last; reset() starts every sequence again."""

    def __init__(self, sigma, length, v0, seed=0, every=1):
        self.sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (3,)).copy()
        self.length = np.broadcast_to(np.asarray(length, dtype=np.float64), (3,)).copy()
        self.v0, self.seed, self.every = float(v0), int(seed), int(every)
        if self.every < 1:
            raise ValueError("every must be >= 1")
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must fit 64 bits")
        gust_coefficients(self.sigma, self.length, self.v0, 1.0)      # (the argument rules)
        self.reset()

    def reset(self):
        self._seqs, self._last = {}, None      # {(B, dt, device): [ga, gb, gstate, row]}; the key used last

    @property
    def row(self):
        return self._seqs[self._last][3] if self._last is not None else 0

    def coefficients(self, dt):
        return gust_coefficients(self.sigma, self.length, self.v0, self.every * float(dt))

    def device_state(self, B, dt, device):
        """(ga [3, B], gb [3, B], gstate [3, B]) on the device for a batch of B aircraft stepping with dt: that batch's sequence, which
        `row` and advance() refer to until another batch asks"""
        import torch
        key = (int(B), float(dt), str(device))
        if key not in self._seqs:
            a, b = self.coefficients(dt)
            col = lambda v: torch.as_tensor(v, dtype=torch.float64, device=device).unsqueeze(1).expand(3, B).contiguous()
            self._seqs[key] = [col(a), col(b), torch.zeros((3, B), dtype=torch.float64, device=device), 0]
        self._last = key
        return tuple(self._seqs[key][:3])

    def advance(self, nsteps):
        """the sequence used last has drawn ceil(nsteps / every) rows"""
        seq = self._seqs[self._last]
        seq[3] = (seq[3] + (int(nsteps) + self.every - 1) // self.every) & 0xffffffff
