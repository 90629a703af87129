"""The two rules of an MPPI (model-predictive path integral control) step that the library defines, stated on the CPU: the softmin blend
in plain torch, and the counter-based sampler (Philox4x32-10 + Box-Muller) in numpy.

These are the rules the device entries `f16_mppi_blend` and `f16_mppi_sample` (include/f16_hip.h; F16Batch.blend_schedules,
F16Batch.sample_schedules) and the fused loop `f16_rollout_mppi` implement, written out once as documentation and as the tests'
reference.  They are not a fallback: F16Batch never calls them.
"""
import numpy as np
import torch

from . import parameters as P

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57      # multipliers on counter words 0 and 2
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85      # key increments


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) on arrays: counter [..., 4], key [..., 2] (uint32 values) -> [..., 4] uint32.
    Per round (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); ten rounds, the key bumped after
    each."""
    c = [np.asarray(counter, dtype=np.uint64)[..., i] & 0xffffffff for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & 0xffffffff for i in range(2)]
    c = list(np.broadcast_arrays(*c, *k)[:4])
    mask = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]       # 64-bit products of 32-bit values: exact
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(PHILOX_W0)) & mask, (k[1] + np.uint64(PHILOX_W1)) & mask]
    return np.stack(c, -1).astype(np.uint32)


def normals_reference(seed, period, rows, samples, aircraft):
    """The three standard normals of every (row, sample, aircraft) of one period: [rows, samples, aircraft, 3] fp64.  Counter =
    (period, row, k, a), key = (seed & 0xffffffff, seed >> 32); U_i = (r_i + 0.5) 2^-32; Box-Muller on (U0, U1) -> n0 (cos), n1 (sin)
    and on (U2, U3) -> n2 (cos)."""
    seed = int(seed)
    s, k, a = np.meshgrid(np.arange(rows, dtype=np.uint64), np.arange(samples, dtype=np.uint64), np.arange(aircraft, dtype=np.uint64),
                          indexing="ij")
    ctr = np.stack([np.full_like(s, int(period) & 0xffffffff), s, k, a], -1)
    r = philox4x32_10(ctr, np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], dtype=np.uint64))
    U = (r.astype(np.float64) + 0.5) * 2.0 ** -32
    ra, rb = np.sqrt(-2.0 * np.log(U[..., 0])), np.sqrt(-2.0 * np.log(U[..., 2]))
    return np.stack([ra * np.cos(2.0 * np.pi * U[..., 1]), ra * np.sin(2.0 * np.pi * U[..., 1]), rb * np.cos(2.0 * np.pi * U[..., 3])], -1)


def sample_reference(nominal, sigma, samples, seed, period):
    """The sample set of an MPPI period as the device entry `f16_mppi_sample` (include/f16_hip.h; F16Batch.sample_schedules) writes it,
    restated in numpy: nominal [S, B, 4], sigma a scalar or the three surface deviations -> [S, K, B, 4].  The thrust command is the
    nominal one; the three surface commands are clip(nominal + sigma * n, limits of parameters.py:125-126), a NaN staying NaN.
    Documentation and the tests' reference, like blend_reference: the product never calls it."""
    nom = np.asarray(nominal, dtype=np.float64)
    if nom.ndim != 3 or nom.shape[2] != 4:
        raise ValueError(f"nominal must be [S, B, 4], not {nom.shape}")
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (3,))
    S, B = nom.shape[:2]
    n = normals_reference(seed, period, S, int(samples), B)
    out = np.repeat(nom[:, None], int(samples), 1).copy()
    out[..., 1:] = np.clip(out[..., 1:] + sg * n, np.asarray(P.u_lb[1:], dtype=np.float64), np.asarray(P.u_ub[1:], dtype=np.float64))
    return out


def blend_reference(cost, actions, lam, return_info=False):
    """cost [K, B]: the trajectory cost of sample k of aircraft b; actions [S, K, B, C]: the sampled schedules; lam > 0: the temperature.

    Per aircraft, over its K samples:
        m   = min of the FINITE costs
        w_k = exp(-(cost_k - m) / lam)    for finite cost_k, else 0 (such a sample is not read at all: NaN commands do not spread)
        u   = sum_k w_k actions[:, k] / sum_k w_k        summed over k ascending in fp64
    The minimum-cost sample has weight exactly 1, so the sums never vanish; an aircraft WITHOUT a finite cost gets sample 0's rows,
    weights 0 and statistics 0.  Returns u [S, B, C]; with return_info also dict(weights [K, B] normalised to sum 1, min_cost [B],
    ess [B] = (sum w)^2 / sum w^2, the effective sample size)."""
    cost = torch.as_tensor(cost, dtype=torch.float64).cpu()
    actions = torch.as_tensor(actions, dtype=torch.float64).cpu()
    lam = float(lam)
    if not (lam > 0.0 and lam < float("inf")):
        raise ValueError(f"lam must be finite and > 0 (got {lam})")
    if cost.dim() != 2 or actions.dim() != 4 or tuple(actions.shape[1:3]) != tuple(cost.shape):
        raise ValueError(f"cost [K, B] and actions [S, K, B, C] must agree, not {tuple(cost.shape)} and {tuple(actions.shape)}")
    K, B = cost.shape
    finite = torch.isfinite(cost)
    some = finite.any(0)
    m = torch.where(finite, cost, torch.full_like(cost, float("inf"))).min(0).values
    m = torch.where(some, m, torch.zeros_like(m))
    w = torch.where(finite, torch.exp(-(cost - m) / lam), torch.zeros_like(cost))
    sw, sw2 = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    acc = torch.zeros_like(actions[:, 0])
    for k in range(K):
        sw = sw + w[k]
        sw2 = sw2 + w[k] * w[k]
        acc = acc + torch.where(finite[k][None, :, None], w[k][None, :, None] * actions[:, k], torch.zeros_like(acc))
    safe = torch.where(some, sw, torch.ones_like(sw))
    u = torch.where(some[None, :, None], acc / safe[None, :, None], actions[:, 0])
    if not return_info:
        return u
    ess = torch.where(some, sw * sw / torch.where(some, sw2, torch.ones_like(sw2)), torch.zeros_like(sw))
    return u, dict(weights=w / safe, min_cost=m, ess=ess)
