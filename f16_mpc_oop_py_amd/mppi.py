"""The softmin blend of an MPPI (model-predictive path integral control) step, stated in plain torch on the CPU.

This is the rule the device entry `f16_mppi_blend` (include/f16_hip.h; F16Batch.blend_schedules) implements, written out once as
documentation and as the tests' reference.  It is not a fallback: F16Batch never calls it.
"""
import torch


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
