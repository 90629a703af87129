"""Ensemble statistics of rollouts (include/f16_hip.h "ENSEMBLE STATISTICS": f16_rollout_wind_ens, f16_rollout_lqr_wind_ens,
f16_ens_from_traj): the result type, the rule restated in numpy operation for operation, and one step of the group fold.

The rule in short (the header states it in full): aircraft b belongs to group b // group (group a multiple of 64); an aircraft
contributes to a sample iff its 18 values are finite and, with the envelope test on, inside the box of env.py:117-124; every
wavefront of 64 consecutive aircraft forms (n, mean, M2, min, max) per state row through balanced-tree sums; a group folds its
wave records in ascending order by Chan's update, every operation rounded on its own.  numpy never contracts a * b + c, so the
expressions below are the device's.
"""
import numpy as np

from . import parameters as P

WAVE = 64
X_LB, X_UB = np.array(P.x_lb, dtype=np.float64), np.array(P.x_ub, dtype=np.float64)


class Ensemble:
    """count [S, G] (int32), mean, m2, min, max [S, G, 18]: per sample and group the number of contributing aircraft and, per state,
    their mean, sum of squared deviations from it, minimum and maximum.  numpy arrays or torch tensors alike.  var = m2 / (count - 1),
    NaN where count < 2; an empty group has mean 0, m2 0, min +inf, max -inf."""

    def __init__(self, count, mean, m2, min, max, group=None):
        self.count, self.mean, self.m2, self.min, self.max, self.group = count, mean, m2, min, max, group

    def parts(self):
        return self.count, self.mean, self.m2, self.min, self.max

    @property
    def var(self):
        c = self.count[..., None]
        if isinstance(self.m2, np.ndarray):
            with np.errstate(invalid="ignore", divide="ignore"):
                return np.where(c >= 2, self.m2 / (c - 1.0), np.nan)
        import torch
        return torch.where(c >= 2, self.m2 / (c.to(self.m2.dtype) - 1.0), torch.full_like(self.m2, float("nan")))

    def numpy(self):
        """the same result as numpy arrays on the host"""
        return Ensemble(*(v if isinstance(v, np.ndarray) else v.detach().cpu().numpy() for v in self.parts()), group=self.group)


def contributes(traj, envelope=True):
    """the mask of the rule: traj [S, 18, B] -> [S, B] bool"""
    x = np.asarray(traj, dtype=np.float64)
    m = np.isfinite(x).all(1)
    if envelope:
        with np.errstate(invalid="ignore"):
            m &= ((x >= X_LB[None, :, None]) & (x <= X_UB[None, :, None])).all(1)
    return m


def _tree(v):
    """the balanced tree over the last axis (64 lanes): v = v[0::2] + v[1::2], six times"""
    for _ in range(6):
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def wave_records(traj, envelope=True):
    """traj [S, 18, B] -> (n [S, W], mean, m2, min, max [S, 18, W]) with W = ceil(B / 64): the per-wavefront records of the rule"""
    x = np.asarray(traj, dtype=np.float64)
    S, K, B = x.shape
    assert K == 18 and B >= 1
    W = (B + WAVE - 1) // WAVE
    m = np.zeros((S, W * WAVE), dtype=bool)
    m[:, :B] = contributes(x, envelope)
    xp = np.zeros((S, 18, W * WAVE))
    xp[..., :B] = x
    m = np.broadcast_to(m.reshape(S, 1, W, WAVE), (S, 18, W, WAVE))
    xp = xp.reshape(S, 18, W, WAVE)
    n = m[:, 0].sum(-1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = _tree(np.where(m, xp, 0.0))
        mean = np.where(n[:, None] > 0, s / n[:, None].astype(np.float64), 0.0)
        d = np.where(m, xp - mean[..., None], 0.0)
        m2 = np.where(n[:, None] > 0, _tree(d * d), 0.0)
    mn = np.where(m, xp, np.inf).min(-1)
    mx = np.where(m, xp, -np.inf).max(-1)
    return n, mean, m2, mn, mx


def combine(a, b):
    """One step of the group fold on (count, mean, m2, min, max) tuples (arrays of matching shapes: count [...], the others
    [..., 18] -- or every one of the same shape): a with b folded in behind it.  An empty b leaves a as it is, an empty a gives b as
    it is; otherwise N = n + n_b, delta = mean_b - mean, mean + delta * (n_b / N), (M2 + M2_b) + (delta * delta) * ((n * n_b) / N),
    every operation rounded on its own; min and max by fmin and fmax.  Not associative: the order of the folds is part of a result."""
    na, nb = np.asarray(a[0]), np.asarray(b[0])
    ma, mb = (np.asarray(v, dtype=np.float64) for v in (a[1], b[1]))
    ea = na[..., None] if ma.ndim == na.ndim + 1 else na
    eb = nb[..., None] if mb.ndim == nb.ndim + 1 else nb
    fa, fb = ea.astype(np.float64), eb.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        N = fa + fb
        delta = mb - ma
        mean = ma + delta * (fb / N)
        m2 = (np.asarray(a[2]) + np.asarray(b[2])) + (delta * delta) * ((fa * fb) / N)
    keep_a, keep_b = eb == 0, (ea == 0) & (eb != 0)
    mean = np.where(keep_a, ma, np.where(keep_b, mb, mean))
    m2 = np.where(keep_a, a[2], np.where(keep_b, b[2], m2))
    return (na + nb).astype(na.dtype), mean, m2, np.fmin(a[3], b[3]), np.fmax(a[4], b[4])


def ensemble_reference(traj, group, envelope=True):
    """The statistic of include/f16_hip.h in numpy: traj [S, 18, B] (the layout the rollouts return), group = aircraft per group (a
    multiple of 64, >= 64; True: one group, the whole batch) -> Ensemble of numpy arrays, count [S, G], the others [S, G, 18]."""
    x = np.asarray(traj, dtype=np.float64)
    S, _, B = x.shape
    group = group_size(group, B)
    n, mean, m2, mn, mx = wave_records(x, envelope)
    W = n.shape[1]
    wpg = min(group // WAVE, W)
    G = (B + group - 1) // group
    acc = (np.zeros((S, G), dtype=np.int32), np.zeros((S, G, 18)), np.zeros((S, G, 18)), np.full((S, G, 18), np.inf), np.full((S, G, 18), -np.inf))
    for j in range(wpg):
        rec = [np.zeros((S, G), dtype=np.int32), np.zeros((S, G, 18)), np.zeros((S, G, 18)), np.full((S, G, 18), np.inf), np.full((S, G, 18), -np.inf)]
        w = np.arange(G) * wpg + j
        ok = w < W
        rec[0][:, ok] = n[:, w[ok]]
        for dst, src in zip(rec[1:], (mean, m2, mn, mx)):
            dst[:, ok] = src[:, :, w[ok]].transpose(0, 2, 1)
        acc = combine(acc, tuple(rec))
    return Ensemble(*acc, group=group)


def group_size(group, B):
    """the `ensemble=` keyword -> aircraft per group: True = one group holding the whole batch; else a multiple of 64, >= 64"""
    if group is True:
        return max(WAVE, (int(B) + WAVE - 1) // WAVE * WAVE)
    if isinstance(group, bool) or int(group) != group or int(group) < WAVE or int(group) % WAVE:
        raise ValueError(f"ensemble / group must be True or a multiple of 64 (>= 64), not {group!r}")
    return int(group)
