"""A gain schedule over (altitude, airspeed) for the LQR loop: the table f16_rollout_lqr_gs interpolates while flying.

Between the frozen gain of `F16Batch.rollout_LQR(K=...)` (valid near the trim point it was derived at) and the gain re-derived at every
step (`relinearise=True`) stands flight-control practice: derive the gain once over a grid of flight conditions and interpolate it on
the measured altitude and airspeed.  `GainSchedule.build` derives the table in one batch through calls the package already has (trim ->
linearise -> ZOH -> dlqr, one aircraft per node); `lookup` restates the lookup rule of include/f16_hip.h in numpy, operation by operation,
so its bits are those of the C function f16_gain_lookup_host and of the kernels.
"""
import ctypes

import numpy as np

from . import lib as _lib

ENTRIES = _lib.F16_GS_ENTRIES


class GainSchedule:
    """table [nh, nv, 12] on the uniform grid h0 + ih dh, v0 + iv dv: entries 3 i + j = K[i][4 + j] (K = -dlqr, as `_calc_LQR_gain`
    returns it), entries 9 + i = the trim surface command u_trim[1 + i].  ok [nh, nv]: whether the node's trim and gain are good."""

    def __init__(self, h0, dh, nh, v0, dv, nv, table, ok=None):
        self.h0, self.dh, self.nh = float(h0), float(dh), int(nh)
        self.v0, self.dv, self.nv = float(v0), float(dv), int(nv)
        if self.nh < 2 or self.nv < 2:
            raise ValueError("a gain schedule needs nh >= 2 and nv >= 2")
        if not (np.isfinite(self.dh) and np.isfinite(self.dv) and self.dh > 0 and self.dv > 0):
            raise ValueError("dh and dv must be finite and > 0")
        if not (np.isfinite(self.h0) and np.isfinite(self.v0)):
            raise ValueError("h0 and v0 must be finite")
        self.table = np.ascontiguousarray(table, dtype=np.float64)
        if self.table.shape != (self.nh, self.nv, ENTRIES):
            raise ValueError(f"table must be [{self.nh}, {self.nv}, {ENTRIES}], not {self.table.shape}")
        self.ok = np.ones((self.nh, self.nv), dtype=bool) if ok is None else np.asarray(ok, dtype=bool).reshape(self.nh, self.nv)
        self._device_tables = {}

    # ------------------------------------------------------------------ the rule
    def _axis(self, c, c0, d, n):
        """t = (c - c0) / d -> (cell index in 0..n-2, weight in [0, 1], outside): f16_gain_sched.hpp gain_axis"""
        with np.errstate(invalid="ignore", over="ignore"):
            t = (np.asarray(c, dtype=np.float64) - c0) / d
            i = np.fmin(np.fmax(np.floor(t), 0.0), float(n - 2))
            w = np.fmin(np.fmax(t - i, 0.0), 1.0)
            outside = ~((t >= 0.0) & (t <= float(n - 1)))
        return i.astype(np.int64), w, outside

    def lookup(self, h, v):
        """The 12 values at altitude h and airspeed v (arrays of one shape, or scalars) -> [..., 12].  Outside the grid the edge cell
        is extended flat (a clamp, no extrapolation); a NaN coordinate takes index 0 with weight 0."""
        h, v = np.broadcast_arrays(np.asarray(h, dtype=np.float64), np.asarray(v, dtype=np.float64))
        ih, lh, _ = self._axis(h, self.h0, self.dh, self.nh)
        iv, lv, _ = self._axis(v, self.v0, self.dv, self.nv)
        G, lh, lv = self.table, lh[..., None], lv[..., None]
        with np.errstate(invalid="ignore", over="ignore"):
            # (the weight 1 takes the upper value itself: p + (q - p) need not round to q -- gain_lerp of f16_gain_sched.hpp)
            lerp = lambda p, q, w: np.where(w >= 1.0, q, p + w * (q - p))
            return lerp(lerp(G[ih, iv], G[ih, iv + 1], lv), lerp(G[ih + 1, iv], G[ih + 1, iv + 1], lv), lh)

    def outside(self, h, v):
        """Whether (h, v) lies outside [h0, h0 + (nh-1) dh] x [v0, v0 + (nv-1) dv] or is not finite: what gs_out counts."""
        h, v = np.broadcast_arrays(np.asarray(h, dtype=np.float64), np.asarray(v, dtype=np.float64))
        return self._axis(h, self.h0, self.dh, self.nh)[2] | self._axis(v, self.v0, self.dv, self.nv)[2]

    # ------------------------------------------------------------------ what the C calls take
    def grid(self):
        """include/f16_hip.h f16_gain_grid"""
        return _lib.GainGrid(self.h0, self.dh, self.v0, self.dv, self.nh, self.nv)

    def device_table(self, device):
        """the table as a contiguous fp64 tensor on `device` (kept: the launch reads it in place)"""
        import torch
        key = str(torch.device(device))
        if key not in self._device_tables:
            self._device_tables[key] = torch.as_tensor(self.table).to(device=device).contiguous()
        return self._device_tables[key]

    def lookup_host(self, h, v):
        """f16_gain_lookup_host at the points (h, v): the C statement of the rule, on the host -> [n, 12]"""
        L, g = _lib.load(), self.grid()
        h, v = np.broadcast_arrays(np.asarray(h, dtype=np.float64), np.asarray(v, dtype=np.float64))
        h, v = h.ravel(), v.ravel()
        out = np.empty((h.size, ENTRIES), dtype=np.float64)
        for k in range(h.size):
            _lib.check(L.f16_gain_lookup_host(ctypes.byref(g), ctypes.c_void_p(self.table.ctypes.data), float(h[k]), float(v[k]),
                                              ctypes.c_void_p(out[k].ctypes.data)), L)
        return out

    # ------------------------------------------------------------------ files
    def save(self, path):
        np.savez(path, grid=np.array([self.h0, self.dh, self.v0, self.dv]), shape=np.array([self.nh, self.nv]), table=self.table, ok=self.ok)

    @classmethod
    def load(cls, path):
        with np.load(path) as f:
            (h0, dh, v0, dv), (nh, nv) = f["grid"], f["shape"]
            return cls(h0, dh, nh, v0, dv, nv, f["table"], f["ok"])

    # ------------------------------------------------------------------ the table from the plant
    @classmethod
    def build(cls, h0, dh, nh, v0, dv, nv, *, stab_flag=None, xcg=None, fi_flag=None, dt=None, Q=None, R=None, device="cuda:0",
              max_trim_cost=1e-4, strict=True, **trim_kw):
        """Trim, linearise, discretise and solve the LQR problem at every node, as ONE batch (node (ih, iv) = aircraft ih * nv + iv):
        `F16Batch.from_trim` then `_calc_LQR_gain(Q, R)`; K[:, :, 4:7] and the trim x[13:16] go into the table.  A node is bad when
        its trim cost exceeds max_trim_cost (the reference's Nelder-Mead is a knife edge at some conditions) or its trim or LQR status
        word is non-zero: strict=True raises a ValueError naming the bad nodes, strict=False returns the schedule with `ok` set.
        trim_kw (gamma, turn_rate, pullup_rate, runs, q0) goes to `F16Batch.from_trim`: the table is then derived about that climb,
        turn or pull-up at every node."""
        import torch
        from .env import F16Batch
        nh, nv = int(nh), int(nv)
        hh, vv = np.meshgrid(float(h0) + float(dh) * np.arange(nh), float(v0) + float(dv) * np.arange(nv), indexing="ij")
        kw = {k: val for k, val in dict(stab_flag=stab_flag, xcg=xcg, fi_flag=fi_flag, dt=dt).items() if val is not None}
        env = F16Batch.from_trim(hh.ravel(), vv.ravel(), device=device, **kw, **trim_kw)
        K = env._calc_LQR_gain(Q, R)                                         # [B, 3, 9]
        lqr_status = env.last_status
        table = torch.cat((K[:, :, 4:7].reshape(env.B, 9), env.x_values[:, 13:16]), 1).reshape(nh, nv, ENTRIES).cpu().numpy()
        cost, trim_status = env.trim_info["cost"].cpu().numpy(), env.trim_info["status"].cpu().numpy()
        ok = ((cost <= max_trim_cost) & (trim_status == 0) & (lqr_status.cpu().numpy() == 0)).reshape(nh, nv)
        gs = cls(h0, dh, nh, v0, dv, nv, table, ok)
        if strict and not ok.all():
            bad = [(int(i), int(j)) for i, j in zip(*np.nonzero(~ok))]
            raise ValueError(f"gain schedule: bad nodes (ih, iv) {bad}: trim cost above {max_trim_cost} or a non-zero trim / LQR status "
                             "(strict=False returns the schedule with `ok` set)")
        return gs
