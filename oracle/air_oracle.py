"""oracle/air_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT.

ctypes view of the moving-air entries of oracle/f16_oracle.c (f16o_xdot_wind_batch, f16o_xdot_air_parts_batch, f16o_rollout_wind),
for any of its three builds (oracle/lin_oracle.py: fp64, fma, ld).  Results come back in the type the build computes in (numpy
float64 or longdouble), never rounded on the way.
"""
import ctypes

import numpy as np

from oracle.lin_oracle import LinOracle


def _f64(a, *shape):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(*shape)


class AirOracle(LinOracle):
    def __init__(self, build="fp64", path=None):
        super().__init__(build, path)
        vp, d, i, l = ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_long
        L = self.lib
        L.f16o_xdot_wind_batch.argtypes = [vp, vp, vp, l, vp, vp, vp, i, d]
        L.f16o_xdot_air_parts_batch.argtypes = [vp, vp, vp, l, vp, vp, i, d]
        L.f16o_rollout_wind.argtypes = [vp] * 6 + [l, i, i, i, d, i, i, d] + [vp] * 4
        for f in (L.f16o_xdot_wind_batch, L.f16o_xdot_air_parts_batch, L.f16o_rollout_wind):
            f.restype = None

    def xdot_wind_batch(self, x, u, air, fi_flag=1, xcg=0.25, fix_clr=0):
        """x [B,18], u [B,4], air [B,6] = wN wE wD gx gy gz -> xdot [B,18], triple [B,6] = Ua Va Wa vt_a alpha_a beta_a, status [B]"""
        x, u, air = _f64(x, -1, 18), _f64(u, -1, 4), _f64(air, -1, 6)
        B = len(x)
        assert len(u) == B and len(air) == B
        out, tri, st = np.zeros((B, 18), self.dtype), np.zeros((B, 6), self.dtype), np.zeros(B, np.int32)
        self.set_fix_clr(fix_clr)
        try:
            self.lib.f16o_xdot_wind_batch(x.ctypes.data, u.ctypes.data, air.ctypes.data, B, out.ctypes.data, tri.ctypes.data, st.ctypes.data,
                                          int(fi_flag), float(xcg))
        finally:
            self.set_fix_clr(0)
        return out, tri, st

    def xdot_air_parts_batch(self, x, u, parts, fi_flag=1, xcg=0.25, fix_clr=0):
        """parts [B,6] = vt (atmosphere), vt (damping quotients), alpha, beta (lookups), V, alpha (flap model) -> xdot [B,18], status [B]"""
        x, u = _f64(x, -1, 18), _f64(u, -1, 4)
        parts = np.ascontiguousarray(parts, dtype=self.dtype).reshape(-1, 6)
        B = len(x)
        assert len(u) == B and len(parts) == B
        out, st = np.zeros((B, 18), self.dtype), np.zeros(B, np.int32)
        self.set_fix_clr(fix_clr)
        try:
            self.lib.f16o_xdot_air_parts_batch(x.ctypes.data, u.ctypes.data, parts.ctypes.data, B, out.ctypes.data, st.ctypes.data,
                                               int(fi_flag), float(xcg))
        finally:
            self.set_fix_clr(0)
        return out, st

    def rollout_wind(self, x0, rows, nsteps, hold, dt, method, fi_flag=1, xcg=0.25, wind=None, gusts=None, gust_hold=1, K=None, u0=None):
        """x0 [B,18]; rows [S,B,4] commands, or with K [B,27] / [27] and u0 [B,4]: rows [S,B,3] demanded rates; wind [B,3] or None;
        gusts [Sg,B,3] or None; method 1 = Euler, 4 = Runge-Kutta -> dict(x [B,18], traj [nsteps,B,18], u [B,4] or None, status [B])"""
        x0 = _f64(x0, -1, 18)
        B = len(x0)
        rows = _f64(rows, -1, B, 3 if K is not None else 4)
        assert len(rows) * hold >= nsteps
        keep = [x0, rows]
        ptr = lambda a: None if a is None else (keep.append(a), a.ctypes.data)[1]
        if K is not None:
            K = np.ascontiguousarray(np.broadcast_to(_f64(K, -1, 27), (B, 27)))
            u0 = _f64(u0, B, 4)
        wind = None if wind is None else _f64(wind, B, 3)
        if gusts is not None:
            gusts = _f64(gusts, -1, B, 3)
            assert len(gusts) * gust_hold >= nsteps
        x, traj = np.zeros((B, 18), self.dtype), np.zeros((nsteps, B, 18), self.dtype)
        uo, st = (np.zeros((B, 4), self.dtype) if K is not None else None), np.zeros(B, np.int32)
        self.lib.f16o_rollout_wind(ptr(x0), ptr(rows), ptr(K), ptr(u0), ptr(wind), ptr(gusts), B, int(nsteps), int(hold), int(gust_hold),
                                   float(dt), int(method), int(fi_flag), float(xcg), x.ctypes.data, traj.ctypes.data, ptr(uo), st.ctypes.data)
        return dict(x=x, traj=traj, u=uo, status=st)
