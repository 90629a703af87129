"""The plant in steady wind and gusts (include/f16_hip.h: f16_xdot_wind_batch, f16_rollout_wind, f16_rollout_lqr_wind) restated in
numpy on the checker's existing exports only, and the cases tests/test_wind_cpu.py and tests/test_gpu_wind.py share.

The twin of one derivative.  With C = body from NED and the air triple of the rule (include/f16_hip.h):
    xa = x with entries 6..8 replaced by (vt_a, alpha_a, beta_a);   d0 = oracle.calc_xdot(x, u);   dA = oracle.calc_xdot(xa, u)
    result[0:6] = d0[0:6] (navigation and kinematics: the ground triple);   result[9:18] = dA[9:18] (moments, actuators, flap: the air)
    result[6:9]: dA[6:9] turned into the body-axis derivative of the AIR velocity by differentiating (V ca cb, V sb, V sa cb) at the
    air triple, minus omega x (C w_ned + g_b) -- exact: the force equations are those of a still-air aircraft at the air triple --
    turned into (Vdot, alphadot, betadot) of the GROUND triple by the three quotients of nlplant.c:397-405.
The grid bits are those of the evaluation at xa (oracle.lib.f16o_last_status after it).

The twin of a rollout: rk4_cases.restate -- the Runge-Kutta restatement of the suite -- with f replaced, through an object that
stands for the oracle and answers calc_xdot with the twin at ONE aircraft's wind and gust row; the rollout is restated aircraft by
aircraft and segment by segment (split at every hold and gust_hold boundary, the status carried along), which is the chain the
device call promises to equal.  envelope_cases.restate_schedule steps inside the checker's C loop, where f cannot be replaced, so
the Euler method is restated here by the same walk with one stage (x + dt f, the box test in front).
"""
import numpy as np

import envelope_cases as ec
import rk4_cases as rk

XCG = ec.XCG
HOLD, GUST_HOLD, T_MAX = 7, 3, 40
EPS = 2.0 ** -52


def body_from_ned(phi, theta, psi):
    sphi, cphi, st, ct, spsi, cpsi = np.sin(phi), np.cos(phi), np.sin(theta), np.cos(theta), np.sin(psi), np.cos(psi)
    return np.array([[ct * cpsi, ct * spsi, -st],
                     [sphi * st * cpsi - cphi * spsi, sphi * st * spsi + cphi * cpsi, sphi * ct],
                     [cphi * st * cpsi + sphi * spsi, cphi * st * spsi - sphi * cpsi, cphi * ct]])


def ground_uvw(x):
    vt = 0.01 if x[6] <= 0.01 else x[6]
    ca, sa, cb, sb = np.cos(x[7]), np.sin(x[7]), np.cos(x[8]), np.sin(x[8])
    return np.array([vt * ca * cb, vt * sb, vt * sa * cb]), vt, cb


def air_state(x, w_ned, g_b):
    """x with entries 6..8 replaced by the air triple"""
    uvw, _, _ = ground_uvw(x)
    a = uvw - body_from_ned(x[3], x[4], x[5]) @ np.asarray(w_ned, dtype=np.float64) - np.asarray(g_b, dtype=np.float64)
    xa = np.array(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        xa[6] = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
        xa[7] = np.arctan2(a[2], a[0])
        xa[8] = np.arcsin(a[1] / xa[6])
    return xa


def twin_xdot(oracle, x, u, w_ned, g_b, fi, xcg=XCG):
    """-> (xdot [18], the grid bits of the evaluation at the air triple)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    xa = air_state(x, w_ned, g_b)
    d0 = oracle.calc_xdot(x, u, fi, xcg)
    dA = oracle.calc_xdot(xa, u, fi, xcg)
    st = int(oracle.lib.f16o_last_status())
    out = d0.copy()
    out[9:18] = dA[9:18]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        V = 0.01 if xa[6] <= 0.01 else xa[6]
        ca, sa, cb, sb = np.cos(xa[7]), np.sin(xa[7]), np.cos(xa[8]), np.sin(xa[8])
        vd, ad, bd = dA[6:9]
        acc = np.array([vd * ca * cb - V * sa * cb * ad - V * ca * sb * bd,
                        vd * sb + V * cb * bd,
                        vd * sa * cb + V * ca * cb * ad - V * sa * sb * bd])
        v = body_from_ned(x[3], x[4], x[5]) @ np.asarray(w_ned, dtype=np.float64) + np.asarray(g_b, dtype=np.float64)
        P, Q, R = x[9:12]
        acc -= np.array([Q * v[2] - R * v[1], R * v[0] - P * v[2], P * v[1] - Q * v[0]])
        (U, Vg, W), vt, cbg = ground_uvw(x)
        out[6] = (U * acc[0] + Vg * acc[1] + W * acc[2]) / vt
        out[7] = (U * acc[2] - W * acc[0]) / (U * U + W * W)
        out[8] = (acc[1] * vt - Vg * out[6]) / (vt * vt * cbg)
    return out, st


class WindOracle:
    """stands for the oracle in rk4_cases.restate: calc_xdot is the twin at one aircraft's wind and gust row"""

    def __init__(self, oracle, w_ned, g_b):
        self.oracle, self.w, self.g, self._st = oracle, w_ned, g_b, 0
        self.lib, self._p = self, oracle._p

    def calc_xdot(self, x, u, fi, xcg):
        out, self._st = twin_xdot(self.oracle, x, u, self.w, self.g, fi, xcg)
        return out

    def f16o_last_status(self):
        return self._st

    def f16o_envelope_bits(self, p):
        return self.oracle.lib.f16o_envelope_bits(p)


def _euler(proxy, x0, rows, T, dt, fi, xcg, K, u0, status0):
    """rk4_cases.restate's walk with one stage, for one aircraft and one row -> what restate returns (stages: none)"""
    x, st = np.array(x0, dtype=np.float64), np.array(status0, dtype=np.int32)
    traj, lqr = np.zeros((T, 1, 18)), K is not None
    u_last = np.array(u0 if lqr else rows[0], dtype=np.float64)
    for t in range(T):
        if not st[0] & ec.ST_ENVELOPE:
            st[0] |= proxy.f16o_envelope_bits(proxy._p(x[0]))
        if not st[0] & ec.ST_ENVELOPE:
            if lqr:
                e = rows[0, 0] - x[0, 9:12]
                u = u0[0].copy()
                for i in range(3):
                    u[1 + i] = (((-K[i, 4]) * e[0] + (-K[i, 5]) * e[1]) + (-K[i, 6]) * e[2]) + u0[0, 1 + i]
                u_last[0] = u
            else:
                u = rows[0, 0]
            with np.errstate(invalid="ignore", over="ignore"):
                x[0] = x[0] + proxy.calc_xdot(x[0], u, fi, xcg) * dt
            st[0] |= proxy.f16o_last_status()
        traj[t] = x
    return dict(traj=traj, raw_status=st, stages=np.full((T, 0, 1, 18), np.nan), u_last=u_last if lqr else None, x=x)


def fly(oracle, x0, rows, hold, T, dt, fi, method, wind=None, gusts=None, gust_hold=1, K=None, u0=None, xcg=XCG):
    """The twin of f16_rollout_wind (rows [S, B, 4]) / f16_rollout_lqr_wind (K [3, 9], u0 [B, 4], rows [S, B, 3]); wind [B, 3] or None,
    gusts [Sg, B, 3] or None -> dict(traj [T, B, 18], status [B], u_last [B, 4] or None, stages [n, B, 18]: every stage state)"""
    x0 = np.asarray(x0, dtype=np.float64)
    B = len(x0)
    wind = np.zeros((B, 3)) if wind is None else np.broadcast_to(np.asarray(wind, dtype=np.float64), (B, 3))
    gusts, gust_hold = (np.zeros((1, B, 3)), T) if gusts is None else (np.asarray(gusts, dtype=np.float64), gust_hold)
    cuts = sorted(set(range(0, T, hold)) | set(range(0, T, gust_hold)) | {T})
    traj, status, u_last, stages = np.zeros((T, B, 18)), np.zeros(B, dtype=np.int32), None if K is None else np.zeros((B, 4)), []
    for b in range(B):
        x, st, sb = x0[b:b + 1].copy(), np.zeros(1, dtype=np.int32), []
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            proxy = WindOracle(oracle, wind[b], gusts[t0 // gust_hold, b])
            row = np.ascontiguousarray(rows[t0 // hold][None, b:b + 1])
            kw = dict(K=K, u0=None if K is None else np.ascontiguousarray(u0[b:b + 1]))
            if method == "rk4":
                r = rk.restate(proxy, x, row, t1 - t0, t1 - t0, dt, fi, xcg=xcg, status0=st, **kw)
            else:
                r = _euler(proxy, x, row, t1 - t0, dt, fi, xcg, kw["K"], kw["u0"], st)
            x, st = r["x"], r["raw_status"]
            traj[t0:t1, b] = r["traj"][:, 0]
            sb.append(r["stages"].reshape(-1, 18))
            if K is not None:
                u_last[b] = r["u_last"][0]
        status[b] = st[0]
        stages.append(np.concatenate(sb))
    n = max(len(s) for s in stages)
    stg = np.stack([np.concatenate((s, np.full((n - len(s), 18), np.nan))) for s in stages], 1) if n else np.zeros((0, B, 18))
    return dict(traj=traj, status=ec._nonfinite(status, traj[-1]), u_last=u_last, stages=stg)


# ------------------------------------------------------------------------------------------------ batches and air
def subset(fi, B=None, seed=0):
    """every third aircraft of the lattice of envelope_cases (hifi_lattice / lofi_lattice); with B, the first B of a seeded shuffle
    of the lattice's aircraft whose start lies inside the envelope box (a batch of frozen aircraft would test nothing)"""
    b = ec.hifi_lattice() if fi == 1 else ec.lofi_lattice()
    idx = np.arange(0, b.B, 3)
    if B is not None:
        idx = np.nonzero(np.all((b.x >= ec.X_LB) & (b.x <= ec.X_UB), 1))[0]
        idx = np.random.default_rng(seed + 7000).permutation(idx)[:B]
        assert len(idx) == B
    return ec.Batch(b, x=b.x[idx].copy(), u=b.u[idx].copy(), cell=b.cell[idx].copy(), edge={})


def air(B, seed, wind_max=100.0, gust_max=30.0, rows=1, horizontal=False):
    """seeded wind [B, 3] with magnitudes up to wind_max and gust rows [rows, B, 3] with components up to gust_max / sqrt(3), ft/s"""
    rng = np.random.default_rng(seed + 8000)
    d = rng.normal(size=(B, 3))
    if horizontal:
        d[:, 2] = 0.0
    w = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0, wind_max, (B, 1))
    return w, rng.uniform(-gust_max, gust_max, (rows, B, 3)) / np.sqrt(3.0)


def near_edges_air(batch, x0, traj, stages, wind, gusts, gust_hold):
    """envelope_cases.near_edges on the ground states (the box, 35,000 ft) and on the air triple (the table axes) of the initial
    state, every sample and every stage state; a stage state is given the gust row of the sample's step it belongs to"""
    T, B = traj.shape[:2]
    per = len(stages) // T if T and len(stages) else 0
    pts = [(np.asarray(x0), 0)] + [(traj[t], min(t + 1, T - 1)) for t in range(T)] + [(stages[k], k // per) for k in range(len(stages))]
    X, XA = [], []
    for p, t in pts:
        p = np.where(np.isnan(p), np.asarray(x0), p)
        X.append(p)
        XA.append(np.stack([air_state(p[b], wind[b], gusts[min(t // gust_hold, len(gusts) - 1), b]) for b in range(B)]))
    X, XA = np.stack(X), np.stack(XA)
    return ec.near_edges(batch, X[0], X[1:]) | ec.near_edges(batch, XA[0], XA[1:])


def reconstruction_error(oracle, batch):
    """|twin(zero wind) - oracle.calc_xdot| per aircraft of the batch [B], the largest entry relative to max(1, |xdot|): reference
    against reference (0 where the reference itself is not finite)"""
    z, e = np.zeros(3), np.zeros(batch.B)
    for b in range(batch.B):
        ref = oracle.calc_xdot(batch.x[b], batch.u[b], batch.fi, XCG)
        got, _ = twin_xdot(oracle, batch.x[b], batch.u[b], z, z, batch.fi)
        if np.isfinite(ref).all():
            e[b] = float(ec.rel(got, ref).max())
    return e


_REC = {}


def record(oracle, key, batch, rows, hold, T, dt, method, wind, gusts, gust_hold, K=None, u0=None):
    """rk4_cases.record's rule for a wind flight, once per process and key: the twin, its spread against the one-ulp twins, the
    near-edge set on the air triple, states_ok, status_ok"""
    if key in _REC:
        return _REC[key]
    run = lambda x0: fly(oracle, x0, rows, hold, T, dt, batch.fi, method, wind, gusts, gust_hold, K, u0)
    r = run(batch.x)
    traj, st = r["traj"], r["status"]
    spread, same = np.zeros(batch.B), np.ones(batch.B, dtype=bool)
    for d in (+1, -1):
        r2 = run(ec.ulp(batch.x, d))
        e = ec.rel(r2["traj"], traj)
        bad = np.isnan(e)
        e[bad] = np.where(np.isnan(r2["traj"]) & np.isnan(traj), 0.0, np.inf)[bad]
        spread = np.maximum(spread, e.max((0, 2)))
        same &= r2["status"] == st
    g = np.zeros((1, batch.B, 3)) if gusts is None else gusts
    near = near_edges_air(batch, batch.x, traj, r["stages"], wind, g, gust_hold if gusts is not None else T)
    fin = np.isfinite(traj).all((0, 2))
    _REC[key] = dict(batch=batch, traj=traj, status=st, u_last=r["u_last"], near=near, spread=spread, finite=fin,
                     status_ok=~near & same, states_ok=fin & (~near | (spread < 1e-12)))
    return _REC[key]


def band(base, e_rec):
    """A band of the suite widened by the twin's reconstruction error alone, per aircraft (e_rec [B] -> [B]): the suite's bands admit
    differences that start as single roundings (2^-52 relative) of a derivative and grow along the flight; the twin's derivative
    starts e_rec away from the reference's instead, so the same growth is granted e_rec / 2^-52 times over, on top of the band."""
    return base * (1.0 + np.asarray(e_rec) / EPS)
