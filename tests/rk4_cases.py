"""The Runge-Kutta rollouts (include/f16_hip.h: F16_INT_RK4) restated in numpy from what the checker exports, and the cases
tests/test_rk4_cpu.py and tests/test_gpu_rollout_rk4.py run on the whole-envelope batches of tests/envelope_cases.py.

The step rule, in exactly this operation order (f = oracle.calc_xdot, the command u of the step held over the four stages; under
the LQR law u is the action of env.py:360-371 formed from the state at the start of the step):

    if the box test of env.py:117-124 (f16o_envelope_bits) fails on x: freeze, F16_ST_ENVELOPE | the state bits, x untouched
    k1 = f(x, u);  k2 = f(x + (dt/2) k1, u);  k3 = f(x + (dt/2) k2, u);  k4 = f(x + dt k3, u)
    x <- x + (dt/6) ((k1 + 2 k2) + (2 k3 + k4))

The grid bits of all four evaluations (oracle.lib.f16o_last_status) are ORed into the status word; stage states are not box-tested.
restate() returns the trajectory, the status words (F16_ST_NONFINITE formed from the final state) and the three stage states of
every step; record() adds what envelope_cases.reference adds -- the spread against the one-ulp twins, the near-edge set (over the
trajectory AND the stage states: a stage state beside a table edge can flip a grid bit as well), states_ok and status_ok."""
import numpy as np

import envelope_cases as ec
from envelope_cases import (XCG, SCHED_HOLD, ST_ENVELOPE, _nonfinite, hifi_lattice, high_rate, lofi_lattice, lqr_demands, lqr_gain,  # noqa: F401
                            near_edges, rel, schedule_rows, score_weights, ulp)

LQR_HOLD = 3


def restate(oracle, x0, rows, T, hold, dt, fi, xcg=XCG, noenv=False, K=None, u0=None, status0=None):
    """x0 [B, 18]; rows [S, B, 4] the command rows, step t takes row t // hold -- or, with K ([3, 9] or [B, 3, 9]) and u0 [B, 4],
    rows [S, B, 3] the (p, q, r) demands of the LQR law around the offset u0.
    -> dict(traj [T, B, 18], status [B], stages [T, 3, B, 18] (NaN where an aircraft took no step), u_last [B, 4], x [B, 18])"""
    x = np.array(x0, dtype=np.float64)
    B = len(x)
    rows = np.asarray(rows, dtype=np.float64)
    st = np.zeros(B, dtype=np.int32) if status0 is None else np.array(status0, dtype=np.int32)
    traj, stages = np.zeros((T, B, 18)), np.full((T, 3, B, 18), np.nan)
    lqr = K is not None
    if lqr:
        K = np.broadcast_to(np.asarray(K, dtype=np.float64), (B, 3, 9))
        u0 = np.ascontiguousarray(u0, dtype=np.float64)
    u_last = np.array(u0 if lqr else rows[0], dtype=np.float64)
    h2, h6 = dt / 2, dt / 6

    def f(X, U, live):
        out = np.zeros_like(X)
        for b in live:
            out[b] = oracle.calc_xdot(X[b], U[b], fi, xcg)
            st[b] |= oracle.lib.f16o_last_status()
        return out

    for t in range(T):
        r = rows[t // hold]
        if lqr and t % hold == 0:
            u_last = u0.copy()                                                   # (as a new launch: u0 until the aircraft steps)
        if not noenv:
            for b in np.nonzero(~(st & ST_ENVELOPE).astype(bool))[0]:
                st[b] |= oracle.lib.f16o_envelope_bits(oracle._p(x[b]))
        live = np.nonzero(~(st & ST_ENVELOPE).astype(bool))[0]
        if lqr:                                                                  # f16o_rollout_lqr's order: s += -K[i][j] (xr[j] - x9[j])
            u = u0.copy()
            e = r - x[:, 9:12]
            for i in range(3):
                u[:, 1 + i] = (((-K[:, i, 4]) * e[:, 0] + (-K[:, i, 5]) * e[:, 1]) + (-K[:, i, 6]) * e[:, 2]) + u0[:, 1 + i]
            u_last[live] = u[live]
        else:
            u = r
        with np.errstate(invalid="ignore", over="ignore"):
            k1 = f(x, u, live)
            xa = x + h2 * k1
            k2 = f(xa, u, live)
            xb = x + h2 * k2
            k3 = f(xb, u, live)
            xc = x + dt * k3
            k4 = f(xc, u, live)
            xn = x + h6 * ((k1 + 2.0 * k2) + (2.0 * k3 + k4))
        x[live] = xn[live]
        for j, s in enumerate((xa, xb, xc)):
            stages[t, j, live] = s[live]
        traj[t] = x
    return dict(traj=traj, status=_nonfinite(st, x), raw_status=st, stages=stages, u_last=u_last if lqr else None, x=x)


def restate_euler(oracle, x0, rows, T, hold, dt, fi, xcg=XCG):
    """the restated Euler step of the suite (envelope_cases.restate_schedule) -> (traj [T, B, 18], status [B])"""
    return ec.restate_schedule(oracle, x0, rows, T, hold, dt, fi, xcg)


# ------------------------------------------------------------------------------------------------ the cases
def _case(batch, dt, T, rate=False, kind="open", every=1):
    return dict(batch=batch, dt=dt, T=T, rate=rate, kind=kind, every=every, noenv=False)


# (b) of the issue: the lattice at 10 ms, the high-rate lattice at 1 ms (16 steps: the restatement is a Python loop), lofi at 10 ms;
# then what the GPU tests add: a schedule (hold 7 over 40 steps at 1 ms -- at 10 ms the restatement's own spread over 40 steps
# reaches 1e-6 -- on every third aircraft of the lattice, 473 of them) and the LQR loop with constant and with scheduled demands
CASES = {
    "hifi_dt10": _case("hifi", 0.01, 8), "hifi_rate": _case("hifi", 0.001, 16, rate=True), "lofi_dt10": _case("lofi", 0.01, 8),
    "hifi_sched40": _case("hifi", 0.001, 40, kind="sched", every=3),
    "hifi_lqr": _case("hifi", 0.01, 8, kind="lqr"), "hifi_lqr_sched": _case("hifi", 0.01, 8, kind="lqr_sched"),
    "lofi_lqr": _case("lofi", 0.01, 8, kind="lqr"),
}
LATTICE_CASES = ("hifi_dt10", "hifi_rate", "lofi_dt10")


def case_batch(name):
    c = CASES[name]
    b = hifi_lattice() if c["batch"] == "hifi" else lofi_lattice()
    if c["rate"]:
        b = high_rate(b)
    if c["every"] > 1:
        b = ec.Batch(b, x=b.x[::c["every"]].copy(), u=b.u[::c["every"]].copy(), cell=b.cell[::c["every"]].copy(), edge={})
    return b


def case_inputs(name):
    """(batch, rows, hold, K, u0): rows [S, B, 4] commands, or with K [3, 9] the demand rows [S, B, 3] around the offset u0"""
    c, b = CASES[name], case_batch(name)
    T = c["T"]
    if c["kind"] == "open":
        return b, b.u[None].copy(), T, None, None
    if c["kind"] == "sched":
        return b, schedule_rows(b, T), SCHED_HOLD, None, None
    if c["kind"] == "lqr":
        return b, lqr_demands(b)[None].copy(), T, lqr_gain(), b.u
    S = (T + LQR_HOLD - 1) // LQR_HOLD
    dem = np.random.default_rng(ec.SEED + 5000).uniform(-0.15, 0.15, (S, b.B, 3))
    return b, dem, LQR_HOLD, lqr_gain(), b.u


def run_case(oracle, name, x0):
    c = CASES[name]
    b, rows, hold, K, u0 = case_inputs(name)
    return restate(oracle, x0, rows, c["T"], hold, c["dt"], b.fi, K=K, u0=u0)


_REC = {}


def record(oracle, name):
    """envelope_cases.reference for CASES[name] under the Runge-Kutta step, once per process: dict(batch, x0, traj, status, stages,
    u_last, near, spread, finite, twins_status_equal, status_ok, states_ok)"""
    if name in _REC:
        return _REC[name]
    batch = case_batch(name)
    r = run_case(oracle, name, batch.x)
    traj, st = r["traj"], r["status"]
    spread, same = np.zeros(batch.B), np.ones(batch.B, dtype=bool)
    for d in (+1, -1):
        r2 = run_case(oracle, name, ulp(batch.x, d))
        e = rel(r2["traj"], traj)
        bad = np.isnan(e)
        e[bad] = np.where(np.isnan(r2["traj"]) & np.isnan(traj), 0.0, np.inf)[bad]
        spread = np.maximum(spread, e.max((0, 2)))
        same &= r2["status"] == st
    T = len(traj)
    stages = r["stages"].reshape(3 * T, batch.B, 18)
    stages = np.where(np.isnan(stages), np.broadcast_to(batch.x, stages.shape), stages)      # (no step taken: nothing evaluated there)
    near = near_edges(batch, batch.x, np.concatenate((traj, stages)))
    fin = np.isfinite(traj).all((0, 2))
    _REC[name] = dict(CASES[name], batch=batch, x0=batch.x, traj=traj, status=st, stages=r["stages"], u_last=r["u_last"], near=near,
                      spread=spread, finite=fin, twins_status_equal=same, status_ok=~near & same,
                      states_ok=fin & (~near | (spread < 1e-12)))
    return _REC[name]
