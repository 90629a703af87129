"""The whole-envelope batches of tests/test_envelope_cpu.py and tests/test_gpu_envelope.py, defined once, and the restated
reference every comparison of those two modules uses.

hifi_lattice(seed): one aircraft per (ALPHA1 cell, BETA1 cell, DH1 cell) = 19 x 18 x 4 = 1368, alpha / beta / elevator drawn inside
the cell, everything else over the ranges of fixtures G2 / G3 widened to the whole grid, commands over ranges in which every
actuator rate limit and position limit acts in both directions; then a block of edge rows (values exactly on a node, on the first
and last node of an axis, one ulp beside a node, -0.0, the 35,000 ft temperature branch and sixteen aircraft that climb through it,
rows off each grid axis, rows outside the envelope box).  lofi_lattice(seed): the same over the lofi model's own cells
(oracle/f16_oracle.c: lofi_alpha, lofi_dmomdcon, lofi_cxcm -- alpha -10..45 in 5 deg, |beta| 0..30 in 5 deg, elevator -24..24 in
12 deg), both signs of beta.  high_rate(batch): the same aircraft with P, Q, R in +-8 rad/s, so that the angle increments of a 1 ms
step straddle the 4e-3 rad above which the carried sin / cos pairs fall back to an exact evaluation.

CASES lists the (batch, dt, steps) combinations the GPU tests run; reference(oracle, name) restates one of them with the C
restatement alone: states after every step, status words, the ulp-perturbed twins and the near-edge set."""
import ctypes
import functools

import numpy as np

R2D = 180.0 / 3.141592653589793
ALPHA1 = np.array([-20, -15, -10, -5, 0, 5, 10, 15, 20, 25, 30, 35, 40, 45, 50, 55, 60, 70, 80, 90.])
BETA1 = np.array([-30, -25, -20, -15, -10, -8, -6, -4, -2, 0, 2, 4, 6, 8, 10, 15, 20, 25, 30.])
DH1 = np.array([-25, -10, 0, 10, 25.])
ALPHA2_END = 45.0
LOFI_ALPHA = np.arange(-10.0, 50.0, 5.0)            # 12 nodes (lofi_alpha: k = fix(0.2 alpha) in -1..8, one neighbour)
LOFI_BETA = np.arange(-30.0, 35.0, 5.0)             # |beta| in 5 deg rows 0..30 (lofi_dmomdcon, lofi_clcn), both signs
LOFI_EL = np.array([-24.0, -12.0, 0.0, 12.0, 24.0])  # lofi_cxcm: dele / 12 in -2..2
SEED = 1

X_LB = np.array([-np.inf, -np.inf, 0, -np.inf, -np.inf, -np.inf, 0, -20., -30., -300, -100, -50, 1000, -25, -21.5, -30., 0., -np.inf])
X_UB = np.array([np.inf, np.inf, 100000, np.inf, np.inf, np.inf, 900, 90, 30, 300, 100, 50, 19000, 25, 21.5, 30, 25, np.inf])
ST_ENVELOPE, ST_NONFINITE = 16, 32


def on_value(deg):
    """A state in radians whose conversion to degrees in the kernels and in the restatement (x * (180 / pi)) is `deg` bit for bit
    (the search of test_gpu_rollout_cell_cache.py::on_node, for any target double)."""
    if deg == 0.0:
        return deg                                   # +0.0 and -0.0 survive the product
    v = deg / R2D
    for _ in range(64):
        if v * R2D == deg:
            return v
        v = np.nextafter(v, np.inf if v * R2D < deg else -np.inf)
    raise AssertionError(deg)


def beside(deg):
    """The two neighbouring doubles (radians) whose conversions to degrees straddle `deg` where no double converts to it exactly
    (+-30: the product by 180 / pi steps over it): (the one at or inside |deg|, the one beyond)."""
    v = deg / R2D
    while abs(v * R2D) > abs(deg):
        v = np.nextafter(v, 0.0)
    while abs(np.nextafter(v, np.sign(v) * np.inf) * R2D) <= abs(deg):
        v = np.nextafter(v, np.sign(v) * np.inf)
    return v, np.nextafter(v, np.sign(v) * np.inf)


def _draw(rng, n):
    """n aircraft over the wide ranges; alpha, beta and the elevator are filled in by the caller"""
    x = np.zeros((n, 18))
    x[:, 0:2] = rng.uniform(-1e3, 1e3, (n, 2))
    x[:, 2] = rng.uniform(1000, 60000, n)
    x[:, 3] = rng.uniform(-3, 3, n)
    x[:, 4] = rng.uniform(-1.4, 1.4, n)
    x[:, 5] = rng.uniform(-3, 3, n)
    x[:, 6] = rng.uniform(300, 880, n)
    x[:, 9:12] = rng.uniform(-1.5, 1.5, (n, 3))
    x[:, 12] = rng.uniform(1500, 18000, n)
    x[:, 14] = rng.uniform(-21, 21, n)
    x[:, 15] = rng.uniform(-29, 29, n)
    x[:, 16] = rng.uniform(0.5, 24.5, n)
    x[:, 17] = rng.uniform(-20, 5, n)
    u = rng.uniform([0, -30, -25, -35], [20000, 30, 25, 35], (n, 4))
    return x, u


def _cells(rng, axes):
    """one row per cell of the product grid: (values [n, 3] drawn uniformly inside the cell, cell indices [n, 3])"""
    idx = np.stack(np.meshgrid(*[np.arange(len(a) - 1) for a in axes], indexing="ij"), -1).reshape(-1, 3)
    lo = np.stack([a[idx[:, k]] for k, a in enumerate(axes)], 1)
    hi = np.stack([a[idx[:, k] + 1] for k, a in enumerate(axes)], 1)
    f = rng.uniform(0.02, 0.98, lo.shape)            # strictly inside: the nodes have rows of their own
    return lo + f * (hi - lo), idx


class Batch(dict):
    """x [B, 18], u [B, 4], cell [B, 3] (-1 on edge rows), n_lattice, edge {name: row}, axes, fi"""
    __getattr__ = dict.__getitem__

    @property
    def B(self):
        return len(self["x"])


def _finish(x, u, cell, rows, axes, fi, rng):
    """append the edge rows: each is a mid-envelope aircraft (rates +-0.2 rad/s, commands = actuator positions, so that it stays
    where it was put unless the row says otherwise) with the fields of `rows[name]` (state index -> value; 100 + k: command k)"""
    ex, eu = _draw(rng, len(rows))
    ex[:, 2] = rng.uniform(5000, 30000, len(rows))
    ex[:, 3:6] = rng.uniform(-0.3, 0.3, (len(rows), 3))
    ex[:, 7] = np.deg2rad(rng.uniform(1, 4, len(rows)))
    ex[:, 8] = np.deg2rad(rng.uniform(0.5, 1.5, len(rows)))
    ex[:, 9:12] = rng.uniform(-0.2, 0.2, (len(rows), 3))
    ex[:, 13] = rng.uniform(-4, -1, len(rows))
    eu = ex[:, 12:16].copy()
    edge = {}
    for j, (name, fields) in enumerate(rows.items()):
        for k, v in fields.items():
            if k >= 100:
                eu[j, k - 100] = v
            else:
                ex[j, k] = v
        edge[name] = len(x) + j
    n_lat = len(x)
    return Batch(x=np.concatenate((x, ex)), u=np.concatenate((u, eu)), cell=np.concatenate((cell, np.full((len(rows), 3), -1))),
                 n_lattice=n_lat, edge=edge, axes=axes, fi=fi)


@functools.lru_cache(maxsize=None)
def hifi_lattice(seed=SEED):
    rng = np.random.default_rng(seed)
    axes = (ALPHA1, BETA1, DH1)
    v, cell = _cells(rng, axes)
    x, u = _draw(rng, len(v))
    x[:, 7], x[:, 8], x[:, 13] = v[:, 0] / R2D, v[:, 1] / R2D, v[:, 2]
    A, Bt, E = 7, 8, 13
    up, dn = (lambda d: np.nextafter(d, np.inf)), (lambda d: np.nextafter(d, -np.inf))
    rows = {
        "alpha_node": {A: on_value(10.0)}, "beta_node": {Bt: on_value(-4.0)}, "el_node": {E: 10.0},
        "el_node_held": {E: -10.0, 101: -10.0},
        "all_nodes": {A: on_value(25.0), Bt: on_value(8.0), E: 0.0, 101: 0.0},
        "alpha_first": {A: on_value(-20.0)}, "alpha_last": {A: on_value(90.0)}, "alpha2_last": {A: on_value(ALPHA2_END)},
        "beta_first": {Bt: beside(-30.0)[0]}, "beta_first_out": {Bt: beside(-30.0)[1]},       # (no double converts to +-30 exactly)
        "beta_last": {Bt: beside(30.0)[0]}, "beta_last_out": {Bt: beside(30.0)[1]},
        "el_first": {E: -25.0, 101: -30.0}, "el_last": {E: 25.0, 101: 30.0},
        "alpha_node_up": {A: on_value(up(20.0))}, "alpha_node_dn": {A: on_value(dn(20.0))},
        "beta_node_up": {Bt: on_value(up(6.0))}, "beta_node_dn": {Bt: on_value(dn(6.0))},
        "el_node_up": {E: up(10.0)}, "el_node_dn": {E: dn(10.0)},
        "beta_neg_zero": {Bt: -0.0}, "el_neg_zero": {E: -0.0, 101: -0.0},
        "alt_35000": {2: 35000.0}, "alt_below_35000": {2: np.nextafter(35000.0, 0.0)},
        # off each grid axis (test_offgrid_is_clamped_and_flagged_and_envelope_freezes), inside the envelope box unless it says so
        "off_alpha1_hi": {A: np.deg2rad(95.0)}, "off_alpha1_lo": {A: np.deg2rad(-23.0)}, "off_alpha2": {A: np.deg2rad(47.5)},
        "off_beta_hi": {Bt: np.deg2rad(35.0)}, "off_beta_lo": {Bt: np.deg2rad(-34.0)},
        "off_el_hi": {E: 26.0}, "off_el_lo": {E: -25.5},                       # (outside the box as well: frozen at once)
        "out_alt_rudder": {2: -10.0, 15: 31.0}, "out_thrust": {12: 500.0},
        # leaves the box on the way: a dive at full thrust from just below 900 ft/s, frozen after a few steps
        "vt_leaves": {2: 50000.0, 3: 0.0, 4: -1.3, 6: 899.7, A: 0.03, Bt: 0.0, 9: 0.0, 10: 0.0, 11: 0.0, 12: 18000.0, 100: 19000.0},
    }
    # a 16-aircraft group in a steep climb from just below 35,000 ft: 850 ft/s at 72 degrees is ~0.8 ft per 1 ms step
    for j in range(16):
        rows[f"climb_{j}"] = {2: 35000.0 - rng.uniform(0, 20), 3: 0.0, 4: 1.3, 6: 850.0, A: 0.04, Bt: 0.0, 9: 0.0, 10: 0.0, 11: 0.0}
    return _finish(x, u, cell, rows, axes, 1, rng)


@functools.lru_cache(maxsize=None)
def lofi_lattice(seed=SEED):
    rng = np.random.default_rng(seed + 1000)
    axes = (LOFI_ALPHA, LOFI_BETA, LOFI_EL)
    v, cell = _cells(rng, axes)
    x, u = _draw(rng, len(v))
    x[:, 7], x[:, 8], x[:, 13] = v[:, 0] / R2D, v[:, 1] / R2D, v[:, 2]
    A, Bt, E = 7, 8, 13
    rows = {
        "alpha_node": {A: on_value(10.0)}, "alpha_zero": {A: 0.0}, "beta_node": {Bt: on_value(-10.0)}, "el_node": {E: 12.0, 101: 12.0},
        "all_nodes": {A: on_value(25.0), Bt: on_value(5.0), E: 0.0, 101: 0.0},
        "alpha_first": {A: on_value(-10.0)}, "alpha_last": {A: on_value(45.0)},
        "beta_first": {Bt: beside(-30.0)[0]}, "beta_first_out": {Bt: beside(-30.0)[1]},
        "beta_last": {Bt: beside(30.0)[0]}, "beta_last_out": {Bt: beside(30.0)[1]},
        "el_first": {E: -24.0, 101: -24.0}, "el_last": {E: 24.0, 101: 24.0}, "el_box": {E: 25.0, 101: 30.0},
        "beta_neg_zero": {Bt: -0.0}, "el_neg_zero": {E: -0.0, 101: -0.0},
        "alt_35000": {2: 35000.0}, "alt_below_35000": {2: np.nextafter(35000.0, 0.0)},
        "off_alpha_hi": {A: np.deg2rad(60.0)}, "off_alpha_lo": {A: np.deg2rad(-17.0)},
        "off_beta_hi": {Bt: np.deg2rad(33.0)}, "off_beta_lo": {Bt: np.deg2rad(-36.0)},
        "out_alt_rudder": {2: -10.0, 15: 31.0}, "out_thrust": {12: 500.0},
        # leaves the box on the way: a dive at full thrust from just below 900 ft/s, frozen after a few steps
        "vt_leaves": {2: 50000.0, 3: 0.0, 4: -1.3, 6: 899.7, A: 0.03, Bt: 0.0, 9: 0.0, 10: 0.0, 11: 0.0, 12: 18000.0, 100: 19000.0},
    }
    for j in range(16):
        rows[f"climb_{j}"] = {2: 35000.0 - rng.uniform(0, 20), 3: 0.0, 4: 1.3, 6: 850.0, A: 0.04, Bt: 0.0, 9: 0.0, 10: 0.0, 11: 0.0}
    return _finish(x, u, cell, rows, axes, 0, rng)


def high_rate(batch, seed=SEED):
    """the same aircraft with body rates in +-8 rad/s (legal input: the envelope box compares radians with degree limits).
    One other change, forced by the conditioning check: theta is scaled from +-1.4 into +-0.9 rad.  At these rates theta moves up
    to 0.45 rad in 40 steps, and an aircraft that passes +-pi/2 (tan theta and 1 / cos theta in the Euler kinematics) is
    ill-conditioned whatever computes it: with theta left alone the restatement differs from its own ulp-perturbed twin by up
    to 5.7e-11 on the hifi lattice (four aircraft with min |cos theta| < 3e-3) and 1.1e-12 on the lofi one."""
    x = batch.x.copy()
    x[:, 9:12] = np.random.default_rng(seed + 2000).uniform(-8, 8, (len(x), 3))
    x[:, 4] *= 0.9 / 1.4
    return Batch(batch, x=x)


# the deliberate rows that sit on the first / last node of an axis, on the box or on the temperature branch: a one-ulp
# difference may flip a status bit or the branch there, whatever the seed
ON_EDGE = ("alpha_first", "alpha_last", "alpha2_last", "beta_first", "beta_last", "beta_first_out", "beta_last_out", "el_first", "el_last", "el_box", "alt_35000",
           "alt_below_35000")


def axis_values(batch, x=None):
    """(alpha, beta, elevator) in the units of the table axes, as the plant forms them"""
    x = batch.x if x is None else x
    return np.stack((x[..., 7] * R2D, x[..., 8] * R2D, x[..., 13]), -1)


def cell_of(batch, x=None):
    """cell index per axis from the BREAKPOINTS (searchsorted): -1 below the first node, len - 1 above the last"""
    v = axis_values(batch, x)
    return np.stack([np.searchsorted(a, v[..., k], side="right") - 1 - (v[..., k] == a[-1]) for k, a in enumerate(batch.axes)], -1)


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
XCG = 0.25
SCHED_HOLD = 7


def _case(batch, dt=0.001, T=40, rate=False, noenv=False, kind="open"):
    return dict(batch=batch, dt=dt, T=T, rate=rate, noenv=noenv, kind=kind)


CASES = {}
for _b in ("hifi", "lofi"):
    CASES.update({
        _b + "40": _case(_b), _b + "100": _case(_b, T=100), _b + "_rate40": _case(_b, rate=True),
        _b + "_dt10": _case(_b, dt=0.01, T=8),                  # (8 steps: at 40 the restatement's own spread reaches 1e-6)
        _b + "_noenv40": _case(_b, noenv=True), _b + "_sched40": _case(_b, kind="sched"), _b + "_lqr40": _case(_b, kind="lqr")})


def case_batch(name):
    c = CASES[name]
    b = hifi_lattice() if c["batch"] == "hifi" else lofi_lattice()
    return high_rate(b) if c["rate"] else b


def schedule_rows(batch, T=40, seed=SEED):
    """[ceil(T / 7), B, 4] command rows over the full command ranges"""
    S = (T + SCHED_HOLD - 1) // SCHED_HOLD
    return np.random.default_rng(seed + 3000).uniform([0, -30, -25, -35], [20000, 30, 25, 35], (S, batch.B, 4))


def lqr_demands(batch, seed=SEED):
    return np.random.default_rng(seed + 4000).uniform(-0.15, 0.15, (batch.B, 3))


def lqr_gain():
    """the gain fixture G12 carries (the reference's own K = -dlqr at its trim point, xcg 0.25), [3, 9]"""
    from conftest import golden
    return np.ascontiguousarray(golden("g12_lqr_loop.npz")["K_xcg25"], dtype=np.float64).reshape(3, 9)


def score_weights(seed=5):
    """seeded positive cost weights, all different (q [9], qf [9], r [3], pen), for score_schedules on the lattice"""
    import types
    v = np.random.default_rng(seed).uniform(0.5, 2.0, 21)
    return types.SimpleNamespace(q=v[:9], qf=v[9:18], r=v[18:21], pen=2.0)


def ulp(x, direction):
    return np.nextafter(x, np.inf if direction > 0 else -np.inf)


def _nonfinite(st, x):
    st = np.asarray(st).copy()
    st[~np.isfinite(x).all(1)] |= ST_NONFINITE               # formed from the final state, as the kernels form it
    return st


def restate(oracle, x0, u0, T, dt, fi, noenv=False, xcg=XCG):
    """the restatement's rollout: (traj [T, B, 18], status [B]).  noenv: F16_FLAG_NO_ENVELOPE = the same Euler step
    (oracle/f16_oracle.c: f16o_step) without the box test."""
    if not noenv:
        x, traj, st = oracle.rollout(x0, u0, T, dt=dt, fi_flag=fi, xcg=xcg, store=True, nthreads=8)
        return traj, _nonfinite(st, x)
    x = np.array(x0, dtype=np.float64)
    traj, st = np.zeros((T, len(x), 18)), np.zeros(len(x), dtype=np.int32)
    for b in range(len(x)):
        for t in range(T):
            xd = oracle.calc_xdot(x[b], u0[b], fi, xcg)
            st[b] |= oracle.lib.f16o_last_status()
            x[b] += xd * dt
            traj[t, b] = x[b]
    return traj, _nonfinite(st, x)


def restate_schedule(oracle, x0, rows, T, hold, dt, fi, xcg=XCG):
    """the chain of constant-input rollouts a schedule stands for (tests/test_gpu_rollout_sched.py), the status carried along"""
    x, st, out = np.array(x0, dtype=np.float64), np.zeros(len(x0), dtype=np.int32), []
    P, ip = oracle._p, ctypes.POINTER(ctypes.c_int)
    for s in range((T + hold - 1) // hold):
        n = min(hold, T - s * hold)
        traj = np.zeros((n, len(x), 18))
        oracle.lib.f16o_rollout(P(x), P(np.ascontiguousarray(rows[s])), len(x), n, dt, fi, xcg, P(traj), st.ctypes.data_as(ip), 8)
        out.append(traj)
    return np.concatenate(out), _nonfinite(st, x)


def near_edges(batch, x0, traj):
    """aircraft whose restated trajectory (the initial state included) comes within 1e-6 deg of the first / last node of a table
    axis (hifi: alpha -20 / 45 / 90, beta +-30, elevator +-25; lofi: |beta| = 30, the one place its lookup raises a bit), within
    1e-6 relative of a side of the envelope box a state can reach, or within 1e-4 ft of 35,000 ft"""
    X = np.concatenate((np.asarray(x0)[None], traj))
    v = axis_values(batch, X)
    near = np.zeros(X.shape[1], dtype=bool)
    edges = [(v[..., 1], (-30.0, 30.0)), (v[..., 2], (-25.0, 25.0))]
    if batch.fi == 1:
        edges.append((v[..., 0], (-20.0, ALPHA2_END, 90.0)))
    with np.errstate(invalid="ignore"):
        for val, es in edges:
            for e in es:
                near |= (np.abs(val - e) < 1e-6).any(0)
        near |= (np.abs(X[..., 2] - 35000.0) < 1e-4).any(0)
        for k in (2, 6, 12, 14, 15, 16):                       # altitude, speed, thrust, aileron, rudder, flap against their box
            for lim in (X_LB[k], X_UB[k]):
                near |= (np.abs(X[..., k] - lim) < 1e-6 * max(1.0, abs(lim))).any(0)
    return near


def rel(a, b):
    with np.errstate(invalid="ignore"):
        return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def case_inputs(name):
    """(batch, u [B, 4] the constant command or the LQR offset, rows [S, B, 4] or None, K [3, 9] or None, dem [B, 3] or None)"""
    c, b = CASES[name], case_batch(name)
    if c["kind"] == "sched":
        return b, b.u, schedule_rows(b, c["T"]), None, None
    if c["kind"] == "lqr":
        return b, b.u, None, lqr_gain(), lqr_demands(b)
    return b, b.u, None, None, None


def run_case(oracle, name, x0):
    """the restatement of CASES[name] from x0 -> (traj [T, B, 18], status [B], u_last [B, 4] or None)"""
    c = CASES[name]
    b, u, rows, K, dem = case_inputs(name)
    if c["kind"] == "sched":
        return restate_schedule(oracle, x0, rows, c["T"], SCHED_HOLD, c["dt"], b.fi) + (None,)
    if c["kind"] == "lqr":
        x, traj, ul, st = oracle.rollout_lqr(x0, u, K, dem, c["T"], dt=c["dt"], fi_flag=b.fi, xcg=XCG, store=True, nthreads=8)
        return traj, _nonfinite(st, x), ul
    return restate(oracle, x0, u, c["T"], c["dt"], b.fi, c["noenv"]) + (None,)


_REF = {}


def reference(oracle, name):
    """dict(batch, x0, traj [T, B, 18], status [B], u_last, near [B], spread [B], finite [B], states_ok [B], status_ok [B]) of
    CASES[name], from the restatement alone and computed once per process:
      spread     the largest relative distance, over all steps, between the restatement on x0 and on x0 with every entry moved
                 one ulp up / one ulp down (infinite where exactly one of the two is not finite);
      near       near_edges();
      status_ok  aircraft whose status word is compared: not near an edge, and the twins' status words equal its own;
      states_ok  aircraft whose states are compared: finite, and either not near an edge or with both twins within 1e-12 (the rule
                 for the deliberate on-edge rows)."""
    if name in _REF:
        return _REF[name]
    batch = case_batch(name)
    traj, st, ul = run_case(oracle, name, batch.x)
    spread, same = np.zeros(batch.B), np.ones(batch.B, dtype=bool)
    for d in (+1, -1):
        t2, s2, _ = run_case(oracle, name, ulp(batch.x, d))
        e = rel(t2, traj)
        bad = np.isnan(e)
        e[bad] = np.where(np.isnan(t2) & np.isnan(traj), 0.0, np.inf)[bad]
        spread = np.maximum(spread, e.max((0, 2)))
        same &= s2 == st
    near = near_edges(batch, batch.x, traj)
    fin = np.isfinite(traj).all((0, 2))
    _REF[name] = dict(CASES[name], batch=batch, x0=batch.x, traj=traj, status=st, u_last=ul, near=near, spread=spread, finite=fin,
                      twins_status_equal=same, status_ok=~near & same, states_ok=fin & (~near | (spread < 1e-12)))
    return _REF[name]
