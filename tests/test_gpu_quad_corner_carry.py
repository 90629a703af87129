"""The table waves of the four-lane rollout (k_rollout_q<1,*>, B <= 4096) keep the table values of their last full lookup while
every lane of the wave stays in last step's cell, and read the tables again only on a step on which a lane has left its cell.
The smallest shapes at which that can go wrong: one workgroup (B = 16) and the ragged B = 3 and B = 17, 64 steps with every step
stored, aircraft chosen with the C restatement so that EXACTLY ONE of them changes a cell, on one axis, at a known step, and the
others stay in theirs throughout -- one case per axis (alpha, beta, the elevator across a DH1 node: wave 0; the elevator across
0 deg, a node of DH2 as well: wave 1), alpha rising through 45 deg (the end of ALPHA2: hi_a, the clamp of j2, the last ALPHA2
cell), crossings in consecutive steps and a crossing between the first and the second lookup of a launch.  Each case first
asserts on the CPU that the chosen aircraft crosses where it should and nothing else does, then compares the run against the
F16_FLAG_NO_CELL_CACHE run (full lookup, fresh table values on every step) bit for bit on states, status and trajectory, against
the restatement at the suite's 1e-9, and against two launches split at the crossing step.  All four <1,LQR,SCHED> instantiations run
the alpha case at B = 16 through the Python entry points."""
import numpy as np
import pytest

from envelope_cases import ALPHA1, BETA1, DH1, restate_schedule

pytestmark = pytest.mark.gpu
R2D = 180.0 / 3.141592653589793
DH2 = np.array([-25.0, 0.0, 25.0])
GRIDS = (ALPHA1, BETA1, DH1, DH2)
AXIS_OF_GRID = np.array([0, 1, 2, 2])          # alpha, beta, elevator (DH1 and DH2 are two grids on one axis)
T = 64
MARGIN = 1e-6                                   # degrees from a node, so that kernel and restatement agree on the cell
TOL = 1e-9


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(p, q):
    p, q = np.asarray(p), np.asarray(q)
    assert p.shape == q.shape
    return np.array_equal(bits(p), bits(q)) if p.dtype == np.float64 else np.array_equal(p, q)


def make_env(x, u, **kw):
    from f16_mpc_oop_py_amd import F16Batch
    return F16Batch(x, u, device="cuda:0", **kw)


def axis_values(X):
    return np.stack((X[..., 7] * R2D, X[..., 8] * R2D, X[..., 13], X[..., 13]), -1)


def cells(X):
    """[..., 18] states -> [..., 4] cell indices on ALPHA1, BETA1, DH1, DH2, and the distance to the nearest node in degrees"""
    v = axis_values(X)
    c = np.stack([np.searchsorted(g, v[..., k], side="right") - 1 for k, g in enumerate(GRIDS)], -1)
    d = np.stack([np.abs(v[..., k, None] - g).min(-1) for k, g in enumerate(GRIDS)], -1)
    return c, d


def lookups(oracle, x0, u0, steps=T):
    """the states the table waves look up at steps 0 .. steps - 1: x0 and the restated states after steps 1 .. steps - 1"""
    _, traj, st = oracle.rollout(x0, u0, steps, store=True)
    return np.concatenate((np.asarray(x0)[None], traj[:-1])), traj, st


def crossings(oracle, x0, u0, steps=T):
    """[(step, aircraft, axis)] with axis 0 / 1 / 2 = alpha / beta / elevator: the lookup of `step` finds the aircraft in another
    cell than the lookup of step - 1 did; asserts that every looked-up value is MARGIN away from every node"""
    X, traj, st = lookups(oracle, x0, u0, steps)
    c, d = cells(X)
    assert d.min() > MARGIN and np.isfinite(traj).all()
    ch = c[1:] != c[:-1]                                             # [steps - 1, B, 4]
    out = set()
    for t, b, g in zip(*np.nonzero(ch)):
        out.add((int(t) + 1, int(b), int(AXIS_OF_GRID[g])))
    return sorted(out), c, traj, st


_POOL = {}


def calm_pool(oracle):
    """config-2 aircraft that stay in their cells on all four grids for T steps, below 40 deg of alpha"""
    if "p" not in _POOL:
        from f16_mpc_oop_py_amd.workload import config2_states
        x0, u0 = config2_states(512, seed=20261019)
        X, traj, st = lookups(oracle, x0, u0)
        c, d = cells(X)
        ok = (c == c[0]).all((0, 2)) & (d.min((0, 2)) > 0.05) & np.isfinite(traj).all((0, 2)) & (st == 0) & (X[..., 7].max(0) * R2D < 40)
        assert ok.sum() >= 32
        _POOL["p"] = (x0[ok], u0[ok])
    return _POOL["p"]


def crosser(kind, x, u):
    """candidates (a few, the first that does what the case asks is taken) for the one aircraft of a case: (x [18], u [4])"""
    for gap in (0.2, 0.1, 0.3, 0.05):
        for rate in (0.6, -0.6, 0.3, -0.3, 1.5, -1.5):
            y, v = x.copy(), u.copy()
            if kind in ("alpha", "alpha45"):
                if kind == "alpha45" and rate < 0:
                    continue                                          # rising through 45 deg
                above = np.searchsorted(ALPHA1, y[7] * R2D)
                node = 45.0 if kind == "alpha45" else ALPHA1[above if rate > 0 else above - 1]
                y[7] = (node - np.sign(rate) * gap) / R2D
                y[10] = rate
            elif kind == "beta":
                node = BETA1[np.searchsorted(BETA1, y[8] * R2D)]
                y[8] = (node - gap) / R2D
                y[11] = rate
            elif kind in ("el_dh1", "el_dh2_zero"):
                node = 0.0 if kind == "el_dh2_zero" else -10.0
                y[13] = node - np.sign(rate) * gap * 1.5
                v[1] = node + np.sign(rate) * 6.0                     # rate-limited: 60 deg/s = 0.06 deg per step
            yield y, v


def single_case(oracle, kind, B):
    """(x0, u0, step, aircraft): B calm aircraft, aircraft 1 replaced by one that crosses a node of `kind`'s axis once"""
    px, pu = calm_pool(oracle)
    who, want = 1, {"alpha": 0, "alpha45": 0, "beta": 1, "el_dh1": 2, "el_dh2_zero": 2}[kind]
    for y, v in crosser(kind, px[who], pu[who]):
        x0, u0 = px[:B].copy(), pu[:B].copy()
        x0[who], u0[who] = y, v
        try:
            cr, c, _, st = crossings(oracle, x0, u0)
        except AssertionError:
            continue
        quiet = not st.any() if kind != "alpha45" else st[who] == 2 and not np.delete(st, who).any()    # (above 45 deg: ST_ALPHA2)
        if len(cr) == 1 and cr[0][1:] == (who, want) and 2 <= cr[0][0] < T - 2 and quiet:
            return x0, u0, cr[0][0], who
    raise AssertionError(f"no candidate crosses one {kind} node alone")


def run(x0, u0, steps, flags=0):
    env = make_env(x0, u0, flags=flags)
    tr = env.rollout(steps, traj_every=1).cpu().numpy()
    return env.x_values.cpu().numpy(), env.status.cpu().numpy(), tr


def run_split(x0, u0, first, steps):
    env = make_env(x0, u0)
    a = env.rollout(first, traj_every=1).cpu().numpy()
    b = env.rollout(steps - first, traj_every=1).cpu().numpy()
    return env.x_values.cpu().numpy(), env.status.cpu().numpy(), np.concatenate((a, b))


def rel(a, b):
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def compare(oracle, x0, u0, split):
    from f16_mpc_oop_py_amd import lib as L
    xr, trr, str_ = oracle.rollout(x0, u0, T, store=True)
    on = run(x0, u0, T)
    off = run(x0, u0, T, flags=L.F16_FLAG_NO_CELL_CACHE)
    for name, p, q in zip(("states", "status", "trajectory"), on, off):
        assert same(p, q), f"cell re-use changes the {name}"
    parts = run_split(x0, u0, split, T)
    for name, p, q in zip(("states", "status", "trajectory"), on, parts):
        assert same(p, q), f"two launches split at step {split} differ from one in the {name}"
    x, st, tr = on
    assert same(tr[-1], x.T)
    e = rel(tr.transpose(0, 2, 1), trr)
    print(f"B = {len(x0)}: max relative distance to the restatement over {T} steps {e:.2e}")
    assert e < TOL
    assert np.array_equal(st, str_)


@pytest.mark.parametrize("B", [16, 3, 17])
@pytest.mark.parametrize("kind", ["alpha", "beta", "el_dh1", "el_dh2_zero", "alpha45"])
def test_one_aircraft_crosses_one_node(oracle, kind, B):
    x0, u0, step, who = single_case(oracle, kind, B)
    cr, c, _, _ = crossings(oracle, x0, u0)
    assert cr == [(step, who, {"alpha": 0, "alpha45": 0, "beta": 1}.get(kind, 2))]           # this aircraft, this axis, once
    others = np.arange(B) != who
    assert (c[:, others] == c[0, others]).all()                                                # the others stay put
    if kind == "alpha45":
        assert c[step - 1, who, 0] == 12 and c[step, who, 0] == 13                             # ALPHA1 cell 40..45 -> 45..50: hi_a
    if kind == "el_dh2_zero":
        assert c[step - 1, who, 3] != c[step, who, 3] and c[step - 1, who, 2] != c[step, who, 2]   # a node of DH1 and of DH2
    if kind == "el_dh1":
        assert (c[:, who, 3] == c[0, who, 3]).all()                                           # no DH2 node: wave 1 keeps its values
    compare(oracle, x0, u0, step)


def consecutive_case(oracle, B):
    """aircraft 1 crosses an alpha node at step t, aircraft 2 (aircraft 0 at B = 3 has no room: then aircraft 1 itself) an elevator
    node of DH1 at step t + 1"""
    x0, u0, t, who = single_case(oracle, "alpha", B)
    other = 2 if B > 3 else who
    for k in range(-3, 4):
        y0, v0 = x0.copy(), u0.copy()
        y0[other, 13] = -10.0 - 0.06 * (t + 0.5 + 0.25 * k)           # 0.06 deg per step at the rate limit
        v0[other, 1] = -4.0
        try:
            cr, _, _, _ = crossings(oracle, y0, v0)
        except AssertionError:
            continue
        if cr == [(t, who, 0), (t + 1, other, 2)]:
            return y0, v0, t
    raise AssertionError("no elevator start crosses -10 deg one step behind the alpha crossing")


@pytest.mark.parametrize("B", [16, 3, 17])
def test_crossings_in_consecutive_steps(oracle, B):
    x0, u0, t = consecutive_case(oracle, B)
    cr, _, _, _ = crossings(oracle, x0, u0)
    assert [c[0] for c in cr] == [t, t + 1] and cr[0][2] == 0 and cr[1][2] == 2
    compare(oracle, x0, u0, t)
    compare_split_only(x0, u0, t + 1)


def compare_split_only(x0, u0, split):
    on, parts = run(x0, u0, T), run_split(x0, u0, split, T)
    for name, p, q in zip(("states", "status", "trajectory"), on, parts):
        assert same(p, q), f"two launches split at step {split} differ from one in the {name}"


def first_step_case(oracle, B):
    """the state the launch starts from lies one step in front of the node: the values kept at step 0 are stale at step 1"""
    x0, u0, t, who = single_case(oracle, "alpha", B)
    X, _, _ = lookups(oracle, x0, u0)
    y0 = x0.copy()
    y0[who] = X[t - 1, who]                                           # the crosser alone moves on; the others are calm from any start
    return y0, u0, who


@pytest.mark.parametrize("B", [16, 3, 17])
def test_crossing_between_the_first_two_lookups_of_a_launch(oracle, B):
    x0, u0, who = first_step_case(oracle, B)
    cr, _, _, _ = crossings(oracle, x0, u0)
    assert cr == [(1, who, 0)]
    compare(oracle, x0, u0, 1)


# ---------------------------------------------------------------------------------------- the four <1, LQR, SCHED> instantiations
def gpu_crossings(tr, x0):
    """cell changes between consecutive lookups, from a stored trajectory [T, 18, B] of the full-lookup run"""
    X = np.concatenate((np.asarray(x0)[None], tr.transpose(0, 2, 1)[:-1]))
    c, _ = cells(X)
    return int((c[1:] != c[:-1]).any(-1).sum())


@pytest.mark.parametrize("variant", ["plain", "lqr", "sched", "lqr_sched"])
def test_every_one_group_instantiation(oracle, variant):
    from f16_mpc_oop_py_amd import lib as L
    B, hold = 16, 7
    x0, u0, step, who = single_case(oracle, "alpha", B)
    rng = np.random.default_rng(5)
    rows = u0[None] + rng.uniform(-1.0, 1.0, ((T + hold - 1) // hold, B, 4)) * np.array([500.0, 2.0, 2.0, 2.0])
    dem = rng.uniform(-0.15, 0.15, ((T + hold - 1) // hold, B, 3))
    px, pu = calm_pool(oracle)
    K = make_env(px[:B], pu[:B])._calc_LQR_gain() if "lqr" in variant else None      # (the gain is an input here: the calm aircraft's)

    def launch(flags):
        env = make_env(x0, u0, flags=flags)
        if variant == "plain":
            tr = env.rollout(T, traj_every=1)
        elif variant == "lqr":
            tr = env.rollout_LQR(T, dem[0, :, 0], dem[0, :, 1], dem[0, :, 2], K=K, traj_every=1)
        elif variant == "sched":
            tr = env.rollout_schedule(rows, hold=hold, nsteps=T, traj_every=1)
        else:
            tr = env.rollout_LQR(T, dem[:, :, 0], dem[:, :, 1], dem[:, :, 2], K=K, traj_every=1, hold=hold)
        return env.x_values.cpu().numpy(), env.status.cpu().numpy(), tr.cpu().numpy(), env.u_values.cpu().numpy()

    on, off = launch(0), launch(L.F16_FLAG_NO_CELL_CACHE)
    for name, p, q in zip(("states", "status", "trajectory", "last action"), on, off):
        assert same(p, q), f"{variant}: cell re-use changes the {name}"
    assert gpu_crossings(off[2], x0) >= 1                              # a lookup on which the kept values are stale does occur
    assert np.isfinite(on[2]).all()
    # against the restatement of the same loop (the scheduled LQR loop: the chain of restated LQR launches, one per demand row)
    if variant == "plain":
        ref = oracle.rollout(x0, u0, T, store=True)[1]
    elif variant == "lqr":
        ref = oracle.rollout_lqr(x0, u0, K.cpu().numpy(), dem[0], T, store=True)[1]
    elif variant == "sched":
        ref = restate_schedule(oracle, x0, rows, T, hold, 0.001, 1)[0]
    else:
        x, parts = x0, []
        for r in range((T + hold - 1) // hold):
            x, tr, _, _ = oracle.rollout_lqr(x, u0, K.cpu().numpy(), dem[r], min(hold, T - r * hold), store=True)
            parts.append(tr)
        ref = np.concatenate(parts)
    e = rel(on[2].transpose(0, 2, 1), ref)
    print(f"{variant}: max relative distance to the restatement over {T} steps {e:.2e}")
    assert e < TOL
