"""f16_trim_man_batch (csrc/f16_trim.hip: k_trim_man) -- the trim in a climb, a coordinated turn or a pull-up -- through the public C ABI
and F16Batch.trim / from_trim: the cost at the returned point, scipy's Nelder-Mead STEP BY STEP over the first N_LOCK iterations in six
dimensions, the runs, the launch geometry, full trims and the manoeuvre held by the plant (tests/trim_man_cases.py has the restated
cost, the cases, the cost band and the measured spread; tests/test_trim_man_cpu.py shows on the CPU what they rest on).

The shape is that of tests/test_gpu_trim_lockstep.py: every call goes with ld = B + 3 into arrays pre-filled with NaN / a sentinel, the
padding must come back untouched, a foreign status bit must survive, and after a launch that failed no further launch is made."""
import ctypes

import numpy as np
import pytest
import torch

import trim_cases as tc
import trim_man_cases as tm

pytestmark = pytest.mark.gpu

EPS = tc.EPS
PAD = 3
SENT = -777
FOREIGN = 1 << 30
QP_MAXITER = 64                         # F16_ST_QP_MAXITER
NONFINITE = 32                          # F16_ST_NONFINITE
NS = list(range(1, tm.N_LOCK + 1))
IQ = tm.IDX_Q
_STATE = dict(failed=None)
_RUNS = {}
_FULL = {}


@pytest.fixture(scope="module")
def ctx():
    from f16_mpc_oop_py_amd import lib
    assert lib.F16_ST["QP_MAXITER"] == QP_MAXITER and lib.F16_ST["NONFINITE"] == NONFINITE
    c = lib.Context(0)
    yield c
    c.close()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def launch(ctx, q0, fi, xcg, conds, maxiter, runs=1, optional=True, null_givens=False, expect=0):
    """one f16_trim_man_batch call, ld = B + 3, status pre-set to FOREIGN -> dict(x [B, 18], cost, iters, nfev, status [B]).  q0: None
    (NULL), one start [6] for every condition, or [B, 6].  null_givens: gamma, psi_dot and theta_dot go as NULL (they must be zero)."""
    from f16_mpc_oop_py_amd import lib
    if _STATE["failed"]:
        pytest.fail("no launch after a failed one: " + _STATE["failed"])
    B, dev = len(conds), "cuda:0"
    ld = B + PAD
    col = lambda k: torch.as_tensor(np.array([c[k] for c in conds], dtype=np.float64), device=dev)
    hd, vd, gd, pd, td = (col(k) for k in range(5))
    if null_givens:
        assert not gd.any() and not pd.any() and not td.any()
        gd = pd = td = None
    qd = None
    if q0 is not None:
        qd = torch.full((6, ld), np.nan, dtype=torch.float64, device=dev)
        qd[:, :B] = torch.as_tensor(np.array(np.broadcast_to(np.asarray(q0, dtype=np.float64), (B, 6)).T, order="C"), device=dev)
    xt = torch.full((19, ld), np.nan, dtype=torch.float64, device=dev)
    cost = torch.full((ld,), np.nan, dtype=torch.float64, device=dev) if optional else None
    iters, nfev, st = (torch.full((ld,), SENT, dtype=torch.int32, device=dev) if optional else None for _ in range(3))
    if optional:
        st[:B] = FOREIGN
    try:
        rc = ctx.lib.f16_trim_man_batch(ctx.handle, _vp(hd), _vp(vd), _vp(gd), _vp(pd), _vp(td), _vp(qd), _vp(xt), _vp(cost), _vp(iters),
                                        _vp(nfev), _vp(st), B, ld, float(xcg), int(fi), 0, int(maxiter), int(runs), None)
        if expect:
            assert rc == expect
            return None
        lib.check(rc, ctx.lib)
        torch.cuda.synchronize()
    except Exception as e:
        _STATE["failed"] = repr(e)
        raise
    x = xt.cpu().numpy()
    assert np.isnan(x[:18, B:]).all() and np.isnan(x[18]).all(), "x_trim: padding columns or the row beyond were written"
    out = dict(x=x[:18, :B].T.copy())
    if optional:
        c, it, nf, s = cost.cpu().numpy(), iters.cpu().numpy(), nfev.cpu().numpy(), st.cpu().numpy()
        assert np.isnan(c[B:]).all() and (it[B:] == SENT).all() and (nf[B:] == SENT).all() and (s[B:] == SENT).all(), "entries beyond B written"
        assert np.all(s[:B] & FOREIGN), "status is OR-ed into: a bit set before the call survives it"
        out.update(cost=c[:B], iters=it[:B], nfev=nf[:B], status=s[:B] & ~FOREIGN)
    return out


def runs_of(ctx, g):
    """the group's launches for n = 1 .. N_LOCK iterations (runs = 1), once per process: [n - 1] = launch(maxiter = n + 1)"""
    if g not in _RUNS:
        grp = tm.CASES[g]
        _RUNS[g] = [launch(ctx, grp.x0, grp.fi, grp.xcg, grp.conds, n + 1) for n in NS]
    return _RUNS[g]


def full(ctx):
    """the full trims (runs = 2, the reference start through q0 = NULL, hifi, xcg 0.25), once per process"""
    if "full" not in _FULL:
        _FULL["full"] = launch(ctx, None, 1, 0.25, tm.FULL, 0, runs=2)
    return _FULL["full"]


def _same(a, b, idx=slice(None)):
    return all(np.array_equal(a[k], b[k][idx], equal_nan=True) for k in ("x", "cost", "iters", "nfev", "status"))


GROUPS = [pytest.param(g, id=grp.name) for g, grp in enumerate(tm.CASES)]


def check_point(oracle, x, cost, cond, fi, xcg, where):
    """the device's cost is the restated cost at the q read back from x_trim, within that point's band; x[3], x[4], x[9:12] are the
    restated constraints; the rest of x_trim follows the rule -> (cost error in bands, constraint error in allowances)"""
    q = x[IQ]
    assert np.isfinite(x).all() and np.isfinite(cost), where
    c = tm.cost(oracle, q, cond, fi, xcg)
    assert abs(cost - c.cost) <= c.band, (where, cost, c.cost, c.band)
    con, allow = tm.constraint_allowance(q, cond)
    dcon = np.abs(x[[3, 4, 9, 10, 11]] - con)
    assert np.all(dcon <= allow), (where, dcon, allow)
    ref, terms = tc.x_trim_of(q[:5], cond.h, cond.v)
    assert x[2] == cond.h and x[6] == cond.v and np.all(x[[0, 1, 5]] == 0.0), where
    assert abs(x[17] - ref[17]) <= 2 * EPS * abs(ref[17]), where
    assert abs(x[16] - ref[16]) <= 16 * EPS * sum(abs(t) for t in terms), (where, x[16], ref[16])
    return abs(cost - c.cost) / c.band if c.band > 0 else 0.0, float((dcon / allow).max())


# ------------------------------------------------------------------------------------------------ 1. the cost
@pytest.mark.parametrize("g", GROUPS)
def test_cost_and_constraints_at_the_returned_point(ctx, oracle, g):
    grp, worst = tm.CASES[g], np.zeros(2)
    for n, r in zip(NS, runs_of(ctx, g)):
        for b, cond in enumerate(grp.conds):
            worst = np.maximum(worst, check_point(oracle, r["x"][b], r["cost"][b], cond, grp.fi, grp.xcg, (grp.name, n, b)))
    print(f"trim in a manoeuvre {grp.name}: device cost vs restatement at the returned point, largest error {worst[0]:.3g} of its band; "
          f"constraints {worst[1]:.3g} of their allowance")


# ------------------------------------------------------------------------------------------------ 2. lockstep
@pytest.mark.parametrize("g", GROUPS)
def test_lockstep_with_scipy(ctx, oracle, g):
    """After n iterations, n = 1 .. N_LOCK, runs = 1: iters = n + 1, nfev and the F16_ST_QP_MAXITER bit as scipy has them, the nfev
    increments 1 / 2 / 8 those of the restated branch, the best vertex within the yardstick's allowance, its cost within the band.  A
    failure names the first n at which a condition departs and the branch the restatement took there."""
    grp, rs = tm.CASES[g], runs_of(ctx, g)
    departed, worst_v, worst_c = [], 0.0, 0.0
    for b, cond in enumerate(grp.conds):
        rec = tm.path(oracle, g, b)
        yard, scale = tc.vertex_yardstick(rec, grp.x0)
        prev = 7
        for n, r in zip(NS, rs):
            what = []
            best = r["x"][b][IQ]
            allow = tc.vertex_allowance(yard[n], scale)
            dv = np.abs(best - rec[n]["sim"][0])
            dc = abs(r["cost"][b] - rec[n]["fsim"][0]) / rec[n]["band"][0]
            if r["iters"][b] != n + 1:
                what.append(f"iters {r['iters'][b]} != {n + 1}")
            if r["nfev"][b] != rec[n]["nfev"]:
                what.append(f"nfev {r['nfev'][b]} != {rec[n]['nfev']}")
            if r["nfev"][b] - prev != tm.NFEV_OF[rec[n]["branch"]]:
                what.append(f"nfev increment {r['nfev'][b] - prev} != {tm.NFEV_OF[rec[n]['branch']]}")
            if not r["status"][b] & QP_MAXITER:
                what.append("F16_ST_QP_MAXITER not set (scipy: status 2)")
            if not np.all(dv <= allow):
                what.append(f"best vertex off by {dv} (allowed {allow})")
            if not dc <= 1.0:
                what.append(f"cost off by {dc:.3g} bands")
            if what:
                departed.append(f"{grp.name}[{b}] {tuple(cond)}: first departs at n = {n}, restated branch {rec[n]['branch']}: " + "; ".join(what))
                break
            prev = r["nfev"][b]
            worst_v, worst_c = max(worst_v, float((dv / allow).max())), max(worst_c, dc)
    print(f"trim in a manoeuvre lockstep {grp.name}: best vertex vs restatement, largest error {worst_v:.3g} of its allowance "
          f"(max(16 yardstick, 64 eps scale)); cost {worst_c:.3g} of its band")
    assert not departed, "\n".join(departed)


def test_a_launch_capped_before_its_first_iteration(ctx, oracle):
    """maxiter = 1: scipy's loop does not run -- the sorted initial simplex, nit = 1, nfev = 7, status 2"""
    for g in (0, next(k for k, grp in enumerate(tm.CASES) if grp.name == "all_clipped_lofi")):
        grp = tm.CASES[g]
        r = launch(ctx, grp.x0, grp.fi, grp.xcg, grp.conds, 1)
        for b in range(len(grp.conds)):
            rec = tm.path(oracle, g, b)[0]
            assert r["iters"][b] == 1 and r["nfev"][b] == 7 and r["status"][b] & QP_MAXITER
            assert np.array_equal(r["x"][b][IQ], rec["sim"][0])


# ------------------------------------------------------------------------------------------------ 3. runs
def _chain_equals_two_runs(ctx, q0, fi, xcg, conds, maxiter):
    two = launch(ctx, q0, fi, xcg, conds, maxiter, runs=2)
    first = launch(ctx, q0, fi, xcg, conds, maxiter, runs=1)
    second = launch(ctx, first["x"][:, IQ], fi, xcg, conds, maxiter, runs=1)
    assert np.array_equal(two["x"], second["x"]) and np.array_equal(two["cost"], second["cost"])
    assert np.array_equal(two["iters"], first["iters"] + second["iters"]) and np.array_equal(two["nfev"], first["nfev"] + second["nfev"])
    assert np.array_equal(two["status"], first["status"] | second["status"])
    return two, first, second


def test_two_runs_equal_the_chain_of_single_runs_at_a_small_cap(ctx):
    for g in (0, 4):
        grp = tm.CASES[g]
        two, first, second = _chain_equals_two_runs(ctx, grp.x0, grp.fi, grp.xcg, grp.conds, 9)
        assert np.all(two["iters"] == 18) and np.all(two["status"] & QP_MAXITER)


def test_two_full_runs_equal_the_chain_of_single_runs(ctx):
    two, first, second = _chain_equals_two_runs(ctx, None, 1, 0.25, tm.FULL + tm.UNTRIMMABLE, 0)
    assert _same(full(ctx), two, slice(0, len(tm.FULL)))
    n = len(tm.FULL)
    print("trim in a manoeuvre, device: cost after one run", first["cost"][:n], "after two", two["cost"][:n], "iters", first["iters"][:n],
          second["iters"][:n])
    assert np.all(first["cost"][:n] > 1e-8), "one run stalls"


# ------------------------------------------------------------------------------------------------ 4. geometry
GEO_G, GEO_N = 0, 8                     # a hifi group (the workgroup stages the table image in LDS once, then strides)


@pytest.mark.parametrize("B", [1, 3, 5, 67, 16384 + 24])
def test_every_aircraft_of_a_tiled_batch_equals_its_case_bit_for_bit(ctx, B):
    grp = tm.CASES[GEO_G]
    small = runs_of(ctx, GEO_G)[GEO_N - 1]
    idx = np.arange(B) % len(grp.conds)
    big = launch(ctx, grp.x0, grp.fi, grp.xcg, [grp.conds[i] for i in idx], GEO_N + 1)
    assert _same(big, small, idx)


def test_null_q0_is_the_reference_start_and_null_optional_outputs_work(ctx):
    grp = tm.CASES[GEO_G]
    assert grp.x0 == tm.X0_REF
    small = runs_of(ctx, GEO_G)[GEO_N - 1]
    assert _same(launch(ctx, None, grp.fi, grp.xcg, grp.conds, GEO_N + 1), small)
    r = launch(ctx, None, grp.fi, grp.xcg, grp.conds, GEO_N + 1, optional=False)
    assert np.array_equal(r["x"], small["x"])


def test_null_givens_equal_arrays_of_zeros(ctx):
    conds = [tm.Cond(c.h, c.v, 0.0, 0.0, 0.0) for c in tm.CASES[GEO_G].conds]
    a = launch(ctx, None, 1, 0.25, conds, GEO_N + 1)
    b = launch(ctx, None, 1, 0.25, conds, GEO_N + 1, null_givens=True)
    assert _same(a, b)


def test_runs_below_one_is_einval(ctx):
    from f16_mpc_oop_py_amd import cabi
    grp = tm.CASES[GEO_G]
    for runs in (0, -1):
        launch(ctx, None, grp.fi, grp.xcg, grp.conds, 5, runs=runs, expect=cabi.constants()["F16_EINVAL"])


def test_conditions_that_are_not_iterated(ctx):
    """gamma not finite or |gamma| >= pi / 2, psi_dot or theta_dot not finite, constraints not finite at the start point: x_trim and cost
    NaN, iters 0, F16_ST_NONFINITE and nothing else -- and the other conditions of the launch (they share wavefronts) are what they
    are without them"""
    grp = tm.CASES[GEO_G]
    good = list(grp.conds)
    c0 = good[0]
    bad = [c0._replace(gamma=np.nan), c0._replace(gamma=np.pi / 2), c0._replace(gamma=-2.0), c0._replace(psi_dot=np.inf),
           c0._replace(theta_dot=np.nan), c0._replace(gamma=70 * tm.DEG, psi_dot=0.0)]
    q0 = np.tile(np.array(tm.X0_REF), (len(bad), 1))
    q0[-1, 5] = 0.6                                              # sin(gamma) / cos(beta) > 1 at the clipped beta, no turn: phi = atan(0 x NaN)
    assert not np.isfinite(tm.state_of(q0[-1], bad[-1])).all()
    order = [0, 5, 1, 6, 2, 7, 8, 3, 9, 4, 10]                  # good 0 .. 4, bad 5 .. 10, interleaved
    conds, starts = good + bad, np.vstack([np.tile(np.array(tm.X0_REF), (len(good), 1)), q0])
    r = launch(ctx, starts[order], grp.fi, grp.xcg, [conds[i] for i in order], GEO_N + 1, runs=2)
    ref = launch(ctx, None, grp.fi, grp.xcg, good, GEO_N + 1, runs=2)
    for pos, i in enumerate(order):
        if i < len(good):
            assert all(np.array_equal(r[k][pos], ref[k][i]) for k in ("x", "cost", "iters", "nfev", "status")), i
        else:
            assert np.isnan(r["x"][pos]).all() and np.isnan(r["cost"][pos]), i
            assert r["iters"][pos] == 0 and r["nfev"][pos] == 0 and r["status"][pos] == NONFINITE, i


# ------------------------------------------------------------------------------------------------ 5. full trims
def test_full_trims_converge_in_two_runs(ctx, oracle):
    r = full(ctx)
    print("trim in a manoeuvre, device, two runs: cost", r["cost"], "iters", r["iters"], "nfev", r["nfev"])
    for b, cond in enumerate(tm.FULL):
        check_point(oracle, r["x"][b], r["cost"][b], cond, 1, 0.25, tm.FULL_NAMES[b])
    assert np.all(r["status"] == 0)
    assert np.all(r["cost"] <= 1e-20), r["cost"]
    assert np.all((r["x"][:, 12] > 1000) & (r["x"][:, 12] < 19000))


def test_the_level_condition_ends_below_the_level_trim(ctx):
    from f16_mpc_oop_py_amd import F16Batch
    k = tm.FULL_NAMES.index("level")
    cond = tm.FULL[k]
    assert cond.gamma == 0 and cond.psi_dot == 0 and cond.theta_dot == 0
    _, info = F16Batch.trim([cond.h], [cond.v], xcg=0.25, fi_flag=1, context=ctx)
    assert full(ctx)["cost"][k] < float(info["cost"][0])


def test_full_trims_agree_with_scipy_on_the_oracle(ctx, oracle):
    """the unknowns against scipy's two-run point on the oracle, within 50 x the spread of seeded CPU runs under 1e-14 relative plant
    noise (tm.SPREAD; the method of tests/test_gpu_trim.py)"""
    r, worst = full(ctx), np.zeros(6)
    for b, cond in enumerate(tm.FULL):
        ref = tm.scipy_runs(oracle, cond)[1]
        d = np.abs(r["x"][b][IQ] - ref.x)
        worst = np.maximum(worst, d / tm.SPREAD)
        print(f"trim in a manoeuvre {tm.FULL_NAMES[b]}: device vs scipy on the oracle {d} (spread {tm.SPREAD})")
    assert np.all(worst <= 50.0), worst


def test_untrimmable_conditions(ctx):
    r = launch(ctx, None, 1, 0.25, tm.UNTRIMMABLE, 0, runs=2)
    print("trim in a manoeuvre, untrimmable: cost", r["cost"], "thrust unknown", r["x"][:, 12], "status", r["status"], "iters", r["iters"])
    assert np.all(r["cost"] > 1e-3)
    assert np.all((r["x"][:, 12] < 1000) | (r["x"][:, 12] > 19000))
    assert np.all((r["status"] & ~QP_MAXITER) == 0) and np.all((r["status"] == 0) | (r["iters"] > 50000))     # the cap bit needs a capped run


# ------------------------------------------------------------------------------------------------ 6. hold the manoeuvre
def test_the_plant_holds_the_level_turns():
    """F16Batch.from_trim(h, v, turn_rate=...) then 2,000 Euler steps of 1 ms with constant input: V, alpha, beta, phi, theta, p, q, r
    move by <= 1e-6 (ft/s, rad, rad/s), psi advances by turn rate x 2 s to 1e-6 rad, h moves by <= 1e-2 ft.  (Cost <= 1e-20 bounds
    every residual rate by sqrt(1e-20 / 2) = 7e-11 /s, 1.4e-10 over 2 s; the airframe's modes are no faster than |lambda| ~ 4 /s; the
    h bar is V x 1e-6 rad x 2 s ~ 1.4e-3 ft with margin; a stalled single-run point drifts 1e-4 .. 1e-2.)"""
    from f16_mpc_oop_py_amd import F16Batch
    conds = [c for c in tm.FULL if c.gamma == 0 and c.theta_dot == 0 and c.psi_dot != 0] + [tm._c(10000, 700, 0, 2)]
    assert len(conds) >= 3 and {np.sign(c.psi_dot) for c in conds} == {-1.0, 1.0}
    env = F16Batch.from_trim([c.h for c in conds], [c.v for c in conds], turn_rate=[c.psi_dot for c in conds], xcg=0.25, fi_flag=1, dt=0.001)
    assert np.all(env.trim_info["cost"].cpu().numpy() <= 1e-20) and int(env.trim_info["status"].max()) == 0
    x0 = env.x_values.cpu().numpy().copy()
    x0[:, IQ[:5]] = np.clip(x0[:, IQ[:5]], [1000, -25, -21.5, -30, -20 * tm.DEG], [19000, 25, 21.5, 30, 90 * tm.DEG])
    assert np.array_equal(x0, env.x_values.cpu().numpy()), "a trimmable condition's unknowns are inside their clips: x_trim is the plant state"
    env.rollout(2000)
    d = env.x_values.cpu().numpy() - x0
    assert int(env.status.max()) == 0
    psi = d[:, 5] - np.array([c.psi_dot for c in conds]) * 2.0
    print("trim in a manoeuvre, 2 s of level turn: max |d(V, alpha, beta, phi, theta, p, q, r)|", np.abs(d[:, [6, 7, 8, 3, 4, 9, 10, 11]]).max(0),
          "psi error", psi, "dh", d[:, 2])
    assert np.abs(d[:, [6, 7, 8, 3, 4, 9, 10, 11]]).max() <= 1e-6
    assert np.abs(psi).max() <= 1e-6 and np.abs(d[:, 2]).max() <= 1e-2


# ------------------------------------------------------------------------------------------------ 7. the Python surface
def test_trim_without_a_manoeuvre_is_the_level_trim_bit_for_bit(ctx):
    from f16_mpc_oop_py_amd import F16Batch, lib
    grp = tc.CASES[0]
    B = len(grp.h)
    for n in (1, 9):
        x, info = F16Batch.trim(grp.h, grp.v, xcg=grp.xcg, fi_flag=grp.fi, maxiter=n, context=ctx)
        dev = "cuda:0"
        hd, vd = (torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev) for a in (grp.h, grp.v))
        xt = torch.full((18, B), np.nan, dtype=torch.float64, device=dev)
        cost = torch.full((B,), np.nan, dtype=torch.float64, device=dev)
        iters, nfev, st = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
        lib.check(ctx.lib.f16_trim_batch(ctx.handle, _vp(hd), _vp(vd), _vp(xt), _vp(cost), _vp(iters), _vp(nfev), _vp(st), B, B, float(grp.xcg),
                                         int(grp.fi), 0, n, None, None), ctx.lib)
        torch.cuda.synchronize()
        assert torch.equal(x, xt.t()) and torch.equal(info["cost"], cost)
        assert torch.equal(info["iters"], iters) and torch.equal(info["nfev"], nfev) and torch.equal(info["status"], st)


def test_trim_with_a_manoeuvre_is_the_c_call(ctx):
    from f16_mpc_oop_py_amd import F16Batch
    grp = tm.CASES[1]
    cs = grp.conds
    for kw, conds, runs, q0 in ((dict(gamma=[c.gamma for c in cs], turn_rate=[c.psi_dot for c in cs], pullup_rate=[c.theta_dot for c in cs]), cs, 2, None),
                                (dict(turn_rate=3 * tm.DEG), [tm.Cond(c.h, c.v, 0.0, 3 * tm.DEG, 0.0) for c in cs], 1, grp.x0),
                                (dict(gamma=0.0), [tm.Cond(c.h, c.v, 0.0, 0.0, 0.0) for c in cs], 2, None)):
        x, info = F16Batch.trim([c.h for c in cs], [c.v for c in cs], runs=runs, q0=q0, xcg=grp.xcg, fi_flag=grp.fi, maxiter=GEO_N + 1,
                                context=ctx, **kw)
        c = launch(ctx, q0, grp.fi, grp.xcg, conds, GEO_N + 1, runs=runs)
        assert np.array_equal(x.cpu().numpy(), c["x"])
        for k in ("cost", "iters", "nfev", "status"):
            assert np.array_equal(info[k].cpu().numpy(), c[k]), k


def test_a_gain_schedule_about_a_turn():
    """GainSchedule.build passes the manoeuvre through from_trim: a 2 x 2 table about a 3 deg/s level turn has good nodes, and it is not
    the table about level flight (the trim surface commands of a turn differ)"""
    from f16_mpc_oop_py_amd.schedule import GainSchedule
    turn = GainSchedule.build(10000.0, 5000.0, 2, 600.0, 100.0, 2, xcg=0.25, strict=False, turn_rate=3 * tm.DEG)
    level = GainSchedule.build(10000.0, 5000.0, 2, 600.0, 100.0, 2, xcg=0.25, strict=False)
    assert turn.ok.all() and level.ok.all() and np.isfinite(turn.table).all()
    assert np.all(np.abs(turn.table[:, :, 9:] - level.table[:, :, 9:]).max(axis=2) > 1e-3)
