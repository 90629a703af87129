"""GPU tests of soft state rows (C-ABI f16_mpc_plan_soft_rows; F16Batch.prepare_MPC / rollout_MPC / _calc_MPC_action(soft=)): the
one-wavefront solver's soft twins k_mpc_wave_soft / k_rollout_mpc_soft<RELIN>.

Checkers: the numpy twin of the soft solve and the exact minimiser of the equivalent slack QP (tests/mpc_soft_cases.py); a hard plan,
bit for bit, wherever nothing is soft or no soft row binds; and for the closed loops their documented host loops -- the softened
f16_mpc_plan_solve + the F16_FLAG_ONE_LANE plant steps -- bit for bit.  Cases W, S, G: tests/mpc_soft_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import mpc_soft_cases as sc
from conftest import golden
from oracle import mpc_oracle as mo

pytestmark = pytest.mark.gpu

EINVAL = -1
N = sc.HZN
SOFT = sc.SOFT_ACTIVE


def make_env(x, u=None, xcg=sc.XCG, **kw):
    from f16_mpc_oop_py_amd import F16Batch
    return F16Batch(x, u, device="cuda:0", xcg=xcg, **kw)


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    b = _np(b) if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _soa(a):
    a = np.asarray(a, dtype=np.float64)
    return torch.as_tensor(a.reshape(a.shape[0], -1).T.copy(), device="cuda:0")


def _soft_rows(env, w9):
    """f16_mpc_plan_soft_rows on env's plan with nine weights (or None: a NULL pointer) -> rc"""
    return env.lib.f16_mpc_plan_soft_rows(env._plan, None if w9 is None else (ctypes.c_double * 9)(*[float(v) for v in w9]))


def _solve(env, dem=sc.DEMANDS, hzn=N):
    u, info = env._calc_MPC_action(*dem, hzn, return_info=True, use_plan=True)
    torch.cuda.synchronize()
    return u, info


def _same_solve(a, b):
    (ua, ia), (ub, ib) = a, b
    return _same(ua, ub) and all(_same(ia[k], ib[k]) for k in ("u_seq", "iters", "r_prim", "r_dual", "rho", "status"))


# ---- 1. the solve against the twin
@pytest.fixture(scope="module")
def case_w():
    """Case W once: the batch, the device's own models, the QPs of the listed aircraft, the hard solve of the whole batch."""
    x0, u0 = sc.batch_w()
    env = make_env(x0, u0)
    Ad, Bd, Cd = (t.t().cpu().numpy() for t in env.build_ssr())
    qps = {b: mo.mpc_qp(x0[b], Ad[b].reshape(9, 9), Bd[b].reshape(9, 3), Cd[b].reshape(9, 9), N, sc.DT, *sc.DEMANDS) for b in sc.W_AIRCRAFT}
    env.prepare_MPC(N)
    u, info = _solve(env)
    return dict(x0=x0, u0=u0, qps=qps, hard_u=_np(u), hard_st=_np(info["status"]))


@pytest.mark.parametrize("w", [100.0, 1e4])
def test_soft_solve_vs_the_twin(case_w, w):
    """prepare_MPC(30, soft=w) + _calc_MPC_action(use_plan=True) on the 192 perturbed aircraft against admm_osqp_soft on the QPs of
    the device's own models: the bands of test_mpc_batch_of_perturbed_aircraft_vs_oracle_chain (iterations within one test interval,
    first move within 1e-4), the status word exactly the twin's."""
    env = make_env(case_w["x0"], case_w["u0"])
    env.build_ssr()
    env.prepare_MPC(N, soft=w)
    u, info = _solve(env)
    u, st, its = _np(u), _np(info["status"]), _np(info["iters"]).astype(int)
    for b in sc.W_AIRCRAFT:
        P, q, A, l, uu = case_w["qps"][b]
        ref = sc.admm_osqp_soft(P, q, A, l, uu, sc.state_row_weights(w, N, A.shape[0]))
        print(f"w={w:g} aircraft {b}: iterations {its[b]} (twin {ref['iters']}), status {st[b]}, |du| {np.abs(u[b] - ref['x'][:3]).max():.3g}")
        assert ref["converged"] and not ref["infeasible"]
        assert abs(its[b] - ref["iters"]) <= 25, (b, its[b], ref["iters"])
        assert np.abs(u[b] - ref["x"][:3]).max() < 1e-4
        assert st[b] == (SOFT if ref["soft_active"] else 0), (b, st[b])
        assert ref["soft_active"] == (b in (26, 29))
    if w == 100.0:
        assert not (st & (128 | 64)).any() and its.max() <= 1000, (np.nonzero(st & 192)[0], its.max())      # (the twin: 800)
    # the contrast: the hard plan of the same batch loses aircraft 26
    assert case_w["hard_st"][26] == 128 and np.isnan(case_w["hard_u"][26]).all() and np.isfinite(u[26]).all()


# ---- 2. the exact minimiser
@pytest.mark.parametrize("w", [1.0, 100.0, 1e4])
def test_soft_solve_reaches_the_exact_minimiser_of_the_slack_qp(w):
    """Case G: the q-rate box moved off the prediction.  Tight tolerances: u_seq within 1e-5 of the slack QP's exact minimiser (the
    bound of the hard solvers' tight-tolerance test); the hard plan on the same weights is certified infeasible."""
    g5 = golden("g567_trim_lin_lqr.npz")
    env = make_env(np.tile(g5["trim_x_xcg35"], (4, 1)))
    env.build_ssr()
    wg = sc.weights_g()
    P, q, A, l, u = env.setup_OSQP(0.0, 0.0, 0.0, N, b=1, weights=wg)
    xs, _ = mo.qp_exact(*sc.slack_qp(P, q, A, l, u, sc.state_row_weights(w, N, A.shape[0])))
    env.prepare_MPC(N, settings=dict(eps_abs=1e-9, eps_rel=1e-9, max_iter=400000), weights=wg, soft=w)
    _, info = _solve(env, dem=(0.0, 0.0, 0.0))
    err = np.abs(_np(info["u_seq"]) - xs[:3 * N]).max()
    print(f"w={w:g}: |u_seq - exact| = {err:.3g} after {int(info['iters'][1])} iterations")
    assert err < 1e-5 and (_np(info["status"]) == SOFT).all()
    env.prepare_MPC(N, weights=wg)
    uh, infoh = _solve(env, dem=(0.0, 0.0, 0.0))
    assert (_np(infoh["status"]) == 128).all() and bool(torch.isnan(uh).all()) and int(infoh["iters"].max()) == 25


# ---- 3. nothing changes when nothing is soft
def test_zero_weights_and_null_leave_the_plan_as_it_was(case_w):
    idx = [0, 17, 26, 101]                                   # (aircraft 26: a soft row binds at weight 100, test_soft_solve_vs_the_twin)
    x0, u0 = case_w["x0"][idx], case_w["u0"][idx]
    env = make_env(x0, u0)
    env.build_ssr()
    env.prepare_MPC(N)
    fresh = _solve(env)
    for w9 in (np.zeros(9), None):
        e = make_env(x0, u0)
        e.build_ssr()
        e.prepare_MPC(N, soft=100.0)
        assert not _same_solve(_solve(e), fresh)             # (the soft plan is another problem for aircraft 26)
        assert _soft_rows(e, w9) == 0
        assert _same_solve(_solve(e), fresh)
    assert int(fresh[1]["iters"].min()) >= 25


@pytest.mark.parametrize("xcg", [25, 35])
def test_soft_rows_that_never_bind_give_the_hard_result(xcg):
    """The trim batch of test_mpc_action_vs_exact_minimiser_and_same_algorithm_oracle: no state row binds there."""
    g5 = golden("g567_trim_lin_lqr.npz")
    out = []
    for soft in (None, 100.0):
        env = make_env(np.tile(g5[f"trim_x_xcg{xcg}"], (4, 1)), xcg=xcg / 100)
        env.ssr = tuple(_soa(np.tile(g5[f"ssr_{k}_xcg{xcg}"], (4, 1, 1))) for k in ("Ad", "Bd", "Cd"))
        env.prepare_MPC(N, soft=soft)
        out.append(_solve(env, dem=(0.0, 0.0, 0.0)))
    assert _same_solve(*out) and int(out[1][1]["status"].max()) == 0 and int(out[1][1]["iters"].min()) >= 25


# ---- 4. the closed loops
def _host_loop(x0, u0, nctrl, hold, dems, soft, warm=False, models=None):
    """The host loop a closed-loop call equals: per control step the softened f16_mpc_plan_solve, the command into u.values, `hold`
    F16_FLAG_ONE_LANE plant steps.  dems: the demand of every control step.  models: model_traj of the re-linearised call -- the solve
    of step t is then a FRESH softened plan on row t.  -> (env, samples of every plant step, cmd, iters)"""
    from f16_mpc_oop_py_amd import lib as L
    env = make_env(x0, u0, flags=L.F16_FLAG_ONE_LANE)
    if models is None:
        env.build_ssr()
        env.prepare_MPC(N, ctrl_every=hold, soft=soft, warm_start=warm)
    cmds, its, trs = [], [], []
    for t in range(nctrl):
        if models is not None:
            m = models[t]
            env.ssr = (m[:81].contiguous(), m[81:108].contiguous(), m[108:].contiguous())
            env.prepare_MPC(N, soft=soft)
        cmd, info = env._calc_MPC_action(*dems[t], N, return_info=True, use_plan=True, ctrl_every=hold)
        cmds.append(cmd.t().clone()); its.append(info["iters"].to(torch.int32).clone())
        env._u[1:4] = cmd.t()
        trs.append(env.rollout(hold, traj_every=1).clone())
    return env, torch.cat(trs), torch.stack(cmds), torch.stack(its)


LOOPS = {"plain": dict(), "hold2": dict(ctrl_every=2), "relin": dict(relinearise=True), "sched": dict(sched=True), "warm": dict(warm=True)}


@pytest.mark.timeout(300, method="thread")      # (a persistent kernel that never drains must fail the run, not hold it)
@pytest.mark.parametrize("loop", list(LOOPS))
def test_soft_closed_loop_equals_its_host_loop(loop):
    """Case S, N = 30, weight 100, three control steps: f16_rollout_mpc, _hold (hold = 2), _relin, _sched (a new demand at every
    control step), and f16_rollout_mpc once more with the plan's warm start on."""
    kw = dict(LOOPS[loop])
    sched, warm, hold = kw.pop("sched", False), kw.pop("warm", False), kw.get("ctrl_every", 1)
    x0, u0 = sc.batch_s()
    nctrl, w = 3, 100.0
    rows = np.array([sc.DEMANDS, (-0.03, 0.02, 0.0), (0.01, 0.04, -0.02)])
    dems = [tuple(rows[t]) if sched else sc.DEMANDS for t in range(nctrl)]
    env = make_env(x0, u0)
    env.build_ssr()
    if warm:
        env.prepare_MPC(N, soft=w, warm_start=True)
        kw["soft"] = None                                    # (a call that does not name it keeps the plan's soft rows)
    else:
        kw["soft"] = w
    dem_args = (rows[:, 0], rows[:, 1], rows[:, 2]) if sched else sc.DEMANDS
    traj, info = env.rollout_MPC(nctrl * hold, *dem_args, N, traj_every=1, return_info=True, **kw, **(dict(dem_every=1) if sched else {}))
    torch.cuda.synchronize()
    st = _np(env.status)
    print(f"{loop}: iterations per step max {_np(info['iters']).max(1).tolist()}, soft-active aircraft {np.nonzero(st & SOFT)[0].tolist()}")
    assert not (st & (128 | 32)).any(), st
    assert (st[[26, 29]] & SOFT).all() and int(info["iters"].min()) >= 25
    models = info["model"] if loop == "relin" else None
    if models is not None:
        assert bool(torch.isfinite(models).all())
    eh, trh, ch, ih = _host_loop(x0, u0, nctrl, hold, dems, w, warm=warm, models=models)
    inside = torch.as_tensor((st & 16) == 0, device="cuda:0")      # (the host loop goes on solving for an aircraft outside its envelope)
    assert _same(traj, trh) and _same(env._x, eh._x) and _same(env.status, eh.status) and _same(traj[-1], env._x)
    assert _same(info["cmd"][:, :, inside], ch[:, :, inside]) and _same(info["iters"][:, inside], ih[:, inside])
    assert _same(env._u[:, inside], eh._u[:, inside]) and int(inside.sum()) >= sc.S_ROWS - 1


@pytest.mark.timeout(300, method="thread")
def test_hard_closed_loop_loses_the_aircraft_the_soft_one_keeps():
    """The contrast, ONE control step (aircraft 29 runs to max_iter in a hard solve): aircraft 26 is certified infeasible, its NaN command
    reaches the actuators."""
    x0, u0 = sc.batch_s()
    env = make_env(x0, u0)
    env.build_ssr()
    env.rollout_MPC(1, *sc.DEMANDS, N)
    torch.cuda.synchronize()
    assert int(env.status[26]) & (128 | 32) == (128 | 32)
    soft = make_env(x0, u0)
    soft.build_ssr()
    soft.rollout_MPC(1, *sc.DEMANDS, N, soft=100.0)
    torch.cuda.synchronize()
    assert int(soft.status[26]) == SOFT and bool(torch.isfinite(soft._x).all())


# ---- 5. argument rules
def test_soft_rows_argument_rules(case_w):
    from f16_mpc_oop_py_amd import lib as L
    x0, u0 = case_w["x0"][:8], case_w["u0"][:8]
    env = make_env(x0, u0)
    env.build_ssr()
    env.prepare_MPC(10)
    ok = np.array([0, 0, 1, 1, 1, 1, 1, 0, 1], dtype=float)
    assert _soft_rows(env, 100 * ok) == 0
    for bad in (-1.0, float("nan"), float("inf")):
        w9 = 100 * ok
        w9[4] = bad
        assert _soft_rows(env, w9) == EINVAL, bad
    for row in (0, 1, 7):                                     # phi, theta, lf1: no bounds to soften
        w9 = 100 * ok
        w9[row] = 1.0
        assert _soft_rows(env, w9) == EINVAL, row
    assert env.lib.f16_mpc_plan_soft_rows(None, None) == EINVAL
    # plans the one-wavefront solver does not serve
    for hzn, settings in ((31, None), (10, dict(scaling=0, rho=0.0))):
        env.prepare_MPC(hzn, settings=settings)
        assert _soft_rows(env, 100 * ok) == EINVAL, (hzn, settings)
        assert _soft_rows(env, np.zeros(9)) == 0 and _soft_rows(env, None) == 0       # (switching off is always possible)
        with pytest.raises(L.F16HipError):
            env.prepare_MPC(hzn, settings=settings, soft=100.0)
    with pytest.raises(ValueError):
        env._calc_MPC_action(*sc.DEMANDS, 10, soft=100.0)    # soft rows are a property of a plan
    with pytest.raises(ValueError):
        env.prepare_MPC(10, soft=[1.0, 2.0])


def test_switching_soft_rows_on_forgets_the_warm_start(case_w):
    x0, u0 = case_w["x0"][:24], case_w["u0"][:24]
    cold = make_env(x0, u0)
    cold.build_ssr()
    cold.prepare_MPC(N, soft=100.0)
    it_cold = _np(_solve(cold)[1]["iters"])
    env = make_env(x0, u0)
    env.build_ssr()
    env.prepare_MPC(N, warm_start=True)
    it1 = _np(_solve(env)[1]["iters"])
    it2 = _np(_solve(env)[1]["iters"])
    assert it2.sum() < it1.sum()                             # the second hard solve did start warm
    assert _soft_rows(env, np.where(sc.BOUNDED, 100.0, 0.0)) == 0
    assert np.array_equal(_np(_solve(env)[1]["iters"]), it_cold)
    assert _np(_solve(env)[1]["iters"]).sum() < it_cold.sum()      # ... and the warm start itself is still on
