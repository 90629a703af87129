"""GPU tests of the quad rollout (k_rollout_q, B <= 4096) with a step loop per role wave: the four loops must execute the same
barriers on every trip, the extra trip that only publishes and stores the last sample included, each role must report its own
envelope flag and read the others', and every template variant (LQR law, command schedule, demand schedule) must still be the loop
it was.  Yardsticks: the C restatement at rel < 1e-9 as in test_random_batches_vs_oracle, status words exactly; the CPU twins
and tolerances of the existing tests of each entry point (test_gpu_dynamics.py, test_gpu_rollout_sched.py, test_gpu_rollout_cost.py)."""
import numpy as np
import pytest

import test_gpu_rollout_cost as tc
from test_gpu_rollout_sched import Dev, bits, doublet_rows, lqr_gain, make_env, rel, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip):
    return Dev()


_ref = {}


def restated(oracle, n):
    """config-2 states for 33 aircraft and the restatement's n steps from them, every step kept: computed once per n"""
    from f16_mpc_oop_py_amd.workload import config2_states
    if "x0" not in _ref:
        _ref["x0"], _ref["u0"] = config2_states(33, seed=33)
    if n not in _ref:
        _ref[n] = oracle.rollout(_ref["x0"], _ref["u0"], n, store=True)
    return (_ref["x0"], _ref["u0"]) + tuple(_ref[n])


# ------------------------------------------------------------------------------------------------ extra trip, barrier parity
# B: one lane-quad; one full workgroup; a ragged second workgroup; three workgroups
@pytest.mark.parametrize("every", ["1", "nsteps", "none"])
@pytest.mark.parametrize("nsteps", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 16, 17, 33])
def test_extra_trip_and_barrier_parity(oracle, B, nsteps, every):
    x0, u0, xr, trj, st = restated(oracle, nsteps)
    e = {"1": 1, "nsteps": nsteps, "none": None}[every]
    env = make_env(x0[:B], u0[:B])
    traj = env.rollout(nsteps, traj_every=e)
    assert rel(env.x_values.cpu().numpy(), xr[:B]) < 1e-9
    assert np.array_equal(env.status.cpu().numpy(), np.asarray(st)[:B])
    if e is None:
        assert traj is None
        return
    assert tuple(traj.shape) == (nsteps // e, 18, B)
    for k in range(nsteps // e):                                   # sample k = the state after step (k + 1) * every
        assert rel(traj[k].t().cpu().numpy(), trj[(k + 1) * e - 1][:B]) < 1e-9, k
    assert bits(traj[-1], env._x)                                  # the last sample is the state the launch leaves


# ------------------------------------------------------------------------------------------------ each role's envelope flag
def test_every_role_reports_its_envelope_flag_and_reads_the_others(oracle):
    from f16_mpc_oop_py_amd.lib import F16_ST, F16_ST_ENV_STATE
    x0, u0 = restated(oracle, 1)[:2]
    x, u = x0[:17].copy(), u0[:17].copy()
    out = {2: (2, -5.0), 5: (9, 301.0), 9: (12, 19500.0), 12: (16, 26.0)}      # aircraft: (state, value) -- owners: waves 2, 1, 3, 3 (flap)
    for b, (k, v) in out.items():
        x[b, k] = v
    env = make_env(x, u)
    traj = env.rollout(5, traj_every=1)
    xr, trj, st = oracle.rollout(x, u, 5, store=True)
    got, gst = env.x_values.cpu().numpy(), env.status.cpu().numpy()
    assert np.array_equal(gst, np.asarray(st))                     # ST_ENVELOPE with the owner's state bit, nothing on the live ones
    for b, (k, v) in out.items():
        assert gst[b] == F16_ST["ENVELOPE"] | F16_ST_ENV_STATE(k)
        assert np.array_equal(got[b], x[b])                        # frozen: the state it started with, bit for bit
        assert all(np.array_equal(traj[t].t().cpu().numpy()[b], x[b]) for t in range(5))
    live = [b for b in range(17) if b not in out]
    assert not gst[live].any()
    assert rel(got[live], xr[live]) < 1e-9
    for t in range(5):
        assert rel(traj[t].t().cpu().numpy()[live], trj[t][live]) < 1e-9


# ------------------------------------------------------------------------------------------------ template variants
@pytest.mark.parametrize("every", [2, 3])
def test_lqr_law_in_the_role_loops(oracle, every):
    """rollout_LQR against the restated loop, as test_closed_loop_lqr_rollout_every_kernel_vs_oracle_loop (xcg 0.25: 1e-8)"""
    x0, u0 = restated(oracle, 1)[:2]
    x0, u0 = x0[:17], u0[:17]
    dem = np.random.default_rng(17).uniform(-0.1, 0.1, (17, 3))
    env = make_env(x0, u0)
    K = env._calc_LQR_gain()
    traj = env.rollout_LQR(6, dem[:, 0], dem[:, 1], dem[:, 2], K=K, traj_every=every)
    xr, trj, ul, st = oracle.rollout_lqr(x0, u0, K.cpu().numpy(), dem, 6)
    gst = env.status.cpu().numpy()
    assert np.array_equal(np.asarray(st) & 16, gst & 16)
    ok = (gst == 0) & np.isfinite(xr).all(1)
    assert ok.mean() > 0.95
    assert rel(env.x_values.cpu().numpy()[ok], xr[ok]) < 1e-8
    assert rel(env.u_values.cpu().numpy()[ok], ul[ok]) < 1e-8
    for k in range(6 // every):
        assert rel(traj[k].t().cpu().numpy()[ok], trj[(k + 1) * every - 1][ok]) < 1e-8
    assert np.array_equal(env.u_values.cpu().numpy()[:, 0], u0[:, 0])         # the thrust command is not an LQR output


@pytest.mark.parametrize("every", [2, 3])
def test_command_schedule_in_the_role_loops(dev, oracle, every):
    """f16_rollout_sched: the chain of launches bit for bit, the restatement chained per segment at 1e-9 (test_gpu_rollout_sched.py)"""
    x0, u0 = restated(oracle, 1)[:2]
    x0, u0 = x0[:17], u0[:17]
    rows = doublet_rows(u0, 3)
    one = dev.run(x0, rows, 6, 2, every)
    assert same(one, dev.run(x0, rows, 6, 2, every, chain=True), 17)
    xr, steps = x0, []
    for r in range(3):
        xr, tr, so = oracle.rollout(xr, rows[r], 2, store=True)
        assert not np.asarray(so).any()
        steps += list(tr)
    assert rel(one[0].t().cpu().numpy(), xr) < 1e-9 and int(one[2].max()) == 0
    for k in range(6 // every):
        assert rel(one[1][k].t().cpu().numpy(), steps[(k + 1) * every - 1]) < 1e-9


@pytest.mark.parametrize("every", [2, 3])
def test_demand_schedule_under_the_lqr_law_in_the_role_loops(dev, oracle, every):
    """f16_rollout_lqr_sched: the chain of f16_rollout_lqr launches bit for bit; the restated loop chained per row at the 1e-8 of G17"""
    x0, u0 = restated(oracle, 1)[:2]
    x0, u0 = x0[:17], u0[:17]
    rows = doublet_rows(u0, 3, lqr=True)
    K = lqr_gain(x0, u0, 1, 0.25)                                              # [27, B]
    one = dev.run(x0, rows, 6, 2, every, K=K, u0=u0)
    assert same(one, dev.run(x0, rows, 6, 2, every, chain=True, K=K, u0=u0), 17)
    Kh = K.t().reshape(17, 3, 9).cpu().numpy()
    xr, steps = x0, []
    for r in range(3):
        xr, tr, ul, so = oracle.rollout_lqr(xr, u0, Kh, rows[r], 2)
        steps += list(tr)
    ok = (one[2].cpu().numpy() == 0) & np.isfinite(xr).all(1)
    assert ok.mean() > 0.95
    assert rel(one[0].t().cpu().numpy()[ok], xr[ok]) < 1e-8 and rel(one[3].t().cpu().numpy()[ok], ul[ok]) < 1e-8
    for k in range(6 // every):
        assert rel(one[1][k].t().cpu().numpy()[ok], steps[(k + 1) * every - 1][ok]) < 1e-8


@pytest.mark.parametrize("every", [2, 3])
def test_cost_rollout_beside_the_role_loops(dev, oracle, every):
    """f16_rollout_cost at the same shape: the cost is its definition on the launch's own samples (check_cost), the states are the
    restatement's chained per segment at 1e-9, and what is stored changes neither (test_gpu_rollout_cost.py)"""
    x0, u0, rows, xref, uref = tc.case_inputs(17, 1, 3)
    w = tc.weights()
    full = tc.run_cost(dev, x0, rows, xref, uref, w, 6, 2, 1)
    tc.check_cost(dev, full, x0, rows, xref, uref, w, 6, 2)
    xr = x0
    for r in range(3):
        xr, _, so = oracle.rollout(xr, rows[r, 0], 2, store=False)
        assert not np.asarray(so).any()
    assert rel(full["x_end"].t().cpu().numpy()[:17], xr) < 1e-9 and int(full["st"][:17].max()) == 0
    out = tc.run_cost(dev, x0, rows, xref, uref, w, 6, 2, every)
    assert bits(out["cost"], full["cost"]) and bits(out["st"], full["st"]) and bits(out["x_end"], full["x_end"])
    assert bits(out["traj"][:, :, :17], full["traj"][every - 1::every][:, :, :17])


# ------------------------------------------------------------------------------------------------ split launches
def test_split_launches_give_the_bits_of_one_launch(oracle):
    x0, u0 = restated(oracle, 1)[:2]
    one = make_env(x0[:17], u0[:17])
    t1 = one.rollout(6, traj_every=1)
    parts = make_env(x0[:17], u0[:17])
    import torch
    tp = torch.cat([parts.rollout(n, traj_every=1) for n in (1, 2, 3)])
    assert bits(parts._x, one._x) and bits(parts.status, one.status) and bits(tp, t1)
