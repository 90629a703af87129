"""GPU tests of the closed loops under a demand schedule, one launch each: f16_rollout_mpc_sched / f16_rollout_mpc_relin_sched /
F16Batch.rollout_MPC(dem_every=k) and f16_rollout_lqr_relin_sched / F16Batch.rollout_LQR_relin(x_ref=[S, 9, B], hold=k).

Shapes unless said otherwise: N = 10, plant dt 1e-3, OSQP's defaults, xcg 0.35.  A schedule only decides which demand row a (control
step, aircraft) pair reads, so the checker is the CHAIN of existing calls -- one f16_rollout_mpc_hold / f16_rollout_mpc_relin_hold /
f16_rollout_lqr_relin call per row, with that row as the constant demand -- bit for bit; and, for the frozen loop, the CPU twin composed
from the C oracle (tests/test_mpc_sched_cpu.py: cpu_twin_sched)."""

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401
from test_gpu_mpc_hold import DEM, DT, ENV_V, ST_MASK, XCG, _c_hold, _np, _same, _vp, make_env
from test_mpc_sched_cpu import TWIN_ROWS, twin_inputs

pytestmark = pytest.mark.gpu

EINVAL = -1
N = 10


def _rows(S, B, seed=5):
    """demand rows that differ per aircraft and per row: [S, 3, B] on the device"""
    return torch.as_tensor(np.random.default_rng(seed).uniform(-0.05, 0.05, (S, 3, B)), device="cuda:0")


def _const_rows(S, B, dem=DEM):
    return torch.as_tensor(np.asarray(dem, dtype=np.float64)[None, :, None].repeat(S, 0).repeat(B, 2), device="cuda:0").contiguous()


def _c_sched(env, rows, nctrl, hold, dem_hold, every=1, dt=DT, flags=0, relin=False, model_every=1, eps=1e-5):
    """f16_rollout_mpc_sched / f16_rollout_mpc_relin_sched through the C ABI on env's plan, x.values, u.values and status; rows
    [S, 3, B] on the device, or None (a NULL dem_seq).  -> (rc, traj, cmd, iters, model or None)"""
    B, dev = env.B, env.device
    n = max(nctrl, 1)                        # (calls that must be refused still get buffers)
    traj = torch.full((max(nctrl * hold // max(every, 1), 1), 18, B), -7.0, dtype=torch.float64, device=dev)
    cmd = torch.full((n, 3, B), -7.0, dtype=torch.float64, device=dev)
    its = torch.full((n, B), -7, dtype=torch.int32, device=dev)
    if rows is not None:
        assert rows.is_contiguous() and tuple(rows.shape[1:]) == (3, B) and rows.shape[0] >= (n + max(dem_hold, 1) - 1) // max(dem_hold, 1)
    if relin:
        model = torch.full((max(n // max(model_every, 1), 1), 189, B), -7.0, dtype=torch.float64, device=dev)
        rc = env.lib.f16_rollout_mpc_relin_sched(env._plan, _vp(env._x), _vp(env._u), _vp(rows), _vp(traj), _vp(cmd), _vp(its), _vp(model),
                                                 _vp(env.status), nctrl, hold, dem_hold, every, model_every, dt, eps, XCG, 1,
                                                 env.flags | flags, env._stream)
    else:
        model = None
        rc = env.lib.f16_rollout_mpc_sched(env._plan, _vp(env._x), _vp(env._u), _vp(rows), _vp(traj), _vp(cmd), _vp(its), _vp(env.status),
                                           nctrl, hold, dem_hold, every, dt, XCG, 1, env.flags | flags, env._stream)
    torch.cuda.synchronize()
    return rc, traj, cmd, its, model


def _chain(env, rows, nctrl, hold, dem_hold, relin=False, flags=0):
    """The chain the scheduled call equals: one existing call per row (f16_rollout_mpc_hold / f16_rollout_mpc_relin_hold) with that row
    as the constant demand, traj_every = model_every = 1.  -> (samples of every plant step, cmd, iters, model or None)"""
    out = []
    for r in range((nctrl + dem_hold - 1) // dem_hold):
        n = min(dem_hold, nctrl - r * dem_hold)
        rc, tr, c, i, m = _c_hold(env, n, hold, dem=tuple(rows[r]), relin=relin, flags=flags)
        assert rc == 0, env.lib.f16_last_error()
        out.append((tr, c, i, m))
    cat = lambda k: torch.cat([o[k] for o in out])
    return cat(0), cat(1), cat(2), cat(3) if relin else None


def _planned(x0, u0, hold, **plan_kw):
    env = make_env(x0, u0)
    env.build_ssr(); env.prepare_MPC(N, ctrl_every=hold, **plan_kw)
    return env


def _assert_equal(ea, ra, eb, rb, every=1, what=""):
    """x, u, status, every sample bit for bit; commands, iteration counts and models for the aircraft that are not frozen (as the
    host-loop tests of tests/test_gpu_mpc_hold.py do).  ra: the scheduled call's (traj, cmd, iters, model) at `every`; rb: the
    checker's at every plant step.  -> the mask of the aircraft inside their envelope"""
    (tra, ca, ia, ma), (trb, cb, ib, mb) = ra, rb
    assert _same(ea._x, eb._x) and _same(ea._u, eb._u) and _same(ea.status, eb.status), what
    assert _same(tra, trb[every - 1::every]) and _same(tra[-1], ea._x), what
    inside = torch.as_tensor((_np(ea.status) & 16) == 0, device="cuda:0")
    assert _same(ca[:, :, inside], cb[:, :, inside]) and _same(ia[:, inside], ib[:, inside]), what
    assert (ma is None) == (mb is None)
    if ma is not None:
        assert _same(ma[:, :, inside], mb[:, :, inside]), what
    return inside


@pytest.fixture(scope="module")
def states256():
    from f16_mpc_oop_py_amd.workload import config4_states
    return config4_states(256)


@pytest.mark.timeout(300, method="thread")      # (a persistent kernel that never drains must fail the run, not hold it)
@pytest.mark.parametrize("hold,dem_hold,warm", [(1, 1, False), (1, 3, False), (5, 2, False), (5, 2, True)])
def test_identical_rows_equal_the_existing_call(states256, hold, dem_hold, warm):
    """S identical rows against f16_rollout_mpc_hold / f16_rollout_mpc_relin_hold with that row as the constant demand: B = 256, 4
    control steps; once on a plan with the warm start on."""
    x0, u0 = states256
    kw = dict(warm_start=True) if warm else {}
    for relin in (False, True):
        ea, eb = _planned(x0, u0, hold, **kw), _planned(x0, u0, hold, **kw)
        rc, *ra = _c_sched(ea, _const_rows((4 + dem_hold - 1) // dem_hold, 256), 4, hold, dem_hold, relin=relin)
        assert rc == 0, ea.lib.f16_last_error()
        rc, *rb = _c_hold(eb, 4, hold, relin=relin)
        assert rc == 0, eb.lib.f16_last_error()
        inside = _assert_equal(ea, ra, eb, rb, what=f"relin={relin}")
        assert int(inside.sum()) >= 255 and int(ra[2][0].min()) >= 25


CHAIN_CASES = [(1, 1, 6, 2, 1), (1, 17, 6, 2, 1), (1, 256, 6, 1, 1), (5, 100, 6, 2, 3), (5, 256, 5, 2, 1)]


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("relin", [False, True])
@pytest.mark.parametrize("hold,B,nctrl,dem_hold,every", CHAIN_CASES)
def test_one_launch_equals_the_chain_of_existing_calls(states256, hold, B, nctrl, dem_hold, every, relin):
    """Rows that differ per aircraft.  B = 1; B = 17, the first batch size with the ticket permutation; a row per control step; samples
    inside and at the end of a hold across a row change (traj_every = 3, hold = 5); a shorter last segment (5 control steps, rows of 2)."""
    x0, u0 = states256[0][:B], states256[1][:B]
    rows = _rows((nctrl + dem_hold - 1) // dem_hold, B)
    ea, eb = _planned(x0, u0, hold), _planned(x0, u0, hold)
    rc, *ra = _c_sched(ea, rows, nctrl, hold, dem_hold, every=every, relin=relin)
    assert rc == 0, ea.lib.f16_last_error()
    assert tuple(ra[0].shape) == (nctrl * hold // every, 18, B) and tuple(ra[1].shape) == (nctrl, 3, B)
    inside = _assert_equal(ea, ra, eb, _chain(eb, rows, nctrl, hold, dem_hold, relin=relin), every=every)
    assert int(inside.sum()) >= B - 1 and int(ra[2][0].min()) >= 25           # (solves that iterate)


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("relin", [False, True])
def test_rows_are_really_read(states256, relin):
    """Two calls whose rows differ only from row 2 on (B = 256, 6 control steps, a row per step): cmd_traj[0], cmd_traj[1] are
    bit-equal, cmd_traj[2..] differ."""
    x0, u0 = states256
    rows = _rows(6, 256)
    other = rows.clone()
    other[2:] = _rows(4, 256, seed=6)
    ea, eb = _planned(x0, u0, 1), _planned(x0, u0, 1)
    rca, _, ca, ia, _ = _c_sched(ea, rows, 6, 1, 1, relin=relin)
    rcb, _, cb, ib, _ = _c_sched(eb, other, 6, 1, 1, relin=relin)
    assert rca == 0 and rcb == 0
    assert _same(ca[:2], cb[:2]) and _same(ia[:2], ib[:2])
    for c in range(2, 6):
        d = (ca[c] - cb[c]).abs().nan_to_num(0.0).max(0).values                # per aircraft
        # every aircraft that is solved for got another demand, hence another QP; those that are not (outside the envelope: at most one
        # of B in these batches; NaN after an infeasible QP) carry NaN under both schedules -- nine in ten must differ
        assert not _same(ca[c], cb[c]) and float((d > 0).double().mean()) >= 0.9, c
    assert not _same(ea._x, eb._x)


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("hold", [1, 5])
def test_scheduled_launch_vs_the_cpu_twin(oracle, hold):
    """16 config-4 states (seed 20261003), 6 control steps, rows (0, 0, 0), (0.02, -0.01, 0.005), (-0.02, 0.01, -0.005) of two control
    steps each, through rollout_MPC(..., dem_every=2) at ctrl_every 1 and 5, against the loop composed from the C oracle
    (cpu_twin_sched; tests/test_mpc_sched_cpu.py checks that these inputs are fit: 16 resp. 15 of 16 kept, >= 125 iterations, commands
    0.052 / 0.059 away from the constant-row-0 run).  Bands: those of test_one_launch_vs_the_cpu_twin -- every iteration count equal,
    commands <= 5e-5, states <= 1e-6 relative to max(1, |x|); the status words agree on 16|32|64|128; aircraft are dropped only for
    bits 32 / 128 on BOTH sides and at least 14 of 16 are compared.
    The measured differences are printed (run with -s)."""
    B, nctrl = 16, 6
    x0, u0, (xc, cc, ic, sc), _ = twin_inputs(oracle, hold)
    env = make_env(x0, u0)
    env.build_ssr()
    rows = np.asarray(TWIN_ROWS)
    _, info = env.rollout_MPC(nctrl * hold, rows[:, 0], rows[:, 1], rows[:, 2], N, return_info=True, ctrl_every=hold, dem_every=2)
    cg, ig, sg, xg = _np(info["cmd"]).transpose(0, 2, 1), _np(info["iters"]), _np(env.status), _np(env.x_values)
    print("status (GPU):", sg.tolist(), "\nstatus (CPU):", sc.tolist())
    print("iterations (GPU):", ig.tolist(), "\niterations (CPU):", ic.tolist())
    assert np.array_equal(sg & ST_MASK, sc & ST_MASK)
    dropped = ((sg & (128 | 32)) != 0) & ((sc & (128 | 32)) != 0)             # flagged on BOTH sides: NaN from there on
    keep = ~dropped
    assert keep.sum() >= 14
    assert np.array_equal(np.isnan(cg), np.isnan(cc)) and np.array_equal(np.isnan(xg), np.isnan(xc))
    e_cmd = float(np.abs(cg[:, keep] - cc[:, keep]).max())
    e_x = float(np.max(np.abs(xg[keep] - xc[keep]) / np.maximum(1.0, np.abs(xc[keep]))))
    print(f"ctrl_every {hold}: compared {int(keep.sum())} of {B}; counts equal: {np.array_equal(ig, ic)}; max |dcmd| {e_cmd:.3e}; max rel dx {e_x:.3e}")
    assert np.array_equal(ig, ic)                                              # all 16, the dropped ones included
    assert ic[:, keep].min() >= 25 and e_cmd <= 5e-5 and e_x <= 1e-6


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("relin", [False, True])
def test_non_finite_row_for_three_aircraft_equals_the_chain(states256, relin):
    """A non-finite entry in row 1 for three aircraft (B = 64, 6 control steps, rows of 2), with and without F16_FLAG_HOLD_COMMAND: their
    control steps 2 and 3 are PAIR_NONFINITE (NaN command, 0 iterations, F16_ST_NONFINITE).  With the flag they keep the command of
    step 1, fly on and are solved for again under row 2; without it the NaN command reaches the actuators and they are never solved
    for again.  Everybody equals the chain."""
    from f16_mpc_oop_py_amd import lib as L
    B = 64
    x0, u0 = states256[0][:B], states256[1][:B]
    rows = _rows(3, B)
    # three aircraft that the clean schedule solves for at every control step (the edit below must be what stops their solves)
    rc, _, c0, i0, _ = _c_sched(_planned(x0, u0, 1), rows, 6, 1, 2, relin=relin)
    assert rc == 0
    bad = torch.nonzero(torch.isfinite(c0).all(1).all(0) & (i0 >= 25).all(0)).flatten().tolist()[1:4]
    assert len(bad) == 3
    rows = rows.clone()
    rows[1, 0, bad[0]], rows[1, 1, bad[1]], rows[1, 2, bad[2]] = float("nan"), float("inf"), float("nan")
    good = [b for b in range(B) if b not in bad]
    for flags in (0, L.F16_FLAG_HOLD_COMMAND):
        ea, eb = _planned(x0, u0, 1), _planned(x0, u0, 1)
        rc, *ra = _c_sched(ea, rows, 6, 1, 2, relin=relin, flags=flags)
        assert rc == 0, ea.lib.f16_last_error()
        _assert_equal(ea, ra, eb, _chain(eb, rows, 6, 1, 2, relin=relin, flags=flags), what=f"flags={flags}")
        _, cmd, its, model = ra
        assert int(its[:2, bad].min()) >= 25 and bool(torch.isfinite(cmd[:2][:, :, bad]).all())
        assert bool(torch.isnan(cmd[2:4][:, :, bad]).all()) and int(its[2:4, bad].abs().sum()) == 0
        assert bool(((ea.status[bad] & 32) != 0).all()) and int(its[0, good].min()) >= 25
        if relin:
            assert bool(torch.isnan(model[2:4][:, :, bad]).all()) and bool(torch.isfinite(model[0]).all())
        if flags:      # solved for again under row 2
            assert int(its[4:, bad].min()) > 0 and bool(torch.isfinite(ea._x[:, bad]).all())
            assert not relin or bool(torch.isfinite(model[4:][:, :, bad]).all())
        else:
            assert bool(torch.isnan(cmd[4:][:, :, bad]).all()) and int(its[4:, bad].abs().sum()) == 0 and bool(torch.isnan(ea._x[13:16, bad]).all())


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("relin", [False, True])
def test_envelope_exit_inside_a_hold_under_a_schedule(relin):
    """The envelope exit of test_envelope_exit_between_two_control_instants (aircraft 2 of config4_states(16, seed=20261003) with
    x[6] = 899.984 ft/s as number 2 of a batch of 64, hold = 5) under a three-row schedule of two control steps each: found outside
    at the start of a plant step inside the hold of control step 0, frozen there, the later samples repeat that state, control steps
    1.. carry NaN commands and 0 iterations whatever the rows say; its neighbours equal the same batch without the edit; everybody
    equals the chain."""
    from f16_mpc_oop_py_amd.workload import config4_states
    B, hold, nctrl, b = 64, 5, 6, 2
    x16, u16 = config4_states(16, seed=20261003)
    x0, u0 = config4_states(B, seed=20261003)
    x0[b], u0[b] = x16[b], u16[b]
    x1 = x0.copy()
    x1[b, 6] = 899.984
    rows = _rows(3, B)
    rows[0] = _const_rows(1, B)[0]                                             # control steps 0, 1: the demand of the existing test
    ef, ec, eh = _planned(x1, u0, hold), _planned(x0, u0, hold), _planned(x1, u0, hold)
    rc, *rf = _c_sched(ef, rows, nctrl, hold, 2, relin=relin)
    assert rc == 0, ef.lib.f16_last_error()
    trf, cf, itf, mf = rf
    _assert_equal(ef, rf, eh, _chain(eh, rows, nctrl, hold, 2, relin=relin))
    assert (int(ef.status[b]) & ~15) == ENV_V and int(itf[0, b]) >= 25 and bool(torch.isfinite(cf[0, :, b]).all())
    v = _np(trf[:, 6, b])
    first = int(np.argmax(v > 900.0)) + 1                                       # plant steps taken when it is found outside
    assert v[first - 1] > 900.0 and v[first - 2] <= 900.0 and first % hold != 0 and first < hold, first
    frozen = trf[first - 1, :, b]
    assert all(_same(trf[s, :, b], frozen) for s in range(first, nctrl * hold)) and _same(ef._x[:, b], frozen)
    assert bool(torch.isnan(cf[1:, :, b]).all()) and int(itf[1:, b].abs().sum()) == 0 and _same(ef._u[1:4, b], cf[0, :, b])
    if relin:
        assert bool(torch.isnan(mf[1:, :, b]).all()) and bool(torch.isfinite(mf[0, :, b]).all())
    rc, trc, cc, ic, mc = _c_sched(ec, rows, nctrl, hold, 2, relin=relin)
    others = [k for k in range(B) if k != b]
    assert rc == 0 and _same(trf[:, :, others], trc[:, :, others]) and _same(cf[:, :, others], cc[:, :, others])
    assert _same(itf[:, others], ic[:, others]) and _same(ef.status[others], ec.status[others])
    assert not relin or _same(mf[:, :, others], mc[:, :, others])


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("relin", [False, True])
def test_two_calls_at_a_row_boundary_equal_one(states256, relin):
    """B = 100, hold = 5, 6 control steps, rows of 2, cut after control step 4 (cold plan): 4 control steps under rows 0..1, then 2
    under row 2, equal the one call."""
    B, hold = 100, 5
    x0, u0 = states256[0][:B], states256[1][:B]
    rows = _rows(3, B)
    ea, eb = _planned(x0, u0, hold), _planned(x0, u0, hold)
    rc, *ra = _c_sched(ea, rows, 6, hold, 2, relin=relin)
    assert rc == 0, ea.lib.f16_last_error()
    rc1, *p1 = _c_sched(eb, rows[:2].contiguous(), 4, hold, 2, relin=relin)
    rc2, *p2 = _c_sched(eb, rows[2:].contiguous(), 2, hold, 2, relin=relin)
    assert rc1 == 0 and rc2 == 0, eb.lib.f16_last_error()
    rb = [torch.cat([p1[k], p2[k]]) for k in range(3)] + [torch.cat([p1[3], p2[3]]) if relin else None]
    inside = _assert_equal(ea, ra, eb, rb)
    assert int(inside.sum()) >= B - 1


@pytest.mark.timeout(300, method="thread")
def test_sched_argument_checks(states256):
    """F16_EINVAL for dem_hold = 0, a NULL dem_seq, the frozen call on a plan marked by a re-linearised call, and hold x dt unequal to
    the plan's period; x is untouched in each case."""
    B = 8
    x0, u0 = states256[0][:B], states256[1][:B]
    env = _planned(x0, u0, 5)
    rows = _rows(2, B)
    before = env.x_values.clone()
    for relin in (False, True):
        call = lambda r=rows, **kw: _c_sched(env, r, kw.pop("nctrl", 2), kw.pop("hold", 5), kw.pop("dem_hold", 1), relin=relin, **kw)[0]
        assert call(dem_hold=0) == EINVAL and b"dem_hold" in env.lib.f16_last_error()
        assert call(dem_hold=-3) == EINVAL and call(r=None) == EINVAL
        assert call(dt=DT * (1 + 1e-6)) == EINVAL and b"plan" in env.lib.f16_last_error()      # hold x dt off the plan's period
        assert call(hold=1) == EINVAL and call(hold=4) == EINVAL and call(hold=0) == EINVAL and call(nctrl=0) == EINVAL
        assert call(every=3) == EINVAL and call(every=0) == EINVAL                             # 10 plant steps
        if relin:
            assert call(model_every=0) == EINVAL and call(eps=0.0) == EINVAL
    assert env.lib.f16_rollout_mpc_sched(None, None, None, None, None, None, None, None, 1, 1, 1, 1, DT, XCG, 1, 0, None) == EINVAL
    assert bool((env.x_values == before).all()) and int(env.status.max()) == 0
    # a plan marked by the re-linearised call: refused by the frozen call, taken by the re-linearised one
    assert _c_sched(env, rows, 1, 5, 1, relin=True)[0] == 0
    after = env.x_values.clone()
    assert _c_sched(env, rows, 1, 5, 1)[0] == EINVAL and b"model" in env.lib.f16_last_error()
    assert _same(env.x_values, after) and not _same(after, before)          # (equal_nan: an infeasible QP leaves NaN actuator states)
    assert _c_sched(env, rows, 1, 5, 1, relin=True)[0] == 0


@pytest.mark.timeout(300, method="thread")
def test_python_surface_of_the_scheduled_loops(states256):
    """rollout_MPC with [S] and [S, B] histories and scalars mixed = the C call on the composed rows (frozen and re-linearised,
    ctrl_every 1 and 5); dist.closed_loop_mpc_rollout fused = host loop (one_lane) under a schedule; a one-row history with
    dem_every = nsteps = the scalar call."""
    from f16_mpc_oop_py_amd import dist
    B = 64
    x0, u0 = states256[0][:B], states256[1][:B]
    rng = np.random.default_rng(11)
    p, q, r = rng.uniform(-0.03, 0.03, 3), rng.uniform(-0.03, 0.03, (3, B)), 0.004
    rows = torch.empty((3, 3, B), dtype=torch.float64, device="cuda:0")
    rows[:, 0], rows[:, 1], rows[:, 2] = torch.as_tensor(p, device="cuda:0")[:, None], torch.as_tensor(q, device="cuda:0"), r
    for hold, relin in ((1, False), (5, False), (5, True)):
        ea, eb = make_env(x0, u0), _planned(x0, u0, hold)
        kw = dict(relinearise=True) if relin else {}
        tra, infa = ea.rollout_MPC(6 * hold, p, q, r, N, traj_every=1, return_info=True, ctrl_every=hold, dem_every=2, **kw)
        rc, *rb = _c_sched(eb, rows, 6, hold, 2, relin=relin)
        assert rc == 0 and (ea._plan_hzn, ea._plan_ctrl_every) == (N, hold) and bool(ea._plan_foreign) == relin
        _assert_equal(ea, (tra, infa["cmd"], infa["iters"], infa.get("model")), eb, rb)
    assert make_env(x0, u0).rollout_MPC(4, p, q, r, N, dem_every=2) is None    # no samples asked for
    # dist: fused = the call above; the host loop picks the row per control step
    for hold, kw in ((1, {}), (5, {}), (1, dict(relinearise=False, hold_command=True))):
        ef, eh = make_env(x0, u0), make_env(x0, u0)
        trf = dist.closed_loop_mpc_rollout(ef, 6 * hold, N, p, q, r, traj_every=1, gather=False, ctrl_every=hold, dem_every=2, fused=True, **kw)
        trh = dist.closed_loop_mpc_rollout(eh, 6 * hold, N, p, q, r, traj_every=1, gather=False, ctrl_every=hold, dem_every=2, fused=False,
                                           one_lane=True, **kw)
        assert tuple(trf.shape) == (6 * hold, 18, B) and _same(trf, trh) and _same(ef._x, eh._x) and _same(ef.status, eh.status)
        inside = torch.as_tensor((_np(ef.status) & 16) == 0, device="cuda:0")
        assert _same(ef._u[:, inside], eh._u[:, inside]) and int(inside.sum()) >= B - 1
    # a one-row history with dem_every = nsteps is the scalar call
    e1, e2 = make_env(x0, u0), make_env(x0, u0)
    t1, i1 = e1.rollout_MPC(4, np.array([DEM[0]]), DEM[1], np.full((1, B), DEM[2]), N, traj_every=1, return_info=True, dem_every=4)
    t2, i2 = e2.rollout_MPC(4, *DEM, N, traj_every=1, return_info=True)
    assert _same(t1, t2) and _same(i1["cmd"], i2["cmd"]) and _same(i1["iters"], i2["iters"]) and _same(e1._x, e2._x) and _same(e1._u, e2._u)


# ---------------------------------------------------------------------------------------------- f16_rollout_lqr_relin_sched
def _lqr_call(env, xref, u03, nsteps, hold=None, mask=0x70, every=1):
    """f16_rollout_lqr_relin (hold None, xref [9, B]) / f16_rollout_lqr_relin_sched (xref [S, 9, B]) on env's x.values, u.values and
    status.  -> (rc, traj, u_traj, K_traj)"""
    B, dev = env.B, env.device
    mk = lambda rows: torch.full((max(nsteps // every, 1), rows, B), -7.0, dtype=torch.float64, device=dev)
    traj, ut, kt = mk(18), mk(3), mk(27)
    head = (env.ctx.handle, _vp(env._x), _vp(env._u), _vp(xref), _vp(u03), None, _vp(traj), _vp(ut), _vp(kt), _vp(env.status), B, B, nsteps)
    tail = (every, mask, 1e-5, DT, XCG, 1, env.flags, env._stream)
    rc = env.lib.f16_rollout_lqr_relin(*head, *tail) if hold is None else env.lib.f16_rollout_lqr_relin_sched(*head, hold, *tail)
    torch.cuda.synchronize()
    return rc, traj, ut, kt


def _xref_rows(S, B):
    xr = torch.zeros((S, 9, B), dtype=torch.float64, device="cuda:0")
    xr[:, 4:7] = _rows(S, B)                                                   # the entries track_mask 0x70 selects; the others are not read
    xr[:, :4], xr[:, 7:] = float("nan"), float("nan")
    return xr


def _lqr_chain(env, xr, u03, nsteps, hold):
    out = []
    for r in range((nsteps + hold - 1) // hold):
        rc, *o = _lqr_call(env, xr[r].contiguous(), u03, min(hold, nsteps - r * hold))
        assert rc == 0, env.lib.f16_last_error()
        out.append(o)
    return [torch.cat([o[k] for o in out]) for k in range(3)]


def _lqr_equal(ea, ra, eb, rb):
    assert _same(ea._x, eb._x) and _same(ea._u, eb._u) and _same(ea.status, eb.status)
    assert _same(ra[0], rb[0]) and _same(ra[1], rb[1]) and _same(ra[0][-1], ea._x)
    inside = torch.as_tensor((_np(ea.status) & 16) == 0, device="cuda:0")      # (the chain zeroes the gain of an aircraft frozen on entry)
    assert _same(ra[2][:, :, inside], rb[2][:, :, inside])
    return inside


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("hold", [1, 4, 5])
@pytest.mark.parametrize("B", [1, 64])
def test_lqr_relin_under_a_schedule_equals_the_chain(B, hold):
    """12 steps, track_mask 0x70, rows that differ per aircraft (hold = 5: a shorter last segment) against one f16_rollout_lqr_relin
    call per row; identical rows against the one existing call; a freeze mid-schedule (B = 64: aircraft 2 with x[6] = 899.984 passes
    V = 900 after four steps) against the chain; rollout_LQR_relin(x_ref=[S, 9, B], hold=4) against the C call."""
    from f16_mpc_oop_py_amd.workload import config4_states
    n, S = 12, (12 + hold - 1) // hold
    x16, u16 = config4_states(16, seed=20261003)
    x0, u0 = config4_states(max(B, 16), seed=20261003)
    x0, u0 = x0[:B].copy(), u0[:B].copy()
    if B == 64:
        x0[2], u0[2] = x16[2], u16[2]          # (the aircraft of test_envelope_exit_between_two_control_instants)
    xr = _xref_rows(S, B)
    mk = lambda x=x0: (make_env(x, u0), torch.as_tensor(np.ascontiguousarray(u0[:, 1:4].T), device="cuda:0"))
    (ea, u03), (eb, _) = mk(), mk()
    rc, *ra = _lqr_call(ea, xr, u03, n, hold=hold)
    assert rc == 0, ea.lib.f16_last_error()
    inside = _lqr_equal(ea, ra, eb, _lqr_chain(eb, xr, u03, n, hold))
    assert bool(inside.all()) and bool(torch.isfinite(ra[0]).all()) and float(ra[2].abs().max()) > 0
    # the rows are read: the one-row call ends somewhere else
    (ec, _), (ed, _) = mk(), mk()
    same_rows = xr[:1].repeat(S, 1, 1).contiguous()
    rc, *rc_ = _lqr_call(ec, same_rows, u03, n, hold=hold)
    rd, *rd_ = _lqr_call(ed, xr[0].contiguous(), u03, n)
    assert rc == 0 and rd == 0
    _lqr_equal(ec, rc_, ed, rd_)
    assert S == 1 or not _same(ea._u, ec._u)
    if B == 64:
        x1 = x0.copy()
        x1[2, 6] = 899.984
        (ef, _), (eg, _) = mk(x1), mk(x1)
        rc, *rf = _lqr_call(ef, xr, u03, n, hold=hold)
        assert rc == 0
        inside = _lqr_equal(ef, rf, eg, _lqr_chain(eg, xr, u03, n, hold))
        v = _np(rf[0][:, 6, 2])
        first = int(np.argmax(v > 900.0)) + 1                                  # steps taken when it is found outside
        assert int(inside.sum()) == B - 1 and (int(ef.status[2]) & 16) and v[first - 1] > 900.0 and 2 <= first < n - 1, first
        assert all(_same(rf[0][s, :, 2], rf[0][first - 1, :, 2]) for s in range(first, n)) and not _same(rf[0][first - 2, :, 2], rf[0][first - 1, :, 2])
    if hold == 4:
        ep, _ = mk()
        tr, ut, kt = ep.rollout_LQR_relin(n, x_ref=xr, track=(4, 5, 6), u0=u0[:, 1:4], traj_every=1, gains_every=1, hold=4)
        assert _same(tr, ra[0]) and _same(ut, ra[1]) and _same(kt, ra[2].permute(0, 2, 1).reshape(n, B, 3, 9)) and _same(ep._x, ea._x)
        with pytest.raises(ValueError):
            ep.rollout_LQR(n, np.zeros(3), 0.0, 0.0, relinearise=True)          # histories stay refused there


@pytest.mark.timeout(300, method="thread")
def test_lqr_relin_sched_argument_checks():
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(4, seed=1)
    env = make_env(x0, u0)
    xr = _xref_rows(3, 4)
    before = env.x_values.clone()
    assert _lqr_call(env, xr, None, 12, hold=0)[0] == EINVAL and b"hold" in env.lib.f16_last_error()
    assert _lqr_call(env, xr, None, 12, hold=-1)[0] == EINVAL
    assert _lqr_call(env, None, None, 12, hold=4)[0] == EINVAL and b"track_mask" in env.lib.f16_last_error()
    assert _lqr_call(env, xr, None, 0, hold=4)[0] == EINVAL and _lqr_call(env, xr, None, 12, hold=4, every=5)[0] == EINVAL
    assert bool((env.x_values == before).all())
    assert _lqr_call(env, None, None, 2, hold=1, mask=0)[0] == 0                # nothing tracked: no rows needed
    assert _lqr_call(env, xr, None, 12, hold=100)[0] == 0                       # hold >= nsteps: row 0 only
