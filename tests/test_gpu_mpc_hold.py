"""GPU tests of f16_rollout_mpc_hold / f16_rollout_mpc_relin_hold / F16Batch.rollout_MPC(ctrl_every=k): the closed MPC loops at a
control period of k plant steps, as one launch.

Shapes unless said otherwise: N = 10, plant dt 1e-3, 4 control steps, OSQP's defaults, xcg 0.35.  The checkers:
  - hold = 1: the existing calls f16_rollout_mpc / f16_rollout_mpc_relin, bit for bit;
  - the host loop  f16_mpc_plan_solve + f16_rollout(hold, flags | F16_FLAG_ONE_LANE)  per control step, bit for bit;
  - the CPU twin composed from the C oracle: linearise_na + c2d(hold x dt) once, then mpc_qp(dt = hold x dt) + admm(mode=2) +
    rollout(hold, dt) per control step."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401

pytestmark = pytest.mark.gpu

XCG = 0.35
DT = 1e-3
DEM = (0.02, -0.01, 0.005)
ST_MASK = 16 | 32 | 64 | 128
ENV_V = 16 | (1 << (8 + 6))                  # F16_ST_ENVELOPE | F16_ST_ENV_STATE(6) = 16400


def make_env(x, u=None, **kw):
    from f16_mpc_oop_py_amd import F16Batch
    return F16Batch(x, u, device="cuda:0", xcg=XCG, **kw)


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    b = _np(b) if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _c_hold(env, nctrl, hold, every=1, dt=DT, flags=0, dem=DEM, relin=False, model_every=1, eps=1e-5, with_traj=True):
    """f16_rollout_mpc_hold / f16_rollout_mpc_relin_hold through the C ABI on env's plan, x.values, u.values and status.
    -> (rc, traj, cmd, iters, model or None)"""
    B, dev = env.B, env.device
    d = env._demands(*dem)
    rows = max(nctrl, 1)                     # (calls that must be refused still get buffers)
    traj = torch.full((max(nctrl * hold // max(every, 1), 1), 18, B), -7.0, dtype=torch.float64, device=dev) if with_traj else None
    cmd = torch.full((rows, 3, B), -7.0, dtype=torch.float64, device=dev)
    its = torch.full((rows, B), -7, dtype=torch.int32, device=dev)
    if relin:
        model = torch.full((max(rows // max(model_every, 1), 1), 189, B), -7.0, dtype=torch.float64, device=dev)
        rc = env.lib.f16_rollout_mpc_relin_hold(env._plan, _vp(env._x), _vp(env._u), _vp(d), _vp(traj), _vp(cmd), _vp(its), _vp(model),
                                                _vp(env.status), nctrl, hold, every, model_every, dt, eps, XCG, 1, env.flags | flags,
                                                env._stream)
    else:
        model = None
        rc = env.lib.f16_rollout_mpc_hold(env._plan, _vp(env._x), _vp(env._u), _vp(d), _vp(traj), _vp(cmd), _vp(its), _vp(env.status),
                                          nctrl, hold, every, dt, XCG, 1, env.flags | flags, env._stream)
    torch.cuda.synchronize()
    return rc, traj, cmd, its, model


def _host_loop(env, nctrl, N, hold, dem=DEM, hold_command=False, **plan_kw):
    """The host loop the call equals: per control step a solve on the plan of period hold x dt (f16_mpc_plan_solve), the command into
    u.values, then f16_rollout(hold, flags | F16_FLAG_ONE_LANE).  -> (samples of EVERY plant step [nctrl x hold, 18, B], cmd, iters)"""
    from f16_mpc_oop_py_amd import lib as L
    env.flags |= L.F16_FLAG_ONE_LANE
    if getattr(env, "_plan", None) is None:
        env.prepare_MPC(N, ctrl_every=hold, **plan_kw)
    cmds, its, trs = [], [], []
    for _ in range(nctrl):
        cmd, info = env._calc_MPC_action(*dem, N, return_info=True, use_plan=True, ctrl_every=hold)
        cmds.append(cmd.t().clone()); its.append(info["iters"].to(torch.int32).clone())
        c = cmd.t()
        env._u[1:4] = torch.where(torch.isnan(c), env._u[1:4], c) if hold_command else c
        trs.append(env.rollout(hold, traj_every=1).clone())
    return torch.cat(trs), torch.stack(cmds), torch.stack(its)


@pytest.fixture(scope="module")
def states256():
    from f16_mpc_oop_py_amd.workload import config4_states
    return config4_states(256)


@pytest.mark.timeout(300, method="thread")      # (a persistent kernel that never drains must fail the run, not hold it)
def test_hold_one_is_the_existing_call_bit_for_bit(states256):
    """f16_rollout_mpc_hold(hold = 1, dt = the plan's dt) against f16_rollout_mpc, and the re-linearised pair (model_every =
    traj_every = 2): x, u, status, traj, cmd_traj, iters_traj, model_traj identical."""
    x0, u0 = states256
    N, T = 10, 4
    ea, eb = make_env(x0, u0), make_env(x0, u0)
    for e in (ea, eb):
        e.build_ssr(); e.prepare_MPC(N)
    tra, infa = ea.rollout_MPC(T, *DEM, N, traj_every=1, return_info=True)
    rc, trb, cb, ib, _ = _c_hold(eb, T, 1)
    assert rc == 0, eb.lib.f16_last_error()
    assert _same(tra, trb) and _same(infa["cmd"], cb) and _same(infa["iters"], ib)
    assert _same(ea._x, eb._x) and _same(ea._u, eb._u) and _same(ea.status, eb.status)
    assert int(ib.min()) >= 25 and bool(torch.isfinite(trb).all())
    ea, eb = make_env(x0, u0), make_env(x0, u0)
    for e in (ea, eb):
        e.build_ssr(); e.prepare_MPC(N)
    tra, infa = ea.rollout_MPC(T, *DEM, N, traj_every=2, return_info=True, relinearise=True)
    rc, trb, cb, ib, mb = _c_hold(eb, T, 1, every=2, relin=True, model_every=2)
    assert rc == 0, eb.lib.f16_last_error()
    assert tuple(mb.shape) == (2, 189, 256) and _same(infa["model"], mb) and bool(torch.isfinite(mb).all())
    assert _same(tra, trb) and _same(infa["cmd"], cb) and _same(infa["iters"], ib)
    assert _same(ea._x, eb._x) and _same(ea._u, eb._u) and _same(ea.status, eb.status)


def _fused_vs_host(x0, u0, N, nctrl, hold, every, hold_command=False, **plan_kw):
    from f16_mpc_oop_py_amd import lib as L
    B = x0.shape[0]
    envh = make_env(x0, u0)
    envh.build_ssr()
    trh, ch, ih = _host_loop(envh, nctrl, N, hold, hold_command=hold_command, **plan_kw)
    envf = make_env(x0, u0)
    envf.build_ssr(); envf.prepare_MPC(N, ctrl_every=hold, **plan_kw)
    rc, trf, cf, itf, _ = _c_hold(envf, nctrl, hold, every=every, flags=L.F16_FLAG_HOLD_COMMAND if hold_command else 0)
    assert rc == 0, envf.lib.f16_last_error()
    assert tuple(trf.shape) == (nctrl * hold // every, 18, B) and tuple(cf.shape) == (nctrl, 3, B)
    sf, sh = _np(envf.status), _np(envh.status)
    inside = torch.as_tensor((sf & 16) == 0, device="cuda:0")               # (the host loop goes on solving for a frozen aircraft)
    assert _same(trf, trh[every - 1::every]) and _same(envf._x, envh._x)     # every sample and the state, frozen aircraft included
    assert np.array_equal(sf, sh)
    assert _same(cf[:, :, inside], ch[:, :, inside]) and _same(itf[:, inside], ih[:, inside]) and _same(envf._u[:, inside], envh._u[:, inside])
    assert _same(trf[-1], envf._x) and int(inside.sum()) >= B - 1 and int(itf[0].min()) >= 25      # (solves that iterate)
    return envf, envh, (trf, cf, itf)


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("hold,B,nctrl,every", [(2, 1, 4, 1), (2, 100, 4, 1), (2, 256, 4, 1), (5, 1, 4, 1), (5, 100, 4, 1), (5, 256, 4, 1),
                                                (5, 100, 3, 1), (5, 100, 3, 3)])
def test_one_launch_equals_the_host_loop_bit_for_bit(states256, hold, B, nctrl, every):
    """States, commands, iteration counts, every sample and the status words against f16_mpc_plan_solve + f16_rollout(hold, flags |
    F16_FLAG_ONE_LANE) per control step.  traj_every = 3 with hold = 5 over 15 plant steps: samples that fall inside a hold and
    samples that end one."""
    x0, u0 = states256[0][:B], states256[1][:B]
    _fused_vs_host(x0, u0, 10, nctrl, hold, every)


@pytest.mark.timeout(300, method="thread")
def test_one_launch_equals_the_host_loop_with_hold_command_and_with_warm_start(states256):
    """Once with F16_FLAG_HOLD_COMMAND (config 2's flap states sit on their bounds: some QPs are infeasible, their NaN command is not
    written), once with the plan's warm start on (control step c starts from the solution of c - 1)."""
    from f16_mpc_oop_py_amd.workload import config2_states
    x0, u0 = config2_states(100, seed=3)
    envf, _, (_, cf, _) = _fused_vs_host(x0, u0, 10, 4, 5, 1, hold_command=True)
    nanc = torch.isnan(cf).any(1).any(0)
    assert 1 <= int(nanc.sum()) < 50 and not (_np(envf.status) & 32).any()   # infeasible QPs exist; held commands: everybody flies on
    x0, u0 = states256[0][:100], states256[1][:100]
    _, _, (_, _, iw) = _fused_vs_host(x0, u0, 10, 4, 5, 1, warm_start=True)
    _, _, (_, _, ic) = _fused_vs_host(x0, u0, 10, 4, 5, 1)
    assert float(iw[1:].float().mean()) < float(ic[1:].float().mean())       # warm solves are shorter


@pytest.mark.timeout(300, method="thread")
def test_envelope_exit_between_two_control_instants(oracle):
    """Config-4 aircraft 2 (seed 20261003) with x[6] = 899.984 ft/s passes V = 900 after four 1 ms plant steps, i.e. it is found
    outside at the start of plant step 4 of control step 0 (hold = 5): frozen there, the fifth step of its hold not taken, the later
    samples repeat that state, control steps 1.. carry NaN commands and 0 iterations; its neighbours do not notice.  (The aircraft is
    number 2 of config4_states(16, seed=20261003), the batch of the CPU-twin test; it flies here as number 2 of a batch of 64.)"""
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N, hold, nctrl, b = 64, 10, 5, 4, 2
    x16, u16 = config4_states(16, seed=20261003)
    x0, u0 = config4_states(B, seed=20261003)
    x0[b], u0[b] = x16[b], u16[b]
    x1 = x0.copy()
    x1[b, 6] = 899.984
    # the checker on the aircraft's own inputs: a 5-step launch is the first to raise the flag
    for T, want in ((4, 0), (5, ENV_V)):
        _, _, st = oracle.rollout(x1[b:b + 1], u0[b:b + 1], T, dt=DT, xcg=XCG, store=False)
        assert (int(st[0]) & ~15) == want, (T, int(st[0]))
    envh = make_env(x1, u0)
    envh.build_ssr()
    trh, ch, ih = _host_loop(envh, nctrl, N, hold)
    envf = make_env(x1, u0)
    envf.build_ssr(); envf.prepare_MPC(N, ctrl_every=hold)
    rc, trf, cf, itf, _ = _c_hold(envf, nctrl, hold)
    assert rc == 0, envf.lib.f16_last_error()
    # the step index again with the command the controller gave: still inside a hold (else this test would pass for nothing)
    ub = u0[b].copy()
    ub[1:4] = _np(cf[0, :, b])
    assert np.isfinite(ub).all() and int(itf[0, b]) >= 25
    first = next(T for T in range(1, 21) if int(oracle.rollout(x1[b:b + 1], ub[None], T, dt=DT, xcg=XCG, store=False)[2][0]) & 16) - 1
    assert first % hold != 0 and first < hold, f"the MPC command moved the crossing to the start of plant step {first}"
    assert (int(envf.status[b]) & ~15) == ENV_V and int(envh.status[b]) == int(envf.status[b])
    assert _same(trf[:, :, b], trh[:, :, b]) and _same(envf._x[:, b], envh._x[:, b])
    frozen = trf[first - 1, :, b]                                            # the state after `first` plant steps
    assert float(frozen[6]) > 900.0 and float(trf[first - 2, 6, b]) <= 900.0
    assert all(_same(trf[s, :, b], frozen) for s in range(first, nctrl * hold)) and _same(envf._x[:, b], frozen)
    assert bool(torch.isnan(cf[1:, :, b]).all()) and int(itf[1:, b].abs().sum()) == 0 and _same(envf._u[1:4, b], cf[0, :, b])
    # neighbours: the same batch without the edit
    envc = make_env(x0, u0)
    envc.build_ssr(); envc.prepare_MPC(N, ctrl_every=hold)
    rc, trc, cc, ic, _ = _c_hold(envc, nctrl, hold)
    others = [k for k in range(B) if k != b]
    assert rc == 0 and _same(trf[:, :, others], trc[:, :, others]) and _same(cf[:, :, others], cc[:, :, others])
    assert _same(itf[:, others], ic[:, others]) and _same(envf.status[others], envc.status[others])
    assert _same(trf[:, :, others], trh[:, :, others]) and _same(cf[:, :, others], ch[:, :, others]) and _same(itf[:, others], ih[:, others])


def cpu_twin(oracle, x0, u0, N, nctrl, hold, dem=(0.0, 0.0, 0.0)):
    """The loop on the C oracle, per aircraft: linearise_na + c2d(hold x dt) once; per control step mpc_qp(dt = hold x dt) +
    admm(mode=2) + rollout(hold, dt), with the product's rules for frozen, non-finite and infeasible aircraft (those of
    oracle/f16_mpc_oracle.c: f16o_mpc_closed_loop).  -> (x [B,18], cmd [nctrl,B,3], iters [nctrl,B], status [B])"""
    B = x0.shape[0]
    xs, cmds, its, sts = np.zeros((B, 18)), np.full((nctrl, B, 3), np.nan), np.zeros((nctrl, B), dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        x, u, st = x0[b].copy(), u0[b].copy(), 0
        A, Bm, C, _ = oracle.linearise_na(x, u3=u[1:4], xcg=XCG)
        Ad, Bd = oracle.c2d(A, Bm, hold * DT)
        for c in range(nctrl):
            if st & 16:
                continue
            if np.isfinite(x[[3, 4, 7, 8, 9, 10, 11, 17, 16, 13, 14, 15]]).all():
                r = oracle.admm(*oracle.mpc_qp(x, Ad, Bd, C, N, hold * DT, dem), mode=2)
                its[c, b] = r["iters"]
                st |= 128 if r["status"] == 2 else (64 if r["status"] != 0 else 0)
                cmds[c, b] = np.nan if r["status"] == 2 else r["x"][:3]
            else:
                st |= 32
            u[1:4] = cmds[c, b]
            xn, _, s = oracle.rollout(x[None], u[None], hold, dt=DT, xcg=XCG, store=False)
            x, st = xn[0], st | int(s[0])
            if not np.isfinite(x).all():
                st |= 32
        xs[b], sts[b] = x, st
    return xs, cmds, its, sts


@pytest.mark.timeout(300, method="thread")
def test_one_launch_vs_the_cpu_twin(oracle):
    """16 config-4 states (seed 20261003), hold = 5, demands 0, against the loop composed from the C oracle.  On the CPU 15 of the 16
    are solved at all four control steps (150 to 675 iterations); aircraft 0 is certified infeasible at control step 0 and turns NaN.
    At least 14 of 16 are compared at every control step, nobody is dropped for another reason than QP_INFEASIBLE / NONFINITE on BOTH
    sides, the status words of all 16 agree.  Bands: those of test_config5_full_shard_through_both_loops_vs_the_cpu_chain, which
    compares the same two implementations at hold = 1 -- every iteration count equal, commands <= 5e-5, states <= 1e-6 (relative to
    max(1, |x|)); the models differ as there (the device's linearisation against the oracle's).  Measured: all 64 counts equal,
    commands within 9.1e-10, states within 2.7e-10."""
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N, hold, nctrl = 16, 10, 5, 4
    x0, u0 = config4_states(B, seed=20261003)
    xc, cc, ic, sc = cpu_twin(oracle, x0, u0, N, nctrl, hold)
    env = make_env(x0, u0)
    env.build_ssr()
    _, info = env.rollout_MPC(nctrl * hold, 0.0, 0.0, 0.0, N, return_info=True, ctrl_every=hold)
    cg, ig, sg, xg = _np(info["cmd"]).transpose(0, 2, 1), _np(info["iters"]), _np(env.status), _np(env.x_values)
    print("status (GPU):", sg.tolist(), "\nstatus (CPU):", sc.tolist())
    print("iterations (GPU):", ig.tolist(), "\niterations (CPU):", ic.tolist())
    assert np.array_equal(sg & ST_MASK, sc & ST_MASK)
    dropped = ((sg & (128 | 32)) != 0) & ((sc & (128 | 32)) != 0)           # flagged on BOTH sides: NaN from there on
    keep = ~dropped
    assert keep.sum() >= 14
    assert np.array_equal(np.isnan(cg), np.isnan(cc)) and np.array_equal(np.isnan(xg), np.isnan(xc))
    e_cmd = float(np.abs(cg[:, keep] - cc[:, keep]).max())
    e_x = float(np.max(np.abs(xg[keep] - xc[keep]) / np.maximum(1.0, np.abs(xc[keep]))))
    print(f"compared {int(keep.sum())} of {B}; counts equal: {np.array_equal(ig, ic)}; max |dcmd| {e_cmd:.3e}; max rel dx {e_x:.3e}")
    assert np.array_equal(ig, ic)                                            # all 16, the dropped ones included
    assert ic[:, keep].min() >= 25 and e_cmd <= 5e-5 and e_x <= 1e-6


@pytest.mark.timeout(300, method="thread")
def test_relinearised_variant_model_solve_and_host_loop(states256):
    """f16_rollout_mpc_relin_hold, B = 64, hold = 5, model_every = 1.
      - model_traj[c] against f16_linearise_batch -> f16_c2d_batch(dt = 5e-3) at the state before control step c and the command of
        c - 1: within 1e-9 (the band of tests/test_gpu_mpc_relin.py for the model against build_ssr(): the loop differentiates through
        the out-of-line plant evaluation, f16_linearise_batch through the inlined one);
      - f16_mpc_batch_w on the stored model, that state and the demands with dt = 5e-3 returns cmd_traj[c] and iters_traj[c] exactly;
      - the re-linearised host loop of dist.closed_loop_mpc_rollout: the step-0 model within 1e-9 is asserted, the share of equal
        count sequences and the largest command difference are printed (as test_relin_loop_vs_the_host_loop_step0_model does)."""
    from f16_mpc_oop_py_amd import dist, lib as L
    B, N, hold, nctrl = 64, 10, 5, 4
    x0, u0 = states256[0][:B], states256[1][:B]
    env = make_env(x0, u0)
    env.build_ssr()
    traj, info = env.rollout_MPC(nctrl * hold, *DEM, N, traj_every=hold, return_info=True, relinearise=True, ctrl_every=hold)
    cmd, its, model = info["cmd"], info["iters"], info["model"]
    assert tuple(model.shape) == (nctrl, 189, B) and tuple(traj.shape) == (nctrl, 18, B) and env._plan_foreign
    assert not (_np(env.status) & ~(15 | 32 | 128)).any()                    # (nothing but infeasible QPs and what follows: NaN states, clamped lookups)
    nosolve = torch.isnan(model).any(1)                                      # [nctrl,B]: pairs without a solve store a NaN model
    flagged = torch.as_tensor((_np(env.status) & (32 | 128)) != 0, device="cuda:0")
    assert not bool(nosolve[0].any()) and not bool(nosolve[:, ~flagged].any())      # every pair without a solve has its flag
    assert float(nosolve.any(0).double().mean()) <= 0.25                     # ... and three aircraft in four are solved for throughout
    x0s, u0s = torch.as_tensor(np.ascontiguousarray(x0.T), device="cuda:0"), torch.as_tensor(np.ascontiguousarray(u0.T), device="cuda:0")
    xs = [x0s] + [traj[c] for c in range(nctrl - 1)]
    u = u0s
    d_model = 0.0
    for c in range(nctrl):
        ok = ~nosolve[c]
        xc, uc, m = xs[c].clone(), u.clone(), model[c].clone()
        xc[:, ~ok], uc[:, ~ok], m[:, ~ok] = x0s[:, :1], u0s[:, :1], model[0][:, :1]      # a finite stand-in: not compared
        e = make_env(_np(xc).T.copy(), _np(uc).T.copy())
        e.dt = hold * DT                                                     # build_ssr = f16_linearise_batch -> f16_c2d_batch(e.dt)
        Ad, Bd, Cd = e.build_ssr()
        d_model = max(d_model, float((torch.cat([Ad, Bd, Cd]) - m).abs().max()))
        e.ssr = (m[:81].contiguous(), m[81:108].contiguous(), m[108:].contiguous())
        cc, inf = e._calc_MPC_action(*DEM, N, return_info=True)             # f16_mpc_batch_w with dt = e.dt
        assert _same(cc.t()[:, ok], cmd[c][:, ok]) and _same(inf["iters"].to(torch.int32)[ok], its[c][ok]), c
        assert bool(torch.isnan(cmd[c][:, ~ok]).all()) and int(its[c][~ok].abs().sum()) == 0      # the stated rule
        u = u.clone()
        u[1:4] = cmd[c]
    print(f"pairs without a solve: {int(nosolve.sum())} of {nctrl * B}; model_traj vs f16_linearise_batch -> f16_c2d_batch(5e-3): max abs diff {d_model:.3e}")
    assert d_model <= 1e-9
    # the stored model is a model at the control period: not the one of a 1 ms step
    e1 = make_env(x0, u0)
    assert float((torch.cat(e1.build_ssr()[:2]) - model[0][:108]).abs().max()) > 1e-4
    # the host loop of dist.closed_loop_mpc_rollout(relinearise=True, ctrl_every=5)
    eh = make_env(x0, u0, flags=L.F16_FLAG_ONE_LANE)
    dem = eh._demands(*DEM)
    cmds, itsh = [], []
    for c in range(nctrl):
        ch = dist._relin_action_at_period(eh, dem, N, hold * DT)
        if c == 0:
            Ac, Bc, Cc = eh._lin
            Ad0, Bd0 = torch.empty_like(Ac), torch.empty_like(Bc)
            assert eh.lib.f16_c2d_batch(eh.ctx.handle, _vp(Ac), _vp(Bc), _vp(Ad0), _vp(Bd0), B, B, hold * DT, eh._stream) == 0
            m0 = torch.cat([Ad0, Bd0, Cc]).clone()
        cmds.append(ch.t().clone()); itsh.append(eh.last_iters.to(torch.int32).clone())
        eh._u[1:4] = ch.t()
        eh.rollout(hold)
    d0 = float((m0 - model[0]).abs().max())
    seq_equal = float((torch.stack(itsh) == its).all(0).double().mean())
    dcmd = float((torch.stack(cmds) - cmd).abs().nan_to_num(0.0).max())
    print(f"host loop: step-0 model max abs diff {d0:.3e}; aircraft with equal count sequences {seq_equal:.4f}; max |dcmd| {dcmd:.3e}")
    assert d0 <= 1e-9
    eh2 = make_env(x0, u0)
    trh = dist.closed_loop_mpc_rollout(eh2, nctrl * hold, N, *DEM, traj_every=hold, gather=False, fused=False, one_lane=True,
                                       relinearise=True, ctrl_every=hold)
    assert _same(eh2._x, eh._x) and _same(trh[-1], eh._x) and tuple(trh.shape) == (nctrl, 18, B)


@pytest.mark.timeout(300, method="thread")
def test_hold_argument_checks_and_foreign_plans(states256):
    x0, u0 = states256[0][:8], states256[1][:8]
    env = make_env(x0, u0)
    env.build_ssr(); env.prepare_MPC(10, ctrl_every=5)
    before = env.x_values.clone()
    EINVAL = -1
    for relin in (False, True):
        call = lambda **kw: _c_hold(env, kw.pop("nctrl", 2), kw.pop("hold", 5), relin=relin, **kw)[0]
        assert call(hold=0) == EINVAL and call(hold=-1) == EINVAL and call(nctrl=0) == EINVAL and call(nctrl=-2) == EINVAL
        assert call(dt=DT * (1 + 1e-6)) == EINVAL and b"plan" in env.lib.f16_last_error()      # hold x dt off the plan's period
        assert call(dt=DT * (1 - 1e-6)) == EINVAL and call(hold=1) == EINVAL and call(hold=4) == EINVAL and call(dt=float("nan")) == EINVAL
        assert call(nctrl=2, every=3) == EINVAL and call(every=0) == EINVAL                    # 10 plant steps
        if relin:
            assert call(model_every=0) == EINVAL and call(nctrl=3, model_every=2) == EINVAL
            assert call(eps=0.0) == EINVAL and call(eps=float("nan")) == EINVAL
    assert env.lib.f16_rollout_mpc_hold(None, None, None, None, None, None, None, None, 1, 1, 1, DT, XCG, 1, 0, None) == EINVAL
    assert bool((env.x_values == before).all()) and int(env.status.max()) == 0
    # hold x dt within 1e-12 relative of the plan's period is the plan's period
    assert _c_hold(env, 1, 5, dt=DT * (1 + 1e-13))[0] == 0
    # a foreign plan: refused by the frozen call, taken by the re-linearised one
    assert _c_hold(env, 1, 5, relin=True)[0] == 0
    assert _c_hold(env, 1, 5)[0] == EINVAL and b"model" in env.lib.f16_last_error()
    assert _c_hold(env, 1, 5, relin=True)[0] == 0
    env.prepare_MPC(10, ctrl_every=5, settings=dict(scaling=0, rho=0.0))     # no equilibration: not this kernel's solver
    assert _c_hold(env, 1, 5)[0] == EINVAL and b"scaling" in env.lib.f16_last_error()
    with pytest.raises(ValueError):
        env.rollout_MPC(10, *DEM, 10, ctrl_every=5)


@pytest.mark.timeout(300, method="thread")
def test_python_surface_of_the_hold_loops(states256):
    """rollout_MPC(ctrl_every=5) = the C-ABI call; rollout_MPC() without the argument = today's f16_rollout_mpc; 10 + 10 plant steps in
    two calls = 20 in one (cold start, u carried in place); dist.closed_loop_mpc_rollout(ctrl_every=5) fused = host loop; prepare_MPC
    leaves self.ssr alone and keys the plan by (hzn, ctrl_every)."""
    from f16_mpc_oop_py_amd import dist
    B, N, hold = 64, 10, 5
    x0, u0 = states256[0][:B], states256[1][:B]
    ea, eb = make_env(x0, u0), make_env(x0, u0)
    ssr = [m.clone() for m in ea.build_ssr()]
    tra, infa = ea.rollout_MPC(20, *DEM, N, traj_every=2, return_info=True, ctrl_every=hold)
    assert all(_same(a, b) for a, b in zip(ea.ssr, ssr)) and (ea._plan_hzn, ea._plan_ctrl_every) == (N, hold)
    assert tuple(tra.shape) == (10, 18, B) and tuple(infa["cmd"].shape) == (4, 3, B) and tuple(infa["iters"].shape) == (4, B)
    eb.build_ssr(); eb.prepare_MPC(N, ctrl_every=hold)
    rc, trb, cb, ib, _ = _c_hold(eb, 4, hold, every=2)
    assert rc == 0 and _same(tra, trb) and _same(infa["cmd"], cb) and _same(infa["iters"], ib) and _same(ea._x, eb._x) and _same(ea.status, eb.status)
    assert ea.rollout_MPC(5, *DEM, N, ctrl_every=hold) is None                  # no samples asked for
    # without the argument: f16_rollout_mpc as it was, on a plan of the plant's own step (the (hzn, 5) plan is replaced)
    ec = make_env(_np(ea.x_values).copy(), _np(ea.u_values).copy())
    ec.ssr = tuple(m.clone() for m in ssr)
    ec.prepare_MPC(N)
    t1, i1 = ea.rollout_MPC(4, *DEM, N, traj_every=1, return_info=True)
    assert ea._plan_ctrl_every == 1
    d = ec._demands(*DEM)
    t2 = torch.empty((4, 18, B), dtype=torch.float64, device="cuda:0")
    c2 = torch.empty((4, 3, B), dtype=torch.float64, device="cuda:0")
    i2 = torch.empty((4, B), dtype=torch.int32, device="cuda:0")
    assert ec.lib.f16_rollout_mpc(ec._plan, _vp(ec._x), _vp(ec._u), _vp(d), _vp(t2), _vp(c2), _vp(i2), _vp(ec.status), 4, 1, XCG, 1,
                                  ec.flags, ec._stream) == 0
    torch.cuda.synchronize()
    assert _same(t1, t2) and _same(i1["cmd"], c2) and _same(i1["iters"], i2) and _same(ea._x, ec._x)
    # 10 + 10 plant steps in two calls = 20 in one
    e1, e2 = make_env(x0, u0), make_env(x0, u0)
    tr1, in1 = e1.rollout_MPC(20, *DEM, N, traj_every=1, return_info=True, ctrl_every=hold)
    parts = [e2.rollout_MPC(10, *DEM, N, traj_every=1, return_info=True, ctrl_every=hold) for _ in range(2)]
    assert _same(torch.cat([p[0] for p in parts]), tr1) and _same(torch.cat([p[1]["cmd"] for p in parts]), in1["cmd"])
    assert _same(torch.cat([p[1]["iters"] for p in parts]), in1["iters"]) and _same(e1._x, e2._x) and _same(e1._u, e2._u)
    # dist: fused = the call above; host loop (one_lane) = the same samples bit for bit
    ef, eh = make_env(x0, u0), make_env(x0, u0)
    stats = {}
    trf = dist.closed_loop_mpc_rollout(ef, 20, N, *DEM, traj_every=1, gather=False, ctrl_every=hold, stats=stats)
    trh = dist.closed_loop_mpc_rollout(eh, 20, N, *DEM, traj_every=1, gather=False, ctrl_every=hold, fused=False, one_lane=True)
    assert _same(trf, tr1) and _same(trh, tr1) and _same(ef.status, eh.status) and stats["iters_mean"] == float(in1["iters"].double().mean())
    tr3 = dist.closed_loop_mpc_rollout(make_env(x0, u0), 15, N, *DEM, traj_every=3, gather=False, ctrl_every=hold, fused=False, one_lane=True)
    tf3 = dist.closed_loop_mpc_rollout(make_env(x0, u0), 15, N, *DEM, traj_every=3, gather=False, ctrl_every=hold)
    assert tuple(tr3.shape) == (5, 18, B) and _same(tr3, tf3) and _same(tr3, tr1[2:15:3])
