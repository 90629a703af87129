"""GPU tests of f16_rollout_mpc_relin / F16Batch.rollout_MPC(relinearise=True): the closed MPC loop with the reduced model re-derived at
every step, as one launch.

There is no reference fixture for this loop (the reference's MPC calls the absent `osqp` package), and a trajectory-level band against
a CPU loop would have to be ~1e-2: OSQP's default tolerance leaves the first move loose and the loop feeds it back (measured on the CPU
twin alone: 1e-8 of noise on A, B moves commands by up to 3.8e-2 over ten steps with 2,553 of 2,560 iteration counts unchanged).  So
parity is checked PER STEP, from the state the device itself was in, in three links that are each tight:
  1. model link      model_traj[t] against linearise_na + c2d on the CPU at (traj[t-1], cmd_traj[t-1])         Ad, Bd <= 1e-9
  2. solve + step    f16_mpc_batch_w on model_traj[t] returns cmd_traj[t], iters_traj[t]; one F16_FLAG_ONE_LANE step returns traj[t]
                     -- bit for bit (the contract f16_rollout_mpc has with its host loop, the model handed over)
  3. solve vs CPU    mpc_qp + admm(mode=2) on the device's model: iteration counts equal, commands <= 1e-4
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401
from oracle import mpc_oracle as mo

pytestmark = pytest.mark.gpu

DEM = (0.02, -0.01, 0.0)
XCG = 0.35
IDX9 = [3, 4, 7, 8, 9, 10, 11, 17, 16]


def make_env(x, u=None, **kw):
    from f16_mpc_oop_py_amd import F16Batch
    return F16Batch(x, u, device="cuda:0", xcg=XCG, **kw)


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    b = _np(b) if torch.is_tensor(b) else np.asarray(b)
    return np.array_equal(a, b, equal_nan=True)


def _relin(x0, u0, steps, N, every=1, dem=DEM, **kw):
    env = make_env(x0, u0, **{k: kw.pop(k) for k in ("flags",) if k in kw})
    env.build_ssr()
    traj, info = env.rollout_MPC(steps, *dem, N, traj_every=every, return_info=True, relinearise=True, **kw)
    return env, traj, info


def _pre(x0, u0, traj, cmd, u_last=None, hold=False):
    """The point every step started from, state-major on the device: x_pre [T,18,B] = x0 | traj[:-1]; u_pre [T,4,B] = u.values before
    the step (thrust held; u[1:4] = the previous command, or with hold the last command that was not NaN)."""
    T = cmd.shape[0]
    dev = cmd.device
    x0s = torch.as_tensor(np.ascontiguousarray(np.asarray(x0).T), device=dev)
    u0s = torch.as_tensor(np.ascontiguousarray(np.asarray(u0).T), device=dev)
    xp = torch.cat([x0s[None], traj[:-1]], 0)
    up = torch.empty((T, 4, x0s.shape[1]), dtype=torch.float64, device=dev)
    cur = u0s.clone()
    for t in range(T):
        up[t] = cur
        c = cmd[t]
        cur = cur.clone()
        cur[1:4] = torch.where(torch.isnan(c), cur[1:4], c) if hold else c
    return xp, up


def _solve_and_step_link(x0, u0, traj, info, N, dem=DEM, hold=False, frozen=()):
    """Link 2 for every pair: returns (pairs without a solve [T,B] bool, mismatches as a list).  A pair without a solve (NaN model) is
    given aircraft's step-0-style stand-in model only so that the batch call has something finite to build; its outputs are not the
    loop's and are not compared (the loop's own rule for it -- NaN command, zero iterations -- is)."""
    from f16_mpc_oop_py_amd import lib as L
    cmd, its, model = info["cmd"], info["iters"], info["model"]
    T, _, B = cmd.shape
    xp, up = _pre(x0, u0, traj, cmd, hold=hold)
    nosolve = torch.isnan(model).any(1)                                     # [T,B]
    donor = int(torch.nonzero(~nosolve[0])[0])                               # an aircraft with a model at step 0
    bad = []
    for t in range(T):
        env = make_env(_np(xp[t]).T.copy(), _np(up[t]).T.copy(), flags=L.F16_FLAG_ONE_LANE)
        m = model[t].clone()
        m[:, nosolve[t]] = model[0][:, donor:donor + 1]
        env.ssr = (m[:81].contiguous(), m[81:108].contiguous(), m[108:].contiguous())
        c, inf = env._calc_MPC_action(*dem, N, return_info=True)            # f16_mpc_batch_w: build kernel + wavefront solver
        ok = ~nosolve[t]
        if not _same(c.t()[:, ok], cmd[t][:, ok]):
            bad.append(("cmd", t, float((c.t()[:, ok] - cmd[t][:, ok]).abs().nan_to_num(1e9).max())))
        if not _same(inf["iters"].to(torch.int32)[ok], its[t][ok]):
            bad.append(("iters", t))
        assert bool(torch.isnan(cmd[t][:, nosolve[t]]).all()) and int(its[t][nosolve[t]].abs().sum()) == 0      # the stated rule
        cc = cmd[t]
        env._u[1:4] = torch.where(torch.isnan(cc), env._u[1:4], cc) if hold else cc
        env.rollout(1)
        live = torch.ones(B, dtype=torch.bool, device=cmd.device)
        for b in frozen:
            live[b] = False
        if not _same(env._x[:, live], traj[t][:, live]):
            bad.append(("x", t, float((env._x[:, live] - traj[t][:, live]).abs().nan_to_num(1e9).max())))
    return nosolve, bad


def _models(model_t):
    """model_traj row [189,B] -> (Ad [B,9,9], Bd [B,9,3], Cd [B,9,9]) on the host"""
    m = _np(model_t).T
    return m[:, :81].reshape(-1, 9, 9), m[:, 81:108].reshape(-1, 9, 3), m[:, 108:].reshape(-1, 9, 9)


@pytest.mark.timeout(900, method="thread")      # (a persistent kernel that never drains must fail the run, not hold it)
def test_relin_loop_three_links_every_pair(oracle):
    """The main case of the issue: config4_states(256, seed=9), xcg 0.35, N = 30, T = 10, OSQP defaults -- every one of the 2,560
    (step, aircraft) pairs through the three links.  Measured maxima are printed before they are asserted (and written to the file
    F16_MPC_RELIN_PARITY_JSON names, for profiles/mpc_relin_parity.json)."""
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N, T = 256, 30, 10
    x0, u0 = config4_states(B, seed=9)
    env, traj, info = _relin(x0, u0, T, N)
    cmd, its, model = info["cmd"], info["iters"], info["model"]
    assert tuple(traj.shape) == (T, 18, B) and tuple(cmd.shape) == (T, 3, B) and tuple(its.shape) == (T, B) and tuple(model.shape) == (T, 189, B)
    assert _same(traj[-1], env._x) and _same(cmd[-1], env._u[1:4])
    xp, up = _pre(x0, u0, traj, cmd)
    xph, uph = _np(xp).transpose(0, 2, 1), _np(up).transpose(0, 2, 1)        # [T,B,18], [T,B,4]
    # ---- link 2 (and the exclusions: pairs without a solve)
    nosolve, bad = _solve_and_step_link(x0, u0, traj, info, N)
    nosolve = _np(nosolve)
    print(f"pairs without a solve: {int(nosolve.sum())} of {T * B}; status words set: {int((env.status != 0).sum())}; link 2 mismatches: {bad}")
    assert nosolve.sum() <= 25
    assert not bad, bad
    # ---- link 1: the model against the CPU twin at the device's own point
    e_ad = e_bd = e_cd = 0.0
    for t in range(T):
        Ad, Bd, Cd = _models(model[t])
        for b in range(B):
            if nosolve[t, b]:
                continue
            A_, B_, C_, D_ = oracle.linearise_na(xph[t, b], u3=uph[t, b, 1:], xcg=XCG)
            Ado, Bdo, Cdo, _ = mo.c2d(A_, B_, C_, D_, 0.001)
            e_ad = max(e_ad, float(np.abs(Ad[b] - Ado).max())); e_bd = max(e_bd, float(np.abs(Bd[b] - Bdo).max()))
            e_cd = max(e_cd, float(np.abs(Cd[b] - Cdo).max()))
    print(f"link 1 (model vs CPU): max |dAd| {e_ad:.3e}  max |dBd| {e_bd:.3e}  max |dCd| {e_cd:.3e}")
    # ---- link 3: the solve against the CPU twin on the device's model and state (mpc_qp + admm(mode=2) per pair; the C loop
    # f16o_mpc_closed_loop with T = 1 runs exactly that pair of calls per aircraft, on 16 threads)
    n_eq = n_all = 0
    e_cmd = 0.0
    worst = None
    for t in range(T):
        Ad, Bd, Cd = _models(model[t])
        ok = ~nosolve[t]
        r = oracle.mpc_closed_loop(xph[t][ok], uph[t][ok], Ad[ok], Bd[ok], Cd[ok], N, 1, DEM, xcg=XCG, nthreads=16)
        ig, cg = _np(its[t])[ok], _np(cmd[t]).T[ok]
        n_eq += int((r["iters"][0] == ig).sum()); n_all += int(ok.sum())
        d = np.abs(r["cmd"][0] - cg).max(1)
        if d.max() > e_cmd:
            e_cmd, worst = float(d.max()), (t, int(np.where(ok)[0][d.argmax()]))
        if t == 0:      # the named oracle calls themselves, on a sample: the same numbers as the threaded loop
            for b in (0, 101, 255):
                P, q, A, l, uu = oracle.mpc_qp(xph[0, b], Ad[b], Bd[b], Cd[b], N, 0.001, DEM)
                s = oracle.admm(P, q, A, l, uu, mode=2)
                assert s["iters"] == int(its[0, b]) and np.abs(s["x"][:3] - _np(cmd[0])[:, b]).max() < 1e-4
    print(f"link 3 (solve vs CPU): iteration counts equal on {n_eq} of {n_all} pairs; max |dcmd| {e_cmd:.3e} at (t, b) = {worst}")
    out = os.environ.get("F16_MPC_RELIN_PARITY_JSON")
    if out:
        rec = dict(case="config4_states(256, seed=9), xcg 0.35, N 30, T 10, OSQP defaults", pairs=T * B, pairs_without_solve=int(nosolve.sum()),
                   link1_max_abs=dict(Ad=e_ad, Bd=e_bd, Cd=e_cd), link2_bitwise_mismatches=len(bad),
                   link3=dict(counts_equal=n_eq, pairs=n_all, max_abs_cmd=e_cmd))
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert e_ad <= 1e-9 and e_bd <= 1e-9
    assert n_eq == n_all
    assert e_cmd < 1e-4


@pytest.mark.timeout(600, method="thread")
def test_relin_loop_vs_the_host_loop_step0_model(oracle):
    """Against the host loop (`_calc_MPC_action(relinearise=True)` + rollout(1)), whose linearisation runs through the inlined
    k_linearise rather than the out-of-line plant evaluation: the step-0 model within 1e-9, nothing more is asserted.  Recorded only:
    the share of aircraft with equal iteration-count sequences and the largest command difference over 10 steps."""
    from f16_mpc_oop_py_amd import lib as L
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N, T = 256, 30, 10
    x0, u0 = config4_states(B, seed=9)
    env, traj, info = _relin(x0, u0, T, N)
    envh = make_env(x0, u0, flags=L.F16_FLAG_ONE_LANE)
    cmds, its = [], []
    for t in range(T):
        c, inf = envh._calc_MPC_action(*DEM, N, return_info=True, relinearise=True)
        if t == 0:
            m0 = torch.cat([envh.ssr[0], envh.ssr[1], envh.ssr[2]], 0).clone()
        cmds.append(c.t().clone()); its.append(inf["iters"].to(torch.int32).clone())
        envh._u[1:4] = c.t()
        envh.rollout(1)
    d0 = float((m0 - info["model"][0]).abs().max())
    seq_equal = float((torch.stack(its) == info["iters"]).all(0).double().mean())
    dcmd = float((torch.stack(cmds) - info["cmd"]).abs().max())
    print(f"host loop: step-0 model max abs diff {d0:.3e}; aircraft with equal count sequences {seq_equal:.4f}; max |dcmd| over {T} steps {dcmd:.3e}")
    out = os.environ.get("F16_MPC_RELIN_PARITY_JSON")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(dict(case="one launch vs host loop, same workload", step0_model_max_abs=d0,
                                    share_equal_count_sequences=seq_equal, max_abs_cmd_10_steps=dcmd)) + "\n")
    assert d0 <= 1e-9


@pytest.mark.timeout(600, method="thread")
def test_relin_loop_split_calls_and_sampling_bit_for_bit():
    """One call of 10 steps = 10 calls of one step = a 4 + 6 split (every solve starts cold, nothing is carried but x and u);
    traj_every = 5 stores rows 4 and 9 of the traj_every = 1 run, for traj and model_traj."""
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N, T = 64, 30, 10
    x0, u0 = config4_states(B, seed=9)
    env, traj, info = _relin(x0, u0, T, N)
    for split in ([1] * 10, [4, 6]):
        e2 = make_env(x0, u0)
        e2.build_ssr()
        trs, cs, ii, ms = [], [], [], []
        for k in split:
            tr, inf = e2.rollout_MPC(k, *DEM, N, traj_every=1, return_info=True, relinearise=True)
            trs.append(tr); cs.append(inf["cmd"]); ii.append(inf["iters"]); ms.append(inf["model"])
        assert _same(torch.cat(trs), traj) and _same(torch.cat(cs), info["cmd"]) and _same(torch.cat(ii), info["iters"])
        assert _same(torch.cat(ms), info["model"]) and _same(e2._x, env._x) and _same(e2._u, env._u) and _same(e2.status, env.status)
    e5, tr5, inf5 = _relin(x0, u0, T, N, every=5)
    assert tuple(tr5.shape) == (2, 18, B) and tuple(inf5["model"].shape) == (2, 189, B) and tuple(inf5["cmd"].shape) == (T, 3, B)
    assert _same(tr5, traj[[4, 9]]) and _same(inf5["model"], info["model"][[4, 9]]) and _same(inf5["cmd"], info["cmd"])
    # without samples at all: the same final state
    e0 = make_env(x0, u0)
    assert e0.rollout_MPC(T, *DEM, N, relinearise=True) is None and _same(e0._x, env._x) and _same(e0._u, env._u)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _c_relin(x0, u0, ld, N, T, model_from, flags=0, eps=1e-5):
    """f16_rollout_mpc_relin through the C ABI with a leading dimension of its own.  model_from: (Ad, Bd, Cd) [.,B] the plan is created
    from (any finite model: the call does not use it).  -> (x [18,B], u [4,B], traj, cmd, iters, model, status)"""
    from f16_mpc_oop_py_amd import lib as L
    lib = L.load()
    ctx = L.Context(0)
    B = x0.shape[0]
    dev = "cuda:0"
    pad = lambda a, rows: torch.cat([torch.as_tensor(np.ascontiguousarray(np.asarray(a).T), device=dev),
                                     torch.full((rows, ld - B), float("nan"), dtype=torch.float64, device=dev)], 1).contiguous()
    x, u = pad(x0, 18), pad(u0, 4)
    dem = torch.cat([torch.tensor(DEM, dtype=torch.float64, device=dev)[:, None].expand(3, B),
                     torch.full((3, ld - B), float("nan"), dtype=torch.float64, device=dev)], 1).contiguous()
    mdl = [torch.cat([m, torch.zeros((m.shape[0], ld - B), dtype=torch.float64, device=dev)], 1).contiguous() for m in model_from]
    plan = ctypes.c_void_p()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.f16_mpc_plan_create_w(ctx.handle, ctypes.byref(plan), _vp(mdl[0]), _vp(mdl[1]), _vp(mdl[2]), None, B, ld, N, 0.001, None, stream), lib)
    traj = torch.full((T, 18, ld), -7.0, dtype=torch.float64, device=dev)
    cmd = torch.full((T, 3, ld), -7.0, dtype=torch.float64, device=dev)
    its = torch.full((T, ld), -7, dtype=torch.int32, device=dev)
    model = torch.full((T, 189, ld), -7.0, dtype=torch.float64, device=dev)
    st = torch.zeros(ld, dtype=torch.int32, device=dev)
    try:
        L.check(lib.f16_rollout_mpc_relin(plan, _vp(x), _vp(u), _vp(dem), _vp(traj), _vp(cmd), _vp(its), _vp(model), _vp(st), T, 1, eps,
                                          XCG, 1, flags, stream), lib)
        torch.cuda.synchronize()
    finally:
        lib.f16_mpc_plan_destroy(plan)
    for a in (traj, cmd, model):                                            # nothing is written beyond column B
        assert bool((a[..., B:] == -7.0).all())
    assert bool((its[:, B:] == -7).all()) and int(st[B:].abs().sum()) == 0
    return x[:, :B], u[:, :B], traj[..., :B], cmd[..., :B], its[:, :B], model[..., :B], st[:B]


@pytest.mark.timeout(600, method="thread")
def test_relin_loop_column_of_a_padded_batch_equals_a_batch_of_one():
    """Column b of a B = 300, ld = 320 call equals a B = 1 call, bit for bit (work-queue order, stride and leading dimension do not
    enter the results); nothing is written into the padding columns."""
    from f16_mpc_oop_py_amd.workload import config4_states
    B, ld, N, T = 300, 320, 30, 4
    x0, u0 = config4_states(B, seed=9)
    e = make_env(x0, u0)
    ssr = e.build_ssr()
    big = _c_relin(x0, u0, ld, N, T, ssr)
    assert int(big[6].max()) == 0
    for b in (0, 137, 299):
        one = _c_relin(x0[b:b + 1], u0[b:b + 1], 1, N, T, [m[:, b:b + 1].contiguous() for m in ssr])
        for full, single in zip(big, one):
            assert _same(full[..., b:b + 1], single), b


@pytest.mark.timeout(600, method="thread")
def test_relin_loop_is_not_the_frozen_loop():
    """The existing frozen-against-re-linearised assertion through the one-launch paths: build_ssr() and prepare_MPC at x0, then
    rollout(200); from there the first command of f16_rollout_mpc on the frozen plan and of the re-linearised call differ by more than
    1e-6.  On a second object the step-0 model of the re-linearised call is within 1e-9 of build_ssr() at the same state (not
    bit-equal: build_ssr differentiates through the inlined k_linearise)."""
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N = 8, 10
    x0, u0 = config4_states(B, seed=9)
    dem = (0.03, 0.0, -0.01)
    cmds = {}
    for relin in (False, True):
        e = make_env(x0, u0)
        e.build_ssr(); e.prepare_MPC(N)
        e.rollout(200)
        _, inf = e.rollout_MPC(1, *dem, N, return_info=True, **(dict(relinearise=True) if relin else {}))
        assert int(e.status.max()) == 0
        cmds[relin] = inf["cmd"][0].clone()
    assert float((cmds[False] - cmds[True]).abs().max()) > 1e-6
    e = make_env(x0, u0)
    e.rollout(200)
    Ad, Bd, Cd = (m.clone() for m in e.build_ssr())
    _, inf = e.rollout_MPC(1, *dem, N, traj_every=1, return_info=True, relinearise=True)
    m0 = inf["model"][0]
    d = max(float((m0[:81] - Ad).abs().max()), float((m0[81:108] - Bd).abs().max()), float((m0[108:] - Cd).abs().max()))
    print(f"step-0 model vs build_ssr(): max abs diff {d:.3e}")
    assert d <= 1e-9


@pytest.mark.timeout(600, method="thread")
def test_relin_loop_flagged_aircraft_and_hold_command():
    """One state outside the envelope, one NaN state, one NaN demand in a small batch: status words and outputs as the header says,
    neighbours unaffected (bit-equal to a run without the three).  Then infeasible QPs (config 2's flap states sit on their bounds)
    with and without F16_FLAG_HOLD_COMMAND: every pair still obeys the solve-and-step link, NaN commands propagate or are held."""
    from f16_mpc_oop_py_amd.workload import config2_states, config4_states
    B, N, T = 16, 10, 5
    x0, u0 = config4_states(B, seed=9)
    _, traj_c, info_c = _relin(x0, u0, T, N)
    x1 = x0.copy()
    x1[3, 13] = 26.0                         # elevator outside its box on entry: frozen
    x1[7, 0] = np.nan                        # a NaN in a state the QP never reads (north position): the plant evaluation does
    dem = torch.tensor(DEM, dtype=torch.float64, device="cuda:0")[:, None].repeat(1, B)
    dem[1, 11] = float("nan")                # a NaN demand
    env = make_env(x1, u0)
    traj, info = env.rollout_MPC(T, dem, None, None, N, traj_every=1, return_info=True, relinearise=True)
    st = _np(env.status)
    for b in (3, 7, 11):
        assert np.isnan(_np(info["cmd"][:, :, b])).all() and int(info["iters"][:, b].abs().sum()) == 0 and np.isnan(_np(info["model"][:, :, b])).all()
    assert st[3] == 16 | (1 << (8 + 13)) and st[7] & 32 and st[11] & 32 and not (st[7] & 16) and not (st[11] & 16)
    assert np.array_equal(_np(env.x_values)[3], x1[3]) and np.array_equal(_np(env.u_values)[3], u0[3])        # frozen: x and u kept
    assert np.isnan(_np(env.u_values)[11, 1:]).all()                         # no command -> NaN into u.values (no hold) -> NaN states
    others = [b for b in range(B) if b not in (3, 7, 11)]
    assert (st[others] == 0).all()
    assert _same(traj[:, :, others], traj_c[:, :, others]) and _same(info["cmd"][:, :, others], info_c["cmd"][:, :, others])
    assert _same(info["iters"][:, others], info_c["iters"][:, others]) and _same(info["model"][:, :, others], info_c["model"][:, :, others])
    # ---- infeasible QPs, with and without hold
    B, T = 320, 6
    x0, u0 = config2_states(B, seed=3)
    x0[5, 13] = 26.0
    dem0 = (0.0, 0.0, 0.0)
    res = {}
    for hold in (False, True):
        env, traj, info = _relin(x0, u0, T, N, dem=dem0, hold_command=hold)
        nosolve, bad = _solve_and_step_link(x0, u0, traj, info, N, dem=dem0, hold=hold, frozen=(5,))
        assert not bad, (hold, bad)
        res[hold] = (_np(env.status), _np(env.x_values), _np(info["cmd"]), _np(info["iters"]))
        assert res[hold][0][5] == 16 | (1 << (8 + 13)) and np.array_equal(res[hold][1][5], x0[5])
    sf, xg, cg, it = res[False]
    inf = (sf & 128) != 0
    assert 3 <= inf.sum() < B // 2                                           # the workload does contain infeasible QPs
    for b in np.where(inf)[0]:
        t0 = int(np.argmax(np.isnan(cg[:, 0, b])))
        assert sf[b] & 32 and np.isnan(xg[b, 13:16]).all()                   # NaN command -> NaN surface states
        assert (it[t0 + 1:, b] == 0).all() and np.isnan(cg[t0:, :, b]).all()  # ... and nothing to linearise or solve from then on
    sfh, xgh, cgh, ith = res[True]
    assert np.isfinite(np.delete(xgh, 5, 0)).all() and not (np.delete(sfh, 5) & 32).any()      # held commands: everybody flies on
    assert ((sfh & 128) != 0).sum() >= inf.sum()


@pytest.mark.timeout(600, method="thread")
def test_relin_loop_leaves_no_plan_with_a_foreign_model():
    """Plan hygiene: the re-linearised call overwrites the model blocks of the plan it runs on.  F16Batch marks that plan and prepares
    it again before the next frozen-model call, so `_calc_MPC_action(use_plan=True)` afterwards returns exactly what a fresh object at
    the same state with the same frozen model returns; at the C level the plan refuses frozen-model calls from then on."""
    from f16_mpc_oop_py_amd import lib as L
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N = 32, 10
    x0, u0 = config4_states(B, seed=9)
    env = make_env(x0, u0)
    ssr = [m.clone() for m in env.build_ssr()]
    env.prepare_MPC(N)
    assert env._plan is not None
    env.rollout_MPC(5, *DEM, N, relinearise=True)
    assert env._plan_foreign and all(_same(a, b) for a, b in zip(env.ssr, ssr))
    c1, i1 = env._calc_MPC_action(*DEM, N, use_plan=True, return_info=True)
    assert env._plan is not None and not env._plan_foreign
    fresh = make_env(_np(env.x_values).copy(), _np(env.u_values).copy())
    fresh.ssr = tuple(m.clone() for m in ssr)
    c2, i2 = fresh._calc_MPC_action(*DEM, N, use_plan=True, return_info=True)
    assert _same(c1, c2) and _same(i1["iters"], i2["iters"]) and _same(i1["u_seq"], i2["u_seq"])
    c3 = fresh._calc_MPC_action(*DEM, N)                                    # ... which is the one-shot call on the frozen model
    assert _same(c1, c3)
    # the frozen one-launch loop after the re-linearised one: the same as on an object that never ran the latter
    ea, eb = make_env(x0, u0), make_env(x0, u0)
    for e in (ea, eb):
        e.ssr = tuple(m.clone() for m in ssr)
    ea.rollout_MPC(2, *DEM, N, relinearise=True)
    eb.set_state(_np(ea.x_values).copy()); eb.set_input(_np(ea.u_values).copy())
    ta, tb = ea.rollout_MPC(3, *DEM, N, traj_every=1), eb.rollout_MPC(3, *DEM, N, traj_every=1)
    assert _same(ta, tb)
    # C level: the plan itself
    e2 = make_env(x0, u0)
    e2.build_ssr(); e2.prepare_MPC(N)
    lib, plan = e2.lib, e2._plan
    dem = e2._demands(*DEM)
    st = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    assert lib.f16_rollout_mpc_relin(plan, _vp(e2._x), _vp(e2._u), _vp(dem), None, None, None, None, _vp(st), 2, 1, 1e-5, XCG, 1, 0, e2._stream) == 0
    ucmd = torch.empty((3, B), dtype=torch.float64, device="cuda:0")
    assert lib.f16_mpc_plan_solve_w(plan, _vp(e2._x), _vp(dem), None, _vp(ucmd), None, None, None, e2._stream) == -1        # F16_EINVAL
    assert lib.f16_rollout_mpc(plan, _vp(e2._x), _vp(e2._u), _vp(dem), None, None, None, _vp(st), 1, 1, XCG, 1, 0, e2._stream) == -1
    assert lib.f16_rollout_mpc_relin(plan, _vp(e2._x), _vp(e2._u), _vp(dem), None, None, None, None, _vp(st), 1, 1, 1e-5, XCG, 1, 0, e2._stream) == 0
    torch.cuda.synchronize()
    with pytest.raises(L.F16HipError):
        e2._calc_MPC_action(*DEM, N, use_plan=True)


@pytest.mark.timeout(300, method="thread")
def test_relin_loop_argument_checks():
    from f16_mpc_oop_py_amd import lib as L
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(8, seed=1)
    env = make_env(x0, u0)
    env.build_ssr()
    lib = env.lib
    dem = env._demands(*DEM)
    call = lambda plan, nsteps=2, every=1, eps=1e-5, traj=None, model=None: lib.f16_rollout_mpc_relin(
        plan, _vp(env._x), _vp(env._u), _vp(dem), _vp(traj), None, None, _vp(model), None, nsteps, every, eps, XCG, 1, 0, env._stream)
    assert call(None) == -1                                                  # F16_EINVAL
    env.prepare_MPC(10, settings=dict(scaling=0, rho=0.0))                   # no equilibration: not this kernel's solver
    assert call(env._plan) == -1 and b"scaling" in lib.f16_last_error()
    with pytest.raises(ValueError):
        env.rollout_MPC(2, *DEM, 10, relinearise=True)
    env.prepare_MPC(10)
    before = env.x_values.clone()
    assert call(env._plan, eps=0.0) == -1 and call(env._plan, eps=-1e-5) == -1 and call(env._plan, eps=float("nan")) == -1
    buf = torch.empty((2, 189, 8), dtype=torch.float64, device="cuda:0")
    assert call(env._plan, nsteps=3, every=2, model=buf) == -1 and call(env._plan, nsteps=3, every=2, traj=buf) == -1
    assert call(env._plan, nsteps=-1) == -1
    assert call(env._plan, nsteps=0) == 0 and bool((env.x_values == before).all())
    env.prepare_MPC(35)                                                      # beyond the wavefront solver's horizons
    assert call(env._plan) == -1
    for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan"))):
        with pytest.raises(ValueError):
            env.rollout_MPC(2, *DEM, 10, relinearise=True, **kw)
    with pytest.raises(ValueError):
        env.rollout_MPC(2, *DEM, 31, relinearise=True)
    with pytest.raises(ValueError):
        env.rollout_MPC(3, *DEM, 10, traj_every=2, relinearise=True)
    assert bool((env.x_values == before).all())


@pytest.mark.timeout(600, method="thread")
def test_relin_through_dist_closed_loop_mpc_rollout():
    """dist.closed_loop_mpc_rollout(relinearise=True): fused path = rollout_MPC(relinearise=True); host path = per step
    `_calc_MPC_action(relinearise=True)` (runs, stays unflagged and finite: against the host loop nothing beyond the step-0 model
    is asserted, see test_relin_loop_vs_the_host_loop_step0_model)."""
    from f16_mpc_oop_py_amd import dist
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N, T = 16, 10, 4
    x0, u0 = config4_states(B, seed=9)
    env, traj, info = _relin(x0, u0, T, N)
    ef = make_env(x0, u0)
    trf = dist.closed_loop_mpc_rollout(ef, T, N, *DEM, gather=False, relinearise=True)
    assert _same(trf, traj) and _same(ef._x, env._x)
    eh = make_env(x0, u0)
    trh = dist.closed_loop_mpc_rollout(eh, T, N, *DEM, gather=False, fused=False, one_lane=True, relinearise=True)
    assert tuple(trh.shape) == (T, 18, B) and int(eh.status.max()) == 0
    assert bool(torch.isfinite(trh).all())
    print(f"host path vs one launch after {T} steps: max rel state diff {float(((trh - traj).abs() / traj.abs().clamp(min=1.0)).max()):.3e}")
