"""CPU-side checks of the closed loops under a demand schedule (f16_rollout_mpc_sched / f16_rollout_mpc_relin_sched /
f16_rollout_lqr_relin_sched): the C-ABI boundary, the argument checks of F16Batch.rollout_MPC(dem_every=...),
F16Batch.rollout_LQR_relin(hold=...) and dist.closed_loop_mpc_rollout(dem_every=...) that come before any GPU call, and the fitness
of the inputs of the CPU-twin test of tests/test_gpu_mpc_sched.py (a condition on the oracle alone)."""
import ctypes

import numpy as np
import pytest
import torch

from header_cases import header_parameters

XCG = 0.35
DT = 1e-3
SCHED = {"f16_rollout_mpc_sched": "f16_rollout_mpc_hold", "f16_rollout_mpc_relin_sched": "f16_rollout_mpc_relin_hold",
         "f16_rollout_lqr_relin_sched": "f16_rollout_lqr_relin"}
TWIN_ROWS = ((0.0, 0.0, 0.0), (0.02, -0.01, 0.005), (-0.02, 0.01, -0.005))      # the schedule of the CPU-twin test: 6 control steps, dem_hold 2


def test_header_library_and_binding_agree_on_the_scheduled_closed_loops():
    from f16_mpc_oop_py_amd import lib
    exported = ctypes.CDLL(lib.build())
    L = lib.load()
    for name, base in SCHED.items():
        p, q = header_parameters(name), header_parameters(base)
        assert hasattr(exported, name), f"libf16hip.so does not export {name}"
        args, bargs = list(getattr(L, name).argtypes), list(getattr(L, base).argtypes)
        assert len(args) == len(p) == len(q) + 1, (name, p)
        if "mpc" in name:
            # the base call's list with dem -> dem_seq and `int dem_hold` directly behind `int hold`
            assert p.index("int dem_hold") == p.index("int hold") + 1 and "const double *dem_seq" in p
            assert [a for a in p if a != "int dem_hold"] == [("const double *dem_seq" if a == "const double *dem" else a) for a in q]
            k = p.index("int dem_hold")
        else:
            # f16_rollout_lqr_relin's list with x_ref -> xref_seq and `int hold` directly behind `int nsteps`
            assert p.index("int hold") == p.index("int nsteps") + 1 and "const double *xref_seq" in p
            assert [a for a in p if a != "int hold"] == [("const double *xref_seq" if a == "const double *x_ref" else a) for a in q]
            k = p.index("int hold")
        assert args[k] is ctypes.c_int and args[:k] + args[k + 1:] == bargs


def bare_env(B=4):
    """no GPU, no state: anything past the argument checks raises AttributeError (B and the device are all a demand history needs)"""
    from f16_mpc_oop_py_amd import F16Batch
    env = F16Batch.__new__(F16Batch)
    env.B, env.device = B, torch.device("cpu")
    return env


def test_schedule_argument_checks_come_before_any_gpu_call():
    from f16_mpc_oop_py_amd import dist
    env = bare_env(4)
    h6, h3, h2 = np.linspace(-0.02, 0.02, 6), np.zeros(3), np.zeros((2, 4))
    for kw in ({}, dict(relinearise=True), dict(ctrl_every=5), dict(ctrl_every=5, relinearise=True)):
        n = 6 * kw.get("ctrl_every", 1)                                        # six control steps
        with pytest.raises(ValueError, match="dem_every"):
            env.rollout_MPC(n, 0.0, 0.0, 0.0, 10, dem_every=2, **kw)           # no history
        with pytest.raises(ValueError, match="dem_every"):
            env.rollout_MPC(n, np.zeros(4), 0.0, 0.0, 10, dem_every=2, **kw)   # [B] is a constant demand per aircraft
        with pytest.raises(ValueError, match="dem_every"):
            env.rollout_MPC(n, h6, 0.0, 0.0, 10, dem_every=0, **kw)
        with pytest.raises(ValueError, match="dem_every"):
            env.rollout_MPC(n, 0.0, 0.0, 0.0, 10, dem_every=0, **kw)
        with pytest.raises(ValueError, match="rows"):
            env.rollout_MPC(n, h3, 0.0, 0.0, 10, **kw)                         # six rows needed
        with pytest.raises(ValueError, match="rows"):
            env.rollout_MPC(n, 0.0, h2, 0.0, 10, dem_every=2, **kw)            # three rows needed, [2, B] given
        with pytest.raises(ValueError, match="agree"):
            env.rollout_MPC(n, h6, h3, 0.0, 10, **kw)                          # histories of different lengths
        with pytest.raises(ValueError, match="agree"):
            env.rollout_MPC(n, h6, 0.0, np.zeros((6, 3)), 10, **kw)            # [S, 3] for four aircraft
        with pytest.raises(AttributeError):
            env.rollout_MPC(n, h6, 0.0, 0.0, 10, **kw)                         # enough rows: on to the plan
        with pytest.raises(AttributeError):
            env.rollout_MPC(n, h3, 0.0, h2[:1].repeat(3, 0), 10, dem_every=2, **kw)
    with pytest.raises(ValueError, match="hold"):
        env.rollout_LQR_relin(12, x_ref=np.zeros((3, 9, 4)), hold=0)
    with pytest.raises(ValueError, match="hold"):
        env.rollout_LQR_relin(12, hold=0)
    with pytest.raises(ValueError, match="hold"):
        env.rollout_LQR_relin(12, x_ref=np.zeros((4, 9)), hold=4)              # hold without a schedule
    with pytest.raises(ValueError, match="rows"):
        env.rollout_LQR_relin(12, x_ref=np.zeros((2, 9, 4)), hold=4)
    with pytest.raises(ValueError, match=r"\[S, 9, 4\]"):
        env.rollout_LQR_relin(12, x_ref=np.zeros((3, 4, 9)), hold=4)
    with pytest.raises(AttributeError):
        env.rollout_LQR_relin(12, x_ref=np.zeros((3, 9, 4)), hold=4)
    for fused in (True, False):
        for kw in ({}, dict(ctrl_every=5)):
            n = 6 * kw.get("ctrl_every", 1)
            with pytest.raises(ValueError, match="dem_every"):
                dist.closed_loop_mpc_rollout(env, n, 10, 0.0, 0.0, 0.0, dem_every=2, fused=fused, **kw)
            with pytest.raises(ValueError, match="dem_every"):
                dist.closed_loop_mpc_rollout(env, n, 10, h6, 0.0, 0.0, dem_every=0, fused=fused, **kw)
            with pytest.raises(ValueError, match="rows"):
                dist.closed_loop_mpc_rollout(env, n, 10, h3, 0.0, 0.0, fused=fused, **kw)
            with pytest.raises(ValueError, match="agree"):
                dist.closed_loop_mpc_rollout(env, n, 10, h6, h3, 0.0, fused=fused, **kw)
            with pytest.raises(AttributeError):
                dist.closed_loop_mpc_rollout(env, n, 10, h6, 0.0, 0.0, fused=fused, **kw)


def test_demand_rows_of_a_control_step():
    """_mpc_demand_rows: [S] and [S, B] histories and scalars mixed -> [S, 3, B]; a ready [3, B] block stays a constant demand."""
    env = bare_env(4)
    p, q = np.arange(3.0), np.arange(12.0).reshape(3, 4)
    seq, k = env._mpc_demand_rows(p, q, 0.5, 2, 6)
    assert k == 2 and tuple(seq.shape) == (3, 3, 4) and seq.is_contiguous()
    assert np.array_equal(seq[:, 0].numpy(), np.repeat(p[:, None], 4, 1)) and np.array_equal(seq[:, 1].numpy(), q)
    assert bool((seq[:, 2] == 0.5).all())
    assert env._mpc_demand_rows(p, q, 0.5, None, 3)[1] == 1                    # default: a row per control step
    assert env._mpc_demand_rows(p, q, 0.5, 2, 5)[0].shape[0] == 3              # a shorter last segment
    assert env._mpc_demand_rows(torch.zeros(3, 4), None, None, None, 6) == (None, None)
    assert env._mpc_demand_rows(0.0, np.zeros(4), 0.0, None, 6) == (None, None)


def cpu_twin_sched(oracle, x0, u0, N, nctrl, hold, rows, dem_hold):
    """The loop on the C oracle under a schedule, per aircraft: tests/test_gpu_mpc_hold.py's cpu_twin with dem = rows[c // dem_hold]
    (linearise_na + c2d(hold x dt) once; per control step mpc_qp(dt = hold x dt) + admm(mode=2) + rollout(hold, dt), with the product's
    rules for frozen, non-finite and infeasible aircraft).  -> (x [B,18], cmd [nctrl,B,3], iters [nctrl,B], status [B])"""
    B = x0.shape[0]
    xs, cmds, its, sts = np.zeros((B, 18)), np.full((nctrl, B, 3), np.nan), np.zeros((nctrl, B), dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        x, u, st = x0[b].copy(), u0[b].copy(), 0
        A, Bm, C, _ = oracle.linearise_na(x, u3=u[1:4], xcg=XCG)
        Ad, Bd = oracle.c2d(A, Bm, hold * DT)
        for c in range(nctrl):
            if st & 16:
                continue
            dem = tuple(rows[c // dem_hold])
            if np.isfinite(x[[3, 4, 7, 8, 9, 10, 11, 17, 16, 13, 14, 15]]).all() and np.isfinite(dem).all():
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


_TWIN = {}


def twin_inputs(oracle, hold):
    """(x0, u0, result of cpu_twin_sched under TWIN_ROWS, result under row 0 alone), computed once per hold and shared"""
    if hold not in _TWIN:
        from f16_mpc_oop_py_amd.workload import config4_states
        x0, u0 = config4_states(16, seed=20261003)
        _TWIN[hold] = (x0, u0, cpu_twin_sched(oracle, x0, u0, 10, 6, hold, TWIN_ROWS, 2),
                       cpu_twin_sched(oracle, x0, u0, 10, 6, hold, TWIN_ROWS[:1], 6))
    return _TWIN[hold]


@pytest.mark.parametrize("hold", [1, 5])
def test_inputs_of_the_cpu_twin_test_are_fit_for_it(oracle, hold):
    """config4_states(16, seed=20261003), N = 10, 6 control steps, dem_hold = 2, rows TWIN_ROWS: at least 14 of 16 aircraft stay
    unflagged by bits 32 / 128 with at least 25 iterations in every kept solve, and the commands of control steps 2..5 differ from the
    constant-row-0 run by more than 1e-2 (a schedule that is ignored cannot pass the twin test).  The issue's figures: hold = 1 keeps
    16, hold = 5 keeps 15 (aircraft 0 infeasible at control step 0), fewest iterations 125, command difference 0.052 / 0.059."""
    _, _, (xs, cmd, its, st), (_, cmd0, its0, st0) = twin_inputs(oracle, hold)
    keep = (st & (32 | 128)) == 0
    both = keep & ((st0 & (32 | 128)) == 0)
    diff = float(np.abs(cmd[2:, both] - cmd0[2:, both]).max())
    print(f"hold {hold}: kept {int(keep.sum())} of 16; fewest iterations {int(its[:, keep].min())}; max |dcmd| vs row 0 alone {diff:.3e}")
    assert keep.sum() >= 14 and both.sum() >= 14
    assert its[:, keep].min() >= 25 and np.isfinite(xs[keep]).all() and np.isfinite(cmd[:, keep]).all()
    assert diff > 1e-2
    assert np.array_equal(cmd[:2], cmd0[:2], equal_nan=True) and np.array_equal(its[:2], its0[:2])      # the same row until control step 2

