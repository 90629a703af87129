"""The Runge-Kutta step rule (include/f16_hip.h: F16_INT_RK4) checked with the restatement alone (tests/rk4_cases.py; no GPU): what the
device tests of tests/test_gpu_rollout_rk4.py rest on.

(a) Restated RK4 at dt = 10 ms reproduces the Simulink time histories the reference keeps as data (fixture G10: four cases, 10 s,
    the real CLr table) inside conftest.G10_TOL; restated Euler at 10 ms is outside it in all four.  Measured, largest error /
    G10_TOL per case: Euler 1 ms (what the suite asserts elsewhere) 0.20 0.17 0.15 0.21; Euler 10 ms 1.40 1.76 1.55 1.53; RK4 10 ms
    0.17 0.10 0.13 0.16.
(b) The lattice cases are well conditioned under the RK4 step and rarely near an edge, with the caps of test_envelope_cpu.py.
    Measured (states_ok, status_ok, spread of the free aircraft): hifi 8 steps at 10 ms 1416, 1407, 2.7e-14; hifi high rates at
    1 ms 1416, 1407, 5.2e-15 over the 16 steps run here (1.7e-14 over 40); lofi 8 steps at 10 ms 568, 562, 3.2e-14.  About a
    third of the hifi aircraft raise a grid bit (503 of 1418) and five freeze."""
import numpy as np
import pytest

import envelope_cases as ec
import rk4_cases as rk
from conftest import G10_TOL, g10_case, g10_command, g10_rows_of_states


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_g10_rk4_at_10ms_is_inside_the_tolerance_and_euler_at_10ms_is_not(oracle, k):
    a, xcg, x0, trim_u, dis = g10_case(k)
    rows = np.array([[g10_command(trim_u, dis, j)] for j in range(100)])         # [100, 1, 4]: a new row every 10 steps of 10 ms
    oracle.lib.f16o_set_fix_clr(1)
    try:
        r = rk.restate(oracle, x0[None], rows, 1000, 10, 0.01, 1, xcg=xcg)
        eul, est = rk.restate_euler(oracle, x0[None], rows, 1000, 10, 0.01, 1, xcg=xcg)
    finally:
        oracle.lib.f16o_set_fix_clr(0)
    assert int(r["status"][0]) == 0 and int(est[0]) == 0
    hist = np.concatenate((x0[None], r["traj"][9::10, 0]))                       # [101, 18]: every 0.1 s
    err = np.abs(g10_rows_of_states(hist) - a[:, 1:13]).max(0)
    he = np.concatenate((x0[None], eul[9::10, 0]))
    erre = np.abs(g10_rows_of_states(he) - a[:, 1:13]).max(0)
    print(f"G10 case {k}: largest error / G10_TOL: RK4 10 ms {(err / G10_TOL).max():.2f}, Euler 10 ms {(erre / G10_TOL).max():.2f}")
    assert np.all(err < G10_TOL), err / G10_TOL
    assert (erre / G10_TOL).max() > 1.0, erre / G10_TOL
    assert np.abs(hist[:, 13:16] - a[:, 20:23]).max() < 2e-3                     # surface positions, as the Euler tests of G10 ask


def test_the_step_is_fourth_order(oracle):
    """halving dt divides the error against a fine reference by ~16 (a third-order slip would give 8, an Euler-like one 2): a
    trimmed aircraft (G10 case 0) under an elevator command 1 deg off trim -- inside the actuator's rate limit, and the 0.08 s
    flown stay inside one table cell, so f is smooth along the path"""
    _, xcg, x0, trim_u, _ = g10_case(0)
    u = (trim_u + np.array([0.0, 1.0, 0.0, 0.0]))[None, None]
    fine = rk.restate(oracle, x0[None], u, 256, 256, 0.08 / 256, 1, xcg=xcg)["x"][0]
    errs = []
    for n in (2, 4, 8):
        x = rk.restate(oracle, x0[None], u, n, n, 0.08 / n, 1, xcg=xcg)["x"][0]
        errs.append(np.abs(x - fine)[13])                                        # the elevator: 20.2 / s against dt = 40, 20, 10 ms
    print("elevator error against 256 steps:", errs)
    assert 10 < errs[0] / errs[1] < 24 and 10 < errs[1] / errs[2] < 24, errs


@pytest.mark.parametrize("name", rk.LATTICE_CASES)
def test_restated_rk4_case_is_well_conditioned_and_rarely_near_an_edge(oracle, name):
    r = rk.record(oracle, name)
    b = r["batch"]
    free = ~r["near"]
    frozen_at_start = ((b.x < ec.X_LB) | (b.x > ec.X_UB)).any(1)
    grid = int(((r["status"] & 15) != 0).sum())
    print(f"{name}: B = {b.B}, states_ok {int(r['states_ok'].sum())}, status_ok {int(r['status_ok'].sum())}, spread of the free aircraft "
          f"{r['spread'][free].max():.2e}, near-edge {int(r['near'].sum())}, with a grid bit {grid}, frozen {int(((r['status'] & 16) != 0).sum())}")
    assert np.isfinite(r["traj"]).all() and r["finite"].all()
    assert np.array_equal(frozen_at_start, (r["traj"][-1] == b.x).all(1))
    assert r["spread"][free].max() < 1e-12
    assert r["states_ok"].sum() >= b.B - 4
    assert r["status_ok"].sum() >= b.B - len(ec.ON_EDGE) - 0.005 * b.B
    # the status comparison is not vacuous: grid bits and frozen aircraft occur
    if b.fi == 1:
        assert grid > 0.2 * b.B and ((r["status"] & 16) != 0).sum() >= 5
    # a frozen aircraft has no stage states; every other one has all three of every step
    took = ~np.isnan(r["stages"]).any((1, 3))                                    # [T, B]
    assert np.array_equal(took[0], ~frozen_at_start) and (took[1:] <= took[:-1]).all()


def test_restated_rk4_equals_its_own_chain_and_ignores_rows_once_frozen(oracle):
    """the restatement itself: a schedule equals the chain of one call per segment bit for bit (nothing but the state is carried),
    and an aircraft frozen by the box test keeps its state whatever the later rows say"""
    b, rows, hold, _, _ = rk.case_inputs("hifi_sched40")
    sel = np.r_[0:40, b.B - 8:b.B]
    x0, rows = b.x[sel], rows[:, sel]
    one = rk.restate(oracle, x0, rows, 21, hold, 0.001, 1)
    x, st, parts = x0, None, []
    for s in range(3):
        p = rk.restate(oracle, x, rows[s:s + 1], 7, 7, 0.001, 1, status0=st)
        x, st = p["x"], p["raw_status"]
        parts.append(p["traj"])
    assert np.array_equal(np.concatenate(parts), one["traj"], equal_nan=True) and np.array_equal(p["status"], one["status"])
    out = x0.copy()
    out[:4, 2] = -10.0
    r = rk.restate(oracle, out, rows, 14, hold, 0.001, 1)
    assert (r["traj"][:, :4] == out[:4]).all() and (r["status"][:4] == (16 | 1 << (8 + 2))).all()
