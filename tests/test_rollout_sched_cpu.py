"""CPU-side checks of the scheduled rollouts (f16_rollout_sched / f16_rollout_lqr_sched): the C-ABI boundary, and fixture G17
(tools/make_golden.py: g17_input_schedules -- the reference's step loop and LQR loop under inputs that change during the run)
against the C restatement chained per segment.  Tolerances: SURVEY.md 8(d), 1e-8 relative for xcg 0.25, 1e-6 for 0.35."""
import ctypes

import numpy as np
import pytest

from conftest import golden
from header_cases import header_parameters

SCHED = ("f16_rollout_sched", "f16_rollout_lqr_sched")


def rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


def test_header_library_and_binding_agree_on_the_scheduled_entry_points():
    from f16_mpc_oop_py_amd import lib
    exported = ctypes.CDLL(lib.build())
    L = lib.load()
    for name in SCHED:
        params = header_parameters(name)
        assert hasattr(exported, name), f"libf16hip.so does not export {name}"
        assert len(getattr(L, name).argtypes) == len(params), (name, params)
    # the schedule arguments sit where the header says: `hold` in front of `traj_every`, one more int than the constant-input call
    for name, base in zip(SCHED, ("f16_rollout", "f16_rollout_lqr")):
        p, q = header_parameters(name), header_parameters(base)
        assert len(p) == len(q) + 1 and "int hold" in p and p.index("int hold") + 1 == p.index("int traj_every")
        assert [t for t in getattr(L, name).argtypes].count(ctypes.c_int) == [t for t in getattr(L, base).argtypes].count(ctypes.c_int) + 1


def chained(oracle, x0, useq, hold, nsteps, every, xcg):
    """the restated step path, one oracle.rollout per segment with that segment's row -> samples [B, nsteps / every, 18], status"""
    x, out, st = np.array(x0), [], np.zeros(len(x0), dtype=np.int32)
    for r in range((nsteps + hold - 1) // hold):
        n = min(hold, nsteps - r * hold)
        x, tr, s = oracle.rollout(x, useq[r], n, xcg=xcg)
        out.append(tr)
        st |= s
    tr = np.concatenate(out)                                       # [nsteps, B, 18]
    return tr[every - 1::every].transpose(1, 0, 2), st


@pytest.mark.parametrize("xcg,tol", [(25, 1e-8), (35, 1e-6)])
def test_g17_step_loop_under_a_schedule_vs_the_chained_restatement(oracle, xcg, tol):
    g = golden("g17_input_schedules.npz")
    x0 = g[f"x0_xcg{xcg}"]
    tr, st = chained(oracle, x0, g[f"doublet_u_xcg{xcg}"], 100, 1000, 25, xcg / 100)
    assert rel(tr, g[f"doublet_traj_xcg{xcg}"]) < tol and not st.any()
    # the schedule matters: held inputs end somewhere else (a schedule that is ignored cannot pass)
    held, _ = chained(oracle, x0, g[f"doublet_u_xcg{xcg}"][:1], 1000, 1000, 25, xcg / 100)
    assert rel(held[:, -1], g[f"doublet_traj_xcg{xcg}"][:, -1]) > 0.1
    tr, st = chained(oracle, x0, g[f"sin_u_xcg{xcg}"], 1, 300, 25, xcg / 100)
    assert rel(tr, g[f"sin_traj_xcg{xcg}"]) < tol and not st.any()


@pytest.mark.parametrize("xcg,tol", [(25, 1e-8), (35, 1e-6)])
def test_g17_lqr_loop_under_a_demand_schedule_vs_the_chained_restatement(oracle, xcg, tol):
    g, g12 = golden("g17_input_schedules.npz"), golden("g12_lqr_loop.npz")
    K, u0 = g12[f"K_xcg{xcg}"], g12[f"u0_xcg{xcg}"]
    x, out, st = np.array(g12[f"x0_xcg{xcg}"]), [], np.zeros(6, dtype=np.int32)
    for r in range(6):
        x, tr, ul, s = oracle.rollout_lqr(x, u0, K, g["dem_rows"][:, r], 50, xcg=xcg / 100)
        out.append(tr)
        st |= s
    tr = np.concatenate(out)[24::25].transpose(1, 0, 2)
    assert rel(tr, g[f"lqr_traj_xcg{xcg}"]) < tol and not st.any()
    assert rel(ul, g[f"lqr_u_last_xcg{xcg}"]) < tol
