"""CPU-side checks of the re-linearised closed MPC loop (f16_rollout_mpc_relin): the C-ABI boundary, the argument checks of
F16Batch.rollout_MPC(relinearise=True) that come before any GPU call, and the checker loop the GPU tests compose from the C oracle
(tests/test_gpu_mpc_relin.py), guarded here against the numpy pattern of tests/test_gpu_control.py::_oracle_closed_loop(relin=True)."""
import ctypes

import numpy as np
import pytest

from header_cases import header_parameters
from oracle import mpc_oracle as mo


def test_header_library_and_binding_agree_on_the_relinearised_loop():
    from f16_mpc_oop_py_amd import lib
    exported = ctypes.CDLL(lib.build())
    L = lib.load()
    p, q = header_parameters("f16_rollout_mpc_relin"), header_parameters("f16_rollout_mpc")
    assert hasattr(exported, "f16_rollout_mpc_relin"), "libf16hip.so does not export f16_rollout_mpc_relin"
    assert len(L.f16_rollout_mpc_relin.argtypes) == len(p) == len(q) + 2
    # f16_rollout_mpc's arguments with model_traj behind iters_traj and eps behind traj_every
    assert [a for a in p if a not in ("double *model_traj", "double eps")] == q
    assert p.index("double *model_traj") == p.index("int32_t *iters_traj") + 1 and p.index("double eps") == p.index("int traj_every") + 1
    assert L.f16_rollout_mpc_relin.argtypes[p.index("double eps")] is ctypes.c_double


def test_relinearise_argument_checks_come_before_any_gpu_call():
    from f16_mpc_oop_py_amd import F16Batch
    env = F16Batch.__new__(F16Batch)           # no GPU, no state: anything past the argument checks would raise AttributeError
    for kw in (dict(eps=0.0), dict(eps=-1e-5), dict(eps=float("nan"))):
        with pytest.raises(ValueError, match="eps"):
            env.rollout_MPC(10, 0.0, 0.0, 0.0, 10, relinearise=True, **kw)
    for hzn in (0, 31, 150):
        with pytest.raises(ValueError, match="hzn"):
            env.rollout_MPC(10, 0.0, 0.0, 0.0, hzn, relinearise=True)
    with pytest.raises(ValueError, match="traj_every"):
        env.rollout_MPC(10, 0.0, 0.0, 0.0, 10, traj_every=3, relinearise=True)
    with pytest.raises(ValueError, match="nsteps"):
        env.rollout_MPC(-1, 0.0, 0.0, 0.0, 10, relinearise=True)
    with pytest.raises(AttributeError):
        env.rollout_MPC(10, 0.0, 0.0, 0.0, 10, relinearise=True)


def test_composed_c_checker_loop_follows_the_numpy_pattern(oracle):
    """The loop the GPU tests take their CPU figures from -- COracle.linearise_na(x, u3=u[1:]) -> mo.c2d -> .mpc_qp -> .admm(mode=2)
    -> .rollout(..., 1) -- against the numpy pattern of _oracle_closed_loop(relin=True) (mo.mpc_qp + mo.admm_osqp) on two aircraft:
    two codes of one algorithm in fp64, so the bands are those of test_closed_loop_mpc_vs_oracle_loop (same counts, commands 1e-4,
    states 1e-6 relative)."""
    from f16_mpc_oop_py_amd.workload import config4_states
    N, steps, dem = 10, 4, (0.02, -0.01, 0.0)
    x0, u0 = config4_states(8, seed=9)
    for b in (0, 5):
        runs = {}
        for which in ("c", "numpy"):
            x, u = x0[b].copy(), u0[b].copy()
            cmds, its = [], []
            for _ in range(steps):
                A_, B_, C_, D_ = oracle.linearise_na(x, u3=u[1:], xcg=0.35)
                Ad, Bd, Cd, _ = mo.c2d(A_, B_, C_, D_, 0.001)
                if which == "c":
                    r = oracle.admm(*oracle.mpc_qp(x, Ad, Bd, Cd, N, 0.001, dem), mode=2)
                else:
                    r = mo.admm_osqp(*mo.mpc_qp(x, Ad, Bd, Cd, N, 0.001, *dem), drop_unbounded_rows=True)
                cmds.append(r["x"][:3].copy()); its.append(int(r["iters"]))
                u[1:4] = r["x"][:3]
                x, _, st = oracle.rollout(x[None], u[None], 1, xcg=0.35, store=False)
                x = x[0]
                assert st[0] == 0
            runs[which] = (x, np.array(cmds), np.array(its))
        (xc, cc, ic), (xn, cn, inn) = runs["c"], runs["numpy"]
        assert np.array_equal(ic, inn), (b, ic, inn)
        assert np.abs(cc - cn).max() < 1e-4
        assert np.max(np.abs(xc - xn) / np.maximum(1.0, np.abs(xn))) < 1e-6
        assert ic.min() >= 25 and np.abs(cc).max() > 1e-3          # (solves that iterate, commands that are not zero)
