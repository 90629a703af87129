"""Soft state rows without a GPU: the numpy twin of the soft solve (tests/mpc_soft_cases.py) against the exact minimiser of the
equivalent slack QP and against the hard twin it is derived from, and the boundary of the feature (header, library, binding, keywords)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import mpc_soft_cases as sc
from conftest import REPO
from header_cases import defines, header
from oracle import mpc_oracle as mo


@pytest.mark.parametrize("w", [1.0, 100.0, 1e4])
@pytest.mark.parametrize("tag", ["xcg25_N10", "xcg25_N30"])
def test_twin_reaches_the_exact_minimiser_of_the_slack_qp(tag, w):
    """The q-rate box moved off the prediction: the hard QP has no feasible point, the soft one is the slack QP's projection on u."""
    P, q, A, l, u = sc.fixture_qp(tag, moved=True)
    N = P.shape[0] // 3
    wr = sc.state_row_weights(w, N, A.shape[0])
    assert mo.admm_osqp(P, q, A, l, u, drop_unbounded_rows=True)["infeasible"]
    xs, _ = mo.qp_exact(*sc.slack_qp(P, q, A, l, u, wr))
    tight = sc.admm_osqp_soft(P, q, A, l, u, wr, eps_abs=1e-9, eps_rel=1e-9, max_iter=400000)
    err = np.abs(tight["x"] - xs[:3 * N]).max()
    print(f"{tag} w={w:g}: |twin - exact| = {err:.3g} after {tight['iters']} iterations")
    assert tight["converged"] and err < 1e-5           # (the bound of the hard solvers' tight-tolerance tests; measured <= 3.6e-7)
    dflt = sc.admm_osqp_soft(P, q, A, l, u, wr)
    assert dflt["converged"] and not dflt["infeasible"] and dflt["soft_active"]


@pytest.mark.parametrize("tag", ["xcg25_N10", "xcg25_N30"])
def test_twin_is_the_hard_twin_where_nothing_is_soft_or_nothing_binds(tag):
    P, q, A, l, u = sc.fixture_qp(tag, moved=False)
    N = P.shape[0] // 3
    hard = mo.admm_osqp(P, q, A, l, u, drop_unbounded_rows=True)
    for wr in (np.zeros(A.shape[0]), sc.state_row_weights(100.0, N, A.shape[0])):      # no soft row | soft rows that never bind
        soft = sc.admm_osqp_soft(P, q, A, l, u, wr)
        assert np.array_equal(soft["x"], hard["x"]) and soft["iters"] == hard["iters"] and soft["rho"] == hard["rho"]
        assert not soft["soft_active"] and soft["converged"]
    # ... and with zero weights on the QP without a feasible point: the hard twin's certificate, at the same test
    P, q, A, l, u = sc.fixture_qp(tag, moved=True)
    hard, soft = mo.admm_osqp(P, q, A, l, u, drop_unbounded_rows=True), sc.admm_osqp_soft(P, q, A, l, u, np.zeros(A.shape[0]))
    assert hard["infeasible"] and soft["infeasible"] and soft["iters"] == hard["iters"] == 25 and not soft["soft_active"]


# ---- the boundary of the feature, in the manner of tests/test_cabi_symbols.py
def test_header_declares_the_call_and_the_bit():
    assert re.search(r"\bint\s+f16_mpc_plan_soft_rows\s*\(\s*f16_mpc_plan\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*\)\s*;", header())
    assert defines()["F16_ST_QP_SOFT_ACTIVE"] == 1 << 27
    assert defines()["F16_ST_LOOP_STALL"] == 1 << 26      # the first free bit above it


def test_library_exports_the_call():
    from f16_mpc_oop_py_amd import lib
    L = ctypes.CDLL(lib.build())
    assert hasattr(L, "f16_mpc_plan_soft_rows")


def test_binding_carries_the_call_and_the_bit():
    from f16_mpc_oop_py_amd import lib
    assert lib.F16_ST_QP_SOFT_ACTIVE == 1 << 27 == sc.SOFT_ACTIVE
    lib.build()
    assert list(lib.load().f16_mpc_plan_soft_rows.argtypes) == [ctypes.c_void_p, ctypes.c_void_p]
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "f16_mpc_plan_soft_rows" in doc


def test_keywords_of_the_environment():
    from f16_mpc_oop_py_amd import F16Batch
    for name in ("prepare_MPC", "rollout_MPC", "_calc_MPC_action"):
        p = inspect.signature(getattr(F16Batch, name)).parameters
        assert "soft" in p and p["soft"].default is None, name
    rows = F16Batch._soft_rows
    assert rows(None) is None and rows(0.0) is None and rows(np.zeros(9)) is None
    assert rows(100) == (0.0, 0.0, 100.0, 100.0, 100.0, 100.0, 100.0, 0.0, 100.0)
    assert rows(np.arange(9.0)) == tuple(float(i) for i in range(9))
    with pytest.raises(ValueError):
        rows([1.0, 2.0])
