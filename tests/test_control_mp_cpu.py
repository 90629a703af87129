"""Fixture G19 (tools/make_control_golden.py) on the CPU: the multiprecision reference is what it claims to be, the pivot cases
really force the pivoted inverse, and the restatements the other tests rely on (oracle.c2d, oracle.dare, mo.dlqr) meet -- for the
first time -- something more accurate than scipy, at the tolerance rule of tests/test_gpu_control_mp.py: 16 x the error of the numpy
restatement of the kernel's rule on that case (oracle/control_twin.py, recorded in the fixture), floor 64 eps, relative to the
block's largest entry."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO, golden
from oracle import control_twin as ct
from oracle import mpc_oracle as mo

EPS = float(np.finfo(np.float64).eps)


def allowed(twin_err):
    return max(16.0 * float(twin_err), 64.0 * EPS)


def relerr(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.fixture(scope="module")
def G():
    return golden("g19_control_mp.npz")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("make_control_golden", os.path.join(REPO, "tools", "make_control_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _case(G, key, name):
    return list(G[key]).index(name)


# ------------------------------------------------------------------------------------------------ fixture honesty
@pytest.mark.parametrize("tag,name", [("zoh9", "trim_xcg35_dt0.2"), ("zoh9", "rotation_block"), ("zoh18", "trim18_xcg25_dt0.1")])
def test_stored_zoh_is_the_multiprecision_expm(G, tool, tag, name):
    i = _case(G, f"{tag}_names", name)
    Ad, Bd = tool.mp_zoh(G[f"{tag}_A"][i], G[f"{tag}_B"][i], G[f"{tag}_dt"][i])
    assert np.array_equal(Ad, G[f"{tag}_Ad"][i]) and np.array_equal(Bd, G[f"{tag}_Bd"][i])


@pytest.mark.parametrize("name", ["trim_xcg35_QCdCd_R1e4", "pivot_45"])
def test_stored_riccati_solution_is_the_polished_one(G, tool, name):
    """recomputed from scipy's start by the multiprecision Newton-Kleinman iteration: equal to the stored fp64 values"""
    i = _case(G, "dare_names", name)
    Q = tool.mp_ctc(G["dare_C"][i]) if G["dare_q_from_cd"][i] else G["dare_Q"][i]
    X, K, res, rho = tool.mp_dare(G["dare_A"][i], G["dare_B"][i], Q, G["dare_R"][i])
    assert res <= 1e-30 and rho < 1.0
    assert np.array_equal(X, G["dare_X"][i]) and np.array_equal(K, G["dare_K"][i])


def test_every_stored_solution_solves_its_riccati_equation_and_stabilises(G, tool):
    """The stored X is the 60-digit solution (residual <= 1e-30 max|X| asserted by the tool) rounded ONCE to fp64.  A perturbation d
    of the solution changes the residual by Ac' d Ac - d to first order (Ac = A - B K), so the rounding, |d| <= eps/2 max|X|
    entrywise, leaves a multiprecision residual of at most (|Ac|_1 |Ac|_inf + 1) eps/2 max|X|; twice that is allowed (second
    order, the rounding of K).  An fp64 SOLVER's answer is decades above this bound (profiles/control_mp_errors.txt)."""
    for i, name in enumerate(G["dare_names"]):
        A, B, R, X, K = (G[k][i] for k in ("dare_A", "dare_B", "dare_R", "dare_X", "dare_K"))
        Q = tool.mp_ctc(G["dare_C"][i]) if G["dare_q_from_cd"][i] else G["dare_Q"][i]
        res, xmax = tool.mp_dare_residual(A, B, Q, R, X)
        Ac = A - B @ K
        bound = (np.abs(Ac).sum(0).max() * np.abs(Ac).sum(1).max() + 1.0) * EPS * float(xmax)
        assert float(res) <= bound, (name, float(res), bound)
        assert np.abs(np.linalg.eigvals(Ac)).max() < 1.0, name
        assert np.array_equal(X, X.T)


def test_zoh_cases_take_the_squarings_the_issue_measured(G):
    s = dict(zip(G["zoh9_names"], G["zoh9_s"]))
    s.update(zip(G["zoh18_names"], G["zoh18_s"]))
    for xcg in (25, 35):
        assert [s[f"trim_xcg{xcg}_dt{d:g}"] for d in (1e-3, 5e-3, 2e-2, 0.2)] == [2, 4, 6, 9]
        assert [s[f"trim18_xcg{xcg}_dt{d:g}"] for d in (1e-3, 2e-2, 0.1)] == [2, 6, 9]
    assert s["threshold_at_half"] == 0 and s["threshold_one_ulp_above"] == 1
    for tag in ("zoh9", "zoh18"):                # the fixture's yardsticks are the twin's errors, nothing else
        for i in range(len(G[f"{tag}_names"])):
            Ad, Bd, si = ct.zoh(G[f"{tag}_A"][i], G[f"{tag}_B"][i], G[f"{tag}_dt"][i])
            assert si == G[f"{tag}_s"][i]
            assert relerr(Ad, G[f"{tag}_Ad"][i]) <= 2 * G[f"{tag}_twin_err"][i, 0] + EPS
            assert relerr(Bd, G[f"{tag}_Bd"][i]) <= 2 * G[f"{tag}_twin_err"][i, 1] + EPS


# ------------------------------------------------------------------------------------------------ the pivot cases
def test_pivot_cases_force_the_pivoted_inverse(G):
    names = [str(n) for n in G["dare_names"]]
    piv = [i for i, n in enumerate(names) if n.startswith("pivot")]
    assert len(piv) == 4
    for i in piv:
        A, B, Q, R = (G[k][i] for k in ("dare_A", "dare_B", "dare_Q", "dare_R"))
        r, c = int(names[i][6]), int(names[i][7])
        M0 = np.eye(9) + B @ np.linalg.inv(R) @ B.T @ Q
        assert M0[r, r] == 0.0 and np.linalg.cond(M0) < 100
        W, ok = ct.inverse9(M0, False)
        assert not ok and not np.isfinite(W).all()
        Wp, okp = ct.inverse9(M0, True)
        assert okp and np.abs(Wp @ M0 - np.eye(9)).max() < 1e-13
        X, it, pivoted = ct.dare(A, B, Q, R)
        assert it < ct.MAX_DOUBLINGS and pivoted >= 1
        assert relerr(X, G["dare_X"][i]) <= 64 * EPS
        assert ct.dare(A, B, Q, R, allow_pivot=False)[1] == ct.MAX_DOUBLINGS        # natural order alone: not finite
        assert c == r + 1


# ------------------------------------------------------------------------------------------------ the restatements
def test_oracle_c2d_vs_multiprecision_expm(G, oracle):
    bad = []
    for tag in ("zoh9", "zoh18"):
        for i, name in enumerate(G[f"{tag}_names"]):
            Ad, Bd = oracle.c2d(G[f"{tag}_A"][i], G[f"{tag}_B"][i], float(G[f"{tag}_dt"][i]))
            for blk, got, k in (("Ad", Ad, 0), ("Bd", Bd, 1)):
                e, a = relerr(got, G[f"{tag}_{blk}"][i]), allowed(G[f"{tag}_twin_err"][i, k])
                if not e <= a:
                    bad.append((str(name), blk, e, a))
    assert not bad, bad


def test_oracle_dare_and_its_gain_vs_multiprecision_riccati(G, oracle):
    """oracle.dare is the R = I restatement: every R = I case, X and the gain formed from it in numpy"""
    bad, seen = [], 0
    for i, name in enumerate(G["dare_names"]):
        A, B, Q, R = (G[k][i] for k in ("dare_A", "dare_B", "dare_Q", "dare_R"))
        if not np.array_equal(R, np.eye(3)):
            continue
        seen += 1
        X = oracle.dare(A, B, Q)
        K = np.linalg.inv(B.T @ X @ B + R) @ (B.T @ X @ A)
        for blk, got, ref, k in (("X", X, G["dare_X"][i], 0), ("K", K, G["dare_K"][i], 1)):
            e, a = relerr(got, ref), allowed(G["dare_twin_err"][i, k])
            if not e <= a:
                bad.append((str(name), blk, e, a))
    assert seen == 13 and not bad, bad


def test_dlqr_vs_multiprecision_gain(G):
    """mo.dlqr(polish=2) on every case, at the rule.  The default, polish=0, IS scipy.linalg.solve_discrete_are -- the reference's own
    arithmetic, pinned to the gains the reference stored at rtol 1e-12 (tests/test_oracle_vs_golden.py) -- and cannot meet the rule:
    measured 3.6e-14 (dt = 0.02) to 5.7e-8 (R = 1e4 I, xcg 0.35) against 1.4e-14 to 9.7e-10 allowed
    (profiles/control_mp_errors.txt).  So the polish is what a test takes that judges a solver, and on the R = 1e4 I cases it must
    improve on scipy by more than two decades."""
    bad = []
    for i, name in enumerate(G["dare_names"]):
        A, B, Q, R = (G[k][i] for k in ("dare_A", "dare_B", "dare_Q", "dare_R"))
        e, a = relerr(mo.dlqr(A, B, Q, R, polish=2), G["dare_K"][i]), allowed(G["dare_twin_err"][i, 1])
        if not e <= a:
            bad.append((str(name), e, a))
        if np.array_equal(R, 1e4 * np.eye(3)):
            assert e < 1e-2 * relerr(mo.dlqr(A, B, Q, R), G["dare_K"][i]), name
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the non-convergence report
def test_cap_and_non_finite_cases_report_non_convergence_on_both_cpu_twins(G, oracle):
    for i, name in enumerate(G["status_names"]):
        A, B, Q, R = (G[k][i] for k in ("status_A", "status_B", "status_Q", "status_R"))
        X, it, _ = ct.dare(A, B, Q, R)
        assert it == ct.MAX_DOUBLINGS, name
        assert bool(np.isfinite(X).all()) == bool(G["status_finite"][i]), name
        Xo, rc = oracle.dare(A, B, Q, return_status=True)
        assert rc == 1, (name, rc)
        assert bool(np.isfinite(Xo).all()) == bool(G["status_finite"][i]), name
        assert np.isfinite(ct.gain(A, B, X, R)).all() == bool(G["status_finite"][i])
