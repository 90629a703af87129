"""What keeps tests/test_gpu_trim_lockstep.py honest, checked where it can be checked -- on the CPU: the restatement of scipy's
Nelder-Mead iteration (tests/trim_cases.py) IS scipy's, the committed cases take every branch of the iteration, every decision on
their paths is made with a margin of 100 cost bands or more, and none of them terminates inside the lockstep window."""
import collections

import numpy as np
import pytest

import trim_cases as tc
from oracle import mpc_oracle as mo

CONDS = tc.conditions()


def _scipy(oracle, g, i, maxiter, pinned=True):
    """scipy's own run; pinned: with its argsort held to the stable kind (trim_cases: THE TIE RULE)"""
    import contextlib
    from scipy.optimize import minimize
    grp = tc.CASES[g]
    with tc.stable_argsort() if pinned else contextlib.nullcontext():
        return minimize(lambda q: tc.trim_cost(oracle, q, grp.h[i], grp.v[i], grp.fi, grp.xcg).cost, list(grp.x0), method="Nelder-Mead",
                        tol=1e-10, options={"maxiter": maxiter})


def test_the_case_list_holds_what_it_must():
    assert len(tc.CASES) <= 6 and 16 <= len(CONDS) <= 24
    assert all(len(g.h) == len(g.v) and len(g.h) % 4 != 0 for g in tc.CASES)
    for xcg in (0.25, 0.35):                                # the reference start at the two golden conditions
        assert any(g.x0 == tc.X0_REF and g.fi == 1 and g.xcg == xcg and (10000.0, 700.0) in zip(g.h, g.v) for g in tc.CASES)
    lim = np.array([19000.0, 25.0, 21.5, 30.0])
    assert any(np.all(np.abs(np.array(g.x0[:4])) > lim) for g in tc.CASES)           # all four commands beyond their limits
    assert any(0.0 in g.x0 for g in tc.CASES)                                        # the 0.00025 rule
    assert any(g.x0[4] > np.pi / 2 for g in tc.CASES)                                # alpha above the 90 deg clip
    hs = [h for g in tc.CASES for h in g.h]
    assert min(hs) < 35000 < max(hs) and 35000.0 in hs
    assert {g.fi for g in tc.CASES} == {0, 1} and {g.xcg for g in tc.CASES} == {0.25, 0.35}


def test_trim_objective_is_the_one_mo_trim_minimises(oracle):
    """mo.trim kept its behaviour when the objective was lifted out of it: the golden trim point, bit for bit, and the cost of its
    result is the shared objective there"""
    from conftest import golden
    x, opt = mo.trim(oracle, 10000.0, 700.0)
    assert np.array_equal(x, golden("g567_trim_lin_lqr.npz")["trim_x_xcg25"])
    c = tc.trim_cost(oracle, opt.x, 10000.0, 700.0, 1, 0.25)
    assert c.cost == opt.fun and c.band > 0 and c.xd.shape == (18,)


def test_the_cost_band_is_the_first_order_propagation_of_the_xdot_band(oracle):
    """the band covers what an XDOT_TOL max(1, |xd_k|) perturbation of every derivative does to the cost, worst signs"""
    grp = tc.CASES[0]
    c = tc.trim_cost(oracle, grp.x0, grp.h[0], grp.v[0], grp.fi, grp.xcg)
    d = tc.XDOT_TOL * np.maximum(1.0, np.abs(c.xd[:12])) * np.sign(c.xd[:12])
    moved = float(np.dot(tc.W, (c.xd[:12] + d) ** 2))
    assert 0 < moved - c.cost <= c.band * (1 + 1e-6)


@pytest.mark.parametrize("g,i", CONDS)
def test_restatement_equals_scipy(oracle, g, i):
    """after n iterations the restatement holds scipy's simplex: costs bit for bit, nfev equal, nit = n + 1 for maxiter = n + 1.
    A path on which no two vertices ever tie is compared with scipy as it is; one with ties with scipy under the stable sort, the
    only sort for which scipy's answer does not depend on the host."""
    rec = tc.path(oracle, g, i)
    yard, scale = tc.vertex_yardstick(rec, tc.CASES[g].x0)
    ties = any(len(set(r["fsim"])) < 6 for r in rec)
    for n in (1, 5, 17, tc.N_LOCK):
        r = _scipy(oracle, g, i, n + 1, pinned=ties)
        sim, fsim = r.final_simplex
        assert np.array_equal(fsim, rec[n]["fsim"]), n
        assert r.nfev == rec[n]["nfev"] and r.nit == n + 1 and r.status == 2, n
        assert np.all(np.abs(sim - rec[n]["sim"]) <= tc.vertex_allowance(yard[n], scale)), n


def test_the_tie_rule_is_needed_only_where_vertices_tie(oracle):
    """the groups that start with every command beyond its limit do tie, the others never: their comparison is with plain scipy"""
    tied = {tc.CASES[g].name for g, i in CONDS if any(len(set(r["fsim"])) < 6 for r in tc.path(oracle, g, i))}
    assert tied == {grp.name for grp in tc.CASES if np.all(np.abs(np.array(grp.x0[:4])) > [19000.0, 25.0, 21.5, 30.0])}, tied


def test_scipy_maxiter_n_is_one_iteration_behind(oracle):
    """THE OFF-BY-ONE, in words: scipy's counter starts at 1 and the loop runs `while iterations < maxiter`, so `maxiter = n` performs
    n - 1 iterations and reports nit = n.  include/f16_hip.h promises the same meaning for f16_trim_batch's maxiter and iters; a scipy
    that counts otherwise must fail here, not silently move the lockstep test by an iteration."""
    g, i = 0, 0
    rec = tc.path(oracle, g, i)
    for n in (1, 2, 9):
        r = _scipy(oracle, g, i, n, pinned=False)
        assert r.nit == n and r.status == 2
        assert r.nfev == rec[n - 1]["nfev"] and np.array_equal(r.final_simplex[1], rec[n - 1]["fsim"])
        assert np.array_equal(r.final_simplex[0], rec[n - 1]["sim"])
        assert not np.array_equal(r.final_simplex[1], rec[n]["fsim"])


def test_every_branch_is_taken(oracle):
    total, shrinks = collections.Counter(), set()
    for g, i in CONDS:
        for r in tc.path(oracle, g, i)[1:]:
            total[r["branch"]] += 1
            if r["branch"].startswith("shrink"):
                shrinks.add((r["branch"], tc.CASES[g].fi))
    print("trim lockstep cases: branches", dict(total))
    assert all(total[b] >= 3 for b in tc.BRANCHES), dict(total)
    assert shrinks == {(s, fi) for s in ("shrink_out", "shrink_in") for fi in (0, 1)}, shrinks


def test_every_decision_has_a_margin_of_100_bands_and_no_case_terminates(oracle):
    worst = np.inf
    for g, i in CONDS:
        rec = tc.path(oracle, g, i)
        assert len(rec) == tc.N_LOCK + 1, (g, i, len(rec))
        m = [r["margin"] for r in rec]
        assert all(r["nfev"] - q["nfev"] == tc.NFEV_OF[r["branch"]] for q, r in zip(rec[:-1], rec[1:]))
        assert min(m) >= 100, (tc.CASES[g].name, i, int(np.argmin(m)), rec[int(np.argmin(m))]["branch"], min(m))
        worst = min(worst, min(m))
    print(f"trim lockstep cases: smallest decision margin {worst:.1f} bands")


def test_exact_ties_fall_to_the_stability_rule(oracle):
    """the start with all four commands beyond their limits: five vertices of the initial simplex give the plant the same input, so
    their costs are one number, and the stable sort keeps them in the order scipy built them"""
    g = next(k for k, grp in enumerate(tc.CASES) if np.all(np.abs(np.array(grp.x0[:4])) > [19000.0, 25.0, 21.5, 30.0]))
    rec = tc.path(oracle, g, 0)
    f = rec[0]["fsim"]
    assert sum(f == f[0]) == 5 or sum(f == f[-1]) == 5
    tied = [k for k in rec[0]["ind"] if k != 5]
    assert tied == sorted(tied)
