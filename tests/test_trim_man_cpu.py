"""What keeps tests/test_gpu_trim_man.py honest, checked on the CPU: the restated iteration in six dimensions IS scipy's, the committed
cases take every branch with 100 cost bands to spare (or by exact ties), the constraints of tests/trim_man_cases.py do what they are
for -- the plant then flies the manoeuvre -- and on the oracle two Nelder-Mead runs converge where one stalls, to points that hold
a turn."""
import collections

import numpy as np
import pytest

import trim_cases as tc
import trim_man_cases as tm

CONDS = tm.conditions()


def _scipy(oracle, g, i, maxiter):
    from scipy.optimize import minimize
    grp = tm.CASES[g]
    with tc.stable_argsort():
        return minimize(lambda q: tm.cost(oracle, q, grp.conds[i], grp.fi, grp.xcg).cost, list(grp.x0), method="Nelder-Mead", tol=1e-10,
                        options={"maxiter": maxiter})


def test_the_case_list_holds_what_it_must():
    assert all(len(g.conds) % 4 != 0 and len(g.x0) == 6 for g in tm.CASES)
    assert {g.fi for g in tm.CASES} == {0, 1} and {g.xcg for g in tm.CASES} == {0.25, 0.35}
    cs = [c for g in tm.CASES for c in g.conds]
    hs = [c.h for c in cs]
    assert min(hs) < 35000 < max(hs) and 35000.0 in hs
    for f in (lambda c: c.gamma, lambda c: c.psi_dot):
        assert min(map(f, cs)) < 0 < max(map(f, cs))
    assert any(c.theta_dot > 0 for c in cs)
    lim = np.array([19000.0, 25.0, 21.5, 30.0, np.pi / 2, np.pi / 6])
    assert any(np.all(np.abs(np.array(g.x0)) > lim) for g in tm.CASES)            # every unknown beyond its clip
    assert any(g.x0 == tm.X0_REF for g in tm.CASES)


def test_lofi_does_not_read_the_flap_states(oracle):
    """THE TIE RULE of trim_man_cases: xdot[0:12] of the lofi plant is bit for bit the same whatever x[16:18] holds; the hifi plant's
    is not"""
    grp = tm.CASES[0]
    x = tm.state_of(grp.x0, grp.conds[0])
    y = x.copy()
    y[16:18] += (3.0, -2.0)
    lo = [oracle.calc_xdot(s, s[12:16], 0, 0.25)[0:12] for s in (x, y)]
    hi = [oracle.calc_xdot(s, s[12:16], 1, 0.25)[0:12] for s in (x, y)]
    assert np.array_equal(lo[0], lo[1]) and not np.array_equal(hi[0], hi[1])


@pytest.mark.parametrize("g,i", CONDS)
def test_restatement_equals_scipy(oracle, g, i):
    """the same path as scipy.optimize.minimize under the stable sort: after n iterations the costs bit for bit, nfev equal, nit = n +
    1 for maxiter = n + 1"""
    rec = tm.path(oracle, g, i)
    yard, scale = tc.vertex_yardstick(rec, tm.CASES[g].x0)
    for n in (1, 5, 17, tm.N_LOCK):
        r = _scipy(oracle, g, i, n + 1)
        sim, fsim = r.final_simplex
        assert np.array_equal(fsim, rec[n]["fsim"]), n
        assert r.nfev == rec[n]["nfev"] and r.nit == n + 1 and r.status == 2, n
        assert np.all(np.abs(sim - rec[n]["sim"]) <= tc.vertex_allowance(yard[n], scale)), n


def test_nit_and_nfev_at_every_cap(oracle):
    """caps 1 .. 33 on one path without ties and on the all-shrink path: scipy's nit = the cap, nfev the restatement's"""
    for g in (0, next(k for k, grp in enumerate(tm.CASES) if grp.name == "all_clipped_lofi")):
        rec = tm.path(oracle, g, 0)
        for cap in range(1, tm.N_LOCK + 2):
            r = _scipy(oracle, g, 0, cap)
            assert r.nit == cap and r.nfev == rec[cap - 1]["nfev"] and r.status == 2, (g, cap)
            assert np.array_equal(r.final_simplex[1], rec[cap - 1]["fsim"]), (g, cap)


def test_every_branch_is_taken_and_every_decision_has_a_margin_of_100_bands(oracle):
    total, worst = collections.Counter(), np.inf
    for g, i in CONDS:
        rec = tm.path(oracle, g, i)
        assert len(rec) == tm.N_LOCK + 1, (g, i, len(rec))              # no case terminates inside the window
        assert rec[0]["nfev"] == 7
        assert all(r["nfev"] - q["nfev"] == tm.NFEV_OF[r["branch"]] for q, r in zip(rec[:-1], rec[1:]))
        m = [r["margin"] for r in rec]
        assert min(m) >= 100, (tm.CASES[g].name, i, int(np.argmin(m)), rec[int(np.argmin(m))]["branch"], min(m))
        worst = min(worst, min(m))
        total.update(r["branch"] for r in rec[1:])
    print("trim-in-a-manoeuvre lockstep cases: branches", dict(total), f"smallest decision margin {worst:.1f} bands")
    assert all(total[b] >= 3 for b in tm.BRANCHES), dict(total)


def test_the_restated_cost_is_well_conditioned_on_every_case_path(oracle):
    """rounding inside the constraints moves the cost by less than a tenth of its band at every vertex of every case path (measured: <=
    1e-5 band) -- and by far more than the band where no case may go: alpha at its 90 deg clip with gamma = 0"""
    for g, i in CONDS:
        grp = tm.CASES[g]
        assert max(tm.conditioning(oracle, v, grp.conds[i], grp.fi, grp.xcg) for r in tm.path(oracle, g, i) for v in r["sim"]) <= 0.1, (g, i)
        assert grp.x0[4] < np.pi / 2 or grp.conds[i].gamma != 0
    g = next(k for k, grp in enumerate(tm.CASES) if grp.name == "all_clipped_lofi")
    assert tm.conditioning(oracle, tm.CASES[g].x0, tm.CASES[g].conds[1]._replace(gamma=0.0), 0, 0.25) > 1e3


def test_the_all_clipped_start_shrinks_at_every_iteration(oracle):
    g = next(k for k, grp in enumerate(tm.CASES) if grp.name == "all_clipped_lofi")
    for i in range(len(tm.CASES[g].conds)):
        rec = tm.path(oracle, g, i)
        assert all(r["branch"] == "shrink_in" for r in rec[1:])
        assert [r["nfev"] for r in rec] == [7 + 8 * n for n in range(tm.N_LOCK + 1)]
        assert len(set(rec[0]["fsim"])) == 1 and list(rec[0]["ind"]) == list(range(7))      # seven equal costs keep their order


def test_the_constraints_make_the_plant_fly_the_manoeuvre(oracle):
    """at random q the plant reproduces what the constraints were solved for: xdot[2] = V sin(gamma), xdot[3] = 0, xdot[4] = theta_dot,
    xdot[5] = psi_dot, to 1e-12 relative (of max(1, |target|), and of V for the climb rate)"""
    rng = np.random.default_rng(11)
    for k in range(200):
        cond = tm.Cond(rng.uniform(2000, 45000), rng.uniform(350, 900), rng.uniform(-10, 20) * tm.DEG, rng.uniform(-10, 10) * tm.DEG,
                       rng.uniform(-3, 3) * tm.DEG if k % 2 else 0.0)
        q = (rng.uniform(1000, 19000), rng.uniform(-25, 25), rng.uniform(-21.5, 21.5), rng.uniform(-30, 30), rng.uniform(-5, 25) * tm.DEG,
             rng.uniform(-10, 10) * tm.DEG)
        c = tm.cost(oracle, q, cond, k % 2, 0.25 if k % 3 else 0.35)
        t = tm.target_of(cond)
        assert abs(c.xd[2] - t[2]) <= 1e-12 * cond.v, (k, c.xd[2], t[2])
        assert abs(c.xd[3]) <= 1e-12 and abs(c.xd[4] - t[4]) <= 1e-12 and abs(c.xd[5] - t[5]) <= 1e-12, (k, c.xd[3:6], t[3:6])


_TWO = {}


def two_runs(oracle, k):
    if k not in _TWO:
        _TWO[k] = tm.scipy_runs(oracle, tm.FULL[k])
    return _TWO[k]


@pytest.mark.parametrize("k", range(len(tm.FULL)), ids=tm.FULL_NAMES)
def test_one_run_stalls_and_two_converge(oracle, k):
    one, two = two_runs(oracle, k)
    print(f"trim in a manoeuvre, {tm.FULL_NAMES[k]}: cost after one run {one.fun:.3g} (nit {one.nit}), after two {two.fun:.3g} (nit {two.nit})")
    assert one.fun > 1e-8 and two.fun <= 1e-20
    assert one.status == 0 and two.status == 0
    assert 1000 < two.x[0] < 19000


@pytest.mark.parametrize("cond", tm.UNTRIMMABLE)
def test_the_untrimmable_conditions_stay_untrimmed(oracle, cond):
    two = tm.scipy_runs(oracle, cond)[1]
    assert two.fun > 1e-3 and not 1000 <= two.x[0] <= 19000


@pytest.mark.parametrize("k", [k for k, c in enumerate(tm.FULL) if c.gamma == 0 and c.theta_dot == 0 and c.psi_dot != 0],
                         ids=lambda k: tm.FULL_NAMES[k])
def test_the_two_run_point_holds_the_turn(oracle, k):
    """2,000 Euler steps of 1 ms on the oracle from the two-run point, constant input: V, alpha, beta, phi, theta, p, q, r within 1e-6,
    psi = turn rate x 2 s within 1e-6 rad, h within 1e-2 ft (the bars of tests/test_gpu_trim_man.py)"""
    cond = tm.FULL[k]
    x0 = tm.state_of(two_runs(oracle, k)[1].x, cond)
    xf, _, st = oracle.rollout(x0[None], x0[None, 12:16], 2000, 0.001, 1, 0.25, store=False)
    d = xf[0] - x0
    assert st[0] == 0
    assert np.abs(d[[6, 7, 8, 3, 4, 9, 10, 11]]).max() <= 1e-6 and abs(d[5] - cond.psi_dot * 2.0) <= 1e-6 and abs(d[2]) <= 1e-2, d


def test_the_committed_spread_is_the_measured_one(oracle):
    """SPREAD of trim_man_cases (1e-14 relative plant noise, the method of tests/test_gpu_trim.py) re-measured on one condition: the
    noisy two-run point stays within the committed spread of the clean one"""
    k = 1
    clean = two_runs(oracle, k)[1].x
    noisy = tm.scipy_runs(oracle, tm.FULL[k], noise=np.random.default_rng(1))[1].x
    assert np.all(np.abs(noisy - clean) <= tm.SPREAD), (np.abs(noisy - clean), tm.SPREAD)
