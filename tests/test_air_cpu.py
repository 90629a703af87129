"""CPU side of the extended-precision pin of the moving-air derivative (tests/air_cases.py): the yardstick, the reference and the
comparison themselves, from the three builds of oracle/f16_oracle.c alone.

  * every family is well built: finite in both builds, the same grid bits in both, its promise about the air triple kept (asserted
    inside air_cases.reference), and its yardstick printed;
  * the FMA-contracted fp64 build -- the same rule under other rounding -- and the fp64 plant fed a numpy statement of the air
    triple (another libm) stay within 8 Y on every family: the rule is not too tight for a correct implementation;
  * six deliberately WRONG rules, stated in numpy through f16o_xdot_air_parts_batch, each fail in the family named beside them: the
    rule is not too loose for a wrong one;
  * tests/wind_cases.py `twin_xdot`, the yardstick of tests/test_gpu_wind.py, measured against the reference (printed: what the
    older band was worth);
  * f16o_rollout_wind in fp64 against wind_cases.fly, the chain the suite already trusts;
  * the air triple alone against 60-digit mpmath: the C library inside the budgets of air_cases, a wrong stand-in outside.
"""
import numpy as np
import pytest

import air_cases as ac
import envelope_cases as ec
import wind_cases as wc

ALL = ac.FAMILIES + ac.EXACT
# the family in which each wrong rule of air_cases.WRONG is required to fail (it may fail in others too)
CAUGHT_IN = {"beta_atan2": ac.Family("interior", "hifi"), "lef_ground_alpha": ac.Family("interior", "lofi"),
             "damping_ground_vt": ac.Family("interior", "hifi"), "plus_wd": ac.Family("wind_only", "hifi"),
             "gust_dropped_from_va": ac.Family("gust_only", "lofi"), "lef_clamped_vt": ac.Family("exact", "hifi")}


@pytest.mark.parametrize("fam", ALL, ids=ac.fid)
def test_fma_witness_and_numpy_statement_stay_within_the_rule(fam):
    """(air_cases.reference asserts what the family promises; a family that is mis-built fails here)"""
    r = ac.reference(fam)
    fma, _, st = ac.run(ac.libs()["fma"], fam)
    w_fma = ac.check(fma, fam, what="fma witness")
    w_np = ac.check(ac.stand_in(fam), fam, what="numpy statement")
    assert np.array_equal(st, r["status"])
    line = ac.yardstick_line(fam) if fam.kind != "exact" else "Y of the interior family"
    print(f"MEASURED {ac.fid(fam)}: rows {len(r['ref'])}, {line}, FMA witness worst ratio {w_fma.max():.2f}, numpy statement {w_np.max():.2f}")
    if fam.kind != "exact":
        assert (r["Y"] > 0).all()                    # every output row has a yardstick: nothing is compared for equality by accident


@pytest.mark.parametrize("wrong", ac.WRONG)
def test_a_wrong_rule_fails(wrong):
    caught = [ac.fid(f) for f in ALL if ac.fails(ac.stand_in(f, wrong), f)]
    print(f"MEASURED wrong rule {wrong}: fails in {len(caught)} of {len(ALL)} families: {caught}")
    assert ac.fid(CAUGHT_IN[wrong]) in caught


def test_a_wrong_rule_passes_where_it_does_not_differ():
    """the families discriminate: without a gust the dropped gust is no error, and above 0.01 ft/s the early clamp is none"""
    assert not ac.fails(ac.stand_in(ac.Family("wind_only", "hifi"), "gust_dropped_from_va"), ac.Family("wind_only", "hifi"))
    assert not ac.fails(ac.stand_in(ac.Family("gust_only", "hifi"), "plus_wd"), ac.Family("gust_only", "hifi"))
    assert not ac.fails(ac.stand_in(ac.Family("low_0.0101", "hifi"), "lef_clamped_vt"), ac.Family("low_0.0101", "hifi"))


@pytest.mark.parametrize("fidelity", ["hifi", "lofi"])
def test_the_older_twin_measured_against_the_reference(oracle, fidelity):
    """twin_xdot (two still-air evaluations and a reconstruction, fp64) on the interior family: printed, and held only to the band
    tests/test_gpu_wind.py grants it"""
    fam = ac.Family("interior", fidelity)
    c, r = ac.cases(fam), ac.reference(fam)
    twin = np.stack([wc.twin_xdot(oracle, c["x"][k], c["u"][k], c["air"][k, :3], c["air"][k, 3:], ac.fi_of(fam))[0] for k in range(len(c["x"]))])
    worst, bad = ac.ratios(twin, fam)
    rel = ec.rel(twin, r["ref"].astype(np.float64)).max()
    print(f"MEASURED twin_xdot against the long double reference, {ac.fid(fam)}: worst ratio to Y {worst.max():.3g} "
          f"(rows 6..8: {worst[6:9].max():.3g}), {int(bad.sum())} entries beyond 8 Y, largest relative error {rel:.2e}")
    assert rel < 1e-11 * 400


@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("fi", [1, 0])
@pytest.mark.parametrize("lqr", [False, True], ids=["open", "lqr"])
def test_rollout_wind_equals_the_chain_the_suite_trusts(oracle, fi, method, lqr):
    """f16o_rollout_wind in fp64 against wind_cases.fly (the numpy twin stepped by rk4_cases.restate) on one small flight, at the
    band of tests/test_gpu_wind.py: 1e-9 widened by the twin's reconstruction error"""
    import rk4_cases as rk
    B, T, hold, ghold, dt = 8, 12, 5, 2, 0.001
    b = wc.subset(fi, B)
    w, g = wc.air(B, 3 + fi, rows=(T + ghold - 1) // ghold)
    S = (T + hold - 1) // hold
    if lqr:
        rows, K, u0 = np.random.default_rng(2).uniform(-0.15, 0.15, (S, B, 3)), rk.lqr_gain(), b.u
    else:
        rows, K, u0 = np.random.default_rng(1).uniform([0, -30, -25, -35], [20000, 30, 25, 35], (S, B, 4)), None, None
    r = wc.fly(oracle, b.x, rows, hold, T, dt, fi, method, w, g, ghold, K, u0)
    q = ac.libs()["fp64"].rollout_wind(b.x, rows, T, hold, dt, 4 if method == "rk4" else 1, fi, wind=w, gusts=g, gust_hold=ghold,
                                       K=None if K is None else np.asarray(K).reshape(27), u0=u0)
    tol = wc.band(1e-9, wc.reconstruction_error(oracle, b))
    err = ec.rel(q["traj"], r["traj"]).max((0, 2))
    print(f"MEASURED f16o_rollout_wind against wind_cases.fly fi={fi} {method} lqr={lqr}: {err.max():.2e}")
    assert np.isfinite(r["traj"]).all() and (err < tol).all()
    assert np.array_equal(q["x"], q["traj"][-1]) and np.array_equal(ec._nonfinite(q["status"], q["x"]), r["status"])
    if lqr:
        assert (ec.rel(q["u"], r["u_last"]).max(1) < tol).all()


def test_rollout_wind_freezes_at_the_box_and_keeps_the_wide_state():
    """an aircraft outside the box takes no step in either build; the wide build's state is not an fp64 number after a step"""
    x, u = ac.rows_in_box("hifi")
    x, u = x[:4].copy(), u[:4].copy()
    x[1, 6] = 901.0
    for k, L in ac.libs().items():
        r = L.rollout_wind(x, u[None], 3, 3, 0.001, 4, 1, wind=np.full((4, 3), 20.0))
        assert np.array_equal(r["x"][1], x[1].astype(L.dtype)) and r["status"][1] == 16 | 1 << 14 and (r["status"][[0, 2, 3]] & 16 == 0).all()
        assert r["x"].dtype == L.dtype
    wide = ac.libs()["ld"].rollout_wind(x, u[None], 3, 3, 0.001, 4, 1, wind=np.full((4, 3), 20.0))["x"]
    assert (wide[0] != wide[0].astype(np.float64)).any()


# ------------------------------------------------------------------------------------------------ the air triple alone, against mpmath
def test_the_c_library_is_inside_every_budget_of_the_air_triple():
    """numpy's fp64 statement of the rule (the C library's sin / cos / sqrt / atan2 / asin) on air_cases.triple_cases()"""
    in12 = ac.triple_cases()
    fig = ac.triple_figures(in12, ac.triple_numpy(in12))
    for k, (worst, bound) in fig.items():
        print(f"MEASURED air triple, C library, {k}: {worst:.3f} of {bound:.3f} ({in12.shape[1]} cases)")
        assert worst <= bound, k
    assert ac.uvw_budget() < 16 and ac.vt_budget() < 2.6       # the derived figures, not fitted ones


@pytest.mark.parametrize("what", ["uvw", "vt", "alpha", "beta"])
def test_a_wrong_air_triple_is_outside_its_budget(what):
    """cos(psi) rounded to single precision in the rotation; a root, an atan2 and an asin each four ulp off: of the three, only the
    budget named is exceeded"""
    in12 = ac.triple_cases()
    got = ac.triple_numpy(in12)
    if what == "uvw":
        x = np.zeros((in12.shape[1], 18))
        x[:, 3:9] = in12[:6].T
        d = (np.cos(x[:, 5]).astype(np.float32).astype(np.float64) - np.cos(x[:, 5])) * np.cos(x[:, 4]) * in12[6]
        got[0] -= d
    else:
        got[{"vt": 3, "alpha": 4, "beta": 5}[what]] *= 1 + 2.0 ** -50
    fig = ac.triple_figures(in12, got)
    print(f"MEASURED wrong air triple ({what}): " + ", ".join(f"{k} {w:.2f} of {b:.2f}" for k, (w, b) in fig.items()))
    assert fig[what][0] > fig[what][1]
    if what != "uvw":                                           # (vt_a, alpha_a, beta_a are judged on the candidate's own Ua, Va, Wa)
        assert all(w <= b for k, (w, b) in fig.items() if k != what)
