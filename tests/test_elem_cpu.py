"""The elementary functions of the default build without a GPU (tests/elem_cases.py):
  * the error measure on hand-made cases;
  * the host restatement of sincos_bf (oracle/f16_elem_oracle.c) holds the plant header's constants and meets the accuracy rule on
    every family against multiprecision values -- the GPU module then only has to show that the device gives the restatement's bits;
  * the budgets of the atmosphere, the reciprocal, the tangent and the carried pairs evaluated on C-library stand-ins and on the
    restatement of trig_rotate;
  * every rule shown able to fail: a coefficient perturbed in its last digits, the third reduction part dropped, a Newton step
    dropped, the exponent fraction wrong in its 15th digit, a series term dropped from the rotation."""
import math
import os
import re

import mpmath
import numpy as np
import pytest

import elem_cases as ec


# ---------------------------------------------------------------- the measure
def test_the_error_measure_on_hand_made_cases():
    with mpmath.workprec(ec.PREC):
        one = mpmath.mpf(1)
        t = ec.Truth([one + mpmath.ldexp(one, -54), mpmath.mpf(0.75), one * 0, mpmath.mpf(3) / 4 + mpmath.ldexp(one, -60), mpmath.mpf(5e-324)])
    assert t.hi.tolist() == [1.0, 0.75, 0.0, 0.75, 5e-324] and t.lo[0] == 2.0 ** -54 and t.lo[3] == 2.0 ** -60
    got = np.array([1.0, np.nextafter(0.75, 1), 0.0, np.nextafter(0.75, 0), 1e-323])
    # 2^-54 of spacing 2^-52; one spacing of 0.75 (2^-53 ulp: 1.11e-16); exact; one spacing + 2^-60 / 2^-53; one denormal spacing
    assert ec.ulps(got, t).tolist() == [0.25, 1.0, 0.0, 1.0 + 2.0 ** -7, 1.0]
    assert ec.ulps(np.array([np.nextafter(1.0, 2), np.nan, np.inf, 0.75, 5e-324]), t).tolist() == [0.75, np.inf, np.inf, 2.0 ** -7, 0.0]
    # relative, in u = 2^-53: the double above 0.75 is 2^-53 / 0.75 away
    assert ec.rel_u(got, t)[1] == pytest.approx(1 / 0.75, rel=1e-12) and ec.rel_u(got, t)[2] == 0.0
    assert ec.same_bits([np.nan, 0.0, 1.0], [np.nan, 0.0, 1.0]) and not ec.same_bits([0.0], [-0.0]) and not ec.same_bits([np.nan], [1.0])


# ---------------------------------------------------------------- the restatement is the header's
def test_the_restatement_holds_the_constants_of_the_plant_header():
    head, mine = ec.header_sincos_constants(), ec.restated_constants()
    assert head.size == 21 and ec.same_bits(head, mine)
    text = open(os.path.join(ec.REPO, "oracle", "f16_elem_oracle.c")).read()
    assert "f16_plant.hpp" in text and "SINCOS_K" in text
    # 2/pi and pi/2 in three full parts: what the table claims to be
    with mpmath.workprec(400):
        h = mpmath.pi / 2
        p0 = float(h)
        p1 = float(h - mpmath.mpf(p0))
        p2 = float(h - mpmath.mpf(p0) - mpmath.mpf(p1))
        assert mine[:4].tolist() == [float(2 / mpmath.pi), -p0, -p1, -p2]
        for k in range(8):                                          # the exact 1 / k! of the Taylor series, rounded once
            assert mine[4 + k] == float((-1) ** (k + 1) / mpmath.factorial(2 * k + 3)), k
        for k in range(9):
            assert mine[12 + k] == float((-1) ** (k + 1) / mpmath.factorial(2 * k + 2)), k


def test_the_exponent_fraction_is_named_once():
    """POW_FRAC is the double 0.14, and its four users take it by name: atmos_dev and atmos_dev_k (f16_plant.hpp), the quad rollout's
    atmosphere role (f16_quad_steps.inc) and the debug kernels (f16_debug.hip) -- none multiplies a log by a literal of its own.
    What separates 4 + fl(0.14) from the fl(4.14) of the reference's pow is recorded here and weighed by the atmosphere budget below
    (the device figures: tests/test_gpu_elem.py)."""
    c = ec.header_pow_frac()
    assert c == 0.14 and c != ec.fl_4_14_minus_4()
    with mpmath.workprec(ec.PREC):
        off = float(4 + ec.mp(c) - ec.mp(4.14))
    assert 3.3e-16 < off < 3.4e-16                                        # x |log tfac| <= 1.21 on the envelope: up to 3.7 u in the density
    csrc = os.path.dirname(ec.PLANT)
    for f, uses in (("f16_plant.hpp", 2), ("f16_quad_steps.inc", 1), ("f16_debug.hip", 5)):
        text = open(os.path.join(csrc, f)).read()
        assert len(re.findall(r"POW_FRAC \* log", text)) == uses, f
        assert not re.findall(r"\d\.?\d* \* log(_k|_k_tail)?(<\w+>)?\(", text), f


# ---------------------------------------------------------------- sin / cos: accuracy of the restatement (and so of the device)
@pytest.mark.parametrize("family", ec.ACCURACY_FAMILIES)
def test_restated_sincos_within_libm_plus_two_ulp(family):
    x, ts, tc = ec.sincos_truth(family)
    assert np.abs(x).max() <= 1e6
    s, c = ec.restated_sincos(x)
    worst, bound, Y = ec.sincos_rule(x, ts, tc, s, c)
    print(f"MEASURED restated sincos_bf, {family} ({x.size} arguments): worst {worst:.3f} ulp of the true value / bound {bound:.3f} (libm {Y:.3f} + 2)")
    assert worst <= bound
    assert (s[x == 0] == 0).all() and not np.signbit(s[x == 0]).any() and (c[x == 0] == 1).all()       # -0 -> +0, as the code has it


def test_restated_sincos_beyond_1e6_is_finite_and_nan_for_non_finite_arguments():
    x, ts, tc = ec.sincos_truth("ladder")
    s, c = ec.restated_sincos(x)
    assert np.isfinite(s).all() and np.isfinite(c).all()
    e = np.maximum(ec.ulps(s, ts), ec.ulps(c, tc))
    n = np.rint(np.abs(x) * (2 / math.pi))
    for lo in (1e6, 1e7, 1e8, 1e9):
        m = (np.abs(x) >= lo) & (np.abs(x) < 10 * lo) & (n < 2.0 ** 31 - 1)
        print(f"MEASURED restated sincos_bf on [{lo:.0e}, {min(10 * lo, ec.TWO31_PIO2):.3e}): worst {e[m].max():.3f} ulp ({m.sum()} arguments; printed only)")
    m = n >= 2.0 ** 31 - 1
    print(f"MEASURED restated sincos_bf from 2^31 pi/2: worst absolute error {max(np.abs(s[m] - ts.hi[m]).max(), np.abs(c[m] - tc.hi[m]).max()):.3f} "
          f"({m.sum()} arguments; printed only)")
    sn, cn = ec.restated_sincos(ec.sincos_family("nonfinite"))
    assert np.isnan(sn).all() and np.isnan(cn).all()


def perturbed_tables():
    K = ec.restated_constants()
    out = {}
    t = K.copy(); t[4 + 1] *= 1 + 1e-13; out["S1 in its 13th digit"] = t
    t = K.copy(); t[12 + 1] *= 1 - 1e-13; out["C1 in its 13th digit"] = t
    t = K.copy(); t[3] = 0.0; out["third reduction part dropped"] = t
    t = K.copy(); t[1:4] = [-1.57079632673412561417e+00, -6.07710050630396597660e-11, -2.02226624879595063154e-21]
    out["reduction parts of 33 bits"] = t
    return out


@pytest.mark.parametrize("what", ["S1 in its 13th digit", "C1 in its 13th digit", "third reduction part dropped", "reduction parts of 33 bits"])
def test_the_sincos_rule_notices(what):
    table = perturbed_tables()[what]
    tripped = []
    for family in ec.ACCURACY_FAMILIES:
        x, ts, tc = ec.sincos_truth(family)
        s, c = ec.restated_sincos(x, table)
        worst, bound, _ = ec.sincos_rule(x, ts, tc, s, c)
        if worst > bound:
            tripped.append((family, round(worst, 2)))
    print(f"MEASURED {what}: trips {tripped}")
    assert tripped, what


# ---------------------------------------------------------------- atmosphere: the budget on the C-library stand-in
def test_the_atmosphere_budget_on_the_stand_in_and_what_it_can_see():
    frac = ec.header_pow_frac()
    alt, vt, truth = ec.atmos_truth(frac)
    env = ec.envelope_lanes()
    got = ec.atmos_model(alt, vt, frac)
    assert ec.same_bits(got["tfac"][env], truth["tfac"].hi[env])                      # one rounding: the fused 1 - .703e-5 alt
    worst = ec.atmos_worst(got, truth, env)
    show = lambda w: ", ".join(f"{k} {v:.2f} / {ec.FACTOR_ULPS if k == 'factor' else ec.BUDGET_U[k]} {'ulp' if k == 'factor' else 'u'}" for k, v in w.items())
    print(f"MEASURED stand-in atmosphere on [0, 1e5] ft, c = {frac!r}: " + show(worst))
    assert ec.atmos_within_budget(worst), worst
    # The two candidates for the exponent fraction: the 0.14 of the code and 4.14 - 4.0, which would make 4 + c the reference's fl(4.14).
    # The factor's own rule cannot tell them apart (each is a good tfac^c); the density sees the difference as 3.3e-16 |log tfac|: 2.7 u
    # more at 91,000 ft, most of the budget but inside it -- so the constant stays (the device agrees: tests/test_gpu_elem.py).
    both = {}
    for c in (0.14, ec.fl_4_14_minus_4()):
        g = ec.atmos_model(alt, vt, c)
        assert ec.ulps(g["factor"], ec.atmos_truth(c)[2]["factor"])[env].max() <= ec.FACTOR_ULPS
        both[c] = ec.atmos_worst(g, truth, env)
        print(f"MEASURED stand-in atmosphere on [0, 1e5] ft, c = {c!r}: " + show(both[c]))
    assert both[0.14]["rho"] > both[ec.fl_4_14_minus_4()]["rho"] + 2.0
    # ... and the rule is able to fail: the fraction wrong in its 15th digit breaks the density's budget, and only above 35,000 ft
    bad = ec.atmos_model(alt, vt, 0.140000000000001)
    worst_bad = ec.atmos_worst(bad, truth, env)
    print("MEASURED stand-in atmosphere on [0, 1e5] ft, c = 0.140000000000001: " + show(worst_bad))
    assert not ec.atmos_within_budget(worst_bad) and worst_bad["rho"] > ec.budget("rho")
    over = ec.rel_u(bad["rho"], truth["rho"]) > ec.budget("rho")
    assert alt[over & env].min() > 35000.0


# ---------------------------------------------------------------- reciprocal and tangent: the model
def test_the_reciprocal_rule_holds_for_two_newton_steps_and_notices_a_lost_one():
    x, promised = ec.rcp_arguments()
    t = ec.rcp_truth()
    assert promised.sum() > 8000 and (~promised).sum() >= 8
    two = ec.ulps(ec.rcp_model(x, 2), t)[promised].max()
    one = ec.ulps(ec.rcp_model(x, 1), t)[promised].max()
    print(f"MEASURED model of f16_rcp (24-bit seed): two Newton steps {two:.3f} ulp / bound {ec.RCP_ULPS}, one step {one:.1f} ulp")
    assert two <= ec.RCP_ULPS < one


def test_the_tangent_budget_on_the_restatement_and_the_model():
    th = ec.tan_arguments()
    st, ct = ec.restated_sincos(th)
    tt = st * ec.rcp_model(ct, 2)
    bound = ec.tan_budget(ec.start_sincos_ulps(th))
    worst = ec.rel_u(tt, ec.tan_truth()).max()
    lost = ec.rel_u(st * ec.rcp_model(ct, 1), ec.tan_truth()).max()
    print(f"MEASURED st * rcp(ct) against tan(theta): {worst:.2f} u / budget {bound:.2f} u; with a Newton step lost {lost:.1f} u")
    assert worst <= bound < lost


# ---------------------------------------------------------------- carried pairs: the restatement of trig_rotate
@pytest.mark.parametrize("n_steps", ec.CARRY_LENGTHS)
def test_carried_pairs_stay_within_the_rotation_budget(n_steps):
    start, steps = ec.carry_cases(n_steps)
    out = ec.restated_trig_carry(start, steps)
    assert (out[:, 3] == 0).all()                                       # every increment inside the series' range
    assert np.abs(np.diff(np.vstack([start[None], out[:, 2]]), axis=0)).max() <= ec.D_MAX
    crossing = lambda v: ((out[0, 2] - v) * (out[-1, 2] - v) < 0).any()
    assert n_steps == 1 or (crossing(0.0) and crossing(math.pi / 2) and crossing(-math.pi / 2))
    err, norm = ec.carry_worst(out)
    e0 = ec.start_sincos_ulps(start)
    bound = np.array([ec.carry_budget(k + 1, e0) for k in range(n_steps)])
    print(f"MEASURED carried pairs, {n_steps} rotations: |s - sin|, |c - cos| {err[-1]:.2f} u / budget {bound[-1]:.2f} u; "
          f"|s^2 + c^2 - 1| {norm[-1]:.2f} u (per rotation: budget {ec.rotation_budget():.3f} u)")
    assert (err <= bound).all() and (norm <= bound).all()


def test_the_carry_rule_notices_a_dropped_series_term():
    """a numpy copy of the rotation without the d^4 / 24 of cos d: 1e-11 a step at d = 3.9e-3"""
    start, steps = ec.carry_cases(31)
    out = ec.restated_trig_carry(start, steps)
    s, c = ec.restated_sincos(start)
    a, bad = start.copy(), np.empty_like(out)
    for k in range(31):
        an = a + steps[k]
        d = an - a
        d2 = d * d
        sd, cd = d * (1 + d2 * (d2 / 120 - 1 / 6)), 1 - d2 / 2
        s, c = c * sd + s * cd, c * cd - s * sd
        a = an
        bad[k] = np.stack([s, c, a, np.zeros_like(a)])
    assert ec.same_bits(bad[:, 2], out[:, 2])
    err, norm = ec.carry_worst(bad)
    bound = ec.carry_budget(31, ec.start_sincos_ulps(start))
    assert err[-1] > bound and norm[-1] > bound


def test_the_stale_verdict_is_what_the_expression_dictates():
    start, d, verdict = ec.threshold_cases()
    out = ec.restated_trig_carry(start, d)
    assert verdict.tolist() == [0, 0, 1, 0, 1, 0, 1, 1, 0, 1]           # 4e-3 and -4e-3 inside; a lone NaN increment dropped by fmax
    assert out[0, 3].tolist() == verdict.tolist()
