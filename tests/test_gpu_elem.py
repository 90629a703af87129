"""The device's own elementary functions against multiprecision values (tests/elem_cases.py; the rules and budgets are derived there,
and tests/test_elem_cpu.py shows each able to fail):
  * the sin/cos pair in its three forms (literals, table in scalar registers, table in vector registers) gives the bits of the host
    restatement oracle/f16_elem_oracle.c on every argument -- and the restatement, and so the device, lies within the C library's own
    error + 2 ulp of the true value for |x| <= 1e6;
  * the power factor by three routes to 1 ulp of tfac^c, and mach, qbar, ps within their rounding budgets of the multiprecision
    atmosphere on [0, 1e5] ft;
  * f16_rcp to 1 ulp of 1 / x, and the plant's tangent within its budget of tan(theta);
  * the sin/cos pairs carried through 1, 31 and 32 rotations within the rotation budget of the stored angle's sin / cos, the bits of
    the restated rotation, and the stale verdict the threshold expression dictates."""
import ctypes
import math

import numpy as np
import pytest

import elem_cases as ec

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def dev(hip):
    from f16_mpc_oop_py_amd import lib

    class Dev:
        L, ctx = hip, lib.Context(0)

        def run(self, entry, inputs, rows_out, *extra):
            """one launch of a f16_debug_elem_* entry: inputs [rows][n] -> [rows_out][n]"""
            inputs = np.ascontiguousarray(np.atleast_2d(inputs), dtype=np.float64)
            n = inputs.shape[1]
            out = np.full((rows_out, n), 123.0)
            lib.check(getattr(hip, entry)(self.ctx.handle, inputs.ctypes.data_as(ctypes.c_void_p), *extra, n, out.ctypes.data_as(ctypes.c_void_p)), hip)
            return out

    return Dev()


def test_argument_rules_of_the_new_entries(dev):
    L, h = dev.L, dev.ctx.handle
    buf = np.zeros(64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    for name in ("f16_debug_elem_sincos", "f16_debug_elem_atmos", "f16_debug_elem_rcp", "f16_debug_elem_tan"):
        f = getattr(L, name)
        assert f(h, p, 0, p) == 0 and f(None, p, 1, p) == EINVAL and f(h, None, 1, p) == EINVAL and f(h, p, 1, None) == EINVAL and f(h, p, -1, p) == EINVAL, name
        assert name in L.f16_last_error().decode()
    f = L.f16_debug_elem_trig_carry
    assert f(h, p, 1, 0, p) == 0 and f(h, p, 0, 1, p) == EINVAL and f(h, p, 4097, 1, p) == EINVAL and f(None, p, 1, 1, p) == EINVAL and f(h, p, 1, -1, p) == EINVAL
    assert (buf == 0).all()


# ---------------------------------------------------------------- sin / cos
def test_three_forms_of_sincos_give_the_bits_of_the_host_restatement(dev):
    x = ec.sincos_bit_arguments()
    out = dev.run("f16_debug_elem_sincos", x, 6)
    s, c = ec.restated_sincos(x)
    for k, form in enumerate(("literals", "table in scalar registers", "table in vector registers")):
        assert ec.same_bits(out[2 * k], s) and ec.same_bits(out[2 * k + 1], c), form
    fin = np.isfinite(x)
    assert np.isnan(out[:, ~fin]).all() and np.isfinite(out[:, fin]).all() and (~fin).sum() == 3
    zero = x == 0
    assert zero.sum() >= 2 and (out[0::2, zero] == 0).all() and not np.signbit(out[0::2, zero]).any() and (out[1::2, zero] == 1).all()
    print(f"MEASURED sincos_bf, sincos_bf_k<KScalar>, sincos_bf_k<KVector>: {x.size} arguments, 0 differ from the host restatement / 0 allowed")


@pytest.mark.parametrize("family", ec.ACCURACY_FAMILIES)
def test_device_sincos_within_libm_plus_two_ulp_of_the_true_value(dev, family):
    x, ts, tc = ec.sincos_truth(family)
    out = dev.run("f16_debug_elem_sincos", x, 6)
    worst = 0.0
    for k in range(3):
        w, bound, Y = ec.sincos_rule(x, ts, tc, out[2 * k], out[2 * k + 1])
        worst = max(worst, w)
    print(f"MEASURED device sincos, {family} ({x.size} arguments, three forms): worst {worst:.3f} ulp of the true value / bound {bound:.3f} (libm {Y:.3f} + 2)")
    assert worst <= bound


def test_device_sincos_beyond_1e6(dev):
    """printed per decade; asserted: the restatement's bits, finite results, NaN for non-finite arguments"""
    x, ts, tc = ec.sincos_truth("ladder")
    out = dev.run("f16_debug_elem_sincos", x, 6)
    s, c = ec.restated_sincos(x)
    for k in range(3):
        assert ec.same_bits(out[2 * k], s) and ec.same_bits(out[2 * k + 1], c)
    assert np.isfinite(out).all()
    e = np.maximum(ec.ulps(out[4], ts), ec.ulps(out[5], tc))
    n = np.rint(np.abs(x) * (2 / math.pi))
    for lo in (1e6, 1e7, 1e8, 1e9):
        m = (np.abs(x) >= lo) & (np.abs(x) < 10 * lo) & (n < 2.0 ** 31 - 1)
        print(f"MEASURED device sincos on [{lo:.0e}, {min(10 * lo, ec.TWO31_PIO2):.3e}): worst {e[m].max():.3f} ulp ({m.sum()} arguments; printed only)")
    m = n >= 2.0 ** 31 - 1
    print(f"MEASURED device sincos from 2^31 pi/2: worst absolute error {max(np.abs(out[4][m] - ts.hi[m]).max(), np.abs(out[5][m] - tc.hi[m]).max()):.3f} "
          f"({m.sum()} arguments; printed only)")
    assert np.isnan(dev.run("f16_debug_elem_sincos", ec.sincos_family("nonfinite"), 6)).all()


# ---------------------------------------------------------------- power factor and atmosphere
def test_power_factor_and_atmosphere_within_their_budgets(dev):
    frac = ec.header_pow_frac()
    alt, vt, truth = ec.atmos_truth(frac)
    out = dev.run("f16_debug_elem_atmos", np.stack([alt, vt]), 13)
    env = ec.envelope_lanes()
    assert ec.same_bits(out[0][env], truth["tfac"].hi[env])                       # tfac: ONE rounding (the premise of the truth)
    routes = [dict(zip(("factor", "mach", "qbar", "ps"), out[1 + 4 * r:5 + 4 * r])) for r in range(3)]
    for r, name in ((1, "exp_k / log_k, scalar registers"), (2, "exp_k / log_k, vector registers")):
        for k in routes[0]:
            assert ec.same_bits(routes[0][k], routes[r][k]), (name, k)            # identical bits, outside the envelope too
    worst = ec.atmos_worst(routes[0], truth, env)
    print(f"MEASURED device atmosphere on [0, 1e5] ft x vt {ec.VT}, c = {frac!r}, three routes with the same bits: " + ", ".join(
        f"{k} {v:.2f} / {ec.FACTOR_ULPS if k == 'factor' else ec.BUDGET_U[k]} {'ulp' if k == 'factor' else 'u'}" for k, v in worst.items()))
    assert ec.atmos_within_budget(worst), worst
    # outside the envelope: printed only where the truth exists (tfac > 1 below sea level, tfac -> 0+), NaN where it does not
    defined = np.isfinite(truth["factor"].hi) & ~env
    if defined.any():
        w = ec.atmos_worst(routes[0], truth, defined)
        print("MEASURED device atmosphere outside the envelope (printed only): " + ", ".join(f"{k} {v:.2f}" for k, v in w.items()))
    assert np.isnan(routes[0]["factor"][np.isnan(alt)]).all() and np.isnan(routes[0]["qbar"][np.isnan(alt)]).all()


# ---------------------------------------------------------------- reciprocal, tangent
def test_f16_rcp_within_one_ulp_of_the_reciprocal(dev):
    """over ALL normal finite x, as the plant header promises; the arguments above 2^1022, whose reciprocal is a denormal, are part of
    the assertion and printed on their own first"""
    x, promised = ec.rcp_arguments()
    got = dev.run("f16_debug_elem_rcp", x, 1)[0]
    e = ec.ulps(got, ec.rcp_truth())
    big = promised & (np.abs(x) > 2.0 ** 1022)
    inner = promised & ~big
    print(f"MEASURED f16_rcp over {inner.sum()} normal arguments up to 2^1022: worst {e[inner].max():.3f} ulp of 1/x / bound {ec.RCP_ULPS}")
    k = np.flatnonzero(big)[np.argmax(e[big])]
    print(f"MEASURED f16_rcp over {big.sum()} normal arguments above 2^1022 (denormal reciprocal): worst {e[big].max():.3f} ulp of 1/x / bound "
          f"{ec.RCP_ULPS}, at x = {x[k]!r}: {got[k]!r}; {(e[big] > ec.RCP_ULPS).sum()} beyond the bound, {(~np.isfinite(got[big])).sum()} not finite")
    with np.errstate(divide="ignore", over="ignore"):
        for v, g in zip(x[~promised], got[~promised]):
            print(f"MEASURED f16_rcp({v!r}) = {g!r} (1 / x = {np.float64(1) / v!r}; outside the promise, printed only)")
    assert big.sum() >= 12 and e[promised].max() <= ec.RCP_ULPS


def test_tangent_of_the_plant_within_its_budget(dev):
    th = ec.tan_arguments()
    st, ct, tt = dev.run("f16_debug_elem_tan", th, 3)
    s, c = ec.restated_sincos(th)
    assert ec.same_bits(st, s) and ec.same_bits(ct, c)
    bound = ec.tan_budget(ec.start_sincos_ulps(th))
    worst = ec.rel_u(tt, ec.tan_truth()).max()
    print(f"MEASURED st * f16_rcp(ct) against tan(theta), {th.size} angles: {worst:.2f} u / budget {bound:.2f} u")
    assert worst <= bound


# ---------------------------------------------------------------- carried pairs
@pytest.mark.parametrize("n_steps", ec.CARRY_LENGTHS)
def test_carried_pairs_within_the_rotation_budget(dev, n_steps):
    start, steps = ec.carry_cases(n_steps)
    out = dev.run("f16_debug_elem_trig_carry", np.vstack([start[None], steps]), 4 * n_steps, n_steps).reshape(n_steps, 4, start.size)
    assert ec.same_bits(out, ec.restated_trig_carry(start, steps))               # products and fused operations only: the same bits
    assert (out[:, 3] == 0).all()
    err, norm = ec.carry_worst(out)
    bound = np.array([ec.carry_budget(k + 1, ec.start_sincos_ulps(start)) for k in range(n_steps)])
    print(f"MEASURED device carried pairs, {n_steps} rotations: |s - sin|, |c - cos| {err[-1]:.2f} u / budget {bound[-1]:.2f} u; "
          f"|s^2 + c^2 - 1| {norm[-1]:.2f} u / the same budget")
    assert (err <= bound).all() and (norm <= bound).all()


def test_stale_verdict_at_the_threshold(dev):
    start, d, verdict = ec.threshold_cases()
    out = dev.run("f16_debug_elem_trig_carry", np.vstack([start[None], d]), 4, 1)
    print(f"MEASURED trig_advance verdicts for increments {d[0].tolist()}: {out[3].tolist()} / expected {verdict.tolist()}")
    assert out[3].tolist() == verdict.tolist()
