"""The families, the extended-precision reference, the yardstick and the comparison of tests/test_air_cpu.py and
tests/test_gpu_air.py, defined once.

Rule under test (include/f16_hip.h "STEADY WIND"; csrc/f16_wind.hpp: calc_xdot_wind behind f16_xdot_wind_batch and every wind,
ensemble and observer rollout): the derivative of the plant in moving air.

Reference: the same rule in ONE evaluation of the plant in `long double` (oracle/f16_oracle.c: f16o_xdot_wind_batch of
libf16_oracle_ld.so; 64-bit significand) from the same fp64 inputs.  Not tests/wind_cases.py `twin_xdot`, which rebuilds the
derivative from two still-air evaluations in fp64 and is itself up to 1e-13 away.

Yardstick and tolerance: tests/linearise_cases.py's, with its factor.  Per FAMILY and output row k,
    Y[k] = max over the family's rows of |fp64 restatement - reference|,
computed when the test runs from the two CPU libraries alone; a candidate passes when |candidate - reference| <= 8 Y[k] on every
row and entry (Y[k] = 0: equal to the reference).  No finite row is left out.  A family is homogeneous in conditioning on purpose --
Y is a family maximum, and ill-conditioned rows must not lend theirs to well-conditioned ones.

Families, on the in-box rows of envelope_cases.hifi_lattice() / lofi_lattice().  "Residual r": the wind is chosen on the host so that
the air velocity in body axes is the vector r, w_ned = C^T (uvw_ground - r) in fp64; the realised triple differs from r by rounding,
which does not matter: both sides evaluate the rule from the same fp64 inputs.
  interior            wind_cases.air: wind <= 100 ft/s, gust <= 30 ft/s (hifi also at xcg 0.35 and under F16_FLAG_FIX_CLR)
  wind_only, gust_only   the same rows with the other three components zero; the device is called with that pointer NULL
  low_<m>             |r| = m in a seeded random body direction, m = 0.004, 0.0099, 0.0101, 0.02, 1, 10 ft/s: the two straddling values
                      sit either side of every 0.01 clamp
  sideways            r_y = +-300, r_x and r_z of either sign in [1e-3, 1] ft/s: |beta_a| within 0.27 degrees of 90 (asin near +-1)
  backwards, backwards_50   r_x = -200, r_y in +-20, r_z = +-1e-6 (alpha_a next to +-180 degrees on both sides) or +-50
  grid                |r| = 400, alpha_a 1e-6 degrees either side of -20, 45 and 90 degrees, or beta_a 1e-6 degrees either side of +-30,
                      the ground triple wherever the lattice has it
  exact               hand-made rows with phi = theta = psi = alpha = beta = 0, so U = vt and wb = w_ned exactly: vt_a == 0, Ua = Wa = 0,
                      signed zeros, alpha_a = +-pi, NaN wind and gust components, vt_a a power of two either side of 0.01
"""
import collections

import numpy as np

import envelope_cases as ec
import linearise_cases as lc
import wind_cases as wc

FACTOR = lc.FACTOR                               # 8: the project's, not to be raised
GRID_BITS = lc.GRID_BITS
FLAG_FIX_CLR = lc.FLAG_FIX_CLR
R2D = 180.0 / np.pi
LOW = (0.004, 0.0099, 0.0101, 0.02, 1.0, 10.0)
ALPHA_BOUNDS, BETA_BOUNDS, BOUND_STEP = (-20.0, 45.0, 90.0), (-30.0, 30.0), 1e-6     # degrees

Family = collections.namedtuple("Family", "kind fidelity xcg fix_clr", defaults=(0.25, 0))
KINDS = ("interior", "wind_only", "gust_only") + tuple(f"low_{m}" for m in LOW) + ("sideways", "backwards", "backwards_50", "grid")
FAMILIES = [Family(k, f) for f in ("hifi", "lofi") for k in KINDS] + [Family("interior", "hifi", 0.35), Family("interior", "hifi", 0.25, 1)]
EXACT = [Family("exact", "hifi"), Family("exact", "lofi")]


def fid(fam):
    return "/".join([fam.kind, fam.fidelity] + (["xcg35"] if fam.xcg != 0.25 else []) + (["clr"] if fam.fix_clr else []))


def fi_of(fam):
    return 1 if fam.fidelity == "hifi" else 0


def rows_in_box(fidelity):
    """(x, u) of the lattice rows that lie inside the envelope box"""
    b = ec.hifi_lattice() if fidelity == "hifi" else ec.lofi_lattice()
    ok = np.all((b.x >= ec.X_LB) & (b.x <= ec.X_UB), 1)
    return b.x[ok].copy(), b.u[ok].copy()


# ------------------------------------------------------------------------------------------------ the rule in numpy (fp64)
def rotation(x):
    """C = body from NED per row [B, 3, 3], the entries as the rule writes them"""
    sphi, cphi, st, ct, spsi, cpsi = np.sin(x[:, 3]), np.cos(x[:, 3]), np.sin(x[:, 4]), np.cos(x[:, 4]), np.sin(x[:, 5]), np.cos(x[:, 5])
    return np.stack([np.stack([ct * cpsi, ct * spsi, -st], 1),
                     np.stack([sphi * st * cpsi - cphi * spsi, sphi * st * spsi + cphi * cpsi, sphi * ct], 1),
                     np.stack([cphi * st * cpsi + sphi * spsi, cphi * st * spsi - sphi * cpsi, cphi * ct], 1)], 1)


def ground_uvw(x):
    vt = np.where(x[:, 6] <= 0.01, 0.01, x[:, 6])
    ca, sa, cb, sb = np.cos(x[:, 7]), np.sin(x[:, 7]), np.cos(x[:, 8]), np.sin(x[:, 8])
    return np.stack([vt * ca * cb, vt * sb, vt * sa * cb], 1)


def triple_np(x, air, wrong=None):
    """[B, 6] = Ua Va Wa vt_a alpha_a beta_a, the expressions in the rule's order in numpy fp64.  wrong: a deliberately wrong rule"""
    C, g = rotation(x), ground_uvw(x)
    wn, we, wd = air[:, 0], air[:, 1], air[:, 2]
    wb = [C[:, i, 0] * wn + C[:, i, 1] * we + C[:, i, 2] * wd for i in range(3)]
    if wrong == "plus_wd":
        wb[0] = C[:, 0, 0] * wn + C[:, 0, 1] * we + wd
    Ua, Va, Wa = g[:, 0] - wb[0] - air[:, 3], g[:, 1] - wb[1] - air[:, 4], g[:, 2] - wb[2] - air[:, 5]
    if wrong == "gust_dropped_from_va":
        Va = g[:, 1] - wb[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        vt = np.sqrt(Ua * Ua + Va * Va + Wa * Wa)
        beta = np.arctan2(Va, Ua) if wrong == "beta_atan2" else np.arcsin(Va / vt)
        return np.stack([Ua, Va, Wa, vt, np.arctan2(Wa, Ua), beta], 1)


WRONG = ("beta_atan2", "lef_ground_alpha", "damping_ground_vt", "plus_wd", "gust_dropped_from_va", "lef_clamped_vt")


def parts_np(x, air, wrong=None):
    """what oracle f16o_xdot_air_parts_batch takes, [B, 6] = vt (atmosphere), vt (damping), alpha, beta (lookups), V, alpha (flap
    model), under the rule (wrong = None) or one of WRONG"""
    t = triple_np(x, air, wrong)
    vc = np.where(t[:, 3] <= 0.01, 0.01, t[:, 3])
    p = np.stack([vc, vc, t[:, 4], t[:, 5], t[:, 3], t[:, 4]], 1)
    if wrong == "lef_ground_alpha":
        p[:, 5] = x[:, 7]
    if wrong == "damping_ground_vt":
        p[:, 1] = np.where(x[:, 6] <= 0.01, 0.01, x[:, 6])
    if wrong == "lef_clamped_vt":
        p[:, 4] = vc
    return p


def stand_in(fam, wrong=None):
    """the fp64 checker's plant fed the numpy triple: with wrong = None a second fp64 statement of the rule (numpy's sin / cos / atan2
    / asin), else a wrong rule -> xdot [B, 18]"""
    c = cases(fam)
    x = c.get("x_rule", c["x"])
    out, _ = libs()["fp64"].xdot_air_parts_batch(x, c["u"], parts_np(x, c["air"], wrong), fi_of(fam), fam.xcg, fam.fix_clr)
    return out


# ------------------------------------------------------------------------------------------------ the families
def residual_air(x, r):
    """air [B, 6] with the gust zero and the wind such that the air velocity in body axes is r [B, 3]"""
    d = ground_uvw(x) - r
    w = np.einsum("bji,bj->bi", rotation(x), d)
    return np.concatenate((w, np.zeros_like(w)), 1)


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _signed(rng, lo, hi, n):
    return rng.choice([-1.0, 1.0], n) * rng.uniform(lo, hi, n)


def exact_rows(fidelity):
    """(x, u, air): a level aircraft with every angle zero at vt = 512, so that U = vt and wb = w_ned without rounding"""
    x0, u0 = rows_in_box(fidelity)
    x, u = x0[7].copy(), u0[7].copy()
    x[3:6], x[6], x[7], x[8] = 0.0, 512.0, 0.0, 0.0
    x[17], x[16] = 2.0, 4.0                         # the flap model away from both of its clamps: lef_cmd = 4.21, rate 1.5 deg/s
    nan = np.nan
    spec = [  # (alpha, wN, wE, wD, gx, gy, gz)
        (0.0, 512.0, 0, 0, 0, 0, 0),                   # vt_a == 0
        (0.0, 512.0, 0, 0, 0, -300.0, 0),              # Ua = Wa = 0, Va = 300
        (0.0, 512.0, 0, 0, 0, 300.0, 0),               # Va = -300
        (-0.0, 512.0, 0, 0, 0, -300.0, 0),             # Wa = -0
        (-0.0, 512.0, 0, 0, 0, 0, 0),                  # vt_a == 0 with Wa = -0
        (0.0, 712.0, 0, 0, 0, 0, 0),                   # Ua = -200, Wa = +0: alpha_a = +pi
        (-0.0, 712.0, 0, 0, 0, 0, 0),                  # Ua = -200, alpha = -0.0: see x_rule below
        (0.0, 712.0, 0, 0, 0, 0, 2.0 ** -1000),        # Ua = -200, Wa = -2^-1000: alpha_a = -pi
        (0.0, 712.0, 0, 0, 0, 0, -2.0 ** -1000),       # Ua = -200, Wa = +2^-1000: alpha_a = +pi
        (0.0, 512.0, 0, 0, -0.0, 0, -0.0),             # signed-zero gusts
        (0.0, 512.0 - 2.0 ** -7, 0, 0, 0, 0, 0),       # vt_a = 2^-7 exactly: below every 0.01 clamp
        (0.0, 512.0 - 2.0 ** -6, 0, 0, 0, 0, 0),       # vt_a = 2^-6 exactly: above
        (0.0, nan, 0, 0, 0, 0, 0), (0.0, 30.0, nan, 0, 0, 0, 0), (0.0, 30.0, 0, 0, 0, 0, nan), (0.0, 30.0, 0, 0, nan, 0, 0),
        (0.0, 30.0, 5.0, -3.0, 2.0, 1.0, -4.0),        # an ordinary row
    ]
    X, A = np.tile(x, (len(spec), 1)), np.zeros((len(spec), 6))
    for k, s in enumerate(spec):
        X[k, 7], A[k] = s[0], s[1:]
    return X, np.tile(u, (len(spec), 1)), A


_CASES = {}


def cases(fam):
    """dict(x [B, 18], u [B, 4], air [B, 6], wind_null, gust_null: the device is called with that pointer NULL)"""
    key = (fam.kind, fam.fidelity)
    if key in _CASES:
        return _CASES[key]
    kind = fam.kind
    if kind == "exact":
        x, u, air = exact_rows(fam.fidelity)
        # include/f16_hip.h "STEADY WIND": the default build's sin(-0.0) is +0.0, an angle of -0.0 acts as +0.0.  The reference is
        # evaluated at x_rule = x + 0.0 (only a -0.0 changes); the device is given x as it is.
        _CASES[key] = dict(x=x, x_rule=x + 0.0, u=u, air=air, wind_null=False, gust_null=False)
        return _CASES[key]
    x, u = rows_in_box(fam.fidelity)
    B = len(x)
    rng = np.random.default_rng(9000 + KINDS.index(kind) * 2 + fi_of(fam))
    wind_null = gust_null = False
    if kind in ("interior", "wind_only", "gust_only"):
        w, g = wc.air(B, 60 + fi_of(fam))
        air = np.concatenate((w, g[0]), 1)
        if kind == "wind_only":
            air[:, 3:], gust_null = 0.0, True
        if kind == "gust_only":
            air[:, :3], wind_null = 0.0, True
    else:
        if kind.startswith("low_"):
            r = float(kind[4:]) * _unit(rng, B)
        elif kind == "sideways":
            r = np.stack([_signed(rng, 1e-3, 1.0, B), rng.choice([-300.0, 300.0], B), _signed(rng, 1e-3, 1.0, B)], 1)
        elif kind == "backwards":
            r = np.stack([np.full(B, -200.0), rng.uniform(-20, 20, B), rng.choice([-1e-6, 1e-6], B)], 1)
        elif kind == "backwards_50":
            r = np.stack([np.full(B, -200.0), rng.uniform(-20, 20, B), rng.choice([-50.0, 50.0], B)], 1)
        else:
            assert kind == "grid"
            sets = [("a", b_ + s) for b_ in ALPHA_BOUNDS for s in (-BOUND_STEP, BOUND_STEP)] + \
                   [("b", b_ + s) for b_ in BETA_BOUNDS for s in (-BOUND_STEP, BOUND_STEP)]
            al, be = rng.uniform(-15.0, 40.0, B), rng.uniform(-25.0, 25.0, B)
            for k in range(B):
                which, deg = sets[k % len(sets)]
                if which == "a":
                    al[k] = deg
                else:
                    be[k] = deg
            al, be = al / R2D, be / R2D
            r = 400.0 * np.stack([np.cos(al) * np.cos(be), np.sin(be), np.sin(al) * np.cos(be)], 1)
        air = residual_air(x, r)
    _CASES[key] = dict(x=x, u=u, air=air, wind_null=wind_null, gust_null=gust_null)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ reference and yardstick
_LIBS = {}


def libs():
    """{"fp64", "fma", "ld"}: the moving-air view of the three builds (linearise_cases.libs() runs make first)"""
    if not _LIBS:
        from oracle import air_oracle
        for k in lc.libs():
            _LIBS[k] = air_oracle.AirOracle(k)
    return _LIBS


def run(lib, fam):
    c = cases(fam)
    return lib.xdot_wind_batch(c.get("x_rule", c["x"]), c["u"], c["air"], fi_of(fam), fam.xcg, fam.fix_clr)


_REF = {}


def reference(fam):
    """dict(ref [B, 18] longdouble, tri [B, 6] longdouble, x64 the fp64 restatement, Y [18] longdouble, status [B]) once per process.
    Families other than `exact`: every row finite in both builds, the two builds raise the same grid bits (a family where they do
    not is mis-built), and what the family promises about its triple holds on the reference."""
    if fam in _REF:
        return _REF[fam]
    L = libs()
    ref, tri, st = run(L["ld"], fam)
    x64, tri64, st64 = run(L["fp64"], fam)
    assert ref.dtype == np.longdouble and np.finfo(np.longdouble).nmant >= 63
    if fam.kind == "exact":
        assert np.array_equal(np.isnan(ref), np.isnan(x64)) and np.array_equal(st, st64)
        _REF[fam] = dict(ref=ref, tri=tri, x64=x64, Y=reference(Family("interior", fam.fidelity))["Y"], status=st)
        return _REF[fam]
    assert np.isfinite(ref).all() and np.isfinite(x64).all(), fid(fam)
    assert np.array_equal(st, st64), (fid(fam), np.nonzero(st != st64)[0][:5])
    t = tri.astype(np.float64)
    if fam.kind == "sideways":
        assert np.hypot(t[:, 0], t[:, 2]).min() >= 5e-4 and (np.abs(np.abs(t[:, 5]) * R2D - 90.0) < 0.28).all()   # atan(sqrt(2) / 300)
    if fam.kind.startswith("backwards"):
        assert (t[:, 0] < -199.0).all()
        if fam.kind == "backwards":
            assert (np.pi - np.abs(t[:, 4]) < 1e-7).all() and (t[:, 4] > 0).any() and (t[:, 4] < 0).any()
    if fam.kind.startswith("low_"):
        m = float(fam.kind[4:])
        assert np.abs(t[:, 3] / m - 1).max() < 1e-3 and ((t[:, 3] <= 0.01).all() if m < 0.01 else (t[:, 3] > 0.01).all())
    if fam.kind == "grid":
        da = np.abs(tri[:, 4:5] - np.asarray(ALPHA_BOUNDS, dtype=np.longdouble) / R2D)
        db = np.abs(tri[:, 5:6] - np.asarray(BETA_BOUNDS, dtype=np.longdouble) / R2D)
        assert min(da.min(), db.min()) >= 1e-9                        # no row is ON a bound: the status comparison has no excuse
        assert (da.min(1) < 2e-8).sum() + (db.min(1) < 2e-8).sum() == len(t)   # and every row is beside one
        if fam.fidelity == "hifi":
            assert {int(s) for s in st} >= {0, 2, 3, 4}               # inside, ALPHA2, ALPHA1 | ALPHA2, BETA all occur
    Y = np.abs(x64.astype(np.longdouble) - ref).max(0)
    _REF[fam] = dict(ref=ref, tri=tri, x64=x64, Y=Y, status=st)
    return _REF[fam]


def ratios(cand, fam, rows=None):
    """(worst |cand - ref| / Y per output row [18] over the entries with Y > 0, the entries [B, 18] where the rule fails).  In the
    `exact` family the NaN pattern must be the reference's entry by entry and the finite entries fall under the interior family's Y"""
    r = reference(fam)
    ref = r["ref"] if rows is None else r["ref"][rows]
    Y = r["Y"]
    cand = np.asarray(cand)
    assert cand.shape == ref.shape, (cand.shape, ref.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(cand.astype(np.longdouble) - ref)
        bad = ~(err <= FACTOR * Y)                                   # a NaN fails
        both = np.isnan(ref) & np.isnan(cand)
        bad &= ~both
        q = np.where((Y > 0) & ~both, err / np.where(Y > 0, Y, 1), 0)
    return q.max(0).astype(np.float64), bad


def check(cand, fam, rows=None, what=""):
    """the 8 x Y rule on every row and entry; returns the worst ratio per output row [18]"""
    worst, bad = ratios(cand, fam, rows)
    if bad.any():
        r = reference(fam)
        ref = r["ref"] if rows is None else r["ref"][rows]
        lines = [f"  row {a} entry {k}: got {float(cand[a, k])!r} ref {float(ref[a, k])!r} Y {float(r['Y'][k]):.3e}" for a, k in np.argwhere(bad)[:8]]
        raise AssertionError(f"{what} {fid(fam)}: {int(bad.sum())} entries beyond {FACTOR} x Y (worst ratio {np.nanmax(worst):.3g})\n" + "\n".join(lines))
    return worst


def fails(cand, fam):
    return bool(ratios(cand, fam)[1].any())


def yardstick_line(fam):
    """'Y / max|xdot|' over rows 6..11 of the family, smallest .. largest"""
    r = reference(fam)
    with np.errstate(invalid="ignore"):
        rel = (r["Y"][6:12] / np.nanmax(np.abs(r["ref"][:, 6:12]), 0)).astype(np.float64)
    return f"Y / max|xdot| rows 6..11 {rel.min():.1e} .. {rel.max():.1e}"


# ------------------------------------------------------------------------------------------------ the air triple alone, against mpmath
# What f16_debug_air_triple returns (csrc/f16_wind.hpp air_triple, the function calc_xdot_wind evaluates in front of its lookups) held
# to 60-digit mpmath.  Two checks, so that the cancellation and the device's own sqrt / atan2 / asin are each judged on their own:
#   (i)  Ua, Va, Wa against the rule evaluated in mpmath from the fp64 inputs: absolute error in units of u S, u = 2^-53,
#        S = |U| + |V| + |W| + |w|_1 + |g|_1 -- the size of what cancels;
#   (ii) vt_a, alpha_a, beta_a against mpmath applied to the candidate's OWN Ua, Va, Wa.
# The budgets are derived below from the expressions as coded, one u per rounding; nothing in them is fitted to a result.
MP_DIGITS = 60
U53 = 2.0 ** -53
SECOND_ORDER = 1 + 2.0 ** -40                    # (1 + u)^k - 1 <= k u (1 + 2^-40) for every k used here
SINCOS_ULPS = 1.3                                # include/f16_hip.h: the default build's pair is within 1.3 ulp for |x| <= 1e6
LIBM_PLUS = 2.0                                  # elem_cases.py "Y + 2": a device function standing where libm stands


def uvw_budget(sincos_ulps=SINCOS_ULPS):
    """the absolute error of Ua, Va or Wa in units of u S.  One ulp of a sin or cos is at most 2 u relative (e = 2 x sincos_ulps).
      U = fl(fl(vt ca) cb), W likewise      two pairs and two products: (2 e + 2) |U|;      V = fl(vt sb): (e + 1) |V|
      wb_x = c1 wN + c2 wE - st wD          c1 = fl(ct cpsi): two pairs and a product, times wN another: (2 e + 2) |wN|; the third term
                                            (e + 1) |wD|; two additions, each one u of a partial sum <= |w|_1: (2 e + 4) |w|_1
      wb_y, wb_z                            the widest coefficient is fl(fl(fl(sphi st) cpsi) - fl(cphi spsi)): three pairs and two
                                            products on one side, (3 e + 2), one subtraction (the two sides together are <= 1 by
                                            Cauchy-Schwarz), the product with wN, the two additions: (3 e + 6) |w|_1
      Ua = fl(fl(U - wb_x) - g_x)           two roundings of sums <= |U| + |w|_1 + |g_x|: 2 (|U| + |w|_1 + |g|_1)
    In all: Ua <= (2 e + 4) |U| + (2 e + 6) |w|_1 + 2 |g|_1, Va <= (e + 3) |V| + (3 e + 8) |w|_1 + 2 |g|_1, Wa <= (2 e + 4) |W| +
    (3 e + 8) |w|_1 + 2 |g|_1; the largest coefficient, 3 e + 8, bounds each in units of u S (15.8 at 1.3 ulp).  FMA contraction
    removes roundings and adds none."""
    e = 2 * sincos_ulps
    return (3 * e + 8) * SECOND_ORDER


def vt_budget():
    """vt_a = sqrt(Ua Ua + Va Va + Wa Wa) against the true root of the candidate's own three numbers, relative, in u: each square one
    rounding, two additions of non-negative terms one each -- the sum within 3 u; the root halves that and rounds once: 2.5 u"""
    return 2.5 * SECOND_ORDER


QUOTIENT_U = 2.5 + 1.0                           # Va / vt_a: the root's 2.5 u and the division's own rounding


def _mp():
    import mpmath
    return mpmath


def triple_cases():
    """in12 [12, n] = phi theta psi vt alpha beta | wN wE wD | gx gy gz, the layout of f16_debug_air_triple: every sixth row of the
    hifi low-speed, sideways, backwards and grid families, the finite rows of the exact family, and hand-made triples through a level
    aircraft at vt = 1 with every angle zero (Ua = 1 - g_x, Va = -g_y, Wa = -g_z; alpha = -0 gives Wa = -0, beta = -0 gives Va = -0):
    quotients Va / vt_a within a few ulp of +-1, and atan2 arguments on all four half-axes with both signs of a zero Wa.  (Ua = -0
    cannot arise: U - wb_x with U > 0.)"""
    blocks = []
    for kind in KINDS[3:]:
        c = cases(Family(kind, "hifi"))
        blocks.append(np.concatenate((c["x"][::6, 3:9], c["air"][::6]), 1))
    x, _, air = exact_rows("hifi")
    fin = np.isfinite(air).all(1)
    blocks.append(np.concatenate((x[fin, 3:9], air[fin]), 1))
    hand = []
    for va in (300.0, -300.0):
        for k in (0.0, 0.3, 1.0, 2.0, 4.0, 8.0, 64.0):                # 1 - |r| = k 2^-53, to first order
            h = abs(va) * np.sqrt(2 * k) * 2.0 ** -26.5
            hand += [(0.0, 0.0, h, va, 0.0), (0.0, 0.0, -0.6 * h, va, 0.8 * h)]
    hand += [(0.0, 0.0, -7.0, 0.0, 2.0 ** -1000), (0.0, 0.0, -7.0, 0.0, -2.0 ** -1000)]                # either side of +-pi
    for ua in (7.0, -7.0, 2.0 ** -20, -2.0 ** -20, 1e6):
        hand += [(0.0, 0.0, ua, 0.0, 0.0), (-0.0, 0.0, ua, 0.0, 0.0), (0.0, -0.0, ua, 0.0, 0.0)]      # Wa = +0, -0; Va = -0
    for wa in (3.0, -3.0, 2.0 ** -20, -2.0 ** -20):
        hand += [(0.0, 0.0, 0.0, 0.0, wa), (0.0, 0.0, 0.0, 2.0, wa)]                                  # Ua = +0
    rows = np.zeros((len(hand), 12))
    for i, (al, be, ua, va, wa) in enumerate(hand):
        rows[i, 3], rows[i, 4], rows[i, 5] = 1.0, al, be
        rows[i, 9:] = 1.0 - ua, -va, -wa
    blocks.append(rows)
    return np.ascontiguousarray(np.concatenate(blocks).T)


def triple_numpy(in12):
    """[6, n]: the rule in numpy fp64 (the C library's sin / cos / sqrt / atan2 / asin): the stand-in of the CPU module"""
    x = np.zeros((in12.shape[1], 18))
    x[:, 3:9] = in12[:6].T
    return np.ascontiguousarray(triple_np(x, np.ascontiguousarray(in12[6:].T)).T)


_TRUTH = {}


def uvw_truth(in12):
    """(Ua, Va, Wa as lists of mpf [3][n], S [n]) from the fp64 inputs at MP_DIGITS, once per process"""
    key = in12.tobytes()
    if key not in _TRUTH:
        mpm = _mp()
        out, S = [[], [], []], []
        with mpm.workdps(MP_DIGITS):
            for c in in12.T:
                phi, th, psi, vt, al, be, wn, we, wd, gx, gy, gz = [mpm.mpf(float(v)) for v in c]
                vt = max(vt, mpm.mpf(0.01))
                sphi, cphi, st, ct, spsi, cpsi = mpm.sin(phi), mpm.cos(phi), mpm.sin(th), mpm.cos(th), mpm.sin(psi), mpm.cos(psi)
                U, V, W = vt * mpm.cos(al) * mpm.cos(be), vt * mpm.sin(be), vt * mpm.sin(al) * mpm.cos(be)
                out[0].append(U - (ct * cpsi * wn + ct * spsi * we - st * wd) - gx)
                out[1].append(V - ((sphi * st * cpsi - cphi * spsi) * wn + (sphi * st * spsi + cphi * cpsi) * we + sphi * ct * wd) - gy)
                out[2].append(W - ((cphi * st * cpsi + sphi * spsi) * wn + (cphi * st * spsi - sphi * cpsi) * we + cphi * ct * wd) - gz)
                S.append(float(abs(U) + abs(V) + abs(W) + abs(wn) + abs(we) + abs(wd) + abs(gx) + abs(gy) + abs(gz)))
        _TRUTH[key] = (out, np.array(S))
    return _TRUTH[key]


def triple_figures(in12, got):
    """got [6, n] = a candidate's Ua Va Wa vt_a alpha_a beta_a -> dict of (worst figure, bound) per check:
      uvw     |got - truth| / (u S)                                                    against uvw_budget()
      vt      relative error of vt_a against the true root of got's own (Ua, Va, Wa), in u    against vt_budget()
      alpha   error of alpha_a in ulps of the true atan2(Wa, Ua) of got's own numbers         against Y + 2, Y the host libm's own
      beta    error of beta_a beyond what QUOTIENT_U u in the quotient can move asin by -- asin(clip(r (1 +- 3.5 u))) in mpmath,
              no first-order step, so it holds up to |r| = 1 -- in ulps of the true asin      against Y + 2, Y the host libm's own
    and the signs of zero results (alpha_a on the positive Ua half-axis) equal to the host libm's.  Rows where the truth is undefined
    (vt_a = 0: asin(0 / 0)) must be NaN in beta and are left out of the beta figure only."""
    mpm = _mp()
    got = np.asarray(got, dtype=np.float64)
    truth, S = uvw_truth(in12)
    n = in12.shape[1]
    assert got.shape == (6, n) and np.isfinite(got[:5]).all()
    fig = dict(uvw=0.0, vt=0.0, alpha=0.0, beta=0.0, alpha_Y=0.0, beta_Y=0.0)
    with mpm.workdps(MP_DIGITS), np.errstate(invalid="ignore", divide="ignore"):
        lib_alpha, lib_q = np.arctan2(got[2], got[0]), got[1] / got[3]
        lib_beta = np.arcsin(lib_q)
        for i in range(n):
            for k in range(3):
                fig["uvw"] = max(fig["uvw"], float(abs(mpm.mpf(got[k, i]) - truth[k][i]) / (U53 * S[i])))
            a, b, c = mpm.mpf(got[0, i]), mpm.mpf(got[1, i]), mpm.mpf(got[2, i])
            vt = mpm.sqrt(a * a + b * b + c * c)
            if vt == 0:
                assert got[3, i] == 0 and got[4, i] == 0 and np.isnan(got[5, i]), i
                continue
            fig["vt"] = max(fig["vt"], float(abs(mpm.mpf(got[3, i]) - vt) / vt / U53))
            ta = mpm.atan2(c, a)
            if c == 0 and a < 0 and np.signbit(got[2, i]):
                ta = -ta                                  # atan2(-0, Ua < 0) = -pi: mpmath has no signed zero
            ulp_a = float(np.spacing(abs(float(ta)))) if ta != 0 else 1.0
            fig["alpha"] = max(fig["alpha"], float(abs(mpm.mpf(got[4, i]) - ta)) / ulp_a)
            fig["alpha_Y"] = max(fig["alpha_Y"], float(abs(mpm.mpf(lib_alpha[i]) - ta)) / ulp_a)
            assert np.signbit(got[4, i]) == np.signbit(lib_alpha[i]), i
            r = b / vt
            tb = mpm.asin(r)
            d = QUOTIENT_U * SECOND_ORDER * U53
            moved = max(abs(mpm.asin(max(min(r * (1 + s * d), 1), -1)) - tb) for s in (-1, 1))
            ulp_b = float(np.spacing(abs(float(tb)))) if tb != 0 else 1.0
            assert np.isfinite(got[5, i]), i
            fig["beta"] = max(fig["beta"], float(max(abs(mpm.mpf(got[5, i]) - tb) - moved, 0)) / ulp_b)
            fig["beta_Y"] = max(fig["beta_Y"], float(abs(mpm.mpf(lib_beta[i]) - mpm.asin(mpm.mpf(lib_q[i])))) / ulp_b)
    return {"uvw": (fig["uvw"], uvw_budget()), "vt": (fig["vt"], vt_budget()), "alpha": (fig["alpha"], fig["alpha_Y"] + LIBM_PLUS),
            "beta": (fig["beta"], fig["beta_Y"] + LIBM_PLUS)}
