"""Argument families, multiprecision truth, the error measure and the rules for the default build's elementary functions
(f16_mpc_oop_py_amd/csrc/f16_plant.hpp: sincos_bf / sincos_bf_k, exp_k / log_k and the library composition, f16_rcp, trig_rotate /
trig_advance).  Shared by tests/test_elem_cpu.py (the host restatement and the stand-ins) and tests/test_gpu_elem.py (the device).

Truth is mpmath at PREC bits, kept as a pair of doubles (hi = the correctly rounded value, lo = truth - hi) and computed once per
process and family.  Errors are in ulps OF THE TRUE VALUE, |got - truth| / spacing(|hi|), or relative, |got - truth| / |truth|, in units
of u = 2^-53 (one rounding to nearest).  Where a bound is not a figure the project already states, it is a rounding budget derived
here -- one u per rounding of the expression as coded -- never a figure read off the code under test."""
import ctypes
import functools
import math
import os
import re
import subprocess

import mpmath
import numpy as np

from conftest import REPO

PREC = 256
U = 2.0 ** -53
SECOND_ORDER = 1 + 2.0 ** -40          # (1 + u)^k - 1 <= k u (1 + 2^-40) for every k used here
PLANT = os.path.join(REPO, "f16_mpc_oop_py_amd", "csrc", "f16_plant.hpp")
TWO31_PIO2 = 2.0 ** 31 * (math.pi / 2)           # from here on the quadrant of sincos_bf comes from a saturated integer


# ---------------------------------------------------------------- the host restatement and the stand-ins (oracle/f16_elem_oracle.c)
@functools.lru_cache(None)
def elem_lib():
    # always through make (incremental), as the `oracle` fixture does: a stale checker would compare the device with old code
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "oracle"), "libf16_elem_oracle.so"])
    L = ctypes.CDLL(os.path.join(REPO, "oracle", "libf16_elem_oracle.so"))
    L.f16o_sincos_bf_constants.restype = ctypes.c_int
    L.f16o_sincos_bf_constants.argtypes = [ctypes.c_void_p]
    L.f16o_sincos_bf_with.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    for f in (L.f16o_sincos_bf, L.f16o_libm_sincos):
        f.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    L.f16o_rcp_newton.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
    L.f16o_atmos_fast.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_double, ctypes.c_void_p]
    L.f16o_trig_carry.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_void_p]
    for f in (L.f16o_sincos_bf_with, L.f16o_sincos_bf, L.f16o_libm_sincos, L.f16o_rcp_newton, L.f16o_atmos_fast, L.f16o_trig_carry):
        f.restype = None
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def restated_constants():
    k = np.zeros(21)
    assert elem_lib().f16o_sincos_bf_constants(_p(k)) == 21
    return k


def restated_sincos(x, table=None):
    """(sin, cos) by the host restatement of sincos_bf; `table`: another 21 constants (a perturbed copy)"""
    x = _f64(x)
    s, c = np.empty_like(x), np.empty_like(x)
    if table is None:
        elem_lib().f16o_sincos_bf(_p(x), x.size, _p(s), _p(c))
    else:
        table = _f64(table)
        assert table.shape == (21,)
        elem_lib().f16o_sincos_bf_with(_p(table), _p(x), x.size, _p(s), _p(c))
    return s, c


def libm_sincos(x):
    x = _f64(x)
    s, c = np.empty_like(x), np.empty_like(x)
    elem_lib().f16o_libm_sincos(_p(x), x.size, _p(s), _p(c))
    return s, c


def rcp_model(x, steps=2):
    x = _f64(x)
    out = np.empty_like(x)
    elem_lib().f16o_rcp_newton(_p(x), x.size, steps, _p(out))
    return out


def atmos_model(alt, vt, frac):
    """dict of tfac, factor, rho, mach, qbar, ps by the C library stand-in of the fast atmosphere"""
    alt, vt = _f64(alt), _f64(vt)
    out = np.empty((6, alt.size))
    elem_lib().f16o_atmos_fast(_p(alt), _p(vt), alt.size, frac, _p(out))
    return dict(zip(("tfac", "factor", "rho", "mach", "qbar", "ps"), out))


def restated_trig_carry(start, steps):
    """start [n], steps [n_steps][n] -> [n_steps][4][n] = sin, cos, angle, verdict: the layout of f16_debug_elem_trig_carry"""
    buf = _f64(np.vstack([start[None], steps]))
    out = np.empty((steps.shape[0], 4, start.size))
    elem_lib().f16o_trig_carry(_p(buf), steps.shape[0], start.size, _p(out))
    return out


def header_sincos_constants():
    """the 21 literals of `constexpr SinCosK SINCOS_K = {...};` as f16_plant.hpp spells them, in order"""
    text = open(PLANT).read()
    body = re.search(r"constexpr\s+SinCosK\s+SINCOS_K\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
    return np.array([float(t) for t in re.findall(r"[-+]?\d\.\d+e[-+]\d+", body)])


def header_pow_frac():
    """the exponent fraction of the fast density as f16_plant.hpp defines it: the text of `constexpr double POW_FRAC = <expr>;`"""
    expr = re.search(r"constexpr\s+double\s+POW_FRAC\s*=\s*([^;]+);", open(PLANT).read()).group(1)
    assert re.fullmatch(r"[\d.\s+\-]+", expr), expr
    return float(eval(expr))


# ---------------------------------------------------------------- bits
def bits(a):
    return _f64(a).view(np.int64)


def same_bits(p, q):
    """NaN compared as NaN, everything else as bit patterns (-0 is not +0)"""
    p, q = _f64(p), _f64(q)
    nan = np.isnan(p) & np.isnan(q)
    return p.shape == q.shape and np.array_equal(np.isnan(p), np.isnan(q)) and np.array_equal(bits(p)[~nan], bits(q)[~nan])


def neighbours(x):
    """x with the double below and the double above each"""
    x = _f64(x)
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


# ---------------------------------------------------------------- truth and the measure
class Truth:
    """truth = hi + lo to ~2^-106 relative: hi the correctly rounded double, lo the rest"""

    def __init__(self, values):
        self.hi = np.array([float(v) for v in values])
        self.lo = np.array([float(v - mpmath.mpf(h)) if math.isfinite(h) else 0.0 for v, h in zip(values, self.hi)])

    def __getitem__(self, idx):
        t = Truth.__new__(Truth)
        t.hi, t.lo = self.hi[idx], self.lo[idx]
        return t


def ulps(got, truth):
    """|got - truth| / spacing(|fl(truth)|) per element; a NaN or infinite `got` where the truth is finite counts as inf"""
    got = _f64(got)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs((got - truth.hi) - truth.lo) / np.spacing(np.abs(truth.hi))
    return np.where(np.isfinite(got), e, np.inf)


def rel_u(got, truth):
    """|got - truth| / |truth| in units of u = 2^-53 (0 where both are 0)"""
    got = _f64(got)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e = np.abs((got - truth.hi) - truth.lo) / np.abs(truth.hi) / U
    e = np.where((got == 0) & (truth.hi == 0), 0.0, e)
    return np.where(np.isfinite(got), e, np.inf)


def mp(x):
    return mpmath.mpf(float(x))


@functools.lru_cache(None)
def sincos_truth(family):
    """(x, Truth of sin, Truth of cos) of a named family"""
    x = sincos_family(family)
    with mpmath.workprec(PREC):
        pairs = [mpmath.cos_sin(mp(v)) for v in x]
        return x, Truth([p[1] for p in pairs]), Truth([p[0] for p in pairs])


# ---------------------------------------------------------------- sin / cos families
EXPONENT_MANTISSAS = (1.0, 1.6180339887498949, 1.9990234375)
ACCURACY_FAMILIES = ("uniform7", "uniform1e5", "uniform1e6", "exponents", "kpio2", "zeros")      # all |x| <= 1e6: the accuracy rule
K_MAX = int(2 / math.pi * 1e6)                     # the largest k with k pi/2 <= 1e6


@functools.lru_cache(None)
def kpio2_doubles():
    """for k = 1 .. K_MAX: the double nearest k pi/2, and |r| = |that double - k pi/2|.  Integers only: pi/2 as a 300-bit integer P,
    k P / 2^300 rounded by Python's correctly rounded integer division; the double (>= 1.5, so a multiple of 2^-52) as an integer."""
    with mpmath.workprec(400):
        P = int(mpmath.floor(mpmath.ldexp(mpmath.pi / 2, 300)))
    one = 1 << 300
    x, r = np.empty(K_MAX), np.empty(K_MAX)
    for k in range(1, K_MAX + 1):
        kp = k * P
        v = kp / one
        x[k - 1] = v
        r[k - 1] = abs((int(math.ldexp(v, 52)) << 248) - kp) / one
    return x, r


@functools.lru_cache(None)
def sincos_family(name):
    rng = np.random.default_rng(20261021)
    if name == "uniform7":
        return rng.uniform(-7, 7, 3000)
    if name == "uniform1e5":
        return rng.uniform(-1e5, 1e5, 3000)
    if name == "uniform1e6":
        return rng.uniform(-1e6, 1e6, 3000)
    if name == "exponents":                      # every exponent from 2^-1074 to 2^19: three mantissas and both neighbours of each
        e = np.arange(-1074, 20)                 # (2^19 x 1.99 > 1e6 and all of 2^20 lie beyond the rule's range: family "ladder")
        v = neighbours(np.concatenate([np.ldexp(m, e) for m in EXPONENT_MANTISSAS]))
        v = v[(np.abs(v) <= 1e6)]
        return v * np.where(np.arange(v.size) % 2, -1.0, 1.0)
    if name == "kpio2":                          # the hardest 1500 by |r| and a seeded 500 of the rest, with both neighbours, signs alternating
        x, r = kpio2_doubles()
        order = np.argsort(r, kind="stable")
        pick = np.concatenate([order[:1500], rng.choice(order[1500:], 500, replace=False)])
        v = neighbours(x[pick])
        v = v[np.abs(v) <= 1e6]
        return v * np.where(np.arange(v.size) % 2, -1.0, 1.0)
    if name == "zeros":                          # +-0 and denormals (finite specials: inside the accuracy rule)
        return np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-310, -2.2e-310, 2.2250738585072014e-308, -2.2250738585072009e-308])
    if name == "nonfinite":
        return np.array([np.inf, -np.inf, np.nan])
    if name == "ladder":                         # beyond the exact reduction: rungs, either side of 2^31 pi/2, and 150 seeded arguments a decade
        rungs = np.array([1e6, 1e7, 1e8, 1e9, 3.3e9, np.nextafter(TWO31_PIO2, 0), TWO31_PIO2, np.nextafter(TWO31_PIO2, np.inf), 3.4e9, 1e10])
        rungs = np.concatenate([np.nextafter(rungs[:1], np.inf), rungs[1:]])                      # (1e6 itself belongs to the rule above)
        top = neighbours(np.concatenate([np.ldexp(m, [19, 20]) for m in EXPONENT_MANTISSAS]))      # the exponents the rule's range cuts off
        rungs = np.concatenate([rungs, top[top > 1e6]])
        dec = [rng.uniform(lo, 10 * lo, 150) * rng.choice([-1.0, 1.0], 150) for lo in (1e6, 1e7, 1e8, 1e9)]
        return np.concatenate([rungs, -rungs] + dec)
    raise KeyError(name)


def sincos_bit_arguments():
    """the arguments of the bit-for-bit comparison (no multiprecision work): every family above, the double nearest EVERY k pi/2 up to
    1e6, and 100,000 seeded arguments in each range"""
    rng = np.random.default_rng(7)
    fam = [sincos_family(f) for f in ACCURACY_FAMILIES + ("nonfinite", "ladder")]
    x, _ = kpio2_doubles()
    return np.concatenate(fam + [x, -x[::3]] + [rng.uniform(-a, a, 100000) for a in (7.0, 1e5, 1e6, 1e9)])


def sincos_rule(x, ts, tc, s, c):
    """-> (worst error of (s, c) in ulps of the true value, the bound Y + 2, Y).  Y: the C library's own largest error over the same
    arguments, computed here; 2 ulp: DESIGN.md's distance of the default build's forms from the strict (libm) form."""
    ls, lc = libm_sincos(x)
    Y = max(ulps(ls, ts).max(), ulps(lc, tc).max())
    return max(ulps(s, ts).max(), ulps(c, tc).max()), Y + 2.0, Y


# ---------------------------------------------------------------- atmosphere
VT = (0.01, 300.0, 500.0, 900.0)
ALT_EDGE = 1.0 / 0.703e-5                          # tfac = 0 near 142,247 ft


@functools.lru_cache(None)
def altitudes():
    """(altitudes, mask of the envelope [0, 1e5] ft).  A lattice over the envelope, below sea level, 35,000 ft (where the temperature rule
    changes) with its neighbours, and the edge list of tests/test_gpu_quad_constants.py (tfac -> 0+, <= 0, inf, NaN)."""
    lattice = np.linspace(0.0, 1e5, 2501)
    below = np.linspace(-1e4, 0.0, 101)[:-1]
    knee = np.array([np.nextafter(35000.0, 0), 35000.0, np.nextafter(35000.0, 1e9), 34999.0, 35001.0, np.nextafter(1e5, 0)])
    edge = np.array([-1.0, -500.0, -1e4, -1e6, 100000.5, 120000.0, 142000.0, ALT_EDGE, np.nextafter(ALT_EDGE, 0), np.nextafter(ALT_EDGE, 1e9),
                     142248.0, 2e5, 1e7, 1e300, -1e300, np.inf, -np.inf, np.nan])
    alt = np.concatenate([lattice, knee, below, edge])
    return alt, (alt >= 0) & (alt <= 1e5)


def fl_4_14_minus_4():
    """4.14 - 4.0: exact (both doubles, within a factor of two), and 4 + it is the double 4.14 again"""
    c = 4.14 - 4.0
    assert 4.0 + c == 4.14 and mpmath.mpf(4.14) - 4 == mpmath.mpf(c)
    return c


@functools.lru_cache(None)
def _tfac_raw():
    """per altitude of altitudes(): the once-rounded tfac as a multiprecision number (1 - .703e-5 alt is ONE fused operation), None
    where the altitude is not finite"""
    with mpmath.workprec(PREC):
        return [mp(float(1 - mp(.703e-5) * mp(a))) if math.isfinite(a) else None for a in altitudes()[0]]


@functools.lru_cache(None)
def _atmos_base():
    """what does not depend on the exponent fraction, over altitudes() x VT (altitude-major): truths of tfac, rho = rho0 tfac^fl(4.14),
    mach, qbar, ps"""
    alt, _ = altitudes()
    nan = mpmath.mpf("nan")
    rows = {k: [] for k in ("tfac", "rho", "mach", "qbar", "ps")}
    with mpmath.workprec(PREC):
        for a, t in zip(alt, _tfac_raw()):
            ok = t is not None and t > 0
            tfac = t if t is not None else nan
            temp = mpmath.mpf(390) if a >= 35000.0 else 519 * tfac
            rho = mp(2.377e-3) * tfac ** mp(4.14) if ok else nan
            for v in VT:
                rows["tfac"].append(tfac)
                rows["rho"].append(rho)
                rows["mach"].append(mp(v) / mpmath.sqrt(mp(1.4) * mp(1716.3) * temp) if ok else nan)
                rows["qbar"].append(mp(.5) * rho * mp(v) ** 2)
                rows["ps"].append(1715 * rho * temp)
        return {k: Truth(v) for k, v in rows.items()}


@functools.lru_cache(None)
def atmos_truth(frac):
    """Over altitudes() x VT (altitude-major): alt, vt, and the truths of tfac, factor = tfac^frac, rho = rho0 tfac^fl(4.14),
    mach, qbar, ps -- every expression evaluated in multiprecision on the DOUBLES the code holds (its constants, the once-rounded tfac,
    vt); NaN where tfac <= 0 or the altitude is not finite.  Only the factor depends on `frac`; the rest is computed once."""
    alt, _ = altitudes()
    nan = mpmath.mpf("nan")
    with mpmath.workprec(PREC):
        factor = Truth([t ** mp(frac) if t is not None and t > 0 else nan for t in _tfac_raw() for _ in VT])
    return np.repeat(alt, len(VT)), np.tile(np.array(VT), alt.size), dict(_atmos_base(), factor=factor)


# The rounding budget of the fast atmosphere, in u = 2^-53 of relative error, one u per rounding of the expression as coded
# (f16_plant.hpp atmos_alt / atmos_air; tfac itself is an input here: the truth is evaluated ON the rounded tfac):
#   t2 = tfac tfac                       1
#   t4 = t2 t2                           2 x 1 + 1 = 3
#   factor = exp(c log tfac)             1 ulp of its value (the header's figure) <= 2 u
#   t4 factor                            3 + 2 + 1 = 6
#   rho = rho0 (t4 factor)               7
#   qbar = (.5 rho) (vt vt)              7 + 0 (a power of two) + 1 (vt vt) + 1 = 9
#   temp = 519 tfac                      1 (0 where the constant 390 applies)
#   ps = (1715 rho) temp                 7 + 1 + 1 + 1 = 10
#   mach = vt / sqrt((1.4 x 1716.3) temp)   the folded constant 1, temp 1, their product 1: 3 under the root = 1.5; the root 1; the
#                                        quotient 1 = 3.5
FACTOR_ULPS = 1.0
BUDGET_U = {"rho": 7.0, "qbar": 9.0, "ps": 10.0, "mach": 3.5}


def budget(name):
    return BUDGET_U[name] * SECOND_ORDER


# ---------------------------------------------------------------- reciprocal, tangent
RCP_ULPS = 1.0          # the header: "v_rcp_f64 + two Newton steps (<= 1 ulp)" for normal, finite x


@functools.lru_cache(None)
def rcp_arguments():
    """(x, promised): seeded doubles over every normal exponent, powers of two with neighbours, the cosines of pitch angles within a
    few ulp of +-pi/2; then 0, denormals, inf and NaN (reported only).  promised: the header's "normal, finite x" -- all of it, the
    arguments above 2^1022 included, whose reciprocal is a denormal."""
    rng = np.random.default_rng(11)
    e = np.repeat(np.arange(1, 2047, dtype=np.int64), 4)
    seeded = ((e << 52) | rng.integers(0, 1 << 52, e.size, dtype=np.int64) | (rng.integers(0, 2, e.size, dtype=np.int64) << 63)).view(np.float64)
    top = rng.integers(0, 1 << 53, 1000, dtype=np.int64) + (np.int64(2045) << 52)         # 1000 more in [2^1022, 2^1024): denormal reciprocals
    seeded = np.concatenate([seeded, (top | (rng.integers(0, 2, top.size, dtype=np.int64) << 63)).view(np.float64)])
    pow2 = neighbours(np.ldexp(1.0, np.arange(-1022, 1024)))
    pow2 = pow2[np.isfinite(pow2)]
    near = np.array([math.pi / 2, -math.pi / 2])
    for _ in range(4):
        near = np.unique(neighbours(near))
    ct = restated_sincos(near)[1]
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-310, np.inf, -np.inf, np.nan])
    x = np.concatenate([seeded, pow2, -pow2[::7], ct, special])
    with np.errstate(invalid="ignore"):
        promised = (np.abs(x) >= 2.0 ** -1022) & np.isfinite(x)
    return x, promised


@functools.lru_cache(None)
def rcp_truth():
    x, promised = rcp_arguments()
    with mpmath.workprec(PREC):
        return Truth([1 / mp(v) if ok else mpmath.mpf("nan") for v, ok in zip(x, promised)])


@functools.lru_cache(None)
def tan_arguments():
    """pitch angles: seeded over [-pi/2, pi/2] and [-7, 7], and within a few ulp of +-pi/2"""
    rng = np.random.default_rng(13)
    near = np.array([math.pi / 2, -math.pi / 2])
    for _ in range(4):
        near = np.unique(neighbours(near))
    return np.concatenate([rng.uniform(-math.pi / 2, math.pi / 2, 1500), rng.uniform(-7, 7, 500), near, [0.0, 1e-300, math.pi / 4]])


@functools.lru_cache(None)
def tan_truth():
    with mpmath.workprec(PREC):
        return Truth([mpmath.tan(mp(v)) for v in tan_arguments()])


def tan_budget(sincos_ulps):
    """tt = st * f16_rcp(ct) against tan(theta), relative, in u: st and ct each within `sincos_ulps` ulp (<= 2 u each ulp), the reciprocal
    within RCP_ULPS ulp of 1 / ct (<= 2 u), the product 1"""
    return (2 * 2 * sincos_ulps + 2 * RCP_ULPS + 1) * SECOND_ORDER


# ---------------------------------------------------------------- carried pairs
D_MAX = 4e-3            # the series' range: trig_advance's `!(big <= 4e-3)`
CARRY_LENGTHS = (1, 31, 32)


def rotation_budget(d=D_MAX):
    """the ABSOLUTE error one trig_rotate by |d| adds to each of s and c (|s|, |c| <= 1), in u = 2^-53:
      cd = fma(d2, fma(d2, 1/24, -1/2), 1)   the closing fma rounds a value just below 1: 2^-54 = 0.5 u; the roundings inside (the
                                             square, the inner fma) arrive multiplied by d^2: < 2 d^2 u; the dropped term d^6 / 720
      sd = d fma(d2, fma(...), 1)            three roundings of a value of size |d|: 3 |d| u (those inside x d^2: 2 |d|^3 u); the dropped
                                             term d^7 / 5040
      s1 = fma(c, sd, s cd)                  the product s cd rounds once, a value <= 1: 0.5 u; the fma once, |s1| <= 1: 0.5 u; to these
                                             add the error of cd (x |s| <= 1) and of sd (x |c| <= 1).  c1 likewise.
      d = xn - xo                            exact unless the angle changes sign across binades: |d| u"""
    cd = 0.5 + 2 * d * d + d ** 6 / 720 / U
    sd = 3 * d + 2 * d ** 3 + d ** 7 / 5040 / U
    return cd + sd + 0.5 + 0.5 + d


def carry_budget(k, sincos_ulps, d=D_MAX):
    """the absolute error of s or c after k rotations, in u.  The error VECTOR (e_s, e_c) passes through each rotation multiplied by a
    matrix of norm sqrt(sd^2 + cd^2) <= 1 + d^6 (so: unamplified, to second order) and gains at most sqrt(2) x rotation_budget in
    norm; it starts at the full evaluation's error, sincos_ulps ulp of values <= 1 (<= 2 u each).  One component is at most the
    norm.  |s^2 + c^2 - 1| is, to first order, twice the radial part of the error vector; it is held to the same figure as a
    component -- the stricter reading: a bound of twice the budget is what the derivation alone would give."""
    return math.sqrt(2) * (2 * sincos_ulps + k * rotation_budget(d)) * SECOND_ORDER


@functools.lru_cache(None)
def carry_cases(n_steps):
    """(start angles [n], increments [n_steps][n]) -- every increment with |xn - xo| <= D_MAX: constant steps of either sign and several
    sizes, seeded steps, alternating signs, and angles that cross 0, +pi/2 and -pi/2 on the way"""
    rng = np.random.default_rng(100 + n_steps)
    start, steps = [], []
    half = 0.5 * n_steps
    for centre in (0.0, math.pi / 2, -math.pi / 2, 1.0, -2.5, 6.0):
        for d in (3.9e-3, -3.9e-3, 1e-3, -2.5e-4, 1e-9):
            start.append(centre - half * d)                       # crosses `centre` half way
            steps.append(np.full(n_steps, d))
        for _ in range(6):
            start.append(centre + rng.uniform(-2e-3, 2e-3))
            steps.append(rng.uniform(-3.9e-3, 3.9e-3, n_steps))
        start.append(centre + 1e-3)
        steps.append(3.5e-3 * (-1.0) ** np.arange(n_steps))       # sign change every step
    return _f64(start), _f64(np.array(steps).T)


def carry_truth(angles):
    """Truths of sin and cos of the accumulated STORED angles [n_steps][n]"""
    with mpmath.workprec(PREC):
        pairs = [mpmath.cos_sin(mp(v)) for v in angles.ravel()]
    return Truth([p[1] for p in pairs]), Truth([p[0] for p in pairs])


def threshold_cases():
    """(start, one increment each, the verdict `!(big <= 4e-3)` dictates with big = fmax(|d|, 0...) of the increment taken back from the
    stored angle).  Start 0, so that xn - xo is the increment itself.  A NaN increment is dropped by fmax against the other angles'
    zero increments: NOT stale (the pair itself becomes NaN, and the state with it)."""
    d = np.array([4e-3, np.nextafter(4e-3, 0), np.nextafter(4e-3, 1), -4e-3, np.nextafter(-4e-3, -1), np.nan, np.inf, -np.inf, 0.0, 1.0])
    with np.errstate(invalid="ignore"):
        big = np.fmax(np.abs(d), 0.0)
        verdict = ~(big <= 4e-3)
    return np.zeros(d.size), d[None, :], verdict.astype(np.float64)


# ---------------------------------------------------------------- the rules as functions of results (the CPU module feeds them the
# restatement and the stand-ins, the GPU module the device)
def atmos_worst(got, truth, mask):
    """worst errors over the lanes of `mask`: the factor in ulps of tfac^frac, the others relative in u (`got` may lack rho: the device
    returns it only inside qbar and ps)"""
    out = {"factor": float(ulps(got["factor"], truth["factor"])[mask].max())}
    for k in BUDGET_U:
        if k in got:
            out[k] = float(rel_u(got[k], truth[k])[mask].max())
    return out


def atmos_within_budget(worst):
    return worst["factor"] <= FACTOR_ULPS and all(worst[k] <= budget(k) for k in BUDGET_U if k in worst)


def envelope_lanes():
    """mask over altitudes() x VT of the flight envelope [0, 1e5] ft"""
    return np.repeat(altitudes()[1], len(VT))


def carry_worst(out):
    """out [n_steps][4][n] (sin, cos, stored angle, verdict) -> (largest of |s - sin|, |c - cos| per step [n_steps], largest |s^2 + c^2 - 1|
    per step), in u, against the multiprecision sin / cos of the STORED angle"""
    s, c, a = out[:, 0], out[:, 1], out[:, 2]
    ts, tc = carry_truth(a)
    es = np.abs((s.ravel() - ts.hi) - ts.lo).reshape(s.shape)
    ecs = np.abs((c.ravel() - tc.hi) - tc.lo).reshape(c.shape)
    with mpmath.workprec(PREC):
        norm = np.array([abs(float(mp(p) ** 2 + mp(q) ** 2 - 1)) for p, q in zip(s.ravel(), c.ravel())]).reshape(s.shape)
    return np.maximum(es, ecs).max(axis=1) / U, norm.max(axis=1) / U


def start_sincos_ulps(start):
    """the bound of the accuracy rule, Y + 2 ulp, at the start angles of the carried pairs (Y: the C library's error there)"""
    with mpmath.workprec(PREC):
        pairs = [mpmath.cos_sin(mp(v)) for v in start]
        ts, tc = Truth([p[1] for p in pairs]), Truth([p[0] for p in pairs])
    ls, lc = libm_sincos(start)
    return max(ulps(ls, ts).max(), ulps(lc, tc).max()) + 2.0
