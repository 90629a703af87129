"""The trim in a manoeuvre (include/f16_hip.h: f16_trim_man_batch, csrc/f16_trim.hip: k_trim_man) restated in numpy on the oracle's
calc_xdot: what tests/test_trim_man_cpu.py and tests/test_gpu_trim_man.py share.

THE COST, as the header states it.  Unknowns q = (P3, dh, da, dr, alpha, beta); givens h, V, gamma (rad), psi_dot (rad/s), theta_dot
(rad/s).  The four commands and alpha are clipped as the level trim's objective clips them, beta to +-30 deg; the flap states x[16],
x[17] come from the UNCLIPPED alpha.  At the clipped alpha and beta, with g = 32.17 (the plant's own constant),
    G = psi_dot V / g
    a = 1 - G tan(alpha) sin(beta);   b = sin(gamma) / cos(beta);   c = 1 + G^2 cos^2(beta)
    tan(phi)   = G (cos(beta)/cos(alpha)) [ (a - b^2) + b tan(alpha) sqrt(c (1 - b^2) + G^2 sin^2(beta)) ] / [ a^2 - b^2 (1 + c tan^2(alpha)) ]
    a' = cos(alpha) cos(beta);        b' = sin(phi) sin(beta) + cos(phi) sin(alpha) cos(beta)
    tan(theta) = [ a' b' + sin(gamma) sqrt(a'^2 - sin^2(gamma) + b'^2) ] / (a'^2 - sin^2(gamma))
    p = -psi_dot sin(theta);   q = theta_dot cos(phi) + psi_dot sin(phi) cos(theta);   r = -theta_dot sin(phi) + psi_dot cos(phi) cos(theta)
x = (0, 0, h, phi, theta, 0, V, alpha, beta, p, q, r, P3, dh, da, dr, lef, -alpha 180/pi), u = x[12:16],
cost = sum_k w_k (xdot_k - target_k)^2 with the level trim's w and target = 0 but target[2] = V sin(gamma), target[4] = theta_dot,
target[5] = psi_dot.

THE COST BAND is the level trim's (tests/trim_cases.py) with |xdot_k - target_k| in the weighted sum: 2 XDOT_TOL max|xd| sum_k w_k
|xd_k - target_k|.  No new tolerance.

THE TIE RULE.  Two candidates tie exactly when the plant inputs that xdot[0:12] reads are bit-identical: all 18 for hifi, x[0:16] for
lofi, which does not read the flap states (tests/test_trim_man_cpu.py asserts that by perturbing x[16:18]).  Cost.x holds exactly
those bytes, so tc.nelder_mead's tie test is this rule.

tc.nelder_mead, tc.vertex_yardstick and tc.vertex_allowance are generic in the dimension and are used as they are.
"""
import collections

import numpy as np

import trim_cases as tc

G0 = 32.17                             # the plant's constant of gravity (the force equations of calc_xdot)
W = tc.W
X0_REF = tc.X0_REF + (0.0,)            # the level trim's start, beta = 0
N_LOCK = tc.N_LOCK
IDX_Q = [12, 13, 14, 15, 7, 8]         # q read back from x_trim
BRANCHES = tc.BRANCHES
NFEV_OF = dict(expand=2, expand_refused=2, reflect=1, contract_out=2, contract_in=2, shrink_out=8, shrink_in=8)
DEG = np.pi / 180

Cond = collections.namedtuple("Cond", "h v gamma psi_dot theta_dot")


def constraints(alpha, beta, v, gamma, psi_dot, theta_dot, lib=np):
    """(phi, theta, p, q, r) of the manoeuvre at the clipped alpha and beta; lib = np, or a namespace of long-double functions"""
    sa, ca, sb, cb, ta = lib.sin(alpha), lib.cos(alpha), lib.sin(beta), lib.cos(beta), lib.tan(alpha)
    sg = lib.sin(gamma)
    G = psi_dot * v / G0
    a = 1 - G * ta * sb
    b = sg / cb
    c = 1 + G * G * cb * cb
    num = G * (cb / ca) * ((a - b * b) + b * ta * lib.sqrt(c * (1 - b * b) + G * G * sb * sb))
    den = a * a - b * b * (1 + c * ta * ta)
    phi = lib.arctan(num / den)
    a2 = ca * cb
    b2 = lib.sin(phi) * sb + lib.cos(phi) * sa * cb
    theta = lib.arctan((a2 * b2 + sg * lib.sqrt(a2 * a2 - sg * sg + b2 * b2)) / (a2 * a2 - sg * sg))
    p = -psi_dot * lib.sin(theta)
    q = theta_dot * lib.cos(phi) + psi_dot * lib.sin(phi) * lib.cos(theta)
    r = -theta_dot * lib.sin(phi) + psi_dot * lib.cos(phi) * lib.cos(theta)
    return phi, theta, p, q, r


def clipped(q):
    """(alpha, beta) as the plant is given them"""
    return float(np.clip(q[4], -20 * DEG, 90 * DEG)), float(np.clip(q[5], -30 * DEG, 30 * DEG))


def state_of(q, cond):
    """the plant state x [18] of the cost at q (clipped copies)"""
    P3, dh, da, dr, alpha, beta = (float(t) for t in q)
    h, v = float(cond.h), float(cond.v)
    lef = tc.x_trim_of((P3, dh, da, dr, alpha), h, v)[0][16]
    al, be = clipped(q)
    with np.errstate(invalid="ignore", divide="ignore"):
        phi, theta, p, qq, r = constraints(al, be, v, cond.gamma, cond.psi_dot, cond.theta_dot)
    return np.array([0, 0, h, phi, theta, 0, v, al, be, p, qq, r, np.clip(P3, 1000, 19000), np.clip(dh, -25, 25), np.clip(da, -21.5, 21.5),
                     np.clip(dr, -30., 30), lef, -alpha * 180 / np.pi])


def target_of(cond):
    t = np.zeros(12)
    t[2], t[4], t[5] = cond.v * np.sin(cond.gamma), cond.theta_dot, cond.psi_dot
    return t


def cost(oracle, q, cond, fi, xcg):
    """the cost at q -> tc.Cost(cost, xd [18], the cost band, x: the plant inputs that xdot[0:12] reads)"""
    x = state_of(q, cond)
    xd = oracle.calc_xdot(x, x[12:16], int(fi), float(xcg))
    res = xd[0:12] - target_of(cond)
    band = float(2.0 * tc.XDOT_TOL * np.abs(xd).max() * np.dot(W, np.abs(res)))
    return tc.Cost(float(np.dot(W, res ** 2)), xd, band, x if fi == 1 else x[0:16].copy())


def x_trim_of(q, cond):
    """what the call returns for the optimiser's q: the plant state with the six unknowns written back unclipped"""
    x = state_of(q, cond)
    x[IDX_Q] = q
    return x


class _LD:
    """numpy's functions on long doubles"""
    sin, cos, tan, sqrt, arctan = (staticmethod(f) for f in (np.sin, np.cos, np.tan, np.sqrt, np.arctan))


def constraint_allowance(q, cond):
    """what (phi, theta, p, q, r) of the device may differ by from the fp64 restatement: 16 x the distance between the numpy fp64 and
    long-double evaluations, at least 64 eps of scale (the rule of tc.vertex_allowance) -> (values [5], allowance [5])"""
    ld = np.longdouble
    al, be = clipped(q)
    c64 = np.array(constraints(al, be, float(cond.v), cond.gamma, cond.psi_dot, cond.theta_dot))
    cld = np.array(constraints(ld(al), ld(be), ld(cond.v), ld(cond.gamma), ld(cond.psi_dot), ld(cond.theta_dot), _LD), dtype=ld)
    yard = np.abs(c64.astype(ld) - cld).astype(np.float64)
    return c64, tc.vertex_allowance(yard, np.maximum(1.0, np.abs(c64)))


def conditioning(oracle, q, cond, fi, xcg):
    """how far the restated cost at q moves, in cost bands, when the constraints are evaluated in long double (and rounded to fp64 for
    the plant): what rounding inside the constraints alone does to the cost"""
    ld = np.longdouble
    c = cost(oracle, q, cond, fi, xcg)
    al, be = clipped(q)
    x = state_of(q, cond)
    x[[3, 4, 9, 10, 11]] = np.array(constraints(ld(al), ld(be), ld(cond.v), ld(cond.gamma), ld(cond.psi_dot), ld(cond.theta_dot), _LD),
                                    dtype=ld).astype(np.float64)
    xd = oracle.calc_xdot(x, x[12:16], int(fi), float(xcg))
    return abs(float(np.dot(W, (xd[0:12] - target_of(cond)) ** 2)) - c.cost) / c.band


def scipy_runs(oracle, cond, fi=1, xcg=0.25, runs=2, q0=X0_REF, noise=None):
    """`runs` scipy Nelder-Mead runs (tol 1e-10, maxiter 5e4), each from the last one's point -> list of scipy results.  noise: a
    numpy Generator; the plant is then perturbed by 1e-14 relative (the method of tests/test_gpu_trim.py)"""
    from scipy.optimize import minimize

    def f(q):
        c = cost(oracle, q, cond, fi, xcg)
        if noise is None:
            return c.cost
        xd = c.xd[0:12] * (1 + 1e-14 * noise.standard_normal())
        return float(np.dot(W, (xd - target_of(cond)) ** 2))
    out, q = [], list(q0)
    for _ in range(runs):
        out.append(minimize(f, q, method="Nelder-Mead", tol=1e-10, options={"maxiter": 5e4}))
        q = out[-1].x
    return out


# ------------------------------------------------------------------------------------------------ the lockstep cases
Group = collections.namedtuple("Group", "name x0 fi xcg conds")


def _c(h, v, gamma_deg, turn_deg, pull_deg=0.0):
    return Cond(float(h), float(v), gamma_deg * DEG, turn_deg * DEG, pull_deg * DEG)


# Chosen on the CPU oracle (tests/test_trim_man_cpu.py holds the coverage and the margins of exactly this list): the reference start
# at conditions over h 2,000 .. 45,000 ft, V 350 .. 900 ft/s, gamma -3 .. 7 deg, turn rate -8 .. 8 deg/s, some with a 2 deg/s pull-up,
# which take every branch but the shrinks with 100 cost bands to spare; shrinks with such a margin are rare in six dimensions, so they
# are covered by EXACT TIES: a start with every unknown beyond its clip (every candidate gives the plant the same input: every
# iteration is shrink_in), and starts with some unknowns beyond their clips (shrink_out among them).  Group sizes are no multiple of 4.
# WHERE THE COST ITSELF IS ILL CONDITIONED no implementation can be held to the band, so no case goes there: with alpha at its 90 deg
# clip and gamma = 0 the constraints give theta = 90 deg to rounding, and xdot[5] = (q sin(phi) + r cos(phi)) / cos(theta) divides by a
# cos(theta) that is all rounding error (measured: evaluating the constraints in long double moves the restated cost by 1e5 .. 1e8
# bands there, by <= 1e-5 band on every case below).  So the starts with alpha beyond its clip go with gamma != 0, and
# `conditioning` is asserted on every vertex of every case path (tests/test_trim_man_cpu.py).
CASES = (
    Group("ref25", X0_REF, 1, 0.25, (_c(10000, 700, 0, 3), _c(35000, 600, 2, -4), _c(41000, 850, -1, 2, 2), _c(3000, 400, 5, 6),
                                     _c(22000, 500, -3, -8))),
    Group("ref35", X0_REF, 1, 0.35, (_c(10000, 700, 0, 0), _c(34900, 800, 7, 5, 2), _c(15000, 450, -2, -3))),
    Group("ref_lofi", X0_REF, 0, 0.35, (_c(7900, 545, 3, 8), _c(35000, 877, -3, -2), _c(42800, 839, 1, 4, 2))),
    Group("all_clipped_lofi", (25000.0, 30.0, -25.0, 35.0, 1.7, 0.6), 0, 0.25, (_c(7900, 545, 2, 3), _c(35000, 700, -2, -6), _c(21900, 567, 6, 0))),
    Group("some_clipped_lofi", (-500.0, -0.09, 25.0, -0.01, 1.7, 0.0), 0, 0.35, (_c(24100, 696, 1, -4), _c(12600, 513, 2, 4), _c(16000, 833, 1, -7))),
    Group("some_clipped_hifi", (-500.0, 30.0, 25.0, 1.0, 1.7, -0.6), 1, 0.35, (_c(36800, 397, -2, -4, 2), _c(9700, 790, 6, 1), _c(28700, 613, -1, -6))),
)

# The full trims.  Measured on the CPU oracle (scipy 1.15, the reference start): cost after one run 1.3e-6 .. 2.0e-5 (it stalls), after
# two 7e-29 .. 2.1e-27, nit about 1,200 .. 1,500 for the first run and 600 .. 1,100 for the second.  (Some pull-ups -- 10,000 ft, 600
# ft/s, 3 deg/s -- converge in one run; the one listed does not.)  The two untrimmable conditions stay at 0.27 and 0.25 with the thrust
# unknown at -4e5 and -1.1e3 lb.
FULL = (_c(10000, 700, 0, 0), _c(10000, 700, 0, 3), _c(30000, 800, 0, -8), _c(20000, 600, 5, 5), _c(5000, 450, 3, 0), _c(20000, 700, 0, 0, 3))
FULL_NAMES = ("level", "turn+3", "turn-8", "climbing_turn", "climb", "pullup")
UNTRIMMABLE = (_c(10000, 500, -2, 0), _c(15000, 400, 0, 10))       # a descent against idle thrust; a turn the wing cannot hold
# SPREAD: how far the two-run point moves under 1e-14 relative plant noise (the method of tests/test_gpu_trim.py), per unknown (P3 lb;
# dh, da, dr deg; alpha, beta rad): the largest distance of a noisy two-run point from the clean one over the six FULL conditions and
# the seeds 1, 2, 3, measured on the CPU oracle (the climbing turn sets all six; tests/test_trim_man_cpu.py re-measures one condition).
SPREAD = np.array([5.64e-09, 1.75e-11, 1.13e-10, 4.73e-10, 1.53e-13, 3.37e-12])


def conditions():
    return [(g, i) for g, grp in enumerate(CASES) for i in range(len(grp.conds))]


_PATHS = {}


def path(oracle, g, i):
    """tc.nelder_mead over N_LOCK iterations for condition i of group g, once per process"""
    if (g, i) not in _PATHS:
        grp = CASES[g]
        _PATHS[g, i] = tc.nelder_mead(lambda q: cost(oracle, q, grp.conds[i], grp.fi, grp.xcg), grp.x0, N_LOCK)
    return _PATHS[g, i]
