"""The batched trim (include/f16_hip.h: f16_trim_batch, csrc/f16_trim.hip) compared with scipy STEP BY STEP: the restatement and the
cases tests/test_trim_cpu.py and tests/test_gpu_trim_lockstep.py share.

Nelder-Mead run to collapse is a knife edge (tests/test_gpu_trim.py), but its first few dozen iterations are not: the simplex is
large and every comparison the algorithm makes is decided by far more than rounding.  There the device can be held to scipy's path
exactly -- `maxiter` is an argument of the call and `h_x0` sets the start, so the public entry point is enough.

trim_cost     obj_func of env.py:217-262 (oracle/mpc_oracle.py: trim_objective, the definition mo.trim minimises) with its COST BAND
              2 XDOT_TOL max|xd| sum_k w_k |xd_k|:  the device plant may differ from the oracle by XDOT_TOL max(1, |xd_k|) per entry
              (tests/test_gpu_dynamics.py); through cost = sum_k w_k xd_k^2 that is, to first order, 2 sum_k w_k |xd_k| XDOT_TOL
              max(1, |xd_k|).  max|xd| is taken over the whole derivative: xd[0], the northward speed of a level aircraft, is about V
              >= 350 ft/s, so it stands for every max(1, |xd_k|).  No new tolerance.
nelder_mead   scipy/optimize/_optimize.py:_minimize_neldermead restated in its own expression shapes, one record per iteration, with
              the DECISION MARGIN: the smallest gap of any cost comparison the iteration made (the branch tests, and the place of every
              new cost in the sorted list), divided by the sum of the two costs' bands.  Two points whose clipped plant inputs are bit
              for bit the same have the same cost on any implementation: an exact tie, decided by the stability rule, not a margin.
vertex_yardstick  the same path (the recorded decisions) with the vertex arithmetic in long double: its distance from the fp64 path is
              what rounding alone does to the vertices -- the measure of what FMA contraction of `(1 + rho chi) xbar - rho chi x_worst`
              and friends may do on the device.
THE TIE RULE  scipy sorts the simplex with `np.argsort(fsim)`, numpy's default kind.  On six elements that is an insertion sort --
              stable: equal costs keep their order, a new cost goes behind its equals -- except where numpy dispatches the default kind
              to a vectorised sorting network (x86 hosts with AVX-512, numpy >= 1.25), which is NOT stable, so there scipy's own order
              of tied vertices depends on the host.  The kernel follows the stable rule and so does this restatement;
              `stable_argsort` pins scipy to it for the comparison, and paths without ties are compared with scipy as it is.
CASES         the conditions, in call groups: (h_x0, fi_flag, xcg) are per call, h and v per aircraft.
"""
import collections
import contextlib

import numpy as np

from oracle import mpc_oracle as mo

XDOT_TOL = 1e-11                      # tests/test_gpu_dynamics.py: the band the device plant is granted against the oracle
N_LOCK = 32                           # iterations held in lockstep
EPS = 2.0 ** -52
W = np.array([0, 0, 5, 10, 10, 10, 2, 10, 10, 10, 10, 10.])
X0_REF = (5000.0, -0.09, 8.49, -0.01, 0.01)          # env.py:265-271, in the order minimize is given it
BRANCHES = ("expand", "expand_refused", "reflect", "contract_out", "contract_in", "shrink_out", "shrink_in")
NFEV_OF = dict(expand=2, expand_refused=2, reflect=1, contract_out=2, contract_in=2, shrink_out=7, shrink_in=7)

Cost = collections.namedtuple("Cost", "cost xd band x")


def trim_cost(oracle, q, h, v, fi, xcg):
    """obj_func at q = (P3, dh, da, dr, alpha) -> Cost(cost, xd [18], the cost band, x [18]: the clipped state the plant was given)"""
    c, xd, x = mo.trim_objective(oracle, np.asarray(q, dtype=np.float64), float(h), float(v), int(fi), float(xcg))
    return Cost(float(c), xd, float(2.0 * XDOT_TOL * np.abs(xd).max() * np.dot(W, np.abs(xd[0:12]))), x)


def x_trim_of(q, h, v):
    """env.py:275-290: the 18 states F16.trim returns for the optimiser's q -> (x [18], the three terms of the flap formula)"""
    P3, dh, da, dr, al = (float(t) for t in q)
    pi = np.pi
    tfac = 1 - 0.703e-5 * h
    temp = 390 if h >= 35000 else 519 * tfac
    rho = 2.377e-3 * tfac ** 4.14
    terms = (1.38 * al * 180 / pi, -9.05 * (0.5 * rho * v ** 2) / (1715 * rho * temp), 1.45)
    return np.array([0, 0, h, 0, al, 0, v, al, 0, 0, 0, 0, P3, dh, da, dr, terms[0] + terms[1] + terms[2], -al * 180 / pi]), terms


# ------------------------------------------------------------------------------------------------ scipy's iteration
def _gap(a, b):
    """the margin of one comparison between two Costs: |difference| / (sum of the bands); an exact tie (same plant input) is no
    comparison at all"""
    if a.x.tobytes() == b.x.tobytes():
        return np.inf
    d, s = abs(a.cost - b.cost), a.band + b.band
    return d / s if s > 0 else (np.inf if d > 0 else 0.0)


def initial_simplex(x0, dtype=np.float64):
    x0 = np.asarray(x0, dtype=dtype)
    N = len(x0)
    sim = np.empty((N + 1, N), dtype=dtype)
    sim[0] = x0
    for k in range(N):
        y = np.array(x0, copy=True)
        if y[k] != 0:
            y[k] = dtype(1 + 0.05) * y[k]
        else:
            y[k] = dtype(0.00025)
        sim[k + 1] = y
    return sim


def _candidates(sim, dtype=np.float64):
    """every point an iteration can need, in scipy's expressions (rho 1, chi 2, psi 0.5, sigma 0.5)"""
    rho, chi, psi, sigma = 1, 2, 0.5, 0.5
    N = sim.shape[1]
    xbar = np.add.reduce(sim[:-1], 0) / N
    return dict(xr=(1 + rho) * xbar - rho * sim[-1], xe=(1 + rho * chi) * xbar - rho * chi * sim[-1],
                xc=dtype(1 + psi * rho) * xbar - dtype(psi * rho) * sim[-1], xcc=dtype(1 - psi) * xbar + dtype(psi) * sim[-1],
                shrink=[sim[0] + dtype(sigma) * (sim[j] - sim[0]) for j in range(1, N + 1)])


@contextlib.contextmanager
def stable_argsort():
    """numpy.argsort with the stable kind where the caller names none, while the block runs (for scipy's `np.argsort(fsim)`)"""
    plain = np.argsort
    np.argsort = lambda a, *args, **kw: plain(a, *args, **kw) if (len(args) > 1 or "kind" in kw) else plain(a, *args, kind="stable", **kw)
    try:
        yield
    finally:
        np.argsort = plain


TAKES = dict(expand="xe", expand_refused="xr", reflect="xr", contract_out="xc", contract_in="xcc")


def nelder_mead(f, x0, iters, xatol=1e-10, fatol=1e-10):
    """`iters` iterations of scipy's Nelder-Mead on f (q -> Cost) from x0.  Returns the list of records, [0] the sorted initial
    simplex and [n] the state after n iterations: dict(sim [6, 5], fsim [6], band [6], nfev, branch, margin, ind: the argsort that
    closed the iteration).  The list is shorter than iters + 1 if scipy's termination test holds first."""
    sim = initial_simplex(x0)
    N = sim.shape[1]
    cs = [f(sim[k]) for k in range(N + 1)]
    nfev = N + 1
    margin = min([_gap(cs[i], cs[j]) for i in range(N + 1) for j in range(i)])
    ind = np.argsort([c.cost for c in cs], kind="stable")          # THE TIE RULE: see the module's text
    sim, cs = np.take(sim, ind, 0), [cs[i] for i in ind]
    fsim = np.array([c.cost for c in cs])
    out = [dict(sim=sim.copy(), fsim=fsim.copy(), band=np.array([c.band for c in cs]), nfev=nfev, branch="init", margin=margin, ind=ind)]
    for _ in range(iters):
        if np.max(np.ravel(np.abs(sim[1:] - sim[0]))) <= xatol and np.max(np.abs(fsim[0] - fsim[1:])) <= fatol:
            break
        pts = _candidates(sim)
        cxr = f(pts["xr"])
        nfev += 1
        fxr = cxr.cost
        gaps, new = [_gap(cxr, cs[0])], None
        if fxr < fsim[0]:
            cxe = f(pts["xe"])
            nfev += 1
            gaps.append(_gap(cxe, cxr))
            branch, new = ("expand", cxe) if cxe.cost < fxr else ("expand_refused", cxr)
        else:
            gaps.append(_gap(cxr, cs[-2]))
            if fxr < fsim[-2]:
                branch, new = "reflect", cxr
            else:
                gaps.append(_gap(cxr, cs[-1]))
                if fxr < fsim[-1]:
                    cxc = f(pts["xc"])
                    nfev += 1
                    gaps.append(_gap(cxc, cxr))
                    branch, new = ("contract_out", cxc) if cxc.cost <= fxr else ("shrink_out", None)
                else:
                    cxcc = f(pts["xcc"])
                    nfev += 1
                    gaps.append(_gap(cxcc, cs[-1]))
                    branch, new = ("contract_in", cxcc) if cxcc.cost < fsim[-1] else ("shrink_in", None)
        if new is not None:
            sim[-1], cs[-1] = pts[TAKES[branch]], new
            gaps += [_gap(new, c) for c in cs[:-1]]
        else:
            for j in range(1, N + 1):
                sim[j] = pts["shrink"][j - 1]
                cs[j] = f(sim[j])
                nfev += 1
            gaps += [_gap(cs[i], cs[j]) for i in range(N + 1) for j in range(i)]
        ind = np.argsort([c.cost for c in cs], kind="stable")
        sim, cs = np.take(sim, ind, 0), [cs[i] for i in ind]
        fsim = np.array([c.cost for c in cs])
        out.append(dict(sim=sim.copy(), fsim=fsim.copy(), band=np.array([c.band for c in cs]), nfev=nfev, branch=branch, margin=min(gaps),
                        ind=ind))
    return out


# ------------------------------------------------------------------------------------------------ the cases
Group = collections.namedtuple("Group", "name x0 fi xcg h v")

# Chosen on the CPU oracle from seeded scans of h in 2,000 .. 45,000 ft, V in 350 .. 900 ft/s: the reference start at the two golden
# conditions; starts with all four commands beyond their limits (the initial simplex holds five exact ties); a start with zeros (the
# 0.00025 rule); an alpha start above the 90 deg clip; both fidelities, both xcg; h below, at and above 35,000 ft.  The shrinks are
# rare (about one path in twelve has one), so the conditions that shrink with a margin of 100 or more were looked for:
# tests/test_trim_cpu.py holds the coverage and the margins of exactly this list.  Group sizes are no multiple of 4: a wavefront
# holds four conditions, so every group ends in a wavefront with invalid rows.
CASES = (
    Group("ref25", X0_REF, 1, 0.25, (10000.0, 35000.0, 41000.0, 3000.0, 22000.0), (700.0, 600.0, 850.0, 400.0, 500.0)),
    Group("ref35", X0_REF, 1, 0.35, (10000.0, 34900.0, 15000.0), (700.0, 800.0, 450.0)),
    Group("sat_hifi", (20000.0, -26.0, 22.0, -31.0, 0.2), 1, 0.35, (19300.0, 9100.0, 26500.0), (719.0, 641.0, 804.0)),
    Group("sat_lofi", (25000.0, 30.0, -25.0, 35.0, 0.05), 0, 0.25, (7900.0, 35000.0, 42800.0, 21900.0, 4900.0),
          (545.0, 877.0, 839.0, 567.0, 420.0)),
    Group("alpha_above_clip_lofi", (5000.0, -0.09, 8.49, -0.01, 1.7), 0, 0.35, (2900.0, 3900.0, 35000.0, 42300.0, 34800.0),
          (361.0, 362.0, 359.0, 360.0, 357.0)),
    Group("zeros_hifi", (5000.0, 0.0, 0.0, 0.0, 0.0), 1, 0.35, (5500.0, 2100.0, 2500.0), (797.0, 500.0, 533.0)),
)


def conditions():
    """(group index, index in the group) of every condition of CASES"""
    return [(g, i) for g, grp in enumerate(CASES) for i in range(len(grp.h))]


_PATHS = {}


def path(oracle, g, i):
    """nelder_mead over N_LOCK iterations for condition i of group g, once per process"""
    if (g, i) not in _PATHS:
        grp = CASES[g]
        _PATHS[g, i] = nelder_mead(lambda q: trim_cost(oracle, q, grp.h[i], grp.v[i], grp.fi, grp.xcg), grp.x0, N_LOCK)
    return _PATHS[g, i]


def vertex_yardstick(records, x0):
    """The recorded path replayed in long double (the same branch and the same argsort at every iteration, no cost evaluated)
    -> (yard [n + 1, 5]: per iteration and coordinate the largest |fp64 vertex - long double vertex| over the six vertices,
    scale [5]: the largest magnitude of the coordinate on the fp64 path)"""
    ld = np.longdouble
    sim = np.take(initial_simplex(x0, ld), records[0]["ind"], 0)
    yard = [np.abs(records[0]["sim"].astype(ld) - sim).max(0)]
    for r in records[1:]:
        pts = _candidates(sim, ld)
        if r["branch"] in TAKES:
            sim[-1] = pts[TAKES[r["branch"]]]
        else:
            sim[1:] = pts["shrink"]
        sim = np.take(sim, r["ind"], 0)
        yard.append(np.abs(r["sim"].astype(ld) - sim).max(0))
    scale = np.max([np.abs(r["sim"]).max(0) for r in records], 0)
    return np.array(yard, dtype=np.float64), scale


def vertex_allowance(yard_n, scale):
    """what a vertex coordinate may differ by from the fp64 path after n iterations: 16 x the yardstick, at least 64 eps of the
    coordinate's scale (the rule of tests/test_gpu_control_mp.py: the allowance is measured from a twin, the factor covers the same
    algorithm with other rounding)"""
    return np.maximum(16.0 * np.asarray(yard_n), 64.0 * EPS * np.asarray(scale))
