"""The families, the extended-precision reference, the yardstick and the comparison of tests/test_linearise_cpu.py and
tests/test_gpu_linearise.py, defined once.

Rule under test (env.py:294-342; k_linearise / k_linearise_full of csrc/f16_control.hip): J[r, c] = (f(p + eps e_c) - f(p)) / eps
with the perturbed coordinate the fp64 sum fl64(p_c + eps).  At eps = 1e-5 a rounding-level difference in f reaches J 1e5 times
larger, so "equal to 1e-6" says little about which rule was evaluated.

Reference: the same rule on the same fp64 points with the plant, the subtraction and the division evaluated in `long double`
(oracle/libf16_oracle_ld.so; 64-bit significand, so its own rounding error is 2^-11 of the fp64 one).  The tables and literals keep
their fp64 values: it is the same mathematical function.

Yardstick: a FAMILY is (model, fidelity, xcg, eps, CLr switch) over the whole lattice of tests/envelope_cases.py (hifi 1,418 rows, lofi
569 rows: every table cell plus the edge rows).  Y[r, c] = max over the family's cases of |fp64 restatement - reference|: the
rounding error the plain-C fp64 evaluation of this entry shows somewhere in the envelope.  It is computed here, when the test runs,
from the two CPU libraries alone -- never stored and never taken from the code under test.

Tolerance: |candidate - reference| <= 8 Y[r, c] in every case and every entry; where Y[r, c] = 0 (entries whose reference is zero
in every case: the zero structure) the candidate equals the reference exactly.  8 covers the same rule under other rounding --
FMA contraction, another operation order, another libm: the restatement rebuilt with -ffp-contract=fast -mfma stays within 1.1 ..
3.1 Y (tests/test_linearise_cpu.py asserts 8) -- while a wrong term, column map, base point or divisor lands decades beyond it
(entries reach 1.2e3, Y is 4e-11 .. 1.6e-7).  No finite case is left out of a comparison."""
import collections
import os
import subprocess

import numpy as np

import envelope_cases as ec

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FACTOR = 8
MPC_X_IDX = [3, 4, 7, 8, 9, 10, 11, 17, 16]      # parameters.py:135
OBS_X_IDX = [2, 3, 4, 7, 8, 9, 10, 11, 16, 17]   # parameters.py:134
GRID_BITS = 15                                   # F16_ST_ALPHA1 | ALPHA2 | BETA | EL
FLAG_FIX_CLR = 1                                 # F16_FLAG_FIX_CLR

Family = collections.namedtuple("Family", "model fidelity xcg eps fix_clr", defaults=(1e-5, 0))
# (model: "na" = the reduced nine-state model of f16_linearise_batch, "full" = the 18-state model of f16_linearise_full_batch)
FAMILIES = [Family(m, f, xcg) for m in ("na", "full") for f in ("hifi", "lofi") for xcg in (0.25, 0.35)]
EPS_FAMILY = Family("na", "hifi", 0.25, 1e-7)    # Y recomputed: the argument must reach the perturbation AND the divisor
FIX_CLR_FAMILIES = [Family(m, "hifi", xcg, 1e-5, 1) for m in ("na", "full") for xcg in (0.25, 0.35)]   # F16_FLAG_FIX_CLR / f16o_set_fix_clr(1)


def dims(model):
    """(states, inputs, outputs)"""
    return (9, 3, 9) if model == "na" else (18, 4, 10)


def batch(fam):
    return ec.hifi_lattice() if fam.fidelity == "hifi" else ec.lofi_lattice()


_LIBS = {}


def libs():
    """{"fp64", "fma", "ld"}: the three builds of oracle/f16_oracle.c, always through make (a stale checker would compare with old code)"""
    if not _LIBS:
        from oracle import lin_oracle
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "oracle")] + list(lin_oracle.LIBS.values()))
        for k in lin_oracle.LIBS:
            _LIBS[k] = lin_oracle.LinOracle(k)
    return _LIBS


def run(lib, fam, x, u):
    """(J [B, ns, ns + ni] = A | B, C [B, no, ns], status [B]) of one build at the family's settings"""
    lib.set_fix_clr(fam.fix_clr)
    try:
        f = lib.linearise_na_batch if fam.model == "na" else lib.linearise_full_batch
        A, Bm, C, st = f(x, u, fam.eps, 1 if fam.fidelity == "hifi" else 0, fam.xcg)
    finally:
        lib.set_fix_clr(0)
    return np.concatenate((A, Bm), 2), C, st


_REF = {}


def reference(fam):
    """dict(x, u, ref [B, ns, ns + ni] longdouble, J64 the fp64 restatement, Y [ns, ns + ni] longdouble, status [B] of the fp64
    restatement, C64), computed once per process"""
    if fam not in _REF:
        b = batch(fam)
        L = libs()
        ref, _, _ = run(L["ld"], fam, b.x, b.u)
        J64, C64, st = run(L["fp64"], fam, b.x, b.u)
        assert ref.dtype == np.longdouble and np.finfo(np.longdouble).nmant >= 63
        assert np.isfinite(ref).all() and np.isfinite(J64).all()          # every row of the lattice is finite in both models
        Y = np.abs(J64.astype(np.longdouble) - ref).max(0)
        _REF[fam] = dict(x=b.x, u=b.u, ref=ref, J64=J64, Y=Y, status=st, C64=C64, batch=b)
    return _REF[fam]


def ratios(J, fam, rows=None):
    """(worst |J - ref| / Y over the entries with Y > 0, number of entries where the rule fails) for the family's cases `rows`
    (default: all of them, in order); J [len(rows), ns, ns + ni]"""
    r = reference(fam)
    ref = r["ref"] if rows is None else r["ref"][rows]
    Y = r["Y"]
    assert J.shape == ref.shape, (J.shape, ref.shape)
    err = np.abs(np.asarray(J).astype(np.longdouble) - ref)
    bad = ~(err <= FACTOR * Y)                    # a NaN fails; Y = 0: err must be 0, i.e. J equals the (zero) reference exactly
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(Y > 0, err / np.where(Y > 0, Y, 1), 0)
    return float(q.max()), int(bad.sum()), bad


def check(J, fam, rows=None, what=""):
    """the 8 x Y rule on every case and entry; returns the worst ratio"""
    worst, nbad, bad = ratios(J, fam, rows)
    if nbad:
        r = reference(fam)
        ref = r["ref"] if rows is None else r["ref"][rows]
        k = np.argwhere(bad)[:8]
        lines = [f"  case {a} entry ({b_}, {c}): got {float(J[a, b_, c])!r} ref {float(ref[a, b_, c])!r} Y {float(r['Y'][b_, c]):.3e}" for a, b_, c in k]
        raise AssertionError(f"{what} {fam}: {nbad} entries beyond {FACTOR} x Y (worst ratio {worst:.3g})\n" + "\n".join(lines))
    return worst


def cc_numpy(x, u, eps, model):
    """the C matrix in plain numpy, as the kernels form it: (fl(p + eps) - p) / eps on the observed coordinate, exact zeros elsewhere
    -> [B, no, ns]"""
    x = np.asarray(x, dtype=np.float64)
    ns, _, no = dims(model)
    C = np.zeros((len(x), no, ns))
    with np.errstate(invalid="ignore"):
        if model == "na":
            p = x[:, MPC_X_IDX]
            d = ((p + eps) - p) / eps
            for k in range(9):
                C[:, k, k] = d[:, k]
        else:
            d = ((x + eps) - x) / eps
            for r_, k in enumerate(OBS_X_IDX):
                C[:, r_, k] = d[:, k]
    return C


def perturbed_points(x, u, eps, model):
    """the 13 / 23 points one linearisation evaluates, as full (x [18], u [4]) pairs: the base point, then one per column"""
    pts = [(x.copy(), u.copy())]
    for k in (MPC_X_IDX if model == "na" else range(18)):
        xp = x.copy()
        xp[k] = x[k] + eps
        pts.append((xp, u.copy()))
    for k in ((1, 2, 3) if model == "na" else range(4)):
        up = u.copy()
        up[k] = u[k] + eps
        pts.append((x.copy(), up))
    return pts


def nonfinite_rows(fam):
    """three aircraft that cannot be linearised to finite matrices: alpha NaN, V +inf, a NaN aileron command -> (x [3, 18], u [3, 4])"""
    b = batch(fam)
    x, u = b.x[[3, 5, 8]].copy(), b.u[[3, 5, 8]].copy()
    x[0, 7] = np.nan
    x[1, 6] = np.inf
    u[2, 2] = np.nan
    return x, u
