#!/usr/bin/env python3
"""Fixture G19: the ZOH and Riccati kernels of csrc/f16_mpc_model.hpp against a multiprecision reference.  CPU only.

    python tools/make_control_golden.py          -> tests/golden/g19_control_mp.npz, profiles/control_mp_errors.txt

References (mpmath, 60 digits, rounded once to fp64):
  * ZOH:   mpmath.expm([[A, B], [0, 0]] dt), top blocks.
  * DARE:  scipy's solution polished by Newton-Kleinman, every Lyapunov step one 81 x 81 linear solve; K = (R + B'XB)^-1 B'XA.
           Asserted before writing: Riccati residual <= 1e-30 max|X|, spectral radius of A - B K < 1.
The file also holds, per case and per output block, the fp64 error of the numpy restatement of the kernels' rules
(oracle/control_twin.py): the yardstick of the device tolerances (tests/test_gpu_control_mp.py).  The text file lists these and the
errors of the C restatement (oracle.c2d, oracle.dare) and of scipy.  All errors are max|got - ref| / max|ref| over the block.
"""
import os
import sys
import zipfile

import mpmath as mp
import numpy as np
import scipy.linalg

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
from oracle import control_twin as ct      # noqa: E402
from oracle import mpc_oracle as mo        # noqa: E402

DPS = 60
OUT = os.path.join(REPO, "tests", "golden", "g19_control_mp.npz")
TXT = os.path.join(REPO, "profiles", "control_mp_errors.txt")
SEED = 20190


# ------------------------------------------------------------------------------------------------ multiprecision references
def _mpm(a):
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a])


def _np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def mp_zoh(A, B, dt):
    """top blocks of expm([[A, B], [0, 0]] dt) at DPS digits -> fp64 (Ad, Bd)"""
    mp.mp.dps = DPS
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    ns, ni = B.shape
    M = mp.zeros(ns + ni)
    h = mp.mpf(float(dt))
    for i in range(ns):
        for j in range(ns):
            M[i, j] = mp.mpf(float(A[i, j])) * h
        for j in range(ni):
            M[i, ns + j] = mp.mpf(float(B[i, j])) * h
    E = _np(mp.expm(M))
    return E[:ns, :ns].copy(), E[:ns, ns:].copy()


def _mp_gain(A, B, X, R):
    BtX = B.T * X
    return mp.inverse(R + BtX * B) * (BtX * A)


def mp_dare(A, B, Q, R, X0=None):
    """-> (X, K, residual / max|X|, spectral radius of A - B K); X, K rounded once to fp64.  Q may be an mp matrix."""
    mp.mp.dps = DPS
    Am, Bm, Rm = _mpm(A), _mpm(B), _mpm(R)
    Qm = Q if isinstance(Q, mp.matrix) else _mpm(Q)
    n = Am.rows
    if X0 is None:
        X0 = scipy.linalg.solve_discrete_are(np.asarray(A), np.asarray(B), _np(Qm), np.asarray(R))
    X = _mpm(X0)
    for _ in range(12):
        K = _mp_gain(Am, Bm, X, Rm)
        Ac = Am - Bm * K
        C = Qm + K.T * Rm * K
        L = mp.zeros(n * n)
        rhs = mp.zeros(n * n, 1)
        for i in range(n):
            for j in range(n):
                rhs[i * n + j] = C[i, j]
                for k in range(n):
                    for l in range(n):
                        L[i * n + j, k * n + l] = (1 if (i == k and j == l) else 0) - Ac[k, i] * Ac[l, j]
        v = mp.lu_solve(L, rhs)
        Xn = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                Xn[i, j] = (v[i * n + j] + v[j * n + i]) / 2
        xmax = max(abs(Xn[i, j]) for i in range(n) for j in range(n))
        step = max(abs(Xn[i, j] - X[i, j]) for i in range(n) for j in range(n)) / xmax
        X = Xn
        if step < mp.mpf(10) ** (-42):
            break
    K = _mp_gain(Am, Bm, X, Rm)
    res, xmax = mp_dare_residual(Am, Bm, Qm, Rm, X)
    rho = float(np.abs(np.linalg.eigvals(_np(Am - Bm * K))).max())
    return _np(X), _np(K), float(res / xmax), rho


def mp_dare_residual(A, B, Q, R, X):
    mp.mp.dps = DPS
    A, B, R, X = (m if isinstance(m, mp.matrix) else _mpm(m) for m in (A, B, R, X))
    Q = Q if isinstance(Q, mp.matrix) else _mpm(Q)
    BtX = B.T * X
    Rr = A.T * X * A - X - (A.T * X * B) * mp.inverse(R + BtX * B) * (BtX * A) + Q
    n = X.rows
    return max(abs(Rr[i, j]) for i in range(n) for j in range(n)), max(abs(X[i, j]) for i in range(n) for j in range(n))


def mp_ctc(C):
    """C'C exactly (the Q of a q_from_cd case is formed from the fp64 Cd the kernel is given)"""
    mp.mp.dps = DPS
    Cm = _mpm(C)
    return Cm.T * Cm


def relerr(got, ref):
    with np.errstate(all="ignore"):
        return float(np.abs(np.asarray(got) - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------------------------------------ cases
def zoh_cases(g):
    rng = np.random.default_rng(SEED)
    c9, c18 = [], []
    for xcg in (25, 35):
        for dt in (1e-3, 5e-3, 2e-2, 0.2):
            c9.append((f"trim_xcg{xcg}_dt{dt:g}", g[f"ssr_Ac_xcg{xcg}"], g[f"ssr_Bc_xcg{xcg}"], dt))
        for dt in (1e-3, 2e-2, 0.1):
            c18.append((f"trim18_xcg{xcg}_dt{dt:g}", g[f"A18_xcg{xcg}"], g[f"B18_xcg{xcg}"], dt))
    # structure cases
    c9.append(("zeroA", np.zeros((9, 9)), rng.standard_normal((9, 3)), 1e-3))
    N = np.zeros((9, 9))
    for i in range(8):
        N[i, i + 1] = 1.0 + 0.25 * i
    Bn = np.zeros((9, 3))
    Bn[8, 0], Bn[5, 1], Bn[2, 2] = 1.0, -2.0, 0.5
    c9.append(("nilpotent_chain", N, Bn, 0.5))
    Rm = np.diag([0.0, 0.0, -1.0, -2.0, -3.0, -4.0, -5.0, -6.0, -7.0])
    Rm[0, 1], Rm[1, 0] = 40.0, -40.0
    c9.append(("rotation_block", Rm, rng.standard_normal((9, 3)), 0.1))
    # scaling threshold: dyadic entries, so every row sum is exact; row 0 sums to 4 (dt = 1/8: norm exactly 0.5, s = 0) or to
    # 4 + 2^-50 (one ulp above 0.5 after the multiplication: s = 1)
    At = rng.integers(-4, 5, (9, 9)) / 16.0
    Bt = rng.integers(-4, 5, (9, 3)) / 16.0
    rest = np.abs(At[0, 1:]).sum() + np.abs(Bt[0]).sum()
    At[0, 0] = -(4.0 - rest)
    c9.append(("threshold_at_half", At.copy(), Bt, 0.125))
    At[0, 0] = -(4.0 - rest) - 2.0 ** -50
    c9.append(("threshold_one_ulp_above", At.copy(), Bt, 0.125))
    return c9, c18


def flight_models(oracle):
    """(name, Ad, Bd, Cd) at the corners of the (h, V) range tests/test_gpu_trim.py samples: mo.trim -> linearise_na -> mp ZOH"""
    out = []
    for h, v in ((5000, 450), (30000, 450), (5000, 850), (30000, 850)):
        cand = [(h, v)] + [(h + dh, v + dv) for dh, dv in ((0, 50), (0, -50), (5000, 0), (-5000, 0), (0, 100), (0, -100), (0, 150), (0, -150))]
        for hh, vv in cand:
            x, opt = mo.trim(oracle, float(hh), float(vv))
            if opt.success and opt.fun < 1e-3 and np.isfinite(x).all():      # (the golden trim point itself reaches 2e-4 this way)
                break
        else:
            raise RuntimeError(f"no trimmable condition near ({h}, {v})")
        A, B, C, _ = oracle.linearise_na(x)
        Ad, Bd = mp_zoh(A, B, 1e-3)
        name = f"flight_h{hh}_V{vv}" + ("" if (hh, vv) == (h, v) else f"_replaces_h{h}_V{v}")
        out.append((name, Ad, Bd, C))
    return out


def pivot_case(i, j, R, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((9, 9))
    A *= 0.95 / np.abs(np.linalg.eigvals(A)).max()
    B = np.zeros((9, 3))
    B[i, 0], B[j, 0] = 1.0, -1.0
    others = [k for k in range(9) if k not in (i, j)]
    B[others[0], 1], B[others[-1], 2] = 1.0, 1.0
    Q = np.eye(9)
    Q[i, i], Q[i, j], Q[j, i], Q[j, j] = 2.0, 3.0, 3.0, 10.0
    return A, B, Q, R


def cap_case(a00=1.0):
    A = np.diag([a00, 0.5, 0.3, 0.2, 0.1, 0.9, 0.8, 0.7, 0.6])
    B = np.zeros((9, 3))
    B[1, 0] = B[2, 1] = B[3, 2] = 1.0
    return A, B, np.eye(9), np.eye(3)


def dare_cases(g, g8b, oracle):
    """(name, Ad, Bd, Cd, Q or None (= Cd'Cd on the device), R)"""
    I3, I9 = np.eye(3), np.eye(9)
    cases = []
    for xcg in (25, 35):
        Ad, Bd, Cd = (g[f"ssr_{k}_xcg{xcg}"] for k in ("Ad", "Bd", "Cd"))
        cases += [(f"trim_xcg{xcg}_QCdCd_R1", Ad, Bd, Cd, None, I3),
                  (f"trim_xcg{xcg}_QI_R1e4", Ad, Bd, Cd, I9, 1e4 * I3),
                  (f"trim_xcg{xcg}_QCdCd_R1e4", Ad, Bd, Cd, None, 1e4 * I3),
                  (f"trim_xcg{xcg}_QCdCd_R0.01", Ad, Bd, Cd, None, 0.01 * I3),
                  (f"trim_xcg{xcg}_g8b_Qb_Rb", Ad, Bd, Cd, g8b["Qb"], g8b["Rb"])]
    for xcg in (25, 35):
        Ad, Bd = mp_zoh(g[f"ssr_Ac_xcg{xcg}"], g[f"ssr_Bc_xcg{xcg}"], 2e-2)
        cases.append((f"trim_xcg{xcg}_dt0.02_QCdCd_R1", Ad, Bd, g[f"ssr_Cd_xcg{xcg}"], None, I3))
    for name, Ad, Bd, Cd in flight_models(oracle):
        cases.append((name + "_QCdCd_R1", Ad, Bd, Cd, None, I3))
    # an output matrix that is no selection matrix, so that the Q = Cd'Cd of neighbouring aircraft of a batch differ
    for xcg in (25, 35):
        Cw = np.diag([1.0, 2.0, 0.5, 1.5, 0.25, 3.0, 1.0, 0.75, 1.25]) if xcg == 25 else np.diag(np.linspace(0.5, 2.5, 9))
        cases.append((f"trim_xcg{xcg}_Cd_weighted_R1", g[f"ssr_Ad_xcg{xcg}"], g[f"ssr_Bd_xcg{xcg}"], Cw, None, I3))
    for k, (i, j, R) in enumerate(((0, 1, I3), (4, 5, I3), (7, 8, I3), (0, 1, np.diag([1.0, 4.0, 0.25])))):
        A, B, Q, R = pivot_case(i, j, R, SEED + 1 + k)
        cases.append((f"pivot_{i}{j}" + ("" if k < 3 else "_Rdiag"), A, B, I9, Q, R))
    return cases


def status_cases(g):
    """(name, Ad, Bd, Cd, Q, R, finite): no reference; F16_ST_QP_MAXITER expected, outputs finite or not"""
    A, B, Q, R = cap_case(1.0)
    out = [("cap_60_doublings", A, B, np.eye(9), Q, R, 1)]
    A, B, Q, R = cap_case(1.5)
    out.append(("overflow_H", A, B, np.eye(9), Q, R, 0))
    out.append(("nan_Ad", np.full((9, 9), np.nan), g["ssr_Bd_xcg25"], np.eye(9), np.eye(9), np.eye(3), 0))
    return out


# ------------------------------------------------------------------------------------------------ main
def save_npz(path, arrays):
    """np.savez with fixed member timestamps: the same data gives the same bytes"""
    import io
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    g = np.load(os.path.join(REPO, "tests", "golden", "g567_trim_lin_lqr.npz"))
    g8b = np.load(os.path.join(REPO, "tests", "golden", "g8b_mpc_qp_weights.npz"))
    oracle = mo.COracle()
    out, lines = {"seed": np.array(SEED), "digits": np.array(DPS)}, []
    lines.append("# G19 (tools/make_control_golden.py): fp64 error of each implementation against the 60-digit reference,")
    lines.append("# max|got - ref| / max|ref| per output block.  twin = oracle/control_twin.py (the kernels' rules in numpy).")
    lines.append("")
    lines.append("## ZOH: case | s | Ad: twin oracle.c2d scipy.expm | Bd: twin oracle.c2d scipy.expm")
    for tag, cases in zip(("zoh9", "zoh18"), zoh_cases(g)):
        names, A, B, dts, Adr, Bdr, ss, yard = [], [], [], [], [], [], [], []
        for name, a, b, dt in cases:
            ad, bd = mp_zoh(a, b, dt)
            tad, tbd, s = ct.zoh(a, b, dt)
            oad, obd = oracle.c2d(a, b, dt)
            ns = a.shape[0]
            Ms = np.zeros((ns + b.shape[1],) * 2)
            Ms[:ns, :ns], Ms[:ns, ns:] = a * dt, b * dt
            Es = scipy.linalg.expm(Ms)
            e = [relerr(tad, ad), relerr(oad, ad), relerr(Es[:ns, :ns], ad), relerr(tbd, bd), relerr(obd, bd), relerr(Es[:ns, ns:], bd)]
            lines.append(f"{name:32s} s={s:2d} | " + " ".join(f"{v:.2e}" for v in e[:3]) + " | " + " ".join(f"{v:.2e}" for v in e[3:]))
            names.append(name); A.append(a); B.append(b); dts.append(dt); Adr.append(ad); Bdr.append(bd); ss.append(s)
            yard.append([e[0], e[3]])
        d = dict(names=np.array(names), A=np.array(A), B=np.array(B), dt=np.array(dts), Ad=np.array(Adr), Bd=np.array(Bdr),
                 s=np.array(ss, dtype=np.int32), twin_err=np.array(yard))
        out.update({f"{tag}_{k}": v for k, v in d.items()})
    zs = dict(zip(out["zoh9_names"], out["zoh9_s"]))
    assert zs["threshold_at_half"] == 0 and zs["threshold_one_ulp_above"] == 1, zs
    assert [zs[f"trim_xcg25_dt{d:g}"] for d in (1e-3, 5e-3, 2e-2, 0.2)] == [2, 4, 6, 9], zs

    lines.append("")
    lines.append("## DARE: case | doublings pivoted | X: twin oracle.dare scipy | K: twin oracle.dare+numpy scipy mo.dlqr(polish=2) | mp residual, rho(A-BK)")
    lines.append("## (oracle.dare is the R = I restatement: '-' elsewhere)")
    names, A, B, C, Q, R, qcd, Xr, Kr, yard, dbl = [], [], [], [], [], [], [], [], [], [], []
    for name, a, b, c, q, r in dare_cases(g, g8b, oracle):
        qmp = mp_ctc(c) if q is None else q
        qnp = c.T @ c if q is None else q
        xs = scipy.linalg.solve_discrete_are(a, b, qnp, r)
        x, k, res, rho = mp_dare(a, b, qmp, r, xs)
        assert res <= 1e-30, (name, res)
        assert rho < 1.0, (name, rho)
        tx, it, npiv = ct.dare(a, b, qnp, r)
        tk = ct.gain(a, b, tx, r)
        assert it < ct.MAX_DOUBLINGS, (name, it)
        ks = np.linalg.inv(b.T @ xs @ b + r) @ (b.T @ xs @ a)
        e = [relerr(tx, x), None, relerr(xs, x), relerr(tk, k), None, relerr(ks, k), relerr(mo.dlqr(a, b, qnp, r, polish=2), k)]
        if np.array_equal(r, np.eye(3)):
            ox = oracle.dare(a, b, qnp)
            e[1], e[4] = relerr(ox, x), relerr(np.linalg.inv(b.T @ ox @ b + r) @ (b.T @ ox @ a), k)
        if name.startswith("pivot"):
            assert npiv >= 1, name
            _, it_np, _ = ct.dare(a, b, qnp, r, allow_pivot=False)
            assert it_np == ct.MAX_DOUBLINGS, (name, "natural-order elimination alone must not survive")
        f = lambda v: "   -    " if v is None else f"{v:.2e}"
        lines.append(f"{name:40s} {it:2d} {npiv:2d} | " + " ".join(f(v) for v in e[:3]) + " | " + " ".join(f(v) for v in e[3:])
                     + f" | {res:.1e} {rho:.6f}")
        names.append(name); A.append(a); B.append(b); C.append(c); Q.append(qnp); R.append(r); qcd.append(q is None)
        Xr.append(x); Kr.append(k); yard.append([e[0], e[3]]); dbl.append(it)
    out.update(dare_names=np.array(names), dare_A=np.array(A), dare_B=np.array(B), dare_C=np.array(C), dare_Q=np.array(Q),
               dare_R=np.array(R), dare_q_from_cd=np.array(qcd), dare_X=np.array(Xr), dare_K=np.array(Kr), dare_twin_err=np.array(yard),
               dare_doublings=np.array(dbl, dtype=np.int32))

    lines.append("")
    lines.append("## status-only cases: case | twin doublings (60 = F16_ST_QP_MAXITER) | outputs finite")
    sc = status_cases(g)
    for name, a, b, c, q, r, fin in sc:
        tx, it, _ = ct.dare(a, b, q, r)
        assert it == ct.MAX_DOUBLINGS and bool(np.isfinite(tx).all()) == bool(fin), (name, it)
        lines.append(f"{name:32s} {it:2d} {int(np.isfinite(tx).all())}")
    out.update(status_names=np.array([s[0] for s in sc]), status_A=np.array([s[1] for s in sc]), status_B=np.array([s[2] for s in sc]),
               status_C=np.array([s[3] for s in sc]), status_Q=np.array([s[4] for s in sc]), status_R=np.array([s[5] for s in sc]),
               status_finite=np.array([s[6] for s in sc], dtype=np.int32))
    save_npz(OUT, out)
    device = []
    if os.path.exists(TXT):                      # keep the device figures a GPU run appended (tests/test_gpu_control_mp.py)
        txt = open(TXT).read().split("\n## device", 1)
        device = ["## device" + txt[1].rstrip("\n")] if len(txt) == 2 else []
    with open(TXT, "w") as fh:
        fh.write("\n".join(lines + ([""] + device if device else [])) + "\n")
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; {TXT}")


if __name__ == "__main__":
    main()
