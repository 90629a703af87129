"""oracle/control_twin.py -- TEST INFRASTRUCTURE, NOT PRODUCT.

numpy restatement of the RULES of the two model kernels of csrc/f16_mpc_model.hpp, operation for operation in fp64 but with
numpy's own rounding (no FMA contraction, no matrix-core summation order, IEEE divisions):

  * `zoh`       c2d_wave: row-sum norm, s = ceil(log2(norm / 0.5)) squarings, 13 Taylor terms with a reciprocal multiply;
  * `inverse9`  inverse9_tile<PIVOT>: Gauss-Jordan on [M | I] without row swaps, the row map applied at write-back;
  * `dare`      dare_sda_wave: the doubling iteration, the natural-order inverse accepted on max|M W - I| <= 2e-9 and repeated with
                pivoting otherwise, the stop rule dmax <= 1e-16 hmax with NaN-dropping maxima (fmax), at most 60 doublings, and 60
                reported whenever the solution is not finite;
  * `gain`      lqr_gain_wave: K = (R + B'XB)^-1 B'XA.

The error of these functions against the multiprecision fixture G19 (tools/make_control_golden.py) is the yardstick of the device
tolerances in tests/test_gpu_control_mp.py: same algorithm, different rounding.
"""
import numpy as np

MAX_DOUBLINGS = 60


def zoh(A, B, dt, terms=13):
    """-> (Ad, Bd, s): the top blocks of expm([[A, B], [0, 0]] dt) and the number of squarings taken."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    ns = A.shape[0]
    nrm = 0.0
    for i in range(ns):
        rs = 0.0
        for v in A[i]:
            rs += abs(v)
        for v in B[i]:
            rs += abs(v)
        nrm = max(nrm, rs * abs(dt))
    s = 0
    if nrm > 0.5:
        s = min(40, int(np.ceil(np.log2(nrm / 0.5))))
    sc = np.ldexp(dt, -s)
    X = A * sc
    T = np.hstack([A * sc, B * sc])
    EF = T + np.eye(ns, T.shape[1])
    for k in range(2, terms + 1):
        T = (X @ T) * (1.0 / k)
        EF = EF + T
    for _ in range(s):
        Tn = EF[:, :ns] @ EF
        Tn[:, ns:] += EF[:, ns:]
        EF = Tn
    return EF[:, :ns].copy(), EF[:, ns:].copy(), s


def inverse9(M, pivot):
    """-> (W, ok).  pivot=False: natural-order elimination, ok = no exactly zero pivot (W may then be non-finite)."""
    n = M.shape[0]
    r = np.hstack([np.asarray(M, dtype=np.float64), np.eye(n)])
    ok = True
    done, pinv = [False] * n, list(range(n))
    with np.errstate(all="ignore"):
        for p in range(n):
            c = r[:, p].copy()
            if pivot:
                best, piv, cp = -1.0, 0, 1.0
                for i in range(n):
                    v = -1.0 if done[i] else abs(c[i])
                    if v > best:
                        best, piv, cp = v, i, c[i]
                ok = ok and best > 0.0
                done[piv] = True
                pinv[piv] = p
            else:
                piv, cp = p, c[p]
                ok = ok and bool(cp != 0.0)
            rp = r[piv] * (1.0 / cp)
            for i in range(n):
                r[i] = rp if i == piv else r[i] - c[i] * rp
    W = np.empty((n, n))
    for i in range(n):
        W[pinv[i]] = r[i, n:]
    return W, ok


def _rinv(R):
    """the cofactor inverse of fill_prob_qr (f16_control.hip)"""
    R = np.asarray(R, dtype=np.float64).reshape(9)
    c00, c01, c02 = R[4] * R[8] - R[5] * R[7], R[5] * R[6] - R[3] * R[8], R[3] * R[7] - R[4] * R[6]
    det = R[0] * c00 + R[1] * c01 + R[2] * c02
    inv = np.array([c00, R[2] * R[7] - R[1] * R[8], R[1] * R[5] - R[2] * R[4],
                    c01, R[0] * R[8] - R[2] * R[6], R[2] * R[3] - R[0] * R[5],
                    c02, R[1] * R[6] - R[0] * R[7], R[0] * R[4] - R[1] * R[3]])
    return (inv / det).reshape(3, 3)


def _fmax_abs(M):
    return float(np.fmax.reduce(np.abs(M).ravel(), initial=0.0))      # fmax drops NaN, as the kernel's maxima do


def dare(A0, B, Q, R=None, allow_pivot=True):
    """-> (X, doublings, pivoted): doublings == 60 reports non-convergence (or a solution that is not finite); pivoted counts the
    inversions that fell back to partial pivoting.  allow_pivot=False keeps the natural-order inverse whatever its residual."""
    A, B, H = (np.array(a, dtype=np.float64) for a in (A0, B, Q))
    n = A.shape[0]
    identity_r = R is None or np.array_equal(np.asarray(R), np.eye(3))
    G = B @ B.T if identity_r else (B @ _rinv(R)) @ B.T
    eye = np.eye(n)
    it, pivoted = 0, 0
    with np.errstate(all="ignore"):
        while it < MAX_DOUBLINGS:
            M = eye + G @ H
            GAt = G @ A.T
            W, good = inverse9(M, False)
            E = (eye + H @ G).T @ W - eye
            good = good and _fmax_abs(E) <= 2e-9
            if not good and allow_pivot:
                pivoted += 1
                W, ok = inverse9(M, True)
                if not ok:
                    it = MAX_DOUBLINGS
                    break
            T1 = A @ W
            An = T1 @ A
            G = G + T1 @ GAt
            dH = A.T @ ((H @ W) @ A)
            H = H + dH
            A = An
            it += 1
            if _fmax_abs(dH) <= 1e-16 * _fmax_abs(H):
                break
    X = 0.5 * (H + H.T)
    if not np.isfinite(X).all():
        it = MAX_DOUBLINGS
    return X, it, pivoted


def gain(A, B, X, R=None):
    """K = (R + B'XB)^-1 B'XA (utils.py:244); the library returns -K."""
    A, B, X = (np.asarray(a, dtype=np.float64) for a in (A, B, X))
    with np.errstate(all="ignore"):
        XB = X @ B
        S = B.T @ XB + (np.eye(3) if R is None else np.asarray(R, dtype=np.float64))
        if not np.isfinite(S).all():
            return np.full((3, A.shape[0]), np.nan)
        return np.linalg.inv(S) @ (XB.T @ A)
