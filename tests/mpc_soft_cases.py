"""Soft state rows (C-ABI f16_mpc_plan_soft_rows): the CPU twin of the soft solve, the equivalent slack QP, and the cases the CPU and
GPU tests share.  No tests here.

The soft problem:  min 1/2 u'Pu + q'u + sum over soft rows i of (w_i / 2) dist(a_i'u, [l_i, u_i])^2  subject to the hard rows.
admm_osqp_soft is oracle.mpc_oracle.admm_osqp(drop_unbounded_rows=True) with three rule changes, each marked (1) (2) (3) below; every
other line is that function's, in its order."""
import numpy as np
import scipy.linalg

from conftest import golden
from oracle import mpc_oracle as mo

SOFT_ACTIVE = 1 << 27                       # F16_ST_QP_SOFT_ACTIVE
BOUNDED = np.array([0, 0, 1, 1, 1, 1, 1, 0, 1], dtype=bool)      # MPC states with a box: alpha, beta, p, q, r, lf2


def state_row_weights(w, hzn, rows):
    """The per-row weight vector of a QP in the reference's row order (9 hzn state rows first) from a scalar (the six bounded rows)
    or nine weights in MPC-state order."""
    w9 = np.where(BOUNDED, float(w), 0.0) if np.ndim(w) == 0 else np.asarray(w, dtype=float)
    out = np.zeros(rows)
    out[:9 * hzn] = np.tile(w9, hzn)
    return out


def admm_osqp_soft(P, q, A, l, u, w, **kw):
    """w: one weight per row of A (0: the row is hard).  Returns admm_osqp's dict plus soft_active: some soft row's z of the returned
    iterate lies outside its [l, u]."""
    o = dict(mo.OSQP_DEFAULTS)
    o.update(kw)
    l = np.maximum(np.asarray(l, dtype=float), -mo.OSQP_INFTY)
    u = np.minimum(np.asarray(u, dtype=float), mo.OSQP_INFTY)
    n = P.shape[0]
    Ps, qs, As, ls, us, D, E, c = mo.osqp_scale(P, q, A, l, u, o["scaling"])
    loose = (ls < -mo.OSQP_INFTY * mo.MIN_SCALING) & (us > mo.OSQP_INFTY * mo.MIN_SCALING)
    keep = ~loose
    As, ls, us, Ek, wk = As[keep], ls[keep], us[keep], E[keep], np.asarray(w, dtype=float)[keep]
    m = As.shape[0]
    eq = (us - ls) < mo.RHO_TOL
    rho, sigma, alpha = float(o["rho"]), o["sigma"], o["alpha"]
    soft = wk > 0
    wt = c * wk / Ek ** 2                   # the penalty weight in the scaled variables

    def rho_vec(r):
        return np.where(eq, mo.RHO_EQ_OVER_RHO_INEQ * r, r)

    def factor(rv):
        return scipy.linalg.cho_factor(Ps + sigma * np.eye(n) + As.T @ (rv[:, None] * As))

    def kappa_vec(rv):                      # (1) kappa = rho_i / (rho_i + c w_i / E_i^2), 0 on hard rows; changes with rho only
        return np.where(soft, rv / (rv + wt), 0.0)

    rv = rho_vec(rho)
    cho, kappa = factor(rv), kappa_vec(rv)
    x, z, y = np.zeros(n), np.zeros(m), np.zeros(m)
    Einv, Dinv, cinv = 1.0 / Ek, 1.0 / D, 1.0 / c
    it, rp, rd = 0, np.inf, np.inf
    infeasible = converged = False
    for it in range(1, o["max_iter"] + 1):
        xt = scipy.linalg.cho_solve(cho, sigma * x - qs + As.T @ (rv * z - y))
        zt = As @ xt
        x = alpha * xt + (1 - alpha) * x
        zr = alpha * zt + (1 - alpha) * z
        v = zr + y / rv
        zc = np.clip(v, ls, us)
        z_new = zc + kappa * (v - zc)       # (1) the proximal step of the penalty; zc itself where kappa = 0 or v is inside
        dy = rv * (zr - z_new)
        y = y + dy
        z = z_new
        if it % o["check_every"] == 0 or it == o["max_iter"]:
            Ax, Px, Aty = As @ x, Ps @ x, As.T @ y
            rp = np.abs(Einv * (Ax - z)).max()
            eps_p = o["eps_abs"] + o["eps_rel"] * max(np.abs(Einv * z).max(), np.abs(Einv * Ax).max())
            rd = cinv * np.abs(Dinv * (Px + qs + Aty)).max()
            eps_d = o["eps_abs"] + o["eps_rel"] * cinv * max(np.abs(Dinv * qs).max(), np.abs(Dinv * Aty).max(), np.abs(Dinv * Px).max())
            if rp < eps_p and rd < eps_d:
                converged = True
                break
            ndy = np.abs(Ek * dy).max()
            if ndy > o["eps_prim_inf"]:
                # (2) a soft row is a row without bounds: nothing in the support function, and dy must vanish on it
                supp = np.sum(np.where(soft, 0.0, us * np.maximum(dy, 0) + ls * np.minimum(dy, 0)))
                rejected = bool(np.any(soft & (np.abs(Ek * dy) > o["eps_prim_inf"] * ndy)))
                if supp < -o["eps_prim_inf"] * ndy and not rejected and np.abs(Dinv * (As.T @ dy)).max() < o["eps_prim_inf"] * ndy:
                    infeasible = True
                    break
            if o["adaptive_rho"] and it % o["rho_every"] == 0 and it < o["max_iter"]:
                pr = np.abs(Ax - z).max() / (max(np.abs(z).max(), np.abs(Ax).max()) + 1e-10)
                dr = np.abs(Px + qs + Aty).max() / (max(np.abs(qs).max(), np.abs(Aty).max(), np.abs(Px).max()) + 1e-10)
                new = min(max(rho * np.sqrt(pr / (dr + 1e-10)), mo.RHO_MIN), mo.RHO_MAX)
                if new > rho * o["adaptive_rho_tolerance"] or new < rho / o["adaptive_rho_tolerance"]:
                    rho = new
                    rv = rho_vec(rho)
                    cho, kappa = factor(rv), kappa_vec(rv)
    xu = D * x
    if infeasible:
        xu = np.full(n, np.nan)
    # (3) exact comparisons: z == zc whenever v is inside the bounds
    soft_active = (not infeasible) and bool(np.any(soft & ((z < ls) | (z > us))))
    return dict(x=xu, iters=it, r_prim=rp, r_dual=rd, rho=rho, infeasible=infeasible, converged=converged, soft_active=soft_active)


def slack_qp(P, q, A, l, u, w):
    """The hard QP the soft problem equals: variables (u, s), one slack per soft row, cost + (w/2) s's, rows l <= A u + s <= u."""
    w = np.asarray(w, dtype=float)
    idx = np.nonzero(w > 0)[0]
    k = len(idx)
    S = np.zeros((A.shape[0], k))
    S[idx, np.arange(k)] = 1.0
    return scipy.linalg.block_diag(P, np.diag(w[idx])), np.concatenate((q, np.zeros(k))), np.hstack((A, S)), l, u


# ---- the cases
HZN, DT, XCG, DEMANDS = 30, 0.001, 0.35, (0.05, -0.02, 0.01)
W_AIRCRAFT = (0, 17, 101, 150, 26, 29)      # case W: aircraft 26 (hard: infeasible) and 29 (hard: max_iter) among ordinary ones
S_ROWS = 32                                 # case S: the first 32 aircraft of the same batch (26, 29 and 31 among them)
G_Q_BOX = (-240.0, -40.0)                   # case G: the q-rate box moved off the prediction (default -100 .. 100)
G_SHIFT = G_Q_BOX[0] + 100.0                # ... which moves l and u of rows 9 i + 5 of a fixture QP by this much


def batch_w():
    from f16_mpc_oop_py_amd.workload import config2_states
    return config2_states(192, seed=4)


def batch_s():
    x0, u0 = batch_w()
    return x0[:S_ROWS].copy(), u0[:S_ROWS].copy()


def weights_g():
    x_lb, x_ub = mo.MPC_X_LB.copy(), mo.MPC_X_UB.copy()
    x_lb[5], x_ub[5] = G_Q_BOX
    return dict(x_lb=x_lb, x_ub=x_ub)


def fixture_qp(tag, moved):
    """(P, q, A, l, u) of a G8 fixture QP; moved: the rows 9 i + 5 as in case G"""
    g8 = golden("g8_mpc_qp.npz")
    P, q, A, l, u = (np.array(g8[f"{k}_{tag}"], dtype=float) for k in "PqAlu")
    if moved:
        rows = 9 * np.arange(P.shape[0] // 3) + 5
        l[rows] += G_SHIFT
        u[rows] += G_SHIFT
    return P, q, A, l, u
