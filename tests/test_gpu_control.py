"""GPU parity tests of the control chain (linearise -> ZOH -> LQR -> condensed QP -> ADMM) through the C-ABI.

Oracle: golden fixtures captured from the reference's env.py/utils.py (+scipy) and, for the QP solve -- which the
reference delegates to the absent `osqp` package ("parity unpinned") -- the exact minimiser of the
strictly convex QP (tests/golden/g8, computed by oracle.mpc_oracle.qp_exact) and the same-algorithm numpy ADMM.
Tolerances: A,B by differences <= 1e-6 abs; K,P,q <= 1e-6 relative; MPC first move within the
OSQP default tolerance band of the exact minimiser."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import REPO, golden
from oracle import mpc_oracle as mo

pytestmark = pytest.mark.gpu


def make_env(x, u=None, **kw):
    from f16_mpc_oop_py_amd import F16Batch
    return F16Batch(x, u, device="cuda:0", **kw)


def rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


def soa(a, dev="cuda:0"):
    """[B, ...] -> state-major [prod(...), B] device tensor."""
    a = np.asarray(a, dtype=np.float64)
    return torch.as_tensor(a.reshape(a.shape[0], -1).T.copy(), device=dev)


# The two settings of the QP solve and their same-algorithm twins on the CPU: "osqp" = the library default = what the
# reference's call implies (env.py:420-422: osqp defaults -> Ruiz equilibration, rho 0.1, adaptive rho); "builder" = the
# opt-in rule (no equilibration, rho0 = 2 sqrt(tr P / tr A'A)).
MODES = {"osqp": (None, lambda *qp, **kw: mo.admm_osqp(*qp, drop_unbounded_rows=True, **kw)),
         "builder": (dict(scaling=0, rho=0.0), mo.admm_osqp_style)}


def mode_settings(mode, **extra):
    s = dict(MODES[mode][0] or {})
    s.update(extra)
    return s or None


@pytest.mark.parametrize("xcg", [25, 35])
def test_linearise_c2d_lqr_vs_reference(xcg):
    g = golden("g567_trim_lin_lqr.npz")
    x = np.tile(g[f"trim_x_xcg{xcg}"], (3, 1))
    env = make_env(x, xcg=xcg / 100)
    # the reference's own call shape (env.py:49): linearise(x9, u3, _calc_xdot=_calc_xdot_na, get_obs=_get_obs_na)
    Ac, Bc, Cc, Dc = (t.cpu().numpy() for t in env.linearise(env._get_mpc_x(), env._get_mpc_u(), _calc_xdot=env._calc_xdot_na,
                                                              get_obs=env._get_obs_na))
    A18 = env.linearise(env.x_values, env.u_values)[0].cpu().numpy()          # env.py:45: the default is the 18-state model
    np.testing.assert_allclose(A18[1], g[f"A18_xcg{xcg}"], rtol=0, atol=2e-6)
    with pytest.raises(ValueError):
        env.linearise(env.x_values, env.u_values, _calc_xdot=lambda x, u: x)
    for b in range(3):
        np.testing.assert_allclose(Ac[b], g[f"ssr_Ac_xcg{xcg}"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(Bc[b], g[f"ssr_Bc_xcg{xcg}"], rtol=0, atol=1e-6)
        assert np.array_equal(Cc[b], g[f"ssr_Cc_xcg{xcg}"])          # selection matrix + identical rounding noise
    assert not Dc.any()
    # ZOH on the reference's own continuous matrices: isolates the expm kernel
    B = 5
    Ad, Bd = env2 = None, None
    env = make_env(np.tile(g[f"trim_x_xcg{xcg}"], (B, 1)), xcg=xcg / 100)
    Ad, Bd = env.discretise(torch.as_tensor(np.tile(g[f"ssr_Ac_xcg{xcg}"], (B, 1, 1)), device="cuda:0"),
                            torch.as_tensor(np.tile(g[f"ssr_Bc_xcg{xcg}"], (B, 1, 1)), device="cuda:0"))
    Ad = Ad.t().reshape(B, 9, 9).cpu().numpy()
    Bd = Bd.t().reshape(B, 9, 3).cpu().numpy()
    np.testing.assert_allclose(Ad[B - 1], g[f"ssr_Ad_xcg{xcg}"], rtol=0, atol=5e-15)
    np.testing.assert_allclose(Bd[0], g[f"ssr_Bd_xcg{xcg}"], rtol=0, atol=1e-17)
    # LQR gain on the reference's discrete model (isolates the DARE kernel) ...
    K = torch.empty((27, B), dtype=torch.float64, device="cuda:0")
    Pare = torch.empty((81, B), dtype=torch.float64, device="cuda:0")
    st = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    args = [soa(np.tile(g[f"ssr_{k}_xcg{xcg}"], (B, 1, 1))) for k in ("Ad", "Bd", "Cd")]
    from f16_mpc_oop_py_amd.env import _vp
    rc = env.lib.f16_lqr_batch(env.ctx.handle, _vp(args[0]), _vp(args[1]), _vp(args[2]), _vp(K), _vp(Pare), _vp(st), B, B, None)
    assert rc == 0
    Kg = K.t().reshape(B, 3, 9).cpu().numpy()
    Kref = g[f"K_lqr_xcg{xcg}"]
    assert np.abs(Kg[2] - Kref).max() / np.abs(Kref).max() < 1e-8
    assert int(st.max()) == 0
    import scipy.linalg
    Xref = scipy.linalg.solve_discrete_are(g[f"ssr_Ad_xcg{xcg}"], g[f"ssr_Bd_xcg{xcg}"],
                                           g[f"ssr_Cd_xcg{xcg}"].T @ g[f"ssr_Cd_xcg{xcg}"], np.eye(3))
    Xg = Pare.t().reshape(B, 9, 9).cpu().numpy()[1]
    assert np.abs(Xg - Xref).max() / np.abs(Xref).max() < 1e-9
    # ... and the whole env.py:344-358 chain from the trim state
    env = make_env(np.tile(g[f"trim_x_xcg{xcg}"], (2, 1)), xcg=xcg / 100)
    Kc = env._calc_LQR_gain().cpu().numpy()
    assert np.abs(Kc[1] - Kref).max() / np.abs(Kref).max() < 1e-6
    if xcg == 25:
        u = env._calc_LQR_action(0.1, -0.05, 0.02, torch.as_tensor(np.tile(Kref, (2, 1, 1)), device="cuda:0"),
                                 np.tile(g["lqr_action_x9"], (2, 1)), np.tile(g["trim_x_xcg25"][13:16], (2, 1)))
        np.testing.assert_allclose(u[0].cpu().numpy(), g["lqr_action_u"], rtol=1e-12)


def qp_debug(env, Ad, Bd, Cd, dem, b, N):
    n, rows = 3 * N, 15 * N
    P, q, A = np.zeros((n, n)), np.zeros(n), np.zeros((rows, n))
    l, u = np.zeros(rows), np.zeros(rows)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    from f16_mpc_oop_py_amd.env import _vp
    rc = env.lib.f16_mpc_qp_debug(env.ctx.handle, _vp(Ad), _vp(Bd), _vp(Cd), _vp(env._x), _vp(dem), b, env.B, N, env.dt,
                                  p(P), p(q), p(A), p(l), p(u))
    assert rc == 0, env.lib.f16_last_error()
    return P, q, A, l, u


@pytest.mark.parametrize("xcg", [25, 35])
@pytest.mark.parametrize("N", [4, 10, 30])
def test_qp_build_vs_reference_setup_OSQP(xcg, N):
    g5, g8 = golden("g567_trim_lin_lqr.npz"), golden("g8_mpc_qp.npz")
    B = 3
    env = make_env(np.tile(g5[f"trim_x_xcg{xcg}"], (B, 1)), xcg=xcg / 100)
    Ad, Bd, Cd = (soa(np.tile(g5[f"ssr_{k}_xcg{xcg}"], (B, 1, 1))) for k in ("Ad", "Bd", "Cd"))
    dem = torch.zeros((3, B), dtype=torch.float64, device="cuda:0")
    P, q, A, l, u = qp_debug(env, Ad, Bd, Cd, dem, 1, N)
    env.ssr = (Ad, Bd, Cd)                                   # the class-level mirror of utils.py:21 gives the same QP
    for got, ref in zip(env.setup_OSQP(0.0, 0.0, 0.0, N, b=1), (P, q, A, l, u)):
        assert np.array_equal(got, ref)
    tag = f"xcg{xcg}_N{N}"
    assert np.abs(P - g8[f"P_{tag}"]).max() / np.abs(g8[f"P_{tag}"]).max() < 1e-9
    assert np.abs(q - g8[f"q_{tag}"]).max() / np.abs(g8[f"q_{tag}"]).max() < 1e-7
    np.testing.assert_allclose(A, g8[f"A_{tag}"], rtol=1e-12, atol=1e-18)
    fin = np.isfinite(g8[f"l_{tag}"])
    assert np.array_equal(np.isfinite(l), fin) and np.array_equal(np.isfinite(u), np.isfinite(g8[f"u_{tag}"]))
    np.testing.assert_allclose(l[fin], g8[f"l_{tag}"][fin], rtol=1e-12, atol=1e-12)
    fin = np.isfinite(u)
    np.testing.assert_allclose(u[fin], g8[f"u_{tag}"][fin], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("mode", ["osqp", "builder"])
@pytest.mark.parametrize("xcg", [25, 35])
def test_mpc_action_vs_exact_minimiser_and_same_algorithm_oracle(xcg, mode):
    g5, g8 = golden("g567_trim_lin_lqr.npz"), golden("g8_mpc_qp.npz")
    B, N = 4, 30
    env = make_env(np.tile(g5[f"trim_x_xcg{xcg}"], (B, 1)), xcg=xcg / 100)
    env.ssr = tuple(soa(np.tile(g5[f"ssr_{k}_xcg{xcg}"], (B, 1, 1))) for k in ("Ad", "Bd", "Cd"))
    tag = f"xcg{xcg}_N{N}"
    xstar = g8[f"xstar_{tag}"]
    u, info = env._calc_MPC_action(0.0, 0.0, 0.0, N, settings=mode_settings(mode), return_info=True)
    u = u.cpu().numpy()
    # (a) OSQP-default tolerances: inside the solver band around the exact minimiser (eps_rel 1e-3 on rows of size ~10)
    assert np.abs(u[0] - xstar[:3]).max() < 2e-2
    assert int(info["status"].max()) == 0
    # (b) same algorithm, same settings, in numpy: iterates agree to rounding, same iteration count, same final rho
    ref = MODES[mode][1](*(g8[f"{k}_{tag}"] for k in "PqAlu"))
    assert int(info["iters"][0]) == ref["iters"]
    assert np.abs(info["u_seq"][0].cpu().numpy() - ref["x"]).max() < 1e-7
    assert abs(float(info["rho"][0]) - ref["rho"]) < 1e-8 * ref["rho"]
    assert abs(float(info["r_prim"][0]) - ref["r_prim"]) < 1e-7 and abs(float(info["r_dual"][0]) - ref["r_dual"]) < 1e-7
    # (c) tight tolerances: converges to the exact minimiser
    u, info = env._calc_MPC_action(0.0, 0.0, 0.0, N, settings=mode_settings(mode, eps_abs=1e-9, eps_rel=1e-9, max_iter=400000),
                                   return_info=True)
    assert np.abs(info["u_seq"][2].cpu().numpy() - xstar).max() < 1e-5
    assert int(info["status"].max()) == 0
    if xcg == 35 and mode == "builder":
        np.testing.assert_allclose(u[3].cpu().numpy(), [-0.56435742, -0.01095324, 0.00097151], atol=2e-6)


@pytest.mark.parametrize("mode", ["osqp", "builder"])
def test_mpc_batch_of_perturbed_aircraft_vs_oracle_chain(oracle, mode):
    """Config-4 shape at reduced batch: each aircraft linearised at its own state (xcg 0.35), N=30, demands != 0."""
    from f16_mpc_oop_py_amd.workload import config2_states
    B, N = 192, 30
    x0, u0 = config2_states(B, seed=4)
    env = make_env(x0, u0, xcg=0.35)
    Ad, Bd, Cd = env.build_ssr()
    dem = np.array([0.05, -0.02, 0.01])
    u, info = env._calc_MPC_action(dem[0], dem[1], dem[2], N, settings=mode_settings(mode), return_info=True)
    u = u.cpu().numpy()
    st = info["status"].cpu().numpy()
    Adh, Bdh, Cdh = (t.t().cpu().numpy() for t in (Ad, Bd, Cd))
    # aircraft 26 sits on the lf2 = 25 bound and its linear model predicts leaving it: infeasible QP (OSQP would
    # return NaN); aircraft 29 violates lf2 >= 0 by ~3e-5 only and converges slowly.
    for b in (0, 17, 101, 150, 26, 29):
        A_, B_, C_, D_ = oracle.linearise_na(x0[b], u3=u0[b, 1:], xcg=0.35)
        Ado, Bdo, _, _ = mo.c2d(A_, B_, C_, D_, 0.001)
        np.testing.assert_allclose(Adh[b].reshape(9, 9), Ado, rtol=0, atol=1e-9)
        np.testing.assert_allclose(Bdh[b].reshape(9, 3), Bdo, rtol=0, atol=1e-9)
        # QP + solve from the GPU's own (Ad,Bd,Cd): same-algorithm agreement + exact-minimiser band
        P, q, A, l, uu = mo.mpc_qp(x0[b], Adh[b].reshape(9, 9), Bdh[b].reshape(9, 3), Cdh[b].reshape(9, 9), N, 0.001, *dem)
        ref = MODES[mode][1](P, q, A, l, uu)
        assert abs(int(info["iters"][b]) - ref["iters"]) <= 25, (b, int(info["iters"][b]), ref["iters"])
        if ref["infeasible"]:
            assert st[b] == 128 and np.isnan(u[b]).all()
            continue
        if not ref.get("converged", True):
            # with OSQP's defaults aircraft 29 (and four more of this set) runs into max_iter = 40000 (env.py:421) on the CPU
            # twin as on the GPU: OSQP would report "maximum iterations reached" -> status bit 64, the last iterate returned
            assert st[b] == 64 and int(info["iters"][b]) == 40000
            assert np.abs(u[b] - ref["x"][:3]).max() < 1e-6
            continue
        assert st[b] == 0
        assert np.abs(u[b] - ref["x"][:3]).max() < 1e-4
        if b != 29:
            xs, _ = mo.qp_exact(P, q, A, l, uu)
            assert np.abs(u[b] - xs[:3]).max() < 5e-2
    assert set(np.unique(st)) <= ({0, 128} if mode == "builder" else {0, 64, 128})


def test_config4_workload_is_feasible_everywhere():
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(1024)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    u, info = env._calc_MPC_action(0.0, 0.0, 0.0, 30, return_info=True)
    assert int(info["status"].max()) == 0 and torch.isfinite(u).all()
    assert int(info["iters"].max()) <= 5000


def test_mpc_horizon_limits_and_closed_loop_smoke():
    g5 = golden("g567_trim_lin_lqr.npz")
    env = make_env(np.tile(g5["trim_x_xcg35"], (8, 1)), xcg=0.35)
    env.build_ssr()
    from f16_mpc_oop_py_amd import lib
    with pytest.raises(lib.F16HipError):
        env._calc_MPC_action(0, 0, 0, 151)
    for N in (1, 2, 10, 40, 41):
        u = env._calc_MPC_action(0, 0, 0, N)
        assert torch.isfinite(u).all()
    # test_env.py:480-495 closed-loop pattern: cmd = MPC(...,10); u.values[1:] = cmd; step(u.values)
    for _ in range(20):
        cmd = env._calc_MPC_action(0.0, 0.0, 0.0, 10)
        env._u[1:4] = cmd.t()
        env.step()
    assert int(env.status.max()) == 0 and torch.isfinite(env.x_values).all()
    assert torch.allclose(env.x_values[0], env.x_values[7])       # identical aircraft stay identical


@pytest.mark.parametrize("xcg", [25, 35])
def test_linearise_full_18_state_and_zoh_vs_reference(xcg):
    """env.py:45-46: 18-state forward-difference model + 22x22 zero-order hold."""
    g = golden("g567_trim_lin_lqr.npz")
    x = np.tile(g[f"trim_x_xcg{xcg}"], (3, 1))
    env = make_env(x, xcg=xcg / 100)
    r = {k: v.cpu().numpy() for k, v in env.linearise_full().items()}
    for b in (0, 2):
        np.testing.assert_allclose(r["Ac"][b], g[f"A18_xcg{xcg}"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(r["Bc"][b], g[f"B18_xcg{xcg}"], rtol=0, atol=1e-6)
        assert np.array_equal(r["Cc"][b], g[f"C18_xcg{xcg}"])
        np.testing.assert_allclose(r["Ad"][b], g[f"Ad18_xcg{xcg}"], rtol=0, atol=1e-8)
        np.testing.assert_allclose(r["Bd"][b], g[f"Bd18_xcg{xcg}"], rtol=0, atol=1e-8)
    assert int(env.last_status.max()) == 0


def test_relinearised_mpc_and_trajectory_writers(tmp_path):
    """per-step re-linearised closed loop; npz + runF16Sim-style CSV writers."""
    from f16_mpc_oop_py_amd import io as fio
    g5 = golden("g567_trim_lin_lqr.npz")
    env = make_env(np.tile(g5["trim_x_xcg25"], (4, 1)))
    frozen = env._calc_MPC_action(0.0, 0.0, 0.0, 10).clone()
    relin = env._calc_MPC_action(0.0, 0.0, 0.0, 10, relinearise=True)
    assert torch.allclose(frozen, relin, atol=1e-9)                # same point -> same model -> same action
    steps = 12
    traj = torch.empty((steps, 18, 4), dtype=torch.float64, device="cuda:0")
    for k in range(steps):
        cmd = env._calc_MPC_action(0.02, 0.0, 0.0, 10, relinearise=True)
        env._u[1:4] = cmd.t()
        env.step()
        traj[k] = env._x
    assert torch.isfinite(traj).all() and int(env.status.max()) == 0
    fio.save_npz(tmp_path / "t.npz", traj, env.dt, status=env.status)
    z = np.load(tmp_path / "t.npz")
    assert z["traj"].shape == (steps, 18, 4) and abs(z["time"][-1] - steps * env.dt) < 1e-12
    rows = fio.save_csv(tmp_path / "t.txt", env, traj, aircraft=1)
    txt = open(tmp_path / "t.txt").read()
    assert "time,npos,epos,alt,phi,theta,psi,vel,alpha,beta,p,q,r,nx,ny,nz,mach,qbar,ps," in txt
    assert rows.shape == (steps, 23) and abs(rows[0, 3] - 10000.0) < 1.0 and abs(rows[0, 7] - 700.0) < 1.0
    assert 0.5 < rows[0, 16] < 0.8                                  # mach at 700 ft/s, 10 kft


def test_config5_closed_loop_rollout_single_rank():
    """BASELINE config 5 shape on one rank: per step calc_MPC_action then step, trajectory collated by dist (no group)."""
    from f16_mpc_oop_py_amd import dist as fdist
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(128)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    traj = fdist.closed_loop_mpc_rollout(env, steps=6, hzn=10, traj_every=2)
    assert tuple(traj.shape) == (3, 18, 128) and torch.isfinite(traj).all()
    assert torch.equal(traj[-1], env._x)
    assert fdist.or_status(env.status) == 0


@pytest.mark.parametrize("n", [3, 12, 30, 47, 90, 96])
def test_mfma_inverse(n):
    """KKT-inverse routine of the MPC solver on its own: blocked fp64-MFMA sweep against numpy.linalg.inv on random
    SPD matrices shaped like P + sigma I + rho A'A (condition ~1e3)."""
    from f16_mpc_oop_py_amd import lib
    L = lib.load()
    ctx = lib.Context()
    rng = np.random.default_rng(100 + n)
    Bn = 5
    mats, packed = [], []
    for _ in range(Bn):
        G = rng.standard_normal((n, n))
        Q, _ = np.linalg.qr(G)
        M = (Q * np.geomspace(1.0, 1e3, n)) @ Q.T
        M = 0.5 * (M + M.T)
        mats.append(M)
        packed.append(M[np.tril_indices(n)])
    pk = torch.tensor(np.stack(packed), dtype=torch.float64, device="cuda")
    out = torch.empty((Bn, n * n), dtype=torch.float64, device="cuda")
    lib.check(L.f16_debug_spd_inverse(ctx.handle, ctypes.c_void_p(pk.data_ptr()), ctypes.c_void_p(out.data_ptr()), n, Bn,
                                      None), L)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(Bn, n, n)
    for b in range(Bn):
        ref = np.linalg.inv(mats[b])
        assert np.isfinite(got[b]).all()
        assert np.abs(got[b] - ref).max() <= 1e-11 * np.abs(ref).max()
        assert np.abs(got[b] @ mats[b] - np.eye(n)).max() < 1e-10


def test_mpc_full_size_properties():
    """BASELINE config 4 at full size (B = 4096, N = 30, xcg 0.35) through size-independent properties:
    every solve meets OSQP's termination test; the first move respects the command and first-step rate rows
    (utils.py:139-152) up to the termination tolerance; results do not depend on an aircraft's position in the batch
    (bit-identical under a permutation); the register-resident solver and the generic one-wave solver (negative
    max_iter) agree to solver tolerance on a sample."""
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N = 4096, 30
    x0, u0 = config4_states(B)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    u, info = env._calc_MPC_action(0.0, 0.0, 0.0, N, return_info=True)
    u = u.cpu().numpy()
    assert int(info["status"].max()) == 0 and np.isfinite(u).all()
    # termination: r_prim <= eps_abs + eps_rel * max(|Ax|,|z|) needs the norms; the absolute part alone bounds the rest
    useq = info["u_seq"].cpu().numpy()                       # [B, 3N]
    scale = np.maximum(1.0, np.abs(useq).max(axis=1))
    assert (info["r_prim"].cpu().numpy() <= 1e-3 * (1 + 130 * scale)).all()
    assert np.isfinite(info["r_dual"].cpu().numpy()).all()
    lim = np.array([25.0, 21.5, 30.0])
    assert (np.abs(useq.reshape(B, N, 3)) <= lim + 5e-2).all()             # command rows, whole horizon
    act = x0[:, 13:16]
    rate = np.array([60.0, 80.0, 120.0]) * 0.001
    assert (np.abs(u - act) <= rate + 5e-2).all()                            # first-step rate rows
    # permutation invariance (bit-exact)
    perm = np.random.default_rng(5).permutation(B)
    env2 = make_env(x0[perm], u0[perm], xcg=0.35)
    env2.build_ssr()
    u2 = env2._calc_MPC_action(0.0, 0.0, 0.0, N).cpu().numpy()
    assert np.array_equal(u2, u[perm])
    # fast solver vs generic solver on a sample
    idx = np.arange(0, B, 64)
    env3 = make_env(x0[idx], u0[idx], xcg=0.35)
    env3.build_ssr()
    u3 = env3._calc_MPC_action(0.0, 0.0, 0.0, N, settings=dict(max_iter=-40000)).cpu().numpy()
    assert np.abs(u3 - u[idx]).max() < 2e-3


def test_config4_full_size_every_aircraft_vs_oracle_chain(oracle):
    """BASELINE config 4 at FULL size (B = 4096, N = 30, xcg 0.35, the reference's solver settings) against the checker:
    EVERY aircraft's first move, iteration count and status word vs the C restatement of the whole chain on the CPU
    (its own linearisation + ZOH + DARE + dense setup_OSQP + the OSQP twin, env.py:373-424; 4096 solves, ~2 s on the GPU box's
    16 cores).  The two chains differ at the 1e-9 level in (Ad, Bd) (device libm), so iterates agree to ~1e-7 until a
    termination test falls the other way; then the answers are one test interval apart, i.e. inside the solver's own tolerance.
    Observed (round 4): every status word and every iteration count equal, first moves within 2.7e-5."""
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N = 4096, 30
    x0, u0 = config4_states(B)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    u, info = env._calc_MPC_action(0.0, 0.0, 0.0, N, return_info=True)
    ref = oracle.mpc_batch(x0, N, xcg=0.35, nthreads=16)
    ug, itg, stg = u.cpu().numpy(), info["iters"].cpu().numpy().astype(int), info["status"].cpu().numpy()
    assert np.array_equal(stg, ref["status"]), np.flatnonzero(stg != ref["status"])
    same = itg == ref["iters"]
    assert same.mean() >= 0.98, (itg[~same], ref["iters"][~same])
    assert np.abs(itg - ref["iters"]).max() <= 100
    assert np.abs(ug[same] - ref["u"][same]).max() < 5e-5
    assert np.abs(ug - ref["u"]).max() < 5e-3


@pytest.mark.parametrize("N", [10, 30])
def test_prepared_plan_is_bit_identical_and_closed_loop(N):
    """f16_mpc_plan_*: the model-only part of calc_MPC_action prepared once (the reference freezes the model,
    env.py:49-60) -- commands, iteration counts and residuals equal the one-shot call bit for bit, also after the state
    has moved; a closed loop driven through the plan equals the one driven through one-shot calls."""
    from f16_mpc_oop_py_amd.workload import config4_states
    from f16_mpc_oop_py_amd import dist as fdist
    x0, u0 = config4_states(300, seed=11)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    dem = (0.03, -0.01, 0.02)
    u1, i1 = env._calc_MPC_action(*dem, N, return_info=True)
    env.prepare_MPC(N)
    u2, i2 = env._calc_MPC_action(*dem, N, return_info=True, use_plan=True)
    assert torch.equal(u1, u2) and torch.equal(i1["iters"], i2["iters"]) and torch.equal(i1["u_seq"], i2["u_seq"])
    assert torch.equal(i1["r_prim"], i2["r_prim"]) and torch.equal(i1["rho"], i2["rho"])
    env.rollout(25)                                            # move the state, keep the plan
    u3 = env._calc_MPC_action(*dem, N)
    u4 = env._calc_MPC_action(*dem, N, use_plan=True)
    assert torch.equal(u3, u4)
    with pytest.raises(ValueError):
        env._calc_MPC_action(*dem, N, use_plan=True, settings=dict(max_iter=50))
    ea = make_env(x0[:64], u0[:64], xcg=0.35); ea.build_ssr()
    eb = make_env(x0[:64], u0[:64], xcg=0.35); eb.build_ssr()
    ta = fdist.closed_loop_mpc_rollout(ea, steps=8, hzn=N, gather=False, use_plan=False)
    tb = fdist.closed_loop_mpc_rollout(eb, steps=8, hzn=N, gather=False, use_plan=True, fused=False)      # (host loop against host loop)
    assert torch.equal(ta, tb)
    if N <= 30:                       # the default for a plan: the ONE-launch loop (same commands; its step is the out-of-line one: ulps)
        ec = make_env(x0[:64], u0[:64], xcg=0.35); ec.build_ssr()
        tc = fdist.closed_loop_mpc_rollout(ec, steps=8, hzn=N, gather=False)
        assert float(((tc - tb).abs() / tb.abs().clamp(min=1.0)).max()) < 1e-9 and float((ec._u - eb._u).abs().max()) < 1e-9


def test_prepared_plan_beyond_the_register_resident_horizons():
    """Plans accept horizons up to 40: for 33..40 they keep the model part (DARE, prediction blocks, P) and every solve runs the
    long-horizon workgroup solver -- bit-identical to the one-shot call; warm start is refused there."""
    from f16_mpc_oop_py_amd import lib
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(48, seed=3)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    for N in (33, 36, 40):
        u1 = env._calc_MPC_action(0.01, 0.0, -0.01, N).clone()
        env.prepare_MPC(N)
        u2 = env._calc_MPC_action(0.01, 0.0, -0.01, N, use_plan=True)
        assert torch.equal(u1, u2, ) or (torch.isnan(u1) == torch.isnan(u2)).all() and torch.equal(torch.nan_to_num(u1), torch.nan_to_num(u2)), N
    with pytest.raises(lib.F16HipError):
        env.prepare_MPC(36, warm_start=True)
    with pytest.raises(lib.F16HipError):
        env.prepare_MPC(41)


def test_plan_warm_start_closed_loop():
    """Opt-in warm start of a prepared plan (OSQP's in-object default; the reference always starts cold): the closed
    loop stays within solver tolerance of the cold-started one and needs fewer iterations per step."""
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(256, seed=3)
    runs = {}
    for warm in (False, True):
        env = make_env(x0, u0, xcg=0.35)
        env.build_ssr()
        env.prepare_MPC(30, warm_start=warm)
        its = []
        for _ in range(12):
            cmd, info = env._calc_MPC_action(0.0, 0.0, 0.0, 30, return_info=True, use_plan=True)
            assert int(info["status"].max()) == 0
            its.append(float(info["iters"].mean()))
            env._u[1:4] = cmd.t()
            env.rollout(1)
        runs[warm] = (env.x_values.cpu().numpy(), np.array(its))
    assert runs[True][1][0] == runs[False][1][0]                # the first solve has nothing to start from
    assert runs[True][1][1:].mean() < 0.8 * runs[False][1][1:].mean()
    assert np.abs(runs[True][0] - runs[False][0]).max() < 1e-2 * max(1.0, np.abs(runs[False][0]).max()) * 1e-2 + 5e-3


def test_dispatch_order_does_not_change_results(monkeypatch):
    """The workgroup -> aircraft map of k_mpc_fast (longest solve of the previous call first) is scheduling only: the
    second call of a batch (ordered) returns bit for bit what the first call (caller's order) and an unordered call return."""
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(512, seed=11)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    u1, i1 = env._calc_MPC_action(0.0, 0.0, 0.0, 30, return_info=True)        # no history yet for this batch size
    u2, i2 = env._calc_MPC_action(0.0, 0.0, 0.0, 30, return_info=True)        # dispatched longest-first
    monkeypatch.setenv("F16_MPC_DISPATCH_ORDER", "0")
    u3, i3 = env._calc_MPC_action(0.0, 0.0, 0.0, 30, return_info=True)
    assert len(set(i1["iters"].cpu().numpy().tolist())) > 1                     # a mix of iteration counts to order
    for u, i in ((u2, i2), (u3, i3)):
        assert torch.equal(u, u1) and torch.equal(i["iters"], i1["iters"]) and torch.equal(i["u_seq"], i1["u_seq"])


# ---------------------------------------------------------------------------------------------------------------------
# Round-2 additions: oracle-checked horizons, closed loop, re-linearised loop, config-3 LQR sample
def _model_np(env):
    Ad, Bd, Cd = env.ssr
    return (Ad.t().cpu().numpy().reshape(-1, 9, 9), Bd.t().cpu().numpy().reshape(-1, 9, 3), Cd.t().cpu().numpy().reshape(-1, 9, 9))


HORIZONS = [1, 2, 5, 6, 11, 16, 21, 22, 32, 33, 40]


@pytest.mark.parametrize("mode", ["osqp", "builder"])
@pytest.mark.parametrize("generic", [False, True])
def test_every_horizon_instantiation_vs_same_algorithm_oracle(generic, mode):
    """Regression for the round-1 abort: every N in 1..40 once through the solver that owns it -- the
    register-resident kernel instantiations k_mpc_fast<2> (N <= 5), <4> (N <= 10), <6> (N <= 32, incl. the padded tile
    counts at N = 6, 11, 22) and the generic one-wave kernel (N = 33..40; forced for every N when `generic`) -- with
    status / finiteness for all N and iterate-level parity against mo.admm_osqp_style at the listed horizons."""
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(8, seed=21)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    Ad, Bd, Cd = _model_np(env)
    dem = (0.02, -0.01, 0.01)
    sett = mode_settings(mode, **(dict(max_iter=-40000) if generic else {}))
    for N in range(1, 41):
        u, info = env._calc_MPC_action(*dem, N, settings=sett, return_info=True)
        torch.cuda.synchronize()
        st = info["status"].cpu().numpy()
        fin = torch.isfinite(u).all(dim=1).cpu().numpy()
        # a long horizon can make an aircraft's QP infeasible (its linear model leaves the state box): OSQP's certificate
        # -> status bit 128 and a NaN command, exactly for those aircraft
        assert set(np.unique(st)) <= {0, 128} and np.array_equal(fin, st == 0), (N, st)
        assert tuple(info["u_seq"].shape) == (8, 3 * N)
        if N in HORIZONS:
            for b in (0, 2, 5):
                P, q, A, l, uu = mo.mpc_qp(x0[b], Ad[b], Bd[b], Cd[b], N, 0.001, *dem)
                ref = MODES[mode][1](P, q, A, l, uu)
                assert int(info["iters"][b]) == ref["iters"], (N, b)
                assert bool(ref["infeasible"]) == (st[b] == 128), (N, b)
                if not ref["infeasible"]:
                    assert np.abs(info["u_seq"][b].cpu().numpy() - ref["x"]).max() < 1e-6, (N, b)
    from f16_mpc_oop_py_amd import lib
    with pytest.raises(lib.F16HipError):
        env._calc_MPC_action(0, 0, 0, 151)
    with pytest.raises(lib.F16HipError):
        env._calc_MPC_action(0, 0, 0, 0)


def _oracle_closed_loop(oracle, x0, u0, Ad, Bd, Cd, steps, N, dem, relin, solver):
    """test_env.py:480-495 on the CPU: cmd = calc_MPC_action(p, q, r, N); u.values[1:] = cmd; step(u.values)."""
    x, u = x0.copy(), u0.copy()
    its, cmds = [], []
    for _ in range(steps):
        if relin:
            A_, B_, C_, D_ = oracle.linearise_na(x, u3=u[1:], xcg=0.35)
            Ad, Bd, Cd, _ = mo.c2d(A_, B_, C_, D_, 0.001)
        P, q, A, l, uu = mo.mpc_qp(x, Ad, Bd, Cd, N, 0.001, *dem)
        r = solver(P, q, A, l, uu)
        its.append(r["iters"])
        cmds.append(r["x"][:3].copy())
        u[1:4] = r["x"][:3]
        x, _, st = oracle.rollout(x[None], u[None], 1, xcg=0.35, store=False)
        x = x[0]
        assert st[0] == 0
    return x, np.array(cmds), np.array(its)


@pytest.mark.parametrize("mode", ["osqp", "builder"])
def test_closed_loop_mpc_vs_oracle_loop(oracle, mode):
    """BASELINE config 5 workload on one rank against the same loop on the CPU oracle (reference pattern
    test_env.py:480-495): 16 config-4 aircraft, 20 steps of calc_MPC_action(N = 30) + step -- commands <= 1e-4, states
    <= 1e-6 relative, the same iteration counts -- through one-shot calls and through a prepared plan."""
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N, steps = 16, 30, 20
    x0, u0 = config4_states(B, seed=5)
    dem = (0.02, -0.01, 0.0)
    runs = {}
    for use_plan in (False, True):
        env = make_env(x0, u0, xcg=0.35)
        env.build_ssr()
        if use_plan:
            env.prepare_MPC(N, settings=MODES[mode][0])
        cmds, its = [], []
        for _ in range(steps):
            cmd, info = env._calc_MPC_action(*dem, N, return_info=True, use_plan=use_plan,
                                             settings=None if use_plan else mode_settings(mode))
            assert int(info["status"].max()) == 0
            cmds.append(cmd.cpu().numpy().copy()); its.append(info["iters"].cpu().numpy().copy())
            env._u[1:4] = cmd.t()
            env.step()
        runs[use_plan] = (env.x_values.cpu().numpy(), np.array(cmds), np.array(its), _model_np(env))
    assert np.array_equal(runs[False][1], runs[True][1])               # plan = one-shot, bit for bit
    xg, cg, ig, (Ad, Bd, Cd) = runs[False]
    for b in (0, 3, 7, 12):
        xr, cr, ir = _oracle_closed_loop(oracle, x0[b], u0[b], Ad[b], Bd[b], Cd[b], steps, N, dem, False, MODES[mode][1])
        assert np.array_equal(ig[:, b], ir), (b, ig[:, b], ir)
        assert np.abs(cg[:, b] - cr).max() < 1e-4
        assert np.max(np.abs(xg[b] - xr) / np.maximum(1.0, np.abs(xr))) < 1e-6


def test_relinearised_closed_loop_vs_oracle_loop(oracle):
    """SURVEY.md 8f-2 (pattern of test_env.py:625-687): the reduced model re-derived at the CURRENT state before every
    solve, against oracle.linearise_na + mo.c2d + the same QP + solve on the CPU.  A, B come from forward differences
    with eps 1e-5 (device trigonometry differs from libm in the last ulps, amplified 1e5), hence the looser bands."""
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N, steps = 8, 10, 12
    x0, u0 = config4_states(B, seed=9)
    dem = (0.03, 0.0, -0.01)
    env = make_env(x0, u0, xcg=0.35)
    cmds, its = [], []
    for k in range(steps):
        cmd, info = env._calc_MPC_action(*dem, N, return_info=True, relinearise=True, settings=mode_settings("builder"))
        assert int(info["status"].max()) == 0
        cmds.append(cmd.cpu().numpy().copy()); its.append(info["iters"].cpu().numpy().copy())
        if k == steps - 1:                                              # the model of the LAST solve, at the moved state
            Ad, Bd, Cd = _model_np(env)
            xk, uk = env.x_values.cpu().numpy().copy(), env.u_values.cpu().numpy().copy()
        env._u[1:4] = cmd.t()
        env.step()
    cmds, its = np.array(cmds), np.array(its)
    xg = env.x_values.cpu().numpy()
    for b in (0, 2, 5):
        A_, B_, C_, D_ = oracle.linearise_na(xk[b], u3=uk[b, 1:], xcg=0.35)       # re-linearised AFTER the state moved
        Ado, Bdo, _, _ = mo.c2d(A_, B_, C_, D_, 0.001)
        np.testing.assert_allclose(Ad[b], Ado, rtol=0, atol=1e-9)
        np.testing.assert_allclose(Bd[b], Bdo, rtol=0, atol=1e-9)
        xr, cr, ir = _oracle_closed_loop(oracle, x0[b], u0[b], None, None, None, steps, N, dem, True, mo.admm_osqp_style)
        assert np.abs(its[:, b] - ir).max() <= 25                                   # a test interval at most (knife edges)
        assert np.abs(cmds[:, b] - cr).max() < 2e-3
        assert np.max(np.abs(xg[b] - xr) / np.maximum(1.0, np.abs(xr))) < 1e-5
    # frozen vs re-linearised differ once the state has moved (the re-derivation is not a no-op)
    env2 = make_env(x0, u0, xcg=0.35)
    env2.build_ssr()
    env2.rollout(200)
    fr = env2._calc_MPC_action(*dem, N, settings=mode_settings("builder")).clone()
    rl = env2._calc_MPC_action(*dem, N, relinearise=True, settings=mode_settings("builder"))
    assert float((fr - rl).abs().max()) > 1e-6


@pytest.mark.parametrize("xcg", [25, 35])
def test_g14_per_step_relinearised_lqr_loop_on_the_device(xcg):
    """The reference's `test_LQR_dynamic_nl` (test_env.py:625-687): per step `_calc_LQR_gain(Q = I, R = 1e4 I)` at the CURRENT state
    (device linearise -> ZOH -> doubling DARE), cmd = -dlqr (x9 - x_ref), step -- against fixture G14 (the reference's loop run in the build
    container, 150 steps).  The device's libm differs from glibc in the last ulp, eps = 1e-5 amplifies it 1e5 x, the gain carries it into
    the command: 2e-5 absolute on commands up to 2.7 deg; states 1e-6."""
    g = golden("g14_dynamic_lqr.npz")
    env = make_env(g[f"x0_xcg{xcg}"][None], g[f"u0_xcg{xcg}"][None], xcg=xcg / 100)
    xref = env._get_mpc_x().clone()
    Q, R = np.eye(9), np.eye(3) * 1e4
    worst = 0.0
    for t in range(150):
        K = env._calc_LQR_gain(Q=Q, R=R)                                  # [1,3,9] = -dlqr(Ad, Bd, Q, R) at the current state
        if t in (0, 50, 149):
            assert rel(-K[0].cpu().numpy(), g[f"K{t}_xcg{xcg}"]) < 1e-5
        cmd = (K @ (env._get_mpc_x() - xref).unsqueeze(-1)).squeeze(-1)    # -dlqr (x9 - x_ref)
        worst = max(worst, float((cmd[0].cpu() - torch.as_tensor(g[f"cmd_xcg{xcg}"][t])).abs().max()))
        env._u[1:4] = cmd.t()
        env.step()
        if (t + 1) % 10 == 0:
            r = g[f"x_xcg{xcg}"][(t + 1) // 10 - 1]
            assert np.max(np.abs(env.x_values.cpu().numpy()[0] - r) / np.maximum(1.0, np.abs(r))) < 1e-6, t
    assert worst < 2e-5, worst
    assert int(env.status.max()) == 0


def test_lqr_gain_on_config3_workload_sample(oracle):
    """BASELINE config 3 at full size (4096 perturbed flight conditions, xcg 0.25): linearise + ZOH + dlqr per aircraft;
    a 64-aircraft sample against env.py:344-358 restated on the CPU (oracle.linearise_na + scipy cont2discrete + scipy
    solve_discrete_are), K <= 1e-6 relative; the DARE kernel alone on the device's own discrete model <= 1e-8."""
    import scipy.linalg
    from f16_mpc_oop_py_amd.workload import config2_states
    from f16_mpc_oop_py_amd.env import _vp
    B = 4096
    x0, u0 = config2_states(B)
    env = make_env(x0, u0, xcg=0.25)
    K = env._calc_LQR_gain().cpu().numpy()
    assert np.isfinite(K).all() and int(env.last_status.max()) == 0
    Ad, Bd, Cd = _model_np(env)
    Pare = torch.empty((81, B), dtype=torch.float64, device="cuda:0")
    Kd = torch.empty((27, B), dtype=torch.float64, device="cuda:0")
    st = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    assert env.lib.f16_lqr_batch(env.ctx.handle, _vp(env.ssr[0]), _vp(env.ssr[1]), _vp(env.ssr[2]), _vp(Kd), _vp(Pare), _vp(st), B, B, None) == 0
    Xg = Pare.t().cpu().numpy().reshape(B, 9, 9)
    worst_k, worst_x = 0.0, 0.0
    for b in range(0, B, 64):
        Kref = mo.lqr_gain_from_linearisation(*oracle.linearise_na(x0[b], u3=u0[b, 1:], xcg=0.25), 0.001)
        worst_k = max(worst_k, np.abs(K[b] - Kref).max() / np.abs(Kref).max())
        Xref = scipy.linalg.solve_discrete_are(Ad[b], Bd[b], Cd[b].T @ Cd[b], np.eye(3))
        worst_x = max(worst_x, np.abs(Xg[b] - Xref).max() / np.abs(Xref).max())
    assert worst_x < 1e-8, worst_x
    assert worst_k < 1e-6, worst_k


def test_plan_solves_replay_from_a_hip_graph_and_one_shot_calls_refuse_capture():
    """A prepared plan owns its workspace, so its solve can be captured into a HIP graph (through torch) and replayed: six
    replays return what the eager call returns, bit for bit.  The one-shot call allocates per call, stream-ordered; graphs
    holding those allocation nodes replayed with wrong results intermittently on ROCm 7.2, so it refuses to be captured."""
    from f16_mpc_oop_py_amd import F16Batch, lib
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(256, seed=5)
    env = F16Batch(x0, u0, xcg=0.35)
    env.build_ssr()
    env.prepare_MPC(30)
    u_eager = env._calc_MPC_action(0, 0, 0, 30, use_plan=True).clone()
    assert torch.equal(u_eager, env._calc_MPC_action(0, 0, 0, 30))       # plan == one-shot
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env._calc_MPC_action(0, 0, 0, 30, use_plan=True)        # (first call on a side stream outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        u_cap = env._calc_MPC_action(0, 0, 0, 30, use_plan=True)
    for _ in range(6):
        u_cap.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(u_cap, u_eager)
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(lib.F16HipError):
        with torch.cuda.graph(g2):
            env._calc_MPC_action(0, 0, 0, 30)
    torch.cuda.synchronize()
    assert torch.equal(env._calc_MPC_action(0, 0, 0, 30), u_eager)       # the context is still usable afterwards


def _g8b_env(g, xcg, B=4):
    x = np.tile(g[f"x_full_xcg{xcg}"], (B, 1))
    env = make_env(x, xcg=xcg / 100)
    env.ssr = tuple(soa(np.tile(g[f"{k}_xcg{xcg}"], (B, 1, 1))) for k in ("Ad", "Bd", "Cd"))
    return env


def _g8b_weights(g, tag):
    return dict(Q=g[f"Q{tag}"], R=g[f"R{tag}"], x_lb=g[f"xlb_{tag}"], x_ub=g[f"xub_{tag}"], u_lb=g[f"ulb_{tag}"], u_ub=g[f"uub_{tag}"],
                udot_lb=g[f"rlb_{tag}"], udot_ub=g[f"rub_{tag}"])


@pytest.mark.parametrize("xcg", [25, 35])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_g8b_qp_build_with_weights_reference_and_bounds_as_arguments(xcg, tag):
    """utils.py:21 `setup_OSQP(x_ref, A, B, Q, R, hzn, dt, x, act_states, x_lb, ...)` takes weights, reference and bounds as
    ARGUMENTS; env.py fills them with constants, and so did this library until round 4.  G8b = the reference's setup_OSQP run by
    tools/make_golden.py --g12 with (a) the weights its author left commented out at env.py:391-403 and R = 0.01 I, (b) dense SPD
    Q / R, a free reference and other boxes.  The device build (f16_mpc_qp_debug_w through F16Batch.setup_OSQP) reproduces P, q,
    A, l, u; with no arguments it is bit for bit the plain entry point; utils.py:219 dlqr with the same weights too."""
    g = golden("g8b_mpc_qp_weights.npz")
    env = _g8b_env(g, xcg)
    w = _g8b_weights(g, tag)
    xref = np.tile(g[f"xref_{tag}_xcg{xcg}"], (env.B, 1))
    for N in (4, 10, 30):
        P, q, A, l, u = env.setup_OSQP(0.0, 0.0, 0.0, N, b=2, weights=w, x_ref=xref)
        t = f"{tag}_xcg{xcg}_N{N}"
        assert np.abs(P - g[f"P_{t}"]).max() / np.abs(g[f"P_{t}"]).max() < 1e-9
        assert np.abs(q - g[f"q_{t}"]).max() / np.abs(g[f"q_{t}"]).max() < 1e-7
        for got, ref in ((l, g[f"l_{t}"]), (u, g[f"u_{t}"])):
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(got), fin)
            np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-12, atol=1e-12)
        if N < 30:
            np.testing.assert_allclose(A, g[f"A_{t}"], rtol=1e-12, atol=1e-18)
    # defaults through the new entry point == the plain one, bit for bit
    for got, ref in zip(env.setup_OSQP(0.1, -0.05, 0.02, 10, b=1, weights=dict(R=np.eye(3))), env.setup_OSQP(0.1, -0.05, 0.02, 10, b=1)):
        assert np.array_equal(got, ref)
    Kt = torch.empty((27, env.B), dtype=torch.float64, device=env.device)
    st = torch.zeros(env.B, dtype=torch.int32, device=env.device)
    from f16_mpc_oop_py_amd import lib as L
    from f16_mpc_oop_py_amd.env import _vp
    ww = L.make_weights(Q=w["Q"], R=w["R"])
    Ad, Bd, Cd = env.ssr
    L.check(env.lib.f16_lqr_batch_w(env.ctx.handle, _vp(Ad), _vp(Bd), _vp(Cd), ctypes.byref(ww), _vp(Kt), None, _vp(st), env.B, env.B,
                                    env._stream))
    Kd = -Kt.t().reshape(env.B, 3, 9)[0].cpu().numpy()       # the library returns K = -dlqr (env.py:356)
    Kref = g[f"K_{tag}_xcg{xcg}"]
    assert np.abs(Kd - Kref).max() / np.abs(Kref).max() < 1e-8          # (entries span seven decades: relative to the gain's scale)
    assert int(st.max()) == 0


@pytest.mark.parametrize("tag", ["a", "b"])
def test_solves_with_weights_as_arguments_follow_the_cpu_twin_and_reach_the_minimiser(tag):
    """The solvers with the caller's weights / reference / bound values (the pattern of bounded rows stays the reference's): same
    QP as the reference builds (G8b), the solve iterate for iterate with the numpy twin of the same rules, the first move inside
    the solver band of the KKT-verified exact minimiser; one-shot call == prepared plan; N = 10 and 30 (wavefront solver),
    36 (long-horizon solver); a pattern the solvers do not keep is refused."""
    from f16_mpc_oop_py_amd import lib as L
    g = golden("g8b_mpc_qp_weights.npz")
    xcg = 35
    env = _g8b_env(g, xcg)
    w = _g8b_weights(g, tag)
    xref = np.tile(g[f"xref_{tag}_xcg{xcg}"], (env.B, 1))
    for N in (10, 30):
        t = f"{tag}_xcg{xcg}_N{N}"
        P, q, l, u = (g[f"{k}_{t}"] for k in ("P", "q", "l", "u"))
        A = g[f"A_{t}"] if N < 30 else env.setup_OSQP(0, 0, 0, N, weights=w, x_ref=xref)[2]
        uu, info = env._calc_MPC_action(0.0, 0.0, 0.0, N, return_info=True, weights=w, x_ref=xref)
        ref = mo.admm_osqp(P, q, A, l, u, drop_unbounded_rows=True)
        assert int(info["status"].max()) == 0 and int(info["iters"][0]) == ref["iters"]
        assert np.abs(info["u_seq"][0].cpu().numpy() - ref["x"]).max() < 1e-7
        # tight tolerances -> the KKT-verified exact minimiser of the reference-built QP (OSQP's default band is wide on these
        # weakly regularised costs: R = 0.01 I)
        xs, lam = mo.qp_exact(P, q, A, l, u)
        ut, it_ = env._calc_MPC_action(0.0, 0.0, 0.0, N, return_info=True, weights=w, x_ref=xref,
                                       settings=dict(eps_abs=1e-9, eps_rel=1e-9, max_iter=400000))
        assert int(it_["status"].max()) == 0 and np.abs(it_["u_seq"][0].cpu().numpy() - xs).max() < 1e-5 * max(1.0, np.abs(xs).max())
        env.prepare_MPC(N, weights=w)
        up = env._calc_MPC_action(0.0, 0.0, 0.0, N, use_plan=True, x_ref=xref)
        assert torch.equal(up, uu)
    uu36, info36 = env._calc_MPC_action(0.0, 0.0, 0.0, 36, return_info=True, weights=w, x_ref=xref)
    P, q, A, l, u = env.setup_OSQP(0, 0, 0, 36, weights=w, x_ref=xref)
    ref = mo.admm_osqp(P, q, A, l, u, drop_unbounded_rows=True)
    assert int(info36["iters"][0]) == ref["iters"] and np.abs(info36["u_seq"][0].cpu().numpy() - ref["x"]).max() < 1e-7
    bad = dict(w, x_lb=np.where(np.arange(9) == 0, -1.0, w["x_lb"]))       # a bound on phi: not a row the solvers carry
    with pytest.raises(L.F16HipError):
        env._calc_MPC_action(0.0, 0.0, 0.0, 10, weights=bad)
    env.setup_OSQP(0.0, 0.0, 0.0, 10, weights=bad)                        # ... the QP alone: any pattern


def test_weights_argument_validation_and_defaults():
    """f16_mpc_weights: the default struct IS env.py's constants (the `_w` entry points with it are bit for bit the plain ones, the
    LQR gain included); Q must be finite and symmetric, R symmetric positive definite, every box lb <= ub with a finite side, and
    the pattern of bounded state rows is the reference's -- anything else is F16_EINVAL, not a silently different problem."""
    from f16_mpc_oop_py_amd import lib as L
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(96, seed=3)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    w = L.MPCWeights()
    env.lib.f16_mpc_default_weights(ctypes.byref(w))
    assert w.q_from_cd == 1 and list(w.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(w.u_lb) == [-25.0, -21.5, -30.0]
    assert list(w.x_lb)[2:7] == [-20.0, -30.0, -300.0, -100.0, -50.0] and w.x_lb[0] == -np.inf and w.x_ub[8] == 25.0
    u_plain = env._calc_MPC_action(0.02, -0.01, 0.0, 12)
    u_w = env._calc_MPC_action(0.02, -0.01, 0.0, 12, weights=dict(R=np.eye(3), u_lb=[-25.0, -21.5, -30.0]))
    assert torch.equal(u_plain, u_w)
    assert torch.equal(env._calc_LQR_gain(), env._calc_LQR_gain(R=np.eye(3)))
    Qc = (env.ssr[2].t()[0].reshape(9, 9).t() @ env.ssr[2].t()[0].reshape(9, 9)).cpu().numpy()      # Cd'Cd of aircraft 0
    Kq = env._calc_LQR_gain(Q=Qc)[0]
    assert torch.allclose(Kq, env._calc_LQR_gain()[0], rtol=1e-9, atol=1e-12)
    bad = [dict(Q=np.triu(np.ones((9, 9)))), dict(Q=np.full((9, 9), np.nan)), dict(R=-np.eye(3)), dict(R=np.array([[1, 2, 0], [0, 1, 0], [0, 0, 1.0]])),
           dict(u_lb=[30.0, 0, 0]), dict(udot_lb=[-np.inf] * 3, udot_ub=[np.inf] * 3), dict(x_ub=[np.inf] * 9, x_lb=[-np.inf] * 9),
           dict(x_lb=[-1.0] + [-np.inf] * 8)]
    for kw in bad:
        with pytest.raises(L.F16HipError):
            env._calc_MPC_action(0.0, 0.0, 0.0, 8, weights=kw)
    # one-sided boxes are fine (OSQP's infinity on the other side): same solve as a box far away
    u1 = env._calc_MPC_action(0.0, 0.0, 0.0, 8, weights=dict(u_ub=[np.inf] * 3))
    u2 = env._calc_MPC_action(0.0, 0.0, 0.0, 8, weights=dict(u_ub=[1e30] * 3))
    assert torch.equal(u1, u2) and torch.isfinite(u1).all()


def test_dispatch_orders_do_not_change_results():
    """Scheduling only: the same batch with no ordering, with the first-call order (by ||q||_inf), with the order of a previous
    call, and with the hardware's distribution of workgroups instead of the kernel's own work queue returns the same commands,
    iteration counts and status words, bit for bit.  Fresh processes (the switch is read per call,
    the history lives in the context)."""
    import subprocess
    import sys
    import textwrap
    code = textwrap.dedent("""
        import sys, numpy as np, torch
        from f16_mpc_oop_py_amd import F16Batch
        from f16_mpc_oop_py_amd.workload import config4_states
        x0, u0 = config4_states(2048, seed=11)
        env = F16Batch(x0, u0, xcg=0.35)
        env.build_ssr()
        out = []
        for _ in range(2):
            u, info = env._calc_MPC_action(0.0, 0.0, 0.0, 30, return_info=True)
            out.append((u.cpu().numpy(), info["iters"].cpu().numpy(), info["status"].cpu().numpy()))
        assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1]))
        np.savez(sys.argv[1], u=out[0][0], it=out[0][1], st=out[0][2])
    """)
    import tempfile
    res = []
    with tempfile.TemporaryDirectory() as d:
        for mode, queue in (("0", "1"), ("first", "1"), ("1", "1"), ("1", "0")):      # queue = 0: one workgroup per aircraft, dealt by the hardware
            f = os.path.join(d, f"o_{mode}_{queue}.npz")
            r = subprocess.run([sys.executable, "-c", code, f],
                               env=dict(os.environ, PYTHONPATH=REPO, F16_MPC_DISPATCH_ORDER=mode, F16_MPC_WAVE_QUEUE=queue),
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            res.append(np.load(f))
    for k in ("u", "it", "st"):
        for other in res[1:]:
            assert np.array_equal(res[0][k], other[k], equal_nan=True), k
    assert res[0]["it"].min() >= 25 and res[0]["it"].max() > res[0]["it"].min()


def test_work_queue_batches_equal_small_batches_bit_for_bit():
    """Batches above 4 x the CU count run the wavefront solver as one workgroup per SIMD with a work queue, smaller ones as one
    workgroup per aircraft: an aircraft's answer does not depend on which -- 1100 aircraft (a last, partial round of the queue), their
    first 64 and their last 36 on their own, commands, iteration counts, residuals and status words bit for bit; twice (the second
    call is ordered by the first one's history)."""
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(1100, seed=23)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    outs = []
    for _ in range(2):
        u, info = env._calc_MPC_action(0.01, -0.02, 0.0, 30, return_info=True)
        outs.append((u.clone(), info["iters"].clone(), info["r_prim"].clone(), info["r_dual"].clone(), info["status"].clone()))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    for sl in (slice(0, 64), slice(1064, 1100)):
        es = make_env(x0[sl], u0[sl], xcg=0.35)
        es.build_ssr()
        u, info = es._calc_MPC_action(0.01, -0.02, 0.0, 30, return_info=True)
        assert torch.equal(u, outs[0][0][sl]) and torch.equal(info["iters"], outs[0][1][sl])
        assert torch.equal(info["r_prim"], outs[0][2][sl]) and torch.equal(info["r_dual"], outs[0][3][sl]) and torch.equal(info["status"], outs[0][4][sl])


def test_more_batch_sizes_than_history_slots_on_one_context():
    """The dispatch-order history has F16_MAX_SCHED = 16 slots per context ((stream, batch size) pairs): a 17th pair recycles the oldest
    slot instead of running unordered for ever; results never depend on it."""
    from f16_mpc_oop_py_amd import lib
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(64, seed=17)
    ctx = lib.Context(0)
    ref = {}
    for rnd in range(2):
        for B in range(20, 44):                                 # 24 batch sizes, twice round
            env = make_env(x0[:B], u0[:B], xcg=0.35, context=ctx)
            env.build_ssr()
            u = env._calc_MPC_action(0.0, 0.0, 0.0, 6).cpu().numpy()
            if rnd == 0:
                ref[B] = u
            else:
                assert np.array_equal(u, ref[B], equal_nan=True)
    fresh = make_env(x0[:20], u0[:20], xcg=0.35)
    fresh.build_ssr()
    assert np.array_equal(fresh._calc_MPC_action(0.0, 0.0, 0.0, 6).cpu().numpy(), ref[20], equal_nan=True)


def test_first_solve_of_a_wide_plan_inside_a_capture():
    """Plans accept horizons 33..40 (every solve runs the long-horizon workgroup solver) and plan solves are capturable: the
    kernel's dynamic-LDS opt-in (hipFuncSetAttribute, not legal under capture) must therefore have happened in
    f16_mpc_plan_create.  Fresh process, so that no earlier call has set the attribute: the FIRST solve of an N = 36 plan is
    captured, replayed, and compared with the eager solve."""
    import subprocess
    import sys
    import textwrap
    code = textwrap.dedent("""
        import torch
        from f16_mpc_oop_py_amd import F16Batch
        from f16_mpc_oop_py_amd.workload import config4_states
        x0, u0 = config4_states(48, seed=9)
        env = F16Batch(x0, u0, xcg=0.35)
        env.build_ssr()
        env.prepare_MPC(36)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            u_cap = env._calc_MPC_action(0, 0, 0, 36, use_plan=True)
        for _ in range(3):
            u_cap.zero_()
            g.replay()
            torch.cuda.synchronize()
            u1 = u_cap.clone()
        u_eager = env._calc_MPC_action(0, 0, 0, 36, use_plan=True)
        torch.cuda.synchronize()
        assert torch.isfinite(u_eager).all() and torch.equal(u1, u_eager), (u1 - u_eager).abs().max()
        print("captured-first-solve ok")
    """)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "captured-first-solve ok" in r.stdout, r.stderr[-3000:]


@pytest.mark.parametrize("mode", ["osqp", "builder"])
def test_horizons_beyond_the_on_chip_solvers_vs_same_algorithm_oracle(mode):
    """Horizons 41..150 (the reference sweeps N = 1..150, env.py:426-436) run through the slow path of the generic
    solver (per-row values and the packed KKT inverse in the per-aircraft HBM workspace): the QP it builds equals the
    restated setup_OSQP, and the solve follows the CPU twin iterate for iterate (same iteration count, u_seq to 1e-8)."""
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(3, seed=21)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    Ad, Bd, Cd = _model_np(env)
    dem = (0.02, -0.01, 0.01)
    for N in (41, 57, 150):
        u, info = env._calc_MPC_action(*dem, N, settings=mode_settings(mode), return_info=True)
        torch.cuda.synchronize()
        st = info["status"].cpu().numpy()
        assert set(np.unique(st)) <= {0, 128} and tuple(info["u_seq"].shape) == (3, 3 * N)
        b = 1
        Pd, qd, Ad_, ld_, ud_ = env.setup_OSQP(*dem, N, b=b)
        P, q, A, l, uu = mo.mpc_qp(x0[b], Ad[b], Bd[b], Cd[b], N, 0.001, *dem)
        assert np.abs(Pd - P).max() <= 1e-10 * np.abs(P).max() and np.abs(qd.ravel() - q.ravel()).max() <= 1e-10 * np.abs(q).max()
        assert np.array_equal(Ad_ != 0, A != 0) and np.abs(Ad_ - A).max() <= 1e-12 * np.abs(A).max()
        fin = np.isfinite(l)
        assert np.array_equal(np.isfinite(ld_.ravel()), fin) and np.abs(ld_.ravel()[fin] - l[fin]).max() < 1e-9
        ref = MODES[mode][1](P, q, A, l, uu)
        assert int(info["iters"][b]) == ref["iters"], N
        assert bool(ref["infeasible"]) == (st[b] == 128), N
        if not ref["infeasible"]:
            assert np.abs(info["u_seq"][b].cpu().numpy() - ref["x"]).max() < 1e-8, N
            assert np.abs(u[b].cpu().numpy() - ref["x"][:3]).max() < 1e-8


@pytest.mark.parametrize("solver,mode,N,max_iter", [("k_mpc_fast<2>", "builder", 2, 25), ("k_mpc_wave", "osqp", 10, 25),
                                                    ("k_mpc_big", "builder", 33, 25), ("k_mpc<false>", "builder", 2, -25)])
def test_max_iter_branch_of_every_solver_vs_same_algorithm_oracle(solver, mode, N, max_iter):
    """The one branch of the stopping rules (csrc/f16_osqp_rules.hpp) that the horizon tests above leave to a single solver: the
    solve that ends at max_iter.  Each solver once, at its smallest horizon, with max_iter = the first termination test: on
    these eight aircraft the CPU twin converges AT that test for some (status 0: convergence is asked before the iteration
    limit) and not for the others (status 64, the last iterate handed back); the wavefront solver's QPs (OSQP's defaults,
    which need hundreds of iterations) all stop at the limit.  Iteration counts and status words equal the twin's, the input
    sequence to the 1e-6 of the horizon tests.  (A negative max_iter selects the generic solver.)"""
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(8, seed=21)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    Ad, Bd, Cd = _model_np(env)
    dem = (0.02, -0.01, 0.01)
    u, info = env._calc_MPC_action(*dem, N, settings=mode_settings(mode, max_iter=max_iter), return_info=True)
    torch.cuda.synchronize()
    st, it = info["status"].cpu().numpy(), info["iters"].cpu().numpy()
    hit = 0
    for b in range(8):
        P, q, A, l, uu = mo.mpc_qp(x0[b], Ad[b], Bd[b], Cd[b], N, 0.001, *dem)
        ref = MODES[mode][1](P, q, A, l, uu, max_iter=abs(max_iter))
        assert not ref["infeasible"]
        assert int(it[b]) == ref["iters"], (solver, b)
        assert int(st[b]) == (0 if ref["converged"] else 64), (solver, b, int(st[b]))
        assert np.abs(info["u_seq"][b].cpu().numpy() - ref["x"]).max() < 1e-6, (solver, b)
        assert np.abs(u[b].cpu().numpy() - ref["x"][:3]).max() < 1e-6, (solver, b)
        hit += not ref["converged"]
    assert hit >= 2                                             # the case does reach the branch


def test_constraint_checking_horizon_sweep_surface(tmp_path):
    """F16._calc_constr_checking_hzn (env.py:426-436): first moves for N = 1..max_hzn, here for a batch, as ONE library call
    (f16_mpc_hzn_sweep: the long horizons solved by a single launch over every (horizon, aircraft) pair, taken from a work
    queue).  Every slice equals the direct call at that horizon bit for bit -- commands, iteration counts, residuals, rho, status
    words -- whatever the order the pairs were solved in, and also when the workspace budget cuts the sweep into groups of horizons
    (F16_SWEEP_WS_GB, read once per process: a child process)."""
    import os
    import subprocess
    import sys
    from conftest import REPO
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(5, seed=9)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    sw, inf = env._calc_constr_checking_hzn(max_hzn=58, return_info=True)
    assert tuple(sw.shape) == (5, 3, 58)
    for N in (1, 10, 30, 31, 32, 33, 34, 41, 42, 57, 58):
        u, i1 = env._calc_MPC_action(0, 0, 0, N, return_info=True)
        assert torch.equal(torch.nan_to_num(sw[:, :, N - 1], nan=1e300), torch.nan_to_num(u, nan=1e300)), N
        for k in ("iters", "r_prim", "r_dual", "rho"):
            assert torch.equal(inf[k][N - 1], i1[k]), (N, k)
        assert torch.equal(inf["status"][N - 1], i1["status"]), N
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, %r)
from f16_mpc_oop_py_amd import F16Batch
from f16_mpc_oop_py_amd.workload import config4_states
x0, u0 = config4_states(5, seed=9)
env = F16Batch(x0, u0, xcg=0.35)
env.build_ssr()
sw, inf = env._calc_constr_checking_hzn(max_hzn=58, return_info=True)
np.savez(sys.argv[1], u=sw.cpu().numpy(), iters=inf["iters"].cpu().numpy(), status=inf["status"].cpu().numpy())
''' % REPO
    # a repeated sweep takes its pairs in another order (costliest first by the first one's iteration counts): same results
    sw_b, inf_b = env._calc_constr_checking_hzn(max_hzn=58, return_info=True)
    assert torch.equal(torch.nan_to_num(sw, nan=1e300), torch.nan_to_num(sw_b, nan=1e300))
    assert torch.equal(inf["iters"], inf_b["iters"]) and torch.equal(inf["status"], inf_b["status"])
    # other settings go through the same call: the opt-in rule (no equilibration, automatic rho) and the generic one-wave kernels
    for st in (dict(scaling=0, rho=0.0), dict(max_iter=-40000)):
        sw2, inf2 = env._calc_constr_checking_hzn(max_hzn=36, settings=st, return_info=True)
        for N in (1, 30, 33, 36):
            u, i1 = env._calc_MPC_action(0, 0, 0, N, settings=st, return_info=True)
            assert torch.equal(torch.nan_to_num(sw2[:, :, N - 1], nan=1e300), torch.nan_to_num(u, nan=1e300)), (st, N)
            assert torch.equal(inf2["iters"][N - 1], i1["iters"]) and torch.equal(inf2["status"][N - 1], i1["status"]), (st, N)
    f = str(tmp_path / "groups.npz")
    r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, F16_SWEEP_WS_GB="0.002"), capture_output=True, text=True,
                       timeout=600)          # 2 MB: a group per horizon or two (N = 58: 0.46 MB per aircraft)
    assert r.returncode == 0, r.stderr[-2000:]
    g = np.load(f)
    assert np.array_equal(g["u"], sw.cpu().numpy(), equal_nan=True)
    assert np.array_equal(g["iters"], inf["iters"].cpu().numpy()) and np.array_equal(g["status"], inf["status"].cpu().numpy())


def test_one_table_of_qp_settings_through_the_one_shot_call_the_plan_and_the_sweep():
    """The QP settings are checked by one rule (mpc_check_settings) behind the three calls that take them: the one-shot call
    (f16_mpc_batch_w), prepare_MPC (f16_mpc_plan_create_w) and the horizon sweep (f16_mpc_hzn_sweep; horizons 1..3: its one-shot
    part).  One table through all three: what is refused is refused everywhere with the library's error, what is accepted runs
    everywhere, and max_iter <= 0 (negative: the generic kernel) is the one setting on which they differ -- a plan needs
    iterations.  A refusal leaves nothing behind: the default call on the same environment returns finite commands after each."""
    from f16_mpc_oop_py_amd import lib
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(2, seed=9)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    dem, N = (0.01, 0.0, -0.01), 4

    def plan(st):
        env.prepare_MPC(N, settings=st)
        return env._calc_MPC_action(*dem, N, use_plan=True)

    calls = {"one_shot": lambda st: env._calc_MPC_action(*dem, N, settings=st), "plan": plan,
             "sweep": lambda st: env._calc_constr_checking_hzn(max_hzn=3, settings=st)}
    refused = [dict(check_every=0), dict(rho_every=0), dict(rho=-1.0), dict(rho=float("nan")), dict(sigma=0.0), dict(scaling=-1),
               dict(scaling=101), dict(scaling=10, rho=0.0), dict(adaptive_rho=1, rho_every=30, check_every=25)]
    accepted = [dict(adaptive_rho=0, rho_every=30, check_every=25), dict(scaling=0, rho=0.0)]
    no_iterations = [dict(max_iter=-50), dict(max_iter=0)]
    for name, call in calls.items():
        for st in refused + (no_iterations if name == "plan" else []):
            with pytest.raises(lib.F16HipError):
                call(st)
            assert bool(torch.isfinite(call(None)).all()), (name, st)
        for st in accepted + (no_iterations if name != "plan" else []):
            call(st)
            torch.cuda.synchronize()


def test_wavefront_solver_vs_the_512_lane_solver_and_its_equilibration(tmp_path):
    """The one-wavefront-per-aircraft solver (k_mpc_wave, the default for equilibrated solves up to N = 30) against the
    512-lane solver (F16_MPC_WAVE=0) on the same QPs: same iteration counts, status words and final rho, input sequences to
    2e-7 (observed: 1.4e-8 on sequences of magnitude 25, after up to 40,000 iterations) -- the two follow the same rules in
    different summation orders.  Also with the equilibration done by the 512-lane
    kernel instead of the wavefront itself (F16_WAVE_RUIZ=0): the wavefront's own Ruiz passes must give the same D, E, c."""
    import json
    import os
    import subprocess
    import sys
    from conftest import REPO
    code = r'''
import json, sys, numpy as np, torch
sys.path.insert(0, %r)
from f16_mpc_oop_py_amd import F16Batch
from f16_mpc_oop_py_amd.workload import config4_states, config2_states
out = {}
for name, (x0, u0) in (("c4", config4_states(384)), ("c2", config2_states(192, seed=4))):
    env = F16Batch(x0, u0, xcg=0.35)
    env.build_ssr()
    for N in (30, 29, 17, 6, 1):
        for st in (None, dict(rho_every=25), dict(adaptive_rho=0, max_iter=300)):
            u, info = env._calc_MPC_action(0.02, -0.01, 0.0, N, settings=st, return_info=True)
            out[f"{name}_{N}_{json.dumps(st)}"] = dict(it=info["iters"].cpu().numpy().tolist(), st=info["status"].cpu().numpy().tolist(),
                                                      rho=info["rho"].cpu().numpy().tolist(), us=info["u_seq"].cpu().numpy().tolist())
json.dump(out, open(sys.argv[1], "w"))
''' % REPO
    res = {}
    for tag, extra in (("wave", {}), ("fast", {"F16_MPC_WAVE": "0"}), ("wave_ruiz_outside", {"F16_WAVE_RUIZ": "0"})):
        f = tmp_path / (tag + ".json")
        r = subprocess.run([sys.executable, "-c", code, str(f)], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        res[tag] = json.load(open(f))
    for key, w in res["wave"].items():
        for other in ("fast", "wave_ruiz_outside"):
            o = res[other][key]
            assert w["it"] == o["it"] and w["st"] == o["st"], (key, other)
            us_w, us_o = np.array(w["us"], dtype=float), np.array(o["us"], dtype=float)
            assert np.array_equal(np.isnan(us_w), np.isnan(us_o)), (key, other)
            assert np.nanmax(np.abs(us_w - us_o), initial=0.0) < 2e-7, (key, other, np.nanmax(np.abs(us_w - us_o)))
            assert np.allclose(w["rho"], o["rho"], rtol=1e-6, atol=0), (key, other)


# ---------------------------------------------------------------------------------------------------------------- round 5
def _host_loop(env, steps, N, dem, hold=False):
    """dist.closed_loop_mpc_rollout's loop, step by step, keeping what every step returned (the checker of f16_rollout_mpc)."""
    from f16_mpc_oop_py_amd import lib as L
    env.flags |= L.F16_FLAG_ONE_LANE                   # the step of the fused kernel = the one-lane rollout kernel's
    cmds, its, trs = [], [], []
    for _ in range(steps):
        cmd, info = env._calc_MPC_action(*dem, N, return_info=True, use_plan=True)
        cmds.append(cmd.t().clone()); its.append(info["iters"].to(torch.int32).clone())
        c = cmd.t()
        env._u[1:4] = torch.where(torch.isnan(c), env._u[1:4], c) if hold else c
        env.rollout(1)
        trs.append(env._x.clone())
    return torch.stack(trs), torch.stack(cmds), torch.stack(its)


def _same(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.timeout(300, method="thread")      # (a persistent kernel that never drains must fail the run, not hold it)
@pytest.mark.parametrize("B,N,steps", [(256, 30, 8), (100, 10, 12), (1, 30, 5), (3, 4, 40), (1500, 29, 3), (1100, 10, 30)])
def test_fused_closed_loop_mpc_rollout_equals_the_host_loop_bit_for_bit(oracle, B, N, steps):
    """f16_rollout_mpc (the reference's loop test_env.py:480-495 as ONE launch: (step, aircraft) pairs from a work queue, a wavefront
    builds the QP vectors, solves, writes the command and steps its pair) against the host loop of six launches per step: every
    command, every iteration count, every trajectory sample, the final state, u.values and the status words are IDENTICAL; and
    against the same loop on the CPU twin for a sample (commands <= 1e-4, states <= 1e-6: the bands of the host-loop test)."""
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(B, seed=11)
    dem = (0.02, -0.01, 0.005)
    envh = make_env(x0, u0, xcg=0.35)
    envh.build_ssr(); envh.prepare_MPC(N)
    trh, ch, ih = _host_loop(envh, steps, N, dem)
    envf = make_env(x0, u0, xcg=0.35)
    envf.build_ssr(); envf.prepare_MPC(N)
    trf, info = envf.rollout_MPC(steps, *dem, N, traj_every=1, return_info=True)
    assert _same(info["cmd"], ch) and _same(info["iters"], ih) and _same(trf, trh)
    assert _same(envf._x, envh._x) and _same(envf._u, envh._u) and _same(envf.status, envh.status)
    assert int(envf.status.max()) == 0 and int(info["iters"].min()) >= 25
    Ad, Bd, Cd = _model_np(envf)
    idx = sorted(set([0, B // 3, B - 1]))
    r = oracle.mpc_closed_loop(x0[idx], u0[idx], Ad[idx], Bd[idx], Cd[idx], N, steps, dem, nthreads=4)
    assert np.array_equal(r["iters"], info["iters"].cpu().numpy()[:, idx])
    assert np.abs(r["cmd"] - info["cmd"].permute(0, 2, 1).cpu().numpy()[:, idx]).max() < 1e-4
    xg = envf.x_values.cpu().numpy()[idx]
    assert np.max(np.abs(xg - r["x"]) / np.maximum(1.0, np.abs(r["x"]))) < 1e-6
    # a second call goes on from where the first one stopped (counters of the plan are re-armed per call); samples every 2nd step
    tr2 = envf.rollout_MPC(4, *dem, N, traj_every=2)
    _host_loop(envh, 4, N, dem)
    assert tuple(tr2.shape) == (2, 18, B) and _same(envf._x, envh._x) and _same(tr2[-1], envf._x)


@pytest.mark.timeout(300, method="thread")      # (a persistent kernel that never drains must fail the run, not hold it)
def test_fused_closed_loop_flagged_aircraft_nan_commands_hold_and_frozen(oracle):
    """What a flagged aircraft does next, fused kernel = host loop = CPU loop (oracle/f16_mpc_oracle.c: f16o_mpc_closed_loop):
    an INFEASIBLE QP returns a NaN command as OSQP does (env.py:420-424); the actuator models propagate it (np.clip,
    utils.py:308-330: fixture G3b), the surface states turn NaN and every later solve of that aircraft is skipped (NaN, zero
    iterations) -- status bits QP_INFEASIBLE | NONFINITE are sticky; with F16_FLAG_HOLD_COMMAND the previous command is kept and
    the aircraft flies on; an aircraft outside its envelope is frozen and not solved for."""
    from f16_mpc_oop_py_amd.workload import config2_states
    B, N, steps = 320, 10, 6
    x0, u0 = config2_states(B, seed=3)                      # (config 2's flap states sit ON their bounds: some QPs are infeasible)
    x0[5, 13] = 26.0                                        # elevator outside its box: env.py:117-124 would exit()
    dem = (0.0, 0.0, 0.0)
    out = {}
    for hold in (False, True):
        envh = make_env(x0, u0, xcg=0.35)
        envh.build_ssr(); envh.prepare_MPC(N)
        trh, ch, ih = _host_loop(envh, steps, N, dem, hold=hold)
        envf = make_env(x0, u0, xcg=0.35)
        envf.build_ssr(); envf.prepare_MPC(N)
        trf, info = envf.rollout_MPC(steps, *dem, N, traj_every=1, return_info=True, hold_command=hold)
        live = np.ones(B, bool); live[5] = False            # (the host loop goes on solving for the frozen aircraft)
        lv = torch.as_tensor(live, device="cuda:0")
        assert _same(info["cmd"][:, :, lv], ch[:, :, lv]) and _same(info["iters"][:, lv], ih[:, lv]) and _same(trf, trh)
        assert _same(envf._x, envh._x) and _same(envf._u[:, lv], envh._u[:, lv])
        sf, sh = envf.status.cpu().numpy(), envh.status.cpu().numpy()
        assert np.array_equal(sf[live], sh[live])
        assert sf[5] == 16 | (1 << (8 + 13)) and np.isnan(info["cmd"][:, :, 5].cpu().numpy()).all() and int(info["iters"][:, 5].max()) == 0
        assert np.array_equal(envf.x_values.cpu().numpy()[5], x0[5]) and np.array_equal(envf.u_values.cpu().numpy()[5], u0[5])
        Ad, Bd, Cd = _model_np(envf)
        r = oracle.mpc_closed_loop(x0, u0, Ad, Bd, Cd, N, steps, dem, hold=hold, nthreads=16)
        assert np.array_equal(r["status"] & (16 | 32 | 64 | 128), sf & (16 | 32 | 64 | 128))
        assert np.array_equal(r["iters"], info["iters"].cpu().numpy())
        cg = info["cmd"].permute(0, 2, 1).cpu().numpy()
        assert np.array_equal(np.isnan(cg), np.isnan(r["cmd"]))
        fin = ~np.isnan(cg)
        assert np.abs(cg[fin] - r["cmd"][fin]).max() < 1e-4
        xg = envf.x_values.cpu().numpy()
        assert np.array_equal(np.isnan(xg), np.isnan(r["x"]))
        out[hold] = (sf, xg, info["iters"].cpu().numpy(), cg)
    sf, xg, it, cg = out[False]
    inf = (sf & 128) != 0
    assert 3 <= inf.sum() < B // 2                          # the workload does contain infeasible QPs
    first = np.array([np.argmax(np.isnan(cg[:, b, 0])) for b in np.where(inf)[0]])
    for b, t0 in zip(np.where(inf)[0], first):
        assert sf[b] & 32 and np.isnan(xg[b, 13:16]).all()                            # NaN command -> NaN surface states
        assert (it[t0 + 1:, b] == 0).all() and np.isnan(cg[t0:, b]).all()              # ... and no QP to solve from then on
    sfh, xgh, ith, cgh = out[True]
    assert np.array_equal((sfh & 128) != 0, inf) or ((sfh & 128) != 0).sum() >= inf.sum()
    assert np.isfinite(np.delete(xgh, 5, 0)).all() and not (np.delete(sfh, 5) & 32).any()   # held commands: everybody flies on


@pytest.mark.timeout(300, method="thread")
def test_fused_closed_loop_with_the_opt_in_warm_start():
    """f16_mpc_plan_warm_start (OSQP's in-object default; the reference starts cold) inside the one-launch loop: step t starts from the
    solution of step t - 1, handed from wavefront to wavefront with the state -- identical to the host loop on a warm-started plan,
    fewer iterations than the cold loop, and a second call goes on from the first one's last solution."""
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N, steps = 300, 30, 8
    x0, u0 = config4_states(B, seed=13)
    dem = (0.02, 0.0, -0.01)
    envh = make_env(x0, u0, xcg=0.35)
    envh.build_ssr(); envh.prepare_MPC(N, warm_start=True)
    trh, ch, ih = _host_loop(envh, steps, N, dem)
    envf = make_env(x0, u0, xcg=0.35)
    envf.build_ssr(); envf.prepare_MPC(N, warm_start=True)
    trf, info = envf.rollout_MPC(steps, *dem, N, traj_every=1, return_info=True)
    assert _same(info["cmd"], ch) and _same(info["iters"], ih) and _same(trf, trh) and _same(envf.status, envh.status)
    assert float(info["iters"][1:].float().mean()) < 0.7 * float(info["iters"][0].float().mean())       # warm solves are shorter
    trh2, ch2, ih2 = _host_loop(envh, 3, N, dem)
    _, info2 = envf.rollout_MPC(3, *dem, N, return_info=True)
    assert _same(info2["cmd"], ch2) and _same(info2["iters"], ih2) and _same(envf._x, envh._x)


@pytest.mark.timeout(300, method="thread")      # (a persistent kernel that never drains must fail the run, not hold it)
def test_fused_closed_loop_lofi_model_and_horizon_one():
    """The one-launch loop on the lofi Stevens-Lewis model (fi_flag = 0: the out-of-line step takes the fidelity at run time) and at
    the shortest horizon, N = 1: identical to the host loop."""
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(64, seed=21)
    x0[:, 7] = np.clip(x0[:, 7], np.deg2rad(-8.0), np.deg2rad(40.0))       # the lofi tables cover alpha -10..45 deg
    for fi, N in ((0, 10), (1, 1)):
        dem = (0.01, 0.0, -0.01)
        envh = make_env(x0, u0, xcg=0.35, fi_flag=fi)
        envh.build_ssr(); envh.prepare_MPC(N)
        trh, ch, ih = _host_loop(envh, 6, N, dem)
        envf = make_env(x0, u0, xcg=0.35, fi_flag=fi)
        envf.build_ssr(); envf.prepare_MPC(N)
        trf, info = envf.rollout_MPC(6, *dem, N, traj_every=1, return_info=True)
        assert _same(info["cmd"], ch) and _same(info["iters"], ih) and _same(trf, trh) and _same(envf.status, envh.status)
        assert bool(torch.isfinite(trf).all())


@pytest.mark.timeout(300, method="thread")      # (a persistent kernel that never drains must fail the run, not hold it)
def test_fused_closed_loop_argument_checks():
    from f16_mpc_oop_py_amd import lib as L
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(8, seed=1)
    env = make_env(x0, u0, xcg=0.35)
    env.build_ssr()
    env.prepare_MPC(10, settings=dict(scaling=0, rho=0.0))           # no equilibration: not this kernel's solver
    with pytest.raises(L.F16HipError):
        env.rollout_MPC(2, 0, 0, 0, 10)
    env.prepare_MPC(10)
    before = env.x_values.clone()
    assert env.rollout_MPC(0, 0, 0, 0, 10) is None and bool((env.x_values == before).all())
    assert env.lib.f16_rollout_mpc(None, None, None, None, None, None, None, None, 1, 1, 0.35, 1, 0, None) == -1      # F16_EINVAL


@pytest.mark.timeout(300, method="thread")      # (a persistent kernel that never drains must fail the run, not hold it)
def test_config5_full_shard_through_both_loops_vs_the_cpu_chain(oracle):
    """A quarter of a config-5 shard (2,048 aircraft, N = 30, 10 closed-loop steps, reference settings, cold start) through the host
    loop AND through the one-launch loop -- identical bit for bit -- and against the same loop on the host cores (C twin with the
    device's own frozen models: oracle.mpc_closed_loop): the config-4 rule carried over T steps -- iteration counts and status words
    equal, commands <= 5e-5 where the counts agree (a count that differs by one test interval at a knife edge moves the command by
    the termination tolerance, and the aircraft's later steps with it: such aircraft are counted, not compared)."""
    from f16_mpc_oop_py_amd.workload import config4_states
    B, N, steps = 2048, 30, 10
    x0, u0 = config4_states(B)
    dem = (0.0, 0.0, 0.0)
    envh = make_env(x0, u0, xcg=0.35)
    envh.build_ssr(); envh.prepare_MPC(N)
    trh, ch, ih = _host_loop(envh, steps, N, dem)
    envf = make_env(x0, u0, xcg=0.35)
    envf.build_ssr(); envf.prepare_MPC(N)
    trf, info = envf.rollout_MPC(steps, *dem, N, traj_every=1, return_info=True)
    assert _same(info["cmd"], ch) and _same(info["iters"], ih) and _same(trf, trh) and _same(envf.status, envh.status)
    Ad, Bd, Cd = _model_np(envf)
    r = oracle.mpc_closed_loop(x0, u0, Ad, Bd, Cd, N, steps, dem, nthreads=len(os.sched_getaffinity(0)))
    ig, cg = info["iters"].cpu().numpy(), info["cmd"].permute(0, 2, 1).cpu().numpy()
    same = ig == r["iters"]                                             # [steps, B]
    agree = np.logical_and.accumulate(same, axis=0)                     # ... up to and including this step
    print("iteration counts equal: %.4f of %d solves; aircraft equal over all steps: %d of %d" % (same.mean(), same.size, agree[-1].sum(), B))
    assert agree[0].all()                                               # the first call = the config-4 test: every count
    assert agree[-1].mean() > 0.99
    fin = agree[:, :, None] & ~np.isnan(r["cmd"]) & ~np.isnan(cg)
    assert np.abs(cg - r["cmd"])[fin].max() < 5e-5
    assert np.array_equal(np.isnan(cg)[agree], np.isnan(r["cmd"])[agree])
    ok = agree[-1]
    sg = envf.status.cpu().numpy()
    assert np.array_equal(sg[ok] & (16 | 32 | 64 | 128), r["status"][ok] & (16 | 32 | 64 | 128))
    xg = envf.x_values.cpu().numpy()
    good = ok & np.isfinite(r["x"]).all(1)
    assert np.max(np.abs(xg[good] - r["x"][good]) / np.maximum(1.0, np.abs(r["x"][good]))) < 1e-6
