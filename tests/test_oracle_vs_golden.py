"""Pin the CPU oracle (oracle/f16_oracle.c, oracle/mpc_oracle.py) against fixtures produced by
RUNNING the reference (tools/make_golden.py: prebuilt C/nlplant_xcg{25,35}.so + the reference's
env.py/utils.py).  Tolerance: |d| <= 1e-12*max(1,|ref|) per SURVEY.md 8(d) (observed ~1e-15)."""
import numpy as np
import pytest

from conftest import golden
from oracle import mpc_oracle as mo

TOL = 1e-12


def rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


def test_g1_every_table_function(oracle):
    g = golden("g1_tables.npz")
    for tid in range(43):
        got = np.array([oracle.table(tid, *p) for p in g["pts"][tid]])
        if g["names"][tid] == "_CLr":
            # reference defect: table never loaded -> heap garbage (denormals); restated as 0
            assert np.all(np.abs(g["vals"][tid]) < 1e-300)
            assert np.all(got == 0.0)
            continue
        assert np.array_equal(got, g["vals"][tid]), g["names"][tid]   # bit-exact incl. nodes/edges


@pytest.mark.parametrize("name,fi", [("hifi", 1), ("lofi", 0)])
@pytest.mark.parametrize("xcg", [25, 35])
def test_g2_nlplant(oracle, name, fi, xcg):
    g = golden("g2_nlplant.npz")
    out = np.array([oracle.nlplant(x, fi, xcg / 100) for x in g[f"xu_{name}"]])
    assert rel(out, g[f"xdot_{name}_xcg{xcg}"]) < TOL


def test_g2_atmos(oracle):
    g = golden("g2_nlplant.npz")
    out = np.array([oracle.atmos(*p) for p in g["atmos_in"]])
    assert np.array_equal(out, g["atmos_out"])


def test_known_answers_from_survey(oracle):
    """SURVEY.md 8c sample values at parameters.py:105 x0."""
    g = golden("g2_nlplant.npz")
    x0 = g["xu_hifi"][0]
    np.testing.assert_allclose(oracle.nlplant(x0, 1, 0.25)[6:12],
                               [6.118049e-01, 2.059944e-03, -4.340897e-04, -8.778729e-05, 1.113977e-02, -2.893308e-04],
                               rtol=2e-6)
    np.testing.assert_allclose(oracle.nlplant(x0, 1, 0.35)[9:12], [-4.474235e-04, 4.079459e-01, -3.767035e-03], rtol=2e-6)
    np.testing.assert_allclose(oracle.nlplant(x0, 0, 0.25)[6:12],
                               [3.958124e-01, 1.824711e-03, -5.699302e-05, 8.328066e-02, -9.694392e-02, 9.918715e-03],
                               rtol=2e-6)


@pytest.mark.parametrize("xcg", [25, 35])
def test_g3_calc_xdot_and_na(oracle, xcg):
    g = golden("g3_calc_xdot.npz")
    out = oracle.xdot_batch(g["x"], g["u"], 1, xcg / 100)
    assert rel(out, g[f"xdot_xcg{xcg}"]) < TOL
    xf = g[f"na_x_full_xcg{xcg}"]
    out = np.array([oracle.calc_xdot_na(xf, a, b, 1, xcg / 100) for a, b in zip(g["na_x9"], g["na_u3"])])
    assert rel(out, g[f"xdot_na_xcg{xcg}"]) < TOL


@pytest.mark.parametrize("xcg", [25, 35])
def test_g3b_nan_and_infinite_commands_through_the_actuator_models(oracle, xcg):
    """np.clip (utils.py:303-330) propagates NaN: a NaN command (OSQP's answer to an infeasible QP, env.py:420-424) gives a NaN
    actuator derivative in the reference, never a hard-over; +-inf saturates.  Fixture G3b = the reference's `_calc_xdot` / `step`."""
    g = golden("g3b_nan_actuators.npz")
    x, u, ref = g[f"x_xcg{xcg}"], g[f"u_xcg{xcg}"], g[f"xdot_xcg{xcg}"]
    out = np.array([oracle.calc_xdot(a, b, 1, xcg / 100) for a, b in zip(x, u)])
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    assert np.isnan(ref).sum() == 1 + 1 + 1 + 1 + 3 + 2                      # (the cases of the fixture really carry NaN)
    fin = ~np.isnan(ref)
    assert rel(out[fin], ref[fin]) < TOL
    assert np.array_equal(out[5:7, 13:15][[0, 1], [0, 1]], [60.0, -80.0])    # +-inf commands saturate
    # one `step` from the reference's trim point under u[1] = NaN
    xt = oracle.rollout(golden("g567_trim_lin_lqr.npz")[f"trim_x_xcg{xcg}"][None], g[f"step_u_xcg{xcg}"][None], 1, xcg=xcg / 100, store=False)[0][0]
    refs = g[f"step1_xcg{xcg}"]
    assert np.isnan(xt[13]) and np.isnan(refs[13]) and np.isnan(xt).sum() == 1
    assert rel(np.delete(xt, 13), np.delete(refs, 13)) < 1e-10


@pytest.mark.parametrize("xcg", [25, 35])
def test_g13_linear_model_closed_loops(xcg):
    """The reference's LINEAR closed loops: test_env_mk2.py:46-62 (`LQR(linear=True)`, what main.py:35 runs: the frozen reduced model
    under `_calc_LQR_action`, 10,000 steps) and test_env.py:501-576 (`test_LQR_lin`: u = -K (x - x_ref)).  The first one grows like
    exp(14 t) (the spurious eigenvalue of the swapped flap derivatives) to 1e60: compared relative to the state norm."""
    g = golden("g13_linear_loops.npz")
    Ad, Bd, K, u0 = g[f"Ad_xcg{xcg}"], g[f"Bd_xcg{xcg}"], g[f"K_xcg{xcg}"], g[f"u0_xcg{xcg}"]
    for c in range(3):
        xr = np.zeros(9)
        xr[4:7] = g[f"dem_xcg{xcg}"][c]
        xs, us = mo.rollout_lqr_linear(g[f"x0_xcg{xcg}"][c], Ad, Bd, K, xr, u0, 10000, track=(4, 5, 6), every=100)
        rx, ru = g[f"xtraj_xcg{xcg}"][c], g[f"utraj_xcg{xcg}"][c]
        assert np.max(np.linalg.norm(xs - rx, axis=1) / np.linalg.norm(rx, axis=1)) < 1e-10
        assert np.max(np.linalg.norm(us - ru, axis=1) / np.maximum(1.0, np.linalg.norm(ru, axis=1))) < 1e-10
    assert np.abs(g[f"xtraj_xcg{xcg}"][0][-1]).max() > 1e50                    # (it does diverge: the reference's own behaviour)
    xs, us = mo.rollout_lqr_linear(g[f"lin_x0_xcg{xcg}"], g[f"lin_A_xcg{xcg}"], g[f"lin_B_xcg{xcg}"], -g[f"lin_K_xcg{xcg}"],
                                   g[f"lin_xref_xcg{xcg}"], np.zeros(3), 10000, every=100)
    assert rel(xs, g[f"lin_xtraj_xcg{xcg}"]) < 1e-9 and rel(us, g[f"lin_utraj_xcg{xcg}"]) < 1e-9
    # the model and the gain of test_env.py:509-545 themselves: the restated linearise -> ZOH -> dlqr(A, B, I, I)
    Kl = mo.dlqr(g[f"lin_A_xcg{xcg}"], g[f"lin_B_xcg{xcg}"], np.eye(9), np.eye(3))
    assert rel(Kl, g[f"lin_K_xcg{xcg}"]) < 1e-8


def test_g13_toy_double_integrator_of_test_LQR_lin():
    """test_env.py:528-541 (f16=False): the 2-state toy, here as a 9-state system padded with zeros -- the shape the device kernel has."""
    g = golden("g13_linear_loops.npz")
    A, B = np.zeros((9, 9)), np.zeros((9, 3))
    A[:2, :2] = [[1, 1.0], [0, 1]]
    B[1, 0] = 1.0
    K = np.zeros((3, 9))
    K[0, :2] = mo.dlqr(A[:2, :2], B[:2, :1], np.array([[1.0, 0.0], [0.0, 0.0]]), np.array([[1.0]]))
    assert rel(K[:1, :2], g["toy_K"]) < 1e-10
    xs, us = mo.rollout_lqr_linear([3, 1, 0, 0, 0, 0, 0, 0, 0], A, B, -K, [-3, 0, 0, 0, 0, 0, 0, 0, 0], np.zeros(3), 30)
    assert rel(xs[:, :2], g["toy_xtraj"]) < 1e-10 and rel(us[:, :1], g["toy_utraj"]) < 1e-10


def test_reference_asserting_tests(oracle):
    """test_env.py:40-147 (test_act_cmd_lims, test_act_rate_lims) restated on the oracle."""
    g = golden("g567_trim_lin_lqr.npz")
    x = np.copy(g["trim_x_xcg25"])
    u_lb, u_ub = np.array([1000, -25, -21.5, -30.]), np.array([19000, 25, 21.5, 30.])
    xs = np.copy(x); xs[12] = u_lb[0] - 1; xs[13:16] = u_lb[1:]
    xd = oracle.calc_xdot(xs, u_lb - 1000)
    assert xd[12] > 0 and np.allclose(xd[13:16], 0, atol=1e-7)
    xs = np.copy(x); xs[12] = u_ub[0] + 1; xs[13:16] = u_ub[1:]
    xd = oracle.calc_xdot(xs, u_ub + 1000)
    assert xd[12] < 0 and np.allclose(xd[13:16], 0, atol=1e-7)
    u = np.copy(x[12:16]); u[1:] = u_ub[1:]
    np.testing.assert_allclose(oracle.calc_xdot(x, u)[13:16], [60, 80, 120], atol=1e-7)
    u[1:] = u_lb[1:]
    np.testing.assert_allclose(oracle.calc_xdot(x, u)[13:16], [-60, -80, -120], atol=1e-7)


@pytest.mark.parametrize("xcg", [25, 35])
def test_g4_rollouts(oracle, xcg):
    g = golden("g4_rollout.npz")
    g5 = golden("g567_trim_lin_lqr.npz")
    x0 = g5[f"trim_x_xcg{xcg}"][None]
    _, traj, st = oracle.rollout(x0, g[f"trim_u_xcg{xcg}"][None], 1000, 0.001, 1, xcg / 100)
    assert st[0] == 0
    assert rel(traj[49::50, 0], g[f"trim_traj_xcg{xcg}"]) < 1e-10
    _, traj, st = oracle.rollout(g[f"pert_x0_xcg{xcg}"], g[f"pert_u_xcg{xcg}"], 300, 0.001, 1, xcg / 100)
    assert not st.any()
    assert rel(traj[24::25].transpose(1, 0, 2), g[f"pert_traj_xcg{xcg}"]) < 1e-10


@pytest.mark.parametrize("xcg", [25, 35])
def test_g12_nonlinear_lqr_loop(oracle, xcg):
    """G12: the reference's closed loop under its LQR controller (test_env_mk2.py:70-85 run by tools/make_golden.py --g12):
    six cases x 300 steps, every 25th state and the last action -- the restated loop (env.py:360-371 action + step)."""
    g = golden("g12_lqr_loop.npz")
    x0, dem = g[f"x0_xcg{xcg}"], g[f"dem_xcg{xcg}"]
    xf, traj, u_last, st = oracle.rollout_lqr(x0, g[f"u0_xcg{xcg}"], g[f"K_xcg{xcg}"], dem, 300, 0.001, 1, xcg / 100)
    assert not st.any()
    assert rel(traj[24::25].transpose(1, 0, 2), g[f"traj_xcg{xcg}"]) < 1e-10
    assert rel(u_last, g[f"u_last_xcg{xcg}"]) < 1e-10
    # the action itself, as numpy computes it (oracle.mpc_oracle.lqr_action: env.py:360-371 literally)
    x9 = x0[3][mo.MPC_X_IDX]
    ua = mo.lqr_action(*dem[3], g[f"K_xcg{xcg}"], x9, g[f"u0_xcg{xcg}"][1:])
    e = dem[3] - x0[3][9:12]
    np.testing.assert_allclose(ua, -(g[f"K_xcg{xcg}"][:, 4:7] @ e) + g[f"u0_xcg{xcg}"][1:], rtol=1e-13)
    # the controller does something: the rates move towards the demands of case 1
    assert np.abs(g[f"traj_xcg{xcg}"][1, -1, 9:12] - dem[1]).max() < np.abs(x0[1][9:12] - dem[1]).max()


@pytest.mark.parametrize("xcg", [25, 35])
def test_g6_g7_linearise_c2d_lqr(oracle, xcg):
    g = golden("g567_trim_lin_lqr.npz")
    x = g[f"trim_x_xcg{xcg}"]
    A, B, C, D = oracle.linearise_na(x, xcg=xcg / 100)
    # forward differences amplify 1e-16 by 1/eps = 1e5
    np.testing.assert_allclose(A, g[f"ssr_Ac_xcg{xcg}"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(B, g[f"ssr_Bc_xcg{xcg}"], rtol=0, atol=1e-8)
    assert np.array_equal(C, g[f"ssr_Cc_xcg{xcg}"]) and np.array_equal(D, g[f"ssr_Dc_xcg{xcg}"])
    A18, B18, C18, D18 = oracle.linearise_full(x, x[12:16], xcg=xcg / 100)
    np.testing.assert_allclose(A18, g[f"A18_xcg{xcg}"], rtol=0, atol=2e-7)
    np.testing.assert_allclose(B18, g[f"B18_xcg{xcg}"], rtol=0, atol=1e-8)
    assert np.array_equal(C18, g[f"C18_xcg{xcg}"])
    Ad, Bd, Cd, Dd = mo.c2d(g[f"ssr_Ac_xcg{xcg}"], g[f"ssr_Bc_xcg{xcg}"], g[f"ssr_Cc_xcg{xcg}"], g[f"ssr_Dc_xcg{xcg}"], 0.001)
    assert np.array_equal(Ad, g[f"ssr_Ad_xcg{xcg}"]) and np.array_equal(Bd, g[f"ssr_Bd_xcg{xcg}"])
    K = mo.lqr_gain_from_linearisation(g[f"ssr_Ac_xcg{xcg}"], g[f"ssr_Bc_xcg{xcg}"], g[f"ssr_Cc_xcg{xcg}"],
                                       g[f"ssr_Dc_xcg{xcg}"], 0.001)
    np.testing.assert_allclose(K, g[f"K_lqr_xcg{xcg}"], rtol=1e-9)
    if xcg == 25:   # SURVEY.md 8c known answer
        np.testing.assert_allclose(K[0, :3], [-3.22345e-3, -0.984279, 1782.79], rtol=1e-5)
        u = mo.lqr_action(0.1, -0.05, 0.02, K, g["lqr_action_x9"], x[13:16])
        np.testing.assert_allclose(u, g["lqr_action_u"], rtol=1e-9)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_g10_restated_step_path_vs_the_time_histories_the_reference_holds(oracle, k):
    """The reference keeps output of its Simulink driver as data files (C/ele_0.100...vel300.txt, Nguyen_m/ele_0.000...txt;
    runF16Sim.m:100-150): 30 s of the trimmed hifi model at 1 ms, one of them with a 0.1 deg surface doublet.  The restated step
    path (Nlplant + atmos + actuators + flap model + Euler, env.py:65-130) started from a file's first row reproduces its first
    10 s -- 12 states and the six plant outputs nx ny nz mach qbar ps at every 0.1 s -- once the roll-damping-by-yaw-rate table is
    really loaded (the Python reference's C never loads CLr, hifi_F16_AeroData.c:964-972: flag FIX_CLR): an independent pin of
    rows a1-a11 that owes nothing to the Python reference's own binaries.  Without the flag the lateral states are 30 x further
    off (asserted: this is what the defect does)."""
    from conftest import G10_OUT_TOL, G10_TOL, g10_case, g10_command, g10_rows_of_states
    a, xcg, x0, trim_u, dis = g10_case(k)

    def run(fix):
        oracle.lib.f16o_set_fix_clr(fix)
        try:
            x = x0[None].copy()
            hist, outs = [x[0].copy()], [oracle.nlplant(x[0], 1, xcg)[12:18]]
            for j in range(100):
                x, _, st = oracle.rollout(x, g10_command(trim_u, dis, j)[None], 100, dt=0.001, fi_flag=1, xcg=xcg, store=False)
                assert int(st[0]) == 0
                hist.append(x[0].copy())
                outs.append(oracle.nlplant(x[0], 1, xcg)[12:18])
        finally:
            oracle.lib.f16o_set_fix_clr(0)
        return np.array(hist), np.array(outs)

    s, outs = run(1)
    err = np.abs(g10_rows_of_states(s) - a[:, 1:13])
    assert np.all(err.max(0) < G10_TOL), err.max(0)
    assert np.all(np.abs(outs[0] - a[0, 13:19]) < 6e-6)                  # the first row: the printed precision
    assert np.all(np.abs(outs - a[:, 13:19]).max(0) < G10_OUT_TOL), np.abs(outs - a[:, 13:19]).max(0)
    assert np.abs(s[:, 13:16] - a[:, 20:23]).max() < 2e-3               # surface positions (actuator model, utils.py:314-330)
    if k == 0:
        s0, _ = run(0)
        e0 = np.abs(g10_rows_of_states(s0) - a[:, 1:13]).max(0)
        assert e0[3] > 30 * err[:, 3].max() and e0[9] > 30 * err[:, 9].max()      # phi, p without the real CLr table


def test_g11_derivatives_of_the_restated_model_vs_the_state_space_file_the_reference_holds(oracle):
    """Nguyen_m/StateSpace_alt10000_vel700.txt: A, B of the 18-state hifi and lofi models as the reference's Simulink tooling
    linearised them (five decimals).  Central differences of the restated `_calc_xdot` (env.py:65-103: plant, actuators, flap
    model) at the same trim points give the same matrices -- hifi: all 18 x 18 + 18 x 4 entries with the real CLr table (without
    it d pdot / d r is 0.455 instead of the file's 0.621: asserted); lofi: the 12 rigid-body rows."""
    from conftest import g11_case, g11_jacobians, g11_perturbations

    def jac(tag, fix):
        A, B, x, u, fi = g11_case(tag)
        X, U = g11_perturbations(x, u)
        oracle.lib.f16o_set_fix_clr(fix)
        try:
            xd = np.array([oracle.calc_xdot(X[i], U[i], fi, 0.25) for i in range(44)])
        finally:
            oracle.lib.f16o_set_fix_clr(0)
        return A, B, *g11_jacobians(xd)

    A, B, Ao, Bo = jac("hi", 1)
    assert np.all(np.abs(Ao - A) < 1.5e-4 * np.maximum(1, np.abs(A))) and np.all(np.abs(Bo - B) < 1e-5)
    A, B, Ao, Bo = jac("hi", 0)
    assert abs(A[9, 11] - 0.62087) < 1e-9 and abs(Ao[9, 11] - 0.45504) < 1e-4
    A, B, Ao, Bo = jac("lo", 0)
    assert np.all(np.abs(Ao[:12, :16] - A[:12, :16]) < 1.5e-4 * np.maximum(1, np.abs(A[:12, :16])))
    assert np.all(np.abs(Bo[:16] - B[:16]) < 1e-5)
    # MATLAB_SS.mat, the file the reference's own test_linearisation loads (test_env.py:186): the same lofi model in full
    # precision (the trim point is still known to five decimals only); and its eigenvalues as quoted there (:159-176)
    g = golden("g11_state_space.npz")
    assert np.abs(g["A_mat"] - A).max() < 6e-6 and np.abs(g["B_mat"] - B).max() < 6e-6
    assert np.all(np.abs(Ao[:12, :16] - g["A_mat"][:12, :16]) < 5e-5 * np.maximum(1, np.abs(g["A_mat"][:12, :16])))
    ev = np.linalg.eigvals(np.block([[Ao[:12, :16]], [g["A_mat"][12:16, :16]]]))
    for known in (-1.3929 + 2.7668j, -0.4478 + 3.9347j, -0.0067 + 0.0670j, -3.7888, -0.0089):
        assert np.abs(ev - known).min() < 2e-4, known


def test_g5_trim_known_answers():
    g = golden("g567_trim_lin_lqr.npz")
    x = g["trim_x_xcg25"]
    np.testing.assert_allclose([x[7], x[12], x[13], x[14], x[15], x[16], x[17]],
                               [0.0205901002, 2886.64684, -2.03851753, -0.0875768294, -0.0387697724, 0.398604403,
                                -1.17972584], rtol=1e-6)
    x = g["trim_x_xcg35"]
    np.testing.assert_allclose([x[7], x[12], x[13]], [0.01682719, 2626.586, -0.5043574], rtol=1e-6)


def test_g8_prediction_matrices_and_qp():
    g = golden("g8_mpc_qp.npz")
    At, Bt, Ct = np.array([[1.1, 2], [0, 0.95]]), np.array([[0], [0.0787]]), np.array([[-1.0, 1.0]])
    MM, CC = mo.calc_MC(At, Bt, 1, 4)
    assert np.array_equal(MM, g["toy_MM"]) and np.array_equal(CC, g["toy_CC"])
    H = CC.T @ mo.dmom(Ct.T @ Ct, 4) @ CC + mo.dmom(np.eye(1) * 0.01, 4)
    np.testing.assert_allclose(H, g["toy_H"], rtol=1e-14)
    np.testing.assert_allclose(mo.dlqr(At, Bt, Ct.T @ Ct, np.eye(1) * 0.01), g["toy_K"], rtol=1e-12)
    g5 = golden("g567_trim_lin_lqr.npz")
    for xcg in (25, 35):
        Ad, Bd, Cd = g5[f"ssr_Ad_xcg{xcg}"], g5[f"ssr_Bd_xcg{xcg}"], g5[f"ssr_Cd_xcg{xcg}"]
        MM, CC = mo.calc_MC(Ad, Bd, 0.001, 10)
        assert np.array_equal(MM, g[f"MM10_xcg{xcg}"]) and np.array_equal(CC, g[f"CC10_xcg{xcg}"])
        for N in (4, 10, 30):
            P, q, A, l, u = mo.mpc_qp(g5[f"trim_x_xcg{xcg}"], Ad, Bd, Cd, N, 0.001)
            tag = f"xcg{xcg}_N{N}"
            np.testing.assert_allclose(P, g[f"P_{tag}"], rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(q, g[f"q_{tag}"], rtol=1e-10, atol=1e-12)
            assert np.array_equal(A, g[f"A_{tag}"])
            assert np.array_equal(l, g[f"l_{tag}"]) and np.array_equal(u, g[f"u_{tag}"])


@pytest.mark.parametrize("xcg", [25, 35])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_g8b_setup_osqp_with_other_weights_reference_and_bounds(xcg, tag):
    """G8b: the reference's setup_OSQP (utils.py:21-167) run with arguments OTHER than the ones env.py:373-424 hard-wires --
    (a) the weights its author left commented out at env.py:391-403 with R = 0.01 I; (b) a dense SPD Q / R, a free reference and
    tightened / widened boxes -- against the restated setup_OSQP / dlqr (oracle.mpc_oracle)."""
    g = golden("g8b_mpc_qp_weights.npz")
    Q, R = g[f"Q{tag}"], g[f"R{tag}"]
    x_full = g[f"x_full_xcg{xcg}"]
    x9, act = x_full[mo.MPC_X_IDX], x_full[mo.MPC_U_IN_X_IDX]
    Ad, Bd = g[f"Ad_xcg{xcg}"], g[f"Bd_xcg{xcg}"]
    bnds = [g[f"{nm}_{tag}"] for nm in ("xlb", "xub", "ulb", "uub", "rlb", "rub")]
    np.testing.assert_allclose(mo.dlqr(Ad, Bd, Q, R), g[f"K_{tag}_xcg{xcg}"], rtol=1e-8, atol=1e-12)
    for N in (4, 10, 30):
        P, q, A, l, u = mo.setup_OSQP(g[f"xref_{tag}_xcg{xcg}"], Ad, Bd, Q, R, N, 0.001, x9, act, *bnds)
        t = f"{tag}_xcg{xcg}_N{N}"
        assert np.abs(P - g[f"P_{t}"]).max() / np.abs(g[f"P_{t}"]).max() < 1e-9
        assert np.abs(q.ravel() - g[f"q_{t}"]).max() / np.abs(g[f"q_{t}"]).max() < 1e-8
        for got, ref in ((l.ravel(), g[f"l_{t}"]), (u.ravel(), g[f"u_{t}"])):
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(got), fin)
            np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-12, atol=1e-12)
        if N < 30:
            np.testing.assert_allclose(A, g[f"A_{t}"], rtol=1e-12, atol=1e-18)


@pytest.mark.parametrize("xcg", [25, 35])
def test_g9_admm_reaches_exact_minimiser_band(xcg):
    """OSQP-style ADMM at OSQP's default tolerances lands within the solver band of the exact
    minimiser (first-block rate rows active at trim, first move ~ act-0.06, act+0.08)."""
    g = golden("g8_mpc_qp.npz")
    tag = f"xcg{xcg}_N30"
    P, q, A, l, u = (g[f"{k}_{tag}"] for k in "PqAlu")
    xs = g[f"xstar_{tag}"]
    r = mo.admm_osqp_style(P, q, A, l, u)
    assert r["iters"] <= 1000
    assert np.abs(r["x"][:3] - xs[:3]).max() < 2e-2
    tight = mo.admm_osqp_style(P, q, A, l, u, eps_abs=1e-9, eps_rel=1e-9, max_iter=200000)
    assert np.abs(tight["x"] - xs).max() < 1e-6
    if xcg == 35:
        np.testing.assert_allclose(xs[:3], [-0.56435742, -0.01095324, 0.00097151], atol=2e-6)


@pytest.mark.parametrize("xcg", [25, 35])
def test_g5_trim_restatement_reproduces_the_reference_trim(oracle, xcg):
    """scipy Nelder-Mead on the restated objective lands on the reference's trim point bit for bit (1,932 evaluations
    at xcg 0.25)."""
    g = golden("g567_trim_lin_lqr.npz")
    x, opt = mo.trim(oracle, 10000, 700, xcg=xcg / 100)
    assert np.array_equal(x, g[f"trim_x_xcg{xcg}"])
    if xcg == 25:
        assert opt.nfev == 1932


# ---------------------------------------------------------------------------------------------------------------------
# Round-2 additions: the C control chain (oracle/f16_mpc_oracle.c), the OSQP restatement, the reference's own C rebuilt
@pytest.mark.parametrize("xcg", [25, 35])
def test_c_control_chain_vs_reference_fixtures_and_numpy_twin(oracle, xcg):
    """oracle/f16_mpc_oracle.c against the reference's captured outputs (G6-G8) and against the numpy/scipy restatement:
    ZOH, DARE, setup_OSQP, and the three solver modes rule for rule (same iteration counts, x to 1e-9)."""
    g5, g8 = golden("g567_trim_lin_lqr.npz"), golden("g8_mpc_qp.npz")
    Ad, Bd = oracle.c2d(g5[f"ssr_Ac_xcg{xcg}"], g5[f"ssr_Bc_xcg{xcg}"], 0.001)
    np.testing.assert_allclose(Ad, g5[f"ssr_Ad_xcg{xcg}"], rtol=0, atol=5e-15)
    np.testing.assert_allclose(Bd, g5[f"ssr_Bd_xcg{xcg}"], rtol=0, atol=1e-17)
    import scipy.linalg
    Cd = g5[f"ssr_Cd_xcg{xcg}"]
    X = oracle.dare(g5[f"ssr_Ad_xcg{xcg}"], g5[f"ssr_Bd_xcg{xcg}"], Cd.T @ Cd)
    Xref = scipy.linalg.solve_discrete_are(g5[f"ssr_Ad_xcg{xcg}"], g5[f"ssr_Bd_xcg{xcg}"], Cd.T @ Cd, np.eye(3))
    assert np.abs(X - Xref).max() / np.abs(Xref).max() < 1e-9
    for N in (4, 10, 30):
        tag = f"xcg{xcg}_N{N}"
        P, q, A, l, u = oracle.mpc_qp(g5[f"trim_x_xcg{xcg}"], g5[f"ssr_Ad_xcg{xcg}"], g5[f"ssr_Bd_xcg{xcg}"], Cd, N, 0.001)
        assert np.abs(P - g8[f"P_{tag}"]).max() / np.abs(g8[f"P_{tag}"]).max() < 1e-9
        assert np.abs(q - g8[f"q_{tag}"]).max() / np.abs(g8[f"q_{tag}"]).max() < 1e-7
        assert np.array_equal(A, g8[f"A_{tag}"]) or np.abs(A - g8[f"A_{tag}"]).max() < 1e-17
        fin = np.isfinite(g8[f"l_{tag}"])
        assert np.array_equal(np.isfinite(l), fin) and np.array_equal(np.isfinite(u), np.isfinite(g8[f"u_{tag}"]))
        np.testing.assert_allclose(l[fin], g8[f"l_{tag}"][fin], rtol=1e-12, atol=1e-12)
        Pg, qg, Ag, lg, ug = (g8[f"{k}_{tag}"] for k in "PqAlu")
        twins = ((0, mo.admm_osqp_style(Pg, qg, Ag, lg, ug)), (1, mo.admm_osqp(Pg, qg, Ag, lg, ug)),
                 (2, mo.admm_osqp(Pg, qg, Ag, lg, ug, drop_unbounded_rows=True)))
        for mode, ref in twins:
            r = oracle.admm(Pg, qg, Ag, lg, ug, mode=mode)
            assert r["iters"] == ref["iters"] and r["status"] == 0, (tag, mode, r["iters"], ref["iters"])
            assert np.abs(r["x"] - ref["x"]).max() < 1e-9 and abs(r["rho"] - ref["rho"]) < 1e-9 * ref["rho"]


@pytest.mark.parametrize("xcg", [25, 35])
def test_osqp_restatement_vs_exact_minimiser(xcg):
    """mo.admm_osqp = the solve env.py:420-422 implies (osqp defaults).  "Parity unpinned" at this boundary (no osqp, no
    reference fixture): what can be pinned is that it solves the reference-built QP -- first move inside OSQP's own
    tolerance band around the exact minimiser (eps_rel 1e-3 on rows of magnitude ~10), tight tolerances -> the minimiser --
    and that dropping the unbounded rows after the equilibration (what the kernels do) changes nothing visible."""
    g8 = golden("g8_mpc_qp.npz")
    for N in (4, 10, 30):
        tag = f"xcg{xcg}_N{N}"
        P, q, A, l, u = (g8[f"{k}_{tag}"] for k in "PqAlu")
        xs = g8[f"xstar_{tag}"]
        r = mo.admm_osqp(P, q, A, l, u)
        assert r["converged"] and np.abs(r["x"][:3] - xs[:3]).max() < 2e-2
        assert r["r_prim"] < 1e-3 * (1 + np.abs(A @ r["x"]).max()) and np.all(r["D"] > 0) and np.all(r["E"] > 0) and r["c"] > 0
        rd = mo.admm_osqp(P, q, A, l, u, drop_unbounded_rows=True)
        assert rd["iters"] == r["iters"] and np.abs(rd["x"] - r["x"]).max() < 1e-5
        rt = mo.admm_osqp(P, q, A, l, u, eps_abs=1e-9, eps_rel=1e-9, max_iter=400000)
        assert np.abs(rt["x"] - xs).max() < 1e-5
    # the equilibration itself: scaled data reproduce the original problem, norms are equilibrated
    Ps, qs, As, ls, us, D, E, c = mo.osqp_scale(P, q, A, np.maximum(l, -1e30), np.minimum(u, 1e30))
    np.testing.assert_allclose(Ps, c * D[:, None] * P * D[None, :], rtol=1e-12)
    np.testing.assert_allclose(As, E[:, None] * A * D[None, :], rtol=1e-12, atol=1e-300)
    kkt_cols = np.maximum(np.abs(Ps).max(axis=0) / c, np.abs(As).max(axis=0))
    assert kkt_cols.max() / kkt_cols.min() < 2.0


def test_reference_c_rebuilt_here_agrees_with_the_restatement(oracle):
    """Fixture G2r = the reference's own C compiled from its sources by oracle/Makefile (oracle/_ref/, tools/make_golden.py --g2r)
    on the first 400 hifi inputs of G2, against libf16_oracle.so.  The reference's `_CLr` interpolates uninitialised heap
    (C/hifi_F16_AeroData.c:964-972): the fixture was taken in a process where it reads ~0, so all 18 outputs are compared."""
    g = golden("g2r_ref_rebuilt.npz")
    xu = golden("g2_nlplant.npz")["xu_hifi"][:int(g["n"])]
    for xcg in (25, 35):
        mine = np.array([oracle.nlplant(x, 1, xcg / 100) for x in xu])
        assert rel(mine, g[f"xdot_hifi_xcg{xcg}"]) < TOL, xcg


def test_reference_c_rebuilt_here_agrees_with_the_restatement_on_the_lattice(oracle):
    """Fixture G18 = the same rebuilt reference C (tools/make_golden.py --g2r) on the whole-grid batch of tests/envelope_cases.py:
    one aircraft per (alpha, beta, elevator) cell and the edge rows (values on a node, on the first / last node, one ulp beside a
    node, -0.0, 35,000 ft), wherever the reference is defined: alpha in [-20, 45] (its leading-edge-flap tables end there and its
    bracket search is undefined off a grid), |beta| <= 30, |elevator| <= 25.  The fixture carries its inputs; they must still be
    the batch's rows."""
    import envelope_cases as ec
    g = golden("g18_lattice_nlplant.npz")
    b = ec.hifi_lattice(int(g["seed"]))
    rows, xu = g["rows"], g["xu"]
    assert np.array_equal(xu.view(np.int64), b.x[rows].view(np.int64))
    cells = b.cell[rows[rows < b.n_lattice]]
    assert len(set(map(tuple, cells))) == 13 * 18 * 4 and set(cells[:, 0]) == set(range(13))      # every cell up to alpha = 45
    named = {k for k, r in b.edge.items() if r in set(rows)}
    assert {"alpha_node", "beta_node", "el_node", "all_nodes", "alpha_first", "alpha2_last", "beta_first", "beta_last", "el_first",
            "el_last", "alpha_node_up", "alpha_node_dn", "beta_node_up", "beta_node_dn", "el_node_up", "el_node_dn", "beta_neg_zero",
            "el_neg_zero", "alt_35000", "alt_below_35000", "climb_0"} <= named
    for xcg in (25, 35):
        mine = np.array([oracle.nlplant(x, 1, xcg / 100) for x in xu])
        assert rel(mine, g[f"xdot_hifi_xcg{xcg}"]) < TOL, xcg
        assert all(oracle.nlplant(x, 1, xcg / 100) is not None and oracle.lib.f16o_last_status() == 0 for x in xu[::7])
    # the lofi model: a quarter of its lattice and its edge rows; beyond alpha -10 / 45 deg the reference extrapolates along the last
    # cell (lofi_F16_AeroData.c:33-38) and so must the restatement, without a status bit
    lb = ec.lofi_lattice(int(g["seed"]))
    rows, xu = g["rows_lofi"], g["xu_lofi"]
    assert np.array_equal(xu.view(np.int64), lb.x[rows].view(np.int64))
    assert {lb.edge[k] for k in ("off_alpha_hi", "off_alpha_lo", "alpha_first", "alpha_last", "alpha_zero", "el_box", "beta_last")} <= set(rows)
    assert len(set(lb.cell[rows[rows < lb.n_lattice], 0])) == 11
    for xcg in (25, 35):
        mine = np.array([oracle.nlplant(x, 0, xcg / 100) for x in xu])
        assert rel(mine, g[f"xdot_lofi_xcg{xcg}"]) < TOL, xcg
        assert oracle.nlplant(lb.x[lb.edge["off_alpha_hi"]], 0, xcg / 100) is not None and oracle.lib.f16o_last_status() == 0


def test_closed_mpc_loop_of_the_checker_and_its_rules_for_flagged_aircraft(oracle):
    """oracle.mpc_closed_loop (oracle/f16_mpc_oracle.c: f16o_mpc_closed_loop) = test_env.py:480-495 for B aircraft with a frozen model:
    equal to the same loop written out call by call (QP of the reference's setup_OSQP, the C solve, one `step`), and the stated rules for
    the cases the reference does not survive: outside the envelope -> frozen, flagged, not solved for; state not finite -> no QP, NaN
    command, zero iterations; the hold rule keeps the previous command where a step has none."""
    g = golden("g567_trim_lin_lqr.npz")
    x = np.tile(g["trim_x_xcg35"], (3, 1))
    u = np.copy(x[:, 12:16])
    x[1, 13] = 26.0                                            # elevator outside its box (env.py:117-124 would exit())
    x[2, 9] = np.nan                                           # a roll rate that is not finite
    A_, B_, C_, D_ = oracle.linearise_na(x[0], u3=u[0, 1:], xcg=0.35)
    Ad, Bd, Cd, _ = mo.c2d(A_, B_, C_, D_, 0.001)
    N, T, dem = 6, 4, (0.02, -0.01, 0.0)
    r = oracle.mpc_closed_loop(x, u, Ad, Bd, Cd, N, T, dem, store=True)
    assert r["status"][0] == 0 and r["status"][1] == 16 | (1 << (8 + 13)) and r["status"][2] & 32
    assert np.array_equal(r["x"][1], x[1]) and np.array_equal(r["u"][1], u[1])               # frozen: nothing moved
    assert np.isnan(r["cmd"][:, 1:]).all() and (r["iters"][:, 1:] == 0).all()
    assert np.isnan(r["u"][2, 1:]).all() and np.isnan(r["x"][2, 13:16]).all()                # NaN command -> NaN surface states (np.clip)
    xs, us = x[0].copy(), u[0].copy()                          # aircraft 0, call by call
    for t in range(T):
        P, q, A, l, uu = oracle.mpc_qp(xs, Ad, Bd, Cd, N, 0.001, dem)             # (the C builder: the loop's own)
        sol = oracle.admm(P, q, A, l, uu, mode=2)
        assert sol["iters"] == r["iters"][t, 0] and np.array_equal(sol["x"][:3], r["cmd"][t, 0])
        Pn, qn, An, ln, un = mo.mpc_qp(xs, Ad, Bd, Cd, N, 0.001, *dem)              # (... which is the restated setup_OSQP)
        assert rel(P, Pn) < 1e-12 and rel(q, qn) < 1e-10 and np.array_equal(np.isinf(l), np.isinf(ln))
        us[1:4] = sol["x"][:3]
        xs = oracle.rollout(xs[None], us[None], 1, xcg=0.35, store=False)[0][0]
        assert np.array_equal(xs, r["traj"][t, 0])
    rh = oracle.mpc_closed_loop(x, u, Ad, Bd, Cd, N, T, dem, hold=True)
    assert np.array_equal(rh["u"][2], u[2]) and not np.isnan(rh["x"][2, 13:16]).any()       # held: the surfaces keep their command
    assert np.array_equal(rh["cmd"][:, 0], r["cmd"][:, 0])


@pytest.mark.parametrize("xcg", [25, 35])
def test_g14_per_step_relinearised_lqr_loop(oracle, xcg):
    """The reference's `test_LQR_dynamic_nl` (test_env.py:625-687; SURVEY.md 8f-2's pattern), 150 steps: at EVERY step linearise at the
    current state (env.py:294-342) -> cont2discrete -> K = dlqr(A, B, I, 1e4 I); cmd = -K (x9 - x_ref); step.  Pins the chain
    linearise -> ZOH -> dlqr along a moving trajectory (G6 / G7 pin it at the trim point only).  Forward differences with eps = 1e-5
    amplify last-bit differences of the plant by 1e5, the gain (entries up to 1,400) carries them into the command: 5e-6 absolute."""
    g = golden("g14_dynamic_lqr.npz")
    x, u = g[f"x0_xcg{xcg}"].copy(), g[f"u0_xcg{xcg}"].copy()
    idx = [3, 4, 7, 8, 9, 10, 11, 17, 16]
    xref, Q, R = x[idx].copy(), np.eye(9), np.eye(3) * 1e4
    for t in range(150):
        A_, B_, C_, D_ = oracle.linearise_na(x, u3=u[1:], xcg=xcg / 100)
        Ad, Bd, _, _ = mo.c2d(A_, B_, C_, D_, 0.001)
        K = mo.dlqr(Ad, Bd, Q, R)
        if t in (0, 50, 149):
            assert rel(K, g[f"K{t}_xcg{xcg}"]) < 1e-6
        cmd = -K @ (x[idx] - xref)
        assert np.abs(cmd - g[f"cmd_xcg{xcg}"][t]).max() < 5e-6, t
        u[1:4] = cmd
        x = oracle.rollout(x[None], u[None], 1, xcg=xcg / 100, store=False)[0][0]
        if (t + 1) % 10 == 0:
            assert rel(x, g[f"x_xcg{xcg}"][(t + 1) // 10 - 1]) < 1e-7

