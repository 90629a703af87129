"""GPU tests of the per-step re-linearised LQR loop as one launch (C-ABI f16_rollout_lqr_relin, F16Batch.rollout_LQR_relin and
rollout_LQR(relinearise=True)): the reference's `test_LQR_dynamic_nl` (test_env.py:625-687, fixture G14), the batch chain it fuses
(f16_linearise_batch -> f16_c2d_batch -> f16_lqr_batch_w -> action -> f16_rollout(F16_FLAG_ONE_LANE)), the CPU twin and the
bit-for-bit properties of the launch."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import mpc_oracle as mo

pytestmark = pytest.mark.gpu

IDX9 = [3, 4, 7, 8, 9, 10, 11, 17, 16]          # parameters.py:135 mpc_x_idx
DEM = (0.05, -0.02, 0.01)
ENVELOPE, QP_MAXITER = 16, 64
F16_EINVAL = -1
# Closed loops are compared on the aircraft whose re-derived gains stay moderate.  At untrimmed config-2 points the per-step gains
# reach 1e5 - 1e9 (|K| of G14's trimmed loop: 1.4e3), the commands saturate and ulp-level differences of the linearisation (1e5 x by the
# forward difference, <= 1e-8 of max |K| in the gain: test_gains_equal_the_batch_chain_at_the_same_point) grow with |K| along the loop.
# Measured, fused vs host chain, 256 aircraft, 100 steps, worst state difference (relative) by max |K| over the run:
#   dynamic_nl  <= 1e3: 43 aircraft 1.6e-10;  <= 3e3: 101 aircraft 1.7e-7;  <= 1e4: 134 aircraft 7.9e-5;  all: 1.0
#   env_law     <= 1e3: 30 aircraft 1.9e-10;  <= 3e3:  93 aircraft 4.2e-10; <= 1e4: 144 aircraft 1.5e-9;  all: 4.8e-7
# (median aircraft over all 256: 3e-10).  Beyond KMAX an aircraft has no trajectory reproducible to the bands below.
KMAX = 1e3


def conditioned(Kt, status):
    """[B] bool: max |K| over every sampled step <= KMAX and every DARE converged (no F16_ST_QP_MAXITER)."""
    km = Kt.abs().amax(dim=(0, 2, 3)).cpu().numpy()
    return (km <= KMAX) & ((status.cpu().numpy() & QP_MAXITER) == 0)


def make_env(x, u=None, **kw):
    from f16_mpc_oop_py_amd import F16Batch
    return F16Batch(x, u, device="cuda:0", **kw)


def rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def workload(B, seed=20261003):
    from f16_mpc_oop_py_amd.workload import config2_states
    return config2_states(B, seed=seed)


def law(name, env):
    """The two argument sets of the issue: (x_ref [B,9] or None, track, u0 [B,3] or None, Q, R)."""
    if name == "dynamic_nl":        # test_env.py:625-687: fixed full reference = the initial x9, Q = I, R = 1e4 I, no offset
        return dict(x_ref=None, track=None, u0=None, Q=np.eye(9), R=np.eye(3) * 1e4)
    xr = np.zeros((env.B, 9))       # env.py:360-371 re-derived every step: demands on p, q, r, offset u.initial_condition[1:]
    xr[:, 4:7] = DEM
    return dict(x_ref=xr, track=(4, 5, 6), u0=env._u_init[1:4].t().cpu().numpy(), Q=None, R=None)


@pytest.mark.parametrize("xcg", [25, 35])
def test_g14_in_one_launch(xcg):
    """Fixture G14 (the reference's loop, 150 steps) through ONE call: the bands of the B = 1 host-loop test
    (tests/test_gpu_control.py::test_g14_per_step_relinearised_lqr_loop_on_the_device)."""
    g = golden("g14_dynamic_lqr.npz")
    env = make_env(g[f"x0_xcg{xcg}"][None], g[f"u0_xcg{xcg}"][None], xcg=xcg / 100)
    traj, ut, Kt = env.rollout_LQR_relin(150, Q=np.eye(9), R=np.eye(3) * 1e4, traj_every=1, gains_every=1)
    assert traj.shape == (150, 18, 1) and ut.shape == (150, 3, 1) and Kt.shape == (150, 1, 3, 9)
    for t in (0, 50, 149):
        assert rel(-Kt[t, 0].cpu().numpy(), g[f"K{t}_xcg{xcg}"]) < 1e-5, t
    cmd = ut[:, :, 0].cpu().numpy()
    assert np.abs(cmd - g[f"cmd_xcg{xcg}"]).max() < 2e-5
    x = traj[:, :, 0].cpu().numpy()
    for i in range(15):
        assert rel(x[10 * i + 9], g[f"x_xcg{xcg}"][i]) < 1e-6, i
    assert int(env.status.max()) == 0
    assert torch.equal(env._u[1:4, 0], ut[-1, :, 0]) and torch.equal(env._x[:, 0], traj[-1, :, 0])


@pytest.mark.parametrize("name", ["dynamic_nl", "env_law"])
def test_gains_equal_the_batch_chain_at_the_same_point(name):
    """K_traj[t] equals f16_linearise_batch -> f16_c2d_batch -> f16_lqr_batch_w evaluated at the state before step t and the
    command of step t - 1 (read back from traj / u_traj): <= 1e-8 relative to max|K| of the aircraft.  The two sides evaluate the
    same plant through different instruction sequences (an out-of-line function reading the tables from global memory against
    the linearise kernel's inlined one on LDS tables): ulp-level differences of xdot, amplified 1e5 x by the forward difference."""
    from f16_mpc_oop_py_amd import lib
    B, T = 256, 100
    x0, u0 = workload(B)
    env = make_env(x0, u0, xcg=0.25)
    a = law(name, env)
    traj, ut, Kt = env.rollout_LQR_relin(T, **a, traj_every=1, gains_every=1)
    live = ((env.status & ENVELOPE) == 0).cpu().numpy()
    assert live.sum() >= B // 2, live.sum()
    w = lib.make_weights(Q=a["Q"], R=a["R"])
    worst = 0.0
    for t in (0, 1, 37, 99):
        xs = env._x_init.clone() if t == 0 else traj[t - 1].clone()
        us = env._u_init.clone()
        if t > 0:
            us[1:4] = ut[t - 1]
        Ac, Bc, Cc = (torch.empty((n, B), dtype=torch.float64, device="cuda:0") for n in (81, 27, 81))
        Ad, Bd, K = torch.empty_like(Ac), torch.empty_like(Bc), torch.empty_like(Bc)
        L, h = env.lib, env.ctx.handle
        assert L.f16_linearise_batch(h, vp(xs), vp(us), vp(Ac), vp(Bc), vp(Cc), None, B, B, 1e-5, 0.25, 1, 0, None) == 0
        assert L.f16_c2d_batch(h, vp(Ac), vp(Bc), vp(Ad), vp(Bd), B, B, 0.001, None) == 0
        assert L.f16_lqr_batch_w(h, vp(Ad), vp(Bd), vp(Cc), ctypes.byref(w) if w else None, vp(K), None, None, B, B, None) == 0
        Kc = K.t().reshape(B, 3, 9).cpu().numpy()[live]
        Kf = Kt[t].cpu().numpy()[live]
        d = np.abs(Kf - Kc).max(axis=(1, 2)) / np.abs(Kc).max(axis=(1, 2))
        worst = max(worst, float(d.max()))
    assert worst <= 1e-8, worst


def host_chain(env, name, T):
    """The loop written out on the host: _calc_LQR_gain (f16_linearise_batch -> f16_c2d_batch -> f16_lqr_batch_w), the action,
    step() (F16_FLAG_ONE_LANE in the env).  A frozen aircraft keeps its command (the fused loop computes none for it); the DARE's
    F16_ST_QP_MAXITER goes into the status word of an aircraft that was stepped."""
    a = law(name, env)
    x_ref = env._get_mpc_x().clone()
    if a["x_ref"] is not None:
        x_ref = torch.as_tensor(a["x_ref"], device="cuda:0")
    mask = torch.zeros(9, dtype=torch.bool, device="cuda:0")
    mask[list(a["track"] or range(9))] = True
    u0 = torch.zeros((env.B, 3), dtype=torch.float64, device="cuda:0") if a["u0"] is None else torch.as_tensor(a["u0"], device="cuda:0")
    xs, us = [], []
    for _ in range(T):
        K = env._calc_LQR_gain(Q=a["Q"], R=a["R"])                                  # -dlqr
        x9 = env._get_mpc_x()
        e = torch.where(mask, x9 - x_ref, torch.zeros_like(x9))
        cmd = (K @ e.unsqueeze(-1)).squeeze(-1) + u0                                 # -dlqr (x9 - x_ref) + u0
        held = env._u[1:4].clone()
        env._u[1:4] = cmd.t()
        env.step()
        frozen = (env.status & ENVELOPE) != 0
        env._u[1:4][:, frozen] = held[:, frozen]
        env.status[~frozen] |= env.last_status[~frozen] & QP_MAXITER
        xs.append(env._x.clone())
        us.append(env._u[1:4].clone())
    return torch.stack(xs), torch.stack(us)


@pytest.mark.parametrize("name", ["dynamic_nl", "env_law"])
def test_closed_loop_equals_the_host_chain(name):
    """Fused loop vs the host chain step by step over 100 steps, B = 256 config-2 aircraft: the same status words for every
    aircraft; states <= 1e-9 relative and commands <= 5e-8 absolute on the well-conditioned ones (KMAX).  The command band is wider
    than the issue's starting 1e-8: measured 1.5e-8 (env_law, commands up to tens of degrees) -- the gains of the two sides differ by
    up to 1e-8 of max |K| at the same point (the forward difference amplifies ulp differences of xdot 1e5 x) and |K| <= 1e3 multiplies
    that into the command."""
    from f16_mpc_oop_py_amd import lib
    B, T = 256, 100
    x0, u0 = workload(B)
    envh = make_env(x0, u0, xcg=0.25, flags=lib.F16_FLAG_ONE_LANE)
    xh, uh = host_chain(envh, name, T)
    env = make_env(x0, u0, xcg=0.25)
    traj, ut, Kt = env.rollout_LQR_relin(T, **law(name, env), traj_every=1, gains_every=1)
    assert torch.equal(env.status, envh.status)
    ok = conditioned(Kt, env.status)
    assert ok.sum() >= 24, ok.sum()
    xr, xf = xh.cpu().numpy()[..., ok], traj.cpu().numpy()[..., ok]
    assert np.max(np.abs(xf - xr) / np.maximum(1.0, np.abs(xr))) <= 1e-9
    assert np.abs(ut.cpu().numpy()[..., ok] - uh.cpu().numpy()[..., ok]).max() <= 5e-8


@pytest.mark.parametrize("name", ["dynamic_nl", "env_law"])
def test_cpu_twin(oracle, name):
    """B = 32 well-conditioned config-2 aircraft (KMAX; the first 32 of 1024), 100 steps, against the loop composed on the CPU:
    oracle.linearise_na -> scipy cont2discrete -> scipy solve_discrete_are (mpc_oracle.dlqr) -> action -> one oracle.rollout step;
    the G14 bands (gains 1e-5 relative, commands 2e-5 absolute, every 10th state 1e-6 relative)."""
    B, T, xcg = 32, 100, 0.25
    x0, u0 = workload(1024)
    env = make_env(x0, u0, xcg=xcg)
    a = law(name, env)
    traj, ut, Kt = env.rollout_LQR_relin(T, **a, traj_every=1, gains_every=1)
    pick = np.flatnonzero(conditioned(Kt, env.status))[:B]          # (results do not depend on the batch: bit-for-bit test)
    assert len(pick) == B, len(pick)
    traj, ut, Kt = traj.cpu().numpy()[..., pick], ut.cpu().numpy()[..., pick], Kt.cpu().numpy()[:, pick]
    status = env.status.cpu().numpy()[pick]
    x_ref = x0[pick][:, IDX9].copy() if a["x_ref"] is None else a["x_ref"][pick]
    track = list(a["track"] or range(9))
    off = np.zeros((B, 3)) if a["u0"] is None else a["u0"][pick]
    x0, u0 = x0[pick], u0[pick]
    x, u = x0.copy(), u0.copy()
    live = np.ones(B, dtype=bool)
    compared = 0
    outside = lambda xb: oracle.lib.f16o_envelope_bits(np.ascontiguousarray(xb).ctypes.data_as(ctypes.c_void_p)) != 0
    for t in range(T):
        for b in np.flatnonzero(live):
            if outside(x[b]):                 # env.py:117-124 at the start of the step: frozen, no gain, no command
                live[b] = False
                continue
            A_, B_, C_, D_ = oracle.linearise_na(x[b], u3=u[b, 1:], xcg=xcg)
            Ad, Bd, Cd, _ = mo.c2d(A_, B_, C_, D_, 0.001)
            Q = C_.T @ C_ if a["Q"] is None else a["Q"]
            R = np.eye(3) if a["R"] is None else a["R"]
            Kd = mo.dlqr(Ad, Bd, Q, R)
            assert np.abs(-Kt[t, b] - Kd).max() / np.abs(Kd).max() < 1e-5, (t, b)
            e = np.zeros(9)
            e[track] = x[b, IDX9][track] - x_ref[b][track]
            u[b, 1:4] = -Kd @ e + off[b]
            assert np.abs(ut[t, :, b] - u[b, 1:4]).max() < 2e-5, (t, b)
        xn, _, st = oracle.rollout(x[live], u[live], 1, xcg=xcg, store=False)
        assert not (st & ENVELOPE).any()
        x[live] = xn
        if (t + 1) % 10 == 0:
            for b in np.flatnonzero(live):
                assert rel(traj[t, :, b], x[b]) < 1e-6, (t, b)
                compared += 1
    assert compared >= 5 * B, compared
    assert np.array_equal((status & ENVELOPE) != 0, ~live)


def test_bit_for_bit_properties():
    """60 + 40 steps (u carried in place) == 100 steps; two identical calls agree; an aircraft frozen on entry is left untouched
    (x, u, status; held command, zero gain); aircraft 0, 1234, 4095 of a 4096 batch == the same aircraft alone."""
    B = 4096
    x0, u0 = workload(B)
    Q, R = np.eye(9), np.eye(3) * 1e4

    def run(rows, n, parts=None, status=None):
        env = make_env(x0[rows], u0[rows], xcg=0.25)
        if status is not None:
            env.status.copy_(torch.as_tensor(status, device="cuda:0"))
        xr = x0[rows][:, IDX9]
        outs = [env.rollout_LQR_relin(p, x_ref=xr, Q=Q, R=R, traj_every=p, gains_every=p) for p in (parts or (n,))]
        return env, outs[-1]

    s256 = slice(0, 256)
    env_a, _ = run(s256, 100)
    env_b, _ = run(s256, 100, parts=(60, 40))
    env_c, _ = run(s256, 100)
    for e in (env_b, env_c):
        assert torch.equal(e._x, env_a._x) and torch.equal(e._u, env_a._u) and torch.equal(e.status, env_a.status)
    st = np.zeros(256, dtype=np.int32)
    st[5] = ENVELOPE
    env_f, (_, ut, Kt) = run(s256, 20, status=st)
    assert torch.equal(env_f._x[:, 5], torch.as_tensor(x0[5], device="cuda:0"))
    assert torch.equal(env_f._u[:, 5], torch.as_tensor(u0[5], device="cuda:0"))
    assert int(env_f.status[5]) == ENVELOPE
    assert torch.equal(ut[-1, :, 5], torch.as_tensor(u0[5, 1:4], device="cuda:0")) and float(Kt[-1, 5].abs().max()) == 0.0
    env_big, _ = run(slice(0, B), 20)
    for b in (0, 1234, 4095):
        env_one, _ = run(slice(b, b + 1), 20)
        assert torch.equal(env_one._x[:, 0], env_big._x[:, b]) and torch.equal(env_one._u[:, 0], env_big._u[:, b]), b
        assert int(env_one.status[0]) == int(env_big.status[b]), b


def test_python_surface_and_argument_checks():
    """rollout_LQR(relinearise=True) == rollout_LQR_relin with track = (4, 5, 6) bit for bit; rollout_LQR without the flag still
    equals f16_rollout_lqr; the argument checks of f16_rollout_lqr_relin return F16_EINVAL."""
    from f16_mpc_oop_py_amd import lib
    B, T = 128, 30
    x0, u0 = workload(B)
    e1 = make_env(x0, u0, xcg=0.25)
    tr1 = e1.rollout_LQR(T, *DEM, traj_every=10, relinearise=True)
    e2 = make_env(x0, u0, xcg=0.25)
    xr = np.zeros((B, 9))
    xr[:, 4:7] = DEM
    tr2, _, _ = e2.rollout_LQR_relin(T, x_ref=xr, track=(4, 5, 6), u0=u0[:, 1:4], traj_every=10)
    assert torch.equal(tr1, tr2) and torch.equal(e1._x, e2._x) and torch.equal(e1._u, e2._u) and torch.equal(e1.status, e2.status)
    with pytest.raises(ValueError):
        e1.rollout_LQR(T, *DEM, K=torch.zeros((B, 3, 9)), relinearise=True)
    # the frozen-gain loop is unchanged
    e3, e4 = make_env(x0, u0, xcg=0.25), make_env(x0, u0, xcg=0.25)
    K = e3._calc_LQR_gain()
    e3.rollout_LQR(T, *DEM, K=K)
    Ks = K.reshape(B, 27).t().contiguous()
    dem = e4._demands(*DEM)
    u0s = e4._u.clone()
    assert e4.lib.f16_rollout_lqr(e4.ctx.handle, vp(e4._x), vp(u0s), vp(Ks), vp(dem), None, vp(e4._u), vp(e4.status), B, B, T, 1,
                                  e4.dt, e4.xcg, e4.fi_flag, e4.flags, None) == 0
    assert torch.equal(e3._x, e4._x) and torch.equal(e3._u, e4._u)
    # F16_EINVAL
    L, h = e2.lib, e2.ctx.handle
    x, u = e2._x.clone(), e2._u.clone()
    xrs = torch.zeros((9, B), dtype=torch.float64, device="cuda:0")

    def call(x=x, u=u, B=B, ld=B, n=10, k=1, eps=1e-5, xref=xrs, mask=0x1FF):
        return L.f16_rollout_lqr_relin(h, vp(x), vp(u), vp(xref), None, None, None, None, None, None, B, ld, n, k, mask, eps, 0.001,
                                       0.25, 1, 0, None)
    assert call() == 0
    for bad in (dict(x=None), dict(u=None), dict(ld=B - 1), dict(n=0), dict(n=10, k=3), dict(k=0), dict(eps=0.0),
                dict(eps=-1e-5), dict(xref=None)):
        assert call(**bad) == F16_EINVAL, bad
