"""GPU tests of the scheduled rollouts: f16_rollout_sched / f16_rollout_lqr_sched through the C-ABI, and F16Batch.rollout_schedule /
rollout_LQR(hold=) on top of them.

Contract (include/f16_hip.h): one scheduled launch equals the chain of f16_rollout (f16_rollout_lqr) launches, one per segment with
that segment's row -- bit for bit for any hold at B <= 16,384 and under F16_FLAG_ONE_LANE, for hold % 32 == 0 beyond; other holds on
the large-batch kernels within the 1e-12 relative of split launches.  Fixture G17 is the reference's own loops under inputs that
change during the run (tools/make_golden.py: g17_input_schedules); tolerances SURVEY.md 8(d): 1e-8 relative for xcg 0.25, 1e-6 for
0.35; 1e-9 against the restatement over 100 steps as test_random_batches_vs_oracle."""
import ctypes

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

# one B per kernel family, as test_random_batches_vs_oracle lists them: quad (1, 15, 65, 4096), two-group quad (8000: a ragged
# tail), 4-wave (12000), one-lane 128 / 256 lanes (20000, 70000), 512 lanes on the integer image (140000); lofi 64 and 512 lanes
SIZES = [(1, 1), (15, 1), (65, 1), (4096, 1), (8000, 1), (12000, 1), (20000, 1), (70000, 1), (140000, 1), (4096, 0), (140000, 0)]
SIGN = np.array([0, 1, 1, -1, -1, 0, 0, 0, 0, 0.0])           # the doublet of Nguyen_m/runF16Sim.m per segment


def rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


def bits(a, b):
    """bit-for-bit equality of two fp64 / int32 tensors (NaNs included)"""
    import torch
    v = torch.int64 if a.dtype == torch.float64 else a.dtype
    return a.shape == b.shape and bool((a.contiguous().view(v) == b.contiguous().view(v)).all())


def make_env(x, u=None, **kw):
    from f16_mpc_oop_py_amd import F16Batch
    return F16Batch(x, u, device="cuda:0", **kw)


def doublet_rows(u0, S, seed=7, lqr=False):
    """[S, B, 4] commands u0 + s_k d (d per aircraft: thrust U[-500, 500] lb, each surface U[-1, 1] deg), or [S, B, 3] demands s_k d
    (d U[-0.1, 0.1] rad/s)"""
    rng = np.random.default_rng(seed)
    B = len(u0)
    d = rng.uniform([-500, -1, -1, -1], [500, 1, 1, 1], (B, 4))
    s = SIGN[np.arange(S) % len(SIGN)]
    if lqr:
        return s[:, None, None] * rng.uniform(-0.1, 0.1, (B, 3))[None]
    return u0[None] + s[:, None, None] * d[None]


class Dev:
    """the C-ABI on state-major device tensors"""

    def __init__(self):
        import torch
        from f16_mpc_oop_py_amd import lib
        self.t, self.L = torch, lib.load()
        self.ctx = lib.Context(0)

    def soa(self, a, ld=None):
        """[B, k] host -> [k, ld] device (columns beyond B hold NaN: nothing may read them)"""
        a = np.asarray(a, dtype=np.float64)
        out = self.t.full((a.shape[1], ld or a.shape[0]), float("nan"), dtype=self.t.float64, device="cuda:0")
        out[:, :a.shape[0]] = self.t.as_tensor(a.T.copy(), device="cuda:0")
        return out

    def seq(self, rows, ld=None):
        """[S, B, k] host -> [S, k, ld] device"""
        rows = np.asarray(rows, dtype=np.float64)
        out = self.t.full((rows.shape[0], rows.shape[2], ld or rows.shape[1]), float("nan"), dtype=self.t.float64, device="cuda:0")
        out[:, :, :rows.shape[1]] = self.t.as_tensor(rows.transpose(0, 2, 1).copy(), device="cuda:0")
        return out

    @staticmethod
    def p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def run(self, x0, rows, nsteps, hold, every=None, *, chain=False, fi=1, xcg=0.25, flags=0, ld=None, K=None, u0=None, status0=None,
            stream=None):
        """One scheduled launch (chain=False) or the chain of constant-input launches it stands for, rows [S, B, 4] commands or
        (with K [27, ld] and u0 [B, 4]) [S, B, 3] demands.  -> x [18, ld], traj [nsteps / every, 18, ld] or None, status [ld],
        u_out [4, ld] (LQR)"""
        t, L, p = self.t, self.L, self.p
        B = len(x0)
        ld = ld or B
        x = self.soa(x0, ld)
        sq = rows if t.is_tensor(rows) else self.seq(rows, ld)
        st = t.zeros(ld, dtype=t.int32, device="cuda:0") if status0 is None else status0.clone()
        traj = t.full((nsteps // every, 18, ld), float("nan"), dtype=t.float64, device="cuda:0") if every else None
        lqr = K is not None
        u0d = self.soa(u0, ld) if lqr else None
        uo = t.full((4, ld), float("nan"), dtype=t.float64, device="cuda:0") if lqr else None
        if not chain:
            if lqr:
                rc = L.f16_rollout_lqr_sched(self.ctx.handle, p(x), p(u0d), p(K), p(sq), p(traj), p(uo), p(st), B, ld, nsteps, hold,
                                             every or 1, 0.001, xcg, fi, flags, stream)
            else:
                rc = L.f16_rollout_sched(self.ctx.handle, p(x), p(sq), p(traj), p(st), B, ld, nsteps, hold, every or 1, 0.001, xcg, fi,
                                         flags, stream)
            assert rc == 0, L.f16_last_error()
        else:
            # one launch per segment with that segment's row; its samples go where they fall.  With `every` not a divisor of
            # `hold` a segment's launch cannot store them, so the chain is then cut at every sample as well (per_segment=False)
            fine = bool(every) and hold % every != 0
            cuts = sorted(set(range(0, nsteps, hold)) | (set(range(0, nsteps, every)) if fine else set()) | {nsteps})
            for a, b in zip(cuts[:-1], cuts[1:]):
                row = sq[a // hold]
                if fine:
                    tr, k = (traj[b // every - 1] if b % every == 0 else None), b - a
                else:
                    tr, k = (traj[a // every:b // every] if every else None), every or b - a
                if lqr:
                    rc = L.f16_rollout_lqr(self.ctx.handle, p(x), p(u0d), p(K), p(row), p(tr), p(uo), p(st), B, ld, b - a, k, 0.001,
                                           xcg, fi, flags, stream)
                else:
                    rc = L.f16_rollout(self.ctx.handle, p(x), p(row), p(tr), p(st), B, ld, b - a, k, 0.001, xcg, fi, flags, stream)
                assert rc == 0, L.f16_last_error()
        t.cuda.synchronize()
        return x, traj, st, uo


@pytest.fixture(scope="module")
def dev(hip):
    return Dev()


def lqr_gain(x0, u0, fi, xcg):
    env = make_env(x0, u0, xcg=xcg, fi_flag=fi)
    return env._calc_LQR_gain().reshape(len(x0), 27).t().contiguous()      # [27, B]


def same(a, b, B):
    """final state, every stored sample, status (and u_out) of two runs, bit for bit over the B aircraft"""
    for s, c in zip(a, b):
        if s is not None and not bits(s[..., :B], c[..., :B]):
            return False
    return True


# ------------------------------------------------------------------------------------------------ G17 on the device
@pytest.mark.parametrize("xcg,tol", [(25, 1e-8), (35, 1e-6)])
def test_g17_the_reference_loops_under_changing_inputs(dev, xcg, tol):
    g, g12 = golden("g17_input_schedules.npz"), golden("g12_lqr_loop.npz")
    x0 = g[f"x0_xcg{xcg}"]
    for name, hold, n in (("doublet", 100, 1000), ("sin", 1, 300)):
        rows = g[f"{name}_u_xcg{xcg}"]
        x, traj, st, _ = dev.run(x0, rows, n, hold, 25, xcg=xcg / 100)
        err = rel(traj.cpu().numpy().transpose(2, 0, 1), g[f"{name}_traj_xcg{xcg}"])
        print(f"G17 {name} xcg {xcg}: C-ABI {err:.3e}")
        assert err < tol and int(st.max()) == 0
        env = make_env(x0, g[f"u0_xcg{xcg}"], xcg=xcg / 100)                      # and through F16Batch
        tr = env.rollout_schedule(rows, hold=hold, traj_every=25)
        assert bits(tr, traj) and bits(env._x, x) and int(env.status.max()) == 0
        assert np.array_equal(env.u_values.cpu().numpy(), rows[-1])               # u.values = the last action
    K, u0 = g12[f"K_xcg{xcg}"], g12[f"u0_xcg{xcg}"]
    dem = g["dem_rows"].transpose(1, 0, 2)                                        # [6 rows, 6 cases, 3]
    Kd = dev.soa(np.tile(K.reshape(1, 27), (6, 1)))
    x, traj, st, uo = dev.run(g12[f"x0_xcg{xcg}"], dem, 300, 50, 25, xcg=xcg / 100, K=Kd, u0=np.tile(u0, (6, 1)))
    err = rel(traj.cpu().numpy().transpose(2, 0, 1), g[f"lqr_traj_xcg{xcg}"])
    erru = rel(uo.t().cpu().numpy(), g[f"lqr_u_last_xcg{xcg}"])
    print(f"G17 lqr xcg {xcg}: states {err:.3e} last action {erru:.3e}")
    assert err < tol and erru < tol and int(st.max()) == 0
    env = make_env(g12[f"x0_xcg{xcg}"], np.tile(u0, (6, 1)), xcg=xcg / 100)
    tr = env.rollout_LQR(300, dem[:, :, 0], dem[:, :, 1], dem[:, :, 2], K=np.tile(K, (6, 1, 1)), traj_every=25, hold=50)
    assert bits(tr, traj) and bits(env._u, uo) and int(env.status.max()) == 0


# ------------------------------------------------------------------------------------------------ chain equivalence
@pytest.mark.parametrize("B,fi", SIZES)
@pytest.mark.parametrize("lqr", [False, True], ids=["open", "lqr"])
def test_one_scheduled_launch_equals_the_chain_of_launches(dev, B, fi, lqr):
    from f16_mpc_oop_py_amd.lib import F16_FLAG_ONE_LANE
    from f16_mpc_oop_py_amd.workload import config2_states
    x0, u0 = config2_states(B, seed=B)
    xcg = 0.35 if lqr else 0.25
    kw = dict(fi=fi, xcg=xcg)
    if lqr:
        kw.update(K=lqr_gain(x0, u0, fi, xcg), u0=u0)
    cases = [(128, 32, 32, 0, True)]                                  # T, hold, traj_every, flags, bit for bit
    cases.append((200, 20, 20, 0, B <= 16384))
    if B == 20000:
        cases.append((200, 20, 20, F16_FLAG_ONE_LANE, True))
    for T, hold, every, flags, exact in cases:
        rows = doublet_rows(u0, T // hold, lqr=lqr)
        one = dev.run(x0, rows, T, hold, every, flags=flags, **kw)
        chn = dev.run(x0, rows, T, hold, every, flags=flags, chain=True, **kw)
        if exact:
            assert same(one, chn, B), (T, hold, flags)
        else:
            # the large-batch kernels carry their sin / cos pairs through other steps than the chain's launches: 1e-12 relative
            # over 100 steps (include/f16_hip.h, split launches); compared where both runs kept integrating
            assert bits(one[2], chn[2])
            ok = (one[2] == 0).cpu().numpy()
            err = rel(one[0].t().cpu().numpy()[ok], chn[0].t().cpu().numpy()[ok])
            errm = rel(one[1][4].t().cpu().numpy()[ok], chn[1][4].t().cpu().numpy()[ok])      # the sample after 100 steps
            print(f"B {B} fi {fi} lqr {lqr} hold 20: one launch vs chain {errm:.3e} after 100 steps, {err:.3e} after 200")
            assert errm < 1e-12
        if not lqr and fi == 1 and B in (4096, 8000, 20000):
            assert int(one[2].max()) == 0                             # (checked on the CPU restatement: none of them leaves the envelope)
        # the schedule is used: held inputs end somewhere else
        held = dev.run(x0, rows[:1], T, T, None, flags=flags, **kw)
        assert not bits(held[0], one[0])


@pytest.mark.parametrize("seed", [4096, 20261003])
def test_config2_batch_under_the_doublet_raises_no_status_bit(dev, seed):
    from f16_mpc_oop_py_amd.workload import config2_states
    x0, u0 = config2_states(4096, seed=seed)
    for T, hold in ((1000, 100), (200, 20), (128, 32)):
        _, _, st, _ = dev.run(x0, doublet_rows(u0, T // hold), T, hold)
        assert int(st.max()) == 0


@pytest.mark.parametrize("B,fi", SIZES)
def test_scheduled_rollout_vs_the_restatement_chained_per_segment(dev, oracle, B, fi):
    from f16_mpc_oop_py_amd.workload import config2_states
    x0, u0 = config2_states(B, seed=B)
    rows = doublet_rows(u0, 5)
    x, _, st, _ = dev.run(x0, rows, 100, 20, fi=fi)
    idx = np.arange(0, B, max(1, B // 2048))[:2048]
    xr = x0[idx]
    for r in range(5):
        xr, _, so = oracle.rollout(xr, rows[r][idx], 20, fi_flag=fi, store=False, nthreads=16)
        assert not np.asarray(so).any()
    err = rel(x.t().cpu().numpy()[idx], xr)
    print(f"B {B} fi {fi}: scheduled launch vs chained restatement, 100 steps hold 20: {err:.3e}")
    assert err < 1e-9 and int(st.max()) == 0


# ------------------------------------------------------------------------------------------------ degenerate schedules
@pytest.mark.parametrize("B,fi", [(65, 1), (8000, 1), (12000, 1), (20000, 1), (140000, 1), (4096, 0)])
def test_degenerate_schedules(dev, B, fi):
    import torch
    from f16_mpc_oop_py_amd.workload import config2_states
    x0, u0 = config2_states(B, seed=B)
    rows = doublet_rows(u0, 7)
    # hold >= nsteps reads row 0 only (the rows behind it are not even there) == f16_rollout
    ref = dev.run(x0, rows[1:2], 64, 64, 16, chain=True, fi=fi)
    assert same(dev.run(x0, rows[1:2], 64, 64, 16, fi=fi), ref, B)
    assert same(dev.run(x0, rows[1:2], 64, 1000, 16, fi=fi), ref, B)
    # S identical rows == f16_rollout, whatever the hold.  (One exception, by the contract's own rule: the 64-lane lofi kernel of
    # B <= 16,384 restarts its carried sin / cos pairs with every row, as the chain of launches does -- there a hold that is not a
    # multiple of 32 gives the chain's bits, which f16_rollout's own split launches differ from by <= 1e-12.)
    for hold in (1, 7, 32):
        one = dev.run(x0, np.repeat(rows[1:2], (64 + hold - 1) // hold, 0), 64, hold, 16, fi=fi)
        if fi == 0 and B <= 16384 and hold % 32:
            seg = dev.run(x0, np.repeat(rows[1:2], (64 + hold - 1) // hold, 0), 64, hold, None, fi=fi, chain=True)
            assert bits(one[0], seg[0]) and bits(one[2], seg[2]), hold
            assert bits(one[2], ref[2]) and rel(one[1].cpu().numpy(), ref[1].cpu().numpy()) < 1e-12
        else:
            assert same(one, ref, B), hold
    # nsteps not a multiple of hold (the last segment is shorter), traj_every not a divisor of hold.  The final state against the
    # chain of one launch per segment; the samples against a chain that is cut at every sample too -- bit for bit where no sin / cos
    # pair is carried (hifi, B <= 16,384), else within the 1e-12 of split launches
    for T, hold, every in ((70, 32, 35), (96, 32, 24), (50, 20, 5)):
        one = dev.run(x0, rows, T, hold, every, fi=fi)
        seg = dev.run(x0, rows, T, hold, None, fi=fi, chain=True)
        chn = dev.run(x0, rows, T, hold, every, fi=fi, chain=True)
        if B <= 16384 or hold % 32 == 0:
            assert bits(one[0], seg[0]) and bits(one[2], seg[2]), (T, hold, every)
        if B <= 16384 and (fi == 1 or hold % every == 0):
            assert same(one, chn, B), (T, hold, every)
        else:
            assert bits(one[2], chn[2]) and rel(one[0].t().cpu().numpy(), chn[0].t().cpu().numpy()) < 1e-12
            assert rel(one[1].cpu().numpy(), chn[1].cpu().numpy()) < 1e-12
    # ld > B: nothing beyond column B is read (NaN there) or written
    ld = B + 37
    one = dev.run(x0, rows, 64, 32, 32, fi=fi, ld=ld)
    assert same(one, dev.run(x0, rows, 64, 32, 32, fi=fi), B)
    assert bool(torch.isnan(one[0][:, B:]).all()) and bool(torch.isnan(one[1][:, :, B:]).all()) and int(one[2][B:].abs().max()) == 0


# ------------------------------------------------------------------------------------------------ freeze and NaN
def near_the_ground(x, alt):
    """a start that is already near a bound: a shallow dive (theta - 0.1 rad, about 70 ft/s down) `alt` ft above the zero-altitude
    bound of env.py:117-124 -- checked on the CPU restatement: from 2.5 ft it is outside after step 36, from 4.0 ft after step 58"""
    x = x.copy()
    x[2], x[4] = alt, x[4] - 0.1
    return x


@pytest.mark.parametrize("B", [40, 6000, 12000, 40000])
def test_freeze_mid_schedule_and_nan_rows_as_the_chain(dev, B):
    """quad, two-group quad, 4-wave and one-lane kernels: an aircraft that leaves the envelope during the second segment is
    frozen at the same step with the same bits as the chain and ignores the rows that follow; NaN / infinite rows give what the
    chain gives."""
    from f16_mpc_oop_py_amd.lib import F16_ST, F16_ST_ENV_STATE
    g = golden("g567_trim_lin_lqr.npz")
    x0 = np.tile(g["trim_x_xcg25"], (B, 1))
    u0 = x0[:, 12:16].copy()
    x0[5], x0[B - 1] = near_the_ground(x0[5], 2.5), near_the_ground(x0[B - 1], 4.0)
    rows = np.tile(u0, (4, 1, 1))
    rows[1:, 5, 1] += 10.0                             # (the elevator row changes WHERE it ends up, a few 1e-5 ft)
    rows[1:, B - 1, 1] -= 10.0
    rows[3, 7] = np.nan                                # a NaN row for one aircraft (fixture G3b: through the actuator models)
    rows[2, 9, 2] = np.inf
    one = dev.run(x0, rows, 128, 32, 1)                # (hold 32: bit for bit on every kernel)
    chn = dev.run(x0, rows, 128, 32, 1, chain=True)
    assert same(one, chn, B)
    st = one[2].cpu().numpy()
    out = F16_ST["ENVELOPE"] | F16_ST_ENV_STATE(2)
    assert st[5] == out and st[B - 1] == out and st[0] == 0
    tr = one[1].cpu().numpy()                          # [128, 18, B]
    for b in (5, B - 1):
        at = int(np.argmax(tr[:, 2, b] < 0))           # first sample outside, in the second segment: every later one equals it
        assert 32 <= at < 64 and np.array_equal(tr[at:, :, b], np.tile(tr[at, :, b], (128 - at, 1)))
        assert np.array_equal(one[0].cpu().numpy()[:, b], tr[at, :, b])
    held = dev.run(x0, rows[:1], 128, 128, 1)
    assert not np.array_equal(held[0].cpu().numpy()[:, 5], one[0].cpu().numpy()[:, 5])       # the row did act before the freeze


@pytest.mark.parametrize("B", [40, 6000, 12000, 40000])
def test_lqr_freeze_mid_schedule_as_the_chain(dev, B):
    from f16_mpc_oop_py_amd.lib import F16_ST, F16_ST_ENV_STATE
    g = golden("g12_lqr_loop.npz")
    x0 = np.tile(g["x0_xcg25"][0], (B, 1))
    x0[5], x0[B - 1] = near_the_ground(x0[5], 2.5), near_the_ground(x0[B - 1], 4.0)
    u0 = np.tile(g["u0_xcg25"], (B, 1))
    K = dev.soa(np.tile(g["K_xcg25"].reshape(1, 27), (B, 1)))
    dem = np.zeros((4, B, 3))
    dem[1:, :, 1] = 0.5
    dem[2, 7] = np.nan
    one = dev.run(x0, dem, 80, 20, 4, K=K, u0=u0)
    chn = dev.run(x0, dem, 80, 20, 4, K=K, u0=u0, chain=True)
    assert same(one, chn, B)
    st = one[2].cpu().numpy()
    assert st[5] == st[B - 1] == F16_ST["ENVELOPE"] | F16_ST_ENV_STATE(2) and st[0] == 0
    # a frozen aircraft's last launch of the chain never steps: u_out is u0 there, and so it is here
    assert np.array_equal(one[3].cpu().numpy()[:, 5], u0[5])


# ------------------------------------------------------------------------------------------------ split calls
@pytest.mark.parametrize("B,fi", [(4096, 1), (8000, 1), (20000, 1), (140000, 1), (4096, 0)])
def test_a_schedule_cut_at_a_segment_boundary_equals_one_call(dev, B, fi):
    from f16_mpc_oop_py_amd.workload import config2_states
    x0, u0 = config2_states(B, seed=B)
    for T, hold, cut in ((128, 32, 2), (200, 20, 3)):
        rows = doublet_rows(u0, T // hold)
        one = dev.run(x0, rows, T, hold, hold, fi=fi)
        a = dev.run(x0, rows[:cut], cut * hold, hold, hold, fi=fi)
        b = dev.run(a[0].t().cpu().numpy()[:B], rows[cut:], T - cut * hold, hold, hold, fi=fi, status0=a[2])
        if hold % 32 == 0 or B <= 16384:
            assert bits(one[0], b[0]) and bits(one[2], b[2]) and bits(one[1][:cut], a[1]) and bits(one[1][cut:], b[1])
        else:
            assert bits(one[2], b[2]) and rel(one[1][4].cpu().numpy(), b[1][4 - cut].cpu().numpy()) < 1e-12


# ------------------------------------------------------------------------------------------------ G10 as one launch per xcg group
def test_g10_time_histories_as_one_launch_per_xcg_group(dev):
    import torch
    from conftest import G10_OUT_TOL, G10_TOL, g10_case, g10_command, g10_rows_of_states
    from f16_mpc_oop_py_amd.lib import F16_FLAG_FIX_CLR
    for xcg_sel, ks in ((0.30, (0, 1, 2)), (0.25, (3,))):
        cases = [g10_case(k) for k in ks]
        x0 = np.array([c[2] for c in cases])
        rows = np.array([[g10_command(c[3], c[4], j) for c in cases] for j in range(100)])       # [100, B, 4]
        env = make_env(x0, rows[0], xcg=xcg_sel, flags=F16_FLAG_FIX_CLR)
        traj = env.rollout_schedule(rows, hold=100, traj_every=100)                                # ONE launch: 10,000 steps
        assert tuple(traj.shape) == (100, 18, len(ks)) and int(env.status.max()) == 0
        loop = make_env(x0, rows[0], xcg=xcg_sel, flags=F16_FLAG_FIX_CLR)                          # the 100-launch loop it replaces
        tl = torch.empty_like(traj)
        for j in range(100):
            loop._u.copy_(torch.as_tensor(rows[j].T.copy(), device="cuda:0"))
            loop.rollout(100)
            tl[j] = loop._x
        assert bits(traj, tl) and bits(env._x, loop._x) and bits(env._u, loop._u)
        hist = np.concatenate((x0[None], traj.permute(0, 2, 1).cpu().numpy()))                     # [101, B, 18]
        for b, (a, *_r) in enumerate(cases):
            err = np.abs(g10_rows_of_states(hist[:, b]) - a[:, 1:13]).max(0)
            assert np.all(err < G10_TOL), (ks[b], err)
            assert np.abs(hist[:, b, 13:16] - a[:, 20:23]).max() < 2e-3
        outs = np.array([env.nlplant(torch.as_tensor(hist[t], device="cuda:0")).cpu().numpy()[:, 12:18] for t in range(0, 101, 10)])
        for b, (a, *_r) in enumerate(cases):
            assert np.all(np.abs(outs[:, b] - a[::10, 13:19]).max(0) < G10_OUT_TOL)


# ------------------------------------------------------------------------------------------------ arguments, Python surface
def test_argument_errors(dev):
    L, h = dev.L, dev.ctx.handle
    assert L.f16_rollout_sched(h, 1, 1, None, None, 4, 4, 10, 0, 1, 0.001, 0.25, 1, 0, None) == -1        # hold < 1
    assert b"hold" in L.f16_last_error()
    assert L.f16_rollout_sched(h, 1, None, None, None, 4, 4, 10, 1, 1, 0.001, 0.25, 1, 0, None) == -1     # u_seq NULL
    assert L.f16_rollout_sched(h, None, 1, None, None, 4, 4, 10, 1, 1, 0.001, 0.25, 1, 0, None) == -1     # x NULL
    assert L.f16_rollout_sched(h, 1, 1, None, None, 4, 2, 10, 1, 1, 0.001, 0.25, 1, 0, None) == -1        # ld < B
    assert L.f16_rollout_sched(h, 1, 1, 1, None, 4, 4, 10, 1, 3, 0.001, 0.25, 1, 0, None) == -1           # traj_every does not divide
    assert L.f16_rollout_sched(h, 1, 1, None, None, 4, 4, -1, 1, 1, 0.001, 0.25, 1, 0, None) == -1        # nsteps < 0
    assert L.f16_rollout_sched(h, 1, 1, None, None, 0, 0, 10, 1, 1, 0.001, 0.25, 1, 0, None) == 0         # B = 0: no-op
    assert L.f16_rollout_sched(h, 1, 1, None, None, 4, 4, 0, 1, 1, 0.001, 0.25, 1, 0, None) == 0          # nsteps = 0: no-op
    assert L.f16_rollout_lqr_sched(h, 1, 1, 1, 1, None, None, None, 4, 4, 10, 0, 1, 0.001, 0.25, 1, 0, None) == -1    # hold < 1
    assert L.f16_rollout_lqr_sched(h, 1, 1, 1, None, None, None, None, 4, 4, 10, 1, 1, 0.001, 0.25, 1, 0, None) == -1  # dem_seq NULL
    assert L.f16_rollout_lqr_sched(h, 1, 1, None, 1, None, None, None, 4, 4, 10, 1, 1, 0.001, 0.25, 1, 0, None) == -1  # K NULL
    assert L.f16_rollout_lqr_sched(h, 1, None, 1, 1, None, None, None, 4, 4, 10, 1, 1, 0.001, 0.25, 1, 0, None) == -1  # u0 NULL


def test_python_surface(dev):
    import torch
    from f16_mpc_oop_py_amd.workload import config2_states
    B = 300
    x0, u0 = config2_states(B, seed=3)
    rows = doublet_rows(u0, 6)
    ref = dev.run(x0, rows, 60, 10, 5)
    for form in ("numpy", "torch_host", "torch_device", "state_major"):
        env = make_env(x0, u0)
        a = {"numpy": rows, "torch_host": torch.as_tensor(rows), "torch_device": torch.as_tensor(rows, device="cuda:0"),
             "state_major": torch.as_tensor(rows.transpose(0, 2, 1).copy(), device="cuda:0")}[form]
        traj = env.rollout_schedule(a, hold=10, traj_every=5)
        assert tuple(traj.shape) == (12, 18, B) and bits(traj, ref[1]) and bits(env._x, ref[0]) and bits(env.status, ref[2]), form
        assert np.array_equal(env.u_values.cpu().numpy(), rows[5])
    env = make_env(x0, u0)
    assert env.rollout_schedule(rows, hold=10, nsteps=35) is None               # a shorter run: rows 0..3, the last segment cut
    assert np.array_equal(env.u_values.cpu().numpy(), rows[3]) and bits(env._x, dev.run(x0, rows, 35, 10)[0])
    env = make_env(x0, u0)
    env.rollout_schedule(rows)                                                   # hold = 1: six steps
    assert bits(env._x, dev.run(x0, rows, 6, 1)[0])
    with pytest.raises(ValueError):
        env.rollout_schedule(rows, hold=0)
    with pytest.raises(ValueError):
        env.rollout_schedule(rows, hold=10, nsteps=61)                           # needs seven rows
    with pytest.raises(ValueError):
        env.rollout_schedule(rows[:, :10])                                       # wrong batch
    with pytest.raises(ValueError):
        env.rollout_schedule(rows[0])                                            # not 3-D
    with pytest.raises(ValueError):
        env.rollout_schedule(rows, hold=10, traj_every=7)
    # rollout_LQR: histories [S] and [S, B] with scalars broadcast; constant demands keep the constant-input call
    env = make_env(x0, u0, xcg=0.35)
    K = env._calc_LQR_gain()
    p = np.linspace(-0.05, 0.05, 4)
    q = np.random.default_rng(5).uniform(-0.05, 0.05, (4, B))
    dem = np.stack((np.tile(p[:, None], (1, B)), q, np.full((4, B), 0.01)), -1)                       # [4, B, 3]
    refl = dev.run(x0, dem, 40, 10, 10, xcg=0.35, K=K.reshape(B, 27).t().contiguous(), u0=np.concatenate((u0[:, :1], u0[:, 1:]), 1))
    traj = env.rollout_LQR(40, p, q, 0.01, K=K, traj_every=10, hold=10)
    assert bits(traj, refl[1]) and bits(env._x, refl[0]) and bits(env._u, refl[3])
    envc = make_env(x0, u0, xcg=0.35)
    envd = make_env(x0, u0, xcg=0.35)
    envc.rollout_LQR(40, 0.02, q[0], 0.01, K=K)                                                      # scalar / [B]: f16_rollout_lqr
    envd.rollout_LQR(40, np.full(1, 0.02), q[:1], 0.01, K=K, hold=40)                                # the same as a one-row history
    assert bits(envc._x, envd._x) and bits(envc._u, envd._u)
    with pytest.raises(ValueError):
        env.rollout_LQR(40, p, q, 0.01, K=K, hold=10, linear=True)
    with pytest.raises(ValueError):
        env.rollout_LQR(40, p, q, 0.01, hold=10, relinearise=True)
    with pytest.raises(ValueError):
        env.rollout_LQR(41, p, q, 0.01, K=K, hold=10)                            # needs five rows
    with pytest.raises(ValueError):
        env.rollout_LQR(40, p, q[:3], 0.01, K=K, hold=10)                        # histories of different length
    with pytest.raises(ValueError):
        env.rollout_LQR(40, 0.0, 0.0, 0.0, K=K, hold=10)                         # hold without a history


# ------------------------------------------------------------------------------------------------ stream capture
def test_scheduled_rollout_replays_from_a_captured_graph(dev):
    """The entry point allocates nothing: one f16_rollout_sched call captured into a graph and replayed twice from the same start
    gives the direct call's result."""
    import torch
    from f16_mpc_oop_py_amd.workload import config2_states
    B = 4096
    x0, u0 = config2_states(B, seed=11)
    rows = doublet_rows(u0, 4)
    ref = dev.run(x0, rows, 64, 16, 16)
    L, p = dev.L, dev.p
    xs, sq = dev.soa(x0), dev.seq(rows)
    x = xs.clone()
    st = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    traj = torch.zeros((4, 18, B), dtype=torch.float64, device="cuda:0")
    call = lambda: L.f16_rollout_sched(dev.ctx.handle, p(x), p(sq), p(traj), p(st), B, B, 64, 16, 16, 0.001, 0.25, 1, 0,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert call() == 0                                  # (the kernel is loaded outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert call() == 0
    for _ in range(2):
        x.copy_(xs); st.zero_(); traj.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert bits(x, ref[0]) and bits(traj, ref[1]) and bits(st, ref[2])
