"""GPU tests of the LQR loop under a gain schedule over (altitude, airspeed): f16_rollout_lqr_gs and f16_debug_gain_lookup through the
C-ABI, F16Batch.rollout_LQR(schedule=) and GainSchedule.build on top of them.

Contract (include/f16_hip.h): split the steps wherever t % gs_every == 0 or t % hold == 0; the one call equals the chain of
f16_rollout_lqr_rk calls, one per segment with that segment's demand row and with K and u0 = [thrust, g[9..11]] of the most recent gain
update as the HOST computes it (GainSchedule.lookup, whose bits are f16_gain_lookup_host's: tests/test_lqr_gs_cpu.py) from the chain's
own state -- bit for bit in the final state, every stored sample, the status and u_out: under F16_FLAG_ONE_LANE, with RK4 at every
size, for lofi, and for hifi Euler above 16,384 aircraft when every segment is a multiple of 32 steps long.

Tables are synthetic unless a test says otherwise: the G7 gain (tests/golden/g567_trim_lin_lqr.npz) scaled per node by
1 + 0.2 U(-1, 1), offsets trim +- 0.5 deg.  States: the G5 trim point plus config-2-style perturbations, xcg 0.25, at most 96 steps.
Cells are small (2 ft x 0.25 ft/s) so that aircraft cross several of them within a run (asserted)."""
import ctypes

import numpy as np
import pytest

from conftest import golden
from gs_cases import lookup_points, same_bits, small_schedule

pytestmark = pytest.mark.gpu

EULER, RK4 = 1, 4
ONE_LANE = 4                                                                   # F16_FLAG_ONE_LANE
ENVELOPE = 16                                                                  # F16_ST_ENVELOPE
DT, XCG = 1e-3, 0.25
H0, DH, NH, V0, DV, NV = 9992.0, 2.0, 8, 699.0, 0.25, 8                        # nodes up to 10,006 ft and 700.75 ft/s


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def bits(a, b):
    """bit-for-bit equality of two fp64 / int32 tensors (NaNs included)"""
    import torch
    v = torch.int64 if a.dtype == torch.float64 else a.dtype
    return a.shape == b.shape and bool((a.contiguous().view(v) == b.contiguous().view(v)).all())


def synthetic_schedule(seed=11, flat=False):
    from f16_mpc_oop_py_amd.schedule import GainSchedule
    from f16_mpc_oop_py_amd.workload import TRIM_XCG25
    rng = np.random.default_rng(seed)
    K = golden("g567_trim_lin_lqr.npz")["K_lqr_xcg25"][:, 4:7].ravel()
    scale, off = 1.0 + 0.2 * rng.uniform(-1, 1, (NH, NV, 1)), rng.uniform(-0.5, 0.5, (NH, NV, 3))
    if flat:
        scale, off = np.broadcast_to(scale[:1, :1], (NH, NV, 1)), np.broadcast_to(off[:1, :1], (NH, NV, 3))
    return GainSchedule(H0, DH, NH, V0, DV, NV, np.concatenate((K * scale, TRIM_XCG25[13:16] + off), 2))


def six_aircraft():
    """crossing cell boundaries in both axes | exactly on a node | below h0 | beyond the last V | frozen on entry | NaN airspeed"""
    from f16_mpc_oop_py_amd.workload import TRIM_XCG25
    rng = np.random.default_rng(5)
    x = np.tile(TRIM_XCG25, (6, 1))
    x[:, 3:6] += rng.uniform(-0.05, 0.05, (6, 3))
    x[:, 7:9] += rng.uniform(-0.02, 0.02, (6, 2))
    x[:, 9:12] += rng.uniform(-0.1, 0.1, (6, 3))
    x[:, 2], x[:, 6] = 9999.3, 700.1
    x[0, 7] += 0.2                                                             # a high angle of attack: it decelerates through the V cells
    x[0, 4] = x[0, 7] + 0.15                                                   # ... and climbs through the h cells
    x[0, 2], x[0, 6] = 9995.3, 700.6
    x[1, 2], x[1, 6] = H0 + 2 * DH, V0 + 2 * DV
    x[2, 2] = H0 - 12.0
    x[3, 6] = V0 + (NV - 1) * DV + 1.25
    x[4, 6] = 950.0
    x[5, 6] = np.nan
    return x


def many_aircraft(B, seed=6):
    """B aircraft around the grid, about a fifth of them outside it, a few frozen on entry or with a NaN airspeed"""
    from f16_mpc_oop_py_amd.workload import TRIM_XCG25
    rng = np.random.default_rng(seed)
    x = np.tile(TRIM_XCG25, (B, 1))
    x[:, 2] = rng.uniform(H0 - 1.0, H0 + (NH - 1) * DH + 1.0, B)
    x[:, 6] = rng.uniform(V0 - 0.1, V0 + (NV - 1) * DV + 0.1, B)
    x[:, 3:6] += rng.uniform(-0.05, 0.05, (B, 3))
    x[:, 7] += rng.uniform(-0.02, 0.15, B)
    x[:, 4] += rng.uniform(-0.1, 0.2, B)
    x[:, 8] += rng.uniform(-0.02, 0.02, B)
    x[:, 9:12] += rng.uniform(-0.1, 0.1, (B, 3))
    x[::997, 6] = 950.0
    x[5::1013, 6] = np.nan
    return x


def demands(S, B, seed=8):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.1, 0.1, (S, 3, B))


class Dev:
    """the C-ABI on state-major device tensors"""

    def __init__(self):
        import torch
        from f16_mpc_oop_py_amd import lib
        self.t, self.L, self.lib = torch, lib.load(), lib
        self.ctx = lib.Context(0)

    def dev(self, a, dtype=None):
        return self.t.as_tensor(np.ascontiguousarray(a), device="cuda:0") if dtype is None else self.t.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")

    @staticmethod
    def p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def buffers(self, x0, nsteps, every, status0=None):
        t, B = self.t, len(x0)
        x = self.dev(np.asarray(x0, dtype=np.float64).T)
        st = t.zeros(B, dtype=t.int32, device="cuda:0") if status0 is None else status0.clone()
        traj = t.full((nsteps // every, 18, B), float("nan"), dtype=t.float64, device="cuda:0") if every else None
        uo = t.full((4, B), float("nan"), dtype=t.float64, device="cuda:0")
        return x, st, traj, uo

    def one(self, gs, x0, dem, nsteps, gs_every, hold, every, method, *, fi=1, flags=0, status0=None, thrust=None):
        """ONE launch of f16_rollout_lqr_gs -> x [18, B], traj, status, u_out [4, B], gs_out [B]"""
        t, L, p = self.t, self.L, self.p
        B = len(x0)
        x, st, traj, uo = self.buffers(x0, nsteps, every, status0)
        u0 = t.full((4, B), float("nan"), dtype=t.float64, device="cuda:0")    # rows 1..3 are not read
        u0[0] = x[12] if thrust is None else thrust
        out = t.full((B,), -1, dtype=t.int32, device="cuda:0")
        g, tab, dm = gs.grid(), gs.device_table("cuda:0"), dem if t.is_tensor(dem) else self.dev(dem)
        rc = L.f16_rollout_lqr_gs(self.ctx.handle, p(x), p(u0), ctypes.byref(g), p(tab), gs_every, p(dm), p(traj), p(uo), p(out), p(st), B, B,
                                  nsteps, hold, every or 1, DT, XCG, fi, method, flags, None)
        assert rc == 0, L.f16_last_error()
        t.cuda.synchronize()
        return x, traj, st, uo, out

    def chain(self, gs, x0, dem, nsteps, gs_every, hold, every, method, *, fi=1, flags=0):
        """The chain the contract names: one f16_rollout_lqr_rk per segment, K and u0 from GainSchedule.lookup (numpy, on the host) at
        the chain's own state at every gain update -> x, traj, status, u_out, the numpy count of updates outside the grid, and the
        cells (ih, iv) every aircraft was looked up in"""
        t, L, p = self.t, self.L, self.p
        B = len(x0)
        x, st, traj, uo = self.buffers(x0, nsteps, every)
        dm = self.dev(dem)
        u0 = t.empty((4, B), dtype=t.float64, device="cuda:0")
        u0[0] = x[12]
        K = t.full((27, B), float("nan"), dtype=t.float64, device="cuda:0")    # the law reads K[:, 4:7] only
        count, cells = np.zeros(B, dtype=np.int32), []
        cuts = sorted(set(range(0, nsteps, gs_every)) | set(range(0, nsteps, hold)) | {nsteps})
        assert not every or all(c % every == 0 for c in cuts)
        for a, b in zip(cuts[:-1], cuts[1:]):
            if a % gs_every == 0:
                h, v = x[2].cpu().numpy(), x[6].cpu().numpy()
                g = gs.lookup(h, v)                                            # [B, 12]
                count += gs.outside(h, v)
                cells.append((gs._axis(h, gs.h0, gs.dh, gs.nh)[0], gs._axis(v, gs.v0, gs.dv, gs.nv)[0]))
                gd = self.dev(g.T)
                for i in range(3):
                    K[9 * i + 4:9 * i + 7] = gd[3 * i:3 * i + 3]
                u0[1:4] = gd[9:12]
            tr = traj[a // every:b // every] if every else None
            rc = L.f16_rollout_lqr_rk(self.ctx.handle, p(x), p(u0), p(K), p(dm[a // hold]), p(tr), p(uo), p(st), B, B, b - a, b - a,
                                      every or 1, DT, XCG, fi, method, flags, None)
            assert rc == 0, L.f16_last_error()
        t.cuda.synchronize()
        return x, traj, st, uo, count, cells


@pytest.fixture(scope="module")
def dev(hip):
    return Dev()


def assert_same(one, chain, what):
    x, traj, st, uo, out = one
    cx, ctraj, cst, cuo, count = chain[:5]
    assert bits(x, cx), f"{what}: final state"
    assert traj is None or bits(traj, ctraj), f"{what}: stored samples"
    assert bits(st, cst), f"{what}: status {st.tolist()[:8]} vs {cst.tolist()[:8]}"
    assert bits(uo, cuo), f"{what}: u_out"
    assert np.array_equal(out.cpu().numpy(), count), f"{what}: gs_out {out.tolist()[:8]} vs {count.tolist()[:8]}"


# ------------------------------------------------------------------------------------------------ 1. the device lookup
def test_device_lookup_equals_numpy_bit_for_bit(dev):
    gs = small_schedule()
    h, v = lookup_points()
    out = np.full((h.size, 12), np.nan)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)
    g = gs.grid()
    rc = dev.L.f16_debug_gain_lookup(dev.ctx.handle, ctypes.byref(g), dev.p(gs.device_table("cuda:0")), hp(h), hp(v), h.size, hp(out))
    assert rc == 0, dev.L.f16_last_error()
    want = gs.lookup(h, v)
    assert same_bits(out, want), int((out.view(np.int64) != want.view(np.int64)).sum())


# ------------------------------------------------------------------------------------------------ 2. the chain, six aircraft
@pytest.mark.parametrize("method", [EULER, RK4])
def test_chain_of_six_under_one_lane(dev, method):
    gs, x0 = synthetic_schedule(), six_aircraft()
    n, gs_every, hold = 45, 7, 5
    dem = demands((n + hold - 1) // hold, 6)
    one = dev.one(gs, x0, dem, n, gs_every, hold, 1, method, flags=ONE_LANE)
    chain = dev.chain(gs, x0, dem, n, gs_every, hold, 1, method, flags=ONE_LANE)
    assert_same(one, chain, f"method {method}")
    x, traj, st, uo, out = one
    ih, iv = np.array([c[0] for c in chain[5]]), np.array([c[1] for c in chain[5]])      # [updates, B]
    assert len(set(ih[:, 0])) > 1 and len(set(iv[:, 0])) > 1, "aircraft 0 crosses cell boundaries in both axes"
    st, out = st.cpu().numpy(), out.cpu().numpy()
    updates = (n + gs_every - 1) // gs_every
    assert out[1] < updates and out[2] == updates and out[3] == updates and out[4] == updates and out[5] == updates
    assert st[4] & ENVELOPE and not st[0] & ENVELOPE and st[5] & 32           # frozen on entry; NaN airspeed: F16_ST_NONFINITE
    assert bits(x[:, 4], dev.dev(x0[4])), "the frozen aircraft keeps its state"
    # a frozen aircraft reports the offset of the last update at its frozen state: u_out = [thrust, g[9..11]]
    g4 = gs.lookup(x0[4, 2], x0[4, 6])
    assert same_bits(uo[:, 4].cpu().numpy(), np.concatenate(([x0[4, 12]], g4[9:12])))
    assert np.isfinite(traj[:, :, :4].cpu().numpy()).all()


# ------------------------------------------------------------------------------------------------ 3. the chain, default flags
@pytest.mark.parametrize("method,gs_every,hold,n", [(EULER, 7, 5, 45), (RK4, 7, 5, 45)])
def test_chain_lofi_two_workgroups(dev, method, gs_every, hold, n):
    gs, x0 = synthetic_schedule(), many_aircraft(70)
    dem = demands((n + hold - 1) // hold, 70)
    one = dev.one(gs, x0, dem, n, gs_every, hold, 1, method, fi=0)
    assert_same(one, dev.chain(gs, x0, dem, n, gs_every, hold, 1, method, fi=0), f"lofi B = 70 method {method}")


@pytest.mark.parametrize("B", [20000, 140000])
def test_chain_hifi_euler_large_batches(dev, B):
    """128 lanes per workgroup (B = 20,000: the sin / cos pairs are carried) and 512 on the integer table image (140,000); every
    segment is 32 steps long"""
    gs, x0 = synthetic_schedule(), many_aircraft(B)
    n, gs_every, hold = 96, 32, 64
    dem = demands(2, B)
    one = dev.one(gs, x0, dem, n, gs_every, hold, 32, EULER)
    chain = dev.chain(gs, x0, dem, n, gs_every, hold, 32, EULER)
    assert_same(one, chain, f"hifi Euler B = {B}")
    out = one[4].cpu().numpy()
    assert 0 < (out > 0).sum() < B and out.max() == 3


def test_chain_hifi_rk4_20000(dev):
    gs, x0 = synthetic_schedule(), many_aircraft(20000)
    n, gs_every, hold = 21, 7, 5
    dem = demands(5, 20000)
    one = dev.one(gs, x0, dem, n, gs_every, hold, 1, RK4)
    assert_same(one, dev.chain(gs, x0, dem, n, gs_every, hold, 1, RK4), "hifi RK4 B = 20,000")


# ------------------------------------------------------------------------------------------------ 4. a table of identical nodes
def frozen_gain_call(dev, gs, x0, dem, n, hold, every, method, fi=1, flags=0):
    """f16_rollout_lqr_rk with the ONE gain and offset a table of identical nodes holds"""
    t, p = dev.t, dev.p
    B = len(x0)
    x, st, traj, uo = dev.buffers(x0, n, every)
    g = dev.dev(gs.table[0, 0])
    K = t.full((27, B), float("nan"), dtype=t.float64, device="cuda:0")
    u0 = t.empty((4, B), dtype=t.float64, device="cuda:0")
    u0[0] = x[12]
    for i in range(3):
        K[9 * i + 4:9 * i + 7] = g[3 * i:3 * i + 3, None]
    u0[1:4] = g[9:12, None]
    rc = dev.L.f16_rollout_lqr_rk(dev.ctx.handle, p(x), p(u0), p(K), p(dev.dev(dem)), p(traj), p(uo), p(st), B, B, n, hold, every or 1, DT, XCG,
                                  fi, method, flags, None)
    assert rc == 0, dev.L.f16_last_error()
    t.cuda.synchronize()
    return x, traj, st, uo


@pytest.mark.parametrize("method", [EULER, RK4])
def test_identical_nodes_equal_the_frozen_gain_loop_under_one_lane(dev, method):
    gs, x0 = synthetic_schedule(flat=True), six_aircraft()[:5]
    n, gs_every, hold = 64, 7, 5
    dem = demands(13, 5)
    x, traj, st, uo, _ = dev.one(gs, x0, dem, n, gs_every, hold, 1, method, flags=ONE_LANE)
    fx, ftraj, fst, fuo = frozen_gain_call(dev, gs, x0, dem, n, hold, 1, method, flags=ONE_LANE)
    assert bits(x, fx) and bits(traj, ftraj) and bits(st, fst) and bits(uo, fuo)


@pytest.mark.parametrize("method,gs_every", [(EULER, 5), (RK4, 7)])
def test_identical_nodes_equal_the_frozen_gain_loop_lofi(dev, method, gs_every):
    """default flags, lofi, two 64-lane workgroups -- the same kernel family in both calls.  The Euler kernel of this size carries its
    sin / cos pairs and restarts them at every segment start, so its bits are f16_rollout_lqr_rk's when the gain updates fall on row
    starts (gs_every = hold); the Runge-Kutta kernel carries nothing: any period."""
    gs, x0 = synthetic_schedule(flat=True), many_aircraft(70)
    n, hold = 64, 5
    dem = demands(13, 70)
    x, traj, st, uo, _ = dev.one(gs, x0, dem, n, gs_every, hold, 1, method, fi=0)
    fx, ftraj, fst, fuo = frozen_gain_call(dev, gs, x0, dem, n, hold, 1, method, fi=0)
    assert bits(x, fx) and bits(traj, ftraj) and bits(st, fst) and bits(uo, fuo)


# ------------------------------------------------------------------------------------------------ 5. the period and split launches
@pytest.mark.parametrize("method,flags,fi", [(EULER, ONE_LANE, 1), (RK4, ONE_LANE, 1), (RK4, 0, 1), (RK4, 0, 0)])
def test_period_beyond_the_run_and_split_launches(dev, method, flags, fi):
    gs, x0 = synthetic_schedule(), six_aircraft()
    n, m, gs_every, hold = 35, 10, 7, 5
    dem = dev.dev(demands(9, 6))
    a = dev.one(gs, x0, dem, n + m, n + m, hold, 1, method, fi=fi, flags=flags)
    b = dev.one(gs, x0, dem, n + m, n + m + 100, hold, 1, method, fi=fi, flags=flags)
    assert all(bits(p, q) for p, q in zip(a, b)), "gs_every >= nsteps is one update at step 0"
    assert set(a[4].cpu().numpy()[:4]) == {0, 1}
    whole = dev.one(gs, x0, dem, n + m, gs_every, hold, 1, method, fi=fi, flags=flags)
    x1, t1, s1, u1, o1 = dev.one(gs, x0, dem, n, gs_every, hold, 1, method, fi=fi, flags=flags)
    x2, t2, s2, u2, o2 = dev.one(gs, x1.t().cpu().numpy(), dem[n // hold:], m, gs_every, hold, 1, method, fi=fi, flags=flags, status0=s1,
                                 thrust=dev.dev(x0[:, 12]))                   # (the thrust COMMAND of the whole run, not the engine state)
    assert bits(whole[0], x2) and bits(whole[1], dev.t.cat((t1, t2))) and bits(whole[2], s2) and bits(whole[3], u2)
    assert bits(whole[4], o1 + o2)


# ------------------------------------------------------------------------------------------------ 6. default flags vs the flag
# The 64-lane kernel (table image in LDS, sin / cos pairs carried) against k_rollout_exact_gs.  Status words: equal.  States: the bound
# is 10 x the distance measured ON THE PARENT COMMIT between its two kernels of the same families on these six states over the same 45
# steps, open loop: f16_rollout_lqr_sched under F16_FLAG_ONE_LANE with K = 0 (the law then commands u0: k_rollout_exact) against
# f16_rollout_cost's x_end under default flags with every row = u0 (the 64-lane one-lane kernel) -- the closed loop feeds such ulp
# differences back through the gains for 45 steps.  Measured on the parent on an MI355X: 1.136e-16 between the two final states
# (|a - b| / max(1, |b|), max over the 18 states of the four aircraft that fly; 3.2e-16 over all 45 stored samples); for scale, the
# fused MPPI loop observed 1.6e-16 on a comparable case.  Bound: 1.136e-15, applied here to every stored sample and to u_out.
# Measured with this loop: 3.2e-16.
PARENT_DISTANCE = 1.136251e-16
KERNEL_BOUND = 10 * PARENT_DISTANCE


def test_default_flags_against_the_flagged_result(dev):
    gs, x0 = synthetic_schedule(), six_aircraft()
    n, gs_every, hold = 45, 7, 5
    dem = demands(9, 6)
    a = dev.one(gs, x0, dem, n, gs_every, hold, 1, EULER)
    b = dev.one(gs, x0, dem, n, gs_every, hold, 1, EULER, flags=ONE_LANE)
    assert bits(a[2], b[2]), f"status {a[2].tolist()} vs {b[2].tolist()}"
    fly = [0, 1, 2, 3]                                                         # (4 is frozen: the same bits; 5 is NaN)
    d = max(rel(a[1][:, :, fly].cpu().numpy(), b[1][:, :, fly].cpu().numpy()), rel(a[3][:, fly].cpu().numpy(), b[3][:, fly].cpu().numpy()))
    print(f"MEASURED default flags against F16_FLAG_ONE_LANE: {d:.3e} (bound {KERNEL_BOUND})")
    assert bits(a[0][:, 4], b[0][:, 4]) and np.array_equal(a[4].cpu().numpy(), b[4].cpu().numpy())
    assert d <= KERNEL_BOUND


# ------------------------------------------------------------------------------------------------ 7. Python
def test_rollout_LQR_with_a_schedule_equals_the_C_call(dev):
    from f16_mpc_oop_py_amd import F16Batch
    gs, x0 = synthetic_schedule(), six_aircraft()
    n, hold = 45, 5
    dem = demands(9, 6)
    x, traj, st, uo, out = dev.one(gs, x0, dem, n, 7, hold, 1, EULER, flags=ONE_LANE)
    env = F16Batch(x0, None, xcg=XCG, dt=DT, flags=ONE_LANE, device="cuda:0")
    ptraj, info = env.rollout_LQR(n, dem[:, 0], dem[:, 1], dem[:, 2], schedule=gs, gains_every=7, hold=hold, traj_every=1, return_info=True)
    assert bits(ptraj, traj) and bits(env._x, x) and bits(env.status, st) and bits(env._u, uo) and bits(info["gs_out"], out)
    # constant demands: one row held for every step
    env = F16Batch(x0, None, xcg=XCG, dt=DT, flags=ONE_LANE, device="cuda:0")
    env.rollout_LQR(n, 0.05, -0.02, 0.01, schedule=gs, gains_every=7, method="rk4")
    row = np.broadcast_to(np.array([0.05, -0.02, 0.01])[None, :, None], (1, 3, 6))
    x, _, st, uo, _ = dev.one(gs, x0, row, n, 7, n, None, RK4, flags=ONE_LANE)
    assert bits(env._x, x) and bits(env.status, st) and bits(env._u, uo)


def test_build_on_a_two_by_two_grid(dev):
    from f16_mpc_oop_py_amd import F16Batch
    from f16_mpc_oop_py_amd.schedule import GainSchedule
    gs = GainSchedule.build(9000.0, 2000.0, 2, 650.0, 100.0, 2, xcg=XCG, strict=False)
    env = F16Batch.from_trim([9000.0, 9000.0, 11000.0, 11000.0], [650.0, 750.0, 650.0, 750.0], xcg=XCG, device="cuda:0")
    K = env._calc_LQR_gain().cpu().numpy()
    lqr_status = env.last_status.cpu().numpy()
    xt = env.x_values.cpu().numpy()
    cost, status = env.trim_info["cost"].cpu().numpy(), env.trim_info["status"].cpu().numpy()
    print("trim cost", cost, "trim status", status, "LQR status", lqr_status, "ok", gs.ok.tolist())
    for ih in range(2):
        for iv in range(2):
            b = ih * 2 + iv
            assert same_bits(gs.table[ih, iv, :9], K[b, :, 4:7].ravel()) and same_bits(gs.table[ih, iv, 9:], xt[b, 13:16])
            assert bool(gs.ok[ih, iv]) == bool(cost[b] <= 1e-4 and status[b] == 0 and lqr_status[b] == 0)
    if not gs.ok.all():
        with pytest.raises(ValueError, match="bad nodes"):
            GainSchedule.build(9000.0, 2000.0, 2, 650.0, 100.0, 2, xcg=XCG, strict=True)
