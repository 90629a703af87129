"""GPU tests of the scored rollout f16_rollout_cost, the softmin blend f16_mppi_blend and the MPPI surface of F16Batch on top of them.

Contract (include/f16_hip.h): lane j is sample j / B0 of aircraft j % B0; its cost is the sum defined there, accumulated in fp64 in
step order; the states are f16_rollout_sched's on the K-fold replicated initial states, bit for bit wherever both run the same kernel.
Tolerances are derived, not measured: see each test."""
import ctypes

import numpy as np
import pytest

from conftest import golden
from test_gpu_rollout_sched import Dev, bits, doublet_rows, near_the_ground, rel

pytestmark = pytest.mark.gpu

MPC_X = [3, 4, 7, 8, 9, 10, 11, 17, 16]                 # parameters.py:135
X_LB = np.array([-np.inf, -np.inf, 0, -np.inf, -np.inf, -np.inf, 0, -20., -30., -300, -100, -50, 1000, -25, -21.5, -30., 0., -np.inf])
X_UB = np.array([np.inf, np.inf, 100000, np.inf, np.inf, np.inf, 900, 90, 30, 300, 100, 50, 19000, 25, 21.5, 30, 25, np.inf])
EPS = 2.0 ** -52
NSTEPS, HOLD = 50, 20                                    # the last segment is short
# (B0, K, fi, flags as a name): one per kernel family
SHAPES = [(3, 5, 1, ""), (70, 3, 1, ""),                 # 64 lanes: a partial wavefront; fan-out across a workgroup boundary
          (250, 80, 1, ""), (250, 280, 1, ""),           # 128 and 256 lanes
          (250, 560, 1, ""),                             # 512 lanes on the integer image
          (64, 64, 0, ""), (250, 560, 0, ""),            # lofi: 64 and 512 lanes
          (70, 3, 1, "one_lane")]
SHAPE_IDS = [f"{b0}x{k}-fi{fi}{'-' + fl if fl else ''}" for b0, k, fi, fl in SHAPES]


def flag_bits(name):
    from f16_mpc_oop_py_amd import lib
    return {"": 0, "one_lane": lib.F16_FLAG_ONE_LANE, "no_envelope": lib.F16_FLAG_NO_ENVELOPE}[name]


def weights(seed=5, pen=0.0):
    """seeded positive weights, all different, so that a swapped index shows"""
    from f16_mpc_oop_py_amd import lib
    v = np.random.default_rng(seed).uniform(0.5, 2.0, 21)
    return lib.make_cost_weights(v[:9], v[9:18], v[18:21], pen)


def case_inputs(B0, K, S, seed=None):
    """config-2 states, the doublet schedule with a seeded perturbation per sample, a reference per aircraft: the initial x9 with the
    three rate entries set to seeded demands in +-0.1 rad/s; a seeded command reference"""
    from f16_mpc_oop_py_amd.workload import config2_states
    x0, u0 = config2_states(B0, seed=B0 if seed is None else seed)
    base = doublet_rows(u0, S)                                                    # [S, B0, 4]
    rows = np.stack([base + np.random.default_rng(1000 + k).uniform(-1, 1, (S, B0, 4)) * [100.0, 0.5, 0.5, 0.5] for k in range(K)], 1)
    rng = np.random.default_rng(77 + B0)
    xref = x0[:, MPC_X].copy()
    xref[:, 4:7] = rng.uniform(-0.1, 0.1, (B0, 3))
    uref = u0[:, 1:4] + rng.uniform(-0.2, 0.2, (B0, 3))
    return x0, u0, rows, xref, uref


def run_cost(dev, x0, rows, xref, uref, w, nsteps, hold, every=None, *, fi=1, flags=0, want_end=True, pad=True, stream=None):
    """One f16_rollout_cost launch.  x0 [B0, 18], rows [S, K, B0, 4], xref [B0, 9], uref [B0, 3] or None.  With pad: ld = B + 37,
    ld0 = B0 + 5, NaN (status: -7) in the padding and in every output.  -> dict(cost [ld], x_end [18, ld], traj [n, 18, ld], st [ld], seq)"""
    t, p = dev.t, dev.p
    S, K, B0 = rows.shape[:3]
    B = K * B0
    ld, ld0 = (B + 37, B0 + 5) if pad else (B, B0)
    xs, xr = dev.soa(x0, ld0), dev.soa(xref, ld0)
    ur = dev.soa(uref, ld0) if uref is not None else None
    sq = dev.seq(rows.reshape(S, B, 4), ld)
    nan = lambda *shape: t.full(shape, float("nan"), dtype=t.float64, device="cuda:0")
    cost, x_end = nan(ld), (nan(18, ld) if want_end else None)
    traj = nan(nsteps // every, 18, ld) if every else None
    st = t.full((ld,), -7, dtype=t.int32, device="cuda:0")
    rc = dev.L.f16_rollout_cost(dev.ctx.handle, p(xs), B0, ld0, p(sq), p(xr), p(ur), ctypes.byref(w), p(cost), p(x_end), p(traj), p(st),
                                B, ld, nsteps, hold, every or 1, 0.001, 0.25, fi, flags, stream)
    assert rc == 0, dev.L.f16_last_error()
    t.cuda.synchronize()
    assert bits(xs, dev.soa(x0, ld0))                                             # x0 is read-only
    return dict(cost=cost, x_end=x_end, traj=traj, st=st, seq=sq, B=B, ld=ld)


def cost_definition(x0, rows, xref, uref, w, traj, hold, no_envelope=False):
    """J of include/f16_hip.h in numpy fp64, in step order, from the stored samples traj [T, 18, B] (every step), the rows
    [S, K, B0, 4] and the box of env.py:117-124.  -> (J [B], frozen_from [B]: the first step a lane does not take, T if none)"""
    S, K, B0 = rows.shape[:3]
    T, B = traj.shape[0], K * B0
    a = np.arange(B) % B0
    q, qf, r = np.array(w.q), np.array(w.qf), np.array(w.r)
    xr = xref[a]                                                                  # [B, 9]
    ur = uref[a] if uref is not None else np.zeros((B, 3))
    u = rows.reshape(S, B, 4)
    x = x0[a]                                                                     # the state before step t
    J, frozen, frozen_from = np.zeros(B), np.zeros(B, dtype=bool), np.full(B, T)
    for t in range(T):
        with np.errstate(invalid="ignore"):
            out = ((x < X_LB) | (x > X_UB)).any(1)
        newly = out & ~frozen & (not no_envelope)
        frozen_from[newly] = t
        frozen |= newly
        xn = traj[t].T                                                            # [B, 18] after step t
        du = u[t // hold][:, 1:4] - ur
        step = np.zeros(B)
        for i in range(3):
            step = step + r[i] * du[:, i] * du[:, i]
        Jt = J + step
        for k in range(9):
            d = xn[:, MPC_X[k]] - xr[:, k]
            Jt = Jt + q[k] * d * d
        J = np.where(frozen, J + w.pen, Jt)
        x = xn
    for k in range(9):
        d = x[:, MPC_X[k]] - xr[:, k]
        J = J + qf[k] * d * d
    return J, frozen_from


def check_cost(dev, out, x0, rows, xref, uref, w, nsteps, hold, no_envelope=False):
    """the launch's cost against its definition on the launch's own samples; the padding untouched.  Tolerance: every term is
    non-negative, so either summation is off by rounding alone: 2^-52 (terms + 4) relative, terms = 12 nsteps + 9."""
    from f16_mpc_oop_py_amd.lib import F16_ST
    B, t = out["B"], dev.t
    J, frozen_from = cost_definition(x0, rows, xref, uref, w, out["traj"].cpu().numpy()[:, :, :B], hold, no_envelope)
    got = out["cost"].cpu().numpy()[:B]
    st = out["st"].cpu().numpy()
    assert np.array_equal((st[:B] & F16_ST["ENVELOPE"]) != 0, frozen_from < nsteps)
    fin = np.isfinite(J)
    assert np.array_equal(fin, np.isfinite(got))
    tol = EPS * (12 * nsteps + 9 + 4)
    err = float(np.max(np.abs(got[fin] - J[fin]) / J[fin])) if fin.any() else 0.0
    print(f"cost vs definition: max rel {err:.3e} (bound {tol:.3e}), {int((frozen_from < nsteps).sum())} frozen of {B}")
    assert err <= tol
    assert bool(t.isnan(out["cost"][B:]).all()) and bool(t.isnan(out["traj"][:, :, B:]).all()) and bool((out["st"][B:] == -7).all())
    if out["x_end"] is not None:
        assert bool(t.isnan(out["x_end"][:, B:]).all()) and bits(out["x_end"][:, :B], out["traj"][-1][:, :B])
    return J, frozen_from


@pytest.fixture(scope="module")
def dev(hip):
    return Dev()


_scored = {}


def scored(dev, shape):
    """the launch of a shape (every step stored), computed once and shared; the samples are dropped after the tests that need them"""
    if shape not in _scored:
        B0, K, fi, fl = shape
        x0, u0, rows, xref, uref = case_inputs(B0, K, (NSTEPS + HOLD - 1) // HOLD)
        w = weights()
        out = run_cost(dev, x0, rows, xref, uref, w, NSTEPS, HOLD, 1, fi=fi, flags=flag_bits(fl))
        _scored[shape] = dict(out=out, x0=x0, rows=rows, xref=xref, uref=uref, w=w)
    return _scored[shape]


# ------------------------------------------------------------------------------------------------ 1. the cost is its definition
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_cost_equals_its_definition(dev, shape):
    c = scored(dev, shape)
    check_cost(dev, c["out"], c["x0"], c["rows"], c["xref"], c["uref"], c["w"], NSTEPS, HOLD)
    if shape[0] * shape[1] > 20000:
        _scored[shape]["out"]["traj"] = None                 # (a GB of samples at the largest shapes: test 2 re-runs those)


@pytest.mark.parametrize("shape", SHAPES[:2], ids=SHAPE_IDS[:2])
@pytest.mark.parametrize("hold", [1, 1000])
def test_cost_equals_its_definition_for_a_row_per_step_and_for_one_row(dev, shape, hold):
    B0, K, fi, fl = shape
    x0, u0, rows, xref, uref = case_inputs(B0, K, (NSTEPS + hold - 1) // hold)
    w = weights(seed=6)
    uref = None if hold == 1 else uref                       # (u_ref = NULL is 0)
    out = run_cost(dev, x0, rows, xref, uref, w, NSTEPS, hold, 1, fi=fi)
    check_cost(dev, out, x0, rows, xref, uref, w, NSTEPS, hold)


def test_cost_equals_its_definition_in_the_strict_build():
    """The expression-exact build (no contraction, IEEE divisions) compiles the scored kernels too: the same check on one shape, in a
    child process because a process holds one libf16hip."""
    import json
    import os
    import subprocess
    import sys
    from conftest import REPO
    from f16_mpc_oop_py_amd import lib
    so = lib.strict_path()          # never compiles here: this process has initialised the GPU
    code = r'''
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")
import test_gpu_rollout_cost as tc
dev = tc.Dev()
x0, u0, rows, xref, uref = tc.case_inputs(70, 3, 3)
w = tc.weights()
out = tc.run_cost(dev, x0, rows, xref, uref, w, tc.NSTEPS, tc.HOLD, 1)
tc.check_cost(dev, out, x0, rows, xref, uref, w, tc.NSTEPS, tc.HOLD)
print(json.dumps({"ok": True, "so": dev.L._name}))
''' % (REPO, REPO)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, F16HIP_SO=so), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["ok"] and rec["so"] == so, rec


# ------------------------------------------------------------------------------------------------ 2. the states are f16_rollout_sched's
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_states_are_those_of_the_scheduled_rollout(dev, oracle, shape):
    B0, K, fi, fl = shape
    B = B0 * K
    c = scored(dev, shape)
    out = c["out"]
    if out["traj"] is None:
        out = run_cost(dev, c["x0"], c["rows"], c["xref"], c["uref"], c["w"], NSTEPS, HOLD, 1, fi=fi, flags=flag_bits(fl))
        assert bits(out["cost"], c["out"]["cost"])
    lanes = c["rows"].reshape(-1, B, 4)
    same_kernel = fi == 0 or B > 16384 or fl == "one_lane"
    if same_kernel:
        x, traj, st, _ = dev.run(np.tile(c["x0"], (K, 1)), lanes, NSTEPS, HOLD, 1, fi=fi, flags=flag_bits(fl), ld=out["ld"])
        assert bits(out["x_end"][:, :B], x[:, :B]) and bits(out["traj"][:, :, :B], traj[:, :, :B]) and bits(out["st"][:B], st[:B])
        del traj
    else:
        # hifi at or below 16,384 lanes: f16_rollout_sched runs a four-lanes-per-aircraft kernel there, so the yardstick is the
        # restatement chained per segment, at the 1e-9 of test_scheduled_rollout_vs_the_restatement_chained_per_segment
        xr = np.tile(c["x0"], (K, 1))
        for s0 in range(0, NSTEPS, HOLD):
            xr, _, so = oracle.rollout(xr, lanes[s0 // HOLD], min(HOLD, NSTEPS - s0), fi_flag=fi, store=False, nthreads=16)
            assert not np.asarray(so).any()
        err = rel(out["x_end"].t().cpu().numpy()[:B], xr)
        print(f"{B0} x {K}: scored launch vs chained restatement over {NSTEPS} steps: {err:.3e}")
        assert err < 1e-9 and int(out["st"][:B].max()) == 0
    # the cost does not depend on what else is stored
    bare = run_cost(dev, c["x0"], c["rows"], c["xref"], c["uref"], c["w"], NSTEPS, HOLD, None, fi=fi, flags=flag_bits(fl), want_end=False)
    assert bits(bare["cost"], c["out"]["cost"]) and bits(bare["st"], c["out"]["st"])
    if B > 1000:
        _scored[shape]["out"]["traj"] = None


# ------------------------------------------------------------------------------------------------ 3. freeze and penalty
def test_freeze_penalty_no_envelope_and_nan_rows(dev, oracle):
    from f16_mpc_oop_py_amd.lib import F16_FLAG_NO_ENVELOPE, F16_ST, F16_ST_ENV_STATE
    B0, K, T, hold, pen = 40, 3, 128, 32, 7.5
    g = golden("g567_trim_lin_lqr.npz")
    x0 = np.tile(g["trim_x_xcg25"], (B0, 1))
    u0 = x0[:, 12:16].copy()
    x0[5], x0[B0 - 1] = near_the_ground(x0[5], 2.5), near_the_ground(x0[B0 - 1], 4.0)
    # the CPU restatement: outside after steps 36 and 58 (the sample of index 35 / 57 is the first one below zero altitude)
    _, tr, so = oracle.rollout(x0[[5, B0 - 1]], u0[[5, B0 - 1]], T)
    assert [int(np.argmax(tr[:, b, 2] < 0)) + 1 for b in (0, 1)] == [36, 58] and np.all(so == (F16_ST["ENVELOPE"] | F16_ST_ENV_STATE(2)))
    rows = np.tile(u0, (4, K, 1, 1))                                              # [4, K, B0, 4]
    for k in range(K):
        rows[1:, k, :, 1] += 0.5 * (k + 1)                                        # (the samples differ from the second row on)
    rows[3, 1, 7] = np.nan                                                        # a NaN row for ONE lane: sample 1 of aircraft 7
    xref = x0[:, MPC_X].copy()
    xref[:, 4:7] = np.random.default_rng(9).uniform(-0.1, 0.1, (B0, 3))
    w = weights(seed=8, pen=pen)
    out = run_cost(dev, x0, rows, xref, None, w, T, hold, 1)
    J, frozen_from = check_cost(dev, out, x0, rows, xref, None, w, T, hold)
    st = out["st"].cpu().numpy()[:K * B0]
    frozen = np.array([k * B0 + a for k in range(K) for a in (5, B0 - 1)])
    expect = np.zeros(K * B0, dtype=np.int32)
    expect[frozen] = F16_ST["ENVELOPE"] | F16_ST_ENV_STATE(2)
    others = np.arange(K * B0) != B0 + 7
    assert np.array_equal(st[others], expect[others]) and st[B0 + 7] & F16_ST["NONFINITE"] and not st[B0 + 7] & F16_ST["ENVELOPE"]
    assert np.array_equal(frozen_from[frozen], [36, 58] * K)                      # so the penalty counts 92 and 70 steps
    got = out["cost"].cpu().numpy()[:K * B0]
    assert np.array_equal(np.isfinite(got), np.arange(K * B0) != B0 + 7)          # the NaN row: that lane only
    # the penalty is what it is said to be: the same launch without it is smaller by pen * (steps not taken), up to the roundings of
    # the two sums (the bound of check_cost, on the larger of the two)
    w0 = weights(seed=8, pen=0.0)
    got0 = run_cost(dev, x0, rows, xref, None, w0, T, hold, None, want_end=False)["cost"].cpu().numpy()[:K * B0]
    steps_lost = np.zeros(K * B0)
    steps_lost[frozen] = T - frozen_from[frozen]
    fin = np.isfinite(got)
    assert np.all(np.abs(got[fin] - got0[fin] - pen * steps_lost[fin]) <= 2 * EPS * (12 * T + 13) * got[fin])
    assert np.array_equal(got[steps_lost == 0], got0[steps_lost == 0], equal_nan=True)
    # F16_FLAG_NO_ENVELOPE: nobody is frozen, no penalty is ever added, the lanes keep integrating
    free = run_cost(dev, x0, rows, xref, None, w, T, hold, 1, flags=F16_FLAG_NO_ENVELOPE)
    free0 = run_cost(dev, x0, rows, xref, None, w0, T, hold, None, flags=F16_FLAG_NO_ENVELOPE, want_end=False)
    assert bits(free["cost"], free0["cost"])
    check_cost(dev, free, x0, rows, xref, None, w, T, hold, no_envelope=True)
    stf = free["st"].cpu().numpy()[:K * B0]
    assert not (stf & F16_ST["ENVELOPE"]).any()
    trf = free["traj"].cpu().numpy()
    for j in frozen:
        assert trf[-1, 2, j] < trf[64, 2, j] < 0 and not np.array_equal(trf[-1, :, j], trf[-2, :, j])


# ------------------------------------------------------------------------------------------------ 4. the blend
def run_blend(dev, cost, seq, lam, B0, K, S, ld, ld0, w_out=True, stats=True, stream=None):
    t, p = dev.t, dev.p
    nan = lambda *shape: t.full(shape, float("nan"), dtype=t.float64, device="cuda:0")
    ub, wo, sts = nan(S, 4, ld0), (nan(ld) if w_out else None), (nan(2, ld0) if stats else None)
    rc = dev.L.f16_mppi_blend(dev.ctx.handle, p(cost), p(seq), lam, p(ub), p(wo), p(sts), B0 * K, ld, B0, ld0, S, stream)
    assert rc == 0, dev.L.f16_last_error()
    t.cuda.synchronize()
    return ub, wo, sts


@pytest.mark.parametrize("shape", SHAPES[:3], ids=SHAPE_IDS[:3])
@pytest.mark.parametrize("lam", [0.1, 10.0])
def test_blend_against_the_reference_rule(dev, shape, lam):
    """Tolerance 16 K 2^-52 relative to max(1, max |u|): each weight is at most 1 and the minimum-cost sample has weight exactly 1
    (so the denominator is >= 1); an error dz in the exponent moves w by at most |z| e^-|z| dz <= dz / e; the two sums add K
    roundings each."""
    from f16_mpc_oop_py_amd.mppi import blend_reference
    B0, K, fi, fl = shape
    c = scored(dev, shape)
    out, B, ld, ld0 = c["out"], B0 * K, c["out"]["ld"], B0 + 5
    S = c["rows"].shape[0]
    ub, wo, sts = run_blend(dev, out["cost"], out["seq"], lam, B0, K, S, ld, ld0)
    ref, info = blend_reference(out["cost"][:B].cpu().view(K, B0), c["rows"], lam, return_info=True)
    tol = 16 * K * EPS
    got = ub[:, :, :B0].permute(0, 2, 1).cpu().numpy()
    err = np.abs(got - ref.numpy()).max() / max(1.0, np.abs(c["rows"]).max())
    w = wo[:B].view(K, B0).cpu().numpy()
    errw = np.abs(w - info["weights"].numpy()).max()
    ess = sts[1, :B0].cpu().numpy()
    erre = np.abs(ess / info["ess"].numpy() - 1).max()
    print(f"{B0} x {K} lam {lam}: blend {err:.3e}, weights {errw:.3e}, ess {erre:.3e} (bound {tol:.3e}); ess {ess.min():.2f} .. {ess.max():.2f}")
    assert err <= tol and errw <= tol and erre <= tol
    assert np.abs(w.sum(0) - 1).max() <= K * EPS
    assert np.array_equal(sts[0, :B0].cpu().numpy(), info["min_cost"].numpy())
    t = dev.t
    assert bool(t.isnan(ub[:, :, B0:]).all()) and bool(t.isnan(wo[B:]).all()) and bool(t.isnan(sts[:, B0:]).all())
    ub2, _, _ = run_blend(dev, out["cost"], out["seq"], lam, B0, K, S, ld, ld0, w_out=False, stats=False)
    assert bits(ub2, ub)


def test_blend_exact_cases(dev):
    t = dev.t
    rng = np.random.default_rng(12)
    B0, K, S = 70, 6, 3
    rows = rng.normal(size=(S, K, B0, 4)) * [1000.0, 5, 5, 5]
    seq = dev.seq(rows.reshape(S, K * B0, 4))
    cost = rng.uniform(1.0, 3.0, (K, B0))
    # K = 1: the sample's rows, bit for bit
    one = dev.seq(rows[:, 0])
    ub, wo, sts = run_blend(dev, t.as_tensor(cost[0], device="cuda:0"), one, 0.7, B0, 1, S, B0, B0)
    assert bits(ub, one) and bool((wo == 1).all()) and bool((sts[1] == 1).all()) and np.array_equal(sts[0].cpu().numpy(), cost[0])
    # lambda = 1e-300: the minimum-cost sample's rows, bit for bit
    cd = t.as_tensor(cost.reshape(-1), device="cuda:0")
    ub, wo, sts = run_blend(dev, cd, seq, 1e-300, B0, K, S, K * B0, B0)
    best = cost.argmin(0)
    pick = rows[:, best, np.arange(B0)]                                           # [S, B0, 4]
    assert np.array_equal(ub.permute(0, 2, 1).cpu().numpy(), pick)
    assert np.array_equal(wo.view(K, B0).cpu().numpy(), (np.arange(K)[:, None] == best[None]).astype(float))
    # a NaN and a +inf cost get weight 0 (their commands, NaN here, are not read); an aircraft without a finite cost gets sample 0
    bad = cost.copy()
    bad[1, 0], bad[4, 0] = np.nan, np.inf
    bad[:, 9] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
    rows_bad = rows.copy()
    rows_bad[:, 1, 0], rows_bad[:, 4, 0] = np.nan, np.nan
    ub, wo, sts = run_blend(dev, t.as_tensor(bad.reshape(-1), device="cuda:0"), dev.seq(rows_bad.reshape(S, K * B0, 4)), 0.5, B0, K, S, K * B0, B0)
    keep = [0, 2, 3, 5]
    sub, _, _ = run_blend(dev, t.as_tensor(cost[keep].reshape(-1), device="cuda:0"), dev.seq(rows[:, keep].reshape(S, 4 * B0, 4)), 0.5, B0, 4, S, 4 * B0, B0)
    w = wo.view(K, B0).cpu().numpy()
    assert w[1, 0] == 0 and w[4, 0] == 0 and bits(ub[:, :, 0], sub[:, :, 0]) and bool(t.isfinite(ub).all())
    assert np.array_equal(ub[:, :, 9].cpu().numpy(), rows[:, 0, 9]) and not w[:, 9].any() and not sts[:, 9].cpu().numpy().any()
    assert abs(w[:, 0].sum() - 1) <= K * EPS


# ------------------------------------------------------------------------------------------------ 5. arguments and capture
def test_argument_errors_and_no_ops(dev):
    from f16_mpc_oop_py_amd import lib
    L, h = dev.L, dev.ctx.handle
    w = ctypes.byref(lib.make_cost_weights())
    #            x0 B0 ld0 u_seq x_ref u_ref w cost x_end traj status B ld nsteps hold every
    good = dict(x0=1, B0=2, ld0=2, u_seq=1, x_ref=1, u_ref=None, w=w, cost=1, x_end=None, traj=None, status=None, B=4, ld=4, nsteps=10,
                hold=1, every=1)

    def call(**kw):
        a = dict(good, **kw)
        return L.f16_rollout_cost(h, a["x0"], a["B0"], a["ld0"], a["u_seq"], a["x_ref"], a["u_ref"], a["w"], a["cost"], a["x_end"],
                                  a["traj"], a["status"], a["B"], a["ld"], a["nsteps"], a["hold"], a["every"], 0.001, 0.25, 1, 0, None)
    bad = [dict(x0=None), dict(u_seq=None), dict(x_ref=None), dict(w=None), dict(cost=None), dict(hold=0), dict(nsteps=-1), dict(ld=3),
           dict(ld0=1), dict(B0=0), dict(B0=3, ld0=3), dict(traj=1, every=0), dict(traj=1, every=3)]
    for j in range(22):                                       # a negative and a non-finite weight, at every position
        for v in (-1.0, float("nan"), float("inf")):
            wb = lib.make_cost_weights()
            ctypes.cast(ctypes.pointer(wb), ctypes.POINTER(ctypes.c_double))[j] = v
            bad.append(dict(w=ctypes.byref(wb)))
    for kw in bad:
        assert call(**kw) == -1, kw
        assert len(L.f16_last_error()) > 0, kw
    assert call(B=0, ld=0) == 0 and call(B=0, ld=0, B0=0, ld0=0) == 0       # B = 0: no-op
    # nsteps = 0: the terminal term of x0 alone; no row is read (there is none: the one given here holds NaN)
    B0, K = 70, 3
    x0, u0, rows, xref, uref = case_inputs(B0, K, 1)
    wt = weights()
    out = run_cost(dev, x0, rows * np.nan, xref, uref, wt, 0, 5)
    a = np.arange(B0 * K) % B0
    term = np.zeros(B0 * K)
    for k in range(9):
        d = x0[a][:, MPC_X[k]] - xref[a][:, k]
        term = term + wt.qf[k] * d * d
    got = out["cost"].cpu().numpy()[:B0 * K]
    assert np.all(np.abs(got - term) <= EPS * 13 * term) and np.array_equal(out["x_end"].cpu().numpy()[:, :B0 * K], x0[a].T)
    assert not out["st"][:B0 * K].any()
    # f16_mppi_blend
    blend = lambda cost=1, u=1, lam=1.0, ub=1, B=4, ld=4, B0=2, ld0=2, nrows=1: L.f16_mppi_blend(h, cost, u, lam, ub, None, None, B, ld, B0, ld0, nrows, None)
    for kw in (dict(lam=0.0), dict(lam=-1.0), dict(lam=float("nan")), dict(lam=float("inf")), dict(cost=None), dict(u=None), dict(ub=None),
               dict(B0=3, ld0=3), dict(ld=3), dict(ld0=1), dict(B0=0), dict(nrows=-1)):
        assert blend(**kw) == -1, kw
        assert len(L.f16_last_error()) > 0
    assert blend(B=0, ld=0) == 0


def test_score_and_blend_replay_from_a_captured_graph(dev):
    """Neither entry allocates, the weights travel in the argument block: one call of each captured into a graph and replayed twice
    gives the direct calls' bits (4096 lanes = 64 x 64)."""
    import torch
    B0, K, T, hold = 64, 64, 64, 16
    B = B0 * K
    x0, u0, rows, xref, uref = case_inputs(B0, K, T // hold, seed=11)
    w = weights()
    ref = run_cost(dev, x0, rows, xref, uref, w, T, hold, 16, pad=False)
    rb = run_blend(dev, ref["cost"], ref["seq"], 2.0, B0, K, T // hold, B, B0)
    L, p = dev.L, dev.p
    xs, xr, ur, sq = dev.soa(x0), dev.soa(xref), dev.soa(uref), ref["seq"]
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda:0")
    cost, x_end, traj, st = z(B), z(18, B), z(T // 16, 18, B), torch.zeros(B, dtype=torch.int32, device="cuda:0")
    ub, wo, sts = z(T // hold, 4, B0), z(B), z(2, B0)

    def call():
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = L.f16_rollout_cost(dev.ctx.handle, p(xs), B0, B0, p(sq), p(xr), p(ur), ctypes.byref(w), p(cost), p(x_end), p(traj), p(st), B, B,
                                T, hold, 16, 0.001, 0.25, 1, 0, s)
        return rc or L.f16_mppi_blend(dev.ctx.handle, p(cost), p(sq), 2.0, p(ub), p(wo), p(sts), B, B, B0, B0, T // hold, s)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert call() == 0                                  # (the kernels are loaded outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert call() == 0
    for _ in range(2):
        for v in (cost, x_end, traj, st, ub, wo, sts):
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert bits(cost, ref["cost"]) and bits(x_end, ref["x_end"]) and bits(traj, ref["traj"]) and bits(st, ref["st"])
        assert bits(ub, rb[0]) and bits(wo, rb[1]) and bits(sts, rb[2])


# ------------------------------------------------------------------------------------------------ 6. the Python surface
def make_env(x, u=None, **kw):
    from f16_mpc_oop_py_amd import F16Batch
    return F16Batch(x, u, device="cuda:0", **kw)


def test_score_and_blend_schedules(dev):
    import torch
    B0, K, T, hold = 300, 4, 60, 10
    x0, u0, rows, xref, uref = case_inputs(B0, K, T // hold, seed=3)
    w = weights()
    kw = dict(q=list(w.q), qf=list(w.qf), r=list(w.r), penalty=2.0)
    w.pen = 2.0
    ref = run_cost(dev, x0, rows, xref, uref, w, T, hold, 5, pad=False)
    for form in ("numpy", "torch_host", "torch_device"):
        env = make_env(x0, u0)
        keep = (env._x.clone(), env._u.clone(), env.status.clone())
        a = {"numpy": rows, "torch_host": torch.as_tensor(rows), "torch_device": torch.as_tensor(rows, device="cuda:0")}[form]
        cost, fin, traj = env.score_schedules(a, hold=hold, x_ref=xref, u_ref=uref, traj_every=5, return_final=True, **kw)
        assert tuple(cost.shape) == (K, B0) and tuple(fin.shape) == (18, K, B0) and tuple(traj.shape) == (T // 5, 18, K, B0), form
        assert bits(cost.reshape(-1), ref["cost"]) and bits(fin.reshape(18, -1), ref["x_end"]) and bits(traj.reshape(T // 5, 18, -1), ref["traj"])
        assert bits(env.last_score_status.reshape(-1), ref["st"])
        assert bits(env._x, keep[0]) and bits(env._u, keep[1]) and bits(env.status, keep[2]), form
    only = env.score_schedules(rows, hold=hold, x_ref=xref, u_ref=uref, **kw)
    assert torch.is_tensor(only) and bits(only.reshape(-1), ref["cost"])
    # the defaults: x_ref = the current x9, no command reference, unit weights
    from f16_mpc_oop_py_amd import lib
    dflt = run_cost(dev, x0, rows, x0[:, MPC_X], None, lib.make_cost_weights(), T, hold, None, pad=False, want_end=False)
    assert bits(env.score_schedules(rows, hold=hold).reshape(-1), dflt["cost"])
    # a shorter run: the last segment cut
    cut = run_cost(dev, x0, rows, x0[:, MPC_X], None, lib.make_cost_weights(), 35, hold, None, pad=False, want_end=False)
    assert bits(env.score_schedules(rows, hold=hold, nsteps=35).reshape(-1), cut["cost"])
    # blend_schedules = f16_mppi_blend
    rb = run_blend(dev, ref["cost"], ref["seq"], 3.0, B0, K, T // hold, B0 * K, B0)
    u, info = env.blend_schedules(only, rows, 3.0, return_info=True)
    assert tuple(u.shape) == (T // hold, B0, 4) and bits(u.permute(0, 2, 1), rb[0]) and bits(info["weights"].reshape(-1), rb[1])
    assert bits(info["min_cost"], rb[2][0]) and bits(info["ess"], rb[2][1])
    assert bits(env.blend_schedules(only.cpu().numpy(), torch.as_tensor(rows), 3.0), u)
    for call in (lambda: env.score_schedules(rows[0]),                              # wrong rank
                 lambda: env.score_schedules(rows[:, :, :10]),                      # wrong batch
                 lambda: env.score_schedules(rows[..., :3]),
                 lambda: env.score_schedules(rows, hold=0),
                 lambda: env.score_schedules(rows, hold=hold, nsteps=61),           # needs seven rows
                 lambda: env.score_schedules(rows, hold=hold, traj_every=7),
                 lambda: env.blend_schedules(only, rows, 0.0),                      # lam <= 0
                 lambda: env.blend_schedules(only, rows, -1.0),
                 lambda: env.blend_schedules(only[:2], rows, 1.0),                  # samples mismatch
                 lambda: env.blend_schedules(only, rows[0], 1.0)):
        with pytest.raises(ValueError):
            call()


def mppi_by_hand(env, nsteps, dem, horizon, hold, samples, sigma, lam, seed, **kw):
    """rollout_MPPI written out: calc_MPPI_action + rollout + shift, per control period"""
    import torch
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    nominal = env.u_values.clone().unsqueeze(0).repeat(horizon, 1, 1)
    trajs, infos = [], []
    for _ in range(nsteps // hold):
        noise = sigma * torch.randn((horizon, samples, env.B, 3), generator=g, device="cuda:0", dtype=torch.float64)
        u, info = env.calc_MPPI_action(*dem, nominal, noise, hold=hold, lam=lam, **kw)
        env.set_input(u[0])
        trajs.append(env.rollout(hold, traj_every=1))
        nominal = torch.cat((u[1:], u[-1:]), 0)
        infos.append(info)
    return torch.cat(trajs, 0), infos


def test_mppi_action_and_closed_loop(dev):
    import torch
    B = 8
    g = golden("g567_trim_lin_lqr.npz")
    x0 = np.tile(g["trim_x_xcg25"], (B, 1))
    x0[:, 9:12] += np.random.default_rng(21).uniform(-0.05, 0.05, (B, 3))         # off trim: something to do
    u0 = np.tile(g["trim_x_xcg25"][12:16], (B, 1))
    dem = (0.05, np.linspace(-0.03, 0.03, B), 0.0)
    env = make_env(x0, u0)
    # zero noise, one sample: the nominal schedule, bit for bit
    nominal = torch.as_tensor(doublet_rows(u0, 5), device="cuda:0")
    u, info = env.calc_MPPI_action(*dem, nominal, torch.zeros((5, 1, B, 3), dtype=torch.float64), hold=4, lam=1.0)
    assert bits(u, nominal) and tuple(info["cost"].shape) == (1, B) and bool((info["ess"] == 1).all()) and bits(info["min_cost"], info["cost"][0])
    assert tuple(info["status"].shape) == (1, B) and int(info["status"].abs().max()) == 0
    # it is one score_schedules plus one blend_schedules, on x_ref = x9 with the demands, samples clipped to the command limits
    noise = 40.0 * torch.randn((5, 16, B, 3), generator=torch.Generator().manual_seed(1), dtype=torch.float64)     # (40 deg: some clip)
    u, info = env.calc_MPPI_action(*dem, nominal, noise, hold=4, lam=0.5, penalty=3.0, r=[0.1, 0.2, 0.3])
    samples = nominal.cpu().unsqueeze(1).repeat(1, 16, 1, 1)
    samples[..., 1:] = torch.minimum(torch.maximum(samples[..., 1:] + noise, torch.tensor([-25, -21.5, -30.0], dtype=torch.float64)),
                                     torch.tensor([25, 21.5, 30.0], dtype=torch.float64))
    assert float(samples[..., 1].abs().max()) == 25.0
    xref = x0[:, MPC_X].copy()
    xref[:, 4], xref[:, 5], xref[:, 6] = dem
    cost = env.score_schedules(samples, hold=4, x_ref=xref, penalty=3.0, r=[0.1, 0.2, 0.3])
    assert bits(cost, info["cost"]) and bits(env.last_score_status, info["status"])
    ub, binfo = env.blend_schedules(cost, samples, 0.5, return_info=True)
    assert bits(ub, u) and bits(binfo["ess"], info["ess"]) and bits(binfo["min_cost"], info["min_cost"])
    assert bits(env._x, make_env(x0, u0)._x) and np.array_equal(env.u_values.cpu().numpy(), u0)
    # the closed loop = the composition written out by hand, bit for bit; the same seed repeats, another one differs
    args = dict(horizon=5, hold=4, samples=16, sigma=0.5, lam=0.5)
    a = make_env(x0, u0)
    ta, ia = a.rollout_MPPI(24, *dem, seed=7, traj_every=1, return_info=True, penalty=3.0, **args)
    b = make_env(x0, u0)
    tb, ib = mppi_by_hand(b, 24, dem, seed=7, penalty=3.0, **args)
    assert tuple(ta.shape) == (24, 18, B) and bits(ta, tb) and bits(a._x, b._x) and bits(a._u, b._u) and bits(a.status, b.status)
    assert tuple(ia["min_cost"].shape) == (6, B) and bits(ia["min_cost"], torch.stack([i["min_cost"] for i in ib]))
    assert bits(ia["ess"], torch.stack([i["ess"] for i in ib]))
    c = make_env(x0, u0)
    assert bits(c.rollout_MPPI(24, *dem, seed=7, traj_every=1, penalty=3.0, **args), ta)
    d = make_env(x0, u0)
    assert not bits(d.rollout_MPPI(24, *dem, seed=8, traj_every=1, penalty=3.0, **args), ta)
    assert make_env(x0, u0).rollout_MPPI(8, *dem, seed=7, **args) is None
    # for the log only (no threshold: the reference has no such loop): the tracking cost of the closed loop next to holding the trim command
    held = make_env(x0, u0)
    th = held.rollout(24, traj_every=1)
    demv = torch.as_tensor(np.stack([np.broadcast_to(np.asarray(v, dtype=np.float64), (B,)) for v in dem]), device="cuda:0")
    track = lambda tr: float(((tr[:, 9:12] - demv[None]) ** 2).sum())
    print(f"rate tracking cost over 24 steps: MPPI {track(ta):.6e}, trim command held {track(th):.6e}")
    for call in (lambda: env.calc_MPPI_action(*dem, nominal[0], noise),                               # wrong ranks
                 lambda: env.calc_MPPI_action(*dem, nominal, noise[0]),
                 lambda: env.calc_MPPI_action(*dem, nominal, noise[:, :, :4]),                        # batch mismatch
                 lambda: env.calc_MPPI_action(*dem, nominal, noise[:3]),                              # rows mismatch
                 lambda: env.calc_MPPI_action(*dem, nominal, noise, lam=0.0),
                 lambda: env.rollout_MPPI(24, *dem, 5, 4, 16, 0.5, -1.0),
                 lambda: env.rollout_MPPI(24, *dem, 5, 4, 0, 0.5, 1.0),                               # no samples
                 lambda: env.rollout_MPPI(25, *dem, 5, 4, 16, 0.5, 1.0),                              # not whole periods
                 lambda: env.rollout_MPPI(24, *dem, 5, 4, 16, [0.5, 0.5], 1.0)):
        with pytest.raises(ValueError):
            call()
