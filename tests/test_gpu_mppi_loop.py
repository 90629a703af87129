"""GPU tests of the counter-based MPPI sampler (f16_mppi_sample, f16_debug_philox), the fused closed MPPI loop f16_rollout_mppi and
the Python surface on top of them (rollout_MPPI(sampler="counter", fused=...), sample_schedules).

Contract (include/f16_hip.h): under F16_FLAG_ONE_LANE the fused call equals the host loop f16_mppi_sample -> f16_rollout_cost(_rk) ->
f16_mppi_blend -> f16_rollout(_rk) -> shift bit for bit, for both integrators; split calls and the batch size do not change a bit;
without the flag the results agree with the flagged ones to the kernel-to-kernel band.

Every run: S = 3 rows, hold = 4, 3 periods (the shift and the period counter each act twice), traj_every = 2, ld / ld0 padded with NaN
that must survive.  The aircraft of a batch: 0 is healthy everywhere; a batch of three adds one that leaves the envelope during the
second period (near_the_ground) and one with a NaN entry in its nominal schedule (all its samples score non-finite: the sample-0 rule);
a batch of two adds one that is frozen on entry (F16_ST_ENVELOPE in its status word).  (The three cannot share one aircraft -- a frozen
aircraft's samples take no step, so their costs are finite whatever the commands -- and the issue's batches hold two or three.)"""
import ctypes

import numpy as np
import pytest

from conftest import golden
from test_gpu_rollout_cost import MPC_X, weights
from test_gpu_rollout_sched import Dev, bits, near_the_ground
from test_mppi_loop_cpu import HI, LO, VECTORS

pytestmark = pytest.mark.gpu

S, HOLD, PERIODS, EVERY = 3, 4, 3, 2
SEED, LAM, SIGMA = 11, 2.0, (0.5, 0.3, 0.4)
SHAPES = [(3, 5), (2, 64), (2, 130), (3, 256)]            # a partial wavefront; one wave; 256 lanes with idle ones; full
# (method, dt, the altitude [ft] from which the dive of near_the_ground -- about 0.069 ft per ms -- is below zero after 6 of the 12 steps)
RULES = {"euler": (1, 0.001, 0.38), "rk4": (4, 0.010, 3.8)}
EINVAL = -1


@pytest.fixture(scope="module")
def dev(hip):
    return Dev()


def one_lane():
    from f16_mpc_oop_py_amd import lib
    return lib.F16_FLAG_ONE_LANE


class Case:
    """The inputs of one closed loop on the device, padded: x [18, ld0], u [4, ld0], u_nom [S, 4, ld0], dem / u_ref [3, ld0],
    status [ld0]; ld0 = B0 + 5, ld = K * B0 + 37; NaN (status: the value it had) in the padding."""

    def __init__(self, dev, B0, K, rule, fi=1, only=None):
        from f16_mpc_oop_py_amd.lib import F16_ST
        t = dev.t
        self.dev, self.B0, self.K, self.fi = dev, B0, K, fi
        self.method, self.dt, alt = RULES[rule]
        g = golden("g567_trim_lin_lqr.npz")
        x0 = np.tile(g["trim_x_xcg25"], (B0, 1))
        x0[:, 9:12] += np.random.default_rng(B0).uniform(-0.01, 0.01, (B0, 3))      # (aircraft differ)
        u0 = x0[:, 12:16].copy()
        st0 = np.zeros(B0, dtype=np.int32)
        nom = np.tile(u0, (S, 1, 1))                                                 # [S, B0, 4]
        if B0 == 3:
            x0[1] = near_the_ground(x0[1], alt)
            nom[1, 2, 2] = np.nan
        elif B0 == 2:
            st0[1] = F16_ST["ENVELOPE"]
        dem = np.random.default_rng(7).uniform(-0.02, 0.02, (B0, 3))
        if only is not None:                                                         # that aircraft alone, as a batch of one
            x0, u0, st0, nom, dem = x0[only:only + 1], u0[only:only + 1], st0[only:only + 1], nom[:, only:only + 1], dem[only:only + 1]
            self.B0 = B0 = 1
        self.ld0, self.ld = B0 + 5, K * B0 + 37
        self.x, self.u, self.dem, self.uref = dev.soa(x0, self.ld0), dev.soa(u0, self.ld0), dev.soa(dem, self.ld0), dev.soa(u0[:, 1:4], self.ld0)
        self.nom = dev.seq(nom, self.ld0)
        self.st = t.full((self.ld0,), 3, dtype=t.int32, device="cuda:0")
        self.st[:B0] = t.as_tensor(st0, device="cuda:0")
        self.w = weights(pen=3.0)
        self.sg = (ctypes.c_double * 3)(*SIGMA)

    def nan(self, *shape):
        return self.dev.t.full(shape, float("nan"), dtype=self.dev.t.float64, device="cuda:0")

    def fused(self, flags, periods=PERIODS, period0=0, state=None, stream=None, sync=True):
        """ONE f16_rollout_mppi call from `state` (x, u, nom, st of an earlier call; default: the case's start) -> dict of every output"""
        d, p = self.dev, self.dev.p
        x, u, nom, st = [v.clone() for v in (state or (self.x, self.u, self.nom, self.st))]
        seq, cost = self.nan(S, 4, self.ld), self.nan(self.ld)
        stats, traj = self.nan(periods, 2, self.ld0), self.nan(periods * HOLD // EVERY, 18, self.ld0)
        rc = d.L.f16_rollout_mppi(d.ctx.handle, p(x), p(u), p(nom), p(self.dem), p(self.uref), ctypes.byref(self.w), self.sg, LAM, SEED, period0,
                                  p(seq), p(cost), p(stats), p(traj), p(st), self.B0, self.ld0, self.K, self.ld, periods, S, HOLD, EVERY,
                                  self.dt, 0.25, self.fi, self.method, flags, stream)
        assert rc == 0, d.L.f16_last_error()
        if sync:
            d.t.cuda.synchronize()
        return dict(x=x, u=u, nom=nom, st=st, seq=seq, cost=cost, stats=stats, traj=traj)

    def host_loop(self, flags):
        """the same loop over the stand-alone C entries, one round per period"""
        d, p, t, L, h = self.dev, self.dev.p, self.dev.t, self.dev.L, self.dev.ctx.handle
        x, u, nom, st = [v.clone() for v in (self.x, self.u, self.nom, self.st)]
        stats, traj = self.nan(PERIODS, 2, self.ld0), self.nan(PERIODS * HOLD // EVERY, 18, self.ld0)
        B, n = self.K * self.B0, HOLD // EVERY
        for k in range(PERIODS):
            xr = x[MPC_X].clone()
            xr[4:7] = self.dem
            seq, cost, ub = self.nan(S, 4, self.ld), self.nan(self.ld), self.nan(S, 4, self.ld0)
            assert L.f16_mppi_sample(h, p(nom), self.sg, SEED, k, p(seq), B, self.ld, self.B0, self.ld0, S, None) == 0
            if self.method == 1:
                rc = L.f16_rollout_cost(h, p(x), self.B0, self.ld0, p(seq), p(xr), p(self.uref), ctypes.byref(self.w), p(cost), None, None, None,
                                        B, self.ld, S * HOLD, HOLD, 1, self.dt, 0.25, self.fi, flags, None)
            else:
                rc = L.f16_rollout_cost_rk(h, p(x), self.B0, self.ld0, p(seq), p(xr), p(self.uref), ctypes.byref(self.w), p(cost), None, None, None,
                                           B, self.ld, S * HOLD, HOLD, 1, self.dt, 0.25, self.fi, self.method, flags, None)
            assert rc == 0, L.f16_last_error()
            assert L.f16_mppi_blend(h, p(cost), p(seq), LAM, p(ub), None, p(stats[k]), B, self.ld, self.B0, self.ld0, S, None) == 0
            u.copy_(ub[0])
            tr = traj[k * n:(k + 1) * n]
            if self.method == 1:
                rc = L.f16_rollout(h, p(x), p(u), p(tr), p(st), self.B0, self.ld0, HOLD, EVERY, self.dt, 0.25, self.fi, flags, None)
            else:
                rc = L.f16_rollout_rk(h, p(x), p(u), p(tr), p(st), self.B0, self.ld0, HOLD, HOLD, EVERY, self.dt, 0.25, self.fi, self.method, flags, None)
            assert rc == 0, L.f16_last_error()
            nom = t.cat((ub[1:], ub[-1:]), 0)
        t.cuda.synchronize()
        return dict(x=x, u=u, nom=nom, st=st, seq=seq, cost=cost, stats=stats, traj=traj)


def equal(a, b, keys=("x", "u", "nom", "st", "seq", "cost", "stats", "traj")):
    bad = [k for k in keys if not bits(a[k], b[k])]
    assert not bad, bad
    return True


def padding_kept(c, out):
    """NaN (status: 3) beyond B0 / K * B0 in every buffer the call writes"""
    t, B0, B = c.dev.t, c.B0, c.K * c.B0
    for k in ("x", "u", "nom", "stats", "traj"):
        assert bool(t.isnan(out[k][..., B0:]).all()), k
    assert bool(t.isnan(out["seq"][..., B:]).all()) and bool(t.isnan(out["cost"][B:]).all()) and bool((out["st"][B0:] == 3).all())


# ------------------------------------------------------------------------------------------------ 1. Philox on the device
def test_philox_on_the_device(dev):
    from f16_mpc_oop_py_amd.mppi import philox4x32_10
    rng = np.random.default_rng(1)
    ctr = np.concatenate([np.array([v[0] for v in VECTORS], dtype=np.uint32), rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64).astype(np.uint32)])
    key = np.concatenate([np.array([v[1] for v in VECTORS], dtype=np.uint32), rng.integers(0, 2 ** 32, (1000, 2), dtype=np.uint64).astype(np.uint32)])
    out = np.zeros_like(ctr)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert dev.L.f16_debug_philox(dev.ctx.handle, hp(ctr), hp(key), len(ctr), hp(out)) == 0, dev.L.f16_last_error()
    assert out[:3].tolist() == [v[2] for v in VECTORS]
    assert np.array_equal(out, philox4x32_10(ctr, key))
    assert dev.L.f16_debug_philox(dev.ctx.handle, hp(ctr), hp(key), 0, hp(out)) == 0
    assert dev.L.f16_debug_philox(dev.ctx.handle, None, hp(key), 3, hp(out)) == EINVAL


# ------------------------------------------------------------------------------------------------ 2. the sampler
def run_sample(dev, nom, sigma, K, seed, period, pad=True):
    """nom [S, B0, 4] host -> u_seq [S, 4, ld] device, and the view [S, K, B0, 4] of its lanes on the host"""
    rows, B0 = nom.shape[:2]
    B = K * B0
    ld, ld0 = (B + 37, B0 + 5) if pad else (B, B0)
    seq = dev.t.full((rows, 4, ld), float("nan"), dtype=dev.t.float64, device="cuda:0")
    sg = (ctypes.c_double * 3)(*np.broadcast_to(np.asarray(sigma, dtype=np.float64), (3,)))
    rc = dev.L.f16_mppi_sample(dev.ctx.handle, dev.p(dev.seq(nom, ld0)), sg, seed, period, dev.p(seq), B, ld, B0, ld0, rows, None)
    assert rc == 0, dev.L.f16_last_error()
    dev.t.cuda.synchronize()
    return seq, seq[:, :, :B].cpu().numpy().reshape(rows, 4, K, B0).transpose(0, 2, 3, 1)


@pytest.mark.parametrize("B0,K", SHAPES)
def test_sampler_against_the_reference(dev, B0, K):
    """|n| <= 6.8 and sigma <= 1: 1e-13 absolute is about 60 ulp of the largest perturbation -- room for the device's log / sincos, while a
    wrong word, pairing or channel order is an error of order 1."""
    from f16_mpc_oop_py_amd.mppi import normals_reference, sample_reference
    rng = np.random.default_rng(B0 * 1000 + K)
    nom = np.concatenate([rng.uniform(2000, 9000, (S, B0, 1)), rng.uniform(-3, 3, (S, B0, 3))], 2)
    sigma = [1.0, 0.25, 0.6]
    seed = 0x1234567890abcdef
    seq, got = run_sample(dev, nom, sigma, K, seed, 7)
    ref = sample_reference(nom, sigma, K, seed, 7)
    err = np.abs(got - ref).max()
    print(f"({B0}, {K}): max |device - reference| = {err:.3e}")
    assert err <= 1e-13
    assert np.array_equal(got[..., 0], ref[..., 0])                                  # the thrust row: the nominal, bit for bit
    assert bool(dev.t.isnan(seq[:, :, K * B0:]).all())                               # padding untouched
    _, zero = run_sample(dev, nom, 0.0, K, seed, 7)
    assert np.array_equal(zero.view(np.int64), np.repeat(nom[:, None], K, 1).view(np.int64))
    # near the limits: what the rule clips lies exactly on the bound, nothing lies outside, a NaN nominal stays NaN
    edge = nom.copy()
    edge[..., 1:] = np.where(rng.uniform(size=(S, B0, 3)) < 0.5, LO + 0.3, HI - 0.3)
    edge[0, 0, 3] = np.nan
    _, got = run_sample(dev, edge, 1.0, K, 5, 0)
    raw = edge[:, None, :, 1:] + normals_reference(5, 0, S, K, B0)
    v = got[..., 1:]
    assert np.isnan(v[0, :, 0, 2]).all() and np.isnan(v).sum() == K
    ok = ~np.isnan(raw)
    assert (v[ok] >= np.broadcast_to(LO, v.shape)[ok]).all() and (v[ok] <= np.broadcast_to(HI, v.shape)[ok]).all()
    over, under = ok & (raw > HI + 1e-12), ok & (raw < LO - 1e-12)
    assert over.any() and under.any()
    assert np.array_equal(v[over], np.broadcast_to(HI, v.shape)[over]) and np.array_equal(v[under], np.broadcast_to(LO, v.shape)[under])


# ------------------------------------------------------------------------------------------------ 3. fused = host loop, bit for bit
RUNS = [(b0, k, 1) for b0, k in SHAPES] + [(2, 64, 0)]


@pytest.mark.parametrize("rule", ["euler", "rk4"])
@pytest.mark.parametrize("B0,K,fi", RUNS, ids=[f"{b}x{k}-fi{f}" for b, k, f in RUNS])
def test_fused_equals_the_host_loop_bit_for_bit(dev, B0, K, fi, rule):
    from f16_mpc_oop_py_amd.lib import F16_ST, F16_ST_ENV_STATE
    c = Case(dev, B0, K, rule, fi)
    host = c.host_loop(one_lane())
    one = c.fused(one_lane())
    assert equal(one, host)
    padding_kept(c, one)
    # the blend is a real blend for the healthy aircraft
    ess = host["stats"][:, 1, 0].cpu().numpy()
    print(f"({B0}, {K}) {rule} fi {fi}: ess of aircraft 0 per period {ess}, min cost {host['stats'][:, 0, 0].cpu().numpy()}")
    assert (ess >= 1.5).all() and (K == 5 or (ess <= K / 2).all())
    st, tr = one["st"].cpu().numpy(), one["traj"].cpu().numpy()
    assert st[0] == 0
    if B0 == 3:
        # aircraft 1 leaves the envelope during the second period: inside after 4 steps, outside -- and frozen -- from step 8 on
        assert st[1] == F16_ST["ENVELOPE"] | F16_ST_ENV_STATE(2), hex(st[1])
        assert tr[1, 2, 1] >= 0 and tr[3, 2, 1] < 0 and np.array_equal(tr[3, :, 1], tr[5, :, 1])
        # aircraft 2: the NaN entry of row 1 makes every sample's cost non-finite: sample 0's rows, statistics 0; the entry reaches
        # u with the first shift and the state with the second advance
        assert (host["stats"][:, :, 2] == 0).all() and st[2] & F16_ST["NONFINITE"]
        assert bool(dev.t.isnan(one["cost"][2:K * B0:B0]).all())
    else:
        # aircraft 1 was frozen on entry: it never moves, while its samples are still drawn, scored and blended
        assert st[1] == F16_ST["ENVELOPE"] and bits(one["x"][:, 1], c.x[:, 1]) and not bits(one["u"][:, 1], c.u[:, 1])


# ------------------------------------------------------------------------------------------------ 4. split calls, batch size
@pytest.mark.parametrize("rule", ["euler", "rk4"])
def test_split_calls_and_batch_independence(dev, rule):
    c = Case(dev, 3, 5, rule)
    whole = c.fused(one_lane())
    a = c.fused(one_lane(), periods=1)
    b = c.fused(one_lane(), periods=2, period0=1, state=(a["x"], a["u"], a["nom"], a["st"]))
    assert equal(b, whole, ("x", "u", "nom", "st", "seq", "cost"))
    n = HOLD // EVERY
    assert bits(dev.t.cat((a["traj"], b["traj"])), whole["traj"]) and bits(dev.t.cat((a["stats"], b["stats"])), whole["stats"])
    assert not bits(a["traj"][:n], whole["traj"][n:2 * n])                       # (the periods do differ)
    # without period0 the second call would draw period 0's noise again
    again = c.fused(one_lane(), periods=2, period0=0, state=(a["x"], a["u"], a["nom"], a["st"]))
    assert not bits(again["seq"], whole["seq"])
    alone = Case(dev, 3, 5, rule, only=0).fused(one_lane())
    for k in ("x", "u", "st"):
        assert bits(alone[k][..., :1], whole[k][..., :1]), k
    for k in ("nom", "stats", "traj"):
        assert bits(alone[k][:, :, :1], whole[k][:, :, :1]), k
    assert bits(alone["cost"][:5], whole["cost"][0:15:3]) and bits(alone["seq"][:, :, :5], whole["seq"][:, :, 0:15:3])


# ------------------------------------------------------------------------------------------------ 5. default flags vs the flagged result
# Measured once on this case (MI355X, ROCm 7.2), the largest over the six runs: the blended commands (u, u_nom), relative to
# max(1, |value|), and the statistics (min cost, ess), relative: BOTH EXACTLY 0 -- observed 0.0, asserted 10 x 0.0 = 0.0.  The states
# of the Euler runs do differ (up to 1.6e-16; the RK4 runs: 0), but over 12 steps the state terms of a cost, which carry that
# difference, are small beside the command terms, which do not: the blended commands and statistics came out the same doubles.
# The margin of 10 was meant for the softmin multiplying ulp-level cost differences by cost / lambda; there is no difference to
# multiply on this case.  If a later compiler moves a cost by an ulp this assertion will say so, and the band is then that factor.
BAND_MEASURED = {"cmd": 0.0, "stats": 0.0}


def dist(a, b, relative_to_one=True):
    """max |a - b| / max(1, |b|) over the entries (NaN in the same places required)"""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(b)
    if not m.any():
        return 0.0
    return float(np.max(np.abs(a[m] - b[m]) / np.maximum(1.0 if relative_to_one else 1e-300, np.abs(b[m]))))


@pytest.mark.parametrize("rule", ["euler", "rk4"])
@pytest.mark.parametrize("B0,K", SHAPES[1:])
def test_default_flags_against_the_flagged_result(dev, B0, K, rule):
    """Without F16_FLAG_ONE_LANE the lane body of the scored LDS kernel runs: same terms, ulp-level differences.  Status words equal,
    states within 1e-9 relative (the band of tests/test_gpu_envelope.py between a fast kernel and the restatement); every aircraft --
    frozen, NaN and healthy -- takes part."""
    c = Case(dev, B0, K, rule)
    one, fast = c.fused(one_lane()), c.fused(0)
    padding_kept(c, fast)
    assert bits(fast["st"], one["st"])
    dx = max(dist(fast["x"][:, :B0], one["x"][:, :B0]), dist(fast["traj"][:, :, :B0], one["traj"][:, :, :B0]))
    dc = max(dist(fast["u"][:, :B0], one["u"][:, :B0]), dist(fast["nom"][:, :, :B0], one["nom"][:, :, :B0]))
    ds = dist(fast["stats"][:, :, :B0], one["stats"][:, :, :B0], relative_to_one=False)
    print(f"({B0}, {K}) {rule}: default vs one-lane: states {dx:.3e}, commands {dc:.3e}, stats {ds:.3e}")
    assert dx <= 1e-9
    assert dc <= 10 * BAND_MEASURED["cmd"] and ds <= 10 * BAND_MEASURED["stats"]
    # the sample sets are the same rule on nominals that agree to the band
    assert dist(fast["seq"][:, :, :K * B0], one["seq"][:, :, :K * B0]) <= 10 * BAND_MEASURED["cmd"]


# ------------------------------------------------------------------------------------------------ 6. errors and no-ops
def test_argument_errors_and_no_ops(dev):
    c = Case(dev, 2, 64, "euler")
    L, h, p, t = dev.L, dev.ctx.handle, dev.p, dev.t
    buf = dict(x=c.x.clone(), u=c.u.clone(), nom=c.nom.clone(), st=c.st.clone(), seq=c.nan(S, 4, c.ld), cost=c.nan(c.ld),
               stats=c.nan(PERIODS, 2, c.ld0), traj=c.nan(PERIODS * HOLD // EVERY, 18, c.ld0))
    keep = {k: v.clone() for k, v in buf.items()}
    inf, nan = float("inf"), float("nan")

    def call(**kw):
        a = dict(ctx=h, x=p(buf["x"]), u=p(buf["u"]), nom=p(buf["nom"]), dem=p(c.dem), uref=p(c.uref), w=c.w, sg=SIGMA, lam=LAM, seq=p(buf["seq"]),
                 cost=p(buf["cost"]), stats=p(buf["stats"]), traj=p(buf["traj"]), st=p(buf["st"]), B0=c.B0, ld0=c.ld0, K=c.K, ld=c.ld,
                 periods=PERIODS, S=S, hold=HOLD, every=EVERY, method=1)
        a.update(kw)
        w = ctypes.byref(a["w"]) if a["w"] is not None else None
        sg = (ctypes.c_double * 3)(*a["sg"]) if a["sg"] is not None else None
        rc = L.f16_rollout_mppi(a["ctx"], a["x"], a["u"], a["nom"], a["dem"], a["uref"], w, sg, a["lam"], SEED, 0, a["seq"], a["cost"], a["stats"],
                                a["traj"], a["st"], a["B0"], a["ld0"], a["K"], a["ld"], a["periods"], a["S"], a["hold"], a["every"], 0.001, 0.25, 1,
                                a["method"], one_lane(), None)
        t.cuda.synchronize()
        return rc
    bad_w = weights()
    bad_w.q[3] = -1.0
    nan_w = weights()
    nan_w.pen = nan
    for kw in ([dict(K=0), dict(K=257, ld=257 * c.B0), dict(K=-1), dict(ld=c.K * c.B0 - 1), dict(ld0=c.B0 - 1), dict(B0=-1), dict(S=0), dict(hold=0),
                dict(periods=-1), dict(every=3), dict(every=0), dict(lam=0.0), dict(lam=-1.0), dict(lam=inf), dict(lam=nan),
                dict(sg=(0.5, -0.1, 0.5)), dict(sg=(0.5, 0.5, inf)), dict(sg=(nan, 0.5, 0.5)), dict(w=bad_w), dict(w=nan_w), dict(method=2), dict(method=0)]
               + [{k: None} for k in ("ctx", "x", "u", "nom", "dem", "w", "sg", "seq", "cost")]):
        assert call(**kw) == EINVAL, kw
    # (without traj, traj_every is not looked at; u_ref, stats, traj and status may be NULL)
    assert call(traj=None, every=3, periods=0) == 0 and call(uref=None, stats=None, traj=None, st=None, periods=0) == 0
    assert call(B0=0) == 0 and call(periods=0) == 0 and call(B0=0, ld0=0, ld=0) == 0
    for k, v in buf.items():
        assert bits(v, keep[k]), k                                                  # nothing was touched by any of these
    # f16_mppi_sample: the rules of f16_mppi_blend
    seq = c.nan(S, 4, c.ld)
    sg = lambda *v: (ctypes.c_double * 3)(*v)
    smp = lambda nom=p(c.nom), s=sg(*SIGMA), out=p(seq), B=c.K * c.B0, ld=c.ld, B0=c.B0, ld0=c.ld0, rows=S: \
        L.f16_mppi_sample(h, nom, s, SEED, 0, out, B, ld, B0, ld0, rows, None)
    for kw in (dict(nom=None), dict(s=None), dict(out=None), dict(s=sg(0.1, -1.0, 0.1)), dict(s=sg(0.1, nan, 0.1)), dict(B=-1), dict(ld=c.K * c.B0 - 1),
               dict(rows=-1), dict(B0=0), dict(B=c.K * c.B0 - 1), dict(ld0=c.B0 - 1)):
        assert smp(**kw) == EINVAL, kw
    assert smp(B=0) == 0 and smp(rows=0) == 0
    t.cuda.synchronize()
    assert bool(t.isnan(seq).all())


# ------------------------------------------------------------------------------------------------ 7. graph capture
def test_fused_loop_replays_from_a_captured_graph(dev):
    """The call allocates nothing and its weights and sigmas travel in the argument block: captured on one stream and replayed twice it
    gives the eager call's bits."""
    import torch
    c = Case(dev, 2, 130, "rk4")
    ref = c.fused(0)
    d, p = dev, dev.p
    keys = ("x", "u", "nom", "st")
    start = dict(zip(keys, (c.x, c.u, c.nom, c.st)))
    out = {k: v.clone() for k, v in start.items()}
    out.update(seq=c.nan(S, 4, c.ld), cost=c.nan(c.ld), stats=c.nan(PERIODS, 2, c.ld0), traj=c.nan(PERIODS * HOLD // EVERY, 18, c.ld0))

    def call():
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        return d.L.f16_rollout_mppi(d.ctx.handle, p(out["x"]), p(out["u"]), p(out["nom"]), p(c.dem), p(c.uref), ctypes.byref(c.w), c.sg, LAM, SEED, 0,
                                    p(out["seq"]), p(out["cost"]), p(out["stats"]), p(out["traj"]), p(out["st"]), c.B0, c.ld0, c.K, c.ld, PERIODS,
                                    S, HOLD, EVERY, c.dt, 0.25, c.fi, c.method, 0, s)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert call() == 0                                  # (the kernel is loaded outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in keys:
        out[k].copy_(start[k])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert call() == 0
    for _ in range(2):
        for k in keys:
            out[k].copy_(start[k])
        for k in ("seq", "cost", "stats", "traj"):
            out[k].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert equal(out, ref)


# ------------------------------------------------------------------------------------------------ 8. the Python surface
def test_python_surface(dev):
    import torch
    from f16_mpc_oop_py_amd import F16Batch
    from f16_mpc_oop_py_amd.lib import F16_ST
    B0, K = 3, 40
    c = Case(dev, B0, K, "rk4")
    x0, u0 = c.x[:, :B0].t().cpu().numpy(), c.u[:, :B0].t().cpu().numpy()
    dem = [c.dem[k, :B0].cpu().numpy() for k in range(3)]
    args = dict(horizon=S, hold=HOLD, samples=K, sigma=list(SIGMA), lam=LAM, seed=SEED, traj_every=EVERY, method="rk4", penalty=3.0,
                q=list(c.w.q), qf=list(c.w.qf), r=list(c.w.r), u_ref=u0[:, 1:4], sampler="counter", return_info=True)
    envs = [F16Batch(x0, u0, device="cuda:0", dt=c.dt, flags=one_lane()) for _ in range(3)]
    ta, ia = envs[0].rollout_MPPI(PERIODS * HOLD, *dem, fused=True, **args)
    tb, ib = envs[1].rollout_MPPI(PERIODS * HOLD, *dem, **args)
    assert bits(ta, tb) and bits(ia["min_cost"], ib["min_cost"]) and bits(ia["ess"], ib["ess"]) and ta.shape == (PERIODS * HOLD // EVERY, 18, B0)
    assert bits(envs[0]._x, envs[1]._x) and bits(envs[0]._u, envs[1]._u) and bits(envs[0].status, envs[1].status)
    for k, shape in (("nominal", (S, B0, 4)), ("cost", (K, B0)), ("samples", (S, K, B0, 4))):
        assert tuple(envs[0].last_mppi[k].shape) == shape and bits(envs[0].last_mppi[k].contiguous(), envs[1].last_mppi[k].contiguous()), k
    assert int(envs[0].status[1]) & F16_ST["ENVELOPE"]                              # (the aircraft near the ground, without the NaN nominal)
    # period0 is the counter word of the call's first period, in both forms (the nominal schedule starts anew with every call)
    e0, e1, e2 = [F16Batch(x0, u0, device="cuda:0", dt=c.dt, flags=one_lane()) for _ in range(3)]
    tc, _ = e0.rollout_MPPI(HOLD, *dem, fused=True, period0=1, **args)
    td, _ = e1.rollout_MPPI(HOLD, *dem, period0=1, **args)
    assert bits(tc, td) and bits(e0.last_mppi["samples"].contiguous(), e1.last_mppi["samples"].contiguous()) and not bits(tc, ta[:HOLD // EVERY])
    ref = run_sample(dev, np.tile(u0, (S, 1, 1)), SIGMA, K, SEED, 1, pad=False)[1]
    assert np.array_equal(e0.last_mppi["samples"].cpu().numpy().view(np.int64), ref.view(np.int64))
    assert e2.rollout_MPPI(HOLD, *dem, fused=True, **{**args, "return_info": False, "traj_every": None}) is None
    # sample_schedules is f16_mppi_sample
    nom = np.tile(u0, (S, 1, 1))
    got = envs[0].sample_schedules(nom, list(SIGMA), K, SEED, 2)
    _, ref = run_sample(dev, nom, SIGMA, K, SEED, 2, pad=False)
    assert tuple(got.shape) == (S, K, B0, 4) and np.array_equal(got.cpu().numpy().view(np.int64), ref.view(np.int64))
    for kw in (dict(fused=True, sampler="torch"), dict(fused=True, samples=257), dict(sampler="philox")):
        with pytest.raises(ValueError):
            envs[0].rollout_MPPI(HOLD, *dem, **{**args, **kw})
