"""LQR loops on noisy sensors through a Kalman observer (f16_kalman_batch, f16_observer_step, f16_rollout_lqg_wind,
f16_rollout_lqg_wind_ens) on the device, against scipy, against the numpy restatements of f16_mpc_oop_py_amd/observer.py and against
their own contracts.

Shapes: B = 65 (a short second wave; two model groups at mgroup = 64) and B = 130 (three groups) with ld = B + 3 (padding columns
filled with NaN that must not be read), 24 steps, hold = 5, gust_hold = 2, traj_every = 3: the row boundaries interleave with the
sample points.  The filter test flies 128 aircraft for 1,500 Euler steps from the golden trim.

Bands.  f16_kalman_batch: per case the distance of kalman_reference (the same doubling in numpy) from scipy, widened by the factor
tests/test_gpu_control_mp.py grants the Riccati kernel over its twin (`allowed`: 16 x, floor 64 eps).  f16_observer_step: the
dot-product bound 13 x 2^-52 x sum|terms| per entry, an entry that reads earlier results carrying their bounds through its
coefficients; the noise within 1e-13 per unit of sigma, the band tests/test_gpu_wind.py grants gust_normals, plus the rounding of
the sum.  Everything else is bit for bit, except the zero-noise pass-through against the sibling, whose band comes from the sibling.

Measured on an MI355X: f16_kalman_batch P 6.7e-14 .. 2.6e-13 and Lf 3.7e-13 .. 7.7e-12 against scipy on the six golden cases, the
largest error / band over the 71 models 0.45; one step: noise 0.19, prediction 0.05, command 0.05 of their bounds; the zero-noise
pass-through equals the sibling bit for bit under F16_FLAG_ONE_LANE.
"""
import ctypes

import numpy as np
import pytest

import lqg_cases as lc
import rk4_cases as rk
import wind_cases as wc
from test_gpu_control_mp import allowed
from test_gpu_wind import DT, METHOD, ONE_LANE, Dev, fly, gust_sample, vp

pytestmark = pytest.mark.gpu
T, HOLD, GHOLD, EVERY = 24, 5, 2, 3
S, SG = (T + HOLD - 1) // HOLD, (T + GHOLD - 1) // GHOLD
EPS = lc.EPS
SEED, GSEED = 0x0123456789abcdef, 77
ENVELOPE = 16


@pytest.fixture(scope="module")
def dev():
    return Dev()


# ------------------------------------------------------------------------------------------------ calling the library
def kalman(d, Ad, w, v, sensed):
    """f16_kalman_batch on M models: Ad [M, 9, 9], w, v [M, 9] -> (Lf [M, 9, 9], P [M, 9, 9], iters [M], status [M])"""
    torch, M = d.torch, len(Ad)
    ld = M + 3
    dA, dw, dv = d.soa(Ad.reshape(M, 81)), d.soa(np.broadcast_to(w, (M, 9))), d.soa(np.broadcast_to(v, (M, 9)))
    Lf, Pm = (torch.full((81, ld), np.nan, dtype=torch.float64, device="cuda") for _ in range(2))
    it, st = torch.zeros(ld, dtype=torch.int32, device="cuda"), torch.zeros(ld, dtype=torch.int32, device="cuda")
    d.check(d.L.f16_kalman_batch(d.ctx.handle, vp(dA), vp(dw), vp(dv), sensed, vp(Lf), vp(Pm), vp(it), vp(st), M, ld, None))
    torch.cuda.synchronize()
    assert not st[M:].any()
    return d.back(Lf, M).reshape(M, 9, 9), d.back(Pm, M).reshape(M, 9, 9), it.cpu().numpy()[:M], st.cpu().numpy()[:M]


def h_sigma(sigma):
    arr = (ctypes.c_double * 9)(*np.broadcast_to(np.asarray(sigma, dtype=np.float64), (9,)))
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def obs_step(d, x, st, u0, K, dem, models, mgroup, sensed, sigma, mrow, xhat, flags=0):
    """one f16_observer_step -> dict(xhat [B, 9], y [B, 9], u [B, 4] (NaN where nothing was written))"""
    torch, B = d.torch, len(x)
    ld = B + 3
    dx, du0, dK, ddem, dxh = d.soa(x), d.soa(u0), d.soa(np.broadcast_to(np.asarray(K).reshape(-1, 27), (B, 27))), d.soa(dem), d.soa(xhat)
    dst = torch.zeros(ld, dtype=torch.int32, device="cuda")
    dst[:B] = torch.as_tensor(np.asarray(st, dtype=np.int32)).cuda()
    dm = torch.as_tensor(np.ascontiguousarray(models)).cuda()
    y, u = torch.full((9, ld), np.nan, dtype=torch.float64, device="cuda"), torch.full((4, ld), np.nan, dtype=torch.float64, device="cuda")
    keep, hs = h_sigma(sigma)
    d.check(d.L.f16_observer_step(d.ctx.handle, vp(dx), vp(dst), vp(du0), vp(dK), vp(ddem), vp(dm), mgroup, sensed, hs, SEED, mrow, vp(dxh), vp(y),
                                  vp(u), B, ld, flags, None))
    torch.cuda.synchronize()
    return dict(xhat=d.back(dxh, B), y=d.back(y, B), u=d.back(u, B))


def lqg(d, x0, rows, method, fi, flags, wind, gen, K, u0, models, mgroup, sensed, sigma, mrow0, xhat, T=T, hold=HOLD, ghold=GHOLD, every=EVERY,
        status0=None, group=None, traj=True, still=False, gusts=None):
    """one call of f16_rollout_lqg_wind (group: f16_rollout_lqg_wind_ens) -> dict(x, traj, xhat, xhat_traj, st, u, gstate[, ens])"""
    torch, B = d.torch, len(x0)
    ld = B + 3
    x, seq, dxh = d.soa(x0), d.soa(rows), d.soa(xhat)
    st = torch.zeros(ld, dtype=torch.int32, device="cuda")
    if status0 is not None:
        st[:B] = torch.as_tensor(np.asarray(status0, dtype=np.int32)).cuda()
    ns = T // every
    tr = torch.full((ns, 18, ld), np.nan, dtype=torch.float64, device="cuda") if traj else None
    xtr = torch.full((ns, 9, ld), np.nan, dtype=torch.float64, device="cuda")
    air, keep, gs = d.libm.Wind(), [], None
    if wind is not None:
        keep.append(d.soa(wind)); air.wind_ned = keep[-1].data_ptr()
    if gusts is not None:
        keep.append(d.soa(gusts)); air.gust_seq, air.gust_hold = keep[-1].data_ptr(), ghold
    if gen is not None:
        ga, gb, gs = d.soa(gen[0]), d.soa(gen[1]), d.soa(gen[2])
        keep += [ga, gb]
        air.ga, air.gb, air.gstate, air.gust_hold, air.seed, air.row0 = ga.data_ptr(), gb.data_ptr(), gs.data_ptr(), ghold, gen[3], gen[4]
    Kd, u0d = d.soa(np.broadcast_to(np.asarray(K).reshape(-1, 27), (B, 27))), d.soa(u0)
    uo = torch.full((4, ld), np.nan, dtype=torch.float64, device="cuda")
    dm = torch.as_tensor(np.ascontiguousarray(models)).cuda()
    hk, hs = h_sigma(sigma)
    head = (d.ctx.handle, vp(x), vp(u0d), vp(Kd), vp(seq), None if still else ctypes.byref(air), vp(dm), mgroup, sensed, hs, SEED, mrow0, vp(dxh),
            vp(tr), vp(xtr))
    tail = (vp(uo), vp(st), B, ld, T, hold, every, DT, wc.XCG, fi, METHOD[method], flags, None)
    out = {}
    if group is None:
        d.check(d.L.f16_rollout_lqg_wind(*head, *tail))
    else:
        from test_gpu_ensemble import ens_back, ens_buffers
        e, t, G = ens_buffers(d, B, ns, group)
        d.check(d.L.f16_rollout_lqg_wind_ens(*head, ctypes.byref(e), *tail))
        torch.cuda.synchronize()
        out["ens"], out["traj_dev"] = ens_back(t, G), tr
    torch.cuda.synchronize()
    out.update(x=d.back(x, B), traj=None if tr is None else d.back(tr, B), xhat=d.back(dxh, B), xhat_traj=d.back(xtr, B),
               st=st.cpu().numpy()[:B].copy(), u=d.back(uo, B), gstate=None if gs is None else d.back(gs, B))
    return out


KEYS = ("x", "traj", "xhat", "xhat_traj", "st", "u", "gstate")


def same(a, b, keys=KEYS):
    return [k for k in keys if not ((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True))]


# ------------------------------------------------------------------------------------------------ the cases
def group_models(n, sensed, gain="kalman", same_model=False):
    """n model records around the xcg25 golden model (group g: Ad, Bd moved by a seeded 0.1 %), the gain by kalman_reference"""
    from f16_mpc_oop_py_amd.observer import kalman_reference, pack_models
    Ad, Bd, x_trim, _ = lc.model("xcg25")
    rng = np.random.default_rng(31)
    recs = []
    for g in range(n):
        k = 0.0 if same_model else 1e-3 * g
        A, Bm = Ad * (1.0 + k * rng.standard_normal((9, 9))), Bd * (1.0 + k * rng.standard_normal((9, 3)))
        Lf = kalman_reference(A, lc.W_FLIGHT, lc.SIGMA_FLIGHT ** 2, sensed)[1] if gain == "kalman" else np.diag([float((sensed >> c) & 1) for c in range(9)])
        assert np.isfinite(Lf).all()
        recs.append(pack_models(A[None], Bm[None], Lf[None], x_trim[None, lc.MPC_IDX], x_trim[None, 13:16])[0])
    return np.stack(recs)


def flight(B, method):
    """(x0 [B, 18], dem rows [S, B, 3], wind [B, 3], gust generator, K [3, 9], u0 [B, 4], xhat0 [B, 9]): hifi aircraft of the lattice that
    start inside the box, small demands, steady wind and generated gusts"""
    from f16_mpc_oop_py_amd.wind import gust_coefficients
    b = wc.subset(1, B)
    w, _ = wc.air(B, B + 1)
    a, bc = gust_coefficients([8.0, 6.0, 5.0], [1750.0, 1750.0, 500.0], 600.0, GHOLD * DT)
    gen = (np.tile(a, (B, 1)), np.tile(bc, (B, 1)), np.random.default_rng(3).normal(size=(B, 3)), GSEED, 5)
    rows = np.random.default_rng(B).uniform(-0.15, 0.15, (S, B, 3))
    xhat0 = b.x[:, lc.MPC_IDX] + 1e-3 * np.random.default_rng(B + 9).standard_normal((B, 9))
    return b.x, rows, w, gen, rk.lqr_gain(), b.u, xhat0


# ------------------------------------------------------------------------------------------------ 5. the filter gain
def test_kalman_batch_against_scipy(dev):
    from f16_mpc_oop_py_amd.observer import kalman_reference
    v = lc.SIGMA_DESIGN ** 2
    worst = 0.0
    for tag, sensed in lc.CASES:
        many = lc.perturbed(tag, 11 if (tag, sensed) != lc.CASES[-1] else 10, sensed + 1000 * lc.TAGS.index(tag))      # 65 perturbed models over the six cases
        Ad = np.concatenate((lc.model(tag)[0][None], many))
        Lf, Pm, it, st = kalman(dev, Ad, lc.W_DESIGN, v, sensed)
        unsensed = [k for k in range(9) if k not in lc.channels(sensed)]
        assert np.all(Lf[:, :, unsensed] == 0.0) and not np.signbit(Lf[:, :, unsensed]).any()
        for m in range(len(Ad)):
            Ps, Ls = lc.scipy_filter(Ad[m], lc.W_DESIGN, v, sensed)
            Pr, Lr, itr = kalman_reference(Ad[m], lc.W_DESIGN, v, sensed)
            eP, eL, bP, bL = lc.relerr(Pm[m], Ps), lc.relerr(Lf[m], Ls), allowed(lc.relerr(Pr, Ps)), allowed(lc.relerr(Lr, Ls))
            worst = max(worst, eP / bP, eL / bL)
            if m == 0 or eP > bP or eL > bL:
                print(f"MEASURED f16_kalman_batch {tag} sensed={sensed:#x} model {m}: {it[m]} doublings (numpy {itr}), P {eP:.2e} (band {bP:.2e}), Lf {eL:.2e} (band {bL:.2e})")
            assert st[m] == 0 and it[m] < 60 and eP <= bP and eL <= bL, (tag, sensed, m)
    print(f"MEASURED largest error / band over all models: {worst:.2f}")


def test_kalman_batch_flags_what_does_not_converge_and_nothing_else(dev):
    """an undetectable unstable mode (Ad = 1.01 I, only phi sensed) between two models that converge: F16_ST_QP_MAXITER on that model
    alone, the neighbours' results those of a call without it, bit for bit; rates only (0x70) on the golden model is ill-conditioned
    but converges"""
    v = lc.SIGMA_DESIGN ** 2
    good = 0.9 * np.eye(9) + 0.01 * np.random.default_rng(2).standard_normal((9, 9))
    Lf, Pm, it, st = kalman(dev, np.stack([good, 1.01 * np.eye(9), good]), lc.W_DESIGN, v, 0x01)
    Lf2, Pm2, it2, st2 = kalman(dev, np.stack([good, good]), lc.W_DESIGN, v, 0x01)
    assert list(st) == [0, 64, 0] and it[1] == 60 and list(st2) == [0, 0]
    assert np.array_equal(Lf[[0, 2]], Lf2) and np.array_equal(Pm[[0, 2]], Pm2) and np.array_equal(it[[0, 2]], it2)
    _, _, it3, st3 = kalman(dev, lc.model("xcg25")[0][None], lc.W_DESIGN, v, 0x70)
    print(f"MEASURED rates only (0x70): {it3[0]} doublings, status {st3[0]}")
    assert st3[0] == 0 and it3[0] < 60


# ------------------------------------------------------------------------------------------------ 6. one step
@pytest.mark.parametrize("B", [65, 130])
def test_observer_step_against_the_reference(dev, B):
    from f16_mpc_oop_py_amd.observer import meas_normals, observer_reference
    x0, rows, _, _, K, u0, xhat0 = flight(B, "euler")
    models = group_models((B + 63) // 64, 0x7f)
    st0 = np.zeros(B, dtype=np.int32)
    st0[3] = ENVELOPE                                                          # a frozen aircraft: nothing of it is touched
    mrow = 0xfffffffe
    got = obs_step(dev, x0, st0, u0, K, rows[0], models, 64, 0x7f, lc.SIGMA_FLIGHT, mrow, xhat0)
    x9, s = x0[:, lc.MPC_IDX], x0[:, 13:16]
    live = np.arange(B) != 3
    assert np.array_equal(got["xhat"][3], xhat0[3]) and np.isnan(got["u"][3]).all() and np.isnan(got["y"][3]).all()
    # the noise
    n = meas_normals(SEED, mrow, 1, B, 0x7f)[0]
    ch = lc.channels(0x7f)
    want_y = x9 + (lc.SIGMA_FLIGHT * n)
    err_y = np.abs(got["y"] - want_y)[live][:, ch]
    band_y = (1e-13 * lc.SIGMA_FLIGHT + EPS * np.abs(want_y))[live][:, ch]
    print(f"MEASURED B={B} measurement noise: largest error / band {(err_y / band_y).max():.2e}")
    assert (err_y <= band_y).all() and np.isnan(got["y"][:, 7:]).all()
    # the rule, fed the device's own measurements
    r = observer_reference(models, 64, 0x7f, x9, s, xhat0, K, rows[0], u0, y=np.where(np.isnan(got["y"]), 0.0, got["y"]))
    Ad = models[np.arange(B) // 64][:, :81].reshape(B, 9, 9)
    b_xh = 13 * EPS * r["mag_xh"]
    b_xm = 13 * EPS * r["mag_xm"] + np.einsum("bij,bj->bi", np.abs(Ad), b_xh)
    b_u = 13 * EPS * r["mag_u"] + b_xh[:, 4:7] @ np.abs(np.asarray(K)[:, 4:7]).T
    e_xm, e_u = np.abs(got["xhat"] - r["xm"])[live], np.abs(got["u"][:, 1:] - r["u"][:, 1:])[live]
    print(f"MEASURED B={B} one step: prediction error / bound {(e_xm / b_xm[live]).max():.2e}, command error / bound {(e_u / b_u[live]).max():.2e}")
    assert (e_xm <= b_xm[live]).all() and (e_u <= b_u[live]).all() and np.array_equal(got["u"][live, 0], u0[live, 0])
    # unsensed channels draw nothing: with 0x0f no call j >= 1 is made, and call 0 is the one of the 0x7f run
    few = obs_step(dev, x0, st0, u0, K, rows[0], group_models((B + 63) // 64, 0x0f, gain="passthrough"), 64, 0x0f, lc.SIGMA_FLIGHT, mrow, xhat0)
    assert np.array_equal(few["y"][live][:, :4], got["y"][live][:, :4]) and np.isnan(few["y"][:, 4:]).all()
    # one model for the whole batch (mgroup = 0) is group 0's
    one = obs_step(dev, x0[:64], st0[:64], u0[:64], K, rows[0][:64], models[:1], 0, 0x7f, lc.SIGMA_FLIGHT, mrow, xhat0[:64])
    assert all(np.array_equal(one[k], got[k][:64], equal_nan=True) for k in ("xhat", "y", "u"))


# ------------------------------------------------------------------------------------------------ 7. fused equals the chain
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_one_call_equals_the_chain_of_steps_under_one_lane(dev, method):
    """f16_rollout_lqg_wind against 24 x (f16_observer_step -> one step of f16_rollout_wind with that u_cmd); a gust row is generated
    by the first step of its two and handed to the second as a one-row gust_seq (the generator's state IS the row in use)"""
    B = 65
    x0, rows, w, gen, K, u0, xhat0 = flight(B, method)
    models = group_models(2, 0x7f)
    mrow0 = 0xfffffff0                                                         # (the counter wraps inside the flight)
    one = lqg(dev, x0, rows, method, 1, ONE_LANE, w, gen, K, u0, models, 64, 0x7f, lc.SIGMA_FLIGHT, mrow0, xhat0)
    x, st, xh, gs, ucmd = x0, np.zeros(B, dtype=np.int32), xhat0, gen[2], u0.copy()
    traj, xtraj = [], []
    for t in range(T):
        o = obs_step(dev, x, st, u0, K, rows[t // HOLD], models, 64, 0x7f, lc.SIGMA_FLIGHT, (mrow0 + t) & 0xffffffff, xh, flags=ONE_LANE)
        xh = o["xhat"]
        ucmd = np.where(np.isnan(o["u"]), ucmd, o["u"])
        if t % GHOLD == 0:
            r = fly(dev, x, ucmd[None], method, 1, ONE_LANE, w, gen=(gen[0], gen[1], gs, GSEED, gen[4] + t // GHOLD), T=1, hold=1, ghold=1, status0=st)
            gs = r["gstate"]
        else:
            r = fly(dev, x, ucmd[None], method, 1, ONE_LANE, w, gusts=gs[None], T=1, hold=1, ghold=1, status0=st)
        x, st = r["x"], r["st"]
        if (t + 1) % EVERY == 0:
            traj.append(x)
            xtraj.append(xh)
    flying = (st & ENVELOPE) == 0
    print(f"MEASURED chain {method}: {flying.sum()} of {B} aircraft flying at the end")
    assert flying.sum() >= 0.9 * B
    chain = dict(x=x, traj=np.stack(traj), xhat=xh, xhat_traj=np.stack(xtraj), st=st, gstate=gs)
    assert not same(one, chain, ("x", "traj", "xhat", "xhat_traj", "st", "gstate")), method
    assert np.array_equal(one["u"][flying], ucmd[flying])                      # (u_out of an aircraft frozen before a row change is u0)
    assert not np.array_equal(one["x"], lqg(dev, x0, rows, method, 1, ONE_LANE, w, gen, K, u0, models, 64, 0x7f, 0.0, mrow0, xhat0)["x"])   # the noise acts


# ------------------------------------------------------------------------------------------------ 8. split calls
@pytest.mark.parametrize("flags", [0, ONE_LANE])
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_split_calls_continue_one_flight(dev, method, flags):
    B, n = 130, 10                                                             # n: a multiple of hold and gust_hold
    x0, rows, w, gen, K, u0, xhat0 = flight(B, method)
    models = group_models(3, 0x7f, same_model=flags == ONE_LANE)
    args = (K, u0, models, 64, 0x7f, lc.SIGMA_FLIGHT)
    one = lqg(dev, x0, rows, method, 1, flags, w, gen, *args, 7, xhat0)
    # (the halves store every step: the whole flight's sample points are no multiples of traj_every inside them)
    f1 = lqg(dev, x0, rows, method, 1, flags, w, gen, *args, 7, xhat0, T=n, every=1)
    f2 = lqg(dev, f1["x"], rows[n // HOLD:], method, 1, flags, w, (gen[0], gen[1], f1["gstate"], GSEED, gen[4] + n // GHOLD), *args, 7 + n, f1["xhat"],
             T=T - n, status0=f1["st"], every=1)
    assert not same(one, f2, ("x", "xhat", "st", "u", "gstate")), (method, flags)
    at = [(k + 1) * EVERY - 1 for k in range(T // EVERY)]
    for key in ("traj", "xhat_traj"):
        assert np.array_equal(one[key], np.concatenate((f1[key], f2[key]))[at], equal_nan=True), (method, flags, key)
    if flags == ONE_LANE:                                                      # an aircraft's result does not depend on the batch size
        m = 65
        small = lqg(dev, x0[:m], rows[:, :m], method, 1, flags, w[:m], (gen[0][:m], gen[1][:m], gen[2][:m], GSEED, gen[4]), K, u0[:m], models[:2], 64,
                    0x7f, lc.SIGMA_FLIGHT, 7, xhat0[:m])
        cut = {k: (v[:m] if v.ndim <= 2 else v[:, :m]) for k, v in one.items() if k in KEYS}
        assert not same(cut, small), method


# ------------------------------------------------------------------------------------------------ 9. pass-through without noise
def test_passthrough_without_noise_is_the_sibling_to_rounding(dev):
    """passthrough(0x70), sigma = 0, 24 steps, B = 65 against f16_rollout_lqr_wind: the estimate of the rates is xm + (y - xm), the
    rates to rounding.  Both bands come from the sibling, the parent's code, flown in this test, and are taken per state over the
    batch at the final state; both are printed beside the measured difference.
      F16_FLAG_ONE_LANE: both kernels step through the one out-of-line plant step and only the observer's arithmetic separates them.
        Band: f16_rollout_lqr_wind flown twice, the second time with u0[1..3] moved by one ulp, 16 x the largest difference.
      Default flags: each kernel inlines the plant step and contracts it with its surroundings (include/f16_hip.h says so of the
        ensemble twin), so the twin differs from the sibling by roundings of the plant step that a moved command does not reach.
        Band: 16 x the sibling's own distance between its default kernel and its F16_FLAG_ONE_LANE kernel -- the same step inlined
        and out of line, which is that contraction and nothing else -- plus the command band above.
    Measured on an MI355X: see the MEASURED lines (F16_FLAG_ONE_LANE: the difference is zero in every state)."""
    B = 65
    x0, rows, w, gen, K, u0, xhat0 = flight(B, "euler")
    models = group_models(2, 0x70, gain="passthrough")
    u1 = u0.copy()
    u1[:, 1:] = np.nextafter(u0[:, 1:], np.inf)
    sibling = lambda flags, u: fly(dev, x0, rows, "euler", 1, flags, w, gen=gen, K=K, u0=u, T=T, hold=HOLD, ghold=GHOLD, every=EVERY)
    twin = lambda flags: lqg(dev, x0, rows, "euler", 1, flags, w, gen, K, u0, models, 64, 0x70, 0.0, 0, xhat0)
    got, sib, sib2 = twin(ONE_LANE), sibling(ONE_LANE, u0), sibling(ONE_LANE, u1)
    got0, sib0 = twin(0), sibling(0, u0)
    ok = ((sib["st"] | sib2["st"] | got["st"] | got0["st"] | sib0["st"]) & ENVELOPE) == 0
    assert ok.sum() >= 0.9 * B
    cmd = 16 * np.abs(sib["x"] - sib2["x"])[ok].max(0)
    diff = np.abs(got["x"] - sib["x"])[ok].max(0)
    print(f"MEASURED pass-through against the sibling under F16_FLAG_ONE_LANE, {ok.sum()} aircraft: band per state {cmd}\n  difference per state {diff}")
    assert (diff <= cmd).all() and np.array_equal(got["st"], sib["st"]) and np.array_equal(got["gstate"], sib["gstate"])
    band0 = 16 * np.abs(sib0["x"] - sib["x"])[ok].max(0) + cmd
    diff0 = np.abs(got0["x"] - sib0["x"])[ok].max(0)
    print(f"MEASURED pass-through against the sibling under default flags: band per state {band0}\n  difference per state {diff0}")
    assert (diff0 <= band0).all() and np.array_equal(got0["st"], sib0["st"]) and np.array_equal(got0["gstate"], sib0["gstate"])


# ------------------------------------------------------------------------------------------------ 10. the ensemble twin
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_ensemble_twin(dev, method):
    from test_gpu_ensemble import equal, from_traj
    B, group = 130, 64
    x0, rows, w, gen, K, u0, xhat0 = flight(B, method)
    args = (K, u0, group_models(3, 0x7f), 64, 0x7f, lc.SIGMA_FLIGHT, 3, xhat0)
    for flags in (0, ONE_LANE):
        full = lqg(dev, x0, rows, method, 1, flags, w, gen, *args, group=group)
        bare = lqg(dev, x0, rows, method, 1, flags, w, gen, *args, group=group, traj=False)
        equal(full["ens"], bare["ens"], "without traj")
        assert not same(full, bare, ("x", "xhat", "xhat_traj", "st", "u", "gstate"))
        equal(full["ens"], from_traj(dev, full["traj_dev"], B, group, flags), "f16_ens_from_traj of its own samples")
    plain = lqg(dev, x0, rows, method, 1, ONE_LANE, w, gen, *args)
    assert not same(full, plain), method
    still = lqg(dev, x0, rows, method, 1, ONE_LANE, None, None, *args, group=group, still=True)           # a NULL h_wind: zero air, no forward
    zero = lqg(dev, x0, rows, method, 1, ONE_LANE, np.zeros((B, 3)), None, *args, group=group)
    assert not same(still, zero)
    equal(still["ens"], zero["ens"], "a NULL h_wind")


# ------------------------------------------------------------------------------------------------ 11. the filter filters
def test_the_filter_filters_on_the_device(dev):
    """128 aircraft from the xcg25 golden trim, 1,500 Euler steps of 1 ms, sensors 0x7f with 0.5 deg/s on the rates: the rms error of
    the (p, q, r) estimate over the last two thirds, averaged over the batch, with the gain of f16_kalman_batch below half of
    pass-through's.  The estimate sampled is the PREDICTION of the stored state (include/f16_hip.h), and pass-through's prediction
    carries its open-loop flap states and the raw noise of seven channels through Ad -- an easy baseline.  So the filter is also held
    to half of what pass-through's CORRECTED estimate has, which is the measurement itself: an rms error of sigma, 0.5 deg/s.
    (On the CPU oracle plant, tests/test_lqg_cpu.py, prediction and corrected estimate of the filter differ by 2 % in rms.)
    Measured on an MI355X: Kalman / sigma 0.073, 0.177, 0.074; Kalman / pass-through's prediction 1.8e-3, 4.0e-5, 2.4e-4."""
    from f16_mpc_oop_py_amd.observer import pack_models
    B, N = 128, 1500
    Ad, Bd, x_trim, K = lc.model("xcg25")
    Lf, _, it, st = kalman(dev, Ad[None], lc.W_FLIGHT, lc.SIGMA_FLIGHT ** 2, 0x7f)
    assert st[0] == 0
    x0, u0 = np.tile(x_trim, (B, 1)), np.tile(x_trim[12:16], (B, 1))
    rms = {}
    for name, gain in (("kalman", Lf[0]), ("passthrough", np.diag([1.0] * 7 + [0.0] * 2))):
        models = pack_models(Ad[None], Bd[None], gain[None], x_trim[None, lc.MPC_IDX], x_trim[None, 13:16])
        r = lqg(dev, x0, np.zeros((1, B, 3)), "euler", 1, 0, None, None, K, u0, models, 0, 0x7f, lc.SIGMA_FLIGHT, 0, x0[:, lc.MPC_IDX], T=N, hold=N,
                every=1, still=True)
        assert np.isfinite(r["x"]).all() and np.isfinite(r["traj"]).all() and np.isfinite(r["xhat_traj"]).all() and not r["st"].any(), name
        err = r["xhat_traj"][N // 3:, :, 4:7] - r["traj"][N // 3:][:, :, [9, 10, 11]]
        rms[name] = np.sqrt((err ** 2).mean((0, 1)))
    ratio = rms["kalman"] / rms["passthrough"]
    raw = rms["kalman"] / lc.SIGMA_FLIGHT[4:7]
    print(f"MEASURED rms error of the (p, q, r) estimate, Kalman / pass-through ({it[0]} doublings): {ratio}; Kalman / sigma: {raw}")
    assert (ratio < 0.5).all() and (raw < 0.5).all()


# ------------------------------------------------------------------------------------------------ the Python layer
def test_python_keywords_fly_the_observer(dev):
    import torch
    from f16_mpc_oop_py_amd import F16Batch
    from f16_mpc_oop_py_amd.observer import Observer
    from f16_mpc_oop_py_amd.wind import GustModel
    B = 130
    Ad, Bd, x_trim, K = lc.model("xcg25")
    src = (Ad, Bd, x_trim, x_trim[12:16])
    obs, info = Observer.build(src, lc.W_FLIGHT, lc.SIGMA_FLIGHT, sensed=0x7f, context=dev.ctx, return_info=True)
    assert info["status"][0] == 0 and np.abs(obs.models[0, 108:189]).max() > 0
    Kb = torch.as_tensor(np.broadcast_to(K, (B, 3, 9)).copy())
    fl = lambda: F16Batch(np.tile(x_trim, (B, 1)), np.tile(x_trim[12:16], (B, 1)), xcg=0.25, device="cuda:0", context=dev.ctx)
    env = fl()
    traj, est = env.rollout_LQR(24, 0.0, 0.0, 0.0, K=Kb, observer=obs, meas_seed=5, traj_every=3, return_estimate=True,
                                gusts=GustModel(5.0, 1750.0, 700.0, seed=5, every=2))
    assert tuple(traj.shape) == (8, 18, B) and tuple(est.shape) == (8, 9, B) and obs.row == 24
    assert torch.isfinite(traj).all() and not torch.equal(est[:, 4:7], traj[:, 9:12]) and not env.status.any()
    # two calls continue one flight: 10 + 14 steps are the 24 (a second batch of the same size starts a flight of its own)
    env2 = fl()
    gm = GustModel(5.0, 1750.0, 700.0, seed=5, every=2)
    env2.rollout_LQR(10, 0.0, 0.0, 0.0, K=Kb, observer=obs, meas_seed=5, gusts=gm)
    env2.rollout_LQR(14, 0.0, 0.0, 0.0, K=Kb, observer=obs, meas_seed=5, gusts=gm)
    assert torch.equal(env2._x, env._x) and obs.row == 24
    ens, est2 = fl().rollout_LQR(24, 0.0, 0.0, 0.0, K=Kb, observer=obs, meas_seed=5, traj_every=3, return_estimate=True, ensemble=64,
                                 gusts=GustModel(5.0, 1750.0, 700.0, seed=5, every=2))
    assert tuple(ens.mean.shape) == (8, 3, 18) and int(ens.count.sum()) == 8 * B and tuple(est2.shape) == (8, 9, B)
