"""Rollouts and LQR loops in steady wind and sampled gusts (f16_xdot_wind_batch, f16_rollout_wind, f16_rollout_lqr_wind,
f16_gust_sample) on the device, against the numpy twin of tests/wind_cases.py and against their own contracts.

Shapes: B = 65 and 257 with ld = B + 3 (a partial workgroup, a second workgroup, padding columns filled with NaN that must not be
read), 40 steps, hold = 7 and gust_hold = 3 (the boundaries interleave and the last segment of each is short); the single derivative
on every third aircraft of the lattices.  The 128- and 256-lane kernels run in a child process each (the launch rules read
F16_DYN_BLOCK once per process), one after another under a timeout of their own; a child that fails stops the ones after it.

Bands.  States where states_ok (finite, and not near a table edge -- judged on the AIR triple -- or the box, or with one-ulp twins
within 1e-12), status words where status_ok: the per-aircraft rule of tests/test_gpu_rollout_rk4.py, 1e-9 relative for rollouts and
1e-11 for one derivative (tests/test_gpu_dynamics.py), each widened per aircraft by the twin's reconstruction error alone --
wind_cases.band: the factor 1 + e_rec / 2^-52 with e_rec = |twin(zero wind) - oracle.calc_xdot| at the aircraft's initial state, a
CPU number, reference against reference.  Over the batches used here e_rec has median 6e-16..9e-16 and maximum 8.6e-14 (tests/
test_wind_cpu.py prints them), so the factors are 4 to 5 for the typical aircraft and at most 390: 5e-9 typical, 3.9e-7 at most for
a rollout.  At least 90 % of every batch is compared (asserted; the twin alone gives 98 % and more).
The numerical pin of the moving-air derivative is tests/test_gpu_air.py (the `long double` plant, 8 Y, no row left out); this module
keeps the contracts between kernels and the comparison with the twin.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import envelope_cases as ec
import rk4_cases as rk
import wind_cases as wc

pytestmark = pytest.mark.gpu
ROLLOUT_TOL, XDOT_TOL = 1e-9, 1e-11
ONE_LANE = 4      # F16_FLAG_ONE_LANE
EULER, RK4 = 1, 4
METHOD = {"euler": EULER, "rk4": RK4}
T, HOLD, GHOLD, DT = wc.T_MAX, wc.HOLD, wc.GUST_HOLD, 0.001
S, SG = (T + HOLD - 1) // HOLD, (T + GHOLD - 1) // GHOLD


# ------------------------------------------------------------------------------------------------ calling the library
class Dev:
    def __init__(self):
        import torch
        from f16_mpc_oop_py_amd import lib
        self.torch, self.libm = torch, lib
        self.ctx = lib.Context(0)
        self.L = self.ctx.lib

    def soa(self, a, pad=3):
        """[..., B, k] host -> [..., k, B + pad] device, the padding NaN"""
        a = np.asarray(a, dtype=np.float64)
        out = np.full(a.shape[:-2] + (a.shape[-1], a.shape[-2] + pad), np.nan)
        out[..., :a.shape[-2]] = np.swapaxes(a, -1, -2)
        return self.torch.as_tensor(out).cuda()

    def back(self, t, B):
        return np.swapaxes(t.cpu().numpy()[..., :B], -1, -2).copy()

    def check(self, rc):
        self.libm.check(rc, self.L)


@pytest.fixture(scope="module")
def dev():
    return Dev()


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def fly(d, x0, rows, method, fi, flags=0, wind=None, gusts=None, gen=None, K=None, u0=None, T=T, hold=HOLD, ghold=GHOLD, every=1, status0=None,
        still=False):
    """one call of f16_rollout_wind / f16_rollout_lqr_wind (K given).  gen = (a [B, 3], b [B, 3], gstate [B, 3], seed, row0): in-kernel
    gusts.  still: a NULL h_wind.  -> dict(x [B, 18], traj [T / every, B, 18], st [B], u [B, 4] or None, gstate [B, 3] or None)"""
    torch, B = d.torch, len(x0)
    ld = B + 3
    x, seq = d.soa(x0), d.soa(rows)
    st = torch.zeros(ld, dtype=torch.int32, device="cuda")
    if status0 is not None:
        st[:B] = torch.as_tensor(np.asarray(status0, dtype=np.int32)).cuda()
    traj = torch.full((T // every, 18, ld), np.nan, dtype=torch.float64, device="cuda") if every else None
    air, keep = d.libm.Wind(), []
    if wind is not None:
        keep.append(d.soa(wind)); air.wind_ned = keep[-1].data_ptr()
    if gusts is not None:
        keep.append(d.soa(gusts)); air.gust_seq, air.gust_hold = keep[-1].data_ptr(), ghold
    gs = None
    if gen is not None:
        ga, gb, gs = d.soa(gen[0]), d.soa(gen[1]), d.soa(gen[2])
        keep += [ga, gb]
        air.ga, air.gb, air.gstate, air.gust_hold, air.seed, air.row0 = ga.data_ptr(), gb.data_ptr(), gs.data_ptr(), ghold, gen[3], gen[4]
    h = None if still else ctypes.byref(air)
    tail = (B, ld, T, hold, max(every, 1), DT, wc.XCG, fi, METHOD[method], flags, None)
    if K is None:
        uo = None
        d.check(d.L.f16_rollout_wind(d.ctx.handle, vp(x), vp(seq), h, vp(traj), vp(st), *tail))
    else:
        Kd, u0d = d.soa(np.broadcast_to(np.asarray(K).reshape(1, 27), (B, 27))), d.soa(u0)
        uo = torch.full((4, ld), np.nan, dtype=torch.float64, device="cuda")
        d.check(d.L.f16_rollout_lqr_wind(d.ctx.handle, vp(x), vp(u0d), vp(Kd), vp(seq), h, vp(traj), vp(uo), vp(st), *tail))
    torch.cuda.synchronize()
    return dict(x=d.back(x, B), traj=None if traj is None else d.back(traj, B), st=st.cpu().numpy()[:B].copy(),
                u=None if uo is None else d.back(uo, B), gstate=None if gs is None else d.back(gs, B))


def same(a, b, keys=("x", "traj", "st", "u", "gstate")):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


# ------------------------------------------------------------------------------------------------ the cases shared with their twin
def flight(name):
    """(batch, rows, method, wind, gusts, K, u0) of a named flight: B, fidelity, method, law"""
    B, fi, method, lqr = {"hifi_rk4_257": (257, 1, "rk4", False), "hifi_euler_65": (65, 1, "euler", False),
                          "hifi_lqr_rk4_65": (65, 1, "rk4", True), "lofi_lqr_euler_257": (257, 0, "euler", True)}[name]
    b = wc.subset(fi, B)
    w, g = wc.air(B, B + fi, rows=SG)
    if lqr:
        rows = np.random.default_rng(B).uniform(-0.15, 0.15, (S, B, 3))
        return b, rows, method, w, g, rk.lqr_gain(), b.u
    rows = np.random.default_rng(B + 1).uniform([0, -30, -25, -35], [20000, 30, 25, 35], (S, B, 4))      # the full command ranges
    return b, rows, method, w, g, None, None


FLIGHTS = ("hifi_rk4_257", "hifi_euler_65", "hifi_lqr_rk4_65", "lofi_lqr_euler_257")


def twin(oracle, name):
    b, rows, method, w, g, K, u0 = flight(name)
    return wc.record(oracle, name, b, rows, HOLD, T, DT, method, w, g, GHOLD, K, u0)


def against_the_twin(oracle, name, got, tag):
    b = flight(name)[0]
    r = twin(oracle, name)
    tol = wc.band(ROLLOUT_TOL, wc.reconstruction_error(oracle, b))
    ok, okst = r["states_ok"], r["status_ok"]
    assert ok.mean() >= 0.9 and okst.mean() >= 0.9, (name, ok.mean(), okst.mean())
    assert got["traj"].shape == r["traj"].shape and np.array_equal(got["traj"][-1], got["x"], equal_nan=True)
    err = ec.rel(got["traj"], r["traj"]).max((0, 2))
    if r["u_last"] is not None:
        err = np.maximum(err, ec.rel(got["u"], r["u_last"]).max(1))
    worst = float((err[ok] / tol[ok]).max())
    print(f"MEASURED {tag} {name}: largest error {err[ok].max():.2e}, largest error / band {worst:.2e}, compared {ok.mean():.3f}")
    assert worst < 1.0, (name, np.nonzero(ok & (err >= tol))[0][:5], err[ok].max())
    assert np.array_equal(got["st"][okst], r["status"][okst]), (name, np.nonzero(okst & (got["st"] != r["status"]))[0][:5])


def xdot_case(oracle, fi):
    """the single-derivative batch: every third aircraft of the lattice, wind up to 100 ft/s, gusts up to 30 ft/s ->
    (batch, wind [B, 3], gust [B, 3], the twin's xdot [B, 18] and grid bits [B], near [B], compared [B])"""
    b = wc.subset(fi)
    w, g = wc.air(b.B, 40 + fi)
    ref = np.array([wc.twin_xdot(oracle, b.x[k], b.u[k], w[k], g[0, k], fi) for k in range(b.B)], dtype=object)
    xd, st_ref = np.stack(ref[:, 0]), ref[:, 1].astype(np.int32)
    xa = np.stack([wc.air_state(b.x[k], w[k], g[0, k]) for k in range(b.B)])
    near = ec.near_edges(b, xa, xa[None])
    return b, w, g[0], xd, st_ref, near, np.isfinite(xd).all(1) & ~near


def invariance_case():
    """the invariance batch: (batch, horizontal wind [B, 3] up to 30 ft/s, command rows [S, B, 4], the air-triple start [B, 18])"""
    b = wc.subset(1, 257, seed=1)
    w, _ = wc.air(b.B, 5, wind_max=30.0, horizontal=True)
    rows = np.random.default_rng(9).uniform([2000, -10, -8, -10], [15000, 10, 8, 10], (S, b.B, 4))
    return b, w, rows, np.stack([wc.air_state(b.x[k], w[k], np.zeros(3)) for k in range(b.B)])


# ------------------------------------------------------------------------------------------------ 1. one derivative
@pytest.mark.parametrize("fi", [1, 0])
def test_xdot_against_the_twin(oracle, dev, fi):
    """wind up to 100 ft/s, gusts up to 30 ft/s on every third aircraft of the lattice; status words away from the table edges"""
    d = dev
    b, w, g0, xd, st_ref, near, ok = xdot_case(oracle, fi)
    B, ld = b.B, b.B + 3
    out = d.torch.full((18, ld), np.nan, dtype=d.torch.float64, device="cuda")
    st = d.torch.zeros(ld, dtype=d.torch.int32, device="cuda")
    xs, us, ws, gs = d.soa(b.x), d.soa(b.u), d.soa(w), d.soa(g0)
    d.check(d.L.f16_xdot_wind_batch(d.ctx.handle, vp(xs), vp(us), vp(ws), vp(gs), vp(out), vp(st), B, ld, wc.XCG, fi, 0, None))
    got, gst = d.back(out, B), st.cpu().numpy()[:B]
    tol = wc.band(XDOT_TOL, wc.reconstruction_error(oracle, b))
    err = ec.rel(got, xd).max(1)
    print(f"MEASURED xdot fi={fi}: largest error {err[ok].max():.2e}, largest error / band {(err[ok] / tol[ok]).max():.2e}, compared {ok.mean():.3f}")
    assert ok.mean() >= 0.9
    assert (err[ok] < tol[ok]).all(), np.nonzero(ok & (err >= tol))[0][:5]
    assert np.array_equal(gst[~near], st_ref[~near])
    # the wind acts: the derivative is not the still-air one; and both pointers NULL forward to f16_xdot_batch
    still = d.torch.full((18, ld), np.nan, dtype=d.torch.float64, device="cuda")
    d.check(d.L.f16_xdot_batch(d.ctx.handle, vp(xs), vp(us), vp(still), None, B, ld, wc.XCG, fi, 0, None))
    fwd = d.torch.full((18, ld), np.nan, dtype=d.torch.float64, device="cuda")
    d.check(d.L.f16_xdot_wind_batch(d.ctx.handle, vp(xs), vp(us), None, None, vp(fwd), None, B, ld, wc.XCG, fi, 0, None))
    assert np.array_equal(d.back(fwd, B), d.back(still, B), equal_nan=True)
    assert np.abs(got[ok, 9:12] - d.back(still, B)[ok, 9:12]).max() > 1e-3


# ------------------------------------------------------------------------------------------------ 2. rollouts and loops
@pytest.mark.parametrize("flags", [0, ONE_LANE])
@pytest.mark.parametrize("name", FLIGHTS)
def test_rollouts_against_the_twin(oracle, dev, name, flags):
    b, rows, method, w, g, K, u0 = flight(name)
    got = fly(dev, b.x, rows, method, b.fi, flags, w, g, K=K, u0=u0)
    against_the_twin(oracle, name, got, "one lane" if flags else "default")
    if K is not None:     # the law acts
        ok = twin(oracle, name)["states_ok"]
        assert np.abs(got["u"][ok, 1:] - u0[ok, 1:]).max() > 1e-3


_DEAD = []


@pytest.mark.parametrize("block", [128, 256])
def test_wider_workgroups_against_the_twin(oracle, tmp_path, block):
    """k_rollout_wind<128, ..> and <256, ..> (F16_DYN_BLOCK in a child process): the same flights, the same bands"""
    if _DEAD:
        pytest.fail(f"not started: {_DEAD[0]}")
    out = str(tmp_path / "w.npz")
    env = dict(os.environ, F16_DYN_BLOCK=str(block))
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _DEAD.append(f"the child for {block} lanes did not finish in 120 s")
        pytest.fail(_DEAD[0])
    if p.returncode != 0:
        _DEAD.append(f"the child for {block} lanes ended with status {p.returncode}: {p.stderr[-2000:]}")
        pytest.fail(_DEAD[0])
    with np.load(out) as z:
        for name in FLIGHTS:
            got = {k: (z[f"{name}/{k}"] if f"{name}/{k}" in z.files else None) for k in ("x", "traj", "st", "u")}
            against_the_twin(oracle, name, got, f"{block} lanes")


def child_main(out):
    import conftest  # noqa: F401  (puts the repository root on sys.path)
    d, res = Dev(), {}
    for name in FLIGHTS:
        b, rows, method, w, g, K, u0 = flight(name)
        got = fly(d, b.x, rows, method, b.fi, 0, w, g, K=K, u0=u0)
        res.update({f"{name}/{k}": v for k, v in got.items() if v is not None})
    np.savez(out, **res)


# ------------------------------------------------------------------------------------------------ 3. the chain
@pytest.mark.parametrize("flags", [0, ONE_LANE])
@pytest.mark.parametrize("name", ["hifi_rk4_257", "hifi_euler_65", "hifi_lqr_rk4_65", "lofi_lqr_euler_257"])
def test_one_call_equals_the_chain_of_calls(dev, name, flags):
    """split at every hold and gust_hold boundary; n + m steps equal n then m"""
    b, rows, method, w, g, K, u0 = flight(name)
    one = fly(dev, b.x, rows, method, b.fi, flags, w, g, K=K, u0=u0)
    cuts = sorted(set(range(0, T, HOLD)) | set(range(0, T, GHOLD)) | {T})
    x, st, traj, last = b.x, None, [], None
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        n = t1 - t0
        last = fly(dev, x, rows[t0 // HOLD][None], method, b.fi, flags, w, g[t0 // GHOLD][None], K=K, u0=u0, T=n, hold=n, ghold=n, status0=st)
        x, st = last["x"], last["st"]
        traj.append(last["traj"])
    chain = dict(last, traj=np.concatenate(traj))
    assert same(one, chain), name
    n = 21      # a multiple of hold and gust_hold
    first = fly(dev, b.x, rows, method, b.fi, flags, w, g, K=K, u0=u0, T=n)
    second = fly(dev, first["x"], rows[n // HOLD:], method, b.fi, flags, w, g[n // GHOLD:], K=K, u0=u0, T=T - n, status0=first["st"])
    assert same(one, dict(second, traj=np.concatenate((first["traj"], second["traj"])))), name


@pytest.mark.parametrize("name", ["hifi_rk4_257", "lofi_lqr_euler_257"])
def test_one_lane_results_do_not_depend_on_the_batch_size(dev, name):
    """under F16_FLAG_ONE_LANE the first 65 aircraft flown alone equal their columns of the 257-aircraft call, bit for bit, with
    supplied and with generated gusts (an aircraft's index is its counter word, so the first columns keep their sequences)"""
    from f16_mpc_oop_py_amd.wind import gust_coefficients
    b, rows, method, w, g, K, u0 = flight(name)
    n = 65
    a, bc = gust_coefficients([8.0, 6.0, 5.0], [1750.0, 1750.0, 500.0], 600.0, GHOLD * DT)
    A, Bc, state = np.tile(a, (b.B, 1)), np.tile(bc, (b.B, 1)), np.random.default_rng(6).normal(size=(b.B, 3))
    cut = lambda r: {k: (None if v is None else v[:n] if k == "st" else v[..., :n, :]) for k, v in r.items()}
    u0n = None if u0 is None else u0[:n]
    whole = fly(dev, b.x, rows, method, b.fi, ONE_LANE, w, g, K=K, u0=u0)
    assert same(cut(whole), fly(dev, b.x[:n], rows[:, :n], method, b.fi, ONE_LANE, w[:n], g[:, :n], K=K, u0=u0n)), name
    whole = fly(dev, b.x, rows, method, b.fi, ONE_LANE, w, gen=(A, Bc, state, 9, 3), K=K, u0=u0)
    assert same(cut(whole), fly(dev, b.x[:n], rows[:, :n], method, b.fi, ONE_LANE, w[:n], gen=(A[:n], Bc[:n], state[:n], 9, 3), K=K, u0=u0n)), name


# ------------------------------------------------------------------------------------------------ 4. gusts generated in the kernel
def gust_sample(d, a, b, state, seed, row0, nrows):
    B, ld = len(state), len(state) + 3
    gs, seq = d.soa(state), d.torch.full((nrows, 3, ld), np.nan, dtype=d.torch.float64, device="cuda")
    ga, gb = d.soa(a), d.soa(b)
    d.check(d.L.f16_gust_sample(d.ctx.handle, vp(ga), vp(gb), vp(gs), seed, row0, vp(seq), nrows, B, ld, None))
    d.torch.cuda.synchronize()
    return d.back(seq, B), d.back(gs, B)


@pytest.mark.parametrize("B", [65, 257])
def test_gust_sample_against_the_reference(dev, B):
    """the absolute band tests/test_gpu_mppi_loop.py grants the same normals against sample_reference (1e-13 per unit of sigma),
    scaled by b: every row within 1e-13 b of the recurrence restated from the DEVICE's own previous row (the carried state for the
    first), (a g(r-1)) + (b n(r)) with gust_reference's normals -- a row's band then carries nothing of the rows before it.  The
    rows are also held to gust_reference's own chain, whose rows differ from these by what the recurrence (a < 1) hands on: the
    sum of the per-row bands, at most.  Measured on an MI355X: 8.9e-16 per row (4 % of the band), 1.8e-15 against the chain."""
    from f16_mpc_oop_py_amd.wind import gust_coefficients, gust_normals, gust_reference
    a, b = gust_coefficients([5.0, 4.0, 3.0], [1750.0, 1750.0, 500.0], 700.0, 0.003)
    rng = np.random.default_rng(B)
    A, Bc, state = np.tile(a, (B, 1)), np.tile(b, (B, 1)) * rng.uniform(0.5, 1.5, (B, 1)), rng.normal(size=(B, 3))
    seed, row0, n = 0x1234567890abcdef, 0xfffffffe, SG          # (the row counter wraps inside the call)
    rows, last = gust_sample(dev, A, Bc, state, seed, row0, n)
    normals = gust_normals(seed, row0, n, B)
    prev = np.concatenate((state[None], rows[:-1]))
    err = np.abs(rows - ((A[None] * prev) + (Bc[None] * normals)))
    tol = 1e-13 * Bc[None]
    ref, _ = gust_reference(A, Bc, state, seed, row0, n)
    print(f"MEASURED gust rows B={B}: largest error {err.max():.2e}, largest error / band {(err / tol).max():.2e}; "
          f"against the reference's own chain {np.abs(rows - ref).max():.2e}")
    assert (err <= tol).all() and np.array_equal(rows[-1], last)
    assert (np.abs(rows - ref) <= np.arange(1, n + 1)[:, None, None] * tol).all()
    # continuation: n rows then m rows from the carried state equal n + m rows, bit for bit
    r1, s1 = gust_sample(dev, A, Bc, state, seed, row0, 5)
    r2, s2 = gust_sample(dev, A, Bc, s1, seed, (row0 + 5) & 0xffffffff, n - 5)
    assert np.array_equal(np.concatenate((r1, r2)), rows) and np.array_equal(s2, last)
    assert np.abs(rows).max() > 1.0 and np.abs(rows[1] - rows[0]).max() > 1e-3


@pytest.mark.parametrize("flags", [0, ONE_LANE])
@pytest.mark.parametrize("name", ["hifi_rk4_257", "lofi_lqr_euler_257", "hifi_euler_65"])
def test_fused_gusts_equal_sampled_rows_then_the_rollout(dev, name, flags):
    from f16_mpc_oop_py_amd.wind import gust_coefficients
    b, rows, method, w, _, K, u0 = flight(name)
    B = b.B
    a, bc = gust_coefficients([8.0, 6.0, 5.0], [1750.0, 1750.0, 500.0], 600.0, GHOLD * DT)
    A, Bc, state, seed, row0 = np.tile(a, (B, 1)), np.tile(bc, (B, 1)), np.random.default_rng(3).normal(size=(B, 3)), 77, 5
    seq, last = gust_sample(dev, A, Bc, state, seed, row0, SG)
    host = fly(dev, b.x, rows, method, b.fi, flags, w, seq, K=K, u0=u0)
    fused = fly(dev, b.x, rows, method, b.fi, flags, w, gen=(A, Bc, state, seed, row0), K=K, u0=u0)
    assert same(host, fused, ("x", "traj", "st", "u")) and np.array_equal(fused["gstate"], last)
    n = 21
    f1 = fly(dev, b.x, rows, method, b.fi, flags, w, gen=(A, Bc, state, seed, row0), K=K, u0=u0, T=n)
    f2 = fly(dev, f1["x"], rows[n // HOLD:], method, b.fi, flags, w, gen=(A, Bc, f1["gstate"], seed, row0 + n // GHOLD), K=K, u0=u0, T=T - n,
             status0=f1["st"])
    assert same(fused, dict(f2, traj=np.concatenate((f1["traj"], f2["traj"])))), name
    assert not np.array_equal(fused["x"], fly(dev, b.x, rows, method, b.fi, flags, w, K=K, u0=u0)["x"])       # the gusts act


# ------------------------------------------------------------------------------------------------ 5. invariance on the device
def test_horizontal_wind_carries_the_flight_along(oracle, dev):
    """RK4, 40 steps, the envelope test on: under a horizontal steady wind the air triple and states 2..5, 9..17 of the flight equal
    f16_rollout_rk's still-air flight from the air-triple start, and the position differs by w t.  Both are device flights through
    different arithmetic (the wind kernel forms the air triple through sqrt / atan2 / asin at every evaluation), so the band is the
    rollout band of the suite, widened by the reconstruction error as everywhere else; compared are the aircraft neither flight
    freezes (the box test reads the ground triple in one flight and what is the air triple in the other) and that stay off the edges."""
    d = dev
    b, w, rows, xa0 = invariance_case()
    B = b.B
    windy = fly(d, b.x, rows, "rk4", 1, 0, w)
    still = fly(d, xa0, rows, "rk4", 1, 0, still=True)
    air = np.stack([[wc.air_state(windy["traj"][t, k], w[k], np.zeros(3)) for k in range(B)] for t in range(T)])
    near = wc.near_edges_air(b, b.x, windy["traj"], np.zeros((0, B, 18)), w, np.zeros((1, B, 3)), T)
    ok = ~near & ((windy["st"] | still["st"]) & 16 == 0) & np.isfinite(still["traj"]).all((0, 2))
    tol = wc.band(ROLLOUT_TOL, wc.reconstruction_error(oracle, b))
    keep = [2, 3, 4, 5] + list(range(6, 18))
    err = ec.rel(air[..., keep], still["traj"][..., keep]).max((0, 2))
    t = DT * np.arange(1, T + 1)[:, None, None]
    drift = (windy["traj"][..., :2] - b.x[None, :, :2]) - (still["traj"][..., :2] - xa0[None, :, :2]) - w[None, :, :2] * t
    derr = np.abs(drift).max((0, 2)) / np.maximum(1.0, np.abs(windy["traj"][..., :2]).max((0, 2)))
    print(f"MEASURED invariance: states {err[ok].max():.2e}, position against w t {derr[ok].max():.2e}, compared {ok.mean():.3f}")
    assert ok.mean() >= 0.9
    assert (err[ok] < tol[ok]).all() and (derr[ok] < tol[ok]).all()
    assert np.abs(windy["traj"][-1, ok, :2] - still["traj"][-1, ok, :2] - (b.x - xa0)[ok, :2]).max() > 0.5      # the wind is there


# ------------------------------------------------------------------------------------------------ 6. NULL, frozen, NaN, refusals
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_still_air_forwards_frozen_ignores_and_nan_is_flagged(dev, method):
    d, b = dev, wc.subset(1, 65)
    B, ld = 65, 68
    rows = np.random.default_rng(2).uniform([2000, -10, -8, -10], [15000, 10, 8, 10], (S, B, 4))
    # a NULL h_wind and one with NULL pointers give f16_rollout_rk's bits
    x, seq = d.soa(b.x), d.soa(rows)
    st = d.torch.zeros(ld, dtype=d.torch.int32, device="cuda")
    traj = d.torch.full((T, 18, ld), np.nan, dtype=d.torch.float64, device="cuda")
    d.check(d.L.f16_rollout_rk(d.ctx.handle, vp(x), vp(seq), vp(traj), vp(st), B, ld, T, HOLD, 1, DT, wc.XCG, 1, METHOD[method], 0, None))
    want = dict(x=d.back(x, B), traj=d.back(traj, B), st=st.cpu().numpy()[:B], u=None, gstate=None)
    assert same(want, fly(d, b.x, rows, method, 1, still=True)) and same(want, fly(d, b.x, rows, method, 1))
    # the same for the loop: f16_rollout_lqr_wind without air is f16_rollout_lqr_rk
    dem, K = np.random.default_rng(4).uniform(-0.15, 0.15, (S, B, 3)), rk.lqr_gain()
    xl, dl, u0d, uo = d.soa(b.x), d.soa(dem), d.soa(b.u), d.torch.full((4, ld), np.nan, dtype=d.torch.float64, device="cuda")
    Kd, stl = d.soa(np.broadcast_to(K.reshape(1, 27), (B, 27))), d.torch.zeros(ld, dtype=d.torch.int32, device="cuda")
    trl = d.torch.full((T, 18, ld), np.nan, dtype=d.torch.float64, device="cuda")
    d.check(d.L.f16_rollout_lqr_rk(d.ctx.handle, vp(xl), vp(u0d), vp(Kd), vp(dl), vp(trl), vp(uo), vp(stl), B, ld, T, HOLD, 1, DT, wc.XCG, 1,
                                   METHOD[method], 0, None))
    wantl = dict(x=d.back(xl, B), traj=d.back(trl, B), st=stl.cpu().numpy()[:B], u=d.back(uo, B), gstate=None)
    assert same(wantl, fly(d, b.x, dem, method, 1, K=K, u0=b.u, still=True)) and same(wantl, fly(d, b.x, dem, method, 1, K=K, u0=b.u))
    # a frozen aircraft ignores wind and gusts; a NaN wind component is flagged and stays with its aircraft
    x0 = b.x.copy()
    x0[3, 2] = -10.0
    w, g = wc.air(B, 3, rows=SG)
    clean = fly(d, x0, rows, method, 1, 0, w, g)
    assert (clean["traj"][:, 3] == x0[3]).all() and clean["st"][3] == 16 | 1 << (8 + 2)
    w2 = w.copy()
    w2[7, 1] = np.nan
    dirty = fly(d, x0, rows, method, 1, 0, w2, g)
    assert dirty["st"][7] & 32 and np.isnan(dirty["x"][7]).any()
    others = np.arange(B) != 7
    assert same({k: (v[..., others, :] if k != "st" else v[others]) for k, v in clean.items() if v is not None},
                {k: (v[..., others, :] if k != "st" else v[others]) for k, v in dirty.items() if v is not None}, ("x", "traj", "st"))
    # refusals reach the caller as F16_EINVAL with nothing launched
    air = d.libm.Wind()
    air.gust_seq = air.ga = air.gb = air.gstate = x.data_ptr()
    air.gust_hold = 1
    rc = d.L.f16_rollout_wind(d.ctx.handle, vp(x), vp(seq), ctypes.byref(air), None, None, B, ld, T, HOLD, 1, DT, wc.XCG, 1, METHOD[method], 0, None)
    assert rc == -1 and "gust_seq and ga" in d.L.f16_last_error().decode()
    air.gust_seq, air.gust_hold = None, 0
    rc = d.L.f16_rollout_wind(d.ctx.handle, vp(x), vp(seq), ctypes.byref(air), None, None, B, ld, T, HOLD, 1, DT, wc.XCG, 1, METHOD[method], 0, None)
    assert rc == -1 and "gust_hold" in d.L.f16_last_error().decode()
    assert np.array_equal(d.back(x, B), want["x"], equal_nan=True)


def test_python_keywords_reach_the_wind_calls(dev):
    """F16Batch.rollout_schedule / rollout_LQR / _calc_xdot with wind= and gusts= equal the C calls; a GustModel continues its sequence"""
    import torch
    from f16_mpc_oop_py_amd import F16Batch
    from f16_mpc_oop_py_amd.wind import GustModel
    b, rows, method, w, g, _, _ = flight("hifi_euler_65")
    B = b.B
    env = F16Batch(b.x, b.u, xcg=wc.XCG, dt=DT, context=dev.ctx)
    traj = env.rollout_schedule(rows, hold=HOLD, nsteps=T, traj_every=1, method=method, wind=w, gusts=g, gust_every=GHOLD)
    want = fly(dev, b.x, rows, method, 1, 0, w, g)
    assert np.array_equal(traj.cpu().numpy().transpose(0, 2, 1), want["traj"]) and np.array_equal(env.status.cpu().numpy(), want["st"])
    # _calc_xdot(wind=, gust=) is f16_xdot_wind_batch on the same arrays, bit for bit (the gust differs from the wind: a swap shows)
    xd = env._calc_xdot(b.x, b.u, wind=w, gust=g[0]).cpu().numpy()
    out = dev.torch.full((18, B + 3), np.nan, dtype=dev.torch.float64, device="cuda")
    xs, us, ws, gs = dev.soa(b.x), dev.soa(b.u), dev.soa(w), dev.soa(g[0])
    dev.check(dev.L.f16_xdot_wind_batch(dev.ctx.handle, vp(xs), vp(us), vp(ws), vp(gs), vp(out), None, B, B + 3, wc.XCG, 1, 0, None))
    assert np.array_equal(xd, dev.back(out, B)) and not np.array_equal(xd, env._calc_xdot(b.x, b.u, wind=g[0], gust=w).cpu().numpy())
    assert not np.array_equal(xd, env._calc_xdot(b.x, b.u).cpu().numpy())
    only = env._calc_xdot(b.x, b.u, gust=g[0]).cpu().numpy()
    dev.check(dev.L.f16_xdot_wind_batch(dev.ctx.handle, vp(xs), vp(us), None, vp(gs), vp(out), None, B, B + 3, wc.XCG, 1, 0, None))
    assert np.array_equal(only, dev.back(out, B))
    gm = GustModel([8.0, 6.0, 5.0], [1750.0, 1750.0, 500.0], 600.0, seed=77, every=GHOLD)
    one = F16Batch(b.x, b.u, xcg=wc.XCG, dt=DT, context=dev.ctx)
    one.rollout_schedule(rows, hold=HOLD, nsteps=T, method="rk4", wind=w[0], gusts=gm)
    assert gm.row == SG
    gm.reset()
    two = F16Batch(b.x, b.u, xcg=wc.XCG, dt=DT, context=dev.ctx)
    two.rollout_schedule(rows[:3], hold=HOLD, nsteps=21, method="rk4", wind=w[0], gusts=gm)
    two.rollout_schedule(rows[3:], hold=HOLD, nsteps=T - 21, method="rk4", wind=w[0], gusts=gm)
    assert gm.row == SG and torch.equal(one.x_values, two.x_values)
    # two batches that alternate on one model each keep their own sequence
    small = F16Batch(b.x[:9], b.u[:9], xcg=wc.XCG, dt=DT, context=dev.ctx)
    both = F16Batch(b.x, b.u, xcg=wc.XCG, dt=DT, context=dev.ctx)
    gm.reset()
    both.rollout_schedule(rows[:3], hold=HOLD, nsteps=21, method="rk4", wind=w[0], gusts=gm)
    small.rollout_schedule(rows[:3, :9], hold=HOLD, nsteps=21, method="rk4", wind=w[0], gusts=gm)
    assert gm.row == 7
    both.rollout_schedule(rows[3:], hold=HOLD, nsteps=T - 21, method="rk4", wind=w[0], gusts=gm)
    assert gm.row == SG and torch.equal(one.x_values, both.x_values)
    K = torch.as_tensor(np.broadcast_to(rk.lqr_gain(), (B, 3, 9)).copy())
    lq = F16Batch(b.x, b.u, xcg=wc.XCG, dt=DT, context=dev.ctx)
    lq.rollout_LQR(T, 0.05, -0.02, 0.01, K=K, method="rk4", wind=w, gusts=g, gust_every=GHOLD)
    dem = np.broadcast_to(np.array([0.05, -0.02, 0.01]), (1, B, 3))
    want = fly(dev, b.x, dem, "rk4", 1, 0, w, g, K=rk.lqr_gain(), u0=b.u, hold=T)
    assert np.array_equal(lq.x_values.cpu().numpy(), want["x"], equal_nan=True) and np.array_equal(lq.u_values.cpu().numpy(), want["u"])


if __name__ == "__main__":
    child_main(sys.argv[1])
