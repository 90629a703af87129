"""CPU-side checks of the wind and gust entries (include/f16_hip.h: f16_xdot_wind_batch, f16_rollout_wind, f16_rollout_lqr_wind,
f16_gust_coeffs_host, f16_gust_sample): what tests/test_gpu_wind.py rests on, and everything that needs no device.

  * the numpy twin of tests/wind_cases.py, reference against reference: with zero wind it reproduces oracle.calc_xdot (its
    reconstruction error, the only thing the GPU bands are widened by), and under a horizontal steady wind the flight's air triple,
    attitude, rates and actuator states are those of the still-air flight from the air-triple start while the position differs by w t;
  * f16_gust_coeffs_host against numpy; gust_reference: continuation, independence of the batch size, the stationary deviation;
  * the argument rules of the C entry points on calls the library refuses or treats as a no-op (nothing is launched and no array is
    dereferenced: a zeroed host buffer stands for the context and for every array), and the ValueErrors of the Python keywords on
    the recording environment of tests/test_rollout_calls_cpu.py.
"""
import ctypes

import numpy as np
import pytest

import envelope_cases as ec
import wind_cases as wc
from header_cases import header_parameters, names
from test_rollout_calls_cpu import BAD_ARGUMENT, BAD_STEPS, F16_EINVAL, F16_OK, env_of
from test_rollout_rk_calls_cpu import BAD_METHOD, METHODS, clib  # noqa: F401  (clib: the fixture)

# the twin rebuilds xdot[6..8] through ~40 roundings (two conversions between the triple and body axes), each amplified by at most
# 1 / cos(beta) and by U^2 + W^2 in a quotient; on the lattices (|beta| <= 30 deg, alpha to 90 deg) 2^-52 x 40 x 16 is a generous cap
E_REC_CAP = 40 * 16 * wc.EPS
SIBLING = {"f16_rollout_wind": "f16_rollout_rk", "f16_rollout_lqr_wind": "f16_rollout_lqr_rk"}


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("fi", [1, 0])
def test_twin_with_zero_wind_is_the_reference(oracle, fi):
    for B in (None, 65, 257):
        b = wc.subset(fi, B)
        e = wc.reconstruction_error(oracle, b)
        print(f"MEASURED reconstruction error fi={fi} B={b.B}: median {np.median(e):.2e}, max {e.max():.2e}, largest band factor {1 + e.max() / wc.EPS:.0f}")
        assert e.max() < E_REC_CAP
        st = [wc.twin_xdot(oracle, b.x[k], b.u[k], np.zeros(3), np.zeros(3), fi)[1] for k in range(b.B)]
        ref = []
        for k in range(b.B):
            oracle.calc_xdot(b.x[k], b.u[k], fi, wc.XCG)
            ref.append(int(oracle.lib.f16o_last_status()))
        near = ec.near_edges(b, b.x, b.x[None])
        assert np.array_equal(np.array(st)[~near], np.array(ref)[~near])


@pytest.mark.parametrize("fi", [1, 0])
def test_twin_flight_in_horizontal_wind_is_the_still_air_flight_carried_along(oracle, fi):
    """every third aircraft of the lattice that starts inside the box, RK4, 40 steps of 1 ms, horizontal wind up to 30 ft/s (larger
    winds push more of the lattice's corner cells over a table edge in one flight and not the other; at 30 ft/s >= 90 % compare)"""
    lat = wc.subset(fi)
    inside = np.all((lat.x >= ec.X_LB) & (lat.x <= ec.X_UB), 1)
    b = ec.Batch(lat, x=lat.x[inside], u=lat.u[inside], cell=lat.cell[inside])
    B, T, dt = b.B, 40, 0.001
    w, _ = wc.air(B, 11 + fi, wind_max=30.0, horizontal=True)
    rows = b.u[None]
    xa0 = np.stack([wc.air_state(b.x[k], w[k], np.zeros(3)) for k in range(B)])
    windy = wc.fly(oracle, b.x, rows, T, T, dt, fi, "rk4", wind=w)
    still = wc.fly(oracle, xa0, rows, T, T, dt, fi, "rk4")
    air = np.stack([[wc.air_state(windy["traj"][t, k], w[k], np.zeros(3)) for k in range(B)] for t in range(T)])
    near = wc.near_edges_air(b, b.x, windy["traj"], windy["stages"], w, np.zeros((1, B, 3)), T)
    ok = ~near & (((windy["status"] | still["status"]) & 16) == 0) & np.isfinite(still["traj"]).all((0, 2)) & np.isfinite(air).all((0, 2))
    keep = list(range(2, 18))
    err = ec.rel(air[..., keep], still["traj"][..., keep]).max((0, 2))
    t = dt * np.arange(1, T + 1)[:, None, None]
    drift = (windy["traj"][..., :2] - b.x[None, :, :2]) - (still["traj"][..., :2] - xa0[None, :, :2]) - w[None, :, :2] * t
    tol = wc.band(1e-9, wc.reconstruction_error(oracle, b))
    print(f"MEASURED twin invariance fi={fi}: states {err[ok].max():.2e}, position against w t {np.abs(drift[:, ok]).max():.2e} ft, compared {ok.mean():.3f}")
    assert ok.mean() >= 0.9
    assert (err[ok] < tol[ok]).all()
    assert (np.abs(drift).max((0, 2))[ok] < tol[ok] * np.maximum(1.0, np.abs(windy["traj"][..., :2]).max((0, 2))[ok])).all()


def test_the_batches_of_the_gpu_tests_compare_nine_in_ten(oracle):
    """the shares tests/test_gpu_wind.py asserts, from the twin alone: its four flights, its two single-derivative batches and its
    invariance batch (there two device flights are compared; here the same two flights of the twin decide who is left out)"""
    from test_gpu_wind import DT, FLIGHTS, T, invariance_case, twin, xdot_case
    for name in FLIGHTS:
        r = twin(oracle, name)
        print(f"MEASURED compared {name}: states {r['states_ok'].mean():.3f}, status {r['status_ok'].mean():.3f}")
        assert r["states_ok"].mean() >= 0.9 and r["status_ok"].mean() >= 0.9, name
    for fi in (1, 0):
        ok = xdot_case(oracle, fi)[-1]
        print(f"MEASURED compared xdot fi={fi}: {ok.mean():.3f}")
        assert ok.mean() >= 0.9
    b, w, rows, xa0 = invariance_case()
    windy = wc.fly(oracle, b.x, rows, wc.HOLD, T, DT, 1, "rk4", wind=w)
    still = wc.fly(oracle, xa0, rows, wc.HOLD, T, DT, 1, "rk4")
    near = wc.near_edges_air(b, b.x, windy["traj"], np.zeros((0, b.B, 18)), w, np.zeros((1, b.B, 3)), T)
    ok = ~near & (((windy["status"] | still["status"]) & 16) == 0) & np.isfinite(still["traj"]).all((0, 2))
    print(f"MEASURED compared invariance: {ok.mean():.3f}")
    assert ok.mean() >= 0.9


# ------------------------------------------------------------------------------------------------ the gust sampler
def test_gust_coeffs_host_against_numpy():
    from f16_mpc_oop_py_amd.wind import gust_coefficients, gust_coefficients_host
    for sigma, length, v0, dt in (([5.0, 4.0, 3.0], [1750.0, 1750.0, 500.0], 700.0, 0.01), (2.5, 300.0, 250.0, 0.003), ([0.0, 1.0, 9.0], 1e4, 900.0, 1e-3)):
        a, b = gust_coefficients(sigma, length, v0, dt)
        ah, bh = gust_coefficients_host(sigma, length, v0, dt)
        assert np.all(np.abs(ah - a) <= 2 * wc.EPS * a) and np.all(np.abs(bh - b) <= 8 * wc.EPS * np.maximum(b, 1e-300) / np.sqrt(1 - a * a))
        assert np.all((0 < a) & (a < 1))
    from f16_mpc_oop_py_amd import cabi, lib
    L = cabi.declare(ctypes.CDLL(lib.build()))
    d3 = ctypes.c_double * 3
    ok = (d3(1, 1, 1), d3(100, 100, 100), 500.0, 0.01, d3(), d3())
    assert L.f16_gust_coeffs_host(*ok) == F16_OK
    for k, bad in ((0, None), (1, None), (4, None), (5, None), (0, d3(1, -1, 1)), (0, d3(1, float("nan"), 1)), (1, d3(100, 0, 100)),
                   (1, d3(100, float("inf"), 100)), (2, 0.0), (2, float("nan")), (3, -0.01), (3, float("inf"))):
        args = list(ok)
        args[k] = bad
        assert L.f16_gust_coeffs_host(*args) == F16_EINVAL, (k, bad)
    with pytest.raises(ValueError):
        gust_coefficients(1.0, -5.0, 500.0, 0.01)


def test_gust_reference_continues_and_does_not_depend_on_the_batch():
    from f16_mpc_oop_py_amd.wind import gust_coefficients, gust_reference
    a, b = gust_coefficients([5.0, 4.0, 3.0], [1750.0, 1750.0, 500.0], 700.0, 0.01)
    s0 = np.random.default_rng(0).normal(size=(9, 3))
    whole, last = gust_reference(a, b, s0, 99, 0xfffffffa, 20)
    first, s1 = gust_reference(a, b, s0, 99, 0xfffffffa, 8)
    second, s2 = gust_reference(a, b, s1, 99, 0xfffffffa + 8, 12)
    assert np.array_equal(np.concatenate((first, second)), whole) and np.array_equal(s2, last) and np.array_equal(whole[-1], last)
    few, _ = gust_reference(a, b, s0[:4], 99, 0xfffffffa, 20)
    assert np.array_equal(few, whole[:, :4])
    other, _ = gust_reference(a, b, s0, 100, 0xfffffffa, 20)
    assert not np.array_equal(other, whole)


def test_gust_reference_is_stationary_at_sigma():
    """200,000 rows with a = exp(-700 * 0.01 / 1750): the standard deviation of the sigma-5 sequence of one aircraft within 2 % of
    sigma.  Neighbouring rows are correlated (a = 0.996), so 200,000 rows carry 200,000 (1 - a) / (1 + a) = 400 independent ones
    and the deviation of ONE sequence has a standard error of 1 / sqrt(2 x 400) = 3.5 %: the three axes are therefore held to the
    same 2 % on the deviation pooled over sixteen aircraft (standard error 0.9 %), which also shows b = sigma sqrt(1 - a^2) per axis."""
    from f16_mpc_oop_py_amd.wind import gust_coefficients, gust_reference
    sigma = np.array([5.0, 4.0, 3.0])
    a, b = gust_coefficients(sigma, 1750.0, 700.0, 0.01)
    rows, _ = gust_reference(a, b, np.zeros((16, 3)), 0, 0, 200000)
    one, pooled = rows[:, 0, 0].std(), np.sqrt((rows ** 2).mean((0, 1)))
    print(f"MEASURED stationary deviation: one sequence {one:.3f} for sigma 5; pooled / sigma {pooled / sigma}")
    assert abs(one / 5.0 - 1.0) < 0.02
    assert np.all(np.abs(pooled / sigma - 1.0) < 0.02)
    assert abs(rows.mean()) < 0.2


# ------------------------------------------------------------------------------------------------ the C rules
def wind_struct(buf, **fields):
    from f16_mpc_oop_py_amd import lib
    w = lib.Wind()
    for k, v in fields.items():
        setattr(w, k, buf.value if v == "buf" else v)
    return w


def call(clib, symbol, method, wind, **over):
    """`symbol` on a call that is complete except for `over` (None = a NULL pointer): four aircraft, five steps, no traj -> (rc, message)"""
    L, buf, _, _ = clib
    base = dict(B=4, ld=4, nsteps=5, hold=2, traj_every=1, dt=1e-3, xcg=0.35, fi_flag=1, method=method, flags=0, stream=None, traj=None,
                u_out=None, status=None, h_wind=None if wind is None else ctypes.byref(wind))
    args = [over[n] if n in over else base.get(n, buf) for n in names(symbol)]
    rc = getattr(L, symbol)(*args)
    return rc, L.f16_last_error().decode()


def refused(clib, symbol, method, wind, words, **over):
    rc, msg = call(clib, symbol, method, wind, **over)
    assert rc == F16_EINVAL and words in msg, (symbol, method, over, rc, msg)


@pytest.mark.parametrize("symbol", list(SIBLING))
def test_parameter_lists_are_the_siblings_plus_the_air(symbol):
    from f16_mpc_oop_py_amd import lib
    new, old = header_parameters(symbol), header_parameters(SIBLING[symbol])
    k = [p.replace("*", " ").split()[-1] for p in old].index("traj")
    assert new == old[:k] + ["const f16_wind *h_wind"] + old[k:]
    L = lib.load()
    at, bt = getattr(L, symbol).argtypes, getattr(L, SIBLING[symbol]).argtypes
    assert list(at) == list(bt[:k]) + [ctypes.POINTER(lib.Wind)] + list(bt[k:])
    assert [f[0] for f in lib.Wind._fields_] == ["wind_ned", "gust_seq", "gust_hold", "ga", "gb", "gstate", "seed", "row0"]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("symbol", list(SIBLING))
def test_what_the_sibling_refuses_is_refused_first_then_the_wind_fields(clib, symbol, method):
    buf = clib[1]
    quiet = dict(B=0, ld=0)
    lqr = symbol == "f16_rollout_lqr_wind"
    missing = "K / dem_seq is NULL" if lqr else "u_seq is NULL"
    for wind in (None, wind_struct(buf), wind_struct(buf, wind_ned="buf"), wind_struct(buf, gust_seq="buf", ga="buf", gust_hold=0)):
        refused(clib, symbol, method, wind, BAD_ARGUMENT, ctx=None, **quiet)
        refused(clib, symbol, method, wind, BAD_ARGUMENT, x=None, **quiet)
        refused(clib, symbol, method, wind, BAD_ARGUMENT, B=4, ld=3, nsteps=0)
        refused(clib, symbol, method, wind, BAD_STEPS, nsteps=-1, **quiet)
        refused(clib, symbol, method, wind, BAD_STEPS, nsteps=5, traj=buf, traj_every=2, **quiet)
        refused(clib, symbol, method, wind, missing, **{"dem_seq" if lqr else "u_seq": None}, **quiet)
        refused(clib, symbol, method, wind, "hold must be >= 1", hold=0, **quiet)
        rc, msg = call(clib, symbol, 3, wind, **quiet)
        assert rc == F16_EINVAL and BAD_METHOD in msg
    refused(clib, symbol, method, wind_struct(buf, gust_seq="buf", ga="buf", gb="buf", gstate="buf", gust_hold=1), "gust_seq and ga are both given", **quiet)
    for some in (dict(ga="buf"), dict(ga="buf", gb="buf"), dict(gb="buf"), dict(gstate="buf", wind_ned="buf")):
        refused(clib, symbol, method, wind_struct(buf, gust_hold=1, **some), "ga, gb and gstate go together", **quiet)
    for hold in (0, -2):
        refused(clib, symbol, method, wind_struct(buf, gust_seq="buf", gust_hold=hold), "gust_hold must be >= 1", **quiet)
        refused(clib, symbol, method, wind_struct(buf, ga="buf", gb="buf", gstate="buf", gust_hold=hold), "gust_hold must be >= 1", **quiet)
    # a steady wind alone does not read gust_hold; B == 0 and nsteps == 0 are no-ops
    assert call(clib, symbol, method, wind_struct(buf, wind_ned="buf", gust_hold=-1), **quiet)[0] == F16_OK
    assert call(clib, symbol, method, wind_struct(buf, gust_seq="buf", gust_hold=3), nsteps=0)[0] == F16_OK


def test_xdot_and_gust_sample_check_their_arguments(clib):
    L, buf, _, _ = clib
    xdot = lambda **o: L.f16_xdot_wind_batch(*[o.get(n, dict(B=0, ld=0, xcg=0.35, fi_flag=1, flags=0, stream=None, status=None).get(n, buf))
                                               for n in names("f16_xdot_wind_batch")])
    assert xdot() == F16_OK and xdot(wind=None) == F16_OK and xdot(wind=None, gust=None) == F16_OK
    for bad in (dict(ctx=None), dict(x=None), dict(xdot=None), dict(u=None), dict(B=-1), dict(B=4, ld=3)):
        assert xdot(**bad) == F16_EINVAL and xdot(wind=None, gust=None, **bad) == F16_EINVAL, bad
    gs = lambda **o: L.f16_gust_sample(*[o.get(n, dict(B=0, ld=0, nrows=3, seed=1, row0=0, stream=None).get(n, buf)) for n in names("f16_gust_sample")])
    assert gs() == F16_OK and gs(B=4, ld=4, nrows=0) == F16_OK
    for bad in (dict(ctx=None), dict(ga=None), dict(gb=None), dict(gstate=None), dict(g_seq=None), dict(B=-1), dict(B=4, ld=3), dict(nrows=-1)):
        assert gs(**bad) == F16_EINVAL, bad


# ------------------------------------------------------------------------------------------------ the Python keywords
def test_keywords_end_in_the_wind_calls_and_defaults_in_todays():
    import torch
    from f16_mpc_oop_py_amd.wind import GustModel
    B = 4
    env = env_of(B)
    env.rollout_schedule(np.zeros((3, B, 4)), hold=2, nsteps=5)
    env.rollout_LQR(5, 0.0, 0.0, 0.0, K=torch.zeros((B, 3, 9), dtype=torch.float64))
    assert [c[0] for c in env.lib.calls if c[0].startswith("f16_rollout")] == ["f16_rollout_sched", "f16_rollout_lqr"]
    env = env_of(B)
    env.rollout_schedule(np.zeros((3, B, 4)), hold=2, nsteps=5, method="rk4", wind=[10.0, 0.0, -2.0], gusts=np.zeros((2, B, 3)), gust_every=3)
    gm = GustModel(5.0, 1750.0, 700.0, seed=3, every=2)
    env.rollout_LQR(5, 0.0, 0.0, 0.0, K=torch.zeros((B, 3, 9), dtype=torch.float64), wind=np.zeros((B, 3)), gusts=gm)
    calls = [c for c in env.lib.calls if c[0].startswith("f16_rollout")]
    assert [c[0] for c in calls] == ["f16_rollout_wind", "f16_rollout_lqr_wind"]
    for c in calls:
        assert len(c[1]) == len(names(c[0]))
    got = dict(zip(names("f16_rollout_wind"), calls[0][1]))
    assert (got["nsteps"], got["hold"], got["method"]) == (5, 2, 4)
    assert gm.row == 3                                                              # ceil(5 / 2) rows were drawn


def test_value_errors_before_any_call():
    import torch
    from f16_mpc_oop_py_amd.wind import GustModel
    B = 4
    env = env_of(B)
    K = torch.zeros((B, 3, 9), dtype=torch.float64)
    gm = GustModel(5.0, 1750.0, 700.0)
    for kw in (dict(linear=True), dict(relinearise=True, K=None)):
        with pytest.raises(ValueError, match="wind"):
            env.rollout_LQR(5, 0.0, 0.0, 0.0, **dict(dict(K=K, wind=[1.0, 0.0, 0.0]), **kw))
    with pytest.raises(ValueError, match="wind"):
        env.rollout_LQR(5, 0.0, 0.0, 0.0, schedule=object(), gusts=gm)
    with pytest.raises(ValueError, match="gust_every"):
        env.rollout_schedule(np.zeros((3, B, 4)), hold=2, nsteps=5, gust_every=2)
    with pytest.raises(ValueError, match="gust_every"):
        env.rollout_schedule(np.zeros((3, B, 4)), hold=2, nsteps=5, gusts=gm, gust_every=2)
    with pytest.raises(ValueError, match="gust rows"):
        env.rollout_schedule(np.zeros((3, B, 4)), hold=2, nsteps=5, gusts=np.zeros((2, B, 3)), gust_every=2)
    with pytest.raises(ValueError, match="gusts must be"):
        env.rollout_schedule(np.zeros((3, B, 4)), hold=2, nsteps=5, gusts=np.zeros((5, 3, B + 1)))
    with pytest.raises(ValueError):
        GustModel(5.0, 1750.0, 700.0, every=0)
    with pytest.raises(ValueError):
        GustModel(-5.0, 1750.0, 700.0)
    assert env.lib.calls == []
