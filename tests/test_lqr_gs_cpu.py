"""CPU-side checks of the LQR loop under a gain schedule over (altitude, airspeed) (f16_rollout_lqr_gs, f16_gain_lookup_host,
f16_debug_gain_lookup; f16_mpc_oop_py_amd/schedule.py GainSchedule):
  1. the host statement of the lookup rule against its numpy restatement, bit for bit;
  2. the restatement against scipy's RegularGridInterpolator inside the grid;
  3. the argument rules of f16_rollout_lqr_gs on the zeroed-buffer harness of tests/test_rollout_rk_calls_cpu.py (nothing is launched
     and no array is dereferenced), for both methods;
  4. header against binding, the exported symbols, and on the recording stub which symbol rollout_LQR ends in with and without
     schedule=, the ValueErrors, save / load."""
import ctypes

import numpy as np
import pytest
import torch

from gs_cases import DH, DV, H0, NH, NV, V0, lookup_points, same_bits, small_schedule
from header_cases import header, header_parameters, kind, names
from test_mpc_loop_calls_cpu import B, DT, FI, FLAGS, XCG
from test_rollout_calls_cpu import BAD_ARGUMENT, BAD_STEPS, F16_EINVAL, F16_OK, address, env_of
from test_rollout_rk_calls_cpu import BAD_METHOD, EULER, METHODS, RK4, call, calls_of, clib  # noqa: F401  (clib: the fixture)

GS = "f16_rollout_lqr_gs"


# ------------------------------------------------------------------------------------------------ 1, 2: the lookup rule
def test_host_lookup_equals_the_numpy_restatement_bit_for_bit():
    gs = small_schedule()
    h, v = lookup_points()
    inside = ~gs.outside(h[:10000], v[:10000])
    assert 0.30 < 1.0 - inside.mean() < 0.37                                   # a third of the random points lie outside
    want, got = gs.lookup(h, v), gs.lookup_host(h, v)
    assert np.isfinite(want).all()                                             # (clamped: NaN and the infinities included)
    assert same_bits(got, want), int((got.view(np.int64) != want.view(np.int64)).sum())


def test_lookup_properties_at_nodes_outside_and_for_odd_coordinates():
    gs = small_schedule()
    hn, vn = np.meshgrid(H0 + DH * np.arange(NH), V0 + DV * np.arange(NV), indexing="ij")
    assert same_bits(gs.lookup(hn, vn), gs.table)                              # at a node: the node's values
    assert same_bits(gs.lookup_host(hn, vn).reshape(NH, NV, 12), gs.table)
    # outside: the edge cell extended flat (a clamp, no extrapolation)
    assert same_bits(gs.lookup(H0 - 123.0, 420.0), gs.lookup(H0, 420.0)) and same_bits(gs.lookup(1e9, 420.0), gs.lookup(H0 + 3 * DH, 420.0))
    assert same_bits(gs.lookup(1700.0, -5.0), gs.lookup(1700.0, V0)) and same_bits(gs.lookup(1700.0, np.inf), gs.lookup(1700.0, V0 + 2 * DV))
    assert same_bits(gs.lookup(-np.inf, 420.0), gs.lookup(H0, 420.0))
    # a NaN coordinate: index 0, weight 0
    assert same_bits(gs.lookup(np.nan, 420.0), gs.lookup(H0, 420.0)) and same_bits(gs.lookup(1700.0, np.nan), gs.lookup(1700.0, V0))
    assert gs.outside([np.nan, 1700.0, np.inf, H0 - 1e-9, 1700.0], [420.0, np.nan, 420.0, 420.0, V0 + 2 * DV + 1e-9]).all()
    assert not gs.outside([H0, H0 + 3 * DH, 1700.0], [V0, V0 + 2 * DV, 420.0]).any()


def test_restatement_against_scipy_inside_the_grid():
    from scipy.interpolate import RegularGridInterpolator
    from f16_mpc_oop_py_amd.schedule import GainSchedule
    gs = small_schedule()
    h, v = lookup_points()
    keep = ~gs.outside(h, v)
    h, v = h[keep], v[keep]
    ref = RegularGridInterpolator((H0 + DH * np.arange(NH), V0 + DV * np.arange(NV)), gs.table, method="linear")(np.stack((h, v), 1))
    err = np.abs(gs.lookup(h, v) - ref).max()
    print(f"lookup against scipy: max abs error {err:.3e}, max |table| {np.abs(gs.table).max():.3e}")
    assert err <= 1e-12 * np.abs(gs.table).max()
    hn, vn = np.meshgrid(H0 + DH * np.arange(NH), V0 + DV * np.arange(NV), indexing="ij")
    assert np.array_equal(gs.lookup(hn, vn), gs.table)                         # exact at nodes
    node = np.random.default_rng(3).normal(size=12)
    flat = GainSchedule(H0, DH, NH, V0, DV, NV, np.broadcast_to(node, (NH, NV, 12)))
    assert same_bits(flat.lookup(h, v), np.broadcast_to(node, (h.size, 12)))   # a table of identical nodes: exactly those values
    assert same_bits(flat.lookup_host(h[:500], v[:500]), np.broadcast_to(node, (500, 12)))


# ------------------------------------------------------------------------------------------------ 3: the C rules, both methods
def grid(**over):
    from f16_mpc_oop_py_amd import lib
    return lib.GainGrid(**dict(dict(h0=H0, dh=DH, v0=V0, dv=DV, nh=NH, nv=NV), **over))


def gs_call(clib, method, h_grid="good", **over):
    g = grid() if h_grid == "good" else h_grid
    return call(clib, GS, method, h_grid=None if g is None else ctypes.byref(g), **dict(dict(gs_every=1, gs_out=None), **over))


def refused(clib, method, words, **over):
    rc, msg = gs_call(clib, method, **over)
    assert rc == F16_EINVAL and words in msg, (method, over, rc, msg)


@pytest.mark.parametrize("method", METHODS)
def test_what_the_call_it_extends_refuses(clib, method):
    buf = clib[1]
    quiet = dict(B=0, ld=0)
    refused(clib, method, BAD_ARGUMENT, ctx=None, **quiet)
    refused(clib, method, BAD_ARGUMENT, x=None, **quiet)
    refused(clib, method, BAD_ARGUMENT, u0=None, **quiet)
    refused(clib, method, BAD_ARGUMENT, B=-1, ld=0, nsteps=0)
    refused(clib, method, BAD_ARGUMENT, B=0, ld=-1)
    refused(clib, method, BAD_ARGUMENT, B=4, ld=3, nsteps=0)
    refused(clib, method, BAD_STEPS, nsteps=-1, **quiet)
    refused(clib, method, BAD_STEPS, nsteps=4, traj=buf, traj_every=0, **quiet)
    refused(clib, method, BAD_STEPS, nsteps=5, traj=buf, traj_every=2, **quiet)
    refused(clib, method, "dem_seq is NULL", dem_seq=None, **quiet)
    for hold in (0, -1):
        refused(clib, method, "hold must be >= 1", hold=hold, **quiet)
    # ... and each of them speaks before the schedule's rules do
    refused(clib, method, BAD_STEPS, nsteps=-1, h_grid=None, tab=None, gs_every=0, **quiet)
    refused(clib, method, "hold must be >= 1", hold=0, h_grid=None, **quiet)


@pytest.mark.parametrize("method", METHODS)
def test_the_rules_of_the_schedule_name_their_argument(clib, method):
    quiet = dict(B=0, ld=0)
    refused(clib, method, "h_grid", h_grid=None, **quiet)
    refused(clib, method, "tab", tab=None, **quiet)
    for bad in (dict(nh=1), dict(nv=1), dict(nh=0), dict(nv=-3)):
        refused(clib, method, "nh and nv", h_grid=grid(**bad), **quiet)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(clib, method, "dh and dv", h_grid=grid(dh=bad), **quiet)
        refused(clib, method, "dh and dv", h_grid=grid(dv=bad), **quiet)
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(clib, method, "h0 and v0", h_grid=grid(h0=bad), **quiet)
        refused(clib, method, "h0 and v0", h_grid=grid(v0=bad), **quiet)
    for bad in (0, -1):
        refused(clib, method, "gs_every", gs_every=bad, **quiet)
        refused(clib, method, "gs_every", gs_every=bad, nsteps=0)
    assert gs_call(clib, method, gs_every=1, **quiet)[0] == F16_OK
    assert gs_call(clib, method, gs_every=10 ** 6, **quiet)[0] == F16_OK


@pytest.mark.parametrize("method", METHODS)
def test_no_aircraft_or_no_steps_is_a_no_op(clib, method):
    _, buf, _, zeros = clib
    assert gs_call(clib, method, B=0, ld=0)[0] == F16_OK
    assert gs_call(clib, method, B=0, ld=4, traj=buf, traj_every=5, gs_out=buf)[0] == F16_OK
    assert gs_call(clib, method, nsteps=0)[0] == F16_OK
    assert zeros.raw == bytes(4096)                                            # nothing was written either


def test_an_unknown_method_is_refused_last(clib):
    for method in (0, 2, 3, 5, -1, 44):
        refused(clib, method, BAD_METHOD, B=0, ld=0)
        refused(clib, method, BAD_METHOD, nsteps=0)
    # every other rule speaks before the method does
    refused(clib, 3, BAD_ARGUMENT, ctx=None, B=0, ld=0)
    refused(clib, 3, "dem_seq is NULL", dem_seq=None, B=0, ld=0)
    refused(clib, 3, "h_grid", h_grid=None, B=0, ld=0)
    refused(clib, 3, "tab", tab=None, B=0, ld=0)
    refused(clib, 3, "nh and nv", h_grid=grid(nv=1), B=0, ld=0)
    refused(clib, 3, "gs_every", gs_every=0, B=0, ld=0)


def test_host_and_debug_lookups_check_their_arguments(clib):
    L, buf, _, _ = clib
    g, out = grid(), (ctypes.c_double * 12)()
    assert L.f16_gain_lookup_host(None, buf, 0.0, 0.0, out) == F16_EINVAL and "h_grid" in L.f16_last_error().decode()
    assert L.f16_gain_lookup_host(ctypes.byref(grid(nh=1)), buf, 0.0, 0.0, out) == F16_EINVAL
    assert L.f16_gain_lookup_host(ctypes.byref(g), None, 0.0, 0.0, out) == F16_EINVAL
    assert L.f16_gain_lookup_host(ctypes.byref(g), buf, 0.0, 0.0, None) == F16_EINVAL
    assert L.f16_gain_lookup_host(ctypes.byref(g), buf, 1700.0, 420.0, out) == F16_OK and list(out) == [0.0] * 12      # (the zeroed table)
    assert L.f16_debug_gain_lookup(None, ctypes.byref(g), buf, buf, buf, 0, buf) == F16_EINVAL
    assert L.f16_debug_gain_lookup(buf, ctypes.byref(grid(dv=0.0)), buf, buf, buf, 0, buf) == F16_EINVAL
    assert L.f16_debug_gain_lookup(buf, ctypes.byref(g), buf, buf, buf, -1, buf) == F16_EINVAL
    assert L.f16_debug_gain_lookup(buf, ctypes.byref(g), buf, buf, buf, 0, buf) == F16_OK


# ------------------------------------------------------------------------------------------------ 4: header, binding, Python
def test_header_library_and_binding_agree():
    from f16_mpc_oop_py_amd import lib
    L, exported = lib.load(), ctypes.CDLL(lib.build())
    old, new = header_parameters("f16_rollout_lqr_rk"), header_parameters(GS)
    # f16_rollout_lqr_rk's list with K replaced by the grid, the table and the period, and gs_out in front of status
    k, s = old.index("const double *K"), old.index("int32_t *status")
    assert new == old[:k] + ["const f16_gain_grid *h_grid", "const double *tab", "int gs_every"] + old[k + 1:s] + ["int32_t *gs_out"] + old[s:]
    for symbol in (GS, "f16_gain_lookup_host", "f16_debug_gain_lookup"):
        assert hasattr(exported, symbol), symbol
        assert list(getattr(L, symbol).argtypes) == [kind(p, lib) for p in header_parameters(symbol)], symbol
    assert kind("const f16_gain_grid *h_grid", lib) == ctypes.POINTER(lib.GainGrid) and kind("const double *tab", lib) == ctypes.c_void_p
    src = header(comments=True)
    assert "#define F16_GS_ENTRIES 12" in src and lib.F16_GS_ENTRIES == 12
    assert "typedef struct f16_gain_grid { double h0, dh, v0, dv; int nh, nv; } f16_gain_grid;" in src
    assert [f[0] for f in lib.GainGrid._fields_] == ["h0", "dh", "v0", "dv", "nh", "nv"]
    assert ctypes.sizeof(lib.GainGrid) == 40


NSTEPS, EVERY, S, HOLD = 6, 3, 3, 2


def gs_call_of(env):
    calls = calls_of(env)
    assert [c[0] for c in calls] == [GS]
    params, args = names(GS), calls[0][1]
    assert len(args) == len(params)
    return dict(zip(params, args))


@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_rollout_LQR_with_a_schedule_ends_in_the_new_call(method):
    gs = small_schedule()
    env = env_of()
    traj, info = env.rollout_LQR(NSTEPS, 0.02, np.full(B, -0.01), 0.01, schedule=gs, gains_every=4, traj_every=EVERY, method=method,
                                 return_info=True)
    got = gs_call_of(env)
    want = dict(B=B, ld=B, nsteps=NSTEPS, hold=NSTEPS, traj_every=EVERY, gs_every=4, method={"euler": EULER, "rk4": RK4}[method],
                dt=DT, xcg=XCG, fi_flag=FI, flags=FLAGS)
    for k, val in want.items():
        assert type(got[k]) is type(val) and got[k] == val, (k, got[k], val)
    assert address(got["x"]) == env._x.data_ptr() and address(got["u_out"]) == env._u.data_ptr()
    assert address(got["status"]) == env.status.data_ptr() and address(got["traj"]) == traj.data_ptr() and tuple(traj.shape) == (2, 18, B)
    assert address(got["gs_out"]) == info["gs_out"].data_ptr() and info["gs_out"].dtype == torch.int32 and tuple(info["gs_out"].shape) == (B,)
    assert address(got["tab"]) == gs.device_table(env.device).data_ptr()
    assert torch.equal(gs.device_table(env.device), torch.as_tensor(gs.table))
    g = got["h_grid"]._obj                                                     # (ctypes.byref keeps its object)
    assert (g.h0, g.dh, g.v0, g.dv, g.nh, g.nv) == (H0, DH, V0, DV, NH, NV)
    # demand histories: the rows and the hold as rollout_LQR hands them to the frozen-gain call
    env = env_of()
    p, q = np.linspace(-0.05, 0.05, S), np.zeros((S, B))
    assert env.rollout_LQR(NSTEPS, p, q, 0.01, schedule=gs, hold=HOLD, method=method) is None
    got = gs_call_of(env)
    assert (got["hold"], got["gs_every"], got["nsteps"], got["traj"]) == (HOLD, 1, NSTEPS, None)


def test_rollout_LQR_without_a_schedule_makes_todays_call():
    K0 = np.zeros((B, 3, 9))
    for kw, symbol, n in ((dict(), "f16_rollout_lqr", 17), (dict(method="rk4"), "f16_rollout_lqr_rk", 19)):
        env = env_of()
        env.rollout_LQR(NSTEPS, 0.02, np.full(B, -0.01), 0.01, K=K0, traj_every=EVERY, **kw)
        calls = calls_of(env)
        assert [c[0] for c in calls] == [symbol] and len(calls[0][1]) == n == len(names(symbol))
        got = dict(zip(names(symbol), calls[0][1]))
        assert (got["B"], got["ld"], got["nsteps"], got["traj_every"], got["dt"], got["xcg"], got["fi_flag"], got["flags"]) == \
            (B, B, NSTEPS, EVERY, DT, XCG, FI, FLAGS)
        assert address(got["u_out"]) == env._u.data_ptr() and got["K"] is not None


def test_value_errors_before_any_call():
    gs, K0 = small_schedule(), np.zeros((B, 3, 9))
    env = env_of()
    for kw in (dict(K=K0), dict(linear=True), dict(relinearise=True)):
        with pytest.raises(ValueError, match="schedule"):
            env.rollout_LQR(NSTEPS, 0.0, 0.0, 0.0, schedule=gs, **kw)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="gains_every"):
            env.rollout_LQR(NSTEPS, 0.0, 0.0, 0.0, schedule=gs, gains_every=bad)
    with pytest.raises(ValueError, match="schedule"):
        env.rollout_LQR(NSTEPS, 0.0, 0.0, 0.0, K=K0, return_info=True)
    with pytest.raises(ValueError, match="method"):
        env.rollout_LQR(NSTEPS, 0.0, 0.0, 0.0, schedule=gs, method="heun")
    assert env.lib.calls == [] and not env._u.any() and not env._x.any()


def test_schedule_constructor_save_and_load(tmp_path):
    from f16_mpc_oop_py_amd.schedule import GainSchedule
    gs = small_schedule()
    gs.ok[1, 2] = False
    path = str(tmp_path / "schedule.npz")
    gs.save(path)
    back = GainSchedule.load(path)
    assert (back.h0, back.dh, back.nh, back.v0, back.dv, back.nv) == (H0, DH, NH, V0, DV, NV)
    assert type(back.nh) is int and same_bits(back.table, gs.table) and np.array_equal(back.ok, gs.ok) and back.ok.dtype == bool
    h, v = lookup_points()
    assert same_bits(back.lookup(h, v), gs.lookup(h, v))
    for bad in (dict(nh=1), dict(dv=0.0), dict(h0=float("nan"))):
        args = dict(dict(h0=H0, dh=DH, nh=NH, v0=V0, dv=DV, nv=NV), **bad)
        with pytest.raises(ValueError):
            GainSchedule(table=np.zeros((args["nh"], args["nv"], 12)), **args)
    with pytest.raises(ValueError, match="table"):
        GainSchedule(H0, DH, NH, V0, DV, NV, np.zeros((NH, NV, 9)))
