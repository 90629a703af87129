"""CPU-side checks of the three rollouts that take the step rule as an argument (f16_rollout_rk, f16_rollout_lqr_rk,
f16_rollout_cost_rk), in the manner of tests/test_rollout_calls_cpu.py: the argument rules of the C entry points on calls the library
refuses or treats as a no-op (nothing is launched and no array is dereferenced, so a zeroed host buffer stands for the context and
for every array), for both methods; the refusal of an unknown method; the parameter lists against include/f16_hip.h; and, on the
recording stub, which symbol every Python call ends in with method="rk4" -- and that it is today's symbol, with today's arguments,
with method="euler" -- and the ValueErrors."""
import ctypes
import re

import numpy as np
import pytest
import torch

from test_mpc_loop_calls_cpu import B, DT, FI, FLAGS, XCG
from header_cases import header, header_parameters, names
from test_rollout_calls_cpu import BAD_ARGUMENT, BAD_STEPS, F16_EINVAL, F16_OK, POINTERS, address, env_of

EULER, RK4 = 1, 4                                                              # F16_INT_EULER, F16_INT_RK4 (include/f16_hip.h)
THREE = {"f16_rollout_rk": "f16_rollout_sched", "f16_rollout_lqr_rk": "f16_rollout_lqr_sched", "f16_rollout_cost_rk": "f16_rollout_cost"}
STATE = {"f16_rollout_rk": "x", "f16_rollout_lqr_rk": "x", "f16_rollout_cost_rk": "x0"}
NEEDED = {"f16_rollout_rk": (("u_seq",), "u_seq is NULL"),
          "f16_rollout_cost_rk": (("u_seq", "x_ref", "h_w", "cost"), "u_seq / x_ref / h_w / cost is NULL"),
          "f16_rollout_lqr_rk": (("K", "dem_seq"), "K / dem_seq is NULL")}
BAD_METHOD = "method must be F16_INT_EULER (1) or F16_INT_RK4 (4)"
METHODS = [EULER, RK4]


@pytest.fixture(scope="module")
def clib():
    from f16_mpc_oop_py_amd import lib
    lib.build()
    L = lib.load()
    zeros = ctypes.create_string_buffer(4096)
    return L, ctypes.c_void_p(ctypes.addressof(zeros)), lib.make_cost_weights(), zeros


def call(clib, symbol, method, weights=None, **over):
    """`symbol` on a call that is complete except for `over` (None = a NULL pointer): four aircraft, five steps, no traj -> (rc, message)"""
    L, buf, w, _ = clib
    base = dict(B=4, ld=4, B0=4, ld0=4, nsteps=5, hold=2, traj_every=1, dt=1e-3, xcg=0.35, fi_flag=1, method=method, flags=0, stream=None,
                traj=None, x_end=None, u_ref=None, u_out=None, status=None, h_w=ctypes.byref(weights or w))
    args = [over[n] if n in over else base.get(n, buf) for n in names(symbol)]
    rc = getattr(L, symbol)(*args)
    return rc, L.f16_last_error().decode()


def refused(clib, symbol, method, words, **over):
    rc, msg = call(clib, symbol, method, **over)
    assert rc == F16_EINVAL and words in msg, (symbol, method, over, rc, msg)


# ------------------------------------------------------------------------------------------------ header, library, binding
@pytest.mark.parametrize("symbol", list(THREE))
def test_parameter_lists_are_the_scheduled_ones_plus_the_method(symbol):
    """the header declares each call as the call it stands for with `int method` between fi_flag and flags; the binding's argtypes
    have the same length and an int there; the library exports the symbol"""
    from f16_mpc_oop_py_amd import lib
    new, old = header_parameters(symbol), header_parameters(THREE[symbol])
    k = [p.split()[-1] for p in old].index("fi_flag") + 1
    assert new == old[:k] + ["int method"] + old[k:]
    L = lib.load()
    at, bt = getattr(L, symbol).argtypes, getattr(L, THREE[symbol]).argtypes
    assert list(at) == list(bt[:k]) + [ctypes.c_int] + list(bt[k:])
    assert hasattr(ctypes.CDLL(lib.build()), symbol)
    assert re.search(r"#define\s+F16_INT_EULER\s+1\b", header()) and re.search(r"#define\s+F16_INT_RK4\s+4\b", header())
    assert (lib.F16_INT_EULER, lib.F16_INT_RK4) == (EULER, RK4)


# ------------------------------------------------------------------------------------------------ the C rules, both methods
# Every refused call is also a no-op (B = 0, or nsteps = 0 where that is one), as in test_rollout_calls_cpu.py: a rule that went
# missing shows as a wrong return code, never as a kernel on the zeroed buffer.
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("symbol", list(THREE))
def test_null_pointers_and_sizes_are_refused(clib, symbol, method):
    quiet = dict(B=0, ld=0)
    refused(clib, symbol, method, BAD_ARGUMENT, ctx=None, **quiet)
    refused(clib, symbol, method, BAD_ARGUMENT, **{STATE[symbol]: None}, **quiet)
    if "u0" in names(symbol):
        refused(clib, symbol, method, BAD_ARGUMENT, u0=None, **quiet)
    refused(clib, symbol, method, BAD_ARGUMENT, B=-1, ld=0, nsteps=0)
    refused(clib, symbol, method, BAD_ARGUMENT, B=0, ld=-1)
    if symbol != "f16_rollout_cost_rk":                                        # (its nsteps = 0 is no no-op)
        refused(clib, symbol, method, BAD_ARGUMENT, B=4, ld=3, nsteps=0)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("symbol", list(THREE))
def test_step_count_sampling_interval_pointers_and_hold(clib, symbol, method):
    buf = clib[1]
    refused(clib, symbol, method, BAD_STEPS, B=0, ld=0, nsteps=-1)
    refused(clib, symbol, method, BAD_STEPS, B=0, ld=0, nsteps=4, traj=buf, traj_every=0)
    refused(clib, symbol, method, BAD_STEPS, B=0, ld=0, nsteps=5, traj=buf, traj_every=2)
    assert call(clib, symbol, method, B=0, ld=0, nsteps=6, traj=buf, traj_every=2)[0] == F16_OK
    for every in (0, -3, 2, 7):                                                # without traj the interval is not read
        assert call(clib, symbol, method, B=0, ld=0, nsteps=5, traj=None, traj_every=every)[0] == F16_OK
    pointers, words = NEEDED[symbol]
    for p in pointers:
        refused(clib, symbol, method, words, B=0, ld=0, **{p: None})
    for hold in (0, -1):
        refused(clib, symbol, method, "hold must be >= 1", B=0, ld=0, hold=hold)
    assert call(clib, symbol, method, B=0, ld=0, hold=1)[0] == F16_OK


@pytest.mark.parametrize("method", METHODS)
def test_cost_lanes_and_weights(clib, method):
    from f16_mpc_oop_py_amd import lib
    words = "B lanes are K samples of B0 aircraft"
    for B0, ld0 in ((0, 4), (2, 1), (3, 4)):
        refused(clib, "f16_rollout_cost_rk", method, words, B=4, ld=4, B0=B0, ld0=ld0)
        assert call(clib, "f16_rollout_cost_rk", method, B=0, ld=0, B0=B0, ld0=ld0)[0] == F16_OK      # B = 0: the rule does not apply
    for bad in (-1.0, float("nan"), float("inf")):
        w = lib.make_cost_weights()
        w.qf[4] = bad
        rc, msg = call(clib, "f16_rollout_cost_rk", method, weights=w, B=0, ld=0)
        assert rc == F16_EINVAL and "cost weights" in msg, (bad, rc, msg)


@pytest.mark.parametrize("symbol", list(THREE))
def test_an_unknown_method_is_refused_and_the_message_names_the_argument(clib, symbol):
    for method in (0, 2, 3, 5, -1, 44):
        refused(clib, symbol, method, BAD_METHOD, B=0, ld=0)
        if symbol != "f16_rollout_cost_rk":
            refused(clib, symbol, method, BAD_METHOD, nsteps=0)
    assert "method" in BAD_METHOD
    # the existing order of checks stays: every older rule speaks before the method does
    refused(clib, symbol, 3, BAD_ARGUMENT, ctx=None, B=0, ld=0)
    refused(clib, symbol, 3, BAD_STEPS, B=0, ld=0, nsteps=-1)
    refused(clib, symbol, 3, "hold must be >= 1", B=0, ld=0, hold=0)
    refused(clib, symbol, 3, NEEDED[symbol][1], B=0, ld=0, **{NEEDED[symbol][0][0]: None})


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("symbol", list(THREE))
def test_no_aircraft_or_no_steps_is_a_no_op(clib, symbol, method):
    _, buf, _, zeros = clib
    assert call(clib, symbol, method, B=0, ld=0)[0] == F16_OK
    assert call(clib, symbol, method, B=0, ld=4, traj=buf, traj_every=5)[0] == F16_OK
    if symbol != "f16_rollout_cost_rk":                                        # (its nsteps = 0 launches: the cost is the terminal term)
        assert call(clib, symbol, method, nsteps=0)[0] == F16_OK
        assert call(clib, symbol, method, nsteps=0, traj=buf, traj_every=3)[0] == F16_OK
    assert zeros.raw == bytes(4096)                                            # nothing was written either


# ------------------------------------------------------------------------------------------------ the Python mapping
S, HOLD, NSTEPS, EVERY, K = 3, 2, 5, 5, 2


def calls_of(env):
    return [c for c in env.lib.calls if c[0].startswith("f16_rollout")]


def the_call(env, symbol, scalars, null):
    """exactly one rollout call, and it is `symbol`; its scalars by position against the header, its NULL pointers"""
    calls = calls_of(env)
    assert [c[0] for c in calls] == [symbol]
    params, args = names(symbol), calls[0][1]
    assert len(args) == len(params)
    got = dict(zip(params, args))
    want = dict(scalars, dt=DT, xcg=XCG, fi_flag=FI, flags=FLAGS)
    assert set(want) <= set(params), (symbol, want)
    for k in params:
        if k in POINTERS:
            if k not in ("ctx", "stream"):
                assert (got[k] is None) == (k in null), (k, got[k])
        elif k in want:
            assert type(got[k]) is type(want[k]) and got[k] == want[k], (k, got[k], want[k])
        else:
            assert k == "traj_every" and "traj" in null and type(got[k]) is int and got[k] >= 1, (k, got[k])
    return got


def both(run):
    """run(env, method keywords) under the default, under method="euler" and under method="rk4" -> the three recorded call lists"""
    out = []
    for kw in ({}, dict(method="euler"), dict(method="rk4")):
        env = env_of()
        run(env, kw)
        out.append((env, calls_of(env)))
    return out


def same_calls(a, b):
    """two recorded call lists agree in symbols and in every scalar argument (pointers: NULL or not)"""
    assert [c[0] for c in a] == [c[0] for c in b]
    for (_, x), (_, y) in zip(a, b):
        assert len(x) == len(y)
        for p, q in zip(x, y):
            if isinstance(p, (int, float)) and not isinstance(q, ctypes.c_void_p):
                assert type(p) is type(q) and p == q
            else:
                assert (p is None) == (q is None)


def test_rollout():
    (e0, c0), (e1, c1), (e4, _) = both(lambda env, kw: env.rollout(NSTEPS, traj_every=EVERY, **kw))
    same_calls(c0, c1)
    assert [c[0] for c in c0] == ["f16_rollout"]
    got = the_call(e4, "f16_rollout_rk", dict(B=B, ld=B, nsteps=NSTEPS, hold=NSTEPS, traj_every=EVERY, method=RK4), set())
    assert address(got["x"]) == e4._x.data_ptr() and address(got["u_seq"]) == e4._u.data_ptr()      # the constant input: one row, held
    assert address(got["status"]) == e4.status.data_ptr()
    env = env_of()
    assert env.rollout(NSTEPS, action=np.ones((B, 4)), method="rk4") is None
    got = the_call(env, "f16_rollout_rk", dict(B=B, ld=B, nsteps=NSTEPS, hold=NSTEPS, method=RK4), {"traj"})
    assert address(got["u_seq"]) != env._u.data_ptr() and not env._u.any()


def test_rollout_schedule():
    rows = np.arange(S * B * 4, dtype=np.float64).reshape(S, B, 4)
    (e0, c0), (e1, c1), (e4, _) = both(lambda env, kw: env.rollout_schedule(rows, hold=HOLD, nsteps=NSTEPS, traj_every=EVERY, **kw))
    same_calls(c0, c1)
    assert [c[0] for c in c0] == ["f16_rollout_sched"]
    the_call(e4, "f16_rollout_rk", dict(B=B, ld=B, nsteps=NSTEPS, hold=HOLD, traj_every=EVERY, method=RK4), set())
    assert np.array_equal(e4.u_values.numpy(), rows[(NSTEPS - 1) // HOLD])     # the last row used, as under Euler


def test_rollout_LQR():
    K0 = np.zeros((B, 3, 9))
    (e0, c0), (e1, c1), (e4, _) = both(lambda env, kw: env.rollout_LQR(NSTEPS, 0.02, np.full(B, -0.01), 0.01, K=K0, traj_every=EVERY, **kw))
    same_calls(c0, c1)
    assert [c[0] for c in c0] == ["f16_rollout_lqr"]
    got = the_call(e4, "f16_rollout_lqr_rk", dict(B=B, ld=B, nsteps=NSTEPS, hold=NSTEPS, traj_every=EVERY, method=RK4), set())
    assert address(got["u_out"]) == e4._u.data_ptr() and address(got["x"]) == e4._x.data_ptr()
    p, q = np.linspace(-0.05, 0.05, S), np.zeros((S, B))
    (e0, c0), (e1, c1), (e4, _) = both(lambda env, kw: env.rollout_LQR(NSTEPS, p, q, 0.01, K=K0, hold=HOLD, **kw))
    same_calls(c0, c1)
    assert [c[0] for c in c0] == ["f16_rollout_lqr_sched"]
    the_call(e4, "f16_rollout_lqr_rk", dict(B=B, ld=B, nsteps=NSTEPS, hold=HOLD, method=RK4), {"traj"})


def test_score_schedules_and_the_MPPI_calls():
    lanes = K * B
    actions = np.zeros((S, K, B, 4))
    sizes = dict(B0=B, ld0=B, B=lanes, ld=lanes, nsteps=NSTEPS, hold=HOLD)
    (e0, c0), (e1, c1), (e4, _) = both(lambda env, kw: env.score_schedules(actions, hold=HOLD, nsteps=NSTEPS, traj_every=EVERY,
                                                                           return_final=True, **kw))
    same_calls(c0, c1)
    assert [c[0] for c in c0] == ["f16_rollout_cost"]
    got = the_call(e4, "f16_rollout_cost_rk", dict(sizes, traj_every=EVERY, method=RK4), {"u_ref"})
    assert address(got["x0"]) == e4._x.data_ptr() and address(got["status"]) == e4.last_score_status.data_ptr()
    # calc_MPPI_action: the scoring alone takes the method (the blend has no step)
    nominal, noise = np.zeros((S, B, 4)), np.zeros((S, K, B, 3))
    (e0, c0), (e1, c1), (e4, c4) = both(lambda env, kw: env.calc_MPPI_action(0.0, 0.0, 0.0, nominal, noise, hold=HOLD, **kw))
    same_calls(c0, c1)
    assert [c[0] for c in c0] == ["f16_rollout_cost"] and [c[0] for c in c4] == ["f16_rollout_cost_rk"]
    assert [c[0] for c in e4.lib.calls] == ["f16_rollout_cost_rk", "f16_mppi_blend"]
    assert dict(zip(names("f16_rollout_cost_rk"), c4[0][1]))["method"] == RK4
    # rollout_MPPI: the scoring and the plant advance, one pair per control period
    (e0, c0), (e1, c1), (e4, c4) = both(lambda env, kw: env.rollout_MPPI(2 * HOLD, 0.0, 0.0, 0.0, S, HOLD, K, 0.1, 1.0, **kw))
    same_calls(c0, c1)
    assert [c[0] for c in c0] == ["f16_rollout_cost", "f16_rollout"] * 2
    assert [c[0] for c in c4] == ["f16_rollout_cost_rk", "f16_rollout_rk"] * 2
    adv = dict(zip(names("f16_rollout_rk"), c4[1][1]))
    assert adv["method"] == RK4 and adv["nsteps"] == HOLD and adv["hold"] == HOLD and adv["traj"] is None


def test_value_errors_before_any_call():
    K0, p, q = np.zeros((B, 3, 9)), np.linspace(-0.05, 0.05, S), np.zeros((S, B))
    actions = np.zeros((S, K, B, 4))
    env = env_of()
    for bad in ("RK4", "heun", "", None, 4, b"rk4"):                           # any other method, on every call that takes one
        for f in (lambda: env.rollout(NSTEPS, method=bad), lambda: env.rollout_schedule(actions[:, 0], method=bad),
                  lambda: env.rollout_LQR(NSTEPS, 0.0, 0.0, 0.0, K=K0, method=bad), lambda: env.score_schedules(actions, method=bad),
                  lambda: env.calc_MPPI_action(0.0, 0.0, 0.0, actions[:, 0], np.zeros((S, K, B, 3)), method=bad),
                  lambda: env.rollout_MPPI(HOLD, 0.0, 0.0, 0.0, S, HOLD, K, 0.1, 1.0, method=bad),
                  lambda: env.rollout_MPC(4, 0.0, 0.0, 0.0, 10, method=bad)):
            with pytest.raises(ValueError, match="method"):
                f()
    # the loops whose kernels step with euler_step_exact (or on the linear model) have no Runge-Kutta step
    with pytest.raises(ValueError, match="rk4"):
        env.rollout_LQR(NSTEPS, 0.0, 0.0, 0.0, K=K0, linear=True, method="rk4")
    with pytest.raises(ValueError, match="rk4"):
        env.rollout_LQR(NSTEPS, 0.0, 0.0, 0.0, relinearise=True, method="rk4")
    for kw in (dict(), dict(relinearise=True), dict(ctrl_every=2), dict(p=p)):
        dem = (kw.pop("p"), q, 0.0) if "p" in kw else (0.0, 0.0, 0.0)
        with pytest.raises(ValueError, match="rk4"):
            env.rollout_MPC(4, *dem, 10, method="rk4", **kw)
    assert env.lib.calls == [] and not env._u.any() and not env._x.any()
    # "euler" is accepted by all of them: the MPC loop then makes today's call
    env.rollout_MPC(4, 0.0, 0.0, 0.0, 10, method="euler")
    assert [c[0] for c in env.lib.calls if c[0].startswith("f16_rollout")] == ["f16_rollout_mpc"]
