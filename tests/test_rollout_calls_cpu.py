"""CPU-side checks of the five rollouts on the nonlinear plant (f16_rollout, _sched, _cost, _lqr, _lqr_sched) from Python down to the
launch: the argument rules of the C entry points, row by row, on calls the library refuses or treats as a no-op (nothing is launched
and no array is dereferenced, so a zeroed host buffer stands for the context and for every array); and the mapping from
F16Batch.rollout / rollout_schedule / rollout_LQR / score_schedules to those entry points on the recording stub of
test_mpc_loop_calls_cpu.py: which symbol a call ends in, every scalar by position against include/f16_hip.h, which pointers are
NULL and what comes back."""
import ctypes

import numpy as np
import pytest
import torch

from header_cases import names
from test_mpc_loop_calls_cpu import B, DT, FI, FLAGS, XCG, recording_env

F16_OK, F16_EINVAL = 0, -1                                                     # include/f16_hip.h
FIVE = ("f16_rollout", "f16_rollout_sched", "f16_rollout_cost", "f16_rollout_lqr", "f16_rollout_lqr_sched")
BAD_ARGUMENT = "bad argument (NULL pointer, B < 0 or ld < B)"
BAD_STEPS = "nsteps must be >= 0 and a multiple of traj_every >= 1 when traj is given"
STATE = {name: "x0" if name == "f16_rollout_cost" else "x" for name in FIVE}    # the state column of each call
# the pointers a call needs beyond ctx, the state and u / u0, and what it says when one of them is NULL
NEEDED = {"f16_rollout_sched": (("u_seq",), "u_seq is NULL"),
          "f16_rollout_cost": (("u_seq", "x_ref", "h_w", "cost"), "u_seq / x_ref / h_w / cost is NULL"),
          "f16_rollout_lqr": (("K", "dem"), "K / dem is NULL"),
          "f16_rollout_lqr_sched": (("K", "dem_seq"), "K / dem_seq is NULL")}
HELD = ("f16_rollout_sched", "f16_rollout_lqr_sched", "f16_rollout_cost")      # the calls that take `hold`


# ------------------------------------------------------------------------------------------------ the C rules
@pytest.fixture(scope="module")
def clib():
    from f16_mpc_oop_py_amd import lib
    lib.build()
    L = lib.load()
    zeros = ctypes.create_string_buffer(4096)
    weights = lib.make_cost_weights()
    return L, ctypes.c_void_p(ctypes.addressof(zeros)), weights, zeros


def call(clib, symbol, weights=None, **over):
    """`symbol` on a call that is complete except for `over` (None = a NULL pointer): four aircraft, five steps, no traj -> (rc, message)"""
    L, buf, w, _ = clib
    base = dict(B=4, ld=4, B0=4, ld0=4, nsteps=5, hold=2, traj_every=1, dt=1e-3, xcg=0.35, fi_flag=1, flags=0, stream=None,
                traj=None, x_end=None, u_ref=None, u_out=None, status=None, h_w=ctypes.byref(weights or w))
    args = [over[n] if n in over else base.get(n, buf) for n in names(symbol)]
    rc = getattr(L, symbol)(*args)
    return rc, L.f16_last_error().decode()


def refused(clib, symbol, words, **over):
    rc, msg = call(clib, symbol, **over)
    assert rc == F16_EINVAL and words in msg, (symbol, over, rc, msg)


# Every refused call below is ALSO a no-op (B = 0, or nsteps = 0 where that is one; B = -1 makes an empty grid): a rule that went
# missing shows as a wrong return code, never as a kernel on the zeroed buffer.  The one exception is the B0 rule of f16_rollout_cost,
# which holds for B > 0 only.
@pytest.mark.parametrize("symbol", FIVE)
def test_null_pointers_and_sizes_are_refused(clib, symbol):
    quiet = dict(B=0, ld=0)
    refused(clib, symbol, BAD_ARGUMENT, ctx=None, **quiet)
    refused(clib, symbol, BAD_ARGUMENT, **{STATE[symbol]: None}, **quiet)
    for u in ("u", "u0"):                                                      # (u_seq of the other two has a message of its own)
        if u in names(symbol):
            refused(clib, symbol, BAD_ARGUMENT, **{u: None}, **quiet)
    refused(clib, symbol, BAD_ARGUMENT, B=-1, ld=0, nsteps=0)
    refused(clib, symbol, BAD_ARGUMENT, B=0, ld=-1)
    if symbol != "f16_rollout_cost":                                           # (its nsteps = 0 is no no-op)
        refused(clib, symbol, BAD_ARGUMENT, B=4, ld=3, nsteps=0)


@pytest.mark.parametrize("symbol", FIVE)
def test_step_count_and_sampling_interval(clib, symbol):
    buf = clib[1]
    refused(clib, symbol, BAD_STEPS, B=0, ld=0, nsteps=-1)
    refused(clib, symbol, BAD_STEPS, B=0, ld=0, nsteps=4, traj=buf, traj_every=0)
    refused(clib, symbol, BAD_STEPS, B=0, ld=0, nsteps=4, traj=buf, traj_every=-2)
    refused(clib, symbol, BAD_STEPS, B=0, ld=0, nsteps=5, traj=buf, traj_every=2)
    assert call(clib, symbol, B=0, ld=0, nsteps=6, traj=buf, traj_every=2)[0] == F16_OK
    for every in (0, -3, 2, 7):                                                # without traj the interval is not read
        assert call(clib, symbol, B=0, ld=0, nsteps=5, traj=None, traj_every=every)[0] == F16_OK, (symbol, every)


@pytest.mark.parametrize("symbol", list(NEEDED))
def test_the_pointers_a_variant_needs(clib, symbol):
    pointers, words = NEEDED[symbol]
    for p in pointers:
        refused(clib, symbol, words, B=0, ld=0, **{p: None})


@pytest.mark.parametrize("symbol", HELD)
def test_hold_below_one_is_refused(clib, symbol):
    for hold in (0, -1):
        refused(clib, symbol, "hold must be >= 1", B=0, ld=0, hold=hold)
    assert call(clib, symbol, B=0, ld=0, hold=1)[0] == F16_OK


def test_cost_lanes_are_samples_of_aircraft(clib):
    words = "B lanes are K samples of B0 aircraft"
    refused(clib, "f16_rollout_cost", words, B=4, ld=4, B0=0, ld0=4)
    refused(clib, "f16_rollout_cost", words, B=4, ld=4, B0=2, ld0=1)
    refused(clib, "f16_rollout_cost", words, B=4, ld=4, B0=3, ld0=4)
    for B0, ld0 in ((0, 4), (2, 1), (3, 4)):                                   # B = 0: the rule does not apply
        assert call(clib, "f16_rollout_cost", B=0, ld=0, B0=B0, ld0=ld0)[0] == F16_OK


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), -float("inf")])
def test_cost_weights_are_checked_even_without_lanes(clib, bad):
    from f16_mpc_oop_py_amd import lib
    for field, k in (("q", 0), ("q", 8), ("qf", 4), ("r", 2), ("pen", None)):
        w = lib.make_cost_weights()
        if k is None:
            w.pen = bad
        else:
            getattr(w, field)[k] = bad
        rc, msg = call(clib, "f16_rollout_cost", weights=w, B=0, ld=0)
        assert rc == F16_EINVAL and "cost weights" in msg, (field, k, rc, msg)


@pytest.mark.parametrize("symbol", FIVE)
def test_no_aircraft_or_no_steps_is_a_no_op(clib, symbol):
    _, buf, _, zeros = clib
    assert call(clib, symbol, B=0, ld=0)[0] == F16_OK
    assert call(clib, symbol, B=0, ld=4, traj=buf, traj_every=5)[0] == F16_OK
    if symbol != "f16_rollout_cost":                                           # (its nsteps = 0 launches: the cost is the terminal term)
        assert call(clib, symbol, nsteps=0)[0] == F16_OK
        assert call(clib, symbol, nsteps=0, traj=buf, traj_every=3)[0] == F16_OK
    assert zeros.raw == bytes(4096)                                            # nothing was written either


# ------------------------------------------------------------------------------------------------ the Python mapping
S, HOLD, NSTEPS, EVERY, K = 3, 2, 5, 5, 2        # a short last segment: rows 0, 0, 1, 1, 2
POINTERS = {"ctx", "x", "x0", "u", "u0", "u_seq", "K", "dem", "dem_seq", "traj", "u_out", "status", "x_ref", "u_ref", "h_w", "cost",
            "x_end", "stream"}


def env_of(nb=B):
    """the recording environment of test_mpc_loop_calls_cpu.py, resized to nb aircraft"""
    env = recording_env()
    if nb != B:
        env.B = nb
        env._x, env._u = torch.zeros((18, nb), dtype=torch.float64), torch.zeros((4, nb), dtype=torch.float64)
        env._u_init, env.status = env._u.clone(), torch.zeros(nb, dtype=torch.int32)
    env._u_init[:] = torch.arange(4.0 * nb).reshape(4, nb)
    return env


def the_call(env, symbol, scalars, null):
    """exactly one call of the five, and it is `symbol`; its scalars by position, its NULL pointers -> the arguments by name"""
    calls = [c for c in env.lib.calls if c[0].startswith("f16_rollout")]
    assert [c[0] for c in calls] == [symbol]
    params, args = names(symbol), calls[0][1]
    assert len(args) == len(params)
    got = dict(zip(params, args))
    want = dict(scalars, dt=DT, xcg=XCG, fi_flag=FI, flags=FLAGS)
    assert set(want) <= set(params), (symbol, want)
    for k in params:
        if k in POINTERS:
            if k in ("ctx", "stream"):
                continue                                                       # (the stub environment has neither)
            assert (got[k] is None) == (k in null), (k, got[k])
        elif k in want:
            assert type(got[k]) is type(want[k]) and got[k] == want[k], (k, got[k], want[k])
        else:
            # traj_every without traj: not read by the library, but it must be a legal value
            assert k == "traj_every" and "traj" in null and type(got[k]) is int and got[k] >= 1, (k, got[k])
    return got


def address(arg):
    assert isinstance(arg, ctypes.c_void_p), arg
    return arg.value


def test_rollout():
    env = env_of()
    traj = env.rollout(NSTEPS, traj_every=EVERY)
    got = the_call(env, "f16_rollout", dict(B=B, ld=B, nsteps=NSTEPS, traj_every=EVERY), set())
    assert tuple(traj.shape) == (1, 18, B) and traj.dtype == torch.float64 and address(got["traj"]) == traj.data_ptr()
    assert address(got["x"]) == env._x.data_ptr() and address(got["u"]) == env._u.data_ptr()
    assert address(got["status"]) == env.status.data_ptr()
    env = env_of()
    assert env.rollout(NSTEPS, action=np.ones((B, 4))) is None
    got = the_call(env, "f16_rollout", dict(B=B, ld=B, nsteps=NSTEPS), {"traj"})
    assert address(got["u"]) != env._u.data_ptr()                              # the given action, u.values untouched
    assert not env._u.any()
    env = env_of()
    with pytest.raises((ValueError, AssertionError)):
        env.rollout(10, traj_every=3)
    assert env.lib.calls == []


@pytest.mark.parametrize("form", ["numpy", "torch_host", "state_major"])
def test_rollout_schedule(form):
    nb = 5 if form == "state_major" else B       # (with four aircraft a [S, 4, 4] tensor is read as [S, B, 4])
    rows = np.arange(S * nb * 4, dtype=np.float64).reshape(S, nb, 4)
    a = {"numpy": rows, "torch_host": torch.as_tensor(rows), "state_major": torch.as_tensor(rows.transpose(0, 2, 1).copy())}[form]
    env = env_of(nb)
    traj = env.rollout_schedule(a, hold=HOLD, nsteps=NSTEPS, traj_every=EVERY)
    got = the_call(env, "f16_rollout_sched", dict(B=nb, ld=nb, nsteps=NSTEPS, hold=HOLD, traj_every=EVERY), set())
    assert tuple(traj.shape) == (1, 18, nb) and traj.dtype == torch.float64 and address(got["traj"]) == traj.data_ptr()
    assert np.array_equal(env.u_values.numpy(), rows[(NSTEPS - 1) // HOLD])   # the last row used
    if form == "state_major":
        assert address(got["u_seq"]) == a.data_ptr()                           # taken as it is, without a copy
    env = env_of(nb)
    assert env.rollout_schedule(a) is None                                     # hold = 1, every row: S steps
    the_call(env, "f16_rollout_sched", dict(B=nb, ld=nb, nsteps=S, hold=1), {"traj"})
    assert np.array_equal(env.u_values.numpy(), rows[S - 1])


def test_rollout_schedule_refuses_before_any_call():
    rows = np.zeros((S, B, 4))
    env = env_of()
    with pytest.raises(ValueError, match="hold"):
        env.rollout_schedule(rows, hold=0)
    with pytest.raises(ValueError, match="rows.*actions"):
        env.rollout_schedule(rows, hold=HOLD, nsteps=7)                        # needs four rows
    with pytest.raises(ValueError):
        env.rollout_schedule(rows[:, :3])                                      # wrong batch
    with pytest.raises(ValueError):
        env.rollout_schedule(rows[0])                                          # not 3-D
    with pytest.raises(ValueError, match="traj_every"):
        env.rollout_schedule(rows, hold=HOLD, traj_every=4)                    # six steps
    assert env.lib.calls == [] and not env._u.any()


@pytest.mark.parametrize("every", [EVERY, None])
def test_rollout_LQR_with_constant_demands(every):
    env = env_of()
    env._u[0] = 7.0
    traj = env.rollout_LQR(NSTEPS, 0.02, np.full(B, -0.01), 0.01, K=np.zeros((B, 3, 9)), traj_every=every)
    got = the_call(env, "f16_rollout_lqr", dict(B=B, ld=B, nsteps=NSTEPS, **(dict(traj_every=every) if every else {})),
                   set() if every else {"traj"})
    assert traj is None if not every else (tuple(traj.shape) == (1, 18, B) and traj.dtype == torch.float64)
    assert address(got["u_out"]) == env._u.data_ptr() and address(got["x"]) == env._x.data_ptr()
    assert address(got["u0"]) not in (env._u.data_ptr(), env._u_init.data_ptr())      # the current thrust over the initial surfaces


@pytest.mark.parametrize("every", [EVERY, None])
def test_rollout_LQR_with_demand_histories(every):
    env = env_of()
    p, q = np.linspace(-0.05, 0.05, S), np.zeros((S, B))
    traj = env.rollout_LQR(NSTEPS, p, q, 0.01, K=np.zeros((B, 3, 9)), traj_every=every, hold=HOLD)
    got = the_call(env, "f16_rollout_lqr_sched", dict(B=B, ld=B, nsteps=NSTEPS, hold=HOLD, **(dict(traj_every=every) if every else {})),
                   set() if every else {"traj"})
    assert traj is None if not every else (tuple(traj.shape) == (1, 18, B) and traj.dtype == torch.float64)
    assert address(got["u_out"]) == env._u.data_ptr()
    env = env_of()
    env.rollout_LQR(S, p, q, 0.01, K=np.zeros((B, 3, 9)))                      # hold defaults to 1
    the_call(env, "f16_rollout_lqr_sched", dict(B=B, ld=B, nsteps=S, hold=1), {"traj"})


def test_rollout_LQR_refuses_before_any_call():
    env = env_of()
    p, q, K0 = np.linspace(-0.05, 0.05, S), np.zeros((S, B)), np.zeros((B, 3, 9))
    with pytest.raises(ValueError):
        env.rollout_LQR(NSTEPS, p, q, 0.01, K=K0, hold=HOLD, linear=True)
    with pytest.raises(ValueError):
        env.rollout_LQR(NSTEPS, p, q, 0.01, hold=HOLD, relinearise=True)
    with pytest.raises(ValueError, match="rows.*the demands"):
        env.rollout_LQR(7, p, q, 0.01, K=K0, hold=HOLD)                        # needs four rows
    with pytest.raises(ValueError, match="hold"):
        env.rollout_LQR(NSTEPS, p, q, 0.01, K=K0, hold=0)
    with pytest.raises(ValueError):
        env.rollout_LQR(NSTEPS, p, q[:2], 0.01, K=K0, hold=HOLD)               # histories of different length
    with pytest.raises(ValueError, match="hold"):
        env.rollout_LQR(NSTEPS, 0.0, 0.0, 0.0, K=K0, hold=HOLD)                # hold without a history
    assert env.lib.calls == []


def test_score_schedules():
    lanes = K * B
    actions = np.zeros((S, K, B, 4))
    sizes = dict(B0=B, ld0=B, B=lanes, ld=lanes, nsteps=NSTEPS, hold=HOLD)
    env = env_of()
    cost, final, traj = env.score_schedules(actions, hold=HOLD, nsteps=NSTEPS, traj_every=EVERY, return_final=True)
    got = the_call(env, "f16_rollout_cost", dict(sizes, traj_every=EVERY), {"u_ref"})
    assert tuple(cost.shape) == (K, B) and tuple(final.shape) == (18, K, B) and tuple(traj.shape) == (1, 18, K, B)
    assert cost.dtype == final.dtype == traj.dtype == torch.float64
    assert tuple(env.last_score_status.shape) == (K, B) and env.last_score_status.dtype == torch.int32
    assert address(got["x0"]) == env._x.data_ptr() and address(got["cost"]) == cost.data_ptr()
    assert address(got["status"]) == env.last_score_status.data_ptr() != env.status.data_ptr()
    env = env_of()
    cost = env.score_schedules(actions, hold=HOLD, nsteps=NSTEPS, u_ref=np.zeros(3))
    the_call(env, "f16_rollout_cost", sizes, {"x_end", "traj"})
    assert tuple(cost.shape) == (K, B)
    env = env_of()
    assert tuple(env.score_schedules(actions).shape) == (K, B)                 # hold = 1, every row
    the_call(env, "f16_rollout_cost", dict(sizes, nsteps=S, hold=1), {"u_ref", "x_end", "traj"})
    for kw in (dict(hold=0), dict(hold=HOLD, nsteps=7), dict(hold=HOLD, traj_every=4)):
        env = env_of()
        with pytest.raises(ValueError, match="hold|rows.*actions|traj_every"):
            env.score_schedules(actions, **kw)
        assert env.lib.calls == []
