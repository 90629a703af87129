"""CPU-side check of the mapping from F16Batch.rollout_MPC to the six closed-loop entry points of the C ABI (f16_rollout_mpc, _relin,
_hold, _relin_hold, _sched, _relin_sched): which symbol a call ends in, every scalar argument by position, which pointers are NULL and
what comes back.  The environment is built by hand on CPU tensors over a library stub that records its calls; the expectations are
written out from the declarations and contracts of include/f16_hip.h."""
import ctypes
import types

import numpy as np
import pytest
import torch

B, DT, XCG, FI, FLAGS, EPS, HZN = 4, 1e-3, 0.35, 1, 2, 2e-5, 10
HOLD_COMMAND = 8                                                               # F16_FLAG_HOLD_COMMAND (include/f16_hip.h)
FRONT = ["plan", "x", "u", "dem", "traj", "cmd_traj", "iters_traj"]            # every call begins with these pointers
TAIL = ["xcg", "fi_flag", "flags", "stream"]                                   # ... and ends with these
PARAMS = {                                                                     # the parameter lists of include/f16_hip.h
    "f16_rollout_mpc": FRONT + ["status", "nsteps", "traj_every"] + TAIL,
    "f16_rollout_mpc_relin": FRONT + ["model_traj", "status", "nsteps", "traj_every", "eps"] + TAIL,
    "f16_rollout_mpc_hold": FRONT + ["status", "nctrl", "hold", "traj_every", "dt"] + TAIL,
    "f16_rollout_mpc_relin_hold": FRONT + ["model_traj", "status", "nctrl", "hold", "traj_every", "model_every", "dt", "eps"] + TAIL,
    "f16_rollout_mpc_sched": FRONT + ["status", "nctrl", "hold", "dem_hold", "traj_every", "dt"] + TAIL,
    "f16_rollout_mpc_relin_sched": FRONT + ["model_traj", "status", "nctrl", "hold", "dem_hold", "traj_every", "model_every", "dt", "eps"]
    + TAIL,
}
POINTERS = set(FRONT) | {"model_traj", "status", "stream"}
# Four control steps each.  variant -> (rollout_MPC's nsteps, keywords, suffix of the symbol, the call's scalars, rows of the model record):
# nsteps / traj_every are in PLANT steps, cmd / iters / model have one row per control step (model: per model_every-th, and in the two
# oldest calls per traj_every-th step); dem_hold is dem_every, hold is ctrl_every, dt the plant's step.
VARIANTS = {
    "const": (4, dict(traj_every=2), "", dict(nsteps=4, traj_every=2), 2),
    "const_hold5": (20, dict(ctrl_every=5, traj_every=10), "_hold", dict(nctrl=4, hold=5, traj_every=10, model_every=1, dt=DT), 4),
    "hist_S": (4, dict(traj_every=2, dem_every=2), "_sched", dict(nctrl=4, hold=1, dem_hold=2, traj_every=2, model_every=1, dt=DT), 4),
    "hist_SB_hold5": (20, dict(ctrl_every=5, traj_every=10, dem_every=2, model_every=2), "_sched",
                      dict(nctrl=4, hold=5, dem_hold=2, traj_every=10, model_every=2, dt=DT), 2),
}


def demands(variant):
    if variant == "hist_S":
        return np.array([0.01, -0.01]), 0.0, 0.005                              # [S]: two rows for four control steps at dem_every = 2
    if variant == "hist_SB_hold5":
        return 0.01, np.linspace(-0.01, 0.01, 2 * B).reshape(2, B), 0.0        # [S, B]
    return 0.01, np.full(B, -0.01), 0.0                                         # scalars and [B]: constant demands


class RecordingLib:
    """every attribute is a callable that records (name, args) and returns 0 (F16_OK)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def recording_env():
    """an F16Batch without a GPU: B = 4 aircraft on CPU tensors, a frozen model, the recording stub as its library"""
    from f16_mpc_oop_py_amd import F16Batch

    class Env(F16Batch):
        _stream = None                                                         # (the property asks torch for a GPU stream)

    env = Env.__new__(Env)
    env.B, env.device, env.dt, env.xcg, env.fi_flag, env.flags = B, torch.device("cpu"), DT, XCG, FI, FLAGS
    env.lib, env.ctx = RecordingLib(), types.SimpleNamespace(handle=None)
    env._x, env._u = torch.zeros((18, B), dtype=torch.float64), torch.zeros((4, B), dtype=torch.float64)
    env._u_init, env.status = env._u.clone(), torch.zeros(B, dtype=torch.int32)
    z = lambda rows: torch.zeros((rows, B), dtype=torch.float64)
    env.ssr, env._ssr_cont = (z(81), z(27), z(81)), (z(81), z(27))
    return env


def the_rollout_call(env):
    calls = [c for c in env.lib.calls if c[0].startswith("f16_rollout_mpc")]
    assert len(calls) == 1, [c[0] for c in calls]                             # exactly one closed-loop call
    return calls[0]


def check_call(name, args, symbol, scalars, null, relin, hold_command):
    assert name == symbol
    params = PARAMS[symbol]
    assert len(args) == len(params)
    got = dict(zip(params, args))
    want = dict(scalars, xcg=XCG, fi_flag=FI, flags=FLAGS | (HOLD_COMMAND if hold_command else 0), **(dict(eps=EPS) if relin else {}))
    for k in params:
        if k in POINTERS:
            if k == "stream":
                continue                                                       # (the stub environment has no stream)
            assert (got[k] is None) == (k in null), (k, got[k])
            assert got[k] is None or isinstance(got[k], ctypes.c_void_p), (k, got[k])
        elif k in want:
            assert type(got[k]) is type(want[k]) and got[k] == want[k], (k, got[k], want[k])
        else:
            # traj_every without traj (model_every without model_traj): not read by the library, but it must be a legal value
            assert k in ("traj_every", "model_every") and "traj" in null and type(got[k]) is int and got[k] >= 1, (k, got[k])
    assert set(want) <= set(params), (symbol, want)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("relin", [False, True])
def test_rollout_MPC_ends_in_one_call_of_the_narrowest_entry_point(relin, variant):
    nsteps, kw, suffix, scalars, model_rows = VARIANTS[variant]
    symbol = "f16_rollout_mpc" + ("_relin" if relin else "") + suffix
    scalars = {k: v for k, v in scalars.items() if k in PARAMS[symbol]}
    hold_command = variant in ("const_hold5", "hist_S")
    env = recording_env()
    traj, info = env.rollout_MPC(nsteps, *demands(variant), HZN, return_info=True, hold_command=hold_command, relinearise=relin,
                                 eps=EPS, **kw)
    name, args = the_rollout_call(env)
    check_call(name, args, symbol, scalars, set() if relin else {"model_traj"}, relin, hold_command)
    assert tuple(traj.shape) == (2, 18, B) and traj.dtype == torch.float64      # 4 or 20 plant steps, a sample after every 2nd or 10th
    assert tuple(info["cmd"].shape) == (4, 3, B) and info["cmd"].dtype == torch.float64
    assert tuple(info["iters"].shape) == (4, B) and info["iters"].dtype == torch.int32
    assert set(info) == ({"cmd", "iters", "model"} if relin else {"cmd", "iters"})
    if relin:
        assert tuple(info["model"].shape) == (model_rows, 189, B) and info["model"].dtype == torch.float64


@pytest.mark.parametrize("variant", ["const", "const_hold5", "hist_SB_hold5"])
@pytest.mark.parametrize("relin", [False, True])
def test_rollout_MPC_without_outputs_passes_null_pointers(relin, variant):
    nsteps, kw, suffix, scalars, _ = VARIANTS[variant]
    symbol = "f16_rollout_mpc" + ("_relin" if relin else "") + suffix
    kw = {k: v for k, v in kw.items() if k != "traj_every"}
    scalars = {k: v for k, v in scalars.items() if k in PARAMS[symbol] and k != "traj_every"}
    if symbol == "f16_rollout_mpc_relin":
        scalars.pop("model_every", None)
    env = recording_env()
    assert env.rollout_MPC(nsteps, *demands(variant), HZN, relinearise=relin, eps=EPS, **kw) is None
    name, args = the_rollout_call(env)
    check_call(name, args, symbol, scalars, {"traj", "cmd_traj", "iters_traj", "model_traj"}, relin, False)


@pytest.mark.parametrize("relin", [False, True])
def test_zero_steps_with_constant_demands_still_make_the_call(relin):
    """nsteps = 0 is the library's no-op (f16_rollout_mpc / f16_rollout_mpc_relin return F16_OK): the call is made, None comes back"""
    symbol = "f16_rollout_mpc_relin" if relin else "f16_rollout_mpc"
    env = recording_env()
    assert env.rollout_MPC(0, *demands("const"), HZN, relinearise=relin, eps=EPS) is None
    name, args = the_rollout_call(env)
    check_call(name, args, symbol, dict(nsteps=0), {"traj", "cmd_traj", "iters_traj", "model_traj"}, relin, False)
