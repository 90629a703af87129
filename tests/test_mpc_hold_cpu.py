"""CPU-side checks of the closed MPC loops at a control period of several plant steps (f16_rollout_mpc_hold /
f16_rollout_mpc_relin_hold): the C-ABI boundary, and the argument checks of F16Batch.rollout_MPC(ctrl_every=...) and
dist.closed_loop_mpc_rollout(ctrl_every=...) that come before any GPU call."""
import ctypes

import pytest

from header_cases import header_parameters

HOLD = {"f16_rollout_mpc_hold": "f16_rollout_mpc", "f16_rollout_mpc_relin_hold": "f16_rollout_mpc_relin"}


def test_header_library_and_binding_agree_on_the_hold_entry_points():
    from f16_mpc_oop_py_amd import lib
    exported = ctypes.CDLL(lib.build())
    L = lib.load()
    for name, base in HOLD.items():
        p, q = header_parameters(name), header_parameters(base)
        assert hasattr(exported, name), f"libf16hip.so does not export {name}"
        args = getattr(L, name).argtypes
        assert len(args) == len(p), (name, p)
        # `hold` sits in front of `traj_every`; the plant step `dt` is declared; nsteps became nctrl; everything else is the base call's
        assert "int hold" in p and p.index("int hold") + 1 == p.index("int traj_every")
        assert "double dt" in p and "int nctrl" in p and p.index("int nctrl") + 1 == p.index("int hold")
        extra = ("int hold", "double dt") + (("int model_every",) if "relin" in name else ())
        assert [a for a in p if a not in extra] == [("int nctrl" if a == "int nsteps" else a) for a in q]
        assert args[p.index("double dt")] is ctypes.c_double and args[p.index("int hold")] is ctypes.c_int
        assert list(args).count(ctypes.c_int) == list(getattr(L, base).argtypes).count(ctypes.c_int) + len(extra) - 1
    p = header_parameters("f16_rollout_mpc_relin_hold")
    assert p.index("int model_every") == p.index("int traj_every") + 1 and p.index("double dt") == p.index("int model_every") + 1
    assert p.index("double eps") == p.index("double dt") + 1
    p = header_parameters("f16_rollout_mpc_hold")
    assert p.index("double dt") == p.index("int traj_every") + 1


def test_ctrl_every_argument_checks_come_before_any_gpu_call():
    from f16_mpc_oop_py_amd import F16Batch, dist
    env = F16Batch.__new__(F16Batch)           # no GPU, no state: anything past the argument checks would raise AttributeError
    for relin in (False, True):
        kw = dict(relinearise=True) if relin else {}
        with pytest.raises(ValueError, match="ctrl_every"):
            env.rollout_MPC(12, 0.0, 0.0, 0.0, 10, ctrl_every=5, **kw)          # nsteps is no multiple of the control period
        with pytest.raises(ValueError, match="ctrl_every"):
            env.rollout_MPC(10, 0.0, 0.0, 0.0, 10, ctrl_every=0, **kw)
        with pytest.raises(ValueError, match="ctrl_every"):
            env.rollout_MPC(0, 0.0, 0.0, 0.0, 10, ctrl_every=5, **kw)           # no control step at all
        with pytest.raises(ValueError, match="traj_every"):
            env.rollout_MPC(10, 0.0, 0.0, 0.0, 10, ctrl_every=5, traj_every=3, **kw)
        with pytest.raises(ValueError, match="hzn"):
            env.rollout_MPC(10, 0.0, 0.0, 0.0, 31, ctrl_every=5, **kw)
        with pytest.raises(ValueError, match="model_every"):
            env.rollout_MPC(10, 0.0, 0.0, 0.0, 10, ctrl_every=5, model_every=0, **kw)
        with pytest.raises(AttributeError):
            env.rollout_MPC(10, 0.0, 0.0, 0.0, 10, ctrl_every=5, **kw)
    with pytest.raises(ValueError, match="model_every"):
        env.rollout_MPC(20, 0.0, 0.0, 0.0, 10, ctrl_every=5, model_every=3, relinearise=True)      # 4 control steps
    with pytest.raises(ValueError, match="eps"):
        env.rollout_MPC(10, 0.0, 0.0, 0.0, 10, ctrl_every=5, relinearise=True, eps=0.0)
    with pytest.raises(ValueError, match="model_every"):
        env.rollout_MPC(10, 0.0, 0.0, 0.0, 10, model_every=2)                    # belongs to ctrl_every > 1
    with pytest.raises(ValueError, match="ctrl_every"):
        env.prepare_MPC(10, ctrl_every=0)
    with pytest.raises(ValueError, match="use_plan"):
        env._calc_MPC_action(0.0, 0.0, 0.0, 10, ctrl_every=5)
    for fused in (True, False):
        with pytest.raises(ValueError, match="ctrl_every"):
            dist.closed_loop_mpc_rollout(env, 12, 10, ctrl_every=5, fused=fused)
        with pytest.raises(ValueError, match="traj_every"):
            dist.closed_loop_mpc_rollout(env, 10, 10, ctrl_every=5, traj_every=3, fused=fused)
