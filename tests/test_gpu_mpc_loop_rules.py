"""GPU test of argument rules of the closed MPC loops (f16_rollout_mpc*, include/f16_hip.h) that the tests of the single entry points
leave out: negative step counts, the zero-step no-op and the plan mark, traj_every without an output that is sampled, and the limit
nctrl x hold < 2^31.  B = 16, N = 10, two control steps."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

XCG, DT, EINVAL = 0.35, 1e-3, -1


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.timeout(300, method="thread")      # (a persistent kernel that never drains must fail the run, not hold it)
def test_step_counts_zero_step_no_op_and_sampling_rules():
    from f16_mpc_oop_py_amd import F16Batch
    from f16_mpc_oop_py_amd.workload import config4_states
    x0, u0 = config4_states(16, seed=1)
    env = F16Batch(x0, u0, device="cuda:0", xcg=XCG)
    env.build_ssr(); env.prepare_MPC(10)
    lib, plan, dem = env.lib, env._plan, env._demands(0.02, -0.01, 0.005)
    buf = torch.empty((2, 189, 16), dtype=torch.float64, device="cuda:0")
    mpc = lambda nsteps, every=1, traj=None: lib.f16_rollout_mpc(
        plan, _vp(env._x), _vp(env._u), _vp(dem), _vp(traj), None, None, _vp(env.status), nsteps, every, XCG, 1, 0, env._stream)
    relin = lambda nsteps, every=1, traj=None, model=None: lib.f16_rollout_mpc_relin(
        plan, _vp(env._x), _vp(env._u), _vp(dem), _vp(traj), None, None, _vp(model), _vp(env.status), nsteps, every, 1e-5, XCG, 1, 0,
        env._stream)
    before = env.x_values.clone()
    assert mpc(-1) == EINVAL and relin(-1) == EINVAL
    # traj_every is read only with an output that is sampled by it: traj, and in the re-linearised call model_traj
    assert mpc(0, every=0) == 0 and relin(0, every=0) == 0
    assert mpc(0, every=0, traj=buf) == EINVAL and relin(0, every=0, traj=buf) == EINVAL and relin(0, every=0, model=buf) == EINVAL
    # hold x nctrl = 2^31 (the period does not fit either: nothing can be launched whichever check speaks first -- the first one must)
    assert lib.f16_rollout_mpc_hold(plan, _vp(env._x), _vp(env._u), _vp(dem), None, None, None, _vp(env.status), 1 << 16, 1 << 15, 1, DT,
                                    XCG, 1, 0, env._stream) == EINVAL and b"2^31" in lib.f16_last_error()
    torch.cuda.synchronize()
    assert bool((env.x_values == before).all()) and int(env.status.max()) == 0
    # zero steps of the re-linearised call are a no-op that leaves the plan unmarked: the frozen-model call still takes it
    assert relin(0) == 0 and mpc(2, every=0) == 0
    torch.cuda.synchronize()
    assert not bool((env.x_values == before).all())
    # ... and one re-linearised step marks it
    assert relin(1) == 0 and mpc(1) == EINVAL and b"model" in lib.f16_last_error()
