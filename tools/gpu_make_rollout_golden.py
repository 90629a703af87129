"""Fixture G16 (tests/golden/g16_quad_rollout.npz): what the quad rollout kernel returns for three seeded launches, kept so that
a later kernel can be checked against it bit for bit (tests/test_gpu_rollout_cell_cache.py).  Run on the GPU box with the
library whose results are to be recorded:   python tools/gpu_make_rollout_golden.py OUT.npz
  hdg: B = 4096 (one group per workgroup), 1000 steps;  g2: B = 4100 (two groups, ragged tail), 300 steps;
  lqr: B = 4096 under the LQR law, 300 steps.  Stored: 128 fixed aircraft (the tail included), every 50th sample."""
import sys
sys.path.insert(0, ".")
import numpy as np


def pick(B):
    idx = np.random.default_rng(0).choice(B - 8, 120, replace=False)
    return np.sort(np.concatenate([idx, np.arange(B - 8, B)]))


def main(out):
    from f16_mpc_oop_py_amd import F16Batch
    from f16_mpc_oop_py_amd.workload import config2_states
    res = {}
    for name, B, T, seed in (("hdg", 4096, 1000, 20261003), ("g2", 4100, 300, 11)):
        x0, u0 = config2_states(B, seed=seed)
        env = F16Batch(x0, u0, device="cuda:0")
        tr = env.rollout(T, traj_every=50).cpu().numpy()
        i = pick(B)
        res.update({f"{name}_idx": i, f"{name}_x": env.x_values.cpu().numpy()[i], f"{name}_status": env.status.cpu().numpy()[i],
                    f"{name}_traj": tr[:, :, i]})
    x0, u0 = config2_states(4096, seed=5)
    env = F16Batch(x0, u0, device="cuda:0")
    K = env._calc_LQR_gain()
    tr = env.rollout_LQR(300, 0.05, -0.02, 0.01, K=K, traj_every=50).cpu().numpy()
    i = pick(4096)
    res.update({"lqr_idx": i, "lqr_K": K.cpu().numpy()[i], "lqr_x": env.x_values.cpu().numpy()[i],
                "lqr_u": env.u_values.cpu().numpy()[i], "lqr_status": env.status.cpu().numpy()[i], "lqr_traj": tr[:, :, i]})
    np.savez_compressed(out, **res)
    print({k: v.shape for k, v in res.items()})


if __name__ == "__main__":
    main(sys.argv[1])
