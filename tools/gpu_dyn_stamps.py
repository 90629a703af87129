"""Diagnostic: per-wave cycles of the quad rollout from a -DF16_EXP_STAMPQ build (run on the GPU box).
-DF16_EXP_STAMPQ (or =1): every stamp waits for all counters, wave 2's sample stores included; -DF16_EXP_STAMPQ=2: for the LDS /
scalar counter only, so that wave 2's first half reads without the completion of its stores.
usage: F16HIP_SO=build/libf16hip_stampq.so python tools/gpu_dyn_stamps.py [B]"""
import sys
sys.path.insert(0, ".")
import numpy as np, torch
from f16_mpc_oop_py_amd import F16Batch
from f16_mpc_oop_py_amd.workload import config2_states
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
x0, u0 = config2_states(B)
env = F16Batch(x0, u0)
T = 1000
traj = env.rollout(T, traj_every=1)
torch.cuda.synchronize()
flat = traj[2].reshape(-1)
# (the store wave's row stands in state row 2 of the sample: with a library that has no store wave it reads that row's states)
d = torch.cat((flat[:16], flat[2 * B:2 * B + 4])).cpu().numpy().reshape(5, 4) / T
np.set_printoptions(linewidth=200, precision=0, suppress=True)
print("cycles per step; rows = waves (long, lat, trig/forces, atmos/act, sample stores); cols = second half+publish, barrier A, first half, barrier B")
print(d, d.sum(1))
print("cycles from kernel entry to the first barrier (table staging), per wave:", traj[2].reshape(-1)[B:B + 5].cpu().numpy())
