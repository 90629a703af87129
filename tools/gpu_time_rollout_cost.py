"""GPU timing of the scored rollout: K sampled command schedules per aircraft, one number per trajectory.  Per size B0 x K, in the
same process, alternating, `--repeats` timed runs of each after a warm-up, device events around each run:
    (a) f16_rollout_cost, traj = NULL      one launch; the cost is accumulated in registers, x0 is read through the fan-out
    (b) the path without it on the same lanes: f16_rollout_sched on the K-fold replicated initial states storing every step
        (traj_every = 1), then the same cost formed by torch from the stored trajectory (box check of env.py:117-124 included)
    (c) f16_rollout_sched, traj = NULL on the replicated states: the floor, the same rollout without scoring
Below 16,385 lanes (c) and (b) run the four-lanes-per-aircraft kernels, (a) the 64-lane one-lane kernel (include/f16_hip.h).
Prints ONE JSON line: per size the ms per run (median, min, max over the repeats) of the three and the largest relative difference
between the costs of (a) and (b).  No ratio is asserted.  Run from the repository root on the GPU:
    python tools/gpu_time_rollout_cost.py > profiles/rollout_cost_time.jsonl"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from f16_mpc_oop_py_amd import lib
from f16_mpc_oop_py_amd import parameters as P
from f16_mpc_oop_py_amd.workload import config2_states

SIGN = np.array([0, 1, 1, -1, -1, 0, 0, 0, 0, 0.0])
CHUNK = 50           # steps of the stored trajectory reduced at a time in (b)


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def torch_cost(traj, x_rep, rows, hold, xr, ur, w, pen):
    """the cost of include/f16_hip.h from the stored samples traj [T, 18, B]: x_rep [18, B] the initial states, rows [S, 4, B],
    xr [9, B], ur [3, B]; w = (q [9, 1], qf [9, 1], r [3, 1]) on the device"""
    q, qf, r = w
    T, B = traj.shape[0], traj.shape[2]
    lb = torch.as_tensor(P.x_lb, dtype=torch.float64, device=traj.device)[:, None]
    ub = torch.as_tensor(P.x_ub, dtype=torch.float64, device=traj.device)[:, None]
    cmd = (r[None] * (rows[:, 1:4] - ur[None]) ** 2).sum(1)                                  # [S, B]: one term per row
    J = torch.zeros(B, dtype=torch.float64, device=traj.device)
    frozen = torch.zeros(B, dtype=torch.bool, device=traj.device)
    prev = x_rep
    for t0 in range(0, T, CHUNK):
        xs = traj[t0:t0 + CHUNK]                                                             # states AFTER steps t0 .. t0 + n - 1
        before = torch.cat((prev[None], xs[:-1]), 0)                                         # states BEFORE them
        outside = ((before < lb[None]) | (before > ub[None])).any(1)                         # [n, B]
        fr = (torch.cumsum(outside.to(torch.int32), 0) > 0) | frozen[None]
        state = (q[None] * (xs[:, P.mpc_x_idx] - xr[None]) ** 2).sum(1)                      # [n, B]
        rows_of = torch.arange(t0, t0 + xs.shape[0], device=traj.device) // hold
        J += torch.where(fr, torch.full_like(state, pen), state + cmd[rows_of]).sum(0)
        frozen, prev = fr[-1], xs[-1]
    return J + (qf * (prev[P.mpc_x_idx] - xr) ** 2).sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="64x256x100,256x256x100,1024x256x100,1024x256x1000", help="B0 x K x nsteps, comma separated")
    ap.add_argument("--hold", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev, hold = "cuda:0", args.hold
    L = lib.load()
    ctx = lib.Context(0)
    h = ctx.handle
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wv = np.random.default_rng(5).uniform(0.5, 2.0, 21)
    pen = 7.5
    w = lib.make_cost_weights(wv[:9], wv[9:18], wv[18:21], pen)
    wd = tuple(torch.as_tensor(v, device=dev)[:, None] for v in (wv[:9], wv[9:18], wv[18:21]))
    out = dict(tool="gpu_time_rollout_cost", hold=hold, repeats=args.repeats, timer="device events", so=os.path.basename(lib.SO_PATH), cases={})
    for case in args.cases.split(","):
        B0, K, T = (int(v) for v in case.split("x"))
        B, S = B0 * K, (T + hold - 1) // hold
        x0, u0 = config2_states(B0, seed=B0)
        xi = torch.as_tensor(np.ascontiguousarray(x0.T), device=dev)                         # [18, B0]
        x_rep = xi.repeat(1, K)                                                              # [18, B]: lane k * B0 + a = aircraft a
        g = torch.Generator(device=dev)
        g.manual_seed(B0)
        s = torch.as_tensor(SIGN[np.arange(S) % len(SIGN)], device=dev)
        d = torch.as_tensor(np.random.default_rng(7).uniform([-500, -1, -1, -1], [500, 1, 1, 1], (B0, 4)).T.copy(), device=dev)
        base = torch.as_tensor(np.ascontiguousarray(u0.T), device=dev)[None] + s[:, None, None] * d[None]          # [S, 4, B0]
        scale = torch.tensor([100.0, 0.5, 0.5, 0.5], dtype=torch.float64, device=dev)[None, :, None]
        rows = (base.repeat(1, 1, K) + scale * (2 * torch.rand((S, 4, B), generator=g, device=dev, dtype=torch.float64) - 1)).contiguous()
        xr = xi[P.mpc_x_idx].clone()
        xr[4:7] = torch.as_tensor(np.random.default_rng(77 + B0).uniform(-0.1, 0.1, (3, B0)), device=dev)
        ur = (xi[13:16] + 0.1).contiguous()
        xr_rep, ur_rep = xr.repeat(1, K), ur.repeat(1, K)
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        st = torch.zeros(B, dtype=torch.int32, device=dev)
        x = torch.empty_like(x_rep)
        traj = torch.empty((T, 18, B), dtype=torch.float64, device=dev)
        keep = {}

        def scored():
            lib.check(L.f16_rollout_cost(h, vp(xi), B0, B0, vp(rows), vp(xr), vp(ur), ctypes.byref(w), vp(cost), None, None, vp(st), B, B,
                                         T, hold, 1, 0.001, 0.25, 1, 0, stream), L)
            keep["scored"] = cost

        def stored():
            x.copy_(x_rep); st.zero_()                                                      # (the K copies of the initial state)
            lib.check(L.f16_rollout_sched(h, vp(x), vp(rows), vp(traj), vp(st), B, B, T, hold, 1, 0.001, 0.25, 1, 0, stream), L)
            keep["stored"] = torch_cost(traj, x_rep, rows, hold, xr_rep, ur_rep, wd, pen)

        def floor():
            x.copy_(x_rep); st.zero_()
            lib.check(L.f16_rollout_sched(h, vp(x), vp(rows), None, vp(st), B, B, T, hold, 1, 0.001, 0.25, 1, 0, stream), L)

        fns = [("cost_ms", scored), ("sched_stored_plus_torch_cost_ms", stored), ("sched_floor_ms", floor)]
        for _, fn in fns:                                                                    # warm-up: code objects, allocator
            fn()
        torch.cuda.synchronize()
        a, b = keep["scored"].clone(), keep["stored"].clone()
        fin = torch.isfinite(a) & torch.isfinite(b)
        times = {name: [] for name, _ in fns}
        for _ in range(args.repeats):
            for name, fn in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
        res = {name: stat(v) for name, v in times.items()}
        res.update(B0=B0, K=K, lanes=B, nsteps=T, lanes_with_status_bits=int((st != 0).sum()),
                   lanes_with_finite_cost_in_both=int(fin.sum()),
                   max_rel_diff_cost_vs_torch=float(((a - b).abs() / b.abs().clamp(min=1.0))[fin].max()),
                   stored_trajectory_bytes=int(traj.numel() * 8),
                   cost_lane_steps_per_s=B * T / (np.median(times["cost_ms"]) * 1e-3))
        out["cases"][case] = res
        del traj, keep, x, rows, a, b
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
