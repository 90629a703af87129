"""GPU timing of the LQR loop under a gain schedule (f16_rollout_lqr_gs) beside the loops it stands between: medians of `--repeats`
device-event timings of 1,000 Euler steps, hifi, config-2 flight conditions (xcg 0.25), a 32 x 32 table over their altitudes and
airspeeds (the G7 gain scaled per node: what is timed does not depend on the values), gs_every = 1, 10, 100.  Baselines, same states:
  lqr        f16_rollout_lqr, default flags (the frozen gain; below 16,385 aircraft the four-lanes-per-aircraft / four-wavefront kernels)
  cost       f16_rollout_cost at the same number of lanes (the one-lane kernel family the scheduled-gain loop runs, open loop)
  lqr_relin  f16_rollout_lqr_relin (the gain re-derived at every step), `--relin-steps` steps, reported per step
Every loop runs under F16_FLAG_NO_ENVELOPE, so that no lane is frozen and every lane does the work of every step.  Nothing is
asserted.  Writes one JSON line per batch size to --out (default profiles/lqr_gs_time.jsonl) and prints it.
Run from the repository root on the GPU: python tools/gpu_time_lqr_gs.py"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from f16_mpc_oop_py_amd import F16Batch, lib
from f16_mpc_oop_py_amd.schedule import GainSchedule
from f16_mpc_oop_py_amd.workload import TRIM_XCG25, config2_states

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX9 = [3, 4, 7, 8, 9, 10, 11, 17, 16]
NO_ENVELOPE = lib.F16_FLAG_NO_ENVELOPE


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def table_32x32():
    K = np.load(os.path.join(REPO, "tests", "golden", "g567_trim_lin_lqr.npz"))["K_lqr_xcg25"][:, 4:7].ravel()
    rng = np.random.default_rng(1)
    scale, off = 1.0 + 0.2 * rng.uniform(-1, 1, (32, 32, 1)), rng.uniform(-0.5, 0.5, (32, 32, 3))
    return GainSchedule(5e3, 2.5e4 / 31, 32, 400.0, 450.0 / 31, 32, np.concatenate((K * scale, TRIM_XCG25[13:16] + off), 2))


def timed(fn, reset, repeats):
    """median, min, max [ms] of `repeats` device-event timings of fn(), reset() before each (untimed)"""
    ms = []
    for _ in range(repeats + 1):                                               # (the first run warms up: code objects, allocator)
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms = ms[1:]
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--relin-steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lqr_gs_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    T, xcg, dev = args.steps, 0.25, "cuda:0"
    gs = table_32x32()
    grid, tab = gs.grid(), gs.device_table(dev)
    lines = []
    for B in (int(s) for s in args.sizes.split(",")):
        x0, u0 = config2_states(B)
        env = F16Batch(x0, u0, xcg=xcg, device=dev, flags=NO_ENVELOPE)
        L, h, stream = env.lib, env.ctx.handle, env._stream
        K = torch.zeros((27, B), dtype=torch.float64, device=dev)
        g0 = torch.as_tensor(gs.table[16, 16], device=dev)
        for i in range(3):
            K[9 * i + 4:9 * i + 7] = g0[3 * i:3 * i + 3, None]
        dem = torch.zeros((3, B), dtype=torch.float64, device=dev)
        gs_out = torch.zeros(B, dtype=torch.int32, device=dev)
        xr = torch.as_tensor(np.ascontiguousarray(x0[:, IDX9].T), device=dev)
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        cst = torch.empty(B, dtype=torch.int32, device=dev)
        w, wl = lib.make_cost_weights(), lib.make_weights(Q=np.eye(9), R=np.eye(3) * 1e4)

        def run_gs(every):
            return lambda: lib.check(L.f16_rollout_lqr_gs(h, vp(env._x), vp(env._u_init), ctypes.byref(grid), vp(tab), every, vp(dem), None, None,
                                                          vp(gs_out), vp(env.status), B, B, T, T, 1, env.dt, xcg, 1, lib.F16_INT_EULER,
                                                          NO_ENVELOPE, stream), L)

        run_lqr = lambda: lib.check(L.f16_rollout_lqr(h, vp(env._x), vp(env._u_init), vp(K), vp(dem), None, None, vp(env.status), B, B, T, 1,
                                                      env.dt, xcg, 1, NO_ENVELOPE, stream), L)
        run_cost = lambda: lib.check(L.f16_rollout_cost(h, vp(env._x), B, B, vp(env._u_init), vp(xr), None, ctypes.byref(w), vp(cost), None, None,
                                                        vp(cst), B, B, T, T, 1, env.dt, xcg, 1, NO_ENVELOPE, stream), L)
        run_relin = lambda: lib.check(L.f16_rollout_lqr_relin(h, vp(env._x), vp(env._u), vp(xr), None, ctypes.byref(wl), None, None, None,
                                                              vp(env.status), B, B, args.relin_steps, args.relin_steps, 0x1FF, 1e-5, env.dt,
                                                              xcg, 1, NO_ENVELOPE, stream), L)
        rate = lambda t, steps: B * steps / (t["median"] * 1e-3)
        rec = dict(tool="gpu_time_lqr_gs", B=B, steps=T, repeats=args.repeats, xcg=xcg, fi="hifi", method="euler", table="32 x 32",
                   flags="F16_FLAG_NO_ENVELOPE", so=os.path.basename(lib.SO_PATH), ms={}, aircraft_steps_per_s={})
        for every in (1, 10, 100):
            t = timed(run_gs(every), env.reset, args.repeats)
            rec["ms"][f"lqr_gs_every_{every}"], rec["aircraft_steps_per_s"][f"lqr_gs_every_{every}"] = t, rate(t, T)
            rec[f"outside_updates_every_{every}"] = int(gs_out.sum())
        for name, fn, steps in (("lqr", run_lqr, T), ("cost", run_cost, T), ("lqr_relin", run_relin, args.relin_steps)):
            t = timed(fn, env.reset, args.repeats)
            rec["ms"][name], rec["aircraft_steps_per_s"][name] = t, rate(t, steps)
        rec["relin_steps"] = args.relin_steps
        print(json.dumps(rec))
        lines.append(json.dumps(rec))
        del env
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
