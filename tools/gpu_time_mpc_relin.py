"""GPU timing of the closed MPC loop with per-step re-linearisation: the one-launch loop f16_rollout_mpc_relin against
the host loop it replaces, per step
    _calc_MPC_action(dem, None, None, 30, relinearise=True)  ->  u.values[1:4] = cmd  ->  rollout(1)
(linearise, ZOH, QP build, first-order kernel, solve, order kernel, one-step rollout: the whole batch joins after each), in the same
process, alternating, `--repeats` timed runs of each after a warm-up of each (config-4 flight conditions, xcg 0.35, N = 30, OSQP's
defaults, demands (0.02, -0.01, 0)).  Also timed, same states: f16_rollout_mpc, the frozen-model loop, so that the cost of the model
stage per (step, aircraft) pair is visible.  The one-launch calls go through the C ABI on a plan that is kept across the runs (what a
caller who loops does); F16Batch.rollout_MPC(relinearise=True) is that call plus the allocation of its outputs.

Every batch size runs in a child process of its own under a time limit; the first child that fails or runs out of time ends the
run (nothing more is started on the GPU).  Prints ONE JSON line: per B the ms per step (median, min, max over the repeats) of the three
loops, the mean ADMM iterations per solve of each, the flagged aircraft, and whether the one launch beats the host loop by more than
the spread of the alternating runs.  Run from the repository root on the GPU: python tools/gpu_time_mpc_relin.py"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEM = (0.02, -0.01, 0.0)
N = 30


def child(B, T, repeats):
    import numpy as np
    import torch

    from f16_mpc_oop_py_amd import F16Batch, lib
    from f16_mpc_oop_py_amd.workload import config4_states

    assert torch.cuda.is_available(), "needs the MI355X"
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    x0, u0 = config4_states(B)
    env = F16Batch(x0, u0, xcg=0.35, device="cuda:0")
    env.build_ssr()
    env.prepare_MPC(N)
    L, plan_relin = env.lib, env._plan
    dem = env._demands(*DEM)
    its = torch.zeros((T, B), dtype=torch.int32, device="cuda:0")
    envf = F16Batch(x0, u0, xcg=0.35, device="cuda:0")        # the frozen loop keeps a plan (and a model) of its own
    envf.build_ssr()
    envf.prepare_MPC(N)
    itf = torch.zeros((T, B), dtype=torch.int32, device="cuda:0")
    envh = F16Batch(x0, u0, xcg=0.35, device="cuda:0")
    ith = torch.zeros((), dtype=torch.float64, device="cuda:0")

    def fused():
        env.reset()
        lib.check(L.f16_rollout_mpc_relin(plan_relin, vp(env._x), vp(env._u), vp(dem), None, None, vp(its), None, vp(env.status), T, 1, 1e-5,
                                          env.xcg, env.fi_flag, env.flags, env._stream), L)

    def frozen():
        envf.reset()
        lib.check(L.f16_rollout_mpc(envf._plan, vp(envf._x), vp(envf._u), vp(dem), None, None, vp(itf), vp(envf.status), T, 1, envf.xcg,
                                    envf.fi_flag, envf.flags, envf._stream), L)

    def host():
        envh.reset()
        ith.zero_()
        for _ in range(T):
            cmd = envh._calc_MPC_action(dem, None, None, N, relinearise=True)
            ith.add_(envh.last_iters.sum())
            envh._u[1:4] = cmd.t()
            envh.rollout(1)

    for fn in (fused, host, frozen):                          # warm-up of each (code objects, allocator, dispatch-order history)
        fn()
        torch.cuda.synchronize()
    t = dict(fused=[], host=[], frozen=[])
    for _ in range(repeats):
        for name, fn in (("fused", fused), ("host", host), ("frozen", frozen)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3 / T)
    stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
    spread = max(max(t["fused"]) - min(t["fused"]), max(t["host"]) - min(t["host"]))
    gain = float(np.median(t["host"]) - np.median(t["fused"]))
    flagged = lambda e: {k: int((e.status & v).ne(0).sum()) for k, v in (("envelope", 16), ("nonfinite", 32), ("qp_maxiter", 64), ("qp_infeasible", 128))}
    print(json.dumps(dict(
        B=B, fused_ms_per_step=stat(t["fused"]), host_ms_per_step=stat(t["host"]), frozen_ms_per_step=stat(t["frozen"]),
        host_minus_fused_ms_per_step=gain, spread_of_the_alternating_runs_ms=float(spread), fused_faster_than_spread=bool(gain > spread),
        speedup_median=float(np.median(t["host"]) / np.median(t["fused"])),
        model_stage_us_per_pair_on_1024_simds=float((np.median(t["fused"]) - np.median(t["frozen"])) * 1e3 * 1024 / B),
        iters_mean=dict(fused=float(its.double().mean()), host=float(ith) / (T * B), frozen=float(itf.double().mean())),
        iters_max=dict(fused=int(its.max()), frozen=int(itf.max())),
        flagged=dict(fused=flagged(env), host=flagged(envh), frozen=flagged(envf)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,4096")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per batch size (its child process)")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps, args.repeats)
    out = dict(tool="gpu_time_mpc_relin", steps=args.steps, repeats=args.repeats, xcg=0.35, hzn=N, demands=DEM, settings="OSQP defaults",
               so=os.path.basename(os.environ.get("F16HIP_SO", "libf16hip.so")), sizes={})
    for B in (int(s) for s in args.sizes.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B), "--steps", str(args.steps), "--repeats", str(args.repeats)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            out["stopped"] = f"B = {B}: no result within {args.limit} s; nothing more was started"
            break
        if r.returncode != 0:
            out["stopped"] = f"B = {B}: exit status {r.returncode}; nothing more was started"
            break
        out["sizes"][str(B)] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return 1 if "stopped" in out else 0


if __name__ == "__main__":
    sys.exit(main())
