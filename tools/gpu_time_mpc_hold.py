"""GPU timing of the closed MPC loops at a control period of `hold` plant steps: the one-launch loops f16_rollout_mpc_hold /
f16_rollout_mpc_relin_hold against the host loops they replace (dist.closed_loop_mpc_rollout(fused=False, ctrl_every=hold)), per
control step
    frozen:          f16_mpc_plan_solve on the plan of period hold x dt   ->  u.values[1:4] = cmd  ->  rollout(hold)
    re-linearised:   linearise -> ZOH(hold x dt) -> f16_mpc_batch_w       ->  u.values[1:4] = cmd  ->  rollout(hold)
(the whole batch joins after each solve), in the same process, alternating: `--repeats` timed runs of each after a warm-up of each.
Config-4 flight conditions, xcg 0.35, N = 30, OSQP's defaults, demands (0.02, -0.01, 0), plant dt 1 ms, `--nctrl` control steps
(`--period P`: the control period P at every hold, the plant stepped at P / hold).  The
one-launch calls go through the C ABI on a plan that is kept across the runs; the host loops step with the default rollout kernel.

Every batch size runs in a child process of its own under a time limit; the first child that fails or runs out of time ends the
run (nothing more is started on the GPU).  Appends one JSON line per (B, hold) to profiles/mpc_hold_time.jsonl (--out): ms per CONTROL
step (median, min, max over the repeats) of the four loops, the mean ADMM iterations per solve of each, the flagged aircraft.
Run from the repository root on the GPU: python tools/gpu_time_mpc_hold.py"""
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
PLANT_DT = 1e-3


def child(B, nctrl, repeats, holds, period):
    import numpy as np
    import torch

    from f16_mpc_oop_py_amd import F16Batch, dist, lib
    from f16_mpc_oop_py_amd.workload import config4_states

    assert torch.cuda.is_available(), "needs the MI355X"
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    x0, u0 = config4_states(B)
    for hold in holds:
        DT = period / hold if period else PLANT_DT      # (--period: the same control period at every hold)
        envs = {}
        for name in ("fused", "fused_relin", "host", "host_relin"):
            e = envs[name] = F16Batch(x0, u0, xcg=0.35, dt=DT, device="cuda:0")
            e.build_ssr()
            if name != "host_relin":                         # (the re-linearised host loop has no plan: a new model per solve)
                e.prepare_MPC(N, ctrl_every=hold)
        L = envs["fused"].lib
        dem = envs["fused"]._demands(*DEM)
        its = {k: torch.zeros((nctrl, B), dtype=torch.int32, device="cuda:0") for k in ("fused", "fused_relin")}
        ith = {k: torch.zeros((), dtype=torch.float64, device="cuda:0") for k in ("host", "host_relin")}

        def fused():
            e = envs["fused"]
            e.reset()
            lib.check(L.f16_rollout_mpc_hold(e._plan, vp(e._x), vp(e._u), vp(dem), None, None, vp(its["fused"]), vp(e.status), nctrl, hold,
                                             1, DT, e.xcg, e.fi_flag, e.flags, e._stream), L)

        def fused_relin():
            e = envs["fused_relin"]
            e.reset()
            lib.check(L.f16_rollout_mpc_relin_hold(e._plan, vp(e._x), vp(e._u), vp(dem), None, None, vp(its["fused_relin"]), None,
                                                   vp(e.status), nctrl, hold, 1, 1, DT, 1e-5, e.xcg, e.fi_flag, e.flags, e._stream), L)

        def host():
            e = envs["host"]
            e.reset()
            ith["host"].zero_()
            for _ in range(nctrl):
                cmd = e._calc_MPC_action(dem, None, None, N, use_plan=True, ctrl_every=hold)
                ith["host"].add_(e.last_iters.sum())
                e._u[1:4] = cmd.t()
                e.rollout(hold)

        def host_relin():
            e = envs["host_relin"]
            e.reset()
            ith["host_relin"].zero_()
            for _ in range(nctrl):
                cmd = dist._relin_action_at_period(e, dem, N, hold * DT)
                ith["host_relin"].add_(e.last_iters.sum())
                e._u[1:4] = cmd.t()
                e.rollout(hold)

        loops = (("fused", fused), ("host", host), ("fused_relin", fused_relin), ("host_relin", host_relin))
        for _, fn in loops:                                  # warm-up of each (code objects, allocator, dispatch-order history)
            fn()
            torch.cuda.synchronize()
        t = {k: [] for k, _ in loops}
        for _ in range(repeats):
            for name, fn in loops:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) * 1e3 / nctrl)
        stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
        flagged = lambda e: {k: int((e.status & v).ne(0).sum()) for k, v in (("envelope", 16), ("nonfinite", 32), ("qp_maxiter", 64), ("qp_infeasible", 128))}
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps(dict(
            B=B, hold=hold, nctrl=nctrl, plant_dt=DT, ms_per_control_step={k: stat(v) for k, v in t.items()},
            speedup_median=dict(frozen=med["host"] / med["fused"], relin=med["host_relin"] / med["fused_relin"]),
            iters_mean=dict(fused=float(its["fused"].double().mean()), fused_relin=float(its["fused_relin"].double().mean()),
                            host=float(ith["host"]) / (nctrl * B), host_relin=float(ith["host_relin"]) / (nctrl * B)),
            flagged={k: flagged(e) for k, e in envs.items()})), flush=True)
        for e in envs.values():
            e.release_MPC_plan()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,8192")
    ap.add_argument("--holds", default="1,10,20")
    ap.add_argument("--nctrl", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--period", type=float, default=0.0,
                    help="seconds: keep the CONTROL period fixed and step the plant at period / hold (the same QPs at every hold: what "
                         "the hold - 1 extra Euler steps of a pair cost); default: plant dt 1 ms, control period hold x 1 ms")
    ap.add_argument("--limit", type=int, default=300, help="seconds per batch size (its child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_hold_time.jsonl"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    holds = [int(h) for h in args.holds.split(",")]
    if args.child:
        return child(args.child, args.nctrl, args.repeats, holds, args.period)
    head = dict(tool="gpu_time_mpc_hold", nctrl=args.nctrl, repeats=args.repeats, xcg=0.35, hzn=N, demands=DEM,
                settings="OSQP defaults")
    stopped = None
    for B in (int(s) for s in args.sizes.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B), "--nctrl", str(args.nctrl), "--repeats", str(args.repeats),
               "--holds", args.holds, "--period", str(args.period)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            stopped = f"B = {B}: no result within {args.limit} s; nothing more was started"
            break
        rows = [json.loads(ln) for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(dict(head, **row)) + "\n")
                print(json.dumps(dict(head, **row)))
        if r.returncode != 0:
            stopped = f"B = {B}: exit status {r.returncode}; nothing more was started"
            break
    if stopped:
        print(json.dumps(dict(head, stopped=stopped)))
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
