"""GPU timing of the closed MPC loop with soft state rows (f16_mpc_plan_soft_rows) on the config-5 shard: config-4 flight conditions,
xcg 0.35, N = 30, T = 100 control steps of the plant's 1 ms, zero demands, reference settings (OSQP's defaults, every solve cold), ONE
launch of f16_rollout_mpc per run:
    hard        the hard loop on this build,
    parent      the hard loop on the parent commit's library (`--parent-so PATH`, loaded through F16HIP_SO),
    soft        the soft loop on this build, weight `--weight` (default 100) on the six bounded state rows.
Every run is a process of its own (one warm-up launch of two steps, one timed launch), the three alternating, `--repeats` of each.

Every child process runs under a time limit; the first that fails or runs out of time ends the run (nothing more is started on the
GPU).  Appends one JSON line per batch size to profiles/mpc_soft_time.jsonl (--out): ms per step (median, min, max over the repeats) of
the three, the aircraft that end with status bits 64 / 128 / 32 (and with F16_ST_QP_SOFT_ACTIVE), the mean and the longest ADMM
iteration count, and the two comparisons: hard on this build over the parent (inside the parent's own spread?), soft over hard.
Run from the repository root on the GPU: python tools/gpu_time_mpc_soft.py --parent-so PATH"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 30
DT = 1e-3


def _stat(v):
    import numpy as np
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def child(B, T, weight):
    import torch

    from f16_mpc_oop_py_amd import F16Batch
    from f16_mpc_oop_py_amd.workload import config4_states

    assert torch.cuda.is_available(), "needs the MI355X"
    x0, u0 = config4_states(B)
    env = F16Batch(x0, u0, xcg=0.35, dt=DT, device="cuda:0")
    env.build_ssr()
    env.prepare_MPC(N, **(dict(soft=weight) if weight > 0 else {}))      # (weight 0: the keyword is not passed -- the parent's binding has none)
    env.rollout_MPC(2, 0.0, 0.0, 0.0, N)                                  # warm-up: code objects, the plan's counters
    torch.cuda.synchronize()
    env.reset()
    t0 = time.perf_counter()
    _, info = env.rollout_MPC(T, 0.0, 0.0, 0.0, N, return_info=True)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / T
    st, its = env.status, info["iters"]
    solved = its > 0
    print(json.dumps(dict(B=B, T=T, ms_per_step=ms,
                          flagged={k: int((st & v).ne(0).sum()) for k, v in (("qp_maxiter_64", 64), ("qp_infeasible_128", 128), ("nonfinite_32", 32),
                                                                              ("envelope_16", 16), ("soft_active", 1 << 27))},
                          iters_mean=float(its[solved].double().mean()), iters_max=int(its.max()), solves=int(solved.sum()))), flush=True)


def run_child(args, B, weight, so=None):
    """-> (row or None, error or None)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B), "--steps", str(args.steps), "--weight", str(weight)]
    env = dict(os.environ, **({"F16HIP_SO": os.path.abspath(so)} if so else {}))
    try:
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=args.limit, env=env)
    except subprocess.TimeoutExpired:
        return None, f"B = {B}: no result within {args.limit} s; nothing more was started"
    rows = [json.loads(ln) for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    if r.returncode or not rows:
        return None, f"B = {B}: exit status {r.returncode}; nothing more was started"
    return rows[0], None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,4096")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--weight", type=float, default=100.0)
    ap.add_argument("--parent-so", default="", help="libf16hip.so of the parent commit: adds the hard loop on the parent's library")
    ap.add_argument("--limit", type=int, default=300, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_soft_time.jsonl"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps, args.weight)
    head = dict(tool="gpu_time_mpc_soft", steps=args.steps, repeats=args.repeats, xcg=0.35, hzn=N, demands=[0.0, 0.0, 0.0], weight=args.weight,
                settings="OSQP defaults, cold start, one launch of f16_rollout_mpc")
    legs = [("hard", 0.0, None)] + ([("parent", 0.0, args.parent_so)] if args.parent_so else []) + [("soft", args.weight, None)]
    out, stopped = [], None
    for B in (int(s) for s in args.sizes.split(",")):
        runs = {name: [] for name, _, _ in legs}
        last = {}
        for _ in range(args.repeats):
            for name, weight, so in legs:
                row, stopped = run_child(args, B, weight, so)
                if stopped:
                    break
                runs[name].append(row["ms_per_step"])
                last[name] = row
            if stopped:
                break
        if stopped:
            break
        st = {k: _stat(v) for k, v in runs.items()}
        rec = dict(head, B=B, ms_per_step=st, flagged={k: v["flagged"] for k, v in last.items()},
                   iters_mean={k: v["iters_mean"] for k, v in last.items()}, iters_max={k: v["iters_max"] for k, v in last.items()},
                   solves={k: v["solves"] for k, v in last.items()},
                   soft_over_hard=dict(median=st["soft"]["median"] / st["hard"]["median"], min=st["soft"]["min"] / st["hard"]["max"],
                                       max=st["soft"]["max"] / st["hard"]["min"]))
        if "parent" in st:
            rec.update(hard_over_parent_median=st["hard"]["median"] / st["parent"]["median"],
                       hard_median_inside_parent_min_max=bool(st["parent"]["min"] <= st["hard"]["median"] <= st["parent"]["max"]))
        out.append(rec)
    if stopped:
        out.append(dict(head, stopped=stopped))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for row in out:
            f.write(json.dumps(row) + "\n")
            print(json.dumps(row))
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
