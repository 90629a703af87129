"""GPU timing of the closed MPC loop under a demand schedule: the same schedule of one demand row per control step through
    (i)   sched:  ONE launch of f16_rollout_mpc_sched (dem_hold = 1),
    (ii)  chain:  one existing call per row, f16_rollout_mpc_hold(nctrl = 1) with that row as the constant demand -- every launch
                  boundary joins the batch, as the host loop does,
    (iii) const:  ONE existing launch of f16_rollout_mpc_hold with row 0 as the constant demand (other QPs: the cost of a launch that
                  reads no schedule),
in the same process, alternating: `--repeats` timed runs of each after a warm-up of each.  Config-4 flight conditions, xcg 0.35,
N = 30, OSQP's defaults, plant dt 1 ms, `--nctrl` control steps, rows (+0.02, -0.02, 0) / (-0.02, +0.02, 0) rad/s in turn.

`--parent-so PATH` (a libf16hip.so built from the parent commit) adds the no-slowdown check of the unchanged call: f16_rollout_mpc_hold at
`--ab-size` aircraft, the same holds, on this build and on the parent's library (loaded through F16HIP_SO in a process of its own),
the two alternating process by process, `--repeats` processes of each with one warm-up and one timed run per hold.

Every child process runs under a time limit; the first that fails or runs out of time ends the run (nothing more is started on the
GPU).  Appends one JSON line per (B, hold), and one per hold of the A/B, to profiles/mpc_sched_time.jsonl (--out): ms per CONTROL step
(median, min, max over the repeats), the ratios sched / chain and sched / const of the medians with the spread of each, the mean
ADMM iterations per solve.  Run from the repository root on the GPU: python tools/gpu_time_mpc_sched.py"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW = (0.02, -0.02, 0.0)
N = 30
DT = 1e-3


def _stat(v):
    import numpy as np
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def child(B, nctrl, repeats, holds, ab):
    import torch

    from f16_mpc_oop_py_amd import F16Batch, lib
    from f16_mpc_oop_py_amd.workload import config4_states

    assert torch.cuda.is_available(), "needs the MI355X"
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    x0, u0 = config4_states(B)
    sign = torch.as_tensor([1.0 if c % 2 == 0 else -1.0 for c in range(nctrl)], dtype=torch.float64, device="cuda:0")
    rows = (sign[:, None, None] * torch.as_tensor(ROW, dtype=torch.float64, device="cuda:0")[None, :, None]).expand(nctrl, 3, B).contiguous()
    for hold in holds:
        names = ("const",) if ab else ("sched", "chain", "const")
        envs = {}
        for name in names:
            e = envs[name] = F16Batch(x0, u0, xcg=0.35, dt=DT, device="cuda:0")
            e.build_ssr()
            e.prepare_MPC(N, ctrl_every=hold)
        L = envs["const"].lib
        its = {k: torch.zeros((nctrl, B), dtype=torch.int32, device="cuda:0") for k in names}

        def sched():
            e = envs["sched"]
            e.reset()
            lib.check(L.f16_rollout_mpc_sched(e._plan, vp(e._x), vp(e._u), vp(rows), None, None, vp(its["sched"]), vp(e.status), nctrl, hold,
                                              1, 1, DT, e.xcg, e.fi_flag, e.flags, e._stream), L)

        def chain():
            e = envs["chain"]
            e.reset()
            for c in range(nctrl):
                lib.check(L.f16_rollout_mpc_hold(e._plan, vp(e._x), vp(e._u), vp(rows[c]), None, None, vp(its["chain"][c]), vp(e.status), 1,
                                                 hold, 1, DT, e.xcg, e.fi_flag, e.flags, e._stream), L)

        def const():
            e = envs["const"]
            e.reset()
            lib.check(L.f16_rollout_mpc_hold(e._plan, vp(e._x), vp(e._u), vp(rows[0]), None, None, vp(its["const"]), vp(e.status), nctrl, hold,
                                             1, DT, e.xcg, e.fi_flag, e.flags, e._stream), L)

        loops = [(k, dict(sched=sched, chain=chain, const=const)[k]) for k in names]
        for _, fn in loops:                                  # warm-up of each (code objects, allocator, counters of the plan)
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
        if not ab:      # the two paths solve the same QPs
            assert bool((its["sched"] == its["chain"]).all()) and bool((envs["sched"]._x == envs["chain"]._x).all()), "sched != chain"
        flagged = lambda e: {k: int((e.status & v).ne(0).sum()) for k, v in (("envelope", 16), ("nonfinite", 32), ("qp_maxiter", 64), ("qp_infeasible", 128))}
        print(json.dumps(dict(B=B, hold=hold, nctrl=nctrl, ms_per_control_step_runs=t,
                              iters_mean={k: float(v.double().mean()) for k, v in its.items()},
                              flagged={k: flagged(e) for k, e in envs.items()})), flush=True)
        for e in envs.values():
            e.release_MPC_plan()


def run_child(args, B, ab=False, so=None, repeats=None):
    """-> (rows, error or None)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B), "--nctrl", str(args.nctrl), "--holds", args.holds,
           "--repeats", str(repeats or args.repeats)] + (["--ab"] if ab else [])
    env = dict(os.environ, **({"F16HIP_SO": os.path.abspath(so)} if so else {}))
    try:
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=args.limit, env=env)
    except subprocess.TimeoutExpired:
        return [], f"B = {B}: no result within {args.limit} s; nothing more was started"
    rows = [json.loads(ln) for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    return rows, (f"B = {B}: exit status {r.returncode}; nothing more was started" if r.returncode else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,8192")
    ap.add_argument("--holds", default="1,20")
    ap.add_argument("--nctrl", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-so", default="", help="libf16hip.so of the parent commit: adds the A/B of the unchanged f16_rollout_mpc_hold")
    ap.add_argument("--ab-size", type=int, default=4096)
    ap.add_argument("--limit", type=int, default=300, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_sched_time.jsonl"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--ab", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    holds = [int(h) for h in args.holds.split(",")]
    if args.child:
        return child(args.child, args.nctrl, args.repeats, holds, args.ab)
    head = dict(tool="gpu_time_mpc_sched", nctrl=args.nctrl, repeats=args.repeats, xcg=0.35, hzn=N, dem_hold=1, rows=[ROW, [-v for v in ROW]],
                settings="OSQP defaults")
    out = []
    stopped = None
    for B in (int(s) for s in args.sizes.split(",")):
        rows, stopped = run_child(args, B)
        for row in rows:
            t = row.pop("ms_per_control_step_runs")
            st = {k: _stat(v) for k, v in t.items()}
            ratio = lambda a, b: dict(median=st[a]["median"] / st[b]["median"], min=st[a]["min"] / st[b]["max"], max=st[a]["max"] / st[b]["min"])
            out.append(dict(head, **row, ms_per_control_step=st, sched_over_chain=ratio("sched", "chain"), sched_over_const=ratio("sched", "const")))
        if stopped:
            break
    if args.parent_so and not stopped:
        # the unchanged call on both builds, alternating process by process: one warm-up and one timed run per hold in each
        runs = {"this": {h: [] for h in holds}, "parent": {h: [] for h in holds}}
        iters = {"this": {}, "parent": {}}
        for _ in range(args.repeats):
            for build, so in (("this", None), ("parent", args.parent_so)):
                rows, stopped = run_child(args, args.ab_size, ab=True, so=so, repeats=1)
                for row in rows:
                    runs[build][row["hold"]] += row["ms_per_control_step_runs"]["const"]
                    iters[build][row["hold"]] = row["iters_mean"]["const"]
                if stopped:
                    break
            if stopped:
                break
        for h in holds:
            if runs["this"][h] and runs["parent"][h]:
                a, b = _stat(runs["this"][h]), _stat(runs["parent"][h])
                out.append(dict(head, check="f16_rollout_mpc_hold on this build against the parent commit's library", B=args.ab_size, hold=h,
                                ms_per_control_step=dict(this=a, parent=b), this_over_parent_median=a["median"] / b["median"],
                                this_median_inside_parent_min_max=bool(b["min"] <= a["median"] <= b["max"]),
                                iters_mean=dict(this=iters["this"][h], parent=iters["parent"][h])))
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
