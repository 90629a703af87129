"""GPU timing of a rollout under a command schedule: ONE launch of f16_rollout_sched against the chain of f16_rollout launches it
replaces -- one launch per input change, each behind the host-to-device copy of its row (pinned host memory, asynchronous: the
cheapest way to run the chain) -- and against f16_rollout with a constant input, in the same process, alternating, `--repeats`
timed runs of each after a warm-up, every step stored (traj_every = 1).  Per batch size (config-2 flight conditions, the doublet
of the tests with a new row every `hold` steps, hold = 100, 10, 1):
    (a) f16_rollout                       constant input, one launch
    (b) f16_rollout_sched                 one launch per hold
    (c) chain of f16_rollout + row copy   steps / hold launches per hold
Prints ONE JSON line: per B the ms per run (median, min, max over the repeats), the ratios, and the largest (b) - (c) difference of
the final states and of the stored samples (relative, max(1, |x|)), which is zero wherever the contract of include/f16_hip.h says bit
for bit.  Run from the repository root on the GPU: python tools/gpu_time_rollout_sched.py > profiles/rollout_sched_time.jsonl"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from f16_mpc_oop_py_amd import lib
from f16_mpc_oop_py_amd.workload import config2_states

SIGN = np.array([0, 1, 1, -1, -1, 0, 0, 0, 0, 0.0])


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,8192,262144")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--holds", default="100,10,1")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    T, dev = args.steps, "cuda:0"
    holds = [int(h) for h in args.holds.split(",")]
    L = lib.load()
    ctx = lib.Context(0)
    h = ctx.handle
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = dict(tool="gpu_time_rollout_sched", steps=T, traj_every=1, repeats=args.repeats, pinned=True, so=os.path.basename(lib.SO_PATH), sizes={})
    for B in (int(s) for s in args.sizes.split(",")):
        x0, u0 = config2_states(B)
        xi = torch.as_tensor(np.ascontiguousarray(x0.T), device=dev)
        ui = torch.as_tensor(np.ascontiguousarray(u0.T), device=dev)
        d = np.random.default_rng(7).uniform([-500, -1, -1, -1], [500, 1, 1, 1], (B, 4)).T           # [4, B]
        x = torch.empty_like(xi)
        u = torch.empty_like(ui)
        st = torch.zeros(B, dtype=torch.int32, device=dev)
        traj = torch.empty((T, 18, B), dtype=torch.float64, device=dev)
        keep = {}

        def const():
            x.copy_(xi); st.zero_()
            lib.check(L.f16_rollout(h, vp(x), vp(ui), vp(traj), vp(st), B, B, T, 1, 0.001, 0.25, 1, 0, stream), L)

        def make(hold):
            S = (T + hold - 1) // hold
            s = SIGN[np.arange(S) % len(SIGN)]
            rows_h = torch.as_tensor(u0.T[None] + s[:, None, None] * d[None]).contiguous()                  # [S, 4, B] on the host
            try:
                rows_h = rows_h.pin_memory()
            except RuntimeError:                                                    # (a page-lock limit: the copies are then synchronous)
                out["pinned"] = False
            rows_d = rows_h.to(dev)

            def sched():
                x.copy_(xi); st.zero_()
                lib.check(L.f16_rollout_sched(h, vp(x), vp(rows_d), vp(traj), vp(st), B, B, T, hold, 1, 0.001, 0.25, 1, 0, stream), L)

            def chain():
                x.copy_(xi); st.zero_()
                for r in range(S):
                    n = min(hold, T - r * hold)
                    u.copy_(rows_h[r], non_blocking=True)
                    lib.check(L.f16_rollout(h, vp(x), vp(u), vp(traj[r * hold:r * hold + n]), vp(st), B, B, n, 1, 0.001, 0.25, 1, 0,
                                            stream), L)
            return sched, chain

        fns = [("const", const)]
        for hold in holds:
            sc, ch = make(hold)
            fns += [(f"sched_hold{hold}", sc), (f"chain_hold{hold}", ch)]
        res = {}
        for name, fn in fns:                                                        # warm-up (code objects, allocator) + results
            fn(); torch.cuda.synchronize()
            keep[name] = (x.clone(), traj[T - 1].clone(), traj[T // 2].clone(), int((st != 0).sum()))
        times = {name: [] for name, _ in fns}
        for _ in range(args.repeats):
            for name, fn in fns:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
        rel = lambda a, b: float(((a - b).abs() / b.abs().clamp(min=1.0)).max())
        res["const_ms"] = stat(times["const"])
        for hold in holds:
            a, b = keep[f"sched_hold{hold}"], keep[f"chain_hold{hold}"]
            ts, tc = times[f"sched_hold{hold}"], times[f"chain_hold{hold}"]
            res[f"hold{hold}"] = dict(sched_ms=stat(ts), chain_ms=stat(tc), chain_launches=(T + hold - 1) // hold,
                                      chain_over_sched_median=float(np.median(tc) / np.median(ts)),
                                      sched_over_const_median=float(np.median(ts) / np.median(times["const"])),
                                      max_rel_diff_sched_vs_chain=max(rel(a[0], b[0]), rel(a[1], b[1]), rel(a[2], b[2])),
                                      aircraft_with_status_bits=a[3])
        res["sched_aircraft_steps_per_s"] = {f"hold{hd}": B * T / (np.median(times[f"sched_hold{hd}"]) * 1e-3) for hd in holds}
        out["sizes"][str(B)] = res
        del traj, keep
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
