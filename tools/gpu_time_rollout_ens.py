"""GPU timing of the ensemble statistics inside the launch (f16_rollout_wind_ens, traj = NULL) against the way of the commit before
it: the unchanged f16_rollout_wind storing every sample, followed by torch mean / var / amin / amax over the aircraft.

1,000 steps of 1 ms, hifi, steady wind and in-kernel gusts at gust_hold = 10, B = 4,096 and 262,144, a sample every step and every
10 steps, both methods, one group (the whole batch).  Per point:
    ens        f16_rollout_wind_ens, traj = NULL: both launches of the call (the rollout and the finishing kernel)
    baseline   f16_rollout_wind with traj [S][18][B] + the four torch reductions over the last axis (unmasked: the least a user would
               do today); `store` and `reduce` are its two parts, timed in the same runs
Protocol: a process per batch size (the parent never touches the GPU; the children run one after another, each under a time limit,
and the first that fails ends the run); in it, per point, one warm-up of each variant and then `--repeats` rounds of the two
variants alternating, each call between device events with the state put back before the first event; medians with min .. max.
The sibling's own time (f16_rollout_wind, steady wind only, no samples, B = 4,096 -- the `wind` variant of
tools/gpu_time_rollout_wind.py) is measured the same way and held against profiles/rollout_wind_time.jsonl: `sibling_matches` says
whether its median lies within 3 % of the recorded one (another day, another machine of the pool; the recorded spread is 1 %).
From the repository root, on the GPU:
    python tools/gpu_time_rollout_ens.py            (writes profiles/rollout_ens_time.jsonl; --out FILE for another place)
--against-parent: instead, f16_rollout_wind_ens and f16_rollout_lqr_wind_ens (steady wind, one group, one sample, no traj) of this build
against the same calls of the parent commit's library, by the protocol of tools/gpu_time_rollout_wind.py (alternate: a process per
run at B = 4,096 and 65,536, this build's median inside the parent's min .. max); prints the lines."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import gpu_time_rollout_wind as W  # noqa: E402

PAIRS = ("wind_ens_parent", "wind_ens", "lqr_ens_parent", "lqr_ens")
SIZES = (4096, 262144)
NSTEPS, DT, GHOLD = 1000, 0.001, 10
PERIODS = (1, 10)


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def run(B, repeats):
    """one process: every point of one batch size -> JSON lines"""
    import numpy as np
    import torch
    from f16_mpc_oop_py_amd import lib
    from f16_mpc_oop_py_amd.wind import gust_coefficients
    from f16_mpc_oop_py_amd.workload import config2_states
    assert torch.cuda.is_available(), "needs the MI355X"
    L = lib.load()
    ctx = lib.Context(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x0, u0 = config2_states(B, seed=B)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
    x0, u = dev(x0.T), dev(u0.T)
    x, st = x0.clone(), torch.zeros(B, dtype=torch.int32, device="cuda:0")
    rng = np.random.default_rng(B)
    wind = dev(rng.uniform(-20, 20, (3, B)))
    a, b = gust_coefficients([5.0, 5.0, 3.0], [1750.0, 1750.0, 500.0], 600.0, GHOLD * DT)
    ga, gb, gs = dev(np.repeat(a[:, None], B, 1)), dev(np.repeat(b[:, None], B, 1)), torch.zeros((3, B), dtype=torch.float64, device="cuda:0")
    steady, gusty = lib.Wind(), lib.Wind()
    steady.wind_ned = gusty.wind_ned = wind.data_ptr()
    gusty.ga, gusty.gb, gusty.gstate, gusty.gust_hold, gusty.seed = ga.data_ptr(), gb.data_ptr(), gs.data_ptr(), GHOLD, 7

    def reset():
        x.copy_(x0); st.zero_(); gs.zero_()

    def timed(f):
        reset()
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        mid = f()
        if mid:
            e[1].record()
            mid()
        e[2].record()
        torch.cuda.synchronize()
        return (e[0].elapsed_time(e[2]),) + ((e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])) if mid else ())

    stats = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
    for name, method in (("euler", lib.F16_INT_EULER), ("rk4", lib.F16_INT_RK4)):
        if B == SIZES[0]:          # the sibling as tools/gpu_time_rollout_wind.py times its `wind` variant
            sib = lambda: lib.check(L.f16_rollout_wind(ctx.handle, vp(x), vp(u), ctypes.byref(steady), None, vp(st), B, B, NSTEPS, NSTEPS, 1, DT, 0.25,
                                                       1, method, 0, stream), L)
            timed(sib)
            t = [timed(sib)[0] for _ in range(repeats)]
            print(json.dumps(dict(point="sibling", B=B, method=name, nsteps=NSTEPS, repeats=repeats, ms=stats(t))), flush=True)
        for every in PERIODS:
            S, G = NSTEPS // every, 1
            group = (B + 63) // 64 * 64
            traj = torch.empty((S, 18, B), dtype=torch.float64, device="cuda:0")
            work = torch.empty(L.f16_ens_work_doubles(B, S), dtype=torch.float64, device="cuda:0")
            count = torch.zeros((S, G), dtype=torch.int32, device="cuda:0")
            res = [torch.zeros((S, 18, G), dtype=torch.float64, device="cuda:0") for _ in range(4)]
            e = lib.Ens()
            e.work, e.group, e.ldg, e.count = work.data_ptr(), group, G, count.data_ptr()
            e.mean, e.m2, e.min, e.max = (r.data_ptr() for r in res)

            def ens():
                lib.check(L.f16_rollout_wind_ens(ctx.handle, vp(x), vp(u), ctypes.byref(gusty), None, ctypes.byref(e), vp(st), B, B, NSTEPS, NSTEPS,
                                                 every, DT, 0.25, 1, method, 0, stream), L)

            def baseline():
                lib.check(L.f16_rollout_wind(ctx.handle, vp(x), vp(u), ctypes.byref(gusty), vp(traj), vp(st), B, B, NSTEPS, NSTEPS, every, DT, 0.25,
                                             1, method, 0, stream), L)
                return lambda: (traj.mean(-1), traj.var(-1), traj.amin(-1), traj.amax(-1))

            timed(ens); timed(baseline)
            te, tb = [], []
            for _ in range(repeats):
                te.append(timed(ens)[0])
                tb.append(timed(baseline))
            tb = np.array(tb)
            out = dict(point="ensemble", B=B, method=name, nsteps=NSTEPS, sample_every=every, group=group, repeats=repeats,
                       timer="device events, variants alternating in one process", contributing_last_sample=int(count[-1, 0]),
                       ms=dict(ens=stats(te), baseline=stats(tb[:, 0]), store=stats(tb[:, 1]), reduce=stats(tb[:, 2])))
            out["ens_over_baseline"] = out["ms"]["ens"]["median"] / out["ms"]["baseline"]["median"]
            out["traj_bytes_not_written"] = S * 18 * B * 8
            print(json.dumps(out), flush=True)
            del traj, work, res
            torch.cuda.empty_cache()


def run_pair(variant, B):
    """one process of --against-parent: per method one warm-up call and one timed call -> a JSON line"""
    import numpy as np
    import torch
    from f16_mpc_oop_py_amd import lib
    from f16_mpc_oop_py_amd.workload import config2_states
    assert torch.cuda.is_available(), "needs the MI355X"
    L = lib.load()
    ctx = lib.Context(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x0, u0 = config2_states(B, seed=B)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
    x0, u = dev(x0.T), dev(u0.T)
    x, st = x0.clone(), torch.zeros(B, dtype=torch.int32, device="cuda:0")
    wind = dev(np.random.default_rng(B).uniform(-20, 20, (3, B)))
    air, e = lib.Wind(), lib.Ens()
    air.wind_ned = wind.data_ptr()
    keep = [torch.zeros(L.f16_ens_work_doubles(B, 1), dtype=torch.float64, device="cuda:0"), torch.zeros((1, 1), dtype=torch.int32, device="cuda:0")]
    keep += [torch.zeros((1, 18, 1), dtype=torch.float64, device="cuda:0") for _ in range(4)]
    e.group, e.ldg = (B + 63) // 64 * 64, 1
    e.work, e.count, e.mean, e.m2, e.min, e.max = (t.data_ptr() for t in keep)
    K = dev(np.repeat(np.load(os.path.join(REPO, "tests", "golden", "g567_trim_lin_lqr.npz"))["K_lqr_xcg25"].reshape(27, 1), B, 1))
    dem = torch.zeros((3, B), dtype=torch.float64, device="cuda:0")

    def reset():
        x.copy_(x0); st.zero_()

    def call(method):
        if variant.startswith("lqr"):
            rc = L.f16_rollout_lqr_wind_ens(ctx.handle, vp(x), vp(u), vp(K), vp(dem), ctypes.byref(air), None, ctypes.byref(e), None, vp(st), B, B, W.NSTEPS,
                                            W.NSTEPS, W.NSTEPS, W.DT, 0.25, 1, method, 0, stream)
        else:
            rc = L.f16_rollout_wind_ens(ctx.handle, vp(x), vp(u), ctypes.byref(air), None, ctypes.byref(e), vp(st), B, B, W.NSTEPS, W.NSTEPS, W.NSTEPS, W.DT,
                                        0.25, 1, method, 0, stream)
        lib.check(rc, L)

    print(json.dumps(W.timed_methods(variant, B, reset, call, st)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", nargs="+", metavar="B", help="one batch size in this process, or VARIANT B of --against-parent (what the parent starts)")
    ap.add_argument("--against-parent", action="store_true")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rollout_ens_time.jsonl"))
    args = ap.parse_args()
    if args.run:
        return run(int(args.run[0]), args.repeats) if len(args.run) == 1 else run_pair(args.run[0], int(args.run[1]))
    if args.against_parent:
        return W.alternate(__file__, PAIRS, W.SIZES, args.repeats, W.ONE_LANE_FAMILY)
    recorded = {}
    for line in open(os.path.join(REPO, "profiles", "rollout_wind_time.jsonl")):
        r = json.loads(line)
        recorded[(r["B"], r["method"])] = r["ms"]["wind"]
    env = {k: v for k, v in os.environ.items() if k not in ("F16_DYN_BLOCK", "F16_ROLLOUT_I32", "F16HIP_SO")}
    lines = []
    for B in SIZES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--run", str(B), "--repeats", str(args.repeats)], env=env,
                           capture_output=True, text=True, timeout=540)
        if p.returncode != 0:
            sys.exit(f"the run at B = {B} ended with status {p.returncode}: nothing more is started\n{p.stderr[-2000:]}")
        for line in p.stdout.splitlines():
            if not line.startswith("{"):
                continue
            r = json.loads(line)
            if r["point"] == "sibling":
                was = recorded[(r["B"], r["method"])]
                r["recorded"] = was
                r["sibling_matches"] = bool(abs(r["ms"]["median"] / was["median"] - 1.0) <= 0.03)
            lines.append(json.dumps(r))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
