"""GPU timing of the Runge-Kutta rollouts against the Euler ones.  Three parts, each one JSON line; medians of `--repeats` device-event
timings after a warm-up, the two sides of a comparison alternating in one process:

  (i)   per_step   time per RK4 step over time per Euler step on the SAME kernel family (one lane per aircraft): the Euler side needs
                   F16_ROLLOUT_QUAD_MAXB=0 F16_ROLLOUT_4W_MAXB=0, so this part runs in a child process of its own with those set.
                   B = 4,096 / 32,768 / 262,144, every step stored and none stored.  Ideal 4 (four evaluations, one store); RK4
                   gives up the carried sin / cos pairs, so somewhat above.  Recorded, not asserted.
  (ii)  flight     10 s of flight with 1,000 stored samples: f16_rollout_rk, 1,000 RK4 steps of 10 ms, every step stored, against
                   the default Euler path f16_rollout, 10,000 steps of 1 ms, every 10th stored, at the same three sizes.
  (iii) scored     a 1 s horizon under ten command rows: f16_rollout_cost_rk, 100 RK4 steps of 10 ms, against f16_rollout_cost,
                   1,000 Euler steps of 1 ms, at 4,096 lanes (64 x 64) and 65,536 lanes (256 x 256).  Both run the one-lane kernels
                   and RK4 does 0.4 x the evaluations: RK4 must take LESS time at both sizes -- asserted after the line is written.

The parent process never touches the GPU; the children run one after another, each under a time limit, and the first that fails
ends the run.  From the repository root on the GPU:
    python tools/gpu_time_rollout_rk4.py > profiles/rollout_rk4_time.jsonl"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ONE_LANE_FAMILY = {"F16_ROLLOUT_QUAD_MAXB": "0", "F16_ROLLOUT_4W_MAXB": "0"}
SIZES = (4096, 32768, 262144)


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Bench:
    def __init__(self, repeats):
        import torch
        from f16_mpc_oop_py_amd import lib
        assert torch.cuda.is_available(), "needs the MI355X"
        self.t, self.lib, self.L, self.repeats = torch, lib, lib.load(), repeats
        self.ctx = lib.Context(0)
        self.h = self.ctx.handle
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def states(self, B):
        import numpy as np
        from f16_mpc_oop_py_amd.workload import config2_states
        x0, u0 = config2_states(B, seed=B)
        return (self.t.as_tensor(np.ascontiguousarray(x0.T), device="cuda:0"), self.t.as_tensor(np.ascontiguousarray(u0.T), device="cuda:0"))

    def time(self, fns):
        """{name: median / min / max ms} of the alternating runs of fns = [(name, callable)]"""
        import numpy as np
        t = self.t
        for _, fn in fns:
            fn()
        t.cuda.synchronize()
        times = {name: [] for name, _ in fns}
        for _ in range(self.repeats):
            for name, fn in fns:
                e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                t.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        return {name: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for name, v in times.items()}

    def euler(self, x, u, traj, st, B, n, every, dt):
        self.lib.check(self.L.f16_rollout(self.h, vp(x), vp(u), vp(traj), vp(st), B, B, n, every, dt, 0.25, 1, 0, self.stream), self.L)

    def rk4(self, x, u, traj, st, B, n, every, dt):
        self.lib.check(self.L.f16_rollout_rk(self.h, vp(x), vp(u), vp(traj), vp(st), B, B, n, n, every, dt, 0.25, 1, self.lib.F16_INT_RK4, 0,
                                             self.stream), self.L)


def part_per_step(b):
    t = b.t
    assert all(os.environ.get(k) == v for k, v in ONE_LANE_FAMILY.items()), "per_step runs under F16_ROLLOUT_QUAD_MAXB=0 F16_ROLLOUT_4W_MAXB=0"
    out = dict(part="per_step", knobs=ONE_LANE_FAMILY, dt=0.001, repeats=b.repeats, timer="device events", sizes={})
    for B in SIZES:
        x0, u = b.states(B)
        x, st = x0.clone(), t.zeros(B, dtype=t.int32, device="cuda:0")
        res = {}
        for stored, (ne, nr) in (("none_stored", (400, 100)), ("every_step_stored", (100, 50))):
            traj = t.empty((ne, 18, B), dtype=t.float64, device="cuda:0") if stored == "every_step_stored" else None

            def euler():
                x.copy_(x0); st.zero_()
                b.euler(x, u, traj, st, B, ne, 1, 0.001)

            def rk4():
                x.copy_(x0); st.zero_()
                b.rk4(x, u, traj, st, B, nr, 1, 0.001)

            r = b.time([("euler_ms", euler), ("rk4_ms", rk4)])
            pe, pr = r["euler_ms"]["median"] / ne, r["rk4_ms"]["median"] / nr
            res[stored] = dict(r, euler_steps=ne, rk4_steps=nr, euler_us_per_step=1e3 * pe, rk4_us_per_step=1e3 * pr, rk4_over_euler_per_step=pr / pe)
            del traj
            t.cuda.empty_cache()
        out["sizes"][str(B)] = res
    print(json.dumps(out), flush=True)


def part_flight(b):
    t = b.t
    out = dict(part="flight", what="10 s of flight, 1,000 stored samples: RK4 1,000 steps of 10 ms against the default Euler path 10,000 steps of 1 ms",
               repeats=b.repeats, timer="device events", sizes={})
    for B in SIZES:
        x0, u = b.states(B)
        x, st = x0.clone(), t.zeros(B, dtype=t.int32, device="cuda:0")
        traj = t.empty((1000, 18, B), dtype=t.float64, device="cuda:0")
        keep = {}

        def euler():
            x.copy_(x0); st.zero_()
            b.euler(x, u, traj, st, B, 10000, 10, 0.001)
            keep["euler"] = (x.clone(), st.clone())

        def rk4():
            x.copy_(x0); st.zero_()
            b.rk4(x, u, traj, st, B, 1000, 1, 0.01)
            keep["rk4"] = (x.clone(), st.clone())

        r = b.time([("euler_1ms_ms", euler), ("rk4_10ms_ms", rk4)])
        (xe, se), (xr, sr) = keep["euler"], keep["rk4"]
        both = (se == 0) & (sr == 0) & t.isfinite(xe).all(0) & t.isfinite(xr).all(0)
        d = ((xe - xr).abs() / xe.abs().clamp(min=1.0))[:, both]
        out["sizes"][str(B)] = dict(r, rk4_over_euler=r["rk4_10ms_ms"]["median"] / r["euler_1ms_ms"]["median"],
                                    euler_kernel="k_rollout_q<1>" if B <= 4096 else ("k_rollout<128>" if B <= 32768 else "k_rollout_i<512>"),
                                    rk4_kernel=f"k_rollout<{64 if B <= 16384 else (128 if B <= 32768 else 256)}, STAGES = 4>",
                                    aircraft_unflagged_in_both=int(both.sum()), max_rel_diff_final_state=float(d.max()) if d.numel() else None,
                                    stored_trajectory_bytes=int(traj.numel() * 8))
        del traj, keep
        t.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def part_scored(b):
    import numpy as np
    t, lib, L = b.t, b.lib, b.L
    from f16_mpc_oop_py_amd import parameters as P
    out = dict(part="scored", what="1 s horizon, ten command rows: f16_rollout_cost_rk 100 RK4 steps of 10 ms against f16_rollout_cost 1,000 Euler steps of 1 ms",
               ideal_ratio=0.4, repeats=b.repeats, timer="device events", sizes={})
    w = lib.make_cost_weights()
    for B0, K in ((64, 64), (256, 256)):
        lanes, S = B0 * K, 10
        xi, u0 = b.states(B0)
        g = t.Generator(device="cuda:0")
        g.manual_seed(B0)
        scale = t.tensor([100.0, 0.5, 0.5, 0.5], dtype=t.float64, device="cuda:0")[None, :, None]
        rows = (u0[None].repeat(S, 1, K) + scale * (2 * t.rand((S, 4, lanes), generator=g, device="cuda:0", dtype=t.float64) - 1)).contiguous()
        xr = xi[P.mpc_x_idx].contiguous()
        ce, cr = t.empty(lanes, dtype=t.float64, device="cuda:0"), t.empty(lanes, dtype=t.float64, device="cuda:0")
        se, sr = t.zeros(lanes, dtype=t.int32, device="cuda:0"), t.zeros(lanes, dtype=t.int32, device="cuda:0")

        def euler():
            lib.check(L.f16_rollout_cost(b.h, vp(xi), B0, B0, vp(rows), vp(xr), None, ctypes.byref(w), vp(ce), None, None, vp(se), lanes, lanes,
                                         1000, 100, 1, 0.001, 0.25, 1, 0, b.stream), L)

        def rk4():
            lib.check(L.f16_rollout_cost_rk(b.h, vp(xi), B0, B0, vp(rows), vp(xr), None, ctypes.byref(w), vp(cr), None, None, vp(sr), lanes, lanes,
                                            100, 10, 1, 0.01, 0.25, 1, lib.F16_INT_RK4, 0, b.stream), L)

        r = b.time([("euler_1ms_ms", euler), ("rk4_10ms_ms", rk4)])
        both = (se == 0) & (sr == 0) & t.isfinite(ce) & t.isfinite(cr)
        # (the two costs are sums over 1,000 and over 100 states: compared per step of horizon, as a plausibility figure only)
        out["sizes"][f"{B0}x{K}"] = dict(r, lanes=lanes, rk4_over_euler=r["rk4_10ms_ms"]["median"] / r["euler_1ms_ms"]["median"],
                                         lanes_unflagged_in_both=int(both.sum()),
                                         median_cost_per_step_euler=float((ce[both] / 1000).median()) if both.any() else None,
                                         median_cost_per_step_rk4=float((cr[both] / 100).median()) if both.any() else None)
    print(json.dumps(out), flush=True)
    slow = [k for k, v in out["sizes"].items() if not v["rk4_over_euler"] < 1.0]
    assert not slow, f"RK4 at 10 ms must take less time than Euler at 1 ms over the same horizon: not at {slow}"


PARTS = {"per_step": part_per_step, "flight": part_flight, "scored": part_scored}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=list(PARTS), help="run one part in this process (what the parent starts)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if args.part:
        PARTS[args.part](Bench(args.repeats))
        return
    for part in PARTS:
        env = {k: v for k, v in os.environ.items() if k not in ("F16_ROLLOUT_QUAD_MAXB", "F16_ROLLOUT_4W_MAXB", "F16_DYN_BLOCK", "F16_ROLLOUT_I32")}
        if part == "per_step":
            env.update(ONE_LANE_FAMILY)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--repeats", str(args.repeats)], env=env, timeout=420)
        if p.returncode != 0:
            sys.exit(f"part {part} ended with status {p.returncode}: nothing more is started")


if __name__ == "__main__":
    main()
