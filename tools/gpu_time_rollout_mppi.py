"""GPU timing of the closed MPPI loop in its three forms, through F16Batch.rollout_MPPI (default flags):
  (a) fused          sampler="counter", fused=True: ONE launch, f16_rollout_mppi
  (b) host_counter   sampler="counter": the host loop over f16_mppi_sample -> f16_rollout_cost(_rk) -> f16_mppi_blend -> f16_rollout(_rk)
  (c) host_torch     sampler="torch": the host loop with torch.randn noise (rollout_MPPI's default)
Medians of `--repeats` device-event timings after a warm-up, the three sides alternating in one process.  Configuration: Runge-Kutta
steps of 10 ms, S = 10 rows, hold = 10, K = 256 samples, 20 control periods, at B0 = 16, 256 and 1,024 aircraft; the Euler twin (1 ms)
at B0 = 256.  One JSON line per configuration.  No ratio is promised.  Asserted, after the lines are written: at B0 = 256 (a) is not
slower than (b) -- both occupy one workgroup per CU there and (a) stages the tables once and launches once.  From the repository
root on the GPU:
    python tools/gpu_time_rollout_mppi.py            (writes profiles/rollout_mppi_time.jsonl)"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
S, HOLD, K, PERIODS = 10, 10, 256, 20
CONFIGS = [("rk4", 0.010, 16), ("rk4", 0.010, 256), ("rk4", 0.010, 1024), ("euler", 0.001, 256)]
SIDES = {"fused": dict(sampler="counter", fused=True), "host_counter": dict(sampler="counter"), "host_torch": dict(sampler="torch")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rollout_mppi_time.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from f16_mpc_oop_py_amd import F16Batch
    from f16_mpc_oop_py_amd.workload import config2_states
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = []
    for method, dt, B0 in CONFIGS:
        x0, u0 = config2_states(B0, seed=B0)
        env = F16Batch(x0, u0, device="cuda:0", dt=dt)
        xs, us = env._x.clone(), env._u.clone()
        info = {}

        def run(side):
            env._x.copy_(xs); env._u.copy_(us); env.status.zero_()
            _, info[side] = env.rollout_MPPI(PERIODS * HOLD, 0.0, 0.0, 0.0, S, HOLD, K, 0.5, 2.0, seed=1, method=method, return_info=True,
                                             u_ref=u0[:, 1:4], penalty=3.0, **SIDES[side])

        for side in SIDES:                                   # warm-up: kernels loaded, allocator pools filled
            run(side)
        torch.cuda.synchronize()
        times = {side: [] for side in SIDES}
        for _ in range(args.repeats):
            for side in SIDES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(side)
                e1.record()
                torch.cuda.synchronize()
                times[side].append(e0.elapsed_time(e1))
        r = {side + "_ms": dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for side, v in times.items()}
        ess = {side: float(info[side]["ess"].median()) for side in SIDES}
        same = bool((info["fused"]["min_cost"] - info["host_counter"]["min_cost"]).abs().max() <= 1e-9 * info["host_counter"]["min_cost"].abs().max())
        lines.append(dict(method=method, dt=dt, B0=B0, K=K, S=S, hold=HOLD, periods=PERIODS, lanes=K * B0, repeats=args.repeats, timer="device events",
                          **r, fused_over_host_counter=r["fused_ms"]["median"] / r["host_counter_ms"]["median"],
                          fused_over_host_torch=r["fused_ms"]["median"] / r["host_torch_ms"]["median"],
                          median_ess=ess, fused_min_cost_agrees_with_host_counter=same,
                          aircraft_flagged=int((env.status != 0).sum())))
        del env
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    at256 = [v for v in lines if v["B0"] == 256 and v["method"] == "rk4"][0]
    assert at256["fused_over_host_counter"] <= 1.0, f"the fused loop is slower than the host loop at B0 = 256: {at256['fused_over_host_counter']:.3f}"


if __name__ == "__main__":
    main()
