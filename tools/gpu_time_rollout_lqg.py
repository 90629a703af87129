"""GPU timing of the output-feedback loop (f16_rollout_lqg_wind) against the loop it extends (f16_rollout_lqr_wind), steady wind, no
samples stored: 1,000 steps of 1 ms at B = 4,096 and 65,536, hifi, both methods.  Variants:
    lqr_parent   f16_rollout_lqr_wind of the PARENT commit's library (built without a GPU by tools/gpu_time_rollout_wind.py
                 --build-parent REV, loaded through F16HIP_SO)
    lqr          f16_rollout_lqr_wind of this build: the same instructions (tools/rollout_lqg_resources.py), so its median must lie
                 inside lqr_parent's min .. max (asserted after the lines are written)
    lqg_all      f16_rollout_lqg_wind, all nine channels sensed (three Philox calls per step), the gain of kalman_reference
    lqg_rates    rates only, 0x70 (one call), a fixed small gain (the design is ill-conditioned and not the subject here)
    lqg_pass     pass-through on 0x7f (two calls), Lf = I on the sensed channels
Protocol of tools/gpu_time_rollout_wind.py: a process per run (one warm-up call, one device-event timing per method around the library
call alone), the variants alternating, `--repeats` rounds; medians with min .. max.  The parent process never touches the GPU; the
children run one after another, each under a time limit, and the first that fails ends the run.  From the repository root:
    python tools/gpu_time_rollout_wind.py --build-parent HEAD~1         (no GPU needed; writes _exp/parent/libf16hip.so)
    python tools/gpu_time_rollout_lqg.py > profiles/rollout_lqg_time.jsonl     (on the GPU)
The committed profiles/rollout_lqg_time.jsonl was taken with --repeats 5 (each line says so); the default is 15."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PARENT_SO = os.path.join(REPO, "_exp", "parent", "libf16hip.so")
ONE_LANE_FAMILY = {"F16_ROLLOUT_QUAD_MAXB": "0", "F16_ROLLOUT_4W_MAXB": "0"}
VARIANTS = ("lqr_parent", "lqr", "lqg_all", "lqg_rates", "lqg_pass")
SIZES = (4096, 65536)
NSTEPS, DT = 1000, 0.001
MPC_IDX = [3, 4, 7, 8, 9, 10, 11, 17, 16]


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def run(variant, B):
    """one process: per method one warm-up call and one timed call -> a JSON line"""
    import numpy as np
    import torch
    from f16_mpc_oop_py_amd import lib
    from f16_mpc_oop_py_amd.workload import config2_states
    assert torch.cuda.is_available(), "needs the MI355X"
    L = lib.load()
    ctx = lib.Context(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x0h, u0h = config2_states(B, seed=B)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
    x0, u0 = dev(x0h.T), dev(u0h.T)
    x, st = x0.clone(), torch.zeros(B, dtype=torch.int32, device="cuda:0")
    rng = np.random.default_rng(B)
    g = np.load(os.path.join(REPO, "tests", "golden", "g567_trim_lin_lqr.npz"))
    Ad, Bd, K = g["ssr_Ad_xcg25"], g["ssr_Bd_xcg25"], g["K_lqr_xcg25"]
    Kd, dem = dev(np.repeat(K.reshape(27, 1), B, 1)), torch.zeros((3, B), dtype=torch.float64, device="cuda:0")
    wind = dev(rng.uniform(-20, 20, (3, B)))
    air = lib.Wind()
    air.wind_ned = wind.data_ptr()
    lqg = variant.startswith("lqg")
    if lqg:
        from f16_mpc_oop_py_amd.observer import kalman_reference, pack_models
        sensed = {"lqg_all": 0x1ff, "lqg_rates": 0x70, "lqg_pass": 0x7f}[variant]
        sigma = np.deg2rad(np.array([0.1, 0.1, 0.1, 0.1, 0.5, 0.5, 0.5, 0.1, 0.1]))
        if variant == "lqg_all":
            Lf = kalman_reference(Ad, np.full(9, 1e-8), sigma ** 2, sensed)[1]
        else:
            Lf = np.diag([(0.05 if variant == "lqg_rates" else 1.0) * ((sensed >> k) & 1) for k in range(9)])
        # (one model for the batch, mgroup = 0, linearised at the golden trim and set around the first aircraft's start: what the
        # estimate is worth does not change the work of a step; how many aircraft stay unflagged, and so keep stepping, is recorded)
        models = dev(pack_models(Ad[None], Bd[None], Lf[None], x0h[:1, MPC_IDX], x0h[:1, 13:16]))
        xhat0 = x0[MPC_IDX].clone().contiguous()
        xhat = xhat0.clone()
        hs = (ctypes.c_double * 9)(*sigma)

    def reset():
        x.copy_(x0); st.zero_()
        if lqg:
            xhat.copy_(xhat0)

    def call(method):
        if lqg:
            rc = L.f16_rollout_lqg_wind(ctx.handle, vp(x), vp(u0), vp(Kd), vp(dem), ctypes.byref(air), vp(models), 0, sensed, ctypes.cast(hs, ctypes.c_void_p),
                                        7, 0, vp(xhat), None, None, None, vp(st), B, B, NSTEPS, NSTEPS, 1, DT, 0.25, 1, method, 0, stream)
        else:
            rc = L.f16_rollout_lqr_wind(ctx.handle, vp(x), vp(u0), vp(Kd), vp(dem), ctypes.byref(air), None, None, vp(st), B, B, NSTEPS, NSTEPS, 1, DT,
                                        0.25, 1, method, 0, stream)
        lib.check(rc, L)

    out = dict(variant=variant, B=B)
    for name, method in (("euler", lib.F16_INT_EULER), ("rk4", lib.F16_INT_RK4)):
        reset()
        call(method)
        reset()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(method)
        e1.record()
        torch.cuda.synchronize()
        out[name + "_ms"] = e0.elapsed_time(e1)
        out[name + "_unflagged"] = int((st == 0).sum())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", nargs=2, metavar=("VARIANT", "B"), help="one run in this process (what the parent starts)")
    ap.add_argument("--repeats", type=int, default=15)
    args = ap.parse_args()
    if args.run:
        return run(args.run[0], int(args.run[1]))
    import numpy as np
    assert os.path.exists(PARENT_SO), f"{PARENT_SO} is missing: run tools/gpu_time_rollout_wind.py --build-parent REV first"
    base = {k: v for k, v in os.environ.items() if k not in ("F16_DYN_BLOCK", "F16_ROLLOUT_I32", "F16HIP_SO")}
    base.update(ONE_LANE_FAMILY)
    late = []
    for B in SIZES:
        times = {v: dict(euler=[], rk4=[]) for v in VARIANTS}
        flying = {v: dict(euler=[], rk4=[]) for v in VARIANTS}
        for _ in range(args.repeats):
            for v in VARIANTS:
                env = dict(base, F16HIP_SO=PARENT_SO) if v == "lqr_parent" else base
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--run", v, str(B)], env=env, capture_output=True, text=True, timeout=180)
                if p.returncode != 0:
                    sys.exit(f"run {v} at B = {B} ended with status {p.returncode}: nothing more is started\n{p.stderr[-2000:]}")
                r = json.loads(p.stdout.strip().splitlines()[-1])
                for m in ("euler", "rk4"):
                    times[v][m].append(r[m + "_ms"])
                    flying[v][m].append(r[m + "_unflagged"])
        for m in ("euler", "rk4"):
            stats = {v: dict(median=float(np.median(t[m])), min=float(np.min(t[m])), max=float(np.max(t[m]))) for v, t in times.items()}
            ref = stats["lqr"]["median"]
            print(json.dumps(dict(B=B, method=m, nsteps=NSTEPS, dt=DT, repeats=args.repeats, timer="device events, a process per run", knobs=ONE_LANE_FAMILY,
                                  ms=stats, unflagged={v: int(min(f[m])) for v, f in flying.items()}, over_sibling={v: stats[v]["median"] / ref for v in VARIANTS[2:]})), flush=True)
            if not stats["lqr_parent"]["min"] <= ref <= stats["lqr_parent"]["max"]:
                late.append((B, m, ref, stats["lqr_parent"]))
    assert not late, f"the sibling of this build lies outside the parent's min .. max: {late}"


if __name__ == "__main__":
    main()
