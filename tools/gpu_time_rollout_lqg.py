"""GPU timing of the output-feedback loop (f16_rollout_lqg_wind) against the loop it extends (f16_rollout_lqr_wind), steady wind, no
samples stored: 1,000 steps of 1 ms at B = 4,096 and 65,536, hifi, both methods.  Variants:
    lqr_parent   f16_rollout_lqr_wind of the PARENT commit's library (built without a GPU by tools/gpu_time_rollout_wind.py
                 --build-parent REV, loaded through F16HIP_SO)
    lqr          f16_rollout_lqr_wind of this build: the same instructions (tools/rollout_lqg_resources.py), so its median must lie
                 inside lqr_parent's min .. max (asserted after the lines are written)
    lqg_all      f16_rollout_lqg_wind, all nine channels sensed (three Philox calls per step), the gain of kalman_reference
    lqg_ens      f16_rollout_lqg_wind_ens on the inputs of lqg_all: one group, one sample (the last step), no sample arrays
    lqg_all_parent, lqg_ens_parent    the same two calls of the parent's library: held against them like lqr against lqr_parent
    lqg_rates    rates only, 0x70 (one call), a fixed small gain (the design is ill-conditioned and not the subject here)
    lqg_pass     pass-through on 0x7f (two calls), Lf = I on the sensed channels
Protocol of tools/gpu_time_rollout_wind.py: a process per run (one warm-up call, one device-event timing per method around the library
call alone), the variants alternating, `--repeats` rounds; medians with min .. max.  The parent process never touches the GPU; the
children run one after another, each under a time limit, and the first that fails ends the run (gpu_time_rollout_wind.py: alternate).  --variants A B ... times a subset.  From the repository root:
    python tools/gpu_time_rollout_wind.py --build-parent HEAD~1         (no GPU needed; writes _exp/parent/libf16hip.so)
    python tools/gpu_time_rollout_lqg.py > profiles/rollout_lqg_time.jsonl     (on the GPU)
The committed profiles/rollout_lqg_time.jsonl was taken with --repeats 5 (each line says so); the default is 15."""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from gpu_time_rollout_wind import DT, NSTEPS, ONE_LANE_FAMILY, SIZES, alternate, timed_methods  # noqa: E402

VARIANTS = ("lqr_parent", "lqr", "lqg_all_parent", "lqg_all", "lqg_rates", "lqg_pass", "lqg_ens_parent", "lqg_ens")
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
    variant = variant[:-len("_parent")] if variant.endswith("_parent") else variant      # (the library is chosen by the environment)
    lqg, ens = variant.startswith("lqg"), variant == "lqg_ens"
    if lqg:
        from f16_mpc_oop_py_amd.observer import kalman_reference, pack_models
        sensed = {"lqg_all": 0x1ff, "lqg_ens": 0x1ff, "lqg_rates": 0x70, "lqg_pass": 0x7f}[variant]
        sigma = np.deg2rad(np.array([0.1, 0.1, 0.1, 0.1, 0.5, 0.5, 0.5, 0.1, 0.1]))
        if variant in ("lqg_all", "lqg_ens"):
            Lf = kalman_reference(Ad, np.full(9, 1e-8), sigma ** 2, sensed)[1]
        else:
            Lf = np.diag([(0.05 if variant == "lqg_rates" else 1.0) * ((sensed >> k) & 1) for k in range(9)])
        # (one model for the batch, mgroup = 0, linearised at the golden trim and set around the first aircraft's start: what the
        # estimate is worth does not change the work of a step; how many aircraft stay unflagged, and so keep stepping, is recorded)
        models = dev(pack_models(Ad[None], Bd[None], Lf[None], x0h[:1, MPC_IDX], x0h[:1, 13:16]))
        xhat0 = x0[MPC_IDX].clone().contiguous()
        xhat = xhat0.clone()
        hs = (ctypes.c_double * 9)(*sigma)
    if ens:
        e, group = lib.Ens(), (B + 63) // 64 * 64
        keep = [torch.zeros(L.f16_ens_work_doubles(B, 1), dtype=torch.float64, device="cuda:0"), torch.zeros((1, 1), dtype=torch.int32, device="cuda:0")]
        keep += [torch.zeros((1, 18, 1), dtype=torch.float64, device="cuda:0") for _ in range(4)]
        e.group, e.ldg = group, 1
        e.work, e.count, e.mean, e.m2, e.min, e.max = (t.data_ptr() for t in keep)

    def reset():
        x.copy_(x0); st.zero_()
        if lqg:
            xhat.copy_(xhat0)

    def call(method):
        if ens:
            rc = L.f16_rollout_lqg_wind_ens(ctx.handle, vp(x), vp(u0), vp(Kd), vp(dem), ctypes.byref(air), vp(models), 0, sensed, ctypes.cast(hs, ctypes.c_void_p),
                                            7, 0, vp(xhat), None, None, ctypes.byref(e), None, vp(st), B, B, NSTEPS, NSTEPS, NSTEPS, DT, 0.25, 1, method, 0,
                                            stream)
        elif lqg:
            rc = L.f16_rollout_lqg_wind(ctx.handle, vp(x), vp(u0), vp(Kd), vp(dem), ctypes.byref(air), vp(models), 0, sensed, ctypes.cast(hs, ctypes.c_void_p),
                                        7, 0, vp(xhat), None, None, None, vp(st), B, B, NSTEPS, NSTEPS, 1, DT, 0.25, 1, method, 0, stream)
        else:
            rc = L.f16_rollout_lqr_wind(ctx.handle, vp(x), vp(u0), vp(Kd), vp(dem), ctypes.byref(air), None, None, vp(st), B, B, NSTEPS, NSTEPS, 1, DT,
                                        0.25, 1, method, 0, stream)
        lib.check(rc, L)

    print(json.dumps(timed_methods(variant, B, reset, call, st)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", nargs=2, metavar=("VARIANT", "B"), help="one run in this process (what the parent starts)")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--variants", nargs="+", default=list(VARIANTS), choices=VARIANTS)
    args = ap.parse_args()
    if args.run:
        return run(args.run[0], int(args.run[1]))
    def extra(B, m, stats, runs):
        over = {v: stats[v]["median"] / stats["lqr"]["median"] for v in args.variants if "lqr" in stats and v.startswith("lqg") and not v.endswith("_parent")}
        return dict(unflagged={v: int(min(r[m + "_unflagged"] for r in rs)) for v, rs in runs.items()}, over_sibling=over)
    alternate(__file__, args.variants, SIZES, args.repeats, ONE_LANE_FAMILY, extra)


if __name__ == "__main__":
    main()
