"""GPU timing of the wind rollouts (f16_rollout_wind) against the still-air call they extend (f16_rollout_rk), on the same kernel family
(one lane per aircraft: every run under F16_ROLLOUT_QUAD_MAXB=0 F16_ROLLOUT_4W_MAXB=0, which matters for the Euler method).

1,000 steps of 1 ms at B = 4,096 and 65,536, hifi, no samples stored, both methods.  Variants:
    rk_parent    f16_rollout_rk of the PARENT commit's library (built without a GPU by --build-parent, loaded through F16HIP_SO)
    rk           f16_rollout_rk of this build: the same code, so its median must lie inside rk_parent's min .. max (asserted after
                 the lines are written)
    wind_parent  f16_rollout_wind of the parent commit's library, steady wind only
    wind         f16_rollout_wind, steady wind only: held against wind_parent like rk against rk_parent
    gust_seq10   + a gust_seq at gust_hold = 10
    gust_gen10   + in-kernel gusts at gust_hold = 10
    gust_gen1    + in-kernel gusts at gust_hold = 1
Protocol: a process per run (one warm-up call, one device-event timing per method around the library call alone: the state is put
back before the first event), the variants alternating, `--repeats` rounds; medians with min .. max.  Fifteen rounds by default: with
five, the median of one sample of identical code falls outside the min .. max of another with probability 1 / 6 per point (the three
smallest, or the three largest, of the ten pooled values all come from the one sample: 2 x 5/10 x 4/9 x 3/8), one point in two
of four-point records; with fifteen it is 0.2 %, so a miss then means a difference.  The parent process never touches the GPU; the children run one after another, each under a time limit, and
the first that fails ends the run.  From the repository root:
    python tools/gpu_time_rollout_wind.py --build-parent HEAD~1          (no GPU needed; writes _exp/parent/libf16hip.so)
    python tools/gpu_time_rollout_wind.py > profiles/rollout_wind_time.jsonl      (on the GPU)
--variants A B ... times a subset (a line of a subset is appended to the file, not written over it)."""
import argparse
import ast
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PARENT_SO = os.path.join(REPO, "_exp", "parent", "libf16hip.so")
ONE_LANE_FAMILY = {"F16_ROLLOUT_QUAD_MAXB": "0", "F16_ROLLOUT_4W_MAXB": "0"}
VARIANTS = ("rk_parent", "rk", "wind_parent", "wind", "gust_seq10", "gust_gen10", "gust_gen1")
SIZES = (4096, 65536)
NSTEPS, DT = 1000, 0.001


def build_parent(rev):
    from f16_mpc_oop_py_amd import lib
    os.makedirs(os.path.dirname(PARENT_SO), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", REPO, "archive", rev, "f16_mpc_oop_py_amd/csrc", "include", "f16_mpc_oop_py_amd/lib.py"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        # (read, not imported: lib.py is a module of its package and does not import on its own)
        names = ast.literal_eval(re.search(r"^SOURCES = (\[.*\])$", open(os.path.join(tmp, "f16_mpc_oop_py_amd", "lib.py")).read(), re.M).group(1))
        srcs = [os.path.join(tmp, "f16_mpc_oop_py_amd", "csrc", s) for s in names]
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + lib.HIPCC_FLAGS + ["-o", PARENT_SO] + srcs, check=True)
    print(f"{PARENT_SO}: built from {rev}")


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def run(variant, B):
    """one process: per method one warm-up call and one timed call -> a JSON line"""
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
    air, keep = lib.Wind(), []
    variant = variant[:-len("_parent")] if variant.endswith("_parent") else variant      # (the library is chosen by the environment)
    if variant != "rk":
        keep.append(dev(rng.uniform(-20, 20, (3, B))))
        air.wind_ned = keep[-1].data_ptr()
    hold = 1 if variant == "gust_gen1" else 10
    if variant == "gust_seq10":
        keep.append(dev(rng.normal(0, 5, (NSTEPS // hold, 3, B))))
        air.gust_seq, air.gust_hold = keep[-1].data_ptr(), hold
    if variant.startswith("gust_gen"):
        a, b = gust_coefficients([5.0, 5.0, 3.0], [1750.0, 1750.0, 500.0], 600.0, hold * DT)
        keep += [dev(np.repeat(a[:, None], B, 1)), dev(np.repeat(b[:, None], B, 1)), torch.zeros((3, B), dtype=torch.float64, device="cuda:0")]
        air.ga, air.gb, air.gstate, air.gust_hold, air.seed = keep[-3].data_ptr(), keep[-2].data_ptr(), keep[-1].data_ptr(), hold, 7

    def reset():
        x.copy_(x0); st.zero_()

    def call(method):
        if variant == "rk":
            rc = L.f16_rollout_rk(ctx.handle, vp(x), vp(u), None, vp(st), B, B, NSTEPS, NSTEPS, 1, DT, 0.25, 1, method, 0, stream)
        else:
            rc = L.f16_rollout_wind(ctx.handle, vp(x), vp(u), ctypes.byref(air), None, vp(st), B, B, NSTEPS, NSTEPS, 1, DT, 0.25, 1, method, 0, stream)
        lib.check(rc, L)

    print(json.dumps(timed_methods(variant, B, reset, call, st)), flush=True)


def timed_methods(variant, B, reset, call, st):
    """per method one warm-up call and one call between device events, the state put back before each -> the JSON line of a run"""
    import torch
    from f16_mpc_oop_py_amd import lib
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
    return out


def alternate(script, variants, sizes, repeats, knobs, extra=lambda B, m, stats, runs: {}):
    """The protocol for the parent process of a timing tool: per batch size `repeats` rounds of one child process per variant
    (`script --run VARIANT B`; a *_parent variant under F16HIP_SO = the parent's library), one JSON line per (B, method) with the
    medians and min .. max, then the assertion that every variant with a *_parent twin has its median inside the twin's min .. max."""
    import numpy as np
    assert os.path.exists(PARENT_SO), f"{PARENT_SO} is missing: run tools/gpu_time_rollout_wind.py --build-parent REV first"
    base = {k: v for k, v in os.environ.items() if k not in ("F16_DYN_BLOCK", "F16_ROLLOUT_I32", "F16HIP_SO")}
    base.update(knobs)
    late = []
    for B in sizes:
        runs = {v: [] for v in variants}
        for _ in range(repeats):
            for v in variants:
                env = dict(base, F16HIP_SO=PARENT_SO) if v.endswith("_parent") else base
                p = subprocess.run([sys.executable, os.path.abspath(script), "--run", v, str(B)], env=env, capture_output=True, text=True, timeout=180)
                if p.returncode != 0:
                    sys.exit(f"run {v} at B = {B} ended with status {p.returncode}: nothing more is started\n{p.stderr[-2000:]}")
                runs[v].append(json.loads(p.stdout.strip().splitlines()[-1]))
        for m in ("euler", "rk4"):
            t = {v: [r[m + "_ms"] for r in rs] for v, rs in runs.items()}
            stats = {v: dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x))) for v, x in t.items()}
            print(json.dumps(dict(B=B, method=m, nsteps=NSTEPS, dt=DT, repeats=repeats, timer="device events, a process per run", knobs=knobs,
                                  ms=stats, **extra(B, m, stats, runs))), flush=True)
            late += [(B, m, v, stats[v]["median"], stats[v + "_parent"]) for v in variants
                     if v + "_parent" in stats and not stats[v + "_parent"]["min"] <= stats[v]["median"] <= stats[v + "_parent"]["max"]]
    assert not late, f"calls of this build whose median lies outside the min .. max of the parent's: {late}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-parent", metavar="REV")
    ap.add_argument("--run", nargs=2, metavar=("VARIANT", "B"), help="one run in this process (what the parent starts)")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--variants", nargs="+", default=list(VARIANTS), choices=VARIANTS)
    args = ap.parse_args()
    if args.build_parent:
        return build_parent(args.build_parent)
    if args.run:
        return run(args.run[0], int(args.run[1]))
    still = lambda stats: {v: stats[v]["median"] / stats["rk"]["median"] for v in args.variants if "rk" in stats and not v.startswith("rk") and not v.endswith("_parent")}
    alternate(__file__, args.variants, SIZES, args.repeats, ONE_LANE_FAMILY, lambda B, m, stats, runs: dict(over_still_air=still(stats)))


if __name__ == "__main__":
    main()
