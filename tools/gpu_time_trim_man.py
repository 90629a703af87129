"""GPU timing of the trim in a manoeuvre (f16_trim_man_batch) beside the level trim (f16_trim_batch) on the same conditions: medians of
`--repeats` device-event timings of one call over 4,096 seeded flight conditions (h 5,000 .. 30,000 ft, V 450 .. 800 ft/s: the
conditions of tests/test_gpu_trim.py's fast-forward test), hifi, xcg 0.25, the reference start, --maxiter (default 50,000) per run.
  trim           f16_trim_batch: five unknowns, one run
  man_level_1/2  f16_trim_man_batch with gamma = turn rate = pull-up rate = 0, runs = 1 and 2 (six unknowns, the level condition)
  man_turn_1/2   f16_trim_man_batch in level turns of -6 .. 6 deg/s with gamma -2 .. 5 deg, runs = 1 and 2
Beside the times: the median and the largest cost and iteration count of each call, and how many conditions ended above 1e-20 and on
the cap.  A wavefront holds four conditions and ends with its slowest, so the times follow the slowest conditions, not the median.
Nothing is asserted.  Writes one JSON line to --out (default profiles/trim_man_time.jsonl) and prints it.
Run from the repository root on the GPU: python tools/gpu_time_trim_man.py"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from f16_mpc_oop_py_amd import lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def timed(fn, repeats):
    """median, min, max [ms] of `repeats` device-event timings of fn() (the first, untimed run warms up)"""
    ms = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms = ms[1:]
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=50000, help="the cap of every run (scipy's maxiter; the reference's 50,000)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trim_man_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    B, dev, xcg = args.B, "cuda:0", 0.25
    ctx = lib.Context(0)
    L, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(7)
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    hh, vv = dv(rng.uniform(5e3, 3e4, B)), dv(rng.uniform(450.0, 800.0, B))
    gam, psd = dv(np.deg2rad(rng.uniform(-2.0, 5.0, B))), dv(np.deg2rad(rng.uniform(-6.0, 6.0, B)))
    xt = torch.empty((18, B), dtype=torch.float64, device=dev)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    iters, nfev, st = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))

    def level():
        st.zero_()
        lib.check(L.f16_trim_batch(h, vp(hh), vp(vv), vp(xt), vp(cost), vp(iters), vp(nfev), vp(st), B, B, xcg, 1, 0, args.maxiter, None, None), L)

    def man(g, p, runs):
        def call():
            st.zero_()
            lib.check(L.f16_trim_man_batch(h, vp(hh), vp(vv), vp(g), vp(p), None, None, vp(xt), vp(cost), vp(iters), vp(nfev), vp(st), B, B, xcg,
                                           1, 0, args.maxiter, runs, None), L)
        return call

    rec = dict(tool="gpu_time_trim_man", B=B, repeats=args.repeats, xcg=xcg, fi="hifi", maxiter=args.maxiter, so=os.path.basename(lib.SO_PATH),
               ms={}, result={})
    for name, fn in (("trim", level), ("man_level_1", man(None, None, 1)), ("man_level_2", man(None, None, 2)),
                     ("man_turn_1", man(gam, psd, 1)), ("man_turn_2", man(gam, psd, 2))):
        rec["ms"][name] = timed(fn, args.repeats)
        c, it, s = cost.cpu().numpy(), iters.cpu().numpy(), st.cpu().numpy()
        rec["result"][name] = dict(cost_median=float(np.median(c)), cost_max=float(np.max(c)), above_1e_20=int((c > 1e-20).sum()),
                                   iters_median=float(np.median(it)), iters_max=int(it.max()),
                                   capped=int(((s & lib.F16_ST["QP_MAXITER"]) != 0).sum()))
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
