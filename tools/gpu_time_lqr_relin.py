"""GPU timing of the per-step re-linearised LQR loop (test_env.py:625-687 `test_LQR_dynamic_nl`): the one-launch loop
f16_rollout_lqr_relin against the host chain it fuses, per step
    f16_linearise_batch -> f16_c2d_batch -> f16_lqr_batch_w -> action (torch) -> f16_rollout(1, F16_FLAG_ONE_LANE),
in the same process, alternating, `--repeats` timed runs of each per batch size (config-2 flight conditions, xcg 0.25, Q = I,
R = 1e4 I, x_ref = the initial x9).  Prints ONE JSON line: per B the ms per step (median, min, max over the repeats) and
aircraft-steps/s of both loops, and the largest fused-vs-host difference of the final states (relative, max(1, |x|)) over the
aircraft that neither loop froze and that stayed finite, and over those of them whose DARE converged at every step (no
F16_ST_QP_MAXITER).  Run from the repository root on the GPU: python tools/gpu_time_lqr_relin.py"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from f16_mpc_oop_py_amd import F16Batch, lib
from f16_mpc_oop_py_amd.workload import config2_states

IDX9 = [3, 4, 7, 8, 9, 10, 11, 17, 16]


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,8192")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    T, xcg, dev = args.steps, 0.25, "cuda:0"
    w = lib.make_weights(Q=np.eye(9), R=np.eye(3) * 1e4)
    out = dict(tool="gpu_time_lqr_relin", steps=T, repeats=args.repeats, xcg=xcg, law="test_LQR_dynamic_nl (Q = I, R = 1e4 I)",
               so=os.path.basename(lib.SO_PATH), sizes={})
    for B in (int(s) for s in args.sizes.split(",")):
        x0, u0 = config2_states(B)
        env = F16Batch(x0, u0, xcg=xcg, device=dev)
        L, h, stream = env.lib, env.ctx.handle, env._stream
        xr = torch.as_tensor(np.ascontiguousarray(x0[:, IDX9].T), device=dev)
        bufs = {n: torch.empty((r, B), dtype=torch.float64, device=dev) for n, r in
                (("Ac", 81), ("Bc", 27), ("Cc", 81), ("Ad", 81), ("Bd", 27), ("K", 27))}
        xh = torch.empty((18, B), dtype=torch.float64, device=dev)
        uh = torch.empty((4, B), dtype=torch.float64, device=dev)
        sth = torch.zeros(B, dtype=torch.int32, device=dev)

        def fused():
            env.reset()
            lib.check(L.f16_rollout_lqr_relin(h, vp(env._x), vp(env._u), vp(xr), None, ctypes.byref(w), None, None, None,
                                              vp(env.status), B, B, T, T, 0x1FF, 1e-5, env.dt, xcg, 1, 0, stream), L)

        def host():
            xh.copy_(env._x_init); uh.copy_(env._u_init); sth.zero_()
            b = bufs
            for _ in range(T):
                lib.check(L.f16_linearise_batch(h, vp(xh), vp(uh), vp(b["Ac"]), vp(b["Bc"]), vp(b["Cc"]), None, B, B, 1e-5, xcg, 1, 0,
                                                stream), L)
                lib.check(L.f16_c2d_batch(h, vp(b["Ac"]), vp(b["Bc"]), vp(b["Ad"]), vp(b["Bd"]), B, B, env.dt, stream), L)
                lib.check(L.f16_lqr_batch_w(h, vp(b["Ad"]), vp(b["Bd"]), vp(b["Cc"]), ctypes.byref(w), vp(b["K"]), None, None, B, B,
                                            stream), L)
                e = xh[IDX9] - xr                                                   # K = -dlqr: cmd = K (x9 - x_ref)
                uh[1:4] = (b["K"].view(3, 9, B) * e.unsqueeze(0)).sum(1)
                lib.check(L.f16_rollout(h, vp(xh), vp(uh), None, vp(sth), B, B, 1, 1, env.dt, xcg, 1, lib.F16_FLAG_ONE_LANE,
                                        stream), L)

        fused(); host(); torch.cuda.synchronize()                                  # warm-up (code objects, allocator)
        tf, th = [], []
        for _ in range(args.repeats):
            for fn, acc in ((fused, tf), (host, th)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3 / T)
        live = (((env.status | sth) & (16 | 32)) == 0) & torch.isfinite(env._x).all(0) & torch.isfinite(xh).all(0)
        xf, xhost = env._x[:, live].cpu().numpy(), xh[:, live].cpu().numpy()
        d = (np.abs(xf - xhost) / np.maximum(1.0, np.abs(xhost))).max(axis=0) if xf.size else np.zeros(1)
        conv = ((env.status[live] & 64) == 0).cpu().numpy()
        stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
        out["sizes"][str(B)] = dict(
            fused_ms_per_step=stat(tf), host_ms_per_step=stat(th),
            fused_aircraft_steps_per_s=B / (np.median(tf) * 1e-3), host_aircraft_steps_per_s=B / (np.median(th) * 1e-3),
            speedup_median=float(np.median(th) / np.median(tf)), aircraft_compared=int(live.sum()),
            max_rel_state_diff=float(d.max()), max_rel_state_diff_dare_converged=float(d[conv].max()) if conv.any() else None,
            frozen_fused=int((env.status & 16).ne(0).sum()), nonfinite_fused=int((env.status & 32).ne(0).sum()),
            dare_maxiter_fused=int((env.status & 64).ne(0).sum()))
        del env
    print(json.dumps(out))


if __name__ == "__main__":
    main()
