"""Child process of tests/test_gpu_envelope.py: the launch rules of the rollouts read their knobs (F16_ROLLOUT_QUAD_MAXB,
F16_ROLLOUT_4W_MAXB, F16_DYN_BLOCK, F16_ROLLOUT_I32) once per process, so every routing runs in a process of its own.

    python envelope_child.py OUT.npz hifi|lofi [one_lane] [score]

runs every case of envelope_cases.CASES on that batch once and writes final states, status words, the per-step samples of the
40-step and 8-step cases and (LQR loop) the last action to OUT.npz; `one_lane` repeats them under F16_FLAG_ONE_LANE (keys "ol/..."),
`score` adds score_schedules on the lattice states (keys "score/...")."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def run_case(name, extra_flags, out, prefix):
    import torch
    import envelope_cases as ec
    from f16_mpc_oop_py_amd import F16Batch, lib as L
    c = ec.CASES[name]
    b, u, rows, K, dem = ec.case_inputs(name)
    flags = extra_flags | (L.F16_FLAG_NO_ENVELOPE if c["noenv"] else 0)
    env = F16Batch(b.x, u, fi_flag=b.fi, xcg=ec.XCG, dt=c["dt"], flags=flags, device="cuda:0")
    T = c["T"]
    every = 1 if T <= 40 else T                        # a sample at every step; the 100-step case keeps the final state only
    if c["kind"] == "sched":
        tr = env.rollout_schedule(rows, hold=ec.SCHED_HOLD, nsteps=T, traj_every=every)
    elif c["kind"] == "lqr":
        Kb = np.ascontiguousarray(np.broadcast_to(K, (b.B, 3, 9)))
        tr = env.rollout_LQR(T, dem[:, 0], dem[:, 1], dem[:, 2], K=Kb, traj_every=every)
        out[prefix + name + "/u"] = env.u_values.cpu().numpy()
    else:
        tr = env.rollout(T, traj_every=every)
    torch.cuda.synchronize()
    out[prefix + name + "/traj"] = tr.permute(0, 2, 1).cpu().numpy()          # [n, B, 18]
    out[prefix + name + "/x"] = env.x_values.cpu().numpy()
    out[prefix + name + "/st"] = env.status.cpu().numpy()


def run_score(which, out):
    import envelope_cases as ec
    from f16_mpc_oop_py_amd import F16Batch
    b, u, rows, _, _ = ec.case_inputs(which + "_sched40")
    w = ec.score_weights()
    env = F16Batch(b.x, u, fi_flag=b.fi, xcg=ec.XCG, device="cuda:0")
    cost, fin, tr = env.score_schedules(rows[:, None], hold=ec.SCHED_HOLD, nsteps=40, q=list(w.q), qf=list(w.qf), r=list(w.r),
                                        penalty=w.pen, traj_every=1, return_final=True)
    out["score/cost"] = cost.reshape(-1).cpu().numpy()
    out["score/x"] = fin.reshape(18, -1).t().cpu().numpy()
    out["score/traj"] = tr.reshape(40, 18, -1).permute(0, 2, 1).cpu().numpy()
    out["score/st"] = env.last_score_status.reshape(-1).cpu().numpy()


def main():
    import envelope_cases as ec
    from f16_mpc_oop_py_amd import lib as L
    path, which, opts = sys.argv[1], sys.argv[2], sys.argv[3:]
    out = {}
    names = [n for n, c in ec.CASES.items() if c["batch"] == which]
    for n in names:
        run_case(n, 0, out, "")
    if "one_lane" in opts:
        for n in names:
            run_case(n, L.F16_FLAG_ONE_LANE, out, "ol/")
    if "score" in opts:
        run_score(which, out)
    knobs = ("F16_ROLLOUT_QUAD_MAXB", "F16_ROLLOUT_4W_MAXB", "F16_DYN_BLOCK", "F16_ROLLOUT_I32")
    out["knobs"] = np.array([os.environ.get(k, "") for k in knobs])
    np.savez(path, **out)
    print("ok", len(out))


if __name__ == "__main__":
    main()
