"""Child process of tests/test_gpu_rollout_rk4.py: the launch rules read F16_DYN_BLOCK once per process, so every routing runs in a
process of its own.

    python rk4_child.py OUT.npz JOB [JOB ...]

JOBS: cases (every case of rk4_cases.CASES under F16_INT_RK4, a sample per step), one_lane (the same under F16_FLAG_ONE_LANE, keys
"ol/..."), ceiling (the first lattice case alone), forward, split, score, sizes, g10, nan -- see the tests that read them.  Arrays go
to OUT.npz as they come from the device; comparisons that would need large arrays (bit-for-bit equality of whole trajectories) are
made here and stored as flags."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
EULER, RK4 = 1, 4


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Dev:
    """raw calls into the library on device tensors"""

    def __init__(self):
        import torch
        from f16_mpc_oop_py_amd import lib
        self.t, self.lib = torch, lib
        self.L = lib.load()
        self.ctx = lib.Context(0)

    def soa(self, a):
        return self.t.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64).T), device="cuda:0")

    def seq(self, rows):
        return self.t.as_tensor(np.ascontiguousarray(np.asarray(rows, dtype=np.float64).transpose(0, 2, 1)), device="cuda:0")

    def check(self, rc):
        assert rc == 0, (rc, self.L.f16_last_error())

    def run(self, x0, rows, T, hold, every, dt, fi, flags=0, xcg=0.25, K=None, u0=None, status0=None, method=RK4, old=False):
        """one scheduled rollout: f16_rollout_rk / f16_rollout_lqr_rk with `method`, or (old) f16_rollout_sched / f16_rollout_lqr_sched
        -> dict(x [B, 18], traj [n, B, 18] or None, st [B], u [B, 4] or None) as numpy"""
        t, L = self.t, self.L
        B = len(x0)
        x, sq = self.soa(x0), self.seq(rows)
        st = t.zeros(B, dtype=t.int32, device="cuda:0") if status0 is None else t.as_tensor(status0, dtype=t.int32, device="cuda:0")
        traj = t.full((T // every, 18, B), float("nan"), dtype=t.float64, device="cuda:0") if every else None
        rule = () if old else (method,)
        uo = None
        if K is not None:
            Kd = self.soa(np.broadcast_to(np.asarray(K, dtype=np.float64).reshape(-1, 27), (B, 27)))
            u0d, uo = self.soa(u0), t.full((4, B), float("nan"), dtype=t.float64, device="cuda:0")
            f = L.f16_rollout_lqr_sched if old else L.f16_rollout_lqr_rk
            self.check(f(self.ctx.handle, p(x), p(u0d), p(Kd), p(sq), p(traj), p(uo), p(st), B, B, T, hold, every or 1, dt, xcg, fi, *rule,
                         flags, None))
        else:
            f = L.f16_rollout_sched if old else L.f16_rollout_rk
            self.check(f(self.ctx.handle, p(x), p(sq), p(traj), p(st), B, B, T, hold, every or 1, dt, xcg, fi, *rule, flags, None))
        t.cuda.synchronize()
        return dict(x=x.t().cpu().numpy(), traj=None if traj is None else traj.permute(0, 2, 1).cpu().numpy(), st=st.cpu().numpy(),
                    u=None if uo is None else uo.t().cpu().numpy())

    def score(self, x0, rows, xref, uref, w, T, hold, every, dt, fi, flags=0, xcg=0.25, want_end=True, method=RK4, old=False):
        """f16_rollout_cost_rk (old: f16_rollout_cost) on rows [S, K, B0, 4] -> dict(cost [B], x [B, 18] or None, traj, st)"""
        t, L = self.t, self.L
        S, K, B0 = rows.shape[:3]
        B = K * B0
        x, sq = self.soa(x0), self.seq(rows.reshape(S, B, 4))
        xr, ur = self.soa(xref), None if uref is None else self.soa(uref)
        cost = t.full((B,), float("nan"), dtype=t.float64, device="cuda:0")
        xe = t.full((18, B), float("nan"), dtype=t.float64, device="cuda:0") if want_end else None
        traj = t.full((T // every, 18, B), float("nan"), dtype=t.float64, device="cuda:0") if every else None
        st = t.full((B,), -1, dtype=t.int32, device="cuda:0")
        f, rule = (L.f16_rollout_cost, ()) if old else (L.f16_rollout_cost_rk, (method,))
        self.check(f(self.ctx.handle, p(x), B0, B0, p(sq), p(xr), p(ur), ctypes.byref(w), p(cost), p(xe), p(traj), p(st), B, B, T, hold,
                     every or 1, dt, xcg, fi, *rule, flags, None))
        t.cuda.synchronize()
        return dict(cost=cost.cpu().numpy(), x=None if xe is None else xe.t().cpu().numpy(),
                    traj=None if traj is None else traj.permute(0, 2, 1).cpu().numpy(), st=st.cpu().numpy())


def same(a, b):
    """bit for bit, NaNs included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def put(out, key, r):
    for k, v in r.items():
        if v is not None:
            out[f"{key}/{k}"] = v


# ------------------------------------------------------------------------------------------------ the jobs
def job_cases(dev, out, names=None, flags=0, prefix=""):
    import rk4_cases as rk
    for name in names or rk.CASES:
        c = rk.CASES[name]
        b, rows, hold, K, u0 = rk.case_inputs(name)
        put(out, prefix + name, dev.run(b.x, rows, c["T"], hold, 1, c["dt"], b.fi, flags=flags, K=K, u0=u0))


def job_forward(dev, out):
    """method = F16_INT_EULER against the calls it stands for, at B = 100 (the quad kernel); the Python surface against the raw call"""
    import rk4_cases as rk
    from f16_mpc_oop_py_amd import F16Batch
    b = rk.hifi_lattice()
    x0, u0 = b.x[:100], b.u[:100]
    rows = rk.schedule_rows(b, 40)[:, :100]
    dem = np.random.default_rng(3).uniform(-0.15, 0.15, (6, 100, 3))
    kw = dict(T=40, hold=7, every=1, dt=0.001, fi=1)
    a, o = dev.run(x0, rows, method=EULER, **kw), dev.run(x0, rows, old=True, **kw)
    out["forward/open"] = all(same(a[k], o[k]) for k in ("x", "traj", "st"))
    a, o = dev.run(x0, dem, K=rk.lqr_gain(), u0=u0, method=EULER, **kw), dev.run(x0, dem, K=rk.lqr_gain(), u0=u0, old=True, **kw)
    out["forward/lqr"] = all(same(a[k], o[k]) for k in ("x", "traj", "st", "u"))
    w = dev.lib.make_cost_weights(*[list(v) for v in (rk.score_weights().q, rk.score_weights().qf, rk.score_weights().r)], 2.0)
    r3 = np.stack([rows, rows * 0.9, rows * 1.1], 1)                             # [S, 3, 100, 4]
    xref = x0[:, [3, 4, 7, 8, 9, 10, 11, 17, 16]]
    a, o = dev.score(x0, r3, xref, None, w, method=EULER, **kw), dev.score(x0, r3, xref, None, w, old=True, **kw)
    out["forward/cost"] = all(same(a[k], o[k]) for k in ("cost", "x", "traj", "st"))
    # an RK4 run differs from the Euler one (the method argument is read), and by little at 1 ms
    r = dev.run(x0, rows, **kw)
    out["forward/rk4_differs"] = not same(r["x"], dev.run(x0, rows, old=True, **kw)["x"])
    # the Python surface: rollout_schedule(method="rk4") and rollout(method="rk4") are that call
    env = F16Batch(x0, u0, fi_flag=1, xcg=0.25, dt=0.001, device="cuda:0")
    tr = env.rollout_schedule(rows, hold=7, nsteps=40, traj_every=1, method="rk4")
    out["forward/python_schedule"] = same(tr.permute(0, 2, 1).cpu().numpy(), r["traj"]) and same(env.status.cpu().numpy(), r["st"])
    env = F16Batch(x0, u0, fi_flag=1, xcg=0.25, dt=0.01, device="cuda:0")
    tr = env.rollout(8, traj_every=1, method="rk4")
    r1 = dev.run(x0, u0[None], 8, 8, 1, 0.01, 1)
    out["forward/python_rollout"] = same(tr.permute(0, 2, 1).cpu().numpy(), r1["traj"]) and same(env.x_values.cpu().numpy(), r1["x"])


def job_split(dev, out):
    """rows with hold 7 over 40 steps: one call, the chain of one call per segment, a constant row given as S rows"""
    import rk4_cases as rk
    name = "hifi_sched40"
    c = rk.CASES[name]
    b, rows, hold, _, _ = rk.case_inputs(name)
    one = dev.run(b.x, rows, 40, hold, 1, c["dt"], 1)
    x, st, parts = b.x, None, []
    for s in range(len(rows)):
        n = min(hold, 40 - s * hold)
        r = dev.run(x, rows[s:s + 1], n, n, 1, c["dt"], 1, status0=st)
        x, st = r["x"], r["st"]
        parts.append(r["traj"])
    out["split/chain"] = same(np.concatenate(parts), one["traj"]) and same(x, one["x"]) and same(st, one["st"])
    # a split that is not at a row boundary: 40 = 17 + 23 steps cannot be given as two schedules with hold 7, so hold 1 rows
    r1 = np.repeat(rows, hold, 0)[:40]
    a = dev.run(b.x, r1[:17], 17, 1, 1, c["dt"], 1)
    bb = dev.run(a["x"], r1[17:], 23, 1, 1, c["dt"], 1, status0=a["st"])
    out["split/n_plus_m"] = same(np.concatenate((a["traj"], bb["traj"])), one["traj"]) and same(bb["st"], one["st"])
    const = np.repeat(rows[:1], len(rows), 0)
    out["split/constant_rows"] = all(same(dev.run(b.x, const, 40, hold, 1, c["dt"], 1)[k], dev.run(b.x, rows[:1], 40, 40, 1, c["dt"], 1)[k])
                                     for k in ("x", "traj", "st"))
    put(out, "split/one", one)


def job_score(dev, out):
    """the scored call against f16_rollout_rk on the K-fold replicated states, against its formula, with and without x_end / traj"""
    import rk4_cases as rk
    from test_gpu_rollout_cost import case_inputs
    w = rk.score_weights()
    cw = dev.lib.make_cost_weights(list(w.q), list(w.qf), list(w.r), w.pen)
    shapes = {"16x8": (16, 8, 0), "16x8_one_lane": (16, 8, dev.lib.F16_FLAG_ONE_LANE), "70x3": (70, 3, 0)}
    for key, (B0, K, flags) in shapes.items():
        T, hold, dt = 20, 7, 0.01
        x0, u0, rows, xref, uref = case_inputs(B0, K, 3)
        x0 = x0.copy()
        x0[1, 2] = 101000.0                                                      # one aircraft outside the box: frozen from the start
        x0[2, 6] = 899.99                                                        # ... and one that may leave it on the way
        full = dev.score(x0, rows, xref, uref, cw, T, hold, 1, dt, 1, flags=flags)
        rep = dev.run(np.tile(x0, (K, 1)), rows.reshape(len(rows), K * B0, 4), T, hold, 1, dt, 1, flags=flags)
        out[f"score/{key}/states_equal_rollout_rk"] = same(full["x"], rep["x"]) and same(full["traj"], rep["traj"]) and same(full["st"], rep["st"])
        bare = dev.score(x0, rows, xref, uref, cw, T, hold, 0, dt, 1, flags=flags, want_end=False)
        out[f"score/{key}/cost_same_bits_bare"] = same(full["cost"], bare["cost"]) and same(full["st"], bare["st"])
        put(out, f"score/{key}", full)
        out[f"score/{key}/x0"], out[f"score/{key}/rows"], out[f"score/{key}/xref"], out[f"score/{key}/uref"] = x0, rows, xref, uref


def job_sizes(dev, out):
    """F16_FLAG_ONE_LANE: aircraft i in a batch of 1, of 100 and of the whole lattice"""
    import rk4_cases as rk
    b = rk.hifi_lattice()
    OL = dev.lib.F16_FLAG_ONE_LANE
    K, dem = rk.lqr_gain(), rk.lqr_demands(b)
    whole = dev.run(b.x, b.u[None], 8, 8, 1, 0.01, 1, flags=OL)
    wl = dev.run(b.x, dem[None], 8, 8, 1, 0.01, 1, flags=OL, K=K, u0=b.u)
    ok = True
    for sel in (slice(0, 100), slice(37, 38), slice(b.B - 1, b.B), slice(1300, 1400)):
        r = dev.run(b.x[sel], b.u[None, sel], 8, 8, 1, 0.01, 1, flags=OL)
        ok &= same(r["traj"], whole["traj"][:, sel]) and same(r["st"], whole["st"][sel])
        r = dev.run(b.x[sel], dem[None, sel], 8, 8, 1, 0.01, 1, flags=OL, K=K, u0=b.u[sel])
        ok &= same(r["traj"], wl["traj"][:, sel]) and same(r["u"], wl["u"][sel])
    out["sizes/one_lane_same_bits"] = ok
    # and the scored variant steps through the same function: lane b of a scored launch of the whole lattice = the open loop
    cw = dev.lib.make_cost_weights()
    s = dev.score(b.x, b.u[None, None], b.x[:, [3, 4, 7, 8, 9, 10, 11, 17, 16]], None, cw, 8, 8, 1, 0.01, 1, flags=OL)
    out["sizes/scored_same_bits"] = same(s["traj"], whole["traj"]) and same(s["st"], whole["st"])
    # without the flag the default routing is another instruction sequence: it may differ (reported, not asserted)
    d = dev.run(b.x, b.u[None], 8, 8, 1, 0.01, 1)
    out["sizes/default_equals_one_lane"] = same(d["traj"], whole["traj"])


def job_g10(dev, out):
    """1,000 RK4 steps at 10 ms, every 10th stored, F16_FLAG_FIX_CLR; and f16_rollout_sched (Euler) on the same rows at 10 ms"""
    from conftest import g10_case, g10_command
    FIX = dev.lib.F16_FLAG_FIX_CLR
    for k in range(4):
        a, xcg, x0, trim_u, dis = g10_case(k)
        rows = np.array([[g10_command(trim_u, dis, j)] for j in range(100)])
        put(out, f"g10/rk4_{k}", dev.run(x0[None], rows, 1000, 10, 10, 0.01, 1, flags=FIX, xcg=xcg))
        put(out, f"g10/euler_{k}", dev.run(x0[None], rows, 1000, 10, 10, 0.01, 1, flags=FIX, xcg=xcg, old=True))


def nan_inputs():
    """B = 8: NaN in each of the four commands, a far-out-of-box command, an infinite one, an aircraft outside the box from the
    start and an ordinary one; the second row (from step 3 on) is ordinary for everyone but aircraft 7, whose commands turn NaN"""
    import rk4_cases as rk
    b = rk.hifi_lattice()
    x0 = b.x[b.edge["alpha_node"]:b.edge["alpha_node"] + 1].repeat(8, 0)
    u = x0[:, 12:16].copy()
    rows = np.stack([u, u])
    for k in range(4):
        rows[0, k, k] = np.nan
    rows[0, 4] = [1e30, -1e30, 1e30, -1e30]
    rows[0, 5, 1] = np.inf
    x0[6, 2] = -5.0                                                              # frozen from the start; its later row is never read
    rows[1, 6] = np.nan
    rows[1, 7] = np.nan
    return x0, rows


def job_nan(dev, out):
    x0, rows = nan_inputs()
    OL = dev.lib.F16_FLAG_ONE_LANE
    put(out, "nan/default", dev.run(x0, rows, 6, 3, 1, 0.01, 1))
    put(out, "nan/one_lane", dev.run(x0, rows, 6, 3, 1, 0.01, 1, flags=OL))


def main():
    import rk4_cases as rk
    path, jobs = sys.argv[1], sys.argv[2:]
    dev = Dev()
    out = {}
    for j in jobs:
        if j == "cases":
            job_cases(dev, out)
        elif j == "one_lane":
            job_cases(dev, out, flags=dev.lib.F16_FLAG_ONE_LANE, prefix="ol/")
        elif j == "ceiling":
            job_cases(dev, out, names=rk.LATTICE_CASES[:1])
        else:
            {"forward": job_forward, "split": job_split, "score": job_score, "sizes": job_sizes, "g10": job_g10, "nan": job_nan}[j](dev, out)
    out["knobs"] = np.array([os.environ.get(k, "") for k in ("F16_ROLLOUT_QUAD_MAXB", "F16_ROLLOUT_4W_MAXB", "F16_DYN_BLOCK", "F16_ROLLOUT_I32")])
    np.savez(path, **out)
    print("ok", len(out))


if __name__ == "__main__":
    main()
