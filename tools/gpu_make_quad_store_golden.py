"""Fixture G21q (the number G21 is the moving-air fixture's; tests/golden/g21_quad_store_wave_every1.npz, g21_quad_store_wave_every7.npz): what the four instantiations of the quad
rollout kernel k_rollout_q<1,*> return and STORE -- final state, status word, last action and the samples at three sample
periods -- kept so that a kernel whose samples are stored by another wave can be checked against it bit
for bit (tests/test_gpu_quad_store_wave.py, which takes the batch, the launch sequence and the sample bookkeeping from this file).
The batch is that of fixture G17 (tools/gpu_make_quad_variants_golden.py: its batch(), schedules() and gains() are used here),
B = 48, re-arranged so that the first workgroup (aircraft 0..15) can stay inside its table cells:
  0, 1   leave the envelope in mid-run (altitude, airspeed): frozen from then on, the samples repeat
  2, 3   frozen at launch          4  psi = NaN
  7      G17's aircraft 25, whose alpha leaves its 5-degree cell in mid-run (the step is found here and recorded: `cross`)
  20     G17's aircraft 5, alpha = NaN: an axis value that is in no cell, every step a full lookup for its workgroup
  21     elevator and its command at +25 degrees, the last node of the elevator axis (v == x1 of the last cell), held there
T = 84 steps (the entry points take a launch whose length is a multiple of the sample period only: 84 = 3 * 28 = 7 * 12).  Kept per
variant: final state, status, last action; every sample of a launch with traj_every = 1 for aircraft 0..16 (`_every1.npz`); the 12
samples of a launch with traj_every = 7 for all 48 (`_every7.npz`).
The launches go through F16Batch with its sample buffer replaced by one that is longer than the launch needs and filled with a
sentinel (run()): the rows behind the last sample must come back untouched.
Run on the GPU box with the library whose results are to be recorded (the parent commit's):
    F16HIP_SO=<parent build>/libf16hip.so python tools/gpu_make_quad_store_golden.py OUT_PREFIX
Before anything is recorded the restatement on the CPU (oracle/) is asked whether the placed aircraft do what they are there for."""
import importlib.util
import os
import sys
sys.path.insert(0, ".")
import numpy as np

_spec = importlib.util.spec_from_file_location("gpu_make_quad_variants_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_make_quad_variants_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

B_FIX, T_FIX, KEEP, PAD = 48, 84, 17, 2
SENTINEL = -1.2345678e300
CROSSER, NAN_AXIS, LAST_NODE = 7, 20, 21


def batch(B=B_FIX):
    """the re-arranged batch -> x0 [B, 18], u0 [B, 4], the same without the hand-placed values (the LQR gains: all finite)"""
    x0, u0, base = G.batch(B_FIX)
    for a, b in ((5, NAN_AXIS), (CROSSER, 25)):
        for arr in (x0, u0, base):
            arr[[a, b]] = arr[[b, a]]
    x0[LAST_NODE, 13] = 25.0; u0[LAST_NODE, 1] = 25.0
    return x0[:B].copy(), u0[:B].copy(), base[:B].copy()


def alpha_cell(tr):
    """the 5-degree cell of alpha (ALPHA1: -20, -15, ..., 90 degrees) in samples [n, 18, B]"""
    return np.floor((tr[:, 7] * (180.0 / np.pi) + 20.0) / 5.0)


def crossing_steps(tr1, aircraft):
    """the steps (1-based: behind that many steps the state is in another cell) at which alpha of `aircraft` changes its cell, from
    every-step samples [n, 18, B]"""
    c = alpha_cell(tr1)[:, aircraft]
    return np.flatnonzero(c[1:] != c[:-1]) + 2


def check_on_the_restatement(x0, u0):
    from oracle import mpc_oracle as mo
    x, tr, st = mo.COracle().rollout(x0, u0, T_FIX)              # tr[k] = the state after step k + 1, [T, B, 18]
    tr = tr.transpose(0, 2, 1)
    frozen = G.settle_step(tr)
    assert all(st[a] & G.ST_ENVELOPE and 10 < frozen[a] < T_FIX - 10 for a in (0, 1)), f"aircraft 0, 1 must freeze in mid-run: {st[:2]}, {frozen[:2]}"
    c = crossing_steps(tr, CROSSER)
    assert len(c) and 5 < c[0] < T_FIX - 5 and st[CROSSER] == 0, f"aircraft {CROSSER} must leave its alpha cell in mid-run and stay live: {c}"
    first = min([int(crossing_steps(tr, a)[0]) for a in range(16) if a not in (CROSSER, 5) and len(crossing_steps(tr, a))] + [T_FIX])
    assert c[0] < first, f"aircraft {CROSSER} is the first of its workgroup to change its alpha cell: {c[0]}, another behind step {first}"
    assert np.isnan(x[NAN_AXIS, 7]) and (tr[:, 13, LAST_NODE] == 25.0).all(), "NaN alpha; the elevator stays on its last node"
    print("restatement: aircraft 0, 1 frozen from samples", frozen[:2], " alpha crossing of aircraft", CROSSER, "behind step", c)
    return int(c[0])


def run(variant, K, cols=slice(None), parts=(T_FIX,), every=1, flags=0):
    """`variant` on the aircraft `cols` of the batch (their states, commands, schedules and rows of K [48, 3, 9]) as len(parts)
    launches in a row, every launch into a sample buffer of its own that is PAD rows longer than it needs and filled with SENTINEL
    (every = None: no buffer) -> final x [B, 18], status [B], u [B, 4], and per launch (steps done before it, its steps, its whole
    buffer [n // every + PAD, 18, B] or None)"""
    import torch
    from f16_mpc_oop_py_amd import F16Batch
    x0, u0, _ = batch()
    act, dem = G.schedules(B_FIX, u0)                            # (for the whole batch: an aircraft's rows do not depend on `cols`)
    x0, u0, act, dem = x0[cols], u0[cols], np.ascontiguousarray(act[:, cols]), np.ascontiguousarray(dem[:, :, cols])
    B = x0.shape[0]
    env = F16Batch(x0, u0, device="cuda:0", flags=flags)
    Kt = torch.as_tensor(np.ascontiguousarray(K[cols]), device="cuda:0")
    launches = []

    def samples(nsteps, traj_every, rows=18, lanes=None):      # in place of F16Batch._samples: PAD rows more, all SENTINEL
        if not traj_every:
            launches[-1][2] = None
            return None
        buf = torch.full((nsteps // int(traj_every) + PAD, rows, B), SENTINEL, dtype=torch.float64, device="cuda:0")
        launches[-1][2] = buf
        return buf
    env._samples = samples
    t = 0
    for n in parts:
        end = t + n
        while t < end:
            # a schedule counts its rows from the launch: a part that starts inside a held row first runs out that row in a launch
            # of its own, then whole rows (tools/gpu_make_quad_variants_golden.py run())
            m = end - t
            if variant in ("sched", "lqr_sched") and t % G.HOLD:
                m = min(m, G.HOLD - t % G.HOLD)
            r = slice(t // G.HOLD, (t + m - 1) // G.HOLD + 1)
            launches.append([t, m, None])
            if variant == "plain":
                env.rollout(m, traj_every=every)
            elif variant == "lqr":
                env.rollout_LQR(m, 0.05, -0.02, 0.01, K=Kt, traj_every=every)
            elif variant == "sched":
                env.rollout_schedule(act[r], hold=G.HOLD, nsteps=m, traj_every=every)
            else:
                env.rollout_LQR(m, dem[0][r], dem[1][r], dem[2][r], K=Kt, hold=G.HOLD, traj_every=every)
            t += m
    out = [(t0, m, None if buf is None else buf.cpu().numpy()) for t0, m, buf in launches]
    return env.x_values.cpu().numpy(), env.status.cpu().numpy(), env.u_values.cpu().numpy(), out


def stored(launches, every):
    """the samples the launches stored -> (the step each stands behind, counted over all launches [n]; samples [n, 18, B]); asserts
    that every launch left the PAD rows behind its last sample untouched"""
    steps, rows = [], []
    for t0, m, buf in launches:
        k = m // every
        assert buf.shape[0] == k + PAD
        assert (buf[k:] == SENTINEL).all(), f"launch of {m} steps from step {t0}: a row behind its {k} samples was written"
        steps += [t0 + every * (j + 1) for j in range(k)]
        rows.append(buf[:k])
    return np.array(steps, dtype=np.int64), np.concatenate(rows)


def main(prefix):
    x0, u0, base = batch()
    cross = check_on_the_restatement(x0, u0)
    K = G.gains(base, u0)
    e1, e7 = {"K": K}, {}
    for v in G.VARIANTS:
        x, st, u, l1 = run(v, K, every=1)
        _, tr1 = stored(l1, 1)
        x7, st7, u7, l7 = run(v, K, every=7)
        s7, tr7 = stored(l7, 7)
        assert np.array_equal(G.bits(x7), G.bits(x)) and np.array_equal(st7, st) and np.array_equal(G.bits(tr7), G.bits(tr1[s7 - 1]))
        assert np.array_equal(G.bits(tr1[-1]), G.bits(x.T)), "the last sample is the state the launch leaves"
        c = crossing_steps(tr1, CROSSER)
        # (under the LQR law and the schedules the aircraft flies another path: its own first crossing is recorded, 0 = none in mid-run)
        cr = int(c[0]) if len(c) and 5 < c[0] < T_FIX - 5 else 0
        assert v != "plain" or cr == cross, f"alpha crossing of aircraft {CROSSER} behind step {c}, the restatement's {cross}"
        e1.update({f"{v}_x": x, f"{v}_status": st, f"{v}_u": u, f"{v}_traj": tr1[:, :, :KEEP], f"{v}_cross": np.int64(cr)})
        e7[f"{v}_traj7"] = tr7
        print(v, "status of aircraft 0..7, 20, 21:", st[:8], st[[NAN_AXIS, LAST_NODE]], " crossing behind step", c)
    for name, res in (("every1", e1), ("every7", e7)):
        out = f"{prefix}_{name}.npz"
        np.savez_compressed(out, **res)
        print(out, {k: a.shape for k, a in res.items()}, os.path.getsize(out), "bytes")
        assert os.path.getsize(out) < 1000000


if __name__ == "__main__":
    main(sys.argv[1])
