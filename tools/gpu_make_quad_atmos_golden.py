"""Fixture G20 (tests/golden/g20_quad_atmosphere_cases.npz): what the four instantiations of the quad rollout kernel k_rollout_q<1,*>
return on the batch of fixture G17 (tools/gpu_make_quad_variants_golden.py: its batch(), schedules(), gains() and run() are used
here; B = 48, T = 200) with FIVE MORE aircraft placed by hand in the first workgroup, chosen for the atmosphere of wave 3 -- the part
of a step that k_rollout_q<1,*> evaluates half a step ahead from the altitude alone (tests/test_gpu_quad_atmos_ahead.py):
  6   x[2] = 34,990 ft, climbing (theta 0.45, alpha 0.05): crosses 35,000 ft, where the temperature stops falling (the `temp` select)
  7   x[2] = 99,995 ft, same attitude: leaves the envelope through the top of the altitude box
  8   x[2] = NaN
  9   x[6] = 0.005 ft/s: V <= 0.01, the flap model's own atmosphere call
  10  x[2] = 150,000 ft: frozen at launch; with F16_FLAG_NO_ENVELOPE it flies on, tfac < 0 and the log takes a negative argument
Every variant is recorded twice, with flags 0 and with F16_FLAG_NO_ENVELOPE.  Kept per recording: final state, status word, last
action, every 10th sample and per aircraft the step from which its every-step samples no longer change.  The samples under
F16_FLAG_NO_ENVELOPE are kept for the aircraft whose samples differ from the flags-0 recording (`<v>_ne_aircraft`); all others have
the bits of `<v>_traj` (file size).  Run on the GPU box with the library whose results are to be recorded (the parent commit's):
    F16HIP_SO=<parent build>/libf16hip.so python tools/gpu_make_quad_atmos_golden.py OUT.npz
Before anything is recorded the restatement on the CPU (oracle/) is asked whether the placed aircraft do what they are there for."""
import importlib.util
import os
import sys
sys.path.insert(0, ".")
import numpy as np

_spec = importlib.util.spec_from_file_location("gpu_make_quad_variants_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_make_quad_variants_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

EVERY = 10
NO_ENVELOPE = 2                    # F16_FLAG_NO_ENVELOPE (include/f16_hip.h; main() checks it against the header)
RECORDINGS = (("", 0), ("_ne", NO_ENVELOPE))


def batch(B):
    """G17's batch with aircraft 6..10 placed (B >= 11) -> x0 [B, 18], u0 [B, 4], the unplaced batch (LQR gains: all finite)"""
    x0, u0, base = G.batch(B)
    x0[6, 2] = 34990.0; x0[6, 4] = 0.45; x0[6, 7] = 0.05
    x0[7, 2] = 99995.0; x0[7, 4] = 0.45; x0[7, 7] = 0.05
    x0[8, 2] = np.nan
    x0[9, 6] = 0.005
    x0[10, 2] = 150000.0
    return x0, u0, base


def check_on_the_restatement(x0, u0):
    from oracle import mpc_oracle as mo
    x, tr, st = mo.COracle().rollout(x0, u0, G.T_FIX)           # tr[k] = the state after step k + 1
    h6, h7, v9 = tr[:, 6, 2], tr[:, 7, 2], tr[:, 9, 6]
    c6, c7 = int(np.argmax(h6 >= 35000)), int(np.argmax(h7 > 100000))
    assert x0[6, 2] < 35000 and (h6 >= 35000).any() and (h6[c6:] >= 35000).all() and st[6] == 0, "aircraft 6 must climb across 35,000 ft and stay live"
    assert x0[7, 2] < 100000 and (h7 > 100000).any() and st[7] == G.ST_ENVELOPE | 1 << (8 + 2), f"aircraft 7 must leave through the altitude: {st[7]}"
    assert 5 < c6 + 1 < 195 and 5 < c7 + 1 < 195, f"both crossings between steps 5 and 195: {c6 + 1}, {c7 + 1}"
    assert not np.isfinite(np.delete(x[8], [12, 13, 14, 15])).any(), "aircraft 8: every state but the four actuators' NaN"
    live9 = int(np.argmax((tr[1:, 9] == tr[:-1, 9]).all(axis=1))) + 1      # samples that still moved = steps it was live
    assert st[9] & G.ST_ENVELOPE and st[9] & 1 << (8 + 6) and live9 >= 3, f"aircraft 9 must fly three steps and leave through the airspeed: {st[9]}, {live9}"
    assert x0[9, 6] <= 0.01 and (v9[1:3] <= 0.01).all(), f"aircraft 9: V <= 0.01 at the start of steps 1, 3 and 4: {v9[:4]}"
    assert np.array_equal(tr[-1, 10], x0[10]) and st[10] == G.ST_ENVELOPE | 1 << (8 + 2), "aircraft 10 frozen at launch"
    print("restatement: aircraft 6 at 35,000 ft after step", c6 + 1, " aircraft 7 above 100,000 ft after step", c7 + 1,
          " aircraft 9 live for", live9, "steps, V", v9[:4], " status 6..10:", st[6:11])


def main(out):
    from f16_mpc_oop_py_amd import lib
    assert lib.F16_FLAG_NO_ENVELOPE == NO_ENVELOPE
    x0, u0, base = batch(G.B_FIX)
    check_on_the_restatement(x0, u0)
    K = G.gains(base, u0)
    res = {"K": K}
    for v in G.VARIANTS:
        for tag, flags in RECORDINGS:
            x, st, u, tr = G.run(v, x0, u0, K, every=EVERY, flags=flags)
            _, _, _, tr1 = G.run(v, x0, u0, K, every=1, flags=flags)
            res.update({f"{v}{tag}_x": x, f"{v}{tag}_status": st, f"{v}{tag}_u": u, f"{v}{tag}_settle": G.settle_step(tr1)})
            if not tag:
                res[f"{v}_traj"] = tr
            else:
                diff = np.flatnonzero((G.bits(tr) != G.bits(res[f"{v}_traj"])).any(axis=(0, 1)))
                res[f"{v}_ne_aircraft"], res[f"{v}_ne_traj"] = diff, tr[:, :, diff]
            print(v + tag, "status of aircraft 6..10:", st[6:11], " settle:", res[f"{v}{tag}_settle"][6:11])
    np.savez_compressed(out, **res)
    print({k: a.shape for k, a in res.items()}, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1000000


if __name__ == "__main__":
    main(sys.argv[1])
