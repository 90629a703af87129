"""Fixture G21 (tests/golden/g21_air_rollout_bits.json): SHA-256 digests of everything the six rollouts in moving air write, on the
cases of tests/test_gpu_air_rollout_bits.py (its cases() and Flight are used here; what they are is said there).  Before anything is
recorded the restatement on the CPU (oracle/) is asked whether the placed aircraft leaves the envelope inside the flight.  Run on the
GPU with the library whose results are to be recorded (the parent commit's):
    F16HIP_SO=_exp/parent/libf16hip.so python tools/gpu_make_air_rollout_golden.py tests/golden/g21_air_rollout_bits.json"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
from test_gpu_air_rollout_bits import GHOLD, GROUP, HOLD, LEAVING, NSTEPS, OUTSIDE, SIZES, DT, Flight, batch, cases  # noqa: E402


def leaving_step(x0, u0):
    """the step of the restatement (Euler, still air) after which the placed aircraft is above 100,000 ft: frozen from the next on"""
    from oracle import mpc_oracle as mo
    _, tr, st = mo.COracle().rollout(x0[:8], u0[:8], NSTEPS, dt=DT)
    h = tr[:, LEAVING, 2]
    k = int(np.argmax(h > 100000.0)) + 1
    assert x0[LEAVING, 2] < 100000.0 and (h > 100000.0).any() and 2 <= k <= NSTEPS - 2, f"aircraft {LEAVING} must leave inside the 12 steps: {h}"
    assert st[LEAVING] != 0 and st[OUTSIDE] != 0 and np.array_equal(tr[-1, OUTSIDE], x0[OUTSIDE]), (st[LEAVING], st[OUTSIDE])
    assert np.array_equal(tr[-1, LEAVING], tr[k - 1, LEAVING]) and not np.array_equal(tr[k - 1, LEAVING], tr[k - 2, LEAVING]), "frozen from step k + 1 on"
    return k


def main(out):
    x0, u0 = batch(SIZES[0])
    meta = dict(nsteps=NSTEPS, hold=HOLD, gust_hold=GHOLD, dt=DT, group=GROUP, outside=OUTSIDE, leaving=LEAVING, leaves_after_step=leaving_step(x0, u0))
    print("restatement: aircraft", LEAVING, "is above 100,000 ft after step", meta["leaves_after_step"])
    digests, apart = {}, 0
    for B in SIZES:
        f = Flight(B)
        for cid, *c in cases(B):
            digests[cid] = d = f.case(*c)
            apart += "b5_x" in d and d["b5_x"] != d["x"]
    print(len(digests), "cases,", sum(len(d) for d in digests.values()), "digests; the 7 + 5 split ends in another state than the one launch in",
          apart, "of", sum("b5_x" in d for d in digests.values()), "cases with generated gusts")
    with open(out, "w") as fh:
        json.dump(dict(meta=meta, digests=digests), fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1000000


if __name__ == "__main__":
    main(sys.argv[1])
