"""Fixture G22 (tests/golden/g22_model_stage_bits.json): SHA-256 digests of everything the model stage of the control chain writes, on
the cases of tests/test_gpu_model_stage_bits.py (its cases() and Stage are used here; what they are is said there).  Every case is
flown twice and nothing is written unless the two flights agree in every digest.  Before anything is recorded the restatement on the
CPU (oracle/) is asked whether the placed aircraft of the LQR loops leaves the envelope inside the flight, and the recorded status words
are asked the same.  Run on the GPU with the library whose results are to be recorded (the parent commit's):
    F16HIP_SO=_exp/parent/libf16hip.so python tools/gpu_make_model_stage_golden.py tests/golden/g22_model_stage_bits.json"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]
from gpu_make_air_rollout_golden import leaving_step  # noqa: E402
from test_gpu_model_stage_bits import HOLD, LEAVING, LQR_DT, NSTEPS, OUTSIDE, SIZES, Stage, air_batch, cases  # noqa: E402

ST_ENVELOPE = 16


def main(out):
    from f16_mpc_oop_py_amd import lib
    assert (NSTEPS, LQR_DT) == (12, 0.01)              # (the flight leaving_step restates)
    meta = dict(nsteps=NSTEPS, hold=HOLD, dt=LQR_DT, outside=OUTSIDE, leaving=LEAVING, leaves_after_step=leaving_step(*air_batch(SIZES[0])),
                so=os.path.basename(lib.SO_PATH))
    print("restatement: aircraft", LEAVING, "is above 100,000 ft after step", meta["leaves_after_step"])
    stage, digests = Stage(), {}
    for cid, method, args in cases():
        first, second = stage.case(method, args), stage.case(method, args)
        apart = [k for k in first if first[k] != second.get(k)]
        if apart or sorted(first) != sorted(second):
            sys.exit(f"{cid}: two flights of the same case differ in {apart}: nothing written")
        if method == "lqr_relin":
            st = stage.status
            assert st[OUTSIDE] & ST_ENVELOPE and st[LEAVING] & ST_ENVELOPE and not (st & ST_ENVELOPE).all(), (cid, st[:8])
        digests[cid] = first
        print(cid, len(first), "digests", flush=True)
    print(len(digests), "cases,", sum(len(d) for d in digests.values()), "digests")
    with open(out, "w") as fh:
        json.dump(dict(meta=meta, digests=digests), fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1000000


if __name__ == "__main__":
    main(sys.argv[1])
