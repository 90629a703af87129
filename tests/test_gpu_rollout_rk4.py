"""The Runge-Kutta rollouts (f16_rollout_rk, f16_rollout_lqr_rk, f16_rollout_cost_rk with F16_INT_RK4) on the device against the
restatement of tests/rk4_cases.py; the conditions these comparisons rest on are checked without a GPU in tests/test_rk4_cpu.py.

The launch rules read F16_DYN_BLOCK once per process, so every routing runs in a child process (tests/rk4_child.py), one after
another, each under its own timeout.  A child that ends by a signal, an abort, a timeout or any other failure stops the module: the
tests after it fail without starting another GPU process.

  routing   kernel of the ~1.4 k-aircraft lattice
  lane64    k_rollout<64, ., STAGES = 4> (the default), + k_rollout_exact<., 4> under F16_FLAG_ONE_LANE
  lane128   k_rollout<128, ., 4>   (F16_DYN_BLOCK=128)
  lane256   k_rollout<256, ., 4>   (F16_DYN_BLOCK=256)
  ceiling   F16_DYN_BLOCK=512: the 512-lane RK4 kernels are not instantiated (they spill: profiles/rollout_rk4_resources.txt), the
            launch rules fall back to 256 lanes -- asserted as the bits of lane256

Bounds: states within 1e-9 relative of the restatement on states_ok (the band of test_gpu_envelope.py), status words bit for bit on
status_ok, every routing within 1e-11 of the F16_FLAG_ONE_LANE result, the scored cost within 1e-12 relative of its formula
evaluated in fp64 on the stored trajectory.

Largest relative errors measured on an MI355X (every test prints its own as a MEASURED line): states against the restatement 5.8e-15
(lattice at 10 ms), 1.1e-15 (high rates), 1.0e-15 (schedule), 1.2e-14 (LQR loop), lofi 9.3e-15, the same on every routing; against
the one-lane kernel 0 (hifi: the same bits) and 3.6e-15 (lofi); scored cost against its formula 4.4e-16; G10 at 10 ms, largest
error / G10_TOL: RK4 0.17 0.10 0.13 0.16, Euler 1.40 1.76 1.55 1.53."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rk4_cases as rk

pytestmark = pytest.mark.gpu
ROLLOUT_TOL = 1e-9
ONE_LANE_TOL = 1e-11
COST_TOL = 1e-12
HERE = os.path.dirname(os.path.abspath(__file__))
MPC_X = [3, 4, 7, 8, 9, 10, 11, 17, 16]
KNOBS = ("F16_ROLLOUT_QUAD_MAXB", "F16_ROLLOUT_4W_MAXB", "F16_DYN_BLOCK", "F16_ROLLOUT_I32")
# routing: (environment of the child, its jobs)
ROUTINGS = {
    "lane64": ({}, ["cases", "one_lane", "forward", "split", "score", "sizes", "g10", "nan"]),
    "lane128": ({"F16_DYN_BLOCK": "128"}, ["cases"]),
    "lane256": ({"F16_DYN_BLOCK": "256"}, ["cases", "split", "score"]),
    "ceiling": ({"F16_DYN_BLOCK": "512"}, ["ceiling"]),
}
_RESULTS, _DEAD = {}, []


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def child(routing, tmp_path_factory):
    """the results of one routing (npz as a dict), from a child process that is started at most once"""
    if routing in _RESULTS:
        return _RESULTS[routing]
    if _DEAD:
        pytest.fail(f"{routing} not started: {_DEAD[0]}")
    knobs, jobs = ROUTINGS[routing]
    out = str(tmp_path_factory.mktemp("rk4") / f"{routing}.npz")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs)
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "rk4_child.py"), out] + jobs, env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        _DEAD.append(f"the child of {routing} did not finish in 240 s")
        pytest.fail(_DEAD[0])
    if p.returncode != 0:
        _DEAD.append(f"the child of {routing} ended with status {p.returncode}: {p.stderr[-2000:]}")
        pytest.fail(_DEAD[0])
    with np.load(out) as z:
        _RESULTS[routing] = {k: z[k] for k in z.files}
    assert list(_RESULTS[routing]["knobs"]) == [knobs.get(k, "") for k in KNOBS]
    return _RESULTS[routing]


def compare(got, prefix, oracle, names, one_lane=None):
    """states vs the restatement (1e-9 on states_ok) and, with one_lane, vs the device's F16_FLAG_ONE_LANE result (1e-11); status
    words bit for bit on status_ok; under the LQR law the last action as well -> ({case: (err, err vs one lane)}, failures)"""
    report, failures = {}, []
    for name in names:
        r = rk.record(oracle, name)
        ok, okst = r["states_ok"], r["status_ok"]
        traj, x, st = got[prefix + name + "/traj"], got[prefix + name + "/x"], got[prefix + name + "/st"]
        assert traj.shape == r["traj"].shape and np.array_equal(traj[-1], x, equal_nan=True)
        err = max(rel(traj[t][ok], r["traj"][t][ok]) for t in range(len(traj)))
        if r["u_last"] is not None:
            err = max(err, rel(got[prefix + name + "/u"][ok], r["u_last"][ok]))
        if not err < ROLLOUT_TOL:
            failures.append(f"{name}: states off by {err:.3e} (bound {ROLLOUT_TOL})")
        if not np.array_equal(st[okst], r["status"][okst]):
            bad = np.nonzero(okst & (st != r["status"]))[0]
            failures.append(f"{name}: {len(bad)} status words differ, e.g. aircraft {bad[:5].tolist()} got {st[bad[:5]].tolist()} "
                            f"want {r['status'][bad[:5]].tolist()}")
        e1 = float("nan")
        if one_lane is not None:
            o = one_lane["ol/" + name + "/traj"]
            e1 = max(rel(traj[t][ok], o[t][ok]) for t in range(len(traj)))
            if r["u_last"] is not None:
                e1 = max(e1, rel(got[prefix + name + "/u"][ok], one_lane["ol/" + name + "/u"][ok]))
            if not e1 < ONE_LANE_TOL:
                failures.append(f"{name}: {e1:.3e} from the one-lane kernel's result (bound {ONE_LANE_TOL})")
        report[name] = (err, e1)
    return report, failures


def show(tag, report):
    print(f"MEASURED {tag}: " + json.dumps({k: [float(f"{a:.2e}"), float(f"{b:.2e}")] for k, (a, b) in report.items()}))


# ------------------------------------------------------------------------------------------------ 1. the lattice, every routing
@pytest.mark.parametrize("routing", ["lane64", "lane128", "lane256"])
def test_lattice_against_the_restatement(oracle, tmp_path_factory, routing):
    got, ol = child(routing, tmp_path_factory), child("lane64", tmp_path_factory)
    report, failures = compare(got, "", oracle, rk.LATTICE_CASES, ol)
    show(routing, report)
    assert not failures, f"{routing}:\n" + "\n".join(failures)


def test_lattice_one_lane_against_the_restatement(oracle, tmp_path_factory):
    report, failures = compare(child("lane64", tmp_path_factory), "ol/", oracle, list(rk.CASES))
    show("one_lane", report)
    assert not failures, "\n".join(failures)


def test_rk4_stops_at_256_lanes(tmp_path_factory):
    """F16_DYN_BLOCK=512 asks for 512-lane workgroups; an RK4 rollout runs its 256-lane kernel instead, bit for bit"""
    a, b = child("ceiling", tmp_path_factory), child("lane256", tmp_path_factory)
    name = rk.LATTICE_CASES[0]
    for k in ("traj", "x", "st"):
        assert np.array_equal(a[f"{name}/{k}"], b[f"{name}/{k}"], equal_nan=True), k


# ------------------------------------------------------------------------------------------------ 2. Euler forwarding
def test_euler_method_forwards_to_the_existing_calls(tmp_path_factory):
    got = child("lane64", tmp_path_factory)
    for k in ("open", "lqr", "cost"):
        assert bool(got["forward/" + k]), k
    assert bool(got["forward/rk4_differs"])
    assert bool(got["forward/python_schedule"]) and bool(got["forward/python_rollout"])


# ------------------------------------------------------------------------------------------------ 3. split and schedule
@pytest.mark.parametrize("routing", ["lane64", "lane256"])
def test_split_and_schedule(oracle, tmp_path_factory, routing):
    got = child(routing, tmp_path_factory)
    assert bool(got["split/chain"]), "one call per segment"
    assert bool(got["split/n_plus_m"]), "n steps then m steps"
    assert bool(got["split/constant_rows"]), "a constant row given as S rows"
    r = rk.record(oracle, "hifi_sched40")
    assert np.array_equal(got["split/one/traj"], got["hifi_sched40/traj"], equal_nan=True)
    report, failures = compare(got, "", oracle, ["hifi_sched40"])
    show(routing + " schedule", report)
    assert not failures and r["states_ok"].sum() >= r["batch"].B - 4, failures


# ------------------------------------------------------------------------------------------------ 4. the LQR loop
@pytest.mark.parametrize("routing", ["lane64", "lane128", "lane256"])
def test_lqr_loop_against_the_restated_loop(oracle, tmp_path_factory, routing):
    """constant and scheduled demands; the action formed from the start-of-step state and held over the stages; u_out"""
    got, ol = child(routing, tmp_path_factory), child("lane64", tmp_path_factory)
    report, failures = compare(got, "", oracle, ["hifi_lqr", "hifi_lqr_sched", "lofi_lqr"], ol)
    show(routing + " LQR", report)
    assert not failures, "\n".join(failures)
    # the law acts: the last action is not the offset it started from
    r = rk.record(oracle, "hifi_lqr")
    assert np.abs(r["u_last"][r["states_ok"], 1:] - r["batch"].u[r["states_ok"], 1:]).max() > 1e-3


# ------------------------------------------------------------------------------------------------ 5. scored
@pytest.mark.parametrize("routing", ["lane64", "lane256"])
def test_scored_rollout(tmp_path_factory, routing):
    from test_gpu_rollout_cost import cost_definition
    got = child(routing, tmp_path_factory)
    w = rk.score_weights()
    for key in ("16x8", "16x8_one_lane", "70x3"):
        g = lambda k: got[f"score/{key}/{k}"]
        assert bool(g("states_equal_rollout_rk")), key
        assert bool(g("cost_same_bits_bare")), key
        traj = g("traj")                                                         # [T, B, 18]
        J, frozen_from = cost_definition(g("x0"), g("rows"), g("xref"), g("uref"), w, traj.transpose(0, 2, 1), 7)
        cost = g("cost")
        err = float(np.max(np.abs(cost - J) / np.abs(J)))
        print(f"MEASURED {routing} score {key}: cost vs its formula {err:.2e} (bound {COST_TOL}); frozen lanes {int((frozen_from < len(traj)).sum())}")
        assert np.isfinite(J).all() and err <= COST_TOL
        assert np.array_equal((g("st") & 16) != 0, frozen_from < len(traj)) and (frozen_from == 0).any()
        assert np.array_equal(g("x"), traj[-1])


# ------------------------------------------------------------------------------------------------ 6. ONE_LANE and the batch size
def test_one_lane_results_do_not_depend_on_the_batch_size(tmp_path_factory):
    got = child("lane64", tmp_path_factory)
    assert bool(got["sizes/one_lane_same_bits"]) and bool(got["sizes/scored_same_bits"])
    print("default routing bit-identical to one lane:", bool(got["sizes/default_equals_one_lane"]))


# ------------------------------------------------------------------------------------------------ 7. G10 on the device
def test_g10_on_the_device_rk4_inside_euler_outside_at_10ms(tmp_path_factory):
    from conftest import G10_TOL, g10_case, g10_rows_of_states
    got = child("lane64", tmp_path_factory)
    for k in range(4):
        a, _, x0, _, _ = g10_case(k)
        errs = {}
        for m in ("rk4", "euler"):
            assert int(got[f"g10/{m}_{k}/st"][0]) == 0
            hist = np.concatenate((x0[None], got[f"g10/{m}_{k}/traj"][:, 0]))    # [101, 18]
            errs[m] = np.abs(g10_rows_of_states(hist) - a[:, 1:13]).max(0) / G10_TOL
        print(f"MEASURED G10 case {k}: largest error / G10_TOL, RK4 10 ms {errs['rk4'].max():.2f}, Euler 10 ms {errs['euler'].max():.2f}")
        assert errs["rk4"].max() < 1.0, errs["rk4"]
        assert errs["euler"].max() > 1.0, errs["euler"]


# ------------------------------------------------------------------------------------------------ 8. NaN and extreme commands
@pytest.mark.parametrize("which", ["default", "one_lane"])
def test_nan_and_extreme_commands(oracle, tmp_path_factory, which):
    from rk4_child import nan_inputs
    got = child("lane64", tmp_path_factory)
    x0, rows = nan_inputs()
    r = rk.restate(oracle, x0, rows, 6, 3, 0.01, 1)
    traj, st = got[f"nan/{which}/traj"], got[f"nan/{which}/st"]
    assert np.array_equal(np.isnan(traj), np.isnan(r["traj"])) and np.array_equal(np.isinf(traj), np.isinf(r["traj"]))
    fin = np.isfinite(r["traj"])
    assert rel(traj[fin], r["traj"][fin]) < ROLLOUT_TOL
    assert np.array_equal(st[4:7], r["status"][4:7]), (st, r["status"])             # (the aircraft whose states stay finite)
    assert np.isnan(r["traj"][:, :4]).any((0, 2)).all() and (st[:4] & 32).all()      # a NaN command reaches the state, and the flag
    assert np.isfinite(traj[:, 4]).all() and np.isfinite(traj[:, 5]).all()            # huge and infinite commands are clipped
    # the frozen aircraft keeps its state and never reads its NaN row; aircraft 7 is ordinary until its row turns NaN
    assert (traj[:, 6] == x0[6]).all() and st[6] == 16 | 1 << (8 + 2)
    assert np.isfinite(traj[:3, 7]).all() and np.isnan(traj[3:, 7]).any(1).all()
