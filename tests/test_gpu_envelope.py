"""Every plant kernel against the C restatement over the WHOLE table grid and envelope (tests/envelope_cases.py: one aircraft per
(alpha, beta, elevator) cell of the hifi and of the lofi tables, edge rows, commands that drive every actuator limit; the conditions
these comparisons rest on are checked without a GPU in tests/test_envelope_cpu.py).

Single-evaluation kernels (_calc_xdot, nlplant, _calc_xdot_na): xcg 0.25 / 0.35, with and without F16_FLAG_FIX_CLR, at XDOT_TOL;
status words bit for bit.

Rollout kernels: the launch rules read their knobs once per process, so each routing of ROUTINGS runs in a child process
(tests/envelope_child.py) on the same ~1.4 k aircraft: open loop 40 steps with a sample per step and 100 steps, high body rates
(the carried sin / cos pairs fall back to exact evaluation), dt = 10 ms, a command schedule (hold 7), the LQR closed loop, the same
without the envelope test, and (default routing) the scored rollout.  States within 1e-9 relative of the restatement and within
1e-11 of the device's own F16_FLAG_ONE_LANE result; status words equal to the restatement's bit for bit outside the near-edge set.
A child that ends by a signal, an abort, a timeout or any other failure stops the module: the routings after it fail without
starting another GPU process.

Largest relative errors measured on an MI355X (every test prints its own as a MEASURED line):
  single evaluation   hifi xdot / nlplant 6.3e-14, xdot_na 2.4e-14; lofi 5.1e-14, 5.8e-15
  routing             states vs restatement   vs one-lane kernel
  quad1, quad2        7.1e-15                 5.5e-15      (bit-identical to each other)
  4wave               7.1e-15                 3.4e-15
  lane64              1.2e-14                 1.2e-14
  lane128, lane256    1.3e-14                 1.3e-14
  int512              1.3e-14                 1.3e-14
  lane512             7.1e-15                 2.4e-15
  lofi64              1.9e-14                 2.0e-14
  lofi512             1.1e-14                 0 (the same bits)
  one lane            hifi 7.1e-15, lofi 1.1e-14
  scored rollout      cost vs its definition 8.9e-16 / 4.8e-16 (bound 1.1e-13), states 3.7e-15 / 2.3e-15
The worst case of every hifi routing is the LQR loop or the 40 / 100-step open loop; none comes within four orders of a bound."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import envelope_cases as ec

pytestmark = pytest.mark.gpu
XDOT_TOL = 1e-11            # tests/test_gpu_dynamics.py
ROLLOUT_TOL = 1e-9          # the suite's rollout bound against the restatement (test_random_batches_vs_oracle)
ONE_LANE_TOL = 1e-11        # test_one_lane_flag_results_do_not_depend_on_the_batch_size
MPC_X = [3, 4, 7, 8, 9, 10, 11, 17, 16]
HERE = os.path.dirname(os.path.abspath(__file__))

NO4 = {"F16_ROLLOUT_QUAD_MAXB": "0", "F16_ROLLOUT_4W_MAXB": "0"}
# routing: (batch, environment of the child, kernel, options of the child)
ROUTINGS = {
    "quad1": ("hifi", {}, "k_rollout_q<1> (+ k_rollout_exact under F16_FLAG_ONE_LANE, k_rollout<64, COST> scored)", ["one_lane", "score"]),
    "quad2": ("hifi", {"F16_ROLLOUT_QUAD_MAXB": "1024"}, "k_rollout_q<2>", []),
    "4wave": ("hifi", {"F16_ROLLOUT_QUAD_MAXB": "0"}, "k_rollout_4w", []),
    "lane64": ("hifi", NO4, "k_rollout<64,-1>, carried trig", []),
    "lane128": ("hifi", dict(NO4, F16_DYN_BLOCK="128"), "k_rollout<128,-1>, carried trig", []),
    "lane256": ("hifi", dict(NO4, F16_DYN_BLOCK="256"), "k_rollout<256,-1>, carried trig (LQR: full sincos)", []),
    "int512": ("hifi", dict(NO4, F16_DYN_BLOCK="512"), "k_rollout_i<512>, integer table image", []),
    "lane512": ("hifi", dict(NO4, F16_DYN_BLOCK="512", F16_ROLLOUT_I32="0"), "k_rollout<512,-1>, full sincos (LQR: k_rollout<256>)", []),
    "lofi64": ("lofi", {"F16_DYN_BLOCK": "64"}, "k_rollout<64,0> (+ k_rollout_exact, k_rollout<64,0,COST>)", ["one_lane", "score"]),
    "lofi512": ("lofi", {"F16_DYN_BLOCK": "512"}, "k_rollout<512,0>", []),
}
ONE_LANE_OF = {"hifi": "quad1", "lofi": "lofi64"}
# routings that run different code on the same numbers and must therefore differ in at least one bit (four lanes per aircraft vs one,
# carried vs full sincos, integer vs fp64 table image, 64-lane lofi carried trig vs 512-lane full); pairs that may agree are reported
MUST_DIFFER = [("quad1", "lane64"), ("4wave", "lane64"), ("lane64", "lane512"), ("int512", "lane512"), ("quad1", "int512"),
               ("lofi64", "lofi512")]
KNOBS = ("F16_ROLLOUT_QUAD_MAXB", "F16_ROLLOUT_4W_MAXB", "F16_DYN_BLOCK", "F16_ROLLOUT_I32")

_RESULTS, _DEAD = {}, []


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def make_env(x, u=None, **kw):
    from f16_mpc_oop_py_amd import F16Batch
    return F16Batch(x, u, device="cuda:0", **kw)


# ------------------------------------------------------------------------------------------------ single-evaluation kernels
@pytest.mark.parametrize("fix_clr", [0, 1])
@pytest.mark.parametrize("xcg", [0.25, 0.35])
@pytest.mark.parametrize("which", ["hifi", "lofi"])
def test_single_evaluation_kernels_over_the_whole_grid(oracle, which, xcg, fix_clr):
    b = ec.hifi_lattice() if which == "hifi" else ec.lofi_lattice()
    x, u, fi = b.x, b.u, b.fi
    rng = np.random.default_rng(11)
    x9 = x[:, MPC_X] + rng.uniform(-1e-3, 1e-3, (b.B, 9))                     # the scattered vectors differ from x_full
    u3 = np.clip(u[:, 1:4], [-26, -21.5, -30], [26, 21.5, 30])              # (the elevator slightly beyond its table: F16_ST_EL)
    oracle.lib.f16o_set_fix_clr(fix_clr)
    try:
        ref, rst = oracle.xdot_batch(x, u, fi_flag=fi, xcg=xcg), np.zeros(b.B, dtype=np.int32)
        refn, refa, ast = np.zeros((b.B, 18)), np.zeros((b.B, 9)), np.zeros(b.B, dtype=np.int32)
        for i in range(b.B):
            refn[i] = oracle.nlplant(x[i], fi, xcg)
            rst[i] = oracle.lib.f16o_last_status()
            refa[i] = oracle.calc_xdot_na(x[i], x9[i], u3[i], fi, xcg)
            ast[i] = oracle.lib.f16o_last_status()
    finally:
        oracle.lib.f16o_set_fix_clr(0)
    if _DEAD:
        pytest.fail(f"not started: {_DEAD[0]}")
    try:
        env = make_env(x, u, xcg=xcg, fi_flag=fi, flags=fix_clr)
        xd = env._calc_xdot().cpu().numpy()
        st = env.last_status.cpu().numpy()
        xn = env.nlplant(x).cpu().numpy()
        stn = env.last_status.cpu().numpy()
        xa = env._calc_xdot_na(x9, u3).cpu().numpy()
        sta = env.last_status.cpu().numpy()
    except Exception as e:                                                        # a HIP error: nothing more of this module runs on the GPU
        _DEAD.append(f"single-evaluation kernels ({which}, xcg {xcg}, fix_clr {fix_clr}): {e!r}")
        raise
    errs = rel(xd, ref), rel(xn, refn), rel(xa, refa)
    print(f"{which} xcg {xcg} fix_clr {fix_clr}: xdot {errs[0]:.2e}, nlplant {errs[1]:.2e}, xdot_na {errs[2]:.2e}")
    assert max(errs) < XDOT_TOL and np.isfinite(ref).all() and np.isfinite(refa).all()
    assert np.array_equal(st, rst) and np.array_equal(stn, rst) and np.array_equal(sta, ast)
    assert (rst != 0).any() and ((ast & 8).any() or fi == 0)                    # (the lofi lookups raise F16_ST_BETA alone)
    if which == "hifi" and fix_clr:                                               # the flag changes the answer all over the grid
        assert np.abs(make_env(x, u, xcg=xcg)._calc_xdot().cpu().numpy()[:, 9] - xd[:, 9]).max() > 1e-3


# ------------------------------------------------------------------------------------------------ rollout kernels, one child each
def child(routing, tmp_path_factory):
    """the results of one routing (npz as a dict), from a child process that is started at most once"""
    if routing in _RESULTS:
        return _RESULTS[routing]
    if _DEAD:
        pytest.fail(f"{routing} not started: {_DEAD[0]}")
    which, knobs, _, opts = ROUTINGS[routing]
    out = str(tmp_path_factory.mktemp("envelope") / f"{routing}.npz")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs)
    cmd = [sys.executable, os.path.join(HERE, "envelope_child.py"), out, which] + opts
    try:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)      # ~10 s of import and launches
    except subprocess.TimeoutExpired:
        _DEAD.append(f"the child of {routing} did not finish in 240 s")
        pytest.fail(_DEAD[0])
    if p.returncode != 0:
        _DEAD.append(f"the child of {routing} ended with status {p.returncode}: {p.stderr[-2000:]}")
        pytest.fail(_DEAD[0])
    with np.load(out) as z:
        _RESULTS[routing] = {k: z[k] for k in z.files}
    return _RESULTS[routing]


def compare(got, prefix, oracle, which, one_lane=None):
    """every case of the batch: states vs the restatement (1e-9) and, with one_lane (another child's "ol/" results), vs the
    device's own one-lane kernel (1e-11); status words bit for bit.  -> {case: (err vs restatement, err vs one lane)}"""
    report, failures = {}, []
    for name, c in ec.CASES.items():
        if c["batch"] != which:
            continue
        r = ec.reference(oracle, name)
        ok, okst = r["states_ok"], r["status_ok"]
        traj, x, st = got[prefix + name + "/traj"], got[prefix + name + "/x"], got[prefix + name + "/st"]
        want = r["traj"] if len(traj) == c["T"] else r["traj"][-1:]
        assert traj.shape == want.shape and np.array_equal(traj[-1], x, equal_nan=True)
        per_step = [rel(traj[t][ok], want[t][ok]) for t in range(len(traj))]
        err = max(per_step)
        if c["kind"] == "lqr":
            err = max(err, rel(got[prefix + name + "/u"][ok], r["u_last"][ok]))
        if not err < ROLLOUT_TOL:
            t = int(np.argmax(np.array(per_step) >= ROLLOUT_TOL)) if np.isfinite(per_step).all() else int(np.argmax(~np.isfinite(per_step)))
            e = np.abs(traj[t] - want[t]) / np.maximum(1.0, np.abs(want[t]))
            e[~ok] = 0
            worst = np.argsort(-np.nan_to_num(e.max(1), nan=np.inf))[:5]
            failures.append(f"{name}: states off by {err:.3e} (bound {ROLLOUT_TOL}); first at sample {t}; worst aircraft {worst.tolist()} "
                            f"cells {r['batch'].cell[worst].tolist()} states {e[worst].argmax(1).tolist()}")
        if not np.array_equal(st[okst], r["status"][okst]):
            bad = np.nonzero(okst & (st != r["status"]))[0]
            failures.append(f"{name}: {len(bad)} status words differ, e.g. aircraft {bad[:5].tolist()} cells {r['batch'].cell[bad[:5]].tolist()} "
                            f"got {st[bad[:5]].tolist()} want {r['status'][bad[:5]].tolist()}")
        e1 = float("nan")
        if one_lane is not None:
            o = one_lane["ol/" + name + "/traj"]
            e1 = max(rel(traj[t][ok], o[t][ok]) for t in range(len(traj)))
            if c["kind"] == "lqr":
                e1 = max(e1, rel(got[prefix + name + "/u"][ok], one_lane["ol/" + name + "/u"][ok]))
            if not e1 < ONE_LANE_TOL:
                failures.append(f"{name}: {e1:.3e} from the one-lane kernel's result (bound {ONE_LANE_TOL})")
        report[name] = (err, e1)
    return report, failures


@pytest.mark.parametrize("routing", list(ROUTINGS))
def test_rollout_routing_against_the_restatement(oracle, tmp_path_factory, routing):
    which, knobs, kernel, opts = ROUTINGS[routing]
    got = child(routing, tmp_path_factory)
    assert list(got["knobs"]) == [knobs.get(k, "") for k in KNOBS]              # the child ran under the intended knobs
    ol = child(ONE_LANE_OF[which], tmp_path_factory)
    report, failures = compare(got, "", oracle, which, ol)
    worst = max(v[0] for v in report.values()), max(v[1] for v in report.values())
    print(f"MEASURED {routing} [{kernel}]: vs restatement {worst[0]:.2e}, vs one lane {worst[1]:.2e}; per case "
          + json.dumps({k: [float(f"{a:.2e}"), float(f"{b:.2e}")] for k, (a, b) in report.items()}))
    assert not failures, f"{routing} [{kernel}]:\n" + "\n".join(failures)


@pytest.mark.parametrize("which", ["hifi", "lofi"])
def test_one_lane_kernel_against_the_restatement(oracle, tmp_path_factory, which):
    """k_rollout_exact (F16_FLAG_ONE_LANE), every case"""
    got = child(ONE_LANE_OF[which], tmp_path_factory)
    report, failures = compare(got, "ol/", oracle, which)
    print(f"MEASURED one_lane {which} [k_rollout_exact]: vs restatement {max(v[0] for v in report.values()):.2e}; per case "
          + json.dumps({k: float(f"{a:.2e}") for k, (a, _) in report.items()}))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("which", ["hifi", "lofi"])
def test_scored_rollout_on_the_lattice(oracle, tmp_path_factory, which):
    """score_schedules (f16_rollout_cost: the scored twin of the 64-lane kernel) on the lattice states: the cost against its
    definition (the helper of test_gpu_rollout_cost.py, on the launch's own samples), states and status against the restated
    schedule"""
    from test_gpu_rollout_cost import EPS, cost_definition
    got = child(ONE_LANE_OF[which], tmp_path_factory)
    name = which + "_sched40"
    r = ec.reference(oracle, name)
    b, _, rows, _, _ = ec.case_inputs(name)
    w = ec.score_weights()
    traj = got["score/traj"]                                                     # [40, B, 18]
    J, frozen_from = cost_definition(b.x, rows[:, None], b.x[:, MPC_X], None, w, traj.transpose(0, 2, 1), ec.SCHED_HOLD)
    cost, st = got["score/cost"], got["score/st"]
    assert np.array_equal((st & 16) != 0, frozen_from < 40) and np.isfinite(J).all() and np.isfinite(cost).all()
    tol = EPS * (12 * 40 + 9 + 4)
    err = float(np.max(np.abs(cost - J) / J))
    ok, okst = r["states_ok"], r["status_ok"]
    es = max(rel(traj[t][ok], r["traj"][t][ok]) for t in range(40))
    print(f"MEASURED score {which}: cost vs definition {err:.2e} (bound {tol:.2e}), states vs restatement {es:.2e}")
    assert err <= tol and es < ROLLOUT_TOL
    assert np.array_equal(got["score/x"], traj[-1]) and np.array_equal(st[okst], r["status"][okst])
    # the lanes the definition finds frozen are the restatement's; some at the start (the rows outside the box), one on the way
    assert np.array_equal((frozen_from < 40)[okst], ((r["status"] & 16) != 0)[okst])
    assert (frozen_from == 0).sum() >= 2 and ((frozen_from > 0) & (frozen_from < 40)).any()


def test_routings_that_must_differ_do(tmp_path_factory):
    """the cheapest evidence that a knob did select another kernel: different code on the same numbers differs in some bit"""
    same = []
    for a, b in MUST_DIFFER + [("quad1", "quad2"), ("quad1", "4wave"), ("lane64", "lane128"), ("lane128", "lane256"), ("lane256", "lane512")]:
        ra, rb = child(a, tmp_path_factory), child(b, tmp_path_factory)
        keys = [k for k in ra if k.endswith("/traj") and not k.startswith(("ol/", "score/"))]
        equal = all(np.array_equal(ra[k], rb[k], equal_nan=True) for k in keys)
        if equal:
            same.append((a, b))
        print(f"{a} vs {b}: {'bit-identical everywhere' if equal else 'differ'}")
    wrong = [p for p in same if p in MUST_DIFFER]
    assert not wrong, f"agree bit for bit everywhere, so one knob did not take: {wrong} (all identical pairs: {same})"
