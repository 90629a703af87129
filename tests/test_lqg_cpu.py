"""CPU-side checks of the output-feedback entries (include/f16_hip.h "OUTPUT FEEDBACK": f16_kalman_batch, f16_observer_step,
f16_rollout_lqg_wind, f16_rollout_lqg_wind_ens) and of f16_mpc_oop_py_amd/observer.py: what tests/test_gpu_lqg.py rests on, and
everything that needs no device.

  * kalman_reference (the doubling, in numpy) against scipy.linalg.solve_discrete_are on both golden models x three sensor sets:
    P to 1e-10 relative (measured here 2e-14 .. 6e-13: the cap leaves two orders for other variances and is far below anything a
    wrong recursion gives), and Lf = P (I + G P)^-1 C'V^-1 against P C'(C P C' + V)^-1 to 1e-9 of max|Lf|;
  * observer_reference on the linear plant it models: without noise and from the true state the innovations stay at rounding level;
  * the loop on the CPU oracle plant: finite, and the Kalman observer's rate estimates at less than half the rms error of raw
    measurements (pass-through) -- a condition any working filter meets and pass-through, at ratio 1, does not;
  * the argument rules of the four C entry points on calls the library refuses or treats as a no-op (a zeroed host buffer stands for
    the context and for every array), and the ValueErrors of the Python keywords on the recording environment.
"""
import ctypes

import numpy as np
import pytest

import lqg_cases as lc
from header_cases import header_parameters, names
from test_rollout_calls_cpu import BAD_ARGUMENT, BAD_STEPS, F16_EINVAL, F16_OK, env_of
from test_rollout_rk_calls_cpu import BAD_METHOD, METHODS, clib  # noqa: F401  (clib: the fixture)

ROLLOUTS = {"f16_rollout_lqg_wind": "f16_rollout_lqr_wind", "f16_rollout_lqg_wind_ens": "f16_rollout_lqr_wind_ens"}
OBS_NULL = "obs / h_sigma / xhat is NULL"


# ------------------------------------------------------------------------------------------------ 1. the doubling
@pytest.mark.parametrize("tag,sensed", lc.CASES)
def test_kalman_reference_against_scipy(tag, sensed):
    from f16_mpc_oop_py_amd.observer import kalman_reference
    Ad = lc.model(tag)[0]
    v = lc.SIGMA_DESIGN ** 2
    Pm, Lf, it = kalman_reference(Ad, lc.W_DESIGN, v, sensed)
    Ps, Ls = lc.scipy_filter(Ad, lc.W_DESIGN, v, sensed)
    eP, eL = lc.relerr(Pm, Ps), float(np.abs(Lf - Ls).max() / np.abs(Ls).max())
    print(f"MEASURED kalman_reference {tag} sensed={sensed:#x}: {it} doublings, P rel. error {eP:.2e}, Lf forms differ by {eL:.2e} of max|Lf| = {np.abs(Ls).max():.1f}")
    assert it < 60 and eP <= 1e-10 and eL <= 1e-9
    unsensed = [k for k in range(9) if k not in lc.channels(sensed)]
    assert np.all(Lf[:, unsensed] == 0.0)


def test_kalman_reference_reports_what_does_not_converge():
    """an unstable mode no sensor sees: the doubling runs into its cap"""
    from f16_mpc_oop_py_amd.observer import kalman_reference
    assert kalman_reference(1.01 * np.eye(9), lc.W_DESIGN, lc.SIGMA_DESIGN ** 2, 0x01)[2] == 60


# ------------------------------------------------------------------------------------------------ 2. the rule on its own model
def test_observer_reference_on_the_linear_plant_it_models():
    """200 steps of the linear plant x9+ = trim + Ad (x9 - trim) + Bd (s - s_trim) (numpy's matrix products) under moving surfaces,
    observed without noise from the true state: every innovation is what the two ways of summing the same terms differ by.  Bound:
    one prediction differs from the plant's step by at most 13 eps sum|terms| (13 terms per entry); a correction hands an
    innovation on multiplied by at most 1 + max|Lf|, and at most 200 steps add up."""
    from f16_mpc_oop_py_amd.observer import kalman_reference, observer_reference, pack_models
    Ad, Bd, x_trim, K = lc.model("xcg25")
    trim, strim = x_trim[lc.MPC_IDX], x_trim[13:16]
    _, Lf, _ = kalman_reference(Ad, lc.W_FLIGHT, lc.SIGMA_FLIGHT ** 2, 0x7f)
    models = pack_models(Ad[None], Bd[None], Lf[None], trim[None], strim[None])
    rng = np.random.default_rng(5)
    x9 = trim + 0.01 * rng.standard_normal(9)
    xm, worst, mag = x9[None].copy(), 0.0, 0.0
    for t in range(200):
        s = strim + np.array([1.0, -0.5, 0.3]) * np.sign(np.sin(0.05 * t))
        r = observer_reference(models, 0, 0x7f, x9[None], s[None], xm, K, np.zeros((1, 3)), x_trim[None, 12:16], sigma=np.zeros(9), normals=np.zeros((1, 9)))
        worst = max(worst, float(np.abs(r["y"][0, :7] - xm[0, :7]).max()))
        mag = max(mag, float(r["mag_xm"].max()))
        xm = r["xm"]
        x9 = trim + Ad @ (x9 - trim) + Bd @ (s - strim)
    bound = 200 * (1.0 + np.abs(Lf).max()) * 13 * lc.EPS * mag
    print(f"MEASURED largest innovation over 200 noise-free steps: {worst:.2e} (bound {bound:.2e})")
    assert worst <= bound


# ------------------------------------------------------------------------------------------------ 3. the loop on the oracle plant
@pytest.mark.parametrize("seed", [1, 2])
def test_the_filter_filters_on_the_oracle_plant(oracle, seed):
    from f16_mpc_oop_py_amd.observer import kalman_reference, pack_models
    Ad, Bd, x_trim, _ = lc.model("xcg25")
    trim, strim = x_trim[lc.MPC_IDX], x_trim[13:16]
    _, Lf, it = kalman_reference(Ad, lc.W_FLIGHT, lc.SIGMA_FLIGHT ** 2, 0x7f)
    assert it < 60
    T = 1500
    rms = {}
    for name, gain in (("kalman", Lf), ("passthrough", np.diag([1.0] * 7 + [0.0] * 2))):
        r = lc.oracle_loop(oracle, pack_models(Ad[None], Bd[None], gain[None], trim[None], strim[None]), 0x7f, lc.SIGMA_FLIGHT, seed, T)
        assert all(np.isfinite(v).all() for v in r.values()), name
        rms[name] = np.sqrt(((r["xh"] - r["x9"])[T // 3:, 4:7] ** 2).mean(0))
        rms[name + "_u"] = r["u"][T // 3:, 1].std()
    ratio = rms["kalman"] / rms["passthrough"]
    print(f"MEASURED seed {seed}: rms error of the (p, q, r) estimate, Kalman / pass-through: {ratio}; elevator command deviation "
          f"{rms['passthrough_u']:.3f} -> {rms['kalman_u']:.3f} deg")
    assert (ratio < 0.5).all()


# ------------------------------------------------------------------------------------------------ 4. the C rules
def ens_struct(buf, **fields):
    from f16_mpc_oop_py_amd import lib
    e = lib.Ens()
    for k in ("work", "count", "mean", "m2", "min", "max"):
        setattr(e, k, buf.value)
    e.group, e.ldg = 64, 1
    for k, v in fields.items():
        setattr(e, k, v)
    return e


def call(clib, symbol, **over):
    """`symbol` on a call that is complete except for `over` (None = a NULL pointer): no aircraft -> (rc, message)"""
    L, buf, _, _ = clib
    base = dict(B=0, ld=0, M=0, nsteps=6, hold=2, traj_every=1, dt=1e-3, xcg=0.35, fi_flag=1, method=1, flags=0, stream=None, traj=None,
                xhat_traj=None, u_out=None, status=buf, h_wind=None, y_out=None, Pm=None, iters=None, mgroup=0, sensed=0x7f, meas_seed=7, mrow0=0,
                mrow=0)
    if "h_ens" in names(symbol) and "h_ens" not in over:
        over = dict(over, h_ens=ctypes.byref(ens_struct(buf)))
    args = [over[n] if n in over else base.get(n, buf) for n in names(symbol)]
    rc = getattr(L, symbol)(*args)
    return rc, L.f16_last_error().decode()


def refused(clib, symbol, words, **over):
    rc, msg = call(clib, symbol, **over)
    assert rc == F16_EINVAL and words in msg, (symbol, over, rc, msg)


@pytest.mark.parametrize("symbol", list(ROLLOUTS))
def test_parameter_lists_are_the_siblings_plus_the_observer(symbol):
    new, old = header_parameters(symbol), header_parameters(ROLLOUTS[symbol])
    name = lambda p: p.replace("*", " ").split()[-1]
    k = [name(p) for p in old].index("traj")
    added = ["const double *obs", "long mgroup", "int sensed", "const double *h_sigma", "uint64_t meas_seed", "uint32_t mrow0", "double *xhat"]
    assert new == old[:k] + added + [old[k], "double *xhat_traj"] + old[k + 1:]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("symbol", list(ROLLOUTS))
def test_what_the_sibling_refuses_is_refused_first_then_the_observer(clib, symbol, method):
    buf = clib[1]
    for broken in (dict(), dict(obs=None), dict(sensed=0)):                     # the sibling's rules come first, whatever the observer
        refused(clib, symbol, BAD_ARGUMENT, method=method, ctx=None, **broken)
        refused(clib, symbol, BAD_ARGUMENT, method=method, x=None, **broken)
        refused(clib, symbol, BAD_ARGUMENT, method=method, B=4, ld=3, nsteps=0, **broken)
        refused(clib, symbol, BAD_STEPS, method=method, nsteps=-1, **broken)
        refused(clib, symbol, BAD_STEPS, method=method, nsteps=5, traj=buf, traj_every=2, **broken)
        refused(clib, symbol, "K / dem_seq is NULL", method=method, dem_seq=None, **broken)
        refused(clib, symbol, "hold must be >= 1", method=method, hold=0, **broken)
        refused(clib, symbol, BAD_METHOD, method=3, **broken)
    refused(clib, symbol, BAD_STEPS, method=method, nsteps=5, xhat_traj=buf, traj_every=2)      # the estimate's samples follow traj's rule
    if symbol.endswith("_ens"):
        refused(clib, symbol, "sample period of the ensemble", method=method, nsteps=5, traj_every=2, obs=None)
        refused(clib, symbol, "h_ens or one of its members is NULL", method=method, h_ens=None, obs=None)
        refused(clib, symbol, "group must be a multiple of 64", method=method, h_ens=ctypes.byref(ens_struct(buf, group=32)), obs=None)
    for p in ("obs", "h_sigma", "xhat"):
        refused(clib, symbol, OBS_NULL, method=method, **{p: None})
    for mgroup in (-64, 32, 100):
        refused(clib, symbol, "mgroup must be 0", method=method, mgroup=mgroup)
    for sensed in (0, -1, 0x200):
        refused(clib, symbol, "sensed must be a mask", method=method, sensed=sensed)
    for bad in (-1e-3, float("nan"), float("inf")):
        sg = (ctypes.c_double * 9)(*([0.0] * 4 + [bad] + [0.1] * 4))
        refused(clib, symbol, "a sigma is negative or not finite", method=method, h_sigma=ctypes.cast(sg, ctypes.c_void_p))
    # B == 0 and nsteps == 0 are no-ops; mgroup 0 and multiples of 64 pass; a NULL h_wind is no forward (the observer is still checked)
    for ok in (dict(), dict(mgroup=64), dict(mgroup=256), dict(B=4, ld=4, nsteps=0), dict(sensed=0x1ff), dict(sensed=1)):
        assert call(clib, symbol, method=method, **ok)[0] == F16_OK, ok


def test_kalman_batch_and_observer_step_check_their_arguments(clib):
    buf = clib[1]
    assert call(clib, "f16_kalman_batch")[0] == F16_OK
    for p in ("ctx", "Ad", "w", "v", "Lf", "status"):
        refused(clib, "f16_kalman_batch", "bad argument to f16_kalman_batch", **{p: None})
    refused(clib, "f16_kalman_batch", "bad argument to f16_kalman_batch", M=-1)
    refused(clib, "f16_kalman_batch", "bad argument to f16_kalman_batch", M=4, ld=3)
    for sensed in (0, 0x200):
        refused(clib, "f16_kalman_batch", "sensed must be a mask", sensed=sensed)
    assert call(clib, "f16_kalman_batch", Pm=buf, iters=buf)[0] == F16_OK
    assert call(clib, "f16_observer_step")[0] == F16_OK and call(clib, "f16_observer_step", status=None, y_out=buf)[0] == F16_OK
    for p in ("ctx", "x", "u0"):
        refused(clib, "f16_observer_step", BAD_ARGUMENT, **{p: None})
    refused(clib, "f16_observer_step", BAD_ARGUMENT, B=4, ld=3)
    for p in ("K", "dem", "u_cmd"):
        refused(clib, "f16_observer_step", "K / dem / u_cmd is NULL", **{p: None})
    for p in ("obs", "h_sigma", "xhat"):
        refused(clib, "f16_observer_step", OBS_NULL, **{p: None})
    refused(clib, "f16_observer_step", "mgroup must be 0", mgroup=65)
    refused(clib, "f16_observer_step", "sensed must be a mask", sensed=0)


# ------------------------------------------------------------------------------------------------ the Python keywords
def observer_of(B, group=0, sensed=0x7f):
    from f16_mpc_oop_py_amd.observer import Observer
    Ad, Bd, x_trim, _ = lc.model("xcg25")
    M = (B + group - 1) // group if group else 1
    return Observer.passthrough((np.tile(Ad, (M, 1, 1)), np.tile(Bd, (M, 1, 1)), np.tile(x_trim, (M, 1)), np.tile(x_trim[12:16], (M, 1))),
                                lc.SIGMA_FLIGHT, sensed=sensed, group=group)


def test_keywords_end_in_the_lqg_calls_and_the_flight_continues():
    import torch
    from f16_mpc_oop_py_amd.wind import GustModel
    B = 4
    env, obs = env_of(B), observer_of(B)
    K = torch.zeros((B, 3, 9), dtype=torch.float64)
    env.rollout_LQR(5, 0.0, 0.0, 0.0, K=K)
    assert [c[0] for c in env.lib.calls if c[0].startswith("f16_rollout")] == ["f16_rollout_lqr"]      # without observer=: today's call
    env = env_of(B)
    traj, est = env.rollout_LQR(6, 0.0, 0.0, 0.0, K=K, observer=obs, meas_seed=11, traj_every=3, method="rk4", return_estimate=True)
    assert tuple(traj.shape) == (2, 18, B) and tuple(est.shape) == (2, 9, B) and obs.row == 6
    gm = GustModel(5.0, 1750.0, 700.0, seed=3, every=2)
    env.rollout_LQR(4, 0.0, 0.0, 0.0, K=K, observer=obs, meas_seed=11, wind=[10.0, 0.0, 0.0], gusts=gm, ensemble=True)
    calls = [c for c in env.lib.calls if c[0].startswith("f16_rollout")]
    assert [c[0] for c in calls] == ["f16_rollout_lqg_wind", "f16_rollout_lqg_wind_ens"]
    for c in calls:
        assert len(c[1]) == len(names(c[0]))
    first, second = (dict(zip(names(c[0]), c[1])) for c in calls)
    assert (first["nsteps"], first["traj_every"], first["method"], first["mgroup"], first["sensed"], first["meas_seed"], first["mrow0"]) == (6, 3, 4, 0, 0x7f, 11, 0)
    assert first["h_wind"] is None and second["h_wind"] is not None and (second["mrow0"], second["nsteps"]) == (6, 4)
    assert obs.row == 10 and gm.row == 2 and first["xhat"].value == second["xhat"].value      # one flight, continued
    assert np.array_equal(np.ctypeslib.as_array((ctypes.c_double * 9).from_address(first["h_sigma"].value)), lc.SIGMA_FLIGHT)


def test_value_errors_before_any_call():
    import torch
    from f16_mpc_oop_py_amd.observer import Observer
    B = 4
    env, obs = env_of(B), observer_of(B)
    K = torch.zeros((B, 3, 9), dtype=torch.float64)
    for kw in (dict(linear=True), dict(relinearise=True, K=None), dict(schedule=object(), K=None)):
        with pytest.raises(ValueError, match="observer"):
            env.rollout_LQR(5, 0.0, 0.0, 0.0, **dict(dict(K=K, observer=obs), **kw))
    for kw in (dict(meas_seed=3), dict(return_estimate=True)):
        with pytest.raises(ValueError, match="observer"):
            env.rollout_LQR(5, 0.0, 0.0, 0.0, K=K, **kw)
    with pytest.raises(ValueError, match="meas_seed"):
        env.rollout_LQR(5, 0.0, 0.0, 0.0, K=K, observer=obs, meas_seed=-1)
    with pytest.raises(ValueError, match="models"):
        env_of(130).rollout_LQR(5, 0.0, 0.0, 0.0, K=torch.zeros((130, 3, 9), dtype=torch.float64), observer=observer_of(64, group=64))
    Ad, Bd, x_trim, _ = lc.model("xcg25")
    src = (Ad, Bd, x_trim, x_trim[12:16])
    for bad in (dict(sensed=0), dict(sensed=0x200), dict(group=32), dict(group=-64)):
        with pytest.raises(ValueError):
            Observer.passthrough(src, lc.SIGMA_FLIGHT, **bad)
    for sigma in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            Observer.passthrough(src, sigma)
    with pytest.raises(ValueError, match="variances"):
        Observer.build(src, lc.W_FLIGHT, 0.0)                                  # (refused before any GPU call)
    assert env.lib.calls == []


def test_meas_normals_draw_only_the_sensed_calls_and_share_nothing_with_the_gusts():
    from f16_mpc_oop_py_amd.observer import meas_normals
    from f16_mpc_oop_py_amd.wind import gust_normals
    full = meas_normals(99, 0xfffffffe, 6, 5)
    assert np.array_equal(meas_normals(99, 0xfffffffe, 6, 5, 0x0f)[..., :4], full[..., :4]) and not meas_normals(99, 0xfffffffe, 6, 5, 0x0f)[..., 4:].any()
    assert np.array_equal(meas_normals(99, 0xfffffffe, 2, 5), full[:2]) and np.array_equal(meas_normals(99, 0, 4, 5), full[2:])      # the counter wraps
    assert np.array_equal(meas_normals(99, 0, 4, 3), full[2:, :3]) and not np.array_equal(meas_normals(100, 0, 4, 5), full[2:])
    assert not np.isin(gust_normals(99, 0, 4, 5), full).any()
    big = meas_normals(1, 0, 400, 50)
    assert abs(big.mean()) < 0.02 and abs(big.std() - 1.0) < 0.02
