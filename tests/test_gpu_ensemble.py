"""Ensemble statistics inside the launch (f16_rollout_wind_ens, f16_rollout_lqr_wind_ens, f16_ens_from_traj) on the device, against
f16_mpc_oop_py_amd.ensemble.ensemble_reference -- the rule of include/f16_hip.h in numpy, itself held to exact rational arithmetic
by tests/test_ensemble_cpu.py -- and against their own contracts.  The statistics are compared for EQUALITY (np.array_equal: counts
equal, the other four numerically equal, no NaN anywhere; the sign of a zero minimum or maximum is not specified).

Shapes follow tests/test_gpu_wind.py: 40 steps, hold = 7, gust_hold = 3, ld = B + 3 with the padding columns NaN, the batches of
tests/wind_cases.py, gusts generated in the kernel; samples every step and every 5 steps; B = 1, 65, 257; group = 64, 128.  A few
aircraft of every batch with B > 1 are overwritten: one outside the box from step 0, one with a NaN state, and one whole group of
such aircraft -- at B = 257 the 64 aircraft 64..127, at B = 65 the (short) last group, aircraft 64 -- so that a count is 0, and the
reference is asserted to hold groups with 0 < count < group.  The 128- and 256-lane kernels run in a child process each
(F16_DYN_BLOCK is read once per process), one after another under a timeout of their own; a child that fails stops the ones after it.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import envelope_cases as ec
import rk4_cases as rk
import test_gpu_wind as tw
import wind_cases as wc
from test_gpu_wind import Dev, vp

pytestmark = pytest.mark.gpu
ONE_LANE, NO_ENVELOPE = 4, 2
T, HOLD, GHOLD, DT = tw.T, tw.HOLD, tw.GHOLD, tw.DT
KEYS = ("count", "mean", "m2", "min", "max")
# (fidelity, method, LQR law): both methods, hifi and lofi, both entries
FLIGHTS = {"hifi_rk4": (1, "rk4", False), "hifi_euler": (1, "euler", False), "hifi_lqr_rk4": (1, "rk4", True), "lofi_lqr_euler": (0, "euler", True),
           "lofi_rk4": (0, "rk4", False)}


@pytest.fixture(scope="module")
def dev():
    return Dev()


# ------------------------------------------------------------------------------------------------ calling the library
def ens_buffers(d, B, S, group):
    """(lib.Ens, its tensors): ldg = G + 1, the padding column a sentinel that must survive"""
    torch = d.torch
    G = (B + group - 1) // group
    ldg = G + 1
    n = d.L.f16_ens_work_doubles(B, S)
    assert n == 73 * ((B + 63) // 64) * S
    t = dict(work=torch.full((max(n, 1),), np.nan, dtype=torch.float64, device="cuda"),
             count=torch.full((S, ldg), -7, dtype=torch.int32, device="cuda"))
    for k in KEYS[1:]:
        t[k] = torch.full((S, 18, ldg), 12345.0, dtype=torch.float64, device="cuda")
    e = d.libm.Ens()
    e.group, e.ldg = group, ldg
    for k, v in t.items():
        setattr(e, k, v.data_ptr())
    return e, t, G


def ens_back(t, G):
    """the device results as the reference shapes them: count [S, G], the others [S, G, 18]; the padding column untouched"""
    c = t["count"].cpu().numpy()
    assert (c[:, G:] == -7).all()
    out = dict(count=c[:, :G].copy())
    for k in KEYS[1:]:
        v = t[k].cpu().numpy()
        assert (v[:, :, G:] == 12345.0).all()
        out[k] = v[:, :, :G].transpose(0, 2, 1).copy()
    return out


def fly(d, x0, rows, method, fi, flags=0, wind=None, gusts=None, gen=None, K=None, u0=None, T=T, hold=HOLD, ghold=GHOLD, every=1, status0=None,
        group=None, keep_traj=True, still=False):
    """one call of f16_rollout_wind[_ens] / f16_rollout_lqr_wind[_ens] (K given; group given: the _ens entry) on the arrays of
    tests/test_gpu_wind.py `fly` -> its dict plus ens = dict(count [S, G], mean, m2, min, max [S, G, 18]) or None"""
    torch, B = d.torch, len(x0)
    ld = B + 3
    x, seq = d.soa(x0), d.soa(rows)
    st = torch.zeros(ld, dtype=torch.int32, device="cuda")
    if status0 is not None:
        st[:B] = torch.as_tensor(np.asarray(status0, dtype=np.int32)).cuda()
    traj = torch.full((T // every, 18, ld), np.nan, dtype=torch.float64, device="cuda") if keep_traj else None
    air, keep = d.libm.Wind(), []
    if wind is not None:
        keep.append(d.soa(wind)); air.wind_ned = keep[-1].data_ptr()
    if gusts is not None:
        keep.append(d.soa(gusts)); air.gust_seq, air.gust_hold = keep[-1].data_ptr(), ghold
    gs = None
    if gen is not None:
        ga, gb, gs = d.soa(gen[0]), d.soa(gen[1]), d.soa(gen[2])
        keep += [ga, gb]
        air.ga, air.gb, air.gstate, air.gust_hold, air.seed, air.row0 = ga.data_ptr(), gb.data_ptr(), gs.data_ptr(), ghold, gen[3], gen[4]
    h = None if still else ctypes.byref(air)
    tail = (B, ld, T, hold, every, DT, wc.XCG, fi, tw.METHOD[method], flags, None)
    e = t = G = None
    if group is not None:
        e, t, G = ens_buffers(d, B, T // every, group)
    extra = () if group is None else (ctypes.byref(e),)
    sfx = "" if group is None else "_ens"
    if K is None:
        uo = None
        d.check(getattr(d.L, "f16_rollout_wind" + sfx)(d.ctx.handle, vp(x), vp(seq), h, vp(traj), *extra, vp(st), *tail))
    else:
        Kd, u0d = d.soa(np.broadcast_to(np.asarray(K).reshape(1, 27), (B, 27))), d.soa(u0)
        uo = torch.full((4, ld), np.nan, dtype=torch.float64, device="cuda")
        d.check(getattr(d.L, "f16_rollout_lqr_wind" + sfx)(d.ctx.handle, vp(x), vp(u0d), vp(Kd), vp(seq), h, vp(traj), *extra, vp(uo), vp(st), *tail))
    torch.cuda.synchronize()
    return dict(x=d.back(x, B), traj=None if traj is None else d.back(traj, B), st=st.cpu().numpy()[:B].copy(),
                u=None if uo is None else d.back(uo, B), gstate=None if gs is None else d.back(gs, B),
                ens=None if group is None else ens_back(t, G), traj_dev=traj)


def from_traj(d, traj_dev, B, group, flags=0):
    """f16_ens_from_traj of a device trajectory [S, 18, ld]"""
    S, _, ld = traj_dev.shape
    e, t, G = ens_buffers(d, B, S, group)
    d.check(d.L.f16_ens_from_traj(d.ctx.handle, vp(traj_dev), S, B, ld, flags, ctypes.byref(e), None))
    d.torch.cuda.synchronize()
    return ens_back(t, G)


def reference(traj, group, flags=0):
    """ensemble_reference of a host trajectory [S, B, 18] as the dict of ens_back"""
    from f16_mpc_oop_py_amd.ensemble import ensemble_reference
    r = ensemble_reference(np.ascontiguousarray(traj.transpose(0, 2, 1)), group, envelope=not flags & NO_ENVELOPE)
    return dict(zip(KEYS, r.parts()))


def equal(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape and not np.isnan(a[k]).any(), (what, k)
        assert np.array_equal(a[k], b[k]), (what, k, np.argwhere(a[k] != b[k])[:4])


# ------------------------------------------------------------------------------------------------ the cases
def case(name, B):
    """(x0 [B, 18], rows, method, fi, wind, gen, K, u0) of a named flight at B aircraft, with the overwritten aircraft of the head"""
    from f16_mpc_oop_py_amd.wind import gust_coefficients
    fi, method, lqr = FLIGHTS[name]
    b = wc.subset(fi, B)
    x0 = b.x.copy()
    if B > 1:
        bad = [3, 7] + list(range(64, min(128, B)))
        for j, i in enumerate(bad):
            if j % 2 == 0:
                x0[i, 6] = -10.0                  # outside the box from step 0: frozen, never contributes
            else:
                x0[i, 4] = np.nan                 # a NaN state: every state NaN after one step
    w, _ = wc.air(B, B + fi)
    a, bc = gust_coefficients([8.0, 6.0, 5.0], [1750.0, 1750.0, 500.0], 600.0, GHOLD * DT)
    gen = (np.tile(a, (B, 1)), np.tile(bc, (B, 1)), np.random.default_rng(3).normal(size=(B, 3)), 77, 5)
    S = (T + HOLD - 1) // HOLD
    if lqr:
        return x0, np.random.default_rng(B).uniform(-0.15, 0.15, (S, B, 3)), method, fi, w, gen, rk.lqr_gain(), b.u
    return x0, np.random.default_rng(B + 1).uniform([0, -30, -25, -35], [20000, 30, 25, 35], (S, B, 4)), method, fi, w, gen, None, None


def check_flight(d, name, flags, sizes=(1, 65, 257)):
    """contracts 1 to 4 of one flight at every B, sample period and group size"""
    for B in sizes:
        x0, rows, method, fi, w, gen, K, u0 = case(name, B)
        kw = dict(wind=w, gen=gen, K=K, u0=u0)
        for every in (1, 5):
            sib = fly(d, x0, rows, method, fi, flags, every=every, **kw)
            for group in (64, 128):
                tag = (name, flags, B, every, group)
                got = fly(d, x0, rows, method, fi, flags, every=every, group=group, **kw)
                ref = reference(got["traj"], group)
                # 1. the statistics of the call are the reference's of the samples of the same call
                equal(got["ens"], ref, tag + ("reference",))
                if B > 1:
                    gsz = np.minimum(group, B - group * np.arange(ref["count"].shape[1]))
                    assert (group != 64 or (ref["count"] == 0).any()) and ((ref["count"] > 0) & (ref["count"] < gsz)).any(), tag
                    assert ref["count"].max() > 1 and (ref["m2"] > 0).any()
                # 2. ... and f16_ens_from_traj's of those samples, bit for bit
                equal(from_traj(d, got["traj_dev"], B, group), got["ens"], tag + ("from_traj",))
                # 4. without traj the same statistics, the same final state
                bare = fly(d, x0, rows, method, fi, flags, every=every, group=group, keep_traj=False, **kw)
                equal(bare["ens"], got["ens"], tag + ("traj = NULL",))
                assert tw.same(bare, got, ("x", "st", "u", "gstate")), tag
                # 3. under F16_FLAG_ONE_LANE everything else is the sibling's, bit for bit (default flags: test_default_flags_...)
                if flags & ONE_LANE:
                    assert tw.same(got, sib), tag


# ------------------------------------------------------------------------------------------------ 1 - 4
@pytest.mark.parametrize("flags", [0, ONE_LANE])
@pytest.mark.parametrize("name", list(FLIGHTS))
def test_statistics_equal_the_reference_of_the_same_samples(dev, name, flags):
    check_flight(dev, name, flags)


_DEAD = []


@pytest.mark.parametrize("block", [128, 256])
def test_wider_workgroups(block):
    """k_rollout_wind_ens<128, ..> and <256, ..> (F16_DYN_BLOCK in a child process): the same checks, default flags"""
    if _DEAD:
        pytest.fail(f"not started: {_DEAD[0]}")
    env = dict(os.environ, F16_DYN_BLOCK=str(block))
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _DEAD.append(f"the child for {block} lanes did not finish in 120 s")
        pytest.fail(_DEAD[0])
    if p.returncode != 0 or "CHILD OK" not in p.stdout:
        _DEAD.append(f"the child for {block} lanes ended with status {p.returncode}: {p.stdout[-1000:]} {p.stderr[-3000:]}")
        pytest.fail(_DEAD[0])


def child_main():
    import conftest  # noqa: F401  (puts the repository root on sys.path)
    d = Dev()
    for name in FLIGHTS:
        check_flight(d, name, 0, sizes=(65, 257))
    print("CHILD OK")


def test_no_envelope_flag_counts_every_finite_aircraft(dev):
    """F16_FLAG_NO_ENVELOPE: nothing freezes and the mask is finiteness alone -- the aircraft that start outside the box contribute"""
    x0, rows, method, fi, w, gen, K, u0 = case("hifi_euler", 257)
    with_box = fly(dev, x0, rows, method, fi, 0, wind=w, gen=gen, group=64)
    got = fly(dev, x0, rows, method, fi, NO_ENVELOPE, wind=w, gen=gen, group=64)
    equal(got["ens"], reference(got["traj"], 64, NO_ENVELOPE), "no envelope")
    equal(from_traj(dev, got["traj_dev"], 257, 64, NO_ENVELOPE), got["ens"], "no envelope, from_traj")
    assert (got["ens"]["count"] >= with_box["ens"]["count"]).all() and with_box["ens"]["count"][0, 1] == 0 and got["ens"]["count"][0, 1] > 0


# ------------------------------------------------------------------------------------------------ 3. default flags against the sibling
@pytest.mark.parametrize("name", tw.FLIGHTS)
def test_default_flags_agree_with_the_sibling_within_the_band_of_the_wind_suite(oracle, dev, name):
    """the flights of tests/test_gpu_wind.py as they are (supplied gusts): final state, samples and u_out of the _ens call against the
    sibling call within ROLLOUT_TOL widened by the twin's reconstruction error, at the states_ok aircraft of the twin's record -- the
    band and the set test_gpu_wind.py uses between kernels; status words equal where status_ok.  (An inlined step's contraction
    follows its surroundings, so bits are promised under F16_FLAG_ONE_LANE only.)"""
    b, rows, method, w, g, K, u0 = tw.flight(name)
    sib = tw.fly(dev, b.x, rows, method, b.fi, 0, w, g, K=K, u0=u0)
    got = fly(dev, b.x, rows, method, b.fi, 0, wind=w, gusts=g, K=K, u0=u0, group=64)
    r = tw.twin(oracle, name)
    ok, okst = r["states_ok"], r["status_ok"]
    tol = wc.band(tw.ROLLOUT_TOL, wc.reconstruction_error(oracle, b))
    err = np.maximum(ec.rel(got["traj"], sib["traj"]).max((0, 2)), ec.rel(got["x"], sib["x"]).max(1))
    if K is not None:
        err = np.maximum(err, ec.rel(got["u"], sib["u"]).max(1))
    print(f"MEASURED {name}: largest difference from the sibling {err[ok].max():.2e}, / band {(err[ok] / tol[ok]).max():.2e}, "
          f"bit-identical: {tw.same(got, sib, ('x', 'traj', 'st', 'u'))}")
    assert ok.mean() >= 0.9 and (err[ok] < tol[ok]).all()
    assert np.array_equal(got["st"][okst], sib["st"][okst])
    equal(got["ens"], reference(got["traj"], 64), name)


def test_null_wind_is_zero_air_through_the_wind_kernels(dev):
    """a NULL h_wind and one with NULL pointers: the bits of f16_rollout_wind with a zero wind_ned under F16_FLAG_ONE_LANE -- not the
    still-air kernel's"""
    x0, rows, method, fi, _, _, _, _ = case("hifi_rk4", 65)
    zero = tw.fly(dev, x0, rows, method, fi, ONE_LANE, np.zeros((65, 3)))
    for still in (True, False):
        got = fly(dev, x0, rows, method, fi, ONE_LANE, group=64, still=still)
        assert tw.same(got, zero, ("x", "traj", "st")), still
        equal(got["ens"], reference(got["traj"], 64), "zero air")


# ------------------------------------------------------------------------------------------------ 5. a lane's second pass
def big_case(B, fi, seed):
    b = wc.subset(fi, 257)
    idx = np.arange(B) % 257
    x0 = b.x[idx].copy()
    x0[:, 2] += np.random.default_rng(seed).uniform(0.0, 50.0, B)          # (altitude: no two aircraft alike)
    x0[5::1000, 6] = -10.0
    x0[7::1000, 4] = np.nan
    x0[640:704] = x0[5]                                                      # a whole wave outside: the first half of group 5
    x0[B - 1] = x0[7]                                                        # and the last aircraft of the second pass NaN
    from f16_mpc_oop_py_amd.wind import gust_coefficients
    a, bc = gust_coefficients([8.0, 6.0, 5.0], [1750.0, 1750.0, 500.0], 600.0, DT)
    gen = (np.tile(a, (B, 1)), np.tile(bc, (B, 1)), np.zeros((B, 3)), 5, 0)
    return x0, b.u[idx][None].copy(), wc.air(B, seed)[0], gen


@pytest.mark.parametrize("B,flags,method,steps,every", [(65601, 0, "euler", 4, 2), (262209, ONE_LANE, "euler", 2, 1)])
def test_a_lanes_second_pass_over_the_grid(dev, B, flags, method, steps, every):
    """B = 65,601 on the natural 256-lane geometry: 257 workgroups of aircraft on a grid of 256, so workgroup 0 comes round again
    with 65 aircraft -- one full wave, one wave with a single lane, two waves with none, which must leave together.  B = 262,209
    under F16_FLAG_ONE_LANE: 4,098 waves on a grid of 4,096.  Both against the reference of their own samples, and the second
    against the sibling bit for bit."""
    x0, rows, w, gen = big_case(B, 1, B)
    got = fly(dev, x0, rows, method, 1, flags, wind=w, gen=gen, T=steps, hold=steps, ghold=1, every=every, group=128)
    ref = reference(got["traj"], 128)
    equal(got["ens"], ref, B)
    assert (ref["count"][:, 5] > 0).all() and (ref["count"][:, 5] <= 64).all() and 0 < ref["count"][0, -1] <= 64      # (the last group: 65 aircraft)
    equal(from_traj(dev, got["traj_dev"], B, 128), got["ens"], (B, "from_traj"))
    if flags & ONE_LANE:
        assert tw.same(got, tw.fly(dev, x0, rows, method, 1, flags, w, gen=gen, T=steps, hold=steps, ghold=1, every=every))


# ------------------------------------------------------------------------------------------------ 6. two calls against one
@pytest.mark.parametrize("flags", [0, ONE_LANE])
@pytest.mark.parametrize("name", ["hifi_rk4", "lofi_lqr_euler"])
def test_two_calls_concatenate_to_one(dev, name, flags):
    """n steps then m steps against n + m, n a multiple of hold, gust_hold and the sample period: (hold, gust_hold, period, n) =
    (7, 3, 1, 21) and (5, 5, 5, 20).  The samples' statistics concatenate bit for bit, and so does everything else."""
    x0, rows, method, fi, w, gen, K, u0 = case(name, 257)
    rows = np.concatenate((rows, rows[::-1]))                                # (eight rows at hold = 5)
    for hold, ghold, every, n in ((HOLD, GHOLD, 1, 21), (5, 5, 5, 20)):
        kw = dict(wind=w, K=K, u0=u0, hold=hold, ghold=ghold, every=every, group=128)
        one = fly(dev, x0, rows, method, fi, flags, gen=gen, **kw)
        first = fly(dev, x0, rows, method, fi, flags, gen=gen, T=n, **kw)
        gen2 = gen[:2] + (first["gstate"], gen[3], gen[4] + n // ghold)
        second = fly(dev, first["x"], rows[n // hold:], method, fi, flags, gen=gen2, T=T - n, status0=first["st"], **kw)
        assert tw.same(one, dict(second, traj=np.concatenate((first["traj"], second["traj"])))), (name, hold)
        both = {k: np.concatenate((first["ens"][k], second["ens"][k])) for k in KEYS}
        for k in KEYS:
            assert np.array_equal(both[k], one["ens"][k]), (name, hold, k)


# ------------------------------------------------------------------------------------------------ the Python keywords
def test_python_keywords_reach_the_ensemble_calls(dev):
    """F16Batch.rollout_schedule / rollout_LQR with ensemble= equal the C calls; ensemble=True is one group; keep_traj returns both"""
    from f16_mpc_oop_py_amd import F16Batch
    from f16_mpc_oop_py_amd.ensemble import Ensemble
    x0, rows, method, fi, w, _, _, _ = case("hifi_euler", 257)
    b = wc.subset(1, 257)
    g = wc.air(257, 9, rows=(T + GHOLD - 1) // GHOLD)[1]
    env = F16Batch(x0, b.u, xcg=wc.XCG, dt=DT, context=dev.ctx)
    traj, e = env.rollout_schedule(rows, hold=HOLD, nsteps=T, traj_every=5, method=method, wind=w, gusts=g, gust_every=GHOLD, ensemble=128,
                                   keep_traj=True)
    want = fly(dev, x0, rows, method, 1, 0, wind=w, gusts=g, every=5, group=128)
    assert isinstance(e, Ensemble) and np.array_equal(traj.cpu().numpy().transpose(0, 2, 1), want["traj"], equal_nan=True)
    equal(dict(zip(KEYS, e.numpy().parts())), want["ens"], "rollout_schedule")
    var = e.var.cpu().numpy()
    assert np.array_equal(np.isnan(var), np.broadcast_to(want["ens"]["count"][..., None] < 2, var.shape))
    env = F16Batch(x0, b.u, xcg=wc.XCG, dt=DT, context=dev.ctx)
    e = env.rollout_schedule(rows, hold=HOLD, nsteps=T, traj_every=5, method=method, wind=w, gusts=g, gust_every=GHOLD, ensemble=True)
    equal(dict(zip(KEYS, e.numpy().parts())), reference(want["traj"], 320), "one group")
    import torch
    K = torch.as_tensor(np.broadcast_to(rk.lqr_gain(), (257, 3, 9)).copy())
    lq = F16Batch(x0, b.u, xcg=wc.XCG, dt=DT, context=dev.ctx)
    e = lq.rollout_LQR(T, 0.05, -0.02, 0.01, K=K, method="rk4", wind=w, gusts=g, gust_every=GHOLD, ensemble=64)
    dem = np.broadcast_to(np.array([0.05, -0.02, 0.01]), (1, 257, 3))
    want = fly(dev, x0, dem, "rk4", 1, 0, wind=w, gusts=g, K=rk.lqr_gain(), u0=b.u, hold=T, group=64)
    equal(dict(zip(KEYS, e.numpy().parts())), want["ens"], "rollout_LQR")
    assert np.array_equal(lq.x_values.cpu().numpy(), want["x"], equal_nan=True)


if __name__ == "__main__":
    child_main()
