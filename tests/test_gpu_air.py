"""The moving-air derivative on the device (f16_xdot_wind_batch; calc_xdot_wind of csrc/f16_wind.hpp behind it and behind every wind,
ensemble and observer rollout) against the `long double` plant of oracle/f16_oracle.c, under the rule of tests/air_cases.py:
|device - reference| <= 8 Y[k] on every row and entry of every family, Y the fp64 restatement's own distance from the reference,
no finite row left out; the grid bits equal to the reference's on every row.  This module is the NUMERICAL pin of the wind path;
tests/test_gpu_wind.py keeps its wider bands against the numpy twin and the bit-for-bit contracts between kernels.

  1. f16_xdot_wind_batch on every family (hifi 1,414 rows, lofi 567: below and above one workgroup), always at ld = B + 3 with NaN
     padding that must neither be read nor written, once more at ld = B for the same bits; a wind or gust pointer given alone;
     the exact family's NaN pattern entry by entry, and F16_ST_NONFINITE where the header puts it: at a rollout's write-back.
  2. Three steps through f16_rollout_wind and f16_rollout_lqr_wind (hold = 2, gust_hold = 1, a sample every step; Euler and RK4; the
     interior and the 0.02 ft/s families; B = 65 and 257; default flags and F16_FLAG_ONE_LANE; through f16_rollout_wind_ens's traj;
     with gusts generated in the kernel, the rows restated by gust_reference) against f16o_rollout_wind in `long double`, the same
     8 Y rule with Y from the fp64 f16o_rollout_wind per state row: a check of the launch paths' plumbing (LDS slots, row indexing)
     at a band no wrong index survives.  The 128- and 256-lane kernels run in a child process each (F16_DYN_BLOCK is read once per
     process) under a timeout of their own; a child that fails stops the one after it.
  3. The air triple alone (f16_debug_air_triple) against 60-digit mpmath, within the budgets derived in air_cases.py.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import air_cases as ac
import rk4_cases as rk
import test_gpu_ensemble as te
from test_gpu_wind import Dev, vp

pytestmark = pytest.mark.gpu
ONE_LANE, NONFINITE = 4, 32
STEPS, HOLD, GHOLD, DT = 3, 2, 1, 0.001
S_ROWS = (STEPS + HOLD - 1) // HOLD


@pytest.fixture(scope="module")
def dev():
    return Dev()


# ------------------------------------------------------------------------------------------------ 1. one derivative
def xdot(d, fam, pad=3):
    """f16_xdot_wind_batch on the family's rows -> (xdot [B, 18], status [B]); the padding columns of out and status checked untouched"""
    c = ac.cases(fam)
    B = len(c["x"])
    ld = B + pad
    out = d.torch.full((18, ld), np.nan, dtype=d.torch.float64, device="cuda")
    st = d.torch.zeros(ld, dtype=d.torch.int32, device="cuda")
    xs, us = d.soa(c["x"], pad), d.soa(c["u"], pad)
    ws = None if c["wind_null"] else d.soa(c["air"][:, :3], pad)
    gs = None if c["gust_null"] else d.soa(c["air"][:, 3:], pad)
    flags = ac.FLAG_FIX_CLR if fam.fix_clr else 0
    d.check(d.L.f16_xdot_wind_batch(d.ctx.handle, vp(xs), vp(us), vp(ws), vp(gs), vp(out), vp(st), B, ld, fam.xcg, ac.fi_of(fam), flags, None))
    d.torch.cuda.synchronize()
    full, fst = out.cpu().numpy(), st.cpu().numpy()
    assert np.isnan(full[:, B:]).all() and (fst[B:] == 0).all()
    return d.back(out, B), fst[:B].copy()


@pytest.mark.parametrize("fam", ac.FAMILIES, ids=ac.fid)
def test_xdot_wind_within_8_y_of_the_long_double_plant(dev, fam):
    r = ac.reference(fam)
    got, st = xdot(dev, fam)
    assert np.isfinite(got).all()
    worst, bad = ac.ratios(got, fam)
    print(f"MEASURED xdot {ac.fid(fam)}: rows {len(got)}, {ac.yardstick_line(fam)}, device worst ratio {worst.max():.2f}, "
          f"per entry {' '.join(f'{w:.2f}' for w in worst)}")
    ac.check(got, fam, what="f16_xdot_wind_batch")
    assert np.array_equal(st, r["status"]), np.nonzero(st != r["status"])[0][:8]


@pytest.mark.parametrize("fam", [ac.Family("interior", "hifi"), ac.Family("gust_only", "lofi")], ids=ac.fid)
def test_xdot_wind_bits_do_not_depend_on_the_leading_dimension(dev, fam):
    a, sa = xdot(dev, fam, pad=3)
    b, sb = xdot(dev, fam, pad=0)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)


@pytest.mark.parametrize("fam", ac.EXACT, ids=ac.fid)
def test_exact_rows_nan_pattern_and_finite_entries(dev, fam):
    """vt_a == 0, Ua = Wa = 0, signed zeros, NaN wind and gust components: the device's NaN pattern is the reference's entry by entry,
    the finite entries fall under the interior family's Y; f16_xdot_wind_batch reports grid bits only"""
    r = ac.reference(fam)
    got, st = xdot(dev, fam)
    assert np.array_equal(np.isnan(got), np.isnan(r["ref"])), np.argwhere(np.isnan(got) != np.isnan(r["ref"]))[:8]
    worst = ac.check(got, fam, what="f16_xdot_wind_batch")
    print(f"MEASURED xdot {ac.fid(fam)}: NaN entries {int(np.isnan(got).sum())} as the reference's, finite entries worst ratio {worst.max():.2f}; "
          f"grid bits device {st.tolist()} reference {r['status'].tolist()}")
    assert (st & ~ac.GRID_BITS == 0).all()
    ok = np.isfinite(r["tri"].astype(np.float64)).all(1)           # rows whose air triple is a number: the grid bits are the reference's
    assert np.array_equal(st[ok], r["status"][ok])


@pytest.mark.parametrize("fam", ac.EXACT, ids=ac.fid)
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_nonfinite_is_reported_at_write_back(dev, fam, method):
    """one step of f16_rollout_wind on the exact rows: F16_ST_NONFINITE exactly on the aircraft whose state is no longer finite, and
    those are the reference's"""
    c = ac.cases(fam)
    got = te.fly(dev, c["x"], c["u"][None], method, ac.fi_of(fam), 0, c["air"][:, :3], c["air"][None, :, 3:], T=1, hold=1, ghold=1)
    ref = ac.libs()["ld"].rollout_wind(c["x"], c["u"][None], 1, 1, DT, 4 if method == "rk4" else 1, ac.fi_of(fam), wind=c["air"][:, :3],
                                       gusts=c["air"][None, :, 3:])
    bad = ~np.isfinite(got["x"]).all(1)
    assert np.array_equal(np.isnan(got["x"]), np.isnan(ref["x"])) and bad.any() and not bad.all()
    assert np.array_equal((got["st"] & NONFINITE) != 0, bad)


# ------------------------------------------------------------------------------------------------ 2. three steps through the launch paths
FLIGHTS = [(kind, fidelity, B, method, lqr) for kind, fidelity in (("interior", "hifi"), ("low_0.02", "hifi"), ("interior", "lofi"))
           for B in (65, 257) for method in ("euler", "rk4") for lqr in (False, True)]
fl_id = lambda f: f"{f[0]}-{f[1]}-{f[2]}-{f[3]}-{'lqr' if f[4] else 'open'}"
_FL = {}


def flight(key, generated=False):
    """inputs of a flight and its references: B seeded rows of the family, the family's wind, three gust rows (interior: up to 30 ft/s;
    the 0.02 ft/s family: up to 0.01, so that the first step starts at the residual), two command or demand rows.  generated: the gust
    rows are those of the in-kernel generator, restated by gust_reference"""
    if (key, generated) in _FL:
        return _FL[key, generated]
    kind, fidelity, B, method, lqr = key
    fam = ac.Family(kind, fidelity)
    c, fi = ac.cases(fam), ac.fi_of(fam)
    rng = np.random.default_rng(500 + B + fi)
    idx = np.sort(rng.permutation(len(c["x"]))[:B])
    x, u, wind = c["x"][idx], c["u"][idx], c["air"][idx, :3]
    gusts = rng.uniform(-1, 1, (STEPS, B, 3)) * (30.0 / np.sqrt(3.0) if kind == "interior" else 0.01)
    gen = None
    if generated:
        from f16_mpc_oop_py_amd.wind import gust_coefficients, gust_reference
        a, bc = gust_coefficients([8.0, 6.0, 5.0], [1750.0, 1750.0, 500.0], 600.0, GHOLD * DT)
        gen = (np.tile(a, (B, 1)), np.tile(bc, (B, 1)), rng.normal(size=(B, 3)), 77, 5)
        gusts = gust_reference(*gen, STEPS)[0]
    if lqr:
        rows, K, u0 = rng.uniform(-0.15, 0.15, (S_ROWS, B, 3)), rk.lqr_gain(), u
    else:
        rows, K, u0 = np.concatenate((u[None], rng.uniform([1000, -25, -21, -30], [19000, 25, 21, 30], (S_ROWS - 1, B, 4)))), None, None
    L = ac.libs()
    run = lambda lib: lib.rollout_wind(x, rows, STEPS, HOLD, DT, 4 if method == "rk4" else 1, fi, wind=wind, gusts=gusts, gust_hold=GHOLD,
                                       K=None if K is None else np.asarray(K).reshape(27), u0=u0)
    ref, r64 = run(L["ld"]), run(L["fp64"])
    assert np.isfinite(ref["traj"]).all() and np.array_equal(ref["status"], r64["status"]), fl_id(key)     # else: the flight is mis-built
    Y = np.abs(r64["traj"].astype(np.longdouble) - ref["traj"]).max((0, 1))
    Yu = None if not lqr else np.abs(r64["u"].astype(np.longdouble) - ref["u"]).max(0)
    _FL[key, generated] = dict(x=x, u=u, wind=wind, gusts=gusts, gen=gen, rows=rows, K=K, u0=u0, fi=fi, method=method, ref=ref, Y=Y, Yu=Yu)
    return _FL[key, generated]


def fly(d, f, flags=0, group=None, generated=False):
    return te.fly(d, f["x"], f["rows"], f["method"], f["fi"], flags, f["wind"], None if generated else f["gusts"], f["gen"] if generated else None,
                  K=f["K"], u0=f["u0"], T=STEPS, hold=HOLD, ghold=GHOLD, every=1, group=group)


def against_the_reference(key, f, got, tag):
    ref, Y = f["ref"], f["Y"]
    assert got["traj"].shape == ref["traj"].shape and np.array_equal(got["traj"][-1], got["x"])
    err = np.abs(got["traj"].astype(np.longdouble) - ref["traj"])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(Y > 0, err / np.where(Y > 0, Y, 1), 0).max((0, 1)).astype(np.float64)
    print(f"MEASURED rollout {tag} {fl_id(key)}: worst ratio {q.max():.2f}, per state {' '.join(f'{w:.2f}' for w in q)}")
    bad = ~(err <= ac.FACTOR * Y)
    assert not bad.any(), (tag, fl_id(key), np.argwhere(bad)[:6])
    assert np.array_equal(got["st"], ref["status"]), (tag, fl_id(key))
    if f["Yu"] is not None:
        assert (np.abs(got["u"].astype(np.longdouble) - ref["u"]) <= ac.FACTOR * f["Yu"]).all(), (tag, fl_id(key))


@pytest.mark.parametrize("flags", [0, ONE_LANE], ids=["default", "one_lane"])
@pytest.mark.parametrize("key", FLIGHTS, ids=fl_id)
def test_three_steps_within_8_y(dev, key, flags):
    f = flight(key)
    against_the_reference(key, f, fly(dev, f, flags), "one lane" if flags else "default")


ENS_FLIGHTS = [("interior", "hifi", 257, "rk4", False), ("low_0.02", "hifi", 65, "euler", True), ("interior", "lofi", 257, "rk4", True)]


@pytest.mark.parametrize("key", ENS_FLIGHTS, ids=fl_id)
def test_three_steps_through_the_ensemble_entry(dev, key):
    f = flight(key)
    got = fly(dev, f, 0, group=64)
    against_the_reference(key, f, got, "ensemble traj")
    assert int(got["ens"]["count"].sum()) > 0


@pytest.mark.parametrize("flags", [0, ONE_LANE], ids=["default", "one_lane"])
@pytest.mark.parametrize("key", [("interior", "hifi", 257, "rk4", False), ("interior", "lofi", 65, "euler", True)], ids=fl_id)
def test_three_steps_with_gusts_generated_in_the_kernel(dev, key, flags):
    f = flight(key, generated=True)
    against_the_reference(key, f, fly(dev, f, flags, generated=True), "generated gusts")


_DEAD = []


@pytest.mark.parametrize("block", [128, 256])
def test_three_steps_on_wider_workgroups(tmp_path, block):
    """k_rollout_wind<128, ..> and <256, ..> (F16_DYN_BLOCK in a child process): the same flights, the same rule"""
    if _DEAD:
        pytest.fail(f"not started: {_DEAD[0]}")
    out = str(tmp_path / "a.npz")
    env = dict(os.environ, F16_DYN_BLOCK=str(block))
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _DEAD.append(f"the child for {block} lanes did not finish in 120 s")
        pytest.fail(_DEAD[0])
    if p.returncode != 0:
        _DEAD.append(f"the child for {block} lanes ended with status {p.returncode}: {p.stderr[-2000:]}")
        pytest.fail(_DEAD[0])
    with np.load(out) as z:
        for key in FLIGHTS:
            got = {k: (z[f"{fl_id(key)}/{k}"] if f"{fl_id(key)}/{k}" in z.files else None) for k in ("x", "traj", "st", "u")}
            against_the_reference(key, flight(key), got, f"{block} lanes")


def child_main(out):
    import conftest  # noqa: F401  (puts the repository root on sys.path)
    d, res = Dev(), {}
    for key in FLIGHTS:
        got = fly(d, flight(key))
        res.update({f"{fl_id(key)}/{k}": got[k] for k in ("x", "traj", "st", "u") if got[k] is not None})
    np.savez(out, **res)


# ------------------------------------------------------------------------------------------------ 3. the air triple alone
def test_air_triple_against_mpmath(dev):
    """f16_debug_air_triple on air_cases.triple_cases(): Ua, Va, Wa within the derived rounding budget of the rule at 60 digits; the
    root within its budget, atan2 and asin within the host libm's own error + 2 ulp, each judged on the device's own Ua, Va, Wa"""
    in12 = ac.triple_cases()
    n = in12.shape[1]
    out = np.full((6, n), np.nan)
    hp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    dev.check(dev.L.f16_debug_air_triple(dev.ctx.handle, hp(in12), n, hp(out)))
    fig = ac.triple_figures(in12, out)
    for k, (worst, bound) in fig.items():
        print(f"MEASURED air triple, device, {k}: {worst:.3f} of {bound:.3f} ({n} cases)")
    for k, (worst, bound) in fig.items():
        assert worst <= bound, k
    assert dev.L.f16_debug_air_triple(dev.ctx.handle, hp(in12), 0, hp(out)) == 0
    assert dev.L.f16_debug_air_triple(dev.ctx.handle, None, n, hp(out)) == -1


if __name__ == "__main__":
    child_main(sys.argv[1])
