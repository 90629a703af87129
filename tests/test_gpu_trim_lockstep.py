"""f16_trim_batch (csrc/f16_trim.hip) held to scipy's Nelder-Mead STEP BY STEP over the first N_LOCK iterations, through the public C
ABI: `maxiter` stops the launch after any number of iterations and `h_x0` sets the start (tests/trim_cases.py has the restatement,
the cases, the cost band and the vertex yardstick; tests/test_trim_cpu.py shows on the CPU that the restatement is scipy's, that the
cases take every branch and that every decision on their paths is made with 100 cost bands to spare).

maxiter = n + 1 performs n iterations (scipy's counter starts at 1: include/f16_hip.h).  Every launch is at most N_LOCK iterations of
a few conditions -- the kernel's loop is bounded by maxiter, nothing here waits on a child process -- and after a launch that
failed no further launch is made.  All calls go with ld = B + 3 into arrays pre-filled with NaN / a sentinel; the padding must come
back untouched."""
import ctypes

import numpy as np
import pytest
import torch

import trim_cases as tc

pytestmark = pytest.mark.gpu

EPS = tc.EPS
PAD = 3
SENT = -777
FOREIGN = 1 << 30                       # a status bit no kernel sets: it must survive the call (status is OR-ed into)
QP_MAXITER = 64                         # F16_ST_QP_MAXITER
NS = list(range(1, tc.N_LOCK + 1))
_STATE = dict(failed=None)
_RUNS = {}


@pytest.fixture(scope="module")
def ctx():
    from f16_mpc_oop_py_amd import lib
    assert lib.F16_ST["QP_MAXITER"] == QP_MAXITER
    c = lib.Context(0)
    yield c
    c.close()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def launch(ctx, x0, fi, xcg, h, v, maxiter, optional=True):
    """one f16_trim_batch call, ld = B + 3, status pre-set to FOREIGN -> dict(x [B, 18], cost, iters, nfev, status [B]); the padding
    columns, the entries beyond B and a sentinel row below x_trim are checked here"""
    from f16_mpc_oop_py_amd import lib
    if _STATE["failed"]:
        pytest.fail("no launch after a failed one: " + _STATE["failed"])
    B, dev = len(h), "cuda:0"
    ld = B + PAD
    hd, vd = torch.as_tensor(np.asarray(h, dtype=np.float64), device=dev), torch.as_tensor(np.asarray(v, dtype=np.float64), device=dev)
    xt = torch.full((19, ld), np.nan, dtype=torch.float64, device=dev)
    cost = torch.full((ld,), np.nan, dtype=torch.float64, device=dev) if optional else None
    iters, nfev, st = (torch.full((ld,), SENT, dtype=torch.int32, device=dev) if optional else None for _ in range(3))
    if optional:
        st[:B] = FOREIGN
    hx0 = np.ascontiguousarray(x0, dtype=np.float64) if x0 is not None else None
    try:
        lib.check(ctx.lib.f16_trim_batch(ctx.handle, _vp(hd), _vp(vd), _vp(xt), _vp(cost), _vp(iters), _vp(nfev), _vp(st), B, ld, float(xcg),
                                         int(fi), 0, int(maxiter), ctypes.c_void_p(hx0.ctypes.data) if hx0 is not None else None, None), ctx.lib)
        torch.cuda.synchronize()
    except Exception as e:
        _STATE["failed"] = repr(e)
        raise
    x = xt.cpu().numpy()
    assert np.isnan(x[:18, B:]).all() and np.isnan(x[18]).all(), "x_trim: padding columns or the row beyond were written"
    out = dict(x=x[:18, :B].T.copy())
    if optional:
        c, it, nf, s = cost.cpu().numpy(), iters.cpu().numpy(), nfev.cpu().numpy(), st.cpu().numpy()
        assert np.isnan(c[B:]).all() and (it[B:] == SENT).all() and (nf[B:] == SENT).all() and (s[B:] == SENT).all(), "entries beyond B written"
        assert np.all(s[:B] & FOREIGN), "status is OR-ed into: a bit set before the call survives it"
        out.update(cost=c[:B], iters=it[:B], nfev=nf[:B], status=s[:B] & ~FOREIGN)
    return out


def runs(ctx, g):
    """the group's launches for n = 1 .. N_LOCK iterations, once per process: [n - 1] = launch(maxiter = n + 1)"""
    if g not in _RUNS:
        grp = tc.CASES[g]
        _RUNS[g] = [launch(ctx, grp.x0, grp.fi, grp.xcg, grp.h, grp.v, n + 1) for n in NS]
    return _RUNS[g]


GROUPS = [pytest.param(g, id=grp.name) for g, grp in enumerate(tc.CASES)]


@pytest.mark.parametrize("g", GROUPS)
def test_cost_function_at_the_returned_point(ctx, oracle, g):
    """Independent of the path: the device's cost is the oracle's objective AT THE POINT THE DEVICE RETURNED, within that point's cost
    band -- both temperature branches, both fidelities, clipped and unclipped commands, alpha beyond its clip -- and the other
    entries of x_trim follow env.py:275-290."""
    grp, worst, worst_flap = tc.CASES[g], 0.0, 0.0
    for n, r in zip(NS, runs(ctx, g)):
        for b in range(len(grp.h)):
            x, h, v = r["x"][b], grp.h[b], grp.v[b]
            q = x[[12, 13, 14, 15, 7]]
            assert np.isfinite(x).all() and np.isfinite(r["cost"][b])
            c = tc.trim_cost(oracle, q, h, v, grp.fi, grp.xcg)
            worst = max(worst, abs(r["cost"][b] - c.cost) / c.band)
            assert abs(r["cost"][b] - c.cost) <= c.band, (grp.name, n, b, r["cost"][b], c.cost, c.band)
            ref, terms = tc.x_trim_of(q, h, v)
            assert x[2] == h and x[6] == v and x[4] == x[7]
            assert np.all(x[[0, 1, 3, 5, 8, 9, 10, 11]] == 0.0)
            assert abs(x[17] - ref[17]) <= 2 * EPS * abs(ref[17])           # one product, one quotient
            flap = 16 * EPS * sum(abs(t) for t in terms)
            worst_flap = max(worst_flap, abs(x[16] - ref[16]) / flap)
            assert abs(x[16] - ref[16]) <= flap, (grp.name, n, b, x[16], ref[16])
    print(f"trim lockstep {grp.name}: device cost vs oracle at the returned point, largest error {worst:.3g} of its band; "
          f"flap {worst_flap:.3g} of 16 eps of its terms")


@pytest.mark.parametrize("g", GROUPS)
def test_lockstep_with_scipy(ctx, oracle, g):
    """After n iterations, n = 1 .. N_LOCK: iters = n + 1, nfev and the F16_ST_QP_MAXITER bit as scipy has them, the best vertex within
    the yardstick's allowance of the restatement's, its cost within the cost band; the nfev increments 1 / 2 / 7 are those of the
    restated branch.  A failure names the first n at which a condition departs and the branch the restatement took there."""
    grp, rs = tc.CASES[g], runs(ctx, g)
    departed, worst_v, worst_c = [], 0.0, 0.0
    for b in range(len(grp.h)):
        rec = tc.path(oracle, g, b)
        yard, scale = tc.vertex_yardstick(rec, grp.x0)
        prev = 6
        for n, r in zip(NS, rs):
            what = []
            best = r["x"][b][[12, 13, 14, 15, 7]]
            allow = tc.vertex_allowance(yard[n], scale)
            dv = np.abs(best - rec[n]["sim"][0])
            dc = abs(r["cost"][b] - rec[n]["fsim"][0]) / rec[n]["band"][0]
            if r["iters"][b] != n + 1:
                what.append(f"iters {r['iters'][b]} != {n + 1}")
            if r["nfev"][b] != rec[n]["nfev"]:
                what.append(f"nfev {r['nfev'][b]} != {rec[n]['nfev']}")
            if r["nfev"][b] - prev != tc.NFEV_OF[rec[n]["branch"]]:
                what.append(f"nfev increment {r['nfev'][b] - prev} != {tc.NFEV_OF[rec[n]['branch']]}")
            if not r["status"][b] & QP_MAXITER:
                what.append("F16_ST_QP_MAXITER not set (scipy: status 2)")
            if not np.all(dv <= allow):
                what.append(f"best vertex off by {dv} (allowed {allow})")
            if not dc <= 1.0:
                what.append(f"cost off by {dc:.3g} bands")
            if what:
                departed.append(f"{grp.name}[{b}] h {grp.h[b]} V {grp.v[b]}: first departs at n = {n}, restated branch {rec[n]['branch']}: "
                                + "; ".join(what))
                break
            prev = r["nfev"][b]
            worst_v, worst_c = max(worst_v, float((dv / allow).max())), max(worst_c, dc)
    print(f"trim lockstep {grp.name}: best vertex vs restatement, largest error {worst_v:.3g} of its allowance "
          f"(max(16 yardstick, 64 eps scale)); cost {worst_c:.3g} of its band")
    assert not departed, "\n".join(departed)


def test_a_launch_capped_before_its_first_iteration(ctx, oracle):
    """maxiter = 1: scipy's loop does not run -- the sorted initial simplex, nit = 1, nfev = 6, status 2"""
    grp = tc.CASES[0]
    r = launch(ctx, grp.x0, grp.fi, grp.xcg, grp.h, grp.v, 1)
    for b in range(len(grp.h)):
        rec = tc.path(oracle, 0, b)[0]
        assert r["iters"][b] == 1 and r["nfev"][b] == 6 and r["status"][b] & QP_MAXITER
        assert np.array_equal(r["x"][b][[12, 13, 14, 15, 7]], rec["sim"][0])


# ------------------------------------------------------------------------------------------------ launch geometry
GEO_G, GEO_N = 2, 8                     # a hifi group (the workgroup stages the table image in LDS once, then strides)


def _same(a, b, idx):
    return all(np.array_equal(a[k], b[k][idx]) for k in ("x", "cost", "iters", "nfev", "status"))


@pytest.mark.parametrize("B", [1, 3, 5, 67, 16384 + 24])
def test_every_aircraft_of_a_tiled_batch_equals_its_case_bit_for_bit(ctx, B):
    """B = 1, 3, 5, 67: wavefronts whose rows are partly invalid and share one loop exit; B = 16,384 + 24: the grid is capped at
    1024 workgroups of 16 conditions, so 24 conditions are a second pass of workgroups whose table image is already loaded"""
    grp = tc.CASES[GEO_G]
    small = runs(ctx, GEO_G)[GEO_N - 1]
    idx = np.arange(B) % len(grp.h)
    big = launch(ctx, grp.x0, grp.fi, grp.xcg, np.array(grp.h)[idx], np.array(grp.v)[idx], GEO_N + 1)
    assert _same(big, small, idx)


def test_null_optional_outputs(ctx):
    grp = tc.CASES[GEO_G]
    r = launch(ctx, grp.x0, grp.fi, grp.xcg, grp.h, grp.v, GEO_N + 1, optional=False)
    assert np.array_equal(r["x"], runs(ctx, GEO_G)[GEO_N - 1]["x"])


def test_the_python_call_equals_the_c_call(ctx):
    """F16Batch.trim(h, v, maxiter=n) is the C call with the reference's start (h_x0 = NULL) and ld = B"""
    from f16_mpc_oop_py_amd import F16Batch
    g = 0
    grp = tc.CASES[g]
    assert grp.x0 == tc.X0_REF
    for n in (1, GEO_N + 1, tc.N_LOCK + 1):
        x, info = F16Batch.trim(grp.h, grp.v, xcg=grp.xcg, fi_flag=grp.fi, maxiter=n, context=ctx)
        c = launch(ctx, None, grp.fi, grp.xcg, grp.h, grp.v, n)
        assert np.array_equal(x.cpu().numpy(), c["x"])
        for k in ("cost", "iters", "nfev", "status"):
            assert np.array_equal(info[k].cpu().numpy(), c[k]), k
        if n > 1:
            assert _same(c, runs(ctx, g)[n - 2], np.arange(len(grp.h)))           # and h_x0 = NULL is the reference start
