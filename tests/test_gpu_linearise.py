"""GPU tests of f16_linearise_batch and f16_linearise_full_batch through the C ABI, over the whole envelope and on every launch
path, against the extended-precision reference and the 8 x Y rule of tests/linearise_cases.py (read its docstring first).

Launch paths (csrc/f16_control.hip): one lane per (aircraft, column), 12 / 22 columns.  Up to 64 * 256 lanes the <64> instantiation
runs (B <= 1,365 / 744); above, the <256> instantiation, with a grid of at most 256 blocks, so that above 256 * 256 lanes (B > 5,461
/ 2,978) every lane walks a grid-stride loop.  Each path is held to the rule on every case of the family."""
import ctypes
import types

import numpy as np
import pytest

import linearise_cases as lc

pytestmark = pytest.mark.gpu

PAD = -7.25                      # what the output buffers hold before a call (a value no Jacobian entry takes)
ALL = lc.FAMILIES + [lc.EPS_FAMILY] + lc.FIX_CLR_FAMILIES


@pytest.fixture(scope="module")
def dev():
    import torch
    from f16_mpc_oop_py_amd import lib
    return types.SimpleNamespace(torch=torch, L=lib.load(), ctx=lib.Context(0))


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def call(dev, fam, x, u, ld=None, status="zero"):
    """one C call at the family's settings -> J [B, ns, ns + ni] (A | B), C [B, no, ns], status [B] or None, and the raw [n, ld]
    buffers.  status: "zero" (a zeroed word per aircraft), None (NULL) or an int the words hold before the call."""
    t = dev.torch
    ns, ni, no = lc.dims(fam.model)
    B = len(x)
    ld = B if ld is None else ld

    def soa(a, k):
        buf = np.full((k, ld), 0.5)
        buf[:, :B] = np.asarray(a, dtype=np.float64).T
        return t.as_tensor(buf, device="cuda:0")
    xs, us = soa(x, 18), soa(u, 4)
    Ac, Bc, Cc = (t.full((n, ld), PAD, dtype=t.float64, device="cuda:0") for n in (ns * ns, ns * ni, no * ns))
    st = None if status is None else t.full((ld,), 0 if status == "zero" else int(status), dtype=t.int32, device="cuda:0")
    f = dev.L.f16_linearise_batch if fam.model == "na" else dev.L.f16_linearise_full_batch
    rc = f(dev.ctx.handle, vp(xs), vp(us), vp(Ac), vp(Bc), vp(Cc), vp(st), B, ld, fam.eps, fam.xcg, 1 if fam.fidelity == "hifi" else 0,
           lc.FLAG_FIX_CLR if fam.fix_clr else 0, None)
    assert rc == 0, dev.L.f16_last_error().decode()
    raw = types.SimpleNamespace(Ac=Ac.cpu().numpy(), Bc=Bc.cpu().numpy(), Cc=Cc.cpu().numpy(), st=None if st is None else st.cpu().numpy())
    A = raw.Ac[:, :B].T.reshape(B, ns, ns)
    Bm = raw.Bc[:, :B].T.reshape(B, ns, ni)
    C = raw.Cc[:, :B].T.reshape(B, no, ns)
    return np.concatenate((A, Bm), 2), C, (None if st is None else raw.st[:B]), raw


def thresholds(model):
    """(largest B of the <64> path, largest B of the <256> path without the grid-stride loop)"""
    cols = 12 if model == "na" else 22
    return 64 * 256 // cols, 256 * 256 // cols


_PATHS = {}


def paths(dev, fam):
    """the family on the three launch paths, computed once: {"<64>": J of the two halves joined, "<256>": [tiles], "<256> strided":
    [tiles]} plus the C matrices and status words of each"""
    if fam in _PATHS:
        return _PATHS[fam]
    r = lc.reference(fam)
    x, u = r["x"], r["u"]
    B0 = len(x)
    t64, t256 = thresholds(fam.model)
    h = (B0 + 1) // 2
    assert h <= t64
    halves = [call(dev, fam, x[:h], u[:h]), call(dev, fam, x[h:], u[h:])]
    out = {"<64>": types.SimpleNamespace(J=[np.concatenate([p[0] for p in halves])], C=np.concatenate([p[1] for p in halves]),
                                         st=np.concatenate([p[2] for p in halves]), B=h)}
    n1 = t64 // B0 + 1                      # the fewest copies of the family that leave the <64> path (hifi: 1; 1,418 rows)
    n2 = t256 // B0 + 1                     # ... and that need the grid-stride loop (hifi: 4 -> 5,672 rows / 3 -> 4,254 rows)
    assert t64 < n1 * B0 <= t256 < n2 * B0
    for name, n in (("<256>", n1), ("<256> strided", n2)):
        J, C, st, _ = call(dev, fam, np.tile(x, (n, 1)), np.tile(u, (n, 1)))
        out[name] = types.SimpleNamespace(J=list(J.reshape(n, B0, *J.shape[1:])), C=C.reshape(n, B0, *C.shape[1:]),
                                          st=st.reshape(n, B0), B=n * B0)
    _PATHS[fam] = out
    return out


@pytest.mark.parametrize("fam", ALL, ids=str)
def test_every_launch_path_holds_the_rule_over_the_whole_envelope(dev, fam):
    """|device - reference| <= 8 Y[r, c] in every case and entry, exact where Y = 0, on the <64> path (the family in halves), the
    <256> path and the <256> path with its grid-stride loop (the family tiled); tiled copies of a case are equal bit for bit.
    Measured on an MI355X (worst |device - reference| / Y per family, the same on all three paths): DESIGN.md, "The linearisation
    kernels against an extended-precision plant"."""
    r = lc.reference(fam)
    B0 = len(r["x"])
    assert B0 == {"hifi": 1418, "lofi": 569}[fam.fidelity]
    P = paths(dev, fam)
    worst = {}
    for name, p in P.items():
        worst[name] = max(lc.ratios(J, fam)[0] for J in p.J)
    same = np.array_equal(P["<64>"].J[0], P["<256>"].J[0])
    print(f"{fam}: cases {B0} (launches of {', '.join(str(p.B) for p in P.values())} aircraft); worst |device - ref| / Y: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; <64> and <256> bit-identical: {same}")
    for name, p in P.items():
        for J in p.J:
            assert J.shape[0] == B0 and np.isfinite(J).all()
            lc.check(J, fam, what=name)
        for J in p.J[1:]:
            assert np.array_equal(J, p.J[0]), name            # tiled copies of one case within a launch


@pytest.mark.parametrize("fam", ALL, ids=str)
def test_cc_is_the_plain_quotient_and_status_is_the_restatements_or(dev, fam):
    """Cc = (fl(p + eps) - p) / eps on the observed coordinate, bit for bit against plain numpy, exact zeros elsewhere; the status
    word of every aircraft = the OR of the grid-clamp bits over all of its evaluated points, as the fp64 restatement reports it
    (tests/test_linearise_cpu.py pins that OR to the points taken one by one)."""
    r = lc.reference(fam)
    b = r["batch"]
    want = lc.cc_numpy(r["x"], r["u"], fam.eps, fam.model)
    assert np.array_equal(want, r["C64"])
    for name, p in paths(dev, fam).items():
        for C in (p.C if p.C.ndim == 4 else p.C[None]):
            assert np.array_equal(C, want), name
        for st in (p.st if p.st.ndim == 2 else p.st[None]):
            assert np.array_equal(st, r["status"]), (name, np.flatnonzero(st != r["status"])[:8])
    # the off-grid rows of the lattice raise their bit, rows inside their cells raise none (above the last ALPHA2 node, 45
    # degrees, the flap tables clamp by design; the reduced model reads the elevator from the command u[1], env.py:175-177)
    st = paths(dev, fam)["<64>"].st
    lat = np.arange(b.B) < b.n_lattice
    e = b.edge
    if fam.fidelity == "hifi":
        el = b.u[:, 1] if fam.model == "na" else b.x[:, 13]
        a2 = np.where(b.x[:, 7] * lc.ec.R2D > lc.ec.ALPHA2_END, 2, 0)
        inside = lat & (np.abs(el) < 25 - 1e-3)
        assert inside.sum() >= 1000 and np.array_equal(st[inside], a2[inside]) and (st[inside] == 0).sum() > 500
        assert st[e["off_alpha1_hi"]] & 1 and st[e["off_alpha1_lo"]] & 1 and st[e["off_alpha2"]] & 3 == 2
        assert st[e["off_beta_hi"]] & 4 and st[e["off_beta_lo"]] & 4
        if fam.model == "full":
            assert st[e["off_el_hi"]] & 8 and st[e["off_el_lo"]] & 8
    else:
        assert not st[lat].any() and st[e["off_beta_hi"]] == 4 and st[e["off_beta_lo"]] == 4


@pytest.mark.parametrize("fam", [lc.Family("na", "hifi", 0.25), lc.Family("full", "hifi", 0.25)], ids=str)
def test_leading_dimension_null_status_and_sticky_status(dev, fam):
    """ld > B: the same matrices, every element of the padding columns untouched; a NULL status is accepted and changes nothing;
    status words are ORed into, not overwritten."""
    r = lc.reference(fam)
    n = 700
    x, u = r["x"][-n:], r["u"][-n:]                  # (the edge rows are at the end: status words that are not zero)
    J0, C0, st0, _ = call(dev, fam, x, u)
    assert st0.any()
    J1, C1, st1, raw = call(dev, fam, x, u, ld=n + 37)
    assert np.array_equal(J1, J0) and np.array_equal(C1, C0) and np.array_equal(st1, st0)
    for buf in (raw.Ac, raw.Bc, raw.Cc):
        assert (buf[:, n:] == PAD).all()
    assert not raw.st[n:].any()
    J2, C2, st2, _ = call(dev, fam, x, u, status=None)
    assert st2 is None and np.array_equal(J2, J0) and np.array_equal(C2, C0)
    J3, _, st3, _ = call(dev, fam, x, u, status=1 << 20)
    assert np.array_equal(J3, J0) and np.array_equal(st3, st0 | (1 << 20))


@pytest.mark.parametrize("fam", [f for f in lc.FAMILIES if f.xcg == 0.25], ids=str)
def test_nonfinite_rows_stay_in_their_rows(dev, fam):
    """alpha NaN, V +inf and a NaN aileron command appended to a batch: their matrices are not finite exactly where the fp64
    restatement's are not (nothing else is compared on them), and every other aircraft's result is unchanged bit for bit."""
    r = lc.reference(fam)
    n = min(len(r["x"]), 709)
    x, u = r["x"][:n], r["u"][:n]
    xn, un = lc.nonfinite_rows(fam)
    J0, C0, st0, _ = call(dev, fam, x, u)
    J1, C1, st1, _ = call(dev, fam, np.concatenate((x, xn)), np.concatenate((u, un)))
    assert np.array_equal(J1[:n], J0) and np.array_equal(C1[:n], C0) and np.array_equal(st1[:n], st0)
    Jr, Cr, _ = lc.run(lc.libs()["fp64"], fam, xn, un)
    assert not np.isfinite(Jr).all(axis=(1, 2)).any()                 # (each of the three does break its matrices)
    assert np.array_equal(np.isfinite(J1[n:]), np.isfinite(Jr))
    assert np.array_equal(np.isfinite(C1[n:]), np.isfinite(Cr))


@pytest.mark.parametrize("xcg", [0.25, 0.35])
def test_python_surface_returns_the_c_calls_matrices(dev, xcg):
    """F16Batch._linearise_na, linearise(...) in the reference's call shape (env.py:49) and linearise_full(discretise=False) on the
    first 37 rows of the hifi family: the C call's matrices bit for bit, as [B, rows, cols]; Dc is zero."""
    from f16_mpc_oop_py_amd import F16Batch
    na, full = lc.Family("na", "hifi", xcg), lc.Family("full", "hifi", xcg)
    r = lc.reference(na)
    x, u = r["x"][:37], r["u"][:37]
    env = F16Batch(x, u, device="cuda:0", xcg=xcg, fi_flag=1)
    J, C, st, _ = call(dev, na, x, u)
    got = [[t.cpu().numpy() for t in env._linearise_na()]]
    assert np.array_equal(env.last_status.cpu().numpy(), st)
    got.append([t.cpu().numpy() for t in env.linearise(env._get_mpc_x(), env._get_mpc_u(), _calc_xdot=env._calc_xdot_na,
                                                       get_obs=env._get_obs_na)])
    for A, Bm, Cm, D in got:
        assert A.shape == (37, 9, 9) and Bm.shape == (37, 9, 3) and Cm.shape == (37, 9, 9) and D.shape == (37, 9, 3)
        assert np.array_equal(A, J[:, :, :9]) and np.array_equal(Bm, J[:, :, 9:]) and np.array_equal(Cm, C) and not D.any()
    lc.check(np.concatenate((got[0][0], got[0][1]), 2), na, rows=slice(0, 37), what="F16Batch._linearise_na")
    J, C, st, _ = call(dev, full, x, u)
    d = env.linearise_full(discretise=False)
    assert set(d) == {"Ac", "Bc", "Cc", "Dc"} and np.array_equal(env.last_status.cpu().numpy(), st)
    A, Bm, Cm, D = (d[k].cpu().numpy() for k in ("Ac", "Bc", "Cc", "Dc"))
    assert A.shape == (37, 18, 18) and Bm.shape == (37, 18, 4) and Cm.shape == (37, 10, 18) and D.shape == (37, 10, 4)
    assert np.array_equal(A, J[:, :, :18]) and np.array_equal(Bm, J[:, :, 18:]) and np.array_equal(Cm, C) and not D.any()
    lc.check(np.concatenate((A, Bm), 2), full, rows=slice(0, 37), what="F16Batch.linearise_full")
    A2, B2, C2, D2 = (t.cpu().numpy() for t in env.linearise(env.x_values, env.u_values))        # env.py:45: the default model
    assert np.array_equal(A2, A) and np.array_equal(B2, Bm) and np.array_equal(C2, Cm) and not D2.any()
