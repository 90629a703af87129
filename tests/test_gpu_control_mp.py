"""The ZOH and Riccati kernels (csrc/f16_mpc_model.hpp: c2d_wave, dare_sda_wave, lqr_gain_wave) through the public C ABI against
fixture G19 (tools/make_control_golden.py): a 60-digit mpmath reference rounded once to fp64.

Tolerance rule (no number is fixed here): per case and output block the device may be 16 x as far from the reference as the numpy
restatement of the kernel's own rule is on that case (oracle/control_twin.py, recorded in the fixture), with a floor of 64 eps; all
errors relative to the block's largest entry.  The factor covers FMA contraction, the matrix-core summation order and the
Newton-refined reciprocals -- the same algorithm with other rounding; a wrong term, a wrong row map or a missing squaring lands
decades beyond it.  This file reads the fixture only (no mpmath, no CPU oracle)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
SMALL = 37                      # aircraft of a small batch: ragged, no multiple of the wavefront
BIG = 8192 + 70                 # wave_grid caps at 8192 workgroups: 70 of them take a second aircraft
MAXITER = 64                    # F16_ST_QP_MAXITER


def allowed(twin_err):
    return max(16.0 * float(twin_err), 64.0 * EPS)


def relerr(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.fixture(scope="module")
def G():
    return golden("g19_control_mp.npz")


@pytest.fixture(scope="module")
def ctx():
    from f16_mpc_oop_py_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _soa(a):
    """[B, r, c] -> state-major [r c, B] device tensor"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return torch.as_tensor(a.reshape(a.shape[0], -1).T.copy(), device="cuda:0")


def _aos(t, r, c):
    return t.t().reshape(-1, r, c).cpu().numpy()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def run_c2d(ctx, A, B, dt, nb):
    """aircraft b holds case b % len(A) -> (Ad [nb, ns, ns], Bd [nb, ns, ni])"""
    from f16_mpc_oop_py_amd import lib
    n, ns, ni = len(A), A.shape[1], B.shape[2]
    idx = np.arange(nb) % n
    Ad = torch.full((ns * ns, nb), np.nan, dtype=torch.float64, device="cuda:0")
    Bd = torch.full((ns * ni, nb), np.nan, dtype=torch.float64, device="cuda:0")
    a, b = _soa(A[idx]), _soa(B[idx])
    fn = ctx.lib.f16_c2d_batch if ns == 9 else ctx.lib.f16_c2d_full_batch
    lib.check(fn(ctx.handle, _vp(a), _vp(b), _vp(Ad), _vp(Bd), nb, nb, float(dt), None))
    torch.cuda.synchronize()
    return _aos(Ad, ns, ns), _aos(Bd, ns, ni)


def run_lqr(ctx, A, B, C, weights, nb, plain=False):
    """aircraft b holds case b % len(A) -> (K [nb, 3, 9] = +dlqr, X [nb, 9, 9], status [nb])"""
    from f16_mpc_oop_py_amd import lib
    idx = np.arange(nb) % len(A)
    K = torch.full((27, nb), np.nan, dtype=torch.float64, device="cuda:0")
    X = torch.full((81, nb), np.nan, dtype=torch.float64, device="cuda:0")
    st = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    a, b, c = _soa(A[idx]), _soa(B[idx]), _soa(C[idx])
    if plain:
        lib.check(ctx.lib.f16_lqr_batch(ctx.handle, _vp(a), _vp(b), _vp(c), _vp(K), _vp(X), _vp(st), nb, nb, None))
    else:
        lib.check(ctx.lib.f16_lqr_batch_w(ctx.handle, _vp(a), _vp(b), _vp(c), ctypes.byref(weights) if weights is not None else None,
                                          _vp(K), _vp(X), _vp(st), nb, nb, None))
    torch.cuda.synchronize()
    return -_aos(K, 3, 9), _aos(X, 9, 9), st.cpu().numpy()      # the library returns K = -dlqr (env.py:356)


def _copies_agree(out, n):
    """every aircraft of a tiled batch equals the first aircraft of its case, bit for bit"""
    idx = np.arange(len(out)) % n
    return np.array_equal(out, out[idx], equal_nan=True)


# ------------------------------------------------------------------------------------------------ ZOH
@pytest.mark.parametrize("tag", ["zoh9", "zoh18"])
def test_zoh_vs_multiprecision_expm(G, ctx, tag):
    """f16_c2d_batch / f16_c2d_full_batch on every ZOH case of G19 (step sizes with 0 to 9 squarings, both sides of the scaling
    threshold, nilpotent and rotating structure); the step is an argument of the call, so the cases of one step share a batch."""
    names, A, B, dts = G[f"{tag}_names"], G[f"{tag}_A"], G[f"{tag}_B"], G[f"{tag}_dt"]
    bad = []
    for dt in np.unique(dts):
        sel = np.flatnonzero(dts == dt)
        Ad, Bd = run_c2d(ctx, A[sel], B[sel], dt, SMALL)
        assert _copies_agree(Ad, len(sel)) and _copies_agree(Bd, len(sel))
        for k, i in enumerate(sel):
            for blk, got, ref, yard in (("Ad", Ad[k], G[f"{tag}_Ad"][i], G[f"{tag}_twin_err"][i, 0]),
                                        ("Bd", Bd[k], G[f"{tag}_Bd"][i], G[f"{tag}_twin_err"][i, 1])):
                e = relerr(got, ref)
                print(f"G19 device {tag} {names[i]} s={G[f'{tag}_s'][i]} {blk} err {e:.2e} allowed {allowed(yard):.2e}")
                if not e <= allowed(yard):
                    bad.append((str(names[i]), blk, e, allowed(yard)))
            if names[i] == "zeroA":              # A = 0: Ad = I and Bd = B dt exactly
                assert np.array_equal(Ad[k], np.eye(9)) and np.array_equal(Bd[k], B[i] * dt)
    assert not bad, bad


def _dare_groups(G):
    """the weights are an argument of the call: cases with the same (Q source, Q, R) share a batch"""
    groups = {}
    for i in range(len(G["dare_names"])):
        qcd = bool(G["dare_q_from_cd"][i])
        key = (qcd, b"" if qcd else G["dare_Q"][i].tobytes(), G["dare_R"][i].tobytes())
        groups.setdefault(key, []).append(i)
    return list(groups.values())


def _weights(G, i):
    from f16_mpc_oop_py_amd import lib
    return lib.make_weights(Q=None if G["dare_q_from_cd"][i] else G["dare_Q"][i], R=G["dare_R"][i])


# ------------------------------------------------------------------------------------------------ DARE and gain
def test_dare_and_gain_vs_multiprecision_riccati(G, ctx):
    """f16_lqr_batch_w on every DARE case of G19: the trim models under five weight sets, the dt = 0.02 models, four other flight
    conditions, two weighted output matrices and the four pivot cases (an exactly zero natural-order pivot at the first doubling:
    inverse9_tile<true> and its row map must run).  Status 0 everywhere."""
    names = G["dare_names"]
    bad = []
    for sel in _dare_groups(G):
        sel = np.array(sel)
        K, X, st = run_lqr(ctx, G["dare_A"][sel], G["dare_B"][sel], G["dare_C"][sel], _weights(G, sel[0]), SMALL)
        assert _copies_agree(K, len(sel)) and _copies_agree(X, len(sel))
        assert not st.any(), (names[sel], st)
        for k, i in enumerate(sel):
            for blk, got, ref, yard in (("Pare", X[k], G["dare_X"][i], G["dare_twin_err"][i, 0]),
                                        ("K", K[k], G["dare_K"][i], G["dare_twin_err"][i, 1])):
                e = relerr(got, ref)
                print(f"G19 device dare {names[i]} {blk} err {e:.2e} allowed {allowed(yard):.2e}")
                if not e <= allowed(yard):
                    bad.append((str(names[i]), blk, e, allowed(yard)))
    assert not bad, bad


def test_plain_entry_point_equals_the_weighted_one_with_default_weights(G, ctx):
    """f16_lqr_batch is f16_lqr_batch_w without weights: bit for bit on the Q = Cd'Cd, R = I cases"""
    sel = np.array(next(s for s in _dare_groups(G) if G["dare_q_from_cd"][s[0]] and np.array_equal(G["dare_R"][s[0]], np.eye(3))))
    a = run_lqr(ctx, G["dare_A"][sel], G["dare_B"][sel], G["dare_C"][sel], None, SMALL, plain=True)
    b = run_lqr(ctx, G["dare_A"][sel], G["dare_B"][sel], G["dare_C"][sel], _weights(G, sel[0]), SMALL)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------ the grid-stride pass
def test_zoh_second_grid_stride_pass_equals_the_small_batch(G, ctx):
    """B = 8192 + 70: workgroups 0..69 take a second aircraft on LDS they have used for ANOTHER model (8192 is no multiple of the
    number of cases); every aircraft equals the same case of a small batch bit for bit."""
    A, B = G["zoh9_A"], G["zoh9_B"]
    n = len(A)
    assert 8192 % n != 0
    small = run_c2d(ctx, A, B, 2e-2, SMALL)
    big = run_c2d(ctx, A, B, 2e-2, BIG)
    idx = np.arange(BIG) % n
    assert (idx[:70] != idx[8192:]).all()
    for s, b in zip(small, big):
        assert np.isfinite(s).all()
        assert np.array_equal(b, s[idx])


def test_lqr_second_grid_stride_pass_equals_the_small_batch(G, ctx):
    """the same for f16_lqr_batch_w with Q = Cd'Cd: the models AND the output matrices of aircraft b and b + 8192 differ for some of
    the 70 workgroups that run twice, so A, B, Cd and Q all have to be loaded again."""
    sel = np.array(next(s for s in _dare_groups(G) if G["dare_q_from_cd"][s[0]] and np.array_equal(G["dare_R"][s[0]], np.eye(3))))
    n = len(sel)
    A, B, C = G["dare_A"][sel], G["dare_B"][sel], G["dare_C"][sel]
    idx = np.arange(BIG) % n
    assert (idx[:70] != idx[8192:]).all()
    Q = np.einsum("bki,bkj->bij", C, C)
    assert sum(not np.array_equal(Q[idx[b]], Q[idx[b + 8192]]) for b in range(70)) >= 8
    w = _weights(G, sel[0])
    small = run_lqr(ctx, A, B, C, w, SMALL)
    big = run_lqr(ctx, A, B, C, w, BIG)
    assert not small[2].any()
    for s, b in zip(small, big):
        assert np.array_equal(b, s[idx])


# ------------------------------------------------------------------------------------------------ the non-convergence report
def test_doubling_cap_and_non_finite_solutions_report_maxiter(G, ctx):
    """F16_ST_QP_MAXITER: the cap case runs all 60 doublings (an uncontrollable, weighted mode at 1: H grows without limit) and stays
    finite; a model whose H overflows and an all-NaN model hand back a non-finite Pare and K and must say so.  A converging aircraft
    in the same batch keeps status 0."""
    names = [str(s) for s in G["status_names"]]
    i0 = list(G["dare_names"]).index("trim_xcg25_QCdCd_R1")
    A = np.concatenate([G["status_A"], G["dare_A"][i0:i0 + 1]])
    B = np.concatenate([G["status_B"], G["dare_B"][i0:i0 + 1]])
    C = np.concatenate([G["status_C"], G["dare_C"][i0:i0 + 1]])
    for k in range(len(names)):                  # (Cd = I: the plain entry point forms Q = Cd'Cd = I exactly)
        assert np.array_equal(C[k], np.eye(9)) and np.array_equal(G["status_Q"][k], np.eye(9)) and np.array_equal(G["status_R"][k], np.eye(3))
    n = len(A)
    K, X, st = run_lqr(ctx, A, B, C, None, 11, plain=True)
    bad = []
    for b in range(11):
        k = b % n
        finite = bool(np.isfinite(X[b]).all() and np.isfinite(K[b]).all())
        print(f"G19 device status {names[k] if k < len(names) else 'trim_xcg25_QCdCd_R1'} status {st[b]} finite {finite}")
        if k == n - 1:
            ok = st[b] == 0 and finite and relerr(X[b], G["dare_X"][i0]) <= allowed(G["dare_twin_err"][i0, 0])
        else:
            ok = (st[b] & MAXITER) != 0 and finite == bool(G["status_finite"][k])
            if not G["status_finite"][k]:
                ok = ok and not np.isfinite(X[b]).all()
        if not ok:
            bad.append((b, names[k] if k < len(names) else "converging", int(st[b]), finite))
    assert not bad, bad
