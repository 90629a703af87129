"""CPU tests of the checker the linearisation kernels are pinned to (tests/linearise_cases.py): the fp64 restatement is what it
was, the extended-precision build is the same function on the same points, a second fp64 build under other rounding (FMA
contraction) stays inside the 8 x Y rule the device is held to, and the batched status word is the OR over every evaluated point."""
import numpy as np
import pytest

import linearise_cases as lc
from conftest import golden


@pytest.mark.parametrize("xcg", [25, 35])
def test_fp64_library_is_unchanged_on_the_g6_g7_fixtures(oracle, xcg):
    """linearise_na / linearise_full of libf16_oracle.so against the reference's own matrices (fixtures G6 / G7), at the bounds of
    tests/test_oracle_vs_golden.py::test_g6_g7_linearise_c2d_lqr; and the batched entry returns the single call's matrices bit for bit"""
    g = golden("g567_trim_lin_lqr.npz")
    x = g[f"trim_x_xcg{xcg}"]
    A, B, C, D = oracle.linearise_na(x, xcg=xcg / 100)
    np.testing.assert_allclose(A, g[f"ssr_Ac_xcg{xcg}"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(B, g[f"ssr_Bc_xcg{xcg}"], rtol=0, atol=1e-8)
    assert np.array_equal(C, g[f"ssr_Cc_xcg{xcg}"]) and np.array_equal(D, g[f"ssr_Dc_xcg{xcg}"])
    A18, B18, C18, D18 = oracle.linearise_full(x, x[12:16], xcg=xcg / 100)
    np.testing.assert_allclose(A18, g[f"A18_xcg{xcg}"], rtol=0, atol=2e-7)
    np.testing.assert_allclose(B18, g[f"B18_xcg{xcg}"], rtol=0, atol=1e-8)
    assert np.array_equal(C18, g[f"C18_xcg{xcg}"]) and not D18.any()
    L = lc.libs()["fp64"]
    Ab, Bb, Cb, st = L.linearise_na_batch(x[None], x[None, 12:16], xcg=xcg / 100)
    assert Ab.dtype == np.float64 and np.array_equal(Ab[0], A) and np.array_equal(Bb[0], B) and np.array_equal(Cb[0], C) and st[0] == 0
    Ab, Bb, Cb, st = L.linearise_full_batch(x[None], x[None, 12:16], xcg=xcg / 100)
    assert np.array_equal(Ab[0], A18) and np.array_equal(Bb[0], B18) and np.array_equal(Cb[0], C18) and st[0] == 0


@pytest.mark.parametrize("fam", lc.FAMILIES + [lc.EPS_FAMILY] + lc.FIX_CLR_FAMILIES, ids=str)
def test_extended_precision_agrees_with_fp64_within_the_present_bound(fam):
    """every row of the lattice, finite in both builds (asserted in reference()); at eps = 1e-5 the two agree within the project's
    present 1e-6, and the extended-precision matrices at the G6 / G7 trim points are the fixtures' within the same"""
    r = lc.reference(fam)
    assert len(r["ref"]) == {"hifi": 1418, "lofi": 569}[fam.fidelity]
    worst = float(np.abs(r["J64"] - r["ref"]).max())
    print(f"{fam}: cases {len(r['ref'])}, max |fp64 - ref| {worst:.3e}, Y == 0 on {int((r['Y'] == 0).sum())} of {r['Y'].size} entries, "
          f"max |J| {float(np.abs(r['ref']).max()):.3e}")
    assert worst < 1e-6 * (1e-5 / fam.eps)              # (rounding / eps: the bound scales with the divisor)
    # Y = 0 exactly on the entries whose reference is zero in every case: "exact where Y = 0" tests the zero structure alone
    assert np.array_equal(r["Y"] == 0, (r["ref"] == 0).all(0))
    if fam in lc.FAMILIES and fam.fidelity == "hifi":
        g = golden("g567_trim_lin_lqr.npz")
        k = int(round(fam.xcg * 100))
        x = g[f"trim_x_xcg{k}"]
        J, C, st = lc.run(lc.libs()["ld"], fam, x[None], x[None, 12:16])
        want = np.concatenate((g[f"ssr_Ac_xcg{k}"], g[f"ssr_Bc_xcg{k}"]), 1) if fam.model == "na" else \
            np.concatenate((g[f"A18_xcg{k}"], g[f"B18_xcg{k}"]), 1)
        assert float(np.abs(J[0] - want).max()) < 1e-6 and st[0] == 0


@pytest.mark.parametrize("fam", lc.FAMILIES + [lc.EPS_FAMILY] + lc.FIX_CLR_FAMILIES, ids=str)
def test_fma_witness_stays_inside_the_rule(fam):
    """the restatement rebuilt with -ffp-contract=fast -mfma: the same rule under other rounding lies within 8 x Y of the reference
    in every case and entry, and is exact where Y = 0.  The worst ratio is what the factor 8 is judged against."""
    r = lc.reference(fam)
    J, C, st = lc.run(lc.libs()["fma"], fam, r["x"], r["u"])
    worst = lc.check(J, fam, what="FMA witness")
    print(f"{fam}: FMA witness worst |J - ref| / Y = {worst:.3f}")
    assert np.array_equal(C, r["C64"]) and np.array_equal(st, r["status"])
    # and the rule has teeth: ONE entry of ONE case off by 1e-6 relative, the columns in another order, a divisor off by 1e-6
    one = J.copy()
    k = np.unravel_index(np.argmax(np.abs(J)), J.shape)
    one[k] *= 1 + 1e-6
    assert lc.ratios(one, fam)[1] == 1
    assert lc.ratios(np.ascontiguousarray(J[:, :, ::-1]), fam)[1] > 0 and lc.ratios(J / (1 + 1e-6), fam)[1] > 0


def test_wide_build_holds_fp64_tables_and_perturbs_in_fp64():
    L = lc.libs()
    t64, tld = L["fp64"].table_image(), L["ld"].table_image()
    assert tld.dtype == np.longdouble and t64.dtype == np.float64
    assert np.array_equal(tld, t64.astype(np.longdouble))                 # the same table, value for value
    assert np.array_equal(tld[:20], lc.ec.ALPHA1) and np.count_nonzero(tld) > 13000
    # C = (perturbed - base) / eps of the wide build: the perturbed point is fl64(p + eps), so the quotient in wide arithmetic is
    # NOT 1 -- it carries the fp64 rounding of the sum -- and equals numpy's longdouble quotient of the fp64 sum bit for bit
    for fam in (lc.Family("na", "hifi", 0.25), lc.Family("full", "lofi", 0.35), lc.EPS_FAMILY):
        b = lc.batch(fam)
        _, C, _ = lc.run(L["ld"], fam, b.x, b.u)
        idx = lc.MPC_X_IDX if fam.model == "na" else lc.OBS_X_IDX
        p = b.x[:, idx]
        want = ((p + fam.eps).astype(np.longdouble) - p.astype(np.longdouble)) / np.longdouble(fam.eps)
        got = np.stack([C[:, r, (r if fam.model == "na" else k)] for r, k in enumerate(idx)], 1)
        assert np.array_equal(got, want)
        wide_sum = ((p.astype(np.longdouble) + np.longdouble(fam.eps)) - p.astype(np.longdouble)) / np.longdouble(fam.eps)
        assert (want != wide_sum).mean() > 0.5                            # (the extended sum would have given another matrix)
        off = np.ones(C.shape[1:], bool)
        for r, k in enumerate(idx):
            off[r, r if fam.model == "na" else k] = False
        assert not C[:, off].any()


@pytest.mark.parametrize("fam", [lc.Family("na", "hifi", 0.25), lc.Family("full", "hifi", 0.35), lc.Family("na", "lofi", 0.35),
                                 lc.Family("full", "lofi", 0.25)], ids=str)
def test_batched_status_is_the_or_over_every_evaluated_point(fam):
    """status[b] of the batched entries = OR of f16o_last_status over the 13 / 23 points evaluated one by one (the kernels' atomicOr
    over the columns); the off-grid edge rows raise their bit, cell-interior rows raise none"""
    r = lc.reference(fam)
    b, st = r["batch"], r["status"]
    L = lc.libs()["fp64"]
    fi = 1 if fam.fidelity == "hifi" else 0
    rows = list(range(0, b.n_lattice, 23)) + list(range(b.n_lattice, b.B))
    for k in rows:
        pts = lc.perturbed_points(b.x[k], b.u[k], fam.eps, fam.model)
        assert len(pts) == (13 if fam.model == "na" else 23)
        each = [L.status_at(x, u, fi, fam.xcg, fam.model == "na") for x, u in pts]
        assert st[k] == int(np.bitwise_or.reduce(each)), (k, st[k], each)
    assert not (st & ~lc.GRID_BITS).any()
    # the reduced model reads the elevator from the command u[1] (env.py:175-177), the 18-state model from the state x[13]
    el = b.u[:, 1] if fam.model == "na" else b.x[:, 13]
    lat = np.arange(b.B) < b.n_lattice
    if fam.fidelity == "hifi":
        # (the lattice covers ALPHA1 up to 90 degrees: above the last ALPHA2 node, 45, the flap tables clamp by design)
        a2 = np.where(b.x[:, 7] * lc.ec.R2D > lc.ec.ALPHA2_END, 2, 0)
        inside = lat & (np.abs(el) < 25 - 1e-3)
        assert inside.sum() >= 1000 and np.array_equal(st[inside], a2[inside]) and (a2[inside] == 0).sum() > 500
        out = lat & (np.abs(el) > 25)
        assert np.array_equal(st[out], a2[out] | 8)
        e = b.edge
        assert st[e["off_alpha1_hi"]] & 1 and st[e["off_alpha1_lo"]] & 1 and st[e["off_alpha2"]] & 3 == 2
        assert st[e["off_beta_hi"]] & 4 and st[e["off_beta_lo"]] & 4
        if fam.model == "full":
            assert st[e["off_el_hi"]] & 8 and st[e["off_el_lo"]] & 8
    else:
        assert not st[lat].any()
        e = b.edge
        assert st[e["off_beta_hi"]] == 4 and st[e["off_beta_lo"]] == 4
    if fam.fidelity == "hifi":
        # one ulp inside the last beta node: the base point is on the grid, the perturbed beta is not -- only the OR reports it
        k = b.edge["beta_last"]
        assert st[k] & 4 and not L.status_at(b.x[k], b.u[k], fi, fam.xcg, fam.model == "na") & 4
