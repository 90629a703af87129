"""CPU-side checks of the ensemble statistics (include/f16_hip.h "ENSEMBLE STATISTICS": f16_rollout_wind_ens,
f16_rollout_lqr_wind_ens, f16_ens_from_traj; f16_mpc_oop_py_amd/ensemble.py): what tests/test_gpu_ensemble.py rests on, and
everything that needs no device.

  * ensemble_reference, the numpy restatement the device is held to bit for bit, against exact rational arithmetic within the
    bound of the rule's own error analysis (error_bounds below); the mask rule; empty waves and groups; every batch / group size at
    which the grouping takes another path; combine of two halves against the fold;
  * the argument rules of the three C entries on calls the library refuses or treats as a no-op (nothing is launched and no array is
    dereferenced: a zeroed host buffer stands for the context and for every array), and their parameter lists against the siblings';
  * on the recording environment of tests/test_rollout_calls_cpu.py: which symbol a Python call ends in with and without ensemble=.
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from header_cases import header_parameters, names
from test_rollout_calls_cpu import BAD_ARGUMENT, BAD_STEPS, F16_EINVAL, F16_OK, env_of
from test_rollout_rk_calls_cpu import BAD_METHOD, METHODS, clib  # noqa: F401  (clib: the fixture)

U = 2.0 ** -53
SIBLING = {"f16_rollout_wind_ens": "f16_rollout_wind", "f16_rollout_lqr_wind_ens": "f16_rollout_lqr_wind"}


def error_bounds(X, R, M2, W):
    """Bounds on |mean - exact| and |m2 - exact| of one group and state row: X = max |x|, R = max - min and M2 = the exact sum of
    squared deviations over the contributing aircraft, W = the group's wavefronts; u = 2^-53, gamma_k = k u / (1 - k u) <= 1.01 k u.

    A wave.  The pairwise sum of <= 64 terms has six levels: |s^ - s| <= gamma_6 sum |x|; the division adds one rounding, so
        |mean_w^ - mean_w| <= gamma_7 X <= e_w := 8.1 u X.
    Around the computed mean, sum (x - mean_w^)^2 = M2_w + n_w (mean_w^ - mean_w)^2 exactly (the deviations from the true mean sum to
    zero).  Each d = fl(x - mean_w^) carries one rounding, its square three, the tree six more: a relative gamma_9 on that sum, so
        |M2_w^ - M2_w| <= gamma_9 M2_w + (1 + gamma_9) 64 e_w^2 <= 1.01 * 9 u M2_w + 65 e_w^2.
    A fold (Chan's update), at most W - 1 of them.  With exact arithmetic the new mean is a convex combination of the two means, so
    the errors of its inputs do not grow; the update rounds delta, n_w / N, their product and the sum (N and n n_w are integers below
    2^53, exact): at most gamma_3 |delta| + u |mean| <= (3 * 2 X + X) 1.01 u <= e_w per fold.  Hence
        |mean^ - mean| <= e_m := W e_w = 8.1 W u X.
    M2 of the union is M2_a + M2_b + delta^2 c exactly, c = n n_w / N <= n_w <= 64, and the true means of parts of the data differ by
    |delta| <= R.  The computed delta is off by at most 2 e_m, which moves delta^2 c by <= 64 (2 R * 2 e_m + 4 e_m^2); the roundings
    (delta one, its square one more, c one, the product one, the two sums one each) are a relative gamma_5 on the result, and a partial
    M2 never exceeds the group's.  Summed over the waves and the folds:
        |m2^ - m2| <= 1.01 u (9 + 5 W) M2 + 65 W e_w^2 + 256 W (R e_m + e_m^2).
    Nothing here is fitted: on shifted data (X >> R) the last term, first order in u X R, is what remains -- a sum of squares
    without the shift would be off by u N X^2 instead."""
    e_w = 8.1 * U * X
    e_m = W * e_w
    return e_m, 1.01 * U * (9 + 5 * W) * M2 + 65 * W * e_w * e_w + 256 * W * (R * e_m + e_m * e_m)


def exact_group(col):
    """exact (n, mean, M2, min, max) of the finite doubles in col, as Fractions / floats"""
    v = [Fraction(float(x)) for x in col]
    n = len(v)
    if n == 0:
        return 0, Fraction(0), Fraction(0), np.inf, -np.inf
    mean = sum(v) / n
    return n, mean, sum((x - mean) ** 2 for x in v), float(min(v)), float(max(v))


def against_exact(traj, group, ref, mask):
    """ref = ensemble_reference(traj, group, envelope as in mask) against exact rational arithmetic on the masked aircraft"""
    S, _, B = traj.shape
    worst = [0.0, 0.0]
    for s in range(S):
        for g in range(ref.count.shape[1]):
            lo, hi = g * group, min((g + 1) * group, B)
            keep = mask[s, lo:hi]
            W = (hi - lo + 63) // 64
            assert ref.count[s, g] == keep.sum()
            for k in range(18):
                col = traj[s, k, lo:hi][keep]
                n, mean, m2, mn, mx = exact_group(col)
                if n == 0:
                    assert (ref.mean[s, g, k], ref.m2[s, g, k], ref.min[s, g, k], ref.max[s, g, k]) == (0.0, 0.0, np.inf, -np.inf)
                    continue
                assert ref.min[s, g, k] == mn and ref.max[s, g, k] == mx
                bm, b2 = error_bounds(float(np.abs(col).max()), mx - mn, float(m2), W)
                em, e2 = abs(float(Fraction(float(ref.mean[s, g, k])) - mean)), abs(float(Fraction(float(ref.m2[s, g, k])) - m2))
                assert em <= bm and e2 <= b2, (s, g, k, em, bm, e2, b2)
                if bm > 0 and b2 > 0:
                    worst = [max(worst[0], em / bm), max(worst[1], e2 / b2)]
    return worst


def synthetic(B, S=2, seed=0):
    """[S, 18, B] samples: rows of very different scale, row 3 a large offset with a small spread (1e4 + 1e-3 noise), row 5 constant"""
    rng = np.random.default_rng(seed + B)
    x = rng.normal(size=(S, 18, B)) * (10.0 ** rng.integers(-3, 6, size=(1, 18, 1)))
    x[:, 3] = 1e4 + 1e-3 * rng.normal(size=(S, B))
    x[:, 4] = -3e5 + 1e-2 * rng.normal(size=(S, B))
    x[:, 5] = 0.1
    return x


# ------------------------------------------------------------------------------------------------ the reference against exact arithmetic
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_reference_against_exact_rational_arithmetic(B):
    """every batch size at which a wave or a group is full, short or single, with group = 64, 128 and one group for the whole batch;
    a few aircraft NaN or infinite, so that waves are thinned.  The bounds: error_bounds (its docstring is the derivation)."""
    from f16_mpc_oop_py_amd.ensemble import contributes, ensemble_reference, group_size
    x = synthetic(B)
    if B > 2:
        x[0, 7, B // 2] = np.nan
        x[1, 0, B - 1] = np.inf
    mask = contributes(x, envelope=False)
    assert mask.sum() == 2 * B - (2 if B > 2 else 0)
    for group in (64, 128, True):
        ref = ensemble_reference(x, group, envelope=False)
        gs = group_size(group, B)
        G = (B + gs - 1) // gs
        assert ref.count.shape == (2, G) and ref.mean.shape == ref.m2.shape == ref.min.shape == ref.max.shape == (2, G, 18)
        assert ref.count.dtype == np.int32 and ref.count.sum() == mask.sum()
        worst = against_exact(x, gs, ref, mask)
        print(f"MEASURED B={B} group={group}: largest error / bound, mean {worst[0]:.2e}, m2 {worst[1]:.2e}")
        var = ref.var
        assert np.array_equal(np.isnan(var), np.broadcast_to(ref.count[..., None] < 2, var.shape))
        ok = ref.count >= 2
        assert np.array_equal(var[ok], ref.m2[ok] / (ref.count[ok][:, None] - 1.0))
    with pytest.raises(ValueError):
        ensemble_reference(x, 96)
    with pytest.raises(ValueError):
        ensemble_reference(x, 0)


def test_the_shifted_rows_keep_their_spread():
    """1e4 + 1e-3 noise over 257 aircraft: the bound of error_bounds, stated as a number for this case, holds M2 to 1e-5 of itself
    (a sum of squares about zero would be off by u N X^2 = 3e-6 against M2 = 3e-4, a hundredth of it)"""
    from f16_mpc_oop_py_amd.ensemble import ensemble_reference
    x = synthetic(257, S=1)
    ref = ensemble_reference(x, True, envelope=False)
    n, mean, m2, _, _ = exact_group(x[0, 3])
    bm, b2 = error_bounds(float(np.abs(x[0, 3]).max()), float(np.ptp(x[0, 3])), float(m2), 5)
    assert b2 < 1e-5 * float(m2) and bm < 1e-7
    assert abs(float(Fraction(float(ref.m2[0, 0, 3])) - m2)) <= b2 and abs(float(Fraction(float(ref.mean[0, 0, 3])) - mean)) <= bm


# ------------------------------------------------------------------------------------------------ the mask, empty waves and groups
def inside_box(B, S=1, seed=0):
    """[S, 18, B] samples inside the box of env.py:117-124"""
    from f16_mpc_oop_py_amd.ensemble import X_LB, X_UB
    rng = np.random.default_rng(seed)
    lo, hi = np.where(np.isfinite(X_LB), X_LB, -1e3), np.where(np.isfinite(X_UB), X_UB, 1e3)
    return rng.uniform(lo[None, :, None], hi[None, :, None], (S, 18, B))


def test_the_mask_is_a_function_of_the_sample():
    from f16_mpc_oop_py_amd.ensemble import X_LB, X_UB, contributes, ensemble_reference
    B = 130
    x = inside_box(B)
    assert contributes(x).all()
    x[0, :, 3] = X_UB                                         # on the box: inside (the kernel freezes on < and >)
    x[0, :, 4] = X_LB
    x[0, [0, 1, 3, 4, 5, 17], 3] = 1e300                     # the six states without a limit
    x[0, [0, 1, 3, 4, 5, 17], 4] = -1e300
    assert contributes(x).all()
    bad = {}
    for j, k in enumerate(np.nonzero(np.isfinite(X_UB))[0]):
        x[0, k, 10 + 2 * j] = np.nextafter(X_UB[k], np.inf)
        x[0, k, 11 + 2 * j] = np.nextafter(X_LB[k], -np.inf)
        bad[10 + 2 * j] = bad[11 + 2 * j] = True
    x[0, 2, 70], x[0, 17, 71], x[0, 9, 72] = np.nan, np.inf, -np.inf
    m = contributes(x)
    assert set(np.nonzero(~m[0])[0]) == set(bad) | {70, 71, 72}
    free = contributes(x, envelope=False)
    assert set(np.nonzero(~free[0])[0]) == {70, 71, 72}      # F16_FLAG_NO_ENVELOPE: finiteness alone
    ref = ensemble_reference(x, 64)
    assert list(ref.count[0]) == [64 - len(bad), 64 - 3, 2]
    keep = m[0, :64]
    assert ref.max[0, 0, 6] == x[0, 6, :64][keep].max() and ref.min[0, 0, 6] == x[0, 6, :64][keep].min()


def test_empty_waves_and_empty_groups():
    from f16_mpc_oop_py_amd.ensemble import ensemble_reference, wave_records
    B = 64 * 5 + 7
    x = inside_box(B, S=2, seed=1)
    x[:, 6, 64:128] = -1.0                                    # wave 1: every aircraft outside the box
    x[0, 0, 128:256] = np.nan                                 # waves 2 and 3 at sample 0
    n, mean, m2, mn, mx = wave_records(x)
    assert list(n[0]) == [64, 0, 0, 0, 64, 7] and list(n[1]) == [64, 0, 64, 64, 64, 7]
    assert (mean[:, :, 1] == 0).all() and (m2[:, :, 1] == 0).all() and (mn[:, :, 1] == np.inf).all() and (mx[:, :, 1] == -np.inf).all()
    r64, r128, r256 = (ensemble_reference(x, g) for g in (64, 128, 256))
    assert list(r64.count[0]) == [64, 0, 0, 0, 64, 7] and list(r128.count[0]) == [64, 0, 71] and list(r256.count[0]) == [64, 71]
    for r, g in ((r64, 1), (r128, 1)):                        # an empty group
        assert (r.mean[0, g] == 0).all() and (r.m2[0, g] == 0).all() and (r.min[0, g] == np.inf).all() and (r.max[0, g] == -np.inf).all()
        assert np.isnan(r.var[0, g]).all()
    # a group whose first waves are empty takes its first non-empty wave as it is; empty waves in the middle change nothing
    assert np.array_equal(r128.mean[0, 0], mean[0, :, 0]) and np.array_equal(r128.m2[0, 0], m2[0, :, 0])
    assert np.array_equal(r256.mean[0, 0], mean[0, :, 0]) and np.array_equal(r256.min[0, 0], mn[0, :, 0])
    alone = ensemble_reference(np.concatenate((x[:, :, :64], x[:, :, 256:]), 2), 256)
    assert np.array_equal(alone.mean[0], ensemble_reference(x, 512).mean[0]) and np.array_equal(alone.m2[0], ensemble_reference(x, 512).m2[0])


def test_combine_of_two_halves_is_the_fold():
    from f16_mpc_oop_py_amd.ensemble import combine, ensemble_reference
    x = synthetic(512, seed=3)
    x[0, 1, 320:384] = np.nan                                 # (an empty wave in the second half)
    whole = ensemble_reference(x, 512, envelope=False)
    # the fold takes the waves one by one: folding the first 7 waves and then the eighth is the fold of all eight
    first, last = ensemble_reference(x[:, :, :448], 448, envelope=False), ensemble_reference(x[:, :, 448:], 64, envelope=False)
    got = combine(first.parts(), last.parts())
    for a, b in zip(got, whole.parts()):
        assert np.array_equal(a, b)
    # two halves of four waves each: the same statistic by another order of the update -- equal within the bound, not bit for bit
    a, b = ensemble_reference(x[:, :, :256], 256, envelope=False), ensemble_reference(x[:, :, 256:], 256, envelope=False)
    halves = combine(a.parts(), b.parts())
    assert np.array_equal(halves[0], whole.count) and np.array_equal(halves[3], whole.min) and np.array_equal(halves[4], whole.max)
    for s in range(2):
        for k in range(18):
            col = x[s, k][np.isfinite(x[s]).all(0)]
            _, mean, m2, mn, mx = exact_group(col)
            bm, b2 = error_bounds(float(np.abs(col).max()), mx - mn, float(m2), 8)
            assert abs(float(Fraction(float(halves[1][s, 0, k])) - mean)) <= bm and abs(float(Fraction(float(halves[2][s, 0, k])) - m2)) <= b2
    # an empty side leaves the other as it is
    empty = (np.zeros_like(a.count), np.zeros_like(a.mean), np.zeros_like(a.m2), np.full_like(a.min, np.inf), np.full_like(a.max, -np.inf))
    for got in (combine(a.parts(), empty), combine(empty, a.parts())):
        for u, v in zip(got, a.parts()):
            assert np.array_equal(u, v)


# ------------------------------------------------------------------------------------------------ the C rules
def ens_struct(buf, **fields):
    from f16_mpc_oop_py_amd import lib
    e = lib.Ens()
    for k in ("work", "count", "mean", "m2", "min", "max"):
        setattr(e, k, buf.value)
    e.group, e.ldg = 64, 1
    for k, v in fields.items():
        setattr(e, k, v)
    return e


def call(clib, symbol, method, ens, wind=None, **over):
    """`symbol` on a call that is complete except for `over` (None = a NULL pointer): four aircraft, five steps, no traj -> (rc, message)"""
    L, buf, _, _ = clib
    base = dict(B=4, ld=4, nsteps=5, hold=2, traj_every=1, dt=1e-3, xcg=0.35, fi_flag=1, method=method, flags=0, stream=None, traj=None,
                u_out=None, status=None, h_wind=None if wind is None else ctypes.byref(wind), nsamples=5,
                h_ens=None if ens is None else ctypes.byref(ens))
    if symbol == "f16_ens_from_traj":
        base["traj"] = buf
    args = [over[n] if n in over else base.get(n, buf) for n in names(symbol)]
    rc = getattr(L, symbol)(*args)
    return rc, L.f16_last_error().decode()


def refused(clib, symbol, method, ens, words, **over):
    rc, msg = call(clib, symbol, method, ens, **over)
    assert rc == F16_EINVAL and words in msg, (symbol, method, over, rc, msg)


@pytest.mark.parametrize("symbol", list(SIBLING))
def test_parameter_lists_are_the_siblings_plus_the_ensemble(symbol):
    from f16_mpc_oop_py_amd import lib
    new, old = header_parameters(symbol), header_parameters(SIBLING[symbol])
    k = [p.replace("*", " ").split()[-1] for p in old].index("traj") + 1
    assert new == old[:k] + ["const f16_ens *h_ens"] + old[k:]
    L = lib.load()
    at, bt = getattr(L, symbol).argtypes, getattr(L, SIBLING[symbol]).argtypes
    assert list(at) == list(bt[:k]) + [ctypes.POINTER(lib.Ens)] + list(bt[k:])
    assert [f[0] for f in lib.Ens._fields_] == ["work", "group", "ldg", "count", "mean", "m2", "min", "max"]
    assert names("f16_ens_from_traj") == ["ctx", "traj", "nsamples", "B", "ld", "flags", "h_ens", "stream"]
    assert len(L.f16_ens_from_traj.argtypes) == 8 and L.f16_ens_from_traj.argtypes[6] == ctypes.POINTER(lib.Ens)


def test_the_workspace_size_is_host_code():
    from f16_mpc_oop_py_amd import lib
    L = lib.load()
    for B, S in ((1, 1), (64, 3), (65, 3), (257, 40), (262144, 1000)):
        assert L.f16_ens_work_doubles(B, S) == 73 * ((B + 63) // 64) * S
    assert L.f16_ens_work_doubles(0, 5) == 0 and L.f16_ens_work_doubles(5, 0) == 0


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("symbol", list(SIBLING))
def test_what_the_sibling_refuses_is_refused_first_then_the_ensemble_fields(clib, symbol, method):
    from test_wind_cpu import wind_struct
    buf = clib[1]
    quiet = dict(B=0, ld=0)
    lqr = symbol == "f16_rollout_lqr_wind_ens"
    missing = "K / dem_seq is NULL" if lqr else "u_seq is NULL"
    for ens in (None, ens_struct(buf), ens_struct(buf, group=0)):          # the sibling's refusals come first, whatever h_ens holds
        refused(clib, symbol, method, ens, BAD_ARGUMENT, ctx=None, **quiet)
        refused(clib, symbol, method, ens, BAD_ARGUMENT, x=None, **quiet)
        refused(clib, symbol, method, ens, BAD_ARGUMENT, B=4, ld=3, nsteps=0)
        refused(clib, symbol, method, ens, BAD_STEPS, nsteps=-1, **quiet)
        refused(clib, symbol, method, ens, BAD_STEPS, nsteps=5, traj=buf, traj_every=2, **quiet)
        refused(clib, symbol, method, ens, missing, **{"dem_seq" if lqr else "u_seq": None}, **quiet)
        refused(clib, symbol, method, ens, "hold must be >= 1", hold=0, **quiet)
        rc, msg = call(clib, symbol, 3, ens, **quiet)
        assert rc == F16_EINVAL and BAD_METHOD in msg
        rc, msg = call(clib, symbol, method, ens, wind=wind_struct(buf, gust_seq="buf", gust_hold=0), **quiet)
        assert rc == F16_EINVAL and "gust_hold must be >= 1" in msg
    ok = ens_struct(buf)
    # the sample period is required with or without traj
    for every in (0, -1, 2):
        refused(clib, symbol, method, ok, "sample period", nsteps=5, traj_every=every, **quiet)
    refused(clib, symbol, method, None, "h_ens or one of its members is NULL", **quiet)
    for member in ("work", "count", "mean", "m2", "min", "max"):
        refused(clib, symbol, method, ens_struct(buf, **{member: None}), "h_ens or one of its members is NULL", **quiet)
    for group in (0, 63, 65, 96, -64):
        refused(clib, symbol, method, ens_struct(buf, group=group), "group must be a multiple of 64", **quiet)
    refused(clib, symbol, method, ens_struct(buf, group=64, ldg=1), "ldg < G", B=65, ld=65, nsteps=0)
    refused(clib, symbol, method, ens_struct(buf, group=128, ldg=2), "ldg < G", B=257, ld=257, nsteps=0)
    # B == 0 and nsteps == 0 are no-ops, with and without air; nothing was written
    assert call(clib, symbol, method, ok, **quiet)[0] == F16_OK
    assert call(clib, symbol, method, ens_struct(buf, group=128, ldg=3), B=257, ld=257, nsteps=0)[0] == F16_OK
    assert call(clib, symbol, method, ok, wind=wind_struct(buf, wind_ned="buf"), nsteps=0)[0] == F16_OK
    assert call(clib, symbol, method, ok, nsteps=6, traj_every=3, traj=buf, **quiet)[0] == F16_OK
    assert clib[3].raw == bytes(4096)


def test_ens_from_traj_checks_its_arguments(clib):
    buf, zeros = clib[1], clib[3]
    ok = ens_struct(buf)
    sym = "f16_ens_from_traj"
    bad = "bad argument (NULL pointer, B < 0, ld < B or nsamples < 0)"
    quiet = dict(B=0, ld=0)
    for ens in (None, ok):
        refused(clib, sym, 0, ens, bad, ctx=None, **quiet)
        refused(clib, sym, 0, ens, bad, traj=None, **quiet)
        refused(clib, sym, 0, ens, bad, B=-1, ld=0)
        refused(clib, sym, 0, ens, bad, B=4, ld=3, nsamples=0)
        refused(clib, sym, 0, ens, bad, nsamples=-1, **quiet)
    refused(clib, sym, 0, None, "h_ens or one of its members is NULL", **quiet)
    refused(clib, sym, 0, ens_struct(buf, m2=None), "h_ens or one of its members is NULL", **quiet)
    refused(clib, sym, 0, ens_struct(buf, group=32), "group must be a multiple of 64", **quiet)
    refused(clib, sym, 0, ens_struct(buf, group=64, ldg=4), "ldg < G", B=257, ld=257, nsamples=0)
    assert call(clib, sym, 0, ok, **quiet)[0] == F16_OK and call(clib, sym, 0, ok, nsamples=0)[0] == F16_OK
    assert zeros.raw == bytes(4096)


# ------------------------------------------------------------------------------------------------ the Python keywords
def test_keywords_end_in_the_ensemble_calls_and_defaults_in_todays():
    import torch
    from f16_mpc_oop_py_amd.ensemble import Ensemble
    from f16_mpc_oop_py_amd.wind import GustModel
    B = 4
    K0 = torch.zeros((B, 3, 9), dtype=torch.float64)
    env = env_of(B)
    assert env.rollout_schedule(np.zeros((3, B, 4)), hold=2, nsteps=5) is None
    env.rollout_LQR(5, 0.0, 0.0, 0.0, K=K0)
    env.rollout_schedule(np.zeros((3, B, 4)), hold=2, nsteps=5, method="rk4", wind=[10.0, 0.0, -2.0])
    env.rollout_LQR(5, 0.0, 0.0, 0.0, K=K0, gusts=GustModel(5.0, 1750.0, 700.0, seed=3, every=2))
    calls = [c for c in env.lib.calls if c[0].startswith("f16_rollout")]
    assert [c[0] for c in calls] == ["f16_rollout_sched", "f16_rollout_lqr", "f16_rollout_wind", "f16_rollout_lqr_wind"]
    for c in calls:
        assert len(c[1]) == len(names(c[0]))                                   # today's symbols with today's arguments
    env = env_of(B)
    gm = GustModel(5.0, 1750.0, 700.0, seed=3, every=2)
    e1 = env.rollout_schedule(np.zeros((3, B, 4)), hold=2, nsteps=6, method="rk4", traj_every=3, wind=[10.0, 0.0, -2.0], ensemble=True)
    traj, e2 = env.rollout_LQR(6, 0.0, 0.0, 0.0, K=K0, gusts=gm, ensemble=64, keep_traj=True, traj_every=2)
    e3 = env.rollout_schedule(np.zeros((3, B, 4)), hold=2, nsteps=5, ensemble=128)          # no air, every step
    calls = [c for c in env.lib.calls if c[0].startswith("f16_rollout")]
    assert [c[0] for c in calls] == ["f16_rollout_wind_ens", "f16_rollout_lqr_wind_ens", "f16_rollout_wind_ens"]
    for c in calls:
        assert len(c[1]) == len(names(c[0]))
    got = [dict(zip(names(c[0]), c[1])) for c in calls]
    assert (got[0]["nsteps"], got[0]["hold"], got[0]["traj_every"], got[0]["method"]) == (6, 2, 3, 4)
    assert got[0]["traj"] is None and got[0]["h_wind"] is not None and got[2]["h_wind"] is None and got[2]["traj_every"] == 1
    assert got[1]["traj"].value == traj.data_ptr() and tuple(traj.shape) == (3, 18, B) and gm.row == 3
    for e, S in ((e1, 2), (e2, 3), (e3, 5)):
        assert isinstance(e, Ensemble) and tuple(e.count.shape) == (S, 1) and e.count.dtype == torch.int32
        assert all(tuple(t.shape) == (S, 1, 18) and t.dtype == torch.float64 for t in (e.mean, e.m2, e.min, e.max, e.var))
    assert (e1.group, e2.group, e3.group) == (64, 64, 128)


def test_value_errors_before_any_call():
    import torch
    B = 4
    env = env_of(B)
    K = torch.zeros((B, 3, 9), dtype=torch.float64)
    for kw in (dict(linear=True), dict(relinearise=True, K=None), dict(schedule=object())):
        with pytest.raises(ValueError, match="ensemble"):
            env.rollout_LQR(5, 0.0, 0.0, 0.0, **dict(dict(K=K, ensemble=64), **kw))
    for group in (0, 32, 96, 64.5, False):
        with pytest.raises(ValueError, match="multiple of 64"):
            env.rollout_schedule(np.zeros((3, B, 4)), hold=2, nsteps=5, ensemble=group)
    with pytest.raises(ValueError, match="sample period"):
        env.rollout_schedule(np.zeros((3, B, 4)), hold=2, nsteps=5, traj_every=2, ensemble=64)
    with pytest.raises(ValueError, match="keep_traj"):
        env.rollout_schedule(np.zeros((3, B, 4)), hold=2, nsteps=5, keep_traj=True)
    assert [c for c in env.lib.calls if c[0].startswith("f16_rollout")] == []
