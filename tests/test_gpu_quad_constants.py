"""The four-lane rollout at B <= 4096 (k_rollout_q<1,*>) takes the constants of its sin/cos pair and of its atmosphere's
exp / log from scalar registers (loaded from one constant table, defined from the tables of the literal forms) and reads a
trajectory sample in the same LDS round trip as the step's inputs.  Neither may change a bit:
  * the scalar-operand forms equal the literal forms on every argument (f16_debug_sincos, f16_debug_pow);
  * at the smallest batches that can break the hand-over between the role waves -- a ragged tail, one and two workgroups --
    every stored sample is the state separate shorter launches reach, for the plain, the LQR and the scheduled kernel, with and
    without cell re-use; a batch of 4100 runs the two-group kernel, which keeps its code."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
R2D = 180.0 / 3.141592653589793


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(p, q):
    p, q = np.asarray(p), np.asarray(q)
    assert p.shape == q.shape
    if p.dtype != np.float64:
        return np.array_equal(p, q)
    nan = np.isnan(p) & np.isnan(q)                    # NaN compared as NaN, everything else as bit patterns (-0 is not +0)
    return np.array_equal(bits(p)[~nan], bits(q)[~nan]) and np.array_equal(np.isnan(p), np.isnan(q))


# ---------------------------------------------------------------- 1. the two forms of the sin/cos pair
def sincos_arguments():
    rng = np.random.default_rng(20261018)
    k = np.arange(-400, 401) * (np.pi / 2)             # the doubles at and on either side of multiples of pi/2
    big = np.arange(-63000, 63001, 997) * (np.pi / 2)  # ... and out to +-1e5
    near = np.concatenate([f(v, d) for v in (k, big) for f in (np.nextafter,) for d in (-np.inf, np.inf)] + [k, big])
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-310, 2.2250738585072014e-308, np.inf, -np.inf, np.nan,
                        np.pi / 4, -np.pi / 4, np.nextafter(np.pi / 4, 1), 1e5, -1e5])
    return np.concatenate([rng.uniform(-7, 7, 50000), rng.uniform(-1e5, 1e5, 50000), near, special])


def test_scalar_operand_sincos_equals_the_literal_form_bit_for_bit(hip):
    from f16_mpc_oop_py_amd import lib
    ctx = lib.Context(0)
    x = np.ascontiguousarray(sincos_arguments())
    n = x.size
    out = np.full((4, n), 123.0)
    lib.check(hip.f16_debug_sincos(ctx.handle, x.ctypes.data_as(ctypes.c_void_p), n, out.ctypes.data_as(ctypes.c_void_p)), hip)
    sn, cs, snk, csk = out
    assert same(sn, snk) and same(cs, csk)
    assert np.isnan(sn[~np.isfinite(x)]).all() and np.isnan(csk[~np.isfinite(x)]).all()
    assert (sn[x == 0] == 0).all() and (cs[x == 0] == 1).all()            # (the reduction turns -0 into +0, in both forms)
    # the pair itself (not only the agreement of its two forms): documented <= 2 ulp from libm, values <= 1 -> 2 * 2.2e-16
    small = np.abs(x) <= 7
    err = max(np.abs(sn[small] - np.sin(x[small])).max(), np.abs(cs[small] - np.cos(x[small])).max())
    print(f"sincos_bf vs libm on [-7, 7]: max abs error {err:.3e}")
    assert err <= 4.5e-16


# ---------------------------------------------------------------- 2. exp(0.14 log tfac): the library composition and its restatement
def test_restated_exp_log_equals_the_library_composition_bit_for_bit(hip):
    from f16_mpc_oop_py_amd import lib
    ctx = lib.Context(0)
    edge = 1.0 / 0.703e-5                                                  # tfac = 0 near 142,247 ft
    alt = np.concatenate([np.linspace(0.0, 100000.0, 100001),
                          [-1.0, -500.0, -1e4, -1e6, 100000.5, 120000.0, 142000.0, edge, np.nextafter(edge, 0), np.nextafter(edge, 1e9),
                           142248.0, 2e5, 1e7, 1e300, -1e300, np.inf, -np.inf, np.nan, 35000.0, np.nextafter(35000.0, 0)]])
    n = alt.size
    out = np.full((6, n), 123.0)
    lib.check(hip.f16_debug_pow(ctx.handle, alt.ctypes.data_as(ctypes.c_void_p), n, out.ctypes.data_as(ctypes.c_void_p)), hip)
    tfac = 1 - 0.703e-5 * alt
    assert (tfac[100001:] <= 0).sum() >= 4 and np.isnan(out[0][np.isnan(alt)]).all()
    for k, name in enumerate(("factor", "qbar", "ps")):
        assert same(out[k], out[3 + k]), name
    # the factor itself: tfac^0.14 to the 1 ulp the plant header states for the flight envelope (+ 1 ulp of numpy's pow)
    env = slice(0, 100001)
    rel = np.abs(out[3][env] / tfac[env] ** 0.14 - 1).max()
    print(f"exp(0.14 log tfac) vs numpy on [0, 1e5] ft: max rel error {rel:.3e}")
    assert rel <= 2 * 2.3e-16


# ---------------------------------------------------------------- 3. hand-over of samples and states
def make_env(x, u, **kw):
    from f16_mpc_oop_py_amd import F16Batch
    return F16Batch(x, u, device="cuda:0", **kw)


def small_batch(B, seed=3):
    """config-2 states with (cyclically, so that B = 3 has all of them) a NaN elevator command, an aircraft that starts inside
    the alpha grid and leaves it during the run (pitching up from 89 degrees: past the last node after 8 or 9 steps), and one that starts off the grid."""
    from f16_mpc_oop_py_amd.workload import config2_states
    x0, u0 = config2_states(B, seed=seed)
    u0[1 % B, 1] = np.nan
    x0[2 % B, 7] = 89.0 / R2D
    x0[2 % B, 10] = 2.0
    if B > 3:
        x0[3, 7] = 1.65                                                   # 94.5 degrees
    return x0, u0


_GAINS = {}


def lqr_gain(B):
    """K [B, 3, 9] of the undisturbed batch, computed once per batch size (the gain is an input here, not the thing under test)"""
    if B not in _GAINS:
        from f16_mpc_oop_py_amd.workload import config2_states
        _GAINS[B] = make_env(*config2_states(B, seed=3))._calc_LQR_gain()
    return _GAINS[B]


def schedule(B, rows, seed=5):
    """[rows, B, 4] commands around u0 = x0[:, 12:16]"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (rows, B, 4)) * np.array([500.0, 2.0, 2.0, 2.0])


def run_variant(variant, x0, u0, T, every, flags, chunks):
    """One launch of T steps storing every `every`-th state (chunks = False), or T / every launches of `every` steps with the
    state read back after each (chunks = True).  Returns (samples [T / every, 18, B], final x, status, last action)."""
    B = x0.shape[0]
    env = make_env(x0, u0, flags=flags)
    K = lqr_gain(B) if variant == "lqr" else None
    seq = u0[None] + schedule(B, T // every) if variant == "sched" else None
    if variant == "sched":
        seq[:, 1 % B, 1] = np.nan

    def launch(first, n, ev):
        if variant == "plain":
            return env.rollout(n, traj_every=ev)
        if variant == "lqr":
            return env.rollout_LQR(n, 0.05, -0.02, 0.01, K=K, traj_every=ev)
        return env.rollout_schedule(seq[first // every:(first + n + every - 1) // every], hold=every, nsteps=n, traj_every=ev)   # a row per sample

    if not chunks:
        tr = launch(0, T, every).cpu().numpy()
    else:
        tr = []
        for j in range(T // every):
            launch(j * every, every, None)
            tr.append(env.x_values.cpu().numpy().T.copy())
        tr = np.stack(tr)
    return tr, env.x_values.cpu().numpy(), env.status.cpu().numpy(), env.u_values.cpu().numpy()


# T = 40 with every sample stored; with every third the nearest length the entry points accept (nsteps % traj_every == 0) at
# or above it
CASES = [(B, T, every) for B in (3, 16, 19) for T, every in ((40, 1), (42, 3))] + [(4100, 60, 3)]


@pytest.mark.parametrize("variant", ["plain", "lqr", "sched"])
@pytest.mark.parametrize("B,T,every", CASES)
def test_samples_equal_the_states_of_shorter_launches(variant, B, T, every):
    from f16_mpc_oop_py_amd import lib as L
    x0, u0 = small_batch(B)
    one = run_variant(variant, x0, u0, T, every, 0, chunks=False)
    parts = run_variant(variant, x0, u0, T, every, 0, chunks=True)
    nocache = run_variant(variant, x0, u0, T, every, L.F16_FLAG_NO_CELL_CACHE, chunks=False)
    tr, x, st, u = one
    assert tr.shape == (T // every, 18, B)
    for j in range(T // every):
        assert same(tr[j], parts[0][j]), (variant, B, "sample", j)
    assert same(tr[-1], x.T)                                              # the last sample is the final state
    for p, q in zip(one, parts):
        assert same(p, q)
    for p, q in zip(one, nocache):
        assert same(p, q)
    # the special aircraft did what they are there for
    assert st[1 % B] & L.F16_ST["NONFINITE"] and np.isnan(x[1 % B]).any()
    assert tr[0, 7, 2 % B] * R2D < 90.0 < x[2 % B, 7] * R2D and st[2 % B] & L.F16_ST["ALPHA1"]
    if B > 3:
        assert st[3] & L.F16_ST["ALPHA1"]
    assert np.isfinite(x[0]).all() and not st[0] & L.F16_ST["NONFINITE"]
