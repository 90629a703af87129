"""k_rollout_q<1,*> keeps every role's constants in registers for the whole launch and publishes x[0..5] where they become final
(behind barrier B).  Neither moves an fp64 operation, so all four instantiations -- plain, LQR law, input schedule, LQR law under a
demand schedule -- must return the bits of the kernel before: fixture G17 (tools/gpu_make_quad_variants_golden.py, recorded with
the parent commit's library; the batch, the schedules and the launch sequence are taken from that file).  Split launches must give
the bits of one launch (constants per launch, the prologue's psi, the early publish across a launch boundary), and an aircraft
that leaves the envelope must freeze at the same step with the same status word."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO, golden

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("gpu_make_quad_variants_golden", os.path.join(REPO, "tools", "gpu_make_quad_variants_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
bits = G.bits
_cache = {}


def setup(B):
    """the batch of B aircraft and its LQR gains (taken once per size)"""
    if B not in _cache:
        x0, u0, base = G.batch(B)
        K = golden("g17_quad_rollout_variants.npz")["K"] if B == G.B_FIX else G.gains(base, u0)
        _cache[B] = (x0, u0, K)
    return _cache[B]


def one_launch(variant, B, every, flags=0):
    key = (variant, B, every, flags)
    if key not in _cache:
        x0, u0, K = setup(B)
        _cache[key] = G.run(variant, x0, u0, K, every=every, flags=flags)
    return _cache[key]


def same(a, b):
    return a.shape == b.shape and (np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b))


@pytest.mark.parametrize("variant", G.VARIANTS)
def test_every_instantiation_keeps_the_recorded_bits(variant):
    g = golden("g17_quad_rollout_variants.npz")
    x, st, u, tr = one_launch(variant, G.B_FIX, G.EVERY)
    assert same(x, g[f"{variant}_x"])                      # (bit patterns: the NaN aircraft included, sign and payload)
    assert same(st, g[f"{variant}_status"])
    assert same(u, g[f"{variant}_u"])
    assert same(tr, g[f"{variant}_traj"])


def test_the_hand_placed_aircraft_do_what_they_are_there_for():
    g = golden("g17_quad_rollout_variants.npz")
    st = g["plain_status"]
    assert st[0] & G.ST_ENVELOPE and st[0] & (1 << (8 + 2))           # altitude: the test that now sits behind barrier B
    assert st[1] & G.ST_ENVELOPE and st[1] & (1 << (8 + 6))           # airspeed
    assert st[2] & G.ST_ENVELOPE and st[2] & (1 << (8 + 14))          # aileron state
    assert st[3] & G.ST_ENVELOPE and st[3] & (1 << (8 + 12))          # thrust state
    assert st[4] & G.ST_NONFINITE and st[5] & G.ST_NONFINITE          # NaN psi, NaN alpha
    assert 5 < g["plain_settle"][0] < G.T_FIX - 5 and 5 < g["plain_settle"][1] < G.T_FIX - 5     # frozen inside the run


@pytest.mark.parametrize("variant", G.VARIANTS)
@pytest.mark.parametrize("B", [16, 17, 48])
def test_split_launches_equal_one_launch(variant, B):
    x0, u0, K = setup(B)
    x, st, u, tr = one_launch(variant, B, 1)
    xs, sts, us, trs = G.run(variant, x0, u0, K, parts=(1, 99, 100), every=1)
    assert same(xs, x) and same(sts, st) and same(trs, tr)
    # the last action: a frozen aircraft reports the command of its last live step IN THAT LAUNCH, and u0 from a launch it never
    # stepped in (f16_dynamics.hip: `ulast` starts at the command) -- compared for the aircraft still flying at the end
    live = (st & G.ST_ENVELOPE) == 0
    assert same(us[live], u[live])


def outside(x):
    """env.py:117-124 on samples [n, 18, B] -> [n, B]"""
    lo = {2: 0, 6: 0, 7: -20, 8: -30, 9: -300, 10: -100, 11: -50, 12: 1000, 13: -25, 14: -21.5, 15: -30, 16: 0}
    hi = {2: 100000, 6: 900, 7: 90, 8: 30, 9: 300, 10: 100, 11: 50, 12: 19000, 13: 25, 14: 21.5, 15: 30, 16: 25}
    bad = np.zeros((x.shape[0], x.shape[2]), dtype=bool)
    for k in lo:
        bad |= (x[:, k] < lo[k]) | (x[:, k] > hi[k])
    return bad


@pytest.mark.parametrize("variant", G.VARIANTS)
def test_frozen_aircraft_freeze_at_the_same_step_with_the_same_status(variant):
    from f16_mpc_oop_py_amd import lib as L
    g = golden("g17_quad_rollout_variants.npz")
    x, st, u, tr = one_launch(variant, G.B_FIX, 1)
    xn, stn, un, trn = one_launch(variant, G.B_FIX, 1, flags=L.F16_FLAG_NO_CELL_CACHE)
    assert same(st, stn) and same(tr, trn) and same(x, xn)             # status word and every sample: the step of freezing with them
    assert same(st, g[f"{variant}_status"])
    settle = G.settle_step(tr)
    assert np.array_equal(settle, g[f"{variant}_settle"])              # the step from which an aircraft's samples stay the same
    frozen = np.flatnonzero(st & G.ST_ENVELOPE)
    assert {0, 1, 2, 3} <= set(frozen.tolist())
    bad = outside(tr)
    for a in frozen:
        if not bad[:, a].any():          # outside at launch (no sample shows the crossing): every sample is the launch state
            x0 = setup(G.B_FIX)[0]
            assert outside(x0.T[None])[0, a]
            first, ref = 0, x0[a]
        else:
            first = int(np.argmax(bad[:, a]))
            ref = tr[first, :, a]
        assert (bits(tr[first:, :, a]) == bits(ref)[None]).all(), f"aircraft {a} moved after sample {first}"
