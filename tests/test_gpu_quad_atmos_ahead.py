"""k_rollout_q<1,*> evaluates the altitude part of a step's atmosphere (tfac, the temperature with its 35,000 ft select, tfac^4, log
tfac's quotient) half a step ahead, behind barrier B of the step before (in front of the loop for the first step), and takes a
wave's own states from its registers.  No fp64 operation changes, so all four
instantiations must return the bits of the kernel before: fixture G20 (tools/gpu_make_quad_atmos_golden.py, recorded with the
parent commit's library) holds them for the batch of fixture G17 plus five aircraft placed for the atmosphere -- one that climbs
across 35,000 ft, one that leaves through the top of the altitude box, a NaN altitude, one slower than 0.01 ft/s (the flap model's
own atmosphere call) and one at 150,000 ft (frozen at launch; with F16_FLAG_NO_ENVELOPE the log takes a negative argument) -- with
flags 0 and with F16_FLAG_NO_ENVELOPE.  Split launches must give the bits of one launch with a launch boundary right behind each
crossing: there the altitude part evaluated in front of the loop must agree with the loop's."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO, golden

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("gpu_make_quad_atmos_golden", os.path.join(REPO, "tools", "gpu_make_quad_atmos_golden.py"))
A = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(A)
G = A.G
bits = G.bits
FIXTURE = "g20_quad_atmosphere_cases.npz"
PARTS = (1, 15, 40, 144)           # launch boundaries behind step 16 (aircraft 7 is above 100,000 ft) and step 56 (aircraft 6 at 35,000 ft)
_cache = {}


def setup(B):
    """the batch of B aircraft and its LQR gains (taken once per size); B = 1: aircraft 6 alone"""
    if B not in _cache:
        x0, u0, base = A.batch(max(B, 16))
        if B == 1:
            x0, u0, base = x0[6:7], u0[6:7], base[6:7]
        else:
            x0, u0, base = x0[:B], u0[:B], base[:B]
        K = golden(FIXTURE)["K"] if B == G.B_FIX else G.gains(base, u0)
        _cache[B] = (x0, u0, K)
    return _cache[B]


def one_launch(variant, B, every, flags=0, steps=G.T_FIX):
    key = (variant, B, every, flags, steps)
    if key not in _cache:
        x0, u0, K = setup(B)
        _cache[key] = G.run(variant, x0, u0, K, parts=(steps,), every=every, flags=flags)
    return _cache[key]


def same(a, b):
    return a.shape == b.shape and (np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b))


def recorded(g, variant, tag):
    """(x, status, u, samples) of a recording; the samples under F16_FLAG_NO_ENVELOPE are stored where they differ from flags 0"""
    tr = g[f"{variant}_traj"]
    if tag:
        tr = tr.copy()
        tr[:, :, g[f"{variant}_ne_aircraft"]] = g[f"{variant}_ne_traj"]
    return g[f"{variant}{tag}_x"], g[f"{variant}{tag}_status"], g[f"{variant}{tag}_u"], tr


@pytest.mark.parametrize("tag,flags", A.RECORDINGS)
@pytest.mark.parametrize("variant", G.VARIANTS)
def test_every_instantiation_keeps_the_recorded_bits(variant, tag, flags):
    gx, gst, gu, gtr = recorded(golden(FIXTURE), variant, tag)
    x, st, u, tr = one_launch(variant, G.B_FIX, A.EVERY, flags)
    assert same(x, gx)                                     # (bit patterns: the NaN aircraft included, sign and payload)
    assert same(st, gst)
    assert same(u, gu)
    assert same(tr, gtr)
    # the step from which an aircraft's every-step samples stay the same: the step of freezing, with and without the envelope test
    assert np.array_equal(G.settle_step(one_launch(variant, G.B_FIX, 1, flags)[3]), golden(FIXTURE)[f"{variant}{tag}_settle"])


def test_the_hand_placed_aircraft_do_what_they_are_there_for():
    g = golden(FIXTURE)
    st, tr, settle = g["plain_status"], g["plain_traj"], g["plain_settle"]           # sample j = the state after step 10 (j + 1)
    h6 = tr[:, 2, 6]
    assert st[6] == 0 and h6[4] < 35000 <= h6[5] and (h6[5:] >= 35000).all()          # crosses 35,000 ft between steps 50 and 60, flies on
    assert st[7] == G.ST_ENVELOPE | 1 << (8 + 2) and 5 < settle[7] < G.T_FIX - 5      # out through the top of the altitude box, inside the run
    assert tr[0, 2, 7] < 100000 < tr[-1, 2, 7]
    x8 = g["plain_x"][8]
    assert st[8] & G.ST_NONFINITE and not np.isfinite(np.delete(x8, [12, 13, 14, 15])).any()      # NaN altitude: every state but the actuators'
    assert st[9] & G.ST_ENVELOPE and st[9] & 1 << (8 + 6) and 3 <= settle[9] < 10      # flew at least three steps at V <= 0.01 or near it
    assert st[10] == G.ST_ENVELOPE | 1 << (8 + 2) and settle[10] == 0                 # frozen at launch ...
    assert same(g["plain_x"][10], A.batch(G.B_FIX)[0][10])
    ne = g["plain_ne_aircraft"].tolist()
    assert {7, 9, 10} <= set(ne) and g["plain_ne_status"][10] & G.ST_ENVELOPE == 0     # ... and flying on without the envelope test:
    assert 1 - .703e-5 * A.batch(G.B_FIX)[0][10, 2] < 0 and np.isnan(g["plain_ne_x"][10, 16])      # tfac < 0, log of a negative number: NaN into the flap


@pytest.mark.parametrize("variant", G.VARIANTS)
@pytest.mark.parametrize("B", [16, 17, 48])
def test_split_launches_equal_one_launch(variant, B):
    x0, u0, K = setup(B)
    x, st, u, tr = one_launch(variant, B, 1)
    xs, sts, us, trs = G.run(variant, x0, u0, K, parts=PARTS, every=1)
    assert same(xs, x) and same(sts, st) and same(trs, tr)
    live = (st & G.ST_ENVELOPE) == 0                       # (the last action of a frozen aircraft is that of its launch: tests/test_gpu_quad_resident.py)
    assert same(us[live], u[live])


@pytest.mark.parametrize("variant", G.VARIANTS)
def test_split_launches_equal_one_launch_for_one_aircraft(variant):
    x0, u0, K = setup(1)
    x, st, u, tr = one_launch(variant, 1, 1, steps=3)
    xs, sts, us, trs = G.run(variant, x0, u0, K, parts=(1, 1, 1), every=1)
    assert same(xs, x) and same(sts, st) and same(us, u) and same(trs, tr)


@pytest.mark.parametrize("tag,flags", A.RECORDINGS)
@pytest.mark.parametrize("variant", G.VARIANTS)
def test_no_cell_cache_flag_gives_the_same_bits(variant, tag, flags):
    from f16_mpc_oop_py_amd import lib as L
    gx, gst, gu, gtr = recorded(golden(FIXTURE), variant, tag)
    x, st, u, tr = one_launch(variant, G.B_FIX, A.EVERY, flags | L.F16_FLAG_NO_CELL_CACHE)
    assert same(x, gx) and same(st, gst) and same(u, gu) and same(tr, gtr)
