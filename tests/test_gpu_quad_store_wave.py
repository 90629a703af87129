"""k_rollout_q<1,*> stores its trajectory samples from a fifth wave of the workgroup, which reads the published state behind barrier A
and does nothing else; the table waves carry a cell's reciprocal width with the cell; wave 3 evaluates the log's polynomial half a
step ahead.  No result changes, so all four instantiations must return and store the bits of the kernel before: fixture G21q
(tools/gpu_make_quad_store_golden.py, recorded with the parent commit's library; the batch, the launch sequence with its
sentinel-filled sample buffers and the sample bookkeeping are taken from that file) holds, for a batch of 48 with two aircraft
frozen by the envelope in mid-run, one whose alpha leaves its table cell in mid-run, a NaN alpha and an elevator on the last node
of its axis, over T = 84 steps: final state, status, last action, every sample of traj_every = 1 for aircraft 0..16 and the
samples of traj_every = 7 for all 48.  Every launch stores into a buffer that is longer than it needs and filled with a sentinel:
the rows behind the last sample must come back untouched.  (A launch whose length is no multiple of its sample period is not
among the cases: the entry points reject it, as test_a_launch_that_is_no_multiple_of_its_sample_period_is_rejected holds.)
An aircraft's bits do not depend on the batch it flies in, so B = 1, 16, 17 are checked against the columns of the same fixture."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO, golden

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("gpu_make_quad_store_golden", os.path.join(REPO, "tools", "gpu_make_quad_store_golden.py"))
A = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(A)
G = A.G
bits = G.bits
E1, E7 = "g21_quad_store_wave_every1.npz", "g21_quad_store_wave_every7.npz"
T = A.T_FIX
COLS = {48: slice(0, 48), 17: slice(0, 17), 16: slice(0, 16), 1: slice(A.CROSSER, A.CROSSER + 1)}      # B = 1: the aircraft that leaves its cell
_cache = {}


def same(a, b):
    return a.shape == b.shape and (np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b))


def launch(variant, B, every, parts=(T,)):
    """(x, status, u, launches) of tools/gpu_make_quad_store_golden.py run(), computed once per case"""
    key = (variant, B, every, parts)
    if key not in _cache:
        _cache[key] = A.run(variant, golden(E1)["K"], COLS[B], parts=parts, every=every)
    return _cache[key]


def every_step(variant, B):
    """the every-step samples of one launch of T steps [T, 18, B]: sample t - 1 is the state behind step t"""
    steps, tr = A.stored(launch(variant, B, 1)[3], 1)
    assert np.array_equal(steps, np.arange(1, T + 1))
    return tr


def cross(variant):
    g = golden(E1)
    c = int(g[f"{variant}_cross"])
    return c if c else int(g["plain_cross"])


@pytest.mark.parametrize("B", [48, 17, 16, 1])
@pytest.mark.parametrize("variant", G.VARIANTS)
def test_final_state_status_and_every_sample_keep_the_recorded_bits(variant, B):
    g, cols = golden(E1), COLS[B]
    x, st, u, _ = launch(variant, B, 1)
    tr = every_step(variant, B)                            # (asserts the rows behind the last sample untouched)
    assert same(x, g[f"{variant}_x"][cols]) and same(st, g[f"{variant}_status"][cols]) and same(u, g[f"{variant}_u"][cols])
    keep = cols if B == 1 else slice(0, min(B, A.KEEP))
    assert same(tr[:, :, :A.KEEP], g[f"{variant}_traj"][:, :, keep])
    assert same(tr[-1], np.ascontiguousarray(x.T))          # the last sample is the state the launch leaves


def test_the_placed_aircraft_do_what_they_are_there_for():
    g = golden(E1)
    st, tr = g["plain_status"], g["plain_traj"]
    frozen = G.settle_step(tr)
    assert all(st[a] & G.ST_ENVELOPE and 10 < frozen[a] < T - 10 for a in (0, 1))          # frozen in mid-run
    c = A.crossing_steps(tr, A.CROSSER)
    assert st[A.CROSSER] == 0 and len(c) and c[0] == g["plain_cross"] and 5 < c[0] < T - 5  # leaves its alpha cell in mid-run, flies on
    assert all(c[0] < s for a in range(16) if a != A.CROSSER for s in A.crossing_steps(tr, a))      # the first alpha crossing of its workgroup
    assert np.isnan(g["plain_x"][A.NAN_AXIS, 7]) and st[A.NAN_AXIS] & G.ST_NONFINITE
    assert g["plain_x"][A.LAST_NODE, 13] == 25.0 and (golden(E7)["plain_traj7"][:, 13, A.LAST_NODE] == 25.0).all()


def axis_cells(states):
    """per table axis (alpha on ALPHA1, beta, elevator on DH1 and on DH2) the cell index of every aircraft in `states` [n, 18, B] and
    whether the value lies in a cell at all (x0 <= v < x1 for some cell: on the grid, not NaN, not on the last node) -- against
    the breakpoints of the device's own table image"""
    import ctypes
    from f16_mpc_oop_py_amd import lib
    L = lib.load()
    ctx = lib.Context(0)
    img = np.zeros(L.f16_table_image_doubles())
    lib.check(L.f16_debug_read_tables(ctx.handle, ctypes.c_void_p(img.ctypes.data)))
    r2d = 180.0 / 3.141592653589793
    out = {}
    for name, v, bp in (("alpha", states[:, 7] * r2d, img[0:20]), ("beta", states[:, 8] * r2d, img[20:39]),
                        ("elevator, DH1", states[:, 13], img[39:44]), ("elevator, DH2", states[:, 13], img[44:47])):
        out[name] = (np.searchsorted(bp, v, side="right") - 1, (v >= bp[0]) & (v < bp[-1]))
    return out


@pytest.mark.parametrize("variant", G.VARIANTS)
def test_the_first_workgroup_runs_the_hit_path_before_the_crossing(variant):
    """What the split-launch test stands on, for all three axes of both table waves: every aircraft of the first workgroup lies in
    a cell throughout, aircraft 7 leaves its alpha cell with step c, and no aircraft of the workgroup changes a cell on any axis
    with steps c - 2 and c - 1: steps c - 1 and c re-use the cell and its reciprocal (hits), step c + 1 is a full lookup."""
    g = golden(E1)
    c = cross(variant)
    x0 = A.batch()[0][:16]
    states = np.concatenate([x0.T[None], g[f"{variant}_traj"][:, :, :16]])      # states[t]: behind t steps
    cells = axis_cells(states)
    assert all(inside.all() for _, inside in cells.values())
    changed = {name: np.flatnonzero((cell[1:] != cell[:-1]).any(axis=1)) + 1 for name, (cell, _) in cells.items()}    # with which steps
    assert c in changed["alpha"] and cells["alpha"][0][c, A.CROSSER] != cells["alpha"][0][c - 1, A.CROSSER]
    assert not any(t in ch for t in (c - 2, c - 1) for ch in changed.values()), changed
    assert any((ch < c - 2).any() for ch in changed.values())          # (and there were full lookups before: the cells are not the launch's)


@pytest.mark.parametrize("every", [3, 7])
@pytest.mark.parametrize("B", [48, 17, 16, 1])
@pytest.mark.parametrize("variant", G.VARIANTS)
def test_every_third_and_every_seventh_sample(variant, B, every):
    g, cols = golden(E1), COLS[B]
    x, st, u, launches = launch(variant, B, every)
    steps, tr = A.stored(launches, every)                  # (asserts the rows behind the last sample untouched)
    assert np.array_equal(steps, every * np.arange(1, T // every + 1))
    assert same(x, g[f"{variant}_x"][cols]) and same(st, g[f"{variant}_status"][cols]) and same(u, g[f"{variant}_u"][cols])
    assert same(tr, every_step(variant, B)[steps - 1])     # the samples of the every-step launch, which the test above pins
    if every == 7:
        assert same(tr, golden(E7)[f"{variant}_traj7"][:, :, cols])


@pytest.mark.parametrize("variant", G.VARIANTS)
def test_a_launch_that_is_no_multiple_of_its_sample_period_is_rejected(variant):
    from f16_mpc_oop_py_amd.lib import F16HipError
    with pytest.raises(F16HipError, match="multiple of traj_every"):
        A.run(variant, golden(E1)["K"], COLS[16], parts=(80,), every=3)


@pytest.mark.parametrize("B", [48, 17, 16, 1])
@pytest.mark.parametrize("variant", G.VARIANTS)
def test_without_a_trajectory_buffer(variant, B):
    g, cols = golden(E1), COLS[B]
    x, st, u, launches = launch(variant, B, None)
    assert all(buf is None for _, _, buf in launches)
    assert same(x, g[f"{variant}_x"][cols]) and same(st, g[f"{variant}_status"][cols]) and same(u, g[f"{variant}_u"][cols])


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("B", [48, 17, 16, 1])
@pytest.mark.parametrize("variant", G.VARIANTS)
def test_split_launches_give_the_bits_of_one_launch(variant, B, every):
    """every = 1: launch boundaries behind step c, on which a lane leaves its table cell (the step behind it is the first full
    lookup), and behind step c + 1.  every = 3: a boundary behind step 30, directly behind a sample (a launch is a multiple of its
    sample period, so no boundary can stand between two samples; 30 is a multiple of the schedules' hold too).  Every stored sample
    is compared with the every-step launch's sample of the step it stands behind."""
    c = cross(variant)
    parts = (c, 1, T - c - 1) if every == 1 else (30, T - 30)
    x, st, u, _ = launch(variant, B, 1)
    xs, sts, us, launches = A.run(variant, golden(E1)["K"], COLS[B], parts=parts, every=every)
    steps, tr = A.stored(launches, every)
    assert same(xs, x) and same(sts, st)
    live = (st & G.ST_ENVELOPE) == 0                       # (the last action of a frozen aircraft is that of its launch: tests/test_gpu_quad_resident.py)
    assert same(us[live], u[live])
    assert len(steps) and same(tr, every_step(variant, B)[steps - 1])
    if every == 1:
        assert np.array_equal(steps, np.arange(1, T + 1))
