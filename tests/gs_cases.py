"""What the CPU and GPU tests of the scheduled-gain LQR loop share: the small random schedule and the lookup points of the bit-for-bit
comparisons (tests/test_lqr_gs_cpu.py: host function against numpy; tests/test_gpu_lqr_gs.py: the device against numpy)."""
import numpy as np

H0, DH, NH, V0, DV, NV = 1000.0, 500.0, 4, 300.0, 100.0, 3


def small_schedule(seed=0):
    """a 4 x 3 grid with random finite entries of mixed magnitude"""
    from f16_mpc_oop_py_amd.schedule import GainSchedule
    rng = np.random.default_rng(seed)
    table = rng.normal(size=(NH, NV, 12)) * 10.0 ** rng.integers(-3, 4, size=(NH, NV, 12))
    return GainSchedule(H0, DH, NH, V0, DV, NV, table)


def lookup_points(seed=1):
    """(h, v): 10,000 random points, a third of them outside the grid; every node and every edge midpoint; h or V = NaN, +inf, -inf"""
    rng = np.random.default_rng(seed)
    h1, v1 = H0 + (NH - 1) * DH, V0 + (NV - 1) * DV
    n = 10000
    h, v = rng.uniform(H0, h1, n), rng.uniform(V0, v1, n)
    out = np.arange(n) % 3 == 0                                               # a third outside: below / above in one or both axes
    side = rng.choice([0, 1, 2, 4, 5, 6, 7], n)                               # (3 would move neither coordinate)
    h = np.where(out & (side & 3 == 1), H0 - rng.uniform(0, 2 * DH, n), np.where(out & (side & 3 == 2), h1 + rng.uniform(0, 2 * DH, n), h))
    v = np.where(out & (side & 3 == 0), V0 - rng.uniform(0, 2 * DV, n), np.where(out & (side >= 4), v1 + rng.uniform(0, 2 * DV, n), v))
    hn, vn = H0 + DH * np.arange(NH), V0 + DV * np.arange(NV)
    hm, vm = H0 + DH * (np.arange(NH - 1) + 0.5), V0 + DV * (np.arange(NV - 1) + 0.5)
    grids = [np.meshgrid(a, b, indexing="ij") for a, b in ((hn, vn), (hm, vn), (hn, vm))]      # nodes, edge midpoints in h, in V
    odd = [np.nan, np.inf, -np.inf]
    hs = [h] + [g[0].ravel() for g in grids] + [np.array(odd), np.full(3, 1700.0), np.array(odd)]
    vs = [v] + [g[1].ravel() for g in grids] + [np.full(3, 420.0), np.array(odd), np.array(odd[::-1])]
    return np.concatenate(hs), np.concatenate(vs)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
