"""CPU-side checks of the counter-based MPPI sampler and the fused loop's C-ABI surface: the header, the exported symbols, and the
sampling rule as mppi.sample_reference restates it (Philox4x32-10 + Box-Muller, include/f16_hip.h).  The device entries are tested in
tests/test_gpu_mppi_loop.py."""
import ctypes
import re

import numpy as np

from header_cases import header

# (counter, key, output) of Philox4x32-10: the known answers of include/f16_hip.h
VECTORS = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
LO, HI = np.array([-25.0, -21.5, -30.0]), np.array([25.0, 21.5, 30.0])      # parameters.py:125-126, the three surfaces


def nominal(S=3, B=4):
    """a seeded nominal schedule well inside the command limits"""
    rng = np.random.default_rng(3)
    return np.concatenate([rng.uniform(2000, 9000, (S, B, 1)), rng.uniform(-3, 3, (S, B, 3))], 2)


def test_philox_known_answers():
    from f16_mpc_oop_py_amd.mppi import philox4x32_10
    for ctr, key, out in VECTORS:
        assert philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64)).tolist() == out
    got = philox4x32_10(np.array([v[0] for v in VECTORS], dtype=np.uint64), np.array([v[1] for v in VECTORS], dtype=np.uint64))
    assert got.dtype == np.uint32 and got.tolist() == [v[2] for v in VECTORS]          # batched as well


def test_header_declares_the_three_entries():
    src = header()
    for name in ("f16_mppi_sample", "f16_debug_philox", "f16_rollout_mppi"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*f16_ctx\s*\*", src), name


def test_library_exports_the_three_symbols():
    from f16_mpc_oop_py_amd import lib
    L = ctypes.CDLL(lib.build())
    assert hasattr(L, "f16_mppi_sample") and hasattr(L, "f16_debug_philox") and hasattr(L, "f16_rollout_mppi")


def test_normals_have_mean_zero_and_variance_one():
    """3 x 2^16 draws: five-sigma bounds.  The mean of n standard normals has deviation 1 / sqrt(n), their sample variance sqrt(2 / n)."""
    from f16_mpc_oop_py_amd.mppi import normals_reference
    z = normals_reference(seed=20261019, period=3, rows=4, samples=128, aircraft=128)
    assert z.shape == (4, 128, 128, 3)
    n = z.size
    assert n == 3 * 2 ** 16
    print(f"mean {z.mean():.3e} (bound {5 / np.sqrt(n):.3e}), variance - 1 {z.var() - 1:.3e} (bound {5 * np.sqrt(2 / n):.3e})")
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
    assert np.abs(z).max() <= 6.8
    for i in range(3):                                                              # every channel on its own, n / 3 draws each
        assert abs(z[..., i].mean()) <= 5 / np.sqrt(n / 3) and abs(z[..., i].var() - 1.0) <= 5 * np.sqrt(6.0 / n)


def test_clipping_thrust_row_zero_sigma_and_nan():
    from f16_mpc_oop_py_amd.mppi import sample_reference
    nom = nominal()
    s = sample_reference(nom, 40.0, 64, seed=1, period=0)                          # [S, K, B, 4]
    assert s.shape == (3, 64, 4, 4)
    for i in range(3):
        v = s[..., 1 + i]
        assert (v == LO[i]).any() and (v == HI[i]).any() and v.min() >= LO[i] and v.max() <= HI[i]
    assert np.array_equal(s[..., 0], np.repeat(nom[:, None, :, 0], 64, 1))           # the thrust command is never perturbed
    z = sample_reference(nom, 0.0, 5, seed=1, period=0)
    assert np.array_equal(z.view(np.int64), np.repeat(nom[:, None], 5, 1).view(np.int64))      # sigma = 0: the nominal, bit for bit
    z3 = sample_reference(nom, [0.0, 0.5, 0.0], 5, seed=1, period=0)               # per-channel sigma
    assert np.array_equal(z3[..., [0, 1, 3]], z[..., [0, 1, 3]]) and not np.array_equal(z3[..., 2], z[..., 2])
    bad = nom.copy()
    bad[1, 2, 2] = np.nan
    b = sample_reference(bad, 0.5, 5, seed=1, period=0)
    assert np.isnan(b[1, :, 2, 2]).all() and np.isnan(b).sum() == 5                  # a NaN nominal entry stays NaN, and only it


def test_every_counter_word_and_the_seed_change_the_draw():
    from f16_mpc_oop_py_amd.mppi import normals_reference, sample_reference
    nom = nominal()
    a = sample_reference(nom, 0.5, 6, seed=9, period=2)
    assert np.array_equal(a, sample_reference(nom, 0.5, 6, seed=9, period=2))       # the same arguments repeat it
    assert not np.array_equal(a, sample_reference(nom, 0.5, 6, seed=10, period=2))
    assert not np.array_equal(a, sample_reference(nom, 0.5, 6, seed=9 + 2 ** 32, period=2))      # the high half of the seed is key word 1
    assert not np.array_equal(a, sample_reference(nom, 0.5, 6, seed=9, period=3))
    z = normals_reference(9, 2, 3, 6, 4)                                            # [row, k, a, 3]
    flat = z.reshape(-1, 3)
    assert len(np.unique(flat, axis=0)) == len(flat)                               # no two (row, k, a) share a draw
    # a larger sample set or batch extends the smaller one: the draw depends on (period, row, k, a) alone
    assert np.array_equal(normals_reference(9, 2, 5, 8, 7)[:3, :6, :4], z)
