"""CPU-side checks of the scored rollout and the MPPI blend: the C-ABI surface (header, exported symbols, the ctypes structure) and
the blend rule as mppi.blend_reference states it.  The device entries are tested in tests/test_gpu_rollout_cost.py."""
import ctypes
import math
import re

import numpy as np
import pytest

from header_cases import header


def test_header_declares_the_two_entries_and_the_weights():
    src = header()
    assert re.search(r"\bint\s+f16_rollout_cost\s*\(\s*f16_ctx\s*\*", src)
    assert re.search(r"\bint\s+f16_mppi_blend\s*\(\s*f16_ctx\s*\*", src)
    m = re.search(r"typedef\s+struct\s+f16_cost_weights\s*\{([^}]*)\}\s*f16_cost_weights\s*;", src)
    assert m and re.sub(r"\s+", "", m.group(1)) == "doubleq[9],qf[9],r[3],pen;"


def test_library_exports_both_symbols():
    from f16_mpc_oop_py_amd import lib
    L = ctypes.CDLL(lib.build())
    assert hasattr(L, "f16_rollout_cost") and hasattr(L, "f16_mppi_blend")


def test_ctypes_weights_are_22_doubles():
    from f16_mpc_oop_py_amd import lib
    assert ctypes.sizeof(lib.CostWeights) == 22 * 8
    assert [(n, ctypes.sizeof(t) // 8) for n, t in lib.CostWeights._fields_] == [("q", 9), ("qf", 9), ("r", 3), ("pen", 1)]
    w = lib.make_cost_weights()
    assert list(w.q) == [1.0] * 9 and list(w.qf) == [1.0] * 9 and list(w.r) == [1.0] * 3 and w.pen == 0.0
    w = lib.make_cost_weights(q=np.arange(9), r=[3, 2, 1], penalty=7.5)
    assert list(w.q) == list(range(9)) and list(w.r) == [3.0, 2.0, 1.0] and w.pen == 7.5 and list(w.qf) == [1.0] * 9


def test_blend_reference_two_samples_is_the_logistic_weighting():
    import torch
    from f16_mpc_oop_py_amd.mppi import blend_reference
    # K = 2, B = 2, S = 1, one command; aircraft 0: costs (3, 5), aircraft 1: (9, 2); lam = 4
    cost = torch.tensor([[3.0, 9.0], [5.0, 2.0]], dtype=torch.float64)
    act = torch.tensor([[[[10.0], [-1.0]], [[20.0], [4.0]]]], dtype=torch.float64)           # [1, 2, 2, 1]
    u, info = blend_reference(cost, act, 4.0, return_info=True)
    for b, (lo, hi, d) in enumerate(((10.0, 20.0, 2.0), (4.0, -1.0, 7.0))):                     # (the cheaper sample's value, the other's)
        w_lo = 1.0 / (1.0 + math.exp(-d / 4.0))
        assert abs(float(u[0, b, 0]) - (w_lo * lo + (1 - w_lo) * hi)) < 1e-14 * 20
        assert abs(float(info["weights"][:, b].max()) - w_lo) < 1e-15 and abs(float(info["weights"][:, b].sum()) - 1) < 1e-15
        e = math.exp(-d / 4.0)
        assert abs(float(info["ess"][b]) - (1 + e) ** 2 / (1 + e * e)) < 1e-14
    assert info["min_cost"].tolist() == [3.0, 2.0]
    assert tuple(u.shape) == (1, 2, 1)
    with pytest.raises(ValueError):
        blend_reference(cost, act, 0.0)
    with pytest.raises(ValueError):
        blend_reference(cost[:1], act, 1.0)


def test_blend_reference_ignores_nan_and_inf_costs():
    import torch
    from f16_mpc_oop_py_amd.mppi import blend_reference
    rng = np.random.default_rng(3)
    act = rng.normal(size=(3, 5, 4, 4))
    cost = rng.uniform(1, 2, (5, 4))
    cost[1, 0], cost[3, 0], cost[0, 2] = np.nan, np.inf, np.inf
    act[:, 1, 0], act[:, 0, 2] = np.nan, np.inf                    # the commands of those samples must not spread
    u, info = blend_reference(cost, act, 0.5, return_info=True)
    keep = np.array([0, 2, 4])
    ref = blend_reference(cost[keep][:, :1], act[:, keep][:, :, :1], 0.5)
    assert torch.equal(u[:, :1], ref) and bool(torch.isfinite(u).all())
    w = info["weights"].numpy()
    assert w[1, 0] == 0 and w[3, 0] == 0 and w[0, 2] == 0 and np.allclose(w.sum(0), 1, atol=1e-15)


def test_blend_reference_without_a_finite_cost_returns_sample_0():
    import torch
    from f16_mpc_oop_py_amd.mppi import blend_reference
    rng = np.random.default_rng(4)
    act = torch.as_tensor(rng.normal(size=(2, 3, 2, 4)))
    cost = torch.tensor([[np.nan, 1.0], [np.inf, 2.0], [-np.inf, 3.0]], dtype=torch.float64)
    u, info = blend_reference(cost, act, 1.0, return_info=True)
    assert torch.equal(u[:, 0], act[:, 0, 0])
    assert float(info["min_cost"][0]) == 0 and float(info["ess"][0]) == 0 and float(info["weights"][:, 0].abs().max()) == 0
    assert float(info["min_cost"][1]) == 1.0 and float(info["ess"][1]) > 1
