"""The conditions tests/test_gpu_envelope.py rests on, checked with the C restatement alone (no GPU): the whole-envelope batches of
tests/envelope_cases.py hit every cell of every table axis, keep every edge row, give finite restated rollouts, are well conditioned
(the restatement on x0 and on x0 moved by one ulp stay within 1e-12 over every case the GPU tests run) and have a near-edge set
below its cap.

Measured here (seed 1, spread of the restatement against its ulp-perturbed twins over the aircraft that are not near an edge):
hifi 40 steps 1.0e-14, 100 steps 2.6e-14, high rates 1.2e-14, dt = 10 ms x 8 steps 1.8e-14, schedule 8.6e-15, LQR loop 1.2e-14;
lofi 7.1e-15, 2.3e-14, 8.1e-15, 2.2e-14, 4.5e-15, 5.2e-15.  The near-edge set holds the deliberate on-edge rows and nothing else."""
import numpy as np
import pytest

import envelope_cases as ec

LATTICES = {"hifi": ec.hifi_lattice, "lofi": ec.lofi_lattice}


@pytest.mark.parametrize("which", ["hifi", "lofi"])
def test_every_cell_of_every_axis_is_hit_once(which):
    """from the breakpoints (searchsorted on the degrees the plant forms), not from the ranges the rows were drawn from"""
    b = LATTICES[which]()
    n = b.n_lattice
    cells = ec.cell_of(b)[:n]
    shape = tuple(len(a) - 1 for a in b.axes)
    assert n == int(np.prod(shape)) and n == {"hifi": 19 * 18 * 4, "lofi": 11 * 12 * 4}[which]
    assert (cells >= 0).all() and (cells < shape).all()
    assert len(np.unique(np.ravel_multi_index(cells.T, shape))) == n              # every (alpha, beta, elevator) cell exactly once
    assert np.array_equal(cells, b.cell[:n])
    v = ec.axis_values(b)[:n]
    for k, a in enumerate(b.axes):                                               # strictly inside: nodes have rows of their own
        assert (v[:, k] > a[cells[:, k]]).all() and (v[:, k] < a[cells[:, k] + 1]).all()
    assert b.B % 16 != 0 and b.B % 64 != 0
    for hr in (ec.high_rate(b),):
        assert np.array_equal(np.delete(hr.x, [4, 9, 10, 11], 1), np.delete(b.x, [4, 9, 10, 11], 1))
        assert np.abs(hr.x[:, 9:12]).max() > 7.9 and (np.abs(hr.x[:, 9:12]) * 0.001 > 4e-3).mean() > 0.3   # straddles 4e-3 rad per step
        assert (np.abs(hr.x[:, 9:12]) * 0.001 < 4e-3).mean() > 0.3


def test_no_hifi_edge_row_is_lost(oracle):
    b = ec.hifi_lattice()
    v, e = ec.axis_values(b), b.edge
    up, dn = (lambda d: np.nextafter(d, np.inf)), (lambda d: np.nextafter(d, -np.inf))
    A, Bt, E = 0, 1, 2
    exact = {"alpha_node": (A, 10.0), "beta_node": (Bt, -4.0), "el_node": (E, 10.0), "el_node_held": (E, -10.0),
             "alpha_first": (A, -20.0), "alpha_last": (A, 90.0), "alpha2_last": (A, 45.0), "el_first": (E, -25.0), "el_last": (E, 25.0),
             "alpha_node_up": (A, up(20.0)), "alpha_node_dn": (A, dn(20.0)), "beta_node_up": (Bt, up(6.0)), "beta_node_dn": (Bt, dn(6.0)),
             "el_node_up": (E, up(10.0)), "el_node_dn": (E, dn(10.0))}
    for name, (k, val) in exact.items():
        assert v[e[name], k] == val, name                                        # the degree value in the plant, bit for bit
    assert tuple(v[e["all_nodes"]]) == (25.0, 8.0, 0.0)
    # +-30 deg: no double converts to it exactly, so the pair of neighbours that straddles it
    assert v[e["beta_first"], Bt] == up(-30.0) and v[e["beta_first_out"], Bt] == dn(-30.0)
    assert v[e["beta_last"], Bt] == dn(30.0) and v[e["beta_last_out"], Bt] == up(30.0)
    for name, k in (("beta_neg_zero", Bt), ("el_neg_zero", E)):
        assert v[e[name], k] == 0.0 and np.signbit(v[e[name], k]), name
    assert b.x[e["alt_35000"], 2] == 35000.0 and b.x[e["alt_below_35000"], 2] == np.nextafter(35000.0, 0.0)
    # what the restatement makes of the rows off the grid and outside the box (status after 40 steps)
    r = ec.reference(oracle, "hifi40")
    st = r["status"]
    want = {"off_alpha1_hi": 1 | 2, "off_alpha1_lo": 1 | 2, "off_alpha2": 2, "off_beta_hi": 4, "off_beta_lo": 4,
            "off_el_hi": 16 | 1 << (8 + 13), "off_el_lo": 16 | 1 << (8 + 13), "out_alt_rudder": 16 | 1 << (8 + 2) | 1 << (8 + 15),
            "out_thrust": 16 | 1 << (8 + 12), "alpha_node": 0, "all_nodes": 0, "beta_last_out": 4}
    for name, bits in want.items():
        assert st[e[name]] == bits, (name, st[e[name]])
    ne = ec.reference(oracle, "hifi_noenv40")["status"]
    assert ne[e["off_el_hi"]] == 8 and ne[e["off_el_lo"]] == 8 and not (ne & 16).any()   # the elevator bit needs the box test off
    # the sixteen climbers start below 35,000 ft and end above it inside 40 steps: the temperature branch is crossed in a rollout
    climb = [e[f"climb_{j}"] for j in range(16)]
    alt = r["traj"][:, climb, 2]
    assert (b.x[climb, 2] < 35000.0).all() and (alt[-1] > 35000.0).all() and len(set(np.argmax(alt >= 35000.0, 0))) >= 8
    assert climb == list(range(climb[0], climb[0] + 16))
    # every actuator limit acts in both directions somewhere in the batch (utils.py:308-330: position clip, then rate clip)
    lim = np.array([19000, 25, 21.5, 30.0])
    rate = np.array([10000, 60, 80, 120.0])
    gain = np.array([1.0, 20.2, 20.2, 20.2])
    cmd = np.clip(b.u, [1000, -25, -21.5, -30], lim)
    for k in range(4):
        assert (b.u[:, k] > lim[k]).any() and (b.u[:, k] < [1000, -25, -21.5, -30][k]).any(), k
        d = gain[k] * (cmd[:, k] - b.x[:, 12 + k])
        assert (d > rate[k]).any() and (d < -rate[k]).any() and (np.abs(d) < rate[k]).any(), k


def test_no_lofi_edge_row_is_lost(oracle):
    b = ec.lofi_lattice()
    v, e = ec.axis_values(b), b.edge
    for name, (k, val) in {"alpha_node": (0, 10.0), "alpha_zero": (0, 0.0), "beta_node": (1, -10.0), "el_node": (2, 12.0),
                           "alpha_first": (0, -10.0), "alpha_last": (0, 45.0), "el_first": (2, -24.0), "el_last": (2, 24.0),
                           "el_box": (2, 25.0)}.items():
        assert v[e[name], k] == val, name
    assert tuple(v[e["all_nodes"]]) == (25.0, 5.0, 0.0)
    assert v[e["beta_last"], 1] == np.nextafter(30.0, 0) and v[e["beta_last_out"], 1] == np.nextafter(30.0, 99)
    assert np.signbit(v[e["beta_neg_zero"], 1]) and np.signbit(v[e["el_neg_zero"], 2])
    r = ec.reference(oracle, "lofi40")
    st = r["status"]
    # (beta_last is the double below 30 deg: the reference's row index fix(0.2 |beta|) is 6 there already -- the product rounds to
    # 6.0 -- so that value reads past the table like 30 deg itself and carries the bit)
    assert 0.2 * v[e["beta_last"], 1] == 6.0
    for name, bits in {"off_beta_hi": 4, "off_beta_lo": 4, "off_alpha_hi": 0, "off_alpha_lo": 0, "beta_last_out": 4, "beta_last": 4,
                       "beta_first": 4, "beta_node": 0,
                       "out_alt_rudder": 16 | 1 << (8 + 2) | 1 << (8 + 15), "out_thrust": 16 | 1 << (8 + 12)}.items():
        assert st[e[name]] == bits, (name, st[e[name]])
    climb = [e[f"climb_{j}"] for j in range(16)]
    assert (b.x[climb, 2] < 35000.0).all() and (r["traj"][-1, climb, 2] > 35000.0).all()


@pytest.mark.parametrize("name", list(ec.CASES))
def test_restated_case_is_finite_well_conditioned_and_rarely_near_an_edge(oracle, name):
    r = ec.reference(oracle, name)
    b = r["batch"]
    frozen_at_start = ((b.x < ec.X_LB) | (b.x > ec.X_UB)).any(1) & (not r["noenv"])
    # finite for every aircraft the restatement steps (a frozen one keeps its finite initial state)
    assert np.isfinite(r["traj"]).all() and r["finite"].all()
    assert np.array_equal(frozen_at_start, (r["traj"][-1] == b.x).all(1))
    # conditioning, over every aircraft that is not near an edge: one ulp in x0 moves nothing by more than 1e-12
    free = ~r["near"]
    print(f"{name}: B = {b.B}, spread against the ulp-perturbed twins {r['spread'][free].max():.2e}, near-edge {int(r['near'].sum())}, "
          f"status bits in use {sorted(set(r['status'] & 63))}")
    assert r["spread"][free].max() < 1e-12
    assert r["twins_status_equal"][free].all()                                   # and no status bit
    # near-edge set: the deliberate on-edge rows, and at most 0.5 % of the batch beside them
    deliberate = np.zeros(b.B, dtype=bool)
    deliberate[[b.edge[k] for k in ec.ON_EDGE if k in b.edge]] = True
    assert (r["near"] & ~deliberate).sum() <= 0.005 * b.B
    assert r["near"].sum() <= deliberate.sum() + 0.005 * b.B
    # what is compared on the GPU is nearly everything
    assert r["states_ok"].sum() >= b.B - 4 and r["status_ok"].sum() >= b.B - len(ec.ON_EDGE) - 0.005 * b.B
    assert r["states_ok"][:b.n_lattice].all() and r["status_ok"][:b.n_lattice].sum() >= b.n_lattice * 0.995
    if not r["noenv"] and r["kind"] == "open" and not r["rate"]:
        # one aircraft leaves the box on the way (speed above 900 ft/s) and is frozen there: it takes at least one step and misses at least one
        k = b.edge["vt_leaves"]
        first = int(np.argmax((r["traj"][1:, k] == r["traj"][:-1, k]).all(1))) + 1
        assert r["status"][k] == 16 | 1 << (8 + 6) and 1 <= first < r["T"] - 1, (r["status"][k], first)
        assert r["traj"][first - 1, k, 6] > 900.0 and free[k]


def test_the_lattice_moves_through_cells_and_status_bits(oracle):
    """the rollouts do what the batch is for: aircraft change cells on every axis, and every grid bit occurs"""
    r = ec.reference(oracle, "hifi_rate40")
    b = r["batch"]
    c0, c1 = ec.cell_of(b)[:b.n_lattice], ec.cell_of(b, r["traj"][-1])[:b.n_lattice]
    moved = (c0 != c1) & ~(r["status"][:b.n_lattice, None] & 16 != 0)
    assert moved[:, 0].sum() > 100 and moved[:, 1].sum() > 100 and moved[:, 2].sum() > 20
    seen = np.bitwise_or.reduce(ec.reference(oracle, "hifi_noenv40")["status"])
    assert seen & 15 == 15
