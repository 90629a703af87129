"""The six rollouts in moving air (f16_rollout_wind, f16_rollout_lqr_wind, their _ens twins, f16_rollout_lqg_wind and its _ens twin)
write the bits they wrote before their host path became one launcher (csrc/f16_wind_lanes.hpp: wind_rollout).  The kernels were not
touched by that, so a wrongly filled argument block is the only way to another bit.  Fixture G21 (recorded by
tools/gpu_make_air_rollout_golden.py, which flies the cases of THIS file on the library of the commit before) holds a SHA-256 digest
of every array every case writes: final x, status, u_out, traj, xhat, xhat_traj, gstate and the six arrays of an f16_ens.  No
tolerance, no case left out.

Cases (cases()): per entry point both methods, with and without F16_FLAG_ONE_LANE, and in each of these four combinations three
cases that rotate through
  the air     steady wind only / + a gust_seq at gust_hold 4 / + generated gusts (ga, gb, gstate) at gust_hold 4 / a NULL h_wind
              (the plain calls forward to the _rk sibling; the others fly zero air through the wind kernels)
  the samples mode 0: traj (and xhat_traj) given, traj_every 3;  mode 1: the plain calls traj at traj_every 1, the ensemble calls
              no traj at traj_every 1, the observer calls xhat_traj WITHOUT traj at traj_every 1;  mode 2: no sample array at all
at B = 70 (one full wave and a partial one), nsteps 12, hold 5, dt 10 ms, hifi, ensemble groups of 64.  The default-flag cases run
again at B = 16,400 and 32,800, the smallest batches of the 128-lane and 256-lane instantiations.  Inputs: workload.config2_states(B,
seed=B) with aircraft 3 started above the envelope and aircraft 5 placed 10 ft under its top, climbing: it leaves within the 12 steps
(the recording tool asks the CPU restatement; the step is in the fixture's metadata).

A case with generated gusts is flown a second time as two launches of 7 and 5 steps (samples at every step), the second continuing
the first as a caller would: the schedule from the row step 7 lies in, the gust and measurement counters advanced.  With hold 5 and
gust_hold 4, step 7 lies INSIDE a row of both schedules, where a launch starts new rows (wind.GustModel: "a call whose step count is
not a multiple of `every` ends inside a row; the next call starts a new one"), so that flight is not the one launch of 12 -- in the
recording it ended in another state in 36 of 36 cases -- and is pinned by digests of its own (a7_*, b5_*) instead of by equality."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, REPO

ENTRIES = ("f16_rollout_wind", "f16_rollout_lqr_wind", "f16_rollout_wind_ens", "f16_rollout_lqr_wind_ens", "f16_rollout_lqg_wind",
           "f16_rollout_lqg_wind_ens")
AIRS = ("steady", "gust_seq", "gust_gen", "null")
SIZES = (70, 16400, 32800)
NSTEPS, HOLD, GHOLD, DT, XCG, GROUP = 12, 5, 4, 0.01, 0.25, 64
OUTSIDE, LEAVING = 3, 5            # the two placed aircraft
MPC_IDX = [3, 4, 7, 8, 9, 10, 11, 17, 16]
SENSED, MEAS_SEED, MROW0, GUST_SEED, GROW0 = 0x1ff, 11, 5, 7, 3


def batch(B):
    """x0 [B, 18], u0 [B, 4]: config 2 with the two placed aircraft"""
    from f16_mpc_oop_py_amd.workload import config2_states
    x0, u0 = config2_states(B, seed=B)
    x0[OUTSIDE, 2] = 150000.0
    x0[LEAVING, 2] = 99990.0; x0[LEAVING, 3] = 0.0; x0[LEAVING, 4] = 0.45; x0[LEAVING, 6] = 600.0; x0[LEAVING, 7] = 0.05; x0[LEAVING, 8] = 0.0
    return x0, u0


def cases(B):
    """[(case id, entry, method name, one_lane, air, sample mode)] of one batch size"""
    out = []
    for e, entry in enumerate(ENTRIES):
        for k, (method, one_lane) in enumerate((m, f) for m in ("euler", "rk4") for f in (False, True)):
            if one_lane and B != SIZES[0]:
                continue
            for c in range(3):
                air, mode = AIRS[(e + k + c) % 4], (e + 2 * k + c) % 3
                out.append((f"B{B}/{entry}/{method}{'/one_lane' if one_lane else ''}/{air}/samples{mode}", entry, method, one_lane, air, mode))
    return out


class Flight:
    """the inputs of one batch size on the device, and the calls on them"""

    def __init__(self, B, L=None):
        import torch
        from f16_mpc_oop_py_amd import cabi, lib
        from f16_mpc_oop_py_amd.observer import pack_models
        from f16_mpc_oop_py_amd.wind import gust_coefficients
        self.torch, self.lib, self.L, self.B = torch, lib, L or lib.load(), B
        self.ctx = lib.Context(0)
        self.params = {n: [p for _, p in cabi.functions()[n][1]] for n in ENTRIES}
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.x0h, self.u0h = batch(B)
        dev = self.dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
        rng = np.random.default_rng(B)
        rows = (NSTEPS - 1) // HOLD + 1
        self.x0, self.u0 = dev(self.x0h.T), dev(self.u0h.T)
        self.u_seq = dev(self.u0h.T[None] + rng.normal(0, 0.01, (rows, 4, B)) * np.array([100.0, 1.0, 1.0, 1.0])[None, :, None])
        self.dem_seq = dev(rng.normal(0, 0.02, (rows, 3, B)))
        g = np.load(os.path.join(REPO, "tests", "golden", "g567_trim_lin_lqr.npz"))
        self.K = dev(np.repeat(g["K_lqr_xcg25"].reshape(27, 1), B, 1))
        self.wind = dev(rng.uniform(-20, 20, (3, B)))
        self.gust_seq = dev(rng.normal(0, 5, ((NSTEPS - 1) // GHOLD + 1, 3, B)))
        a, b = gust_coefficients([5.0, 5.0, 3.0], [1750.0, 1750.0, 500.0], 600.0, GHOLD * DT)
        self.ga, self.gb = dev(np.repeat(a[:, None], B, 1)), dev(np.repeat(b[:, None], B, 1))
        self.gstate0 = dev(rng.normal(0, 3, (3, B)))
        self.models = dev(pack_models(g["ssr_Ad_xcg25"][None], g["ssr_Bd_xcg25"][None], (0.3 * np.eye(9))[None], self.x0h[:1, MPC_IDX], self.x0h[:1, 13:16]))
        self.sigma = (ctypes.c_double * 9)(*np.deg2rad([0.1, 0.1, 0.1, 0.1, 0.5, 0.5, 0.5, 0.1, 0.1]))
        self.xhat0 = self.x0[MPC_IDX].clone().contiguous()

    def start(self):
        """fresh state, status, last action, estimate and generator state"""
        t = self.torch
        self.x, self.xhat, self.gstate = self.x0.clone(), self.xhat0.clone(), self.gstate0.clone()
        self.st = t.zeros(self.B, dtype=t.int32, device="cuda:0")
        self.u_out = t.full((4, self.B), -1.0, dtype=t.float64, device="cuda:0")

    def launch(self, entry, method, one_lane, air, mode, nsteps=NSTEPS, first=0, every=None):
        """one call of `entry` for steps first .. first + nsteps of the flight -> {array name: sha256}"""
        t, lib, B = self.torch, self.lib, self.B
        vp = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr())
        lqr, ens, obs = "lqr" in entry or "lqg" in entry, entry.endswith("_ens"), "lqg" in entry
        every = every or (1 if mode == 1 else 3)
        S = nsteps // every
        zeros = lambda *shape, dtype=t.float64: t.zeros(shape, dtype=dtype, device="cuda:0")
        traj = zeros(S, 18, B) if mode == 0 or (mode == 1 and not ens and not obs) else None
        est = zeros(S, 9, B) if obs and mode != 2 else None
        wind = lib.Wind()
        if air != "null":
            wind.wind_ned = self.wind.data_ptr()
        if air == "gust_seq":
            wind.gust_seq, wind.gust_hold = self.gust_seq[first // GHOLD:].data_ptr(), GHOLD
        if air == "gust_gen":
            wind.ga, wind.gb, wind.gstate, wind.gust_hold = self.ga.data_ptr(), self.gb.data_ptr(), self.gstate.data_ptr(), GHOLD
            wind.seed, wind.row0 = GUST_SEED, GROW0 + (first + GHOLD - 1) // GHOLD
        out = {"x": self.x, "status": self.st}
        e = lib.Ens()
        if ens:
            G = (B + GROUP - 1) // GROUP
            res = dict(work=zeros(max(int(self.L.f16_ens_work_doubles(B, S)), 1)), count=zeros(S, G, dtype=t.int32), mean=zeros(S, 18, G), m2=zeros(S, 18, G),
                       min=zeros(S, 18, G), max=zeros(S, 18, G))
            e.group, e.ldg = GROUP, G
            for k, v in res.items():
                setattr(e, k, v.data_ptr())
                out["ens_" + k] = v
        seq = (self.dem_seq if lqr else self.u_seq)[first // HOLD:]
        vals = dict(ctx=self.ctx.handle, x=vp(self.x), u_seq=vp(seq), u0=vp(self.u0), K=vp(self.K), dem_seq=vp(seq),
                    h_wind=None if air == "null" else ctypes.byref(wind), obs=vp(self.models), mgroup=0, sensed=SENSED,
                    h_sigma=ctypes.cast(self.sigma, ctypes.c_void_p), meas_seed=MEAS_SEED, mrow0=MROW0 + first, xhat=vp(self.xhat), traj=vp(traj),
                    xhat_traj=vp(est), h_ens=ctypes.byref(e), u_out=vp(self.u_out), status=vp(self.st), B=B, ld=B, nsteps=nsteps, hold=HOLD,
                    traj_every=every, dt=DT, xcg=XCG, fi_flag=1, method=lib.integrator(method), flags=lib.F16_FLAG_ONE_LANE if one_lane else 0,
                    stream=self.stream)
        lib.check(getattr(self.L, entry)(*(vals[p] for p in self.params[entry])), self.L)
        t.cuda.synchronize()
        out.update({k: v for k, v in (("u_out", self.u_out if lqr else None), ("traj", traj), ("xhat", self.xhat if obs else None), ("xhat_traj", est),
                                      ("gstate", self.gstate if air == "gust_gen" else None)) if v is not None})
        return {k: hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest() for k, v in out.items()}

    def case(self, entry, method, one_lane, air, mode):
        """{array name: sha256} of one case: the one launch, and with generated gusts the 7 + 5 split as a7_* and b5_*"""
        self.start()
        d = self.launch(entry, method, one_lane, air, mode)
        if air == "gust_gen":
            self.start()
            d.update({"a7_" + k: v for k, v in self.launch(entry, method, one_lane, air, mode, nsteps=7, every=1).items()})
            d.update({"b5_" + k: v for k, v in self.launch(entry, method, one_lane, air, mode, nsteps=5, first=7, every=1).items()})
        return d


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "g21_air_rollout_bits.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    ids = [c[0] for B in SIZES for c in cases(B)]
    assert sorted(ids) == sorted(recorded["digests"]) and len(ids) == 144
    meta = recorded["meta"]
    assert (meta["nsteps"], meta["hold"], meta["gust_hold"], meta["group"]) == (NSTEPS, HOLD, GHOLD, GROUP) == (12, 5, 4, 64)
    assert 2 <= meta["leaves_after_step"] <= 10


@pytest.mark.gpu
@pytest.mark.parametrize("B", SIZES)
def test_bits_of_the_recording(hip, recorded, B):
    flight = Flight(B, hip)
    wrong = []
    for cid, *case in cases(B):
        got, want = flight.case(*case), recorded["digests"][cid]
        assert sorted(got) == sorted(want), (cid, sorted(got), sorted(want))
        wrong += [f"{cid}: {k}" for k in want if got[k] != want[k]]
    assert not wrong, f"{len(wrong)} arrays with other bits than recorded: {wrong[:20]}"
