"""The model stage of the control chain -- linearise, ZOH, dlqr, and the loops that run them per step -- writes the bits it wrote before
the forward-difference rule of the reduced model became one definition (csrc/f16_linearise.hpp).  That change alters the instruction
streams of k_linearise, k_lqr, k_rollout_lqr_relin, the k_mpc instantiations and wave::pair_model / pair_prepare, so "the same device
code" is no yardstick for them; the bits are.  Fixture G22 (recorded by tools/gpu_make_model_stage_golden.py, which flies the cases of
THIS file on the library of the commit before) holds a SHA-256 digest of every array every case writes.  No tolerance, no case left
out.

Cases (cases()), all through the C ABI:
  1 linearise   f16_linearise_batch / f16_linearise_full_batch on the lattice of every family of tests/linearise_cases.py (FAMILIES,
                EPS_FAMILY, FIX_CLR_FAMILIES) and on the three launch paths of tests/test_gpu_linearise.py: <64> (the family in two
                halves), <256> and <256> with its grid-stride loop (the family tiled).  Ac, Bc, Cc, status per path.
  2 c2d_lqr     f16_c2d_batch, f16_c2d_full_batch, f16_lqr_batch and f16_lqr_batch_w (Q = I, R = 1e4 I) on group 1's models of the two
                hifi, xcg 0.25 families (the first B rows of the lattice, repeated cyclically), at B = 70 and B = 8,200: the smallest
                batch with a second pass of the 8,192-workgroup grid.
  3 lqr_relin   f16_rollout_lqr_relin and f16_rollout_lqr_relin_sched (hold 5) on test_gpu_air_rollout_bits.batch(B) -- aircraft 3
                starts outside the envelope, aircraft 5 leaves it inside the flight -- at B = 70 and 8,200: 12 steps, dt 10 ms, hifi;
                weights NULL | Q = I, R = 1e4 I; track_mask 0x1FF | 0x70; traj_every 1 | 3; and one lofi case at B = 70.
                x, u, status, traj, u_traj, K_traj.
  4 mpc_loop    the states and settings of tests/test_gpu_mpc_relin.py at B = 70, hzn 10, six control steps: f16_rollout_mpc_relin,
                f16_rollout_mpc_relin_hold (hold 2), f16_rollout_mpc_relin_sched (a new demand every second control step), model_every 1,
                and the frozen f16_rollout_mpc; each with hard rows and with soft state rows (weight 100).  x, u, status, traj,
                cmd_traj, iters_traj, model_traj.
  5 mpc_batch   the one-shot f16_mpc_batch_w at B = 70, hzn 10 (one-wavefront solver) and hzn 40 (workgroup solver), default weights
                and Q = I, R = 1e4 I.  u_cmd, u_seq, info, status."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import linearise_cases as lc
from conftest import GOLDEN
from test_gpu_air_rollout_bits import LEAVING, OUTSIDE, batch as air_batch
from test_gpu_linearise import thresholds

FAMILIES = lc.FAMILIES + [lc.EPS_FAMILY] + lc.FIX_CLR_FAMILIES
NA25, FULL25 = lc.Family("na", "hifi", 0.25), lc.Family("full", "hifi", 0.25)
SIZES = (70, 8200)
MODEL_DT = 0.001                                   # the ZOH period of groups 2, 4 and 5 (parameters.py: dt)
NSTEPS, HOLD, LQR_DT, LQR_XCG, EPS = 12, 5, 0.01, 0.25, 1e-5      # group 3
MPC_B, MPC_T, MPC_XCG, MPC_DEM, SOFT_W = 70, 6, 0.35, (0.02, -0.01, 0.0), 100.0      # groups 4 and 5 (tests/test_gpu_mpc_relin.py)
MPC_LOOPS = ("f16_rollout_mpc_relin", "f16_rollout_mpc_relin_hold", "f16_rollout_mpc_relin_sched", "f16_rollout_mpc")


def cases():
    """[(case id, method of Stage, its arguments)]"""
    out = [(f"linearise/{f.model}/{f.fidelity}/xcg{f.xcg}/eps{f.eps:g}/clr{f.fix_clr}", "linearise", (f,)) for f in FAMILIES]
    out += [(f"c2d_lqr/B{B}", "c2d_lqr", (B,)) for B in SIZES]
    for B in SIZES:
        for sched in (False, True):
            for custom in (False, True):
                for track in (0x1FF, 0x70):
                    for every in (1, 3):
                        out.append((f"lqr_relin/B{B}/{'sched' if sched else 'plain'}/hifi/{'qr' if custom else 'null'}/track{track:x}/every{every}",
                                    "lqr_relin", (B, sched, 1, custom, track, every)))
    out.append((f"lqr_relin/B{SIZES[0]}/plain/lofi/null/track1ff/every1", "lqr_relin", (SIZES[0], False, 0, False, 0x1FF, 1)))
    out += [(f"mpc_loop/{entry}/{'soft' if soft else 'hard'}", "mpc_loop", (entry, soft)) for entry in MPC_LOOPS for soft in (False, True)]
    out += [(f"mpc_batch/hzn{N}/{'qr' if custom else 'null'}", "mpc_batch", (N, custom)) for N in (10, 40) for custom in (False, True)]
    return out


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


class Stage:
    """the calls of the five groups; every method returns {array name: sha256}"""

    def __init__(self, L=None):
        import torch
        from f16_mpc_oop_py_amd import cabi, lib
        self.t, self.lib, self.L = torch, lib, L or lib.load()
        self.ctx = lib.Context(0)
        self.params = {n: [p for _, p in sig[1]] for n, sig in cabi.functions().items()}
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.status = None                             # the status words of the last lqr_relin case (the recording tool reads them)
        self._cache = {}

    def dev(self, a):
        return self.t.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")

    def new(self, *shape, dtype=None):
        """an output buffer: filled with a value no result takes, so that an element a call leaves out shows in the digest"""
        t = self.t
        return t.full(shape, -7 if dtype is t.int32 else -7.25, dtype=dtype or t.float64, device="cuda:0")

    def words(self, B):
        return self.t.zeros(B, dtype=self.t.int32, device="cuda:0")

    def weights(self, custom):
        """NULL, or Q = I, R = 1e4 I"""
        if not custom:
            return None
        if "w" not in self._cache:
            w = self.lib.MPCWeights()
            self.L.f16_mpc_default_weights(ctypes.byref(w))
            w.q_from_cd = 0
            w.Q[:] = list(np.eye(9).reshape(81))
            w.R[:] = list((1e4 * np.eye(3)).reshape(9))
            self._cache["w"] = w
        return ctypes.byref(self._cache["w"])

    def call(self, entry, **vals):
        vals.setdefault("stream", self.stream)
        if "ctx" in self.params[entry]:                # (the closed MPC loops take a plan instead)
            vals.setdefault("ctx", self.ctx.handle)
        ptr = lambda v: ctypes.c_void_p(v.data_ptr()) if self.t.is_tensor(v) else v
        args = [ptr(vals.pop(p)) for p in self.params[entry]]
        assert not vals, (entry, sorted(vals))
        self.lib.check(getattr(self.L, entry)(*args), self.L)
        self.t.cuda.synchronize()

    # ---- group 1
    def lattice(self, fam):
        if fam.fidelity not in self._cache:
            self._cache[fam.fidelity] = lc.batch(fam)
        return self._cache[fam.fidelity]

    def linearise_call(self, fam, x, u):
        """one call at the family's settings on x [B, 18], u [B, 4] -> dict(Ac, Bc, Cc, status) on the device"""
        ns, ni, no = lc.dims(fam.model)
        B = len(x)
        o = dict(Ac=self.new(ns * ns, B), Bc=self.new(ns * ni, B), Cc=self.new(no * ns, B), status=self.words(B))
        self.call("f16_linearise_batch" if fam.model == "na" else "f16_linearise_full_batch", x=self.dev(x.T), u=self.dev(u.T), B=B, ld=B,
                  eps=fam.eps, xcg=fam.xcg, fi_flag=1 if fam.fidelity == "hifi" else 0, flags=lc.FLAG_FIX_CLR if fam.fix_clr else 0, **o)
        return o

    def linearise(self, fam):
        b = self.lattice(fam)
        B0 = len(b.x)
        t64, t256 = thresholds(fam.model)
        h, n1, n2 = (B0 + 1) // 2, t64 // B0 + 1, t256 // B0 + 1
        assert h <= t64 < n1 * B0 <= t256 < n2 * B0
        halves = [self.linearise_call(fam, b.x[:h], b.u[:h]), self.linearise_call(fam, b.x[h:], b.u[h:])]
        out = {f"p64_{k}": sha(halves[0][k], halves[1][k]) for k in halves[0]}
        for name, n in (("p256", n1), ("p256_strided", n2)):
            out.update({f"{name}_{k}": sha(v) for k, v in self.linearise_call(fam, np.tile(b.x, (n, 1)), np.tile(b.u, (n, 1))).items()})
        return out

    # ---- group 2
    def c2d_lqr(self, B):
        b = self.lattice(NA25)
        rows = np.arange(B) % len(b.x)
        na, full = self.linearise_call(NA25, b.x[rows], b.u[rows]), self.linearise_call(FULL25, b.x[rows], b.u[rows])
        Ad, Bd, Adf, Bdf = self.new(81, B), self.new(27, B), self.new(324, B), self.new(72, B)
        self.call("f16_c2d_batch", Ac=na["Ac"], Bc=na["Bc"], Ad=Ad, Bd=Bd, B=B, ld=B, dt=MODEL_DT)
        self.call("f16_c2d_full_batch", Ac=full["Ac"], Bc=full["Bc"], Ad=Adf, Bd=Bdf, B=B, ld=B, dt=MODEL_DT)
        out = dict(c2d_Ad=sha(Ad), c2d_Bd=sha(Bd), c2d_full_Ad=sha(Adf), c2d_full_Bd=sha(Bdf))
        for name, custom in (("lqr", False), ("lqr_w", True)):
            o = dict(K=self.new(27, B), Pare=self.new(81, B), status=self.words(B))
            self.call("f16_lqr_batch_w" if custom else "f16_lqr_batch", Ad=Ad, Bd=Bd, Cd=na["Cc"], B=B, ld=B,
                      **(dict(h_w=self.weights(True)) if custom else {}), **o)
            out.update({f"{name}_{k}": sha(v) for k, v in o.items()})
        return out

    # ---- group 3
    def lqr_relin(self, B, sched, fi, custom, track, every):
        if ("air", B) not in self._cache:
            x0, u0 = air_batch(B)
            ref = x0[:, lc.MPC_X_IDX].T[None] + np.random.default_rng(B).normal(0, 0.01, ((NSTEPS - 1) // HOLD + 1, 9, B))
            self._cache["air", B] = (self.dev(x0.T), self.dev(u0.T), self.dev(ref), self.dev(u0[:, 1:4].T))
        x0, u0, ref, u03 = self._cache["air", B]
        S = NSTEPS // every
        x, u, st = x0.clone(), u0.clone(), self.words(B)
        o = dict(traj=self.new(S, 18, B), u_traj=self.new(S, 3, B), K_traj=self.new(S, 27, B))
        self.call("f16_rollout_lqr_relin_sched" if sched else "f16_rollout_lqr_relin", x=x, u=u, u0=u03, h_w=self.weights(custom), status=st,
                  B=B, ld=B, nsteps=NSTEPS, traj_every=every, track_mask=track, eps=EPS, dt=LQR_DT, xcg=LQR_XCG, fi_flag=fi, flags=0,
                  **(dict(xref_seq=ref, hold=HOLD) if sched else dict(x_ref=ref)), **o)
        self.status = st.cpu().numpy()
        return {k: sha(v) for k, v in dict(o, x=x, u=u, status=st).items()}

    # ---- groups 4 and 5
    def mpc_inputs(self, dt):
        """config4_states(70, seed=9) on the device and the reduced model at them, through the ZOH at dt: x, u, dem, (Ad, Bd, Cd)"""
        if ("mpc", dt) not in self._cache:
            from f16_mpc_oop_py_amd.workload import config4_states
            x0, u0 = config4_states(MPC_B, seed=9)
            m = self.linearise_call(lc.Family("na", "hifi", MPC_XCG), x0, u0)
            Ad, Bd = self.new(81, MPC_B), self.new(27, MPC_B)
            self.call("f16_c2d_batch", Ac=m["Ac"], Bc=m["Bc"], Ad=Ad, Bd=Bd, B=MPC_B, ld=MPC_B, dt=dt)
            dem = self.dev(np.repeat(np.array(MPC_DEM)[:, None], MPC_B, 1))
            self._cache["mpc", dt] = (self.dev(x0.T), self.dev(u0.T), dem, (Ad, Bd, m["Cc"]))
        return self._cache["mpc", dt]

    def mpc_loop(self, entry, soft, N=10):
        t, B, T = self.t, MPC_B, MPC_T
        relin, hold = "relin" in entry, 2 if entry.endswith("_hold") else 1
        x0, u0, dem, (Ad, Bd, Cd) = self.mpc_inputs(hold * MODEL_DT)
        x, u, st = x0.clone(), u0.clone(), self.words(B)
        o = dict(traj=self.new(T * hold, 18, B), cmd_traj=self.new(T, 3, B), iters_traj=self.new(T, B, dtype=t.int32))
        if relin:
            o["model_traj"] = self.new(T, 189, B)
        vals = dict(x=x, u=u, status=st, traj_every=1, xcg=MPC_XCG, fi_flag=1, flags=0, **o)
        if entry.endswith("_sched"):      # a new demand every second control step
            rows = np.array(MPC_DEM)[None, :, None] + np.array([0.0, 0.01, -0.02])[:, None, None] * np.array([1.0, -1.0, 0.5])[None, :, None]
            vals.update(dem_seq=self.dev(np.repeat(rows, B, 2)), dem_hold=2)
        else:
            vals.update(dem=dem)
        if relin:
            vals.update(eps=EPS)
        if entry.endswith(("_hold", "_sched")):
            vals.update(nctrl=T, hold=hold, dt=MODEL_DT, **(dict(model_every=1) if relin else {}))
        else:
            vals.update(nsteps=T)
        plan = ctypes.c_void_p()
        self.call("f16_mpc_plan_create_w", plan=ctypes.byref(plan), Ad=Ad, Bd=Bd, Cd=Cd, h_w=None, B=B, ld=B, hzn=N, dt=hold * MODEL_DT, s=None)
        try:
            if soft:
                self.lib.check(self.L.f16_mpc_plan_soft_rows(plan, (ctypes.c_double * 9)(0, 0, SOFT_W, SOFT_W, SOFT_W, SOFT_W, SOFT_W, 0, SOFT_W)), self.L)
            self.call(entry, plan=plan, **vals)
        finally:
            self.L.f16_mpc_plan_destroy(plan)
        return {k: sha(v) for k, v in dict(o, x=x, u=u, status=st).items()}

    def mpc_batch(self, N, custom):
        B = MPC_B
        x0, _, dem, (Ad, Bd, Cd) = self.mpc_inputs(MODEL_DT)
        o = dict(u_cmd=self.new(3, B), u_seq=self.new(3 * N, B), info=self.new(4, B), status=self.words(B))
        self.call("f16_mpc_batch_w", Ad=Ad, Bd=Bd, Cd=Cd, x=x0, dem=dem, x_ref=None, h_w=self.weights(custom), B=B, ld=B, hzn=N, dt=MODEL_DT, s=None, **o)
        return {k: sha(v) for k, v in o.items()}

    def case(self, method, args):
        return getattr(self, method)(*args)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "g22_model_stage_bits.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def stage(hip):
    return Stage(hip)


def test_every_case_is_recorded(recorded):
    ids = [c[0] for c in cases()]
    assert sorted(ids) == sorted(recorded["digests"]) and len(ids) == len(set(ids)) == 13 + 2 + 33 + 8 + 4
    meta = recorded["meta"]
    assert (meta["nsteps"], meta["hold"], meta["outside"], meta["leaving"]) == (NSTEPS, HOLD, OUTSIDE, LEAVING) == (12, 5, 3, 5)
    assert 2 <= meta["leaves_after_step"] <= 10


@pytest.mark.gpu
@pytest.mark.parametrize("cid,method,args", cases(), ids=[c[0] for c in cases()])
def test_bits_of_the_recording(stage, recorded, cid, method, args):
    got, want = stage.case(method, args), recorded["digests"][cid]
    assert sorted(got) == sorted(want), (cid, sorted(got), sorted(want))
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, f"{cid}: arrays with other bits than recorded: {wrong}"
