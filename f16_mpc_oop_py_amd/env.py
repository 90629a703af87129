"""Batched mirror of the reference's `F16` environment (env.py:29-436).

Same method names and argument meaning as the reference class, over a leading batch dimension B:
`step / reset / get_obs / _calc_xdot / _calc_xdot_na / linearise / _calc_LQR_gain /
_calc_LQR_action / _calc_MPC_action (calc_MPC_action)`.  Where the reference holds one
`x.values[18]` NumPy vector and calls `nlplant.Nlplant` through ctypes once per evaluation
(env.py:100), this class holds the states of B aircraft resident in HBM, state-major
([18, B] fp64, so that a wavefront's 64 lanes read contiguous memory), and calls the batched
entry points of libf16hip.so through the same ctypes mechanism.  torch is used only to own
device memory and streams.  There is no CPU path in this class.
"""
import ctypes

import numpy as np
import torch

from . import cabi as _cabi
from . import lib as _lib
from . import parameters as P


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class F16Batch:
    def __init__(self, x0, u0=None, *, stab_flag=None, xcg=None, fi_flag=P.fi_flag, dt=P.dt, device="cuda:0",
                 flags=0, context=None):
        """x0: [B,18] (or [18]) initial states in the reference's state order/units
        (parameters.py:116-119); u0: [B,4] inputs, default = x0[:,12:16] (env.py:43).
        stab_flag / xcg: parameters.py:31 (1 -> 0.35) or an explicit value."""
        if not torch.cuda.is_available():
            raise _lib.F16HipError("F16Batch needs an AMD GPU (no CPU fallback)")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.ctx = context or _lib.Context(self.device.index or 0)
        self.lib = self.ctx.lib
        self.xcg = float(xcg) if xcg is not None else P.xcg_of(P.stab_flag if stab_flag is None else stab_flag)
        self.fi_flag = int(fi_flag)
        self.dt = float(dt)
        self.flags = int(flags)
        # host arrays, or tensors already on the device (from_trim: the trim states never leave HBM)
        as2d = lambda a: (a if a.dim() == 2 else a.unsqueeze(0)).to(torch.float64) if isinstance(a, torch.Tensor) \
            else torch.as_tensor(np.atleast_2d(np.asarray(a, dtype=np.float64)))
        x0 = as2d(x0)
        self.B = x0.shape[0]
        assert x0.shape[1] == 18
        u0 = x0[:, 12:16] if u0 is None else as2d(u0)
        self._x_init = self._soa(x0)            # x.initial_condition
        self._u_init = self._soa(u0)            # u.initial_condition
        self._x = self._x_init.clone()          # x.values  [18,B]
        self._u = self._u_init.clone()          # u.values  [4,B]
        self.status = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self.ssr = None                         # (Ad,Bd,Cd) per aircraft once linearised (env.py:49-60)

    # ------------------------------------------------------------------ env.py:198-292
    @staticmethod
    def trim(h_t, v_t, gamma=None, turn_rate=None, pullup_rate=None, runs=2, q0=None, *, stab_flag=None, xcg=None, fi_flag=P.fi_flag,
             device="cuda:0", flags=0, maxiter=50000, context=None):
        """Batched F16.trim: straight-and-level trim at altitudes h_t [B] (ft) and airspeeds v_t [B] (ft/s) by the
        reference's Nelder-Mead, all conditions in one launch.  Returns (x_trim [B,18], info dict).
        `maxiter` and info["iters"] are scipy's option `maxiter` and result `nit`: the counter starts at 1, so at most
        maxiter - 1 iterations are performed, iters = performed + 1, and the F16_ST_QP_MAXITER bit of info["status"] is scipy's
        status 2 (iters >= maxiter); info["nfev"] is scipy's nfev (include/f16_hip.h: f16_trim_batch).

        With any of gamma (flight-path angle, rad), turn_rate (psi_dot, rad/s) or pullup_rate (theta_dot, rad/s) -- a scalar or
        [B] each -- the trim is the steady climb, coordinated turn or pull-up of include/f16_hip.h: f16_trim_man_batch: six
        unknowns (the sideslip is free), `runs` Nelder-Mead runs each from the best point of the last (one run stalls, two
        converge), q0 [B, 6] or [6] an optional start (P3, dh, da, dr, alpha, beta); iters and nfev are totals over the runs.
        With all three None the call is f16_trim_batch as before (runs and q0 are not read)."""
        if not torch.cuda.is_available():
            raise _lib.F16HipError("trim needs an AMD GPU (no CPU fallback)")
        dev = torch.device(device)
        torch.cuda.set_device(dev)
        ctx = context or _lib.Context(dev.index or 0)
        xcg = float(xcg) if xcg is not None else P.xcg_of(P.stab_flag if stab_flag is None else stab_flag)
        h = torch.as_tensor(np.atleast_1d(np.asarray(h_t, dtype=np.float64)), device=dev)
        v = torch.as_tensor(np.atleast_1d(np.asarray(v_t, dtype=np.float64)), device=dev)
        B = h.shape[0]
        assert v.shape[0] == B
        xt = torch.empty((18, B), dtype=torch.float64, device=dev)
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        iters = torch.zeros(B, dtype=torch.int32, device=dev)
        nfev = torch.zeros(B, dtype=torch.int32, device=dev)
        st = torch.zeros(B, dtype=torch.int32, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if gamma is None and turn_rate is None and pullup_rate is None:
            _lib.check(ctx.lib.f16_trim_batch(ctx.handle, _vp(h), _vp(v), _vp(xt), _vp(cost), _vp(iters), _vp(nfev), _vp(st), B, B,
                                              xcg, int(fi_flag), int(flags), int(maxiter), None, stream), ctx.lib)
        else:
            given = lambda a: None if a is None else torch.as_tensor(np.array(np.broadcast_to(np.asarray(a, dtype=np.float64), (B,))), device=dev)
            g, pd, td = given(gamma), given(turn_rate), given(pullup_rate)
            q = None if q0 is None else torch.as_tensor(np.array(np.broadcast_to(np.asarray(q0, dtype=np.float64), (B, 6)).T, order="C"),
                                                        device=dev)       # [6][B]
            _lib.check(ctx.lib.f16_trim_man_batch(ctx.handle, _vp(h), _vp(v), _vp(g), _vp(pd), _vp(td), _vp(q), _vp(xt), _vp(cost),
                                                  _vp(iters), _vp(nfev), _vp(st), B, B, xcg, int(fi_flag), int(flags), int(maxiter),
                                                  int(runs), stream), ctx.lib)
        return xt.t(), dict(cost=cost, iters=iters, nfev=nfev, status=st, context=ctx)

    @classmethod
    def from_trim(cls, h_t, v_t, **kw):
        """env.py:42-44: construct the batch at its trim points (x.initial_condition = trim, u = x[12:16])."""
        man = ("gamma", "turn_rate", "pullup_rate", "runs", "q0")     # the manoeuvre of F16Batch.trim, passed through
        tk = {k: kw[k] for k in ("stab_flag", "xcg", "fi_flag", "device", "flags") + man if k in kw}
        x, info = cls.trim(h_t, v_t, **tk)            # [B,18] view of the device-resident [18,B] result
        env = cls(x, None, context=info["context"], **{k: v for k, v in kw.items() if k != "maxiter" and k not in man})
        env.trim_info = info
        return env

    # ------------------------------------------------------------------ helpers
    def _soa(self, a, rows=None):
        """[B,k] (or [k], broadcast) host/device array -> contiguous state-major [k,B] fp64 on the GPU."""
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))
        t = t.to(device=self.device, dtype=torch.float64)
        if t.dim() == 1:
            t = t.unsqueeze(0).expand(self.B, -1)
        if rows is not None:
            assert t.shape[1] == rows, (tuple(t.shape), rows)
        out = t.t().contiguous()
        # (a [k,B] device tensor viewed as [B,k] comes back as the SAME storage: the resident copies must not alias their source)
        return out.clone() if isinstance(a, torch.Tensor) and out.data_ptr() == a.data_ptr() else out

    @property
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc):
        _lib.check(rc, self.lib)

    @staticmethod
    def _schedule_steps(hold, nsteps, rows, name):
        """A zero-order-hold schedule of `rows` rows (held by `name`), step t reading row t // hold: hold >= 1, nsteps defaults to
        rows * hold, and the ceil(nsteps / hold) rows it reads must be there.  Returns (hold, nsteps) as ints."""
        hold = int(hold)
        if hold < 1:
            raise ValueError("hold must be >= 1")
        nsteps = rows * hold if nsteps is None else int(nsteps)
        if nsteps < 1 or (nsteps + hold - 1) // hold > rows:
            raise ValueError(f"{nsteps} steps with hold {hold} need {max(nsteps + hold - 1, 0) // hold} rows (>= 1); {name}: {rows}")
        return hold, nsteps

    def _samples(self, nsteps, traj_every, rows=18, lanes=None):
        """The buffer of a rollout's samples, one after every traj_every-th step: [nsteps // traj_every, rows, lanes] (lanes: B), or
        None without traj_every, which must divide nsteps."""
        if not traj_every:
            return None
        k = int(traj_every)
        if k < 1 or nsteps % k:
            raise ValueError(f"nsteps ({nsteps}) must be a multiple of traj_every ({traj_every})")
        return torch.empty((nsteps // k, rows, self.B if lanes is None else lanes), dtype=torch.float64, device=self.device)

    # x.values / u.values as [B,18] / [B,4] views of the resident state
    @property
    def x_values(self):
        return self._x.t()

    @property
    def u_values(self):
        return self._u.t()

    def set_state(self, x):
        self._x.copy_(self._soa(x, 18))

    def set_input(self, u):
        self._u.copy_(self._soa(u, 4))

    # ------------------------------------------------------------------ env.py:132-150
    def reset(self):
        self._x.copy_(self._x_init)
        self._u.copy_(self._u_init)
        self.status.zero_()
        return self.get_obs(self._x, self._u)

    def get_obs(self, x=None, u=None):
        """Observed states x[_obs_x_idx] (parameters.py:134,160) -> [B,10]."""
        x = self._x if x is None else x
        return x[P.obs_x_idx].t()

    def _get_obs_na(self, x9, u=None):
        return x9

    def debug_table_lookup(self, tid, alpha, beta=None, el=None):
        """One of the reference's 43 table functions (C/hifi_F16_AeroData.c:109-1861) evaluated by the device lookup code
        at the given points (degrees).  Test entry.  Returns (values, status bits)."""
        a = np.ascontiguousarray(alpha, dtype=np.float64)
        b = np.zeros_like(a) if beta is None else np.ascontiguousarray(beta, dtype=np.float64)
        e = np.zeros_like(a) if el is None else np.ascontiguousarray(el, dtype=np.float64)
        out, st = np.zeros_like(a), np.zeros(a.shape, dtype=np.int32)
        hp = lambda v: ctypes.c_void_p(v.ctypes.data)
        self._check(self.lib.f16_debug_table_lookup(self.ctx.handle, int(tid), hp(a), hp(b), hp(e), a.size, hp(out), hp(st)))
        return out, st

    # ------------------------------------------------------------------ env.py:65-103
    def _calc_xdot(self, x=None, u=None, wind=None, gust=None):
        """xdot [B,18] for states x [B,18] and inputs u [B,4] (defaults: resident x.values/u.values).
        wind ([3] or [B,3]: velocity of the air mass over the ground, north / east / down, ft/s) and gust ([3] or [B,3]: gust velocity
        in body axes, ft/s) evaluate the derivative in moving air (f16_xdot_wind_batch); without them the call is what it always was."""
        xs = self._x if x is None else self._soa(x, 18)
        us = self._u if u is None else self._soa(u, 4)
        out = torch.empty_like(xs)
        st = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        if wind is not None or gust is not None:
            ws, gs = (None if v is None else self._soa(v, 3) for v in (wind, gust))
            self._check(self.lib.f16_xdot_wind_batch(self.ctx.handle, _vp(xs), _vp(us), _vp(ws), _vp(gs), _vp(out), _vp(st), self.B, self.B,
                                                     self.xcg, self.fi_flag, self.flags, self._stream))
            self.last_status = st
            return out.t()
        self._check(self.lib.f16_xdot_batch(self.ctx.handle, _vp(xs), _vp(us), _vp(out), _vp(st), self.B, self.B,
                                            self.xcg, self.fi_flag, self.flags, self._stream))
        self.last_status = st
        return out.t()

    def nlplant(self, xu):
        """C/nlplant.c:23 for B aircraft: xu [B,>=17] -> xdot [B,18] (12..17 = nx,ny,nz,mach,qbar,ps)."""
        xs = self._soa(torch.as_tensor(np.asarray(xu, dtype=np.float64))[:, :18] if not isinstance(xu, torch.Tensor) else xu[:, :18])
        out = torch.empty((18, self.B), dtype=torch.float64, device=self.device)
        st = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._check(self.lib.f16_nlplant_batch(self.ctx.handle, _vp(xs), _vp(out), _vp(st), self.B, self.B, self.xcg,
                                               self.fi_flag, self.flags, self._stream))
        self.last_status = st
        return out.t()

    # ------------------------------------------------------------------ env.py:105-130
    def step(self, action=None, auto_reset=False):
        """One explicit-Euler step of every aircraft (env.py:126).  Returns (obs [B,10], reward, done, info) like
        the reference; where the reference exit()s on an envelope violation (env.py:121-124) the aircraft is frozen
        and `done[b]` is set (status bit F16_ST_ENVELOPE).
        auto_reset (vectorised-env convention): aircraft that are done are put back on their initial
        condition (env.py:132-135 `reset` for those aircraft only) after the step; the returned observation is the
        post-reset one and `info["terminal_observation"]` holds the last pre-reset observation of every aircraft."""
        self.rollout(1, action)
        done = (self.status & _lib.F16_ST["ENVELOPE"]) != 0
        reward = torch.ones(self.B, dtype=torch.float64, device=self.device)
        info = {"fidelity": "high" if self.fi_flag == 1 else "low", "status": self.status.clone() if auto_reset else self.status}
        if auto_reset:
            info["terminal_observation"] = self.get_obs().clone()
            self._x[:, done] = self._x_init[:, done]
            self.status[done] = 0
        return self.get_obs(), reward, done, info

    def rollout(self, nsteps, action=None, traj_every=None, method="euler"):
        """nsteps Euler steps in ONE launch with the state held in registers (the reference's
        `for ...: self.step(u)` loops, test_env.py:456-462).  traj_every=k stores the state after every k-th
        step and returns it as [nsteps//k, 18, B] (state-major).
        method="rk4": classical fourth-order Runge-Kutta steps of self.dt instead (C-ABI f16_rollout_rk, the action held over the
        four stages of a step) -- for a step coarser than the reference's 1 ms, where Euler is no longer accurate."""
        return self._rollout_call(self._u if action is None else self._soa(action, 4), nsteps, traj_every, method=_lib.integrator(method))

    def _air(self, wind, gusts, gust_every, nsteps):
        """The `wind=` / `gusts=` / `gust_every=` keywords of the rollouts -> None for still air, else (lib.Wind, the tensors it points
        at, the GustModel or None).  wind: [3] or [B, 3], ft/s north / east / down.  gusts: a [Sg, B, 3] array of body-axis gust
        velocities, step t reading row t // gust_every (default 1; Sg >= ceil(nsteps / gust_every)), or a wind.GustModel for
        generation inside the kernel.  ValueError for anything else: argument checks, no GPU call."""
        from .wind import GustModel
        if wind is None and gusts is None:
            if gust_every is not None:
                raise ValueError("gust_every goes with a gusts array")
            return None
        air, keep, model = _lib.Wind(), [], None
        if wind is not None:
            keep.append(self._soa(wind, 3))
            air.wind_ned = keep[-1].data_ptr()
        if isinstance(gusts, GustModel):
            if gust_every is not None:
                raise ValueError("a GustModel carries its own row period (every=); gust_every goes with a gusts array")
            model = gusts
            keep += list(model.device_state(self.B, self.dt, self.device))
            air.ga, air.gb, air.gstate = (t.data_ptr() for t in keep[-3:])
            air.gust_hold, air.seed, air.row0 = model.every, model.seed, model.row
        elif gusts is not None:
            g = gusts if isinstance(gusts, torch.Tensor) else torch.as_tensor(np.asarray(gusts, dtype=np.float64))
            k = 1 if gust_every is None else int(gust_every)
            if g.dim() != 3 or tuple(g.shape[1:]) != (self.B, 3):
                raise ValueError(f"gusts must be [Sg, {self.B}, 3] or a wind.GustModel, not {tuple(g.shape)}")
            if k < 1 or (int(nsteps) + k - 1) // k > g.shape[0]:
                raise ValueError(f"{nsteps} steps with gust_every {k} (>= 1) need {(max(int(nsteps), 0) + max(k, 1) - 1) // max(k, 1)} gust rows; gusts: {g.shape[0]}")
            keep.append(g.to(device=self.device, dtype=torch.float64).permute(0, 2, 1).contiguous())
            air.gust_seq, air.gust_hold = keep[-1].data_ptr(), k
        return air, keep, model

    def _ensemble_buffers(self, group, samples):
        """The `ensemble=` keyword -> (lib.Ens, the tensors it points at, the Ensemble the call fills): group = aircraft per group (a
        multiple of 64; True: the whole batch as one group), `samples` samples.  The result tensors are [S, 18, G] on the device, as
        the library writes them, seen as [S, G, 18]."""
        from .ensemble import Ensemble, group_size
        group = group_size(group, self.B)
        G = (self.B + group - 1) // group
        work = torch.empty(max(int(self.lib.f16_ens_work_doubles(self.B, samples)), 1), dtype=torch.float64, device=self.device)
        count = torch.zeros((samples, G), dtype=torch.int32, device=self.device)
        mean, m2, mn, mx = (torch.zeros((samples, 18, G), dtype=torch.float64, device=self.device) for _ in range(4))
        e = _lib.Ens()
        e.work, e.group, e.ldg, e.count = work.data_ptr(), group, G, count.data_ptr()
        e.mean, e.m2, e.min, e.max = (t.data_ptr() for t in (mean, m2, mn, mx))
        return e, (work, count, mean, m2, mn, mx), Ensemble(count, *(t.permute(0, 2, 1) for t in (mean, m2, mn, mx)), group=group)

    def _rollout_call(self, u, nsteps, traj_every, hold=None, K=None, dem=None, method=_lib.F16_INT_EULER, air=None, ensemble=None,
                      keep_traj=False, observer=None):
        """rollout, rollout_schedule and the nonlinear rollout_LQR behind their argument checks: the sample buffers and the ONE call
        into the library.  u [4,B], or with hold (steps per row) the schedule u_seq [S,4,B]; K [27,B] with dem [3,B]: the LQR law
        around the offset u, dem with hold the schedule dem_seq [S,3,B] -- its last action lands in u.values.  method F16_INT_RK4:
        the _rk entry points, which are scheduled ones -- a constant input is one row held for every step.  air (_air): the _wind
        entry points.  ensemble (aircraft per group, or True): the _wind_ens ones, which return the statistics of the samples (an
        ensemble.Ensemble; with keep_traj the samples too; no air = zero air).  observer = (observer.Observer, meas_seed,
        return_estimate) with K: the _lqg_wind ones, the samples of the estimate [S, 9, B] appended when asked for.  The values are
        gathered once under the header's parameter names and passed in its order (cabi.functions())."""
        if ensemble is None and keep_traj:
            raise ValueError("keep_traj goes with ensemble=")
        obs, meas_seed, want_estimate = observer or (None, 0, False)
        if obs is not None and not 0 <= int(meas_seed) < 2 ** 64:
            raise ValueError("meas_seed must fit 64 bits")
        nsteps = int(nsteps)
        name = "f16_rollout" if K is None else "f16_rollout_lqr"
        if obs is not None:
            name = "f16_rollout_lqg_wind" + ("_ens" if ensemble is not None else "")
        elif ensemble is not None or air is not None:
            name += "_wind_ens" if ensemble is not None else "_wind"
        elif method != _lib.F16_INT_EULER or hold is not None:
            name += "_rk" if method != _lib.F16_INT_EULER else "_sched"
        scheduled = name not in ("f16_rollout", "f16_rollout_lqr")
        every = traj_every if ensemble is None else int(traj_every or 1)      # the sample period of the ensemble: every step by default
        if ensemble is not None and (every < 1 or nsteps % every):
            raise ValueError(f"nsteps ({nsteps}) must be a multiple of traj_every ({traj_every}), the sample period of the ensemble")
        traj = self._samples(nsteps, every) if ensemble is None or keep_traj else None
        est = self._samples(nsteps, every or 1, rows=9) if want_estimate else None
        v = dict(ctx=self.ctx.handle, x=_vp(self._x), traj=_vp(traj), status=_vp(self.status), B=self.B, ld=self.B, nsteps=nsteps,
                 traj_every=int(every or 1), dt=self.dt, xcg=self.xcg, fi_flag=self.fi_flag, flags=self.flags, stream=self._stream)
        if K is None:
            v["u_seq" if scheduled else "u"] = _vp(u)
        else:
            v.update(u0=_vp(u), K=_vp(K), u_out=_vp(self._u))
            v["dem_seq" if scheduled else "dem"] = _vp(dem)
        if scheduled:      # a constant input is one row held for every step
            v["hold"] = max(nsteps, 1) if hold is None else hold
        if scheduled and not name.endswith("_sched"):
            v["method"] = int(method)
        if "_wind" in name:
            v["h_wind"] = None if air is None else ctypes.byref(air[0])
        if obs is not None:
            models, xhat = obs.flight(self)
            v.update(obs=_vp(models), mgroup=obs.group, sensed=obs.sensed, h_sigma=obs.h_sigma, meas_seed=int(meas_seed), mrow0=obs.row,
                     xhat=_vp(xhat), xhat_traj=_vp(est))
        if ensemble is not None:
            e, keep, result = self._ensemble_buffers(ensemble, nsteps // every)
            v["h_ens"] = ctypes.byref(e)
        params = [p for _, p in _cabi.functions()[name][1]]
        if set(params) != set(v):
            raise TypeError(f"{name}: no value for {sorted(set(params) - set(v))}, no parameter for {sorted(set(v) - set(params))}")
        self._check(getattr(self.lib, name)(*(v[p] for p in params)))
        if ensemble is not None:
            result._keep = keep      # (the workspace lives as long as the result: the launches may still be running)
        if obs is not None:
            obs.advance(nsteps)
        if air is not None and air[2] is not None:
            air[2].advance(nsteps)
        out = (traj,) if ensemble is None else ((traj, result) if keep_traj else (result,))
        out = out + (est,) if want_estimate else out
        return out[0] if len(out) == 1 else out

    def rollout_schedule(self, actions, hold=1, nsteps=None, traj_every=None, method="euler", wind=None, gusts=None, gust_every=None,
                         ensemble=None, keep_traj=False):
        """The reference's call pattern `u.values = action; step(u.values)` with an action that changes during the run
        (env.py:105-130; the doublets of Nguyen_m/runF16Sim.m) in ONE launch (C-ABI f16_rollout_sched): step t takes
        actions[t // hold], a zero-order hold.  actions: [S, B, 4] (numpy or torch), or a state-major [S, 4, B] fp64 tensor
        already on the device, which is taken as it is, without a copy (for B == 4 a 3-D device tensor is read as [S, B, 4];
        pass a host array or a non-contiguous view to say otherwise).  nsteps defaults to S * hold and needs
        S >= ceil(nsteps / hold) rows.  Returns what `rollout` returns; u.values ends up holding the last row used, as the
        reference's caller leaves it.  method="rk4": Runge-Kutta steps, each row held over the stages of its steps (f16_rollout_rk).
        wind= / gusts= / gust_every= (see _air): the same rollout in steady wind and gusts (f16_rollout_wind), both methods.
        ensemble=group (a multiple of 64, or True for the whole batch as one group): instead of the samples, their statistics over the
        aircraft of each group -- count, mean, M2, min, max per sample and state, formed inside the launch (f16_rollout_wind_ens;
        ensemble.py).  traj_every is then the sample period (default: every step); returns an ensemble.Ensemble, or (traj, Ensemble)
        with keep_traj=True.  Without wind= / gusts= the flight is in zero air through the wind kernels."""
        method = _lib.integrator(method)
        t = actions if isinstance(actions, torch.Tensor) else torch.as_tensor(np.asarray(actions, dtype=np.float64))
        if t.dim() != 3:
            raise ValueError(f"actions must be [S, B, 4] or a state-major [S, 4, B] device tensor, not {tuple(t.shape)}")
        if tuple(t.shape[1:]) == (self.B, 4):
            seq = t.to(device=self.device, dtype=torch.float64).permute(0, 2, 1).contiguous()
        elif tuple(t.shape[1:]) == (4, self.B) and t.device == self.device and t.dtype == torch.float64 and t.is_contiguous():
            seq = t
        else:
            raise ValueError(f"actions must be [S, {self.B}, 4] or a contiguous fp64 [S, 4, {self.B}] tensor on {self.device}, "
                             f"not {tuple(t.shape)} ({t.dtype}, {t.device})")
        hold, nsteps = self._schedule_steps(hold, nsteps, seq.shape[0], "actions")
        traj = self._rollout_call(seq, nsteps, traj_every, hold=hold, method=method, air=self._air(wind, gusts, gust_every, nsteps),
                                  ensemble=ensemble, keep_traj=keep_traj)
        self._u.copy_(seq[(nsteps - 1) // hold])
        return traj

    # ------------------------------------------------------------------ scored rollouts of sampled schedules (MPPI)
    def _sample_lanes(self, actions, width=4, name="actions"):
        """[S, K, B, width] (numpy or torch, host or device) -> contiguous state-major [S, width, K * B] fp64 on the device (lane
        k * B + a = sample k of aircraft a), and K."""
        t = actions if isinstance(actions, torch.Tensor) else torch.as_tensor(np.asarray(actions, dtype=np.float64))
        if t.dim() != 4 or t.shape[2] != self.B or t.shape[3] != width or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{name} must be [S, K, {self.B}, {width}] with S, K >= 1, not {tuple(t.shape)}")
        S, K = t.shape[0], t.shape[1]
        return t.to(device=self.device, dtype=torch.float64).permute(0, 3, 1, 2).reshape(S, width, K * self.B).contiguous(), K

    def _score(self, seq, K, hold, nsteps, x_ref, u_ref, w, traj_every, want_final, method=_lib.F16_INT_EULER):
        """f16_rollout_cost on seq [S, 4, K * B] from the resident state -> cost [K * B], status [K * B], x_end [18, K * B] or None,
        traj [n, 18, K * B] or None.  x_ref [9, B], u_ref [3, B] or None (state-major, contiguous).  method F16_INT_RK4:
        f16_rollout_cost_rk."""
        lanes = K * self.B
        hold, nsteps = self._schedule_steps(hold, nsteps, seq.shape[0], "actions")
        traj = self._samples(nsteps, traj_every, lanes=lanes)
        cost = torch.empty(lanes, dtype=torch.float64, device=self.device)
        st = torch.empty(lanes, dtype=torch.int32, device=self.device)
        x_end = torch.empty((18, lanes), dtype=torch.float64, device=self.device) if want_final else None
        call, rule = (self.lib.f16_rollout_cost, ()) if method == _lib.F16_INT_EULER else (self.lib.f16_rollout_cost_rk, (int(method),))
        self._check(call(self.ctx.handle, _vp(self._x), self.B, self.B, _vp(seq), _vp(x_ref), _vp(u_ref),
                         ctypes.byref(w), _vp(cost), _vp(x_end), _vp(traj), _vp(st), lanes, lanes, nsteps, hold,
                         int(traj_every or 1), self.dt, self.xcg, self.fi_flag, *rule, self.flags, self._stream))
        return cost, st, x_end, traj

    def _blend(self, cost, seq, K, lam):
        """f16_mppi_blend: cost [K * B], seq [S, 4, K * B] -> blended [S, 4, B], normalised weights [K * B], stats [2, B]"""
        lam = float(lam)
        if not (lam > 0.0 and np.isfinite(lam)):
            raise ValueError(f"lam must be finite and > 0 (got {lam})")
        S, lanes = seq.shape[0], K * self.B
        out = torch.empty((S, 4, self.B), dtype=torch.float64, device=self.device)
        wts = torch.empty(lanes, dtype=torch.float64, device=self.device)
        stats = torch.empty((2, self.B), dtype=torch.float64, device=self.device)
        self._check(self.lib.f16_mppi_blend(self.ctx.handle, _vp(cost), _vp(seq), lam, _vp(out), _vp(wts), _vp(stats), lanes, lanes,
                                            self.B, self.B, S, self._stream))
        return out, wts, stats

    def score_schedules(self, actions, hold=1, nsteps=None, x_ref=None, u_ref=None, q=None, qf=None, r=None, penalty=0.0,
                        traj_every=None, return_final=False, method="euler"):
        """K sampled command schedules per aircraft through the nonlinear plant, each scored, in ONE launch (C-ABI
        f16_rollout_cost): actions [S, K, B, 4] (numpy or torch, host or device), step t of sample k takes actions[t // hold, k] as
        rollout_schedule does; every sample starts from the current x.values.  The cost of a sample is
            sum over the steps taken of [ r . (u[1:4] - u_ref)^2 + q . (x9 - x_ref)^2 ] + penalty * (steps not taken: the sample
            left the envelope of env.py:117-124 and is frozen) + qf . (x9_end - x_ref)^2
        with x9 the MPC states (parameters.py:135) after each step.  x_ref [B, 9] or [9] defaults to the current x9, u_ref [B, 3] or
        [3] to 0, q = qf = ones(9), r = ones(3): the diagonals of the reference's Q = Cd'Cd and R = I3 (env.py:385-399).  nsteps
        defaults to S * hold.  Returns cost [K, B]; with return_final also the final states [18, K, B]; with traj_every = k also the
        samples [nsteps // k, 18, K, B] -- (cost, final), (cost, traj) or (cost, final, traj).  x.values, u.values and status are
        not touched; the status words of the samples [K, B] (an output: every sample starts from 0) are kept in
        `last_score_status`.  method="rk4": the samples are integrated with Runge-Kutta steps of self.dt (f16_rollout_cost_rk); the
        cost formula is the same, on the states after each whole step."""
        method = _lib.integrator(method)
        seq, K = self._sample_lanes(actions)
        xr = self._x[P.mpc_x_idx].contiguous() if x_ref is None else self._soa(x_ref, 9)
        ur = None if u_ref is None else self._soa(u_ref, 3)
        w = _lib.make_cost_weights(q, qf, r, penalty)
        cost, st, x_end, traj = self._score(seq, K, hold, nsteps, xr, ur, w, traj_every, return_final, method)
        self.last_score_status = st.view(K, self.B)
        out = (cost.view(K, self.B),)
        if return_final:
            out += (x_end.view(18, K, self.B),)
        if traj_every:
            out += (traj.view(-1, 18, K, self.B),)
        return out[0] if len(out) == 1 else out

    def blend_schedules(self, cost, actions, lam, return_info=False):
        """The softmin blend of an MPPI step (C-ABI f16_mppi_blend; the rule is stated by mppi.blend_reference): cost [K, B],
        actions [S, K, B, 4] -> [S, B, 4] = sum_k w_k actions[:, k] / sum_k w_k with w_k = exp(-(cost_k - min cost) / lam) over the
        samples of finite cost (an aircraft without one gets sample 0).  return_info: also dict(weights [K, B] normalised,
        min_cost [B], ess [B] the effective sample size (sum w)^2 / sum w^2)."""
        seq, K = self._sample_lanes(actions)
        c = cost if isinstance(cost, torch.Tensor) else torch.as_tensor(np.asarray(cost, dtype=np.float64))
        if tuple(c.shape) != (K, self.B):
            raise ValueError(f"cost must be [{K}, {self.B}] for these actions, not {tuple(c.shape)}")
        c = c.to(device=self.device, dtype=torch.float64).contiguous().view(-1)
        out, wts, stats = self._blend(c, seq, K, lam)
        u = out.permute(0, 2, 1)
        return (u, dict(weights=wts.view(K, self.B), min_cost=stats[0], ess=stats[1])) if return_info else u

    def calc_MPPI_action(self, p_dem, q_dem, r_dem, nominal, noise, hold=1, lam=1.0, method="euler", **weights):
        """One step of sampling-based nonlinear MPC (MPPI, model-predictive path integral control) on the plant itself -- for the
        states from which the linear MPC's QP has no feasible point: K command sequences per aircraft, nominal
        [S, B, 4] plus noise [S, K, B, 3] on the three surface commands (the caller's, e.g. sigma * torch.randn(..., generator=g)),
        clipped to the command limits (parameters.py:125-126; the thrust command is the nominal one), are rolled out for S * hold
        steps, scored against x_ref = the current x9 with x_ref[4:7] = (p, q, r)_dem (the convention of _calc_LQR_action,
        env.py:365-367) and blended by softmin weights of temperature lam: one score_schedules plus one blend_schedules.  weights:
        q, qf, r, penalty, u_ref as score_schedules takes them.  Returns (the blended schedule [S, B, 4], dict(cost [K, B],
        min_cost [B], ess [B], status [K, B])); nothing resident is touched.  method="rk4": the samples are scored with
        Runge-Kutta steps (score_schedules' keyword)."""
        method = _lib.integrator(method)
        nom = nominal if isinstance(nominal, torch.Tensor) else torch.as_tensor(np.asarray(nominal, dtype=np.float64))
        eps = noise if isinstance(noise, torch.Tensor) else torch.as_tensor(np.asarray(noise, dtype=np.float64))
        if nom.dim() != 3 or tuple(nom.shape[1:]) != (self.B, 4):
            raise ValueError(f"nominal must be [S, {self.B}, 4], not {tuple(nom.shape)}")
        if eps.dim() != 4 or eps.shape[0] != nom.shape[0] or eps.shape[2] != self.B or eps.shape[3] != 3 or eps.shape[1] < 1:
            raise ValueError(f"noise must be [{nom.shape[0]}, K, {self.B}, 3], not {tuple(eps.shape)}")
        if not (float(lam) > 0.0 and np.isfinite(float(lam))):
            raise ValueError(f"lam must be finite and > 0 (got {lam})")
        extra = set(weights) - {"q", "qf", "r", "penalty", "u_ref"}
        if extra:
            raise TypeError(f"unknown weights {sorted(extra)}")
        nom = nom.to(device=self.device, dtype=torch.float64)
        eps = eps.to(device=self.device, dtype=torch.float64)
        K = eps.shape[1]
        lo = torch.as_tensor(P.u_lb[1:], dtype=torch.float64, device=self.device)
        hi = torch.as_tensor(P.u_ub[1:], dtype=torch.float64, device=self.device)
        samples = nom.unsqueeze(1).repeat(1, K, 1, 1)
        samples[..., 1:] = torch.minimum(torch.maximum(samples[..., 1:] + eps, lo), hi)
        seq, _ = self._sample_lanes(samples)
        xr = self._x[P.mpc_x_idx].clone()
        xr[4:7] = self._demands(p_dem, q_dem, r_dem)
        ur = None if weights.get("u_ref") is None else self._soa(weights["u_ref"], 3)
        w = _lib.make_cost_weights(weights.get("q"), weights.get("qf"), weights.get("r"), weights.get("penalty", 0.0))
        cost, st, _, _ = self._score(seq, K, hold, None, xr, ur, w, None, False, method)
        out, _, stats = self._blend(cost, seq, K, lam)
        return out.permute(0, 2, 1), dict(cost=cost.view(K, self.B), min_cost=stats[0], ess=stats[1], status=st.view(K, self.B))

    @staticmethod
    def _sigma3(sigma):
        """sigma, a scalar or the three surface deviations, as three host doubles (ctypes array)"""
        s = np.asarray(sigma, dtype=np.float64)
        if s.ndim > 1 or (s.ndim == 1 and s.shape[0] != 3):
            raise ValueError(f"sigma is a scalar or the three surface deviations, not {tuple(s.shape)}")
        return (ctypes.c_double * 3)(*np.broadcast_to(s, (3,)))

    def _sample(self, nom, sg, K, seed, period):
        """f16_mppi_sample: the nominal schedule nom [S, 4, B] (state-major, contiguous) -> the sample set [S, 4, K * B] of `period`"""
        S, lanes = nom.shape[0], K * self.B
        seq = torch.empty((S, 4, lanes), dtype=torch.float64, device=self.device)
        self._check(self.lib.f16_mppi_sample(self.ctx.handle, _vp(nom), sg, int(seed), int(period), _vp(seq), lanes, lanes, self.B, self.B,
                                             S, self._stream))
        return seq

    def sample_schedules(self, nominal, sigma, samples, seed, period):
        """The sample set of one MPPI period by the library's own counter-based sampler (C-ABI f16_mppi_sample; the rule -- Philox4x32-10
        with counter (period, row, sample, aircraft) and key `seed`, Box-Muller, clipping to the command limits -- is stated in
        include/f16_hip.h and restated by mppi.sample_reference): nominal [S, B, 4], sigma a scalar or the three surface deviations
        -> [S, K, B, 4] on the device.  The thrust command is the nominal one."""
        nom = nominal if isinstance(nominal, torch.Tensor) else torch.as_tensor(np.asarray(nominal, dtype=np.float64))
        if nom.dim() != 3 or tuple(nom.shape[1:]) != (self.B, 4) or nom.shape[0] < 1 or int(samples) < 1:
            raise ValueError(f"nominal must be [S, {self.B}, 4] with S >= 1 and samples >= 1, not {tuple(nom.shape)}")
        nom = nom.to(device=self.device, dtype=torch.float64).permute(0, 2, 1).contiguous()
        seq = self._sample(nom, self._sigma3(sigma), int(samples), seed, period)
        return seq.view(nom.shape[0], 4, int(samples), self.B).permute(0, 2, 3, 1)

    def _rollout_MPPI_counter(self, periods, dem, horizon, hold, K, sigma, lam, seed, period0, traj_every, method, fused, weights):
        """rollout_MPPI with sampler="counter": the host loop over the C-ABI entries f16_mppi_sample -> f16_rollout_cost(_rk) ->
        f16_mppi_blend -> f16_rollout(_rk), or (fused) the ONE call f16_rollout_mppi that equals it."""
        extra = set(weights) - {"q", "qf", "r", "penalty", "u_ref"}
        if extra:
            raise TypeError(f"unknown weights {sorted(extra)}")
        sg = self._sigma3(sigma)
        ur = None if weights.get("u_ref") is None else self._soa(weights["u_ref"], 3)
        w = _lib.make_cost_weights(weights.get("q"), weights.get("qf"), weights.get("r"), weights.get("penalty", 0.0))
        nom = self._u.unsqueeze(0).repeat(horizon, 1, 1)                       # [S, 4, B]
        if fused:
            lanes = K * self.B
            seq = torch.empty((horizon, 4, lanes), dtype=torch.float64, device=self.device)
            cost = torch.empty(lanes, dtype=torch.float64, device=self.device)
            stats = torch.empty((periods, 2, self.B), dtype=torch.float64, device=self.device)
            traj = self._samples(periods * hold, traj_every)
            self._check(self.lib.f16_rollout_mppi(self.ctx.handle, _vp(self._x), _vp(self._u), _vp(nom), _vp(dem), _vp(ur), ctypes.byref(w), sg,
                                                  float(lam), int(seed), int(period0), _vp(seq), _vp(cost), _vp(stats), _vp(traj),
                                                  _vp(self.status), self.B, self.B, K, lanes, periods, horizon, hold, int(traj_every or 1),
                                                  self.dt, self.xcg, self.fi_flag, int(method), self.flags, self._stream))
            mins, ess = stats[:, 0], stats[:, 1]
        else:
            name = {v: k for k, v in _lib.INTEGRATORS.items()}[method]
            trajs, mins, ess = [], [], []
            for p in range(periods):
                seq = self._sample(nom, sg, K, seed, int(period0) + p)
                xr = self._x[P.mpc_x_idx].clone()
                xr[4:7] = dem
                cost, _, _, _ = self._score(seq, K, hold, None, xr, ur, w, None, False, method)
                out, _, st = self._blend(cost, seq, K, lam)
                self._u.copy_(out[0])
                trajs.append(self.rollout(hold, traj_every=traj_every, method=name))
                nom = torch.cat((out[1:], out[-1:]), 0)
                mins.append(st[0])
                ess.append(st[1])
            traj = torch.cat(trajs, 0) if traj_every else None
            mins, ess = torch.stack(mins), torch.stack(ess)
        self.last_mppi = dict(nominal=nom.permute(0, 2, 1), cost=cost.view(K, self.B),
                              samples=seq.view(horizon, 4, K, self.B).permute(0, 2, 3, 1))
        return traj, dict(min_cost=mins, ess=ess)

    def rollout_MPPI(self, nsteps, p_dem, q_dem, r_dem, horizon, hold, samples, sigma, lam, seed=0, traj_every=None,
                     return_info=False, method="euler", sampler="torch", fused=False, period0=0, **weights):
        """The closed MPPI loop.  Per control period of `hold` plant steps:
        noise = sigma * randn([horizon, samples, B, 3]) from a device torch.Generator seeded once with `seed`; calc_MPPI_action on
        the nominal schedule [horizon, B, 4] (at first the current u.values in every row); u.values = row 0 of the blend and
        `rollout(hold)`; the nominal becomes the blend shifted one row, its last row repeated.  nsteps must be a multiple of hold,
        hold of traj_every.  sigma: a scalar or the three surface deviations (deg).  x.values, u.values and status advance as under
        `rollout`.  Returns the samples [nsteps // traj_every, 18, B] (None without traj_every); with return_info also
        dict(min_cost [periods, B], ess [periods, B]).  method="rk4": Runge-Kutta steps both in the scoring and in the plant advance.
        sampler="torch" (the default) is that host loop.  sampler="counter" draws the noise with the library's own counter-based
        sampler instead (sample_schedules: period p of the call uses the counter word period0 + p), as a host loop over the C-ABI
        entries; with fused=True (sampler="counter", samples <= 256) the whole loop is ONE launch, f16_rollout_mppi, which equals
        that host loop bit for bit under F16_FLAG_ONE_LANE.  Both counter forms leave `last_mppi` = dict(nominal [S, B, 4] the
        shifted schedule, cost [K, B] and samples [S, K, B, 4] of the last period)."""
        method_id = _lib.integrator(method)
        if sampler not in ("torch", "counter"):
            raise ValueError(f'sampler must be "torch" or "counter", not {sampler!r}')
        if fused and (sampler != "counter" or int(samples) > 256):
            raise ValueError('fused=True needs sampler="counter" and samples <= 256 (one workgroup holds an aircraft\'s samples)')
        nsteps, horizon, hold, samples = int(nsteps), int(horizon), int(hold), int(samples)
        if hold < 1 or horizon < 1 or samples < 1:
            raise ValueError("horizon, hold and samples must be >= 1")
        if nsteps < 1 or nsteps % hold:
            raise ValueError(f"nsteps ({nsteps}) must be a positive multiple of hold ({hold})")
        if traj_every and hold % int(traj_every):
            raise ValueError(f"hold ({hold}) must be a multiple of traj_every ({traj_every})")
        if not (float(lam) > 0.0 and np.isfinite(float(lam))):
            raise ValueError(f"lam must be finite and > 0 (got {lam})")
        sig = torch.as_tensor(sigma, dtype=torch.float64, device=self.device)
        if sig.dim() > 1 or (sig.dim() == 1 and sig.shape[0] != 3):
            raise ValueError(f"sigma is a scalar or the three surface deviations, not {tuple(sig.shape)}")
        if sampler == "counter":
            traj, info = self._rollout_MPPI_counter(nsteps // hold, self._demands(p_dem, q_dem, r_dem), horizon, hold, samples, sigma, lam,
                                                    seed, period0, traj_every, method_id, fused, weights)
            return (traj, info) if return_info else traj
        g = torch.Generator(device=self.device)
        g.manual_seed(int(seed))
        nominal = self._u.t().unsqueeze(0).repeat(horizon, 1, 1)
        trajs, mins, ess = [], [], []
        for _ in range(nsteps // hold):
            noise = sig * torch.randn((horizon, samples, self.B, 3), generator=g, device=self.device, dtype=torch.float64)
            u, info = self.calc_MPPI_action(p_dem, q_dem, r_dem, nominal, noise, hold=hold, lam=lam, method=method, **weights)
            self.set_input(u[0])
            trajs.append(self.rollout(hold, traj_every=traj_every, method=method))
            nominal = torch.cat((u[1:], u[-1:]), 0)
            mins.append(info["min_cost"])
            ess.append(info["ess"])
        traj = torch.cat(trajs, 0) if traj_every else None
        return (traj, dict(min_cost=torch.stack(mins), ess=torch.stack(ess))) if return_info else traj

    # ------------------------------------------------------------------ env.py:152-193
    def _get_mpc_x(self):
        return self._x[P.mpc_x_idx].t()

    def _get_mpc_u(self):
        return self._u[P.mpc_u_idx].t()

    def _get_mpc_act_states(self):
        return self._x[P.mpc_u_states_idx].t()

    def _calc_xdot_na(self, x9, u3):
        """x9 [B,9] MPC states, u3 [B,3] actuator positions -> xdot9 [B,9] (other states from x.values)."""
        x9s, u3s = self._soa(x9, 9), self._soa(u3, 3)
        out = torch.empty_like(x9s)
        st = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._check(self.lib.f16_xdot_na_batch(self.ctx.handle, _vp(self._x), _vp(x9s), _vp(u3s), _vp(out), _vp(st),
                                               self.B, self.B, self.xcg, self.fi_flag, self.flags, self._stream))
        self.last_status = st
        return out.t()

    # ------------------------------------------------------------------ env.py:294-358
    def linearise(self, x=None, u=None, _calc_xdot=None, get_obs=None, eps=1e-5):
        """env.py:294 `linearise(self, x, u, _calc_xdot=None, get_obs=None)`: forward-difference linearisation (eps 1e-5,
        env.py:319) of every aircraft at its own point, with the reference's dispatch on the model function:
          * default / `self._calc_xdot` + `self.get_obs`: the 18-state model, x [B,18], u [B,4]
            -> A [B,18,18], B [B,18,4], C [B,10,18], D [B,10,4]                                        (env.py:45)
          * `self._calc_xdot_na` + `self._get_obs_na`: the reduced model, x = x9 [B,9] (self._get_mpc_x()), u = u3 [B,3]
            (self._get_mpc_u()); the other states come from x.values as in env.py:172-177
            -> A [B,9,9], B [B,9,3], C [B,9,9], D [B,9,3]                                              (env.py:49)
        x / u default to the resident values.  Only these two models exist on the device; another callable raises."""
        if _calc_xdot is None or _calc_xdot == self._calc_xdot:
            if get_obs is not None and get_obs != self.get_obs:
                raise ValueError("the 18-state model is linearised with get_obs (env.py:312-313)")
            r = self.linearise_full(eps, discretise=False, x=x, u=u)
            return r["Ac"], r["Bc"], r["Cc"], r["Dc"]
        if _calc_xdot != self._calc_xdot_na:
            raise ValueError("linearise knows the reference's two models: _calc_xdot and _calc_xdot_na")
        if get_obs is not None and get_obs != self._get_obs_na:
            raise ValueError("the reduced model is linearised with _get_obs_na (env.py:49)")
        xs, us = self._x, self._u
        if x is not None or u is not None:          # scatter the given x9 / u3 over a copy of the resident state (env.py:172-177)
            xs, us = self._x.clone(), self._u.clone()
            if x is not None:
                xs[P.mpc_x_idx] = self._soa(x, 9)
            if u is not None:
                us[P.mpc_u_idx] = self._soa(u, 3)
        return self._linearise_na(eps, xs, us)

    def _linearise_na(self, eps=1e-5, xs=None, us=None):
        """The reduced (9-state) linearisation at the resident point (or at state-major xs [18,B] / us [4,B])."""
        xs = self._x if xs is None else xs
        us = self._u if us is None else us
        Ac = torch.empty((81, self.B), dtype=torch.float64, device=self.device)
        Bc = torch.empty((27, self.B), dtype=torch.float64, device=self.device)
        Cc = torch.empty((81, self.B), dtype=torch.float64, device=self.device)
        st = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._check(self.lib.f16_linearise_batch(self.ctx.handle, _vp(xs), _vp(us), _vp(Ac), _vp(Bc), _vp(Cc), _vp(st),
                                                 self.B, self.B, eps, self.xcg, self.fi_flag, self.flags, self._stream))
        self.last_status = st
        self._lin = (Ac, Bc, Cc)
        return (Ac.t().reshape(self.B, 9, 9), Bc.t().reshape(self.B, 9, 3), Cc.t().reshape(self.B, 9, 9),
                torch.zeros((self.B, 9, 3), dtype=torch.float64, device=self.device))

    def linearise_full(self, eps=1e-5, discretise=True, x=None, u=None):
        """env.py:45-46: 18-state linearisation (default _calc_xdot/get_obs) at every aircraft's own (x, u) and its
        zero-order-hold discretisation.  Returns dict(Ac [B,18,18], Bc [B,18,4], Cc [B,10,18], Dc, Ad, Bd)."""
        B = self.B
        xs = self._x if x is None else self._soa(x, 18)
        us = self._u if u is None else self._soa(u, 4)
        Ac = torch.empty((324, B), dtype=torch.float64, device=self.device)
        Bc = torch.empty((72, B), dtype=torch.float64, device=self.device)
        Cc = torch.empty((180, B), dtype=torch.float64, device=self.device)
        st = torch.zeros(B, dtype=torch.int32, device=self.device)
        self._check(self.lib.f16_linearise_full_batch(self.ctx.handle, _vp(xs), _vp(us), _vp(Ac), _vp(Bc), _vp(Cc),
                                                      _vp(st), B, B, eps, self.xcg, self.fi_flag, self.flags, self._stream))
        self.last_status = st
        out = dict(Ac=Ac.t().reshape(B, 18, 18), Bc=Bc.t().reshape(B, 18, 4), Cc=Cc.t().reshape(B, 10, 18),
                   Dc=torch.zeros((B, 10, 4), dtype=torch.float64, device=self.device))
        if discretise:
            Ad, Bd = torch.empty_like(Ac), torch.empty_like(Bc)
            self._check(self.lib.f16_c2d_full_batch(self.ctx.handle, _vp(Ac), _vp(Bc), _vp(Ad), _vp(Bd), B, B, self.dt,
                                                    self._stream))
            out["Ad"], out["Bd"] = Ad.t().reshape(B, 18, 18), Bd.t().reshape(B, 18, 4)
        return out

    def discretise(self, Ac=None, Bc=None):
        """scipy.signal.cont2discrete(..., dt) zero-order hold (env.py:50,351) per aircraft."""
        if Ac is None:
            Ac, Bc, _ = self._lin
        else:
            Ac = Ac.reshape(self.B, 81).t().contiguous()
            Bc = Bc.reshape(self.B, 27).t().contiguous()
        Ad, Bd = torch.empty_like(Ac), torch.empty_like(Bc)
        self._check(self.lib.f16_c2d_batch(self.ctx.handle, _vp(Ac), _vp(Bc), _vp(Ad), _vp(Bd), self.B, self.B, self.dt,
                                           self._stream))
        return Ad, Bd

    def build_ssr(self, eps=1e-5):
        """env.py:49-60: reduced discrete model per aircraft, frozen until called again."""
        self.release_MPC_plan()                 # a new model invalidates a prepared plan
        self._linearise_na(eps)
        Ad, Bd = self.discretise()
        self.ssr = (Ad, Bd, self._lin[2])
        self._ssr_cont = self._lin[:2]          # the continuous (Ac, Bc) of this point: prepare_MPC(ctrl_every > 1) discretises them again
        return self.ssr

    def _calc_LQR_gain(self, Q=None, R=None):
        """env.py:344-358: linearise -> ZOH -> K = -dlqr(Ad,Bd,Cd'Cd,I).  Returns K [B,3,9].
        Q [9,9] / R [3,3]: the weights utils.py:219 `dlqr(A, B, Q, R)` takes (default: env.py's Q = Cd'Cd, R = I)."""
        Ad, Bd, Cd = self.build_ssr()
        K = torch.empty((27, self.B), dtype=torch.float64, device=self.device)
        st = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        w = _lib.make_weights(Q=Q, R=R)
        self._check(self.lib.f16_lqr_batch_w(self.ctx.handle, _vp(Ad), _vp(Bd), _vp(Cd), ctypes.byref(w) if w else None, _vp(K), None,
                                             _vp(st), self.B, self.B, self._stream))
        self.last_status = st
        return K.t().reshape(self.B, 3, 9)

    def _calc_LQR_action(self, p_dem, q_dem, r_dem, K, x, u0):
        """env.py:360-371: u = -K (x_ref - x) + u0 with x_ref[4:7] = demands.  x [B,9], u0 [B,3]."""
        x = torch.as_tensor(x, device=self.device, dtype=torch.float64)
        u0 = torch.as_tensor(u0, device=self.device, dtype=torch.float64)
        x_ref = x.clone()
        x_ref[:, 4], x_ref[:, 5], x_ref[:, 6] = p_dem, q_dem, r_dem
        return -(K @ (x_ref - x).unsqueeze(-1)).squeeze(-1) + u0

    def _demands(self, p_dem, q_dem=None, r_dem=None):
        """(p, q, r) demands, scalars or [B], as a state-major [3,B] device tensor; a 2-D p_dem is that block already (demands on the
        device: graph capture, the host loops) and is returned as it is."""
        if torch.is_tensor(p_dem) and p_dem.dim() == 2:
            return p_dem
        dem = torch.empty((3, self.B), dtype=torch.float64, device=self.device)
        for k, v in enumerate((p_dem, q_dem, r_dem)):
            if isinstance(v, (int, float)):
                dem[k].fill_(float(v))                # scalar demand: a fill kernel, no host-to-device copy
            else:
                dem[k] = torch.as_tensor(v, dtype=torch.float64, device=self.device)
        return dem

    def _qp_settings(self, overrides=None):
        """The library's default QP settings (OSQP's) with the fields of `overrides` replaced."""
        s = _lib.QPSettings()
        self.lib.f16_qp_default_settings(ctypes.byref(s))
        for k, v in (overrides or {}).items():
            setattr(s, k, v)
        return s

    def _demand_schedule(self, p_dem, q_dem, r_dem):
        """Demands of which at least one is a time history [S] or [S, B] (scalars broadcast) -> state-major [S, 3, B] on the device;
        None when none of them is (scalar / [B] demands: the constant-input path)."""
        vs = [v if isinstance(v, (int, float)) else torch.as_tensor(v, dtype=torch.float64, device=self.device) for v in (p_dem, q_dem, r_dem)]
        # ([B] is a constant demand per aircraft, as it always was; a time history for B aircraft is [S, B])
        hist = [v for v in vs if torch.is_tensor(v) and (v.dim() == 2 or (v.dim() == 1 and v.shape[0] != self.B))]
        if not hist:
            return None
        S = hist[0].shape[0]
        seq = torch.empty((S, 3, self.B), dtype=torch.float64, device=self.device)
        for k, v in enumerate(vs):
            if not torch.is_tensor(v) or v.dim() == 0:
                seq[:, k].fill_(float(v))
            elif v.dim() == 2 or v.shape[0] != self.B:
                if v.shape[0] != S or (v.dim() == 2 and v.shape[1] != self.B):
                    raise ValueError(f"demand histories must agree: [{S}] or [{S}, {self.B}], not {tuple(v.shape)}")
                seq[:, k] = v if v.dim() == 2 else v.unsqueeze(1)
            else:
                seq[:, k] = v.unsqueeze(0)
        return seq

    def _mpc_demand_rows(self, p_dem, q_dem, r_dem, dem_every, nctrl):
        """The demands of a closed MPC loop of nctrl control steps -> (dem_seq [S, 3, B], dem_every) when any of them is a history
        ([S] or [S, B]: _demand_schedule's rule), (None, None) for constant demands -- a 2-D p_dem with q_dem is None and r_dem is None
        is a ready [3, B] block, as it always was.  Control step c reads row c // dem_every (default 1).  Raises ValueError for
        dem_every < 1, dem_every without a history, histories that disagree and too few rows: argument checks, no GPU call."""
        if dem_every is not None and int(dem_every) < 1:
            raise ValueError(f"dem_every must be >= 1 (got {dem_every})")
        ready = torch.is_tensor(p_dem) and p_dem.dim() == 2 and q_dem is None and r_dem is None
        seq = None if ready else self._demand_schedule(p_dem, q_dem, r_dem)
        if seq is None:
            if dem_every is not None:
                raise ValueError("dem_every goes with demand histories ([S] or [S, B]); scalar / [B] demands are constant")
            return None, None
        k = 1 if dem_every is None else int(dem_every)
        need = (max(int(nctrl), 0) + k - 1) // k
        if need < 1 or need > seq.shape[0]:
            raise ValueError(f"{nctrl} control steps with dem_every {k} need {need} demand rows (>= 1), the histories have {seq.shape[0]}")
        return seq.contiguous(), k

    def rollout_LQR(self, nsteps, p_dem, q_dem, r_dem, K=None, u0=None, traj_every=None, linear=False, relinearise=False, Q=None,
                    R=None, hold=None, method="euler", schedule=None, gains_every=1, return_info=False, wind=None, gusts=None,
                    gust_every=None, ensemble=None, keep_traj=False, observer=None, meas_seed=0, return_estimate=False):
        """The reference's LQR loops (test_env_mk2.py:25-88 `LQR(linear=...)`; flight_sim.py:139,181) as ONE launch.
        linear=False (test_env_mk2.py:70-85): per step `u = _calc_LQR_action(p_dem, q_dem, r_dem, K, x._get_mpc_x(),
        u.initial_condition[1:])`, `u.values[1:] = u`, `step(u.values)`, the state in registers for all nsteps.  K [B,3,9] defaults
        to `_calc_LQR_gain()` at the current point; u0 [B,4] defaults to the CURRENT thrust command u.values[0] (the loop never
        writes it) with u.initial_condition[1:] as the LQR offset; demands scalars or [B].  u.values ends up holding the last
        action, as in the reference.  traj_every=k returns the states after every k-th step, [nsteps//k, 18, B].
        linear=True (test_env_mk2.py:46-62, what main.py:35 runs): the same law on the frozen reduced model,
        `x = ssr.Ad @ x + ssr.Bd @ u` from x = x._get_mpc_x(); x.values / u.values are not touched (the reference's loop works on
        locals).  Returns (x_storage [nsteps//k, 9, B], u_storage [nsteps//k, 3, B]) with k = traj_every or 1.
        relinearise=True: the same law with K re-derived at EVERY step, `_calc_LQR_gain(Q, R)` at the current (x, u) (Q, R: the
        weights of utils.py:219 dlqr, default env.py's Cd'Cd and I), in one launch (rollout_LQR_relin with track = (4, 5, 6));
        K must be None.  Returns the states as with linear=False.
        Demand histories: when any of p_dem, q_dem, r_dem is [S] or [S, B] (the pilot loop of flight_sim.py:141-182, whose demands
        change from frame to frame under one gain) the loop runs as one launch of f16_rollout_lqr_sched: step t takes row
        t // hold (hold defaults to 1; scalars are broadcast; S >= ceil(nsteps / hold)).  Not combined with linear=True or
        relinearise=True (ValueError).  Scalar / [B] demands call f16_rollout_lqr exactly as before; hold is then not taken.
        method="rk4" (the frozen-gain nonlinear loop only; ValueError with linear=True or relinearise=True, whose kernels step with
        the Euler step): Runge-Kutta steps, the action formed from the state at the start of a step and held over its four stages
        (f16_rollout_lqr_rk; constant demands are one row held for every step).
        schedule=gs (a schedule.GainSchedule), gains_every=k: the same nonlinear loop with K[:, 4:7] and the offset u0[1:] looked up
        in the gain table at the altitude and airspeed of the state at the start of every k-th step and held in between, in one
        launch of f16_rollout_lqr_gs, for both methods; the thrust command is held.  Not combined with K, linear=True or
        relinearise=True, and gains_every >= 1 (ValueError).  return_info=True (with a schedule) returns (traj, info) with
        info["gs_out"] [B]: at how many gain updates the aircraft was outside the table's grid (the edge cell is extended flat there).
        wind= / gusts= / gust_every= (see _air): the frozen-gain nonlinear loop in steady wind and gusts (f16_rollout_lqr_wind), both
        methods -- the disturbance-rejection loop; the controller reads the state, not the air data.  Not combined with linear=True,
        relinearise=True or schedule= (ValueError).
        ensemble=group / keep_traj= (see rollout_schedule): the statistics of the samples over the aircraft of each group instead of the
        samples (f16_rollout_lqr_wind_ens), on the same frozen-gain nonlinear loop, with or without wind= / gusts=; not combined
        with linear=True, relinearise=True or schedule= (ValueError).
        observer=obs (an observer.Observer), meas_seed=, return_estimate=: the same frozen-gain nonlinear loop on NOISY SENSORS -- per
        step the sensed channels of the reduced state are measured with sampled noise (meas_seed: the key of the counter-based
        sampler; it may equal a GustModel's seed), the observer corrects its estimate, the LQR law acts on the estimate and the
        observer predicts (f16_rollout_lqg_wind / f16_rollout_lqg_wind_ens; include/f16_hip.h "OUTPUT FEEDBACK"), both methods, with
        or without wind= / gusts= / ensemble=.  The estimate and the measurement-row counter live on the Observer: consecutive calls
        continue one flight.  return_estimate=True appends the samples of the estimate [S, 9, B] (the content of the estimate at every
        sample point: the prediction of the state stored there) to what the call returns.  Not combined with linear=True,
        relinearise=True or schedule= (ValueError)."""
        if observer is None and (return_estimate or meas_seed != 0):
            raise ValueError("meas_seed and return_estimate go with observer=")
        if observer is not None and (linear or relinearise or schedule is not None):
            raise ValueError("observer= runs on the nonlinear loop with a fixed gain (not with linear=True, relinearise=True or schedule=)")
        if (ensemble is not None or keep_traj) and (linear or relinearise or schedule is not None):
            raise ValueError("ensemble= runs on the nonlinear loop with a fixed gain (not with linear=True, relinearise=True or schedule=)")
        if (wind is not None or gusts is not None) and (linear or relinearise or schedule is not None):
            raise ValueError("wind= / gusts= run on the nonlinear loop with a fixed gain (not with linear=True, relinearise=True or schedule=)")
        if schedule is not None:
            if K is not None or linear or relinearise:
                raise ValueError("schedule= takes the gain from the table: not combined with K, linear=True or relinearise=True")
            if int(gains_every) < 1:
                raise ValueError(f"gains_every must be >= 1 (got {gains_every})")
        elif return_info or gains_every != 1:
            raise ValueError("gains_every and return_info go with schedule=")
        method = _lib.integrator(method, rk4=not (linear or relinearise))
        dem_seq = self._demand_schedule(p_dem, q_dem, r_dem)
        if dem_seq is not None:
            if linear or relinearise:
                raise ValueError("demand histories run on the nonlinear loop with a fixed gain (not with linear=True / relinearise=True)")
            hold, nsteps = self._schedule_steps(1 if hold is None else hold, nsteps, dem_seq.shape[0], "the demands")
        elif hold is not None:
            raise ValueError("hold goes with demand histories ([S] or [S, B]); scalar / [B] demands are constant")
        if relinearise:
            if K is not None or linear:
                raise ValueError("relinearise=True derives K at every step on the nonlinear model (K and linear are not taken)")
            xref = torch.zeros((9, self.B), dtype=torch.float64, device=self.device)
            xref[4:7] = self._demands(p_dem, q_dem, r_dem)                    # env.py:365-367
            u03 = self._u_init[1:4] if u0 is None else self._soa(u0, 4)[1:4]
            if u0 is not None:
                self._u[0] = self._soa(u0, 4)[0]
            k = int(traj_every or nsteps)
            traj = self._rollout_relin(nsteps, xref, 0x70, u03.contiguous(), _lib.make_weights(Q=Q, R=R), 1e-5, k,
                                       bool(traj_every), False, False)[0]
            return traj
        if schedule is not None:
            nsteps = int(nsteps)
            u0s = torch.cat((self._u[0:1], self._u_init[1:4]), 0).contiguous() if u0 is None else self._soa(u0, 4)
            rows, held = (self._demands(p_dem, q_dem, r_dem), max(nsteps, 1)) if dem_seq is None else (dem_seq, hold)
            traj = self._samples(nsteps, traj_every)
            gs_out = torch.zeros(self.B, dtype=torch.int32, device=self.device)
            grid, tab = schedule.grid(), schedule.device_table(self.device)
            self._check(self.lib.f16_rollout_lqr_gs(self.ctx.handle, _vp(self._x), _vp(u0s), ctypes.byref(grid), _vp(tab), int(gains_every),
                                                    _vp(rows), _vp(traj), _vp(self._u), _vp(gs_out), _vp(self.status), self.B, self.B,
                                                    nsteps, held, int(traj_every or 1), self.dt, self.xcg, self.fi_flag, int(method),
                                                    self.flags, self._stream))
            return (traj, dict(gs_out=gs_out)) if return_info else traj
        if K is None:
            K = self._calc_LQR_gain()
        Ks = torch.as_tensor(K, device=self.device, dtype=torch.float64).reshape(self.B, 27).t().contiguous()
        dem = self._demands(p_dem, q_dem, r_dem) if dem_seq is None else None
        if linear:
            if self.ssr is None:
                self.build_ssr()
            Ad, Bd, _ = self.ssr
            xref = torch.zeros((9, self.B), dtype=torch.float64, device=self.device)
            xref[4:7] = dem                                                  # env.py:365-367
            u03 = self._u_init[1:4].contiguous() if u0 is None else self._soa(u0, 4)[1:4].contiguous()
            return self.rollout_linear(self._x[P.mpc_x_idx], Ad, Bd, Ks, xref, u03, nsteps, track=(4, 5, 6), traj_every=traj_every,
                                       state_major=True)
        if u0 is None:       # test_env_mk2.py:76-82: the offset is u.initial_condition[1:], the thrust the CURRENT u.values[0]
            u0s = torch.cat((self._u[0:1], self._u_init[1:4]), 0).contiguous()
        else:
            u0s = self._soa(u0, 4)
        return self._rollout_call(u0s, nsteps, traj_every, hold=hold, K=Ks, dem=dem if dem_seq is None else dem_seq, method=method,
                                  air=self._air(wind, gusts, gust_every, nsteps), ensemble=ensemble, keep_traj=keep_traj,
                                  observer=None if observer is None else (observer, meas_seed, return_estimate))

    def rollout_LQR_relin(self, nsteps, x_ref=None, track=None, u0=None, Q=None, R=None, eps=1e-5, traj_every=None, gains_every=None,
                          hold=None):
        """The per-step re-linearised LQR loop (test_env.py:625-687 `test_LQR_dynamic_nl`) in ONE launch (C-ABI
        f16_rollout_lqr_relin): per step linearise at the current (x, u[1:4]) with eps -> ZOH -> Kd = dlqr(Ad, Bd, Q, R) ->
        u[1:4] = -Kd (x9 - x_ref) + u0 -> step(u.values), the thrust command held.  x_ref [B,9] or [9] defaults to the current x9;
        track (indices into x9) selects the entries of x_ref that are held fixed, the others follow the current x9 (None: all nine);
        u0 [B,3] or None (= 0); Q [9,9] / R [3,3] default to env.py's Cd'Cd and I.  x.values, u.values (the last command) and
        status are updated in place.  Samples every k-th step, k = traj_every or gains_every or 1 (the two must agree when both
        are given).  Returns (traj [n//k, 18, B], u_traj [n//k, 3, B], K_traj [n//k, B, 3, 9] = -dlqr or None without gains_every).
        A schedule of references: x_ref [S, 9, B] (state-major rows) with hold = h runs as one launch of f16_rollout_lqr_relin_sched:
        step t takes row t // h (h defaults to 1; S >= ceil(nsteps / h)); it equals one rollout_LQR_relin call per row.  hold is
        not taken without such a history (ValueError)."""
        if traj_every and gains_every and int(traj_every) != int(gains_every):
            raise ValueError("the states, commands and gains are sampled at one interval: traj_every must equal gains_every")
        k = int(traj_every or gains_every or 1)
        if x_ref is not None and np.ndim(x_ref) == 3:
            xr = torch.as_tensor(x_ref, dtype=torch.float64, device=self.device).contiguous()
            if tuple(xr.shape[1:]) != (9, self.B):
                raise ValueError(f"a schedule of references is [S, 9, {self.B}], not {tuple(xr.shape)}")
            hold, nsteps = self._schedule_steps(1 if hold is None else hold, nsteps, xr.shape[0], "x_ref")
            mask = 0x1FF if track is None else sum(1 << int(j) for j in track)
            u03 = None if u0 is None else self._soa(u0, 3)
            return self._rollout_relin(nsteps, xr, mask, u03, _lib.make_weights(Q=Q, R=R), eps, k, True, True, gains_every is not None,
                                       hold=hold)
        if hold is not None:
            raise ValueError("hold goes with a schedule of references, x_ref [S, 9, B]")
        xr = self._x[P.mpc_x_idx].clone() if x_ref is None else self._soa(x_ref, 9)
        mask = 0x1FF if track is None else sum(1 << int(j) for j in track)
        u03 = None if u0 is None else self._soa(u0, 3)
        return self._rollout_relin(nsteps, xr, mask, u03, _lib.make_weights(Q=Q, R=R), eps, k, True, True, gains_every is not None)

    def _rollout_relin(self, nsteps, xref, mask, u03, w, eps, k, want_x, want_u, want_k, hold=None):
        """f16_rollout_lqr_relin on the resident state: xref [9,B], u03 [3,B] or None (state-major, contiguous); with hold:
        f16_rollout_lqr_relin_sched, xref [S,9,B]."""
        nsteps, k = int(nsteps), int(k)
        if k < 1 or nsteps % k:
            raise ValueError(f"nsteps ({nsteps}) must be a multiple of the sampling interval ({k})")
        mk = lambda want, rows: torch.empty((nsteps // k, rows, self.B), dtype=torch.float64, device=self.device) if want else None
        traj, u_traj, K_traj = mk(want_x, 18), mk(want_u, 3), mk(want_k, 27)
        name, hold = ("f16_rollout_lqr_relin", []) if hold is None else ("f16_rollout_lqr_relin_sched", [int(hold)])
        self._check(getattr(self.lib, name)(self.ctx.handle, _vp(self._x), _vp(self._u), _vp(xref), _vp(u03),
                                            ctypes.byref(w) if w else None, _vp(traj), _vp(u_traj), _vp(K_traj), _vp(self.status),
                                            self.B, self.B, nsteps, *hold, k, int(mask), float(eps), self.dt, self.xcg, self.fi_flag,
                                            self.flags, self._stream))
        return traj, u_traj, None if K_traj is None else K_traj.permute(0, 2, 1).reshape(nsteps // k, self.B, 3, 9)

    def rollout_linear(self, x9, Ad, Bd, K, x_ref, u0, nsteps, track=None, traj_every=None, state_major=False):
        """`u = -K (x_ref - x) + u0; x = Ad x + Bd u` for nsteps on per-aircraft 9-state / 3-input linear models (C-ABI
        f16_rollout_lqr_linear): the loop of test_env_mk2.py:54-62 (track = (4, 5, 6): the reference follows the current state
        except the three rate demands, env.py:360-371; K = -dlqr as `_calc_LQR_gain` returns it) and of test_env.py:553-559
        (track=None: a fixed full reference; pass K = -dlqr(A, B, Q, R)).  x9 [B,9], Ad [B,9,9], Bd [B,9,3], K [B,3,9], x_ref [B,9],
        u0 [B,3] or None -- or, with state_major=True, the device layout itself ([9,B], [81,B], [27,B], [27,B], [9,B], [3,B]: what
        build_ssr and the gain kernel hold).  Returns (x_storage [nsteps//k, 9, B], u_storage [nsteps//k, 3, B]), k = traj_every or 1;
        the final state is kept in `last_linear_state` [B,9]."""
        def sm(a, rows):                      # -> contiguous state-major [rows, B]
            t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))
            t = t.to(device=self.device, dtype=torch.float64)
            if state_major:
                assert tuple(t.shape) == (rows, self.B), (tuple(t.shape), rows)
                return t.contiguous()
            return t.reshape(self.B, rows).t().contiguous()
        xs = sm(x9, 9).clone()
        Ads, Bds, Ks, xr = sm(Ad, 81), sm(Bd, 27), sm(K, 27), sm(x_ref, 9)
        u0s = sm(u0, 3) if u0 is not None else None
        k = int(traj_every or 1)
        trx, tru = self._samples(nsteps, k, 9), self._samples(nsteps, k, 3)
        mask = 0x1FF if track is None else sum(1 << int(j) for j in track)
        self._check(self.lib.f16_rollout_lqr_linear(self.ctx.handle, _vp(xs), _vp(Ads), _vp(Bds), _vp(Ks), _vp(xr), _vp(u0s), _vp(trx),
                                                    _vp(tru), self.B, self.B, int(nsteps), k, mask, self._stream))
        self.last_linear_state = xs.t()
        return trx, tru

    # ------------------------------------------------------------------ env.py:373-424
    @staticmethod
    def _soft_rows(soft):
        """The `soft` keyword as the nine weights of f16_mpc_plan_soft_rows (MPC-state order), or None for hard rows: a scalar is that
        weight on the six bounded rows (alpha, beta, p, q, r, lf2), a 9-vector is taken as it is; None and all zeros mean hard rows."""
        if soft is None:
            return None
        w = np.asarray(soft, dtype=np.float64)
        if w.ndim == 0:
            w = np.where(np.array([0, 0, 1, 1, 1, 1, 1, 0, 1], dtype=bool), float(w), 0.0)
        if w.shape != (9,):
            raise ValueError(f"soft must be a scalar or nine weights in MPC-state order (got shape {w.shape})")
        return None if not w.any() else tuple(float(v) for v in w)

    def prepare_MPC(self, hzn, settings=None, warm_start=False, weights=None, ctrl_every=1, soft=None):
        """Prepare the model-only part of calc_MPC_action for horizon hzn from the frozen reduced model self.ssr
        (env.py:49-60 freezes it; the reference still rebuilds the QP on every call): DARE, terminal weight, prediction
        blocks, P, A'A, start rho and the KKT factorisation stay on the device.  `_calc_MPC_action(..., use_plan=True)`
        then only forms the state-dependent vectors and iterates; results are bit-identical to the one-shot call.
        ctrl_every = k > 1: a plan for a controller that runs every k plant steps (rollout_MPC(..., ctrl_every=k)).  Its model is this
        environment's linearisation -- the continuous (Ac, Bc) of build_ssr's point -- through the zero-order hold at the control
        period k * self.dt, which is also the dt of its rate rows; self.ssr itself is untouched.
        soft: soft state rows (C-ABI f16_mpc_plan_soft_rows) -- a scalar is that penalty weight on the six bounded state rows, a
        9-vector is in MPC-state order; every solve on the plan then penalises leaving the state box instead of forbidding it, and
        status bit F16_ST_QP_SOFT_ACTIVE marks a solve that did leave it.  hzn <= 30 and equilibrated solves only."""
        ctrl_every = int(ctrl_every)
        w9 = self._soft_rows(soft)
        if ctrl_every < 1:
            raise ValueError(f"ctrl_every must be >= 1 (got {ctrl_every})")
        if self.ssr is None:
            self.build_ssr()
        self.release_MPC_plan()
        Ad, Bd, Cd = self.ssr
        plan_dt = self.dt
        if ctrl_every > 1:
            if getattr(self, "_ssr_cont", None) is None:
                raise ValueError("ctrl_every > 1 discretises the continuous model of build_ssr(); self.ssr was set by hand")
            Ac, Bc = self._ssr_cont
            plan_dt = ctrl_every * self.dt
            Ad, Bd = torch.empty_like(Ac), torch.empty_like(Bc)
            self._check(self.lib.f16_c2d_batch(self.ctx.handle, _vp(Ac), _vp(Bc), _vp(Ad), _vp(Bd), self.B, self.B, plan_dt, self._stream))
        s = self._qp_settings(settings)
        h = ctypes.c_void_p()
        w = _lib.make_weights(**weights) if weights else None           # (utils.py:21 Q, R and the six bound vectors; fixed for the plan)
        self._check(self.lib.f16_mpc_plan_create_w(self.ctx.handle, ctypes.byref(h), _vp(Ad), _vp(Bd), _vp(Cd),
                                                   ctypes.byref(w) if w else None, self.B, self.B, int(hzn), plan_dt, ctypes.byref(s),
                                                   self._stream))
        if w9 is not None:
            rc = self.lib.f16_mpc_plan_soft_rows(h, (ctypes.c_double * 9)(*w9))
            if rc:                      # (a plan the one-wavefront solver does not serve: no half-made plan is kept)
                self.lib.f16_mpc_plan_destroy(h)
                self._check(rc)
        self._plan, self._plan_hzn, self._plan_ctrl_every = h, int(hzn), ctrl_every
        self._plan_default_settings = int((settings or {}).get("scaling", 10)) > 0       # (what f16_rollout_mpc takes: equilibrated solves)
        if warm_start:      # OSQP's in-object default; the reference starts cold on every call (new object), so: opt-in
            self._check(self.lib.f16_mpc_plan_warm_start(h, 1))
        self._plan_args = dict(settings=settings, warm_start=warm_start, weights=weights, soft=soft)
        self._plan_foreign = False      # True once rollout_MPC(relinearise=True) has overwritten the plan's model blocks
        return self

    _KEEP_SOFT = object()      # (the `soft` of a call that does not name it: whatever the plan has)

    def _frozen_plan(self, hzn, ctrl_every=1, soft=_KEEP_SOFT):
        """The prepared plan of (horizon hzn, control period ctrl_every plant steps) for a frozen-model call: made if absent; prepared
        AGAIN from self.ssr (same settings, weights, warm-start switch and soft rows) if the re-linearised loop has run on it -- its
        model blocks then hold per-step models, and the library refuses it for frozen-model calls.  soft: the soft rows the call asks
        for; a plan with other ones is prepared again with these."""
        if getattr(self, "_plan", None) is None or (self._plan_hzn, self._plan_ctrl_every) != (int(hzn), int(ctrl_every)):
            self.prepare_MPC(hzn, ctrl_every=ctrl_every, soft=None if soft is self._KEEP_SOFT else soft)
        elif soft is not self._KEEP_SOFT and self._soft_rows(soft) != self._soft_rows(self._plan_args.get("soft")):
            self.prepare_MPC(hzn, ctrl_every=ctrl_every, **dict(self._plan_args, soft=soft))
        elif getattr(self, "_plan_foreign", False):
            self.prepare_MPC(hzn, ctrl_every=ctrl_every, **self._plan_args)
        return self._plan

    def release_MPC_plan(self):
        if getattr(self, "_plan", None) is not None:
            self.lib.f16_mpc_plan_destroy(self._plan)
        self._plan, self._plan_hzn, self._plan_foreign, self._plan_ctrl_every = None, None, False, 1

    def __del__(self):
        try:
            self.release_MPC_plan()
        except Exception:
            pass

    @staticmethod
    def solver_modes():
        """Named QP-solver settings (overrides of f16_qp_default_settings) for benchmarks and tests."""
        return {"osqp_defaults": None,                                        # what env.py:420-422 invokes (the library default)
                "osqp_defaults_rho_every_25": dict(rho_every=25),             # OSQP's wall-clock interval typically lands here
                "builder_rule": dict(scaling=0, rho=0.0),                     # no equilibration, rho0 = 2 sqrt(tr P / tr A'A)
                "rho_0p1_unscaled": dict(scaling=0, rho=0.1)}

    def setup_OSQP(self, p_dem, q_dem, r_dem, hzn, b=0, weights=None, x_ref=None):
        """The QP of aircraft b in the reference's own form (utils.py:21-167 `setup_OSQP`): dense host arrays
        (P [n,n], q [n], A [15 hzn, n], l, u) with n = 3 hzn and the reference's row order (9 hzn state rows, 3 hzn
        command rows, 3 hzn rate rows; unbounded rows carry +-inf), built on the device from the frozen reduced
        model and the current state -- for callers that hand the QP to a solver of their own, and for the tests.
        weights: dict(Q=, R=, x_lb=, x_ub=, u_lb=, u_ub=, udot_lb=, udot_ub=) -- the arguments of utils.py:21 that env.py fills
        with constants (any subset; any bound pattern); x_ref [B,9] (or [9]): the reference itself instead of "x with
        x[5:8] = demands" (env.py:380-383)."""
        if self.ssr is None:
            self.build_ssr()
        Ad, Bd, Cd = self.ssr
        dem = self._demands(p_dem, q_dem, r_dem)
        n, rows = 3 * int(hzn), 15 * int(hzn)
        P, q, A = np.zeros((n, n)), np.zeros(n), np.zeros((rows, n))
        l, u = np.zeros(rows), np.zeros(rows)
        hp = lambda a: ctypes.c_void_p(a.ctypes.data)
        w = _lib.make_weights(**weights) if weights else None
        xr = self._soa(x_ref, 9) if x_ref is not None else None
        self._check(self.lib.f16_mpc_qp_debug_w(self.ctx.handle, _vp(Ad), _vp(Bd), _vp(Cd), _vp(self._x), _vp(dem), _vp(xr),
                                                ctypes.byref(w) if w else None, int(b), self.B, int(hzn), self.dt, hp(P), hp(q), hp(A),
                                                hp(l), hp(u)))
        return P, q, A, l, u

    def _calc_MPC_action(self, p_dem, q_dem, r_dem, hzn, settings=None, return_info=False, relinearise=False,
                         use_plan=False, weights=None, x_ref=None, ctrl_every=1, model=None, period=None, soft=None):
        """First MPC move [B,3] (dh,da,dr commands) for demands p,q,r (scalars or [B]) over horizon hzn, from the
        frozen reduced model self.ssr (env.py:385-387) and the current state.  The QP of utils.py:21-167 is solved
        on the GPU by OSQP-style ADMM (the reference calls the `osqp` package, env.py:420-422).
        weights / x_ref: as in setup_OSQP (the solvers keep the reference's pattern of bounded rows; a plan fixes its weights at
        prepare_MPC, x_ref is per call).  ctrl_every = k > 1 (use_plan only): the plan of control period k * self.dt
        (prepare_MPC(ctrl_every=k)) -- the solve of the multi-rate loop rollout_MPC(..., ctrl_every=k).
        model = (Ad, Bd, Cd) (state-major [81,B], [27,B], [81,B]) and period (seconds, default self.dt; the dt of the rate rows), not
        with use_plan: the solve on that model instead of self.ssr, which is then neither read nor written.
        soft (use_plan only): the plan's soft state rows (prepare_MPC); a plan with other ones is prepared again.  A call that does not
        name it solves with whatever the plan has."""
        if soft is not None and not use_plan:
            raise ValueError("soft state rows are a property of a prepared plan: use_plan=True")
        if int(ctrl_every) != 1 and not use_plan:
            raise ValueError("ctrl_every > 1 is a property of a prepared plan: use_plan=True")
        # relinearise=True: SURVEY.md 8f-2 -- the reduced model is re-derived at the CURRENT state on every call (the
        # reference freezes it at construction, env.py:49-60; its test_env.py:625-687 loops re-linearise per step)
        if model is None:
            if self.ssr is None or relinearise:
                self.build_ssr()
            model = self.ssr
        dem = self._demands(p_dem, q_dem, r_dem)
        ucmd = torch.empty((3, self.B), dtype=torch.float64, device=self.device)
        info = torch.empty((4, self.B), dtype=torch.float64, device=self.device)
        useq = torch.empty((3 * hzn, self.B), dtype=torch.float64, device=self.device) if return_info else None
        st = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        xr = self._soa(x_ref, 9) if x_ref is not None else None
        if use_plan:
            if relinearise or settings or weights or model is not self.ssr or period is not None:
                raise ValueError("a prepared plan fixes the model, the period, the QP settings and the weights (prepare_MPC)")
            self._frozen_plan(hzn, ctrl_every, self._KEEP_SOFT if soft is None else soft)
            self._check(self.lib.f16_mpc_plan_solve_w(self._plan, _vp(self._x), _vp(dem), _vp(xr), _vp(ucmd), _vp(useq), _vp(info),
                                                      _vp(st), self._stream))
        else:
            Ad, Bd, Cd = model
            s = self._qp_settings(settings)
            w = _lib.make_weights(**weights) if weights else None
            self._check(self.lib.f16_mpc_batch_w(self.ctx.handle, _vp(Ad), _vp(Bd), _vp(Cd), _vp(self._x), _vp(dem), _vp(xr),
                                                 ctypes.byref(w) if w else None, _vp(ucmd), _vp(useq), _vp(info), _vp(st), self.B, self.B,
                                                 int(hzn), self.dt if period is None else period, ctypes.byref(s), self._stream))
        self.last_status, self.last_iters = st, info[0]
        self.status |= st          # sticky: F16_ST_QP_INFEASIBLE / QP_MAXITER of ANY step stay visible after a closed loop
        if return_info:
            return ucmd.t(), dict(iters=info[0], r_prim=info[1], r_dual=info[2], rho=info[3], u_seq=useq.t(), status=st)
        return ucmd.t()

    calc_MPC_action = _calc_MPC_action

    def rollout_MPC(self, nsteps, p_dem, q_dem, r_dem, hzn, traj_every=None, return_info=False, hold_command=False,
                    relinearise=False, eps=1e-5, ctrl_every=1, model_every=None, dem_every=None, method="euler", soft=None):
        """The reference's closed MPC loop (test_env.py:480-495; BASELINE config 5) as ONE launch (C-ABI f16_rollout_mpc): per step
        `cmd = _calc_MPC_action(p_dem, q_dem, r_dem, hzn); u.values[1:] = cmd; step(u.values)` from the frozen reduced model
        (env.py:49-60) with OSQP's default settings (every solve cold, as the reference's -- or warm from the step before when the plan was
        prepared with warm_start=True).  Work items are (step, aircraft) pairs taken from one queue by one wavefront per
        SIMD, so no step waits for another aircraft's solve -- the host loop `dist.closed_loop_mpc_rollout` (the checker of this
        call) joins the batch after every solve.  Uses the prepared plan of horizon hzn (prepare_MPC; made here if absent).
        Returns the states after every traj_every-th step [nsteps//k, 18, B] (None without traj_every); with return_info also
        dict(cmd [nsteps, 3, B]: what calc_MPC_action returned per step, iters [nsteps, B]).  x.values / u.values / status are
        updated in place; u.values ends up holding the last command.  hold_command: F16_FLAG_HOLD_COMMAND.
        relinearise=True (C-ABI f16_rollout_mpc_relin): the reduced model is re-derived at EVERY step at the current
        (x.values, u.values[1:4]) with the forward-difference step eps -- `_calc_MPC_action(..., relinearise=True)` per step, still one
        launch.  The info dict then also carries model [nsteps//k, 189, B]: Ad (81) | Bd (27) | Cd (81) of the solve of every stored
        step (NaN where an aircraft was not solved for).  The call takes the plan's weights, bounds and settings but overwrites its
        model blocks, so the plan is marked: further relinearise=True calls go on using it, while the next frozen-model call
        (use_plan=True, rollout_MPC without relinearise) prepares it again from self.ssr, which is untouched.
        ctrl_every = k > 1 (C-ABI f16_rollout_mpc_hold / f16_rollout_mpc_relin_hold): the controller runs every k-th plant step and its
        command is held for k steps of self.dt; the plan's model and rate rows are at the control period k * self.dt
        (prepare_MPC(ctrl_every=k); made here if absent).  nsteps and traj_every stay in PLANT steps, nsteps % k == 0; cmd and iters
        have one row per control step ([nsteps // k, ...]); model (relinearise) [nsteps // k // model_every, 189, B] holds the model of
        every model_every-th control step (default 1).  The envelope is tested before every plant step.
        Demand histories (C-ABI f16_rollout_mpc_sched / f16_rollout_mpc_relin_sched; the pilot loop of flight_sim.py:141-182, whose
        demands change while the controller runs): when any of p_dem, q_dem, r_dem is [S] or [S, B] (rollout_LQR's rule: [B] is a
        constant demand per aircraft, scalars are broadcast) the loop still runs as one launch and control step c takes row
        c // dem_every (default 1; S >= ceil(control steps / dem_every)), with relinearise and ctrl_every alike.  The demand of a control
        step is held over that step's whole horizon, so the call equals one call per row.  A 2-D p_dem with q_dem is None and
        r_dem is None stays a ready [3, B] block of constant demands.  dem_every without a history, too few rows and
        dem_every < 1 raise ValueError.  method: "euler" only -- the loop's plant step is the Euler step; "rk4" raises ValueError.
        soft: the plan's soft state rows (prepare_MPC); the plan is prepared, or prepared again, when it has other ones.  A call that
        does not name it runs with whatever the plan has."""
        _lib.integrator(method, rk4=False)
        nsteps, hold = int(nsteps), int(ctrl_every)
        if hold < 1 or nsteps % hold:      # (argument checks first: they need no GPU)
            raise ValueError(f"nsteps ({nsteps}) must be a multiple of ctrl_every ({hold}) >= 1")
        nctrl = nsteps // hold
        dem_seq, dem_every = self._mpc_demand_rows(p_dem, q_dem, r_dem, dem_every, nctrl)
        # f16_rollout_mpc / f16_rollout_mpc_relin, the oldest calls: zero steps are a no-op, the models are sampled with the states, and
        # without relinearise the library alone checks the arguments.  (A schedule at ctrl_every = 1 is the _sched call with hold = 1.)
        oldest = hold == 1 and dem_seq is None
        if oldest and model_every is not None:
            raise ValueError("model_every belongs to ctrl_every > 1 (with ctrl_every = 1 the models follow traj_every)")
        model_every = int(traj_every or 1) if oldest else 1 if model_every is None else int(model_every)
        if not oldest and nctrl < 1:
            raise ValueError(f"ctrl_every={hold} needs nsteps >= {hold} (got {nsteps})")
        if relinearise or not oldest:
            if nsteps < 0 or (traj_every and (int(traj_every) < 1 or nsteps % int(traj_every))):
                raise ValueError(f"nsteps ({nsteps}) must be >= 0 and a multiple of traj_every ({traj_every})")
            if int(hzn) < 1 or int(hzn) > 30:
                raise ValueError(f"relinearise=True, ctrl_every > 1 and demand histories run on the one-launch loop: 1 <= hzn <= 30 (got {hzn})")
            if relinearise and not float(eps) > 0.0:
                raise ValueError(f"relinearise=True needs a forward-difference step eps > 0 (got {eps})")
            if model_every < 1 or (relinearise and nctrl % model_every):
                raise ValueError(f"the control steps ({nctrl}) must be a multiple of model_every ({model_every}) >= 1")
        dem = self._demands(p_dem, q_dem, r_dem) if dem_seq is None else dem_seq
        return self._rollout_mpc_call(hzn, nctrl, hold, dem, dem_every, traj_every, model_every, relinearise, eps, return_info, hold_command,
                                      self._KEEP_SOFT if soft is None else soft)

    def _rollout_mpc_call(self, hzn, nctrl, hold, dem, dem_every, traj_every, model_every, relinearise, eps, return_info, hold_command,
                          soft=_KEEP_SOFT):
        """rollout_MPC behind its argument checks: the plan, the outputs, the ONE call into the library.  nctrl control steps of `hold`
        plant steps; dem [3,B], or [S,3,B] with dem_every control steps per row; the narrowest entry point that can run the loop."""
        sched, nsteps = dem_every is not None, nctrl * hold
        wide = sched or hold > 1      # the _hold / _sched parameter lists: nctrl, hold and the plant's dt beside the oldest calls' own
        if not relinearise:
            self._frozen_plan(hzn, hold, soft)
        elif getattr(self, "_plan", None) is None or (self._plan_hzn, self._plan_ctrl_every) != (int(hzn), hold):
            self.prepare_MPC(hzn, ctrl_every=hold, soft=None if soft is self._KEEP_SOFT else soft)
        elif soft is not self._KEEP_SOFT and self._soft_rows(soft) != self._soft_rows(self._plan_args.get("soft")):
            self.prepare_MPC(hzn, ctrl_every=hold, **dict(self._plan_args, soft=soft))
        if (relinearise or wide) and not self._plan_default_settings:
            raise ValueError("relinearise=True, ctrl_every > 1 and demand histories need a plan with equilibrated solves (scaling > 0)")
        k = int(traj_every or 1)
        assert nsteps % k == 0
        new = lambda want, *shape, dtype=torch.float64: torch.empty(shape + (self.B,), dtype=dtype, device=self.device) if want else None
        traj, cmd, its = new(traj_every, nsteps // k, 18), new(return_info, nctrl, 3), new(return_info, nctrl, dtype=torch.int32)
        model = new(return_info and relinearise, nctrl // model_every, 189)
        flags = self.flags | (_lib.F16_FLAG_HOLD_COMMAND if hold_command else 0)
        if relinearise:
            self._plan_foreign = nctrl > 0 or self._plan_foreign      # its model blocks are per-step models from here on, not self.ssr
        # the six parameter lists of include/f16_hip.h are this one list; an entry point takes the entries that apply to it
        name = "f16_rollout_mpc" + ("_relin" if relinearise else "") + ("_sched" if sched else "_hold" if wide else "")
        args = [v for v, taken in (
            (self._plan, True), (_vp(self._x), True), (_vp(self._u), True), (_vp(dem), True), (_vp(traj), True), (_vp(cmd), True),
            (_vp(its), True), (_vp(model), relinearise), (_vp(self.status), True), (nctrl, True), (hold, wide), (dem_every, sched),
            (k, True), (model_every, wide and relinearise), (self.dt, wide), (float(eps), relinearise), (self.xcg, True),
            (self.fi_flag, True), (flags, True), (self._stream, True)) if taken]
        self._check(getattr(self.lib, name)(*args))
        info = dict(cmd=cmd, iters=its, **(dict(model=model) if relinearise else {}))
        return (traj, info) if return_info else traj

    def _calc_constr_checking_hzn(self, max_hzn=150, settings=None, return_info=False):
        """env.py:426-436: the first move of calc_MPC_action(0, 0, 0, N) for every horizon N = 1..max_hzn (the reference
        fills u[:, N-1] for one aircraft; here [B, 3, max_hzn]).  One library call (f16_mpc_hzn_sweep): the long horizons
        are solved by a single launch over every (horizon, aircraft) pair; each slice equals _calc_MPC_action(0, 0, 0, N)."""
        if self.ssr is None:
            self.build_ssr()
        Ad, Bd, Cd = self.ssr
        dem = torch.zeros((3, self.B), dtype=torch.float64, device=self.device)
        ucmd = torch.empty((max_hzn, 3, self.B), dtype=torch.float64, device=self.device)
        info = torch.empty((max_hzn, 4, self.B), dtype=torch.float64, device=self.device)
        st = torch.zeros((max_hzn, self.B), dtype=torch.int32, device=self.device)
        s = self._qp_settings(settings)
        self._check(self.lib.f16_mpc_hzn_sweep(self.ctx.handle, _vp(Ad), _vp(Bd), _vp(Cd), _vp(self._x), _vp(dem), _vp(ucmd),
                                               _vp(info), _vp(st), self.B, self.B, 1, int(max_hzn), self.dt, ctypes.byref(s),
                                               self._stream))
        self.last_status = st
        out = ucmd.permute(2, 1, 0)
        if return_info:
            return out, dict(iters=info[:, 0], r_prim=info[:, 1], r_dual=info[:, 2], rho=info[:, 3], status=st)
        return out
