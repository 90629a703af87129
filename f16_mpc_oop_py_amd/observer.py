"""Output feedback for the frozen-gain LQR loop (include/f16_hip.h "OUTPUT FEEDBACK": f16_kalman_batch, f16_observer_step,
f16_rollout_lqg_wind, f16_rollout_lqg_wind_ens): sampled sensor noise, a steady-state Kalman filter on the reduced 9-state model, the
LQR law on the estimate.

`Observer` is what F16Batch.rollout_LQR takes as `observer=`: the model records (Ad, Bd, Lf, x9_trim, s_trim per group of aircraft),
the sensor mask, the noise deviations and the group size, and -- per batch it has flown with -- the estimate and the measurement-row
counter, so that consecutive calls continue one flight (as wind.GustModel keeps its generator's state).  `Observer.build` designs the
gain on the GPU (f16_kalman_batch); `Observer.passthrough` sets Lf = I on the sensed channels: raw noisy feedback, the baseline.
`meas_normals`, `observer_reference` and `kalman_reference` restate the sampler, the per-step rule and the doubling in numpy:
documentation and the tests' reference, like wind.gust_reference; the product never calls them.
"""
import ctypes

import numpy as np

from . import lib as _lib
from . import parameters as P
from .mppi import philox4x32_10

MEAS_COUNTER_WORD = 0xFFFFFFFE        # counter word 2 of a measurement row: gusts use 0xFFFFFFFF, MPPI's sample index values < 256
OBS_DOUBLES = _lib.F16_OBS_DOUBLES
OBS_BD, OBS_LF, OBS_TRIM, OBS_STRIM = 81, 108, 189, 198      # offsets inside a model record
S_IDX = P.mpc_u_in_x_idx              # the three surface positions: the reduced model's inputs


def check_sensed(sensed):
    sensed = int(sensed)
    if not 1 <= sensed <= 0x1ff:
        raise ValueError(f"sensed must be a mask of the nine channels, 1 .. 0x1ff, not {sensed:#x}")
    return sensed


def check_sigma(sigma):
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (9,)).copy()
    if not (np.all(np.isfinite(sg)) and np.all(sg >= 0)):
        raise ValueError("sigma must be finite and >= 0")
    return sg


def channels(sensed):
    return [k for k in range(9) if (int(sensed) >> k) & 1]


# ------------------------------------------------------------------------------------------------ the numpy restatements
def meas_normals(seed, row0, nrows, aircraft, sensed=0x1ff):
    """The standard normals of measurement rows row0 .. row0 + nrows - 1, [nrows, aircraft, 9]: call j (0, 1, 2) is Philox4x32-10 on
    the counter (row, j, 0xFFFFFFFE, aircraft), key = the two halves of the seed; U_i = (r_i + 0.5) 2^-32; Box-Muller on (U0, U1) and
    (U2, U3), all four outputs (ra c1, ra s1, rb c3, rb s3) for channels 4 j .. 4 j + 3.  A call whose channels are all unsensed is
    not made: its channels are 0 here."""
    seed = int(seed)
    r, a = np.meshgrid((np.arange(nrows, dtype=np.uint64) + np.uint64(int(row0))) & np.uint64(0xffffffff), np.arange(aircraft, dtype=np.uint64),
                       indexing="ij")
    out = np.zeros((nrows, aircraft, 12))
    key = np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], dtype=np.uint64)
    for j in range(3):
        if not (int(sensed) >> (4 * j)) & 0xf:
            continue
        ctr = np.stack([r, np.full_like(r, j), np.full_like(r, MEAS_COUNTER_WORD), a], -1)
        U = (philox4x32_10(ctr, key).astype(np.float64) + 0.5) * 2.0 ** -32
        ra, rb = np.sqrt(-2.0 * np.log(U[..., 0])), np.sqrt(-2.0 * np.log(U[..., 2]))
        t1, t3 = 2.0 * np.pi * U[..., 1], 2.0 * np.pi * U[..., 3]
        out[..., 4 * j:4 * j + 4] = np.stack([ra * np.cos(t1), ra * np.sin(t1), rb * np.cos(t3), rb * np.sin(t3)], -1)
    return out[..., :9]


def kalman_reference(Ad, w, v, sensed, maxit=60):
    """f16_kalman_batch restated for one model: the structure-preserving doubling of the filter Riccati equation
        A0 = Ad', G0 = C'V^-1 C, H0 = W;   Wk = (I + G H)^-1;   A+ = A Wk A;   G+ = G + A Wk G A';   H+ = H + A' H Wk A
    (G+ and H+ made symmetric after every doubling)
    until max|dH| <= 1e-16 max|H| (at most maxit doublings), P = (H + H') / 2, Lf = P (I + G0 P)^-1 C'V^-1 in the 9 x 9 frame.
    Ad [9, 9]; w [9]; v [9] (read on sensed channels) -> (P [9, 9], Lf [9, 9], doublings; maxit: not converged or not finite)."""
    Ad, w, v = np.asarray(Ad, dtype=np.float64).reshape(9, 9), np.asarray(w, dtype=np.float64).reshape(9), np.asarray(v, dtype=np.float64).reshape(9)
    g = np.zeros(9)
    for k in channels(check_sensed(sensed)):
        g[k] = 1.0 / v[k]
    A, G0, H, I = Ad.T.copy(), np.diag(g), np.diag(w), np.eye(9)
    G, it = G0.copy(), 0
    with np.errstate(all="ignore"):
        while it < maxit:
            it += 1
            try:
                Wk = np.linalg.inv(I + G @ H)
            except np.linalg.LinAlgError:
                it = maxit
                break
            AW = A @ Wk
            dH = A.T @ H @ Wk @ A
            A, G, H = AW @ A, G + AW @ G @ A.T, H + dH
            G, H = 0.5 * (G + G.T), 0.5 * (H + H.T)      # (the kernel's products rely on both being symmetric: it keeps them so)
            if np.abs(dH).max() <= 1e-16 * np.abs(H).max():
                break
        else:
            it = maxit
        if not np.isfinite(H).all():
            it = maxit
        Pm = 0.5 * (H + H.T)
        try:
            Lf = Pm @ np.linalg.inv(I + G0 @ Pm) @ G0
        except np.linalg.LinAlgError:
            Lf, it = np.full((9, 9), np.nan), maxit
    return Pm, Lf, it


def pack_models(Ad, Bd, Lf, x9_trim, s_trim):
    """The model records obs[M][F16_OBS_DOUBLES] of include/f16_hip.h from Ad [M, 9, 9], Bd [M, 9, 3], Lf [M, 9, 9], x9_trim [M, 9],
    s_trim [M, 3]"""
    Ad = np.asarray(Ad, dtype=np.float64).reshape(-1, 81)
    M = len(Ad)
    rec = np.zeros((M, OBS_DOUBLES))
    rec[:, :81] = Ad
    rec[:, OBS_BD:OBS_BD + 27] = np.asarray(Bd, dtype=np.float64).reshape(M, 27)
    rec[:, OBS_LF:OBS_LF + 81] = np.asarray(Lf, dtype=np.float64).reshape(M, 81)
    rec[:, OBS_TRIM:OBS_TRIM + 9] = np.asarray(x9_trim, dtype=np.float64).reshape(M, 9)
    rec[:, OBS_STRIM:OBS_STRIM + 3] = np.asarray(s_trim, dtype=np.float64).reshape(M, 3)
    return rec


def observer_reference(models, group, sensed, x9, s, xm, K, dem, u0, sigma=None, normals=None, y=None):
    """Steps 1 - 4 of the rule for B aircraft, one step.  models [M, 208], aircraft b uses model b // group (group 0: model 0); x9
    [B, 9], s [B, 3], xm [B, 9] (the prediction), K [B, 3, 9] or [3, 9], dem [B, 3], u0 [B, 4].  The measurements: y [B, 9] as given
    (the sensed channels are read), else x9 + (sigma * normals) with normals [B, 9].
    -> dict(y, xh: the corrected estimate, xm: the new prediction, u [B, 4], mag_xh, mag_xm, mag_u: the sums of |terms| per entry)"""
    models = np.asarray(models, dtype=np.float64).reshape(-1, OBS_DOUBLES)
    x9, s, xm = (np.asarray(v, dtype=np.float64) for v in (x9, s, xm))
    B = len(x9)
    idx = np.arange(B) // int(group) if group else np.zeros(B, dtype=int)
    m = models[idx]
    Ad, Bd, Lf = m[:, :81].reshape(B, 9, 9), m[:, OBS_BD:OBS_BD + 27].reshape(B, 9, 3), m[:, OBS_LF:OBS_LF + 81].reshape(B, 9, 9)
    trim, strim = m[:, OBS_TRIM:OBS_TRIM + 9], m[:, OBS_STRIM:OBS_STRIM + 3]
    ch = channels(check_sensed(sensed))
    if y is None:
        y = x9 + (np.asarray(sigma, dtype=np.float64) * np.asarray(normals, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64)
    xh, mag_xh = xm.copy(), np.abs(xm)
    for k in ch:
        t = Lf[:, :, k] * (y[:, k] - xm[:, k])[:, None]
        xh, mag_xh = xh + t, mag_xh + np.abs(t)
    K = np.broadcast_to(np.asarray(K, dtype=np.float64), (B, 3, 9))
    dem, u0 = np.asarray(dem, dtype=np.float64), np.asarray(u0, dtype=np.float64)
    e = dem - xh[:, 4:7]
    t = K[:, :, 4:7] * e[:, None, :]
    u, mag_u = u0.copy(), np.abs(u0[:, 1:4]) + np.abs(t).sum(2)
    u[:, 1:4] = -((t[:, :, 0] + t[:, :, 1]) + t[:, :, 2]) + u0[:, 1:4]
    xn, mag_xm = trim.copy(), np.abs(trim)
    d, ds = xh - trim, s - strim
    for j in range(9):
        t = Ad[:, :, j] * d[:, j][:, None]
        xn, mag_xm = xn + t, mag_xm + np.abs(t)
    for j in range(3):
        t = Bd[:, :, j] * ds[:, j][:, None]
        xn, mag_xm = xn + t, mag_xm + np.abs(t)
    return dict(y=y, xh=xh, xm=xn, u=u, mag_xh=mag_xh, mag_xm=mag_xm, mag_u=mag_u)


# ------------------------------------------------------------------------------------------------ the object rollout_LQR takes
class Observer:
    """Models, gain, sensors, noise and grouping of an output-feedback loop.  models [M, 208] (pack_models); sensed: the 9-bit mask;
    sigma: the noise deviation per channel ([9] or a scalar, units of the states: rad, rad/s, deg for the flap states); group: aircraft
    per model, a multiple of 64, or 0 = one model for the whole batch.  The object keeps ONE flight per F16Batch object it has
    flown with -- the prediction xhat [9, B] and the measurement-row counter; the estimate of a fresh flight is the batch's state.
    `row` is the counter of the flight used last; reset() starts every flight again."""

    def __init__(self, models, sensed, sigma, group=0):
        self.models = np.ascontiguousarray(np.asarray(models, dtype=np.float64).reshape(-1, OBS_DOUBLES))
        self.sensed, self.sigma, self.group = check_sensed(sensed), check_sigma(sigma), int(group)
        if self.group < 0 or self.group % 64:
            raise ValueError("group must be 0 (one model for the batch) or a multiple of 64")
        if not self.group and len(self.models) != 1:
            raise ValueError(f"group = 0 takes one model, not {len(self.models)}")
        self._h_sigma = (ctypes.c_double * 9)(*self.sigma)
        self._dev = {}
        self.reset()

    # -- construction
    @staticmethod
    def _model_parts(source, group):
        """(Ad [M, 9, 9], Bd [M, 9, 3], x9_trim [M, 9], s_trim [M, 3]) from an F16Batch (its frozen model ssr and initial condition,
        the first aircraft of every group) or from (Ad, Bd, x_trim, u_trim) arrays ([.., 18] / [.., 9] and [.., 4] / [.., 3])"""
        if isinstance(source, (tuple, list)):
            Ad, Bd, xt, ut = (np.asarray(v, dtype=np.float64) for v in source)
            Ad, Bd = Ad.reshape(-1, 9, 9), Bd.reshape(-1, 9, 3)
            xt, ut = xt.reshape(len(Ad), -1), ut.reshape(len(Ad), -1)
            x9 = xt[:, P.mpc_x_idx] if xt.shape[1] == 18 else xt
            st = ut[:, 1:4] if ut.shape[1] == 4 else ut
            if x9.shape[1] != 9 or st.shape[1] != 3:
                raise ValueError("x_trim must be [.., 18] or [.., 9] and u_trim [.., 4] or [.., 3]")
            return Ad, Bd, x9, st
        env = source
        if env.ssr is None:
            env.build_ssr()
        first = list(range(0, env.B, group)) if group else [0]
        Ad = env.ssr[0][:, first].t().reshape(-1, 9, 9).cpu().numpy()
        Bd = env.ssr[1][:, first].t().reshape(-1, 9, 3).cpu().numpy()
        x0 = env._x_init[:, first].t().cpu().numpy()
        return Ad, Bd, x0[:, P.mpc_x_idx], x0[:, S_IDX]

    @classmethod
    def build(cls, source, w, sigma, sensed=0x7f, group=0, v=None, context=None, return_info=False):
        """The steady-state Kalman observer of the models of `source` (an F16Batch, or (Ad, Bd, x_trim, u_trim)): f16_kalman_batch with
        the diagonal process-noise variances w ([9] or [M, 9], per step) and v = sigma^2 (or the design variances `v`, for a sigma of 0
        on a sensed channel).  Raises F16HipError when a model's doubling does not converge (F16_ST_QP_MAXITER).  return_info: also
        dict(P [M, 9, 9], iters [M], status [M])."""
        import torch
        sensed, sg, group = check_sensed(sensed), check_sigma(sigma), int(group)
        Ad, Bd, x9, st = cls._model_parts(source, group)
        M = len(Ad)
        var = np.broadcast_to(np.asarray(sg * sg if v is None else v, dtype=np.float64), (M, 9))
        if not np.all(var[:, channels(sensed)] > 0):
            raise ValueError("the measurement variances of the sensed channels must be > 0 (sigma = 0: pass the design variances v=)")
        wv = np.broadcast_to(np.asarray(w, dtype=np.float64), (M, 9))
        ctx = context or getattr(source, "ctx", None) or _lib.Context(0)
        dev = torch.device("cuda", ctx.device)
        t = lambda a: torch.as_tensor(np.array(a.reshape(M, -1).T, order="C"), device=dev)
        dAd, dw, dv = t(Ad), t(wv), t(var)
        Lf, Pm = torch.empty((81, M), dtype=torch.float64, device=dev), torch.empty((81, M), dtype=torch.float64, device=dev)
        it, status = torch.zeros(M, dtype=torch.int32, device=dev), torch.zeros(M, dtype=torch.int32, device=dev)
        vp = lambda x: ctypes.c_void_p(x.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(ctx.lib.f16_kalman_batch(ctx.handle, vp(dAd), vp(dw), vp(dv), sensed, vp(Lf), vp(Pm), vp(it), vp(status), M, M, stream), ctx.lib)
        status = status.cpu().numpy()
        if status.any():
            raise _lib.F16HipError(f"f16_kalman_batch: the doubling of model(s) {np.nonzero(status)[0].tolist()} did not converge (is the pair detectable?)")
        obs = cls(pack_models(Ad, Bd, Lf.t().cpu().numpy(), x9, st), sensed, sg, group)
        if return_info:
            return obs, dict(P=Pm.t().reshape(M, 9, 9).cpu().numpy(), iters=it.cpu().numpy(), status=status)
        return obs

    @classmethod
    def passthrough(cls, source, sigma, sensed=0x7f, group=0):
        """Lf = I on the sensed channels: the corrected estimate IS the measurement there (raw noisy feedback), the model carries the
        rest.  No GPU call."""
        Ad, Bd, x9, st = cls._model_parts(source, int(group))
        Lf = np.diag([1.0 if (check_sensed(sensed) >> k) & 1 else 0.0 for k in range(9)])
        return cls(pack_models(Ad, Bd, np.broadcast_to(Lf, (len(Ad), 9, 9)), x9, st), sensed, sigma, group)

    # -- the flight
    def reset(self):
        import weakref
        self._flights, self._last = weakref.WeakKeyDictionary(), None      # {the F16Batch: [xhat [9, B], row]}; the flight used last

    @property
    def row(self):
        return self._last[1] if self._last is not None else 0

    @property
    def estimate(self):
        """the prediction [9, B] of the flight used last (a device tensor), or None"""
        return self._last[0] if self._last is not None else None

    def device_models(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.as_tensor(self.models, device=device)
        return self._dev[key]

    def flight(self, env):
        """(models [M, 208], xhat [9, B]) on the device for the batch `env`: that batch's flight, which `row` and advance() refer to
        until another batch asks.  A flight belongs to the F16Batch OBJECT (a second batch of the same size starts its own) and a
        fresh one starts from the batch's current state."""
        B = env.B
        need = (B + self.group - 1) // self.group if self.group else 1
        if len(self.models) < need:
            raise ValueError(f"{B} aircraft in groups of {self.group} need {need} models; the observer has {len(self.models)}")
        if env not in self._flights:
            self._flights[env] = [env._x[P.mpc_x_idx].clone().contiguous(), 0]
        self._last = self._flights[env]
        return self.device_models(env.device), self._last[0]

    def set_estimate(self, env, xhat):
        """the prediction of the batch's flight: xhat [B, 9]"""
        self.flight(env)[1].copy_(env._soa(xhat, 9))

    def advance(self, nsteps):
        self._last[1] = (self._last[1] + int(nsteps)) & 0xffffffff

    @property
    def h_sigma(self):
        return ctypes.c_void_p(ctypes.addressof(self._h_sigma))
