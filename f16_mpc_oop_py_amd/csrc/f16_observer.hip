// f16_observer.hip -- LQR loops on noisy sensors through a steady-state Kalman observer (rule and contracts: include/f16_hip.h
// "OUTPUT FEEDBACK"; the per-step rule: f16_observer.hpp) + the C-ABI launchers.
//
//   k_kalman                     the filter Riccati equation by the doubling of dare_sda_wave and the gain Lf       (f16_kalman_batch)
//   k_observer_step              measurement, correction, LQR law on the estimate, prediction for B aircraft       (f16_observer_step)
//   k_rollout_lqg_wind           k_rollout_wind / k_rollout_wind_ens under the LQR law with the OBS lane loop      (f16_rollout_lqg_wind,
//   k_rollout_lqg_wind_exact     the same for k_rollout_wind_exact / _exact_ens (F16_FLAG_ONE_LANE)                 f16_rollout_lqg_wind_ens)
//
// A translation unit of its own: the kernels of f16_wind.hip, f16_wind_ens.hip and f16_control.hip keep their code.
#include <hip/hip_runtime.h>

#include "../../include/f16_hip.h"
#include "f16_ctx.h"
#include "f16_ensemble.hpp"
#include "f16_mpc_model.hpp"
#include "f16_observer.hpp"
#include "f16_wind_lanes.hpp"

namespace f16 {

// ------------------------------------------------------------------------------------ the filter gain
// The doubling of dare_sda_wave (f16_mpc_model.hpp) from given tiles: A, At = A' and the symmetric G, H in the accumulator layout;
// H becomes the solution.  A second function, operation for operation the loop of the first, so that k_lqr, k_rollout_lqr_relin and
// the MPC kernels keep their instruction streams.  The filter equation P = Ad P Ad' - Ad P C'(C P C' + V)^-1 C P Ad' + W is the
// control equation with A <- Ad', G <- C'V^-1 C, H <- W.  Returns the doublings used; 60: not converged, or not finite.
// One difference: every inverse is the elimination with partial pivoting.  The first function tries the natural order and accepts a
// residual below 2e-9, which is what its callers' gains need; a filter covariance is compared at 1e-13, where that residual shows
// (measured: 1.8e-13 against 7e-15 of the numpy restatement on one of 66 models), and this kernel runs once per design.
// The other: G and H are made symmetric after every doubling (see there).
// T <- (T + T') / 2 through LDS (scr: 81 doubles)
__device__ __forceinline__ void symmetric9_tile(d4_t &T, double *scr) {
  const int l = lane_id(), lc = l & 15, lq = l >> 4;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int r = 4 * q + lq;
    if (r < 9 && lc < 9) scr[r * 9 + lc] = T[q];
  }
  __syncthreads();
  const d4_t Tt = tile9(scr, true);
#pragma unroll
  for (int q = 0; q < 3; ++q) T[q] = 0.5 * (T[q] + Tt[q]);
  __syncthreads();
}

__device__ __forceinline__ int dare_sda_tiles(d4_t A, d4_t At, d4_t G, d4_t &H, double *scr) {
  const int l = lane_id(), lc = l & 15, lq = l >> 4;
  const d4_t zero = {0.0, 0.0, 0.0, 0.0};
  d4_t eye = zero;
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (4 * q + lq == lc && lc < 9) eye[q] = 1.0;
  int it = 0;
  for (; it < 60; ++it) {
    const d4_t M = mm16(G, H, eye);                  // I + G H
    const d4_t GAt = mm16(G, At, zero);              // G A'
    d4_t W;
    if (!inverse9_tile<true>(M, W, scr)) { it = 60; break; }
    const d4_t T1t = mm16(W, At, zero);              // (A W)'
    const d4_t HWt = mm16(W, H, zero);               // (H W)'
    const d4_t An = mm16(T1t, A, zero);              // A W A
    const d4_t Atn = mm16(A, T1t, zero);             // (A W A)'
    G = mm16(T1t, GAt, G);                           // G + A W G A'
    const d4_t HWA = mm16(HWt, A, zero);             // H W A
    const d4_t dH = mm16(A, HWA, zero);              // A' H W A
    double dmax = 0.0, hmax = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      H[q] += dH[q];
      dmax = fmax(dmax, fabs(dH[q]));
      hmax = fmax(hmax, fabs(H[q]));
    }
    dmax = wave_max(dmax);
    hmax = wave_max(hmax);
    A = An; At = Atn;
    // The products above take the tile of G for the tile of G' and the tile of H for that of H': exact only while both ARE
    // symmetric.  Rounding leaves them so to one ulp, and at cond(I + G H) = 1e10 (an unstable model seen through few sensors)
    // that ulp came back as 3e-9 in the solution, against 3e-11 of the numpy restatement.  Both are made symmetric here.
    symmetric9_tile(G, scr);
    symmetric9_tile(H, scr);
    if (dmax <= 1e-16 * hmax) { ++it; break; }
  }
  if (__any(!(isfinite(H[0]) && isfinite(H[1]) && isfinite(H[2])))) it = 60;
  return it;
}

struct KalmanArgs {
  const double *Ad, *w, *v;    // [81][ld], [9][ld], [9][ld]
  double *Lf, *Pm;             // [81][ld]; Pm may be null
  int32_t *iters, *status;     // [M]; iters may be null
  long M, ld;
  int sensed;
};

// one wavefront per model
__global__ __launch_bounds__(64) void k_kalman(KalmanArgs a) {
  __shared__ double smem[82 * 2 + 10 * 2 + DARE_SCRATCH + 2];
  Bump al{smem};
  double *Ad = al.take(81), *X = al.take(81), *wv = al.take(9), *gv = al.take(9), *scr = al.take(DARE_SCRATCH);
  const int l = lane_id(), lc = l & 15, lq = l >> 4;
  const d4_t zero = {0.0, 0.0, 0.0, 0.0};
  for (long m = blockIdx.x; m < a.M; m += gridDim.x) {
    for (int e = l; e < 81; e += F16_WAVE) Ad[e] = a.Ad[e * a.ld + m];
    if (l < 9) {
      wv[l] = a.w[l * a.ld + m];
      gv[l] = ((a.sensed >> l) & 1) ? 1.0 / a.v[l * a.ld + m] : 0.0;      // the diagonal of C'V^-1 C
    }
    __syncthreads();
    d4_t G = zero, H = zero, eye = zero;
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (4 * q + lq == lc && lc < 9) { G[q] = gv[lc]; H[q] = wv[lc]; eye[q] = 1.0; }
    int it = dare_sda_tiles(tile9(Ad, true), tile9(Ad, false), G, H, scr);
    // P = (H + H') / 2 through LDS, as dare_sda_wave leaves its solution
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int r = 4 * q + lq;
      if (r < 9 && lc < 9) scr[r * 9 + lc] = H[q];
    }
    __syncthreads();
    for (int e = l; e < 81; e += F16_WAVE) {
      const int i = e / 9, j = e - i * 9;
      X[e] = 0.5 * (scr[e] + scr[j * 9 + i]);
    }
    __syncthreads();
    // Lf = P (I + G P)^-1 C'V^-1: in the 9 x 9 frame C'V^-1 is G itself, whose columns of unsensed channels are zero
    const d4_t P = tile9(X, false);
    const d4_t M1 = mm16(G, P, eye);                 // I + G P   (G symmetric: its own transpose)
    d4_t W;
    if (!inverse9_tile<true>(M1, W, scr)) it = 60;
    const d4_t PWt = mm16(W, P, zero);               // (P W)' = W' P
    const d4_t L = mm16(PWt, G, zero);               // P W G
    if (__any(!(isfinite(L[0]) && isfinite(L[1]) && isfinite(L[2])))) it = 60;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int r = 4 * q + lq;
      if (r < 9 && lc < 9) a.Lf[(r * 9 + lc) * a.ld + m] = ((a.sensed >> lc) & 1) ? L[q] : 0.0;
    }
    if (a.Pm) { for (int e = l; e < 81; e += F16_WAVE) a.Pm[e * a.ld + m] = X[e]; }
    if (l == 0) {
      if (a.iters) a.iters[m] = it;
      if (it >= 60) a.status[m] |= F16_ST_QP_MAXITER;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ one observer step of a batch
struct ObsStepArgs {
  const double *x, *u0, *K, *dem;      // [18][ld], [4][ld], [27][ld], [3][ld]
  const int32_t *status;               // [B] or null: read only
  double *u_cmd;                       // [4][ld]
  long B, ld;
  unsigned flags;
};

__global__ __launch_bounds__(64) void k_observer_step(ObsStepArgs a, ObsArgs oa) {
  __shared__ double us[4][64];
  __shared__ double kq[12][64];
  __shared__ ObsArgs o;
  if (threadIdx.x == 0) { o = oa; o.kq = &kq[0][0]; o.us = &us[0][0]; o.stride = 64; }
  __syncthreads();
  for (long b = (long)blockIdx.x * 64 + threadIdx.x; b < a.B; b += (long)gridDim.x * 64) {
    double x[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) x[k] = a.x[k * a.ld + b];
    const int st = a.status ? a.status[b] : 0;
    if ((st & ST_ENVELOPE) || (!(a.flags & FLAG_NO_ENVELOPE) && outside_envelope(x))) continue;      // frozen: nothing is touched
#pragma unroll
    for (int k = 0; k < 4; ++k) us[k][threadIdx.x] = a.u0[k * a.ld + b];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) kq[3 * i + j][threadIdx.x] = a.K[(9 * i + 4 + j) * a.ld + b];
#pragma unroll
    for (int j = 0; j < 3; ++j) kq[9 + j][threadIdx.x] = a.dem[j * a.ld + b];
    const Obs3 c = observer_update(&o, b, o.mrow0, x[3], x[4], x[7], x[8], x[9], x[10], x[11], x[17], x[16], x[13], x[14], x[15]);
    a.u_cmd[b] = us[0][threadIdx.x];               // the thrust command is held
#pragma unroll
    for (int i = 0; i < 3; ++i) a.u_cmd[(1 + i) * a.ld + b] = c.v[i];
  }
}

// ------------------------------------------------------------------------------------ the rollouts
template <int BLOCK, int STAGES, bool ENS>
__global__ __launch_bounds__(BLOCK) void k_rollout_lqg_wind(WindArgs a, ObsArgs oa, double *ework) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  __shared__ double us[4][BLOCK];
  __shared__ double kq[12][BLOCK];
  __shared__ double ws[6][BLOCK];
  __shared__ ObsArgs o;
  static_assert(BLOCK <= 256 && sizeof(tab) + sizeof(us) + sizeof(kq) + sizeof(ws) + sizeof(ObsArgs) <= 163840, "static LDS of a CU");
  if (threadIdx.x == 0) { o = oa; o.kq = &kq[0][0]; o.us = &us[0][0]; o.stride = BLOCK; }
  if (a.fi == 1) stage_tables(tab, a.tab);
  else __syncthreads();
  wind_lanes<BLOCK, true, STAGES, false, ENS, true>(a, (const double *)tab, us, kq, ws, ework, &o);
}

template <int STAGES, bool ENS>
__global__ __launch_bounds__(64) void k_rollout_lqg_wind_exact(WindArgs a, ObsArgs oa, double *ework) {
  __shared__ double us[4][64];
  __shared__ double kq[12][64];
  __shared__ double ws[6][64];
  __shared__ ObsArgs o;
  if (threadIdx.x == 0) { o = oa; o.kq = &kq[0][0]; o.us = &us[0][0]; o.stride = 64; }
  __syncthreads();
  wind_lanes<64, true, STAGES, true, ENS, true>(a, a.tab, us, kq, ws, ework, &o);
}

// What an entry point states of the observer (WindRollout::obs; f16_observer_step: its own)
struct ObsInputs {
  const double *obs; long mgroup; int sensed; const double *h_sigma;      // (the entry points' order)
  uint64_t meas_seed; uint32_t mrow0; double *xhat;
};

// the observer's rules, behind the sibling's: the pointers, the grouping, the sensors
static int check_observer(const ObsInputs &i) {
  if (!i.obs || !i.h_sigma || !i.xhat) return set_error(F16_EINVAL, "obs / h_sigma / xhat is NULL");
  if (i.mgroup < 0 || i.mgroup % 64 != 0) return set_error(F16_EINVAL, "mgroup must be 0 (one model) or a multiple of 64");
  if (i.sensed < 1 || i.sensed > 0x1ff) return set_error(F16_EINVAL, "sensed must be a mask of the nine channels, 1 .. 0x1ff");
  for (int k = 0; k < 9; ++k)
    if (!(i.h_sigma[k] >= 0.0) || !__builtin_isfinite(i.h_sigma[k])) return set_error(F16_EINVAL, "a sigma is negative or not finite");
  return F16_OK;
}

static ObsArgs observer_args(const ObsInputs &i, double *y_out, double *xhat_traj, long ld) {
  ObsArgs o{};
  o.obs = i.obs; o.xhat = i.xhat; o.y_out = y_out; o.xhat_traj = xhat_traj;
  o.mgroup = i.mgroup; o.ld = ld;
  o.key0 = (uint32_t)(i.meas_seed & 0xffffffffu); o.key1 = (uint32_t)(i.meas_seed >> 32); o.mrow0 = i.mrow0;
  o.sensed = i.sensed;
  for (int k = 0; k < 9; ++k) o.sigma[k] = i.h_sigma[k];
  return o;
}

// The kernel family of the output-feedback calls (f16_wind_lanes.hpp: wind_rollout): the kernels take the observer's block and the
// ensemble's workspace (null without one) behind the argument block.
template <bool E>
struct LqgKernels {
  static constexpr bool LQR = true, ENS = E, OBS = true;
  static constexpr const char *what = "f16_rollout_lqg_wind launch", *what_finish = "f16_rollout_lqg_wind_ens finishing launch";
  static int rules(const WindRollout &d) { return check_observer(*d.obs); }
  static double *work(const WindRollout &d) { return E ? d.ens->work : nullptr; }
  template <int BLOCK, int STAGES>
  static void launch(dim3 grid, hipStream_t st, const WindArgs &a, const WindRollout &d) {
    hipLaunchKernelGGL((k_rollout_lqg_wind<BLOCK, STAGES, E>), grid, dim3(BLOCK), 0, st, a, observer_args(*d.obs, nullptr, d.xhat_traj, d.ld), work(d));
  }
  template <int STAGES>
  static void launch_exact(dim3 grid, hipStream_t st, const WindArgs &a, const WindRollout &d) {
    hipLaunchKernelGGL((k_rollout_lqg_wind_exact<STAGES, E>), grid, dim3(64), 0, st, a, observer_args(*d.obs, nullptr, d.xhat_traj, d.ld), work(d));
  }
};

}  // namespace f16

using namespace f16;

extern "C" int f16_kalman_batch(f16_ctx *ctx, const double *Ad, const double *w, const double *v, int sensed, double *Lf, double *Pm,
                                int32_t *iters, int32_t *status, long M, long ld, void *stream) {
  if (!ctx || !Ad || !w || !v || !Lf || !status || M < 0 || ld < M)
    return set_error(F16_EINVAL, "bad argument to f16_kalman_batch (NULL pointer, M < 0 or ld < M)");
  if (sensed < 1 || sensed > 0x1ff) return set_error(F16_EINVAL, "sensed must be a mask of the nine channels, 1 .. 0x1ff");
  if (M == 0) return F16_OK;
  KalmanArgs a{Ad, w, v, Lf, Pm, iters, status, M, ld, sensed};
  hipLaunchKernelGGL(k_kalman, dim3((unsigned)(M < 256L * 32 ? M : 256L * 32)), dim3(64), 0, (hipStream_t)stream, a);
  return hip_check(hipGetLastError(), "f16_kalman_batch launch");
}

extern "C" int f16_observer_step(f16_ctx *ctx, const double *x, const int32_t *status, const double *u0, const double *K, const double *dem,
                                 const double *obs, long mgroup, int sensed, const double *h_sigma, uint64_t meas_seed, uint32_t mrow,
                                 double *xhat, double *y_out, double *u_cmd, long B, long ld, unsigned flags, void *stream) {
  if (int rc = check_common(ctx, x, u0, B, ld)) return rc;
  if (!K || !dem || !u_cmd) return set_error(F16_EINVAL, "K / dem / u_cmd is NULL");
  const ObsInputs in{obs, mgroup, sensed, h_sigma, meas_seed, mrow, xhat};
  if (int rc = check_observer(in)) return rc;
  if (B == 0) return F16_OK;
  ObsStepArgs a{x, u0, K, dem, status, u_cmd, B, ld, flags};
  hipLaunchKernelGGL(k_observer_step, one_lane_grid(B), dim3(64), 0, (hipStream_t)stream, a, observer_args(in, y_out, nullptr, ld));
  return hip_check(hipGetLastError(), "f16_observer_step launch");
}

extern "C" int f16_rollout_lqg_wind(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem_seq, const f16_wind *h_wind,
                                    const double *obs, long mgroup, int sensed, const double *h_sigma, uint64_t meas_seed, uint32_t mrow0,
                                    double *xhat, double *traj, double *xhat_traj, double *u_out, int32_t *status, long B, long ld,
                                    int nsteps, int hold, int traj_every, double dt, double xcg, int fi_flag, int method, unsigned flags,
                                    void *stream) {
  const ObsInputs in{obs, mgroup, sensed, h_sigma, meas_seed, mrow0, xhat};
  WindRollout d{"K / dem_seq is NULL", x, u0, dem_seq, h_wind, traj, status, B, ld, nsteps, hold, traj_every, dt, xcg, fi_flag, method, flags};
  d.K = K; d.u_out = u_out; d.obs = &in; d.xhat_traj = xhat_traj;
  return wind_rollout<LqgKernels<false>>(ctx, d, stream);
}

extern "C" int f16_rollout_lqg_wind_ens(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem_seq,
                                        const f16_wind *h_wind, const double *obs, long mgroup, int sensed, const double *h_sigma,
                                        uint64_t meas_seed, uint32_t mrow0, double *xhat, double *traj, double *xhat_traj,
                                        const f16_ens *h_ens, double *u_out, int32_t *status, long B, long ld, int nsteps, int hold,
                                        int traj_every, double dt, double xcg, int fi_flag, int method, unsigned flags, void *stream) {
  const ObsInputs in{obs, mgroup, sensed, h_sigma, meas_seed, mrow0, xhat};
  WindRollout d{"K / dem_seq is NULL", x, u0, dem_seq, h_wind, traj, status, B, ld, nsteps, hold, traj_every, dt, xcg, fi_flag, method, flags};
  d.K = K; d.u_out = u_out; d.ens = h_ens; d.obs = &in; d.xhat_traj = xhat_traj;
  return wind_rollout<LqgKernels<true>>(ctx, d, stream);
}
