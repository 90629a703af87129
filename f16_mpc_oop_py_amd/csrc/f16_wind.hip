// f16_wind.hip -- the plant in steady wind and sampled gusts (rule: f16_wind.hpp; contracts: include/f16_hip.h) + the C-ABI launchers.
//
//   k_xdot_wind           one derivative of B aircraft in moving air                         (f16_xdot_wind_batch)
//   k_rollout_wind        f16_rollout_rk / f16_rollout_lqr_rk in moving air, Euler or Runge-Kutta step, state in registers
//                         (f16_rollout_wind, f16_rollout_lqr_wind)
//   k_rollout_wind_exact  the same through the out-of-line wind_step_exact: one kernel for every batch size (F16_FLAG_ONE_LANE)
//   k_gust_sample         the Gauss-Markov gust rows of B aircraft                           (f16_gust_sample)
//
// Mapping: one lane = one aircraft, 64 / 128 / 256 lanes per workgroup (the launch geometry of the Runge-Kutta rollouts: one wave per
// SIMD at most), the fp64 table image staged in LDS for hifi.  What is constant over a launch or changes only at a row boundary --
// the four commands, under the LQR law K[i][4..6] and the demands, the three wind components and the gust row in use -- sits in
// lane-indexed (conflict-free) LDS slots and is read where a step needs it: 157,984 B of static LDS at 256 lanes under the LQR law.
// Every step evaluates its sin / cos pairs exactly, so nothing but the state and the gust row is carried from step to step.
#include <hip/hip_runtime.h>

#include "../../include/f16_hip.h"
#include "f16_ctx.h"
#include "f16_plant.hpp"
#include "f16_rollout_common.hpp"
#include "f16_wind.hpp"
#include "f16_wind_lanes.hpp"

namespace f16 {

struct XdotWindArgs : DynArgs {
  const double *wind, *gust;   // [3][ld] each, or null (= 0)
};

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_xdot_wind(XdotWindArgs a) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  if (a.fi == 1) stage_tables(tab, a.tab);
  for (long b = (long)blockIdx.x * BLOCK + threadIdx.x; b < a.B; b += (long)gridDim.x * BLOCK) {
    double x[18], u[4], w[6], xd[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) x[k] = a.x[k * a.ld + b];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = a.u[k * a.ld + b];
#pragma unroll
    for (int k = 0; k < 3; ++k) { w[k] = a.wind ? a.wind[k * a.ld + b] : 0.0; w[3 + k] = a.gust ? a.gust[k * a.ld + b] : 0.0; }
    int st = 0;
    calc_xdot_wind<-1>((const double *)tab, a.lofi, x, u, [&](int k) { return w[k]; }, xd, a.xcg, a.fi, a.flags, st);
#pragma unroll
    for (int k = 0; k < 18; ++k) a.out[k * a.ld + b] = xd[k];
    if (a.status) a.status[b] |= st;
  }
}

// The rollout kernels: the lane loop is wind_lanes of f16_wind_lanes.hpp, shared with the ensemble twins of f16_wind_ens.hip.
template <int BLOCK, bool LQR, int STAGES>
__global__ __launch_bounds__(BLOCK) void k_rollout_wind(WindArgs a) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  __shared__ double us[4][BLOCK];
  __shared__ double kq[LQR ? 12 : 1][LQR ? BLOCK : 1];
  __shared__ double ws[6][BLOCK];
  static_assert(BLOCK <= 256 && sizeof(tab) + sizeof(us) + sizeof(kq) + sizeof(ws) <= 163840, "static LDS of a CU");
  if (a.fi == 1) stage_tables(tab, a.tab);
  wind_lanes<BLOCK, LQR, STAGES, false>(a, (const double *)tab, us, reinterpret_cast<double (*)[BLOCK]>(kq), ws);
}

// F16_FLAG_ONE_LANE: 64-lane workgroups at every batch size, the table image read from global memory
template <bool LQR, int STAGES>
__global__ __launch_bounds__(64) void k_rollout_wind_exact(WindArgs a) {
  __shared__ double us[4][64];
  __shared__ double kq[LQR ? 12 : 1][LQR ? 64 : 1];
  __shared__ double ws[6][64];
  wind_lanes<64, LQR, STAGES, true>(a, a.tab, us, reinterpret_cast<double (*)[64]>(kq), ws);
}

struct GustArgs {
  const double *ga, *gb;   // [3][ld]
  double *gstate, *gseq;   // [3][ld]; [nrows][3][ld]
  uint32_t key0, key1, row0;
  long B, ld;
  int nrows;
};

// one lane = one aircraft; the rows of an aircraft are a recurrence, so a lane walks them in order
__global__ __launch_bounds__(64) void k_gust_sample(GustArgs a) {
  for (long b = (long)blockIdx.x * 64 + threadIdx.x; b < a.B; b += (long)gridDim.x * 64) {
    double c[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) { c[k] = a.ga[k * a.ld + b]; c[3 + k] = a.gb[k * a.ld + b]; }
    Gust3 g{{a.gstate[b], a.gstate[a.ld + b], a.gstate[2 * a.ld + b]}};
    for (int r = 0; r < a.nrows; ++r) {
      g = gust_row(a.row0 + (uint32_t)r, (uint32_t)b, a.key0, a.key1, c[0], c[1], c[2], c[3], c[4], c[5], g.v[0], g.v[1], g.v[2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) a.gseq[((long)r * 3 + k) * a.ld + b] = g.v[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) a.gstate[k * a.ld + b] = g.v[k];
  }
}

static bool still_air(const f16_wind *w) { return !w || (!w->wind_ned && !w->gust_seq && !w->ga && !w->gb && !w->gstate); }

// The kernel family of the plain calls (f16_wind_lanes.hpp: wind_rollout): the kernels take the argument block alone.
template <bool L>
struct WindKernels {
  static constexpr bool LQR = L, ENS = false, OBS = false;
  static constexpr const char *what = "f16_rollout_wind launch";
  template <int BLOCK, int STAGES>
  static void launch(dim3 grid, hipStream_t st, const WindArgs &a, const WindRollout &) {
    hipLaunchKernelGGL((k_rollout_wind<BLOCK, L, STAGES>), grid, dim3(BLOCK), 0, st, a);
  }
  template <int STAGES>
  static void launch_exact(dim3 grid, hipStream_t st, const WindArgs &a, const WindRollout &) {
    hipLaunchKernelGGL((k_rollout_wind_exact<L, STAGES>), grid, dim3(64), 0, st, a);
  }
};

}  // namespace f16

using namespace f16;

extern "C" int f16_xdot_wind_batch(f16_ctx *ctx, const double *x, const double *u, const double *wind, const double *gust, double *xdot,
                                   int32_t *status, long B, long ld, double xcg, int fi_flag, unsigned flags, void *stream) {
  if (!wind && !gust) return f16_xdot_batch(ctx, x, u, xdot, status, B, ld, xcg, fi_flag, flags, stream);
  if (int rc = check_common(ctx, x, xdot, B, ld)) return rc;
  if (!u) return set_error(F16_EINVAL, "u is NULL");
  if (B == 0) return F16_OK;
  XdotWindArgs a = base_args<XdotWindArgs>(ctx, B, ld, xcg, fi_flag, flags, status);
  a.x = x; a.u = u; a.out = xdot; a.wind = wind; a.gust = gust;
  const Geometry g = geometry(B, fi_flag, 256);
  by_block(g, [&](auto block) {
    constexpr int BLOCK = decltype(block)::value;
    if constexpr (BLOCK <= 256) hipLaunchKernelGGL((k_xdot_wind<BLOCK>), dim3(g.grid), dim3(BLOCK), 0, (hipStream_t)stream, a);
  });
  return hip_check(hipGetLastError(), "f16_xdot_wind_batch launch");
}

extern "C" int f16_rollout_wind(f16_ctx *ctx, double *x, const double *u_seq, const f16_wind *h_wind, double *traj, int32_t *status, long B,
                                long ld, int nsteps, int hold, int traj_every, double dt, double xcg, int fi_flag, int method,
                                unsigned flags, void *stream) {
  if (still_air(h_wind)) return f16_rollout_rk(ctx, x, u_seq, traj, status, B, ld, nsteps, hold, traj_every, dt, xcg, fi_flag, method, flags, stream);
  WindRollout d{"u_seq is NULL", x, u_seq, u_seq, h_wind, traj, status, B, ld, nsteps, hold, traj_every, dt, xcg, fi_flag, method, flags};
  return wind_rollout<WindKernels<false>>(ctx, d, stream);
}

extern "C" int f16_rollout_lqr_wind(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem_seq, const f16_wind *h_wind,
                                    double *traj, double *u_out, int32_t *status, long B, long ld, int nsteps, int hold, int traj_every,
                                    double dt, double xcg, int fi_flag, int method, unsigned flags, void *stream) {
  if (still_air(h_wind))
    return f16_rollout_lqr_rk(ctx, x, u0, K, dem_seq, traj, u_out, status, B, ld, nsteps, hold, traj_every, dt, xcg, fi_flag, method, flags, stream);
  WindRollout d{"K / dem_seq is NULL", x, u0, dem_seq, h_wind, traj, status, B, ld, nsteps, hold, traj_every, dt, xcg, fi_flag, method, flags};
  d.K = K; d.u_out = u_out;
  return wind_rollout<WindKernels<true>>(ctx, d, stream);
}

extern "C" int f16_gust_coeffs_host(const double *sigma, const double *length, double v0, double dt_row, double *a_out, double *b_out) {
  if (!sigma || !length || !a_out || !b_out) return set_error(F16_EINVAL, "sigma / length / a_out / b_out is NULL");
  if (!(v0 > 0.0) || !__builtin_isfinite(v0) || !(dt_row > 0.0) || !__builtin_isfinite(dt_row))
    return set_error(F16_EINVAL, "v0 and dt_row must be finite and > 0");
  for (int i = 0; i < 3; ++i)
    if (!(sigma[i] >= 0.0) || !__builtin_isfinite(sigma[i]) || !(length[i] > 0.0) || !__builtin_isfinite(length[i]))
      return set_error(F16_EINVAL, "sigma must be finite and >= 0, length finite and > 0");
  for (int i = 0; i < 3; ++i) {
    const double a = exp(-(v0 * dt_row) / length[i]);
    a_out[i] = a;
    b_out[i] = sigma[i] * sqrt(1.0 - a * a);
  }
  return F16_OK;
}

extern "C" int f16_gust_sample(f16_ctx *ctx, const double *ga, const double *gb, double *gstate, uint64_t seed, uint32_t row0, double *g_seq,
                               int nrows, long B, long ld, void *stream) {
  if (!ctx || !ga || !gb || !gstate || !g_seq) return set_error(F16_EINVAL, "ctx / ga / gb / gstate / g_seq is NULL");
  if (B < 0 || ld < B || nrows < 0) return set_error(F16_EINVAL, "bad argument (B < 0, ld < B or nrows < 0)");
  if (B == 0 || nrows == 0) return F16_OK;
  GustArgs a{};
  a.ga = ga; a.gb = gb; a.gstate = gstate; a.gseq = g_seq;
  a.key0 = (uint32_t)(seed & 0xffffffffu); a.key1 = (uint32_t)(seed >> 32); a.row0 = row0;
  a.B = B; a.ld = ld; a.nrows = nrows;
  hipLaunchKernelGGL(k_gust_sample, one_lane_grid(B), dim3(64), 0, (hipStream_t)stream, a);
  return hip_check(hipGetLastError(), "f16_gust_sample launch");
}
