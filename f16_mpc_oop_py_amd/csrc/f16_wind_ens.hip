// f16_wind_ens.hip -- ensemble statistics of wind and gust rollouts inside the launch (rule and contracts: include/f16_hip.h
// "ENSEMBLE STATISTICS"; device functions: f16_ensemble.hpp) + the C-ABI launchers.
//
//   k_rollout_wind_ens        k_rollout_wind with the ENS lane loop: at every sample point each wavefront writes its records of the
//   k_rollout_wind_exact_ens  sample into the caller's workspace; the same for k_rollout_wind_exact (F16_FLAG_ONE_LANE)
//   k_ens_from_traj           the same records from a stored [S][18][ld] trajectory: one wavefront per (sample, 64 aircraft)
//   k_ens_finish              one lane per (sample, row, group): the group's wave records folded in ascending aircraft order
//
// A translation unit of its own: the kernels of f16_wind.hip keep their code, the lane loop is the one of f16_wind_lanes.hpp.
#include <hip/hip_runtime.h>

#include "../../include/f16_hip.h"
#include "f16_ctx.h"
#include "f16_ensemble.hpp"
#include "f16_wind_lanes.hpp"

namespace f16 {

template <int BLOCK, bool LQR, int STAGES>
__global__ __launch_bounds__(BLOCK) void k_rollout_wind_ens(WindArgs a, double *ework) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  __shared__ double us[4][BLOCK];
  __shared__ double kq[LQR ? 12 : 1][LQR ? BLOCK : 1];
  __shared__ double ws[6][BLOCK];
  static_assert(BLOCK <= 256 && sizeof(tab) + sizeof(us) + sizeof(kq) + sizeof(ws) <= 163840, "static LDS of a CU");
  if (a.fi == 1) stage_tables(tab, a.tab);
  wind_lanes<BLOCK, LQR, STAGES, false, true>(a, (const double *)tab, us, reinterpret_cast<double (*)[BLOCK]>(kq), ws, ework);
}

template <bool LQR, int STAGES>
__global__ __launch_bounds__(64) void k_rollout_wind_exact_ens(WindArgs a, double *ework) {
  __shared__ double us[4][64];
  __shared__ double kq[LQR ? 12 : 1][LQR ? 64 : 1];
  __shared__ double ws[6][64];
  wind_lanes<64, LQR, STAGES, true, true>(a, a.tab, us, reinterpret_cast<double (*)[64]>(kq), ws, ework);
}

struct EnsArgs {
  const double *traj;          // k_ens_from_traj: [S][18][ld]
  double *work;                // [S][W][ENS_REC]
  int32_t *count;              // [S][ldg]
  double *mean, *m2, *mn, *mx; // [S][18][ldg]
  long B, ld, W, G, ldg;       // W = ceil(B / 64) waves, G = ceil(B / group) groups
  int S, wpg;                  // samples; waves per group
  unsigned flags;
};

// one wavefront per (sample, wave of aircraft), grid-stride; every lane stays (a lane without an aircraft reads aircraft B - 1)
__global__ __launch_bounds__(64) void k_ens_from_traj(EnsArgs a) {
  const long items = (long)a.S * a.W;
  for (long i = blockIdx.x; i < items; i += gridDim.x) {
    const long s = i / a.W, w = i - s * a.W;
    const long b0 = w * 64 + threadIdx.x;
    const bool live = b0 < a.B;
    const double *col = a.traj + s * 18 * a.ld + (live ? b0 : a.B - 1);
    double x[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) x[k] = col[k * a.ld];
    ens_wave_records(x, live, a.flags, a.work + i * ENS_REC);
  }
}

__global__ __launch_bounds__(64) void k_ens_finish(EnsArgs a) {
  const long items = (long)a.S * 18 * a.G;
  for (long i = (long)blockIdx.x * 64 + threadIdx.x; i < items; i += (long)gridDim.x * 64) {
    const long g = i % a.G, sk = i / a.G;
    const long s = sk / 18;
    const int k = (int)(sk - s * 18);
    const long w0 = g * a.wpg;
    const int nw = (int)(a.W - w0 < a.wpg ? a.W - w0 : a.wpg);
    const EnsGroup r = ens_fold_group(a.work + (s * a.W + w0) * ENS_REC, nw, k);
    const long at = sk * a.ldg + g;
    a.mean[at] = r.mean; a.m2[at] = r.m2; a.mn[at] = r.mn; a.mx[at] = r.mx;
    if (k == 0) a.count[s * a.ldg + g] = r.n;
  }
}

// the rules of an f16_ens behind the sibling's: every member, the group size, the leading dimension of the results
static int check_ens(const f16_ens *e, long B) {
  if (!e || !e->work || !e->count || !e->mean || !e->m2 || !e->min || !e->max)
    return set_error(F16_EINVAL, "h_ens or one of its members is NULL");
  if (e->group < 64 || e->group % 64 != 0) return set_error(F16_EINVAL, "group must be a multiple of 64 and >= 64");
  if (e->ldg < (B + e->group - 1) / e->group) return set_error(F16_EINVAL, "ldg < G = ceil(B / group)");
  return F16_OK;
}

static EnsArgs ens_args(const f16_ens *e, long B, int S, unsigned flags) {
  EnsArgs a{};
  a.work = e->work; a.count = e->count; a.mean = e->mean; a.m2 = e->m2; a.mn = e->min; a.mx = e->max;
  a.B = B; a.W = (B + 63) / 64; a.G = (B + e->group - 1) / e->group; a.ldg = e->ldg;
  a.S = S; a.wpg = (int)(e->group / 64 < a.W ? e->group / 64 : a.W); a.flags = flags;
  return a;
}

static int ens_finish(const EnsArgs &a, hipStream_t st, const char *what) {
  const long blocks = ((long)a.S * 18 * a.G + 63) / 64;
  hipLaunchKernelGGL(k_ens_finish, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(64), 0, st, a);
  return hip_check(hipGetLastError(), what);
}

int ens_rules(const f16_ens *e, long B) { return check_ens(e, B); }
int ens_finish_launch(const f16_ens *e, long B, int S, unsigned flags, void *stream, const char *what) {
  return ens_finish(ens_args(e, B, S, flags), (hipStream_t)stream, what);
}

template <bool LQR>
static int wind_rollout_ens(f16_ctx *ctx, const char *missing, double *x, const double *u, const double *K, const double *seq, const f16_wind *w,
                            double *traj, const f16_ens *e, double *u_out, int32_t *status, long B, long ld, int nsteps, int hold,
                            int traj_every, double dt, double xcg, int fi_flag, int method, unsigned flags, void *stream) {
  if (!w) w = &STILL_AIR;      // zero air THROUGH the wind kernels
  if (int rc = wind_check(ctx, LQR, missing, x, u, K, seq, w, traj, B, ld, nsteps, hold, traj_every, method)) return rc;
  if (traj_every < 1 || nsteps % traj_every != 0)
    return set_error(F16_EINVAL, "nsteps must be a multiple of traj_every >= 1: the sample period of the ensemble, with or without traj");
  if (int rc = check_ens(e, B)) return rc;
  if (B == 0 || nsteps == 0) return F16_OK;
  const WindArgs a = wind_args(ctx, LQR, x, u, K, seq, w, traj, u_out, status, B, ld, nsteps, hold, traj_every, dt, xcg, fi_flag, flags);
  const hipStream_t st = (hipStream_t)stream;
  const bool rk4 = method == F16_INT_RK4;
  if (flags & F16_FLAG_ONE_LANE) {
    const long blocks = (B + 63) / 64;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
    if (rk4) hipLaunchKernelGGL((k_rollout_wind_exact_ens<LQR, 4>), grid, dim3(64), 0, st, a, e->work);
    else hipLaunchKernelGGL((k_rollout_wind_exact_ens<LQR, 1>), grid, dim3(64), 0, st, a, e->work);
  } else {
    const Geometry g = wind_geometry(B, fi_flag);
    by_block(g, [&](auto block) {
      constexpr int BLOCK = decltype(block)::value;
      if constexpr (BLOCK <= 256) {
        if (rk4) hipLaunchKernelGGL((k_rollout_wind_ens<BLOCK, LQR, 4>), dim3(g.grid), dim3(BLOCK), 0, st, a, e->work);
        else hipLaunchKernelGGL((k_rollout_wind_ens<BLOCK, LQR, 1>), dim3(g.grid), dim3(BLOCK), 0, st, a, e->work);
      }
    });
  }
  if (int rc = hip_check(hipGetLastError(), "f16_rollout_wind_ens launch")) return rc;
  return ens_finish(ens_args(e, B, nsteps / traj_every, flags), st, "f16_rollout_wind_ens finishing launch");
}

}  // namespace f16

using namespace f16;

extern "C" long f16_ens_work_doubles(long B, int nsamples) {
  if (B <= 0 || nsamples <= 0) return 0;
  return (long)ENS_REC * ((B + 63) / 64) * nsamples;
}

extern "C" int f16_rollout_wind_ens(f16_ctx *ctx, double *x, const double *u_seq, const f16_wind *h_wind, double *traj, const f16_ens *h_ens,
                                    int32_t *status, long B, long ld, int nsteps, int hold, int traj_every, double dt, double xcg,
                                    int fi_flag, int method, unsigned flags, void *stream) {
  return wind_rollout_ens<false>(ctx, "u_seq is NULL", x, u_seq, nullptr, u_seq, h_wind, traj, h_ens, nullptr, status, B, ld, nsteps, hold,
                                 traj_every, dt, xcg, fi_flag, method, flags, stream);
}

extern "C" int f16_rollout_lqr_wind_ens(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem_seq,
                                        const f16_wind *h_wind, double *traj, const f16_ens *h_ens, double *u_out, int32_t *status, long B,
                                        long ld, int nsteps, int hold, int traj_every, double dt, double xcg, int fi_flag, int method,
                                        unsigned flags, void *stream) {
  return wind_rollout_ens<true>(ctx, "K / dem_seq is NULL", x, u0, K, dem_seq, h_wind, traj, h_ens, u_out, status, B, ld, nsteps, hold,
                                traj_every, dt, xcg, fi_flag, method, flags, stream);
}

extern "C" int f16_ens_from_traj(f16_ctx *ctx, const double *traj, int nsamples, long B, long ld, unsigned flags, const f16_ens *h_ens,
                                 void *stream) {
  if (!ctx || !traj || B < 0 || ld < B || nsamples < 0)
    return set_error(F16_EINVAL, "bad argument (NULL pointer, B < 0, ld < B or nsamples < 0)");
  if (int rc = check_ens(h_ens, B)) return rc;
  if (B == 0 || nsamples == 0) return F16_OK;
  EnsArgs a = ens_args(h_ens, B, nsamples, flags);
  a.traj = traj; a.ld = ld;
  const long items = (long)a.S * a.W;
  hipLaunchKernelGGL(k_ens_from_traj, dim3((unsigned)(items < 65536 ? items : 65536)), dim3(64), 0, (hipStream_t)stream, a);
  if (int rc = hip_check(hipGetLastError(), "f16_ens_from_traj launch")) return rc;
  return ens_finish(a, (hipStream_t)stream, "f16_ens_from_traj finishing launch");
}
