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
int ens_rules(const f16_ens *e, long B) {
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

int ens_finish_launch(const f16_ens *e, long B, int S, unsigned flags, void *stream, const char *what) {
  const EnsArgs a = ens_args(e, B, S, flags);
  const long blocks = ((long)a.S * 18 * a.G + 63) / 64;
  hipLaunchKernelGGL(k_ens_finish, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(64), 0, (hipStream_t)stream, a);
  return hip_check(hipGetLastError(), what);
}

// The kernel family of the ensemble calls (f16_wind_lanes.hpp: wind_rollout): the kernels take the workspace behind the argument block.
template <bool L>
struct WindEnsKernels {
  static constexpr bool LQR = L, ENS = true, OBS = false;
  static constexpr const char *what = "f16_rollout_wind_ens launch", *what_finish = "f16_rollout_wind_ens finishing launch";
  template <int BLOCK, int STAGES>
  static void launch(dim3 grid, hipStream_t st, const WindArgs &a, const WindRollout &d) {
    hipLaunchKernelGGL((k_rollout_wind_ens<BLOCK, L, STAGES>), grid, dim3(BLOCK), 0, st, a, d.ens->work);
  }
  template <int STAGES>
  static void launch_exact(dim3 grid, hipStream_t st, const WindArgs &a, const WindRollout &d) {
    hipLaunchKernelGGL((k_rollout_wind_exact_ens<L, STAGES>), grid, dim3(64), 0, st, a, d.ens->work);
  }
};

}  // namespace f16

using namespace f16;

extern "C" long f16_ens_work_doubles(long B, int nsamples) {
  if (B <= 0 || nsamples <= 0) return 0;
  return (long)ENS_REC * ((B + 63) / 64) * nsamples;
}

extern "C" int f16_rollout_wind_ens(f16_ctx *ctx, double *x, const double *u_seq, const f16_wind *h_wind, double *traj, const f16_ens *h_ens,
                                    int32_t *status, long B, long ld, int nsteps, int hold, int traj_every, double dt, double xcg,
                                    int fi_flag, int method, unsigned flags, void *stream) {
  WindRollout d{"u_seq is NULL", x, u_seq, u_seq, h_wind, traj, status, B, ld, nsteps, hold, traj_every, dt, xcg, fi_flag, method, flags};
  d.ens = h_ens;
  return wind_rollout<WindEnsKernels<false>>(ctx, d, stream);
}

extern "C" int f16_rollout_lqr_wind_ens(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem_seq,
                                        const f16_wind *h_wind, double *traj, const f16_ens *h_ens, double *u_out, int32_t *status, long B,
                                        long ld, int nsteps, int hold, int traj_every, double dt, double xcg, int fi_flag, int method,
                                        unsigned flags, void *stream) {
  WindRollout d{"K / dem_seq is NULL", x, u0, dem_seq, h_wind, traj, status, B, ld, nsteps, hold, traj_every, dt, xcg, fi_flag, method, flags};
  d.K = K; d.u_out = u_out; d.ens = h_ens;
  return wind_rollout<WindEnsKernels<true>>(ctx, d, stream);
}

extern "C" int f16_ens_from_traj(f16_ctx *ctx, const double *traj, int nsamples, long B, long ld, unsigned flags, const f16_ens *h_ens,
                                 void *stream) {
  if (!ctx || !traj || B < 0 || ld < B || nsamples < 0)
    return set_error(F16_EINVAL, "bad argument (NULL pointer, B < 0, ld < B or nsamples < 0)");
  if (int rc = ens_rules(h_ens, B)) return rc;
  if (B == 0 || nsamples == 0) return F16_OK;
  EnsArgs a = ens_args(h_ens, B, nsamples, flags);
  a.traj = traj; a.ld = ld;
  const long items = (long)a.S * a.W;
  hipLaunchKernelGGL(k_ens_from_traj, dim3((unsigned)(items < 65536 ? items : 65536)), dim3(64), 0, (hipStream_t)stream, a);
  if (int rc = hip_check(hipGetLastError(), "f16_ens_from_traj launch")) return rc;
  return ens_finish_launch(h_ens, B, nsamples, flags, stream, "f16_ens_from_traj finishing launch");
}
