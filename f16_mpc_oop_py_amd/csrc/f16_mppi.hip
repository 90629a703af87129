// f16_mppi.hip -- the stand-alone entries of an MPPI step around f16_rollout_cost: the counter-based sampler that writes the sample
// set (f16_mppi_sample; f16_debug_philox for its generator) and the softmin blend over the per-lane costs (f16_mppi_blend).  The
// statements both share with the fused loop f16_rollout_mppi are in f16_mppi.hpp.
//
// Blend mapping: one lane = one aircraft a, so every read of cost[k * B0 + a] and u_seq[row][c][k * B0 + a] is contiguous over a wave; the
// rows of the schedule are spread over grid.y, a lane blends the four commands of its row.  Every lane walks its aircraft's K samples
// in ascending order in plain fp64 -- the minimum, then one pass that forms exp(-(J_k - m) / lambda) once per sample and adds it to
// the two weight sums and the four command sums -- so the result does not depend on the launch geometry.  Per row that is K
// exponentials against 4 K eight-byte reads: bound by the reads.  No scratch memory: the weights are recomputed per row rather than
// stored, and the lanes of row 0 write w_out / stats.
#include <hip/hip_runtime.h>

#include <math.h>

#include "../../include/f16_hip.h"
#include "f16_ctx.h"
#include "f16_mppi.hpp"      // the sampler and the softmin walk, shared with the fused loop k_rollout_mppi (f16_dynamics.hip)

namespace f16 {

struct BlendArgs {
  const double *cost;    // [ld]
  const double *u_seq;   // [nrows][4][ld]
  double *u_blend;       // [nrows][4][ld0]
  double *w_out;         // [ld] or null
  double *stats;         // [2][ld0] or null
  double lambda;
  long B0, ld0, ld, K;
  int nrows;
};

__global__ __launch_bounds__(64) void k_mppi_blend(BlendArgs a) {
  const long ac = (long)blockIdx.x * 64 + threadIdx.x;
  if (ac >= a.B0) return;
  const double m = blend_min(a.cost + ac, a.K, a.B0);
  const bool any = m < INFINITY;                 // at least one finite cost
  // row 0's lanes also own the per-aircraft outputs; with no rows at all they are the only work (grid.y = 1)
  for (int row = blockIdx.y; row < (a.nrows > 0 ? a.nrows : 1); row += gridDim.y) {
    const bool blend = row < a.nrows;
    const double *u = a.u_seq + (long)row * 4 * a.ld + ac;
    double sw = 0, sw2 = 0, acc[4] = {0, 0, 0, 0};
    blend_walk<4>(a.cost + ac, u, a.K, a.B0, a.ld, m, a.lambda, blend, sw, sw2, acc);
    if (blend) {
#pragma unroll
      for (int c = 0; c < 4; ++c) a.u_blend[((long)row * 4 + c) * a.ld0 + ac] = any ? acc[c] / sw : u[c * a.ld];
    }
    if (row == 0) {
      if (a.stats) { a.stats[ac] = any ? m : 0.0; a.stats[a.ld0 + ac] = any ? sw * sw / sw2 : 0.0; }
      if (a.w_out) {
        for (long k = 0; k < a.K; ++k) {
          const double J = a.cost[k * a.B0 + ac];
          a.w_out[k * a.B0 + ac] = isfinite(J) ? exp(-(J - m) / a.lambda) / sw : 0.0;
        }
      }
    }
  }
}

// f16_mppi_sample: one lane = one lane j = k * B0 + a of the sample set, the rows over grid.y; every lane writes its own four
// values of a row through mppi_write_row, the statement the fused loop (k_rollout_mppi) writes its samples with.
struct SampleArgs {
  const double *u_nom;   // [nrows][4][ld0]
  double *u_seq;         // [nrows][4][ld]
  double sg[3];
  uint32_t key0, key1, period;
  long B, B0, ld0, ld;
  int nrows;
};

__global__ __launch_bounds__(64) void k_mppi_sample(SampleArgs a) {
  const long j = (long)blockIdx.x * 64 + threadIdx.x;
  if (j >= a.B) return;
  const long k = j / a.B0, ac = j % a.B0;
  for (int row = blockIdx.y; row < a.nrows; row += gridDim.y)
    mppi_write_row(a.u_nom + (long)row * 4 * a.ld0 + ac, a.ld0, a.u_seq + (long)row * 4 * a.ld + j, a.ld, a.period, (uint32_t)row,
                   (uint32_t)k, (uint32_t)ac, a.key0, a.key1, a.sg[0], a.sg[1], a.sg[2]);
}

__global__ __launch_bounds__(64) void k_dbg_philox(const uint32_t *__restrict__ ctr, const uint32_t *__restrict__ key,
                                                   uint32_t *__restrict__ out, long n) {
  for (long p = (long)blockIdx.x * 64 + threadIdx.x; p < n; p += (long)gridDim.x * 64) {
    const Philox4 r = philox4x32_10(ctr[4 * p], ctr[4 * p + 1], ctr[4 * p + 2], ctr[4 * p + 3], key[2 * p], key[2 * p + 1]);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[4 * p + i] = r.r[i];
  }
}

}  // namespace f16

using namespace f16;

extern "C" int f16_mppi_sample(f16_ctx *ctx, const double *u_nom, const double *h_sigma, uint64_t seed, uint32_t period,
                               double *u_seq, long B, long ld, long B0, long ld0, int nrows, void *stream) {
  if (!ctx || !u_nom || !h_sigma || !u_seq) return set_error(F16_EINVAL, "ctx / u_nom / h_sigma / u_seq is NULL");
  for (int i = 0; i < 3; ++i)
    if (!(h_sigma[i] >= 0.0) || !isfinite(h_sigma[i])) return set_error(F16_EINVAL, "sigma must be finite and >= 0");
  if (B < 0 || ld < B || nrows < 0) return set_error(F16_EINVAL, "bad argument (B < 0, ld < B or nrows < 0)");
  if (B > 0 && (B0 < 1 || ld0 < B0 || B % B0 != 0))
    return set_error(F16_EINVAL, "B lanes are K samples of B0 aircraft: B0 >= 1, ld0 >= B0 and B % B0 == 0");
  if (B == 0 || nrows == 0) return F16_OK;
  SampleArgs a{};
  a.u_nom = u_nom; a.u_seq = u_seq; a.sg[0] = h_sigma[0]; a.sg[1] = h_sigma[1]; a.sg[2] = h_sigma[2];
  a.key0 = (uint32_t)(seed & 0xffffffffu); a.key1 = (uint32_t)(seed >> 32); a.period = period;
  a.B = B; a.B0 = B0; a.ld0 = ld0; a.ld = ld; a.nrows = nrows;
  const unsigned gy = nrows < 65535 ? (unsigned)nrows : 65535u;
  hipLaunchKernelGGL(k_mppi_sample, dim3((unsigned)((B + 63) / 64), gy), dim3(64), 0, (hipStream_t)stream, a);
  return hip_check(hipGetLastError(), "f16_mppi_sample launch");
}

extern "C" int f16_debug_philox(f16_ctx *ctx, const uint32_t *h_ctr, const uint32_t *h_key, long n, uint32_t *h_out) {
  if (!ctx || !h_ctr || !h_key || !h_out || n < 0) return set_error(F16_EINVAL, "bad argument to f16_debug_philox");
  if (n == 0) return F16_OK;
  uint32_t *d = nullptr;
  int rc;
  if ((rc = hip_check(hipMalloc(&d, 10 * (size_t)n * sizeof(uint32_t)), "hipMalloc dbg philox"))) return rc;
  if (!(rc = hip_check(hipMemcpy(d, h_ctr, 4 * (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice), "copy counters")) &&
      !(rc = hip_check(hipMemcpy(d + 4 * n, h_key, 2 * (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice), "copy keys"))) {
    const long blocks = (n + 63) / 64;
    hipLaunchKernelGGL(k_dbg_philox, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(64), 0, nullptr, d, d + 4 * n, d + 6 * n, n);
    rc = hip_check(hipGetLastError(), "f16_debug_philox launch");
    if (!rc) rc = hip_check(hipMemcpy(h_out, d + 6 * n, 4 * (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost), "copy out");
  }
  (void)hipFree(d);
  return rc;
}

extern "C" int f16_mppi_blend(f16_ctx *ctx, const double *cost, const double *u_seq, double lambda, double *u_blend, double *w_out,
                              double *stats, long B, long ld, long B0, long ld0, int nrows, void *stream) {
  if (!ctx || !cost || !u_seq || !u_blend) return set_error(F16_EINVAL, "ctx / cost / u_seq / u_blend is NULL");
  if (!(lambda > 0.0) || !isfinite(lambda)) return set_error(F16_EINVAL, "lambda must be finite and > 0");
  if (B < 0 || ld < B || nrows < 0) return set_error(F16_EINVAL, "bad argument (B < 0, ld < B or nrows < 0)");
  if (B > 0 && (B0 < 1 || ld0 < B0 || B % B0 != 0))
    return set_error(F16_EINVAL, "B lanes are K samples of B0 aircraft: B0 >= 1, ld0 >= B0 and B % B0 == 0");
  if (B == 0) return F16_OK;
  BlendArgs a{};
  a.cost = cost; a.u_seq = u_seq; a.u_blend = u_blend; a.w_out = w_out; a.stats = stats;
  a.lambda = lambda; a.B0 = B0; a.ld0 = ld0; a.ld = ld; a.K = B / B0; a.nrows = nrows;
  const unsigned gy = nrows < 1 ? 1u : (nrows < 65535 ? (unsigned)nrows : 65535u);
  hipLaunchKernelGGL(k_mppi_blend, dim3((unsigned)((B0 + 63) / 64), gy), dim3(64), 0, (hipStream_t)stream, a);
  return hip_check(hipGetLastError(), "f16_mppi_blend launch");
}
