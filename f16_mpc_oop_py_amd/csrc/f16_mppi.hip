// f16_mppi.hip -- the softmin blend of an MPPI step (f16_mppi_blend) over the per-lane costs of f16_rollout_cost.
//
// Mapping: one lane = one aircraft a, so every read of cost[k * B0 + a] and u_seq[row][c][k * B0 + a] is contiguous over a wave; the
// rows of the schedule are spread over grid.y, a lane blends the four commands of its row.  Every lane walks its aircraft's K samples
// in ascending order in plain fp64 -- the minimum, then one pass that forms exp(-(J_k - m) / lambda) once per sample and adds it to
// the two weight sums and the four command sums -- so the result does not depend on the launch geometry.  Per row that is K
// exponentials against 4 K eight-byte reads: bound by the reads.  No scratch memory: the weights are recomputed per row rather than
// stored, and the lanes of row 0 write w_out / stats.
#include <hip/hip_runtime.h>

#include <math.h>

#include "../../include/f16_hip.h"
#include "f16_ctx.h"

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
  double m = INFINITY;
  for (long k = 0; k < a.K; ++k) {
    const double J = a.cost[k * a.B0 + ac];
    if (isfinite(J) && J < m) m = J;
  }
  const bool any = m < INFINITY;                 // at least one finite cost
  // row 0's lanes also own the per-aircraft outputs; with no rows at all they are the only work (grid.y = 1)
  for (int row = blockIdx.y; row < (a.nrows > 0 ? a.nrows : 1); row += gridDim.y) {
    const bool blend = row < a.nrows;
    const double *u = a.u_seq + (long)row * 4 * a.ld + ac;
    double sw = 0, sw2 = 0, acc[4] = {0, 0, 0, 0};
    for (long k = 0; k < a.K; ++k) {
      const double J = a.cost[k * a.B0 + ac];
      if (!isfinite(J)) continue;                // weight 0: its commands (NaN rows among them) are not read
      const double w = exp(-(J - m) / a.lambda);
      sw += w; sw2 += w * w;
      if (blend) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] += w * u[c * a.ld + k * a.B0];
      }
    }
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

}  // namespace f16

using namespace f16;

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
