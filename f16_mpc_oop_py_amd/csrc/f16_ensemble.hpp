// f16_ensemble.hpp -- the ensemble statistic of include/f16_hip.h ("ENSEMBLE STATISTICS") on the device: the two functions every
// entry goes through, so that a rollout's statistics and f16_ens_from_traj of its samples are the same bits.
//   ens_wave_records   one wavefront, one sample: the mask, then per state row n_w, mean_w, M2_w, min_w, max_w -> ENS_REC doubles
//   ens_fold_group     one lane, one (sample, row, group): the wave records of the group folded in ascending order (Chan's update)
// Every operation of the rule is rounded on its own.  The build contracts a * b + c wherever it sees one (-ffp-contract=fast), so a
// product that feeds a sum passes through rounded(): an empty asm the compiler cannot look through.
// The tree is an xor-butterfly over 1, 2, 4, 8, 16, 32: all 64 lanes end with the bits of v[0::2] + v[1::2] applied six times.  Lane
// distances 1 and 2 are DPP quad permutations; 4 and 8 are DPP row_half_mirror / row_mirror (lane ^ 7, lane ^ 15 -- after the
// earlier stages every lane of a group of 4 / 8 holds the same bits, so the mirrored partner holds what lane ^ 4 / lane ^ 8 holds);
// 16 is ds_swizzle, 32 ds_bpermute.  None of them touches LDS memory.  ALL 64 LANES MUST BE ACTIVE: a cross-lane read from a lane
// that is switched off is not defined, which is why the callers run whole wavefronts and pass `live` instead of leaving.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/f16_hip.h"
#include "f16_plant.hpp"

namespace f16 {

constexpr int ENS_REC = 73;   // doubles per (sample, wave): n_w, then mean_w[18], M2_w[18], min_w[18], max_w[18]

F16_DEV double rounded(double v) { asm volatile("" : "+v"(v)); return v; }

template <int CTRL>
F16_DEV double dpp_lane(double v) {
  const long long q = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)q, CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(q >> 32), CTRL, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// the value of the butterfly partner at distance DIST (see the head of the file)
template <int DIST>
F16_DEV double partner(double v) {
  if constexpr (DIST == 1) return dpp_lane<0xB1>(v);         // quad_perm [1, 0, 3, 2]
  else if constexpr (DIST == 2) return dpp_lane<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  else if constexpr (DIST == 4) return dpp_lane<0x141>(v);   // row_half_mirror
  else if constexpr (DIST == 8) return dpp_lane<0x140>(v);   // row_mirror
  else if constexpr (DIST == 16) {
    const long long q = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_ds_swizzle((int)q, 0x401F);          // bit mode: and 0x1f, or 0, xor 0x10
    const int hi = __builtin_amdgcn_ds_swizzle((int)(q >> 32), 0x401F);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
  } else return __shfl_xor(v, 32, 64);
}

struct EnsAdd { static F16_DEV double op(double a, double b) { return a + b; } };
struct EnsMin { static F16_DEV double op(double a, double b) { return fmin(a, b); } };
struct EnsMax { static F16_DEV double op(double a, double b) { return fmax(a, b); } };

template <typename OP>
F16_DEV double ens_tree(double v) {
  v = OP::op(v, partner<1>(v));
  v = OP::op(v, partner<2>(v));
  v = OP::op(v, partner<4>(v));
  v = OP::op(v, partner<8>(v));
  v = OP::op(v, partner<16>(v));
  v = OP::op(v, partner<32>(v));
  return v;
}

// One sample of one wavefront: x[18] of the lane's aircraft, live = the lane has one (b < B).  rec: the wave's ENS_REC doubles of
// this sample, the same address on every lane.  Called by all 64 lanes.
F16_DEV void ens_wave_records(const double *x, bool live, unsigned flags, double *rec) {
  bool m = live;
#pragma unroll
  for (int k = 0; k < 18; ++k) m = m && isfinite(x[k]);
  if (!(flags & FLAG_NO_ENVELOPE)) m = m && !outside_envelope(x);
  const int lane = threadIdx.x & 63;
  const int n = __popcll(__ballot(m));          // the same on every lane: a scalar
  const double nd = (double)n, inf = __builtin_huge_val();
  double r_mean = 0.0, r_m2 = 0.0, r_min = inf, r_max = -inf;      // lane k keeps row k
#pragma unroll
  for (int k = 0; k < 18; ++k) {
    double mean = 0.0, m2 = 0.0, mn = inf, mx = -inf;
    if (n > 0) {
      mean = ens_tree<EnsAdd>(m ? x[k] : 0.0) / nd;
      const double d = m ? x[k] - mean : 0.0;
      m2 = ens_tree<EnsAdd>(rounded(d * d));
      mn = ens_tree<EnsMin>(m ? x[k] : inf);
      mx = ens_tree<EnsMax>(m ? x[k] : -inf);
    }
    if (lane == k) { r_mean = mean; r_m2 = m2; r_min = mn; r_max = mx; }
  }
  if (lane < 18) {
    rec[1 + lane] = r_mean;
    rec[19 + lane] = r_m2;
    rec[37 + lane] = r_min;
    rec[55 + lane] = r_max;
  }
  if (lane == 0) rec[0] = nd;
}

struct EnsGroup { int n; double mean, m2, mn, mx; };

// Row k of one group at one sample: rec = the sample's record of the group's first wave, nw waves (ENS_REC doubles apart)
F16_DEV EnsGroup ens_fold_group(const double *rec, int nw, int k) {
  double n = 0.0, mean = 0.0, m2 = 0.0, mn = __builtin_huge_val(), mx = -__builtin_huge_val();
  for (int w = 0; w < nw; ++w, rec += ENS_REC) {
    const double n_w = rec[0];
    if (n_w == 0.0) continue;
    const double mean_w = rec[1 + k], m2_w = rec[19 + k];
    mn = fmin(mn, rec[37 + k]);
    mx = fmax(mx, rec[55 + k]);
    if (n == 0.0) { n = n_w; mean = mean_w; m2 = m2_w; continue; }
    const double N = n + n_w, delta = mean_w - mean;
    mean = mean + rounded(delta * (n_w / N));
    m2 = (m2 + m2_w) + rounded(rounded(delta * delta) * ((n * n_w) / N));
    n = N;
  }
  return EnsGroup{(int)n, mean, m2, mn, mx};
}

// host, defined in f16_wind_ens.hip for the twins of other translation units (f16_observer.hip): the rules of an f16_ens, and the
// finishing launch behind a rollout whose wavefronts wrote their records of S samples
int ens_rules(const f16_ens *e, long B);
int ens_finish_launch(const f16_ens *e, long B, int S, unsigned flags, void *stream, const char *what);

}  // namespace f16
