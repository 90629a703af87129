// f16_observer.hpp -- output feedback for the frozen-gain LQR loop (include/f16_hip.h "OUTPUT FEEDBACK"): sampled sensor noise, the
// steady-state Kalman filter on the reduced 9-state model and the LQR law on the estimate, written once for f16_observer_step and
// for the rollout kernels of f16_observer.hip (the OBS lane loop of f16_wind_lanes.hpp).
//
// The rule, per step of an aircraft that is not frozen, from the state at the start of the step (x9 = x[3, 4, 7, 8, 9, 10, 11, 17, 16],
// s = x[13..15]; the model record M of the aircraft's group, F16_OBS_DOUBLES doubles):
//     y_k    = x9_k + (sigma_k * n_k)                          sensed k; every operation rounded on its own
//     e_k    = y_k - xm_k;   xh_i = xm_i + sum_k Lf[i][k] e_k  over the sensed k ascending, one fma per term
//     u[1+i] = lqr_action(K[i][4..6], dem - xh[4..6], u0[1+i])
//     xm_i  <- trim_i + sum_j Ad[i][j] (xh_j - trim_j) + sum_j Bd[i][j] (s_j - strim_j)      one fma per term, in this order
// with xm the prediction the xhat array holds between steps.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/f16_hip.h"
#include "f16_mppi.hpp"
#include "f16_rollout_common.hpp"

namespace f16 {

constexpr uint32_t MEAS_COUNTER_WORD = 0xFFFFFFFEu;      // counter word 2 of a measurement row: gusts use 0xFFFFFFFF, MPPI values < 256
constexpr int OBS_BD = 81, OBS_LF = 108, OBS_TRIM = 189, OBS_STRIM = 198;      // offsets inside a model record

// What the observer needs beyond the sibling's argument block.  The kernels keep ONE copy per workgroup in LDS (every field is the
// same on all lanes), so that the out-of-line observer_update takes a pointer and the lane's values only: its arguments stay in
// registers.  kq, us, stride: the lane-indexed LDS slots of the gains, demands and commands (slot j of lane l at [j * stride + l]).
struct ObsArgs {
  const double *obs;           // [M][F16_OBS_DOUBLES]
  double *xhat;                // [9][ld] in / out: the prediction
  double *y_out;               // [9][ld] or null: the measurements (f16_observer_step)
  double *xhat_traj;           // [S][9][ld] or null: the content of xhat at every sample point
  long mgroup, ld;
  uint32_t key0, key1, mrow0;
  int sensed;
  double sigma[9];
  const double *kq, *us;
  int stride;
};

// the model record's values come through wave-uniform addresses in the constant address space: scalar loads
typedef const double __attribute__((address_space(4))) obs_const_double;

// The four standard normals of call j of measurement row `row` (f16_mppi_sample's U_i; Box-Muller on (U0, U1) and (U2, U3), cosine and
// sine of both)
F16_DEV void meas_normals4(uint32_t row, uint32_t j, uint32_t aircraft, uint32_t key0, uint32_t key1, double *n) {
  const Philox4 p = philox4x32_10(row, j, MEAS_COUNTER_WORD, aircraft, key0, key1);
  constexpr double SCALE = 1.0 / 4294967296.0, TWO_PI = 6.283185307179586476925286766559;
  const double U0 = ((double)p.r[0] + 0.5) * SCALE, U1 = ((double)p.r[1] + 0.5) * SCALE;
  const double U2 = ((double)p.r[2] + 0.5) * SCALE, U3 = ((double)p.r[3] + 0.5) * SCALE;
  const double ra = sqrt(-2.0 * log(U0)), rb = sqrt(-2.0 * log(U2));
  double s1, c1, s3, c3;
  sincos(TWO_PI * U1, &s1, &c1);
  sincos(TWO_PI * U3, &s3, &c3);
  n[0] = __dmul_rn(ra, c1); n[1] = __dmul_rn(ra, s1); n[2] = __dmul_rn(rb, c3); n[3] = __dmul_rn(rb, s3);
}

// Steps 1 - 4 of the rule for ONE aircraft.  o: the workgroup's copy in LDS; b: the aircraft (its column, its counter word); row:
// counter word 0; x9[0..8], s[0..2] by value.  Reads xhat, writes the new prediction there (and y_out when given); returns the three
// surface commands.  Inlined into the default rollout kernels, as their plant step is (no frame, no scratch memory).
struct Obs3 { double v[3]; };
F16_DEV Obs3 observer_rule(const ObsArgs *o, long b, uint32_t row, double x0, double x1, double x2, double x3, double x4, double x5, double x6,
                           double x7, double x8, double s0, double s1, double s2) {
  const int sensed = __builtin_amdgcn_readfirstlane(o->sensed);
  const uint32_t key0 = __builtin_amdgcn_readfirstlane(o->key0), key1 = __builtin_amdgcn_readfirstlane(o->key1);
  const long ld = o->ld, mg = o->mgroup;
  // the wavefront's model: aircraft b uses model b / mgroup, the same for the 64 aircraft of a wave (mgroup % 64 == 0)
  const unsigned long at = (unsigned long)(o->obs + (mg ? b / mg : 0) * F16_OBS_DOUBLES);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)at), hi = __builtin_amdgcn_readfirstlane((unsigned)(at >> 32));
  obs_const_double *M = (obs_const_double *)(((unsigned long)hi << 32) | lo);
  double *xh_col = o->xhat + b;
  const double x9[9] = {x0, x1, x2, x3, x4, x5, x6, x7, x8}, s[3] = {s0, s1, s2};
  double xh[9], e[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) xh[i] = xh_col[i * ld];
  // 1. the measurements: call j serves channels 4 j .. 4 j + 3 and is not made when none of them is sensed
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if ((sensed >> (4 * j)) & 0xf) {
      double n[4];
      meas_normals4(row, (uint32_t)j, (uint32_t)b, key0, key1, n);
#pragma unroll
      for (int c = 0; c < 4 && 4 * j + c < 9; ++c) {
        const int k = 4 * j + c;
        const double y = __dadd_rn(x9[k], __dmul_rn(o->sigma[k], n[c]));
        e[k] = __dsub_rn(y, xh[k]);
        if (((sensed >> k) & 1) && o->y_out) o->y_out[k * ld + b] = y;
      }
    }
  }
  // 2. the correction, column by column of Lf: per entry the sensed k in ascending order
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    if ((sensed >> k) & 1) {
#pragma unroll
      for (int i = 0; i < 9; ++i) xh[i] = fma(M[OBS_LF + 9 * i + k], e[k], xh[i]);
    }
  }
  // 3. the LQR law on the estimate
  Obs3 u;
  {
    const double *kq = o->kq + threadIdx.x, *us = o->us + threadIdx.x;
    const int st = o->stride;
    const double e0 = kq[9 * st] - xh[4], e1 = kq[10 * st] - xh[5], e2 = kq[11 * st] - xh[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) u.v[i] = lqr_action(kq[3 * i * st], kq[(3 * i + 1) * st], kq[(3 * i + 2) * st], e0, e1, e2, us[(1 + i) * st]);
  }
  // 4. the prediction
  {
    double d[9], ds[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) d[j] = __dsub_rn(xh[j], M[OBS_TRIM + j]);
#pragma unroll
    for (int j = 0; j < 3; ++j) ds[j] = __dsub_rn(s[j], M[OBS_STRIM + j]);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      double acc = M[OBS_TRIM + i];
#pragma unroll
      for (int j = 0; j < 9; ++j) acc = fma(M[9 * i + j], d[j], acc);
#pragma unroll
      for (int j = 0; j < 3; ++j) acc = fma(M[OBS_BD + 3 * i + j], ds[j], acc);
      xh_col[i * ld] = acc;
    }
  }
  return u;
}

// The same compiled OUT OF LINE, for the reason wind_step_exact is: f16_observer_step and every rollout kernel under F16_FLAG_ONE_LANE
// go through this one instruction sequence, which is what makes the fused call the chain of step calls bit for bit.
static __device__ __noinline__ Obs3 observer_update(const ObsArgs *o, long b, uint32_t row, double x0, double x1, double x2, double x3, double x4,
                                                    double x5, double x6, double x7, double x8, double s0, double s1, double s2) {
  return observer_rule(o, b, row, x0, x1, x2, x3, x4, x5, x6, x7, x8, s0, s1, s2);
}

}  // namespace f16
