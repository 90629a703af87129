// f16_linearise.hpp -- the forward-difference rule of the reduced model (env.py:294-342 with _calc_xdot_na / _get_obs_na), stated once:
// which full-state entry a column perturbs, the u[1:4]-over-actuator-states overwrite, C = diag((fl(x + eps) - x) / eps) and the base
// point.  k_linearise (f16_control.hip) takes the two maps; the per-step loops -- k_rollout_lqr_relin (f16_control.hip) and
// wave::pair_model (f16_mpc_wave.hip) -- call linearise_na_wave, so that f16_mpc_batch_w on a stored model_traj record rebuilds the
// loop's QP bit for bit by construction.
#pragma once
#include <hip/hip_runtime.h>

#include "f16_plant.hpp"
#include "f16_smallmat.hpp"

namespace f16 {

// MPC state j -> index of the full state (parameters.py:135 mpc_x_idx): phi, theta, alpha, beta, p, q, r, lf1, lf2
constexpr int MPC_X_IDX[9] = {3, 4, 7, 8, 9, 10, 11, 17, 16};
// ... as a select chain, for a j that is a lane or a loop counter: folds to the entry where j is known at compile time
__host__ __device__ constexpr int mpc_x_index(int j) {
  int k = MPC_X_IDX[8];
  for (int i = 7; i >= 0; --i) k = j == i ? MPC_X_IDX[i] : k;
  return k;
}
// column c of the reduced model -> the full-state entry it perturbs: 0..8 the MPC states, 9..11 the inputs, which stand in the
// actuator states 13..15 (env.py:175-177); anything else (lane 12 of the wave-level rule: the base point) -> none
__host__ __device__ constexpr int lin_na_index(int c) { return c < 9 ? mpc_x_index(c) : c < 12 ? 13 + (c - 9) : -1; }

// One wavefront, one aircraft at (x18, u[1:4] = u1, u2, u3): lanes 0..11 evaluate the perturbed columns and lane 12 the base point
// through the out-of-line xdot_na_exact into F [13 * 9]; then A [81], Bm [27] (row-major) and cd [9], the diagonal of C, all in LDS.
// A and Bm are published by the caller's next barrier; cd already is.
__device__ __forceinline__ void linearise_na_wave(const double *tab, const double *lofi, const double *x18, double u1, double u2, double u3,
                                                  double eps, double xcg, int fi, unsigned flags, double *F, double *A, double *Bm,
                                                  double *cd, int l) {
  if (l < 13) {
    const int idx = lin_na_index(l);
    double sv[18], f[9];
#pragma unroll
    for (int k = 0; k < 18; ++k) sv[k] = x18[k];
    sv[13] = u1; sv[14] = u2; sv[15] = u3;      // env.py:175-177
    double base = 0.0, pert = 0.0;
#pragma unroll
    for (int k = 0; k < 18; ++k)
      if (k == idx) { base = sv[k]; pert = sv[k] + eps; sv[k] = pert; }
    int sl = 0;      // (the grid bits of the perturbed points are not the aircraft's: _calc_LQR_gain / build_ssr do not keep them)
    xdot_na_exact(tab, lofi, sv, f, xcg, fi, flags, &sl);
#pragma unroll
    for (int r = 0; r < 9; ++r) F[l * 9 + r] = f[r];
    if (l < 9) cd[l] = (pert - base) / eps;
  }
  __syncthreads();
  for (int e = l; e < 108; e += F16_WAVE) {
    if (e < 81) { const int r = e / 9, c = e - r * 9; A[e] = (F[c * 9 + r] - F[12 * 9 + r]) / eps; }
    else { const int e2 = e - 81, r = e2 / 3, c = e2 - r * 3; Bm[e2] = (F[(9 + c) * 9 + r] - F[12 * 9 + r]) / eps; }
  }
}

}  // namespace f16
