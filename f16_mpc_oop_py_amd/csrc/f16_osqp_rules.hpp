// f16_osqp_rules.hpp -- what OSQP decides once a solver has its reduced norms on hand, stated once for the four solvers
// (f16_control.hip k_mpc, f16_mpc_solve.hip k_mpc_fast, f16_mpc_big.hip k_mpc_big, f16_mpc_wave.hip k_mpc_wave / k_rollout_mpc):
// the termination test, the primal-infeasibility certificate, the rho estimate and its band, the opt-in start value of rho, the
// status bits of a finished solve; and the small register-level tools two of the solvers share.  Scalar rules only: layout,
// reductions, LDS traffic and barriers are each solver's own.  Arguments BY VALUE, never the kernel-argument block (f16_mpc.hpp:
// mpc_job_nonfinite).  The order of the floating-point operations is part of the rules: the tests hold every solver to a CPU twin,
// which keeps its own wording of the same rules, iterate for iterate.
#pragma once
#include <math.h>

#include "f16_mpc.hpp"

namespace f16 {

// OSQP termination test on the UNSCALED problem: n_prim = max(|Ax|, |z|), n_dual = max(|Px|, |A'y|, |q|).  (One half alone:
// k_mpc_wave forms the dual side only at the tests that can need it.)
__device__ __forceinline__ bool osqp_residual_small(double r, double n, double eps_abs, double eps_rel) { return r < eps_abs + eps_rel * n; }
__device__ __forceinline__ bool osqp_converged(double rp, double rd, double n_prim, double n_dual, double eps_abs, double eps_rel) {
  return osqp_residual_small(rp, n_prim, eps_abs, eps_rel) && osqp_residual_small(rd, n_dual, eps_abs, eps_rel);
}

// OSQP primal-infeasibility certificate on dy (auxil.c:is_primal_infeasible): ndy = |E dyb|_inf, supp = the support function of
// the bounds at dy; a candidate is certified when nat = |A' dy|_inf is small against ndy (the solvers form nat for candidates only)
__device__ __forceinline__ bool osqp_infeasibility_candidate(double ndy, double supp, double eps_prim_inf) {
  return ndy > eps_prim_inf && supp < -eps_prim_inf * ndy;
}
__device__ __forceinline__ bool osqp_infeasibility_certified(double nat, double ndy, double eps_prim_inf) {
  return nat < eps_prim_inf * ndy;
}

// ---- soft rows (f16_mpc_plan_soft_rows; k_mpc_wave_soft / k_rollout_mpc_soft): row i carries the penalty (w_i / 2) dist(a_i'u, [l_i, u_i])^2
// instead of the constraint.  No slack variable: the z-update of the row is the proximal step of that penalty,
//   v = zr + y / rho_i,  zc = clip(v, l, u),  z = zc + kappa_i (v - zc),  kappa_i = rho_i / (rho_i + c w_i / E_i^2)
// (cw_over_W: c w_i / E_i^2, the penalty weight in the scaled variables; kappa = 0 on a hard row).  z == zc exactly while v is inside.
__device__ __forceinline__ double osqp_soft_kappa(bool soft, double rho_row, double cw_over_W) {
  return soft ? rho_row / (rho_row + cw_over_W) : 0.0;
}
__device__ __forceinline__ double osqp_soft_prox(double v, double zc, double kappa) { return zc + kappa * (v - zc); }
// ... and in the certificate a soft row is a row without bounds: nothing in the support function, and a candidate whose dy does not
// vanish on it is no certificate (is_primal_infeasible: |E_i dyb_i| > eps_prim_inf |E dyb|_inf on a row with two infinite bounds).
// soft_dy: the largest |E_i dyb_i| over the soft rows.
__device__ __forceinline__ bool osqp_soft_rows_reject(double soft_dy, double ndy, double eps_prim_inf) { return soft_dy > eps_prim_inf * ndy; }

// auxil.c:compute_rho_estimate on the SCALED residuals ||Ab xb - zb||, ||Pb xb + qb + Ab' yb|| and their norms: the clamped
// candidate, and whether it leaves the band around the present rho (then the solver factorises again)
__device__ __forceinline__ double osqp_rho_estimate(double rho, double r_prim_s, double n_z_s, double n_Ax_s, double r_dual_s,
                                                    double n_q_s, double n_Aty_s, double n_Px_s) {
  const double pr = r_prim_s / (fmax(n_z_s, n_Ax_s) + 1e-10), dr = r_dual_s / (fmax(fmax(n_q_s, n_Aty_s), n_Px_s) + 1e-10);
  return fmin(fmax(rho * sqrt(pr / (dr + 1e-10)), OSQP_RHO_MIN), OSQP_RHO_MAX);
}
__device__ __forceinline__ bool osqp_rho_accepted(double candidate, double rho) {
  // (two named comparisons: with `a || b` in the return statement the callers' machine code changes, with this form it does not)
  const bool above = candidate > OSQP_ADAPTIVE_RHO_TOLERANCE * rho, below = candidate < rho / OSQP_ADAPTIVE_RHO_TOLERANCE;
  return above || below;
}

// the builder's opt-in start value of rho (f16_qp_settings.rho <= 0, no equilibration): balance the two terms of P + rho A'A
__device__ __forceinline__ double osqp_rho_start(double tr_P, double tr_AtA) {
  return fmin(fmax(RHO_AUTO_SCALE * sqrt(tr_P / tr_AtA), OSQP_RHO_MIN), OSQP_RHO_MAX);
}

// The bits a finished solve ORs into the status word.  ok: every factorisation succeeded.  max_iter <= 0 asks for no iterations
// (factor only), which is no failure to converge.
__device__ __forceinline__ int32_t mpc_status_bits(bool converged, bool infeasible, bool ok, int max_iter) {
  if (infeasible) return F16_ST_QP_INFEASIBLE;
  return max_iter > 0 && (!converged || !ok) ? F16_ST_QP_MAXITER : 0;
}

// The settings the iterations read, handed by value to the solvers' device functions.  iter_settings takes its argument BY VALUE
// too: with `const f16_qp_settings &` the scratch copy of the kernel-argument block is back in k_mpc_fast (296 -> 1640 bytes per lane).
struct IterSettings { double alpha, eps_abs, eps_rel, eps_prim_inf; int max_iter, check_every, rho_every, adaptive_rho; };
__device__ __forceinline__ IterSettings iter_settings(f16_qp_settings s) {
  return IterSettings{s.alpha, s.eps_abs, s.eps_rel, s.eps_prim_inf, s.max_iter, s.check_every, s.rho_every, s.adaptive_rho};
}

// ---- the pivot block of the blocked symmetric sweep (k_mpc_fast: eight waves; k_mpc_wave: one)
// 1/x to <= 1 ulp without the division sequence (v_rcp_f64 + two Newton steps); x is a positive, normal pivot minor
__device__ __forceinline__ double rcp_nr(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(r, fma(-x, r, 1.0), r);
  r = fma(r, fma(-x, r, 1.0), r);
  return r;
}

// inverse of a 4x4 SPD block given by its lower triangle; false if a leading minor is not positive
__device__ __forceinline__ bool inv4_spd(const double (&d)[4][4], double (&o)[4][4]) {
  const double a = d[0][0], b = d[1][0], c = d[1][1];
  const double detA = a * c - b * b;
  const double ia = rcp_nr(detA);
  const double A00 = c * ia, A10 = -b * ia, A11 = a * ia;                  // A^-1
  const double B00 = d[2][0], B01 = d[2][1], B10 = d[3][0], B11 = d[3][1];  // rows 2,3 x cols 0,1
  const double T00 = B00 * A00 + B01 * A10, T01 = B00 * A10 + B01 * A11;    // T = B A^-1
  const double T10 = B10 * A00 + B11 * A10, T11 = B10 * A10 + B11 * A11;
  const double S00 = d[2][2] - (T00 * B00 + T01 * B01);                     // S = E - T B'
  const double S10 = d[3][2] - (T10 * B00 + T11 * B01);
  const double S11 = d[3][3] - (T10 * B10 + T11 * B11);
  const double detS = S00 * S11 - S10 * S10;
  const double is = rcp_nr(detS);
  const double I00 = S11 * is, I10 = -S10 * is, I11 = S00 * is;            // S^-1
  const double L00 = -(I00 * T00 + I10 * T10), L01 = -(I00 * T01 + I10 * T11);   // -S^-1 T
  const double L10 = -(I10 * T00 + I11 * T10), L11 = -(I10 * T01 + I11 * T11);
  o[2][2] = I00; o[3][2] = o[2][3] = I10; o[3][3] = I11;
  o[2][0] = o[0][2] = L00; o[2][1] = o[1][2] = L01; o[3][0] = o[0][3] = L10; o[3][1] = o[1][3] = L11;
  o[0][0] = A00 - (T00 * L00 + T10 * L10);                                    // A^-1 + T' S^-1 T
  o[1][0] = o[0][1] = A10 - (T01 * L00 + T11 * L10);
  o[1][1] = A11 - (T01 * L01 + T11 * L11);
  return a > 0.0 && detA > 0.0 && S00 > 0.0 && detS > 0.0;
}

// lane-dependent pick of one of four values.  Scalars BY VALUE on purpose: with an array reference the optimiser turns
// the selects into a dynamically indexed load before inlining, and the array then lives in scratch memory.
__device__ __forceinline__ double sel4(double v0, double v1, double v2, double v3, int k) {
  const double lo = (k & 1) ? v1 : v0, hi = (k & 1) ? v3 : v2;
  return (k & 2) ? hi : lo;
}

}  // namespace f16
