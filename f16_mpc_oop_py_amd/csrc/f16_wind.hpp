// f16_wind.hpp -- the plant in moving air (include/f16_hip.h: f16_xdot_wind_batch, f16_rollout_wind, f16_rollout_lqr_wind) and the
// gust sampler (f16_gust_sample), written once for the kernels of f16_wind.hip.
//
// The rule.  The states (V, alpha, beta) describe the velocity over the GROUND.  With w_ned the velocity of the air mass over the
// ground (north, east, down) and g_b a gust velocity in body axes, both held over a step:
//     (U, V, W)    = vt (ca cb, sb, sa cb)                            the ground velocity in body axes, vt clamped at 0.01
//     wb           = C(phi, theta, psi) w_ned                         body from NED, the sin / cos pairs plant_pre forms anyway
//     (Ua, Va, Wa) = (U, V, W) - wb - g_b
//     vt_a = sqrt(Ua^2 + Va^2 + Wa^2);  alpha_a = atan2(Wa, Ua);  beta_a = asin(Va / vt_a)
// The AIR triple feeds the lookups and the coefficient build-up (aero_totals), the atmosphere call (mach, qbar, ps) and the
// leading-edge-flap model; the GROUND triple stays in the navigation equations and in the force equations (U, V, W, vt, cb and the
// three quotients of xdot[6..8]) -- R V - Q W etc. on the ground velocity is the still-air force equation at the air velocity plus
// -omega x (wb + g_b), the body-axis derivative of a wind that is constant over the ground.  plant_moments is unchanged: it sees the
// air through qbar and the totals.  No derivative of the wind appears.  vt_a == 0 gives NaN by ordinary arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include "f16_plant.hpp"
#include "f16_mppi.hpp"

namespace f16 {

// The air triple of the rule above, alone: the statements calc_xdot_wind has always had, in their order (f16_debug_air_triple
// launches it on its own against a multiprecision reference, tests/test_gpu_air.py).  x[3..8] are read; w(k) as in calc_xdot_wind.
struct AirTriple { double Ua, Va, Wa, vt, alpha, beta; };
template <typename W>
F16_DEV void air_triple(const double *x, W w, AirTriple &a) {
  Trig5 g;
  trig_exact(x, g);
  double vt = x[6];
  if (vt <= 0.01) vt = 0.01;
  const double U = vt * g.ca * g.cb, V = vt * g.sb, W_ = vt * g.sa * g.cb;
  const double wn = w(0), we = w(1), wd = w(2);
  const double wbx = g.ct * g.cpsi * wn + g.ct * g.spsi * we - g.st * wd;
  const double wby = (g.sphi * g.st * g.cpsi - g.cphi * g.spsi) * wn + (g.sphi * g.st * g.spsi + g.cphi * g.cpsi) * we + g.sphi * g.ct * wd;
  const double wbz = (g.cphi * g.st * g.cpsi + g.sphi * g.spsi) * wn + (g.cphi * g.st * g.spsi - g.sphi * g.cpsi) * we + g.cphi * g.ct * wd;
  a.Ua = U - wbx - w(3); a.Va = V - wby - w(4); a.Wa = W_ - wbz - w(5);
  a.vt = sqrt(a.Ua * a.Ua + a.Va * a.Va + a.Wa * a.Wa);
  a.alpha = atan2(a.Wa, a.Ua);
  a.beta = asin(a.Va / a.vt);
}

// env.py:65-103 `_calc_xdot` in moving air.  w(k), k = 0..5: {wN, wE, wD, g_x, g_y, g_z} of the lane, read where they are used (the
// rollout kernels keep them in LDS slots).  The five sin / cos pairs are evaluated in front of the lookups, for the air triple, and
// AGAIN behind them by plant_pre: ten doubles carried across the lookups were what pushed the Runge-Kutta step (72 doubles of state
// and partial sums live across an evaluation) out of the register file.  The angles pass through an opaque move in between, or the
// compiler would merge the two evaluations and carry the pairs after all.
template <int FI = -1, typename TP, typename W>
F16_DEV void calc_xdot_wind(TP T, const double *__restrict__ LT, const double *x, const double *u, W w, double *xdot, double xcg, int fi_flag,
                            unsigned flags, int &status) {
  double xa[18];
#pragma unroll
  for (int k = 0; k < 18; ++k) xa[k] = x[k];
  {
    AirTriple a;
    air_triple(x, w, a);
    xa[6] = a.vt; xa[7] = a.alpha; xa[8] = a.beta;
  }
  Totals t;
  aero_totals<FI>(T, LT, xa, xcg, fi_flag, flags, t, status);
  // navigation and kinematics on the ground triple; the atmosphere at the air speed, clamped where the still-air code clamps vt
  double xg[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) xg[k] = x[k];
#pragma unroll
  for (int k = 3; k < 9; ++k) if (k != 6) asm volatile("" : "+v"(xg[k]));
  Pre p;
  plant_pre<false>(xg, p, xdot);
  atmos_dev(x[2], xa[6] <= 0.01 ? 0.01 : xa[6], p.mach, p.qbar, p.ps);
  plant_forces(x, p, t.Cx, t.Cy, t.Cz, xdot);
  plant_moments(x[9], x[10], x[11], p.qbar, t.Cl, t.Cm, t.Cn, xdot);
  actuators_dev(xa, u, p.qbar, p.ps, xdot);
}

// The classical Runge-Kutta step of rk4_step (f16_plant.hpp) over ANY derivative f(xs, xd): the same stage weights, the same sums in
// the same order, one copy of f in a loop that is not unrolled.  (rk4_step itself stays what it is: the existing kernels keep their
// instruction streams.)
template <typename F>
F16_DEV void rk4_step_with(double *x, double dt, F f) {
  const double h2 = 0.5 * dt, h6 = dt / 6.0;
  double xs[18], s1[18], s2[18];
#pragma unroll
  for (int k = 0; k < 18; ++k) { xs[k] = x[k]; s1[k] = 0; s2[k] = 0; }
#pragma unroll 1
  for (int s = 0; s < 4; ++s) {
    double xd[18];
    f(xs, xd);
    const double c = s == 2 ? dt : h2;
#pragma unroll
    for (int k = 0; k < 18; ++k) {
      if (s == 0) s1[k] = xd[k];
      else if (s == 1) s1[k] += 2.0 * xd[k];
      else if (s == 2) s2[k] = 2.0 * xd[k];
      else s2[k] += xd[k];
      xs[k] = x[k] + c * xd[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 18; ++k) x[k] += h6 * (s1[k] + s2[k]);
}

// One step of one aircraft in moving air, wind and gust held over it (over the four stages of the Runge-Kutta step, as the command is)
template <int STAGES, int FI = -1, typename TP, typename W>
F16_DEV void wind_step(TP T, const double *__restrict__ LT, double *x, const double *u, W w, double dt, double xcg,
                       int fi_flag, unsigned flags, int &status) {
  if constexpr (STAGES == 4) {
    rk4_step_with(x, dt, [&](const double *xs, double *xd) { calc_xdot_wind<FI>(T, LT, xs, u, w, xd, xcg, fi_flag, flags, status); });
  } else {
    double xd[18];
    calc_xdot_wind<FI>(T, LT, x, u, w, xd, xcg, fi_flag, flags, status);
#pragma unroll
    for (int k = 0; k < 18; ++k) x[k] += xd[k] * dt;   // env.py:126
  }
}

// The same step compiled OUT OF LINE, for the reason euler_step_exact and rk4_step_exact (f16_plant.hpp) are: under F16_FLAG_ONE_LANE
// every wind rollout steps through this one instruction sequence, so an aircraft's result does not depend on the batch size.
// tab: the fp64 table image through a generic pointer (global memory); xio[18] in / out, uin[4], win[6], *stio |= the grid bits.
template <int STAGES>
static __device__ __noinline__ void wind_step_exact(const double *tab, const double *lofi, double *xio, const double *uin, const double *win,
                                                    double dt, double xcg, int fi, unsigned flags, int *stio) {
  double x[18];
#pragma unroll
  for (int k = 0; k < 18; ++k) x[k] = xio[k];
  int st = 0;
  // (the command and the air are read from the caller's frame where an evaluation uses them: ten doubles less across the lookups)
  wind_step<STAGES, -1>(tab, lofi, x, uin, [&](int k) { return win[k]; }, dt, xcg, fi, flags, st);
#pragma unroll
  for (int k = 0; k < 18; ++k) xio[k] = x[k];
  *stio |= st;
}

// The gust sampler: per body axis i a first-order Gauss-Markov process  g_i(r) = (a_i * g_i(r-1)) + (b_i * n_i(r)),  every operation
// rounded on its own (no FMA contraction: numpy restates it), with (n_0, n_1, n_2) the three normals of f16_mppi_sample's rule
// (f16_mppi.hpp: mppi_sample_row) from the Philox counter (row, 0, 0xFFFFFFFF, aircraft), key = the two halves of the seed.  Counter
// word 2 is a value MPPI's sample index (< 256) never takes, so one seed serves both.
// ONE function, compiled OUT OF LINE, for f16_gust_sample and for the rollout kernels that generate their gusts in place: one
// instruction sequence whoever calls it, which is what makes the fused call's rows the stand-alone entry's bit for bit.
struct Gust3 { double v[3]; };
static __device__ __noinline__ Gust3 gust_row(uint32_t row, uint32_t aircraft, uint32_t key0, uint32_t key1, double a0, double a1, double a2,
                                              double b0, double b1, double b2, double g0, double g1, double g2) {
  const Philox4 p = philox4x32_10(row, 0u, 0xFFFFFFFFu, aircraft, key0, key1);
  constexpr double SCALE = 1.0 / 4294967296.0, TWO_PI = 6.283185307179586476925286766559;
  const double U0 = ((double)p.r[0] + 0.5) * SCALE, U1 = ((double)p.r[1] + 0.5) * SCALE;
  const double U2 = ((double)p.r[2] + 0.5) * SCALE, U3 = ((double)p.r[3] + 0.5) * SCALE;
  const double ra = sqrt(-2.0 * log(U0)), rb = sqrt(-2.0 * log(U2));
  double s1, c1;
  sincos(TWO_PI * U1, &s1, &c1);
  const double n[3] = {ra * c1, ra * s1, rb * cos(TWO_PI * U3)};
  const double a[3] = {a0, a1, a2}, b[3] = {b0, b1, b2}, g[3] = {g0, g1, g2};
  Gust3 o;
#pragma unroll
  for (int i = 0; i < 3; ++i) o.v[i] = __dadd_rn(__dmul_rn(a[i], g[i]), __dmul_rn(b[i], n[i]));
  return o;
}

}  // namespace f16
