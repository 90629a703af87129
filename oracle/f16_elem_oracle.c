/* f16_elem_oracle.c -- host restatements of the default build's elementary functions (checker only: tests/elem_cases.py).
 *
 *   f16o_sincos_bf        sincos_bf / sincos_bf_k of f16_mpc_oop_py_amd/csrc/f16_plant.hpp, operation by operation: rint, three fused
 *                         reduction steps, two Horner chains of fused steps, one product, two fused closing steps, the quadrant selects.
 *                         Every operation is correctly rounded, so the device must produce the SAME BITS (tests/test_gpu_elem.py).
 *                         Built with -ffp-contract=off: every fused operation is a written fma(), nothing else is fused.
 *   f16o_libm_sincos      the C library's sin and cos on the same arguments: the yardstick Y of the accuracy rule.
 *   f16o_rcp_newton       a MODEL of f16_rcp (hardware reciprocal + two Newton steps): the seed is 1 / x cut to 24 significant bits,
 *                         not the hardware's bits, so it is a stand-in for the budget and for showing that a dropped step trips the
 *                         rule -- never a reference for the device.
 *   f16o_atmos_fast       atmos_alt / atmos_air of the default build with the C library's exp and log standing in for the device's,
 *                         the exponent fraction a parameter: likewise a stand-in for the budget, never a reference.
 *
 * exp_k / log_k and f16_rcp start from the hardware reciprocal, whose bits no host has; they get no bit-exact restatement and are
 * judged against multiprecision values directly. */
#include <math.h>
#include <stdint.h>
#include <string.h>

/* The 21 constants of the pair, in the order of `struct SinCosK` (f16_plant.hpp: `constexpr SinCosK SINCOS_K = {...}`, the four
 * lines of literals below the struct): 2/pi; -pi/2 in three parts; S[8]; C[9].  tests/test_elem_cpu.py compares this table with the
 * header's text, literal by literal. */
#define F16O_SINCOS_CONSTANTS 21
static const double SINCOS_K[F16O_SINCOS_CONSTANTS] = {
    6.36619772367581382433e-01, -1.57079632679489655800e+00, -6.12323399573676603587e-17, 1.49738490485916983294e-33,
    -1.66666666666666657e-01, 8.33333333333333322e-03, -1.98412698412698413e-04, 2.75573192239858925e-06, -2.50521083854417202e-08,
    1.60590438368216133e-10, -7.64716373181981641e-13, 2.81145725434552060e-15,
    -5.00000000000000000e-01, 4.16666666666666644e-02, -1.38888888888888894e-03, 2.48015873015873016e-05, -2.75573192239858883e-07,
    2.08767569878681002e-09, -1.14707455977297245e-11, 4.77947733238738525e-14, -1.56192069685862253e-16};

int f16o_sincos_bf_constants(double *out) {
  memcpy(out, SINCOS_K, sizeof SINCOS_K);
  return F16O_SINCOS_CONSTANTS;
}

/* (int)n as the device converts it (v_cvt_i32_f64): saturating, NaN -> 0.  In C the conversion of a value outside int is undefined. */
static int to_int_saturating(double n) {
  if (n != n) return 0;
  if (n >= 2147483647.0) return INT32_MAX;
  if (n <= -2147483648.0) return INT32_MIN;
  return (int)n;
}

/* one argument, the table K given (tests perturb a copy of it to show that the rules notice) */
static void sincos_bf_one(const double *K, double x, double *sn, double *cs) {
  const double two_over_pi = K[0], *npio2 = K + 1, *S = K + 4, *C = K + 12;
  const double n = rint(x * two_over_pi);
  double r = fma(npio2[0], n, x);                /* (-(pi/2)_0) n + x: the product and the sum of fma(-n, (pi/2)_0, x), exactly */
  r = fma(npio2[1], n, r);
  r = fma(npio2[2], n, r);
  const double z = r * r;
  double p = S[7], q = C[8];
  for (int k = 6; k >= 0; --k) p = fma(p, z, S[k]);
  for (int k = 7; k >= 0; --k) q = fma(q, z, C[k]);
  const double s0 = fma(r * z, p, r), c0 = fma(z, q, 1.0);
  const int k = to_int_saturating(n) & 3;        /* sincos_quadrant */
  const double a = (k & 1) ? c0 : s0, b = (k & 1) ? s0 : c0;
  *sn = (k & 2) ? -a : a;
  *cs = ((k + 1) & 2) ? -b : b;
}

void f16o_sincos_bf_with(const double *K, const double *x, long n, double *sn, double *cs) {
  for (long i = 0; i < n; ++i) sincos_bf_one(K, x[i], sn + i, cs + i);
}

void f16o_sincos_bf(const double *x, long n, double *sn, double *cs) { f16o_sincos_bf_with(SINCOS_K, x, n, sn, cs); }

void f16o_libm_sincos(const double *x, long n, double *sn, double *cs) {
  for (long i = 0; i < n; ++i) { sn[i] = sin(x[i]); cs[i] = cos(x[i]); }
}

/* f16_rcp with `steps` Newton steps from a seed of 24 significant bits (the low 29 bits of 1 / x cleared) */
void f16o_rcp_newton(const double *x, long n, int steps, double *out) {
  for (long i = 0; i < n; ++i) {
    double r = 1.0 / x[i];
    uint64_t b;
    memcpy(&b, &r, 8);
    b &= ~(uint64_t)0x1fffffff;
    memcpy(&r, &b, 8);
    for (int k = 0; k < steps; ++k) r = fma(r, fma(-x[i], r, 1.0), r);
    out[i] = r;
  }
}

/* atmos_alt + atmos_air (f16_plant.hpp, F16_FAST_POW) in the contracted form of the default build: tfac is ONE fused operation, every
 * other operation a single product, quotient or root.  out [6][n]: tfac, factor, rho, mach, qbar, ps.  frac: the exponent the fast form
 * leaves to exp / log (POW_FRAC of the plant header). */
void f16o_atmos_fast(const double *alt, const double *vt, long n, double frac, double *out) {
  for (long i = 0; i < n; ++i) {
    const double tfac = fma(-.703e-5, alt[i], 1.0);
    double temp = 519.0 * tfac;
    if (alt[i] >= 35000.0) temp = 390;
    const double t2 = tfac * tfac, t4 = t2 * t2;
    const double pw = exp(frac * log(tfac));
    const double rho = 2.377e-3 * (t4 * pw);
    double ps = 1715.0 * rho * temp;
    if (ps == 0) ps = 1715;
    out[i] = tfac; out[n + i] = pw; out[2 * n + i] = rho;
    out[3 * n + i] = vt[i] / sqrt(1.4 * 1716.3 * temp);
    out[4 * n + i] = .5 * rho * (vt[i] * vt[i]);
    out[5 * n + i] = ps;
  }
}

/* trig_rotate of f16_plant.hpp: products and fused operations only, so the same bits as the device */
static void trig_rotate(double *s, double *c, double d) {
  const double d2 = d * d;
  const double sd = d * fma(d2, fma(d2, 1.0 / 120.0, -1.0 / 6.0), 1.0);
  const double cd = fma(d2, fma(d2, 1.0 / 24.0, -0.5), 1.0);
  const double s1 = fma(*c, sd, *s * cd), c1 = fma(-*s, sd, *c * cd);
  *s = s1; *c = c1;
}

/* The pairs a rollout carries (trig_exact at the start, then per step xn = xo + d and trig_advance's rotation by xn - xo and its verdict
 * !(|xn - xo| <= 4e-3) on ONE angle): in [1 + n_steps][n], out [n_steps][4][n] = sin, cos, angle, verdict -- the layout of
 * f16_debug_elem_trig_carry. */
void f16o_trig_carry(const double *in, int n_steps, long n, double *out) {
  for (long i = 0; i < n; ++i) {
    double a = in[i], s, c;
    sincos_bf_one(SINCOS_K, a, &s, &c);
    for (int k = 0; k < n_steps; ++k) {
      const double an = a + in[(long)(1 + k) * n + i], d = an - a;
      const double big = fmax(fabs(d), 0.0);       /* the other four increments are 0 */
      trig_rotate(&s, &c, d);
      a = an;
      double *o = out + (long)k * 4 * n + i;
      o[0] = s; o[n] = c; o[2 * n] = a; o[3 * n] = !(big <= 4e-3) ? 1.0 : 0.0;
    }
  }
}
