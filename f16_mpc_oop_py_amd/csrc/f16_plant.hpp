// f16_plant.hpp -- device-side F-16 plant for gfx950: one wavefront lane = one aircraft.
//
// What it computes (same arithmetic, expression by expression, as the reference CPU path):
//   plant<>()      C/nlplant.c:23-457 Nlplant (hifi: C/hifi_F16_AeroData.c:1871-1934 group functions over
//                  C/mexndinterp.c:97-265 interpolation; lofi: C/lofi_F16_AeroData.c:12-368)
//   atmos_dev()    C/nlplant.c:467-490
//   actuators      utils.py:289-330 (upd_thrust/dstab/ail/rud/lef)
//   calc_xdot()    env.py:65-103          calc_xdot_na(): env.py:152-193
// How it differs structurally from the reference (results are unchanged):
//   * the 5 axis brackets (alpha on ALPHA1/ALPHA2, beta, el on DH1/DH2) are found once and shared by
//     all lookups; the reference searches them again inside each of its 58 interpn() calls;
//   * 58 interpn() calls collapse to 48 distinct evaluations on node-major table groups staged in LDS
//     (f16_tables.h); `_Cy` x4, `_Cn/_Cl(..,0)` x3 are evaluated once;
//   * an exact grid-node hit needs no special case: lambda is exactly 0 (or 1), and
//     lambda*f2 + (1-lambda)*f1 then returns f1 (or f2) exactly -- the value the reference's
//     degenerate-axis rule (mexndinterp.c:126-133,195-200) produces;
//   * no malloc, no file I/O, sin/cos evaluated once per angle (accels() re-evaluates the same
//     arguments, C/nlplant.c:525-545).
// Off-grid coordinates (UB in the reference) are clamped to the grid edge and flagged.
#pragma once
#include <hip/hip_runtime.h>

#include "f16_tables.h"

namespace f16 {

constexpr int ST_ALPHA1 = 1, ST_ALPHA2 = 2, ST_BETA = 4, ST_EL = 8, ST_ENVELOPE = 16, ST_NONFINITE = 32;
constexpr unsigned FLAG_FIX_CLR = 1u, FLAG_NO_ENVELOPE = 2u, FLAG_NO_CELL_CACHE = 16u;

#define F16_DEV __device__ __forceinline__

// Division by a compile-time constant.  Strict build: IEEE division as the reference does.  Default build
// (F16_FAST_DIV): multiplication by the correctly rounded reciprocal -- <= 1 ulp from the quotient, ~10 VALU
// instructions cheaper each (an fp64 division is a 10-deep dependent chain on gfx950).
#ifdef F16_FAST_DIV
#define F16_DIVC(x, c) ((x) * (1.0 / (c)))
#else
#define F16_DIVC(x, c) ((x) / (c))
#endif

// 1/x for a normal, finite x.  Strict build: IEEE division.  Default build: v_rcp_f64 + two Newton steps (<= 1 ulp of 1/x, held by
// tests/test_gpu_elem.py against multiprecision values over every normal exponent: 0.5 ulp measured up to 2^1022, 1 ulp above, where
// the reciprocal is a denormal; NaN for 0, denormals and infinities), 5 instructions instead of the ~15 of the division sequence.
__device__ __forceinline__ double f16_rcp(double x) {
#ifdef F16_FAST_DIV
  double r = __builtin_amdgcn_rcp(x);
  r = fma(r, fma(-x, r, 1.0), r);
  r = fma(r, fma(-x, r, 1.0), r);
  return r;
#else
  return 1.0 / x;
#endif
}

struct Axis {
  int j;       // lower node of the bracketing cell, 0 .. n-2
  double l;    // lambda = (v - X[j]) / (X[j+1] - X[j])     (mexndinterp.c:196)
  double m;    // 1 - lambda
};

F16_DEV double lerp(double f1, double f2, const Axis &a) { return a.l * f2 + a.m * f1; }  // mexndinterp.c:197

// fp64 FMAs pinned to the three-address form with ONE uniform (scalar-register) operand: the plain vector FMA, nothing else.
// Left to itself the compiler prefers the two-address v_fmac_f64 and copies the uniform value into a vector register first.
F16_DEV double fma_vvs(double a, double b, double c) {        // a * b + c, c uniform
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c));
  return d;
}
F16_DEV double fma_svv(double a, double b, double c) {        // a * b + c, a uniform
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "s"(a), "v"(b), "v"(c));
  return d;
}
F16_DEV double fma_vvv(double a, double b, double c) {        // the same instruction, same operand order, the uniform value in a vector register
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
// Where a caller of exp_k / log_k / sincos_bf_k holds the table (the operand class): KScalar -- scalar registers, the constant the
// scalar operand of the FMA; KVector -- lane-uniform vector registers (a role loop that has no scalar registers to spare keeps its
// table there for the whole launch: the FMA then issues with three vector operands, 6.1 cycles against 4.6 at one wave per SIMD).
struct KScalar {
  static F16_DEV double vvk(double a, double b, double k) { return fma_vvs(a, b, k); }
  static F16_DEV double kvv(double k, double b, double c) { return fma_svv(k, b, c); }
};
struct KVector {
  static F16_DEV double vvk(double a, double b, double k) { return fma_vvv(a, b, k); }
  static F16_DEV double kvv(double k, double b, double c) { return fma_vvv(k, b, c); }
};
// a value held in a vector register from here on: the copy is made here, once, and not in front of every use (a table kept across a
// loop: the Horner start coefficients, which are vector operands in either class; every entry under KVector)
F16_DEV void in_vgpr(double &x) { asm volatile("" : "+v"(x)); }
template <typename T>
F16_DEV void table_in_vgprs(T &t) {
  double *d = reinterpret_cast<double *>(&t);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / sizeof(double); ++i) in_vgpr(d[i]);
}

// ---- exp(POW_FRAC log tfac), POW_FRAC = 0.14 (below), of F16_FAST_POW with its constants as uniform values
// The device library's exp and log are inlined from bitcode, so their literals cannot be redirected; in the quad rollout they
// cost the atmosphere wave a register move (accumulation register, 64-bit copy or a pair of scalar moves) in front of almost
// every polynomial step.  exp_k / log_k repeat the library's operation sequence (ROCm device library, double-precision exp and
// log: frexp, an extended-precision quotient and sum for log; reduction by ln 2 in two parts and a degree-11 polynomial for
// exp), operation by operation, in the contracted form the compiler gives it in this build (-ffp-contract=fast: every product
// that feeds a sum is fused with it, also where the product has other uses).  Each such product-sum is WRITTEN as an fma here
// and no product feeds a plain sum, so nothing is left to contract.  tests/test_gpu_quad_constants.py holds the two
// compositions to the same bits.
struct PowK {
  double log2e, ln2_hi, ln2_lo, nln2_hi, nln2_lo, two_thirds;     // (ln 2 in two parts, and negated: exp's reduction)
  double E[10];                    // exp: e^r = 1 + r (1 + r (E9 + r (E8 + ... r E0))), highest degree first
  double L[7];                     // log: highest degree first
};
constexpr PowK POW_K = {
    1.44269504088896338700e+00, 6.93147180559945286227e-01, 2.31904681384629955842e-17, -6.93147180559945286227e-01,
    -2.31904681384629955842e-17, 6.66666666666666629659e-01,
    {2.50223225676461415e-08, 2.76309034901126543e-07, 2.75575145458253105e-06, 2.48014910390950412e-05, 1.98412695891155217e-04,
     1.38888889459163820e-03, 8.33333333345504315e-03, 4.16666666665197541e-02, 1.66666666666664770e-01, 5.00000000000001221e-01},
    {1.53670161652585818e-01, 1.52503063567000663e-01, 1.81863527724766383e-01, 2.22221384831011309e-01, 2.85714293974435540e-01,
     3.99999999961319630e-01, 6.66666666666728247e-01}};

// log_k in the two parts of its straight line (the quad rollout evaluates them in different halves of a step, f16_quad_steps.inc):
// log_k_quot -- mantissa, exponent and the extended-precision quotient (y - 1) / (y + 1); log_k_sum -- polynomial, the sums, the
// special arguments.
struct LogQuot {
  double h, l;                     // the quotient, high and low part
  int e;                           // exponent of the argument
};
template <typename OP = KScalar>
F16_DEV LogQuot log_k_quot(const PowK &K, double x) {
  const double m = __builtin_amdgcn_frexp_mant(x);
  const bool lo = m < K.two_thirds;
  const double sc = lo ? 2.0 : 1.0;
  const int e = __builtin_amdgcn_frexp_exp(x) + (lo ? -1 : 0);
  // y = m sc; (y - 1) / (y + 1) in two parts
  const double ym1 = fma(m, sc, -1.0), yp1 = fma(m, sc, 1.0);
  const double ylo = fma(m, sc, -(yp1 + -1.0));
  double r = __builtin_amdgcn_rcp(yp1);
  r = fma(fma(-yp1, r, 1.0), r, r);
  r = fma(fma(-yp1, r, 1.0), r, r);
  const double q = ym1 * r;
  const double p = yp1 * q;
  const double pl = fma(q, ylo, fma(q, yp1, -p));
  const double s25 = fma(yp1, q, pl);
  const double s27 = pl - fma(-yp1, q, s25);
  const double d28 = ym1 - s25;
  const double d32 = d28 + (((ym1 - d28) - s25) - s27);
  const double h = fma(r, d32, q);                         // quotient, high part
  const double l = fma(r, d32, -fma(-ym1, r, h));          // low part
  return {h, l, e};
}
// log_k_sum in its two parts: log_k_poly -- the square of the quotient and the Horner polynomial in it, which need the quotient alone
// (the quad rollout evaluates them with the quotient, half a step ahead); log_k_tail -- the sums and the special arguments.
struct LogPoly {
  double z, c;                     // h^2, the polynomial in it
};
template <typename OP = KScalar>
F16_DEV LogPoly log_k_poly(const PowK &K, const LogQuot &qt) {
  const double z = qt.h * qt.h;
  double c = OP::vvk(z, K.L[0], K.L[1]);
#pragma unroll
  for (int k = 2; k < 7; ++k) c = OP::vvk(z, c, K.L[k]);
  return {z, c};
}
template <typename OP = KScalar>
F16_DEV double log_k_tail(const PowK &K, double x, const LogQuot &qt, const LogPoly &pl);
template <typename OP = KScalar>
F16_DEV double log_k_sum(const PowK &K, double x, const LogQuot &qt) {
  return log_k_tail<OP>(K, x, qt, log_k_poly<OP>(K, qt));
}
template <typename OP>
F16_DEV double log_k_tail(const PowK &K, double x, const LogQuot &qt, const LogPoly &pl) {
  const double h = qt.h, l = qt.l;
  const int e = qt.e;
  const double z = pl.z, c = pl.c;
  const double a44 = __builtin_ldexp(h, 1), a45 = __builtin_ldexp(l, 1);
  const double t46 = h * z;
  const double u48 = fma(t46, c, a44);
  const double u50 = fma(t46, c, -(u48 - a44));
  const double u51 = a45 + u50;
  const double u52 = u48 + u51;
  const double u54 = u51 - (u52 - u48);
  // + e ln 2 in two parts
  const double f = (double)e;
  const double g56n = f * K.nln2_hi;
  const double g59 = OP::kvv(K.ln2_lo, f, OP::kvv(K.ln2_hi, f, g56n));
  const double g60 = OP::kvv(K.ln2_hi, f, g59);
  const double g62 = g59 - OP::kvv(K.nln2_hi, f, g60);
  const double w63 = g60 + u52;
  const double w64 = w63 - g60;
  const double w68 = (u52 - w64) + (g60 - (w63 - w64));
  const double v69 = g62 + u54;
  const double v70 = v69 - g62;
  const double v74 = (u54 - v70) + (g62 - (v69 - v70));
  const double k75 = v69 + w68;
  const double k76 = w63 + k75;
  const double k80 = k76 + (v74 + (k75 - (k76 - w63)));
  double res = __builtin_fabs(x) == __builtin_inf() ? x : k80;
  res = x < 0.0 ? __builtin_nan("") : res;
  return x == 0.0 ? -__builtin_inf() : res;
}
template <typename OP = KScalar>
F16_DEV double log_k(const PowK &K, double x) {
  return log_k_sum<OP>(K, x, log_k_quot<OP>(K, x));
}

template <typename OP = KScalar>
F16_DEV double exp_k(const PowK &K, double x) {
  const double n = rint(x * K.log2e);
  const double r = OP::kvv(K.nln2_lo, n, OP::kvv(K.nln2_hi, n, x));      // (as the library's fma(-n, ln2, x) compiles: sign on the constant)
  double c = OP::vvk(r, K.E[0], K.E[1]);
#pragma unroll
  for (int k = 2; k < 10; ++k) c = OP::vvk(r, c, K.E[k]);
  c = fma(r, c, 1.0);
  c = fma(r, c, 1.0);
  double res = __builtin_ldexp(c, (int)n);
  res = x > 1024.0 ? __builtin_inf() : res;
  return x < -1075.0 ? 0.0 : res;
}

// C/nlplant.c:467-490 in its two parts; pw(tfac) = exp(POW_FRAC log tfac) of the default build (below).
// The exponent the fast form leaves to exp / log, named once for its four users (atmos_dev, atmos_dev_k, the quad rollout's atmosphere
// role, the debug kernels).  The double 0.14 is not 4.14 - 4.0 (0.13999999999999968, exact): 4 + fl(0.14) lies 3.3e-16 above fl(4.14),
// the exponent of the reference's pow(tfac, 4.14), which moves the density by 3.3e-16 |log tfac| -- 2.7 x 2^-53 at 91,000 ft, nothing
// at sea level.  Measured on the device over [0, 1e5] ft (tests/test_gpu_elem.py): qbar within 7.4 x 2^-53 of the multiprecision
// .5 rho0 tfac^fl(4.14) vt^2 with 0.14, 4.3 with 4.14 - 4.0, both inside the rounding budget of 9 (tests/elem_cases.py); the constant
// therefore stays as every earlier result was computed with it.
constexpr double POW_FRAC = 0.14;
// (1) what the altitude alone decides: the quad rollout evaluates it half a step ahead of (2), f16_quad_steps.inc
struct AtmosAlt {
  double tfac, temp, t4;           // t4 = (tfac^2)^2, F16_FAST_POW only
};
F16_DEV AtmosAlt atmos_alt(double alt) {
  AtmosAlt h;
  h.tfac = 1 - .703e-5 * alt;
  h.temp = 519.0 * h.tfac;
  if (alt >= 35000.0) h.temp = 390;
#ifdef F16_FAST_POW
  // tfac^4.14 = (tfac^2)^2 * exp(POW_FRAC log tfac): |POW_FRAC log tfac| < 0.2 on the flight envelope keeps the exp-of-log
  // error below 1 ulp of tfac^POW_FRAC (measured 0.64); the squarings (1 and 3 roundings), the factor (<= 2) and two products on top
  // => the density within 7 x 2^-53 of rho0 tfac^4.14 in relative terms -- up to 7 ulp, not the 2 ulp once claimed here.
  // tests/elem_cases.py writes the budget out; tests/test_gpu_elem.py holds what the device returns of it, qbar and ps, to 9 and 10 x
  // 2^-53 (measured 7.4 and 7.1) and mach to 3.5 (2.3).
  const double t2 = h.tfac * h.tfac;
  h.t4 = t2 * t2;
#else
  h.t4 = 0;
#endif
  return h;
}
// (2) density, and with the airspeed mach, qbar, ps
template <typename PW>
F16_DEV void atmos_air(const AtmosAlt &h, double vt, double &mach, double &qbar, double &ps, PW pw) {
  const double rho0 = 2.377e-3;
#ifdef F16_FAST_POW
  const double rho = rho0 * (h.t4 * pw(h.tfac));
#else
  const double rho = rho0 * pow(h.tfac, 4.14);
#endif
  mach = vt / sqrt(1.4 * 1716.3 * h.temp);
  qbar = .5 * rho * (vt * vt);
  ps = 1715.0 * rho * h.temp;
  if (ps == 0) ps = 1715;
}
template <typename PW>
F16_DEV void atmos_with(double alt, double vt, double &mach, double &qbar, double &ps, PW pw) {
  atmos_air(atmos_alt(alt), vt, mach, qbar, ps, pw);
}
F16_DEV void atmos_dev(double alt, double vt, double &mach, double &qbar, double &ps) {
  atmos_with(alt, vt, mach, qbar, ps, [](double tfac) { return exp(POW_FRAC * log(tfac)); });
}
// the same with the constants of exp and log as uniform values (quad rollout)
F16_DEV void atmos_dev_k(const PowK &K, double alt, double vt, double &mach, double &qbar, double &ps) {
  atmos_with(alt, vt, mach, qbar, ps, [&K](double tfac) { return exp_k(K, POW_FRAC * log_k(K, tfac)); });
}


// The constants of the branch-free sin/cos pair below live in ONE table: sincos_bf folds them to literals, sincos_bf_k takes the same table as uniform values
// (scalar registers, loaded from QUAD_K below), so the two cannot drift.
struct SinCosK {
  double two_over_pi, npio2[3];    // 2/pi; -pi/2 in three parts, each a FULL double: the double nearest pi/2, nearest the rest, and again
  double S[8], C[9];               // sin: r + r z (S0 + S1 z + ...), cos: 1 + z (C0 + C1 z + ...), z = r^2
};
constexpr SinCosK SINCOS_K = {
    6.36619772367581382433e-01, {-1.57079632679489655800e+00, -6.12323399573676603587e-17, 1.49738490485916983294e-33},
    {-1.66666666666666657e-01, 8.33333333333333322e-03, -1.98412698412698413e-04, 2.75573192239858925e-06, -2.50521083854417202e-08, 1.60590438368216133e-10, -7.64716373181981641e-13, 2.81145725434552060e-15},
    {-5.00000000000000000e-01, 4.16666666666666644e-02, -1.38888888888888894e-03, 2.48015873015873016e-05, -2.75573192239858883e-07, 2.08767569878681002e-09, -1.14707455977297245e-11, 4.77947733238738525e-14, -1.56192069685862253e-16}};

// Both tables as ONE object in constant memory, for code that wants them in scalar registers.  Read at a constant offset the
// values fold back into literals; reloaded() hides the address (passed through a scalar register the compiler cannot see through), so
// that the values are LOADED -- by scalar loads, the address being uniform -- where the call stands, on every pass through it.
// The quad rollout calls it once per launch, in front of each role's step loop (f16_quad_steps.inc), and keeps the table in
// registers across the loop: no step loads it.  The scalar unit only reads here.
struct QuadK { SinCosK sc; PowK pw; };
static __constant__ const QuadK QUAD_K = {SINCOS_K, POW_K};
template <typename T>
F16_DEV T reloaded(const T &t) {
  static_assert(sizeof(T) % sizeof(double) == 0, "a table of doubles");
  unsigned long p = reinterpret_cast<unsigned long>(&t);
  asm volatile("" : "+s"(p));
  const __attribute__((address_space(4))) double *q = (const __attribute__((address_space(4))) double *)p;
  T k;
  double *d = reinterpret_cast<double *>(&k);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / sizeof(double); ++i) d[i] = q[i];
  return k;
}

#ifdef F16_FAST_TRIG
// Branch-free sin/cos pair: 3-part reduction by pi/2 in fused steps + Taylor polynomials on |r| <= pi/4 (coefficients are the
// exact 1/k! values; truncation < 5e-17).  The first step, fma(-n, fl(pi/2), x), is EXACT for every n: its result is a multiple of
// 2^-52 below 1.  The second rounds once, relative to the reduced argument, so nothing is lost where x lies next to a multiple of
// pi/2; the third part leaves n x 5.6e-50.  (Parts of 33 bits, as a reduction without fused steps needs them, left n x 1e-37: 3.4 ulp
// in the cosine of the double nearest 204,551 pi/2.)  Held by tests/test_gpu_elem.py, bit for bit against the checker's host
// restatement and through it against multiprecision values: within 1.3 ulp of the true value for |x| <= 1e6 (the test's
// bound: the C library's own error + 2 ulp) and measured within 1.1 ulp up to 3.3e9.  From |x| >= 2^31 pi/2 (3.37e9 rad) the quadrant
// comes from a saturated (int)n: the result is then a finite number in [-1, 1] unrelated to x, and nothing reports it -- phi, theta and
// psi have no envelope limit, the caller keeps them in range.  Unlike the libm call it contains no large-argument branch, so the
// five independent evaluations of a plant step sit in ONE basic block and the scheduler interleaves their dependency chains (the
// kernel is bound by fp64 dependent-issue latency at one wave per SIMD).
// quadrant selection shared by both forms
F16_DEV void sincos_quadrant(double n, double s0, double c0, double *sn, double *cs) {
  const int k = (int)n & 3;
  const double a = (k & 1) ? c0 : s0, b = (k & 1) ? s0 : c0;
  *sn = (k & 2) ? -a : a;
  *cs = ((k + 1) & 2) ? -b : b;
}

F16_DEV void sincos_bf(double x, double *sn, double *cs) {
  constexpr SinCosK K = SINCOS_K;
  const double n = rint(x * K.two_over_pi);
  double r = fma(-n, -K.npio2[0], x);
  r = fma(-n, -K.npio2[1], r);
  r = fma(-n, -K.npio2[2], r);
  const double z = r * r;
  double p = K.S[7], q = K.C[8];
#pragma unroll
  for (int k = 6; k >= 0; --k) p = fma(p, z, K.S[k]);
#pragma unroll
  for (int k = 7; k >= 0; --k) q = fma(q, z, K.C[k]);
  const double s0 = fma(r * z, p, r), c0 = fma(z, q, 1.0);
  sincos_quadrant(n, s0, c0, sn, cs);
}

// The same operations on the same operands in the same order, with every constant a UNIFORM value the caller holds in scalar
// registers (K: QUAD_K.sc below, defined from SINCOS_K).  As literals the 17 coefficients cost the quad rollout a
// 64-bit register move in front of every Horner step (the compiler prefers the two-address v_fmac_f64) and 28 vector registers
// for the table; an fp64 FMA whose addend is the scalar operand needs neither and issues faster (4.6 against 6.1 cycles at
// one wave per SIMD).  The FMA is pinned to its three-address form: it is the plain vector FMA, nothing else.
template <typename OP = KScalar>
F16_DEV void sincos_bf_k(const SinCosK &K, double x, double *sn, double *cs) {
  const double n = rint(x * K.two_over_pi);
  // (operand for operand what the compiler makes of fma(-n, C, r) with a literal C: (-C) n + r, the sign on the constant --
  //  on a NaN argument the sign of the result follows the operand that carries it)
  double r = OP::kvv(K.npio2[0], n, x);
  r = OP::kvv(K.npio2[1], n, r);
  r = OP::kvv(K.npio2[2], n, r);
  const double z = r * r;
  double p = K.S[7], q = K.C[8];
#pragma unroll
  for (int k = 6; k >= 0; --k) p = OP::vvk(p, z, K.S[k]);
#pragma unroll
  for (int k = 7; k >= 0; --k) q = OP::vvk(q, z, K.C[k]);
  const double s0 = fma(r * z, p, r), c0 = fma(z, q, 1.0);
  sincos_quadrant(n, s0, c0, sn, cs);
}
#define F16_SINCOS(x, s, c) sincos_bf(x, s, c)
#define F16_SINCOS_K(K, x, s, c) sincos_bf_k(K, x, s, c)
#define F16_SINCOS_KC(OP, K, x, s, c) sincos_bf_k<OP>(K, x, s, c)      // the table in the registers of operand class OP
#else
#define F16_SINCOS_KC(OP, K, x, s, c) sincos(x, s, c)
#define F16_SINCOS(x, s, c) sincos(x, s, c)
#define F16_SINCOS_K(K, x, s, c) sincos(x, s, c)
#endif

struct Aero {  // everything C/nlplant.c:185-240 (or :245-323) hands to the coefficient build-up
  double Cx, Cz, Cm, Cy, Cn, Cl;
  double Cxq, Cyr, Cyp, Czq, Clr, Clp, Cmq, Cnr, Cnp;
  double dCx_lef, dCz_lef, dCm_lef, dCy_lef, dCn_lef, dCl_lef;
  double dCxq_lef, dCyr_lef, dCyp_lef, dCzq_lef, dClr_lef, dClp_lef, dCmq_lef, dCnr_lef, dCnp_lef;
  double dCy_r30, dCn_r30, dCl_r30;
  double dCy_a20, dCy_a20_lef, dCn_a20, dCn_a20_lef, dCl_a20, dCl_a20_lef;
  double dCnbeta, dClbeta, dCm, eta_el;
};

// ---- hifi lookups: hifi_C, hifi_damping, hifi_C_lef, hifi_damping_lef, hifi_rudder, hifi_ailerons, hifi_other_coeffs
// (C/hifi_F16_AeroData.c:1871-1934) fused, in scheduling phases.  With one wavefront per SIMD nothing hides an LDS
// round trip, and left to itself the compiler emits lookups in source order (read four corners, wait, interpolate, next
// table: ~14 dependent round trips per role).  Here: (1) ALL breakpoint reads, (2) cell indices -> ALL table-corner
// reads, with the lambda divisions issued behind them, (3) the interpolation arithmetic.
//
// Bracketing v on breakpoints X[0..n-1] (monotone): `guess` must be within one cell of the true cell (the arithmetic
// guesses are exact up to a rounding at a node); the ends and the four breakpoints around the guess are read at once
// (one LDS round trip), the cell is then fixed up with compares and selects.
struct BrRaw { double lo, hi, xm, xg, xg1, xp; int g; };
template <typename TP>
F16_DEV BrRaw br_load(TP X, int n, int guess) {                 // the six breakpoint reads
  BrRaw r;
  r.g = min(max(guess, 0), n - 2);
  r.lo = X[0]; r.hi = X[n - 1];
  r.xm = X[max(r.g - 1, 0)]; r.xg = X[r.g]; r.xg1 = X[r.g + 1]; r.xp = X[min(r.g + 2, n - 1)];
  return r;
}
struct BrCell { int j; double v, x0, x1; };
F16_DEV BrCell br_cell(const BrRaw &r, int n, double v, bool &off) {   // clamp to the grid, cell fix-up
  off = !(v >= r.lo && v <= r.hi);
  v = fmin(fmax(v, r.lo), r.hi);
  const bool down = r.g > 0 && v < r.xg, up = r.g < n - 2 && v >= r.xg1;
  BrCell c;
  c.j = r.g - (down ? 1 : 0) + (up ? 1 : 0);
  c.v = v;
  c.x0 = down ? r.xm : (up ? r.xg1 : r.xg);
  c.x1 = down ? r.xg : (up ? r.xp : r.xg1);
  return c;
}
F16_DEV Axis br_axis(const BrCell &c) {                          // lambda = (v - X[j]) / (X[j+1] - X[j]), mexndinterp.c:196
  Axis a;
  a.j = c.j;
#ifdef F16_FAST_DIV
  // (the Newton-refined reciprocal is <= 1 ulp off 1/d, so d * rcp(d) need not be exactly 1: a hit on the LAST node of an
  //  axis -- the only node reached as the upper end of a cell -- is pinned, every other node gives lambda = 0 by itself)
  a.l = c.v == c.x1 ? 1.0 : (c.v - c.x0) * f16_rcp(c.x1 - c.x0);
#else
  a.l = (c.v - c.x0) / (c.x1 - c.x0);
#endif
  a.m = 1 - a.l;
  return a;
}
struct Q4 { double f00, f10, f01, f11; };                        // corners (a,b), (a+1,b), (a,b+1), (a+1,b+1)
template <typename TP>
F16_DEV Q4 ld4(TP p, int sa, int sb) { Q4 c; c.f00 = p[0]; c.f10 = p[sa]; c.f01 = p[sb]; c.f11 = p[sb + sa]; return c; }
F16_DEV double bil4(const Q4 &c, const Axis &a, const Axis &b) {   // alpha collapsed first, then beta (mexndinterp.c:178-209)
  return lerp(lerp(c.f00, c.f10, a), lerp(c.f01, c.f11, a), b);
}
// Default build: a bilinear interpolation as a weighted sum of the four corners.  The weights depend on the (alpha, beta)
// cell only, so the 31 bilinear evaluations of a plant call share two weight sets (ALPHA1 x BETA1, ALPHA2 x BETA1): four
// operations each instead of the six of the nested form, <= 2 ulp away from it, and still EXACT on a grid node (the
// weights are then 0 / 1).  F16_STRICT keeps the reference's nested form (mexndinterp.c:178-209).
struct W4 { double w00, w10, w01, w11; };
F16_DEV W4 bil_weights(const Axis &a, const Axis &b) { W4 w; w.w00 = a.m * b.m; w.w10 = a.l * b.m; w.w01 = a.m * b.l; w.w11 = a.l * b.l; return w; }
#ifdef F16_FAST_DIV
F16_DEV double bil4w(const Q4 &c, const Axis &, const Axis &, const W4 &w) { return w.w00 * c.f00 + w.w10 * c.f10 + w.w01 * c.f01 + w.w11 * c.f11; }
#else
F16_DEV double bil4w(const Q4 &c, const Axis &a, const Axis &b, const W4 &) { return bil4(c, a, b); }
#endif
#ifndef F16_PHASE_MASK
#define F16_PHASE_MASK 0x7        // LDS / memory instructions stay in their phase, ALU instructions may float (2 % over 0)
#endif
#define F16_PHASE() __builtin_amdgcn_sched_barrier(F16_PHASE_MASK)

F16_DEV int alpha_guess(double alpha) { return (int)((fmin(fmax(alpha, -20.0), 90.0) + 20.0) * 0.2); }
F16_DEV int beta_guess(double beta) {
  const double bc = fmin(fmax(beta, -30.0), 30.0);
  return bc < -10.0 ? (int)((bc + 30.0) * 0.2) : (bc < 10.0 ? 4 + (int)((bc + 10.0) * 0.5) : 14 + (int)((bc - 10.0) * 0.2));
}


// The six totals of C/nlplant.c:333-377 for ONE lane = one aircraft, in four load / compute phases whose live ranges
// stay inside the register file (written as one expression tree, all 168 vertex reads are hoisted to the top of
// the step and the allocator parks ~200 values in AGPRs: ~360 accvgpr moves per step, and a 512-lane workgroup spills
// to scratch).  Same terms, same differences-first order.  Measured at B = 262,144: 14.2 -> 15.8 G steps/s with 256-lane
// workgroups, 5.7 -> 17.1 with 512-lane ones (two waves per SIMD).
struct TotalsOut { double Cx, Cz, Cm, Cy, Cn, Cl; };

// Two table images serve the one-lane plant (f16_tables.h): fp64 values (TP = const double *) and scaled integers
// (TP = TabI32: half the LDS bytes per vertex, one exact int -> double conversion per vertex).  Lay<TP> gives the group
// offsets / node strides of the image and a view whose operator[] yields a double; with the integer image the lookups
// run on k = 1e5 x value and the six totals -- linear in the table values once eta_el is scaled -- are scaled at the end.
struct TabI32 { const int *base; };
struct I32View {
  const int *p;
  F16_DEV I32View operator+(int o) const { return I32View{p + o}; }
  F16_DEV double operator[](int i) const { return (double)p[i]; }
};
template <typename TP> struct Lay {
  static constexpr int G3A = OFF_G3A, SG3A = S_G3A, G3B = OFF_G3B, SG3B = S_G3B, G2A = OFF_G2A, SG2A = S_G2A, G2B = OFF_G2B,
                       SG2B = S_G2B, G1A = OFF_G1A, SG1A = S_G1A, G1B = OFF_G1B, SG1B = S_G1B, ETA = OFF_ETA;
  static constexpr bool SCALED = false;
  static F16_DEV TP tab(TP T) { return T; }
  static F16_DEV TP bp(TP T) { return T; }
};
template <> struct Lay<TabI32> {
  static constexpr int G3A = i32::OFF_G3A, SG3A = i32::S_G3A, G3B = i32::OFF_G3B, SG3B = i32::S_G3B, G2A = i32::OFF_G2A,
                       SG2A = i32::S_G2A, G2B = i32::OFF_G2B, SG2B = i32::S_G2B, G1A = i32::OFF_G1A, SG1A = i32::S_G1A,
                       G1B = i32::OFF_G1B, SG1B = i32::S_G1B, ETA = i32::OFF_ETA;
  static constexpr bool SCALED = true;
  static F16_DEV I32View tab(TabI32 T) { return I32View{T.base}; }
  static F16_DEV const double *bp(TabI32 T) { return reinterpret_cast<const double *>(T.base); }
};

template <typename TP>
F16_DEV void aero_totals_phased(TP T0, const double *xu, double xcg, unsigned flags, TotalsOut &t, int &status) {
  using L = Lay<TP>;
  const auto T = L::tab(T0);
  const auto BP = L::bp(T0);
  constexpr int S_G3A = L::SG3A, S_G3B = L::SG3B, S_G2A = L::SG2A, S_G2B = L::SG2B, S_G1A = L::SG1A, S_G1B = L::SG1B;
  constexpr int OFF_G3A = L::G3A, OFF_G3B = L::G3B, OFF_G2A = L::G2A, OFF_G2B = L::G2B, OFF_G1A = L::G1A, OFF_G1B = L::G1B,
                OFF_ETA = L::ETA;
  const double B = 30.0, cbar = 11.32, xcgr = 0.35, r2d = 180.0 / 3.141592653589793;
  double vt = xu[6];
  if (vt <= 0.01) vt = 0.01;
  const double alpha = xu[7] * r2d, beta = xu[8] * r2d, P = xu[9], Q = xu[10], R = xu[11], el = xu[13];
  const double dail = F16_DIVC(xu[14], 21.5), drud = F16_DIVC(xu[15], 30.0), dlef = 1 - F16_DIVC(xu[16], 25.0);
  const double r2vt = f16_rcp(2 * vt), kq = cbar * r2vt, kb = B * r2vt;
  // (1) breakpoints
  const BrRaw ra = br_load(BP + OFF_BP_A1, N_A1, alpha_guess(alpha));
  const BrRaw rb = br_load(BP + OFF_BP_B1, N_B1, beta_guess(beta));
  const BrRaw r1 = br_load(BP + OFF_BP_D1, N_D1, (el >= -10.0) + (el >= 0.0) + (el >= 10.0));
  const BrRaw r2 = br_load(BP + OFF_BP_D2, N_D2, (int)(el >= 0.0));
  const double a45 = BP[OFF_BP_A1 + N_A2 - 1];
  F16_PHASE();
  bool offa, offb, off1, off2;
  const BrCell ca = br_cell(ra, N_A1, alpha, offa), cb = br_cell(rb, N_B1, beta, offb);
  const BrCell c1 = br_cell(r1, N_D1, el, off1), c2 = br_cell(r2, N_D2, el, off2);
  if (offa) status |= ST_ALPHA1 | ST_ALPHA2;
  if (offb) status |= ST_BETA;
  if (off1) status |= ST_EL;
  const bool hi_a = ca.j > N_A2 - 2;
  if (hi_a && alpha > a45) status |= ST_ALPHA2;
  const int j2 = hi_a ? N_A2 - 2 : ca.j;
  const int n1 = cb.j * N_A1 + ca.j, n2 = cb.j * N_A2 + j2;
  const Axis a1 = br_axis(ca), b = br_axis(cb), d1 = br_axis(c1), d2 = br_axis(c2);
  Axis a2 = a1;
  if (hi_a) { a2.j = N_A2 - 2; a2.l = 1.0; a2.m = 0.0; }
  // (each weight set is formed inside the phase that uses it -- W1 twice, W2 in phase 4 only -- to keep live ranges short:
  //  the 512-lane workgroup has 256 registers per lane)
  const auto g = T + OFF_G1A + ca.j * S_G1A, h = T + OFF_G1B + j2 * S_G1B;
  // (2) longitudinal: G3A (3-D + el = 0 plane), G2B lef, pitch damping, eta_el
  {
    constexpr int SA = S_G3A, SB = S_G3A * N_A1, SD = S_G3A * N_A1 * N_B1;
    const auto p = T + OFF_G3A + n1 * SA;
    Q4 qlo[3], qhi[3], q0[3], ql[3];
    double g0[3], g1[3], h0[3], h1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      qlo[k] = ld4(p + k + c1.j * SD, SA, SB); qhi[k] = ld4(p + k + (c1.j + 1) * SD, SA, SB);
      q0[k] = ld4(p + k + D1_ZERO_NODE * SD, SA, SB);
      ql[k] = ld4(T + OFF_G2B + n2 * S_G2B + k, S_G2B, S_G2B * N_A2);
      g0[k] = g[3 * k]; g1[k] = g[S_G1A + 3 * k]; h0[k] = h[3 * k]; h1[k] = h[S_G1B + 3 * k];
    }
    const double m0 = g[11], m1 = g[S_G1A + 11], e0 = T[OFF_ETA + c1.j], e1 = T[OFF_ETA + c1.j + 1];
    F16_PHASE();
    const W4 W1 = bil_weights(a1, b);
    double Cf[3], dC[3], dQ[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Cf[k] = lerp(bil4w(qlo[k], a1, b, W1), bil4w(qhi[k], a1, b, W1), d1);
      dC[k] = bil4(ql[k], a2, b) - bil4w(q0[k], a1, b, W1);                            // hifi_C_lef
      const double Cq = lerp(g0[k], g1[k], a1), dq = lerp(h0[k], h1[k], a2);
      dQ[k] = kq * (Cq + (k == 1 ? dC[k] : dq) * dlef);                        // dXdQ, dZdQ (reference quirk :339), dMdQ
    }
    // same order of additions as C/nlplant.c:333-347
    t.Cx = Cf[0] + dC[0] * dlef + dQ[0] * Q;
    t.Cz = Cf[1] + dC[1] * dlef + dQ[1] * Q;
    t.Cm = Cf[2] * (L::SCALED ? i32::SCALE * lerp(e0, e1, d1) : lerp(e0, e1, d1)) + t.Cz * (xcgr - xcg) + dC[2] * dlef + dQ[2] * Q + lerp(m0, m1, a1);
  }
  F16_PHASE();
  // (3) lateral, first half: G3B (3-D + plane), G2A
  double base[3], base0[3], dr30[3], da20[3];
  {
    constexpr int SA3 = S_G3B, SB3 = S_G3B * N_A1, SD3 = S_G3B * N_A1 * N_B1;
    const auto p3 = T + OFF_G3B + n1 * SA3;
    Q4 qlo[2], qhi[2], q0[2], qa[7];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      qlo[k] = ld4(p3 + k + c2.j * SD3, SA3, SB3); qhi[k] = ld4(p3 + k + (c2.j + 1) * SD3, SA3, SB3);
      q0[k] = ld4(p3 + k + D2_ZERO_NODE * SD3, SA3, SB3);
    }
    const auto pa = T + OFF_G2A + n1 * S_G2A;
#pragma unroll
    for (int k = 0; k < 7; ++k) qa[k] = ld4(pa + k, S_G2A, S_G2A * N_A1);
    F16_PHASE();
    const W4 W1 = bil_weights(a1, b);
    const double Cy = bil4w(qa[0], a1, b, W1);
    base[0] = Cy; base0[0] = Cy;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      base[k + 1] = lerp(bil4w(qlo[k], a1, b, W1), bil4w(qhi[k], a1, b, W1), d2);
      base0[k + 1] = bil4w(q0[k], a1, b, W1);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      dr30[k] = bil4w(qa[1 + k], a1, b, W1) - base0[k];                              // hifi_rudder
      da20[k] = bil4w(qa[4 + k], a1, b, W1) - base0[k];                              // hifi_ailerons
    }
  }
  F16_PHASE();
  // (4) lateral, second half: G2B lef tables, yaw / roll damping, sideslip corrections
  {
    const auto pb = T + OFF_G2B + n2 * S_G2B;
    Q4 ql[3], qal[3];
    double r0[3], r1v[3], p0[3], p1[3], hr0[3], hr1[3], hp0[3], hp1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ql[k] = ld4(pb + 3 + k, S_G2B, S_G2B * N_A2); qal[k] = ld4(pb + 6 + k, S_G2B, S_G2B * N_A2);
      const int ir = k == 0 ? 1 : (k == 1 ? 7 : 4);
      r0[k] = g[ir]; r1v[k] = g[S_G1A + ir]; p0[k] = g[ir + 1]; p1[k] = g[S_G1A + ir + 1];
      hr0[k] = h[ir]; hr1[k] = h[S_G1B + ir]; hp0[k] = h[ir + 1]; hp1[k] = h[S_G1B + ir + 1];
    }
    const double nb0 = g[9], nb1 = g[S_G1A + 9], lb0 = g[10], lb1 = g[S_G1A + 10];
    F16_PHASE();
    const W4 W2 = bil_weights(a2, b);
    double dl[3], dA[3], dR[3], dP[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double Clef = bil4w(ql[k], a2, b, W2), Ca20lef = bil4w(qal[k], a2, b, W2);
      double Cr = lerp(r0[k], r1v[k], a1);
      if (k == 2 && !(flags & FLAG_FIX_CLR)) Cr = 0.0;                          // reference defect: _CLr never loaded
      const double Cp = lerp(p0[k], p1[k], a1), dCr = lerp(hr0[k], hr1[k], a2), dCp = lerp(hp0[k], hp1[k], a2);
      dl[k] = Clef - base0[k];                                                  // hifi_C_lef
      dA[k] = da20[k] + (Ca20lef - Clef - da20[k]) * dlef;                      // dYdail, dNdail, dLdail
      dR[k] = kb * (Cr + dCr * dlef);
      dP[k] = kb * (Cp + dCp * dlef);
    }
    // same order of additions as C/nlplant.c:353-377
    t.Cy = base[0] + dl[0] * dlef + dA[0] * dail + dr30[0] * drud + dR[0] * R + dP[0] * P;
    t.Cn = base[1] + dl[1] * dlef - t.Cy * (xcgr - xcg) * (cbar / B) + dA[1] * dail + dr30[1] * drud + dR[1] * R + dP[1] * P +
           lerp(nb0, nb1, a1) * beta;
    t.Cl = base[2] + dl[2] * dlef + dA[2] * dail + dr30[2] * drud + dR[2] * R + dP[2] * P + lerp(lb0, lb1, a1) * beta;
  }
  if (L::SCALED) { t.Cx *= i32::SCALE; t.Cz *= i32::SCALE; t.Cm *= i32::SCALE; t.Cy *= i32::SCALE; t.Cn *= i32::SCALE; t.Cl *= i32::SCALE; }
}

// The same totals as sums of four partial triples, so that four wavefronts can each look up one table family
// (k_rollout_4w), every part in load / compute phases:
//   PART 1  longitudinal, 3-D / 2-D tables  {Cx, Cz, Cm}_s        PART 3  longitudinal damping (1-D)  {Cx, Cz, Cm}_d
//   PART 2  lateral, 3-D / 2-D tables       {Cy, Cn, Cl}_s        PART 4  lateral damping (1-D)       {Cy, Cn, Cl}_d
// compose_totals() adds them and applies the cg-offset couplings of C/nlplant.c:347,367.  The terms are exactly those
// of C/nlplant.c:333-377; only the order of the additions differs from the single-expression form (ulp level).
template <int PART, typename TP>
F16_DEV void aero_part(TP T, const double *xu, unsigned flags, double *out, int &status) {
  const double B = 30.0, cbar = 11.32, r2d = 180.0 / 3.141592653589793;
  double vt = xu[6];
  if (vt <= 0.01) vt = 0.01;
  const double alpha = xu[7] * r2d, beta = xu[8] * r2d, P = xu[9], Q = xu[10], R = xu[11], el = xu[13];
  const double dail = F16_DIVC(xu[14], 21.5), drud = F16_DIVC(xu[15], 30.0), dlef = 1 - F16_DIVC(xu[16], 25.0);
  const double r2vt = f16_rcp(2 * vt), kq = cbar * r2vt, kb = B * r2vt;
  constexpr bool TWO_D = PART == 1 || PART == 2;                 // needs beta (and an elevator axis)
  // (1) breakpoints
  const BrRaw ra = br_load(T + OFF_BP_A1, N_A1, alpha_guess(alpha));
  const double a45 = T[OFF_BP_A1 + N_A2 - 1];
  BrRaw rb = ra, rd = ra;
  if (TWO_D) {
    rb = br_load(T + OFF_BP_B1, N_B1, beta_guess(beta));
    rd = PART == 1 ? br_load(T + OFF_BP_D1, N_D1, (el >= -10.0) + (el >= 0.0) + (el >= 10.0))
                   : br_load(T + OFF_BP_D2, N_D2, (int)(el >= 0.0));
  }
  F16_PHASE();
  bool offa, offb = false, offd = false;
  const BrCell ca = br_cell(ra, N_A1, alpha, offa);
  BrCell cb = ca, cd = ca;
  if (TWO_D) { cb = br_cell(rb, N_B1, beta, offb); cd = br_cell(rd, PART == 1 ? N_D1 : N_D2, el, offd); }
  if (offa) status |= ST_ALPHA1 | ST_ALPHA2;
  if (offb) status |= ST_BETA;
  if (offd) status |= ST_EL;
  const bool hi_a = ca.j > N_A2 - 2;
  if (hi_a && alpha > a45) status |= ST_ALPHA2;
  const int j2 = hi_a ? N_A2 - 2 : ca.j;
  const int n1 = cb.j * N_A1 + ca.j, n2 = cb.j * N_A2 + j2;
  TP g = T + OFF_G1A + ca.j * S_G1A, h = T + OFF_G1B + j2 * S_G1B;
  if (PART == 1) {
    constexpr int SA = S_G3A, SB = S_G3A * N_A1, SD = S_G3A * N_A1 * N_B1;
    TP p = T + OFF_G3A + n1 * SA;
    Q4 qlo[3], qhi[3], q0[3], ql[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      qlo[k] = ld4(p + k + cd.j * SD, SA, SB); qhi[k] = ld4(p + k + (cd.j + 1) * SD, SA, SB);
      q0[k] = ld4(p + k + D1_ZERO_NODE * SD, SA, SB);
      ql[k] = ld4(T + OFF_G2B + n2 * S_G2B + k, S_G2B, S_G2B * N_A2);
    }
    const double e0 = T[OFF_ETA + cd.j], e1 = T[OFF_ETA + cd.j + 1];
    F16_PHASE();
    const Axis a1 = br_axis(ca), b = br_axis(cb), d1 = br_axis(cd);
    Axis a2 = a1;
    if (hi_a) { a2.j = N_A2 - 2; a2.l = 1.0; a2.m = 0.0; }
    const W4 W1 = bil_weights(a1, b), W2 = bil_weights(a2, b);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double Cf = lerp(bil4w(qlo[k], a1, b, W1), bil4w(qhi[k], a1, b, W1), d1);
      const double dC = bil4w(ql[k], a2, b, W2) - bil4w(q0[k], a1, b, W1);             // hifi_C_lef :1892-1899
      out[k] = (k == 2 ? Cf * lerp(e0, e1, d1) : Cf) + dC * dlef + (k == 1 ? kq * (dC * dlef) * Q : 0.0);   // dZdQ quirk
    }
  } else if (PART == 3) {
    double g0[3], g1[3], h0[3], h1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { g0[k] = g[3 * k]; g1[k] = g[S_G1A + 3 * k]; h0[k] = h[3 * k]; h1[k] = h[S_G1B + 3 * k]; }
    const double m0 = g[11], m1 = g[S_G1A + 11];
    F16_PHASE();
    const Axis a1 = br_axis(ca);
    Axis a2 = a1;
    if (hi_a) { a2.j = N_A2 - 2; a2.l = 1.0; a2.m = 0.0; }
    out[0] = kq * (lerp(g0[0], g1[0], a1) + lerp(h0[0], h1[0], a2) * dlef) * Q;
    out[1] = kq * lerp(g0[1], g1[1], a1) * Q;
    out[2] = kq * (lerp(g0[2], g1[2], a1) + lerp(h0[2], h1[2], a2) * dlef) * Q + lerp(m0, m1, a1);
  } else if (PART == 2) {
    constexpr int SA3 = S_G3B, SB3 = S_G3B * N_A1, SD3 = S_G3B * N_A1 * N_B1;
    TP p3 = T + OFF_G3B + n1 * SA3;
    Q4 qlo[2], qhi[2], q0[2], qa[7];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      qlo[k] = ld4(p3 + k + cd.j * SD3, SA3, SB3); qhi[k] = ld4(p3 + k + (cd.j + 1) * SD3, SA3, SB3);
      q0[k] = ld4(p3 + k + D2_ZERO_NODE * SD3, SA3, SB3);
    }
    TP pa = T + OFF_G2A + n1 * S_G2A;
#pragma unroll
    for (int k = 0; k < 7; ++k) qa[k] = ld4(pa + k, S_G2A, S_G2A * N_A1);
    F16_PHASE();
    const Axis a1 = br_axis(ca), b = br_axis(cb), d2 = br_axis(cd);
    Axis a2 = a1;
    if (hi_a) { a2.j = N_A2 - 2; a2.l = 1.0; a2.m = 0.0; }
    const W4 W1 = bil_weights(a1, b), W2 = bil_weights(a2, b);
    double base[3], base0[3], dr30[3], da20[3];
    base[0] = base0[0] = bil4w(qa[0], a1, b, W1);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      base[k + 1] = lerp(bil4w(qlo[k], a1, b, W1), bil4w(qhi[k], a1, b, W1), d2);
      base0[k + 1] = bil4w(q0[k], a1, b, W1);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { dr30[k] = bil4w(qa[1 + k], a1, b, W1) - base0[k]; da20[k] = bil4w(qa[4 + k], a1, b, W1) - base0[k]; }
    F16_PHASE();
    TP pb = T + OFF_G2B + n2 * S_G2B;
    Q4 ql[3], qal[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ql[k] = ld4(pb + 3 + k, S_G2B, S_G2B * N_A2); qal[k] = ld4(pb + 6 + k, S_G2B, S_G2B * N_A2); }
    F16_PHASE();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double Clef = bil4w(ql[k], a2, b, W2), Ca20lef = bil4w(qal[k], a2, b, W2);
      out[k] = base[k] + (Clef - base0[k]) * dlef + (da20[k] + (Ca20lef - Clef - da20[k]) * dlef) * dail + dr30[k] * drud;
    }
  } else {
    double r0[3], r1v[3], p0[3], p1[3], hr0[3], hr1[3], hp0[3], hp1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int ir = k == 0 ? 1 : (k == 1 ? 7 : 4);
      r0[k] = g[ir]; r1v[k] = g[S_G1A + ir]; p0[k] = g[ir + 1]; p1[k] = g[S_G1A + ir + 1];
      hr0[k] = h[ir]; hr1[k] = h[S_G1B + ir]; hp0[k] = h[ir + 1]; hp1[k] = h[S_G1B + ir + 1];
    }
    const double nb0 = g[9], nb1 = g[S_G1A + 9], lb0 = g[10], lb1 = g[S_G1A + 10];
    F16_PHASE();
    const Axis a1 = br_axis(ca);
    Axis a2 = a1;
    if (hi_a) { a2.j = N_A2 - 2; a2.l = 1.0; a2.m = 0.0; }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double Cr = lerp(r0[k], r1v[k], a1);
      if (k == 2 && !(flags & FLAG_FIX_CLR)) Cr = 0.0;                          // reference defect: _CLr never loaded
      out[k] = kb * (Cr + lerp(hr0[k], hr1[k], a2) * dlef) * R + kb * (lerp(p0[k], p1[k], a1) + lerp(hp0[k], hp1[k], a2) * dlef) * P;
    }
    out[1] += lerp(nb0, nb1, a1) * beta;
    out[2] += lerp(lb0, lb1, a1) * beta;
  }
}

// ---- lofi (C/lofi_F16_AeroData.c), tables in global/constant memory ---------------------------
F16_DEV int sgn_i(double v) { return (v > 0) - (v < 0); }
F16_DEV int fix_i(double v) { return (int)trunc(v); }

struct LofiAlpha { int k, L; double da; };
F16_DEV LofiAlpha lofi_alpha(double alpha) {   // :31-45
  const double s = .2 * alpha;
  int k = fix_i(s);
  if (k <= -2) k = -1; else if (k >= 9) k = 8;
  LofiAlpha r;
  r.da = s - k;
  r.L = k + fix_i(1.1 * sgn_i(r.da)) + 3;
  r.k = k + 3;
  return r;
}
F16_DEV double lofi_bilin(const double *T, int m, int n, const LofiAlpha &a, double db) {
  const double t = T[(m - 1) * 12 + a.k - 1], u = T[(n - 1) * 12 + a.k - 1];
  const double v = t + fabs(a.da) * (T[(m - 1) * 12 + a.L - 1] - t);
  const double w = u + fabs(a.da) * (T[(n - 1) * 12 + a.L - 1] - u);
  return v + (w - v) * db;
}

F16_DEV void aero_lofi(const double *__restrict__ LT, double alpha, double beta, double el, double dail, double drud,
                       Aero &c, int &status) {
  // Beyond alpha -10 / 45 deg and beyond the elevator rows the reference EXTRAPOLATES along the last cell (k held at -1 / 8,
  // "bounds of table for extrapolation", :33-38; m held at -1 / 1, :303-308) with every index inside its array: defined
  // behaviour, restated as it is, no status bit (k, L and m, n stay inside 1..12 and 1..5 for any input, NaN included).
  // Only the beta rows of dmomdcon are read past their 7-row tables (:141-150), where fix(0.2 |beta|) >= 6: the row index is
  // held at 7 and F16_ST_BETA is raised there, on the reference's own index (the product rounds to 6.0 one double below 30 deg
  // already, so a test on beta itself would miss that value).  A NaN beta raises the bit as well.
  const LofiAlpha a = lofi_alpha(alpha);
  {  // damping :12-56
    const double *A = LT + LOFI_DAMP;
    double d[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] = A[i * 12 + a.k - 1] + fabs(a.da) * (A[i * 12 + a.L - 1] - A[i * 12 + a.k - 1]);
    c.Cxq = d[0]; c.Cyr = d[1]; c.Cyp = d[2]; c.Czq = d[3]; c.Clr = d[4]; c.Clp = d[5]; c.Cmq = d[6]; c.Cnr = d[7]; c.Cnp = d[8];
  }
  {  // dmomdcon :59-183
    const double s = 0.2 * fabs(beta);
    int m = fix_i(s);
    if (m >= 7) m = 6;
    const double db = s - m;
    int n = m + 1;
    m = m + 1; n = n + 1;
    if (n > 7) { n = 7; status |= ST_BETA; }
    if (beta != beta) status |= ST_BETA;
    c.dCl_a20 = lofi_bilin(LT + LOFI_DLDA, m, n, a, db);
    c.dCl_r30 = lofi_bilin(LT + LOFI_DLDR, m, n, a, db);
    c.dCn_a20 = lofi_bilin(LT + LOFI_DNDA, m, n, a, db);
    c.dCn_r30 = lofi_bilin(LT + LOFI_DNDR, m, n, a, db);
  }
  {  // clcn :185-262
    const double s = .2 * fabs(beta);
    int m = fix_i(s);
    if (m == 0) m = 1; else if (m >= 6) m = 5;
    const double db = s - m;
    int n = m + fix_i(1.1 * sgn_i(db));
    m = m + 1; n = n + 1;
    c.Cl = lofi_bilin(LT + LOFI_CL, m, n, a, fabs(db)) * sgn_i(beta);
    c.Cn = lofi_bilin(LT + LOFI_CN, m, n, a, fabs(db)) * sgn_i(beta);
  }
  {  // cxcm :265-336
    const double s = el / 12.0;
    int m = fix_i(s);
    if (m <= -2) m = -1; else if (m >= 2) m = 1;
    const double de = s - m;
    int n = m + fix_i(1.1 * sgn_i(de));
    m = m + 3; n = n + 3;
    n = min(max(n, 1), 5);
    c.Cx = lofi_bilin(LT + LOFI_CX, m, n, a, fabs(de));
    c.Cm = lofi_bilin(LT + LOFI_CM, m, n, a, fabs(de));
  }
  c.Cy = -.02 * beta + .021 * dail + .086 * drud;   // nlplant.c:283
  {  // cz :339-368
    const double *A = LT + LOFI_CZ;
    const double s = A[a.k - 1] + fabs(a.da) * (A[a.L - 1] - A[a.k - 1]);
    const double b573 = beta / 57.3;
    c.Cz = s * (1 - b573 * b573) - .19 * (el) / 25;
  }
  // nlplant.c:295-319
  c.dCx_lef = c.dCz_lef = c.dCm_lef = c.dCy_lef = c.dCn_lef = c.dCl_lef = 0.0;
  c.dCxq_lef = c.dCyr_lef = c.dCyp_lef = c.dCzq_lef = c.dClr_lef = c.dClp_lef = c.dCmq_lef = c.dCnr_lef = c.dCnp_lef = 0.0;
  c.dCy_r30 = c.dCy_a20 = c.dCy_a20_lef = c.dCn_a20_lef = c.dCl_a20_lef = 0.0;
  c.dCnbeta = c.dClbeta = c.dCm = 0.0;
  c.eta_el = 1.0;
}

// ---- C/nlplant.c:23-457 in three pieces ------------------------------------------------------------------------
// (the single-wave kernels run them back to back; k_rollout_4w spreads them over four wavefronts, see f16_dynamics.hip)
struct Totals { double Cx, Cz, Cm, Cy, Cn, Cl; };   // C*_tot of C/nlplant.c:333-377
struct Pre {                                        // trigonometry, atmosphere, body velocities
  double sa, ca, sb, cb, st, ct, sphi, cphi;
  double U, V, W, vt, mach, qbar, ps;
};

// Table lookups + coefficient build-up (C/nlplant.c:183-377).  Needs xu[6..11], xu[13..16] only.
// FI: 1 / 0 = fidelity fixed at compile time, -1 = decided by fi_flag at run time.
// hifi: the phased lookups above; lofi: Stevens & Lewis tables + the same totals with every lef term zero (:295-319).
template <int FI = -1, typename TP>
F16_DEV void aero_totals(TP T, const double *__restrict__ LT, const double *xu, double xcg, int fi_flag, unsigned flags,
                         Totals &t, int &status) {
  const bool hifi = FI < 0 ? fi_flag == 1 : FI == 1;
  if (hifi) {
    TotalsOut o;
    aero_totals_phased(T, xu, xcg, flags, o, status);
    t.Cx = o.Cx; t.Cz = o.Cz; t.Cm = o.Cm; t.Cy = o.Cy; t.Cn = o.Cn; t.Cl = o.Cl;
    return;
  }
  const double B = 30.0, cbar = 11.32, xcgr = 0.35;
  const double r2d = 180.0 / 3.141592653589793;   // 180.0/acos(-1)
  double vt = xu[6];
  const double alpha = xu[7] * r2d, beta = xu[8] * r2d;
  const double P = xu[9], Q = xu[10], R = xu[11];
  if (vt <= 0.01) vt = 0.01;
  const double el = xu[13], ail = xu[14], rud = xu[15];
  const double dail = F16_DIVC(ail, 21.5);
  const double drud = F16_DIVC(rud, 30.0);
  const double dlef = 0.0;
  Aero c;
  aero_lofi(LT, alpha, beta, el, dail, drud, c, status);
  // totals, C/nlplant.c:333-377 (dZdQ uses delta_Cz_lef, as the reference does)
#ifdef F16_FAST_DIV
  const double r2vt = 1.0 / (2 * vt);
  const double kq = cbar * r2vt, kb = B * r2vt;       // cbar/(2 vt), B/(2 vt) off one reciprocal
#else
  const double kq = cbar / (2 * vt), kb = B / (2 * vt);
#endif
  const double dXdQ = kq * (c.Cxq + c.dCxq_lef * dlef);
  t.Cx = c.Cx + c.dCx_lef * dlef + dXdQ * Q;
  const double dZdQ = kq * (c.Czq + c.dCz_lef * dlef);
  t.Cz = c.Cz + c.dCz_lef * dlef + dZdQ * Q;
  const double dMdQ = kq * (c.Cmq + c.dCmq_lef * dlef);
  t.Cm = c.Cm * c.eta_el + t.Cz * (xcgr - xcg) + c.dCm_lef * dlef + dMdQ * Q + c.dCm;
  const double dYdail = c.dCy_a20 + c.dCy_a20_lef * dlef;
  const double dYdR = kb * (c.Cyr + c.dCyr_lef * dlef);
  const double dYdP = kb * (c.Cyp + c.dCyp_lef * dlef);
  t.Cy = c.Cy + c.dCy_lef * dlef + dYdail * dail + c.dCy_r30 * drud + dYdR * R + dYdP * P;
  const double dNdail = c.dCn_a20 + c.dCn_a20_lef * dlef;
  const double dNdR = kb * (c.Cnr + c.dCnr_lef * dlef);
  const double dNdP = kb * (c.Cnp + c.dCnp_lef * dlef);
  t.Cn = c.Cn + c.dCn_lef * dlef - t.Cy * (xcgr - xcg) * (cbar / B) + dNdail * dail + c.dCn_r30 * drud + dNdR * R + dNdP * P +
         c.dCnbeta * beta;
  const double dLdail = c.dCl_a20 + c.dCl_a20_lef * dlef;
  const double dLdR = kb * (c.Clr + c.dClr_lef * dlef);
  const double dLdP = kb * (c.Clp + c.dClp_lef * dlef);
  t.Cl = c.Cl + c.dCl_lef * dlef + dLdail * dail + c.dCl_r30 * drud + dLdR * R + dLdP * P + c.dClbeta * beta;
}


F16_DEV void compose_totals(const double *ls, const double *ld, const double *ts, const double *td, double xcg, Totals &t) {
  const double B = 30.0, cbar = 11.32, xcgr = 0.35;
  t.Cx = ls[0] + ld[0];
  t.Cz = ls[1] + ld[1];
  t.Cm = ls[2] + ld[2] + t.Cz * (xcgr - xcg);
  t.Cy = ts[0] + td[0];
  t.Cn = ts[1] + td[1] - t.Cy * (xcgr - xcg) * (cbar / B);
  t.Cl = ts[2] + td[2];
}

// Trigonometry, atmosphere, navigation + kinematic equations (C/nlplant.c:90-176): xdot[0..5].
// sin / cos of alpha, beta, theta, phi, psi handed in by a caller that keeps them up to date itself (rollout kernels: trig_advance)
struct Trig5 { double sa, ca, sb, cb, st, ct, sphi, cphi, spsi, cpsi; };
F16_DEV void trig_exact(const double *x, Trig5 &g) {
  F16_SINCOS(x[7], &g.sa, &g.ca);
  F16_SINCOS(x[8], &g.sb, &g.cb);
  F16_SINCOS(x[4], &g.st, &g.ct);
  F16_SINCOS(x[3], &g.sphi, &g.cphi);
  F16_SINCOS(x[5], &g.spsi, &g.cpsi);
}
// (sin, cos)(a + d) from (sin, cos)(a) by the angle-sum formulas with sin d, cos d from their series: for |d| <= 4e-3 rad (an Euler
// step of 1 ms moves an angle by |rate| x 1e-3) the terms dropped are d^7 / 5040 < 4e-21 and d^6 / 720 < 6e-18.  11 operations per
// angle against ~42 for the full evaluation (range reduction, two polynomials, quadrant selects).  With its roundings a rotation adds
// at most 1.6 x 2^-53 to the error of s and of c (the budget written out in tests/elem_cases.py; tests/test_gpu_elem.py holds the
// pairs to it over 1, 31 and 32 rotations against the multiprecision sin / cos of the stored angle; measured after 32: 17 x 2^-53,
// and |s^2 + c^2 - 1| = 32 x 2^-53, of 78 allowed).
F16_DEV void trig_rotate(double &s, double &c, double d) {
  const double d2 = d * d;
  const double sd = d * fma(d2, fma(d2, 1.0 / 120.0, -1.0 / 6.0), 1.0);
  const double cd = fma(d2, fma(d2, 1.0 / 24.0, -0.5), 1.0);
  const double s1 = fma(c, sd, s * cd), c1 = fma(-s, sd, c * cd);
  s = s1; c = c1;
}
// The rollout kernels carry the five pairs from step to step in lane-indexed LDS slots (TrigSlots: slot k of this lane at
// base[k * stride]).  A stale set (every 32nd step, or after an increment beyond the series' range) is re-evaluated exactly INTO the
// slots at the top of the step -- a block of its own with nothing live behind it -- and plant_pre always loads the ten doubles where
// it needs them (behind the lookups): a merge of "evaluated" and "loaded" values in front of the lookups was spilled across them.
struct TrigSlots { double *base; int stride; };
F16_DEV void trig_store(const TrigSlots &ts, const Trig5 &g) {
  double *b = ts.base; const int n = ts.stride;
  b[0] = g.sa; b[n] = g.ca; b[2 * n] = g.sb; b[3 * n] = g.cb; b[4 * n] = g.st; b[5 * n] = g.ct; b[6 * n] = g.sphi; b[7 * n] = g.cphi;
  b[8 * n] = g.spsi; b[9 * n] = g.cpsi;
}
// after an Euler step: the pairs follow their angles by the EXACT increment of the stored state (xn - xo: a difference of
// neighbouring doubles), so nothing but the rounding of the rotations (<= 1.6 x 2^-53 a step, above) separates them from the state.
// Returns whether an increment left the series' range (the caller then marks the slots stale: the next step evaluates exactly).  fmax drops
// a NaN beside a number: a NaN increment of ONE angle is not reported here (its pair, and with it the state, becomes NaN).
F16_DEV bool trig_advance(const double *xo5, const double *xn, const TrigSlots &ts) {
  const double da = xn[7] - xo5[0], db = xn[8] - xo5[1], dt = xn[4] - xo5[2], dp = xn[3] - xo5[3], ds = xn[5] - xo5[4];
  const double big = fmax(fmax(fabs(da), fabs(db)), fmax(fmax(fabs(dt), fabs(dp)), fabs(ds)));
  double *b = ts.base; const int n = ts.stride;
  { double s = b[0], c = b[n]; trig_rotate(s, c, da); b[0] = s; b[n] = c; }
  { double s = b[2 * n], c = b[3 * n]; trig_rotate(s, c, db); b[2 * n] = s; b[3 * n] = c; }
  { double s = b[4 * n], c = b[5 * n]; trig_rotate(s, c, dt); b[4 * n] = s; b[5 * n] = c; }
  { double s = b[6 * n], c = b[7 * n]; trig_rotate(s, c, dp); b[6 * n] = s; b[7 * n] = c; }
  { double s = b[8 * n], c = b[9 * n]; trig_rotate(s, c, ds); b[8 * n] = s; b[9 * n] = c; }
  return !(big <= 4e-3);
}

template <bool ATMOS = true, bool GIVEN = false>
F16_DEV void plant_pre(const double *xu, Pre &p, double *xdot, const TrigSlots *tg = nullptr) {
  const double alt = xu[2], phi = xu[3], theta = xu[4], psi = xu[5];
  const double P = xu[9], Q = xu[10], R = xu[11];
  double vt = xu[6];
  if (vt <= 0.01) vt = 0.01;
  p.vt = vt;
  double spsi, cpsi;
  if (GIVEN) {        // (the slots are current: the caller has refreshed them where they were stale)
    const double *b = tg->base; const int n = tg->stride;
    p.sa = b[0]; p.ca = b[n]; p.sb = b[2 * n]; p.cb = b[3 * n]; p.st = b[4 * n]; p.ct = b[5 * n]; p.sphi = b[6 * n]; p.cphi = b[7 * n];
    spsi = b[8 * n]; cpsi = b[9 * n];
    (void)phi; (void)psi;
  } else {
    F16_SINCOS(xu[7], &p.sa, &p.ca);
    F16_SINCOS(xu[8], &p.sb, &p.cb);
    F16_SINCOS(theta, &p.st, &p.ct);
    F16_SINCOS(phi, &p.sphi, &p.cphi);
    F16_SINCOS(psi, &spsi, &cpsi);
  }
#ifdef F16_FAST_DIV
  const double rct = f16_rcp(p.ct);
  const double tt = p.st * rct;
#elif defined(F16_FAST_TAN)
  const double tt = p.st / p.ct;
#else
  const double tt = tan(theta);
#endif
  if (ATMOS) atmos_dev(alt, vt, p.mach, p.qbar, p.ps);
  else { p.mach = p.qbar = p.ps = 0.0; (void)alt; }
  p.U = vt * p.ca * p.cb; p.V = vt * p.sb; p.W = vt * p.sa * p.cb;
  const double U = p.U, V = p.V, W = p.W, st = p.st, ct = p.ct, sphi = p.sphi, cphi = p.cphi;
  xdot[0] = U * (ct * cpsi) + V * (sphi * cpsi * st - cphi * spsi) + W * (cphi * st * cpsi + sphi * spsi);
  xdot[1] = U * (ct * spsi) + V * (sphi * spsi * st + cphi * cpsi) + W * (cphi * st * spsi - sphi * cpsi);
  xdot[2] = U * st - V * (sphi * ct) - W * (cphi * ct);
  xdot[3] = P + tt * (Q * sphi + R * cphi);
  xdot[4] = Q * cphi - R * sphi;
#ifdef F16_FAST_DIV
  xdot[5] = (Q * sphi + R * cphi) * rct;
#else
  xdot[5] = (Q * sphi + R * cphi) / ct;
#endif
}

// Force equations (C/nlplant.c:383-405): xdot[6..8].
F16_DEV void plant_forces(const double *xu, const Pre &p, double Cx_tot, double Cy_tot, double Cz_tot, double *xdot) {
  const double g = 32.17, m = 636.94, S = 300.0;
  const double P = xu[9], Q = xu[10], R = xu[11], Thr = xu[12];
  const double U = p.U, V = p.V, W = p.W, vt = p.vt, qbar = p.qbar;
  const double st = p.st, ct = p.ct, sphi = p.sphi, cphi = p.cphi, cb = p.cb;
  const double Udot = R * V - Q * W - g * st + F16_DIVC(qbar * S * Cx_tot, m) + F16_DIVC(Thr, m);
  const double Vdot = P * W - R * U + g * ct * sphi + F16_DIVC(qbar * S * Cy_tot, m);
  const double Wdot = Q * U - P * V + g * ct * cphi + F16_DIVC(qbar * S * Cz_tot, m);
#ifdef F16_FAST_DIV      // reciprocals by v_rcp_f64 + two Newton steps (<= 1 ulp) instead of three IEEE division sequences
  xdot[6] = (U * Udot + V * Vdot + W * Wdot) * f16_rcp(vt);
  xdot[7] = (U * Wdot - W * Udot) * f16_rcp(U * U + W * W);
  xdot[8] = (Vdot * vt - V * xdot[6]) * f16_rcp(vt * vt * cb);
#else
  xdot[6] = (U * Udot + V * Vdot + W * Wdot) / vt;
  xdot[7] = (U * Wdot - W * Udot) / (U * U + W * W);
  xdot[8] = (Vdot * vt - V * xdot[6]) / (vt * vt * cb);
#endif
}

// Moment equations (C/nlplant.c:413-436): xdot[9..11].  Needs the body rates, qbar and Cl, Cm, Cn only.
F16_DEV void plant_moments(double P, double Q, double R, double qbar, double Cl_tot, double Cm_tot, double Cn_tot, double *xdot) {
  const double B = 30.0, S = 300.0, cbar = 11.32;
  const double Heng = 0.0;
  const double Jy = 55814.0, Jxz = 982.0, Jz = 63100.0, Jx = 9496.0;
  const double L_tot = Cl_tot * qbar * S * B;
  const double M_tot = Cm_tot * qbar * S * cbar;
  const double N_tot = Cn_tot * qbar * S * B;
#ifdef F16_FAST_DIV
  const double rdenom = 1.0 / (9496.0 * 63100.0 - 982.0 * 982.0);
#define F16_DIV_DENOM *rdenom
#else
  const double denom = Jx * Jz - Jxz * Jxz;
#define F16_DIV_DENOM / denom
#endif
  xdot[9] = (Jz * L_tot + Jxz * N_tot - (Jz * (Jz - Jy) + Jxz * Jxz) * Q * R + Jxz * (Jx - Jy + Jz) * P * Q + Jxz * Q * Heng) F16_DIV_DENOM;
  xdot[10] = F16_DIVC(M_tot + (Jz - Jx) * P * R - Jxz * (P * P - R * R) - R * Heng, Jy);
  xdot[11] = (Jx * N_tot + Jxz * L_tot + (Jx * (Jx - Jy) + Jxz * Jxz) * P * Q - Jxz * (Jx - Jy + Jz) * Q * R + Jx * Q * Heng) F16_DIV_DENOM;
}

// Force and moment equations (C/nlplant.c:383-436): xdot[6..11] (+ accels outputs 12..17 when OUTPUTS).
template <bool OUTPUTS>
F16_DEV void plant_post(const double *xu, const Pre &p, const Totals &t, double *xdot) {
  const double P = xu[9], Q = xu[10], R = xu[11];
  const double qbar = p.qbar, st = p.st, ct = p.ct, sphi = p.sphi, cphi = p.cphi, cb = p.cb;
  plant_forces(xu, p, t.Cx, t.Cy, t.Cz, xdot);
  plant_moments(P, Q, R, qbar, t.Cl, t.Cm, t.Cn, xdot);

  if (OUTPUTS) {  // accels(), C/nlplant.c:512-552 (uses the UNclamped state[6])
    const double grav = 32.174;
    const double v6 = xu[6];
    const double sa = p.sa, ca = p.ca, sb = p.sb;
    const double vel_u = v6 * cb * ca, vel_v = v6 * sb, vel_w = v6 * cb * sa;
    const double u_dot = cb * ca * xdot[6] - v6 * sb * ca * xdot[8] - v6 * cb * sa * xdot[7];
    const double v_dot = sb * xdot[6] + v6 * cb * xdot[8];
    const double w_dot = cb * sa * xdot[6] - v6 * sb * sa * xdot[8] + v6 * cb * ca * xdot[7];
    xdot[12] = 1.0 / grav * (u_dot + Q * vel_w - R * vel_v) + st;
    xdot[13] = 1.0 / grav * (v_dot + R * vel_u - P * vel_w) - ct * sphi;
    xdot[14] = -1.0 / grav * (w_dot + P * vel_v - Q * vel_u) + ct * cphi;
    xdot[15] = p.mach;
    xdot[16] = qbar;
    xdot[17] = p.ps;
  }
}

// C/nlplant.c:23-457.  xu[0..16] in, xdot[0..11] out (+ xdot[12..17] = nx,ny,nz,mach,qbar,ps when OUTPUTS).
// Returns qbar/ps of the clamped-vt atmosphere call for reuse by the lef model.  The lookups and the six coefficient
// totals come FIRST: the 45 interpolated values collapse to 6 doubles before the register-hungry sincos/pow code runs.
template <bool OUTPUTS, int FI = -1, typename TP, bool GIVEN = false>
F16_DEV void plant(TP T, const double *__restrict__ LT, const double *xu, double *xdot, double xcg, int fi_flag,
                   unsigned flags, int &status, double &qbar_out, double &ps_out, const TrigSlots *tg = nullptr) {
  Totals t;
  aero_totals<FI>(T, LT, xu, xcg, fi_flag, flags, t, status);
  Pre p;
  plant_pre<true, GIVEN>(xu, p, xdot, tg);
  qbar_out = p.qbar; ps_out = p.ps;
  plant_post<OUTPUTS>(xu, p, t, xdot);
}

// IEEE minNum / maxNum clamp: DROPS a NaN (returns the bound).  For callers whose operand is finite by construction (trim).
F16_DEV double clipd(double a, double lo, double hi) { return fmin(fmax(a, lo), hi); }

// The reference's actuators saturate with np.clip (utils.py:303-330), and np.clip PROPAGATES NaN: a NaN command (what OSQP hands
// back for a QP it certifies infeasible, env.py:420-424) or a NaN state gives a NaN derivative -- fmin / fmax alone would turn it
// into a hard-over at full rate.  One command-saturated, rate-saturated first-order lag
//     clip(k * (clip(cmd, lo, hi) - state), -rate, rate)
// with that rule: the fast clamps, then ONE unordered compare of the command with the unclamped rate (NaN if either is) + a select.
F16_DEV double actuator_rate(double cmd, double lo, double hi, double k, double state, double rate) {
  const double t = k * (clipd(cmd, lo, hi) - state);
  const double r = clipd(t, -rate, rate);
  return __builtin_isunordered(cmd, t) ? __builtin_nan("") : r;
}

// utils.py:289-306 -> lf1_dot (7.25*LF_err), lf2_dot (lef_err).  qbar/ps are those of atmos(h, V) with the
// RAW V (utils.py:291); plant() evaluates atmos with vt clamped to >= 0.01, identical whenever V > 0.01.
// atm: the atmosphere function the caller took qbar_p / ps_p from (the two evaluations then share their exp / log).
template <typename ATM>
F16_DEV void upd_lef_with(double h, double V, double alpha, double lf1, double lf2, double qbar_p, double ps_p,
                          double &lf1_dot, double &lf2_dot, ATM atm) {
  double qbar = qbar_p, ps = ps_p;
  if (V <= 0.01) {
    double mach;
    atm(h, V, mach, qbar, ps);
  }
  const double atmos_out = qbar / ps * 9.05;
  const double alpha_deg = F16_DIVC(alpha * 180, 3.141592653589793);
  const double LF_err = alpha_deg - (lf1 + (2 * alpha_deg));
  const double LF_out = (lf1 + (2 * alpha_deg)) * 1.38;
  const double lef_cmd = LF_out + 1.45 - atmos_out;
  lf2_dot = actuator_rate(lef_cmd, 0., 25, 1 / 0.136, lf2, 25);     // utils.py:303-305 (np.clip: NaN in -> NaN out)
  lf1_dot = LF_err * 7.25;
}
F16_DEV void upd_lef_dev(double h, double V, double alpha, double lf1, double lf2, double qbar_p, double ps_p,
                         double &lf1_dot, double &lf2_dot) {
  upd_lef_with(h, V, alpha, lf1, lf2, qbar_p, ps_p, lf1_dot, lf2_dot,
               [](double h_, double V_, double &m, double &q, double &p) { atmos_dev(h_, V_, m, q, p); });
}

// utils.py:308-330 + env.py:90-102: actuator and leading-edge-flap state derivatives xdot[12..17].
F16_DEV void actuators_dev(const double *x, const double *u, double qbar, double ps, double *xdot) {
  xdot[12] = actuator_rate(u[0], 1000, 19000, 1.0, x[12], 10000);      // utils.py:308-312
  xdot[13] = actuator_rate(u[1], -25, 25, 20.2, x[13], 60);            // :314-318
  xdot[14] = actuator_rate(u[2], -21.5, 21.5, 20.2, x[14], 80);        // :320-324
  xdot[15] = actuator_rate(u[3], -30., 30, 20.2, x[15], 120);          // :326-330
  double lf1_dot, lf2_dot;
  upd_lef_dev(x[2], x[6], x[7], x[17], x[16], qbar, ps, lf1_dot, lf2_dot);
  xdot[16] = lf2_dot;   // env.py:98,102: temp[4] -> xdot[16]
  xdot[17] = lf1_dot;
}

// env.py:65-103: xdot[18] of the full actuated model.
template <int FI = -1, typename TP, bool GIVEN = false>
F16_DEV void calc_xdot(TP T, const double *__restrict__ LT, const double *x, const double *u, double *xdot, double xcg,
                       int fi_flag, unsigned flags, int &status, const TrigSlots *tg = nullptr) {
  double qbar, ps;
  plant<false, FI, TP, GIVEN>(T, LT, x, xdot, xcg, fi_flag, flags, status, qbar, ps, tg);
  actuators_dev(x, u, qbar, ps, xdot);
}

// env.py:152-193: sv = full state with the 9 MPC states / 3 actuator positions already scattered in.
// Returns the 9 derivatives in MPC order {phi,theta,alpha,beta,p,q,r,lf1,lf2}; the two lef derivatives
// land swapped exactly as in the reference (env.py:184,189 vs :98,102).
template <typename TP>
F16_DEV void calc_xdot_na(TP T, const double *__restrict__ LT, const double *sv, double *xdot9, double xcg, int fi_flag,
                          unsigned flags, int &status) {
  double xd[12], qbar, ps;
  plant<false>(T, LT, sv, xd, xcg, fi_flag, flags, status, qbar, ps);
  double lf1_dot, lf2_dot;
  upd_lef_dev(sv[2], sv[6], sv[7], sv[17], sv[16], qbar, ps, lf1_dot, lf2_dot);
  xdot9[0] = xd[3]; xdot9[1] = xd[4]; xdot9[2] = xd[7]; xdot9[3] = xd[8];
  xdot9[4] = xd[9]; xdot9[5] = xd[10]; xdot9[6] = xd[11];
  xdot9[7] = lf2_dot;   // state_vector_dot[17] = lf_state2_dot
  xdot9[8] = lf1_dot;   // state_vector_dot[16] = lf_state1_dot
}

// env.py:117-124 box check (parameters.py:122-123, mixed units as in the reference)
// Which states are outside their box (env.py:117-124 tests all eighteen; six of them carry no finite limit): bit 8 + k for state
// k -- evaluated only once an aircraft has been found outside (outside_envelope), not in the per-step path
F16_DEV int envelope_state_bits(const double *x) {
#ifdef F16_NO_ENV_BITS      // (A/B builds: what the which-state bits cost the rollout kernels)
  return 0;
#endif
  int m = 0;
  m |= (x[2] < 0 || x[2] > 100000) ? 1 << (8 + 2) : 0;
  m |= (x[6] < 0 || x[6] > 900) ? 1 << (8 + 6) : 0;
  m |= (x[7] < -20. || x[7] > 90) ? 1 << (8 + 7) : 0;
  m |= (x[8] < -30. || x[8] > 30) ? 1 << (8 + 8) : 0;
  m |= (x[9] < -300 || x[9] > 300) ? 1 << (8 + 9) : 0;
  m |= (x[10] < -100 || x[10] > 100) ? 1 << (8 + 10) : 0;
  m |= (x[11] < -50 || x[11] > 50) ? 1 << (8 + 11) : 0;
  m |= (x[12] < 1000 || x[12] > 19000) ? 1 << (8 + 12) : 0;
  m |= (x[13] < -25 || x[13] > 25) ? 1 << (8 + 13) : 0;
  m |= (x[14] < -21.5 || x[14] > 21.5) ? 1 << (8 + 14) : 0;
  m |= (x[15] < -30. || x[15] > 30) ? 1 << (8 + 15) : 0;
  m |= (x[16] < 0. || x[16] > 25) ? 1 << (8 + 16) : 0;
  return m;
}
F16_DEV bool outside_envelope(const double *x) {
  bool bad = x[2] < 0 || x[2] > 100000 || x[6] < 0 || x[6] > 900 || x[7] < -20. || x[7] > 90 || x[8] < -30. || x[8] > 30 ||
             x[9] < -300 || x[9] > 300 || x[10] < -100 || x[10] > 100 || x[11] < -50 || x[11] > 50 || x[12] < 1000 ||
             x[12] > 19000 || x[13] < -25 || x[13] > 25 || x[14] < -21.5 || x[14] > 21.5 || x[15] < -30. || x[15] > 30 ||
             x[16] < 0. || x[16] > 25;
  return bad;
}

// ONE explicit-Euler step of ONE aircraft (env.py:105-130 without the envelope test; exact trigonometry), compiled OUT OF LINE: a
// function of its own has one instruction sequence whoever calls it, so the kernels that step through it -- the F16_FLAG_ONE_LANE
// rollout (f16_dynamics.hip: k_rollout_exact) and the closed MPC loop (f16_mpc_wave.hip: k_rollout_mpc) -- agree bit for bit.  (The
// same source inlined into two kernels does not: FMA contraction follows the surrounding code, and the navigation states came out an
// ulp apart.)  tab: the fp64 table image through a generic pointer (LDS or global); xio[18] in / out, uin[4], *stio |= the grid bits.
static __device__ __noinline__ void euler_step_exact(const double *tab, const double *lofi, double *xio, const double *uin, double dt,
                                                     double xcg, int fi, unsigned flags, int *stio) {
  double x[18], u[4], xd[18];
#pragma unroll
  for (int k = 0; k < 18; ++k) x[k] = xio[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) u[k] = uin[k];
  int st = 0;
  calc_xdot<-1>(tab, lofi, x, u, xd, xcg, fi, flags, st);
#pragma unroll
  for (int k = 0; k < 18; ++k) xio[k] = x[k] + xd[k] * dt;   // env.py:126
  *stio |= st;
}

// ONE classical fourth-order Runge-Kutta step of ONE aircraft (include/f16_hip.h: F16_INT_RK4), f = calc_xdot with the command u held
// over the four stages:
//   k1 = f(x)   k2 = f(x + (dt/2) k1)   k3 = f(x + (dt/2) k2)   k4 = f(x + dt k3)      x <- x + (dt/6) ((k1 + 2 k2) + (2 k3 + k4))
// The grid bits of all four evaluations are ORed into status; the stage states are not box-tested.  The four evaluations are ONE
// copy of the plant in a loop that is not unrolled (a step is ~1,500 wave-instructions: four copies would not stay in the instruction
// cache); the stage weights are selected by the uniform stage index, and x, the stage state and the two partial sums (72 doubles)
// stay in registers across an evaluation.  The products by 2 are exact, so the sums round as written whether contracted or not.
template <int FI = -1, typename TP>
F16_DEV void rk4_step(TP T, const double *__restrict__ LT, double *x, const double *u, double dt, double xcg, int fi_flag,
                      unsigned flags, int &status) {
  const double h2 = 0.5 * dt, h6 = dt / 6.0;
  double xs[18], s1[18], s2[18];
#pragma unroll
  for (int k = 0; k < 18; ++k) { xs[k] = x[k]; s1[k] = 0; s2[k] = 0; }
#pragma unroll 1
  for (int s = 0; s < 4; ++s) {
    double xd[18];
    calc_xdot<FI>(T, LT, xs, u, xd, xcg, fi_flag, flags, status);
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

// The same step compiled OUT OF LINE, for the reason euler_step_exact is: the F16_FLAG_ONE_LANE rollouts (k_rollout_exact, open loop,
// LQR law and scored alike) take an RK4 step through this one instruction sequence, so their results do not depend on the batch size.
static __device__ __noinline__ void rk4_step_exact(const double *tab, const double *lofi, double *xio, const double *uin, double dt,
                                                   double xcg, int fi, unsigned flags, int *stio) {
  double x[18], u[4];
#pragma unroll
  for (int k = 0; k < 18; ++k) x[k] = xio[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) u[k] = uin[k];
  int st = 0;
  rk4_step<-1>(tab, lofi, x, u, dt, xcg, fi, flags, st);
#pragma unroll
  for (int k = 0; k < 18; ++k) xio[k] = x[k];
  *stio |= st;
}

// env.py:152-193 _calc_xdot_na at ONE point (sv[18]: the full state with the three MPC inputs already in sv[13..15]) -> xdot9[9],
// compiled out of line for the same reason as euler_step_exact: the per-step re-linearised LQR loop (f16_control.hip:
// k_rollout_lqr_relin) evaluates every column of its forward differences through this one instruction sequence.  tab: the fp64
// table image through a generic pointer (global memory); *stio |= the grid bits.
static __device__ __noinline__ void xdot_na_exact(const double *tab, const double *lofi, const double *sv, double *xdot9, double xcg,
                                                  int fi, unsigned flags, int *stio) {
  double s[18], f[9];
#pragma unroll
  for (int k = 0; k < 18; ++k) s[k] = sv[k];
  int st = 0;
  calc_xdot_na(tab, lofi, s, f, xcg, fi, flags, st);
#pragma unroll
  for (int k = 0; k < 9; ++k) xdot9[k] = f[k];
  *stio |= st;
}

// Cooperative copy of the table image into LDS (16 B per lane per load), ended by a barrier.  BLOCK: the workgroup size where the
// kernel knows it (a constant stride); 0: as the launch has it (a read of the dispatch packet).
template <int BLOCK = 0> F16_DEV void stage_tables(double *lds, const double *__restrict__ g) {
  const double2 *src = reinterpret_cast<const double2 *>(g);
  double2 *dst = reinterpret_cast<double2 *>(lds);
  if constexpr (BLOCK > 0) { for (int i = threadIdx.x; i < TABLE_IMAGE_DOUBLES / 2; i += BLOCK) dst[i] = src[i]; }
  else { for (int i = threadIdx.x; i < TABLE_IMAGE_DOUBLES / 2; i += blockDim.x) dst[i] = src[i]; }
  __syncthreads();
}

}  // namespace f16
