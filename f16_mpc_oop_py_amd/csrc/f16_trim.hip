// f16_trim.hip -- batched straight-and-level trim: the reference's F16.trim (env.py:198-292)
// for B flight conditions (h_t, v_t) at once, one wavefront lane per condition.
//
// The reference minimises  cost(UX0) = w . xdot[0:12]^2  over UX0 = (P3, dh, da, dr, alpha) with
// scipy.optimize.minimize(method='Nelder-Mead', tol=1e-10, maxiter=5e4) -- 1,932 sequential _calc_xdot calls
// per aircraft.  Here the same Nelder-Mead iteration (scipy/optimize/_optimize.py:_minimize_neldermead: rho 1,
// chi 2, psi 0.5, sigma 0.5, initial simplex +5 % / 0.00025, termination max|sim[1:]-sim[0]| <= xatol and
// max|f0 - f[1:]| <= fatol) with SIXTEEN LANES PER CONDITION (one DPP row): every point an iteration could need depends
// on the simplex at the start of the iteration only -- the reflected, expanded and both contracted points, and the five
// vertices of a shrink -- so the row evaluates all nine at once (lane s takes candidate s) and an iteration costs ONE plant
// evaluation of latency whatever branch scipy's rules then take; the decisions, the accepted coordinates and the
// evaluation COUNT are those of the sequential algorithm (nfev counts what scipy would have evaluated).  The simplex is
// replicated in the registers of the row's lanes (identical bookkeeping on every lane: no LDS, no synchronisation).
// A condition that cannot be trimmed runs to the reference's maxiter = 50,000 as scipy does (49,999 iterations: scipy's counter
// starts at 1): as many evaluation latencies (~0.15 s) instead of the ~350,000 of the one-evaluation-per-trip form this replaces.
//
// The iteration is written ONCE (nm_run), templated on the dimension and the cost: k_trim is its five-dimensional instance on the
// level objective, k_trim_man its six-dimensional instance on the objective of a steady climb, turn or pull-up (include/f16_hip.h:
// f16_trim_man_batch; ten candidates per iteration, still one row), run `runs` times, each run from the best point of the last.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>

#include "../../include/f16_hip.h"
#include "f16_ctx.h"
#include "f16_plant.hpp"

namespace f16 {

struct TrimArgs {
  const double *tab, *lofi, *h, *v;
  double *xtrim, *cost;
  int32_t *iters, *nfev, *status;
  long B, ld;
  double xcg;
  int fi;
  unsigned flags;
  int maxiter;
  int fast_forward;     // stop at a fixed point of the iteration and account for the remaining iterations (F16_TRIM_FASTFORWARD=0: run them)
  double xatol, fatol;
  double x0[5];
};

// the leading-edge flap state of a trim point, env.py:219-228 (alpha as the optimiser holds it, unclipped)
__device__ __forceinline__ double trim_flap(double h, double V, double alpha) {
  const double pi = 3.141592653589793;
  const double rho0 = 2.377e-3;
  const double tfac = 1 - 0.703e-5 * h;
  double temp = 519 * tfac;
  if (h >= 35000) temp = 390;
  const double rho = rho0 * pow(tfac, 4.14);
  const double qbar = 0.5 * rho * (V * V);
  const double ps = 1715 * rho * temp;
  return 1.38 * alpha * 180 / pi - 9.05 * qbar / ps + 1.45;
}

// obj_func of env.py:217-262
template <typename TP>
__device__ __forceinline__ double trim_cost(TP T, const double *LT, const double *q, double h, double V, double xcg, int fi,
                                            unsigned flags, int &st, double *xfull) {
  const double pi = 3.141592653589793;
  const double P3 = q[0], dh = q[1], da = q[2], dr = q[3], alpha = q[4];
  const double dlef = trim_flap(h, V, alpha);
  double x[18] = {0, 0, h, 0, alpha, 0, V, alpha, 0, 0, 0, 0, P3, dh, da, dr, dlef, -alpha * 180 / pi};
  x[12] = clipd(x[12], 1000, 19000);
  x[13] = clipd(x[13], -25, 25);
  x[14] = clipd(x[14], -21.5, 21.5);
  x[15] = clipd(x[15], -30., 30);
  x[7] = clipd(x[7], -20. * pi / 180, 90 * pi / 180);
  const double u[4] = {x[12], x[13], x[14], x[15]};
  double xd[18];
  calc_xdot(T, LT, x, u, xd, xcg, fi, flags, st);
  const double w[12] = {0, 0, 5, 10, 10, 10, 2, 10, 10, 10, 10, 10};
  double c = 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) c += w[k] * (xd[k] * xd[k]);
  if (xfull) {
#pragma unroll
    for (int k = 0; k < 18; ++k) xfull[k] = x[k];
  }
  return c;
}

// value of lane `src` of this lane's 16-lane row
__device__ __forceinline__ double row_get(double v, int src) {
  const int lane = (threadIdx.x & 48) | src;                      // within the wavefront
  const int lo = __shfl(__double2loint(v), lane, 64), hi = __shfl(__double2hiint(v), lane, 64);
  return __hiloint2double(hi, lo);
}

// STABLE sort of the N + 1 vertices by cost: tied vertices keep their order.  scipy sorts with numpy's default argsort, on six or
// seven elements an insertion sort (stable) -- except on x86 hosts where numpy dispatches it to a vectorised sorting network, which
// is not stable, so scipy's own order of exact ties depends on the host; the stable rule is the one held here (ties are exact only
// where clipped unknowns give two vertices the same plant input; tests/trim_cases.py: THE TIE RULE)
//   (sim, fs) <- the vertices src(i, k) with the costs fsrc[i], sorted; src may read sim (it is read before anything is written).
// Returns whether any bit of (sim, fs) changed.
__device__ __forceinline__ bool bits_differ(double a, double b) { return __double_as_longlong(a) != __double_as_longlong(b); }

template <int N, typename SRC>
__device__ __forceinline__ bool sort_simplex(double (&sim)[N + 1][N], double (&fs)[N + 1], const double (&fsrc)[N + 1], SRC src) {
  int rank[N + 1];
#pragma unroll
  for (int i = 0; i < N + 1; ++i) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < N + 1; ++j) r += (fsrc[j] < fsrc[i] || (j < i && fsrc[j] == fsrc[i])) ? 1 : 0;
    rank[i] = r;
  }
  double ns[N + 1][N], nf[N + 1];
#pragma unroll
  for (int r = 0; r < N + 1; ++r) {
    nf[r] = fsrc[0];
#pragma unroll
    for (int k = 0; k < N; ++k) ns[r][k] = src(0, k);
#pragma unroll
    for (int i = 1; i < N + 1; ++i) {
      const bool here = rank[i] == r;
      nf[r] = here ? fsrc[i] : nf[r];
#pragma unroll
      for (int k = 0; k < N; ++k) ns[r][k] = here ? src(i, k) : ns[r][k];
    }
  }
  bool changed = false;
#pragma unroll
  for (int r = 0; r < N + 1; ++r) {
    changed = changed || bits_differ(fs[r], nf[r]);
    fs[r] = nf[r];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      changed = changed || bits_differ(sim[r][k], ns[r][k]);
      sim[r][k] = ns[r][k];
    }
  }
  return changed;
}

// ONE RUN of scipy's _minimize_neldermead in N dimensions on the cost f(q, st, xfull), written once for the level trim (N = 5) and
// the manoeuvre trim (N = 6).  Lane s of the row evaluates candidate s: 0 reflected, 1 expanded, 2 and 3 the two contracted points,
// 3 + j the shrunk vertex j (j = 1 .. N) -- N + 4 <= 16 candidates, one plant evaluation of latency per iteration.  x0 is the start,
// `idle` a point the lanes of a finished row evaluate while the wavefront's other rows go on (its cost is not used); skip: the row
// is not iterated at all.  Out: the sorted simplex, its costs, iters = scipy's nit of this run; nfev is added to.
template <int N, typename F>
__device__ __forceinline__ void nm_run(const F &f, const int s, const bool skip, const double (&x0)[N], const double (&idle)[N],
                                       const int maxiter, const int fast_forward, const double xatol, const double fatol,
                                       double (&sim)[N + 1][N], double (&fs)[N + 1], int &iters, int &nfev) {
  // initial simplex (scipy: nonzdelt 0.05, zdelt 0.00025)
#pragma unroll
  for (int p = 0; p < N + 1; ++p)
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double y = x0[k];
      if (p == k + 1) y = (y != 0.0) ? (1 + 0.05) * y : 0.00025;
      sim[p][k] = y;
    }
  // scipy's counter: `iterations = 1` before the loop, `while iterations < maxiter`, += 1 after an iteration -- so iters is
  // the iterations performed + 1 (scipy's nit), a run performs at most maxiter - 1, and iters >= maxiter after the loop
  // is scipy's status 2 (include/f16_hip.h states the rule)
  iters = 1;
  nfev += N + 1;
  {
    double q[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      q[k] = sim[0][k];
#pragma unroll
      for (int p = 1; p < N + 1; ++p) q[k] = s == p ? sim[p][k] : q[k];
    }
    int stq = 0;
    const double fq = f(q, stq, nullptr);
    double f0[N + 1];
#pragma unroll
    for (int p = 0; p < N + 1; ++p) f0[p] = row_get(fq, p);
    sort_simplex<N>(sim, fs, f0, [&](int i, int k) { return sim[i][k]; });
  }
  bool done = skip;
  while (true) {
    if (!done) {
      double dx = 0.0, df = 0.0;
#pragma unroll
      for (int p = 1; p < N + 1; ++p) {
#pragma unroll
        for (int k = 0; k < N; ++k) dx = fmax(dx, fabs(sim[p][k] - sim[0][k]));
        df = fmax(df, fabs(fs[0] - fs[p]));
      }
      if ((dx <= xatol && df <= fatol) || iters >= maxiter) done = true;
    }
    if (__all(done)) break;
    if (!done) ++iters;
    // every point this iteration can need, from the simplex as it stands
    double q[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double sb = sim[0][k];
#pragma unroll
      for (int p = 1; p < N; ++p) sb += sim[p][k];
      const double xbar = sb / N;
      const double xr = (1 + 1.0) * xbar - 1.0 * sim[N][k];
      const double xe = (1 + 1.0 * 2.0) * xbar - 1.0 * 2.0 * sim[N][k];
      const double xc = (1 + 0.5 * 1.0) * xbar - 0.5 * 1.0 * sim[N][k];
      const double xcc = (1 - 0.5) * xbar + 0.5 * sim[N][k];
      double v = s == 1 ? xe : (s == 2 ? xc : (s == 3 ? xcc : xr));
#pragma unroll
      for (int j = 1; j < N + 1; ++j) v = s == 3 + j ? sim[0][k] + 0.5 * (sim[j][k] - sim[0][k]) : v;
      q[k] = done ? idle[k] : v;
    }
    int stq = 0;
    const double fq = f(q, stq, nullptr);
    const double fxr = row_get(fq, 0), fxe = row_get(fq, 1), fxc = row_get(fq, 2), fxcc = row_get(fq, 3);
    double fsh[N + 1];
#pragma unroll
    for (int j = 1; j < N + 1; ++j) fsh[j] = row_get(fq, 3 + j);
    if (done) continue;
    // ---- scipy _minimize_neldermead, one iteration (nfev: the evaluations the sequential algorithm makes)
    const int nfev_in = nfev;
    bool accept = false, shrink = false, changed = false;     // changed: any bit of (sim, fs), for the fixed-point test below
    // the accepted point is fetched from the lane that evaluated it (`take`: its candidate slot) -- the four candidates need not
    // stay in registers across the plant evaluation, and the coordinates are those the cost was taken at, bit for bit
    int take = 0;
    double fa = fxr;
    nfev += 1;
    if (fxr < fs[0]) {
      nfev += 1;
      if (fxe < fxr) {
        fa = fxe; take = 1;
      }
      accept = true;
    } else if (fxr < fs[N - 1]) {
      accept = true;
    } else if (fxr < fs[N]) {
      nfev += 1;
      if (fxc <= fxr) {
        accept = true; fa = fxc; take = 2;
      } else shrink = true;
    } else {
      nfev += 1;
      if (fxcc < fs[N]) {
        accept = true; fa = fxcc; take = 3;
      } else shrink = true;
    }
    double xa[N];
#pragma unroll
    for (int k = 0; k < N; ++k) xa[k] = row_get(q[k], take);
    if (accept) {   // replace the worst vertex, keep the list sorted (stable: after equal costs, like numpy's argsort)
      int pos = N;
#pragma unroll
      for (int p = N - 1; p >= 0; --p) pos = fa < fs[p] ? p : pos;
#pragma unroll
      for (int p = N; p >= 1; --p) {
        const bool shift = p > pos, here = p == pos;
        const double fn = shift ? fs[p - 1] : (here ? fa : fs[p]);
        changed = changed || bits_differ(fs[p], fn);
        fs[p] = fn;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double xn = shift ? sim[p - 1][k] : (here ? xa[k] : sim[p][k]);
          changed = changed || bits_differ(sim[p][k], xn);
          sim[p][k] = xn;
        }
      }
      if (pos == 0) {
        changed = changed || bits_differ(fs[0], fa);
        fs[0] = fa;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          changed = changed || bits_differ(sim[0][k], xa[k]);
          sim[0][k] = xa[k];
        }
      }
    }
    if (shrink) {
      nfev += N;
      fsh[0] = fs[0];
      changed = sort_simplex<N>(sim, fs, fsh, [&](int i, int k) { return i == 0 ? sim[0][k] : sim[0][k] + 0.5 * (sim[i][k] - sim[0][k]); });
    }
    // A FIXED POINT of the iteration: the simplex and its costs come out bit for bit as they went in.  The iteration is a
    // deterministic function of (simplex, costs), so every remaining iteration repeats this one: scipy would run them all
    // to maxiter (env.py:273) and arrive at the same simplex, the same iteration count and nfev + the same increment each
    // time -- fast-forward instead of spending 50,000 plant evaluations of latency on them.  (Seen where the thrust
    // command saturates: the cost is flat in P3, the simplex drifts beyond |P3| ~ 4.5e5 where neighbouring doubles are
    // more than xatol = 1e-10 apart, and a shrink step x0 + 0.5 (xj - x0) of a one-ulp gap rounds back to xj.)
    // The test is made while the simplex is updated (`changed`), not against a saved copy: seven vertices of six coordinates, a
    // copy of them and the sort's own would not fit the register file.
    if (!changed && fast_forward) {
      const int left = maxiter - iters;                     // scipy's loop would run while iters < maxiter (the termination test did not fire for this simplex and never will)
      nfev += left * (nfev - nfev_in);
      iters = maxiter;
    }
  }
}

struct LevelCost {
  const double *tab, *lofi;
  double h, V, xcg;
  int fi;
  unsigned flags;
  __device__ __forceinline__ double operator()(const double *q, int &st, double *xfull) const {
    return trim_cost(tab, lofi, q, h, V, xcg, fi, flags, st, xfull);
  }
};

__global__ __launch_bounds__(256) void k_trim(TrimArgs a) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  if (a.fi == 1) stage_tables<256>(tab, a.tab);      // the table image of the hifi plant in LDS, once per workgroup
  const int s = threadIdx.x & 15;                                 // candidate slot of this lane
  // one row per condition, four conditions per wavefront; wavefronts stride over the batch independently (no barrier below)
  for (long b = (long)blockIdx.x * 16 + (threadIdx.x >> 4); b < ((a.B + 3) & ~3L); b += (long)gridDim.x * 16) {
    const bool valid = b < a.B;
    const LevelCost f{(const double *)tab, a.lofi, valid ? a.h[b] : 10000.0, valid ? a.v[b] : 700.0, a.xcg, a.fi, a.flags};
    double sim[6][5], fs[6];
    int iters, nfev = 0, st = 0;
    nm_run<5>(f, s, !valid, a.x0, a.x0, a.maxiter, a.fast_forward, a.xatol, a.fatol, sim, fs, iters, nfev);
    if (valid && s == 0) {
      // x_trim of env.py:275-290 (unclipped optimiser output; lef from the formula)
      double q[5], xf[18];
#pragma unroll
      for (int k = 0; k < 5; ++k) q[k] = sim[0][k];
      const double c = f(q, st, xf);
      xf[7] = q[4]; xf[12] = q[0]; xf[13] = q[1]; xf[14] = q[2]; xf[15] = q[3];
#pragma unroll
      for (int k = 0; k < 18; ++k) a.xtrim[k * a.ld + b] = xf[k];
      if (a.cost) a.cost[b] = c;
      if (a.iters) a.iters[b] = iters;
      if (a.nfev) a.nfev[b] = nfev;
      if (a.status) a.status[b] |= st | (iters >= a.maxiter ? F16_ST_QP_MAXITER : 0);
    }
  }
}

// ---- trim in a manoeuvre (include/f16_hip.h: f16_trim_man_batch states the rule)
struct TrimManArgs {
  const double *tab, *lofi, *h, *v, *gamma, *psi_dot, *theta_dot, *q0;
  double *xtrim, *cost;
  int32_t *iters, *nfev, *status;
  long B, ld;
  double xcg;
  int fi;
  unsigned flags;
  int maxiter, runs, fast_forward;
  double xatol, fatol;
};

struct ManCost {
  const double *tab, *lofi;
  double h, V, xcg;
  double sg, G, psi_dot, theta_dot;        // sin(gamma); psi_dot V / g
  int fi;
  unsigned flags;

  // phi, theta, p, q, r of the manoeuvre at the (clipped) alpha and beta -> c[5]
  __device__ __forceinline__ void constraints(double alpha, double beta, double *c) const {
    const double sa = sin(alpha), ca = cos(alpha), sb = sin(beta), cb = cos(beta);
    const double ta = sa / ca;
    const double a = 1 - G * ta * sb, b = sg / cb, cc = 1 + G * G * (cb * cb);
    const double num = G * (cb / ca) * ((a - b * b) + b * ta * sqrt(cc * (1 - b * b) + G * G * (sb * sb)));
    const double den = a * a - b * b * (1 + cc * (ta * ta));
    const double phi = atan(num / den);
    const double sp = sin(phi), cp = cos(phi);
    const double a2 = ca * cb, b2 = sp * sb + cp * sa * cb;
    const double theta = atan((a2 * b2 + sg * sqrt(a2 * a2 - sg * sg + b2 * b2)) / (a2 * a2 - sg * sg));
    const double sth = sin(theta), cth = cos(theta);
    c[0] = phi; c[1] = theta;
    c[2] = -psi_dot * sth;
    c[3] = theta_dot * cp + psi_dot * sp * cth;
    c[4] = -theta_dot * sp + psi_dot * cp * cth;
  }

  __device__ __forceinline__ double operator()(const double *q, int &st, double *xfull) const {
    const double pi = 3.141592653589793;
    const double alpha = q[4];
    double x[18] = {0, 0, h, 0, 0, 0, V, 0, 0, 0, 0, 0, 0, 0, 0, 0, trim_flap(h, V, alpha), -alpha * 180 / pi};
    x[12] = clipd(q[0], 1000, 19000);
    x[13] = clipd(q[1], -25, 25);
    x[14] = clipd(q[2], -21.5, 21.5);
    x[15] = clipd(q[3], -30., 30);
    x[7] = clipd(alpha, -20. * pi / 180, 90 * pi / 180);
    x[8] = clipd(q[5], -30. * pi / 180, 30 * pi / 180);
    double c5[5];
    constraints(x[7], x[8], c5);
    x[3] = c5[0]; x[4] = c5[1]; x[9] = c5[2]; x[10] = c5[3]; x[11] = c5[4];
    const double u[4] = {x[12], x[13], x[14], x[15]};
    double xd[18];
    calc_xdot(tab, lofi, x, u, xd, xcg, fi, flags, st);
    xd[2] -= V * sg; xd[4] -= theta_dot; xd[5] -= psi_dot;
    const double w[12] = {0, 0, 5, 10, 10, 10, 2, 10, 10, 10, 10, 10};
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) c += w[k] * (xd[k] * xd[k]);
    if (xfull) {
#pragma unroll
      for (int k = 0; k < 18; ++k) xfull[k] = x[k];
    }
    return c;
  }
};

__global__ __launch_bounds__(256) void k_trim_man(TrimManArgs a) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  if (a.fi == 1) stage_tables<256>(tab, a.tab);      // the table image of the hifi plant in LDS, once per workgroup
  const int s = threadIdx.x & 15;
  const double pi = 3.141592653589793;
  const double x0_ref[6] = {5000, -0.09, 8.49, -0.01, 0.01, 0.0};   // the level trim's start, beta = 0
  for (long b = (long)blockIdx.x * 16 + (threadIdx.x >> 4); b < ((a.B + 3) & ~3L); b += (long)gridDim.x * 16) {
    const bool valid = b < a.B;
    double gam = (valid && a.gamma) ? a.gamma[b] : 0.0, pd = (valid && a.psi_dot) ? a.psi_dot[b] : 0.0;
    double td = (valid && a.theta_dot) ? a.theta_dot[b] : 0.0;
    double x0[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) x0[k] = (valid && a.q0) ? a.q0[k * a.ld + b] : x0_ref[k];
    bool bad = !(fabs(gam) < pi / 2) || !isfinite(pd) || !isfinite(td);        // (a NaN gamma fails the comparison)
    if (bad) gam = pd = td = 0.0;
    ManCost f{(const double *)tab, a.lofi, valid ? a.h[b] : 10000.0, valid ? a.v[b] : 700.0, a.xcg, 0.0, 0.0, pd, td, a.fi, a.flags};
    f.sg = sin(gam);
    f.G = pd * f.V / 32.17;
    {
      double c5[5];
      f.constraints(clipd(x0[4], -20. * pi / 180, 90 * pi / 180), clipd(x0[5], -30. * pi / 180, 30 * pi / 180), c5);
      bool fin = true;
#pragma unroll
      for (int k = 0; k < 5; ++k) fin = fin && isfinite(c5[k]);
      bad = bad || !fin;
    }
    if (bad) {                                  // not iterated: its lanes evaluate the level start beside the wavefront's other rows
#pragma unroll
      for (int k = 0; k < 6; ++k) x0[k] = x0_ref[k];
    }
    double sim[7][6], fs[7];
    int iters = 0, nfev = 0, st = 0;
    bool capped = false;
    for (int run = 0; run < a.runs; ++run) {
      if (run > 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) x0[k] = sim[0][k];
      }
      int it;
      nm_run<6>(f, s, !valid || bad, x0, x0_ref, a.maxiter, a.fast_forward, a.xatol, a.fatol, sim, fs, it, nfev);
      iters += it;
      capped = capped || it >= a.maxiter;
    }
    if (valid && s == 0) {
      double q[6], xf[18];
#pragma unroll
      for (int k = 0; k < 6; ++k) q[k] = sim[0][k];
      double c = f(q, st, xf);
      xf[12] = q[0]; xf[13] = q[1]; xf[14] = q[2]; xf[15] = q[3]; xf[7] = q[4]; xf[8] = q[5];
      if (bad) {
        const double nan = __builtin_nan("");
        c = nan; iters = 0; nfev = 0; st = F16_ST_NONFINITE; capped = false;
#pragma unroll
        for (int k = 0; k < 18; ++k) xf[k] = nan;
      }
#pragma unroll
      for (int k = 0; k < 18; ++k) a.xtrim[k * a.ld + b] = xf[k];
      if (a.cost) a.cost[b] = c;
      if (a.iters) a.iters[b] = iters;
      if (a.nfev) a.nfev[b] = nfev;
      if (a.status) a.status[b] |= st | (capped ? F16_ST_QP_MAXITER : 0);
    }
  }
}

}  // namespace f16

using namespace f16;

extern "C" int f16_trim_batch(f16_ctx *ctx, const double *h, const double *v, double *x_trim, double *cost, int32_t *iters,
                              int32_t *nfev, int32_t *status, long B, long ld, double xcg, int fi_flag, unsigned flags,
                              int maxiter, const double *h_x0, void *stream) {
  if (!ctx || !h || !v || !x_trim || B < 0 || ld < B) return set_error(F16_EINVAL, "bad argument to f16_trim_batch");
  if (B == 0) return F16_OK;
  TrimArgs a{};
  a.tab = ctx->d_tab; a.lofi = ctx->d_lofi; a.h = h; a.v = v; a.xtrim = x_trim; a.cost = cost; a.iters = iters; a.nfev = nfev;
  a.status = status; a.B = B; a.ld = ld; a.xcg = xcg; a.fi = fi_flag; a.flags = flags;
  a.maxiter = maxiter > 0 ? maxiter : 50000;        // env.py:273
  a.xatol = 1e-10; a.fatol = 1e-10;                 // tol=1e-10
  { const char *e = getenv("F16_TRIM_FASTFORWARD"); a.fast_forward = !(e && e[0] == '0'); }
  static const double x0_ref[5] = {5000, -0.09, 8.49, -0.01, 0.01};   // env.py:265-271 (order as passed to minimize)
  for (int k = 0; k < 5; ++k) a.x0[k] = h_x0 ? h_x0[k] : x0_ref[k];
  const long blocks = (B + 15) / 16;       // 16 conditions (16 lanes each) per 256-lane workgroup, one workgroup per CU
  hipLaunchKernelGGL(k_trim, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream, a);
  return hip_check(hipGetLastError(), "f16_trim_batch launch");
}

extern "C" int f16_trim_man_batch(f16_ctx *ctx, const double *h, const double *v, const double *gamma, const double *psi_dot,
                                  const double *theta_dot, const double *q0, double *x_trim, double *cost, int32_t *iters,
                                  int32_t *nfev, int32_t *status, long B, long ld, double xcg, int fi_flag, unsigned flags,
                                  int maxiter, int runs, void *stream) {
  if (!ctx || !h || !v || !x_trim || B < 0 || ld < B || runs <= 0) return set_error(F16_EINVAL, "bad argument to f16_trim_man_batch");
  if (B == 0) return F16_OK;
  TrimManArgs a{};
  a.tab = ctx->d_tab; a.lofi = ctx->d_lofi; a.h = h; a.v = v; a.gamma = gamma; a.psi_dot = psi_dot; a.theta_dot = theta_dot; a.q0 = q0;
  a.xtrim = x_trim; a.cost = cost; a.iters = iters; a.nfev = nfev; a.status = status; a.B = B; a.ld = ld; a.xcg = xcg; a.fi = fi_flag;
  a.flags = flags; a.runs = runs;
  a.maxiter = maxiter > 0 ? maxiter : 50000;
  a.xatol = 1e-10; a.fatol = 1e-10;
  { const char *e = getenv("F16_TRIM_FASTFORWARD"); a.fast_forward = !(e && e[0] == '0'); }
  const long blocks = (B + 15) / 16;
  hipLaunchKernelGGL(k_trim_man, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream, a);
  return hip_check(hipGetLastError(), "f16_trim_man_batch launch");
}
