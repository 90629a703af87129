// f16_gain_sched.hpp -- the lookup rule of a gain schedule over (altitude, airspeed): ONE definition for the host entry
// f16_gain_lookup_host, the test kernel behind f16_debug_gain_lookup and the scheduled-gain rollouts (f16_rollout_lqr_gs).
//
// Table tab[nh][nv][12] of doubles, node (ih, iv) at (ih * nv + iv) * 12: entries 3 i + j = K[i][4 + j] (K = -dlqr, the
// reference's sign), entries 9 + i = the trim surface command u_trim[1 + i].  For h = x[2], V = x[6] (include/f16_hip.h):
//     th = (h - h0) / dh;  ih = (int) fmin(fmax(floor(th), 0), nh - 2);  lh = fmin(fmax(th - ih, 0), 1)      (tv, iv, lv alike)
//     a = G[ih][iv][e] + lv * (G[ih][iv+1][e] - G[ih][iv][e]);  b = the same on row ih + 1;  g[e] = a + lh * (b - a)
//     (each of the three with weight 1 takes its upper value as it is: gain_lerp)
// Every operation is rounded on its own: the products and sums below are never contracted into an FMA, whatever the
// -ffp-contract setting of the translation unit (the pragma for the front end, and an optimisation barrier on every product
// for the device back end, which under -ffp-contract=fast fuses without asking the front end).  So the bits are the same on
// the host, on the device and in the numpy restatement (f16_mpc_oop_py_amd/schedule.py).
// Outside the grid the edge cell is extended flat (a clamp, no extrapolation); a NaN coordinate takes index 0 with weight 0
// (fmax(NaN, 0) = 0); at a node the node's values come back exactly; a table of equal nodes returns them exactly.
#pragma once
#include <math.h>

#include "../../include/f16_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define F16_GS_HD __host__ __device__ inline
#else
#define F16_GS_HD inline
#endif

namespace f16 {

struct GainCell {
  long at;          // (ih * nv + iv) * 12: the cell's first node in the table
  long up;          // nv * 12: the distance to row ih + 1
  double lh, lv;    // weights in [0, 1]
  bool outside;     // (h, V) not inside [h0, h0 + (nh-1) dh] x [v0, v0 + (nv-1) dv], or not finite
};

// a product that no later pass may fuse with the sum it feeds
F16_GS_HD double gs_product(double a, double b) {
#pragma clang fp contract(off)
  double p = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
  __asm__("" : "+v"(p));
#endif
  return p;
}

// one axis: t = (c - c0) / d -> the cell index in 0..n-2 and the weight in [0, 1]
F16_GS_HD void gain_axis(double c, double c0, double d, int n, int &i, double &l, bool &outside) {
#pragma clang fp contract(off)
  const double t = (c - c0) / d;
  i = (int)fmin(fmax(floor(t), 0.0), (double)(n - 2));
  l = fmin(fmax(t - (double)i, 0.0), 1.0);
  outside = !(t >= 0.0 && t <= (double)(n - 1));      // (NaN and the infinities fail the comparisons)
}

F16_GS_HD GainCell gain_cell(const f16_gain_grid &g, double h, double v) {
  GainCell c;
  int ih, iv;
  bool oh, ov;
  gain_axis(h, g.h0, g.dh, g.nh, ih, c.lh, oh);
  gain_axis(v, g.v0, g.dv, g.nv, iv, c.lv, ov);
  c.at = ((long)ih * g.nv + iv) * F16_GS_ENTRIES;
  c.up = (long)g.nv * F16_GS_ENTRIES;
  c.outside = oh || ov;
  return c;
}

// p + l (q - p); the weight 1 -- the last node of an axis and everything beyond it -- takes q itself, because p + (q - p) need not
// round to q: that is what makes "the node's values come back exactly" and "the edge cell is extended flat" true at that edge too
F16_GS_HD double gain_lerp(double p, double q, double l) {
#pragma clang fp contract(off)
  const double r = p + gs_product(l, q - p);
  return l >= 1.0 ? q : r;
}

// the four corners of one entry -> its value
F16_GS_HD double gain_blend(double g00, double g01, double g10, double g11, double lh, double lv) {
  return gain_lerp(gain_lerp(g00, g01, lv), gain_lerp(g10, g11, lv), lh);
}

// The whole lookup: the 48 corner values are read first (on the device: one batch of loads, one wait), then blended.
// Returns whether (h, V) lay outside the grid or was not finite.
F16_GS_HD bool gain_lookup(const f16_gain_grid &g, const double *tab, double h, double v, double *out12) {
  const GainCell c = gain_cell(g, h, v);
  const double *p = tab + c.at;
  double q[4][F16_GS_ENTRIES];
#pragma unroll
  for (int e = 0; e < F16_GS_ENTRIES; ++e) {
    q[0][e] = p[e];
    q[1][e] = p[F16_GS_ENTRIES + e];
    q[2][e] = p[c.up + e];
    q[3][e] = p[c.up + F16_GS_ENTRIES + e];
  }
#pragma unroll
  for (int e = 0; e < F16_GS_ENTRIES; ++e) out12[e] = gain_blend(q[0][e], q[1][e], q[2][e], q[3][e], c.lh, c.lv);
  return c.outside;
}

// the argument rule of a grid (f16_rollout_lqr_gs, f16_gain_lookup_host, f16_debug_gain_lookup): nullptr when it is good
inline const char *gain_grid_error(const f16_gain_grid *g) {
  if (!g) return "h_grid is NULL";
  if (g->nh < 2 || g->nv < 2) return "h_grid: nh and nv must be >= 2";
  if (!(g->dh > 0.0) || !(g->dv > 0.0) || !__builtin_isfinite(g->dh) || !__builtin_isfinite(g->dv))
    return "h_grid: dh and dv must be finite and > 0";
  if (!__builtin_isfinite(g->h0) || !__builtin_isfinite(g->v0)) return "h_grid: h0 and v0 must be finite";
  return nullptr;
}

}  // namespace f16
