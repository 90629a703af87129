// f16_rollout_common.hpp -- what the rollout kernels of f16_dynamics.hip and of f16_wind.hip share, stated once: the argument blocks
// of the constant-input and scheduled rollouts, the look-ahead of a schedule's rows (RowAhead), the LQR action, and on the host the
// launch geometry and the argument rules.  (The staging of the table image, stage_tables, is f16_plant.hpp's: every kernel file uses it.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/f16_hip.h"
#include "f16_ctx.h"
#include "f16_plant.hpp"

namespace f16 {

struct DynArgs {
  const double *tab;    // hifi image, global
  const int *tab32;     // hifi image as scaled integers (f16_tables.h, namespace i32), global
  const double *lofi;   // lofi image, global
  const double *x;      // [18][ld] (or x_full for xdot_na)
  const double *u;      // [4][ld]  (x9 for xdot_na)
  const double *u3;     // xdot_na only
  double *out;          // xdot / x (rollout: in place) / xdot9
  double *traj;
  int32_t *status;
  long B, ld;
  int nsteps, traj_every;
  double dt, xcg;
  int fi;
  unsigned flags;
  // closed loop under the LQR law (f16_rollout_lqr; env.py:360-371 inside the loop of test_env_mk2.py:70-85)
  const double *K;      // [27][ld] the reference's K = -dlqr (3 x 9 row-major), or null
  const double *dem;    // [3][ld] p, q, r demands
  double *u_out;        // [4][ld] the action of the last step (self.u.values after the loop), may be null
};
// The SCHED instantiations (f16_rollout_sched / f16_rollout_lqr_sched) take the input schedule behind the same fields -- a type of
// their own, so that the constant-input kernels keep their argument block byte for byte.  seq: u_seq [nrows][4][ld], or under the
// LQR law dem_seq [nrows][3][ld]; step t takes row t / hold.  u (dem) points at row 0, which every kernel reads like a constant input.
struct SchedArgs : DynArgs {
  const double *seq;
  int hold, nrows;
};

// The schedule of one lane in a SCHED instantiation, N values per row (ld apart, the lane's first at row + lane_off).  A new row
// must never be loaded where it is used: a load that misses to HBM is ~900 cycles, a third of a quad-kernel step.
//   AHEAD = true   the next row waits in registers nx: loaded when the current row is installed, `hold` >= 1 whole steps before its
//                  first use, so the only wait for it stands in the install branch a step or more after the load was issued
//                  (one wave per SIMD: the registers are there)
//   AHEAD = false  no registers of its own: take() loads straight into the caller's.  The split kernels call it right after the
//                  LAST use of the old row -- wave 3 reads its inputs in the first half of a step and idles in the second, so the
//                  load is one step (less a few instructions) ahead of its use; the 512-lane kernels, whose registers already
//                  spill, call it at the end of a step, where the second wave of the SIMD issues while this one waits.
// settle(): every load of the prologue (state, inputs, gains, status) has landed before the step loop is entered.  Without it the
// compiler, which cannot tell the iterations apart, waits for ALL outstanding loads -- the row just requested among them -- at the
// first use of any prologue-loaded register in an iteration, i.e. at the top of the next step: the load would be waited for
// where the step starts instead of where the row is used.
// The bookkeeping (due) is the same on every lane of the workgroup and stays in scalar registers; only take() is per lane, and in
// the split kernels only wave 3 calls it.  A row is addressed FROM THE LANE'S STATE COLUMN col = a.out + b, whose address lives
// through the rollout anyway, by the (uniform) distance rel between the two arrays: no second per-lane address is kept for it.
template <int N, bool AHEAD = true>
struct RowAhead {
  double nx[AHEAD ? N : 1];
  long rel;                      // the next row to install: seq + row * nvals * ld - out, in doubles
  int left, rows;                // steps until it takes over; rows still to install
  F16_DEV void load(double *d, const double *col, long at, long ld) {
#pragma unroll
    for (int k = 0; k < N; ++k) d[k] = col[at + k * ld];
  }
  // nvals: values per row of the schedule (4 commands, or 3 demands); first: the lane's first value within a row (a multiple of ld)
  F16_DEV void init(const SchedArgs &a, int nvals, const double *col, long first = 0, bool owner = true) {
    nx[0] = 0;
    rel = (a.seq - a.out) + nvals * a.ld; left = a.hold; rows = a.nrows - 1;
    if (AHEAD && owner && rows > 0) load(nx, col, rel + first, a.ld);
  }
  F16_DEV static void settle() { __builtin_amdgcn_s_waitcnt(0); }
  F16_DEV bool due(const SchedArgs &a, int nvals) {            // once per step, after its inputs were used: a new row from the next step on?
    if (--left != 0 || rows == 0) return false;
    left = a.hold; --rows; rel += nvals * a.ld;
    return true;
  }
  F16_DEV void take(const SchedArgs &a, int nvals, double *d, const double *col, long first = 0) {   // after due(): the new row into d[0..N)
    if (AHEAD) {
#pragma unroll
      for (int k = 0; k < N; ++k) d[k] = nx[k];
      if (rows > 0) load(nx, col, rel + first, a.ld);
    } else {
      load(d, col, rel - nvals * a.ld + first, a.ld);
    }
  }
};

// env.py:360-371 `_calc_LQR_action`: u = -K (x_ref - x) + u0 with x_ref = x except x_ref[4:7] = (p, q, r)_dem -- x_ref - x is
// exactly zero outside the three rate entries, so row i of the product is K[i][4..6] . (dem - (p, q, r)); the thrust command is
// not an LQR output (test_env_mk2.py:76-79 overwrites u.values[1:] only).  kr = K[i][4..6] of the lane's row.
F16_DEV double lqr_action(double kr0, double kr1, double kr2, double e0, double e1, double e2, double u0) {
  return -(kr0 * e0 + kr1 * e1 + kr2 * e2) + u0;
}

// ---- launch geometry and argument rules (host)
// One lane per aircraft; with the table image in LDS a CU holds one workgroup, so the workgroup size decides how many
// waves share a SIMD: fill all 256 CUs first (64 / 128 / 256 lanes), then two waves per SIMD (512 lanes) from 131,072
// aircraft on -- the phased lookups (aero_totals_phased) keep a hifi step inside 256 registers there; measured with
// every step stored: 15.8 (256 lanes) vs 17.1 (512) G steps/s at B = 262,144, 17.9 vs 21.5 at B = 1,048,576.
// max_block: a ceiling on the workgroup size, with the grid that goes with it (256: the Runge-Kutta rollouts and the wind family)
struct Geometry { int block, grid; };
static Geometry geometry(long B, int fi, int max_block = 512) {
  Geometry g;
  (void)fi;
  if (B <= 64L * 256) g.block = 64;          // <= 256 one-wave workgroups: one per CU
  else if (B <= 128L * 256) g.block = 128;   // fill all 256 CUs before stacking waves on a CU
  else if (B < 512L * 256) g.block = 256;    // one wave per SIMD
  else g.block = 512;                        // two waves per SIMD
  static const int force = [] { const char *e = getenv("F16_DYN_BLOCK"); return e ? atoi(e) : 0; }();   // tuning knob
  if (force == 64 || force == 128 || force == 256 || force == 512) g.block = force;
  if (g.block > max_block) g.block = max_block;
  long blocks = (B + g.block - 1) / g.block;
  g.grid = (int)(blocks < 256 ? blocks : 256);
  return g;
}

// F16_FLAG_ONE_LANE, and the helper kernels of one lane per aircraft: 64-lane workgroups in a grid-stride loop, at most 4096 of them
static dim3 one_lane_grid(long B) {
  const long blocks = (B + 63) / 64;
  return dim3((unsigned)(blocks < 4096 ? blocks : 4096));
}

// Geometry::block as a compile-time constant: f(std::integral_constant<int, BLOCK>) for the workgroup size of g
template <typename F>
static void by_block(const Geometry &g, F f) {
  if (g.block == 64) f(std::integral_constant<int, 64>{});
  else if (g.block == 128) f(std::integral_constant<int, 128>{});
  else if (g.block == 256) f(std::integral_constant<int, 256>{});
  else f(std::integral_constant<int, 512>{});
}

static int check_common(f16_ctx *ctx, const void *p0, const void *p1, long B, long ld) {
  if (!ctx || !p0 || !p1 || B < 0 || ld < B) return set_error(F16_EINVAL, "bad argument (NULL pointer, B < 0 or ld < B)");
  return F16_OK;
}

// what every launcher of these files fills alike (ARGS: DynArgs or one of its rollout extensions; the rest stays zero)
template <typename ARGS>
static ARGS base_args(const f16_ctx *ctx, long B, long ld, double xcg, int fi_flag, unsigned flags, int32_t *status) {
  ARGS a{};
  a.tab = ctx->d_tab; a.lofi = ctx->d_lofi; a.status = status;
  a.B = B; a.ld = ld; a.xcg = xcg; a.fi = fi_flag; a.flags = flags;
  return a;
}

// the argument rules f16_rollout and its scheduled / closed-loop / scored siblings share
static int check_rollout(f16_ctx *ctx, const double *x, const double *u, const double *traj, long B, long ld, int nsteps, int traj_every) {
  if (int rc = check_common(ctx, x, u, B, ld)) return rc;
  if (nsteps < 0 || (traj && (traj_every < 1 || nsteps % traj_every != 0)))
    return set_error(F16_EINVAL, "nsteps must be >= 0 and a multiple of traj_every >= 1 when traj is given");
  return F16_OK;
}

}  // namespace f16
