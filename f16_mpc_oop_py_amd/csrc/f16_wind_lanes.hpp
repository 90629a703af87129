// f16_wind_lanes.hpp -- what the wind rollout kernels of f16_wind.hip, their ensemble twins of f16_wind_ens.hip and the
// output-feedback twins of f16_observer.hip share, stated once: the argument block, the lane loop (wind_lanes) and, on the host, the
// argument rules and the filling of the block.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/f16_hip.h"
#include "f16_ctx.h"
#include "f16_ensemble.hpp"
#include "f16_observer.hpp"
#include "f16_plant.hpp"
#include "f16_rollout_common.hpp"
#include "f16_wind.hpp"

namespace f16 {

// The rollouts: the scheduled argument block (u_seq, or under the LQR law dem_seq, behind SchedArgs) and the air.
struct WindArgs : SchedArgs {
  const double *wind;          // [3][ld] or null (= 0): constant over the launch
  const double *gseq;          // [grows][3][ld] or null: step t reads row t / ghold
  const double *ga, *gb;       // [3][ld] or null: the gust rows are generated in place (gust_row), row r from counter word row0 + r
  double *gstate;              // [3][ld] with ga: the row before row0 in, the last row of the launch out
  int ghold, grows;
  uint32_t key0, key1, row0;
};

// The lane loop of both rollout kernels: rollout_lanes<..., SCHED = true> of f16_dynamics.hip (envelope freeze, sticky status bits,
// trajectory samples, u_out, the command / demand schedule through RowAhead) with the air added.  EXACT: the step through the
// out-of-line wind_step_exact on the table image in global memory (T = a.tab) instead of the inlined step on the LDS image.
// ws[0..2]: the wind, ws[3..5]: the gust row in use, read from the slots where an evaluation uses them.  gw: with a gust_seq the NEXT
// row, loaded when the current one is installed -- ghold >= 1 whole steps before its first use, as RowAhead does it.  With in-place
// generation the row in use is the generator's state and the lane's a[3], b[3] are re-read (L2) at the row change: the generation
// sits there, not in the step, and six more doubles held across the Runge-Kutta step would not stay in registers.
// ENS: the ensemble twin.  At every sample point (a.traj_every steps apart, traj or not) the wave forms its records of the sample
// (ens_wave_records) into ework[sample][wave][ENS_REC].  A WAVEFRONT runs the loop as a whole -- the loop condition looks at the
// wave's first aircraft -- and a lane without an aircraft (b0 >= B: `live` false) flies a copy of aircraft B - 1, which keeps its
// loads inside the arrays (the padding columns are never read), stores nothing and contributes nothing.
// OBS (with LQR): output feedback (f16_observer.hpp).  The action of a step comes from the state at the start of the step through
// measurement, correction, the LQR law on the estimate and prediction (observer_rule; under EXACT the out-of-line observer_update)
// instead of from the state; o is the workgroup's ObsArgs in LDS.  The prediction lives in the xhat array between steps (a coalesced
// 72 B read and write per aircraft and step, L2-resident: nine more doubles held across the Runge-Kutta step would not stay in
// registers); at a sample point it is copied to xhat_traj.  With ENS a lane without an aircraft runs the rule too, as the copy of
// aircraft B - 1 it is: it reads and writes column B - 1 of xhat in the same instructions as that aircraft's own lane of the same
// wavefront, the same bits from the same inputs -- the one store such a lane makes.
template <int BLOCK, bool LQR, int STAGES, bool EXACT, bool ENS = false, bool OBS = false>
__device__ __forceinline__ void wind_lanes(const WindArgs &a, const double *T, double (*us)[BLOCK], double (*kq)[BLOCK], double (*ws)[BLOCK],
                                           double *ework = nullptr, [[maybe_unused]] const ObsArgs *o = nullptr) {
  static_assert(!OBS || LQR, "the observer feeds the LQR law");
  const bool gen = a.ga != nullptr;
  SchedArgs g = a;                   // the gust rows seen as a schedule of three values per row
  g.seq = a.gseq ? a.gseq : a.out; g.hold = a.ghold; g.nrows = a.grows;
  for (long b0 = (long)blockIdx.x * BLOCK + threadIdx.x; (ENS ? b0 - (threadIdx.x & 63) : b0) < a.B; b0 += (long)gridDim.x * BLOCK) {
    const bool live = !ENS || b0 < a.B;
    const long b = live ? b0 : a.B - 1;
    double x[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) x[k] = a.out[k * a.ld + b];
#pragma unroll
    for (int k = 0; k < 4; ++k) us[k][threadIdx.x] = a.u[k * a.ld + b];
    double ul[3] = {us[1][threadIdx.x], us[2][threadIdx.x], us[3][threadIdx.x]};   // (u_out of an aircraft that never steps: u0)
    if (LQR) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) kq[3 * i + j][threadIdx.x] = a.K[(9 * i + 4 + j) * a.ld + b];
#pragma unroll
      for (int j = 0; j < 3; ++j) kq[9 + j][threadIdx.x] = a.dem[j * a.ld + b];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) ws[k][threadIdx.x] = a.wind ? a.wind[k * a.ld + b] : 0.0;
    double gw[3] = {0, 0, 0};
    uint32_t grow = a.row0;
    RowAhead<3, false> rg;
    rg.init(g, 3, a.out + b);
    if (gen) {
      const Gust3 r = gust_row(grow, (uint32_t)b, a.key0, a.key1, a.ga[b], a.ga[a.ld + b], a.ga[2 * a.ld + b], a.gb[b], a.gb[a.ld + b],
                               a.gb[2 * a.ld + b], a.gstate[b], a.gstate[a.ld + b], a.gstate[2 * a.ld + b]);
#pragma unroll
      for (int k = 0; k < 3; ++k) ws[3 + k][threadIdx.x] = r.v[k];
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) ws[3 + k][threadIdx.x] = a.gseq ? a.gseq[k * a.ld + b] : 0.0;
      if (rg.rows > 0) rg.load(gw, a.out + b, rg.rel, a.ld);
    }
    int st = a.status ? a.status[b] : 0;
    double *tr = a.traj ? a.traj + b : nullptr;
    int until_store = a.traj_every;
    [[maybe_unused]] long xsmp = 0;           // (OBS) the sample of xhat_traj to write next, in doubles: the same on every lane
    [[maybe_unused]] double *rec = ENS ? ework + (b0 >> 6) * ENS_REC : nullptr;       // the wave's record of the next sample
    constexpr int NR = LQR ? 3 : 4;
    RowAhead<NR> ra;
    ra.init(a, NR, a.out + b);
    ra.settle();
    for (int t = 0; t < a.nsteps; ++t) {
      // env.py:117-124 on the state, i.e. on the GROUND triple: the reference exit()s; here the aircraft is frozen and flagged
      if (!(a.flags & FLAG_NO_ENVELOPE) && outside_envelope(x)) st |= ST_ENVELOPE;
      if (!(st & ST_ENVELOPE)) {
        double u[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = us[k][threadIdx.x];
        if constexpr (OBS) {   // the controller reads the estimate
          const uint32_t row = o->mrow0 + (uint32_t)t;
          const Obs3 c = EXACT ? observer_update(o, b, row, x[3], x[4], x[7], x[8], x[9], x[10], x[11], x[17], x[16], x[13], x[14], x[15])
                               : observer_rule(o, b, row, x[3], x[4], x[7], x[8], x[9], x[10], x[11], x[17], x[16], x[13], x[14], x[15]);
#pragma unroll
          for (int i = 0; i < 3; ++i) ul[i] = u[1 + i] = c.v[i];
        } else if (LQR) {   // the controller reads the state, not the air data
          const double e0 = kq[9][threadIdx.x] - x[9], e1 = kq[10][threadIdx.x] - x[10], e2 = kq[11][threadIdx.x] - x[11];
#pragma unroll
          for (int i = 0; i < 3; ++i)
            ul[i] = u[1 + i] = lqr_action(kq[3 * i][threadIdx.x], kq[3 * i + 1][threadIdx.x], kq[3 * i + 2][threadIdx.x], e0, e1, e2, u[1 + i]);
        }
        if constexpr (EXACT) {
          double w[6];
#pragma unroll
          for (int k = 0; k < 6; ++k) w[k] = ws[k][threadIdx.x];
          wind_step_exact<STAGES>(T, a.lofi, x, u, w, a.dt, a.xcg, a.fi, a.flags, &st);
        } else {
          wind_step<STAGES, -1>(T, a.lofi, x, u, [&](int k) { return ws[k][threadIdx.x]; }, a.dt, a.xcg, a.fi, a.flags, st);
        }
      }
      if constexpr (ENS) {
        if (--until_store == 0) {      // the same on every lane: the whole wave is here
          until_store = a.traj_every;
          ens_wave_records(x, live, a.flags, rec);
          rec += ((a.B + 63) >> 6) * ENS_REC;
          if constexpr (OBS) {
            if (o->xhat_traj && live) {
#pragma unroll
              for (int k = 0; k < 9; ++k) __builtin_nontemporal_store(o->xhat[k * a.ld + b], o->xhat_traj + xsmp + k * a.ld + b);
            }
            xsmp += 9 * a.ld;
          }
          if (tr) {
            if (live) {
#pragma unroll
              for (int k = 0; k < 18; ++k) __builtin_nontemporal_store(x[k], tr + k * a.ld);
            }
            tr += 18 * a.ld;
          }
        }
      } else if constexpr (OBS) {
        if ((tr || o->xhat_traj) && --until_store == 0) {
          until_store = a.traj_every;
          if (tr) {
#pragma unroll
            for (int k = 0; k < 18; ++k) __builtin_nontemporal_store(x[k], tr + k * a.ld);
            tr += 18 * a.ld;
          }
          if (o->xhat_traj) {
#pragma unroll
            for (int k = 0; k < 9; ++k) __builtin_nontemporal_store(o->xhat[k * a.ld + b], o->xhat_traj + xsmp + k * a.ld + b);
            xsmp += 9 * a.ld;
          }
        }
      } else {
        if (tr && --until_store == 0) {
          until_store = a.traj_every;
#pragma unroll
          for (int k = 0; k < 18; ++k) __builtin_nontemporal_store(x[k], tr + k * a.ld);
          tr += 18 * a.ld;
        }
      }
      if (ra.due(a, NR)) {
        double r[NR];
        ra.take(a, NR, r, a.out + b);
#pragma unroll
        for (int k = 0; k < NR; ++k) (LQR ? kq[9 + k] : us[k])[threadIdx.x] = r[k];
        if (LQR) { ul[0] = us[1][threadIdx.x]; ul[1] = us[2][threadIdx.x]; ul[2] = us[3][threadIdx.x]; }   // (as a new launch: u0 until it steps)
      }
      if (rg.due(g, 3)) {            // a new gust row from the next step on, for frozen aircraft too (the generator does not stop)
        if (LQR) { ul[0] = us[1][threadIdx.x]; ul[1] = us[2][threadIdx.x]; ul[2] = us[3][threadIdx.x]; }   // (a segment start, as above)
        if (gen) {
          const Gust3 r = gust_row(++grow, (uint32_t)b, a.key0, a.key1, a.ga[b], a.ga[a.ld + b], a.ga[2 * a.ld + b], a.gb[b], a.gb[a.ld + b],
                                   a.gb[2 * a.ld + b], ws[3][threadIdx.x], ws[4][threadIdx.x], ws[5][threadIdx.x]);
#pragma unroll
          for (int k = 0; k < 3; ++k) ws[3 + k][threadIdx.x] = r.v[k];
        } else {
#pragma unroll
          for (int k = 0; k < 3; ++k) ws[3 + k][threadIdx.x] = gw[k];
          if (rg.rows > 0) rg.load(gw, a.out + b, rg.rel, a.ld);
        }
      }
    }
    if (!live) continue;             // (ENS only) nothing of a lane without an aircraft is written back
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 18; ++k) finite = finite && isfinite(x[k]);
    if (!finite) st |= ST_NONFINITE;
    if (st & ST_ENVELOPE) st |= envelope_state_bits(x);
    // (OBS: the write-back addresses are formed HERE, from an index the compiler cannot look through -- formed in the prologue they
    // were carried across the Runge-Kutta step in scratch memory, the only values there)
    long bw = b;
    if constexpr (OBS) asm volatile("" : "+v"(bw));
#pragma unroll
    for (int k = 0; k < 18; ++k) a.out[k * a.ld + bw] = x[k];
    if (a.status) a.status[bw] = st;
    if (LQR && a.u_out) {
      a.u_out[bw] = us[0][threadIdx.x];
#pragma unroll
      for (int i = 0; i < 3; ++i) a.u_out[(1 + i) * a.ld + bw] = ul[i];
    }
    if (gen) {
#pragma unroll
      for (int k = 0; k < 3; ++k) a.gstate[k * a.ld + bw] = ws[3 + k][threadIdx.x];
    }
  }
}

// ---- host: the argument rules and the argument block of the wind rollouts, for f16_wind.hip and f16_wind_ens.hip alike
static const f16_wind STILL_AIR = {};

// the sibling's checks in the sibling's order (f16_dynamics.hip: plant_rollout), then the wind fields
static int wind_check(f16_ctx *ctx, bool lqr, const char *missing, const double *x, const double *u, const double *K, const double *seq,
                      const f16_wind *w, const double *traj, long B, long ld, int nsteps, int hold, int traj_every, int method) {
  if (!seq || (lqr && !K)) return set_error(F16_EINVAL, missing);
  if (int rc = check_rollout(ctx, x, u, traj, B, ld, nsteps, traj_every)) return rc;
  if (hold < 1) return set_error(F16_EINVAL, "hold must be >= 1");
  if (method != F16_INT_EULER && method != F16_INT_RK4) return set_error(F16_EINVAL, "method must be F16_INT_EULER (1) or F16_INT_RK4 (4)");
  if (w->gust_seq && w->ga) return set_error(F16_EINVAL, "gust_seq and ga are both given: the gust rows are either read or generated");
  if ((w->ga != nullptr) != (w->gb != nullptr) || (w->ga != nullptr) != (w->gstate != nullptr))
    return set_error(F16_EINVAL, "ga, gb and gstate go together");
  if ((w->gust_seq || w->ga) && w->gust_hold < 1) return set_error(F16_EINVAL, "gust_hold must be >= 1");
  return F16_OK;
}

// traj_every: the sample period as the kernel counts it (without samples: a period the step counter never reaches)
static WindArgs wind_args(f16_ctx *ctx, bool lqr, double *x, const double *u, const double *K, const double *seq, const f16_wind *w,
                          double *traj, double *u_out, int32_t *status, long B, long ld, int nsteps, int hold, int traj_every, double dt,
                          double xcg, int fi_flag, unsigned flags) {
  WindArgs a = base_args<WindArgs>(ctx, B, ld, xcg, fi_flag, flags, status);
  a.u = u; a.out = x; a.traj = traj;
  a.nsteps = nsteps; a.traj_every = traj_every; a.dt = dt;
  a.K = K; a.dem = lqr ? seq : nullptr; a.u_out = u_out;
  a.seq = seq; a.hold = hold; a.nrows = (nsteps - 1) / hold + 1;
  const bool gusts = w->gust_seq || w->ga;
  a.wind = w->wind_ned; a.gseq = w->gust_seq; a.ga = w->ga; a.gb = w->gb; a.gstate = w->gstate;
  a.ghold = gusts ? w->gust_hold : nsteps; a.grows = (nsteps - 1) / a.ghold + 1;
  a.key0 = (uint32_t)(w->seed & 0xffffffffu); a.key1 = (uint32_t)(w->seed >> 32); a.row0 = w->row0;
  return a;
}

// The launch rules of the wind rollouts: the geometry of the one-lane-per-aircraft kernels with the 256-lane ceiling of the
// Runge-Kutta rollouts -- never a role-wave kernel, never 512 lanes.  (F16_FLAG_ONE_LANE: 64-lane workgroups, at most 4096.)
static Geometry wind_geometry(long B, int fi_flag) {
  Geometry g = geometry(B, fi_flag);
  if (g.block == 512) {
    g.block = 256;
    const long blocks = (B + 255) / 256;
    g.grid = (int)(blocks < 256 ? blocks : 256);
  }
  return g;
}

}  // namespace f16
