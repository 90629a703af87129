// f16_wind_lanes.hpp -- what the wind rollout kernels of f16_wind.hip, their ensemble twins of f16_wind_ens.hip and the
// output-feedback twins of f16_observer.hip share, stated once: the argument block, the lane loop (wind_lanes) and, on the host, the
// one way from an entry point to the launch (WindRollout, wind_rollout).
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

// ---- host: one rollout in moving air as its entry point states it, and the one way from there to the launch
static const f16_wind STILL_AIR = {};
struct ObsInputs;                      // f16_observer.hip

// The six f16_rollout*_wind* calls differ in these values and in the kernel family F they hand to wind_rollout.
struct WindRollout {
  const char *missing;                 // the message for a NULL among the pointers the variant needs beyond x and u
  double *x;                           // [18][ld], stepped in place
  const double *u;                     // [4][ld]: row 0 of u_seq; u0 under the LQR law
  const double *seq;                   // u_seq [nrows][4][ld]; under the LQR law dem_seq [nrows][3][ld]
  const f16_wind *w;                   // null: zero air THROUGH the wind kernels (the plain calls forward still air before they come here)
  double *traj;
  int32_t *status;
  long B, ld;
  int nsteps, hold, traj_every;
  double dt, xcg;
  int fi, method;
  unsigned flags;
  // what an entry point leaves alone is the value of the simplest call, f16_rollout_wind:
  const double *K = nullptr;           // LQR: the gain
  double *u_out = nullptr;             // LQR: the last action, may be null
  const f16_ens *ens = nullptr;        // F::ENS: the results and the workspace
  const ObsInputs *obs = nullptr;      // F::OBS: the observer's inputs
  double *xhat_traj = nullptr;         // F::OBS: the estimate at every sample point, with or without traj
};

// A kernel family F is what a translation unit hands over of its kernels: the lane loop's variant (LQR, ENS, OBS), the texts of a
// failed launch (what; ENS: what_finish), with OBS the observer's rules (rules(d), checked last), and launch<BLOCK, STAGES>(grid, st, a, d) /
// launch_exact<STAGES>(grid, st, a, d): its BLOCK-lane and its 64-lane F16_FLAG_ONE_LANE kernel with the family's extra arguments.
// The rest is here.  The rules come in the sibling's order (f16_dynamics.hip: plant_rollout), then the wind fields, the ensemble's,
// the family's.  The step rule looks at whichever sample array is given; the kernel counts a sample period the step counter never
// reaches when nothing is sampled.  Geometry: one lane per aircraft under the 256-lane ceiling -- never a role-wave kernel.
template <typename F>
static int wind_rollout(f16_ctx *ctx, const WindRollout &d, void *stream) {
  const f16_wind *w = d.w ? d.w : &STILL_AIR;
  const double *sampled = d.traj ? d.traj : d.xhat_traj;
  if (!d.seq || (F::LQR && !d.K)) return set_error(F16_EINVAL, d.missing);
  if (int rc = check_rollout(ctx, d.x, d.u, sampled, d.B, d.ld, d.nsteps, d.traj_every)) return rc;
  if (d.hold < 1) return set_error(F16_EINVAL, "hold must be >= 1");
  if (d.method != F16_INT_EULER && d.method != F16_INT_RK4) return set_error(F16_EINVAL, "method must be F16_INT_EULER (1) or F16_INT_RK4 (4)");
  if (w->gust_seq && w->ga) return set_error(F16_EINVAL, "gust_seq and ga are both given: the gust rows are either read or generated");
  if ((w->ga != nullptr) != (w->gb != nullptr) || (w->ga != nullptr) != (w->gstate != nullptr))
    return set_error(F16_EINVAL, "ga, gb and gstate go together");
  const bool gusts = w->gust_seq || w->ga;
  if (gusts && w->gust_hold < 1) return set_error(F16_EINVAL, "gust_hold must be >= 1");
  if constexpr (F::ENS) {
    if (d.traj_every < 1 || d.nsteps % d.traj_every != 0)
      return set_error(F16_EINVAL, "nsteps must be a multiple of traj_every >= 1: the sample period of the ensemble, with or without traj");
    if (int rc = ens_rules(d.ens, d.B)) return rc;
  }
  if constexpr (F::OBS) if (int rc = F::rules(d)) return rc;
  if (d.B == 0 || d.nsteps == 0) return F16_OK;
  WindArgs a = base_args<WindArgs>(ctx, d.B, d.ld, d.xcg, d.fi, d.flags, d.status);
  a.u = d.u; a.out = d.x; a.traj = d.traj;
  a.nsteps = d.nsteps; a.traj_every = F::ENS || sampled ? d.traj_every : d.nsteps + 1; a.dt = d.dt;
  a.K = d.K; a.dem = F::LQR ? d.seq : nullptr; a.u_out = d.u_out;
  a.seq = d.seq; a.hold = d.hold; a.nrows = (d.nsteps - 1) / d.hold + 1;
  a.wind = w->wind_ned; a.gseq = w->gust_seq; a.ga = w->ga; a.gb = w->gb; a.gstate = w->gstate;
  a.ghold = gusts ? w->gust_hold : d.nsteps; a.grows = (d.nsteps - 1) / a.ghold + 1;
  a.key0 = (uint32_t)(w->seed & 0xffffffffu); a.key1 = (uint32_t)(w->seed >> 32); a.row0 = w->row0;
  const hipStream_t st = (hipStream_t)stream;
  const bool rk4 = d.method == F16_INT_RK4;
  if (d.flags & F16_FLAG_ONE_LANE) {
    if (rk4) F::template launch_exact<4>(one_lane_grid(d.B), st, a, d);
    else F::template launch_exact<1>(one_lane_grid(d.B), st, a, d);
  } else {
    const Geometry g = geometry(d.B, d.fi, 256);
    by_block(g, [&](auto block) {
      constexpr int BLOCK = decltype(block)::value;
      if constexpr (BLOCK <= 256) {
        if (rk4) F::template launch<BLOCK, 4>(dim3(g.grid), st, a, d);
        else F::template launch<BLOCK, 1>(dim3(g.grid), st, a, d);
      }
    });
  }
  if (int rc = hip_check(hipGetLastError(), F::what)) return rc;
  if constexpr (F::ENS) return ens_finish_launch(d.ens, d.B, d.nsteps / d.traj_every, d.flags, stream, F::what_finish);
  return F16_OK;
}

}  // namespace f16

