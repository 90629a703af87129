// f16_dynamics.hip -- batched F-16 dynamics kernels for gfx950 + their C-ABI launchers.
//
//   k_xdot      env.py:65-103 _calc_xdot for B aircraft                (f16_xdot_batch)
//   k_nlplant   C/nlplant.c:23-457 incl. accels outputs                (f16_nlplant_batch, drop-in Nlplant)
//   k_rollout   env.py:105-130 step x nsteps, state in registers       (f16_rollout)
//   k_xdot_na   env.py:152-193                                         (f16_xdot_na_batch)
//   k_rollout_exact       the same step x nsteps through the out-of-line euler_step_exact: one kernel for every batch size
//                         (F16_FLAG_ONE_LANE; the step the closed MPC loop f16_rollout_mpc takes)
//   k_rollout / k_rollout_i / k_rollout_exact <..., STAGES = 4>  the scheduled rollouts with the classical Runge-Kutta step instead of
//                         the Euler step (f16_rollout_rk, f16_rollout_lqr_rk, f16_rollout_cost_rk with F16_INT_RK4)
//   k_rollout_gs / k_rollout_i_gs / k_rollout_exact_gs  the LQR loop with K[:, 4:7] and the offset u0[1:4] looked up in a gain table over
//                         (altitude, airspeed) every gs_every steps (f16_rollout_lqr_gs; the rule: f16_gain_sched.hpp)
//   k_rollout_mppi / k_rollout_mppi_exact  the closed MPPI loop -- sample, score, blend, advance, shift per control period -- as one
//                         launch, one workgroup per aircraft, on the lane bodies of the scored and scheduled rollouts (f16_rollout_mppi)
//   k_rollout_lqr_linear  test_env_mk2.py:46-62 / test_env.py:501-576: the linear-model LQR loops (f16_rollout_lqr_linear)
//
// Mapping: one lane = one aircraft; state-major [k][ld] arrays so a wave's 64 lanes read 512 contiguous
// bytes per state component.  Every workgroup first copies the 112,928-byte fp64 table image from
// global memory (L2-resident after the first block) into LDS with 16-byte loads; all 168 table-vertex
// fetches of an evaluation are then LDS reads.  The kernels are bound by fp64 VALU issue and, at the
// reference's batch of 4096 (= 64 wavefronts), by single-wave latency; algorithmic HBM traffic is
// 320 B per aircraft-step for the state-resident step and 144 B per stored trajectory sample.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/f16_hip.h"
#include "f16_ctx.h"
#include "f16_plant.hpp"
#include "f16_rollout_common.hpp"
#include "f16_plant_quad.hpp"
#include "f16_mppi.hpp"
#include "f16_gain_sched.hpp"

namespace f16 {

// (DynArgs, SchedArgs, RowAhead, lqr_action and the launch geometry: f16_rollout_common.hpp, shared with f16_wind.hip; stage_tables: f16_plant.hpp)
// The COST instantiations (f16_rollout_cost) score the scheduled rollout: a third type, DynArgs and SchedArgs stay what they are.  Lane b is
// sample b / B0 of aircraft b % B0: its state comes from column b % B0 of x0 (read-only) and nothing is integrated in place -- `out`
// is the cost column [ld], the per-lane array the schedule rows are addressed from (RowAhead); x_end may be null.  The weights are
// uniform and travel by value (scalar registers; nothing to allocate, so the call can be captured).
struct CostArgs : SchedArgs {
  const double *x0;      // [18][ld0]
  const double *x_ref;   // [9][ld0]  MPC-state order (parameters.py:135)
  const double *u_ref;   // [3][ld0] or null (= 0)
  double *x_end;         // [18][ld] or null
  long B0, ld0;
  f16_cost_weights w;
};
// The GS instantiations (f16_rollout_lqr_gs: LQR && SCHED && !COST) take K[i][4..6] and the offset u0[1..3] from a gain schedule over
// (altitude, airspeed) instead of K / u rows 1..3: a fourth type, the three above stay what they are.  The grid travels by value
// (scalar registers; nothing to allocate, so the call can be captured); the table is read from global memory through L2.
struct GainSchedArgs : SchedArgs {
  f16_gain_grid grid;
  const double *gtab;   // [nh][nv][12]
  int32_t *gs_out;      // [ld] or null: updates at which (h, V) lay outside the grid
  int gs_every;         // steps between gain updates
};
template <bool SCHED, bool COST = false>
using RolloutArgs = std::conditional_t<COST, CostArgs, std::conditional_t<SCHED, SchedArgs, DynArgs>>;
// (an alias of its own: the kernels' mangled names spell RolloutArgs out, and they stay what they are)
template <bool SCHED, bool COST, bool GS>
using RolloutArgsGS = std::conditional_t<GS, GainSchedArgs, RolloutArgs<SCHED, COST>>;

// parameters.py:135 / 198-210: x9 = x[3, 4, 7, 8, 9, 10, 11, 17, 16]
F16_DEV double mpc_state(const double *x, int k) { return x[k < 2 ? 3 + k : (k < 7 ? 5 + k : 24 - k)]; }
// sum_k w[k] (x9[k] - x_ref[k])^2 added to J in the order k = 0..8; ref(k) = the lane's reference entry k
template <typename REF>
F16_DEV double cost_state_term(double J, const double *x, const double (&w)[9], REF ref) {
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double d = mpc_state(x, k) - ref(k);
    J += w[k] * d * d;
  }
  return J;
}
// sum_i r[i] (u[1 + i] - u_ref[i])^2 of one row: formed when the row is installed, added once per step taken under it
F16_DEV double cost_command_term(const CostArgs &a, long b0, double u1, double u2, double u3) {
  const double uc[3] = {u1, u2, u3};
  double s = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double d = uc[i] - (a.u_ref ? a.u_ref[i * a.ld0 + b0] : 0.0);
    s += a.w.r[i] * d * d;
  }
  return s;
}

template <int BLOCK, int FI>
__global__ __launch_bounds__(BLOCK) void k_xdot(DynArgs a) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  if (a.fi == 1) stage_tables(tab, a.tab);
  for (long b = (long)blockIdx.x * BLOCK + threadIdx.x; b < a.B; b += (long)gridDim.x * BLOCK) {
    double x[18], u[4], xd[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) x[k] = a.x[k * a.ld + b];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = a.u[k * a.ld + b];
    int st = 0;
    calc_xdot<FI>((const double *)tab, a.lofi, x, u, xd, a.xcg, a.fi, a.flags, st);
#pragma unroll
    for (int k = 0; k < 18; ++k) a.out[k * a.ld + b] = xd[k];
    if (a.status) a.status[b] |= st;
  }
}

// Nlplant proper.  TAB_LDS=false reads the image straight from global/L2: used for tiny batches (the
// single-aircraft drop-in call), where staging 113 KB would cost more than the ~170 gathers it saves.
template <int BLOCK, bool TAB_LDS>
__global__ __launch_bounds__(BLOCK) void k_nlplant(DynArgs a) {
  __shared__ __attribute__((aligned(16))) double tab[TAB_LDS ? TABLE_IMAGE_DOUBLES : 2];
  if (TAB_LDS && a.fi == 1) stage_tables(tab, a.tab);
  const double *T = TAB_LDS ? (const double *)tab : a.tab;
  for (long b = (long)blockIdx.x * BLOCK + threadIdx.x; b < a.B; b += (long)gridDim.x * BLOCK) {
    double x[17], xd[18], qbar, ps;
#pragma unroll
    for (int k = 0; k < 17; ++k) x[k] = a.x[k * a.ld + b];
    int st = 0;
    plant<true>(T, a.lofi, x, xd, a.xcg, a.fi, a.flags, st, qbar, ps);
#pragma unroll
    for (int k = 0; k < 18; ++k) a.out[k * a.ld + b] = xd[k];
    if (a.status) a.status[b] |= st;
  }
}

// One lane = one aircraft, the whole rollout in registers.  TP = the table image the lookups read (plant header: fp64
// values or scaled integers).
// INCT (default numerics only; the strict build and every single-evaluation kernel keep the full sincos): the five sin / cos pairs
// of a step are carried from step to step (trig_advance: rotated by the exact increment of their angles, re-evaluated exactly every
// 32nd step) instead of evaluated from scratch -- ~155 of the ~1,555 wave-instructions of a hifi step.  tgs: lane-indexed LDS slots.
#if defined(F16_FAST_TRIG) && !defined(F16_NO_INC_TRIG)
constexpr bool INC_TRIG = true;
#else
constexpr bool INC_TRIG = false;
#endif
// COST (f16_rollout_cost; SCHED && !LQR only): the lane's cost J is accumulated in a register pair in step order; the nine x_ref
// entries of the lane sit in lane-indexed LDS slots xr like the inputs (XRL), or -- where those do not fit beside the fp64 image,
// the 512-lane workgroups -- are re-read from global memory (L2) at every step.
// STAGES (f16_rollout_rk / _lqr_rk / _cost_rk; SCHED only): 1 = the explicit Euler step of env.py:126, 4 = the classical Runge-Kutta
// step (rk4_step, f16_plant.hpp) with the command -- under the LQR law the action formed from the state at the start of the step --
// held over its four stages.  INCT is false then: every stage evaluates its sin / cos pairs exactly, so nothing but the state is
// carried from step to step and a rollout of n + m steps equals one of n followed by one of m bit for bit.
// LANES: which lanes the calling thread rolls out, and where a scored lane finds its aircraft and its reference.  GridLanes: the
// grid-stride loop of every k_rollout* kernel.  The fused MPPI loop (k_rollout_mppi) hands over the ONE lane of its thread instead
// (MppiLane), whose reference is formed from the initial state and the demands rather than read from a.x_ref.
// (GS) the schedule bookkeeping of a lane with two more counters: steps until the next gain update; updates outside the grid.  They
// ride on the object the other instantiations have anyway -- a variable of their own there, even a dead one, was enough to make the
// compiler order the operands of a scalar OR differently in existing kernels.
template <int N, bool AHEAD>
struct RowAheadGs : RowAhead<N, AHEAD> { int gs_left = 0, gs_cnt = 0; };
struct GridLanes {
  F16_DEV long first(int block) const { return (long)blockIdx.x * block + threadIdx.x; }
  template <typename ARGS> F16_DEV long end(const ARGS &a) const { return a.B; }
  F16_DEV long stride(int block) const { return (long)gridDim.x * block; }
  F16_DEV long aircraft(const CostArgs &a, long b) const { return b % a.B0; }
  F16_DEV double reference(const CostArgs &a, int k, const double *, long b0) const { return a.x_ref[k * a.ld0 + b0]; }
};
struct MppiLane {
  long b, b0;
  F16_DEV long first(int) const { return b; }
  template <typename ARGS> F16_DEV long end(const ARGS &) const { return b + 1; }
  F16_DEV long stride(int) const { return 1; }
  F16_DEV long aircraft(const CostArgs &, long) const { return b0; }
  // calc_MPPI_action: the lane's initial x9 with entries 4..6 = the demands
  F16_DEV double reference(const CostArgs &a, int k, const double *x, long c) const { return k >= 4 && k < 7 ? a.dem[(k - 4) * a.ld0 + c] : mpc_state(x, k); }
};
template <int BLOCK, int FI, typename TP, bool LQR = false, bool INCT = false, bool SCHED = false, bool COST = false, bool XRL = false,
          int STAGES = 1, typename LANES = GridLanes, bool GS = false>
__device__ __forceinline__ void rollout_lanes(const RolloutArgsGS<SCHED, COST, GS> &a, TP T, double (*us)[BLOCK], double (*kq)[BLOCK] = nullptr,
                                              double (*tgs)[BLOCK] = nullptr, double (*xr)[BLOCK] = nullptr, const LANES lanes = {}) {
  static_assert(!COST || (SCHED && !LQR), "the scored rollout is the open-loop scheduled one");
  static_assert(STAGES == 1 || (STAGES == 4 && SCHED && !INCT), "the Runge-Kutta step: scheduled variants, exact sin / cos");
  static_assert(!GS || (LQR && SCHED && !COST), "the gain schedule: the closed loop under a demand schedule");
  for (long b = lanes.first(BLOCK); b < lanes.end(a); b += lanes.stride(BLOCK)) {
    double x[18];
    long b0 = b;                                         // (COST) the aircraft of this lane: the column of x0 / x_ref / u_ref
    double J = 0, ju = 0;                                // (COST) the cost so far; the command term of the row in use
    if constexpr (COST) {
      b0 = lanes.aircraft(a, b);
#pragma unroll
      for (int k = 0; k < 18; ++k) x[k] = a.x0[k * a.ld0 + b0];
      if (XRL) {
#pragma unroll
        for (int k = 0; k < 9; ++k) xr[k][threadIdx.x] = lanes.reference(a, k, x, b0);
      }
    } else {
#pragma unroll
    for (int k = 0; k < 18; ++k) x[k] = a.out[k * a.ld + b];
    }
    [[maybe_unused]] const auto ref = [&](int k) {       // (COST) entry k of the lane's reference
      if constexpr (COST) return XRL ? xr[k][threadIdx.x] : a.x_ref[k * a.ld0 + b0];
      else return 0.0;
    };
    if (!COST || a.nsteps > 0) {                         // (a scored rollout of no steps has no rows)
#pragma unroll
    for (int k = 0; k < 4; ++k) us[k][threadIdx.x] = a.u[k * a.ld + b];
    }
    double ul[3] = {us[1][threadIdx.x], us[2][threadIdx.x], us[3][threadIdx.x]};   // (u_out of an aircraft that never steps: u0)
    if (LQR) {   // K[i][4..6] and the demands: lane-indexed LDS slots like the inputs (constant over the rollout, used once per step)
      if constexpr (!GS) {                                 // (GS: the first gain update, at step 0, fills the nine slots)
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) kq[3 * i + j][threadIdx.x] = a.K[(9 * i + 4 + j) * a.ld + b];
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) kq[9 + j][threadIdx.x] = a.dem[j * a.ld + b];
    }
    int st = !COST && a.status ? a.status[b] : 0;        // (COST: status is an output, every lane starts from 0)
    double *tr = a.traj ? a.traj + b : nullptr;
    int until_store = a.traj_every;
    bool stale = true;                                   // (INCT) the first step evaluates the five pairs exactly
    if constexpr (COST) if (a.nsteps > 0) ju = cost_command_term(a, b0, ul[0], ul[1], ul[2]);
    // SCHED: the row in use sits where the constant input does (us / kq[9..11]); the next one in registers (<= 256 lanes)
    constexpr int NR = LQR ? 3 : 4;
    // 64-lane workgroups (B <= 16,384) count the 32 steps between exact sin / cos evaluations from the start of the ROW, as the
    // chain of launches does for any hold; the larger ones from the start of the launch (the chain's steps when hold % 32 == 0)
    // GS: every kernel that carries the pairs restarts them at every row AND at every gain update -- the segment starts of the chain
    constexpr bool ROW_TRIG = SCHED && INCT && (BLOCK == 64 || GS);
    int t0 = 0;
    std::conditional_t<GS, RowAheadGs<NR, BLOCK <= 256>, RowAhead<NR, BLOCK <= 256>> ra;
    if constexpr (SCHED) { ra.init(a, NR, a.out + b); ra.settle(); }
    for (int t = 0; t < a.nsteps; ++t) {
      // GS: a gain update at the state this step starts from, for frozen aircraft too.  The 48 corner values come from global
      // memory (L2) as one batch of loads right here -- they depend on the state the previous step produced, so there is no
      // earlier place for them -- and the install writes the slots the frozen-gain loop fills once: kq[0..8], us[1..3].
      if constexpr (GS) {
        if (ra.gs_left == 0) {
          ra.gs_left = a.gs_every;
          double g[F16_GS_ENTRIES];
          ra.gs_cnt += gain_lookup(a.grid, a.gtab, x[2], x[6], g);
#pragma unroll
          for (int e = 0; e < 9; ++e) kq[e][threadIdx.x] = g[e];
#pragma unroll
          for (int i = 0; i < 3; ++i) us[1 + i][threadIdx.x] = ul[i] = g[9 + i];      // (as a new launch: u0 until it steps)
          if (ROW_TRIG) { t0 = t; stale = true; }
        }
        --ra.gs_left;
      }
      // env.py:117-124: the reference exit()s; here the aircraft is frozen and flagged
      if (!(a.flags & FLAG_NO_ENVELOPE) && outside_envelope(x)) st |= ST_ENVELOPE;
      if (!(st & ST_ENVELOPE)) {
        double xd[18], u[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = us[k][threadIdx.x];
        if (LQR) {
          const double e0 = kq[9][threadIdx.x] - x[9], e1 = kq[10][threadIdx.x] - x[10], e2 = kq[11][threadIdx.x] - x[11];
#pragma unroll
          for (int i = 0; i < 3; ++i)
            ul[i] = u[1 + i] = lqr_action(kq[3 * i][threadIdx.x], kq[3 * i + 1][threadIdx.x], kq[3 * i + 2][threadIdx.x], e0, e1, e2, u[1 + i]);
        }
        if constexpr (STAGES == 4) {
          rk4_step<FI>(T, a.lofi, x, u, a.dt, a.xcg, a.fi, a.flags, st);
        } else
        if (INCT) {
          const TrigSlots ts{&tgs[0][threadIdx.x], BLOCK};
          if (stale || ((ROW_TRIG ? t - t0 : t) & 31) == 0) { Trig5 g; trig_exact(x, g); trig_store(ts, g); }
          calc_xdot<FI, TP, true>(T, a.lofi, x, u, xd, a.xcg, a.fi, a.flags, st, &ts);
          const double xo5[5] = {x[7], x[8], x[4], x[3], x[5]};
#pragma unroll
          for (int k = 0; k < 18; ++k) x[k] += xd[k] * a.dt;   // env.py:126
          stale = trig_advance(xo5, x, ts);
        } else {
        calc_xdot<FI>(T, a.lofi, x, u, xd, a.xcg, a.fi, a.flags, st);
#pragma unroll
        for (int k = 0; k < 18; ++k) x[k] += xd[k] * a.dt;   // env.py:126
        }
        if constexpr (COST) J = cost_state_term(J + ju, x, a.w.q, ref);
      } else if constexpr (COST) {
        J += a.w.pen;                                    // a step the frozen lane does not take
      }
      if (tr && --until_store == 0) {
        until_store = a.traj_every;
#pragma unroll
        for (int k = 0; k < 18; ++k) __builtin_nontemporal_store(x[k], tr + k * a.ld);
        tr += 18 * a.ld;
      }
      if constexpr (SCHED) if (ra.due(a, NR)) {
        double r[NR];
        ra.take(a, NR, r, a.out + b);
#pragma unroll
        for (int k = 0; k < NR; ++k) (LQR ? kq[9 + k] : us[k])[threadIdx.x] = r[k];
        if (LQR) { ul[0] = us[1][threadIdx.x]; ul[1] = us[2][threadIdx.x]; ul[2] = us[3][threadIdx.x]; }   // (as a new launch: u0 until it steps)
        if (ROW_TRIG) { t0 = t + 1; stale = true; }
        if constexpr (COST) ju = cost_command_term(a, b0, r[1], r[2], r[3]);
      }
    }
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 18; ++k) finite = finite && isfinite(x[k]);
    if (!finite) st |= ST_NONFINITE;
    // WHICH states were outside: a frozen aircraft keeps the state it was frozen with, so the bits are formed here, once
    if (st & ST_ENVELOPE) st |= envelope_state_bits(x);
    if constexpr (COST) {
      a.out[b] = cost_state_term(J, x, a.w.qf, ref);      // the terminal term; `out` is the cost column
      if (a.x_end) {
#pragma unroll
        for (int k = 0; k < 18; ++k) a.x_end[k * a.ld + b] = x[k];
      }
    } else {
#pragma unroll
    for (int k = 0; k < 18; ++k) a.out[k * a.ld + b] = x[k];
    }
    if (a.status) a.status[b] = st;
    if (LQR && a.u_out) {
      a.u_out[b] = us[0][threadIdx.x];
#pragma unroll
      for (int i = 0; i < 3; ++i) a.u_out[(1 + i) * a.ld + b] = ul[i];
    }
    if constexpr (GS) if (a.gs_out) a.gs_out[b] = ra.gs_cnt;
  }
}

// F16_FLAG_ONE_LANE: one lane per aircraft, 64-lane workgroups, every step through the out-of-line euler_step_exact (table image read
// from global memory: no LDS staging) -- ONE instruction sequence for every batch size, the one the closed MPC loop (f16_rollout_mpc)
// steps with.  Same rules as rollout_lanes (envelope freeze, status bits, trajectory samples, u_out); a reproducibility path, not a
// fast one.
// STAGES = 4: the Runge-Kutta step through the out-of-line rk4_step_exact instead.
// The lane loop itself is f16_rollout_exact.inc: included here, and in rollout_exact_lanes for the fused MPPI loop under the flag.
template <bool LQR, bool SCHED = false, bool COST = false, int STAGES = 1>
__global__ __launch_bounds__(64) void k_rollout_exact(RolloutArgs<SCHED, COST> a) {
  static_assert(!COST || (SCHED && !LQR), "the scored rollout is the open-loop scheduled one");
  static_assert(STAGES == 1 || (STAGES == 4 && SCHED), "the Runge-Kutta step: scheduled variants");
  const GridLanes lanes;
  constexpr bool GS = false;
#include "f16_rollout_exact.inc"
}
template <bool LQR, bool SCHED, bool COST, int STAGES, typename LANES, bool GS = false>
__device__ __forceinline__ void rollout_exact_lanes(const RolloutArgsGS<SCHED, COST, GS> &a, const LANES lanes) {
#include "f16_rollout_exact.inc"
}
// the scheduled-gain loop (f16_rollout_lqr_gs) under the flag: the same lane loop with the gain update in it.  A kernel of its own
// (as k_rollout_gs / k_rollout_i_gs below), so that every existing kernel keeps its name and its argument block.
template <int STAGES>
__global__ __launch_bounds__(64) void k_rollout_exact_gs(GainSchedArgs a) {
  rollout_exact_lanes<true, true, false, STAGES, GridLanes, true>(a, GridLanes{});
}

template <int BLOCK, int FI, bool LQR = false, bool SCHED = false, bool COST = false, int STAGES = 1>
__global__ __launch_bounds__(BLOCK) void k_rollout(RolloutArgs<SCHED, COST> a) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  // the four inputs of a lane are constant over the rollout and used once per step: kept in lane-indexed (conflict-free) LDS
  // slots rather than in eight registers that the 512-lane instantiation (256 registers per lane) spilled and reloaded per step
  __shared__ double us[4][BLOCK];
  __shared__ double kq[LQR ? 12 : 1][LQR ? BLOCK : 1];
  constexpr bool INCT = INC_TRIG && STAGES == 1 && BLOCK <= 256 && !(LQR && BLOCK == 256);      // (the ten slots must fit beside the fp64 table image and, closed loop, the gain slots)
  __shared__ double tgs[INCT ? 10 : 1][INCT ? BLOCK : 1];
  constexpr bool XRL = COST && BLOCK <= 256;           // (nine more slots of 512 lanes do not fit beside the fp64 image)
  __shared__ double xr[XRL ? 9 : 1][XRL ? BLOCK : 1];
  static_assert(sizeof(tab) + sizeof(us) + sizeof(kq) + sizeof(tgs) + sizeof(xr) <= 163840, "static LDS of a CU");
  if (a.fi == 1) stage_tables(tab, a.tab);
  rollout_lanes<BLOCK, FI, const double *, LQR, INCT, SCHED, COST, XRL, STAGES>(a, (const double *)tab, us, reinterpret_cast<double (*)[BLOCK]>(kq),
                                                                        reinterpret_cast<double (*)[BLOCK]>(tgs),
                                                                        reinterpret_cast<double (*)[BLOCK]>(xr));
}

// The same rollout on the scaled-integer table image (hifi, default numerics; large batches: the LDS pipe -- 1.5 KB of
// table vertices per aircraft-step as doubles, more than half of its cycles bank-conflict replays of the per-lane gathers --
// is one of the two ceilings of k_rollout there).
template <int BLOCK, bool LQR = false, bool SCHED = false, bool COST = false, int STAGES = 1>
__global__ __launch_bounds__(BLOCK) void k_rollout_i(RolloutArgs<SCHED, COST> a) {
  __shared__ __attribute__((aligned(16))) int tab[i32::IMAGE_INTS];
  __shared__ double us[4][BLOCK];
  __shared__ double kq[LQR ? 12 : 1][LQR ? BLOCK : 1];
  constexpr bool INCT = INC_TRIG && STAGES == 1 && !LQR;      // (closed loop: the gain slots take the room)
  __shared__ double tgs[INCT ? 10 : 1][INCT ? BLOCK : 1];
  __shared__ double xr[COST ? 9 : 1][COST ? BLOCK : 1];
  static_assert(sizeof(tab) + sizeof(us) + sizeof(kq) + sizeof(tgs) + sizeof(xr) <= 163840, "static LDS of a CU");
  {
    const int4 *src = reinterpret_cast<const int4 *>(a.tab32);
    int4 *dst = reinterpret_cast<int4 *>(tab);
    for (int i = threadIdx.x; i < i32::IMAGE_INTS / 4; i += BLOCK) dst[i] = src[i];
    __syncthreads();
  }
  rollout_lanes<BLOCK, 1, TabI32, LQR, INCT, SCHED, COST, COST, STAGES>(a, TabI32{tab}, us, reinterpret_cast<double (*)[BLOCK]>(kq),
                                                                reinterpret_cast<double (*)[BLOCK]>(tgs), reinterpret_cast<double (*)[BLOCK]>(xr));
}

// The scheduled-gain twins of k_rollout<BLOCK, FI, true, true, false, STAGES> and k_rollout_i<BLOCK, true, true, false, STAGES>: the same
// LDS slots (the install of a gain update writes kq[0..8] and us[1..3]: no new slot), the same lane body with GS = true.
template <int BLOCK, int FI, int STAGES = 1>
__global__ __launch_bounds__(BLOCK) void k_rollout_gs(GainSchedArgs a) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  __shared__ double us[4][BLOCK];
  __shared__ double kq[12][BLOCK];
  constexpr bool INCT = INC_TRIG && STAGES == 1 && BLOCK < 256;      // (as k_rollout under the LQR law)
  __shared__ double tgs[INCT ? 10 : 1][INCT ? BLOCK : 1];
  static_assert(BLOCK <= 256 && sizeof(tab) + sizeof(us) + sizeof(kq) + sizeof(tgs) <= 163840, "static LDS of a CU");
  if (a.fi == 1) stage_tables(tab, a.tab);
  rollout_lanes<BLOCK, FI, const double *, true, INCT, true, false, false, STAGES, GridLanes, true>(
      a, (const double *)tab, us, kq, reinterpret_cast<double (*)[BLOCK]>(tgs));
}
template <int BLOCK, int STAGES = 1>
__global__ __launch_bounds__(BLOCK) void k_rollout_i_gs(GainSchedArgs a) {
  __shared__ __attribute__((aligned(16))) int tab[i32::IMAGE_INTS];
  __shared__ double us[4][BLOCK];
  __shared__ double kq[12][BLOCK];
  static_assert(sizeof(tab) + sizeof(us) + sizeof(kq) <= 163840, "static LDS of a CU");
  {
    const int4 *src = reinterpret_cast<const int4 *>(a.tab32);
    int4 *dst = reinterpret_cast<int4 *>(tab);
    for (int i = threadIdx.x; i < i32::IMAGE_INTS / 4; i += BLOCK) dst[i] = src[i];
    __syncthreads();
  }
  rollout_lanes<BLOCK, 1, TabI32, true, false, true, false, false, STAGES, GridLanes, true>(a, TabI32{tab}, us, kq);
}

// The closed MPPI loop as ONE launch (f16_rollout_mppi): one workgroup = one aircraft, its lanes = that aircraft's K samples
// (K <= 256; lanes >= K idle but take part in the barriers and in the table staging).  Per control period, between workgroup barriers:
//   lanes < K        write their rows of the sample set (mppi_write_row: the statement of f16_mppi_sample) into u_seq, in the host
//                    loop's layout, and score them -- the lane body of the scored rollout (rollout_lane / rollout_exact_lane with
//                    COST), which reads back the lane's own column of u_seq and writes cost[lane];
//   -- fence + barrier: the columns and costs are published to the workgroup
//   lanes < 4 S      one (row, command) entry of the softmin blend each, k ascending (blend_walk: the arithmetic of k_mppi_blend);
//                    row 0 goes to u, row r >= 1 to row r - 1 of u_nom, the last row also to the last row of u_nom (the shift);
//   -- fence + barrier
//   lane 0           advances the aircraft `hold` steps under u: the lane body of the scheduled rollout, one row held;
//   -- fence + barrier: the next period's lanes read the new x and u_nom.
// No spin-wait, no ticket, no state shared between workgroups; aircraft are drawn grid-stride.  The table image is staged once per
// launch; the plant advance costs hold steps of ONE lane per period (the other lanes wait at the barrier) against S * hold scored
// steps of all of them: a fraction 1 / (S + 1) of a period's step time.
struct MppiArgs {
  const double *tab, *lofi;
  double *x, *u, *u_nom;           // [18][ld0], [4][ld0], [S][4][ld0]
  const double *dem, *u_ref;       // [3][ld0]; [3][ld0] or null
  double *u_seq, *cost;            // [S][4][ld], [ld]
  double *stats, *traj;            // [nperiods][2][ld0] or null; [nperiods * hold / traj_every][18][ld0] or null
  int32_t *status;                 // [ld0] or null
  long B0, ld0, K, ld;
  int nperiods, S, hold, traj_every;      // (traj_every = hold + 1 without traj)
  double dt, xcg, lambda, sg[3];
  int fi;
  unsigned flags;
  uint32_t key0, key1, period0;
  f16_cost_weights w;
};
// score(CostArgs, lane, aircraft): one sample; advance(SchedArgs, aircraft): the plant under the blended command
template <typename SCORE, typename ADVANCE>
F16_DEV void mppi_periods(const MppiArgs &m, SCORE score, ADVANCE advance) {
  const int tid = threadIdx.x;
  for (long ac = blockIdx.x; ac < m.B0; ac += gridDim.x) {
    const long b = tid * m.B0 + ac;                      // sample tid of this aircraft: its lane in u_seq / cost
    for (int p = 0; p < m.nperiods; ++p) {
      if (tid < m.K) {
        for (int row = 0; row < m.S; ++row)
          mppi_write_row(m.u_nom + (long)row * 4 * m.ld0 + ac, m.ld0, m.u_seq + (long)row * 4 * m.ld + b, m.ld, m.period0 + (uint32_t)p,
                         (uint32_t)row, (uint32_t)tid, (uint32_t)ac, m.key0, m.key1, m.sg[0], m.sg[1], m.sg[2]);
        CostArgs c{};                                    // what f16_rollout_cost fills for the host loop's call
        c.tab = m.tab; c.lofi = m.lofi; c.B = m.K * m.B0; c.ld = m.ld; c.xcg = m.xcg; c.fi = m.fi; c.flags = m.flags;
        c.u = c.seq = m.u_seq; c.out = m.cost; c.nsteps = m.S * m.hold; c.traj_every = c.nsteps + 1; c.dt = m.dt; c.dem = m.dem;
        c.hold = m.hold; c.nrows = m.S; c.x0 = m.x; c.u_ref = m.u_ref; c.B0 = m.B0; c.ld0 = m.ld0; c.w = m.w;
        score(c, b, ac);
      }
      __threadfence_block();
      __syncthreads();
      if (tid < 4 * m.S) {
        const double *cost = m.cost + ac;
        const double mn = blend_min(cost, m.K, m.B0);
        const bool any = mn < INFINITY;
        for (int e = tid; e < 4 * m.S; e += blockDim.x) {
          const int row = e >> 2, cm = e & 3;
          const double *u = m.u_seq + ((long)row * 4 + cm) * m.ld + ac;
          double sw = 0, sw2 = 0, acc[1] = {0};
          blend_walk<1>(cost, u, m.K, m.B0, m.ld, mn, m.lambda, true, sw, sw2, acc);
          const double v = any ? acc[0] / sw : u[0];
          if (row == 0) m.u[cm * m.ld0 + ac] = v;
          else m.u_nom[((long)(row - 1) * 4 + cm) * m.ld0 + ac] = v;
          if (row == m.S - 1) m.u_nom[((long)row * 4 + cm) * m.ld0 + ac] = v;
          if (e == 0 && m.stats) {
            double *st = m.stats + (long)p * 2 * m.ld0 + ac;
            st[0] = any ? mn : 0.0; st[m.ld0] = any ? sw * sw / sw2 : 0.0;
          }
        }
      }
      __threadfence_block();
      __syncthreads();
      if (tid == 0) {
        SchedArgs s{};                                   // f16_rollout(_rk) of `hold` steps under the one row u
        s.tab = m.tab; s.lofi = m.lofi; s.status = m.status; s.B = m.B0; s.ld = m.ld0; s.xcg = m.xcg; s.fi = m.fi; s.flags = m.flags;
        s.u = s.seq = m.u; s.out = m.x; s.nsteps = m.hold; s.traj_every = m.traj_every; s.dt = m.dt; s.hold = m.hold; s.nrows = 1;
        s.traj = m.traj ? m.traj + (long)p * (m.hold / m.traj_every) * 18 * m.ld0 : nullptr;
        advance(s, ac);
      }
      __threadfence_block();
      __syncthreads();
    }
  }
}

// the twin of k_rollout<BLOCK, FI, false, true, true, STAGES>: the same LDS slots, the same lane body
template <int BLOCK, int FI, int STAGES>
__global__ __launch_bounds__(BLOCK) void k_rollout_mppi(MppiArgs m) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  __shared__ double us[4][BLOCK];
  constexpr bool INCT = INC_TRIG && STAGES == 1;
  __shared__ double tgs[INCT ? 10 : 1][INCT ? BLOCK : 1];
  __shared__ double xr[9][BLOCK];
  static_assert(BLOCK <= 256 && sizeof(tab) + sizeof(us) + sizeof(tgs) + sizeof(xr) <= 163840, "static LDS of a CU");
  if (m.fi == 1) stage_tables(tab, m.tab);
  double (*const tg)[BLOCK] = reinterpret_cast<double (*)[BLOCK]>(tgs);
  mppi_periods(m,
               [&](const CostArgs &c, long b, long ac) {
                 rollout_lanes<BLOCK, FI, const double *, false, INCT, true, true, true, STAGES>(c, (const double *)tab, us, nullptr, tg, xr,
                                                                                                 MppiLane{b, ac});
               },
               [&](const SchedArgs &s, long ac) {
                 rollout_lanes<BLOCK, FI, const double *, false, INCT, true, false, false, STAGES>(s, (const double *)tab, us, nullptr, tg, nullptr,
                                                                                                   MppiLane{ac, ac});
               });
}

// F16_FLAG_ONE_LANE: the lane bodies of k_rollout_exact (out-of-line steps, tables from global memory), which is what makes the call
// equal the host loop bit for bit; 64, 128 or 256 lanes by K.
template <int STAGES>
__global__ __launch_bounds__(256) void k_rollout_mppi_exact(MppiArgs m) {
  mppi_periods(m,
               [&](const CostArgs &c, long b, long ac) { rollout_exact_lanes<false, true, true, STAGES>(c, MppiLane{b, ac}); },
               [&](const SchedArgs &s, long ac) { rollout_exact_lanes<false, true, false, STAGES>(s, MppiLane{ac, ac}); });
}

// Four-wavefront rollout (latency regime, hifi): one workgroup = 64 aircraft on the four SIMDs of a CU; the state is
// split by owner (every wave integrates and range-checks what it owns) and the table lookups -- the LDS-latency-bound
// part of a step -- are spread over all four waves as four partial coefficient triples (aero_part<1..4>):
//   wave 0  x[0..8]   trigonometry, navigation + kinematic eqs, longitudinal damping tables | force equations, Euler
//   wave 1  --        longitudinal 3-D/2-D tables; stores the PREVIOUS step's x[0..8] sample that wave 0 published at
//                     step start (takes 9 stores per sample off wave 0's critical path)
//   wave 2  x[9..11]  lateral-directional 3-D/2-D tables                                    | moment equations, Euler
//   wave 3  x[12..17] atmosphere, actuator + flap models (Euler), lateral damping tables
// Two barriers per step; everything that crosses goes through lane-indexed (conflict-free) LDS arrays.
// Same terms as k_rollout (C/nlplant.c:333-377); the six totals are summed in a different order (ulp level).
#ifdef F16_EXP_STAMP4W
#define STAMP(acc) { __builtin_amdgcn_s_waitcnt(0); unsigned long long t1 = __builtin_amdgcn_s_memtime(); acc += t1 - t0; t0 = t1; }
#else
#define STAMP(acc)
#endif
template <bool LQR, bool SCHED = false>
__global__ __launch_bounds__(256) void k_rollout_4w(RolloutArgs<SCHED> a) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  __shared__ double xs[17][64], xt[14][64];  // xs: x[0..16] published at step start ; xt: 4 x 3 partial totals, qbar, ps
  __shared__ int xenv[3][64], xst[4][64];
  {
    const double2 *src = reinterpret_cast<const double2 *>(a.tab);
    double2 *dst = reinterpret_cast<double2 *>(tab);
    for (int i = threadIdx.x; i < TABLE_IMAGE_DOUBLES / 2; i += 256) dst[i] = src[i];
    __syncthreads();
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool envchk = !(a.flags & FLAG_NO_ENVELOPE);
  for (long b0 = (long)blockIdx.x * 64; b0 < a.B; b0 += (long)gridDim.x * 64) {
    const bool valid = b0 + lane < a.B;
    const long b = valid ? b0 + lane : a.B - 1;           // ragged tail: shadow the last aircraft, never stored
    double x[18], u[4];
#pragma unroll
    for (int k = 0; k < 18; ++k) x[k] = a.out[k * a.ld + b];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = a.u[k * a.ld + b];
    double kq[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, ul[3] = {u[1], u[2], u[3]};   // LQR (wave 3): K[i][4..6], demands; last action (u0 if it never steps)
    if (LQR && wave == 3) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) kq[3 * i + j] = a.K[(9 * i + 4 + j) * a.ld + b];
#pragma unroll
      for (int j = 0; j < 3; ++j) kq[9 + j] = a.dem[j * a.ld + b];
    }
    int st = a.status ? a.status[b] : 0;
    double *tr = a.traj ? a.traj + b : nullptr;           // next sample to be written by THIS wave
    int until_store = a.traj_every;
    constexpr int NR = LQR ? 3 : 4;
    RowAhead<NR, false> ra;                                // SCHED: wave 3 owns the inputs and re-loads them right after their last use
    if constexpr (SCHED) { ra.init(a, NR, a.out + b, 0, wave == 3); ra.settle(); }
#ifdef F16_EXP_STAMP4W
    unsigned long long tA = 0, tB = 0, tC = 0, tD = 0, t0 = __builtin_amdgcn_s_memtime();
#endif
    for (int t = 0; t <= a.nsteps; ++t) {
      const bool last = t == a.nsteps;                    // extra trip: only flushes the final x[0..8] sample
      // ---- step start: envelope test on the owned states (env.py:117-124), publish them
      if (wave == 0) {
        xenv[0][lane] = envchk && (x[2] < 0 || x[2] > 100000 || x[6] < 0 || x[6] > 900 || x[7] < -20. || x[7] > 90 ||
                                   x[8] < -30. || x[8] > 30);
#pragma unroll
        for (int k = 0; k < 9; ++k) xs[k][lane] = x[k];
      } else if (wave == 2) {
        xenv[1][lane] = envchk && (x[9] < -300 || x[9] > 300 || x[10] < -100 || x[10] > 100 || x[11] < -50 || x[11] > 50);
#pragma unroll
        for (int k = 9; k < 12; ++k) xs[k][lane] = x[k];
      } else if (wave == 3) {
        xenv[2][lane] = envchk && (x[12] < 1000 || x[12] > 19000 || x[13] < -25 || x[13] > 25 || x[14] < -21.5 ||
                                   x[14] > 21.5 || x[15] < -30. || x[15] > 30 || x[16] < 0. || x[16] > 25);
#pragma unroll
        for (int k = 12; k < 17; ++k) xs[k][lane] = x[k];
      }
      STAMP(tD)
      __syncthreads();
      STAMP(tA)
      if (wave == 1 && tr && t > 0 && --until_store == 0) {   // sample of the step that just finished
        until_store = a.traj_every;
        if (valid) {
#pragma unroll
          for (int k = 0; k < 9; ++k) __builtin_nontemporal_store(xs[k][lane], tr + k * a.ld);
        }
        tr += 18 * a.ld;
      }
      if (last) break;
      if (xenv[0][lane] | xenv[1][lane] | xenv[2][lane]) st |= ST_ENVELOPE;
      const bool live = !(st & ST_ENVELOPE);
      // every wave sees the full published state (its own part is identical to its registers)
      double xa[17];
#pragma unroll
      for (int k = 0; k < 17; ++k) xa[k] = xs[k][lane];
      Pre p;
      double xd[18], o[3];
      int sa = 0;
      bool newrow = false;
      if constexpr (SCHED) newrow = ra.due(a, NR);
      if (wave == 0) {
        plant_pre<false>(xa, p, xd);
        aero_part<3>((const double *)tab, xa, a.flags, o, sa);       // longitudinal damping derivatives (1-D tables)
      } else if (wave == 1) {
        aero_part<1>((const double *)tab, xa, a.flags, o, sa);       // longitudinal 3-D / 2-D tables
      } else if (wave == 2) {
        aero_part<2>((const double *)tab, xa, a.flags, o, sa);       // lateral-directional 3-D / 2-D tables
      } else {
        double vt = xa[6];
        if (vt <= 0.01) vt = 0.01;
        double mach, qbar, ps;
        atmos_dev(xa[2], vt, mach, qbar, ps);
        xt[12][lane] = qbar; xt[13][lane] = ps;
        aero_part<4>((const double *)tab, xa, a.flags, o, sa);       // lateral damping derivatives (1-D tables)
        if (live) {
          double xq[18];
#pragma unroll
          for (int k = 0; k < 17; ++k) xq[k] = xa[k];
          xq[17] = x[17];
          if (LQR) {
            const double e0 = kq[9] - xa[9], e1 = kq[10] - xa[10], e2 = kq[11] - xa[11];
            double uc[4] = {u[0], 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 3; ++i) ul[i] = uc[1 + i] = lqr_action(kq[3 * i], kq[3 * i + 1], kq[3 * i + 2], e0, e1, e2, u[1 + i]);
            actuators_dev(xq, uc, qbar, ps, xd);
          } else
          actuators_dev(xq, u, qbar, ps, xd);
#pragma unroll
          for (int k = 12; k < 18; ++k) x[k] += xd[k] * a.dt;   // env.py:126 on the actuator / flap states
        }
        if (tr && --until_store == 0) {
          until_store = a.traj_every;
          if (valid) {
#pragma unroll
            for (int k = 12; k < 18; ++k) __builtin_nontemporal_store(x[k], tr + k * a.ld);
          }
          tr += 18 * a.ld;
        }
        if constexpr (SCHED) if (newrow) {
          ra.take(a, NR, LQR ? kq + 9 : u, a.out + b);
          if (LQR) { ul[0] = u[1]; ul[1] = u[2]; ul[2] = u[3]; }      // (as a new launch: u0 until it steps)
        }
      }
      // partial totals: wave 1 -> 0..2 (long. static), wave 0 -> 3..5 (long. damping), wave 2 -> 6..8, wave 3 -> 9..11
      const int slot = wave == 1 ? 0 : (wave == 0 ? 3 : (wave == 2 ? 6 : 9));
      xt[slot][lane] = o[0]; xt[slot + 1][lane] = o[1]; xt[slot + 2][lane] = o[2];
      xst[wave][lane] = sa;
      STAMP(tB)
      __syncthreads();
      STAMP(tC)
      // ---- second half: force equations on wave 0 || moment equations on wave 2
      if (wave == 0 || wave == 2) {
        double ls[3], ldm[3], ts[3], td[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { ls[k] = xt[k][lane]; ldm[k] = xt[3 + k][lane]; ts[k] = xt[6 + k][lane]; td[k] = xt[9 + k][lane]; }
        Totals tt;
        compose_totals(ls, ldm, ts, td, a.xcg, tt);
        if (wave == 0) {
          if (live) {
            p.qbar = xt[12][lane]; p.ps = xt[13][lane];
            st |= xst[0][lane] | xst[1][lane] | xst[2][lane] | xst[3][lane];
            plant_forces(xa, p, tt.Cx, tt.Cy, tt.Cz, xd);
#pragma unroll
            for (int k = 0; k < 9; ++k) x[k] += xd[k] * a.dt;   // env.py:126
          }
        } else {
          if (live) {
            plant_moments(x[9], x[10], x[11], xt[12][lane], tt.Cl, tt.Cm, tt.Cn, xd);
#pragma unroll
            for (int k = 9; k < 12; ++k) x[k] += xd[k] * a.dt;
          }
          if (tr && --until_store == 0) {
            until_store = a.traj_every;
            if (valid) {
#pragma unroll
              for (int k = 9; k < 12; ++k) __builtin_nontemporal_store(x[k], tr + k * a.ld);
            }
            tr += 18 * a.ld;
          }
        }
      }
    }
#ifdef F16_EXP_STAMP4W
    if (lane == 0 && blockIdx.x == 0 && a.traj) {   // diagnostic build: cycles per segment, per wave, into trajectory row 2
      double *d = a.traj + 18 * a.ld * 2 + wave * 4;
      d[0] = (double)tD; d[1] = (double)tA; d[2] = (double)tB; d[3] = (double)tC;
    }
#endif
    if (valid && wave != 1) {
      bool finite = true;
      const int k0 = wave == 0 ? 0 : (wave == 2 ? 9 : 12), k1 = wave == 0 ? 9 : (wave == 2 ? 12 : 18);
#pragma unroll
      for (int k = 0; k < 18; ++k)
        if (k >= k0 && k < k1) { finite = finite && isfinite(x[k]); a.out[k * a.ld + b] = x[k]; }
      // (which states were outside: a frozen aircraft keeps the state it was frozen with; every owner reports its own states)
      if (st & ST_ENVELOPE) st |= envelope_state_bits(x) & (((1 << k1) - (1 << k0)) << 8);
      if (a.status) atomicOr(&a.status[b], st | (finite ? 0 : ST_NONFINITE));
      if (LQR && wave == 3 && a.u_out) {
        a.u_out[b] = u[0];
#pragma unroll
        for (int i = 0; i < 3; ++i) a.u_out[(1 + i) * a.ld + b] = ul[i];
      }
    }
    __syncthreads();
  }
}

// Quad rollout (B <= 4096, hifi): FOUR LANES per aircraft, 16 aircraft per workgroup, so the reference batch of 4096
// fills all 256 CUs (the 4-wave kernel above occupies 64) and every role below runs sub-lane-parallel wherever the
// arithmetic is uniform (f16_plant_quad.hpp): a step costs a CU far fewer wave-instructions.  Lane l = 4 a + s.
//           owns      first half of a step (barrier A .. barrier B)                         | second half (barrier B .. barrier A)
//   wave 0  --        Cx, Cz, Cm totals on sub-lanes 0,1,2 (3-D / 2-D / 1-D longitudinal    | sin/cos of the next step's psi
//                     tables) and the rate-damping parts of Cy, Cn, Cl                      |   (GROUPS = 1)
//   wave 1  x[9..11]  Cy, Cn, Cl static totals on sub-lanes 0,1,2; rate products of the     | moment equations, Euler
//                     moment equations
//   wave 2  x[0..8]   sin/cos of phi, theta, beta, alpha on sub-lanes 0..3; kinematic +     | force equations, Euler
//                     navigation equations, Euler on x[0..5]; GROUPS = 2: the trajectory
//                     sample
//   wave 3  x[12..17] atmosphere; the four actuators on sub-lanes 0..3; flap model, Euler;  | the altitude part of the next step's
//                     the LQR law and the input schedule                                    |   atmosphere, its log's quotient and
//                                                                                           |   polynomial (GROUPS = 1)
//   wave 4  --        GROUPS = 1 only (320 threads): the trajectory sample -- five reads of | --
//                     the published state per lane, five stores when a sample is due
// GROUPS = 1: THE SAMPLES ARE STORED BY A FIFTH WAVE.  None of the sample's work feeds the step, and on wave 2 it stood in a half that
// wave paces: the reads, the counter and its branch, five address computations and stores, and the scalars of all that, which pushed
// wave 2's lane masks out into lane moves.  The store wave runs the same loop text with role index 4, so it executes the same barriers;
// it owns the sample pointer and counter, keeps no state across its loop (what the common prologue loads in front of the role
// switch is dead for it), reads no envelope flag, reports no status and writes nothing in the epilogue.  Five waves on four
// SIMDs: two share one, so the kernel is compiled for 256 vector registers (it used 250 / 254 before) and the dispatcher picks the
// pair (what the stamps say about it).
// Both table waves re-use the last step's cells while every lane stays inside its own (quad_br_cached), with the cell the refined
// reciprocal of its width (lambda on such a step is one subtraction and one product, no v_rcp_f64 chain and no guard), and the
// TABLE VALUES read then (LongCorners / LatCorners, f16_plant_quad.hpp: the four / eight corner sets, the 1-D rows, the 45-degree
// node): on such a step -- 93 % of the workload's -- a table wave forms no table address and reads nothing from LDS but the
// published state; the values are re-read on a step on which a lane has left its cell, at launch start and for every group of
// aircraft.  GROUPS = 2 keeps the full lookup and fresh values on every step and psi on wave 2 (sub-lane 2, beta in a second
// round): the cache's registers spill there.
// Owned states are replicated over the sub-lanes of their wave; two barriers per step as in k_rollout_4w.
// GROUPS = 1: EVERY ROLE HAS A STEP LOOP OF ITS OWN (f16_quad_steps.inc, included once per role): the role index is wave-uniform
// (readfirstlane), one scalar switch behind the common prologue picks the loop, and a loop holds that role's statements alone.  In one shared loop a wave reached
// its code by jumping over the other three roles' blocks three times per step (publish, first half, second half), every jump a
// lane-mask save, test and restore, and every role's loop-carried values were live across the whole body.  All four loops execute
// the same barrier sequence -- A, B per step and A alone on the extra trip -- which is what keeps the workgroup in step:
// s_barrier does not look at the lane mask, so the dispatch must stay a scalar branch (tools/quad_role_loops.py checks both).
// What a role hands from its first half to its second is pinned where the first half ends (quad_taken_here): the compiler would
// otherwise move that arithmetic behind barrier B and contract it differently.  GROUPS = 2 keeps one shared loop (same text).
// GROUPS = 2 (4096 < B <= 8192): two independent 16-aircraft groups per workgroup share the LDS table image, one role
// wave of each on every SIMD -- the two dependency chains interleave.
// GROUPS = 1 takes the constants of its sin/cos pair and of the atmosphere's exp / log from REGISTERS THAT HOLD THEM FOR THE WHOLE
// LAUNCH: each role loads its own table from QUAD_K (constant memory, f16_plant.hpp) once, in front of its own step loop
// (f16_quad_steps.inc), and no step loads it again.  Waves 0 (psi) and 3 (atmosphere) keep theirs in scalar registers, the
// constant the scalar operand of a three-address FMA; wave 2 (trigonometry) keeps its 21 doubles in lane-uniform vector registers
// and issues the same FMA with three vector operands (chosen when its loop's lane masks and sample scalars left no room for 42
// scalar registers; the scalar form with the sample on a wave of its own: DESIGN.md, the store wave's section).  (Loaded at the
// top of a role's part of every step, as before, the loads were issued BEHIND the role's wait for its LDS reads and the first
// multiply waited for them: 228 / 625 / 135 cycles per step on waves 2 / 3 / 0, DESIGN.md.)  As literals
// the constants cost the trigonometry, psi and atmosphere roles a register move in front of nearly every polynomial step, and 28
// vector registers for the sin/cos table.  Same operations, same operands, same order.
// Wave 2 publishes x[0..5] and tests x[2] where they become final, behind barrier B, under the wait for the totals; between the
// last Euler update and barrier A it writes x[6..8] and its envelope flag only.  (The box test on x[6..8] made by the waves that
// read them, with no flag write in front of the barrier, was built and measured: not distinguishable, DESIGN.md.)
// GROUPS = 1: the altitude-only part of the atmosphere -- tfac, the temperature with its 35,000 ft select, tfac^4 and the
// extended-precision quotient of log tfac (atmos_alt, log_k_quot, f16_plant.hpp) -- is evaluated HALF A STEP AHEAD, in wave 3's second
// half, which was empty: x[2] is final since wave 2's first half, which hands it over beside psi.  Behind barrier A wave 3 is left
// with the log's polynomial and sums, the exp, the density and -- the only part that needs this step's airspeed -- qbar.  The cut
// stands where the stamps put it: with the whole log ahead wave 3 paced the second half (883 cycles against wave 1's 728).
// A wave reads its OWN states from its registers, not from LDS: wave 2's sin / cos polynomial starts without an LDS round trip.
constexpr int quad_block_threads(int groups) { return groups == 1 ? 320 : 256 * groups; }
template <int GROUPS, bool LQR = false, bool SCHED = false>
__global__ __launch_bounds__(quad_block_threads(GROUPS)) void k_rollout_q(RolloutArgs<SCHED> a) {
  constexpr int NA = 16 * GROUPS;
  constexpr bool G1 = GROUPS == 1;     // cell re-use and psi on wave 0: one group only (at GROUPS = 2 the registers spill)
  constexpr int NT = quad_block_threads(GROUPS);           // threads of the block: four role waves per group; GROUPS = 1: and the store wave
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  __shared__ double xs[18][NA], xt[11][NA];                // published state; Cx Cz Cm | Cy Cn Cl static | qbar ps | Cy Cn Cl damping
  __shared__ int xenv[3][NA], xst[2][NA];
  // psi after the step (wave 2 -> wave 0), its sin / cos (wave 0 -> wave 2); GROUPS = 1: [3] the altitude after the step (wave 2 ->
  // wave 3, written with psi in one ds_write2_b64)
  __shared__ double xpsi[G1 ? 4 : 3][NA];
#ifdef F16_EXP_STAMPQ
  const unsigned long long tstage0 = __builtin_amdgcn_s_memtime();
#endif
  {
    const double2 *src = reinterpret_cast<const double2 *>(a.tab);
    double2 *dst = reinterpret_cast<double2 *>(tab);
    for (int i = threadIdx.x; i < TABLE_IMAGE_DOUBLES / 2; i += NT) dst[i] = src[i];
    __syncthreads();
  }
#ifdef F16_EXP_STAMPQ
  const unsigned long long tstage = __builtin_amdgcn_s_memtime() - tstage0;     // kernel entry to the first barrier: the table staging
#endif
  // GROUPS = 1: the role index from a scalar register (wave-uniform), so that the role dispatch is a scalar branch; 4 = the store wave
  const int role = G1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : (threadIdx.x >> 6) & 3;
  const int grp = G1 ? 0 : threadIdx.x >> 8, lane = threadIdx.x & 63, ac = 16 * grp + (lane >> 2), s = lane & 3;
  const bool envchk = !(a.flags & FLAG_NO_ENVELOPE);
  for (long b0 = (long)blockIdx.x * NA; b0 < a.B; b0 += (long)gridDim.x * NA) {
    const bool valid = b0 + ac < a.B;
    const long b = valid ? b0 + ac : a.B - 1;              // ragged tail: shadow the last aircraft, never stored
    double x[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) x[k] = a.out[k * a.ld + b];
    double ucmd = a.u[s * a.ld + b];                       // wave 3: sub-lane s drives actuator s
    // LQR (wave 3, sub-lanes 1..3): row s - 1 of K, columns 4..6, and the demands; the action of the last step
    double kr0 = 0, kr1 = 0, kr2 = 0, dm0 = 0, dm1 = 0, dm2 = 0, ulast = ucmd;
    if (LQR && role == 3) {
      const long row = 9 * (s > 0 ? s - 1 : 0) + 4;
      kr0 = a.K[row * a.ld + b]; kr1 = a.K[(row + 1) * a.ld + b]; kr2 = a.K[(row + 2) * a.ld + b];
      dm0 = a.dem[b]; dm1 = a.dem[a.ld + b]; dm2 = a.dem[2 * a.ld + b];
    }
    double xact = s == 0 ? x[12] : (s == 1 ? x[13] : (s == 2 ? x[14] : x[15]));   // wave 3: its actuator state
    int st = a.status ? a.status[b] : 0;
    double *tr = a.traj ? a.traj + b : nullptr;            // next sample (from the published state; GROUPS = 1: by the store wave)
    int until_store = a.traj_every;
    QuadCell qc = quad_cell_none();                        // waves 0 / 1: cells of the last full lookup (none at launch start)
    LongCorners klong = {};                                // GROUPS = 1, wave 0: the table values of that lookup (a role's loop keeps its own alone)
    LatCorners klat = {};                                  //             wave 1
    // SCHED: wave 3 owns the inputs and re-loads them right after their last use in a step -- sub-lane s its own command of the
    // new row; under the LQR law sub-lane j = 0..2 demand j (dmq), handed round the quad at the point of use: one 8-byte load
    // per lane and row either way, and four registers fewer than three demands on every sub-lane (GROUPS = 2 has none to spare)
    RowAhead<1, false> ra;
    double dmq = 0;
    const int rs = LQR && s == 3 ? 2 : s;                  // the value of a row this sub-lane reads
    if constexpr (SCHED) {
      dmq = s == 0 ? dm0 : (s == 1 ? dm1 : dm2);
      ra.init(a, LQR ? 3 : 4, a.out + b, rs * a.ld, role == 3);
      ra.settle();
    }
    // (GROUPS = 1: wave 0 evaluates sin / cos of the first step's psi in front of its own loop, with the table it loads there)
#ifdef F16_EXP_STAMPQ
    unsigned long long tA = 0, tB = 0, tC = 0, tD = 0, t0 = __builtin_amdgcn_s_memtime();
    // -DF16_EXP_STAMPQ (or =1): every stamp waits for ALL counters, wave 2's sample stores included.  -DF16_EXP_STAMPQ=2: for the
    // LDS / scalar counter alone (vmcnt and expcnt left at their maxima), so that wave 2's first half reads without the
    // completion of its stores folded in.
#if F16_EXP_STAMPQ + 0 == 2
#define QSTAMP_WAIT 0xC07F
#else
#define QSTAMP_WAIT 0
#endif
#define QSTAMP(acc) { __builtin_amdgcn_s_waitcnt(QSTAMP_WAIT); unsigned long long t1 = __builtin_amdgcn_s_memtime(); acc += t1 - t0; t0 = t1; }
#else
#define QSTAMP(acc)
#endif
    // The step loop (f16_quad_steps.inc).  GROUPS = 1: one copy per role behind a scalar switch; GROUPS = 2: one shared loop, as
    // before (four loops spill more there).
    if constexpr (G1) {
      switch (role) {
        case 0: {
          constexpr int wave = 0;
#include "f16_quad_steps.inc"
        } break;
        case 1: {
          constexpr int wave = 1;
#include "f16_quad_steps.inc"
        } break;
        case 2: {
          constexpr int wave = 2;
#include "f16_quad_steps.inc"
        } break;
        case 4: {
          constexpr int wave = 4;
#include "f16_quad_steps.inc"
        } break;
        default: {
          constexpr int wave = 3;
#include "f16_quad_steps.inc"
        } break;
      }
    } else {
      const int wave = role;
#include "f16_quad_steps.inc"
    }
#ifdef F16_EXP_STAMPQ
    if (lane == 0 && blockIdx.x == 0 && a.traj) {   // diagnostic build: cycles per segment, per wave, into trajectory row 2
      // (the store wave's row in state row 2: columns 16.. of row 0 belong to the next workgroup's aircraft, whose sample may be
      //  written back from another L2 after this)
      double *d = a.traj + 18 * a.ld * 2 + (role < 4 ? role * 4 : 2 * a.ld);
      d[0] = (double)tD; d[1] = (double)tA; d[2] = (double)tB; d[3] = (double)tC;
      a.traj[18 * a.ld * 2 + a.ld + role] = (double)tstage;   // (state row 1 of the same sample; once per launch, not per step)
    }
#endif
    // ---- write the final state back (owners), flags
    if (valid) {
      if (role == 2 && s == 0) {
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) { finite = finite && isfinite(x[k]); a.out[k * a.ld + b] = x[k]; }
        // (which states were outside: a frozen aircraft keeps the state it was frozen with; every owner reports its own states)
        if (st & ST_ENVELOPE) st |= envelope_state_bits(x) & (0x1FF << 8);
        if (a.status) atomicOr(&a.status[b], st | (finite ? 0 : ST_NONFINITE));
      } else if (role == 1 && s == 0) {
        bool finite = true;
#pragma unroll
        for (int k = 9; k < 12; ++k) { finite = finite && isfinite(x[k]); a.out[k * a.ld + b] = x[k]; }
        if (st & ST_ENVELOPE) st |= envelope_state_bits(x) & (0x7 << 17);
        if (a.status) atomicOr(&a.status[b], st | (finite ? 0 : ST_NONFINITE));
      } else if (role == 3) {
        a.out[(12 + s) * a.ld + b] = xact;
        bool finite = isfinite(xact);
        if (s < 2) { const double v = s == 0 ? x[16] : x[17]; finite = finite && isfinite(v); a.out[(16 + s) * a.ld + b] = v; }
        if (st & ST_ENVELOPE) {
          const double lim = s == 1 ? 25.0 : (s == 2 ? 21.5 : 30.0);
          if (s == 0 ? (xact < 1000 || xact > 19000) : (xact < -lim || xact > lim)) st |= 1 << (8 + 12 + s);
          if (s == 0 && (x[16] < 0. || x[16] > 25)) st |= 1 << (8 + 16);
        }
        if (a.status) atomicOr(&a.status[b], st | (finite ? 0 : ST_NONFINITE));
        if (LQR && a.u_out) a.u_out[s * a.ld + b] = ulast;
      }
    }
    __syncthreads();
  }
}

// The reference's LINEAR-model closed loops (test_env_mk2.py:46-62 `LQR(linear=True)` -- what main.py:35 runs -- and
// test_env.py:501-576 `test_LQR_lin`): per step  u = -K (x_ref - x) + u0,  x = Ad x + Bd u  on the reduced model (9 states, 3 inputs).
// One lane = one aircraft; its three matrices (135 doubles) are loaded ONCE and stay in registers (one wave per SIMD, 512 registers
// per lane), so a step is 135 fused multiply-adds and, with every sample stored, 96 bytes of HBM writes: 2.8 FLOP per byte, under the
// fp64 ridge -- the stored rollout is HBM-write-bound.  track: bit j set = entry j of the reference is given (x_ref[j]); clear =
// the reference follows the current state (env.py:362-367: x_ref = copy(x); x_ref[4:7] = demands).
struct LinArgsL {
  double *x;            // [9][ld] in place
  const double *Ad, *Bd, *K, *xref, *u0;
  double *trx, *tru;    // [T / every][9][ld], [T / every][3][ld]; may be null
  long B, ld;
  int nsteps, every;
  unsigned track;
};
__global__ __launch_bounds__(64, 1) void k_rollout_lqr_linear(LinArgsL a) {
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  double A[81], Bm[27], K[27], x[9], xr[9], u0[3];
#pragma unroll
  for (int e = 0; e < 81; ++e) A[e] = a.Ad[e * a.ld + b];
#pragma unroll
  for (int e = 0; e < 27; ++e) { Bm[e] = a.Bd[e * a.ld + b]; K[e] = a.K[e * a.ld + b]; }
#pragma unroll
  for (int j = 0; j < 9; ++j) { x[j] = a.x[j * a.ld + b]; xr[j] = a.xref[j * a.ld + b]; }
#pragma unroll
  for (int c = 0; c < 3; ++c) u0[c] = a.u0 ? a.u0[c * a.ld + b] : 0.0;
  double *px = a.trx ? a.trx + b : nullptr, *pu = a.tru ? a.tru + b : nullptr;
  int until = a.every;
  for (int t = 0; t < a.nsteps; ++t) {
    double e[9], u[3], xn[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) e[j] = (((a.track >> j) & 1u) ? xr[j] : x[j]) - x[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < 9; ++j) s += K[9 * c + j] * e[j];
      u[c] = -s + u0[c];                                     // env.py:371 / test_env.py:555
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      double s = 0.0, v = 0.0;
#pragma unroll
      for (int j = 0; j < 9; ++j) s += A[9 * r + j] * x[j];
#pragma unroll
      for (int c = 0; c < 3; ++c) v += Bm[3 * r + c] * u[c];
      xn[r] = s + v;                                         // test_env_mk2.py:58 / test_env.py:556
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) x[r] = xn[r];
    if (--until == 0) {
      until = a.every;
      if (px) {
#pragma unroll
        for (int r = 0; r < 9; ++r) __builtin_nontemporal_store(x[r], px + r * a.ld);
        px += 9 * a.ld;
      }
      if (pu) {
#pragma unroll
        for (int c = 0; c < 3; ++c) __builtin_nontemporal_store(u[c], pu + c * a.ld);
        pu += 3 * a.ld;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 9; ++r) a.x[r * a.ld + b] = x[r];
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_xdot_na(DynArgs a) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  if (a.fi == 1) stage_tables(tab, a.tab);
  for (long b = (long)blockIdx.x * BLOCK + threadIdx.x; b < a.B; b += (long)gridDim.x * BLOCK) {
    double sv[18], xd9[9];
#pragma unroll
    for (int k = 0; k < 18; ++k) sv[k] = a.x[k * a.ld + b];
    // env.py:172-177: scatter x9 -> mpc_x_idx [3,4,7,8,9,10,11,17,16], u3 -> [13,14,15]
    sv[3] = a.u[0 * a.ld + b]; sv[4] = a.u[1 * a.ld + b]; sv[7] = a.u[2 * a.ld + b]; sv[8] = a.u[3 * a.ld + b];
    sv[9] = a.u[4 * a.ld + b]; sv[10] = a.u[5 * a.ld + b]; sv[11] = a.u[6 * a.ld + b];
    sv[17] = a.u[7 * a.ld + b]; sv[16] = a.u[8 * a.ld + b];
    sv[13] = a.u3[0 * a.ld + b]; sv[14] = a.u3[1 * a.ld + b]; sv[15] = a.u3[2 * a.ld + b];
    int st = 0;
    calc_xdot_na((const double *)tab, a.lofi, sv, xd9, a.xcg, a.fi, a.flags, st);
#pragma unroll
    for (int k = 0; k < 9; ++k) a.out[k * a.ld + b] = xd9[k];
    if (a.status) a.status[b] |= st;
  }
}

}  // namespace f16

using namespace f16;

// ------------------------------------------------------------------------------------ launchers (geometry and argument rules:
// f16_rollout_common.hpp)

// (k_xdot: the lofi model gets an instantiation with the fidelity fixed at compile time (3.94 vs 4.6 ms per 1000 steps at
// B=4096).  For hifi the run-time-flag kernel measured FASTER than a compile-time one (4.59 vs 4.65 ms; 5.31 vs 4.85 G
// steps/s at B=262144: the scheduler does worse on the merged basic block), so hifi keeps the run-time path.)
extern "C" int f16_xdot_batch(f16_ctx *ctx, const double *x, const double *u, double *xdot, int32_t *status, long B,
                              long ld, double xcg, int fi_flag, unsigned flags, void *stream) {
  if (int rc = check_common(ctx, x, xdot, B, ld)) return rc;
  if (!u) return set_error(F16_EINVAL, "u is NULL");
  if (B == 0) return F16_OK;
  DynArgs a = base_args<DynArgs>(ctx, B, ld, xcg, fi_flag, flags, status);
  a.x = x; a.u = u; a.out = xdot;
  const Geometry g = geometry(B, fi_flag);
  by_block(g, [&](auto block) {
    constexpr int BLOCK = decltype(block)::value;
    if (fi_flag == 0) hipLaunchKernelGGL((k_xdot<BLOCK, 0>), dim3(g.grid), dim3(BLOCK), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_xdot<BLOCK, -1>), dim3(g.grid), dim3(BLOCK), 0, (hipStream_t)stream, a);
  });
  return hip_check(hipGetLastError(), "f16_xdot_batch launch");
}

extern "C" int f16_nlplant_batch(f16_ctx *ctx, const double *xu, double *xdot, int32_t *status, long B, long ld,
                                 double xcg, int fi_flag, unsigned flags, void *stream) {
  if (int rc = check_common(ctx, xu, xdot, B, ld)) return rc;
  if (B == 0) return F16_OK;
  DynArgs a = base_args<DynArgs>(ctx, B, ld, xcg, fi_flag, flags, status);
  a.x = xu; a.out = xdot;
  if (B <= 256) {
    hipLaunchKernelGGL((k_nlplant<64, false>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  } else {
    const Geometry g = geometry(B, fi_flag);
    by_block(g, [&](auto block) {
      constexpr int BLOCK = decltype(block)::value;
      hipLaunchKernelGGL((k_nlplant<BLOCK, true>), dim3(g.grid), dim3(BLOCK), 0, (hipStream_t)stream, a);
    });
  }
  return hip_check(hipGetLastError(), "f16_nlplant_batch launch");
}

// The launch rules of the five plant rollouts, in this one place.
// LQR = true: the closed loop of f16_rollout_lqr (same launch rules; the one-lane kernels keep K[i][4..6] and the demands in
// lane-indexed LDS slots, which a 512-lane workgroup has room for only beside the integer table image)
// SCHED = true: the same rules for f16_rollout_sched / f16_rollout_lqr_sched -- every kernel has a scheduled twin, so a schedule
// never moves a batch to another kernel family.
// COST = true: f16_rollout_cost takes the same rules without the quad and four-wave branches (those kernels split the state
// over four role waves and have no scored twin), so a scored batch of B <= 16,384 hifi lanes runs the 64-lane one-lane kernel.
// STAGES = 4 (f16_rollout_rk / _lqr_rk / _cost_rk with F16_INT_RK4): the same rules without the quad and four-wave branches, as for
// COST (an RK4 twin of the role-wave kernels is out of scope), and with a 256-lane ceiling: the Runge-Kutta step keeps 54 doubles
// more than the Euler step live across a plant evaluation, which the 256 registers per lane of a 512-lane workgroup do not hold
// (profiles/rollout_rk4_resources.txt: the 512-lane instantiations, built with -DF16_RK4_512 for that table alone, have scratch
// traffic inside the step loop), so from 131,072 aircraft on an RK4 rollout stays at one wave per SIMD.
#ifdef F16_RK4_512
constexpr bool RK4_512 = true;      // (resource table only: instantiate and route the 512-lane RK4 kernels)
#else
constexpr bool RK4_512 = false;
#endif
// GS = true (f16_rollout_lqr_gs): the same rules without the quad and four-wave branches, as for COST and STAGES = 4 (a scheduled-gain
// twin of the role-wave kernels is out of scope), on the kernels k_rollout_gs / k_rollout_i_gs / k_rollout_exact_gs.
template <bool LQR, bool SCHED, bool COST, int STAGES = 1, bool GS = false>
static int rollout_dispatch(f16_ctx *ctx, RolloutArgsGS<SCHED, COST, GS> &a, void *stream) {
  const hipStream_t st = (hipStream_t)stream;
  const long B = a.B;
  const bool hifi = a.fi == 1;
  static const long max4w = [] { const char *e = getenv("F16_ROLLOUT_4W_MAXB"); return e ? atol(e) : 64L * 256; }();
  static const long maxq = [] { const char *e = getenv("F16_ROLLOUT_QUAD_MAXB"); return e ? atol(e) : 16L * 256; }();
  const char *const what = COST ? "f16_rollout_cost launch" : "f16_rollout launch";
  if (a.flags & F16_FLAG_ONE_LANE) {
    // results independent of the batch size: ONE kernel for every B, its step an out-of-line function (k_rollout_exact)
    if constexpr (GS) hipLaunchKernelGGL((k_rollout_exact_gs<STAGES>), one_lane_grid(B), dim3(64), 0, st, a);
    else
    hipLaunchKernelGGL((k_rollout_exact<LQR, SCHED, COST, STAGES>), one_lane_grid(B), dim3(64), 0, st, a);
    return hip_check(hipGetLastError(), what);
  }
  if constexpr (!COST && STAGES == 1 && !GS) {
    if (hifi && B <= 2 * maxq) {
      // four lanes per aircraft.  At most 16 aircraft per CU: one 16-aircraft workgroup per CU; at most 32: two 16-aircraft
      // groups per workgroup
      if (B <= maxq) hipLaunchKernelGGL((k_rollout_q<1, LQR, SCHED>), dim3((unsigned)((B + 15) / 16)), dim3(quad_block_threads(1)), 0, st, a);
      else hipLaunchKernelGGL((k_rollout_q<2, LQR, SCHED>), dim3((unsigned)((B + 31) / 32)), dim3(512), 0, st, a);
      return hip_check(hipGetLastError(), what);
    }
    // (three groups per workgroup leave 168 registers per lane: the roles spill, 3.96 ms against the 4-wave kernel's 2.13)
    if (hifi && B <= max4w) {
      // latency regime: four wavefronts per 64 aircraft, one workgroup per CU
      hipLaunchKernelGGL((k_rollout_4w<LQR, SCHED>), dim3((unsigned)((B + 63) / 64)), dim3(256), 0, st, a);
      return hip_check(hipGetLastError(), what);
    }
  }
  constexpr bool WIDE = STAGES == 1 || RK4_512;      // 512-lane workgroups; else the RK4 ceiling of 256 lanes
  Geometry g = geometry(B, a.fi, WIDE ? 512 : 256);
#ifdef F16_FAST_DIV
  // throughput regime, default numerics: lookups on the scaled-integer image
  static const int use_i32 = [] { const char *e = getenv("F16_ROLLOUT_I32"); return e ? atoi(e) : 1; }();
  if constexpr (WIDE) if (hifi && use_i32 && g.block == 512) {
    a.tab32 = ctx->d_tab32;
    if constexpr (GS) hipLaunchKernelGGL((k_rollout_i_gs<512, STAGES>), dim3(g.grid), dim3(512), 0, st, a);
    else
    hipLaunchKernelGGL((k_rollout_i<512, LQR, SCHED, COST, STAGES>), dim3(g.grid), dim3(512), 0, st, a);
    return hip_check(hipGetLastError(), what);
  }
#endif
  if (LQR && g.block == 512) g.block = 256;  // (fp64 image + 16 slots of 512 lanes would not fit the 160 KB of a CU)
  by_block(g, [&](auto block) {
    constexpr int BLOCK = decltype(block)::value;
    if constexpr (GS && BLOCK < 512) {
      if (a.fi == 0) hipLaunchKernelGGL((k_rollout_gs<BLOCK, 0, STAGES>), dim3(g.grid), dim3(BLOCK), 0, st, a);
      else hipLaunchKernelGGL((k_rollout_gs<BLOCK, -1, STAGES>), dim3(g.grid), dim3(BLOCK), 0, st, a);
    } else
    if constexpr (!((LQR || !WIDE) && BLOCK == 512)) {    // (never reached, and not instantiated)
      if (a.fi == 0) hipLaunchKernelGGL((k_rollout<BLOCK, 0, LQR, SCHED, COST, STAGES>), dim3(g.grid), dim3(BLOCK), 0, st, a);
      else hipLaunchKernelGGL((k_rollout<BLOCK, -1, LQR, SCHED, COST, STAGES>), dim3(g.grid), dim3(BLOCK), 0, st, a);
    }
  });
  return hip_check(hipGetLastError(), what);
}

// One rollout on the nonlinear plant as its entry point states it.  The five f16_rollout* calls differ in these values and in
// the kernel variant <LQR, SCHED, COST> only; plant_rollout checks them in one order and fills RolloutArgs<SCHED, COST>.
struct PlantRollout {
  const char *missing;                 // the message for a NULL among the pointers the variant needs beyond x and u
  const double *x;                     // [18][ld], stepped in place (`out`); the scored call: x0 [18][ld0], read only
  const double *u;                     // [4][ld]: the constant input; u0 under the LQR law; row 0 of u_seq
  double *out;                         // x again; the scored call: the cost column [ld]
  double *traj;
  int32_t *status;
  long B, ld;
  int nsteps, traj_every;
  double dt, xcg;
  int fi;
  unsigned flags;
  // what an entry point leaves alone is the value of the oldest call, f16_rollout:
  const double *seq = nullptr;         // SCHED: u_seq [nrows][4][ld], under the LQR law dem_seq [nrows][3][ld]
  int hold = 1;                        // SCHED: steps per row
  const double *K = nullptr, *dem = nullptr;      // LQR: the gain and the demands (row 0 of dem_seq)
  double *u_out = nullptr;             // LQR: the last action, may be null
  // COST: lane b is sample b / B0 of aircraft b % B0
  long B0 = 0, ld0 = 0;
  const double *x_ref = nullptr, *u_ref = nullptr;
  double *x_end = nullptr;
  const f16_cost_weights *w = nullptr;
  int method = F16_INT_EULER;          // the step rule: F16_INT_EULER, or (SCHED entry points f16_rollout*_rk) F16_INT_RK4
  // GS: the gain schedule in place of K and of rows 1..3 of u
  const f16_gain_grid *grid = nullptr;
  const double *gtab = nullptr;
  int gs_every = 1;
  int32_t *gs_out = nullptr;
};

template <bool LQR, bool SCHED, bool COST, bool GS = false>
static int plant_rollout(f16_ctx *ctx, const PlantRollout &d, void *stream) {
  if ((SCHED && !d.seq) || (LQR && ((!GS && !d.K) || !d.dem)) || (COST && (!d.x_ref || !d.w || !d.out))) return set_error(F16_EINVAL, d.missing);
  if (int rc = check_rollout(ctx, d.x, d.u, d.traj, d.B, d.ld, d.nsteps, d.traj_every)) return rc;
  if (d.hold < 1) return set_error(F16_EINVAL, "hold must be >= 1");
  if constexpr (COST) {
    if (d.B > 0 && (d.B0 < 1 || d.ld0 < d.B0 || d.B % d.B0 != 0))
      return set_error(F16_EINVAL, "B lanes are K samples of B0 aircraft: B0 >= 1, ld0 >= B0 and B % B0 == 0");
    const double *w = d.w->q;       // q[9], qf[9], r[3], pen: 22 doubles in a row
    static_assert(sizeof(f16_cost_weights) == 22 * sizeof(double), "f16_cost_weights is 22 doubles");
    for (int k = 0; k < 22; ++k)
      if (!(w[k] >= 0.0) || !__builtin_isfinite(w[k])) return set_error(F16_EINVAL, "cost weights must be finite and >= 0");
  }
  if constexpr (GS) {
    if (!d.gtab) return set_error(F16_EINVAL, "tab is NULL");
    if (const char *bad = gain_grid_error(d.grid)) return set_error(F16_EINVAL, bad);
    if (d.gs_every < 1) return set_error(F16_EINVAL, "gs_every must be >= 1");
  }
  if (d.method != F16_INT_EULER && !(SCHED && d.method == F16_INT_RK4))
    return set_error(F16_EINVAL, "method must be F16_INT_EULER (1) or F16_INT_RK4 (4)");
  // nothing to step; the scored call still launches for nsteps = 0: its cost is then the terminal term
  if (d.B == 0 || (!COST && d.nsteps == 0)) return F16_OK;
  auto a = base_args<RolloutArgsGS<SCHED, COST, GS>>(ctx, d.B, d.ld, d.xcg, d.fi, d.flags, d.status);
  a.u = d.u; a.out = d.out; a.traj = d.traj;
  a.nsteps = d.nsteps; a.traj_every = d.traj ? d.traj_every : d.nsteps + 1; a.dt = d.dt;
  a.K = d.K; a.dem = d.dem; a.u_out = d.u_out;
  if constexpr (SCHED) { a.seq = d.seq; a.hold = d.hold; a.nrows = d.nsteps > 0 ? (d.nsteps - 1) / d.hold + 1 : 0; }
  if constexpr (COST) { a.x0 = d.x; a.x_ref = d.x_ref; a.u_ref = d.u_ref; a.x_end = d.x_end; a.B0 = d.B0; a.ld0 = d.ld0; a.w = *d.w; }
  if constexpr (GS) { a.grid = *d.grid; a.gtab = d.gtab; a.gs_every = d.gs_every; a.gs_out = d.gs_out; }
  if constexpr (SCHED) if (d.method == F16_INT_RK4) return rollout_dispatch<LQR, SCHED, COST, 4, GS>(ctx, a, stream);
  return rollout_dispatch<LQR, SCHED, COST, 1, GS>(ctx, a, stream);
}

// The entry points: each states what distinguishes it.
extern "C" int f16_rollout(f16_ctx *ctx, double *x, const double *u, double *traj, int32_t *status, long B, long ld,
                           int nsteps, int traj_every, double dt, double xcg, int fi_flag, unsigned flags,
                           void *stream) {
  PlantRollout d{nullptr, x, u, x, traj, status, B, ld, nsteps, traj_every, dt, xcg, fi_flag, flags};
  return plant_rollout<false, false, false>(ctx, d, stream);
}

extern "C" int f16_rollout_sched(f16_ctx *ctx, double *x, const double *u_seq, double *traj, int32_t *status, long B, long ld,
                                 int nsteps, int hold, int traj_every, double dt, double xcg, int fi_flag, unsigned flags,
                                 void *stream) {
  PlantRollout d{"u_seq is NULL", x, u_seq, x, traj, status, B, ld, nsteps, traj_every, dt, xcg, fi_flag, flags};
  d.seq = u_seq; d.hold = hold;
  return plant_rollout<false, true, false>(ctx, d, stream);
}

extern "C" int f16_rollout_cost(f16_ctx *ctx, const double *x0, long B0, long ld0, const double *u_seq, const double *x_ref,
                                const double *u_ref, const f16_cost_weights *h_w, double *cost, double *x_end, double *traj,
                                int32_t *status, long B, long ld, int nsteps, int hold, int traj_every, double dt, double xcg,
                                int fi_flag, unsigned flags, void *stream) {
  PlantRollout d{"u_seq / x_ref / h_w / cost is NULL", x0, u_seq, cost, traj, status, B, ld, nsteps, traj_every, dt, xcg, fi_flag, flags};
  d.seq = u_seq; d.hold = hold;
  d.B0 = B0; d.ld0 = ld0; d.x_ref = x_ref; d.u_ref = u_ref; d.x_end = x_end; d.w = h_w;
  return plant_rollout<false, true, true>(ctx, d, stream);
}

extern "C" int f16_rollout_lqr(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem, double *traj,
                               double *u_out, int32_t *status, long B, long ld, int nsteps, int traj_every, double dt,
                               double xcg, int fi_flag, unsigned flags, void *stream) {
  PlantRollout d{"K / dem is NULL", x, u0, x, traj, status, B, ld, nsteps, traj_every, dt, xcg, fi_flag, flags};
  d.K = K; d.dem = dem; d.u_out = u_out;
  return plant_rollout<true, false, false>(ctx, d, stream);
}

extern "C" int f16_rollout_lqr_sched(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem_seq,
                                     double *traj, double *u_out, int32_t *status, long B, long ld, int nsteps, int hold,
                                     int traj_every, double dt, double xcg, int fi_flag, unsigned flags, void *stream) {
  PlantRollout d{"K / dem_seq is NULL", x, u0, x, traj, status, B, ld, nsteps, traj_every, dt, xcg, fi_flag, flags};
  d.seq = dem_seq; d.hold = hold; d.K = K; d.dem = dem_seq; d.u_out = u_out;
  return plant_rollout<true, true, false>(ctx, d, stream);
}

// The same three scheduled rollouts with the step rule as an argument (include/f16_hip.h).  F16_INT_EULER forwards to the call above
// it stands for, so it gives that call's bits on that call's kernel; F16_INT_RK4 takes the same checks in the same order.
extern "C" int f16_rollout_rk(f16_ctx *ctx, double *x, const double *u_seq, double *traj, int32_t *status, long B, long ld,
                              int nsteps, int hold, int traj_every, double dt, double xcg, int fi_flag, int method, unsigned flags,
                              void *stream) {
  if (method == F16_INT_EULER) return f16_rollout_sched(ctx, x, u_seq, traj, status, B, ld, nsteps, hold, traj_every, dt, xcg, fi_flag, flags, stream);
  PlantRollout d{"u_seq is NULL", x, u_seq, x, traj, status, B, ld, nsteps, traj_every, dt, xcg, fi_flag, flags};
  d.seq = u_seq; d.hold = hold; d.method = method;
  return plant_rollout<false, true, false>(ctx, d, stream);
}

extern "C" int f16_rollout_lqr_rk(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem_seq, double *traj,
                                  double *u_out, int32_t *status, long B, long ld, int nsteps, int hold, int traj_every, double dt,
                                  double xcg, int fi_flag, int method, unsigned flags, void *stream) {
  if (method == F16_INT_EULER)
    return f16_rollout_lqr_sched(ctx, x, u0, K, dem_seq, traj, u_out, status, B, ld, nsteps, hold, traj_every, dt, xcg, fi_flag, flags, stream);
  PlantRollout d{"K / dem_seq is NULL", x, u0, x, traj, status, B, ld, nsteps, traj_every, dt, xcg, fi_flag, flags};
  d.seq = dem_seq; d.hold = hold; d.K = K; d.dem = dem_seq; d.u_out = u_out; d.method = method;
  return plant_rollout<true, true, false>(ctx, d, stream);
}

extern "C" int f16_rollout_cost_rk(f16_ctx *ctx, const double *x0, long B0, long ld0, const double *u_seq, const double *x_ref,
                                   const double *u_ref, const f16_cost_weights *h_w, double *cost, double *x_end, double *traj,
                                   int32_t *status, long B, long ld, int nsteps, int hold, int traj_every, double dt, double xcg,
                                   int fi_flag, int method, unsigned flags, void *stream) {
  if (method == F16_INT_EULER)
    return f16_rollout_cost(ctx, x0, B0, ld0, u_seq, x_ref, u_ref, h_w, cost, x_end, traj, status, B, ld, nsteps, hold, traj_every, dt, xcg,
                            fi_flag, flags, stream);
  PlantRollout d{"u_seq / x_ref / h_w / cost is NULL", x0, u_seq, cost, traj, status, B, ld, nsteps, traj_every, dt, xcg, fi_flag, flags};
  d.seq = u_seq; d.hold = hold; d.method = method;
  d.B0 = B0; d.ld0 = ld0; d.x_ref = x_ref; d.u_ref = u_ref; d.x_end = x_end; d.w = h_w;
  return plant_rollout<false, true, true>(ctx, d, stream);
}

// The LQR loop under a gain schedule over (h, V) (include/f16_hip.h): f16_rollout_lqr_rk's checks in its order, then the schedule's,
// the method last; both methods run the GS kernels (there is no older call to forward Euler to).
extern "C" int f16_rollout_lqr_gs(f16_ctx *ctx, double *x, const double *u0, const f16_gain_grid *h_grid, const double *tab, int gs_every,
                                  const double *dem_seq, double *traj, double *u_out, int32_t *gs_out, int32_t *status, long B, long ld,
                                  int nsteps, int hold, int traj_every, double dt, double xcg, int fi_flag, int method, unsigned flags,
                                  void *stream) {
  PlantRollout d{"dem_seq is NULL", x, u0, x, traj, status, B, ld, nsteps, traj_every, dt, xcg, fi_flag, flags};
  d.seq = dem_seq; d.hold = hold; d.dem = dem_seq; d.u_out = u_out; d.method = method;
  d.grid = h_grid; d.gtab = tab; d.gs_every = gs_every; d.gs_out = gs_out;
  return plant_rollout<true, true, false, true>(ctx, d, stream);
}

extern "C" int f16_gain_lookup_host(const f16_gain_grid *g, const double *h_tab, double h, double v, double *h_out12) {
  if (const char *bad = gain_grid_error(g)) return set_error(F16_EINVAL, bad);
  if (!h_tab || !h_out12) return set_error(F16_EINVAL, "h_tab / h_out12 is NULL");
  gain_lookup(*g, h_tab, h, v, h_out12);
  return F16_OK;
}

// The closed MPPI loop as one launch (k_rollout_mppi): one workgroup per aircraft, K rounded up to 64, 128 or 256 lanes.
extern "C" int f16_rollout_mppi(f16_ctx *ctx, double *x, double *u, double *u_nom, const double *dem, const double *u_ref,
                                const f16_cost_weights *h_w, const double *h_sigma, double lambda, uint64_t seed, uint32_t period0,
                                double *u_seq, double *cost, double *stats, double *traj, int32_t *status, long B0, long ld0, long K,
                                long ld, int nperiods, int S, int hold, int traj_every, double dt, double xcg, int fi_flag, int method,
                                unsigned flags, void *stream) {
  if (!ctx || !x || !u || !u_nom || !dem || !h_w || !h_sigma || !u_seq || !cost)
    return set_error(F16_EINVAL, "ctx / x / u / u_nom / dem / h_w / h_sigma / u_seq / cost is NULL");
  if (K < 1 || K > 256) return set_error(F16_EINVAL, "K must be in 1..256: one workgroup holds an aircraft's samples");
  if (B0 < 0 || ld0 < B0 || ld / K < B0) return set_error(F16_EINVAL, "bad argument (B0 < 0, ld0 < B0 or ld < K * B0)");
  if (S < 1 || hold < 1 || nperiods < 0 || (long)S * hold > 0x7fffffffL) return set_error(F16_EINVAL, "S and hold must be >= 1, nperiods >= 0");
  if (traj && (traj_every < 1 || hold % traj_every != 0)) return set_error(F16_EINVAL, "hold must be a multiple of traj_every >= 1 when traj is given");
  if (!(lambda > 0.0) || !__builtin_isfinite(lambda)) return set_error(F16_EINVAL, "lambda must be finite and > 0");
  for (int i = 0; i < 3; ++i)
    if (!(h_sigma[i] >= 0.0) || !__builtin_isfinite(h_sigma[i])) return set_error(F16_EINVAL, "sigma must be finite and >= 0");
  for (int k = 0; k < 22; ++k)
    if (!(h_w->q[k] >= 0.0) || !__builtin_isfinite(h_w->q[k])) return set_error(F16_EINVAL, "cost weights must be finite and >= 0");
  if (method != F16_INT_EULER && method != F16_INT_RK4) return set_error(F16_EINVAL, "method must be F16_INT_EULER (1) or F16_INT_RK4 (4)");
  if (B0 == 0 || nperiods == 0) return F16_OK;
  MppiArgs m{};
  m.tab = ctx->d_tab; m.lofi = ctx->d_lofi; m.x = x; m.u = u; m.u_nom = u_nom; m.dem = dem; m.u_ref = u_ref; m.u_seq = u_seq; m.cost = cost;
  m.stats = stats; m.traj = traj; m.status = status; m.B0 = B0; m.ld0 = ld0; m.K = K; m.ld = ld;
  m.nperiods = nperiods; m.S = S; m.hold = hold; m.traj_every = traj ? traj_every : hold + 1;
  m.dt = dt; m.xcg = xcg; m.lambda = lambda; m.sg[0] = h_sigma[0]; m.sg[1] = h_sigma[1]; m.sg[2] = h_sigma[2];
  m.fi = fi_flag; m.flags = flags; m.key0 = (uint32_t)(seed & 0xffffffffu); m.key1 = (uint32_t)(seed >> 32); m.period0 = period0; m.w = *h_w;
  const hipStream_t st = (hipStream_t)stream;
  const int block = K <= 64 ? 64 : (K <= 128 ? 128 : 256);
  if (flags & F16_FLAG_ONE_LANE) {
    const dim3 grid((unsigned)(B0 < 65535 ? B0 : 65535));
    if (method == F16_INT_RK4) hipLaunchKernelGGL((k_rollout_mppi_exact<4>), grid, dim3(block), 0, st, m);
    else hipLaunchKernelGGL((k_rollout_mppi_exact<1>), grid, dim3(block), 0, st, m);
    return hip_check(hipGetLastError(), "f16_rollout_mppi launch");
  }
  const dim3 grid((unsigned)(B0 < 256 ? B0 : 256));      // one workgroup per CU (the table image in LDS); the rest grid-stride
  Geometry g{block, 0};
  by_block(g, [&](auto blk) {
    constexpr int BLOCK = decltype(blk)::value;
    if constexpr (BLOCK <= 256) {
      if (method == F16_INT_RK4) {
        if (fi_flag == 0) hipLaunchKernelGGL((k_rollout_mppi<BLOCK, 0, 4>), grid, dim3(BLOCK), 0, st, m);
        else hipLaunchKernelGGL((k_rollout_mppi<BLOCK, -1, 4>), grid, dim3(BLOCK), 0, st, m);
      } else {
        if (fi_flag == 0) hipLaunchKernelGGL((k_rollout_mppi<BLOCK, 0, 1>), grid, dim3(BLOCK), 0, st, m);
        else hipLaunchKernelGGL((k_rollout_mppi<BLOCK, -1, 1>), grid, dim3(BLOCK), 0, st, m);
      }
    }
  });
  return hip_check(hipGetLastError(), "f16_rollout_mppi launch");
}

extern "C" int f16_rollout_lqr_linear(f16_ctx *ctx, double *x9, const double *Ad, const double *Bd, const double *K, const double *x_ref,
                                      const double *u0, double *traj_x, double *traj_u, long B, long ld, int nsteps, int traj_every,
                                      unsigned track_mask, void *stream) {
  if (int rc = check_common(ctx, x9, Ad, B, ld)) return rc;
  if (!Bd || !K || !x_ref) return set_error(F16_EINVAL, "Bd / K / x_ref is NULL");
  if (nsteps < 0 || ((traj_x || traj_u) && (traj_every < 1 || nsteps % traj_every != 0)))
    return set_error(F16_EINVAL, "nsteps must be >= 0 and a multiple of traj_every >= 1 when a trajectory is given");
  if (B == 0 || nsteps == 0) return F16_OK;
  LinArgsL a{};
  a.x = x9; a.Ad = Ad; a.Bd = Bd; a.K = K; a.xref = x_ref; a.u0 = u0; a.trx = traj_x; a.tru = traj_u;
  a.B = B; a.ld = ld; a.nsteps = nsteps; a.every = (traj_x || traj_u) ? traj_every : nsteps + 1; a.track = track_mask & 0x1FFu;
  hipLaunchKernelGGL(k_rollout_lqr_linear, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  return hip_check(hipGetLastError(), "f16_rollout_lqr_linear launch");
}

extern "C" int f16_xdot_na_batch(f16_ctx *ctx, const double *x_full, const double *x9, const double *u3, double *xdot9,
                                 int32_t *status, long B, long ld, double xcg, int fi_flag, unsigned flags,
                                 void *stream) {
  if (int rc = check_common(ctx, x_full, xdot9, B, ld)) return rc;
  if (!x9 || !u3) return set_error(F16_EINVAL, "x9/u3 is NULL");
  if (B == 0) return F16_OK;
  DynArgs a = base_args<DynArgs>(ctx, B, ld, xcg, fi_flag, flags, status);
  a.x = x_full; a.u = x9; a.u3 = u3; a.out = xdot9;
  const Geometry g = geometry(B, fi_flag);
  by_block(g, [&](auto block) {
    constexpr int BLOCK = decltype(block)::value;
    hipLaunchKernelGGL(k_xdot_na<BLOCK>, dim3(g.grid), dim3(BLOCK), 0, (hipStream_t)stream, a);
  });
  return hip_check(hipGetLastError(), "f16_xdot_na_batch launch");
}

#ifdef F16_EXP_STAMPQ2
extern "C" int f16_debug_qstamps(unsigned long long *h_out) {     // diagnostic build only
  return hip_check(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(f16::g_qstamp), 8 * sizeof(unsigned long long)), "read stamps");
}
#endif
