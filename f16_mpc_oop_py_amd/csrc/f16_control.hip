// f16_control.hip -- batched control chain for gfx950: linearise -> ZOH -> DARE/LQR -> condensed QP -> ADMM.
//
//   k_linearise   env.py:294-342 (forward differences of _calc_xdot_na, eps 1e-5)          f16_linearise_batch
//   k_c2d         scipy.signal.cont2discrete zoh = expm([[A,B],[0,0]] dt) (env.py:50,351)  f16_c2d_batch
//   k_lqr         utils.py:219-245 dlqr (DARE + gain), Q = Cd'Cd, R = I (env.py:353-356)   f16_lqr_batch
//   k_rollout_lqr_relin  test_env.py:625-687: the four above + step, per step, T steps       f16_rollout_lqr_relin
//   k_mpc         utils.py:21-167 setup_OSQP + the OSQP solve of env.py:420-424            f16_mpc_batch
//
// Mapping.  k_linearise: one lane per (aircraft, perturbed column), tables in LDS as in the dynamics kernels.  The rule of the reduced
// model -- the MPC-state map, the column map, and for the per-step loops the whole wave-level linearisation -- is f16_linearise.hpp's,
// one definition for k_linearise, k_rollout_lqr_relin, k_mpc and the re-linearising MPC loop of f16_mpc_wave.hip.
// The other three: ONE WAVEFRONT PER AIRCRAFT (workgroup = 64 lanes); all per-aircraft matrices live in LDS:
// 9x9 blocks row-major, the 3N x 3N KKT inverse as a packed lower triangle (conflict-free row reads, see
// f16_smallmat.hpp).  The 9N x 3N prediction matrix CC of utils.py:171-197 is never formed: CC[i,j] = A^(i-j) B,
// so CC*U and CC'*v are causal (adjoint) convolutions with the N blocks G_k = A^k B, and CC'QQ CC is built by a
// diagonal recursion over the same blocks (DESIGN.md "QP build").
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdio.h>
#include <math.h>
#include <stdarg.h>

#include <mutex>
#include <vector>

#include "../../include/f16_hip.h"
#include "f16_ctx.h"
#include "f16_plant.hpp"
#include "f16_smallmat.hpp"
#include "f16_mpc.hpp"
#include "f16_mpc_model.hpp"
#include "f16_mpc_state.hpp"
#include "f16_osqp_rules.hpp"
#include "f16_linearise.hpp"

namespace f16 {

// ------------------------------------------------------------------------------------ linearise
struct LinArgs {
  const double *tab, *lofi, *x, *u;
  double *Ac, *Bc, *Cc;
  int32_t *status;
  long B, ld;
  double eps, xcg;
  int fi;
  unsigned flags;
};

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_linearise(LinArgs a) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  if (a.fi == 1) stage_tables<BLOCK>(tab, a.tab);
  const long total = a.B * 12;
  for (long e = (long)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (long)gridDim.x * BLOCK) {
    const int c = (int)(e / a.B);          // perturbed column: 0..8 MPC states, 9..11 inputs
    const long b = e - (long)c * a.B;
    double sv[18], svp[18], f0[9], f1[9];
#pragma unroll
    for (int k = 0; k < 18; ++k) sv[k] = a.x[k * a.ld + b];
    // env.py:175-177: the three MPC inputs (u.values[1:4]) overwrite the actuator positions
    sv[13] = a.u[1 * a.ld + b]; sv[14] = a.u[2 * a.ld + b]; sv[15] = a.u[3 * a.ld + b];
    const int idx = lin_na_index(c);       // column -> full-state index (f16_linearise.hpp)
    double base = 0.0, pert = 0.0;
#pragma unroll
    for (int k = 0; k < 18; ++k) {
      svp[k] = sv[k] + (k == idx ? a.eps : 0.0);      // x + dx with dx = eps*e_c (env.py:327-330)
      if (k == idx) { base = sv[k]; pert = svp[k]; }
    }
    int st = 0;
    calc_xdot_na((const double *)tab, a.lofi, svp, f1, a.xcg, a.fi, a.flags, st);
    calc_xdot_na((const double *)tab, a.lofi, sv, f0, a.xcg, a.fi, a.flags, st);   // base point re-evaluated per column
    if (c < 9) {
      // env.py:331 with _get_obs_na: row r of C is (x9[r] + dx[r] - x9[r]) / eps.  Off the diagonal dx[r] = 0: x - x is an exact
      // zero for a finite state and NaN for a NaN or infinite one (the whole row of such a state is NaN in the reference)
#pragma unroll
      for (int r = 0; r < 9; ++r) {
        a.Ac[(r * 9 + c) * a.ld + b] = (f1[r] - f0[r]) / a.eps;
        a.Cc[(r * 9 + c) * a.ld + b] = r == c ? (pert - base) / a.eps : sv[mpc_x_index(r)] - sv[mpc_x_index(r)];
      }
    } else {
#pragma unroll
      for (int r = 0; r < 9; ++r) a.Bc[(r * 3 + (c - 9)) * a.ld + b] = (f1[r] - f0[r]) / a.eps;
    }
    if (a.status && st) atomicOr(&a.status[b], st);
  }
}

// env.py:294-342 with the default _calc_xdot / get_obs (env.py:45): 18-state model, 22 perturbed columns.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_linearise_full(LinArgs a) {
  __shared__ __attribute__((aligned(16))) double tab[TABLE_IMAGE_DOUBLES];
  if (a.fi == 1) stage_tables<BLOCK>(tab, a.tab);
  const long total = a.B * 22;
  for (long e = (long)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (long)gridDim.x * BLOCK) {
    const int c = (int)(e / a.B);          // 0..17 states, 18..21 inputs
    const long b = e - (long)c * a.B;
    double x[18], xp[18], u[4], up[4], f0[18], f1[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) { x[k] = a.x[k * a.ld + b]; xp[k] = x[k] + (k == c ? a.eps : 0.0); }
#pragma unroll
    for (int k = 0; k < 4; ++k) { u[k] = a.u[k * a.ld + b]; up[k] = u[k] + (k == c - 18 ? a.eps : 0.0); }
    int st = 0;
    calc_xdot((const double *)tab, a.lofi, xp, up, f1, a.xcg, a.fi, a.flags, st);
    calc_xdot((const double *)tab, a.lofi, x, u, f0, a.xcg, a.fi, a.flags, st);
    if (c < 18) {
#pragma unroll
      for (int r = 0; r < 18; ++r) a.Ac[(r * 18 + c) * a.ld + b] = (f1[r] - f0[r]) / a.eps;
      // C = d get_obs / dx, observed states [2,3,4,7,8,9,10,11,16,17] (parameters.py:134,160)
      const int OBS[10] = {2, 3, 4, 7, 8, 9, 10, 11, 16, 17};
#pragma unroll
      for (int r = 0; r < 10; ++r) {
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < 18; ++k) if (k == OBS[r]) d = (xp[k] - x[k]) / a.eps;
        a.Cc[(r * 18 + c) * a.ld + b] = d;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 18; ++r) a.Bc[(r * 4 + (c - 18)) * a.ld + b] = (f1[r] - f0[r]) / a.eps;
    }
    if (a.status && st) atomicOr(&a.status[b], st);
  }
}

__device__ __forceinline__ void load_soa(double *dst, const double *src, int n, long ld, long b) {
  for (int e = lane_id(); e < n; e += F16_WAVE) dst[e] = src[e * ld + b];
  __syncthreads();
}
__device__ __forceinline__ void store_soa(double *dst, const double *src, int n, long ld, long b) {
  for (int e = lane_id(); e < n; e += F16_WAVE) dst[e * ld + b] = src[e];
}

// ------------------------------------------------------------------------------------ c2d (ZOH): c2d_wave, f16_mpc_model.hpp
struct C2dArgs { const double *Ac, *Bc; double *Ad, *Bd; long B, ld; double dt; };

template <int NS, int NI>
__global__ __launch_bounds__(64) void k_c2d(C2dArgs a) {
  constexpr int NW = NS + NI;
  __shared__ double smem[2 * (NS * NS + 2) + 2 * (NS * NI + 2) + (NS * NS + 2) + 3 * (NS * NW + 2)];
  Bump al{smem};
  double *A = al.take(NS * NS), *Bm = al.take(NS * NI), *Ad = al.take(NS * NS), *Bd = al.take(NS * NI);
  double *scr = al.take(NS * NS + 2 + 3 * (NS * NW + 2) - 2);
  for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
    load_soa(A, a.Ac, NS * NS, a.ld, b);
    load_soa(Bm, a.Bc, NS * NI, a.ld, b);
    c2d_wave<NS, NI>(A, Bm, a.dt, Ad, Bd, scr);
    store_soa(a.Ad, Ad, NS * NS, a.ld, b);
    store_soa(a.Bd, Bd, NS * NI, a.ld, b);
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ DARE / dlqr: dare_sda_wave, f16_mpc_model.hpp
// K = (B'XB + R)^-1 (B'XA)  (utils.py:244; Rw: null = R is the identity); scr >= 27+27+9+18+3 (+pad)
__device__ void lqr_gain_wave(const double *A, const double *Bm, const double *X, double *K, double *scr, const double *Rw = nullptr) {
  Bump al{scr};
  double *XB = al.take(27), *BXA = al.take(27), *S = al.take(9), *Wx = al.take(18), *f = al.take(3);
  mm<false, false>(XB, X, Bm, 9, 9, 3);        // X B   (9x3)
  mm<true, false>(S, Bm, XB, 3, 9, 3);         // B' X B
  if (Rw) { for (int e = lane_id(); e < 9; e += F16_WAVE) S[e] += Rw[e]; }
  else { for (int e = lane_id(); e < 3; e += F16_WAVE) S[e * 4] += 1.0; }
  __syncthreads();
  mm<true, false>(BXA, XB, A, 3, 9, 9);        // (X B)' A = B' X A   (X symmetric)
  inverse(S, 3, Wx, f);
  mm<false, false>(K, S, BXA, 3, 3, 9);
}

struct LqrArgs { const double *Ad, *Bd, *Cd; double *K, *Pare; int32_t *status; long B, ld; MpcProb pb; };

__global__ __launch_bounds__(64, 3) void k_lqr(LqrArgs a) {
  __shared__ double smem[82 * 5 + 28 * 2 + DARE_SCRATCH + 100];   // DARE scratch also serves lqr_gain_wave
  Bump al{smem};
  double *A = al.take(81), *Bm = al.take(27), *C = al.take(81), *Q = al.take(81), *X = al.take(81), *K = al.take(27);
  double *scr = al.take(DARE_SCRATCH + 90);
  for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
    load_soa(A, a.Ad, 81, a.ld, b);
    load_soa(Bm, a.Bd, 27, a.ld, b);
    load_soa(C, a.Cd, 81, a.ld, b);
    mpc_model_q(Q, C, a, lane_id());                   // Q = C'C (env.py:353) or utils.py:219 `Q`
    const int it = dare_sda_wave(A, Bm, Q, X, scr, a.pb.custom_r ? a.pb.Rinv : nullptr);
    lqr_gain_wave(A, Bm, X, K, scr, a.pb.custom_r ? a.pb.R : nullptr);
    for (int e = lane_id(); e < 27; e += F16_WAVE) a.K[e * a.ld + b] = -K[e];   // K = -dlqr(...) (env.py:356)
    if (a.Pare) store_soa(a.Pare, X, 81, a.ld, b);
    if (a.status && it >= 60 && lane_id() == 0) a.status[b] |= F16_ST_QP_MAXITER;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ per-step re-linearised LQR loop
// test_env.py:625-687 `test_LQR_dynamic_nl` (and env.py's own law re-derived every step) as ONE launch: per step linearise at the
// current (x, u) -> ZOH -> dlqr -> u[1:4] = -K (x9 - x_ref) + u0 -> step.  One wavefront per aircraft for all nsteps, the aircraft
// independent (no hand-off between waves).  Lanes 0..11 evaluate the perturbed columns and lane 12 the base point through the
// out-of-line xdot_na_exact, the chain runs on the same LDS-resident parts k_c2d / k_lqr use (c2d_wave, dare_sda_wave,
// lqr_gain_wave), lane 0 takes the Euler step through euler_step_exact (the F16_FLAG_ONE_LANE step).  The state, the command and
// the gain live in LDS between steps.
struct RelinArgs {
  const double *tab, *lofi, *xref, *u0;      // xref: [ceil(nsteps / hold)][9][ld], step t reads row t / hold
  double *x, *u, *traj, *utraj, *Ktraj;
  int32_t *status;
  long B, ld;
  int nsteps, every;
  int hold;                // steps per row of xref (f16_rollout_lqr_relin_sched; >= nsteps: the one row of f16_rollout_lqr_relin)
  unsigned track;
  double eps, dt, xcg;
  int fi;
  unsigned flags;
  MpcProb pb;              // Q, R (custom_q / custom_r); the bounds are not read
};
constexpr int RELIN_SCRATCH = C2D_SCRATCH > DARE_SCRATCH + 90 ? C2D_SCRATCH : DARE_SCRATCH + 90;

// Two waves per SIMD: the out-of-line plant evaluation alone takes 248 registers, so one wave per SIMD is what the kernel gets without
// a bound (256 VGPRs + 136 AGPRs); with the bound the DARE spills about a hundred registers to scratch.  A/B builds:
// -DF16_RELIN_MIN_WAVES=1 (DESIGN.md "Per-step re-linearised LQR loop" has the measured comparison).
#ifndef F16_RELIN_MIN_WAVES
#define F16_RELIN_MIN_WAVES 2
#endif
__global__ __launch_bounds__(64, F16_RELIN_MIN_WAVES) void k_rollout_lqr_relin(RelinArgs a) {
  __shared__ double smem[18 + 4 + 10 + 4 + 13 * 9 + 1 + 82 + 28 + 82 + 28 + 82 + 82 + 28 + 10 + RELIN_SCRATCH];
  __shared__ int stl;
  Bump al{smem};
  double *xs = al.take(18), *us = al.take(4), *xr = al.take(9), *u0 = al.take(3);
  double *F = al.take(13 * 9), *A = al.take(81), *Bm = al.take(27), *Ad = al.take(81), *Bd = al.take(27), *Q = al.take(81);
  double *X = al.take(81), *K = al.take(27), *cd = al.take(9), *scr = al.take(RELIN_SCRATCH);
  const int l = lane_id();
  for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
    if (l < 18) xs[l] = a.x[l * a.ld + b];
    if (l < 4) us[l] = a.u[l * a.ld + b];
    if (l < 9) xr[l] = ((a.track >> l) & 1u) ? a.xref[l * a.ld + b] : 0.0;
    if (l < 3) u0[l] = a.u0 ? a.u0[l * a.ld + b] : 0.0;
    if (l < 27) K[l] = 0.0;
    if (l == 0) stl = 0;
    __syncthreads();
    int st = a.status ? a.status[b] : 0;
    double *tr = a.traj ? a.traj + b : nullptr, *tu = a.utraj ? a.utraj + b : nullptr, *tk = a.Ktraj ? a.Ktraj + b : nullptr;
    int until = a.every, seg = a.hold;
    const double *xrow = a.xref;
    for (int t = 0; t < a.nsteps; ++t) {
      if (seg == 0) {      // a segment boundary of the schedule (t % hold == 0): the next row of x_ref, in front of the step's first use
        seg = a.hold;
        xrow += 9 * a.ld;
        if (l < 9) xr[l] = ((a.track >> l) & 1u) ? xrow[l * a.ld + b] : 0.0;
        __syncthreads();
      }
      --seg;
      if (!(a.flags & FLAG_NO_ENVELOPE) && outside_envelope(xs)) st |= ST_ENVELOPE;      // env.py:117-124
      if (!(st & ST_ENVELOPE)) {
        // env.py:294-342 (f16_linearise_batch): forward differences at (x, u[1:4]), eps; C = diag((x + eps - x) / eps)
        linearise_na_wave(a.tab, a.lofi, xs, us[1], us[2], us[3], a.eps, a.xcg, a.fi, a.flags, F, A, Bm, cd, l);
        for (int e = l; e < 81; e += F16_WAVE) {
          const int i = e / 9, j = e - i * 9;
          Q[e] = a.pb.custom_q ? a.pb.Q[e] : (i == j ? cd[i] * cd[i] : 0.0);              // Q = C'C (env.py:353), C diagonal
        }
        __syncthreads();
        c2d_wave<9, 3>(A, Bm, a.dt, Ad, Bd, scr);                                         // f16_c2d_batch
        const int it = dare_sda_wave(Ad, Bd, Q, X, scr, a.pb.custom_r ? a.pb.Rinv : nullptr);      // f16_lqr_batch_w
        lqr_gain_wave(Ad, Bd, X, K, scr, a.pb.custom_r ? a.pb.R : nullptr);
        if (it >= 60) st |= F16_ST_QP_MAXITER;
        // u[1:4] = -K (x9 - x_ref) + u0, x_ref = x9 outside the tracked entries (f16_rollout_lqr_linear's rule); thrust held
        if (l < 3) {
          double s = 0.0;
#pragma unroll
          for (int j = 0; j < 9; ++j) {
            const double x9 = xs[mpc_x_index(j)];
            s += K[l * 9 + j] * (x9 - (((a.track >> j) & 1u) ? xr[j] : x9));
          }
          us[1 + l] = -s + u0[l];
        }
        __syncthreads();
        if (l == 0) {
          double x[18], u[4];
#pragma unroll
          for (int k = 0; k < 18; ++k) x[k] = xs[k];
#pragma unroll
          for (int k = 0; k < 4; ++k) u[k] = us[k];
          int ss = 0;
          euler_step_exact(a.tab, a.lofi, x, u, a.dt, a.xcg, a.fi, a.flags, &ss);
#pragma unroll
          for (int k = 0; k < 18; ++k) xs[k] = x[k];
          stl = ss;
        }
        __syncthreads();
        st |= stl;
      }
      if (--until == 0) {
        until = a.every;
        if (tr) { if (l < 18) __builtin_nontemporal_store(xs[l], tr + l * a.ld); tr += 18 * a.ld; }
        if (tu) { if (l < 3) __builtin_nontemporal_store(us[1 + l], tu + l * a.ld); tu += 3 * a.ld; }
        if (tk) { if (l < 27) __builtin_nontemporal_store(-K[l], tk + l * a.ld); tk += 27 * a.ld; }      // K = -dlqr (env.py:356)
      }
    }
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 18; ++k) finite = finite && isfinite(xs[k]);
    if (!finite) st |= ST_NONFINITE;
    if (st & ST_ENVELOPE) st |= envelope_state_bits(xs);
    if (l < 18) a.x[l * a.ld + b] = xs[l];
    if (l < 4) a.u[l * a.ld + b] = us[l];
    if (a.status && l == 0) a.status[b] = st;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ MPC (QP build + ADMM)
// (CC U)[i][r] = sum_{j<=i} sum_c G_{i-j}[r][c] U[3j+c]
__device__ __forceinline__ double conv_forward_row(const double *G, const double *U, int i, int r) {
  double s = 0.0;
  for (int j = 0; j <= i; ++j) {
    const double *g = G + (i - j) * 27 + r * 3;
    s += g[0] * U[3 * j] + g[1] * U[3 * j + 1] + g[2] * U[3 * j + 2];
  }
  return s;
}

#ifdef F16_EXP_STAMPB   // diagnostic build: cycles per phase of the build kernel, aircraft b -> u_seq column b
#define BSTAMP(i) { __builtin_amdgcn_s_waitcnt(0); unsigned long long t1_ = __builtin_amdgcn_s_memtime(); tB[i] += t1_ - tb0; tb0 = t1_; }
#else
#define BSTAMP(i)
#endif
// Per-lane values of the constraint rows a lane owns (rows l, l + 64, ...): registers up to MAXN; beyond (BIG: horizons up
// to BIG_MAXN, the reference's own sweep range env.py:426-436) they live in the per-aircraft global workspace, as does the
// packed KKT inverse -- a slow path that exists so that the horizon limit is not a hard wall.
template <bool BIG_> struct RowVec;
template <> struct RowVec<false> { double v[MAXT]; __device__ __forceinline__ double &operator[](int i) { return v[i]; } };
template <> struct RowVec<true> { double *p; __device__ __forceinline__ double &operator[](int i) { return p[i]; } };

template <bool SETUP_ONLY, bool BIG = false>
__global__ __launch_bounds__(64, SETUP_ONLY ? 2 : 1) void k_mpc(MpcArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int N = a.N, n = 3 * N, np = n * (n + 1) / 2, ms = 6 * N, m = 12 * N;
  const int l = lane_id();
  Bump al{smem};
  // R0 is time-shared: DARE scratch -> (build) pred | Q-weighted error | q -> (generic solver) packed KKT inverse.
  // Build-only launches keep the footprint at 17.8 KB for N = 30 (eight wavefronts per CU): the Q G_k / Qbar G_k blocks
  // of the P recursion are formed just in time (jit, 54 doubles) instead of being stored for all k.
  const int r0 = (SETUP_ONLY || BIG) ? 1100 : max(np, 1100);
  double *const R0 = al.take(r0);
  double *Minv = R0;                  // packed KKT inverse of the generic solver (BIG: in the global workspace, set per aircraft)
  const int TM = BIG ? (m + 63) / 64 : MAXT;     // constraint rows per lane
  double *G = al.take(N * 27);
  double *A = al.take(81), *Q = al.take(81), *Qb = al.take(81);
  double *jit = al.take(54);
  double *Bm = jit;                   // B is dead once G_0 is copied out, long before the P recursion uses jit
  double *x9 = al.take(9), *xref = al.take(9);
  double *qv, *wbuf, *pred;           // q | QQ (x_ref - MM x) | MM x: A^(i+1) x
  double *xs = nullptr, *xt = nullptr, *rhs = nullptr, *tv = nullptr;      // generic solver only
  double *Dg = nullptr, *E9 = nullptr, *Ec = nullptr, *Er = nullptr;       // generic solver: equilibration, then Gram weights
  if (SETUP_ONLY && !BIG) { pred = R0; wbuf = R0 + 9 * N; qv = R0 + 18 * N; }      // 21 N <= 840 < 1100
  else { qv = al.take(n); wbuf = al.take(m); pred = al.take(9 * N); }
  if (!SETUP_ONLY) { xs = al.take(n); xt = al.take(n); rhs = al.take(n); tv = al.take(n);
                     Dg = al.take(n); E9 = al.take(9 * N); Ec = al.take(n); Er = al.take(n + 3); }
  double *scr = R0, *X = R0 + 760;                  // DARE scratch (748 doubles), then X (82)

#ifdef F16_EXP_STAMPB
  unsigned long long tB[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tb0 = __builtin_amdgcn_s_memtime();
#endif
  for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
    // a prepared plan (mode 2) already holds everything that depends on the model only: A, Q, Qbar, G_k, P, A'A;
    // what is left per call is the state-dependent part, pred_i = A^(i+1) x and q
    const bool update_only = SETUP_ONLY && a.mode == 2;
    double *exm = a.ext ? a.ext + (size_t)b * mpc_ext_doubles(N) + mpc_ext_model(N) : nullptr;
    if (update_only) {
      for (int e = l; e < 81; e += F16_WAVE) { A[e] = exm[e]; Q[e] = exm[81 + e]; Qb[e] = exm[162 + e]; }
      const double *Gg = a.ext + (size_t)b * mpc_ext_doubles(N) + n;
      for (int e = l; e < N * 27; e += F16_WAVE) G[e] = Gg[e];
      __syncthreads();
    } else {
    // ---------------- model + weights (utils.py:82-105)
    {   // one global round trip for the three operands (189 strided loads in flight) instead of three
      const double a0 = a.Ad[(size_t)l * a.ld + b], a1 = l + 64 < 81 ? a.Ad[(size_t)(l + 64) * a.ld + b] : 0.0;
      const double c0 = a.Cd[(size_t)l * a.ld + b], c1 = l + 64 < 81 ? a.Cd[(size_t)(l + 64) * a.ld + b] : 0.0;
      const double b0 = l < 27 ? a.Bd[(size_t)l * a.ld + b] : 0.0;
      A[l] = a0; Qb[l] = c0;                           // Cd staged in Qb
      if (l + 64 < 81) { A[l + 64] = a1; Qb[l + 64] = c1; }
      if (l < 27) Bm[l] = b0;
      __syncthreads();
    }
    mpc_model_q(Q, Qb, a, l);                                // Q = C'C (env.py:389) or utils.py:21 `Q`; the model part: f16_mpc_model.hpp
    }
    if (l < 9) {
      const double v = a.x ? a.x[mpc_x_index(l) * a.ld + b] : 0.0;   // (no state when a plan is prepared)
      x9[l] = v;
      xref[l] = a.xref ? a.xref[l * a.ld + b]                                  // utils.py:21 `x_ref` as the caller gives it
                       : ((l >= 5 && l < 8 && a.dem) ? a.dem[(l - 5) * a.ld + b] : v);   // env.py:380-383 (x_ref[5:8] = demands)
    }
    __syncthreads();
    // a state that is not finite leaves no QP to solve (f16_mpc.hpp: mpc_job_nonfinite)
    bool fin_ = l < 9 ? (isfinite(x9[l]) && isfinite(xref[l])) : true;
    if (l < 3 && a.x) fin_ = fin_ && isfinite(a.x[(13 + l) * a.ld + b]);
    const bool nonfinite = __ballot(!fin_) != 0;
    if (a.ext && l == 0) a.ext[(size_t)b * mpc_ext_doubles(N) + mpc_ext_flag(N)] = nonfinite ? 1.0 : 0.0;
    BSTAMP(0)
    if (!update_only) {
    dare_sda_wave(A, Bm, Q, X, scr, a.pb.custom_r ? a.pb.Rinv : nullptr);
    BSTAMP(1)
    mpc_model_keep(A, Q, Qb, X, exm, l);                // Qbar = X, and A | Q | Qbar to the workspace
    // ---------------- prediction blocks G_k = A^k B, pred_i = A^(i+1) x (utils.py:171-197 without forming CC/MM)
    mpc_model_G(A, Bm, G, N, l);
    BSTAMP(2)
    }
    // ---------------- pred_i = A^(i+1) x and q = -2 CC' QQ (x_ref - MM x)   (utils.py:112; f16_mpc_state.hpp: the closed-loop
    // rollout kernel of f16_mpc_wave.hip runs the very same code per step)
    mpc_state_vectors(A, Q, Qb, G, x9, xref, pred, wbuf, qv, N);
    BSTAMP(3)
    BSTAMP(4)
    // ---------------- P = 2 (CC' QQ CC + RR), packed lower, to the workspace (mpc_model_P, f16_mpc_model.hpp)
    double *Pg = a.Ppk + (size_t)b * np;
    if (!update_only) mpc_model_P<(9 * (BIG ? BIG_MAXN : MAXN) + F16_WAVE - 1) / F16_WAVE>(Q, Qb, G, jit, Pg, N, a, l);
    BSTAMP(5)
    // ---------------- bounds of the kept rows (utils.py:129-152): [6N state | 3N command | 3N rate]
    RowVec<BIG> lo, hi, z, y, dy, Eo, eqf;
    if constexpr (BIG) {
      double *rows = a.bigws + (size_t)b * mpc_big_doubles(N);
      Minv = rows + 7 * (size_t)(64 * TM);
      lo.p = rows; hi.p = rows + 64 * TM; z.p = rows + 2 * 64 * TM; y.p = rows + 3 * 64 * TM; dy.p = rows + 4 * 64 * TM;
      Eo.p = rows + 5 * 64 * TM; eqf.p = rows + 6 * 64 * TM;
    }
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      const int row = l + 64 * t, ri = BIG ? row : t;
      lo[ri] = 0.0; hi[ri] = 0.0; z[ri] = 0.0; y[ri] = 0.0; dy[ri] = 0.0;
      if (row < ms) {
        const int i = row / 6, rr = row - 6 * i;
        const double pm = pred[i * 9 + SROW[rr]];
        lo[ri] = a.pb.slb[rr] - pm;
        hi[ri] = a.pb.sub[rr] - pm;
      } else if (row < ms + n) {
        const int c = (row - ms) % 3;
        lo[ri] = a.pb.ulb[c]; hi[ri] = a.pb.uub[c];
      } else if (row < m) {
        const int k = row - ms - n, c = k % 3;
        if (k < 3) {
          const double act = a.x[(13 + c) * a.ld + b];
          lo[ri] = act + a.pb.rlb[c] * a.dt;
          hi[ri] = act + a.pb.rub[c] * a.dt;
        } else {
          lo[ri] = a.pb.rlb[c]; hi[ri] = a.pb.rub[c];              // reference quirk: not multiplied by dt (utils.py:151-152)
        }
      }
    }
    if (a.ext) {   // per-aircraft extras for the register-resident solver / the debug entry point
      double *ex = a.ext + (size_t)b * mpc_ext_doubles(N);
      for (int e = l; e < n; e += F16_WAVE) ex[e] = qv[e];
      if (!update_only) { for (int e = l; e < N * 27; e += F16_WAVE) ex[n + e] = G[e]; }
      for (int e = l; e < 9 * N; e += F16_WAVE) ex[n + N * 27 + e] = pred[e];
    }
    BSTAMP(6)
#ifdef F16_EXP_STAMPB
    if (SETUP_ONLY && a.useq && l == 0) for (int i = 0; i < 7; ++i) { a.useq[i * a.ld + b] = (double)tB[i]; tB[i] = 0; }
#endif
    if (SETUP_ONLY) { __syncthreads(); continue; }
    if (nonfinite) { mpc_write_nonfinite(a.ucmd, a.useq, a.info, a.iters_out, a.status, a.ld, a.N, a.s.rho, b, l, F16_WAVE); __syncthreads(); continue; }
    // ---------------- the solve (the published OSQP algorithm; same coordinates as f16_mpc_solve.hip:
    // x stays unscaled, the linear system is (c P + sigma D^-2 + rho A'WA) x~ = sigma D^-2 x - c q + A' E (rho zb - yb))
    const double sigma = a.s.sigma, alpha = a.s.alpha;
    double cs = 1.0;
    for (int e = l; e < n; e += F16_WAVE) { Dg[e] = 1.0; Ec[e] = 1.0; Er[e] = 1.0; }
    for (int e = l; e < 3; e += F16_WAVE) Er[n + e] = 0.0;
    for (int e = l; e < 9 * N; e += F16_WAVE) E9[e] = 1.0;
    __syncthreads();
    for (int pass = 0; pass < a.s.scaling; ++pass) {     // scaling.c:scale_data on the original entries and the running D, E, c
      for (int e = l; e < n; e += F16_WAVE) {            // column norms of [Pb; Ab]
        const int jb = e / 3, c = e - 3 * jb;
        double mp = 0.0, ma = 0.0;
        for (int i = 0; i < n; ++i) mp = fmax(mp, fabs(Pg[i >= e ? tri(i, e) : tri(e, i)]) * Dg[i]);
        for (int i = jb; i < N; ++i)
          for (int r = 0; r < 9; ++r) ma = fmax(ma, fabs(G[(i - jb) * 27 + r * 3 + c]) * E9[9 * i + r]);
        ma = fmax(fmax(ma, Ec[e]), fmax(Er[e], Er[e + 3]));
        tv[e] = 1.0 / sqrt(osqp_limit_scaling(Dg[e] * fmax(cs * mp, ma)));
      }
      for (int e = l; e < 9 * N; e += F16_WAVE) {        // row norms of the state block
        const int i = e / 9, r = e - 9 * i;
        double m_ = 0.0;
        for (int jb = 0; jb <= i; ++jb)
          for (int c = 0; c < 3; ++c) m_ = fmax(m_, fabs(G[(i - jb) * 27 + r * 3 + c]) * Dg[3 * jb + c]);
        wbuf[e] = 1.0 / sqrt(osqp_limit_scaling(E9[e] * m_));          // (m = 12N >= 9N)
      }
      for (int e = l; e < n; e += F16_WAVE) {
        rhs[e] = 1.0 / sqrt(osqp_limit_scaling(Ec[e] * Dg[e]));
        xt[e] = 1.0 / sqrt(osqp_limit_scaling(Er[e] * fmax(Dg[e], e >= 3 ? Dg[e - 3] : 0.0)));
      }
      __syncthreads();
      for (int e = l; e < n; e += F16_WAVE) { Dg[e] *= tv[e]; Ec[e] *= rhs[e]; Er[e] *= xt[e]; }
      for (int e = l; e < 9 * N; e += F16_WAVE) E9[e] *= wbuf[e];
      __syncthreads();
      double sm = 0.0, qn = 0.0;                          // cost scaling: mean column norm of Pb, ||qb||
      for (int e = l; e < n; e += F16_WAVE) {
        double mp = 0.0;
        for (int i = 0; i < n; ++i) mp = fmax(mp, fabs(Pg[i >= e ? tri(i, e) : tri(e, i)]) * Dg[i]);
        sm += cs * Dg[e] * mp;
        qn = fmax(qn, cs * Dg[e] * fabs(qv[e]));
      }
      sm = wave_sum(sm); qn = wave_max(qn);
      cs *= 1.0 / fmax(osqp_limit_scaling(sm / n), osqp_limit_scaling(qn));
      __syncthreads();
    }
    // per-row E, scaled bounds, rho-vector factor and Gram weight of the kept rows; sigma D^-2 per variable
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      const int row = l + 64 * t, ri = BIG ? row : t;
      Eo[ri] = 1.0; eqf[ri] = 1.0;
      if (row < m) {
        Eo[ri] = row < ms ? E9[9 * (row / 6) + SROW[row % 6]] : (row < ms + n ? Ec[row - ms] : Er[row - ms - n]);
        lo[ri] *= Eo[ri]; hi[ri] *= Eo[ri];
        eqf[ri] = (hi[ri] - lo[ri] < OSQP_RHO_TOL) ? OSQP_RHO_EQ_OVER_RHO_INEQ : 1.0;
      }
    }
    __syncthreads();                                      // E9 / Ec / Er are read; they now become the Gram weights W
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      const int row = l + 64 * t, ri = BIG ? row : t;
      if (row < ms) E9[9 * (row / 6) + SROW[row % 6]] = Eo[ri] * Eo[ri] * eqf[ri];
      else if (row < ms + n) Ec[row - ms] = Eo[ri] * Eo[ri] * eqf[ri];
      else if (row < m) Er[row - ms - n] = Eo[ri] * Eo[ri] * eqf[ri];
    }
    for (int e = l; e < n; e += F16_WAVE) Dg[e] = sigma / (Dg[e] * Dg[e]);     // Dg <- sigma D^-2  (c D of the rho estimate: sqrt back)
    __syncthreads();
    const double cinv = 1.0 / cs;
    auto build_minv = [&](double r) {                     // Minv <- (c P + sigma D^-2 + r A'WA)^-1, packed
      __syncthreads();
      for (int e = l; e < np; e += F16_WAVE) {
        int ia = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
        while (tri(ia + 1, 0) <= e) ++ia;
        while (tri(ia, 0) > e) --ia;
        const int ib = e - tri(ia, 0), ja = ia / 3, ca = ia - 3 * ja, jb = ib / 3, cb = ib - 3 * jb;
        double s = 0.0;
        for (int i = ja; i < N; ++i) {
          const double *ga = G + (i - ja) * 27 + ca, *gb = G + (i - jb) * 27 + cb, *wv = E9 + 9 * i;
#pragma unroll
          for (int rr = 0; rr < 6; ++rr) s += wv[SROW[rr]] * ga[SROW[rr] * 3] * gb[SROW[rr] * 3];
        }
        if (ia == ib) s += Ec[ia] + Er[ia] + Er[ia + 3];
        else if (ia == ib + 3) s -= Er[ia];
        Minv[e] = cs * Pg[e] + r * s + (ia == ib ? Dg[ia] : 0.0);
      }
      __syncthreads();
      return spd_inverse_packed(Minv, n, tv);
    };
    double rho = a.s.rho;
    if (!(rho > 0.0)) {   // the builder's opt-in start value (no equilibration): balance the two terms of P + rho A'A
      double tp = 0.0, ta = 0.0;
      for (int e = l; e < n; e += F16_WAVE) {
        const int jb = e / 3, c = e - 3 * jb;
        double s = Ec[e] + Er[e] + Er[e + 3];
        for (int i = jb; i < N; ++i)
          for (int rr = 0; rr < 6; ++rr) { const double gv = G[(i - jb) * 27 + SROW[rr] * 3 + c]; s += E9[9 * i + SROW[rr]] * gv * gv; }
        tp += Pg[tri(e, e)]; ta += s;
      }
      rho = osqp_rho_start(wave_sum(tp), wave_sum(ta));
    }
    bool ok = build_minv(rho);
    for (int e = l; e < n; e += F16_WAVE) xs[e] = 0.0;
    __syncthreads();
    int it = 0;
    double rp = INFINITY, rd = INFINITY;
    bool converged = false, infeasible = false;
    bool done = !ok || a.s.max_iter <= 0;
    auto adjoint = [&](const double *wv_, int e) {          // (A' w)_e for w in the [6N | 3N | 3N] layout, tv = CCs' w_s
      return tv[e] + wv_[ms + e] + (wv_[ms + n + e] - (e + 3 < n ? wv_[ms + n + e + 3] : 0.0));
    };
    while (!done) {
      ++it;
      // w = E (rho zb - yb) -> t = A' w ; rhs = sigma D^-2 x - c q + t
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        const int row = l + 64 * t, ri = BIG ? row : t;
        if (row < m) wbuf[row] = Eo[ri] * (rho * eqf[ri] * z[ri] - y[ri]);
      }
      __syncthreads();
      conv_adjoint<6>(tv, G, wbuf, N, SROW);
      for (int e = l; e < n; e += F16_WAVE) rhs[e] = Dg[e] * xs[e] - cs * qv[e] + adjoint(wbuf, e);
      __syncthreads();
      symv(xt, Minv, rhs, n);                               // x~
      // zb~ = E A x~ ; relaxation, projection, dual update
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        const int row = l + 64 * t, ri = BIG ? row : t;
        if (row < m) {
          double zt;
          if (row < ms) zt = conv_forward_row(G, xt, row / 6, SROW[row % 6]);
          else if (row < ms + n) zt = xt[row - ms];
          else { const int k = row - ms - n; zt = xt[k] - (k >= 3 ? xt[k - 3] : 0.0); }
          zt *= Eo[ri];
          const double ro = rho * eqf[ri];
          const double zr = alpha * zt + (1 - alpha) * z[ri];
          const double zn = fmin(fmax(zr + y[ri] / ro, lo[ri]), hi[ri]);
          dy[ri] = ro * (zr - zn);
          y[ri] = y[ri] + dy[ri];
          z[ri] = zn;
        }
      }
      for (int e = l; e < n; e += F16_WAVE) xs[e] = alpha * xt[e] + (1 - alpha) * xs[e];
      __syncthreads();
      if (it % a.s.check_every == 0 || it >= a.s.max_iter) {
        // residuals of the UNSCALED problem (OSQP termination test) + the scaled ones for the rho estimate
        double r1 = 0.0, nAx = 0.0, nz = 0.0, r1s = 0.0, nAxs = 0.0, nzs = 0.0;
#pragma unroll
        for (int t = 0; t < TM; ++t) {
          const int row = l + 64 * t, ri = BIG ? row : t;
          if (row < m) {
            double ax;
            if (row < ms) ax = conv_forward_row(G, xs, row / 6, SROW[row % 6]);
            else if (row < ms + n) ax = xs[row - ms];
            else { const int k = row - ms - n; ax = xs[k] - (k >= 3 ? xs[k - 3] : 0.0); }
            const double zu = z[ri] / Eo[ri];
            r1 = fmax(r1, fabs(ax - zu)); nAx = fmax(nAx, fabs(ax)); nz = fmax(nz, fabs(zu));
            r1s = fmax(r1s, fabs(Eo[ri] * ax - z[ri])); nAxs = fmax(nAxs, fabs(Eo[ri] * ax)); nzs = fmax(nzs, fabs(z[ri]));
            wbuf[row] = Eo[ri] * y[ri];
          }
        }
        __syncthreads();
        symv(xt, Pg, xs, n);                                // P x (packed P from the workspace)
        conv_adjoint<6>(tv, G, wbuf, N, SROW);
        double r2 = 0.0, nPx = 0.0, nAty = 0.0, nq = 0.0, r2s = 0.0, nPxs = 0.0, nAtys = 0.0, nqs = 0.0;
        for (int e = l; e < n; e += F16_WAVE) {
          const double aty = cinv * adjoint(wbuf, e), rr_ = xt[e] + qv[e] + aty, cD = cs * sqrt(sigma / Dg[e]);
          r2 = fmax(r2, fabs(rr_)); nPx = fmax(nPx, fabs(xt[e])); nAty = fmax(nAty, fabs(aty)); nq = fmax(nq, fabs(qv[e]));
          r2s = fmax(r2s, cD * fabs(rr_)); nPxs = fmax(nPxs, cD * fabs(xt[e])); nAtys = fmax(nAtys, cD * fabs(aty)); nqs = fmax(nqs, cD * fabs(qv[e]));
        }
        rp = wave_max(r1);
        rd = wave_max(r2);
        const double np_ = fmax(wave_max(nAx), wave_max(nz));
        const double nd_ = fmax(fmax(wave_max(nPx), wave_max(nAty)), wave_max(nq));
        __syncthreads();
        if (osqp_converged(rp, rd, np_, nd_, a.s.eps_abs, a.s.eps_rel)) { done = true; converged = true; }
        else {
          // OSQP primal-infeasibility certificate on dy (auxil.c:is_primal_infeasible)
          double ndy = 0.0, supp = 0.0;
#pragma unroll
          for (int t = 0; t < TM; ++t) {
            const int row = l + 64 * t, ri = BIG ? row : t;
            if (row < m) {
              ndy = fmax(ndy, fabs(Eo[ri] * dy[ri]));
              supp += hi[ri] * fmax(dy[ri], 0.0) + lo[ri] * fmin(dy[ri], 0.0);
              wbuf[row] = Eo[ri] * dy[ri];
            }
          }
          ndy = wave_max(ndy);
          supp = wave_sum(supp);
          __syncthreads();
          if (osqp_infeasibility_candidate(ndy, supp, a.s.eps_prim_inf)) {
            conv_adjoint<6>(tv, G, wbuf, N, SROW);
            double nat = 0.0;
            for (int e = l; e < n; e += F16_WAVE) nat = fmax(nat, fabs(adjoint(wbuf, e)));
            nat = wave_max(nat);
            if (osqp_infeasibility_certified(nat, ndy, a.s.eps_prim_inf)) { done = true; infeasible = true; }
          }
          __syncthreads();
        }
        if (done) {}
        else if (it >= a.s.max_iter) done = true;
        else if (a.s.adaptive_rho && it % a.s.rho_every == 0) {     // auxil.c:compute_rho_estimate (scaled residuals)
          const double nw = osqp_rho_estimate(rho, wave_max(r1s), wave_max(nzs), wave_max(nAxs), wave_max(r2s), wave_max(nqs), wave_max(nAtys),
                                              wave_max(nPxs));
          if (osqp_rho_accepted(nw, rho)) {
            rho = nw;
            if (!build_minv(rho)) done = true;
          }
        }
      }
    }
    // res.x[0:3] (env.py:424); OSQP hands back NaN for a problem it certifies infeasible
    for (int e = l; e < 3; e += F16_WAVE) a.ucmd[e * a.ld + b] = infeasible ? NAN : xs[e];
    if (a.useq) for (int e = l; e < n; e += F16_WAVE) a.useq[e * a.ld + b] = infeasible ? NAN : xs[e];
    if (l == 0) mpc_write_result(a.info, nullptr, a.status, a.ld, b, it, rp, rd, rho, mpc_status_bits(converged, infeasible, ok, a.s.max_iter));
    __syncthreads();
  }
}

static size_t mpc_lds_doubles(int N, bool setup_only, bool big = false) {      // mirrors the Bump allocations at the top of k_mpc
  const int n = 3 * N, np = n * (n + 1) / 2, m = 12 * N;
  auto ev = [](int v) { return (size_t)((v + 1) & ~1); };
  const int r0 = (!setup_only && !big && np > 1100) ? np : 1100;
  const size_t common = ev(r0) + ev(N * 27) + ev(81) * 3 + ev(54) + ev(9) * 2;
  const size_t vecs = ev(n) + ev(m) + ev(9 * N);             // q | weighted error | pred (build-only launches up to MAXN overlay them on r0)
  if (setup_only) return big ? common + vecs : common;
  return common + vecs + 4 * ev(n) + 2 * ev(n) + ev(9 * N) + ev(n + 3);
}

}  // namespace f16

using namespace f16;

// F16_EINVAL with a formatted message (the entry points that share a launcher name themselves in theirs)
__attribute__((format(printf, 1, 2))) static int einval(const char *fmt, ...) {
  char msg[384];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof msg, fmt, ap);
  va_end(ap);
  return set_error(F16_EINVAL, msg);
}

// the launch of `name` as hip_check reports it: "<name> launch"
static int launch_check(const char *name) {
  char msg[64];
  snprintf(msg, sizeof msg, "%s launch", name);
  return hip_check(hipGetLastError(), msg);
}

// One lane per (aircraft, column): up to 64 x 256 lanes workgroups of 64, beyond that at most 256 workgroups of 256 in a grid-stride loop.
static int linearise_launch(const char *name, void (*k64)(LinArgs), void (*k256)(LinArgs), int cols, f16_ctx *ctx, const double *x,
                            const double *u, double *Ac, double *Bc, double *Cc, int32_t *status, long B, long ld, double eps,
                            double xcg, int fi_flag, unsigned flags, void *stream) {
  if (!ctx || !x || !u || !Ac || !Bc || !Cc || B < 0 || ld < B) return einval("bad argument to %s", name);
  if (B == 0) return F16_OK;
  LinArgs a{ctx->d_tab, ctx->d_lofi, x, u, Ac, Bc, Cc, status, B, ld, eps, xcg, fi_flag, flags};
  const long lanes = B * cols;
  if (lanes <= 64L * 256) {
    hipLaunchKernelGGL(k64, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  } else {
    long blocks = (lanes + 255) / 256;
    hipLaunchKernelGGL(k256, dim3((unsigned)(blocks < 256 ? blocks : 256)), dim3(256), 0, (hipStream_t)stream, a);
  }
  return launch_check(name);
}

extern "C" int f16_linearise_batch(f16_ctx *ctx, const double *x, const double *u, double *Ac, double *Bc, double *Cc,
                                   int32_t *status, long B, long ld, double eps, double xcg, int fi_flag, unsigned flags,
                                   void *stream) {
  return linearise_launch("f16_linearise_batch", k_linearise<64>, k_linearise<256>, 12, ctx, x, u, Ac, Bc, Cc, status, B, ld, eps, xcg,
                          fi_flag, flags, stream);
}

extern "C" int f16_linearise_full_batch(f16_ctx *ctx, const double *x, const double *u, double *Ac, double *Bc, double *Cc,
                                        int32_t *status, long B, long ld, double eps, double xcg, int fi_flag, unsigned flags,
                                        void *stream) {
  return linearise_launch("f16_linearise_full_batch", k_linearise_full<64>, k_linearise_full<256>, 22, ctx, x, u, Ac, Bc, Cc, status, B,
                          ld, eps, xcg, fi_flag, flags, stream);
}

static unsigned wave_grid(long B) { return (unsigned)(B < 256L * 32 ? B : 256L * 32); }

static int c2d_launch(const char *name, void (*k)(C2dArgs), f16_ctx *ctx, const double *Ac, const double *Bc, double *Ad, double *Bd,
                      long B, long ld, double dt, void *stream) {
  if (!ctx || !Ac || !Bc || !Ad || !Bd || B < 0 || ld < B) return einval("bad argument to %s", name);
  if (B == 0) return F16_OK;
  C2dArgs a{Ac, Bc, Ad, Bd, B, ld, dt};
  hipLaunchKernelGGL(k, dim3(wave_grid(B)), dim3(64), 0, (hipStream_t)stream, a);
  return launch_check(name);
}

extern "C" int f16_c2d_batch(f16_ctx *ctx, const double *Ac, const double *Bc, double *Ad, double *Bd, long B, long ld,
                             double dt, void *stream) {
  return c2d_launch("f16_c2d_batch", k_c2d<9, 3>, ctx, Ac, Bc, Ad, Bd, B, ld, dt, stream);
}

extern "C" int f16_c2d_full_batch(f16_ctx *ctx, const double *Ac, const double *Bc, double *Ad, double *Bd, long B, long ld,
                                  double dt, void *stream) {
  return c2d_launch("f16_c2d_full_batch", k_c2d<18, 4>, ctx, Ac, Bc, Ad, Bd, B, ld, dt, stream);
}

// Weights and bounds as the caller gives them (utils.py:21, :219) -> the kernels' MpcProb; null = env.py's constants.
// +-INFINITY (or anything beyond OSQP's infinity 1e30) becomes +-1e30, as OSQP itself reads it.  The solvers keep the six state
// rows the reference bounds (alpha, beta, p, q, r, lf2: parameters.py:59-95) and leave phi, theta, lf1 out of the iteration, so
// THAT pattern is fixed: a finite bound on one of the three, or no bound at all on one of the six, is refused (the QP-build
// entry f16_mpc_qp_debug_w takes any pattern).
// Q and R alone (utils.py:219 `dlqr(A, B, Q, R)`): validated and copied into p, which holds env.py's constants on entry.
static int fill_prob_qr(MpcProb *p, const f16_mpc_weights *w) {
  if (!w->q_from_cd) {
    for (int i = 0; i < 9; ++i)
      for (int j = 0; j < 9; ++j) {
        if (!isfinite(w->Q[i * 9 + j]) || fabs(w->Q[i * 9 + j] - w->Q[j * 9 + i]) > 1e-12 * (fabs(w->Q[i * 9 + j]) + fabs(w->Q[j * 9 + i])))
          return set_error(F16_EINVAL, "f16_mpc_weights: Q must be finite and symmetric");
        p->Q[i * 9 + j] = 0.5 * (w->Q[i * 9 + j] + w->Q[j * 9 + i]);
      }
    p->custom_q = 1;
  }
  {
    const double *R = w->R;
    bool ident = true;
    for (int i = 0; i < 9; ++i) {
      if (!isfinite(R[i])) return set_error(F16_EINVAL, "f16_mpc_weights: R must be finite");
      ident = ident && R[i] == ((i % 4 == 0) ? 1.0 : 0.0);
    }
    if (!ident) {
      if (fabs(R[1] - R[3]) + fabs(R[2] - R[6]) + fabs(R[5] - R[7]) > 1e-12 * (fabs(R[0]) + fabs(R[4]) + fabs(R[8])))
        return set_error(F16_EINVAL, "f16_mpc_weights: R must be symmetric");
      const double c00 = R[4] * R[8] - R[5] * R[7], c01 = R[5] * R[6] - R[3] * R[8], c02 = R[3] * R[7] - R[4] * R[6];
      const double det = R[0] * c00 + R[1] * c01 + R[2] * c02;
      if (!(R[0] > 0) || !(R[0] * R[4] - R[1] * R[3] > 0) || !(det > 0)) return set_error(F16_EINVAL, "f16_mpc_weights: R must be positive definite");
      const double inv[9] = {c00, R[2] * R[7] - R[1] * R[8], R[1] * R[5] - R[2] * R[4],
                             c01, R[0] * R[8] - R[2] * R[6], R[2] * R[3] - R[0] * R[5],
                             c02, R[1] * R[6] - R[0] * R[7], R[0] * R[4] - R[1] * R[3]};
      for (int i = 0; i < 9; ++i) { p->R[i] = R[i]; p->Rinv[i] = inv[i] / det; }
      p->custom_r = 1;
    }
  }
  return F16_OK;
}

int f16::mpc_fill_prob(MpcProb *p, const f16_mpc_weights *w) {
  mpc_default_prob(p);
  if (!w) return F16_OK;
  auto inf = [](double v) { return !(fabs(v) < 1e20); };
  auto clip = [](double v) { return v > 1e30 ? 1e30 : (v < -1e30 ? -1e30 : v); };
  if (int rc = fill_prob_qr(p, w)) return rc;
  static const int srow[6] = {2, 3, 4, 5, 6, 8}, free_rows[3] = {0, 1, 7};
  for (int k = 0; k < 3; ++k)
    if (!inf(w->x_lb[free_rows[k]]) || !inf(w->x_ub[free_rows[k]]))
      return set_error(F16_EINVAL, "f16_mpc_weights: phi, theta and lf1 (MPC states 0, 1, 7) carry no bounds in the solvers (use f16_mpc_qp_debug_w for the QP alone)");
  for (int k = 0; k < 6; ++k) {
    const double lo = w->x_lb[srow[k]], hi = w->x_ub[srow[k]];
    if (lo != lo || hi != hi || (inf(lo) && inf(hi)) || lo > hi) return set_error(F16_EINVAL, "f16_mpc_weights: a bounded state row needs lb <= ub and at least one finite bound");
    p->slb[k] = clip(lo); p->sub[k] = clip(hi);
  }
  for (int c = 0; c < 3; ++c) {
    const double v[4] = {w->u_lb[c], w->u_ub[c], w->udot_lb[c], w->udot_ub[c]};
    if (v[0] != v[0] || v[1] != v[1] || v[2] != v[2] || v[3] != v[3] || v[0] > v[1] || v[2] > v[3] || (inf(v[0]) && inf(v[1])) || (inf(v[2]) && inf(v[3])))
      return set_error(F16_EINVAL, "f16_mpc_weights: command and rate rows need lb <= ub and at least one finite bound");
    p->ulb[c] = clip(v[0]); p->uub[c] = clip(v[1]); p->rlb[c] = clip(v[2]); p->rub[c] = clip(v[3]);
  }
  return F16_OK;
}

extern "C" void f16_mpc_default_weights(f16_mpc_weights *w) {
  if (!w) return;
  *w = f16_mpc_weights{};
  w->q_from_cd = 1;
  static const double xlb[9] = {-INFINITY, -INFINITY, -20., -30., -300., -100., -50., -INFINITY, 0.};      // parameters.py:59-95 in MPC-state order
  static const double xub[9] = {INFINITY, INFINITY, 90., 30., 300., 100., 50., INFINITY, 25.};
  static const double ulb[3] = {-25., -21.5, -30.}, uub[3] = {25., 21.5, 30.}, rlb[3] = {-60., -80., -120.}, rub[3] = {60., 80., 120.};
  for (int i = 0; i < 9; ++i) { w->Q[i * 10] = 1.0; w->x_lb[i] = xlb[i]; w->x_ub[i] = xub[i]; }
  for (int i = 0; i < 3; ++i) { w->R[i * 4] = 1.0; w->u_lb[i] = ulb[i]; w->u_ub[i] = uub[i]; w->udot_lb[i] = rlb[i]; w->udot_ub[i] = rub[i]; }
}

extern "C" int f16_lqr_batch_w(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, const f16_mpc_weights *h_w,
                               double *K, double *Pare, int32_t *status, long B, long ld, void *stream) {
  if (!ctx || !Ad || !Bd || !Cd || !K || B < 0 || ld < B) return set_error(F16_EINVAL, "bad argument to f16_lqr_batch");
  if (B == 0) return F16_OK;
  LqrArgs a{Ad, Bd, Cd, K, Pare, status, B, ld, MpcProb{}};
  if (int rc = mpc_fill_prob(&a.pb, h_w)) return rc;
  hipLaunchKernelGGL(k_lqr, dim3(wave_grid(B)), dim3(64), 0, (hipStream_t)stream, a);
  return hip_check(hipGetLastError(), "f16_lqr_batch launch");
}
extern "C" int f16_lqr_batch(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, double *K, double *Pare,
                             int32_t *status, long B, long ld, void *stream) {
  return f16_lqr_batch_w(ctx, Ad, Bd, Cd, nullptr, K, Pare, status, B, ld, stream);
}

static int rollout_lqr_relin_launch(const char *name, f16_ctx *ctx, double *x, double *u, const double *x_ref, const double *u0,
                                    const f16_mpc_weights *h_w, double *traj, double *u_traj, double *K_traj, int32_t *status,
                                    long B, long ld, int nsteps, int hold, int traj_every, unsigned track_mask, double eps, double dt,
                                    double xcg, int fi_flag, unsigned flags, void *stream) {
  if (!ctx || !x || !u || B < 0 || ld < B) return einval("bad argument to %s", name);
  if (nsteps < 1 || traj_every < 1 || nsteps % traj_every != 0)
    return einval("%s: nsteps must be >= 1 and a multiple of traj_every >= 1", name);
  if (hold < 1) return einval("%s: hold must be >= 1", name);
  if (!(eps > 0)) return einval("%s: eps must be > 0", name);
  if ((track_mask & 0x1FFu) && !x_ref) return einval("%s: x_ref is NULL but track_mask selects entries", name);
  RelinArgs a{};
  mpc_default_prob(&a.pb);
  if (h_w)
    if (int rc = fill_prob_qr(&a.pb, h_w)) return rc;
  if (B == 0) return F16_OK;
  a.tab = ctx->d_tab; a.lofi = ctx->d_lofi; a.xref = x_ref; a.u0 = u0;
  a.x = x; a.u = u; a.traj = traj; a.utraj = u_traj; a.Ktraj = K_traj; a.status = status;
  a.B = B; a.ld = ld; a.nsteps = nsteps; a.every = traj_every; a.hold = hold < nsteps ? hold : nsteps; a.track = track_mask & 0x1FFu;
  a.eps = eps; a.dt = dt; a.xcg = xcg; a.fi = fi_flag; a.flags = flags;
  hipLaunchKernelGGL(k_rollout_lqr_relin, dim3(wave_grid(B)), dim3(64), 0, (hipStream_t)stream, a);
  return launch_check(name);
}

extern "C" int f16_rollout_lqr_relin(f16_ctx *ctx, double *x, double *u, const double *x_ref, const double *u0,
                                     const f16_mpc_weights *h_w, double *traj, double *u_traj, double *K_traj, int32_t *status,
                                     long B, long ld, int nsteps, int traj_every, unsigned track_mask, double eps, double dt,
                                     double xcg, int fi_flag, unsigned flags, void *stream) {
  return rollout_lqr_relin_launch("f16_rollout_lqr_relin", ctx, x, u, x_ref, u0, h_w, traj, u_traj, K_traj, status, B, ld, nsteps,
                                  nsteps > 0 ? nsteps : 1, traj_every, track_mask, eps, dt, xcg, fi_flag, flags, stream);      // (one row)
}

// The same loop under a schedule of references: step t reads row t / hold of xref_seq[ceil(nsteps / hold)][9][ld].
extern "C" int f16_rollout_lqr_relin_sched(f16_ctx *ctx, double *x, double *u, const double *xref_seq, const double *u0,
                                           const f16_mpc_weights *h_w, double *traj, double *u_traj, double *K_traj, int32_t *status,
                                           long B, long ld, int nsteps, int hold, int traj_every, unsigned track_mask, double eps,
                                           double dt, double xcg, int fi_flag, unsigned flags, void *stream) {
  return rollout_lqr_relin_launch("f16_rollout_lqr_relin_sched", ctx, x, u, xref_seq, u0, h_w, traj, u_traj, K_traj, status, B, ld,
                                  nsteps, hold, traj_every, track_mask, eps, dt, xcg, fi_flag, flags, stream);
}

extern "C" void f16_qp_default_settings(f16_qp_settings *s) {
  // what env.py:420-422 invokes: osqp.OSQP().setup(..., max_iter=40000, polish=False), every other setting at OSQP's
  // default; the adaptive-rho interval is OSQP's no-timer constant (its default is wall-clock based)
  s->rho = 0.1; s->scaling = 10;
  s->sigma = 1e-6; s->alpha = 1.6; s->eps_abs = 1e-3; s->eps_rel = 1e-3; s->eps_prim_inf = 1e-4;
  s->max_iter = 40000;            // env.py:421
  s->check_every = 25; s->rho_every = 100; s->adaptive_rho = 1;
}

// k_mpc's dynamic LDS exceeds 64 KB for the generic solver at large N: opt in ONCE per device, to the MAXN size (never
// per launch: a concurrent call with a smaller horizon must not shrink the limit under a larger launch, and attribute
// calls are not legal under stream capture).
static int mpc_lds_opt_in() {
  static std::mutex mu;
  static bool ready[64] = {};
  int dev = 0;
  if (int rc = hip_check(hipGetDevice(&dev), "hipGetDevice")) return rc;
  std::lock_guard<std::mutex> lk(mu);
  if (dev < 0 || dev >= 64 || ready[dev]) return F16_OK;
  hipError_t e = hipFuncSetAttribute((const void *)k_mpc<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(mpc_lds_doubles(MAXN, false) * sizeof(double)));
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void *)k_mpc<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(mpc_lds_doubles(MAXN, true) * sizeof(double)));
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void *)k_mpc<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(mpc_lds_doubles(BIG_MAXN, false, true) * sizeof(double)));
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void *)k_mpc<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(mpc_lds_doubles(BIG_MAXN, true, true) * sizeof(double)));
  if (int rc = hip_check(e, "hipFuncSetAttribute(k_mpc)")) return rc;
  ready[dev] = true;
  return F16_OK;
}

// The QP settings of every MPC solve, checked in one place.  need_iterations: prepared plans (max_iter >= 1); the one-shot call and
// the sweep take any max_iter (negative: the generic kernel for |max_iter| iterations; 0: no iteration at all).
static int mpc_check_settings(const f16_qp_settings &s, bool need_iterations, const char *entry) {
  if (s.check_every < 1 || s.rho_every < 1) return einval("%s: check_every and rho_every must be >= 1", entry);
  if (!(s.rho >= 0) || !(s.sigma > 0)) return einval("%s: rho must be >= 0 and sigma > 0", entry);
  if (s.scaling < 0 || s.scaling > 100) return einval("%s: scaling must be 0..100", entry);
  if (s.scaling > 0 && !(s.rho > 0)) return einval("%s: the automatic start value of rho (rho = 0) needs scaling = 0", entry);
  // the rho estimate is formed from the residuals of a termination test, so it can only run on an iteration that has one
  // (osqp.c adapts independently of check_termination; here an interval that is not a multiple would silently become the
  // least common multiple)
  if (s.adaptive_rho && s.rho_every % s.check_every != 0) return einval("%s: with adaptive_rho, rho_every must be a multiple of check_every", entry);
  if (need_iterations && s.max_iter < 1) return einval("%s: max_iter must be >= 1", entry);
  return F16_OK;
}

// Per-call workspace of `entry`, stream-ordered (see f16_ctx.h) -- and therefore refused under stream capture, here and nowhere
// else.  What round 3 established (profiles/r03_capture_pool.log, r03_capture_probe.log): on ROCm 7.2 a plain-HIP graph with mem-alloc / mem-free nodes (tools/micro/capture_pool.hip, none of this library's kernels) replays
// WRONGLY beside eager allocations from the same pool (302,520 wrong elements at replay 11 of 12); the mechanism is not
// established -- the logged eager blocks never overlap the graph's block.  tools/gpu_capture_probe.py replays the one-shot call
// with no host state in the capture (F16_MPC_DISPATCH_ORDER=0): every replay is bit-identical to the eager call EXCEPT the
// ones with an eager call of the same context enqueued behind them (NaN in 20-200 of 256 aircraft), with either solver.
// The fault is the runtime's, not in what the capture bakes in; the refusal stays.  A prepared plan owns its workspace for
// its lifetime and IS capturable (f16_mpc_plan_solve; tests).  escape: F16_MPC_ALLOW_CAPTURE=1 lifts the refusal (the one-shot
// call only; diagnosis only: tools/gpu_capture_probe.py).
static int mpc_work_alloc(f16_ctx *ctx, size_t bytes, void *stream, const char *entry, bool escape, void **block) {
  static const bool allow_capture = [] { const char *e = getenv("F16_MPC_ALLOW_CAPTURE"); return e && e[0] == '1'; }();
  *block = nullptr;
  if (!(escape && allow_capture) && stream_capturing(stream))
    return einval("%s cannot be captured into a HIP graph (per-call workspace; a prepared plan owns its own: f16_mpc_plan_solve)", entry);
  return hip_check(hipMallocFromPoolAsync(block, bytes, ctx->pool, (hipStream_t)stream), "hipMallocFromPoolAsync QP workspace");
}
static int mpc_work_free(void *block, void *stream) {
  return block ? hip_check(hipFreeAsync(block, (hipStream_t)stream), "hipFreeAsync QP workspace") : F16_OK;
}

// Dispatch-order history of one-shot calls, per (stream, batch size); nullptr = none available (run in caller's order).
static f16_ctx::sched_entry *mpc_sched_entry(f16_ctx *ctx, void *stream, long B, int tag = 0) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  for (int i = 0; i < ctx->n_sched; ++i)
    if (ctx->sched[i].stream == stream && ctx->sched[i].B == B && ctx->sched[i].tag == tag) return &ctx->sched[i];
  if (stream_capturing(stream)) return nullptr;
  int32_t *buf = nullptr;
  if (hipMalloc(&buf, 2 * (size_t)B * sizeof(int32_t)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  int slot = ctx->n_sched;
  if (slot >= F16_MAX_SCHED) {
    // all history slots taken (more than F16_MAX_SCHED (stream, batch size) pairs on one context): the oldest one is recycled, round
    // robin -- hipFree waits for whatever still reads its buffer; a caller that cycles through more pairs than slots loses the
    // ordering gain on the evicted ones, never a result
    static int victim = 0;
    slot = victim++ % F16_MAX_SCHED;
    (void)hipFree(ctx->sched[slot].buf);
  } else {
    ctx->n_sched++;
  }
  f16_ctx::sched_entry &e = ctx->sched[slot];
  e.stream = stream; e.B = B; e.buf = buf; e.valid = 0; e.tag = tag;
  return &e;
}

// The solve behind a build: one wavefront per aircraft where that solver applies (k_mpc_fast then only equilibrates, mode 3),
// else the 512-lane workgroup per aircraft.  F16_MPC_WAVE=0 keeps the latter everywhere (A/B runs, cross-checks).
static int mpc_solve_dispatch(f16_ctx *ctx, const MpcArgs &a, void *stream, const double *soft6 = nullptr) {
  if (soft6 && !(a.mode == 0 && mpc_wave_enabled(a)))
    return set_error(F16_EINVAL, "soft state rows run on the one-wavefront solver only (hzn <= 30, scaling > 0, max_iter > 0)");
  if (a.mode == 0 && mpc_wave_enabled(a)) {
    static const bool ruiz_outside = [] { const char *e = getenv("F16_WAVE_RUIZ"); return e && e[0] == '0'; }();
    MpcArgs w = a;
    w.wave_ruiz = ruiz_outside ? 0 : 1;
    if (ruiz_outside) {
      MpcArgs e = a;
      e.mode = 3; e.order = nullptr; e.iters_out = nullptr; e.warm = nullptr;
      if (int rc = mpc_fast_solve_launch(ctx, e, stream)) return rc;
    }
    return mpc_wave_solve_launch(ctx, w, stream, soft6);
  }
  return mpc_fast_solve_launch(ctx, a, stream);
}

// The one launch of k_mpc: the QP build alone (setup_only; a solver follows), or build + generic ADMM, one wavefront per aircraft.
// Needs mpc_lds_opt_in() once per device before it -- by the caller, for a plan at its creation: a solve may be under capture.
static int mpc_build_launch(const MpcArgs &a, bool setup_only, void *stream, const char *what) {
  const bool big = a.N > MAXN;
  const size_t lds = mpc_lds_doubles(a.N, setup_only, big) * sizeof(double);
  if (lds > 160 * 1024) return set_error(F16_EINVAL, "horizon too large for LDS");
  void (*const k)(MpcArgs) = setup_only ? (big ? k_mpc<true, true> : k_mpc<true, false>) : (big ? k_mpc<false, true> : k_mpc<false, false>);
  hipLaunchKernelGGL(k, dim3(wave_grid(a.B)), dim3(64), lds, (hipStream_t)stream, a);
  return hip_check(hipGetLastError(), what);
}

// The solve behind a build, in dispatch order (see k_plan_order): the reference's closed loops call calc_MPC_action once per step on
// states that move little, so the iteration counts of the previous solve of the same batch predict this one's; any order is valid, a
// stale one only loses the gain.  hist: [2][B] the iteration counts of this solve (written here) | the order made of them for the next
// one; null: the caller's order, nothing recorded.  ordered: hist holds the order of a previous solve.  Without one, and with
// first_order (the solvers up to FAST_MAXN), a batch beyond 1024 is ordered by the QPs themselves (mpc_first_order_launch: by ||q||_inf).
static int mpc_ordered_solve(f16_ctx *ctx, MpcArgs a, int32_t *hist, bool ordered, bool first_order, void *stream,
                             const double *soft6 = nullptr) {      // soft6: a plan's soft state rows, or null
  const bool big = a.N > FAST_MAXN;          // the workgroup solver with its operands in HBM: it starts cold
  a.iters_out = hist;
  a.order = hist && ordered ? hist + a.B : nullptr;
  if (hist && !a.order && first_order && a.B > 1024) {
    if (int rc = mpc_first_order_launch(a, hist, hist + a.B, stream)) return rc;
    a.order = hist + a.B;
  }
  if (big) a.warm = nullptr;
  if (big && soft6) return set_error(F16_EINVAL, "soft state rows run on the one-wavefront solver only (hzn <= 30)");
  if (int rc = big ? mpc_big_solve_launch(ctx, a, stream) : mpc_solve_dispatch(ctx, a, stream, soft6)) return rc;
  return hist ? mpc_plan_order_launch(hist, hist + a.B, a.B, a.s.check_every, stream) : F16_OK;
}

// mode 0: generic one-wave kernel (build + ADMM); 1: build only (workspace P, A'A, q|G|pred; *keep receives the block,
// the caller frees it); 2: build, then the register-resident 512-thread solver (N <= 32); 3: build, then the 512-lane workgroup
// solver for long horizons (N > 32, f16_mpc_big.hip).
static int mpc_launch(f16_ctx *ctx, MpcArgs &a, void *stream, int mode, void **keep = nullptr) {
  const int N = a.N;
  if (N < 1 || N > BIG_MAXN || (N > FAST_MAXN && mode == 2)) return set_error(F16_EINVAL, "horizon must be 1..150 (plans: 1..40)");
  if (int rc = mpc_lds_opt_in()) return rc;
  // the wavefront solver (f16_mpc_wave.hip: N <= 30, equilibrated solves) keeps its per-aircraft workspace in the Gram block
  const bool wave_ok = mode == 2 && N <= WAVE_MAXN && a.s.scaling > 0 && a.s.max_iter > 0;
  // (long horizons: the workgroup solver's operands, or beyond MAXN the generic kernel's -- the block holds either)
  const MpcWork w = mpc_work_one_shot(N, mode, a.s.adaptive_rho, wave_ok, mpc_ext_doubles(N), std::max(mpc_big_ws_doubles(N), mpc_big_doubles(N)));
  void *block = nullptr;
  if (int rc = mpc_work_alloc(ctx, w.total() * (size_t)a.B * sizeof(double), stream, "f16_mpc_batch", true, &block)) return rc;
  w.place(a, (double *)block);
  int rc = mpc_build_launch(a, mode != 0, stream, mode ? "f16_mpc_batch setup launch" : "f16_mpc_batch launch");
#ifdef F16_EXP_STAMPB
  mode = 1;
#endif
  if (!rc && mode >= 2) {
    // The history of a one-shot call is per (stream, batch size); N > 32 keeps none.  F16_MPC_DISPATCH_ORDER=0 keeps the caller's
    // order; =first treats every call as a first one (benchmarks: what BASELINE config 4, one call on an unseen batch, costs).
    const char *ev = getenv("F16_MPC_DISPATCH_ORDER");
    f16_ctx::sched_entry *se = mode == 3 || (ev && ev[0] == '0') ? nullptr : mpc_sched_entry(ctx, stream, a.B);
    rc = mpc_ordered_solve(ctx, a, se ? se->buf : nullptr, se && se->valid && !(ev && ev[0] == 'f'), mode == 2, stream);
    if (!rc && se) se->valid = 1;
  }
  if (keep && !rc) { *keep = block; return F16_OK; }
  const int rf = mpc_work_free(block, stream);
  return rc ? rc : rf;
}

extern "C" int f16_mpc_batch(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, const double *x,
                             const double *dem, double *u_cmd, double *u_seq, double *info, int32_t *status, long B,
                             long ld, int hzn, double dt, const f16_qp_settings *s, void *stream) {
  return f16_mpc_batch_w(ctx, Ad, Bd, Cd, x, dem, nullptr, nullptr, u_cmd, u_seq, info, status, B, ld, hzn, dt, s, stream);
}

extern "C" int f16_mpc_batch_w(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, const double *x,
                               const double *dem, const double *x_ref, const f16_mpc_weights *h_w, double *u_cmd, double *u_seq,
                               double *info, int32_t *status, long B, long ld, int hzn, double dt, const f16_qp_settings *s,
                               void *stream) {
  if (!ctx || !Ad || !Bd || !Cd || !x || (!dem && !x_ref) || !u_cmd || B < 0 || ld < B) return set_error(F16_EINVAL, "bad argument to f16_mpc_batch");
  if (B == 0) return F16_OK;
  MpcArgs a{};
  a.Ad = Ad; a.Bd = Bd; a.Cd = Cd; a.x = x; a.dem = dem; a.xref = x_ref; a.ucmd = u_cmd; a.useq = u_seq; a.info = info; a.status = status;
  a.B = B; a.ld = ld; a.N = hzn; a.dt = dt;
  if (int rc = mpc_fill_prob(&a.pb, h_w)) return rc;
  if (s) a.s = *s; else f16_qp_default_settings(&a.s);
  if (int rc = mpc_check_settings(a.s, false, "f16_mpc_batch")) return rc;
  // solver selection: N <= 32 the register-resident / one-wavefront solvers, longer horizons the workgroup solver with its
  // operands in HBM; a negative max_iter forces the generic one-wave kernel (tests: the cross-check of every other solver)
  const bool generic = a.s.max_iter < 0;
  if (a.s.max_iter < 0) a.s.max_iter = -a.s.max_iter;
  return mpc_launch(ctx, a, stream, generic ? 0 : (hzn > FAST_MAXN ? 3 : 2));
}

// The reference's horizon sweep (env.py:426-436: calc_MPC_action(0, 0, 0, N) of the SAME states for N = 1..150) as a
// throughput call.  Horizons up to FAST_MAXN go through the one-shot path one after the other (milliseconds each); the long
// ones are built per horizon and then solved by ONE launch of the workgroup solver over every (horizon, aircraft) pair: the
// iteration counts of this family grow with N and spread widely (N = 150: mean 2,100, max 26,850), so a launch per horizon
// lasts as long as its slowest aircraft on B of the 256 CUs, while the pairs of all horizons together keep every CU busy.
// Outputs: u_cmd [hi - lo + 1][3][ld], info [..][4][ld] (may be null), status [..][ld] (may be null; OR-ed into).
extern "C" int f16_mpc_hzn_sweep(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, const double *x,
                                 const double *dem, double *u_cmd, double *info, int32_t *status, long B, long ld, int hzn_lo,
                                 int hzn_hi, double dt, const f16_qp_settings *s, void *stream) {
  if (!ctx || !Ad || !Bd || !Cd || !x || !dem || !u_cmd || B < 0 || ld < B || hzn_lo < 1 || hzn_hi < hzn_lo || hzn_hi > BIG_MAXN)
    return set_error(F16_EINVAL, "bad argument to f16_mpc_hzn_sweep (horizons 1..150)");
  if (B == 0) return F16_OK;
  f16_qp_settings st;
  if (s) st = *s; else f16_qp_default_settings(&st);
  if (int rc = mpc_check_settings(st, false, "f16_mpc_hzn_sweep")) return rc;
  int N = hzn_lo;
  for (; N <= hzn_hi && (N <= FAST_MAXN || st.max_iter < 0); ++N) {
    const size_t k = (size_t)(N - hzn_lo);
    if (int rc = f16_mpc_batch(ctx, Ad, Bd, Cd, x, dem, u_cmd + k * 3 * ld, nullptr, info ? info + k * 4 * ld : nullptr,
                               status ? status + k * ld : nullptr, B, ld, N, dt, &st, stream)) return rc;
  }
  if (N > hzn_hi) return F16_OK;
  MpcArgs a{};
  mpc_default_prob(&a.pb);
  a.Ad = Ad; a.Bd = Bd; a.Cd = Cd; a.x = x; a.dem = dem; a.B = B; a.ld = ld; a.dt = dt; a.s = st;
  if (int rc = mpc_lds_opt_in()) return rc;
  // groups of horizons, longest first, each within the workspace budget (N = 150: 4.45 MB per aircraft = mpc_big_sweep_job_doubles(150) x 8)
  static const size_t budget = [] { const char *e = getenv("F16_SWEEP_WS_GB"); const double g = e ? atof(e) : 0; return (size_t)((g > 0 ? g : 32.0) * (1ull << 30)); }();
  int hi = hzn_hi;
  while (hi >= N) {
    int lo = hi;
    size_t doubles = mpc_big_sweep_job_doubles(hi);
    while (lo - 1 >= N && (doubles + mpc_big_sweep_job_doubles(lo - 1)) * (size_t)B * sizeof(double) <= budget) doubles += mpc_big_sweep_job_doubles(--lo);
    void *block = nullptr;
    const size_t wbytes = doubles * (size_t)B * sizeof(double);
    if (int rc = mpc_work_alloc(ctx, wbytes + 256, stream, "f16_mpc_hzn_sweep", false, &block)) return rc;
    unsigned int *next = (unsigned int *)((char *)block + wbytes);      // work-queue counter of the solve launch
    int rc = hip_check(hipMemsetAsync(next, 0, 256, (hipStream_t)stream), "hipMemsetAsync sweep queue");
    size_t off = 0;
    for (int Nn = hi; Nn >= lo && !rc; --Nn) {           // the builds (one wavefront per aircraft each)
      MpcArgs b = a;
      const size_t k = (size_t)(Nn - hzn_lo);
      b.N = Nn;
      mpc_work_sweep(Nn, mpc_ext_doubles(Nn), mpc_big_ws_doubles(Nn)).place(b, (double *)block + off * (size_t)B);
      b.ucmd = u_cmd + k * 3 * ld;
      b.status = status ? status + k * ld : nullptr;
      rc = mpc_build_launch(b, true, stream, "f16_mpc_hzn_sweep build launch");
      off += mpc_big_sweep_job_doubles(Nn);
    }
    // Queue order: the pairs of a previous sweep of the same horizons on this stream, costliest first (iterations x N^2) -- a
    // sweep on states that moved little then ends with its packed phase instead of waiting for a straggler taken late (the
    // first call: longest horizons first, 2.25 s at B = 64; repeated: 1.6 s; bench.py hzn_sweep).  Scheduling only.
    const long npairs = (long)(hi - lo + 1) * B;
    const char *ev = getenv("F16_MPC_DISPATCH_ORDER");
    const bool one_group = lo == N && hi == hzn_hi;        // (a sweep cut into many groups must not use up the context's few history slots)
    f16_ctx::sched_entry *se = (ev && ev[0] == '0') || npairs > 0x3fffffffL || !one_group ? nullptr
                                                                                          : mpc_sched_entry(ctx, stream, npairs, (lo << 16) | hi);
    if (!rc) rc = mpc_big_sweep_launch(ctx, a, lo, hi, (double *)block, u_cmd + (size_t)(lo - hzn_lo) * 3 * ld,
                                       info ? info + (size_t)(lo - hzn_lo) * 4 * ld : nullptr,
                                       status ? status + (size_t)(lo - hzn_lo) * ld : nullptr, next, se ? se->buf : nullptr,
                                       se && se->valid ? se->buf + npairs : nullptr, stream);
    if (!rc && se) {
      rc = mpc_big_sweep_order_launch(se->buf, se->buf + npairs, npairs, B, hi, stream);
      if (!rc) se->valid = 1;
    }
    const int rf = mpc_work_free(block, stream);
    if (rc || rf) return rc ? rc : rf;
    hi = lo - 1;
  }
  return F16_OK;
}

// ---- prepared plans: everything of calc_MPC_action that depends on the model only (the reference freezes the model at
// construction, env.py:49-60, but rebuilds the whole QP on every call) is computed once; a solve then costs the
// state-dependent vectors + the ADMM iterations.
struct f16_mpc_plan {
  f16_ctx *ctx;
  long B, ld;
  int N;
  double dt;
  f16_qp_settings s;
  double *buf;
  double *warm;        // x, z, y of the previous solve (allocated when warm start is switched on)
  bool warm_on, have_prev;
  int32_t *sched;      // [2][B]: iteration counts of the last solve | dispatch order of the next (longest first)
  bool have_order;
  void *last_stream;   // the stream of the creation / the last solve: what f16_mpc_plan_destroy waits for
  void *roll_sync;     // f16_rollout_mpc: ticket counter + per-aircraft progress counters (allocated by its first call)
  double *relin_w;     // f16_rollout_mpc_relin: Q[81] | R[9] | Rinv[9] of the plan's weights on the device (allocated by its first call)
  bool relin_model;    // the model blocks were overwritten by f16_rollout_mpc_relin: no frozen-model call may read them any more
  bool soft_on;        // f16_mpc_plan_soft_rows: some kept state row is a soft row ...
  double soft6[6];     // ... with these penalty weights (SROW order: alpha, beta, p, q, r, lf2; 0: the row stays hard)
  MpcArgs a;
};

extern "C" int f16_mpc_plan_create(f16_ctx *ctx, f16_mpc_plan **plan, const double *Ad, const double *Bd, const double *Cd,
                                   long B, long ld, int hzn, double dt, const f16_qp_settings *s, void *stream) {
  return f16_mpc_plan_create_w(ctx, plan, Ad, Bd, Cd, nullptr, B, ld, hzn, dt, s, stream);
}

extern "C" int f16_mpc_plan_create_w(f16_ctx *ctx, f16_mpc_plan **plan, const double *Ad, const double *Bd, const double *Cd,
                                     const f16_mpc_weights *h_w, long B, long ld, int hzn, double dt, const f16_qp_settings *s,
                                     void *stream) {
  if (!ctx || !plan || !Ad || !Bd || !Cd || B < 1 || ld < B) return set_error(F16_EINVAL, "bad argument to f16_mpc_plan_create");
  MpcProb pb;
  if (int rc = mpc_fill_prob(&pb, h_w)) return rc;
  if (hzn < 1 || hzn > MAXN) return set_error(F16_EINVAL, "prepared plans need 1 <= hzn <= 40");
  f16_qp_settings st;
  if (s) st = *s; else f16_qp_default_settings(&st);
  if (int rc = mpc_check_settings(st, true, "f16_mpc_plan_create")) return rc;      // (before anything is allocated)
  const bool wide = hzn > FAST_MAXN;                   // horizons 33..40: the model part is kept, every solve runs the workgroup solver
  if (int rc = mpc_lds_opt_in()) return rc;            // the LDS opt-ins now: the first solve of the plan may already be under capture
  if (int rc = wide ? mpc_big_opt_in() : F16_OK) return rc;
  f16_mpc_plan *p = new f16_mpc_plan();
  p->ctx = ctx; p->B = B; p->ld = ld; p->N = hzn; p->dt = dt;
  p->warm = nullptr; p->warm_on = false; p->have_prev = false; p->sched = nullptr; p->have_order = false; p->last_stream = stream;
  p->roll_sync = nullptr; p->relin_w = nullptr; p->relin_model = false;
  p->soft_on = false;
  for (double &w : p->soft6) w = 0.0;
  p->s = st;
  const MpcWork w = mpc_work_plan(hzn, mpc_ext_doubles(hzn), mpc_big_ws_doubles(hzn));
  if (int rc = hip_check(hipMalloc(&p->buf, w.total() * (size_t)B * sizeof(double)), "hipMalloc MPC plan")) { delete p; return rc; }
  if (int rc = hip_check(hipMalloc(&p->sched, 2 * (size_t)B * sizeof(int32_t)), "hipMalloc MPC plan")) { (void)hipFree(p->buf); delete p; return rc; }
  MpcArgs &a = p->a;
  a = MpcArgs{};
  a.pb = pb;
  a.Ad = Ad; a.Bd = Bd; a.Cd = Cd; a.B = B; a.ld = ld; a.N = hzn; a.dt = dt; a.s = p->s;
  w.place(a, p->buf);
  a.mode = 1;
  int rc = mpc_build_launch(a, true, stream, "f16_mpc_plan build launch");
  // Without equilibration the start value of rho and the KKT factorisation depend on the model only and are cached too.
  // OSQP's equilibration depends on q (the cost scaling c looks at ||q||, and D, E at c), i.e. on the state of the call:
  // a plan with scaling > 0 keeps the model part (DARE, G_k, P) and redoes equilibration + factorisation per solve.
  if (!rc && p->s.scaling == 0 && !wide) rc = mpc_fast_solve_launch(ctx, a, stream);
  a.Ad = a.Bd = a.Cd = nullptr;                        // not retained
  if (rc) { (void)hipFree(p->buf); (void)hipFree(p->sched); delete p; return rc; }
  *plan = p;
  return F16_OK;
}

extern "C" int f16_mpc_plan_solve(f16_mpc_plan *p, const double *x, const double *dem, double *u_cmd, double *u_seq,
                                  double *info, int32_t *status, void *stream) {
  return f16_mpc_plan_solve_w(p, x, dem, nullptr, u_cmd, u_seq, info, status, stream);
}

extern "C" int f16_mpc_plan_solve_w(f16_mpc_plan *p, const double *x, const double *dem, const double *x_ref, double *u_cmd,
                                    double *u_seq, double *info, int32_t *status, void *stream) {
  if (!p || !x || (!dem && !x_ref) || !u_cmd) return set_error(F16_EINVAL, "bad argument to f16_mpc_plan_solve");
  if (p->relin_model) return set_error(F16_EINVAL, "f16_mpc_plan_solve: f16_rollout_mpc_relin overwrote this plan's model; create a new plan for the frozen model");
  MpcArgs a = p->a;
  a.x = x; a.dem = dem; a.xref = x_ref; a.ucmd = u_cmd; a.useq = u_seq; a.info = info; a.status = status;
  p->last_stream = stream;
  a.mode = 2;
  a.warm = p->warm_on ? p->warm : nullptr;
  a.warm_load = p->warm_on && p->have_prev;
  if (int rc = mpc_build_launch(a, true, stream, "f16_mpc_plan build launch")) return rc;
  if (p->s.scaling > 0 || p->N > FAST_MAXN) a.mode = 0;   // nothing cached beyond the model part: full solver prologue
  // the history is the plan's own; a first solve is ordered by the QPs just built (F16_MPC_DISPATCH_ORDER steers one-shot calls only)
  if (int rc = mpc_ordered_solve(p->ctx, a, p->sched, p->have_order, p->N <= FAST_MAXN, stream, p->soft_on ? p->soft6 : nullptr)) return rc;
  p->have_order = true;
  p->have_prev = p->warm_on;
  return F16_OK;
}

// One closed MPC loop as its entry point states it.  The six f16_rollout_mpc* calls are one launch (k_rollout_mpc, f16_mpc_wave.hip)
// and differ in these values only; rollout_mpc_loop checks them in one order and fills RolloutMpcCall.
constexpr int MPC_LOOP_NEVER = 0x7fffffff;      // traj_every of a loop without traj (pair_finish decides and indexes the traj stores
                                                // with it, nothing else), and dem_hold of a constant demand: row 0 for every control step
struct MpcLoop {
  const char *name;                    // the entry point, for its messages
  double *x, *u;
  const double *dem;                   // [ceil(nctrl / dem_hold)][3][ld]
  double *traj, *cmd_traj;
  int32_t *iters_traj, *status;
  int nctrl, traj_every;               // control steps; the sampling interval of traj in PLANT steps
  double xcg;
  int fi;
  unsigned flags;
  // what an entry point leaves alone is the value of the oldest call, f16_rollout_mpc:
  bool allow_zero = false;             // nctrl = 0 is a no-op behind the checks (f16_rollout_mpc / _relin; the others: F16_EINVAL)
  int hold = 1;                        // plant steps per control step
  double dt = 0.0;                     // the plant's Euler step: hold x dt = the plan's dt
  int dem_hold = MPC_LOOP_NEVER;       // control steps per demand row
  bool relin = false;                  // the model re-derived at every control step (k_rollout_mpc<true>): takes and marks a foreign plan
  double eps = 0.0;                    // relin: the linearisation step
  double *model_traj = nullptr;        // relin: [nctrl / model_every][189][ld] or null
  int model_every = 1;                 // relin: in control steps
  bool models_with_traj = false;       // f16_rollout_mpc_relin: the models are sampled with the states -- model_every IS traj_every
};

static int rollout_mpc_loop(f16_mpc_plan *p, const MpcLoop &d, void *stream) {
  if (!p || !d.x || !d.u || !d.dem) return einval("bad argument to %s", d.name);
  if (d.dem_hold < 1) return einval("%s: dem_hold must be >= 1", d.name);
  if (!d.relin && p->relin_model)
    return einval("%s: a re-linearised loop overwrote this plan's model; create a new plan for the frozen model", d.name);
  if (p->N > WAVE_MAXN || p->s.scaling <= 0)
    return einval("%s needs a plan with hzn <= 30 and equilibrated solves (scaling > 0); other plans run the host loop "
                  "(a solve + f16_rollout per control step)", d.name);
  const long long nplant = (long long)d.nctrl * d.hold;
  if (d.nctrl < (d.allow_zero ? 0 : 1) || d.hold < 1 || nplant > 0x7fffffffLL)
    return einval("%s: the control steps must be >= %d, hold >= 1 and their product < 2^31", d.name, d.allow_zero ? 0 : 1);
  if (!(fabs((double)d.hold * d.dt - p->dt) <= 1e-12 * p->dt))
    return einval("%s: hold x dt (%d x %.17g) is not the plan's dt (%.17g) -- the plan's model and rate rows are discretised at the "
                  "control period", d.name, d.hold, d.dt, p->dt);
  const bool sampled = d.traj || (d.models_with_traj && d.model_traj);
  if (sampled && (d.traj_every < 1 || nplant % d.traj_every != 0))
    return einval("%s: the plant steps (nctrl x hold) must be a multiple of traj_every >= 1 when %s is given", d.name,
                  d.models_with_traj ? "traj or model_traj" : "traj");
  const int model_every = !d.models_with_traj ? d.model_every : sampled ? d.traj_every : 1;
  if (d.relin) {
    if (!(d.eps > 0)) return einval("%s: the linearisation step eps must be > 0", d.name);
    if (model_every < 1 || (d.model_traj && d.nctrl % model_every != 0))
      return einval("%s: model_every must be >= 1, and divide nctrl when model_traj is given", d.name);
  }
  if (d.nctrl == 0) return F16_OK;      // (allow_zero: nothing allocated, the plan not marked)
  // the counters (and, re-linearised, the device copy of the weights) of the plan's first call
  if (!p->roll_sync) {
    if (int rc = hip_check(hipMalloc(&p->roll_sync, 8 + (size_t)p->B * sizeof(int32_t)), "hipMalloc f16_rollout_mpc counters")) return rc;
  }
  if (d.relin && !p->relin_w) {
    if (int rc = hip_check(hipMalloc(&p->relin_w, 99 * sizeof(double)), "hipMalloc f16_rollout_mpc_relin weights")) return rc;
    double h[99];
    for (int i = 0; i < 81; ++i) h[i] = p->a.pb.Q[i];
    for (int i = 0; i < 9; ++i) { h[81 + i] = p->a.pb.R[i]; h[90 + i] = p->a.pb.Rinv[i]; }
    if (int rc = hip_check(hipMemcpy(p->relin_w, h, sizeof(h), hipMemcpyHostToDevice), "f16_rollout_mpc_relin weights")) return rc;
  }
  p->last_stream = stream;
  if (d.relin) p->relin_model = true;
  RolloutMpcCall c{};
  c.x = d.x; c.u = d.u; c.dem = d.dem; c.traj = d.traj; c.cmd_traj = d.cmd_traj; c.iters_traj = d.iters_traj; c.status = d.status;
  c.sync = p->roll_sync; c.T = d.nctrl; c.every = d.traj ? d.traj_every : MPC_LOOP_NEVER; c.hold = d.hold; c.dem_hold = d.dem_hold;
  c.dt = d.dt; c.xcg = d.xcg; c.fi = d.fi; c.flags = d.flags;
  c.relin = d.relin; c.eps = d.eps; c.model_traj = d.model_traj; c.model_every = model_every; c.wq = p->relin_w;
  c.warm = p->warm_on ? p->warm : nullptr;
  c.warm_load = p->warm_on && p->have_prev;
  c.soft6 = p->soft_on ? p->soft6 : nullptr;
  const int rc = mpc_wave_rollout_launch(p->ctx, p->a, c, stream);
  if (!rc) p->have_prev = p->warm_on;
  return rc;
}

// The entry points: each states what distinguishes it.  f16_rollout_mpc / _relin: the control period IS the plant step (hold = 1 at
// the plan's own dt); _hold: `hold` plant steps of dt per control step (pair_finish, f16_mpc_wave.hip); _sched: control step c reads
// row c / dem_hold of dem_seq[ceil(nctrl / dem_hold)][3][ld] (the ticket loop of k_rollout_mpc picks the row); _relin*: the model
// re-derived at every control step, the weights the in-kernel QP build reads from memory, the model record.
extern "C" int f16_rollout_mpc(f16_mpc_plan *p, double *x, double *u, const double *dem, double *traj, double *cmd_traj,
                               int32_t *iters_traj, int32_t *status, int nsteps, int traj_every, double xcg, int fi_flag,
                               unsigned flags, void *stream) {
  MpcLoop d{"f16_rollout_mpc", x, u, dem, traj, cmd_traj, iters_traj, status, nsteps, traj_every, xcg, fi_flag, flags};
  d.allow_zero = true; d.dt = p ? p->dt : 0.0;
  return rollout_mpc_loop(p, d, stream);
}

extern "C" int f16_rollout_mpc_relin(f16_mpc_plan *p, double *x, double *u, const double *dem, double *traj, double *cmd_traj,
                                     int32_t *iters_traj, double *model_traj, int32_t *status, int nsteps, int traj_every, double eps,
                                     double xcg, int fi_flag, unsigned flags, void *stream) {
  MpcLoop d{"f16_rollout_mpc_relin", x, u, dem, traj, cmd_traj, iters_traj, status, nsteps, traj_every, xcg, fi_flag, flags};
  d.allow_zero = true; d.dt = p ? p->dt : 0.0;
  d.relin = true; d.eps = eps; d.model_traj = model_traj; d.models_with_traj = true;
  return rollout_mpc_loop(p, d, stream);
}

extern "C" int f16_rollout_mpc_hold(f16_mpc_plan *p, double *x, double *u, const double *dem, double *traj, double *cmd_traj,
                                    int32_t *iters_traj, int32_t *status, int nctrl, int hold, int traj_every, double dt,
                                    double xcg, int fi_flag, unsigned flags, void *stream) {
  MpcLoop d{"f16_rollout_mpc_hold", x, u, dem, traj, cmd_traj, iters_traj, status, nctrl, traj_every, xcg, fi_flag, flags};
  d.hold = hold; d.dt = dt;
  return rollout_mpc_loop(p, d, stream);
}

extern "C" int f16_rollout_mpc_relin_hold(f16_mpc_plan *p, double *x, double *u, const double *dem, double *traj, double *cmd_traj,
                                          int32_t *iters_traj, double *model_traj, int32_t *status, int nctrl, int hold,
                                          int traj_every, int model_every, double dt, double eps, double xcg, int fi_flag,
                                          unsigned flags, void *stream) {
  MpcLoop d{"f16_rollout_mpc_relin_hold", x, u, dem, traj, cmd_traj, iters_traj, status, nctrl, traj_every, xcg, fi_flag, flags};
  d.hold = hold; d.dt = dt;
  d.relin = true; d.eps = eps; d.model_traj = model_traj; d.model_every = model_every;
  return rollout_mpc_loop(p, d, stream);
}

extern "C" int f16_rollout_mpc_sched(f16_mpc_plan *p, double *x, double *u, const double *dem_seq, double *traj, double *cmd_traj,
                                     int32_t *iters_traj, int32_t *status, int nctrl, int hold, int dem_hold, int traj_every, double dt,
                                     double xcg, int fi_flag, unsigned flags, void *stream) {
  MpcLoop d{"f16_rollout_mpc_sched", x, u, dem_seq, traj, cmd_traj, iters_traj, status, nctrl, traj_every, xcg, fi_flag, flags};
  d.hold = hold; d.dt = dt; d.dem_hold = dem_hold;
  return rollout_mpc_loop(p, d, stream);
}

extern "C" int f16_rollout_mpc_relin_sched(f16_mpc_plan *p, double *x, double *u, const double *dem_seq, double *traj, double *cmd_traj,
                                           int32_t *iters_traj, double *model_traj, int32_t *status, int nctrl, int hold, int dem_hold,
                                           int traj_every, int model_every, double dt, double eps, double xcg, int fi_flag,
                                           unsigned flags, void *stream) {
  MpcLoop d{"f16_rollout_mpc_relin_sched", x, u, dem_seq, traj, cmd_traj, iters_traj, status, nctrl, traj_every, xcg, fi_flag, flags};
  d.hold = hold; d.dt = dt; d.dem_hold = dem_hold;
  d.relin = true; d.eps = eps; d.model_traj = model_traj; d.model_every = model_every;
  return rollout_mpc_loop(p, d, stream);
}

extern "C" int f16_mpc_plan_warm_start(f16_mpc_plan *p, int on) {
  if (!p) return set_error(F16_EINVAL, "bad argument to f16_mpc_plan_warm_start");
  if (on && p->N > FAST_MAXN) return set_error(F16_EINVAL, "warm start needs hzn <= 32 (the long-horizon solver starts cold)");
  if (on && !p->warm) {
    if (int rc = hip_check(hipMalloc(&p->warm, (size_t)p->B * MPC_WARM_DOUBLES * sizeof(double)), "hipMalloc warm start")) return rc;
  }
  p->warm_on = on != 0;
  p->have_prev = false;
  return F16_OK;
}

// Soft state rows (f16_osqp_rules.hpp): a property of the plan, honoured by every call that solves on it.  Served by the one-wavefront
// solver alone (f16_mpc_wave.hip: k_mpc_wave_soft, k_rollout_mpc_soft); the 512-lane solver, the long-horizon solver and the plans
// without equilibration have no soft twin.
extern "C" int f16_mpc_plan_soft_rows(f16_mpc_plan *p, const double *h_w9) {
  if (!p) return set_error(F16_EINVAL, "bad argument to f16_mpc_plan_soft_rows");
  double w6[6] = {0, 0, 0, 0, 0, 0};
  bool on = false;
  if (h_w9) {
    const int kept[9] = {-1, -1, 0, 1, 2, 3, 4, -1, 5};      // MPC state -> kept row (SROW); phi, theta, lf1 carry no bounds
    for (int i = 0; i < 9; ++i) {
      const double w = h_w9[i];
      if (!(w >= 0.0) || isinf(w)) return einval("f16_mpc_plan_soft_rows: weight %d must be finite and >= 0", i);
      if (w > 0.0 && kept[i] < 0) return einval("f16_mpc_plan_soft_rows: MPC state %d (phi, theta, lf1) carries no bounds to soften", i);
      if (kept[i] >= 0) w6[kept[i]] = w;
      on = on || w > 0.0;
    }
  }
  if (on && (p->N > WAVE_MAXN || p->s.scaling <= 0 || p->s.max_iter <= 0))
    return einval("f16_mpc_plan_soft_rows needs a plan of the one-wavefront solver: hzn <= 30 and equilibrated solves (scaling > 0); got hzn %d, "
                  "scaling %d", p->N, p->s.scaling);
  if (on) {
    MpcArgs probe = p->a;
    probe.mode = 0;
    if (!mpc_wave_enabled(probe)) return einval("f16_mpc_plan_soft_rows: the one-wavefront solver is switched off (F16_MPC_WAVE=0)");
  }
  p->soft_on = on;
  for (int i = 0; i < 6; ++i) p->soft6[i] = w6[i];
  p->have_prev = false;      // (as f16_mpc_plan_warm_start: a stored solution of the other problem is forgotten)
  return F16_OK;
}

extern "C" void f16_mpc_plan_destroy(f16_mpc_plan *p) {
  if (!p) return;
  // wait for the plan's own work only (the stream of its creation / last solve), not for every stream of the device
  (void)hipStreamSynchronize((hipStream_t)p->last_stream);
  (void)hipFree(p->buf);
  if (p->sched) (void)hipFree(p->sched);
  if (p->warm) (void)hipFree(p->warm);
  if (p->roll_sync) (void)hipFree(p->roll_sync);
  if (p->relin_w) (void)hipFree(p->relin_w);
  delete p;
}

extern "C" int f16_mpc_qp_debug(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, const double *x,
                                const double *dem, long b, long ld, int hzn, double dt, double *h_P, double *h_q, double *h_A,
                                double *h_l, double *h_u) {
  return f16_mpc_qp_debug_w(ctx, Ad, Bd, Cd, x, dem, nullptr, nullptr, b, ld, hzn, dt, h_P, h_q, h_A, h_l, h_u);
}

extern "C" int f16_mpc_qp_debug_w(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, const double *x,
                                  const double *dem, const double *x_ref, const f16_mpc_weights *h_w, long b, long ld, int hzn,
                                  double dt, double *h_P, double *h_q, double *h_A, double *h_l, double *h_u) {
  if (!ctx || !Ad || !Bd || !Cd || !x || (!dem && !x_ref) || b < 0 || b >= ld || !h_P || !h_q || !h_A || !h_l || !h_u)
    return set_error(F16_EINVAL, "bad argument to f16_mpc_qp_debug");
  f16_mpc_weights wd;
  f16_mpc_default_weights(&wd);
  const f16_mpc_weights *wq = h_w ? h_w : &wd;          // (the bounds of the dense QP below: any pattern)
  f16_mpc_weights wk = *wq;                              // (for the kernel: cost only -- its bounds are not used by the build)
  for (int i = 0; i < 9; ++i) { wk.x_lb[i] = wd.x_lb[i]; wk.x_ub[i] = wd.x_ub[i]; }
  for (int i = 0; i < 3; ++i) { wk.u_lb[i] = wd.u_lb[i]; wk.u_ub[i] = wd.u_ub[i]; wk.udot_lb[i] = wd.udot_lb[i]; wk.udot_ub[i] = wd.udot_ub[i]; }
  const int N = hzn, n = 3 * N, rows = 15 * N;
  if (N < 1 || N > BIG_MAXN) return set_error(F16_EINVAL, "horizon must be 1..150");
  const size_t np = (size_t)n * (n + 1) / 2;
  const size_t ndbg = mpc_ext_doubles(N);
  double *d_u = nullptr;
  int rc;
  if ((rc = hip_check(hipMalloc(&d_u, 3 * ld * sizeof(double)), "hipMalloc dbg u"))) return rc;
  MpcArgs a{};
  a.Ad = Ad; a.Bd = Bd; a.Cd = Cd; a.x = x; a.dem = dem; a.xref = x_ref; a.ucmd = d_u; a.B = b + 1; a.ld = ld; a.N = N; a.dt = dt;
  if ((rc = mpc_fill_prob(&a.pb, &wk))) { (void)hipFree(d_u); return rc; }
  f16_qp_default_settings(&a.s);
  void *block = nullptr;
  rc = mpc_launch(ctx, a, nullptr, 1, &block);      // build only; the workspace stays ours until read back
  std::vector<double> dbg(ndbg), Ppk(np), xcol(18);
  if (!rc) rc = hip_check(hipDeviceSynchronize(), "sync");
  if (!rc) rc = hip_check(hipMemcpy(dbg.data(), a.ext + ndbg * (size_t)b, ndbg * sizeof(double), hipMemcpyDeviceToHost), "copy ext");
  if (!rc) rc = hip_check(hipMemcpy(Ppk.data(), a.Ppk + np * (size_t)b, np * sizeof(double), hipMemcpyDeviceToHost), "copy P");
  for (int k = 0; k < 18 && !rc; ++k)
    rc = hip_check(hipMemcpy(&xcol[k], x + k * ld + b, sizeof(double), hipMemcpyDeviceToHost), "copy x");
  (void)hipFree(d_u);
  (void)mpc_work_free(block, nullptr);
  if (rc) return rc;
  // reference-format QP (utils.py:111-165): P dense, A = [CC; I; D] (15N x 3N), l/u with +-inf rows kept
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) h_P[i * n + j] = i >= j ? Ppk[(size_t)i * (i + 1) / 2 + j] : Ppk[(size_t)j * (j + 1) / 2 + i];
  for (int i = 0; i < n; ++i) h_q[i] = dbg[i];
  const double *G = dbg.data() + n, *pred = dbg.data() + n + N * 27;
  for (size_t i = 0; i < (size_t)rows * n; ++i) h_A[i] = 0.0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j <= i; ++j)
      for (int r = 0; r < 9; ++r)
        for (int c = 0; c < 3; ++c) h_A[(size_t)(9 * i + r) * n + 3 * j + c] = G[(i - j) * 27 + r * 3 + c];
  for (int k = 0; k < n; ++k) {
    h_A[(size_t)(9 * N + k) * n + k] = 1.0;
    h_A[(size_t)(12 * N + k) * n + k] = 1.0;
    if (k >= 3) h_A[(size_t)(12 * N + k) * n + k - 3] = -1.0;
  }
  const double *xlb = wq->x_lb, *xub = wq->x_ub, *ulb = wq->u_lb, *uub = wq->u_ub, *rlb = wq->udot_lb, *rub = wq->udot_ub;
  for (int i = 0; i < N; ++i)
    for (int r = 0; r < 9; ++r) {
      h_l[9 * i + r] = xlb[r] - pred[9 * i + r];
      h_u[9 * i + r] = xub[r] - pred[9 * i + r];
    }
  for (int k = 0; k < n; ++k) {
    h_l[9 * N + k] = ulb[k % 3];
    h_u[9 * N + k] = uub[k % 3];
    if (k < 3) {
      h_l[12 * N + k] = xcol[13 + k] + rlb[k] * dt;
      h_u[12 * N + k] = xcol[13 + k] + rub[k] * dt;
    } else {
      h_l[12 * N + k] = rlb[k % 3];
      h_u[12 * N + k] = rub[k % 3];
    }
  }
  return F16_OK;
}
