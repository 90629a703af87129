// f16_debug.hip -- test entry points that expose pieces of the device plant on their own.
//
//   k_dbg_table   ONE of the reference's 43 table functions (C/hifi_F16_AeroData.c:109-1861, each a lazy file read +
//                 interpn(), C/mexndinterp.c:97-265) evaluated by the SAME device helpers the dynamics kernels use
//                 (br_load / br_cell / br_axis / lerp / ld4 / bil4 on the node-major LDS image, f16_plant.hpp), one lane
//                 per query point.  The kernels never evaluate a single table -- lookups are fused per table group -- so
//                 without this entry the bracket / interpolation code is only checked through whole-Nlplant sums.
//   k_dbg_sincos  the branch-free sin/cos pair in its two forms on the same arguments: sincos_bf (constants as literals) and
//                 sincos_bf_k (the same table loaded into scalar registers, the form of the quad rollout).  The two must agree
//                 bit for bit; the rollouts only show that through whole trajectories.
//   k_dbg_pow     the atmosphere's exp(POW_FRAC log tfac) (POW_FRAC = 0.14, f16_plant.hpp) as the device library composes it and as
//                 exp_k / log_k repeat it with the constants in scalar registers, and qbar / ps of atmos_dev through either: the
//                 same bits.
//   k_dbg_elem_*  each elementary function of the default build on its own, on given arguments, for the multiprecision comparison of
//                 tests/test_gpu_elem.py: the sin/cos pair in its THREE forms (literals, table in scalar registers, table in vector
//                 registers as the quad rollout's G1 role holds it); the power factor by three routes with tfac, mach, qbar and ps
//                 at a given airspeed; f16_rcp; tan as plant_pre forms it; and the sin/cos pairs carried from step to step by
//                 trig_advance / trig_rotate.
//   k_dbg_air_triple  the air triple of the plant in moving air (air_triple, f16_wind.hpp: what calc_xdot_wind evaluates in front of
//                 its lookups) on given attitudes, ground triples, winds and gusts, for the multiprecision comparison of
//                 tests/test_gpu_air.py: the cancellation in U - wb - g and the device's sqrt, atan2 and asin on their own.
//   k_dbg_gain_lookup  the gain-schedule lookup over (h, V) of f16_rollout_lqr_gs (gain_lookup, f16_gain_sched.hpp) at given points:
//                 the same bits as the host function and the numpy restatement.
#include <hip/hip_runtime.h>

#include "../../include/f16_hip.h"
#include "f16_ctx.h"
#include "f16_plant.hpp"
#include "f16_gain_sched.hpp"
#include "f16_wind.hpp"

namespace f16 {

// table id (enum f16_table_id of f16_tables_data.inc) -> group of the node-major image
struct TabLoc { int off, stride, k, na, dims, dgrid; };     // dims 1: alpha; 2: alpha x beta; 3: + elevator; 0: eta(el)
__host__ __device__ inline TabLoc table_location(int tid) {
  if (tid < 3) return {OFF_G3A, S_G3A, tid, N_A1, 3, 1};
  if (tid < 5) return {OFF_G3B, S_G3B, tid - 3, N_A1, 3, 2};
  if (tid < 12) return {OFF_G2A, S_G2A, tid - 5, N_A1, 2, 0};
  if (tid < 21) return {OFF_G2B, S_G2B, tid - 12, N_A2, 2, 0};
  if (tid < 33) return {OFF_G1A, S_G1A, tid - 21, N_A1, 1, 0};
  if (tid < 42) return {OFF_G1B, S_G1B, tid - 33, N_A2, 1, 0};
  return {OFF_ETA, 1, 0, 0, 0, 1};
}

__global__ __launch_bounds__(64) void k_dbg_table(const double *__restrict__ tab, int tid, const double *alpha,
                                                  const double *beta, const double *el, double *out, int32_t *status, int n) {
  __shared__ __attribute__((aligned(16))) double T[TABLE_IMAGE_DOUBLES];
  stage_tables<64>(T, tab);
  const TabLoc L = table_location(tid);
  for (int p = blockIdx.x * 64 + threadIdx.x; p < n; p += gridDim.x * 64) {
    const double a = alpha[p], b = beta[p], e = el[p];
    int st = 0;
    // brackets exactly as aero_totals_phased takes them: alpha on ALPHA1 (the ALPHA2 grid is its prefix; beyond its last
    // node the lef tables are clamped: last cell, lambda = 1), beta on BETA1, elevator on DH1 or DH2
    const double *cT = T;
    const BrRaw ra = br_load(cT + OFF_BP_A1, N_A1, alpha_guess(a));
    const BrRaw rb = br_load(cT + OFF_BP_B1, N_B1, beta_guess(b));
    const BrRaw rd = L.dgrid == 2 ? br_load(cT + OFF_BP_D2, N_D2, (int)(e >= 0.0))
                                  : br_load(cT + OFF_BP_D1, N_D1, (e >= -10.0) + (e >= 0.0) + (e >= 10.0));
    bool offa, offb, offd;
    const BrCell ca = br_cell(ra, N_A1, a, offa), cb = br_cell(rb, N_B1, b, offb);
    const BrCell cd = br_cell(rd, L.dgrid == 2 ? N_D2 : N_D1, e, offd);
    Axis a1 = br_axis(ca);
    const Axis bx = br_axis(cb), dx = br_axis(cd);
    int ja = ca.j;
    if (L.na == N_A2) {
      const bool hi_a = ca.j > N_A2 - 2;
      if (hi_a) { ja = N_A2 - 2; a1.j = ja; a1.l = 1.0; a1.m = 0.0; if (a > cT[OFF_BP_A1 + N_A2 - 1]) st |= ST_ALPHA2; }
    }
    const W4 W1 = bil_weights(a1, bx);
    double v;
    if (L.dims == 0) {
      v = lerp(cT[OFF_ETA + cd.j], cT[OFF_ETA + cd.j + 1], dx);
      if (offd) st |= ST_EL;
    } else if (L.dims == 1) {
      const double *g = cT + L.off + ja * L.stride + L.k;
      v = lerp(g[0], g[L.stride], a1);
      if (offa) st |= ST_ALPHA1;
    } else {
      const int sa = L.stride, sb = L.stride * L.na;
      const double *p2 = cT + L.off + (cb.j * L.na + ja) * sa + L.k;
      if (L.dims == 2) {
        v = bil4w(ld4(p2, sa, sb), a1, bx, W1);
      } else {
        const int sd = L.stride * L.na * N_B1;
        v = lerp(bil4w(ld4(p2 + cd.j * sd, sa, sb), a1, bx, W1), bil4w(ld4(p2 + (cd.j + 1) * sd, sa, sb), a1, bx, W1), dx);
        if (offd) st |= ST_EL;
      }
      if (offa) st |= ST_ALPHA1;
      if (offb) st |= ST_BETA;
    }
    out[p] = v;
    if (status) status[p] = st;
  }
}

#ifdef F16_FAST_TRIG
// out: [4][n] = sin, cos by sincos_bf | sin, cos by sincos_bf_k
__global__ __launch_bounds__(64) void k_dbg_sincos(const double *__restrict__ x, double *__restrict__ out, long n) {
  const SinCosK sk = reloaded(QUAD_K.sc);
  for (long p = (long)blockIdx.x * 64 + threadIdx.x; p < n; p += (long)gridDim.x * 64) {
    double s0, c0, s1, c1;
    sincos_bf(x[p], &s0, &c0);
    sincos_bf_k(sk, x[p], &s1, &c1);
    out[p] = s0; out[n + p] = c0; out[2 * n + p] = s1; out[3 * n + p] = c1;
  }
}
#endif

#ifdef F16_FAST_POW
// out: [6][n] = the power factor, qbar, ps (vt = 500 ft/s) by the library composition | the same three by exp_k / log_k
__global__ __launch_bounds__(64) void k_dbg_pow(const double *__restrict__ alt, double *__restrict__ out, long n) {
  const PowK pk = reloaded(QUAD_K.pw);
  for (long p = (long)blockIdx.x * 64 + threadIdx.x; p < n; p += (long)gridDim.x * 64) {
    double pw0 = 0, pw1 = 0, mach, q0, p0, q1, p1;
    atmos_with(alt[p], 500.0, mach, q0, p0, [&](double tfac) { return pw0 = exp(POW_FRAC * log(tfac)); });
    atmos_with(alt[p], 500.0, mach, q1, p1, [&](double tfac) { return pw1 = exp_k(pk, POW_FRAC * log_k(pk, tfac)); });
    out[p] = pw0; out[n + p] = q0; out[2 * n + p] = p0; out[3 * n + p] = pw1; out[4 * n + p] = q1; out[5 * n + p] = p1;
  }
}
#endif

#ifdef F16_FAST_TRIG
// out: [6][n] = sin, cos by sincos_bf | by sincos_bf_k<KScalar> | by sincos_bf_k<KVector>, the table loaded and moved as the quad
// rollout's role loops do it (f16_quad_steps.inc: reloaded, table_in_vgprs)
__global__ __launch_bounds__(64) void k_dbg_elem_sincos(const double *__restrict__ x, double *__restrict__ out, long n) {
  const SinCosK sk = reloaded(QUAD_K.sc);
  SinCosK sv = reloaded(QUAD_K.sc);
  table_in_vgprs(sv);
  for (long p = (long)blockIdx.x * 64 + threadIdx.x; p < n; p += (long)gridDim.x * 64) {
    double s0, c0, s1, c1, s2, c2;
    sincos_bf(x[p], &s0, &c0);
    sincos_bf_k<KScalar>(sk, x[p], &s1, &c1);
    sincos_bf_k<KVector>(sv, x[p], &s2, &c2);
    out[p] = s0; out[n + p] = c0; out[2 * n + p] = s1; out[3 * n + p] = c1; out[4 * n + p] = s2; out[5 * n + p] = c2;
  }
}

// in: [1 + n_steps][n] = start angle | one increment per step;  out: [n_steps][4][n] = sin, cos, angle, verdict (0 / 1) after every step.
// The lane's angle is the pitch angle of a state whose other angles stay 0 (their pairs rotate (0, 1) by 0: unchanged), so that
// trig_exact, trig_store and trig_advance themselves run, on slots in registers instead of LDS.
__global__ __launch_bounds__(64) void k_dbg_elem_trig_carry(const double *__restrict__ in, int n_steps, double *__restrict__ out, long n) {
  for (long p = (long)blockIdx.x * 64 + threadIdx.x; p < n; p += (long)gridDim.x * 64) {
    double x[9] = {0, 0, 0, 0, in[p], 0, 0, 0, 0}, slots[10];
    const TrigSlots ts = {slots, 1};
    Trig5 g;
    trig_exact(x, g);
    trig_store(ts, g);
    for (int k = 0; k < n_steps; ++k) {
      const double xo5[5] = {0, 0, x[4], 0, 0};
      x[4] = x[4] + in[(long)(1 + k) * n + p];               // xn = xo + d, as the Euler step leaves it in the state
      const bool stale = trig_advance(xo5, x, ts);           // (the increment taken back as xn - xo)
      double *o = out + (long)k * 4 * n + p;
      o[0] = slots[4]; o[n] = slots[5]; o[2 * n] = x[4]; o[3 * n] = stale ? 1.0 : 0.0;
    }
  }
}
#endif

#ifdef F16_FAST_POW
// in: [2][n] = altitude, airspeed;  out: [13][n] = tfac | factor, mach, qbar, ps by atmos_dev (library exp / log) | the same four by
// atmos_dev_k (exp_k / log_k, table in scalar registers) | the same four with the table in vector registers
__global__ __launch_bounds__(64) void k_dbg_elem_atmos(const double *__restrict__ in, double *__restrict__ out, long n) {
  const PowK pk = reloaded(QUAD_K.pw);
  PowK pv = reloaded(QUAD_K.pw);
  table_in_vgprs(pv);
  for (long p = (long)blockIdx.x * 64 + threadIdx.x; p < n; p += (long)gridDim.x * 64) {
    const double alt = in[p], vt = in[n + p], tfac = atmos_alt(alt).tfac;
    double m0, q0, p0, m1, q1, p1, m2, q2, p2, pw2 = 0;
    atmos_dev(alt, vt, m0, q0, p0);
    atmos_dev_k(pk, alt, vt, m1, q1, p1);
    atmos_with(alt, vt, m2, q2, p2, [&](double t) { return pw2 = exp_k<KVector>(pv, POW_FRAC * log_k<KVector>(pv, t)); });
    out[p] = tfac;
    out[n + p] = exp(POW_FRAC * log(tfac)); out[2 * n + p] = m0; out[3 * n + p] = q0; out[4 * n + p] = p0;
    out[5 * n + p] = exp_k<KScalar>(pk, POW_FRAC * log_k<KScalar>(pk, tfac)); out[6 * n + p] = m1; out[7 * n + p] = q1; out[8 * n + p] = p1;
    out[9 * n + p] = pw2; out[10 * n + p] = m2; out[11 * n + p] = q2; out[12 * n + p] = p2;
  }
}
#endif

#ifdef F16_FAST_DIV
// out: [n] = f16_rcp(x)
__global__ __launch_bounds__(64) void k_dbg_elem_rcp(const double *__restrict__ x, double *__restrict__ out, long n) {
  for (long p = (long)blockIdx.x * 64 + threadIdx.x; p < n; p += (long)gridDim.x * 64) out[p] = f16_rcp(x[p]);
}
// out: [3][n] = sin theta, cos theta, tt = sin theta * f16_rcp(cos theta) as plant_pre forms it
__global__ __launch_bounds__(64) void k_dbg_elem_tan(const double *__restrict__ theta, double *__restrict__ out, long n) {
  for (long p = (long)blockIdx.x * 64 + threadIdx.x; p < n; p += (long)gridDim.x * 64) {
    double st, ct;
    F16_SINCOS(theta[p], &st, &ct);
    const double rct = f16_rcp(ct);
    out[p] = st; out[n + p] = ct; out[2 * n + p] = st * rct;
  }
}
#endif

// in [12][n] = phi theta psi vt alpha beta | wN wE wD | g_x g_y g_z; out [6][n] = Ua Va Wa vt_a alpha_a beta_a
__global__ __launch_bounds__(64) void k_dbg_air_triple(const double *__restrict__ in, double *__restrict__ out, long n) {
  for (long p = (long)blockIdx.x * 64 + threadIdx.x; p < n; p += (long)gridDim.x * 64) {
    double x[9], w[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { x[3 + k] = in[k * n + p]; w[k] = in[(6 + k) * n + p]; }
    AirTriple a;
    air_triple(x, [&](int k) { return w[k]; }, a);
    out[p] = a.Ua; out[n + p] = a.Va; out[2 * n + p] = a.Wa; out[3 * n + p] = a.vt; out[4 * n + p] = a.alpha; out[5 * n + p] = a.beta;
  }
}

// the gain-schedule lookup of the scheduled-gain rollouts (gain_lookup, f16_gain_sched.hpp) on its own: out [n][12]
__global__ __launch_bounds__(64) void k_dbg_gain_lookup(f16_gain_grid g, const double *__restrict__ tab, const double *__restrict__ h,
                                                        const double *__restrict__ v, double *__restrict__ out, long n) {
  for (long p = (long)blockIdx.x * 64 + threadIdx.x; p < n; p += (long)gridDim.x * 64) {
    double o[F16_GS_ENTRIES];
    gain_lookup(g, tab, h[p], v[p], o);
#pragma unroll
    for (int e = 0; e < F16_GS_ENTRIES; ++e) out[p * F16_GS_ENTRIES + e] = o[e];
  }
}

}  // namespace f16

using namespace f16;

extern "C" int f16_debug_gain_lookup(f16_ctx *ctx, const f16_gain_grid *g, const double *tab, const double *h_h, const double *h_v, long n,
                                     double *h_out) {
  if (!ctx || !tab || !h_h || !h_v || !h_out || n < 0) return set_error(F16_EINVAL, "bad argument to f16_debug_gain_lookup");
  if (const char *bad = gain_grid_error(g)) return set_error(F16_EINVAL, bad);
  if (n == 0) return F16_OK;
  double *d = nullptr;
  int rc;
  if ((rc = hip_check(hipMalloc(&d, (2 + F16_GS_ENTRIES) * (size_t)n * sizeof(double)), "hipMalloc dbg gain lookup"))) return rc;
  const size_t nb = (size_t)n * sizeof(double);
  if (!(rc = hip_check(hipMemcpy(d, h_h, nb, hipMemcpyHostToDevice), "copy h")) &&
      !(rc = hip_check(hipMemcpy(d + n, h_v, nb, hipMemcpyHostToDevice), "copy v"))) {
    const long blocks = (n + 63) / 64;
    hipLaunchKernelGGL(k_dbg_gain_lookup, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(64), 0, nullptr, *g, tab, d, d + n, d + 2 * n, n);
    rc = hip_check(hipGetLastError(), "f16_debug_gain_lookup launch");
    if (!rc) rc = hip_check(hipMemcpy(h_out, d + 2 * n, F16_GS_ENTRIES * nb, hipMemcpyDeviceToHost), "copy out");
  }
  (void)hipFree(d);
  return rc;
}

extern "C" int f16_debug_table_lookup(f16_ctx *ctx, int tid, const double *h_alpha, const double *h_beta, const double *h_el,
                                      int n, double *h_out, int32_t *h_status) {
  if (!ctx || tid < 0 || tid > 42 || !h_alpha || !h_beta || !h_el || !h_out || n < 0)
    return set_error(F16_EINVAL, "bad argument to f16_debug_table_lookup");
  if (n == 0) return F16_OK;
  double *d = nullptr;
  int32_t *ds = nullptr;
  int rc;
  if ((rc = hip_check(hipMalloc(&d, 4 * (size_t)n * sizeof(double)), "hipMalloc dbg table"))) return rc;
  if ((rc = hip_check(hipMalloc(&ds, (size_t)n * sizeof(int32_t)), "hipMalloc dbg table"))) { (void)hipFree(d); return rc; }
  const size_t nb = (size_t)n * sizeof(double);
  if (!(rc = hip_check(hipMemcpy(d, h_alpha, nb, hipMemcpyHostToDevice), "copy alpha")) &&
      !(rc = hip_check(hipMemcpy(d + n, h_beta, nb, hipMemcpyHostToDevice), "copy beta")) &&
      !(rc = hip_check(hipMemcpy(d + 2 * (size_t)n, h_el, nb, hipMemcpyHostToDevice), "copy el"))) {
    const int blocks = (n + 63) / 64;
    hipLaunchKernelGGL(k_dbg_table, dim3(blocks < 256 ? blocks : 256), dim3(64), 0, nullptr, ctx->d_tab, tid, d, d + n,
                       d + 2 * (size_t)n, d + 3 * (size_t)n, ds, n);
    rc = hip_check(hipGetLastError(), "f16_debug_table_lookup launch");
    if (!rc) rc = hip_check(hipMemcpy(h_out, d + 3 * (size_t)n, nb, hipMemcpyDeviceToHost), "copy out");
    if (!rc && h_status) rc = hip_check(hipMemcpy(h_status, ds, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost), "copy status");
  }
  (void)hipFree(d);
  (void)hipFree(ds);
  return rc;
}

extern "C" int f16_debug_sincos(f16_ctx *ctx, const double *h_x, long n, double *h_out) {
  if (!ctx || !h_x || !h_out || n < 0) return set_error(F16_EINVAL, "bad argument to f16_debug_sincos");
#ifdef F16_FAST_TRIG
  if (n == 0) return F16_OK;
  double *d = nullptr;
  int rc;
  if ((rc = hip_check(hipMalloc(&d, 5 * (size_t)n * sizeof(double)), "hipMalloc dbg sincos"))) return rc;
  if (!(rc = hip_check(hipMemcpy(d, h_x, (size_t)n * sizeof(double), hipMemcpyHostToDevice), "copy x"))) {
    const long blocks = (n + 63) / 64;
    hipLaunchKernelGGL(k_dbg_sincos, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(64), 0, nullptr, d, d + n, n);
    rc = hip_check(hipGetLastError(), "f16_debug_sincos launch");
    if (!rc) rc = hip_check(hipMemcpy(h_out, d + n, 4 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost), "copy out");
  }
  (void)hipFree(d);
  return rc;
#else
  return set_error(F16_EINVAL, "f16_debug_sincos: this library was built without F16_FAST_TRIG (libm sincos, one form only)");
#endif
}

extern "C" int f16_debug_pow(f16_ctx *ctx, const double *h_alt, long n, double *h_out) {
  if (!ctx || !h_alt || !h_out || n < 0) return set_error(F16_EINVAL, "bad argument to f16_debug_pow");
#ifdef F16_FAST_POW
  if (n == 0) return F16_OK;
  double *d = nullptr;
  int rc;
  if ((rc = hip_check(hipMalloc(&d, 7 * (size_t)n * sizeof(double)), "hipMalloc dbg pow"))) return rc;
  if (!(rc = hip_check(hipMemcpy(d, h_alt, (size_t)n * sizeof(double), hipMemcpyHostToDevice), "copy alt"))) {
    const long blocks = (n + 63) / 64;
    hipLaunchKernelGGL(k_dbg_pow, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(64), 0, nullptr, d, d + n, n);
    rc = hip_check(hipGetLastError(), "f16_debug_pow launch");
    if (!rc) rc = hip_check(hipMemcpy(h_out, d + n, 6 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost), "copy out");
  }
  (void)hipFree(d);
  return rc;
#else
  return set_error(F16_EINVAL, "f16_debug_pow: this library was built without F16_FAST_POW (libm pow, one form only)");
#endif
}

// ---- the elementary functions on their own (tests/test_gpu_elem.py)
// The host side the entries below share: rows_in arrays of n doubles up (h_in: contiguous), one launch of `kernel` on (in, out, n) by
// grid-stride workgroups of 64, rows_out arrays of n doubles back.
template <typename LAUNCH>
static int dbg_elem_run(const char *what, const double *h_in, size_t rows_in, long n, double *h_out, size_t rows_out, LAUNCH launch) {
  double *d = nullptr;
  int rc;
  if ((rc = hip_check(hipMalloc(&d, (rows_in + rows_out) * (size_t)n * sizeof(double)), what))) return rc;
  if (!(rc = hip_check(hipMemcpy(d, h_in, rows_in * (size_t)n * sizeof(double), hipMemcpyHostToDevice), what))) {
    const long blocks = (n + 63) / 64;
    launch(dim3((unsigned)(blocks < 1024 ? blocks : 1024)), d, d + rows_in * (size_t)n);
    rc = hip_check(hipGetLastError(), what);
    if (!rc) rc = hip_check(hipMemcpy(h_out, d + rows_in * (size_t)n, rows_out * (size_t)n * sizeof(double), hipMemcpyDeviceToHost), what);
  }
  (void)hipFree(d);
  return rc;
}

extern "C" int f16_debug_elem_sincos(f16_ctx *ctx, const double *h_x, long n, double *h_out) {
  if (!ctx || !h_x || !h_out || n < 0) return set_error(F16_EINVAL, "bad argument to f16_debug_elem_sincos");
#ifdef F16_FAST_TRIG
  if (n == 0) return F16_OK;
  return dbg_elem_run("f16_debug_elem_sincos", h_x, 1, n, h_out, 6, [&](dim3 grid, const double *in, double *out) {
    hipLaunchKernelGGL(k_dbg_elem_sincos, grid, dim3(64), 0, nullptr, in, out, n);
  });
#else
  return set_error(F16_EINVAL, "f16_debug_elem_sincos: this library was built without F16_FAST_TRIG (libm sincos, one form only)");
#endif
}

extern "C" int f16_debug_elem_trig_carry(f16_ctx *ctx, const double *h_angle_and_steps, int n_steps, long n, double *h_out) {
  if (!ctx || !h_angle_and_steps || !h_out || n < 0 || n_steps < 1 || n_steps > 4096)
    return set_error(F16_EINVAL, "bad argument to f16_debug_elem_trig_carry");
#ifdef F16_FAST_TRIG
  if (n == 0) return F16_OK;
  return dbg_elem_run("f16_debug_elem_trig_carry", h_angle_and_steps, 1 + (size_t)n_steps, n, h_out, 4 * (size_t)n_steps,
                      [&](dim3 grid, const double *in, double *out) {
                        hipLaunchKernelGGL(k_dbg_elem_trig_carry, grid, dim3(64), 0, nullptr, in, n_steps, out, n);
                      });
#else
  return set_error(F16_EINVAL, "f16_debug_elem_trig_carry: this library was built without F16_FAST_TRIG (libm sincos, one form only)");
#endif
}

extern "C" int f16_debug_elem_atmos(f16_ctx *ctx, const double *h_alt_vt, long n, double *h_out) {
  if (!ctx || !h_alt_vt || !h_out || n < 0) return set_error(F16_EINVAL, "bad argument to f16_debug_elem_atmos");
#ifdef F16_FAST_POW
  if (n == 0) return F16_OK;
  return dbg_elem_run("f16_debug_elem_atmos", h_alt_vt, 2, n, h_out, 13, [&](dim3 grid, const double *in, double *out) {
    hipLaunchKernelGGL(k_dbg_elem_atmos, grid, dim3(64), 0, nullptr, in, out, n);
  });
#else
  return set_error(F16_EINVAL, "f16_debug_elem_atmos: this library was built without F16_FAST_POW (libm pow, one form only)");
#endif
}

extern "C" int f16_debug_elem_rcp(f16_ctx *ctx, const double *h_x, long n, double *h_out) {
  if (!ctx || !h_x || !h_out || n < 0) return set_error(F16_EINVAL, "bad argument to f16_debug_elem_rcp");
#ifdef F16_FAST_DIV
  if (n == 0) return F16_OK;
  return dbg_elem_run("f16_debug_elem_rcp", h_x, 1, n, h_out, 1, [&](dim3 grid, const double *in, double *out) {
    hipLaunchKernelGGL(k_dbg_elem_rcp, grid, dim3(64), 0, nullptr, in, out, n);
  });
#else
  return set_error(F16_EINVAL, "f16_debug_elem_rcp: this library was built without F16_FAST_DIV (IEEE division, one form only)");
#endif
}

extern "C" int f16_debug_elem_tan(f16_ctx *ctx, const double *h_theta, long n, double *h_out) {
  if (!ctx || !h_theta || !h_out || n < 0) return set_error(F16_EINVAL, "bad argument to f16_debug_elem_tan");
#ifdef F16_FAST_DIV
  if (n == 0) return F16_OK;
  return dbg_elem_run("f16_debug_elem_tan", h_theta, 1, n, h_out, 3, [&](dim3 grid, const double *in, double *out) {
    hipLaunchKernelGGL(k_dbg_elem_tan, grid, dim3(64), 0, nullptr, in, out, n);
  });
#else
  return set_error(F16_EINVAL, "f16_debug_elem_tan: this library was built without F16_FAST_DIV (IEEE division, one form only)");
#endif
}

extern "C" int f16_debug_air_triple(f16_ctx *ctx, const double *h_in, long n, double *h_out) {
  if (!ctx || !h_in || !h_out || n < 0) return set_error(F16_EINVAL, "bad argument to f16_debug_air_triple");
  if (n == 0) return F16_OK;
  return dbg_elem_run("f16_debug_air_triple", h_in, 12, n, h_out, 6, [&](dim3 grid, const double *in, double *out) {
    hipLaunchKernelGGL(k_dbg_air_triple, grid, dim3(64), 0, nullptr, in, out, n);
  });
}
