/* oracle/f16_oracle.h -- TEST INFRASTRUCTURE, NOT PRODUCT.
 *
 * CPU restatement (plain C, fp64 -- or extended precision, below --, no fast-math, no FMA contraction) of the
 * reference's F-16 plant + actuator + Euler path.  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load this library.  The product
 * (f16_mpc_oop_py_amd + libf16hip.so) never links, imports or calls it.
 *
 * Parity pinning: checked in tests/test_oracle_vs_golden.py against fixtures that
 * were generated in the build container from the reference's own prebuilt
 * C/nlplant_xcg25.so / nlplant_xcg35.so and its Python (tools/make_golden.py).
 *
 * State x[18] = {npos,epos,h,phi,theta,psi,V,alpha,beta,p,q,r,T,dh,da,dr,lf2,lf1}
 * (parameters.py:116), input u[4] = {T,dh,da,dr} (parameters.py:117).
 */
#ifndef F16_ORACLE_H
#define F16_ORACLE_H
#ifdef __cplusplus
extern "C" {
#endif

/* The type the restatement computes in: fp64, or -- compiled with -DF16O_LONG_DOUBLE into libf16_oracle_ld.so -- x87 extended
 * precision (64-bit significand), the reference of tests/linearise_cases.py.  Every entry below that takes or returns `double`
 * does so in both builds (the wide build widens on the way in and rounds on the way out); only the entries written on f16o_real
 * hand the wide values over. */
#ifdef F16O_LONG_DOUBLE
typedef long double f16o_real;
#else
typedef double f16o_real;
#endif

/* status bits (sticky per aircraft in the batched calls) */
#define F16O_ST_ALPHA1 1  /* alpha outside ALPHA1 grid [-20,90] deg           */
#define F16O_ST_ALPHA2 2  /* alpha outside ALPHA2 grid [-20,45] deg (lef tabs) */
#define F16O_ST_BETA 4    /* |beta| > 30 deg                                  */
#define F16O_ST_EL 8      /* |el| > 25 deg                                    */
#define F16O_ST_ENVELOPE 16 /* env.py:117-124 box check failed -> frozen       */

void f16o_init(void);
void f16o_set_xcg(double xcg);   /* used by the drop-in Nlplant symbol (default 0.25) */
void f16o_set_fix_clr(int on);   /* 1: use the real CLr table instead of the reference's unloaded one */
int f16o_last_status(void);      /* grid-clamp bits raised by the last single call in this thread */

/* reference-shaped drop-in symbols (C/nlplant.c:23, :467, :512) */
void Nlplant(double *xu, double *xdot, int fidelity);
void atmos(double alt, double vt, double *coeff);
void accels(double *state, double *xdot, double *y);

/* one of the 43 hifi table functions (C/hifi_F16_AeroData.c:109-1861); tid = enum f16_table_id */
double f16o_table(int tid, double alpha, double beta, double el);
/* lofi group functions, C/lofi_F16_AeroData.c:12-368: which = 0 damping(9) 1 dmomdcon(4) 2 clcn(2) 3 cxcm(2) 4 cz(1) */
void f16o_lofi(int which, double alpha, double beta, double el, double *out);

void f16o_nlplant(const double *xu, double *xdot, int fi_flag, double xcg);
/* env.py:65-103 */
void f16o_calc_xdot(const double *x, const double *u, double *xdot, int fi_flag, double xcg);
/* env.py:152-193: x_full/u_full are self.x.values / self.u.values; x9,u3 the MPC vectors */
void f16o_calc_xdot_na(const double *x_full, const double *x9, const double *u3, double *xdot9, int fi_flag, double xcg);
int f16o_envelope_bits(const double *x);   /* env.py:117-124 alone */
/* env.py:105-130; returns status bits (envelope bit => state left untouched) */
int f16o_step(double *x, const double *u, double dt, int fi_flag, double xcg);
/* env.py:294-342 with _calc_xdot_na/_get_obs_na: A[9*9] B[9*3] C[9*9] D[9*3], row-major */
void f16o_linearise_na(const double *x_full, const double *x9, const double *u3, double eps,
                       double *A, double *B, double *C, double *D, int fi_flag, double xcg);
/* env.py:294-342 default (18-state): A[18*18] B[18*4] C[10*18] D[10*4] */
void f16o_linearise_full(const double *x, const double *u, double eps,
                         double *A, double *B, double *C, double *D, int fi_flag, double xcg);

/* sizeof(f16o_real) of this build (8 or 16), and the tables as the build holds them: breakpoints [5][20], the hifi tables, the
 * lofi tables, concatenated; returns their count and writes at most n of them.  In both builds every value is an fp64 number. */
int f16o_real_bytes(void);
long f16o_table_image(f16o_real *out, long n);
/* f16o_linearise_na / _full for B aircraft (x [B][18], u [B][4]; the reduced model at x9 = x[mpc idx], u3 = u[1..3], the point of
 * f16_linearise_batch), matrices in f16o_real: A [B][81] Bm [B][27] C [B][81], 18-state A [B][324] Bm [B][72] C [B][180].  The
 * perturbed coordinate is the fp64 sum fl64(x + eps) in both builds.  status (may be NULL) [B] receives the OR of the grid-clamp
 * bits of the base point and of EVERY perturbed point (f16o_last_status: the last evaluation only).  OpenMP, thread count from the
 * environment. */
void f16o_linearise_na_batch(const double *x, const double *u, long B, double eps, f16o_real *A, f16o_real *Bm, f16o_real *C,
                             int *status, int fi_flag, double xcg);
void f16o_linearise_full_batch(const double *x, const double *u, long B, double eps, f16o_real *A, f16o_real *Bm, f16o_real *C,
                               int *status, int fi_flag, double xcg);

/* The plant in MOVING AIR (include/f16_hip.h "STEADY WIND", csrc/f16_wind.hpp: calc_xdot_wind), written on f16o_real like the rest:
 * the ground U, V, W from the clamped vt, wb = C w_ned, (Ua, Va, Wa), vt_a = sqrt(..), alpha_a = atan2(Wa, Ua), beta_a = asin(Va /
 * vt_a); the air triple feeds the lookups and the coefficient build-up, the damping quotients and the atmosphere call (vt_a clamped
 * at 0.01) and the flap model (the raw vt_a); the ground triple stays in the kinematics and the force equations.  ONE evaluation of
 * the plant, not two still-air evaluations and a reconstruction.
 *   x [B][18], u [B][4], air [B][6] = wN wE wD g_x g_y g_z -> out [B][18]; triple (may be NULL) [B][6] = Ua Va Wa vt_a alpha_a beta_a;
 *   status (may be NULL) [B] = the grid bits of the lookups.  Results in the build's own type, never rounded on the way. */
void f16o_xdot_wind_batch(const double *x, const double *u, const double *air, long B, f16o_real *out, f16o_real *triple, int *status,
                          int fi_flag, double xcg);
/* The same derivative with every consumer of the air triple handed its own copy: parts [B][6] = {vt of the atmosphere call, vt of
 * the damping quotients, alpha and beta of the lookups, V and alpha of the flap model}.  The rule is (max(vt_a, 0.01), max(vt_a,
 * 0.01), alpha_a, beta_a, vt_a, alpha_a); tests/test_air_cpu.py states deliberately WRONG rules through this entry to show that the
 * comparison can fail. */
void f16o_xdot_air_parts_batch(const double *x, const double *u, const f16o_real *parts, long B, f16o_real *out, int *status, int fi_flag,
                               double xcg);
/* nsteps steps of B aircraft in moving air, method 1 = Euler (env.py:126), 4 = classical Runge-Kutta (x + (dt/6) ((k1 + 2 k2) + (2 k3
 * + k4))), the box test of env.py:117-124 in front of every step as in f16o_step (a frozen aircraft keeps its state).  x0 [B][18];
 * rows [S][B][4] commands, step t reads row t / hold -- or, with K [B][27] and u0 [B][4] given, rows [S][B][3] demanded rates and the
 * action of env.py:360-371 from the state at the start of the step; wind [B][3] (NULL = 0) constant; gust [Sg][B][3] (NULL = 0), step
 * t reads row t / gust_hold; wind, gust and command held over the four stages.  The state stays in f16o_real between steps and is
 * handed back so: x_out [B][18], traj (may be NULL) [nsteps][B][18], u_out (may be NULL) [B][4] the action of the last step taken.
 * status [B] in / out, sticky: grid bits of every evaluation | f16o_envelope_bits. */
void f16o_rollout_wind(const double *x0, const double *rows, const double *K, const double *u0, const double *wind, const double *gust,
                       long B, int nsteps, int hold, int gust_hold, double dt, int method, int fi_flag, double xcg,
                       f16o_real *x_out, f16o_real *traj, f16o_real *u_out, int *status);

/* batched helpers (row-major [B][18] / [B][4]); nthreads<=1 => serial. traj may be NULL,
 * else [T][B][18] filled after every step. status[B] in/out (sticky). */
void f16o_xdot_batch(const double *x, const double *u, double *xdot, long B, int fi_flag, double xcg, int nthreads);
void f16o_rollout(double *x, const double *u, long B, int T, double dt, int fi_flag, double xcg,
                  double *traj, int *status, int nthreads);

/* test_env_mk2.py:70-85 (nonlinear LQR loop) for B aircraft: env.py:360-371 action + env.py:105-130 step, T times */
void f16o_rollout_lqr(double *x, const double *u0, const double *K, const double *dem, long B, int T, double dt, int fi_flag,
                      double xcg, double *traj, double *u_out, int *status, int nthreads);

#ifdef __cplusplus
}
#endif
#endif
