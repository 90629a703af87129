/* include/f16_hip.h -- C-ABI of libf16hip.so: the MI355X (gfx950) replacement for the reference's
 * ctypes boundary  CDLL("C/nlplant_xcg{25,35}.so")  (parameters.py:108-114; call sites env.py:100,
 * env.py:187, utils.py:291).
 *
 * Two groups of entry points:
 *  (1) the reference's own two symbols, same signatures, host pointers, synchronous -- so an
 *      unmodified reference-style caller keeps working when its CDLL handle points here;
 *  (2) batched entry points over DEVICE pointers for thousands of independent aircraft per
 *      launch.  They replace the Python loops of env.py:105-130 (step), :65-103 (_calc_xdot),
 *      :152-193 (_calc_xdot_na), :294-342 (linearise), :344-371 (LQR), :373-424 (MPC).
 *
 * Conventions for group (2)
 *  - every pointer is a device pointer unless named h_*; nothing is retained after the call
 *  - batched vectors are state-major ("SoA"): element k of aircraft b lives at  p[k*ld + b],
 *    ld >= B (leading dimension, in doubles).  State order x[18] and input order u[4] are the
 *    reference's (parameters.py:116-117).
 *  - all arithmetic fp64; xcg is a run-time argument (the reference bakes it in at compile time,
 *    C/nlplant.c:34, and ships two binaries); fi_flag 1 = hifi Nguyen, 0 = lofi Stevens-Lewis
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous
 *  - return value: 0 on success, negative F16_E* on a host-side error (bad argument, HIP error);
 *    per-aircraft conditions are reported in the int32 status[] words (sticky OR of F16_ST_* bits).
 *    The reference has no error returns: it printf()s and runs into UB off-grid
 *    (C/mexndinterp.c:121-124) and exit()s on an envelope violation (env.py:117-124).
 */
#ifndef F16_HIP_H
#define F16_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct f16_ctx f16_ctx;

/* host-side error codes */
#define F16_OK 0
#define F16_EINVAL (-1)   /* bad argument (NULL pointer, ld < B, unsupported size) */
#define F16_EHIP (-2)     /* a HIP runtime call failed; see f16_last_error() */
#define F16_ENOGPU (-3)   /* no gfx950 device visible */

/* per-aircraft status bits */
#define F16_ST_ALPHA1 1     /* alpha left the ALPHA1 grid [-20,90] deg: lookup clamped        */
#define F16_ST_ALPHA2 2     /* alpha left the ALPHA2 grid [-20,45] deg (lef tables): clamped  */
#define F16_ST_BETA 4       /* |beta| > 30 deg: clamped                                       */
#define F16_ST_EL 8         /* |el| > 25 deg: clamped                                         */
/* (the four grid bits above belong to the hifi tables.  The lofi model extrapolates beyond alpha -10 / 45 deg and beyond its
 *  elevator rows exactly as the reference's lofi_F16_AeroData.c does, inside its arrays and without a bit; its only off-table
 *  read is at fix(0.2 |beta|) >= 6, i.e. |beta| >= 30 deg and the one double below it: row held, F16_ST_BETA) */
#define F16_ST_ENVELOPE 16  /* env.py:117-124 box check failed: aircraft frozen from then on  */
#define F16_ST_ENV_STATE(k) (1 << (8 + (k))) /* ... and WHICH of the 18 states were outside their box at that step (set with
                                                F16_ST_ENVELOPE; the reference prints the offending state before it exits)       */
#define F16_ST_NONFINITE 32 /* a state became NaN/Inf                                         */
#define F16_ST_QP_MAXITER 64 /* ADMM hit max_iter before meeting the OSQP termination test    */
#define F16_ST_QP_INFEASIBLE 128 /* OSQP primal-infeasibility certificate met: command = NaN  */
#define F16_ST_LOOP_STALL (1 << 26) /* f16_rollout_mpc: a wavefront gave up waiting (tens of seconds) for the previous step of this
                                       aircraft and went on regardless -- a guard that lets the grid drain; never observed          */
#define F16_ST_QP_SOFT_ACTIVE (1 << 27) /* f16_mpc_plan_soft_rows: the returned solve has a soft state row outside its [l, u]        */

/* behaviour flags */
#define F16_FLAG_FIX_CLR 1u      /* use the real CLr table (reference never loads it: hifi_F16_AeroData.c:964-972) */
#define F16_FLAG_NO_ENVELOPE 2u  /* skip the env.py:117-124 box check in step/rollout                               */
#define F16_FLAG_ONE_LANE 4u     /* f16_rollout / f16_rollout_lqr: always the one-lane-per-aircraft kernel (64-lane workgroups), whatever
                                    the batch size -- results then do not depend on B bit for bit (the launch rules otherwise pick a
                                    four-lanes-per-aircraft or four-wavefront kernel for small batches: same terms, the six coefficient
                                    totals summed in another order, ulp-level differences).  f16_rollout_mpc steps with exactly this code. */
#define F16_FLAG_HOLD_COMMAND 8u /* closed MPC loops (f16_rollout_mpc; dist.closed_loop_mpc_rollout(hold_command=True)): a step whose QP
                                    is infeasible (or whose state is not finite) keeps the PREVIOUS surface commands instead of the NaN
                                    the reference would write into u.values (env.py:420-424 -> test_env.py:490-493)                  */
#define F16_FLAG_NO_CELL_CACHE 16u /* diagnostic: the quad rollout kernel (B <= 8192, hifi) re-brackets every table axis on every
                                    step instead of re-using the previous step's cell while the value stays inside it.  Results
                                    are bit-identical either way; the flag exists so that tests can compare the two paths.   */

/* ---- lifetime --------------------------------------------------------------------------- */
/* Builds the fp64 table image (int/1e5, IEEE division) and uploads it to `device`. */
int f16_create(f16_ctx **out, int device);
void f16_destroy(f16_ctx *ctx);
const char *f16_last_error(void);
/* bytes of LDS image / number of doubles, for tests and the roofline bookkeeping */
size_t f16_table_image_doubles(void);
/* copy the device table image back to host (tests): n = f16_table_image_doubles() */
int f16_debug_read_tables(f16_ctx *ctx, double *h_out);
/* the same tables as the scaled-integer image the large-batch rollout reads (value = k / 1e5; breakpoints as doubles in
 * front, csrc/f16_tables.h namespace i32): n_ints = f16_table_image_i32_ints() */
size_t f16_table_image_i32_ints(void);
int f16_debug_read_tables_i32(f16_ctx *ctx, int32_t *h_out);

/* Tests: ONE of the reference's 43 hifi table functions (C/hifi_F16_AeroData.c:109-1861: `_Cx(alpha,beta,el)`,
 * `_CXq(alpha)`, ... each a lazy file read + interpn(), C/mexndinterp.c:97-265) evaluated on the device by the bracket /
 * interpolation helpers the dynamics kernels use, at n query points given on the HOST (degrees, as the reference's
 * functions take them; beta / el ignored by tables without that axis).  tid = enum f16_table_id
 * (csrc/f16_tables_data.inc: 0 Cx, 1 Cz, 2 Cm, 3 Cn, 4 Cl, 5 Cy, 6-8 r30, 9-11 a20, 12-17 lef, 18-20 a20_lef, 21-29 damping,
 * 30-32 brett, 33-41 lef damping, 42 eta_el).  h_status (may be NULL) receives the F16_ST_* grid-clamp bits. */
int f16_debug_table_lookup(f16_ctx *ctx, int tid, const double *h_alpha, const double *h_beta, const double *h_el,
                           int n, double *h_out, int32_t *h_status);

/* Tests: the branch-free sin/cos pair of the default build in its two forms on n arguments given on the HOST -- constants as
 * literals (every kernel but one) and the same table in scalar registers (the four-lane rollout at B <= 4096).
 * h_out [4][n]: sin, cos of the first form, sin, cos of the second.  The two agree bit for bit.  F16_EINVAL from a library
 * built without F16_FAST_TRIG (one form only: libm). */
int f16_debug_sincos(f16_ctx *ctx, const double *h_x, long n, double *h_out);
/* Tests: the atmosphere's exp(0.14 log tfac), tfac = 1 - 0.703e-5 alt, at n altitudes [ft] given on the HOST, composed from the
 * device library's exp and log (every kernel but one) and by the restatement of the same operation sequence with its constants
 * in scalar registers (the four-lane rollout at B <= 4096).  h_out [6][n]: the factor, qbar and ps (at 500 ft/s) of the first
 * form, then of the second.  The two agree bit for bit.  F16_EINVAL from a library built without F16_FAST_POW. */
int f16_debug_pow(f16_ctx *ctx, const double *h_alt, long n, double *h_out);

/* Tests (tests/test_gpu_elem.py): each elementary function of the default build on its own, on n arguments given on the HOST, for
 * the comparison with a multiprecision reference.  All are synchronous, accept n == 0, and return F16_EINVAL from a library built
 * without the F16_FAST_* form they expose.
 *   f16_debug_elem_sincos      the branch-free sin/cos pair in its THREE forms: constants as literals, the table in scalar registers,
 *                              the table in vector registers (the quad rollout's alpha / beta role).  h_out [6][n]: sin, cos of each.
 *                              Domain of the pair: within 1.3 ulp of the true value for |x| <= 1e6 rad (held by the tests at the C
 *                              library's own error + 2 ulp) and, measured, within 1.1 ulp up to 3.3e9; from |x| >= 2^31 pi/2
 *                              (3.37e9 rad) the quadrant is taken from a saturated integer and the result is a finite number in
 *                              [-1, 1] that has nothing to do with the argument.  No status bit reports it: phi, theta and psi have
 *                              no envelope limit, and the caller keeps them in range.  NaN for a NaN or infinite argument.
 *   f16_debug_elem_trig_carry  the pairs the rollouts carry from step to step: h_angle_and_steps [1 + n_steps][n] = a start angle per
 *                              lane, then one increment per step and lane.  Full evaluation at the start angle, then per step
 *                              angle += increment and one trig_advance (rotation by the increment taken back from the stored
 *                              angle).  h_out [n_steps][4][n]: sin, cos, the stored angle, and trig_advance's verdict (1.0: the
 *                              increment left the series' range |d| <= 4e-3, the caller re-evaluates) after every step.  The
 *                              lane's other four angles stay 0, so a NaN increment gives the verdict 0.0: fmax drops a NaN beside a
 *                              number.  1 <= n_steps <= 4096.
 *   f16_debug_elem_atmos       h_alt_vt [2][n] = altitude [ft], airspeed [ft/s] (used as given: no 0.01 floor).  h_out [13][n]:
 *                              tfac; then the factor exp(0.14 log tfac), mach, qbar, ps by the device library's exp / log
 *                              (atmos_dev), by their restatement with the table in scalar registers (atmos_dev_k), and by the same
 *                              with the table in vector registers.  The three routes agree bit for bit.
 *   f16_debug_elem_rcp         h_out [n] = f16_rcp(x): the hardware reciprocal and two Newton steps, <= 1 ulp of 1/x for every normal
 *                              finite x (NaN for 0, denormals and infinities).
 *   f16_debug_elem_tan         h_out [3][n] = sin theta, cos theta, and tan theta as the plant forms it: sin theta * f16_rcp(cos theta). */
int f16_debug_elem_sincos(f16_ctx *ctx, const double *h_x, long n, double *h_out);
int f16_debug_elem_trig_carry(f16_ctx *ctx, const double *h_angle_and_steps, int n_steps, long n, double *h_out);
int f16_debug_elem_atmos(f16_ctx *ctx, const double *h_alt_vt, long n, double *h_out);
int f16_debug_elem_rcp(f16_ctx *ctx, const double *h_x, long n, double *h_out);
int f16_debug_elem_tan(f16_ctx *ctx, const double *h_theta, long n, double *h_out);
/* Tests (tests/test_gpu_air.py): the air triple of the plant in moving air (the rule under "STEADY WIND" below; csrc/f16_wind.hpp
 * air_triple, the function calc_xdot_wind evaluates in front of its lookups) on its own, on n cases given on the HOST, for the
 * comparison with a multiprecision reference.  h_in [12][n] = phi theta psi vt alpha beta (x[3..8]), then wN wE wD, then g_x g_y g_z;
 * h_out [6][n] = Ua Va Wa vt_a alpha_a beta_a.  Synchronous; n == 0 is a no-op; every build has it. */
int f16_debug_air_triple(f16_ctx *ctx, const double *h_in, long n, double *h_out);

/* ---- (1) drop-in symbols of the reference .so ---------------------------------------------- */
/* replaces C/nlplant.c:23  void Nlplant(double *xu, double *xdot, int fidelity)
 * host pointers; reads xu[0..16], writes xdot[0..17]; runs ONE aircraft on the GPU. */
void Nlplant(double *xu, double *xdot, int fidelity);
/* replaces C/nlplant.c:467 void atmos(double alt, double vt, double *coeff) -> coeff[0..2]=mach,qbar,ps */
void atmos(double alt, double vt, double *coeff);
/* replaces the choice between nlplant_xcg25.so / nlplant_xcg35.so (parameters.py:108-111) for the two
 * symbols above; default 0.25.  flags as F16_FLAG_*. */
void f16_dropin_config(double xcg, unsigned flags);

/* ---- (2) batched dynamics --------------------------------------------------------------- */
/* env.py:65-103 _calc_xdot for B aircraft: xdot[18][ld] = f(x[18][ld], u[4][ld]). status may be NULL. */
int f16_xdot_batch(f16_ctx *ctx, const double *x, const double *u, double *xdot, int32_t *status,
                   long B, long ld, double xcg, int fi_flag, unsigned flags, void *stream);
/* C/nlplant.c:23-457 Nlplant itself (no actuator models, outputs 12..17 = nx,ny,nz,mach,qbar,ps). */
int f16_nlplant_batch(f16_ctx *ctx, const double *xu, double *xdot, int32_t *status,
                      long B, long ld, double xcg, int fi_flag, unsigned flags, void *stream);
/* env.py:105-130 step, in place: envelope check, x += xdot*dt.  nsteps Euler steps per launch with the
 * state held in registers; traj (may be NULL) receives the state after every `traj_every`-th step as
 * [nsteps/traj_every][18][ld].
 * Split launches: rollout(n) followed by rollout(m) equals rollout(n + m) BIT FOR BIT for B <= 16,384 (the kernels of that
 * range evaluate every sine / cosine from scratch) and, for larger batches, whenever n is a multiple of 32: the one-lane
 * kernels of the large-batch range carry the five sin / cos pairs of a step to the next one by the exact increment of their
 * angles and re-evaluate them exactly at steps 0, 32, 64, ... of the LAUNCH (default build; -DF16_NO_INC_TRIG switches it off), so
 * a split at another step re-evaluates at other steps: the two results then differ by the rounding of the carried pairs, <= 1e-12
 * relative over 100 steps (tests/test_gpu_dynamics.py::test_split_launches_*).  For the same reason an aircraft's last bits
 * depend on which kernel its batch size selects; F16_FLAG_ONE_LANE pins the kernel (not the carried pairs). */
int f16_rollout(f16_ctx *ctx, double *x, const double *u, double *traj, int32_t *status,
                long B, long ld, int nsteps, int traj_every, double dt, double xcg, int fi_flag,
                unsigned flags, void *stream);
/* The reference's closed loop under its LQR controller (the only controller its drivers actually run: flight_sim.py:139,181;
 * nonlinear loop test_env_mk2.py:70-85) as ONE launch: per step the action of env.py:360-371
 *     u[1:4] = -K (x_ref - x9) + u0[1:4],   x9 = x[mpc idx] (parameters.py:135), x_ref = x9 with x_ref[4:7] = (p, q, r)_dem
 * from the state at the start of the step, the thrust command u0[0] held (test_env_mk2.py:79 overwrites u.values[1:] only),
 * then env.py:105-130 step -- inside the same kernels f16_rollout launches, the state in registers for all nsteps.
 * K[27][ld]: the gain as the reference holds it (`_calc_LQR_gain` returns K = -dlqr; 3 x 9 row-major: f16_lqr_batch's output);
 * dem[3][ld]; u0[4][ld] = u.initial_condition.  x in place; traj as in f16_rollout; u_out (may be NULL) [4][ld] receives the
 * action of the last step (what self.u.values holds after the loop).  (x_ref - x9 is exactly zero outside the three rate
 * entries, so only K[:, 4:7] enters the product.) */
int f16_rollout_lqr(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem, double *traj,
                    double *u_out, int32_t *status, long B, long ld, int nsteps, int traj_every, double dt, double xcg,
                    int fi_flag, unsigned flags, void *stream);
/* f16_rollout / f16_rollout_lqr under an INPUT SCHEDULE, as ONE launch: the reference's caller hands step() a new action at every
 * step (env.py:105-130; the doublets of Nguyen_m/runF16Sim.m; the pilot demands of flight_sim.py:141-182), which with a constant
 * input per launch costs one launch and one row copy per input change.
 *   f16_rollout_sched      u_seq[S][4][ld]   the four commands;
 *   f16_rollout_lqr_sched  dem_seq[S][3][ld] the (p, q, r) demands -- the thrust command stays u0[0], K and u0 are constant;
 * S = ceil(nsteps / hold) rows in the state-major layout of every other argument.  Step t of the launch uses row t / hold: a
 * zero-order hold whose last segment may be shorter.  hold >= 1; hold = 1 is a new input at every step, hold >= nsteps reads row 0
 * only.  Everything else as in f16_rollout / f16_rollout_lqr: x in place, traj and traj_every (independent of hold), envelope freeze
 * (a frozen aircraft ignores the rest of its schedule), sticky status bits, F16_FLAG_*, u_out; NaN / infinite commands go through
 * the actuator models as a constant one does.  F16_EINVAL where f16_rollout returns it, and for hold < 1 or a NULL u_seq / dem_seq.
 * Contract: the result -- final state, status, every stored sample, u_out -- equals the chain of f16_rollout (f16_rollout_lqr)
 * calls, one per segment with that segment's row, BIT FOR BIT wherever f16_rollout's split-launch guarantee holds: any hold for
 * B <= 16,384 (the lofi kernel of that range, which does carry its sin / cos pairs, restarts them with every row as the chain's
 * launches do); any hold under F16_FLAG_ONE_LANE; hold % 32 == 0 beyond that (the carried pairs are re-evaluated at steps 0, 32,
 * ... of the launch, which are then the same steps as in the chain).  Other holds on the large-batch kernels agree with the chain
 * to the 1e-12 relative over 100 steps stated above for split launches.  S identical rows give f16_rollout's own bits for any hold
 * (in that lofi kernel: for hold % 32 == 0, else the chain's).  A schedule cut into two calls at a segment boundary equals
 * one call under the same conditions.  The launch rules are f16_rollout's: every kernel has a scheduled twin, so a schedule never
 * moves a batch to another kernel.  The next row is loaded a step or more before its first use; with hold = 1 that is
 * 32 B (24 B) of reads per aircraft-step beside the 144 B a stored step writes.  Nothing is allocated: the calls can be captured
 * into a graph. */
int f16_rollout_sched(f16_ctx *ctx, double *x, const double *u_seq, double *traj, int32_t *status, long B, long ld, int nsteps,
                      int hold, int traj_every, double dt, double xcg, int fi_flag, unsigned flags, void *stream);
int f16_rollout_lqr_sched(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem_seq, double *traj,
                          double *u_out, int32_t *status, long B, long ld, int nsteps, int hold, int traj_every, double dt,
                          double xcg, int fi_flag, unsigned flags, void *stream);
/* SCORED rollouts under sampled command schedules, as ONE launch: the engine of a sampling-based nonlinear MPC (MPPI, model-predictive
 * path integral control) and of any Monte-Carlo study that wants one number per trajectory.  K = B / B0 perturbed command sequences
 * per aircraft go through the nonlinear plant; each lane accumulates its trajectory cost in registers, so neither [T][18][B] samples
 * nor K copies of the initial state are ever stored.
 *   Lanes: lane j (0 <= j < B) is sample j / B0 of aircraft j % B0 and starts from column j % B0 of x0[18][ld0], which is only read.
 *     B0 == B is an ordinary scored rollout.
 *   u_seq[S][4][ld], S = ceil(nsteps / hold): layout and zero-order hold exactly as in f16_rollout_sched (step t uses row t / hold).
 *   x_ref[9][ld0]: one reference per aircraft in MPC-state order (parameters.py:135: phi theta alpha beta p q r lf1 lf2);
 *     u_ref[3][ld0] (may be NULL = 0): reference of the three surface commands.
 *   h_w (host): diagonal weights, every entry finite and >= 0.
 *   cost[ld] (required):
 *       J = sum over the steps t = 0..nsteps-1 the lane TAKES of
 *               [ sum_i r[i] (u_t[1+i] - u_ref[i])^2  +  sum_k q[k] (x9_{t+1}[k] - x_ref[k])^2 ]
 *         + pen * (number of steps the lane does not take because the envelope check has frozen it)
 *         + sum_k qf[k] (x9_end[k] - x_ref[k])^2
 *     with x9_{t+1} the MPC states after step t and u_t the row in use at step t, accumulated in fp64 in step order (the command term
 *     is formed once per row).  The thrust command is not penalised: no controller of the reference commands it.  A non-finite state
 *     or command makes J non-finite by ordinary arithmetic.  nsteps == 0 reads no row and writes the terminal term of x0 alone
 *     (x_end = x0, status = F16_ST_NONFINITE or 0).
 *   x_end[18][ld] (may be NULL): the final state of every lane.  traj (may be NULL), traj_every: as in f16_rollout_sched, over the B lanes.
 *   status[ld] (may be NULL) is an OUTPUT: every lane starts from 0, it is not sticky -- the one deliberate difference from the
 *     siblings (K samples of one aircraft have no status column to start from).
 * Everything else follows f16_rollout_sched: envelope freeze and F16_FLAG_NO_ENVELOPE (then no penalty is ever added), the status bits
 * including F16_ST_ENV_STATE and F16_ST_NONFINITE, NaN / infinite commands through the actuator models.
 * F16_EINVAL: NULL x0 / u_seq / x_ref / h_w / cost, hold < 1, nsteps < 0, ld < B, ld0 < B0, B0 < 1 while B > 0, B % B0 != 0, traj with
 * traj_every < 1 or nsteps % traj_every != 0, a negative or non-finite weight.  B == 0 is a no-op.
 * Kernels: F16_FLAG_ONE_LANE selects the one-kernel-for-every-size path; otherwise the one-lane-per-aircraft kernels of f16_rollout's
 * launch rules by the number of LANES B (64 / 128 / 256 / 512 lanes per workgroup, the integer table image at 512 in the default
 * build).  The states (x_end, traj, status) then equal f16_rollout_sched's on the K-fold replicated initial states BIT FOR BIT
 * wherever both run the same kernel: every lofi size, hifi above 16,384 lanes, and F16_FLAG_ONE_LANE.  The four-lanes-per-aircraft and
 * four-wavefront kernels that f16_rollout_sched runs for hifi batches of at most 16,384 have no scored twin (their state is split
 * over four role waves), so BELOW 16,385 LANES THE SCORED ENTRY RUNS A DIFFERENT, SLOWER KERNEL than f16_rollout_sched (the 64-lane
 * one-lane kernel: same terms, ulp-level differences); scoring on the split kernels is a possible follow-up.  cost has the same bits
 * whether or not x_end / traj are given.  Nothing is allocated and the weights travel in the kernel argument block: the call can be
 * captured into a graph. */
typedef struct f16_cost_weights { double q[9], qf[9], r[3], pen; } f16_cost_weights;   /* host; all entries >= 0 and finite */
int f16_rollout_cost(f16_ctx *ctx, const double *x0, long B0, long ld0, const double *u_seq,
                     const double *x_ref, const double *u_ref, const f16_cost_weights *h_w,
                     double *cost, double *x_end, double *traj, int32_t *status,
                     long B, long ld, int nsteps, int hold, int traj_every,
                     double dt, double xcg, int fi_flag, unsigned flags, void *stream);
/* The three scheduled rollouts above with the STEP RULE as an argument: explicit Euler (the reference's step, env.py:126) or the
 * classical fourth-order Runge-Kutta step, still ONE launch.  Euler at the reference's dt = 1 ms reproduces the reference; at 10 ms it
 * is outside the tolerance of the reference's Simulink time histories (fixture G10), where RK4 at 10 ms is inside it with 0.4 x the
 * plant evaluations per simulated second.
 *   method = F16_INT_EULER  forwards to f16_rollout_sched / f16_rollout_lqr_sched / f16_rollout_cost: that call's kernel, its bits.
 *   method = F16_INT_RK4    with f = env.py:65-103 `_calc_xdot` (all 18 states, the actuator and leading-edge-flap models inside)
 *     and u the command of the step -- under the LQR law the action of env.py:360-371 formed from the state at the START of the step
 *     -- held over the four stages:
 *         if the box test of env.py:117-124 fails on x: the aircraft is frozen (F16_ST_ENVELOPE), x untouched; else
 *         k1 = f(x, u)   k2 = f(x + (dt/2) k1, u)   k3 = f(x + (dt/2) k2, u)   k4 = f(x + dt k3, u)
 *         x <- x + (dt/6) ((k1 + 2 k2) + (2 k3 + k4))
 *     The grid bits (F16_ST_ALPHA1 .. F16_ST_EL) of all four evaluations are ORed into the sticky status word; the stage states are
 *     not box-tested; NaN and infinite commands or states propagate by ordinary arithmetic; F16_ST_NONFINITE and F16_ST_ENV_STATE
 *     are formed at write-back; trajectory samples, u_out and the scored cost (f16_rollout_cost's formula, unchanged) use the state
 *     after the whole step.
 *   Any other method: F16_EINVAL ("method must be ...").
 * Arguments, layouts, the zero-order hold, the no-op rules and the F16_EINVAL rules are those of the call each stands for, checked
 * in the same order, the method last.  A constant input is one row with hold >= nsteps.
 * Contracts (RK4).  Nothing but the state is carried from step to step (every stage evaluates its sin / cos pairs exactly), so a
 * rollout of n steps followed by one of m steps equals one of n + m steps BIT FOR BIT, and a schedule equals the chain of one call
 * per segment bit for bit, for EVERY batch size and EVERY hold -- a stronger statement than the Euler kernels make.  Under
 * F16_FLAG_ONE_LANE every variant steps through one out-of-line function, so an aircraft's result does not depend on the batch
 * size.  f16_rollout_cost_rk's x_end / traj / status equal f16_rollout_rk's on the K-fold replicated states bit for bit at every
 * size (both run the same kernel family); cost has the same bits with and without x_end / traj.
 * Launch rules (RK4): the one-lane-per-aircraft kernels at every size, 64 / 128 / 256 lanes per workgroup -- never the
 * four-lanes-per-aircraft and four-wavefront kernels, and never 512-lane workgroups (the step's registers do not fit there).
 * OUT OF SCOPE: an RK4 twin of those role-wave kernels.  For hifi batches of at most 16,384 aircraft the Euler call at dt = 1 ms on
 * them remains the fastest way to fly a second of simulated time; RK4 pays where the one-lane kernels run anyway (scored rollouts,
 * batches above 16,384) and wherever a coarser step is wanted.  The closed MPC loops and the per-step re-linearised LQR loop keep
 * the Euler step.  Nothing is allocated: the calls can be captured into a graph. */
#define F16_INT_EULER 1
#define F16_INT_RK4 4
int f16_rollout_rk(f16_ctx *ctx, double *x, const double *u_seq, double *traj, int32_t *status, long B, long ld, int nsteps,
                   int hold, int traj_every, double dt, double xcg, int fi_flag, int method, unsigned flags, void *stream);
int f16_rollout_lqr_rk(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem_seq, double *traj,
                       double *u_out, int32_t *status, long B, long ld, int nsteps, int hold, int traj_every, double dt,
                       double xcg, int fi_flag, int method, unsigned flags, void *stream);
int f16_rollout_cost_rk(f16_ctx *ctx, const double *x0, long B0, long ld0, const double *u_seq,
                        const double *x_ref, const double *u_ref, const f16_cost_weights *h_w,
                        double *cost, double *x_end, double *traj, int32_t *status,
                        long B, long ld, int nsteps, int hold, int traj_every,
                        double dt, double xcg, int fi_flag, int method, unsigned flags, void *stream);
/* The LQR loop under a GAIN SCHEDULE over (altitude, airspeed), as ONE launch: between the frozen gain of f16_rollout_lqr*
 * (valid near the trim point it was derived at) and the gain re-derived at every step (f16_rollout_lqr_relin: linearise -> ZOH ->
 * DARE per step) stands flight-control practice -- a gain table derived once over a grid of flight conditions (one batch through
 * f16_trim_batch -> f16_linearise_batch -> f16_c2d_batch -> f16_lqr_batch_w, one aircraft per node) and interpolated on the measured
 * altitude and airspeed while flying.
 *   The table.  tab[nh][nv][F16_GS_ENTRIES] doubles, row-major, node (ih, iv) at (ih * nv + iv) * 12 + e, on the uniform grid
 *     h0 + ih dh, v0 + iv dv (nh, nv >= 2; dh, dv > 0).  Entry 3 i + j = K[i][4 + j], K as the reference holds it (K = -dlqr,
 *     f16_lqr_batch's output; the law reads nothing else of K); entry 9 + i = the trim surface command u_trim[1 + i].
 *   The lookup rule, for altitude h = x[2] and airspeed V = x[6]:
 *         th = (h - h0) / dh;   ih = (int) fmin(fmax(floor(th), 0), nh - 2);   lh = fmin(fmax(th - ih, 0), 1)
 *         tv, iv, lv            the same from V, v0, dv, nv
 *         a = G[ih][iv][e]   + lv * (G[ih][iv+1][e]   - G[ih][iv][e])
 *         b = G[ih+1][iv][e] + lv * (G[ih+1][iv+1][e] - G[ih+1][iv][e])
 *         g[e] = a + lh * (b - a)
 *     where a lerp p + l * (q - p) with l = 1 (the last node of an axis and everything beyond it) takes q itself -- p + (q - p) need
 *     not round to q, and the properties below are meant to hold at that edge too;
 *     every operation rounded on its own (IEEE division, no FMA contraction), so the host function, the device and the numpy
 *     restatement (f16_mpc_oop_py_amd/schedule.py GainSchedule.lookup) give the same bits.  Outside the grid the edge cell is
 *     extended flat: a clamp, NOT an extrapolation.  A NaN coordinate takes index 0 with weight 0 (fmax(NaN, 0) = 0).  At a node the
 *     node's values come back exactly; a table of equal nodes returns them exactly.  The rule is written once
 *     (csrc/f16_gain_sched.hpp) for the three users: the rollout kernels, f16_gain_lookup_host (pure host code: no context, no
 *     GPU; h_tab on the host) and f16_debug_gain_lookup (tests: DEVICE table, n points and n x 12 results on the HOST; synchronous).
 *   f16_rollout_lqr_gs is f16_rollout_lqr_rk with the per-aircraft K replaced by the schedule:
 *     at every step t with t % gs_every == 0 the 12 values g are looked up at the state at the START of that step -- for frozen
 *     aircraft too, at their frozen state -- and held until the next update; until then the law of env.py:360-371 runs with
 *     K[i][4..6] = g[3 i .. 3 i + 2] and the offset u0[1 + i] = g[9 + i].  The thrust command u0[0][b] is held throughout (the
 *     reference's LQR never commands thrust).
 *     u0[4][ld]: row 0 is the thrust command; ROWS 1..3 ARE NOT READ -- the offset comes from the schedule.
 *     h_grid: HOST, travels by value in the kernel argument block; tab: DEVICE, read through L2 (at 32 x 32 nodes 98 KB).
 *     gs_out[ld] (may be NULL): the number of gain updates of this call at which (h, V) lay outside
 *     [h0, h0 + (nh-1) dh] x [v0, v0 + (nv-1) dv] (th < 0 or th > nh - 1, likewise tv) or was not finite.  The loop does not stop
 *     there and no status bit is set: the count is how a caller learns that the schedule was left.
 *     Everything else is f16_rollout_lqr_rk's: dem_seq, hold, traj, traj_every, the envelope freeze, the sticky status bits, the
 *     flags, method = F16_INT_EULER or F16_INT_RK4 (the action held over the four stages), the NaN rules.  Nothing is allocated:
 *     the call can be captured into a graph.
 *   F16_EINVAL, in the order of the call it extends: everything f16_rollout_lqr_rk refuses but the method (its "K / dem_seq is NULL"
 *     reads "dem_seq is NULL"); a NULL h_grid or tab; nh < 2 or nv < 2; a non-finite or non-positive dh or dv, a non-finite h0 or v0;
 *     gs_every < 1; the method last.  B == 0 (and nsteps == 0) is a no-op.
 *   Contract (the chain).  Split the steps wherever t % gs_every == 0 or t % hold == 0.  The call equals the chain of
 *     f16_rollout_lqr_rk calls, one per segment, each with that segment's demand row and with K and u0 = [thrust, g[9..11]] from the
 *     most recent gain update as f16_gain_lookup_host computes it from the chain's own state, BIT FOR BIT in the final state, the
 *     status, every stored sample and u_out (what the chain's last call reports): under F16_FLAG_ONE_LANE for both methods and every
 *     B; with F16_INT_RK4 at every size and any segmentation; for lofi at every size and for hifi above 16,384 aircraft with Euler
 *     when every segment length is a multiple of 32 (the Euler kernels that carry their sin / cos pairs restart them at every
 *     segment start, as the chain's launches do).  A table of identical nodes gives f16_rollout_lqr_rk's own bits wherever both run
 *     the same kernel and restart their carried pairs at the same steps (RK4 and F16_FLAG_ONE_LANE: always).  gs_every >= nsteps is
 *     one update at step 0; n steps followed by m steps equal n + m steps where n % gs_every == 0 and n % hold == 0, under the
 *     conditions of the chain.
 *   Launch rules: the one-lane-per-aircraft kernels at every size (64 / 128 / 256 lanes per workgroup, 512 on the integer table
 *     image; RK4: at most 256), the single kernel of F16_FLAG_ONE_LANE under the flag -- f16_rollout_lqr_rk's rules without the
 *     four-lanes-per-aircraft and four-wavefront branches.  For hifi batches of at most 16,384 aircraft this is a different, slower
 *     kernel than the one f16_rollout_lqr runs (same terms, ulp-level differences).
 *   OUT OF SCOPE: a scheduled-gain twin of those role-wave kernels; a schedule on anything other than (h, V); scheduled thrust;
 *     extrapolation beyond the grid. */
#define F16_GS_ENTRIES 12
typedef struct f16_gain_grid { double h0, dh, v0, dv; int nh, nv; } f16_gain_grid;   /* host; uniform grid, nh, nv >= 2, dh, dv > 0 and finite */
int f16_gain_lookup_host(const f16_gain_grid *g, const double *h_tab, double h, double v, double *h_out12);
int f16_debug_gain_lookup(f16_ctx *ctx, const f16_gain_grid *g, const double *tab, const double *h_h, const double *h_v, long n,
                          double *h_out);
int f16_rollout_lqr_gs(f16_ctx *ctx, double *x, const double *u0, const f16_gain_grid *h_grid, const double *tab, int gs_every,
                       const double *dem_seq, double *traj, double *u_out, int32_t *gs_out, int32_t *status, long B, long ld,
                       int nsteps, int hold, int traj_every, double dt, double xcg, int fi_flag, int method, unsigned flags,
                       void *stream);
/* The softmin blend of an MPPI step over the costs f16_rollout_cost wrote.  For aircraft a and its samples k = 0..K-1 (K = B / B0) at
 * lanes k * B0 + a:  m = the minimum over the FINITE cost,  w_k = exp(-(J_k - m) / lambda) for finite J_k and 0 otherwise,
 *     u_blend[nrows][4][ld0] = sum_k w_k u_seq[row][c][k * B0 + a] / sum_k w_k        (all four commands; u_seq[nrows][4][ld])
 * summed over k ascending in plain fp64, so the result does not depend on the launch geometry.  An aircraft without any finite cost
 * gets sample 0's rows.  w_out[ld] (may be NULL): the normalised weights (0 everywhere for such an aircraft); stats[2][ld0] (may be
 * NULL): m and the effective sample size (sum w)^2 / sum w^2, both 0 when no cost is finite.
 * F16_EINVAL: lambda <= 0 or not finite, NULL cost / u_seq / u_blend, B0 < 1 while B > 0, B % B0 != 0, ld < B, ld0 < B0, nrows < 0.
 * B == 0 is a no-op; nrows == 0 writes w_out / stats only.  Nothing is allocated. */
int f16_mppi_blend(f16_ctx *ctx, const double *cost, const double *u_seq, double lambda,
                   double *u_blend, double *w_out, double *stats,
                   long B, long ld, long B0, long ld0, int nrows, void *stream);
/* The SAMPLER of an MPPI step, defined by this library (not by a tensor library's generator): Philox4x32-10 plus Box-Muller.
 *   Words.   (r0, r1, r2, r3) = Philox4x32-10(counter, key), counter = (period, row, sample k, aircraft a), each a uint32,
 *     key = (seed & 0xffffffff, seed >> 32).  The round function is the published one (Salmon, Moraes, Dror, Shaw, SC'11): per round
 *         (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0)),   M0 = 0xD2511F53, M1 = 0xCD9E8D57
 *     (hi / lo: the halves of the 64-bit product), ten rounds, the key bumped by (0x9E3779B9, 0xBB67AE85) after each.  Known answers:
 *         counter 00000000 x4, key 00000000 x2                               -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *         counter ffffffff x4, key ffffffff x2                               -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *         counter 243f6a88 85a308d3 13198a2e 03707344, key a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
 *   Normals. U_i = (r_i + 0.5) * 2^-32 (never 0 or 1, so |n| <= 6.8);  n0 = sqrt(-2 ln U0) cos(2 pi U1),  n1 = sqrt(-2 ln U0) sin(2 pi U1),
 *     n2 = sqrt(-2 ln U2) cos(2 pi U3): elevator, aileron, rudder in that order.
 *   Sample.  Lane j = k * B0 + a, row s:  u_seq[s][0][j] = u_nom[s][0][a] (the thrust command is never perturbed),
 *     u_seq[s][1 + i][j] = clip(u_nom[s][1 + i][a] + sigma[i] n_i, lo_i, hi_i) with the command limits of parameters.py:125-126
 *     (+-25, +-21.5, +-30 deg) and np.clip's behaviour: a NaN nominal stays NaN.
 * f16_mppi_sample writes rows 0..nrows-1 for counter word `period`: u_nom[nrows][4][ld0], u_seq[nrows][4][ld], B = K * B0 lanes;
 * h_sigma: 3 values on the HOST, finite and >= 0.  F16_EINVAL: a NULL pointer, a bad sigma, B < 0, ld < B, nrows < 0, B0 < 1 while
 * B > 0, B % B0 != 0, ld0 < B0.  B == 0 or nrows == 0 is a no-op.  Nothing is allocated.  f16_mpc_oop_py_amd/mppi.py
 * `sample_reference` restates the rule in numpy.  The lane's row comes from ONE out-of-line device function, which the fused loop
 * below calls too.
 * f16_debug_philox (tests): the generator alone on n (counter, key) pairs given on the HOST -> h_out[n][4]; synchronous. */
int f16_mppi_sample(f16_ctx *ctx, const double *u_nom, const double *h_sigma, uint64_t seed, uint32_t period, double *u_seq,
                    long B, long ld, long B0, long ld0, int nrows, void *stream);
int f16_debug_philox(f16_ctx *ctx, const uint32_t *h_ctr, const uint32_t *h_key, long n, uint32_t *h_out);
/* The CLOSED MPPI LOOP with in-kernel sampling as ONE launch.  Per aircraft a and control period p = period0 .. period0 + nperiods - 1:
 *   1. x_ref = the current x9 with entries 4..6 = dem (the convention of calc_MPPI_action);
 *   2. the K sample rows u_seq[S][4][ld] by f16_mppi_sample's rule from u_nom, counter word period = p;
 *   3. every sample scored over S * hold steps from the current state: f16_rollout_cost's formula, step rule, envelope freeze,
 *      penalty and NaN behaviour (method F16_INT_RK4: f16_rollout_cost_rk's) -> cost[ld];
 *   4. the blend by f16_mppi_blend's rule (minimum over the finite costs, k ascending in plain fp64, sample 0 when no cost is finite);
 *   5. u[4][ld0] = row 0 of the blend;
 *   6. the aircraft advances `hold` steps under u by f16_rollout's rules (f16_rollout_rk's): x[18][ld0] in place, the sticky
 *      status[ld0] (may be NULL), traj (may be NULL) [nperiods * hold / traj_every][18][ld0] with hold % traj_every == 0;
 *   7. u_nom[S][4][ld0] = the blend shifted by one row, its last row repeated.
 * u_seq / cost are work buffers in the host loop's layout (lane k * B0 + a) and hold the LAST period's samples and costs on
 * return; stats (may be NULL) [nperiods][2][ld0]: the minimum cost and the effective sample size of every period (f16_mppi_blend's).
 * u_ref [3][ld0] may be NULL (= 0).  h_w, h_sigma: HOST.
 * Mapping: one workgroup per aircraft, drawn grid-stride over B0; its lanes are the aircraft's K samples, 1 <= K <= 256, rounded up
 * to 64, 128 or 256 lanes.  The table image is staged into LDS once per launch; sampling, scoring, blend, advance and shift are
 * separated by workgroup barriers only: no waiting between workgroups, no counters.  The advance runs on one lane.
 * Contracts.
 *   Host-loop equality: under F16_FLAG_ONE_LANE the call equals the host loop  f16_mppi_sample -> f16_rollout_cost(_rk) ->
 *     f16_mppi_blend -> u = row 0 -> f16_rollout(_rk) -> shift,  one round per period with the same flags, BIT FOR BIT, for both
 *     integrators: x, u, u_nom, status, every traj sample, stats, and the last period's u_seq / cost.
 *   Split calls: under that flag n periods followed by m periods with period0 + n equal n + m periods bit for bit; with
 *     F16_INT_RK4 at every setting (nothing but the state is carried from step to step).
 *   Batch independence: under that flag an aircraft's result does not depend on B0.
 *   Default flags: the scoring runs the lane body of the 64 / 128 / 256-lane scored kernel (table image in LDS); results agree with
 *     the flagged ones to the kernel-to-kernel band (1e-9 relative on the states; tests/test_gpu_mppi_loop.py).
 * F16_EINVAL: a NULL pointer among ctx, x, u, u_nom, dem, h_w, h_sigma, u_seq, cost; K < 1 or K > 256; B0 < 0, ld0 < B0, ld < K * B0;
 * S < 1, hold < 1, nperiods < 0; traj with traj_every < 1 or hold % traj_every != 0; lambda not finite or <= 0; a negative or
 * non-finite sigma or weight; a method other than F16_INT_EULER / F16_INT_RK4.  B0 == 0 or nperiods == 0 is a no-op.  Nothing is
 * allocated: the call can be captured into a graph.  K > 256 (several workgroups per aircraft) is out of scope. */
int f16_rollout_mppi(f16_ctx *ctx, double *x, double *u, double *u_nom, const double *dem, const double *u_ref,
                     const f16_cost_weights *h_w, const double *h_sigma, double lambda, uint64_t seed, uint32_t period0,
                     double *u_seq, double *cost, double *stats, double *traj, int32_t *status,
                     long B0, long ld0, long K, long ld, int nperiods, int S, int hold, int traj_every,
                     double dt, double xcg, int fi_flag, int method, unsigned flags, void *stream);
/* The plant in STEADY WIND and SAMPLED GUSTS: one derivative, the scheduled rollout and the LQR loop in moving air, each ONE launch.
 * The reference flies in still air only; the rule below is this library's (csrc/f16_wind.hpp), pinned by a numpy twin built on the
 * checker's still-air derivative (tests/wind_cases.py) and by physical invariants.
 *   Inputs per aircraft besides x[18] and u[4]:  w_ned[3] = the velocity of the air mass over the ground, north / east / down, ft/s
 *     (x[2] is altitude, positive UP: an updraft is a NEGATIVE w_ned[2]);  g_b[3] = a gust velocity in body axes (x forward, y right,
 *     z down), ft/s.
 *   The rule.  The states (V, alpha, beta) describe the velocity over the GROUND.  With the sin / cos pairs of phi, theta, psi:
 *         U, V, W      = vt ca cb,  vt sb,  vt sa cb                  (vt clamped at 0.01; the ground velocity in body axes)
 *         wb_x = ct cpsi wN + ct spsi wE - st wD
 *         wb_y = (sphi st cpsi - cphi spsi) wN + (sphi st spsi + cphi cpsi) wE + sphi ct wD
 *         wb_z = (cphi st cpsi + sphi spsi) wN + (cphi st spsi - sphi cpsi) wE + cphi ct wD
 *         Ua, Va, Wa   = U - wb_x - g_x,  V - wb_y - g_y,  W - wb_z - g_z
 *         vt_a = sqrt(Ua^2 + Va^2 + Wa^2);  alpha_a = atan2(Wa, Ua);  beta_a = asin(Va / vt_a)
 *     The AIR triple (vt_a, alpha_a, beta_a) feeds the table lookups and the coefficient build-up (C/nlplant.c:183-377), the
 *     atmosphere call (mach, qbar, ps) and the leading-edge-flap model (utils.py:289-306); the GROUND triple stays in the navigation
 *     equations, in the force equations (U, V, W, vt, cos beta and the three quotients of xdot[6..8], C/nlplant.c:383-405) and in the
 *     envelope box test of env.py:117-124.  The moment equations are unchanged: they see the air through qbar and the totals.  No
 *     derivative of the wind appears: the force equations on the ground velocity are those of a still-air aircraft at the air
 *     velocity plus -omega x (wb + g_b), which is the body-axis derivative of a wind that is constant over the ground.
 *     The grid bits F16_ST_ALPHA1 .. F16_ST_EL come from the lookups, so from the air triple.  The 0.01 clamp applies to vt_a where
 *     the still-air code applies it to vt.  vt_a == 0 gives NaN by ordinary arithmetic (F16_ST_NONFINITE at write-back); a NaN wind
 *     or gust component propagates the same way.  Where the flap model takes its V (utils.py:291) it takes the RAW vt_a, and clamps
 *     for itself.  The default build's sin / cos pair gives sin(-0.0) = +0.0 (its fused reduction adds the -0.0 to a +0.0 product), so an
 *     angle of -0.0 acts as +0.0; the one place the sign of that zero could show is the cut of atan2: flying backwards through the air
 *     (Ua < 0) with alpha = -0.0 and Wa otherwise exactly zero gives alpha_a = +pi where a libm sine gives -pi.
 *     Wind and gust are held over the four stages of a Runge-Kutta step, as the command is.
 *   f16_xdot_wind_batch: env.py:65-103 `_calc_xdot` under the rule.  wind[3][ld], gust[3][ld]: DEVICE, either may be NULL (= 0); both
 *     NULL forwards to f16_xdot_batch (that call's kernel, its bits).  F16_EINVAL as f16_xdot_batch.
 *   f16_rollout_wind is f16_rollout_rk, f16_rollout_lqr_wind is f16_rollout_lqr_rk under the rule (the controller reads the state,
 *     not the air data): same arguments, layouts, zero-order hold, envelope freeze, sticky status bits, samples, u_out, no-op rules,
 *     method = F16_INT_EULER or F16_INT_RK4.  h_wind: HOST, read during the call only:
 *         wind_ned   [3][ld] DEVICE or NULL (= 0): constant over the call
 *         gust_seq   [Sg][3][ld] DEVICE or NULL, Sg = ceil(nsteps / gust_hold): step t reads gust row t / gust_hold, independent of hold
 *         gust_hold  steps per gust row, >= 1 (read when gust_seq or ga is given)
 *         ga, gb     [3][ld] DEVICE or NULL: the gust rows are GENERATED in the kernel by f16_gust_sample's rule instead of read;
 *         gstate     [3][ld] DEVICE, in / out, with ga: the gust row before row0 on entry (zeros for a fresh sequence), the last
 *                    row of the call on return;  seed, row0: the key and the counter word of the call's first row.
 *     A NULL h_wind, or one whose pointers are all NULL, forwards to f16_rollout_rk / f16_rollout_lqr_rk: that call's kernel, its
 *     bits.  F16_EINVAL: what the sibling refuses, in its order, then: gust_seq and ga both given; ga, gb, gstate not all given or all
 *     NULL; gust_hold < 1 with gusts.  Nothing is allocated: the calls can be captured into a graph.
 *   The gust sampler.  Per body axis i a first-order Gauss-Markov process  g_i(r) = (a_i * g_i(r-1)) + (b_i * n_i(r)),  each
 *     operation rounded on its own (no FMA contraction), with (n_0, n_1, n_2) the three normals of f16_mppi_sample's rule from the
 *     Philox counter (row0 + r, 0, 0xFFFFFFFF, aircraft), key = (seed & 0xffffffff, seed >> 32).  Counter word 2 is a value MPPI's
 *     sample index never takes, so one seed serves both.  f16_mpc_oop_py_amd/wind.py `gust_reference` restates it in numpy.
 *     f16_gust_coeffs_host (pure host code, no context): a = exp(-v0 dt_row / L), b = sigma sqrt(1 - a^2) per axis -- the exact
 *     discretisation of the first-order Dryden form at a FROZEN nominal airspeed v0 (the sequence does not depend on the state): the
 *     stationary standard deviation is sigma for any row period dt_row = gust_hold * dt.  F16_EINVAL: a NULL pointer; v0, dt_row or
 *     a length not finite or <= 0; a sigma negative or not finite.
 *     f16_gust_sample writes rows row0 .. row0 + nrows - 1 into g_seq[nrows][3][ld] from gstate (the row before row0) and leaves the
 *     last row in gstate.  ga, gb, gstate, g_seq: DEVICE.  The lane's row comes from ONE out-of-line device function, which the rollout
 *     kernels call too when ga is given.  F16_EINVAL: a NULL pointer, B < 0, ld < B, nrows < 0.  B == 0 or nrows == 0 is a no-op.
 *   Contracts.  Nothing but the state and the gust row is carried from step to step (both step rules evaluate every sin / cos pair
 *     exactly), so for EVERY batch size, both methods, default flags and F16_FLAG_ONE_LANE: one call equals the chain of calls split
 *     at hold and gust_hold boundaries, BIT FOR BIT (final state, samples, status, u_out, gstate); n + m steps equal n steps then m
 *     steps where n is a multiple of hold and gust_hold; the in-kernel generation equals f16_gust_sample followed by the gust_seq
 *     call bit for bit; two generating calls with row0 continued equal one.  Under F16_FLAG_ONE_LANE an aircraft's result does not
 *     depend on the batch size.  Zero wind and gust are NOT the still-air bits (the air triple is recomputed through sqrt / atan2 /
 *     asin): they agree to rounding.  A frozen aircraft ignores the air; the generator advances for it all the same.
 *   Invariance.  Under a horizontal steady wind the air triple, attitude, rates, actuator states and altitude of the flight equal
 *     those of the still-air flight started from the air triple, and the position differs by w t, to rounding.
 *   Launch rules: one lane per aircraft, 64 / 128 / 256 lanes per workgroup, the fp64 table image in LDS; the single out-of-line-step
 *     kernel under F16_FLAG_ONE_LANE; never the four-lanes-per-aircraft, four-wavefront or 512-lane integer-image kernels.
 *   OUT OF SCOPE: wind in the scored, MPPI, gain-scheduled and MPC entries; the second-order Dryden lateral and vertical filters and
 *     gust angular rates; gust scale lengths that follow the state; role-wave twins; air-data outputs in traj. */
typedef struct f16_wind {
  const double *wind_ned;
  const double *gust_seq;
  int gust_hold;
  const double *ga, *gb;
  double *gstate;
  uint64_t seed;
  uint32_t row0;
} f16_wind;
int f16_xdot_wind_batch(f16_ctx *ctx, const double *x, const double *u, const double *wind, const double *gust, double *xdot,
                        int32_t *status, long B, long ld, double xcg, int fi_flag, unsigned flags, void *stream);
int f16_rollout_wind(f16_ctx *ctx, double *x, const double *u_seq, const f16_wind *h_wind, double *traj, int32_t *status, long B,
                     long ld, int nsteps, int hold, int traj_every, double dt, double xcg, int fi_flag, int method, unsigned flags,
                     void *stream);
int f16_rollout_lqr_wind(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem_seq, const f16_wind *h_wind,
                         double *traj, double *u_out, int32_t *status, long B, long ld, int nsteps, int hold, int traj_every,
                         double dt, double xcg, int fi_flag, int method, unsigned flags, void *stream);
int f16_gust_coeffs_host(const double *sigma, const double *length, double v0, double dt_row, double *a_out, double *b_out);
int f16_gust_sample(f16_ctx *ctx, const double *ga, const double *gb, double *gstate, uint64_t seed, uint32_t row0, double *g_seq,
                    int nrows, long B, long ld, void *stream);
/* ENSEMBLE STATISTICS of wind and gust rollouts inside the launch: per sample and per group of aircraft the count, mean, M2 (the sum
 * of squared deviations from the mean), minimum and maximum of each of the 18 states, formed in registers at the sample point, so
 * that a gust study stores [S][18][G] moments instead of [S][18][B] states.  The rule below is stated HERE ONCE; the device code
 * (csrc/f16_ensemble.hpp) and the numpy reference (f16_mpc_oop_py_amd/ensemble.py `ensemble_reference`) follow it operation for
 * operation, and the results are equal, not close.
 *   Groups.  Aircraft b belongs to group b / group; group is a multiple of 64, >= 64.  Any B >= 1: G = ceil(B / group), the last
 *     group may be short.  One wavefront covers the 64 consecutive aircraft from a multiple of 64 on.
 *   Who contributes.  At sample s an aircraft contributes (m = 1) iff all 18 values of its sample are finite AND, unless
 *     F16_FLAG_NO_ENVELOPE is set, the sample lies inside the box of env.py:117-124 (what freezes an aircraft) -- a pure function of
 *     the stored sample.  A frozen or NaN aircraft drops out and count shows the attrition.  Lanes beyond B have m = 0; the padding
 *     columns of the arrays are never read.
 *   Per wavefront, lanes l = 0..63, per state row k:   n_w = sum m_l;   s_w = tree(m_l ? x_l : 0.0);   mean_w = s_w / n_w;
 *     d_l = m_l ? x_l - mean_w : 0.0;   M2_w = tree(d_l * d_l), the product rounded before any add (no FMA contraction);
 *     min_w, max_w over the contributing lanes;  n_w = 0 gives the record (0, 0.0, 0.0, +inf, -inf).
 *     tree = the balanced tree over consecutive lanes, v = v[0::2] + v[1::2] six times (an xor-butterfly over 1, 2, 4, 8, 16, 32
 *     leaves the same bits on every lane).
 *   Per group.  The group's wave records folded in ascending aircraft order from (n, mean, M2) = (0, 0, 0): a wave with n_w = 0 is
 *     skipped, the first non-empty wave is taken as it is, after that, every operation rounded on its own,
 *         N = n + n_w;   delta = mean_w - mean;   mean = mean + delta * (n_w / N);
 *         M2 = (M2 + M2_w) + (delta * delta) * ((n * n_w) / N);   n = N
 *     min and max fold by fmin and fmax.  An empty group gives count 0, mean 0, M2 0, min +inf, max -inf.  The sign of a zero minimum
 *     or maximum is not specified (fmin / fmax of +0 and -0).
 *   f16_ens: HOST struct, DEVICE pointers.  work: f16_ens_work_doubles(B, S) doubles, S = the number of samples (the wave records:
 *     73 per wavefront and sample; contents unspecified after the call); group; ldg >= G; count [S][ldg]; mean, m2, min, max
 *     [S][18][ldg].  Entries g >= G are not written.  f16_ens_work_doubles is host code and needs no context.
 *   f16_rollout_wind_ens / f16_rollout_lqr_wind_ens: f16_rollout_wind / f16_rollout_lqr_wind with the statistics of the samples the
 *     call would store, S = nsteps / traj_every; traj_every >= 1 and nsteps % traj_every == 0 are required whether or not traj is
 *     given, and traj may be NULL (nothing but the statistics leaves the kernel).  Two launches on the stream: the rollout, whose
 *     wavefronts write their records at every sample point, and a finishing kernel, one lane per (sample, row, group).  Nothing is
 *     allocated: the calls can be captured into a graph.  A NULL h_wind, or one whose pointers are all NULL, is zero air THROUGH THE
 *     WIND KERNELS, not a forward to the still-air kernels: the bits are those of f16_rollout_wind with a zero wind_ned.
 *     Under F16_FLAG_ONE_LANE the final state, status, u_out, gstate and traj are those of the sibling call bit for bit (the step is
 *     out of line); under default flags they agree to rounding (an inlined step's contraction follows its surroundings).
 *     F16_EINVAL: what the sibling refuses, in its order; then nsteps % traj_every != 0 or traj_every < 1; a NULL h_ens or a NULL
 *     member; group < 64 or group % 64 != 0; ldg < G.  B == 0 or nsteps == 0 is a no-op.
 *   f16_ens_from_traj: the same statistic of a stored trajectory traj[nsamples][18][ld] through the same two device functions -- the
 *     samples of ANY rollout kernel reduce to the numbers the fused call gives for the same samples.  F16_EINVAL: a NULL ctx or
 *     traj, B < 0, ld < B, nsamples < 0; then the f16_ens rules above.  B == 0 or nsamples == 0 is a no-op.
 *   OUT OF SCOPE: twins of the still-air, role-wave, scored, gain-scheduled and MPC kernels (f16_ens_from_traj serves them); the
 *     plant's output rows; exceedance counts and histograms; groups that are not wave-aligned. */
long f16_ens_work_doubles(long B, int nsamples);
typedef struct f16_ens {
  double *work;
  long group, ldg;
  int32_t *count;
  double *mean, *m2, *min, *max;
} f16_ens;
int f16_rollout_wind_ens(f16_ctx *ctx, double *x, const double *u_seq, const f16_wind *h_wind, double *traj, const f16_ens *h_ens,
                         int32_t *status, long B, long ld, int nsteps, int hold, int traj_every, double dt, double xcg, int fi_flag,
                         int method, unsigned flags, void *stream);
int f16_rollout_lqr_wind_ens(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem_seq, const f16_wind *h_wind,
                             double *traj, const f16_ens *h_ens, double *u_out, int32_t *status, long B, long ld, int nsteps, int hold,
                             int traj_every, double dt, double xcg, int fi_flag, int method, unsigned flags, void *stream);
int f16_ens_from_traj(f16_ctx *ctx, const double *traj, int nsamples, long B, long ld, unsigned flags, const f16_ens *h_ens,
                      void *stream);
/* OUTPUT FEEDBACK: the frozen-gain nonlinear LQR loop of f16_rollout_lqr_wind on NOISY SENSORS, through a steady-state Kalman filter
 * on the reduced 9-state model, in one launch: sampled sensor noise, the filter between sensors and control law, the reference's LQR
 * law on the estimate.  The rule is stated HERE ONCE; the device code (csrc/f16_observer.hpp) and the numpy restatement
 * (f16_mpc_oop_py_amd/observer.py `observer_reference`, `meas_normals`, `kalman_reference`) follow it.
 *   Notation.  MPC-state order (parameters.py:135: phi theta alpha beta p q r lf1 lf2): x9 = x[3, 4, 7, 8, 9, 10, 11, 17, 16];
 *     s = x[13..15], the three surface positions -- the reduced model's inputs (env.py `_calc_xdot_na` writes u into those states).
 *   Observer model: a record of F16_OBS_DOUBLES (208) contiguous doubles per model,
 *         0 .. 80   Ad[81]      81 .. 107  Bd[27]      108 .. 188  Lf[81]      (all row-major)
 *         189 .. 197  x9_trim[9]      198 .. 200  s_trim[3]      201 .. 207  zero padding
 *     obs[M][208]: DEVICE.  Aircraft b uses model b / mgroup; mgroup is a multiple of 64, >= 64, or 0 = one model for the whole
 *     batch (as the ensemble's group): a wavefront reads ONE model, at wave-uniform addresses, through the scalar cache.
 *   Sensors.  sensed: a 9-bit mask, uniform over the batch, bit k = channel k of x9 is measured.  h_sigma[9]: HOST, the noise standard
 *     deviation per channel, finite and >= 0 (0: a noise-free channel); it travels in the argument block.
 *   Per step t of an aircraft that is not frozen, before the plant step, from the state at the start of the step, xm = the prediction
 *     the xhat array holds:
 *         1.  y_k = x9_k + (sigma_k * n_k)                                     sensed k; every operation rounded on its own
 *         2.  e_k = y_k - xm_k;   xh_i = xm_i + sum_k Lf[i][k] e_k             over the sensed k in ascending order, one fma per term
 *         3.  u[1+i] = lqr_action(K[i][4..6], dem - xh[4..6], u0[1+i])         f16_rollout_lqr's law on xh; the thrust command is held
 *         4.  xm <- x9_trim + Ad (xh - x9_trim) + Bd (s - s_trim)              per entry: x9_trim_i, then the nine Ad terms, then the
 *                                                                              three Bd terms, one fma per term
 *         5.  the plant step of f16_rollout_lqr_wind
 *     A frozen aircraft skips 1 - 5 and keeps xm.  The noise is counter-based: nothing "advances".
 *   Noise.  Call j (0, 1, 2) of step t is Philox4x32-10 on the counter (mrow0 + t, j, 0xFFFFFFFE, aircraft), key = (meas_seed &
 *     0xffffffff, meas_seed >> 32).  Gusts use 0xFFFFFFFF in word 2 and MPPI values below 256, so one seed may serve all three.
 *     U_i = (r_i + 0.5) 2^-32 as in the gust sampler; all four Box-Muller outputs are used, (ra c1, ra s1, rb c3, rb s3) with
 *     ra = sqrt(-2 log U0), rb = sqrt(-2 log U2), (c1, s1) = cos, sin(2 pi U1), (c3, s3) = cos, sin(2 pi U3), for channels
 *     4 j .. 4 j + 3.  A call whose channels are all unsensed is not made.
 *   f16_kalman_batch: the steady-state filter of M models.  Ad[81][ld]; w[9][ld] the diagonal process-noise variances per step;
 *     v[9][ld] the measurement variances, > 0 on sensed channels and ignored elsewhere (all DEVICE).  The prediction covariance P
 *     solves P = Ad P Ad' - Ad P C'(C P C' + V)^-1 C P Ad' + W by the doubling f16_lqr_batch runs (A <- Ad', G <- C'V^-1 C, H <- W),
 *     one wavefront per model on the fp64 matrix cores; Lf = P (I + G P)^-1 C'V^-1 (= P C'(C P C' + V)^-1), in the 9 x 9 frame, the
 *     columns of unsensed channels exactly zero.  Lf[81][ld] row-major; Pm[81][ld] (P) and iters[M] may be NULL.  status[M] is OR-ed
 *     into: F16_ST_QP_MAXITER when 60 doublings do not converge or the solution is not finite (f16_lqr_batch's convention).
 *     F16_EINVAL: a NULL pointer among the required ones, M < 0, ld < M, sensed outside 1 .. 0x1ff.  M == 0 is a no-op.
 *   f16_observer_step: steps 1 - 4 for a batch, through the SAME out-of-line device function the rollout kernels call under
 *     F16_FLAG_ONE_LANE (the default kernels inline the rule, as they inline the plant step; every product of steps 2 and 4 is one
 *     fma and step 1 is rounded operation by operation whoever compiles it).  x[18][ld],
 *     u0[4][ld], K[27][ld], dem[3][ld]; status[B] (may be NULL) is only read: an aircraft that carries F16_ST_ENVELOPE, or lies
 *     outside the box of env.py:117-124 (unless F16_FLAG_NO_ENVELOPE), is skipped and nothing of it is written.  mrow: counter word 0.
 *     xhat[9][ld] in / out: xm before and after.  y_out[9][ld] (may be NULL): the measurements, sensed channels only.  u_cmd[4][ld]:
 *     the command of the step, u_cmd[0] = u0[0].
 *   f16_rollout_lqg_wind / f16_rollout_lqg_wind_ens are f16_rollout_lqr_wind / f16_rollout_lqr_wind_ens under the rule: same
 *     arguments, layouts, holds, envelope freeze, status bits, samples, u_out, no-op rules, both methods.  xhat in / out.  xhat_traj
 *     [S][9][ld] (may be NULL): THE CONTENT OF xhat AT EVERY SAMPLE POINT, i.e. the prediction xm of the state stored in traj -- the
 *     sample of the estimate is to xhat what the sample of the state is to x, for frozen aircraft and across split calls alike.
 *     traj_every is read when traj or xhat_traj is given.  A NULL h_wind, or one whose pointers are all NULL, is zero air THROUGH THE
 *     WIND KERNELS, as in the ensemble twin, not a forward.  Nothing is allocated: the calls can be captured into a graph.
 *     F16_EINVAL: what the sibling refuses, in its order; then a NULL obs, h_sigma or xhat; mgroup < 0 or mgroup % 64 != 0; sensed
 *     outside 1 .. 0x1ff; a sigma negative or not finite.  B == 0 or nsteps == 0 is a no-op.
 *   Contracts.  Under F16_FLAG_ONE_LANE one call equals the chain of (f16_observer_step, one step of f16_rollout_wind with that
 *     u_cmd) BIT FOR BIT; for every batch size, both methods and both flag settings n + m steps equal n steps then m steps with mrow0,
 *     row0, xhat and gstate continued, where n is a multiple of hold and gust_hold.
 *   Launch rules: those of the siblings (one lane per aircraft, 64 / 128 / 256 lanes, the exact kernel under F16_FLAG_ONE_LANE; never
 *     the role-wave kernels).  xm lives in the xhat array between steps: a coalesced 72 B read and write per aircraft and step.
 *   OUT OF SCOPE: observers in the MPC, MPPI, gain-scheduled and re-linearised loops; models not grouped by wavefront; a sensor
 *     period other than one step; correlated or coloured sensor noise; time-varying filters; air-data sensors. */
#define F16_OBS_DOUBLES 208
int f16_kalman_batch(f16_ctx *ctx, const double *Ad, const double *w, const double *v, int sensed, double *Lf, double *Pm,
                     int32_t *iters, int32_t *status, long M, long ld, void *stream);
int f16_observer_step(f16_ctx *ctx, const double *x, const int32_t *status, const double *u0, const double *K, const double *dem,
                      const double *obs, long mgroup, int sensed, const double *h_sigma, uint64_t meas_seed, uint32_t mrow,
                      double *xhat, double *y_out, double *u_cmd, long B, long ld, unsigned flags, void *stream);
int f16_rollout_lqg_wind(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem_seq, const f16_wind *h_wind,
                         const double *obs, long mgroup, int sensed, const double *h_sigma, uint64_t meas_seed, uint32_t mrow0,
                         double *xhat, double *traj, double *xhat_traj, double *u_out, int32_t *status, long B, long ld, int nsteps,
                         int hold, int traj_every, double dt, double xcg, int fi_flag, int method, unsigned flags, void *stream);
int f16_rollout_lqg_wind_ens(f16_ctx *ctx, double *x, const double *u0, const double *K, const double *dem_seq, const f16_wind *h_wind,
                             const double *obs, long mgroup, int sensed, const double *h_sigma, uint64_t meas_seed, uint32_t mrow0,
                             double *xhat, double *traj, double *xhat_traj, const f16_ens *h_ens, double *u_out, int32_t *status, long B,
                             long ld, int nsteps, int hold, int traj_every, double dt, double xcg, int fi_flag, int method,
                             unsigned flags, void *stream);
/* The reference's LINEAR-model closed loops as ONE launch (9-state reduced model, 3 inputs; one lane per aircraft, its matrices in
 * registers):   per step   u = -K (x_ref - x) + u0,   x = Ad x + Bd u
 *   test_env_mk2.py:46-62 `LQR(linear=True)` (what main.py:35 runs): the frozen model ssr.Ad / ssr.Bd under env.py:360-371
 *     `_calc_LQR_action` -- K as the reference holds it (K = -dlqr, f16_lqr_batch's output), x_ref = the CURRENT state with
 *     x_ref[4:7] = (p, q, r)_dem: track_mask = 0x70 and x_ref[4..6][ld] = the demands, u0 = u.initial_condition[1:];
 *   test_env.py:501-576 `test_LQR_lin`: u = -K' (x - x_ref) with K' = dlqr and a FIXED reference: track_mask = 0x1FF, K = -K', u0 NULL.
 * x9[9][ld] in place (MPC-state order, parameters.py:135); Ad[81][ld], Bd[27][ld], K[27][ld] row-major per aircraft; x_ref[9][ld]
 * (entries outside track_mask are not read); u0[3][ld] or NULL (= 0).  traj_x (may be NULL) [nsteps / traj_every][9][ld] and traj_u
 * (may be NULL) [..][3][ld] receive the state AFTER and the action OF every traj_every-th step (x_storage / u_storage of the
 * reference's loops).  No envelope, no saturation: the reference's loops have none (on the reference's own model the first loop
 * grows like exp(14 t) -- SURVEY.md 8-Q.3 -- and so does this one, fixture G13). */
int f16_rollout_lqr_linear(f16_ctx *ctx, double *x9, const double *Ad, const double *Bd, const double *K, const double *x_ref,
                           const double *u0, double *traj_x, double *traj_u, long B, long ld, int nsteps, int traj_every,
                           unsigned track_mask, void *stream);
/* env.py:152-193 _calc_xdot_na: x9[9][ld], u3[3][ld] scattered over x_full[18][ld] -> xdot9[9][ld] */
int f16_xdot_na_batch(f16_ctx *ctx, const double *x_full, const double *x9, const double *u3, double *xdot9,
                      int32_t *status, long B, long ld, double xcg, int fi_flag, unsigned flags, void *stream);

/* ---- (2) batched trim ---------------------------------------------------- */
/* env.py:198-292 F16.trim(h_t, v_t) for B flight conditions h[B], v[B] (device): the reference's Nelder-Mead
 * (scipy defaults, tol 1e-10, maxiter 5e4; initial guess env.py:265-271 unless h_x0[5] on the HOST is given)
 * -> x_trim[18][ld]; cost[B], iters[B], nfev[B], status[B] may be NULL.
 *   The iteration count.  maxiter and iters mean what scipy's option `maxiter` and result `nit` mean: scipy's counter starts at
 *     1, the loop runs `while iterations < maxiter` and adds 1 after every iteration.  So a call performs at most maxiter - 1
 *     iterations, iters[b] = iterations performed + 1, and F16_ST_QP_MAXITER is set where scipy reports status 2: iters[b] >=
 *     maxiter after the loop (also when the termination test would have held for that last simplex: the cap is tested first).
 *     maxiter <= 0 stands for the reference's 50,000.  nfev[b] counts what the sequential algorithm evaluates: 6 for the initial
 *     simplex, then 1 (reflection accepted), 2 (expansion or contraction tried) or 7 (shrink) per iteration.
 *   status[b] is OR-ed into, never cleared: the caller zeroes it, and a bit that is already set survives the call.
 *   Columns B .. ld - 1 of x_trim are not written. */
int f16_trim_batch(f16_ctx *ctx, const double *h, const double *v, double *x_trim, double *cost, int32_t *iters,
                   int32_t *nfev, int32_t *status, long B, long ld, double xcg, int fi_flag, unsigned flags,
                   int maxiter, const double *h_x0, void *stream);
/* STEADY-STATE TRIM IN A MANOEUVRE (Stevens & Lewis, section 3.6): a climb or descent at flight-path angle gamma, a coordinated
 * turn at rate psi_dot, a pull-up at rate theta_dot, or any sum of them, at zero roll rate -- for B conditions in one launch.  The
 * rule is stated HERE ONCE; csrc/f16_trim.hip (`trim_man_cost`) and tests/trim_man_cases.py restate it.
 *   Unknowns.  q = (P3, dh, da, dr, alpha, beta): the level trim's five in its order, and the sideslip.
 *   Givens per condition (device arrays [B], each may be NULL = 0 for every condition): h, V, gamma (rad), psi_dot (rad/s),
 *     theta_dot (rad/s).
 *   Clipped copies.  The four commands and alpha are clipped as the level trim's objective clips them (1000 .. 19000, +-25, +-21.5,
 *     +-30, -20 .. 90 deg); beta to +-30 deg, the table range.  The flap states x[16] (the level trim's formula) and x[17] =
 *     -alpha 180 / pi come from the UNCLIPPED alpha.
 *   Constraints, at the clipped alpha and beta, g = 32.17 (the plant's own constant in the force equations):
 *         G = psi_dot V / g
 *         a = 1 - G tan(alpha) sin(beta);   b = sin(gamma) / cos(beta);   c = 1 + G^2 cos^2(beta)
 *         tan(phi)   = G (cos(beta) / cos(alpha)) [ (a - b^2) + b tan(alpha) sqrt(c (1 - b^2) + G^2 sin^2(beta)) ]
 *                      / [ a^2 - b^2 (1 + c tan^2(alpha)) ]
 *         a' = cos(alpha) cos(beta);        b' = sin(phi) sin(beta) + cos(phi) sin(alpha) cos(beta)
 *         tan(theta) = [ a' b' + sin(gamma) sqrt(a'^2 - sin^2(gamma) + b'^2) ] / (a'^2 - sin^2(gamma))
 *         p = -psi_dot sin(theta)
 *         q =  theta_dot cos(phi) + psi_dot sin(phi) cos(theta)
 *         r = -theta_dot sin(phi) + psi_dot cos(phi) cos(theta)
 *     phi and theta by atan of the quotients.
 *   The plant state is x = (0, 0, h, phi, theta, 0, V, alpha, beta, p, q, r, P3, dh, da, dr, lef, -alpha 180 / pi) with the clipped
 *     copies, the commands u = x[12..15], and
 *         cost = sum_k w_k (xdot_k - target_k)^2,   w = (0, 0, 5, 10, 10, 10, 2, 10, 10, 10, 10, 10)   (the level trim's weights)
 *         target = 0 except target[2] = V sin(gamma), target[4] = theta_dot, target[5] = psi_dot.
 *   Returned.  x_trim[18][ld] is that x with the six unknowns written back UNCLIPPED into x[12..15], x[7], x[8] (as the level trim
 *     does for its five): q = x[12, 13, 14, 15, 7, 8] reads the optimiser's point back.  cost[B], iters[B], nfev[B], status[B] may
 *     be NULL; status is OR-ed into; columns B .. ld - 1 are not written.
 *   Not iterated.  A condition whose gamma is not finite or |gamma| >= pi / 2, whose psi_dot or theta_dot is not finite, or whose
 *     constraints (phi, theta, p, q, r) are not finite at its start point returns x_trim and cost NaN, iters 0, nfev 0 and
 *     F16_ST_NONFINITE.
 *   The optimiser is f16_trim_batch's -- scipy's Nelder-Mead, tol 1e-10, the same counter, cap, termination, tie rule and fixed-point
 *     fast-forward -- in six dimensions: seven vertices; nfev is 7 for the initial simplex, then 1, 2 or 8 per iteration.
 *   Runs.  One Nelder-Mead run in six unknowns stalls (cost 1e-6 .. 1e-2); a second run from its best point converges (1e-27).  A call
 *     makes runs >= 1 runs (runs <= 0: F16_EINVAL).  Run k + 1 starts from the best vertex of run k with a fresh initial simplex (5 %
 *     of each coordinate, 0.00025 on a zero); each run has a counter and the cap maxiter of its own (maxiter <= 0: 50,000); iters
 *     and nfev are totals over the runs; F16_ST_QP_MAXITER is set when any run ended on its cap.
 *   q0[6][ld] (device) is a start per condition; NULL is the level trim's start with beta = 0. */
int f16_trim_man_batch(f16_ctx *ctx, const double *h, const double *v, const double *gamma, const double *psi_dot,
                       const double *theta_dot, const double *q0, double *x_trim, double *cost, int32_t *iters,
                       int32_t *nfev, int32_t *status, long B, long ld, double xcg, int fi_flag, unsigned flags,
                       int maxiter, int runs, void *stream);

/* ---- (2) batched control chain ---------------------------------------------------------- */
/* env.py:294-342 with _calc_xdot_na/_get_obs_na at each aircraft's own point: x9 = x[mpc idx] of x[18][ld],
 * u3 = u[1..3] of u[4][ld] (self.u._get_mpc_u(), env.py:348): Ac[81][ld] Bc[27][ld] Cc[81][ld]
 * (row-major element index = r*ncols+c); eps = 1e-5 in the reference (env.py:319).  Cc[r][c] = (x9[r] + dx[r] - x9[r]) / eps with
 * dx = eps e_c: off the diagonal an exact zero, and NaN in the whole row of a state that is NaN or infinite (as in the reference). */
int f16_linearise_batch(f16_ctx *ctx, const double *x, const double *u, double *Ac, double *Bc, double *Cc,
                        int32_t *status, long B, long ld, double eps, double xcg, int fi_flag,
                        unsigned flags, void *stream);
/* scipy.signal.cont2discrete(zoh) (env.py:50,351): Ad[81][ld], Bd[27][ld] = expm([[A,B],[0,0]] dt) blocks */
int f16_c2d_batch(f16_ctx *ctx, const double *Ac, const double *Bc, double *Ad, double *Bd,
                  long B, long ld, double dt, void *stream);
/* env.py:45-46: the 18-state model.  linearise with the default _calc_xdot/get_obs: Ac[324][ld] (18x18), Bc[72][ld]
 * (18x4), Cc[180][ld] (10x18, observed states parameters.py:134); then cont2discrete(zoh): Ad[324][ld], Bd[72][ld]. */
int f16_linearise_full_batch(f16_ctx *ctx, const double *x, const double *u, double *Ac, double *Bc, double *Cc,
                             int32_t *status, long B, long ld, double eps, double xcg, int fi_flag,
                             unsigned flags, void *stream);
int f16_c2d_full_batch(f16_ctx *ctx, const double *Ac, const double *Bc, double *Ad, double *Bd,
                       long B, long ld, double dt, void *stream);
/* utils.py:219-245 dlqr with Q = Cd'Cd, R = I3 (env.py:353-356): K[27][ld] = -dlqr (3x9 row-major),
 * Pare[81][ld] = DARE solution (may be NULL).  status[ld] (may be NULL; OR-ed into): F16_ST_QP_MAXITER when the DARE has not
 * converged within its 60 doublings, and whenever its solution is not finite (a NaN or overflowing model), however few doublings
 * that took; Pare and K are then the last iterate and the gain formed from it. */
int f16_lqr_batch(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, double *K, double *Pare,
                  int32_t *status, long B, long ld, void *stream);
/* env.py:373-424 _calc_MPC_action for B aircraft: per aircraft (Ad,Bd,Cd) + current state x[18][ld]
 * + demands dem[3][ld] (p,q,r; written to x_ref[5:8] exactly as the reference does) -> first move
 * u_cmd[3][ld].  Dense condensed QP of horizon hzn (utils.py:21-167) solved as the reference's call solves it
 * (env.py:420-422: osqp.OSQP().setup(P, q, A, l, u, max_iter=40000, polish=False), every other setting at its default):
 * OSQP's published ADMM with Ruiz equilibration (`scaling` passes, D / E / c), rho = 0.1, sigma 1e-6, alpha 1.6,
 * termination on the UNSCALED residuals (eps 1e-3) every `check_every` iterations, rho re-estimated from the SCALED
 * residuals every `rho_every` iterations (OSQP's own interval is wall-clock based; 100 is its no-timer constant
 * ADAPTIVE_RHO_FIXED; must be a multiple of `check_every`, else F16_EINVAL: the estimate is formed from the residuals of a
 * termination test) and applied when it moves by more than 5x, primal-infeasibility certificate (-> NaN command +
 * F16_ST_QP_INFEASIBLE, as OSQP returns).  Rows of A with two infinite bounds (phi, theta, lf1) take part in the
 * equilibration and are then left out of the iteration (OSQP carries them with rho_min = 1e-6; they never bind).
 * Opt-in alternative (the builder's rule, faster on this family of QPs): scaling = 0, rho = 0 -> no equilibration and
 * the start value rho = 2 sqrt(tr P / tr A'A); scaling = 0, rho > 0 -> no equilibration, fixed start value.
 * Horizons: 1 <= hzn <= 150.  hzn <= 30 (equilibrated solves) runs one wavefront per aircraft, hzn <= 32 the 512-lane
 * register-resident solver, larger horizons (the reference's own sweep goes to 150, env.py:426-436) one 512-lane workgroup
 * per aircraft with the KKT inverse in the HBM workspace (the stream of its symmetric half, 0.93 MB per iteration at hzn = 150,
 * sets the pace; f16_mpc_hzn_sweep below solves all horizons of a sweep in one launch).
 * u_seq (may be NULL) gets the full [3*hzn][ld] sequence, info (may be NULL) gets [4][ld] = iterations, r_prim, r_dual
 * (unscaled), rho.  status[ld] (may be NULL) is OR-ed into, never cleared, by f16_mpc_batch(_w) and f16_mpc_plan_solve(_w) alike:
 * the caller zeroes it, and a bit that is already set survives the call.
 * Nothing the results depend on is retained between calls: the QP workspace is allocated and freed per call, stream-ordered
 * on `stream`; calls on different streams of one context do not share buffers.  Under stream capture the call returns
 * F16_EINVAL (graph replays of the stream-ordered allocation were measured unreliable on ROCm 7.2): capture
 * f16_mpc_plan_solve instead, whose workspace lives with the plan.
 * Scheduling only: workgroups are dispatched longest-first by the iteration counts of the previous call of the same
 * batch size on the same stream (results do not depend on it; F16_MPC_DISPATCH_ORDER=0 keeps the caller's order). */
/* Weights, reference and bounds of the QP as ARGUMENTS -- what utils.py:21 `setup_OSQP(x_ref, A, B, Q, R, hzn, dt, x, act_states,
 * x_lb, x_ub, u_lb, u_ub, udot_lb, udot_ub)` and utils.py:219 `dlqr(A, B, Q, R)` take; env.py:373-424 fills them with
 * constants (Q = Cd'Cd, R = I, x_ref = x with x_ref[5:8] = demands, the boxes of parameters.py:59-129), and the entry points without
 * the `_w` suffix do the same.  The `_w` entry points take a HOST pointer h_w to this struct (NULL = env.py's constants, bit for
 * bit the plain entry point) and, where a reference enters, a DEVICE pointer x_ref[9][ld] (NULL = env.py:380-383 from `dem`; with
 * x_ref given `dem` may be NULL).  Weights and bounds are uniform over the batch; x_ref is per aircraft.  MPC-state order:
 * phi, theta, alpha, beta, p, q, r, lf1, lf2 (parameters.py:135); +-INFINITY = no bound.
 * Solvers: the six state rows the reference bounds (alpha, beta, p, q, r, lf2) stay the bounded ones -- their VALUES are free
 * (one side may be infinite), but a finite bound on phi / theta / lf1 or no bound at all on one of the six is F16_EINVAL;
 * f16_mpc_qp_debug_w (the QP alone, dense, in the reference's form) takes any pattern. */
typedef struct f16_mpc_weights {
  int q_from_cd;                 /* 1: Q = Cd'Cd per aircraft (env.py:389) and Q[] is ignored */
  double Q[81];                  /* 9 x 9 row-major, symmetric positive semidefinite (the author's own alternative: env.py:391-401) */
  double R[9];                   /* 3 x 3 row-major, symmetric positive definite (env.py:403-407) */
  double x_lb[9], x_ub[9];       /* parameters.py _vec_mpc_x_lb / _ub */
  double u_lb[3], u_ub[3];       /* _vec_mpc_u_lb / _ub */
  double udot_lb[3], udot_ub[3]; /* _vec_mpc_udot_lb / _ub */
} f16_mpc_weights;
void f16_mpc_default_weights(f16_mpc_weights *w);      /* env.py's constants */
int f16_lqr_batch_w(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, const f16_mpc_weights *h_w, double *K,
                    double *Pare, int32_t *status, long B, long ld, void *stream);        /* utils.py:219: Q, R of h_w */
/* The PER-STEP RE-LINEARISED LQR loop (test_env.py:625-687 `test_LQR_dynamic_nl`) as ONE launch: per step, for every aircraft that
 * is not frozen,
 *     A, B, C = linearise_na(x, u[1:4], eps)    (f16_linearise_batch: C = diag((x + eps - x) / eps))
 *     Ad, Bd  = zoh(A, B, dt)                    (f16_c2d_batch)
 *     Kd      = dlqr(Ad, Bd, Q, R)               (f16_lqr_batch_w; h_w supplies Q and R only -- NULL or q_from_cd = 1: Q = Cd'Cd,
 *                                                 and R = I unless h_w gives another; no other field of h_w is read)
 *     u[1+i]  = -Kd (x9 - x_ref_eff) + u0[i],   x_ref_eff[j] = x_ref[j] where bit j of track_mask is set, else the current x9[j]
 *     step(u)                                    (env.py:105-130 through the F16_FLAG_ONE_LANE step; thrust u[0] held)
 * with the envelope rule and status bits of f16_rollout(F16_FLAG_ONE_LANE): F16_ST_ENVELOPE freezes (F16_FLAG_NO_ENVELOPE skips the
 * test), F16_ST_NONFINITE and F16_ST_ENV_STATE are set at the end; a DARE that has not converged within its 60 doublings sets
 * F16_ST_QP_MAXITER (as f16_lqr_batch does) and the step goes on with that gain.  The grid bits of the linearisation's perturbed
 * points are not kept (_calc_LQR_gain does not keep them either); those of the steps are.
 * The two reference loops:  test_LQR_dynamic_nl: x_ref = the initial x9, track_mask = 0x1FF, Q = I, R = 1e4 I, u0 = NULL;
 *   env.py's law re-derived every step (_calc_LQR_gain() then _calc_LQR_action(p, q, r, K, x9, u.initial_condition[1:])):
 *   track_mask = 0x70, x_ref[4..6] = the demands, default weights, u0 = u.initial_condition[1:].
 * x[18][ld] and u[4][ld] (u.values) in place: u ends up holding the last command.  x_ref[9][ld] (may be NULL when track_mask
 * selects nothing; untracked entries are not read), u0[3][ld] or NULL (= 0).  status[ld] (may be NULL) is read and written: an
 * aircraft frozen on entry stays frozen.  traj [nsteps/traj_every][18][ld], u_traj [..][3][ld], K_traj [..][27][ld] (each may be
 * NULL) receive, every traj_every-th step, the state after the step, the command of the step and the gain used, K = -dlqr (the sign
 * of f16_lqr_batch and _calc_LQR_gain, 3 x 9 row-major); a frozen step stores the held command and the last gain (zeros if none
 * was computed in this launch).  F16_EINVAL: NULL x / u, ld < B, nsteps < 1, traj_every < 1, nsteps % traj_every != 0, eps <= 0,
 * a track_mask without x_ref, or Q / R not as f16_lqr_batch_w takes them.
 * One wavefront per aircraft for all nsteps (the matrices in LDS); results do not depend on B or on how nsteps is split over
 * calls. */
int f16_rollout_lqr_relin(f16_ctx *ctx, double *x, double *u, const double *x_ref, const double *u0,
                          const f16_mpc_weights *h_w, double *traj, double *u_traj, double *K_traj,
                          int32_t *status, long B, long ld, int nsteps, int traj_every, unsigned track_mask,
                          double eps, double dt, double xcg, int fi_flag, unsigned flags, void *stream);

/* f16_rollout_lqr_relin under a SCHEDULE of references, one launch: x_ref becomes xref_seq[S][9][ld] with S = ceil(nsteps / hold), and
 * step t reads row t / hold (the last segment may be shorter; hold >= nsteps reads row 0 only).  Only the entries selected by
 * track_mask are read.  Everything else is f16_rollout_lqr_relin's, so the call equals the chain of f16_rollout_lqr_relin calls, one
 * per row with that row as x_ref, bit for bit (the chain's K_traj holds zeros for an aircraft that was frozen on entry of a call; this
 * call keeps the last gain of the launch).  F16_EINVAL as f16_rollout_lqr_relin, and for hold < 1 or a track_mask without xref_seq. */
int f16_rollout_lqr_relin_sched(f16_ctx *ctx, double *x, double *u, const double *xref_seq, const double *u0,
                                const f16_mpc_weights *h_w, double *traj, double *u_traj, double *K_traj,
                                int32_t *status, long B, long ld, int nsteps, int hold, int traj_every, unsigned track_mask,
                                double eps, double dt, double xcg, int fi_flag, unsigned flags, void *stream);

typedef struct f16_qp_settings {
  double rho, sigma, alpha, eps_abs, eps_rel, eps_prim_inf;
  int max_iter, check_every, rho_every, adaptive_rho;
  int scaling;     /* Ruiz equilibration passes (OSQP default 10; 0 = none) */
} f16_qp_settings;
void f16_qp_default_settings(f16_qp_settings *s);
int f16_mpc_batch(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, const double *x,
                  const double *dem, double *u_cmd, double *u_seq, double *info, int32_t *status,
                  long B, long ld, int hzn, double dt, const f16_qp_settings *s, void *stream);
int f16_mpc_batch_w(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, const double *x, const double *dem,
                    const double *x_ref, const f16_mpc_weights *h_w, double *u_cmd, double *u_seq, double *info, int32_t *status,
                    long B, long ld, int hzn, double dt, const f16_qp_settings *s, void *stream);
/* env.py:426-436 `_calc_constr_checking_hzn`: the first move of calc_MPC_action for the SAME states, demands and model at
 * every horizon hzn_lo..hzn_hi (1 <= hzn_lo <= hzn_hi <= 150) as one call.  u_cmd [hzn_hi - hzn_lo + 1][3][ld], info (may be
 * NULL) [..][4][ld], status (may be NULL, OR-ed into) [..][ld]; slice k = hzn - hzn_lo holds exactly what f16_mpc_batch returns
 * for that horizon (bit-identical: same kernels).  Horizons <= 32 run one after the other; the longer ones are built per
 * horizon and solved by ONE launch over every (horizon, aircraft) pair, longest horizon first, so that the few solves that
 * need tens of thousands of iterations do not hold a launch of their own.  Workspace: stream-ordered, in groups of horizons
 * of at most F16_SWEEP_WS_GB (default 32) GB (4.45 MB per aircraft at N = 150: P, the QP extras and the solver's 3.59 MB of operands).  Not capturable.
 * Scheduling only: a repeated sweep of the same horizons on the same stream takes its pairs costliest-first by the iteration
 * counts of the previous one (results do not depend on it; F16_MPC_DISPATCH_ORDER=0 switches it off). */
int f16_mpc_hzn_sweep(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, const double *x,
                      const double *dem, double *u_cmd, double *info, int32_t *status, long B, long ld, int hzn_lo,
                      int hzn_hi, double dt, const f16_qp_settings *s, void *stream);
/* Prepared plans.  The reference freezes (Ad,Bd,Cd) at construction (env.py:49-60) yet rebuilds the whole QP on every
 * _calc_MPC_action call (utils.py:21-167 inside env.py:373-424).  A plan computes the model-only part once -- DARE,
 * terminal weight, prediction blocks, P; with scaling = 0 also the start value of rho and the inverse of the KKT matrix
 * (73.7 KB per aircraft) -- and f16_mpc_plan_solve does what is left per call: the state-dependent vectors, the
 * iterations and, with OSQP's defaults, equilibration + factorisation (OSQP's scaling looks at q, i.e. at the state of the
 * call).  Results are bit-identical to f16_mpc_batch with the same settings.  hzn <= 40 (33..40: the model part is kept, every solve runs the
 * long-horizon solver; no warm start there).  (Ad,Bd,Cd) are read during
 * f16_mpc_plan_create only. */
typedef struct f16_mpc_plan f16_mpc_plan;
/* The reference's closed MPC loop (test_env.py:480-495; BASELINE config 5) as ONE launch on a prepared plan (hzn <= 30, OSQP's
 * default settings: scaling > 0; every solve starts cold as the reference's does, unless f16_mpc_plan_warm_start switched the plan's
 * opt-in warm start on: then step t starts from the solution of step t - 1):  per step  cmd = _calc_MPC_action(p, q, r, hzn);  u.values[1:] = cmd;  step(u.values).
 * x[18][ld] in place; u[4][ld] = u.values in place (thrust command held, u[1:4] receives every step's command and ends up
 * holding the last one, as the reference's u.values does); dem[3][ld].  traj (may be NULL) [nsteps / traj_every][18][ld]: the state
 * after every traj_every-th step; cmd_traj (may be NULL) [nsteps][3][ld]: what calc_MPC_action returned at each step; iters_traj
 * (may be NULL) [nsteps][ld] int32: its ADMM iterations; status[ld] (may be NULL): sticky OR of the step's and the solves' bits.
 * Work items are (step, aircraft) pairs drawn from one ticket counter by one wavefront per SIMD; a wavefront builds the state-
 * dependent vectors of the QP, solves it, writes the command and takes the Euler step of its pair, so that no step waits for another
 * aircraft's solve (the host loop joins the batch after every solve).  Results: bit-identical to the host loop
 * (f16_mpc_plan_solve + f16_rollout(..., nsteps = 1, flags | F16_FLAG_ONE_LANE) per step) for every aircraft that stays inside
 * its envelope.  Per-aircraft conditions:
 *   - QP certified infeasible: the command is NaN, as OSQP returns it (F16_ST_QP_INFEASIBLE): the actuator models propagate it
 *     (np.clip, utils.py:308-330), the surface states turn NaN (F16_ST_NONFINITE) and every later solve of that aircraft is skipped
 *     (NaN command, zero iterations) -- the reference's own loop is left with NaN states from there.  F16_FLAG_HOLD_COMMAND keeps
 *     the previous command instead and the aircraft flies on.
 *   - outside the envelope at the start of a step (env.py:117-124: the reference exit()s): frozen, flagged
 *     (F16_ST_ENVELOPE | F16_ST_ENV_STATE(k)) and NOT solved for any more: cmd_traj holds NaN, iters_traj 0, u keeps its value.
 * Not capturable on its first call on a plan (allocates the ticket / progress counters).  A plan serves one call at a time (its
 * workspace and these counters are per plan): order calls on one plan through one stream.  nsteps x B < 2^32 per call. */
int f16_rollout_mpc(f16_mpc_plan *plan, double *x, double *u, const double *dem, double *traj, double *cmd_traj,
                    int32_t *iters_traj, int32_t *status, int nsteps, int traj_every, double xcg, int fi_flag, unsigned flags,
                    void *stream);
/* The same closed loop with the model RE-DERIVED AT EVERY STEP (what `_calc_MPC_action(..., relinearise=True)` does when
 * it is called from a loop), as ONE launch.  Per step, for every aircraft that is neither frozen nor non-finite:
 *     A, B, C = forward differences of the reduced model at (x, u[1:4]) with the step eps   (the point and the rule of f16_linearise_batch:
 *                                                                  u.values, not the actuator states; C = diag((x + eps - x) / eps))
 *     Ad, Bd  = ZOH(A, B, dt)                                                               (f16_c2d_batch)
 *     cmd     = calc_MPC_action built from (Ad, Bd, C) with the plan's weights, bounds, horizon and settings
 *     u[1:4]  = cmd;  step(u)                                                               (the F16_FLAG_ONE_LANE step)
 * Arguments, the in-place x / u, traj, cmd_traj, iters_traj, the sticky status, F16_FLAG_HOLD_COMMAND, F16_FLAG_NO_ENVELOPE, the ticket
 * scheme and the rules for infeasible and frozen aircraft: as f16_rollout_mpc.  Differences:
 *   - the finiteness test comes before the linearisation and covers everything the plant evaluation reads: an aircraft with a
 *     non-finite entry in ANY of its eighteen states, in u[1:4] or in its demands is not linearised and not solved for (NaN command,
 *     zero iterations, F16_ST_NONFINITE); it still takes its step, as in f16_rollout_mpc.  The table-grid bits of the thirteen
 *     evaluation points of the linearisation are not kept (as f16_rollout_lqr_relin);
 *   - model_traj (may be NULL) [nsteps / traj_every][189][ld]: Ad (81) | Bd (27) | Cd (81), row-major, of the solve of every stored
 *     step (the counterpart of K_traj of f16_rollout_lqr_relin).  A pair without a solve (frozen, non-finite) stores NaN.  With the
 *     model of step t, the state before that step and the demands, f16_mpc_batch_w returns exactly cmd_traj[t] and iters_traj[t]: the
 *     loop builds its QP with the build kernel's own code;
 *   - a DARE that has not converged after 60 doublings is not flagged and its last iterate is the terminal weight: what f16_mpc_batch_w
 *     does with the same model;
 *   - eps <= 0 (or NaN) is F16_EINVAL; traj_every applies when traj or model_traj is given.
 * The plan supplies the workspace, weights, bounds, horizon, settings, the warm-start switch and the counters; the model it was created
 * from is NOT used, and the call overwrites the plan's per-aircraft model blocks (A | Q | Qbar, G_k, packed P).  Afterwards they hold,
 * per aircraft, the model of its last solved step, so the plan no longer describes one frozen model: from then on f16_mpc_plan_solve(_w)
 * and f16_rollout_mpc refuse it (F16_EINVAL); f16_rollout_mpc_relin, f16_mpc_plan_warm_start and f16_mpc_plan_destroy still take it.
 * Not capturable on its first call on a plan (allocates the counters and a copy of the weights). */
int f16_rollout_mpc_relin(f16_mpc_plan *plan, double *x, double *u, const double *dem, double *traj, double *cmd_traj,
                          int32_t *iters_traj, double *model_traj, int32_t *status, int nsteps, int traj_every, double eps,
                          double xcg, int fi_flag, unsigned flags, void *stream);
/* The two closed MPC loops at a CONTROL PERIOD OF SEVERAL PLANT STEPS, as ONE launch.  `hold` >= 1 plant steps follow every solve.  At
 * each of the nctrl control instants, for every aircraft:
 *     cmd = calc_MPC_action(p, q, r, hzn)       the existing rules; the model and the rate rows at the plan's dt = the control period
 *     u.values[1:] = cmd                        (F16_FLAG_HOLD_COMMAND as in f16_rollout_mpc)
 *     for j in range(hold): step(u.values)      env.py:105-130 with the PLANT step dt; the envelope test in front of EVERY plant step
 * f16_rollout_mpc_relin_hold: in front of the solve, forward differences at (x, u[1:4]) with the step eps, ZOH at the plan's dt (the
 * control period), the model part of the QP -- the stage of f16_rollout_mpc_relin unchanged.
 * `dt` is the plant's Euler step.  The plan's dt (f16_mpc_plan_create) is the control period, and the call returns F16_EINVAL unless
 * |hold * dt - plan dt| <= 1e-12 * plan dt: a model discretised at another period than the one it is applied at is a caller's
 * mistake, not a mode.
 * The call equals this host loop, bit for bit, for every aircraft that stays inside its envelope (frozen aircraft: equal states and
 * status words; the host loop goes on solving for them):
 *     for c in range(nctrl):
 *         f16_mpc_plan_solve(plan, x, dem, cmd, ...);  u[1:4] = cmd
 *         f16_rollout(ctx, x, u, x, samples, B, ld, hold, traj_every, dt, xcg, fi_flag, flags | F16_FLAG_ONE_LANE, status)
 * (re-linearised: f16_linearise_batch at (x, u[1:4]) -> f16_c2d_batch at hold * dt -> f16_mpc_batch_w in place of the plan's solve).
 * hold = 1 with dt = the plan's dt is f16_rollout_mpc / f16_rollout_mpc_relin (the same kernel: they are this call).
 *   - traj (may be NULL) [nctrl * hold / traj_every][18][ld]: the state after every traj_every-th PLANT step.  traj_every counts plant
 *     steps, is independent of hold, and nctrl * hold % traj_every == 0.
 *   - cmd_traj (may be NULL) [nctrl][3][ld] and iters_traj (may be NULL) [nctrl][ld]: one row per control step.
 *   - model_traj (may be NULL) [nctrl / model_every][189][ld]: Ad | Bd | Cd of control step c, stored when (c + 1) % model_every == 0,
 *     with nctrl % model_every == 0.  f16_mpc_batch_w on a stored model, the state before that control step and the demands, called
 *     with dt = the plan's dt, returns cmd_traj[c] and iters_traj[c] exactly.
 *   - x / u in place, the sticky status, F16_FLAG_*, NaN for infeasible or not-solved pairs, the ticket scheme: as in the two calls above.
 *     The re-linearised call marks the plan as f16_rollout_mpc_relin does (f16_rollout_mpc_hold then refuses it, F16_EINVAL).  Not
 *     capturable on a plan's first call.  nctrl x B < 2^32 and nctrl x hold < 2^31 per call.
 *   - F16_EINVAL also for hold < 1, nctrl < 1, model_every < 1, eps <= 0.
 * Per-aircraft rules at plant-step granularity: an aircraft found outside the envelope at the start of ANY plant step is frozen from
 * that plant step on, as f16_rollout does inside a launch -- the rest of its hold is not stepped, later samples repeat the frozen state,
 * and its later control steps are not solved for (NaN in cmd_traj, 0 iterations; re-linearised: NaN model).  F16_ST_NONFINITE is formed
 * after the last plant step of a control step. */
int f16_rollout_mpc_hold(f16_mpc_plan *plan, double *x, double *u, const double *dem, double *traj, double *cmd_traj,
                         int32_t *iters_traj, int32_t *status, int nctrl, int hold, int traj_every, double dt,
                         double xcg, int fi_flag, unsigned flags, void *stream);
int f16_rollout_mpc_relin_hold(f16_mpc_plan *plan, double *x, double *u, const double *dem, double *traj, double *cmd_traj,
                               int32_t *iters_traj, double *model_traj, int32_t *status, int nctrl, int hold, int traj_every,
                               int model_every, double dt, double eps, double xcg, int fi_flag, unsigned flags, void *stream);
/* The two calls above under a DEMAND SCHEDULE, as ONE launch (the pilot's p/q/r demand changes while the controller runs:
 * flight_sim.py:141-182; _calc_MPC_action takes the demand per call).  dem becomes dem_seq[S][3][ld] with S = ceil(nctrl / dem_hold),
 * state-major with the plan's ld, and control step c reads row c / dem_hold: the last segment may be shorter, dem_hold = 1 is a new
 * demand at every control step, dem_hold >= nctrl reads row 0 only.  The demand of a control step is held over the whole horizon of
 * that step's QP (x_ref[5:8] = demands, env.py:383): no preview, no QP vector built by another rule.  The call therefore equals the
 * chain of f16_rollout_mpc_hold / f16_rollout_mpc_relin_hold calls, one per row with that row as the constant demand, bit for bit.
 * hold = 1 with dt = the plan's dt is the reference's loop under a schedule.  Everything else is the base call's: the in-place x / u,
 * traj / cmd_traj / iters_traj / model_traj and their strides, the sticky status, F16_FLAG_*, the frozen / non-finite / infeasible rules
 * per (control step, aircraft) pair, the |hold * dt - plan dt| check, the plan marking of the re-linearised call, "not capturable on a
 * plan's first call", and the size limits.  A non-finite entry in the row of a control step is that step's F16_ST_NONFINITE (NaN
 * command, zero iterations), as a non-finite constant demand is; the next finite row is solved for again.  A frozen aircraft ignores
 * the rest of its schedule.  The plan's opt-in warm start is untouched: step c starts from step c - 1 whatever the rows are.
 * F16_EINVAL where the base call returns it, and for dem_hold < 1 or a NULL dem_seq. */
int f16_rollout_mpc_sched(f16_mpc_plan *plan, double *x, double *u, const double *dem_seq, double *traj, double *cmd_traj,
                          int32_t *iters_traj, int32_t *status, int nctrl, int hold, int dem_hold, int traj_every, double dt,
                          double xcg, int fi_flag, unsigned flags, void *stream);
int f16_rollout_mpc_relin_sched(f16_mpc_plan *plan, double *x, double *u, const double *dem_seq, double *traj, double *cmd_traj,
                                int32_t *iters_traj, double *model_traj, int32_t *status, int nctrl, int hold, int dem_hold,
                                int traj_every, int model_every, double dt, double eps, double xcg, int fi_flag, unsigned flags,
                                void *stream);
int f16_mpc_plan_create(f16_ctx *ctx, f16_mpc_plan **plan, const double *Ad, const double *Bd, const double *Cd,
                        long B, long ld, int hzn, double dt, const f16_qp_settings *s, void *stream);
int f16_mpc_plan_solve(f16_mpc_plan *plan, const double *x, const double *dem, double *u_cmd, double *u_seq,
                       double *info, int32_t *status, void *stream);
int f16_mpc_plan_create_w(f16_ctx *ctx, f16_mpc_plan **plan, const double *Ad, const double *Bd, const double *Cd,
                          const f16_mpc_weights *h_w, long B, long ld, int hzn, double dt, const f16_qp_settings *s, void *stream);
int f16_mpc_plan_solve_w(f16_mpc_plan *plan, const double *x, const double *dem, const double *x_ref, double *u_cmd,
                         double *u_seq, double *info, int32_t *status, void *stream);
/* Optional: start each solve of the plan from the previous solve's x, z, y (what OSQP does by default inside ONE
 * solver object; the reference builds a new object per call, i.e. always starts cold -- so this is off by default and
 * results then differ from the cold start within the termination tolerance).  Switching it on or off forgets the
 * stored solution; a solve that did not converge is not reused. */
int f16_mpc_plan_warm_start(f16_mpc_plan *plan, int on);
/* Optional: SOFT STATE ROWS.  h_w9 (host): nine penalty weights in MPC-state order (phi, theta, alpha, beta, p, q, r, lf1, lf2).  A
 * state row i with w_i > 0 is no constraint any more: every solve on the plan minimises
 *     1/2 u'Pu + q'u + sum over the soft rows of (w_i / 2) dist(a_i'u, [l_i, u_i])^2     subject to the other rows,
 * so a prediction that leaves the state box no longer makes the QP infeasible.  No slack variables: in the ADMM iteration the z-update
 * of a soft row is v = zr + y / rho_i, zc = clip(v, l, u), z = zc + kappa_i (v - zc), kappa_i = rho_i / (rho_i + c w_i / E_i^2); the
 * primal-infeasibility certificate treats it as a row without bounds; everything else is the hard solve's.  Command and rate rows stay
 * hard, and they alone can still make a QP infeasible (NaN command, F16_ST_QP_INFEASIBLE, F16_FLAG_HOLD_COMMAND as before).
 * F16_ST_QP_SOFT_ACTIVE: the z of some soft row of the returned (not infeasible) solve lies outside its [l, u]; sticky in the loops.
 * The penalty is quadratic and therefore inexact: an active soft row is violated slightly even when the hard QP is feasible.
 * NULL or all zeros switches soft rows off; the plan then is bit for bit what it was.  F16_EINVAL: a negative, NaN or infinite weight; a
 * positive weight on phi, theta or lf1 (no bounds); a plan the one-wavefront solver does not serve (hzn > 30, scaling = 0).  Switching
 * forgets a stored warm-start solution.  Honoured by f16_mpc_plan_solve(_w) and the six f16_rollout_mpc* calls (a re-linearised call
 * keeps the weights); their "equals the host loop" contracts hold unchanged, with the softened f16_mpc_plan_solve in the host loop. */
int f16_mpc_plan_soft_rows(f16_mpc_plan *plan, const double *h_w9);
void f16_mpc_plan_destroy(f16_mpc_plan *plan);      /* waits for the plan's own stream only */

/* utils.py:21-167 setup_OSQP alone for aircraft b (tests): h_P[n*n] h_q[n] h_A[(m rows)*n] h_l h_u on the
 * host, n = 3*hzn, rows = 15*hzn, reference row order. */
int f16_mpc_qp_debug(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, const double *x,
                     const double *dem, long b, long ld, int hzn, double dt,
                     double *h_P, double *h_q, double *h_A, double *h_l, double *h_u);

int f16_mpc_qp_debug_w(f16_ctx *ctx, const double *Ad, const double *Bd, const double *Cd, const double *x, const double *dem,
                       const double *x_ref, const f16_mpc_weights *h_w, long b, long ld, int hzn, double dt,
                       double *h_P, double *h_q, double *h_A, double *h_l, double *h_u);

/* Tests: inverse of B packed (lower triangle, row-major) SPD n x n matrices, n <= 96, on the device through the
 * KKT-inverse routine of the MPC solver (blocked sweep on the fp64 matrix cores, v_mfma_f64_16x16x4_f64).
 * packed [B][n(n+1)/2], out [B][n*n] (device pointers); NaN where a pivot block was not positive definite. */
int f16_debug_spd_inverse(f16_ctx *ctx, const double *packed, double *out, int n, long B, void *stream);

#ifdef __cplusplus
}
#endif
#endif
