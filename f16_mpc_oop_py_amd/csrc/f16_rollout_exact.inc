// f16_rollout_exact.inc -- the lane loop of the F16_FLAG_ONE_LANE rollouts, included once in the kernel k_rollout_exact (whose
// argument block it reads in place, as it always did) and once in rollout_exact_lanes, the device function through which the fused
// MPPI loop (k_rollout_mppi_exact) runs the same statements on the one lane of each thread.  Expects: a (RolloutArgs<SCHED, COST>),
// lanes (GridLanes / MppiLane), and the template parameters LQR, SCHED, COST, STAGES of the including function, and GS (the gain
// schedule of f16_rollout_lqr_gs: a (GainSchedArgs); false in the kernel k_rollout_exact).
  for (long b = lanes.first(64); b < lanes.end(a); b += lanes.stride(64)) {
    double x[18], u[4];
    long b0 = b;                                         // (COST: as in rollout_lanes; the reference in registers)
    double J = 0, ju = 0, xr[COST ? 9 : 1];
    if constexpr (COST) {
      b0 = lanes.aircraft(a, b);
#pragma unroll
      for (int k = 0; k < 18; ++k) x[k] = a.x0[k * a.ld0 + b0];
#pragma unroll
      for (int k = 0; k < 9; ++k) xr[k] = lanes.reference(a, k, x, b0);
    } else {
#pragma unroll
    for (int k = 0; k < 18; ++k) x[k] = a.out[k * a.ld + b];
    }
    [[maybe_unused]] const auto ref = [&](int k) { return xr[COST ? k : 0]; };
    if (!COST || a.nsteps > 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = a.u[k * a.ld + b];
    }
    if constexpr (COST) if (a.nsteps > 0) ju = cost_command_term(a, b0, u[1], u[2], u[3]);
    double kq[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, u0[3] = {u[1], u[2], u[3]};
    if (LQR) {
      if constexpr (!GS) {                                 // (GS: the first gain update, at step 0, fills the nine)
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) kq[3 * i + j] = a.K[(9 * i + 4 + j) * a.ld + b];
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) kq[9 + j] = a.dem[j * a.ld + b];
    }
    int st = !COST && a.status ? a.status[b] : 0;
    double *tr = a.traj ? a.traj + b : nullptr;
    int until_store = a.traj_every;
    constexpr int NR = LQR ? 3 : 4;
    RowAhead<NR> ra;
    if constexpr (SCHED) { ra.init(a, NR, a.out + b); ra.settle(); }
    [[maybe_unused]] int gs_left = 0, gs_cnt = 0;         // (GS: as in rollout_lanes)
    for (int t = 0; t < a.nsteps; ++t) {
      if constexpr (GS) {                                  // a gain update at the state this step starts from, frozen or not
        if (gs_left == 0) {
          gs_left = a.gs_every;
          double g[F16_GS_ENTRIES];
          gs_cnt += gain_lookup(a.grid, a.gtab, x[2], x[6], g);
#pragma unroll
          for (int e = 0; e < 9; ++e) kq[e] = g[e];
#pragma unroll
          for (int i = 0; i < 3; ++i) u0[i] = u[1 + i] = g[9 + i];      // (as a new launch: u0 until it steps)
        }
        --gs_left;
      }
      if (!(a.flags & FLAG_NO_ENVELOPE) && outside_envelope(x)) st |= ST_ENVELOPE;      // env.py:117-124
      if (!(st & ST_ENVELOPE)) {
        if (LQR) {
          const double e0 = kq[9] - x[9], e1 = kq[10] - x[10], e2 = kq[11] - x[11];
#pragma unroll
          for (int i = 0; i < 3; ++i) u[1 + i] = lqr_action(kq[3 * i], kq[3 * i + 1], kq[3 * i + 2], e0, e1, e2, u0[i]);
        }
        if constexpr (STAGES == 4) rk4_step_exact(a.tab, a.lofi, x, u, a.dt, a.xcg, a.fi, a.flags, &st);
        else
        euler_step_exact(a.tab, a.lofi, x, u, a.dt, a.xcg, a.fi, a.flags, &st);
        if constexpr (COST) J = cost_state_term(J + ju, x, a.w.q, ref);
      } else if constexpr (COST) {
        J += a.w.pen;
      }
      if (tr && --until_store == 0) {
        until_store = a.traj_every;
#pragma unroll
        for (int k = 0; k < 18; ++k) __builtin_nontemporal_store(x[k], tr + k * a.ld);
        tr += 18 * a.ld;
      }
      if constexpr (SCHED) if (ra.due(a, NR)) {
        ra.take(a, NR, LQR ? kq + 9 : u, a.out + b);
        if (LQR) { u[1] = u0[0]; u[2] = u0[1]; u[3] = u0[2]; }      // (as a new launch: u0 until it steps)
        if constexpr (COST) ju = cost_command_term(a, b0, u[1], u[2], u[3]);
      }
    }
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 18; ++k) finite = finite && isfinite(x[k]);
    if (!finite) st |= ST_NONFINITE;
    if (st & ST_ENVELOPE) st |= envelope_state_bits(x);
    if constexpr (COST) {
      a.out[b] = cost_state_term(J, x, a.w.qf, ref);
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
#pragma unroll
      for (int i = 0; i < 4; ++i) a.u_out[i * a.ld + b] = u[i];
    }
    if constexpr (GS) if (a.gs_out) a.gs_out[b] = gs_cnt;
  }
