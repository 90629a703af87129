// f16_mpc_wave_kernels.inc -- the two kernels of f16_mpc_wave.hip, included twice by it (inside namespace f16::wave, behind everything
// they use): with WAVE_SOFT 0 as k_mpc_wave / k_rollout_mpc<RELIN> (hard rows), with WAVE_SOFT 1 as k_mpc_wave_soft /
// k_rollout_mpc_soft<RELIN> (soft state rows, f16_mpc_plan_soft_rows: the weights are the second kernel argument).  WAVE_KERNEL names the
// kernel, WAVE_SOFT_PARAM is its extra parameter, WAVE_SOFT_ARGS what solve_aircraft<true> takes beyond solve_aircraft<false>.

// ---- one calc_MPC_action per aircraft (f16_mpc_batch / f16_mpc_plan_solve), aircraft from a work queue
__global__ __launch_bounds__(64, 1) void WAVE_KERNEL(k_mpc_wave)(MpcArgs a WAVE_SOFT_PARAM) {
  const int N = a.N;
  const Role R = role(N);
  const int l = R.l;
  for (long job = blockIdx.x;; ) {
  if (a.wave_queue) {
    unsigned q = 0;
    if (l == 0) q = atomicAdd(a.wave_queue, 1u);
    job = (long)(unsigned)__builtin_amdgcn_readfirstlane((int)q);
    if (job >= a.B) break;
    wave_lds_sync();                                         // (the previous aircraft's LDS traffic is over on every lane)
  }
#ifdef F16_EXP_STAMPW
  const unsigned long long wc0_ = wall_clock64();
  if (job == 0 && l == 0) g_stamp_wg = (int)blockIdx.x;
  unsigned long long tK0 = 0;
#endif
  // No order from a previous call (first call on this stream / batch size): NOT the caller's order either -- workgroup ids go to
  // the XCDs round-robin, and how hard an aircraft is tends to follow its index (the config-4 workload: every aircraft = 0, 3, 6
  // mod 8 needs twice the iterations), so the identity gives three XCDs twice the work of the others.  A fixed stride coprime to
  // B spreads any such pattern; the results do not depend on the map.
  const long b = a.order ? (long)__builtin_amdgcn_readfirstlane(a.order[job])
                         : (a.wave_stride ? (long)(((unsigned long long)job * a.wave_stride) % (unsigned long long)a.B) : job);
  if (mpc_job_nonfinite(a.ext, a.N, b)) {                             // (wave-uniform) no QP to solve: NaN command, zero iterations
    mpc_write_nonfinite(a.ucmd, a.useq, a.info, a.iters_out, a.status, a.ld, a.N, a.s.rho, b, l, 64);
    if (!a.wave_queue) break;
    continue;
  }
  SolveState st;
#if WAVE_SOFT
  bool soft_active = false;
#endif
#ifdef F16_EXP_STAMPW
  const bool ok = solve_aircraft<WAVE_SOFT != 0>(a, b, job, R, st, a.warm_load, tK0 WAVE_SOFT_ARGS);
#else
  const bool ok = solve_aircraft<WAVE_SOFT != 0>(a, b, job, R, st, a.warm_load WAVE_SOFT_ARGS);
#endif
  const int kx = 3 * R.istep;
  const bool converged = st.converged != 0, infeasible = st.infeasible != 0;
  // res.x[0:3] (env.py:424); OSQP hands back NaN for a problem it certifies infeasible
  if (R.act && R.par == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (R.istep == 0) a.ucmd[c * a.ld + b] = infeasible ? NAN : st.x[c];
      if (a.useq) a.useq[(kx + c) * a.ld + b] = infeasible ? NAN : st.x[c];
    }
  }
#ifdef F16_EXP_STAMPW
  if (job == 0 && l == 0 && a.useq) {      // diagnostic build: the stamps replace rows 60.. of this aircraft's u_seq column
    for (int i = 0; i < 8; ++i) a.useq[(60 + i) * a.ld + b] = (double)g_wstamp[i];
    a.useq[68 * a.ld + b] = (double)st.it;
    for (int i = 9; i < 16; ++i) a.useq[(60 + 12 + i - 9) * a.ld + b] = (double)g_wstamp[i];
    for (int i = 0; i < 8; ++i) a.useq[(80 + i) * a.ld + b] = (double)g_tstamp[i];
    a.useq[71 * a.ld + b] = (double)(__builtin_amdgcn_s_memtime() - tK0);
  }
#endif
  if (l == 0) {
#if WAVE_SOFT
    mpc_write_result(a.info, a.iters_out, a.status, a.ld, b, st.it, st.rp, st.rd, st.rho,
                     mpc_status_bits(converged, infeasible, ok, a.s.max_iter) | (soft_active && !infeasible ? F16_ST_QP_SOFT_ACTIVE : 0));
#else
    mpc_write_result(a.info, a.iters_out, a.status, a.ld, b, st.it, st.rp, st.rd, st.rho, mpc_status_bits(converged, infeasible, ok, a.s.max_iter));
#endif
#ifdef F16_EXP_STAMPW
    if (a.info) {
      a.info[1 * a.ld + b] = (double)wc0_;                 // diagnostic build: start / end of this solve on the 100 MHz clock
      a.info[2 * a.ld + b] = (double)wall_clock64();
      a.info[3 * a.ld + b] = (double)((__builtin_amdgcn_s_getreg(63508) & 15) * 65536 + (__builtin_amdgcn_s_getreg(63492) & 0xFFFF));    // XCC_ID | HW_ID: which SIMD
    }
#endif
  }
#ifdef F16_EXP_STAMPW
  if (job == 0 && l == 0) g_stamp_wg = -1;
#endif
  if (!a.wave_queue) break;
  }
}

// ---- the closed loops (f16_rollout_mpc*): (step, aircraft) pairs from a ticket counter; RELIN: the model re-derived per pair
template <bool RELIN>
__global__ __launch_bounds__(64, 1) void WAVE_KERNEL(k_rollout_mpc)(RollArgsOf<RELIN> kargs WAVE_SOFT_PARAM) {
  const RollMpcArgs &ra = rollout_args(kargs);
  const MpcArgs &a = ra.m;
  const int N = a.N;
  const Role R = role(N);
  const int l = R.l;
  const unsigned Bu = (unsigned)a.B;
#ifdef F16_DBG_PAIRSTAMP
  unsigned long long tp0_ = __builtin_amdgcn_s_memtime();
#endif
  for (;;) {
    unsigned k = 0;
    if (l == 0) k = atomicAdd(ra.queue, 1u);
    k = (unsigned)__builtin_amdgcn_readfirstlane((int)k);
    PSTAMP(0)
    DBGM(0, 1000 + k)
    if (k >= ra.total) break;
    const int t = __builtin_amdgcn_readfirstlane((int)(k / Bu));
    const unsigned j = k - (unsigned)t * Bu;
    const long b = (long)(unsigned)__builtin_amdgcn_readfirstlane((int)(ra.stride ? (unsigned)(((unsigned long long)j * ra.stride) % Bu) : j));
    // ---- wait for step t - 1 of this aircraft, then acquire what its wavefront published.  (Every lane polls the same word -- one
    // broadcast load -- and every lane publishes below: no lane-0-only region on either side of the loop's back edge.)
    // The wait is bounded (2^24 polls, tens of seconds -- the longest legitimate wait is one 40,000-iteration solve, ~0.1 s): a wave
    // that never sees its predecessor flags the aircraft (F16_ST_LOOP_STALL) and goes on, so that the grid drains whatever happens.
    int stall = 0;
    if (t > 0) {
      int polls = 0;
      while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&ra.progress[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < t) {
        __builtin_amdgcn_s_sleep(16);
        if (++polls > (1 << 24)) { stall = F16_ST_LOOP_STALL; break; }
      }
    }
    PSTAMP(1)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    PSTAMP(2)
    PairIO io;
    io.x = ra.x; io.u = ra.u; io.dem = ra.dem + (size_t)(t / ra.dem_hold) * 3 * a.ld; io.traj = ra.traj; io.cmd_traj = ra.cmd_traj; io.iters_traj = ra.iters_traj;
    io.status = ra.status; io.tab = ra.tab; io.lofi = ra.lofi; io.exw = a.ext + (size_t)b * mpc_ext_doubles(N);
    io.ld = a.ld; io.b = b; io.t = t; io.N = N; io.every = ra.every; io.fi = ra.fi; io.flags = ra.flags; io.xcg = ra.xcg; io.dt = a.dt;
    io.hold = ra.hold; io.dtp = ra.dtp;
    io.cmd[0] = NAN; io.cmd[1] = NAN; io.cmd[2] = NAN; io.iters = 0; io.stw = 0; io.stall = stall;
    DBGM(1, 2000 + t)
    int code;
    if constexpr (RELIN) {
      ModelIO mo;
      mo.Pg = a.Ppk + (size_t)b * (size_t)(3 * N * (3 * N + 1) / 2);
      mo.model = (kargs.model_traj && (t + 1) % kargs.model_every == 0) ? kargs.model_traj + (size_t)((t + 1) / kargs.model_every - 1) * MODEL_ROWS * a.ld + b : nullptr;
      mo.pb.Q = kargs.wq; mo.pb.R = kargs.wq + 81; mo.pb.Rinv = kargs.wq + 90; mo.pb.custom_q = a.pb.custom_q; mo.pb.custom_r = a.pb.custom_r; mo.eps = kargs.eps;
      code = __builtin_amdgcn_readfirstlane(pair_model(&io, &mo));
      if (code == PAIR_SOLVE) code = __builtin_amdgcn_readfirstlane(pair_prepare(&io));
    } else {
      code = __builtin_amdgcn_readfirstlane(pair_prepare(&io));
    }
    DBGM(2, 3000 + code)
    PSTAMP(3)
    if (code == PAIR_SOLVE) {
      SolveState st;
#if WAVE_SOFT
      bool soft_active = false;
#endif
#ifdef F16_DBG_SKIP_SOLVE      // (measurement build: what a pair costs WITHOUT its solve -- tools/gpu_config5_only.py under F16HIP_SO)
      st.infeasible = 0; st.converged = 1; st.it = 0; st.x[0] = -0.5; st.x[1] = 0.0; st.x[2] = 0.0;
      const bool ok = true;
#elif defined(F16_EXP_STAMPW)
      unsigned long long tK0 = 0;
      const bool ok = solve_aircraft<WAVE_SOFT != 0>(a, b, (long)k + 1, R, st, (t > 0 || a.warm_load) ? 1 : 0, tK0 WAVE_SOFT_ARGS);
#else
      // (warm start, opt-in: step 0 starts from the plan's previous call if there was one, every later step from the step before --
      //  the buffer is handed from wavefront to wavefront with the state, behind the same release / acquire)
      const bool ok = solve_aircraft<WAVE_SOFT != 0>(a, b, (long)k + 1, R, st, (t > 0 || a.warm_load) ? 1 : 0 WAVE_SOFT_ARGS);
#endif
      const bool infeasible = __builtin_amdgcn_readfirstlane(st.infeasible) != 0;
      const bool converged = __builtin_amdgcn_readfirstlane(st.converged) != 0;
      const double c0 = bcast0_f64(st.x[0]), c1 = bcast0_f64(st.x[1]), c2 = bcast0_f64(st.x[2]);      // res.x[0:3], env.py:424 (lane 0 owns step 0)
      io.iters = __builtin_amdgcn_readfirstlane(st.it);
      io.cmd[0] = infeasible ? NAN : c0; io.cmd[1] = infeasible ? NAN : c1; io.cmd[2] = infeasible ? NAN : c2;
      io.stw |= mpc_status_bits(converged, infeasible, uniform_flag(ok), a.s.max_iter);      // (OSQP hands back NaN for a problem it certifies infeasible)
#if WAVE_SOFT
      io.stw |= uniform_flag(soft_active) && !infeasible ? F16_ST_QP_SOFT_ACTIVE : 0;
#endif
      wave_lds_sync();
    }
    DBGM(3, 4000 + io.iters)
    PSTAMP(4)
    pair_finish(&io, code);
    PSTAMP(5)
    DBGM(4, 5000)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(&ra.progress[b], t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (64 lanes, one word, one value)
    PSTAMP(6)
    DBGM(5, 6000 + t)
  }
  DBGM(6, 7000)
}
