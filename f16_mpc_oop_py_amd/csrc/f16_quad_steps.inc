// f16_quad_steps.inc -- the step loop of k_rollout_q (f16_dynamics.hip), included there once per role and once for all roles.
// `wave` is defined by the including scope: a compile-time constant 0..4 in a role's own loop (GROUPS = 1: every `if (wave == ...)`
// below is resolved then, and that copy keeps the statements, the published states and the loop-carried registers of its role
// alone; 4 is the store wave, which reads the sample behind barrier A, stores it when one is due and does nothing else), the
// wave's role index 0..3 itself in the shared loop (GROUPS = 2, where wave 2 stores the samples).  Every copy executes the same
// barriers: A and B per step, A alone on the extra trip.  Text, not a function: the shared loop then compiles exactly as it did inside the kernel.
// GROUPS = 1, in front of a role's loop: the role's constants (QUAD_K, f16_plant.hpp) are loaded HERE, once per launch and group of
// aircraft, and stay in registers across the loop -- wave 2 and wave 0 the sin/cos table, wave 3 the exp / log table; no step
// loads them again.  Wave 0 evaluates the first step's psi with that table (the form of the loop: on a NaN psi the literal form
// differs in the sign of the NaN, and a continued rollout must give the bits of one launch).  Wave 2 publishes x[0..5] and tests
// x[2] for the first trip; from then on it does both where these states become final, behind barrier B (below).  Wave 3 evaluates
// the altitude part of the first step's atmosphere, the quotient of its log and the log's polynomial (atmos_alt, log_k_quot,
// log_k_poly) from the x[2] it loaded; from then on behind barrier B, from the altitude wave 2 hands over beside psi (xpsi[3]) -- half a step ahead of their use.
// GROUPS = 1, behind barrier A: a wave takes the states it owns from its registers, not from the published copy (wave 2 the angles
// of its sin / cos polynomial and the airspeed, wave 1 its P, Q, R).
    [[maybe_unused]] SinCosK ksc = {};
    [[maybe_unused]] PowK kpw = {};
    [[maybe_unused]] bool env_h = false;                   // wave 2: x[2] outside its box, tested where x[2] was last advanced
    [[maybe_unused]] AtmosAlt ah = {};                    // wave 3: the altitude part of the coming step's atmosphere (atmos_alt) ...
    [[maybe_unused]] LogQuot lq = {};                      //         ... and the quotient of log tfac (log_k_quot), taken half a step ahead
    [[maybe_unused]] LogPoly lp = {};                      //         ... and the log's polynomial in that quotient (log_k_poly), with it
    if constexpr (G1) {
      if (wave == 0 || wave == 2) ksc = reloaded(QUAD_K.sc);
      if (wave == 3) kpw = reloaded(QUAD_K.pw);
      // operand class (f16_plant.hpp): waves 0 and 3 keep the table in scalar registers (KScalar) and only the two Horner start
      // coefficients, vector operands of their FMA, in vector registers; wave 2's whole table stays in lane-uniform vector registers
      // (KVector: chosen when its loop had no scalar registers for 42 more; the scalar form since the sample left this wave: DESIGN.md)
      if (wave == 2) table_in_vgprs(ksc);
      if (wave == 0) { in_vgpr(ksc.S[7]); in_vgpr(ksc.C[8]); }
      if (wave == 3) { in_vgpr(kpw.E[0]); in_vgpr(kpw.L[0]); }
      if (wave == 0 && s == 0) {                           // sin / cos of the first step's psi (the loop's first barrier publishes it)
        double sp, cp;
        F16_SINCOS_K(ksc, x[5], &sp, &cp);
        xpsi[1][ac] = sp; xpsi[2][ac] = cp;
      }
      if (wave == 2) {
        env_h = envchk && (x[2] < 0 || x[2] > 100000);
        if (s == 0) {
#pragma unroll
          for (int k = 0; k < 6; ++k) xs[k][ac] = x[k];
        }
      }
      if (wave == 3) {                                     // the first step's altitude part, in the form of the loop (second half, below)
        ah = atmos_alt(x[2]);
        lq = log_k_quot(kpw, ah.tfac);
        lp = log_k_poly(kpw, lq);
        quad_taken_here(ah.tfac, ah.temp, ah.t4, lq.h, lq.l, lq.e, lp.z, lp.c);
      }
      // The states a role neither owns nor reads are dead from here on: the epilogue writes back a role's own states only, but it
      // stands behind the join of the four loops, where the compiler no longer knows the role, and kept all 18 in registers across
      // every role's loop.  (Wave 3's loop is left alone, and so are the commands and LQR rows it owns: clearing those for the other
      // roles moved two fp64 canonicalisations of wave 3's out of its loop -- the same values, but not the same instruction sequence.)
      if (wave != 3) {
#pragma unroll
        for (int k = 0; k < 18; ++k)
          if (!(wave == 2 ? k < 9 : (wave == 1 && k >= 9 && k < 12))) x[k] = 0;
      }
    }
    for (int t = 0; t <= a.nsteps; ++t) {                  // the extra trip only publishes + stores the final sample
      // ---- step start: envelope test on the owned states (env.py:117-124), publish them
      if (wave == 2) {
        if constexpr (G1) {
          // x[0..5] and the x[2] test were published behind barrier B of the last step (in front of the loop for the first trip):
          // what stands between the last Euler update and barrier A is x[6..8], one state per sub-lane (all four hold the same x), and the flag
          xenv[0][ac] = env_h | (envchk & ((x[6] < 0) | (x[6] > 900) | (x[7] < -20.) | (x[7] > 90) | (x[8] < -30.) | (x[8] > 30)));
          xs[6 + (s < 3 ? s : 2)][ac] = s == 0 ? x[6] : (s == 1 ? x[7] : x[8]);   // (sub-lanes 2 and 3 both write x[8]: no lane mask)
        } else {
          xenv[0][ac] = envchk && (x[2] < 0 || x[2] > 100000 || x[6] < 0 || x[6] > 900 || x[7] < -20. || x[7] > 90 ||
                                   x[8] < -30. || x[8] > 30);
          if (s == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) xs[k][ac] = x[k];
          }
        }
      } else if (wave == 1) {
        xenv[1][ac] = envchk && (x[9] < -300 || x[9] > 300 || x[10] < -100 || x[10] > 100 || x[11] < -50 || x[11] > 50);
        if (s < 3) xs[9 + s][ac] = s == 0 ? x[9] : (s == 1 ? x[10] : x[11]);
      } else if (wave == 3) {
        const double lim = s == 1 ? 25.0 : (s == 2 ? 21.5 : 30.0);
        const bool bad = s == 0 ? (xact < 1000 || xact > 19000) : (xact < -lim || xact > lim);
        const bool badl = x[16] < 0. || x[16] > 25;
        // any sub-lane out of range flags the aircraft: combine over the quad through LDS writes of `true` only
        if (s == 0) xenv[2][ac] = 0;
        xs[12 + s][ac] = xact;
        if (s < 2) xs[16 + s][ac] = s == 0 ? x[16] : x[17];
        __builtin_amdgcn_wave_barrier();
        if (envchk && (bad || badl)) xenv[2][ac] = 1;
      }
      QSTAMP(tD)
      __syncthreads();
      QSTAMP(tA)
      // trajectory sample of the step that just finished: all 18 states straight from the published copy (sub-lane s stores states
      // s, s+4, s+8, ...) -- GROUPS = 2 by wave 2, GROUPS = 1 by the store wave (4), which owns tr, until_store and sample_due
      // GROUPS = 1: a wave takes the states it owns from its registers (xs[k] is a copy of x[k], for a frozen aircraft and on the
      // first trip too) -- wave 2 x[3], x[4], x[6..8], so that its sin / cos polynomial starts without an LDS round trip, wave 1 its
      // P, Q, R -- and reads the rest from the published copy.  The store wave issues the sample's five reads behind barrier A,
      // every trip (fenced there, or the compiler moves them into the branch that stores them and splits them round the first four
      // stores: a second round trip); they have landed before barrier B, behind which wave 2 rewrites x[0..5].  On the extra trip the
      // sample is stored on the way out of the loop.
      double xa[17];
      int env_any = 0;
      if constexpr (G1) {
        env_any = xenv[0][ac] | xenv[1][ac] | xenv[2][ac];
#pragma unroll
        for (int k = 0; k < 17; ++k) xa[k] = xs[k][ac];
        if (wave == 2) { xa[3] = x[3]; xa[4] = x[4]; xa[6] = x[6]; xa[7] = x[7]; xa[8] = x[8]; }
        if (wave == 1) { xa[9] = x[9]; xa[10] = x[10]; xa[11] = x[11]; }
      }
      [[maybe_unused]] double smp[5] = {0, 0, 0, 0, 0};    // GROUPS = 1, store wave: read behind barrier A, whether or not a sample is due
      [[maybe_unused]] bool sample_due = false;
      if constexpr (G1) {
        if (wave == 4) {
#pragma unroll
          for (int j = 0; j < 5; ++j) smp[j] = xs[s + 4 * j < 18 ? s + 4 * j : s][ac];
          asm volatile("" ::: "memory");                   // (read HERE: no load moves behind this, into the branch that stores them)
        }
      }
      if (wave == (G1 ? 4 : 2) && tr && t > 0 && --until_store == 0) {
        until_store = a.traj_every;
        if constexpr (G1) {
          sample_due = true;                               // (stored in the store wave's first half below, on the extra trip on the way out)
        } else {
          if (valid) {
#pragma unroll
            for (int j = 0; j < 5; ++j) {
              const int kk = s + 4 * j;
              if (kk < 18) __builtin_nontemporal_store(xs[kk][ac], tr + kk * a.ld);
            }
          }
          tr += 18 * a.ld;
        }
      }
      if (t == a.nsteps) {
        if constexpr (G1) {
          if (sample_due && valid) quad_store_sample(smp, tr, s, a.ld);
        }
        break;
      }
      if constexpr (!G1) {
        env_any = xenv[0][ac] | xenv[1][ac] | xenv[2][ac];
#pragma unroll
        for (int k = 0; k < 17; ++k) xa[k] = xs[k][ac];
      }
      // (a wave 0 with a loop of its own reads no flag: it reports no status; nor does the store wave)
      if ((!G1 || (wave != 0 && wave != 4)) && env_any) st |= ST_ENVELOPE;
      const bool live = !(st & ST_ENVELOPE);
      // first-half results wave 2 keeps in registers for the second half
      double xd[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      double U = 0, V = 0, W = 0, s_t = 0, c_t = 0, s_phi = 0, c_phi = 0, cb = 0, vtc = 0, r1 = 0, r2 = 0, r3 = 0;
      double fu0 = 0, fv0 = 0, fw0 = 0, mo0 = 0, mo1 = 0, mo2 = 0;
      bool newrow = false;
      if constexpr (SCHED) newrow = ra.due(a, LQR ? 3 : 4);
      if (wave == 0) {
        int sa_ = 0;
        double latd;
        const double tot = quad_long<G1>((const double *)tab, xa, s, a.xcg, a.flags, qc, klong, latd, sa_);
        if (s < 3) { xt[s][ac] = tot; xt[8 + s][ac] = latd; }
        xst[0][ac] = sa_;
      } else if (wave == 1) {
        int sa_ = 0;
        const double tot = quad_lat<G1>((const double *)tab, xa, s, a.flags, qc, klat, sa_);
        if (s < 3) xt[3 + s][ac] = tot;
        xst[1][ac] = sa_;
        {   // the rate-product terms of the moment equations (C/nlplant.c:413-436, Heng = 0) do not need the totals: first half
          const double Jy = 55814.0, Jxz = 982.0, Jz = 63100.0, Jx = 9496.0;
          const double rden = 1.0 / (9496.0 * 63100.0 - 982.0 * 982.0);
          const double P = x[9], Q = x[10], R = x[11];
          mo0 = (Jxz * (Jx - Jy + Jz) * P * Q - (Jz * (Jz - Jy) + Jxz * Jxz) * Q * R) * rden;
          mo1 = F16_DIVC((Jz - Jx) * P * R - Jxz * (P * P - R * R), Jy);
          mo2 = ((Jx * (Jx - Jy) + Jxz * Jxz) * P * Q - Jxz * (Jx - Jy + Jz) * Q * R) * rden;
        }
        if constexpr (G1) quad_taken_here(mo0, mo1, mo2);  // (as on wave 2 below: first-half work stays in the first half)
      } else if (wave == 2) {
        // sin / cos of phi, theta, beta, alpha: one angle per sub-lane, then shared across the quad; psi's from wave 0
        // (GROUPS = 2: psi on sub-lane 2, beta in a round of its own on every lane)
        double ang;
        if constexpr (G1) {                                // (from registers: one select behind the other, or the compiler branches round them)
          ang = xa[7];
          ang = s == 2 ? xa[8] : ang;
          ang = s == 1 ? xa[4] : ang;
          ang = s == 0 ? xa[3] : ang;
        } else
          ang = s == 0 ? xa[3] : (s == 1 ? xa[4] : (s == 2 ? xa[5] : xa[7]));
        double sn, cs, sb, s_psi, c_psi;
        if constexpr (G1) F16_SINCOS_KC(KVector, ksc, ang, &sn, &cs);   // (the table loaded in front of the loop, into vector registers)
        else F16_SINCOS(ang, &sn, &cs);
        // (keep this statement order: the FMA contraction of the navigation sums below follows it, and another order
        //  changes x[1] in the last place)
        if constexpr (G1) { sb = quad_bcast<2>(sn); cb = quad_bcast<2>(cs); } else F16_SINCOS(xa[8], &sb, &cb);
        s_phi = quad_bcast<0>(sn); c_phi = quad_bcast<0>(cs);
        s_t = quad_bcast<1>(sn); c_t = quad_bcast<1>(cs);
        if constexpr (G1) { s_psi = xpsi[1][ac]; c_psi = xpsi[2][ac]; } else { s_psi = quad_bcast<2>(sn); c_psi = quad_bcast<2>(cs); }
        const double sal = quad_bcast<3>(sn), cal = quad_bcast<3>(cs);
        vtc = xa[6];
        if (vtc <= 0.01) vtc = 0.01;
        U = vtc * cal * cb; V = vtc * sb; W = vtc * sal * cb;                       // C/nlplant.c:148-150
        const double P = xa[9], Q = xa[10], R = xa[11];
#ifdef F16_FAST_DIV
        const double rct = f16_rcp(c_t);
        const double tt = s_t * rct;
#elif defined(F16_FAST_TAN)
        const double rct = 0.0, tt = s_t / c_t;
#else
        const double rct = 0.0, tt = tan(xa[4]);
#endif
        xd[0] = U * (c_t * c_psi) + V * (s_phi * c_psi * s_t - c_phi * s_psi) + W * (c_phi * s_t * c_psi + s_phi * s_psi);
        xd[1] = U * (c_t * s_psi) + V * (s_phi * s_psi * s_t + c_phi * c_psi) + W * (c_phi * s_t * s_psi - s_phi * c_psi);
        xd[2] = U * s_t - V * (s_phi * c_t) - W * (c_phi * c_t);
        xd[3] = P + tt * (Q * s_phi + R * c_phi);                                     // :169-176
        xd[4] = Q * c_phi - R * s_phi;
#ifdef F16_FAST_DIV
        xd[5] = (Q * s_phi + R * c_phi) * rct;
        r1 = f16_rcp(vtc); r2 = f16_rcp(U * U + W * W); r3 = f16_rcp(vtc * vtc * cb);   // divisors of :393-405, hoisted
#else
        xd[5] = (Q * s_phi + R * c_phi) / c_t;
        (void)rct;
#endif
        // this wave has slack in the first half and sets the pace of the second: what the force equations and the Euler
        // update do not need the coefficient totals for is done here (same expressions, :383-387 regrouped)
        {
          const double g = 32.17, m = 636.94;
          fu0 = R * V - Q * W - g * s_t + F16_DIVC(xa[12], m);
          fv0 = P * W - R * U + g * c_t * s_phi;
          fw0 = Q * U - P * V + g * c_t * c_phi;
          if (live) {
#pragma unroll
            for (int k = 0; k < 6; ++k) x[k] += xd[k] * a.dt;   // env.py:126 (navigation / kinematic states)
          }
          // wave 0 evaluates psi's sin / cos in the second half, wave 3 the altitude part of the next step's atmosphere (a frozen
          // aircraft hands over the values it was frozen with; not through xs[2], which is still being read in this half)
          if constexpr (G1) if (s == 0) { xpsi[0][ac] = x[5]; xpsi[3][ac] = x[2]; }
        }
        // (in a loop of its own a role's two halves are one piece of code: left alone, the compiler moves what only the second
        //  half uses -- the three reciprocals, fu0 .. fw0 -- behind barrier B, into the half this wave sets the pace of, and
        //  contracts it with the force equations there: other last bits)
        if constexpr (G1) quad_taken_here(U, V, W, vtc, r1, r2, r3, fu0, fv0, fw0);
      } else if (G1 && wave == 4) {
        // the store wave: the sample it read behind barrier A, and nothing else up to barrier B
        if (sample_due) {
          if (valid) quad_store_sample(smp, tr, s, a.ld);
          tr += 18 * a.ld;
        }
      } else {
        double vt = xa[6];
        if (vt <= 0.01) vt = 0.01;
        double mach, qbar, ps;
        double pw = 0;                                     // GROUPS = 1: exp(POW_FRAC log tfac) of this altitude, shared with the flap model
        if constexpr (G1) {
          // the altitude part (ah) and the quotient of the log (lq) were evaluated behind barrier B of the last step: what is left
          // needs no LDS read up to the density and runs under the wait for x[6], x[7]; only qbar takes this step's airspeed.
          // (pinned behind barrier A too: the compiler moved the rest of the chain in front of it, into the half wave 3 then paced)
          quad_taken_here(ah.tfac, lq.h, lq.l, lq.e, lp.z, lp.c);
          pw = exp_k(kpw, POW_FRAC * log_k_tail(kpw, ah.tfac, lq, lp));   // (the table loaded in front of the loop)
          atmos_air(ah, vt, mach, qbar, ps, [pw](double) { return pw; });
        } else
          atmos_dev(xa[2], vt, mach, qbar, ps);
        if (s == 0) { xt[6][ac] = qbar; xt[7][ac] = ps; }
        if (live) {
          // utils.py:308-330: thrust on sub-lane 0, elevator / aileron / rudder on 1..3 (same form, own limits)
          const double lim = s == 1 ? 25.0 : (s == 2 ? 21.5 : 30.0), rate = s == 1 ? 60.0 : (s == 2 ? 80.0 : 120.0);
          double uc = ucmd;
          if (LQR) {
            if constexpr (SCHED) { dm0 = quad_bcast<0>(dmq); dm1 = quad_bcast<1>(dmq); dm2 = quad_bcast<2>(dmq); }   // (live is the same over a quad)
            const double ua = lqr_action(kr0, kr1, kr2, dm0 - xa[9], dm1 - xa[10], dm2 - xa[11], ucmd);
            uc = s > 0 ? ua : ucmd;
            ulast = uc;
          }
          const double dth = actuator_rate(ucmd, 1000, 19000, 1.0, xact, 10000);
          const double dsf = actuator_rate(uc, -lim, lim, 20.2, xact, rate);
          double lf1_dot, lf2_dot;
          if constexpr (G1)
            upd_lef_with(0.0, xa[6], xa[7], x[17], x[16], qbar, ps, lf1_dot, lf2_dot,
                         [pw, &ah](double, double V_, double &m_, double &q_, double &p_) {    // (the step's altitude part and factor)
                           atmos_air(ah, V_, m_, q_, p_, [pw](double) { return pw; });
                         });
          else
            upd_lef_dev(xa[2], xa[6], xa[7], x[17], x[16], qbar, ps, lf1_dot, lf2_dot);
          xact += (s == 0 ? dth : dsf) * a.dt;             // env.py:126 on the actuator / flap states
          x[16] += lf2_dot * a.dt;
          x[17] += lf1_dot * a.dt;
        }
        if constexpr (SCHED) if (newrow) {
          // (the sub-lane from the lane number, inside this branch: neither a register kept through the step for it nor -- GROUPS = 2
          //  spills -- a scratch reload in front of the load; volatile so that it is not hoisted out again)
          int rv;
          asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(rv));
          rv &= 3;
          if (LQR && rv == 3) rv = 2;
          ra.take(a, LQR ? 3 : 4, LQR ? &dmq : &ucmd, a.out + b, rv * a.ld);
          if (LQR) ulast = ucmd;                          // (as a new launch: u0 until it steps)
        }
      }
      QSTAMP(tB)
      __syncthreads();
      QSTAMP(tC)
      // ---- second half: force equations on wave 2 || moment equations on wave 1
      if (wave == 2) {
        int sx = 0;                                        // the table waves' status bits and the totals this wave uses, as read from LDS
        double t0_ = 0, t1_ = 0, t3_ = 0, t8_ = 0, t6_ = 0;
        if constexpr (G1) {
          // x[0..5] were advanced in the first half and are final: publish them and test x[2] HERE, under the wait for the totals,
          // not behind the second half.  Nobody reads xs between barrier B and the next barrier A -- the step inputs and the sample
          // are read behind A, the second halves read xt / xst (waves 1, 2) and xpsi (wave 0) -- and every read of the first half
          // has landed before B.  A frozen aircraft publishes the values it was frozen with.
          // The second half's own reads are issued first (whether or not the aircraft is live), the six writes behind them: the
          // writes take issue slots under the wait for the reads.
          sx = xst[0][ac] | xst[1][ac];
          t0_ = xt[0][ac]; t1_ = xt[1][ac]; t3_ = xt[3][ac]; t8_ = xt[8][ac]; t6_ = xt[6][ac];
          __builtin_amdgcn_sched_barrier(0);               // every read above, every write below
          env_h = envchk & ((x[2] < 0) | (x[2] > 100000));   // (no short cut: two compares cost less than a jump round them)
          if (s == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) xs[k][ac] = x[k];
          }
        }
        if (live) {
          if constexpr (!G1) { sx = xst[0][ac] | xst[1][ac]; t0_ = xt[0][ac]; t1_ = xt[1][ac]; t3_ = xt[3][ac]; t8_ = xt[8][ac]; t6_ = xt[6][ac]; }
          st |= sx;
          const double Cx = t0_, Cz = t1_, Cy = t3_ + t8_, qbar = t6_;
          const double m = 636.94, S = 300.0;
          const double qsm = F16_DIVC(qbar * S, m);
          const double Udot = fu0 + qsm * Cx;                                                          // :383-387
          const double Vdot = fv0 + qsm * Cy;
          const double Wdot = fw0 + qsm * Cz;
#ifdef F16_FAST_DIV
          xd[6] = (U * Udot + V * Vdot + W * Wdot) * r1;                                                 // :393-405
          xd[7] = (U * Wdot - W * Udot) * r2;
          xd[8] = (Vdot * vtc - V * xd[6]) * r3;
#else
          xd[6] = (U * Udot + V * Vdot + W * Wdot) / vtc;
          xd[7] = (U * Wdot - W * Udot) / (U * U + W * W);
          xd[8] = (Vdot * vtc - V * xd[6]) / (vtc * vtc * cb);
#endif
#pragma unroll
          for (int k = 6; k < 9; ++k) x[k] += xd[k] * a.dt;   // env.py:126 (x[0..5] were advanced in the first half)
        }
      } else if (wave == 1) {
        if (live) {
          const double Cy = xt[3][ac] + xt[8][ac];
          const double Cn = xt[4][ac] + xt[9][ac] - Cy * (0.35 - a.xcg) * (11.32 / 30.0);   // C/nlplant.c:367
          const double Cl = xt[5][ac] + xt[10][ac];
          const double Jy = 55814.0, Jxz = 982.0, Jz = 63100.0, Jx = 9496.0, S = 300.0;
          const double rden = 1.0 / (9496.0 * 63100.0 - 982.0 * 982.0);
          const double qs = xt[6][ac] * S;
          const double L_tot = Cl * qs * 30.0, M_tot = xt[2][ac] * qs * 11.32, N_tot = Cn * qs * 30.0;   // :413-415
          x[9] += (mo0 + (Jz * L_tot + Jxz * N_tot) * rden) * a.dt;                                  // :417-436 + env.py:126
          x[10] += (mo1 + F16_DIVC(M_tot, Jy)) * a.dt;
          x[11] += (mo2 + (Jx * N_tot + Jxz * L_tot) * rden) * a.dt;
        }
      } else if constexpr (G1) {
        if (wave == 0 && s == 0) {                         // sin / cos of the next step's psi, off wave 2's first half
          double sp, cp;
          F16_SINCOS_K(ksc, xpsi[0][ac], &sp, &cp);
          xpsi[1][ac] = sp; xpsi[2][ac] = cp;
        } else if (wave == 3) {
          // the altitude part of the next step's atmosphere, off wave 3's first half: x[2] is final since wave 2's first half
          // (the extra trip evaluates a log nobody uses).  Pinned here: what crosses barrier A is three values, not the chain.
          ah = atmos_alt(xpsi[3][ac]);
          lq = log_k_quot(kpw, ah.tfac);
          lp = log_k_poly(kpw, lq);                        // (the log's polynomial needs the quotient alone: with it, in the half with slack)
          quad_taken_here(ah.tfac, ah.temp, ah.t4, lq.h, lq.l, lq.e, lp.z, lp.c);
        }
      }
    }
