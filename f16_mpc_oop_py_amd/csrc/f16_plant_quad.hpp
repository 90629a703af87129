// f16_plant_quad.hpp -- the hifi aerodynamic build-up with FOUR lanes per aircraft (used by k_rollout_q).
//
// At the reference's batch of 4096 there are fewer aircraft than SIMD lanes on the chip, so a rollout step is bound by
// how many wave-instructions ONE aircraft group needs, not by throughput.  Here a quad of lanes (l = 4 a + s) shares an
// aircraft and sub-lane s evaluates ONE member of each coefficient family -- the node-major table image keeps the
// members of a family next to each other, so the sub-lanes run the same instructions on payload offset s:
//     longitudinal wave   s = 0,1,2  ->  Cx, Cz, Cm      (C/nlplant.c:333-347)
//     lateral wave        s = 0,1,2  ->  Cy, Cn, Cl      (C/nlplant.c:353-377)
// (sub-lane 3 shadows sub-lane 2).  Same terms as aero_totals_phased(), hifi_F16_AeroData.c:1871-1934; the
// cg-offset couplings (Cm needs Cz_tot, Cn needs Cy_tot) cross the quad with one DPP broadcast.
#pragma once
#include "f16_plant.hpp"

namespace f16 {

// value of sub-lane J of this lane's quad
template <int J>
F16_DEV double quad_bcast(double v) {
  constexpr int ctrl = J | (J << 2) | (J << 4) | (J << 6);      // quad_perm:[J,J,J,J]
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, ctrl, 0xF, 0xF, true);
  hi = __builtin_amdgcn_mov_dpp(hi, ctrl, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

template <int J>
F16_DEV int quad_bcast_i(int v) {
  constexpr int ctrl = J | (J << 2) | (J << 4) | (J << 6);
  return __builtin_amdgcn_mov_dpp(v, ctrl, 0xF, 0xF, true);
}

// The values are computed where this call stands: the compiler may neither move the arithmetic that forms them behind it nor
// fuse it with their later uses (an empty statement that claims to rewrite each of them in its vector registers).
F16_DEV void quad_taken_here_1(double &v) { asm volatile("" : "+v"(v)); }
F16_DEV void quad_taken_here_1(int &v) { asm volatile("" : "+v"(v)); }
template <typename... T>
F16_DEV void quad_taken_here(T &...v) { (quad_taken_here_1(v), ...); }

// One trajectory sample from the five values sub-lane s read of the published state (states s, s + 4, s + 8, ...; the fifth only
// on sub-lanes 0 and 1) to tr + k ld.
F16_DEV void quad_store_sample(const double (&smp)[5], double *tr, int s, long ld) {
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int kk = s + 4 * j;
    if (kk < 18) __builtin_nontemporal_store(smp[j], tr + kk * ld);
  }
}

// The three axis brackets of a role, ONE PER SUB-LANE (0: alpha on ALPHA1, 1: beta, 2/3: elevator on DH1 or DH2), shared
// across the quad by DPP broadcasts: first the cell indices (the table addresses need nothing else), later lambda.
// l: the lane's own lambda where the cell cache forms it with the cell (quad_br_cached, F16_FAST_DIV), else unused
struct QuadBr { BrCell c; int ja, jb, jd; bool offa, offb, offd; double l; };
template <bool USE_D2, typename TP>
F16_DEV BrRaw quad_br_load(TP T, double alpha, double beta, double el, int s, int &nX, double &vX) {
  const int ax = s < 2 ? s : 2;
  const int gel = USE_D2 ? (int)(el >= 0.0) : (el >= -10.0) + (el >= 0.0) + (el >= 10.0);
  const int offX = ax == 0 ? OFF_BP_A1 : (ax == 1 ? OFF_BP_B1 : (USE_D2 ? OFF_BP_D2 : OFF_BP_D1));
  nX = ax == 0 ? N_A1 : (ax == 1 ? N_B1 : (USE_D2 ? N_D2 : N_D1));
  vX = ax == 0 ? alpha : (ax == 1 ? beta : el);
  const int gX = ax == 0 ? alpha_guess(alpha) : (ax == 1 ? beta_guess(beta) : gel);
  return br_load(T + offX, nX, gX);
}
F16_DEV QuadBr quad_br_cells(const BrRaw &r, int nX, double vX) {
  QuadBr q;
  q.l = 0;
  bool off;
  q.c = br_cell(r, nX, vX, off);
  q.ja = quad_bcast_i<0>(q.c.j); q.jb = quad_bcast_i<1>(q.c.j); q.jd = quad_bcast_i<2>(q.c.j);
  const int o = off ? 1 : 0;
  q.offa = quad_bcast_i<0>(o) != 0; q.offb = quad_bcast_i<1>(o) != 0; q.offd = quad_bcast_i<2>(o) != 0;
  return q;
}

// Cell re-use across steps.  At dt = 1 ms an axis value almost never leaves its cell, so each lane keeps the cell of its
// own axis ([x0, x1)) and the quad's three cell indices from the last full lookup.  If every lane of the wave is still
// inside its cell (x0 <= v < x1 -- NaN, off-grid values and a value on the last node all fail it) the wave skips the
// breakpoint reads, the fix-up and the broadcasts; br_axis then sees the same v, x0, x1 and lambda has the same bits.  The
// cell is unique for an on-grid v < x1, so the full path could not have picked another one.  x0 = NaN: no cell yet.
// `hit` tells the caller which path was taken (the same for the whole wave): on a hit the cell indices are last step's, so
// every table address is last step's too, and the role keeps the values it read then (LongCorners / LatCorners below).
// What the cell fixes stays with the cell: rw, the refined reciprocal of its width (F16_FAST_DIV: the f16_rcp of br_axis, taken
// on the miss path where x0 and x1 are read).  On a hit lambda = (v - x0) * rw: the same product as br_axis's, without its
// `v == x1` guard, which a hit (v < x1) cannot meet; the miss path keeps the guard.  The strict build divides, in br_axis.
struct QuadCell { int ja, jb, jd; double x0, x1, rw; };
F16_DEV QuadCell quad_cell_none() { QuadCell c; c.ja = c.jb = c.jd = 0; c.x0 = c.x1 = __builtin_nan(""); c.rw = 0; return c; }
template <bool USE_D2, bool CACHE, typename TP>
F16_DEV QuadBr quad_br_cached(TP T, double alpha, double beta, double el, int s, unsigned flags, QuadCell &cc, bool &hit) {
  const double v = s == 0 ? alpha : (s == 1 ? beta : el);
  QuadBr q;
  q.l = 0;
  if constexpr (CACHE) {
    // every lane inside its cell: the two compares' lane masks themselves (all 64 lanes are live here: a ragged tail shadows)
    // F16_FLAG_NO_CELL_CACHE clears the mask (uniform over the launch): one scalar compare decides, wave-uniform
    const unsigned long long keep = (flags & FLAG_NO_CELL_CACHE) ? 0ull : ~0ull;
    const auto inside = __builtin_amdgcn_ballot_w64(cc.x0 <= v) & __builtin_amdgcn_ballot_w64(v < cc.x1) & keep;
    hit = inside == __builtin_amdgcn_ballot_w64(true);
  } else
    hit = false;
  if (hit) {
    q.c.j = 0; q.c.v = v; q.c.x0 = cc.x0; q.c.x1 = cc.x1;                          // (br_axis's j is not used by the quads)
    q.ja = cc.ja; q.jb = cc.jb; q.jd = cc.jd;
    q.offa = q.offb = q.offd = false;
#ifdef F16_FAST_DIV
    q.l = (v - cc.x0) * cc.rw;
#endif
  } else {
    int nX; double vX;
    const BrRaw rx = quad_br_load<USE_D2>(T, alpha, beta, el, s, nX, vX);
    F16_PHASE();
    q = quad_br_cells(rx, nX, vX);
    if (CACHE) {
      cc.ja = q.ja; cc.jb = q.jb; cc.jd = q.jd; cc.x0 = q.c.x0; cc.x1 = q.c.x1;
#ifdef F16_FAST_DIV
      cc.rw = f16_rcp(q.c.x1 - q.c.x0);
      q.l = q.c.v == q.c.x1 ? 1.0 : (q.c.v - q.c.x0) * cc.rw;                   // (br_axis, with the reciprocal kept)
#endif
    }
  }
  return q;
}
template <bool CACHE>
F16_DEV void quad_br_axes(const QuadBr &q, Axis &a, Axis &b, Axis &d) {
  Axis own;
#ifdef F16_FAST_DIV
  if constexpr (CACHE) {
    own.j = q.c.j; own.l = q.l;
    quad_taken_here(own.l);       // (rounded as br_axis rounds it behind its select: without the guard `1 - l` would fuse with the hit's product)
    own.m = 1 - own.l;
  } else
    own = br_axis(q.c);
#else
  own = br_axis(q.c);                                             // one division per lane
#endif
  a.j = q.ja; a.l = quad_bcast<0>(own.l); a.m = quad_bcast<0>(own.m);
  b.j = q.jb; b.l = quad_bcast<1>(own.l); b.m = quad_bcast<1>(own.m);
  d.j = q.jd; d.l = quad_bcast<2>(own.l); d.m = quad_bcast<2>(own.m);
}

// Table values a role read at its last full lookup, carried across steps beside its QuadCell (CACHE only): while the wave
// stays in its cells it neither forms the table addresses nor reads LDS -- phase (2) of quad_long / quad_lat runs on a
// miss alone, phase (3) reads these.  Zero until the first lookup, which is always a miss (QuadCell starts with x0 = NaN).
struct LongCorners {
  Q4 qlo, qhi, q0, qlef;
  double g0, g1, m0, m1, h0, h1, e0, e1, r0, r1, p0, p1, b0, b1, hr0, hr1, hp0, hp1, a45;
};
struct LatCorners {
  Q4 qlo, qhi, q0, qy, qr, qa, ql, qal;
  double a45;
};

// lerp() across the elevator axis of a 3-D table, both of whose operands are sums of products themselves: `l f2 + m f1` may be
// contracted from either side, and with the corners held in registers the compiler picks the other one.  PIN states the
// choice it made while they were loaded in front of the arithmetic (l f2 fused, m f1 rounded on its own), so that no bit moves.
// Every other lerp / bil4w of phase (3) is still left to -ffp-contract=fast and can flip the same way under another compiler:
// fixture G16 (tests/test_gpu_rollout_cell_cache.py, test_quad_rollout_matches_the_recorded_kernel_bit_for_bit) is the guard.
template <bool PIN>
F16_DEV double lerp_d(double f1, double f2, const Axis &a) {
  if constexpr (PIN) return __builtin_fma(a.l, f2, a.m * f1);
  else return lerp(f1, f2, a);
}

struct QuadIn {            // what both aerodynamic waves derive from the published state (C/nlplant.c:84-125)
  double alpha, beta, el, dail, drud, dlef, P, Q, R, kq, kb;
};
F16_DEV QuadIn quad_inputs(const double *xu) {
  const double B = 30.0, cbar = 11.32, r2d = 180.0 / 3.141592653589793;
  QuadIn in;
  double vt = xu[6];
  if (vt <= 0.01) vt = 0.01;
  in.alpha = xu[7] * r2d; in.beta = xu[8] * r2d;
  in.P = xu[9]; in.Q = xu[10]; in.R = xu[11];
  in.el = xu[13];
  in.dail = F16_DIVC(xu[14], 21.5);
  in.drud = F16_DIVC(xu[15], 30.0);
  in.dlef = 1 - F16_DIVC(xu[16], 25.0);
#ifdef F16_FAST_DIV
  const double r2vt = f16_rcp(2 * vt);
  in.kq = cbar * r2vt; in.kb = B * r2vt;
#else
  in.kq = cbar / (2 * vt); in.kb = B / (2 * vt);
#endif
  return in;
}

// Cx_tot / Cz_tot / Cm_tot on sub-lanes 0 / 1 / 2 (C/nlplant.c:333-347, hifi_C, hifi_damping, hifi_C_lef,
// hifi_damping_lef, hifi_other_coeffs).  dZdQ uses delta_Cz_lef exactly as the reference does (:339).
// latd: the rate-damping part of the LATERAL member k (Cy, Cn, Cl) -- 1-D tables on the same alpha cell, evaluated here
// to balance the two aerodynamic waves: kb (Cr + dCr_lef dlef) R + kb (Cp + dCp_lef dlef) P (+ dC_beta beta), :353-377.
#ifdef F16_EXP_STAMPQ2      // diagnostic build: cycles per phase of the longitudinal role (workgroup 0), tools/gpu_dyn_stamps2.py
__device__ unsigned long long g_qstamp[8];
#define Q2STAMP(i) { __builtin_amdgcn_s_waitcnt(0); const unsigned long long t1_ = __builtin_amdgcn_s_memtime(); if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) g_qstamp[i] += t1_ - tq_; tq_ = t1_; }
#else
#define Q2STAMP(i)
#endif
template <bool CACHE, typename TP>
F16_DEV double quad_long(TP T, const double *xu, int s, double xcg, unsigned flags, QuadCell &cc, LongCorners &kept, double &latd,
                         int &status) {
#ifdef F16_EXP_STAMPQ2
  unsigned long long tq_ = __builtin_amdgcn_s_memtime();
#endif
  const QuadIn in = quad_inputs(xu);
  Q2STAMP(0)
  const int k = s < 2 ? s : 2;
  // (1) breakpoints and cells: one axis per sub-lane (re-used from the last step while every lane stays in its cell)
  bool hit;
  const QuadBr qb = quad_br_cached<false, CACHE>(T, in.alpha, in.beta, in.el, s, flags, cc, hit);
  Q2STAMP(1)
  LongCorners fresh;
  LongCorners &c = CACHE ? kept : fresh;
  const bool hi_a = qb.ja > N_A2 - 2;                            // ALPHA2 ends at 45 deg: last cell, lambda = 1
  if (!CACHE || !hit) {
    c.a45 = T[OFF_BP_A1 + N_A2 - 1];
    const int j2 = hi_a ? N_A2 - 2 : qb.ja;
    const int n1 = qb.jb * N_A1 + qb.ja, n2 = qb.jb * N_A2 + j2;
    struct { int j; } ca = {qb.ja}, cd = {qb.jd};
    // (2) every table corner this role needs
    constexpr int SA = S_G3A, SB = S_G3A * N_A1, SD = S_G3A * N_A1 * N_B1;
    TP p = T + OFF_G3A + n1 * SA + k;
    c.qlo = ld4(p + cd.j * SD, SA, SB); c.qhi = ld4(p + (cd.j + 1) * SD, SA, SB); c.q0 = ld4(p + D1_ZERO_NODE * SD, SA, SB);
    c.qlef = ld4(T + OFF_G2B + n2 * S_G2B + k, S_G2B, S_G2B * N_A2);
    TP g = T + OFF_G1A + ca.j * S_G1A, h = T + OFF_G1B + j2 * S_G1B;
    c.g0 = g[3 * k]; c.g1 = g[S_G1A + 3 * k]; c.m0 = g[11]; c.m1 = g[S_G1A + 11];
    c.h0 = h[3 * k]; c.h1 = h[S_G1B + 3 * k];
    c.e0 = T[OFF_ETA + cd.j]; c.e1 = T[OFF_ETA + cd.j + 1];
    const int ir = k == 0 ? 1 : (k == 1 ? 7 : 4), ib = k == 1 ? 9 : 10;     // CYr CYp | CNr CNp | CLr CLp; dCNbeta, dCLbeta
    c.r0 = g[ir]; c.r1 = g[S_G1A + ir]; c.p0 = g[ir + 1]; c.p1 = g[S_G1A + ir + 1]; c.b0 = g[ib]; c.b1 = g[S_G1A + ib];
    c.hr0 = h[ir]; c.hr1 = h[S_G1B + ir]; c.hp0 = h[ir + 1]; c.hp1 = h[S_G1B + ir + 1];
    // (the off-grid bits with the lookup that finds them: a hit has every lane inside its cell, on the grid)
    if (qb.offa) status |= ST_ALPHA1 | ST_ALPHA2;
    if (qb.offb) status |= ST_BETA;
    if (qb.offd) status |= ST_EL;
  }
  if (hi_a && in.alpha > c.a45) status |= ST_ALPHA2;
  Q2STAMP(2)
  F16_PHASE();
  // (3) arithmetic
  Axis a1, b, d1;
  quad_br_axes<CACHE>(qb, a1, b, d1);
  Axis a2 = a1;
  if (hi_a) { a2.j = N_A2 - 2; a2.l = 1.0; a2.m = 0.0; }
  const W4 W1 = bil_weights(a1, b), W2 = bil_weights(a2, b);
  const double Cf = lerp_d<CACHE>(bil4w(c.qlo, a1, b, W1), bil4w(c.qhi, a1, b, W1), d1);
  const double C0 = bil4w(c.q0, a1, b, W1);
  const double dC = bil4w(c.qlef, a2, b, W2) - C0;                     // hifi_C_lef :1892-1899
  const double Cq = lerp(c.g0, c.g1, a1), dCm = lerp(c.m0, c.m1, a1), dq = lerp(c.h0, c.h1, a2), eta = lerp(c.e0, c.e1, d1);
  const double dql = k == 1 ? dC : dq;                            // reference quirk: dZdQ uses delta_Cz_lef
  double tot = Cf * (k == 2 ? eta : 1.0) + dC * in.dlef + in.kq * (Cq + dql * in.dlef) * in.Q + (k == 2 ? dCm : 0.0);
  const double Cz_tot = quad_bcast<1>(tot);
  if (k == 2) tot += Cz_tot * (0.35 - xcg);                       // :347
  double Cr = lerp(c.r0, c.r1, a1);
  if (k == 2 && !(flags & FLAG_FIX_CLR)) Cr = 0.0;                // reference defect: _CLr is never loaded
  const double Cp = lerp(c.p0, c.p1, a1), Cb = lerp(c.b0, c.b1, a1);
  const double dCr = lerp(c.hr0, c.hr1, a2), dCp = lerp(c.hp0, c.hp1, a2);
  latd = in.kb * (Cr + dCr * in.dlef) * in.R + in.kb * (Cp + dCp * in.dlef) * in.P + (k == 0 ? 0.0 : Cb * in.beta);
  Q2STAMP(3)
  return tot;
}

// Static part (3-D / 2-D tables) of Cy_tot / Cn_tot / Cl_tot on sub-lanes 0 / 1 / 2 (C/nlplant.c:353-377, hifi_C,
// hifi_C_lef, hifi_rudder, hifi_ailerons); the damping part comes from quad_long, the cg coupling of Cn (:367) is
// applied by the consumer once both parts of Cy_tot are known.
template <bool CACHE, typename TP>
F16_DEV double quad_lat(TP T, const double *xu, int s, unsigned flags, QuadCell &cc, LatCorners &kept, int &status) {
  const QuadIn in = quad_inputs(xu);
  const int k = s < 2 ? s : 2;
  // (1) breakpoints and cells: one axis per sub-lane (re-used from the last step while every lane stays in its cell)
  bool hit;
  const QuadBr qb = quad_br_cached<true, CACHE>(T, in.alpha, in.beta, in.el, s, flags, cc, hit);
  LatCorners fresh;
  LatCorners &c = CACHE ? kept : fresh;
  const bool hi_a = qb.ja > N_A2 - 2;
  if (!CACHE || !hit) {
    c.a45 = T[OFF_BP_A1 + N_A2 - 1];
    const int j2 = hi_a ? N_A2 - 2 : qb.ja;
    const int n1 = qb.jb * N_A1 + qb.ja, n2 = qb.jb * N_A2 + j2;
    struct { int j; } cd = {qb.jd};
    // (2) every table corner this role needs
    constexpr int SA3 = S_G3B, SB3 = S_G3B * N_A1, SD3 = S_G3B * N_A1 * N_B1;
    TP p3 = T + OFF_G3B + n1 * SA3 + (k > 0 ? k - 1 : 0);          // sub-lane 0 shadows Cn; its base is Cy
    c.qlo = ld4(p3 + cd.j * SD3, SA3, SB3); c.qhi = ld4(p3 + (cd.j + 1) * SD3, SA3, SB3); c.q0 = ld4(p3 + D2_ZERO_NODE * SD3, SA3, SB3);
    constexpr int SA2 = S_G2A, SB2 = S_G2A * N_A1;
    TP pa = T + OFF_G2A + n1 * SA2;
    c.qy = ld4(pa, SA2, SB2); c.qr = ld4(pa + 1 + k, SA2, SB2); c.qa = ld4(pa + 4 + k, SA2, SB2);
    constexpr int SAB = S_G2B, SBB = S_G2B * N_A2;
    TP pb = T + OFF_G2B + n2 * SAB;
    c.ql = ld4(pb + 3 + k, SAB, SBB); c.qal = ld4(pb + 6 + k, SAB, SBB);
    // (the off-grid bits with the lookup that finds them: a hit has every lane inside its cell, on the grid)
    if (qb.offa) status |= ST_ALPHA1 | ST_ALPHA2;
    if (qb.offb) status |= ST_BETA;
    if (qb.offd) status |= ST_EL;
  }
  if (hi_a && in.alpha > c.a45) status |= ST_ALPHA2;
  F16_PHASE();
  // (3) arithmetic
  Axis a1, b, d2;
  quad_br_axes<CACHE>(qb, a1, b, d2);
  Axis a2 = a1;
  if (hi_a) { a2.j = N_A2 - 2; a2.l = 1.0; a2.m = 0.0; }
  const W4 W1 = bil_weights(a1, b), W2 = bil_weights(a2, b);
  const double C3 = lerp_d<CACHE>(bil4w(c.qlo, a1, b, W1), bil4w(c.qhi, a1, b, W1), d2), C30 = bil4w(c.q0, a1, b, W1);
  const double Cy = bil4w(c.qy, a1, b, W1), Cr30 = bil4w(c.qr, a1, b, W1), Ca20 = bil4w(c.qa, a1, b, W1);
  const double Clef = bil4w(c.ql, a2, b, W2), Ca20lef = bil4w(c.qal, a2, b, W2);
  const double base = k == 0 ? Cy : C3, base0 = k == 0 ? Cy : C30;
  const double dlefC = Clef - base0;                             // hifi_C_lef
  const double dr30 = Cr30 - base0;                              // hifi_rudder
  const double da20 = Ca20 - base0, da20lef = Ca20lef - Clef - da20;   // hifi_ailerons
  return base + dlefC * in.dlef + (da20 + da20lef * in.dlef) * in.dail + dr30 * in.drud;
}

}  // namespace f16
