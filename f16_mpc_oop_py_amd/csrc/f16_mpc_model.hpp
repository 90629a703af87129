// f16_mpc_model.hpp -- the MODEL-DEPENDENT parts of the control chain as wavefront-level device code on LDS-resident operands:
// the zero-order hold (c2d_wave), the DARE by structure-preserving doubling on the fp64 matrix cores (dare_sda_wave) and the model
// part of the condensed MPC QP (Q, Qbar, G_k, packed P).  Shared by f16_control.hip (k_c2d, k_lqr, k_rollout_lqr_relin, k_mpc) and
// f16_mpc_wave.hip (the closed MPC loop that re-derives its model at every step); the library is not built with relocatable
// device code, so what two translation units run has to live in a header.  The stage in front of these -- the linearisation that
// produces the (A, B, C) they take -- is f16_linearise.hpp, shared in the same way.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "f16_mpc_state.hpp"
#include "f16_smallmat.hpp"

namespace f16 {

// ------------------------------------------------------------------------------------ small LDS allocator
struct Bump {
  double *p;
  __device__ double *take(int n) { double *r = p; p += (n + 1) & ~1; return r; }
};

// ------------------------------------------------------------------------------------ c2d (ZOH)
// exp([[A,B],[0,0]] h) = [[E,F],[0,I]]: only the top 9x12 block [E F] is propagated.
// Scaling-and-squaring Taylor: X = A h/2^s, Y = B h/2^s, T_1 = [X Y], T_{k+1} = X T_k/(k+1), 13 terms
// (||X|| <= 0.5 => truncation < 1e-15 relative), then s squarings [E F] <- E [E F] + [0 F].
template <int NS, int NI>
__device__ void c2d_wave(const double *A, const double *Bm, double h, double *Ad, double *Bd, double *scr) {
  constexpr int NW = NS + NI, NE = NS * NW;
  Bump al{scr};
  double *X = al.take(NS * NS), *T = al.take(NE), *Tn = al.take(NE), *EF = al.take(NE);
  const int l = lane_id();
  double rs = 0.0;
  if (l < NS) {
    for (int j = 0; j < NS; ++j) rs += fabs(A[l * NS + j]);
    for (int j = 0; j < NI; ++j) rs += fabs(Bm[l * NI + j]);
    rs *= fabs(h);
  }
  const double nrm = wave_max(rs);
  int s = 0;
  if (nrm > 0.5) s = min(40, (int)ceil(log2(nrm / 0.5)));
  const double sc = ldexp(h, -s);
  for (int e = l; e < NS * NS; e += F16_WAVE) X[e] = A[e] * sc;
  for (int e = l; e < NE; e += F16_WAVE) {
    const int i = e / NW, j = e - i * NW;
    const double v = j < NS ? A[i * NS + j] * sc : Bm[i * NI + (j - NS)] * sc;
    T[e] = v;
    EF[e] = v + (j == i ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int k = 2; k <= 13; ++k) {
    mm<false, false>(Tn, X, T, NS, NS, NW, 1.0 / k);
    for (int e = l; e < NE; e += F16_WAVE) { T[e] = Tn[e]; EF[e] += Tn[e]; }
    __syncthreads();
  }
  for (int q = 0; q < s; ++q) {
    for (int e = l; e < NS * NS; e += F16_WAVE) X[e] = EF[(e / NS) * NW + (e % NS)];   // E
    __syncthreads();
    mm<false, false>(Tn, X, EF, NS, NS, NW);
    for (int e = l; e < NE; e += F16_WAVE) {
      const int j = e % NW;
      EF[e] = Tn[e] + (j >= NS ? EF[e] : 0.0);
    }
    __syncthreads();
  }
  for (int e = l; e < NS * NS; e += F16_WAVE) Ad[e] = EF[(e / NS) * NW + (e % NS)];
  for (int e = l; e < NS * NI; e += F16_WAVE) Bd[e] = EF[(e / NI) * NW + NS + (e % NI)];
  __syncthreads();
}

// ------------------------------------------------------------------------------------ DARE / dlqr
// DARE  X = A'XA - A'XB (R+B'XB)^-1 B'XA + Q  by the structure-preserving doubling algorithm (SDA):
//   A0 = A, G0 = B R^-1 B', H0 = Q;  W = (I + G H)^-1;  A+ = A W A;  G+ = G + A W G A';  H+ = H + A' H W A.
// H_k -> X quadratically (21 doublings at the reference's trim point; scipy.linalg.solve_discrete_are's
// answer is reproduced to ~1e-11 relative).  R = I here (env.py:354, :405-407).
//
// Mapping: one wavefront per aircraft, every 9x9 operand lives in REGISTERS as a zero-padded 16x16 tile in the
// accumulator layout of v_mfma_f64_16x16x4_f64 (register q of lane l holds element (4q + l/16, l%16); rows 12..15 are
// padding and never stored), and every product is three chained MFMAs with no data movement at all, because
//   * the B operand of k-step s (lane l -> B[4s + l/16][l%16]) IS register s of the right factor's tile, and
//   * the A operand of k-step s (lane l -> A[l%16][4s + l/16]) IS register s of the tile of the left factor's TRANSPOSE,
// so the iteration carries A and A' (G, H are symmetric) and forms each intermediate in the orientation its consumer
// needs: 9 products = 27 MFMAs per doubling.  W = (I + G H)^-1 is a register-resident Gauss-Jordan (inverse9_tile).
typedef double d4_t __attribute__((ext_vector_type(4)));
constexpr int DARE_SCRATCH = 9 * 18 + 16;

// D = C + L R, the left factor given as the tile of L'
__device__ __forceinline__ d4_t mm16(const d4_t &Lt, const d4_t &R, d4_t C) {
  C = __builtin_amdgcn_mfma_f64_16x16x4f64(Lt[0], R[0], C, 0, 0, 0);
  C = __builtin_amdgcn_mfma_f64_16x16x4f64(Lt[1], R[1], C, 0, 0, 0);
  C = __builtin_amdgcn_mfma_f64_16x16x4f64(Lt[2], R[2], C, 0, 0, 0);
  return C;
}
// tile of the row-major 9x9 LDS matrix M (or of its transpose)
__device__ __forceinline__ d4_t tile9(const double *M, bool transpose) {
  const int l = lane_id(), lc = l & 15, lq = l >> 4;
  d4_t t = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int r = 4 * q + lq;
    if (r < 9 && lc < 9) t[q] = transpose ? M[lc * 9 + r] : M[r * 9 + lc];
  }
  return t;
}

// W <- M^-1 for the 9x9 tile M: Gauss-Jordan with partial pivoting on [M | I] held one COLUMN per lane (lanes 0..17,
// nine rows in registers).  A pivot step broadcasts the pivot column from its lane (v_readlane -> scalars), so the pivot
// search and the multipliers are wave-uniform and the step needs no LDS and no barrier; rows are not swapped, the row
// map is applied when the inverse is written back.  LDS (Wl, 81 doubles) only converts between the two layouts.
// PIVOT = false: the same elimination in natural order (no search, no row map) -- a third of the instructions.  The
// caller checks the result (residual of M W - I on the matrix cores) and repeats with PIVOT = true if it is not clean.
template <bool PIVOT>
__device__ __forceinline__ bool inverse9_tile(const d4_t &M, d4_t &W, double *Wl) {
  const int l = lane_id(), lc = l & 15, lq = l >> 4;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int r = 4 * q + lq;
    if (r < 9 && lc < 9) Wl[r * 9 + lc] = M[q];
  }
  __syncthreads();
  const int j = l < 18 ? l : 17;                       // lanes beyond 17 shadow column 17
  double r[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) r[i] = j < 9 ? Wl[i * 9 + j] : (i == j - 9 ? 1.0 : 0.0);
  unsigned done = 0;
  int pinv[9];                                         // pinv[i] = the pivot step that used row i
  bool ok = true;
#pragma unroll
  for (int p = 0; p < 9; ++p) {
    double c[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) c[i] = readlane_f64(r[i], p);
    if (PIVOT) {
      int piv = 0;
      double best = -1.0, cp = 1.0;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const double v = ((done >> i) & 1u) ? -1.0 : fabs(c[i]);
        const bool gt = v > best;
        best = gt ? v : best; piv = gt ? i : piv; cp = gt ? c[i] : cp;
      }
      ok = ok && best > 0.0;
      done |= 1u << piv;
      double rp = r[0];
#pragma unroll
      for (int i = 1; i < 9; ++i) rp = piv == i ? r[i] : rp;
      rp *= 1.0 / cp;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        r[i] = piv == i ? rp : fma(-c[i], rp, r[i]);
        pinv[i] = piv == i ? p : (p == 0 ? 0 : pinv[i]);
      }
    } else {
      ok = ok && c[p] != 0.0;
      const double rp = r[p] * (1.0 / c[p]);
#pragma unroll
      for (int i = 0; i < 9; ++i) r[i] = i == p ? rp : fma(-c[i], rp, r[i]);
    }
  }
  if (!PIVOT) {
#pragma unroll
    for (int i = 0; i < 9; ++i) pinv[i] = i;
  }
  __syncthreads();                                     // all reads of Wl are long done; reuse it for the inverse
  if (l >= 9 && l < 18) {
#pragma unroll
    for (int i = 0; i < 9; ++i) Wl[pinv[i] * 9 + (l - 9)] = r[i];
  }
  __syncthreads();
  W = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int rr = 4 * q + lq;
    if (rr < 9 && lc < 9) W[q] = Wl[rr * 9 + lc];
  }
  __syncthreads();
  return ok;
}

// Rinv: null = R is the identity (env.py:405-407), else the inverse of the input weight, 3 x 3 row-major (utils.py:219 `dlqr(A, B, Q, R)`)
__device__ __forceinline__ int dare_sda_wave(const double *A0, const double *Bm, const double *Q, double *X, double *scr, const double *Rinv = nullptr) {
  const int l = lane_id(), lc = l & 15, lq = l >> 4;
  const d4_t zero = {0.0, 0.0, 0.0, 0.0};
  d4_t A = tile9(A0, false), At = tile9(A0, true), H = tile9(Q, false);
  d4_t G;
  {
    d4_t Bt = zero;                                  // tile of B' (3x9): element (k, i) = B[i][k]
    if (lq < 3 && lc < 9) Bt[0] = Bm[lc * 3 + lq];
    double br = Bt[0];                               // element (lc, lq) of B R^-1
    if (Rinv && lq < 3 && lc < 9) br = Bm[lc * 3] * Rinv[lq] + Bm[lc * 3 + 1] * Rinv[3 + lq] + Bm[lc * 3 + 2] * Rinv[6 + lq];
    G = __builtin_amdgcn_mfma_f64_16x16x4f64(br, Bt[0], zero, 0, 0, 0);        // G0 = B R^-1 B'  (R = I: B B')
  }
  d4_t eye = zero;
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (4 * q + lq == lc && lc < 9) eye[q] = 1.0;
  int it = 0;
  for (; it < 60; ++it) {
    const d4_t M = mm16(G, H, eye);                  // I + G H          (G symmetric: its own transpose)
    const d4_t GAt = mm16(G, At, zero);              // G A'             (independent of W: overlaps the inverse)
    d4_t W;
    {
      // natural-order elimination first; accept it if || M W - I ||_max (M' = I + H G as the left factor) is at the level
      // cond(M) eps allows -- cond(M) reaches 3e7 late in the iteration, where partial pivoting leaves the same 1e-9 --
      // otherwise redo with partial pivoting.  Measured on the config-4 models (3,800 inversions): median residual
      // 1.4e-12, 99th percentile 6e-11, 0.05 % above the threshold; worst unpivoted pivot/column-max ratio 5e-5.
      bool good = inverse9_tile<false>(M, W, scr);
      const d4_t Mt = mm16(H, G, eye);
      d4_t neye = zero;
#pragma unroll
      for (int q = 0; q < 3; ++q) neye[q] = -eye[q];
      const d4_t E = mm16(Mt, W, neye);
      double emax = fmax(fmax(fabs(E[0]), fabs(E[1])), fabs(E[2]));
      emax = wave_max(emax);
      good = good && emax <= 2e-9;
      if (!good && !inverse9_tile<true>(M, W, scr)) { it = 60; break; }
    }
    const d4_t T1t = mm16(W, At, zero);              // (A W)' = W' A'   (left W' <- tile of W)
    const d4_t HWt = mm16(W, H, zero);               // (H W)' = W' H
    const d4_t An = mm16(T1t, A, zero);              // A W A            (left A W <- tile of (A W)')
    const d4_t Atn = mm16(A, T1t, zero);             // (A W A)' = A' (A W)'
    G = mm16(T1t, GAt, G);                           // G + A W G A'
    const d4_t HWA = mm16(HWt, A, zero);             // H W A            (left H W <- tile of (H W)')
    const d4_t dH = mm16(A, HWA, zero);              // A' H W A         (left A' <- tile of A)
    double dmax = 0.0, hmax = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      H[q] += dH[q];
      dmax = fmax(dmax, fabs(dH[q]));
      hmax = fmax(hmax, fabs(H[q]));
    }
    dmax = wave_max(dmax);
    hmax = wave_max(hmax);
    A = An; At = Atn;
    if (dmax <= 1e-16 * hmax) { ++it; break; }
  }
  // A solution that is not finite has not converged, whatever the stop rule made of it: the maxima above are built with fmax, which
  // drops NaN (an all-NaN step gives 0 <= 0), and an overflowed H gives inf <= 1e-16 inf.  Tested once here, after the loop, so the
  // doubling itself and every finite result stay as they were.  (Rows 12..15 and the columns beyond 8 of the tile are zero.)
  if (__any(!(isfinite(H[0]) && isfinite(H[1]) && isfinite(H[2])))) it = 60;
  // X = (H + H') / 2 through LDS (the caller wants it there)
  double *Xt = scr;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int r = 4 * q + lq;
    if (r < 9 && lc < 9) Xt[r * 9 + lc] = H[q];
  }
  __syncthreads();
  for (int e = l; e < 81; e += F16_WAVE) {
    const int i = e / 9, j = e - i * 9;
    X[e] = 0.5 * (Xt[e] + Xt[j * 9 + i]);
  }
  __syncthreads();
  return it;
}
constexpr int C2D_SCRATCH = 81 + 2 + 3 * (9 * 12 + 2);                 // c2d_wave<9, 3>: X | T | Tn | EF (Bump-rounded)

// ------------------------------------------------------------------------------------ the model part of the MPC QP
// Everything of the condensed QP (utils.py:21-167) that depends on the MODEL (A, B, C) and the weights only: Q = C'C, the terminal
// weight Qbar (the DARE solution, dare_sda_wave above), the prediction blocks G_k = A^k B and the packed Hessian P.  ONE definition
// for the two callers -- the build kernel k_mpc<true> (f16_control.hip: the model handed in by the caller) and the re-linearising
// closed loop (f16_mpc_wave.hip: pair_model, the model derived at the aircraft's current state at every step) -- so that a QP built
// inside the loop is bit for bit the QP f16_mpc_batch_w builds from the same model.  All operands in LDS; one wavefront; l = lane_id().
// (The weights are read as a.pb.<field> of the caller's own argument struct: k_mpc hands in its kernel arguments, and the accesses
//  compile to what they compiled to when this code stood in the kernel.)

// Q = C'C (env.py:389) from the C staged in Cs, or the caller's Q (utils.py:21 `Q`)
template <class ARGS>
__device__ __forceinline__ void mpc_model_q(double *Q, const double *Cs, const ARGS &a, int l) {
  if (a.pb.custom_q) { for (int e = l; e < 81; e += F16_WAVE) Q[e] = a.pb.Q[e]; __syncthreads(); }       // utils.py:21 `Q`
  else mm<true, false>(Q, Cs, Cs, 9, 9, 9);         // Q = C'C (env.py:389)
}

// (the gain K = -dlqr of utils.py:96 is not needed itself: it only enters through Q_bar)
// Q_bar (utils.py:100) solves X = Phi' X Phi + Q + K'RK with Phi = A + B K: for the LQR gain K that equation IS the
// DARE, so its solution is the DARE solution X itself.  (Measured on the reference's trim models: SDA's X agrees
// with scipy.linalg.solve_discrete_lyapunov's Q_bar to 3e-13 relative -- closer than scipy's own DARE result.)
// exm (may be null): the aircraft's A | Q | Qbar block of the workspace.
__device__ __forceinline__ void mpc_model_keep(const double *A, const double *Q, double *Qb, const double *X, double *exm, int l) {
  copy(Qb, X, 81);
  if (exm) {
    for (int e = l; e < 81; e += F16_WAVE) { exm[e] = A[e]; exm[81 + e] = Q[e]; exm[162 + e] = Qb[e]; }
  }
}

// prediction blocks G_k = A^k B (utils.py:171-197 without forming CC/MM).  Bm may alias memory that is written after the call.
__device__ __forceinline__ void mpc_model_G(const double *A, const double *Bm, double *G, int N, int l) {
  // lane e = (r,c) < 27 carries G_k[r][c]; G_(k+1)[r][c] = sum_p A[r][p] G_k[p][c] takes the nine operands from the
  // lanes (p,c) by ds_bpermute: no LDS round trip + barrier per step of this N-long dependent chain
  const int e = l < 27 ? l : 0, r = e / 3, c = e - 3 * r;
  double ar[9], gv = Bm[e];
#pragma unroll
  for (int p = 0; p < 9; ++p) ar[p] = A[r * 9 + p];
  __syncthreads();                         // (Bm aliases pred: read before anything writes there)
  if (l < 27) G[l] = gv;
  for (int k = 1; k < N; ++k) {
    double sacc = 0.0;
#pragma unroll
    for (int p = 0; p < 9; ++p) sacc += ar[p] * __shfl(gv, p * 3 + c, 64);
    gv = sacc;
    if (l < 27) G[k * 27 + l] = gv;
  }
  __syncthreads();
}

// P = 2 (CC' QQ CC + RR), packed lower, to the workspace.  (A'A is no longer formed here: the solvers
// need the row-WEIGHTED Gram A'WA of the equilibrated problem, which has no Toeplitz recursion, and build it themselves.)
// Block (j,l), j >= l, d = j-l:  T(j,l) = TQ(j,l) + G'_{N-1-j} Qbar G_{N-1-l},
//   TQ(j,l) = TQ(j+1,l+1) + G'_{N-2-j} Q G_{N-2-l} (0 beyond N-2).
// One chain per (diagonal d, element (ra,cb)), up to MAXCH per lane; all chains walk j together, so the two weighted
// blocks a step needs (Q G_{N-2-j}, Qbar G_{N-1-j}) are the same for every lane and are formed once per step (jit).
// This loop is LDS-bandwidth-bound (42 operand reads for 24 FMAs per chain element).  Tried and dropped: one lane per
// block diagonal (216 FMAs for 27 + 72 reads per step, running sums in registers, no jit broadcast conflicts) --
// fewer LDS bytes but only N active lanes and as many address computations for the packed stores: 20 % slower.
// jit: 54 doubles of LDS; a.pb: the weights (custom_r, R -- MpcProb, or anything with these members).
template <int MAXCH, class ARGS>
__device__ __forceinline__ void mpc_model_P(const double *Q, const double *Qb, const double *G, double *jit, double *Pg, int N,
                                            const ARGS &a, int l) {
  double tq[MAXCH];
#pragma unroll
  for (int t = 0; t < MAXCH; ++t) tq[t] = 0.0;
  const int wh = l >= 27 ? 1 : 0, je = l - 27 * wh, jr = je / 3, jc = je - 3 * jr;      // jit roles of lanes 0..53
  const double *Qw = wh ? Qb : Q;
  __syncthreads();
  for (int j = N - 1; j >= 0; --j) {
    const int kq = wh ? N - 1 - j : N - 2 - j;
    if (l < 54 && kq >= 0) {
      double sj = 0.0;
#pragma unroll
      for (int p = 0; p < 9; ++p) sj += Qw[jr * 9 + p] * G[kq * 27 + p * 3 + jc];
      jit[l] = sj;
    }
    __syncthreads();
    const double *QGk = jit, *QbGk = jit + 27;
#pragma unroll
    for (int t = 0; t < MAXCH; ++t) {
      const int ch = l + F16_WAVE * t, d = ch / 9, ee = ch - 9 * d, ra = ee / 3, cb = ee - 3 * ra;
      __builtin_amdgcn_sched_barrier(0);      // one chain at a time: bounds the live operands (two waves per SIMD)
      if (ch < 9 * N && j >= d) {
        const int lcol = j - d;
        if (j <= N - 2) {
          double s = 0.0;
#pragma unroll
          for (int p = 0; p < 9; ++p) s += QGk[p * 3 + ra] * G[(N - 2 - lcol) * 27 + p * 3 + cb];
          tq[t] += s;
        }
        double gc[9];
#pragma unroll
        for (int p = 0; p < 9; ++p) gc[p] = G[(N - 1 - lcol) * 27 + p * 3 + cb];
        double sb = 0.0;
#pragma unroll
        for (int p = 0; p < 9; ++p) sb += QbGk[p * 3 + ra] * gc[p];
        const int gi = 3 * j + ra, gj = 3 * lcol + cb;
        // RR = blkdiag(R, ..., R) (utils.py:108-111); R = I (env.py:405-407) unless the caller gave one
        const double rr_ = a.pb.custom_r ? (d == 0 ? a.pb.R[ra * 3 + cb] : 0.0) : ((gi == gj) ? 1.0 : 0.0);
        if (gi >= gj) Pg[tri(gi, gj)] = 2.0 * (tq[t] + sb + rr_);
      }
    }
    __syncthreads();                                                    // jit is rewritten by the next step
  }
}

}  // namespace f16
