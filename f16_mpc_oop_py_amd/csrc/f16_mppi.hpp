// f16_mppi.hpp -- the device statements an MPPI period shares between its stand-alone entries (f16_mppi.hip: f16_mppi_sample,
// f16_mppi_blend) and the fused closed loop (f16_dynamics.hip: k_rollout_mppi): the counter-based sampler and the softmin walk.
// The rules are stated in include/f16_hip.h and restated in numpy / torch by f16_mpc_oop_py_amd/mppi.py.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace f16 {

#define F16_MPPI_DEV __device__ __forceinline__

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of
//   (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0)),   then (k0, k1) += (W0, W1)
struct Philox4 { uint32_t r[4]; };
F16_MPPI_DEV Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// The command limits of the three surfaces (parameters.py:125-126, entries 1..3: elevator, aileron, rudder) that calc_MPPI_action
// clips its samples to.
__device__ constexpr double MPPI_U_LO[3] = {-25.0, -21.5, -30.0}, MPPI_U_HI[3] = {25.0, 21.5, 30.0};

// The three surface commands of sample k of aircraft a in row `row` of period `period`: counter (period, row, k, a), key = the two
// halves of the seed; U_i = (r_i + 0.5) 2^-32 in (0, 1); Box-Muller on (U0, U1) -> n0, n1 and on (U2, U3) -> n2;
// clip(nom_i + sigma_i n_i) with a NaN passing through (np.clip).  Everything travels by value, in registers.
// ONE function, compiled OUT OF LINE, for f16_mppi_sample and for the fused loop: like euler_step_exact (f16_plant.hpp) it then has
// one instruction sequence whoever calls it (FMA contraction follows the surrounding code otherwise), which is what makes the fused
// loop's sample set the stand-alone entry's bit for bit.
struct Cmd3 { double v[3]; };
static __device__ __noinline__ Cmd3 mppi_sample_row(uint32_t period, uint32_t row, uint32_t k, uint32_t a, uint32_t key0, uint32_t key1,
                                                    double nom0, double nom1, double nom2, double sg0, double sg1, double sg2) {
  const Philox4 p = philox4x32_10(period, row, k, a, key0, key1);
  constexpr double SCALE = 1.0 / 4294967296.0, TWO_PI = 6.283185307179586476925286766559;
  const double U0 = ((double)p.r[0] + 0.5) * SCALE, U1 = ((double)p.r[1] + 0.5) * SCALE;
  const double U2 = ((double)p.r[2] + 0.5) * SCALE, U3 = ((double)p.r[3] + 0.5) * SCALE;
  const double ra = sqrt(-2.0 * log(U0)), rb = sqrt(-2.0 * log(U2));
  double s1, c1;
  sincos(TWO_PI * U1, &s1, &c1);
  const double n[3] = {ra * c1, ra * s1, rb * cos(TWO_PI * U3)};
  const double nom[3] = {nom0, nom1, nom2}, sg[3] = {sg0, sg1, sg2};
  Cmd3 o;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double v = nom[i] + sg[i] * n[i];
    o.v[i] = v < MPPI_U_LO[i] ? MPPI_U_LO[i] : (v > MPPI_U_HI[i] ? MPPI_U_HI[i] : v);      // (a NaN fails both tests and stays)
  }
  return o;
}

// One lane's row of the sample set: lane j = k * B0 + a of u_seq[row] from column a of u_nom[row] (the thrust command is copied).
F16_MPPI_DEV void mppi_write_row(const double *nom /* u_nom[row] + a */, long ld0, double *seq /* u_seq[row] + j */, long ld,
                                 uint32_t period, uint32_t row, uint32_t k, uint32_t a, uint32_t key0, uint32_t key1,
                                 double sg0, double sg1, double sg2) {
  const Cmd3 c = mppi_sample_row(period, row, k, a, key0, key1, nom[ld0], nom[2 * ld0], nom[3 * ld0], sg0, sg1, sg2);
  seq[0] = nom[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) seq[(1 + i) * ld] = c.v[i];
}

// The softmin rule of f16_mppi_blend for ONE aircraft (cost and u already point at its column; its samples are B0 apart):
// the minimum over the finite costs ...
F16_MPPI_DEV double blend_min(const double *cost, long K, long B0) {
  double m = INFINITY;
  for (long k = 0; k < K; ++k) {
    const double J = cost[k * B0];
    if (isfinite(J) && J < m) m = J;
  }
  return m;
}
// ... and one walk over k ascending that forms exp(-(J_k - m) / lambda) once per sample and adds it to the two weight sums and to
// NC command sums (u: the first of NC commands ld apart).  A sample without a finite cost has weight 0 and is not read.
template <int NC>
F16_MPPI_DEV void blend_walk(const double *cost, const double *u, long K, long B0, long ld, double m, double lambda, bool blend,
                             double &sw, double &sw2, double (&acc)[NC]) {
  for (long k = 0; k < K; ++k) {
    const double J = cost[k * B0];
    if (!isfinite(J)) continue;                // weight 0: its commands (NaN rows among them) are not read
    const double w = exp(-(J - m) / lambda);
    sw += w; sw2 += w * w;
    if (blend) {
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] += w * u[c * ld + k * B0];
    }
  }
}

}  // namespace f16
