// potus_ppc.hpp -- posterior predictive checks on the device: replicated polls y_rep, their PIT and LOO-PIT sums, and bias / dispersion / count
// statistics per group of polls.  DESIGN.md section 4s and include/potus_hmc.h state the definitions; tests/ppc_ref.py restates them in numpy.
//
// Polls are numbered as potus_loo numbers them.  For poll i and post-warm-up draw s, eta_is is k_loo_loglik's predictor (without the poll's noise
// term), sigma_i the poll's noise scale, z_is the draw's own noise coordinate:
//   replicate   x = eta_is + sigma_i z_is (integrate = 0: the same poll repeated) or eta_is + sigma_i z', z' ~ N(0, 1) fresh (integrate = 1: a new
//               poll of the same pollster, mode, population, state and day; sigma_i = 0: as integrate = 0);  y_rep_is ~ Binomial(n_i, inv_logit(x))
//               by binomial_logit_draw (inversion below n min(p, 1 - p) = 10, BTRS above); n_i = 0: y_rep = 0.
//   randomness  Philox4x32-10, key = the handle's seed with the chain's global id (chain_id_offset + c + 1) as its chain field, counter
//               { poll number, RNG_PPC | kind << 8 | attempt << 10 | rep << 22, post-warm-up iteration, chain id }: kind 1 = the fresh normal (the
//               first of the Box-Muller pair, attempt 0), 2 = u, 3 = v of the binomial sampler's attempt (< 4096); rep in [0, 1023].  A cell's
//               y_rep depends on seed, chain id, iteration, poll and rep alone: not on the poll block, the grid or the split over handles.
//   residual    m = n a1, v = n a1 (1 - a1) + n (n - 1) max(a2 - a1^2, 0) with k_el_poll_share's a1, a2;  r(k) = (k - m) / sqrt(v), 0 unless v > 0
//   groups      per (group, draw) B = sum r, X = sum r^2, N = sum k over the group's polls with n > 0 in ascending poll number, one after the
//               other, at k = y_i (realised) and k = y_rep_is (replicated); compiled without contraction into fused multiply-adds.
//   PIT         lo_i = sum_s w_is [y_rep_is < y_i], eq_i = sum_s w_is [y_rep_is = y_i]: w = exp(lw) (a weight of -inf is 0, NaN gives NaN) in
//               dg_block_sum's order, or without weights the exact counts divided by S.
// Kernels:
//   k_ppc_rep          k_loo_loglik's sibling: one 256-thread workgroup per draw rebuilds the row, one thread per poll draws y_rep -> [draw][chain][poll]
//   k_ppc_groups       one thread per (group, draw), draws fastest (every load and store coalesced): the six accumulators of the cell are loaded,
//                      the group's polls of this block added in order, and stored: [G][3][2][chains][draws] stays on the device across blocks
//   k_ppc_group_stats  one workgroup per (group, statistic): the means of T_obs and T_rep and the counts of T_rep >, =, < T_obs, fixed-order sums
//   k_ppc_pit          one workgroup per poll
#pragma once
#include "potus_eloo.hpp"

enum { RNG_PPC = 11 };   // after RNG_ADVI = 10 (potus_advi.hpp)
#define PPC_MAX_REP 1023
#define PPC_NSTAT 3      // bias, dispersion, count
#define PPC_NOUT 6       // mean T_obs, mean T_rep, #{T_rep > T_obs}, #{=}, #{<}, p = (gt + eq / 2) / S

// the uniforms of the binomial sampler and the fresh normal of a cell (poll = the counter's index)
struct BinomCtrPpc {
  uint32_t iter, rep;
  __device__ __forceinline__ uint32_t word(uint32_t att, uint32_t kind) const { return (uint32_t)RNG_PPC | (kind << 8) | (att << 10) | (rep << 22); }
  __device__ __forceinline__ double operator()(const RngKey &K, uint32_t att, uint32_t kind, uint32_t idx) const {
    uint32_t o[4];
    philox4x32_10(idx, word(att, kind), iter, K.chain, K.k0, K.k1, o);
    return u53(o[0], o[1]);
  }
  __device__ __forceinline__ double normal(const RngKey &K, uint32_t idx) const {
    uint32_t o[4];
    philox4x32_10(idx, word(0u, 1u), iter, K.chain, K.k0, K.k1, o);
    const double u1 = u53(o[0], o[1]), u2 = u53(o[2], o[3]);
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
  }
};

struct PpcRepParams {
  RowSrc src;
  int ncols, n_post;
  int p0, p1, integrate, rep;
  int chain_id_offset;
  unsigned seed_lo, seed_hi;
  double *scratch;      // [gridDim.x][ncols]
  double *out;          // [n_post][chains][p1 - p0]
};
__global__ __launch_bounds__(256) void k_ppc_rep(const DevModel *Mg, PpcRepParams P) {
  const DevModel M = *Mg;
  __shared__ RowLds lds;
  const int tid = threadIdx.x, nb = P.p1 - P.p0, Np = M.Npad;
  const RowCols c = row_cols(M);
  double *row = P.scratch + (size_t)blockIdx.x * P.ncols;
  for (long long d = blockIdx.x; d < (long long)P.n_post * P.src.chains; d += gridDim.x) {
    const int iter = (int)(d / P.src.chains), chain = (int)(d % P.src.chains);
    const double *src = P.src.at(chain, iter), *q = src + POTUS_N_SAMPLER_COLS;
    const RngKey key{P.seed_lo, P.seed_hi, (uint32_t)(P.chain_id_offset + chain + 1)};
    const BinomCtrPpc ctr{(uint32_t)iter, (uint32_t)P.rep};
    wa_build_row(M, src, row, lds);
    double *dst = P.out + (size_t)d * nb;
    for (int i = tid; i < M.Npoll; i += 256) {
      const int s = M.pi[i], qi = M.pi[5 * Np + i];
      const bool nat = s == M.S;
      const int k = nat ? M.Ns + (qi - M.o_nn) : qi - M.o_ns;
      if (k < P.p0 || k >= P.p1) continue;
      double eta = row_poll_eta(M, c, row, M.pd + 2 * Np, i);
      eta += nat ? row[c.nat_polling_bias] : row[c.polling_bias + s];
      const double sig = M.pd[3 * Np + i];
      double x = eta;
      if (sig != 0.0) x = eta + sig * (P.integrate ? ctr.normal(key, (uint32_t)k) : q[qi]);
      dst[k - P.p0] = (double)binomial_logit_draw(key, (uint32_t)k, (int)M.pd[Np + i], x, ctr);
    }
    __syncthreads();
  }
}

// r(k) = (k - m) / sqrt(v): every product, sum and quotient rounded on its own
__device__ __forceinline__ void ppc_moments(double n, double a1, double a2, double &m, double &sd) {
#pragma clang fp contract(off)
  m = n * a1;
  const double d = a2 - a1 * a1, v = n * a1 * (1.0 - a1) + n * (n - 1.0) * (d > 0.0 ? d : 0.0);
  sd = v > 0.0 ? sqrt(v) : 0.0;
}
__device__ __forceinline__ double ppc_resid(double k, double m, double sd) {
#pragma clang fp contract(off)
  return sd > 0.0 ? (k - m) / sd : 0.0;
}

struct PpcGroupParams {
  const double *yrep, *a1, *a2;   // [NP][S]
  const double *y, *n;            // [NP]
  const int *goff, *gpoll;        // [G + 1]; the polls (of this block, n > 0) of every group, ascending
  double *acc;                    // [G][3][2][S]: (bias, dispersion, count) x (realised, replicated)
  long long S;
  int G;
};
__global__ __launch_bounds__(256) void k_ppc_groups(PpcGroupParams P) {
#pragma clang fp contract(off)
  const long long S = P.S, items = (long long)P.G * S;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < items; e += (long long)gridDim.x * 256) {
    const int g = (int)(e / S);
    const long long s = e % S;
    const int j0 = P.goff[g], j1 = P.goff[g + 1];
    if (j0 == j1) continue;
    double *a = P.acc + (size_t)g * (PPC_NSTAT * 2) * S + s;
    double t[PPC_NSTAT * 2];
#pragma unroll
    for (int k = 0; k < PPC_NSTAT * 2; k++) t[k] = a[(size_t)k * S];
    for (int j = j0; j < j1; j++) {
      const int p = P.gpoll[j];
      const double y = P.y[p], yr = P.yrep[(size_t)p * S + s];
      double m, sd;
      ppc_moments(P.n[p], P.a1[(size_t)p * S + s], P.a2[(size_t)p * S + s], m, sd);
      const double ro = ppc_resid(y, m, sd), rr = ppc_resid(yr, m, sd);
      t[0] = t[0] + ro; t[1] = t[1] + rr;
      t[2] = t[2] + ro * ro; t[3] = t[3] + rr * rr;
      t[4] = t[4] + y; t[5] = t[5] + yr;
    }
#pragma unroll
    for (int k = 0; k < PPC_NSTAT * 2; k++) a[(size_t)k * S] = t[k];
  }
}

// out [G][3][PPC_NOUT] from acc; a group without polls (count[g] = 0): NaN means and p, counts 0
__global__ __launch_bounds__(DG_THREADS) void k_ppc_group_stats(const double *acc, const long long *count, double *out, long long S, int G) {
  __shared__ double red[DG_THREADS / 64];
  for (int e = blockIdx.x; e < G * PPC_NSTAT; e += gridDim.x) {
    const int g = e / PPC_NSTAT;
    double *o = out + (size_t)e * PPC_NOUT;
    if (count[g] == 0) {
      if (threadIdx.x == 0) { o[0] = NAN; o[1] = NAN; o[2] = 0.0; o[3] = 0.0; o[4] = 0.0; o[5] = NAN; }
      continue;
    }
    const double *ob = acc + (size_t)e * 2 * S, *rp = ob + S;
    double so = 0.0, sr = 0.0, gt = 0.0, eq = 0.0, lt = 0.0;     // (the counts are whole numbers below 2^31: exact in doubles)
    for (long long s = threadIdx.x; s < S; s += DG_THREADS) {
      const double a = ob[s], b = rp[s];
      so += a; sr += b;
      gt += b > a ? 1.0 : 0.0; eq += b == a ? 1.0 : 0.0; lt += b < a ? 1.0 : 0.0;
    }
    so = dg_block_sum(so, red); sr = dg_block_sum(sr, red);
    gt = dg_block_sum(gt, red); eq = dg_block_sum(eq, red); lt = dg_block_sum(lt, red);
    if (threadIdx.x == 0) {
      o[0] = so / (double)S; o[1] = sr / (double)S;
      o[2] = (double)(unsigned long long)gt; o[3] = (double)(unsigned long long)eq; o[4] = (double)(unsigned long long)lt;
      o[5] = (gt + 0.5 * eq) / (double)S;
    }
  }
}

// out [NP][2] = lo, eq of every poll; lw = null: equal weights 1 / S
__global__ __launch_bounds__(DG_THREADS) void k_ppc_pit(const double *yrep, const double *y, const double *lw, double *out, long long S, int NP) {
  __shared__ double red[DG_THREADS / 64];
  for (int p = blockIdx.x; p < NP; p += gridDim.x) {
    const double *yr = yrep + (size_t)p * S, *l = lw ? lw + (size_t)p * S : nullptr;
    const double yi = y[p];
    double a = 0.0, b = 0.0;
    for (long long s = threadIdx.x; s < S; s += DG_THREADS) {
      const double w = l ? exp(l[s]) : 1.0, v = yr[s];
      a += w * (v < yi ? 1.0 : 0.0);
      b += w * (v == yi ? 1.0 : 0.0);
    }
    a = dg_block_sum(a, red);
    b = dg_block_sum(b, red);
    if (threadIdx.x == 0) { out[2 * p] = l ? a : a / (double)S; out[2 * p + 1] = l ? b : b / (double)S; }
  }
}
