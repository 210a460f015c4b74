// potus_loo.hpp -- per-poll log-likelihoods of the saved draws and PSIS-LOO (Vehtari, Gelman, Gabry 2017; loo 2.x), on the device.
//
// Polls are numbered as the output row numbers them: state polls in data order, then national polls (logit_pi_democrat_state, then
// logit_pi_democrat_national).  For poll i with outcome y of n and noise scale sigma_i (psig), eta_i is logit_pi_i without its noise term
// raw_measure_noise_i * sigma_i (stan:102, stan:111), computed directly from the output row:
//   plain       log C(n, y) + y log inv_logit(x) + (n - y) log inv_logit(-x),  x = eta_i + sigma_i z_i (the draw's own noise coordinate): binomial_logit_lpmf
//   integrated  log int Binomial(y | n, inv_logit(eta_i + sigma_i z)) phi(z) dz: the poll's own noise coordinate integrated out
//               (Vehtari et al. 2016, JMLR 17, "integrated importance sampling"), by adaptive Gauss-Hermite quadrature: bracketed Newton
//               steps from z = 0 to the mode of the strictly concave f(z) = y x - n softplus(x) - z^2 / 2 (x = eta_i + sigma_i z), nodes scaled by sqrt(2 / -f''(mode)).
// Kernels:
//   1. k_loo_loglik: one 256-thread workgroup per saved draw rebuilds the output row (wa_build_row, as k_sbc_ranks does) and writes the
//      log-likelihoods of a block of polls as one row [draw][chain][poll]; k_dg_transpose turns the block into [poll][chain][draw]
//      (coalesced stores on both sides);
//   2. k_loo_psis: one workgroup per poll over its S pooled draws: r_eff of exp(ll - max ll), the smoothed and truncated tail of the
//      ratios -ll (potus_psis.hpp: psis_reff, psis_tail; any S up to 512 pooled chains), then here the self-normalised weights and
//      elpd_loo_i, p_loo_i, looic_i, k-hat_i.  Every sum runs in a fixed order (lane-strided, then a DPP tree, then the waves in order):
//      same block, same bytes.
#pragma once
#include "potus_psis.hpp"

#define LOO_GH 16             // Gauss-Hermite nodes of the integrated form (the error against scipy.integrate.quad)
#define LOO_MODE_CAP 100      // most trips of the safeguarded mode search (it stops when a step no longer moves the mode: 3 - 60 trips)
#define LOO_NPW 5             // pointwise outputs: elpd_loo, p_loo, looic, pareto_k, r_eff

// physicists' Gauss-Hermite nodes x_k and log(w_k) + x_k^2 (numpy.polynomial.hermite.hermgauss(16))
__constant__ double loo_gh_x[LOO_GH] = {
    -4.688738939305819, -3.869447904860123, -3.176999161979956, -2.5462021578474814, -1.9517879909162539, -1.3802585391988809,
    -0.8229514491446559, -0.27348104613815244, 0.27348104613815244, 0.8229514491446559, 1.3802585391988809, 1.9517879909162539,
    2.5462021578474814, 3.176999161979956, 3.869447904860123, 4.688738939305819};
__constant__ double loo_gh_lw[LOO_GH] = {
    -0.0652059514099399, -0.3034786882399878, -0.4219670092986956, -0.4947276307888995, -0.5425790095739411, -0.5740888178776504,
    -0.5934069056473787, -0.6026207792767783, -0.6026207792767783, -0.5934069056473787, -0.5740888178776504, -0.5425790095739411,
    -0.4947276307888995, -0.4219670092986956, -0.3034786882399878, -0.0652059514099399};

// y log inv_logit(x) + (n - y) log inv_logit(-x), each factor formed without cancellation (the model passes' form).  y x - n softplus(x) is the
// same number but subtracts two products of size n |x| when x > 0: with y = n at x = 745 the result, 0, came out as 4.5e-9.
__device__ __forceinline__ double loo_binom_term(double y, double n, double x) {
  return y * fmin(x, 0.0) - (n - y) * fmax(x, 0.0) - n * log1p(exp(-fabs(x)));
}
__device__ __forceinline__ double loo_inv_logit(double x) { return 1.0 / (1.0 + exp(-x)); }

// log p(y | n, eta, sigma) without log C(n, y): plain at the draw's noise coordinate z, or z integrated out (sigma = 0: plain at z = 0)
__device__ double loo_poll_ll(double y, double n, double eta, double sig, double z, int integrate) {
  if (!integrate || sig == 0.0) {
    const double x = integrate ? eta : eta + sig * z;
    return loo_binom_term(y, n, x);
  }
  // the mode: f'(m) = sig (y - n p(eta + sig m)) - m is strictly decreasing with its root in [sig (y - n), sig y].  Newton steps from 0
  // inside that bracket, which every f' narrows by its sign; a step that does not land strictly inside is replaced by the midpoint
  // (undamped steps oscillate once the poll is ~2.2 logits from eta and sig^2 n is not small: DESIGN.md 4e).
  double m = 0.0, lo = sig * (y - n), hi = sig * y;
  for (int it = 0; it < LOO_MODE_CAP; it++) {
    const double p = loo_inv_logit(eta + sig * m);
    const double g = sig * (y - n * p) - m;
    if (g > 0.0) lo = m; else if (g < 0.0) hi = m; else break;
    double mn = m - g / (-sig * sig * n * p * (1.0 - p) - 1.0);
    if (mn == m) break;
    if (!(mn > lo && mn < hi)) mn = 0.5 * (lo + hi);
    if (mn == m) break;
    m = mn;
  }
  const double p = loo_inv_logit(eta + sig * m);
  const double s = sqrt(2.0 / (sig * sig * n * p * (1.0 - p) + 1.0));
  double f[LOO_GH], fm = -INFINITY;
#pragma unroll
  for (int k = 0; k < LOO_GH; k++) {
    const double zk = m + s * loo_gh_x[k], x = eta + sig * zk;
    f[k] = loo_binom_term(y, n, x) - 0.5 * zk * zk + loo_gh_lw[k];
    fm = fmax(fm, f[k]);
  }
  double a = 0.0;
#pragma unroll
  for (int k = 0; k < LOO_GH; k++) a += exp(f[k] - fm);
  return fm + log(a) + log(s) - 0.91893853320467274178;   // - log(2 pi) / 2
}

struct LlParams {
  RowSrc src;
  int ncols, n_post;    // saved draws src.first .. src.first + n_post - 1 of every chain (the post-warm-up ones)
  int p0, p1, integrate;
  const double *lc;     // [Npoll] log C(n, y) in the model's (day-sorted) poll order
  double *scratch;      // [gridDim.x][ncols]
  double *out;          // [n_post][chains][p1 - p0]
};
__global__ __launch_bounds__(256) void k_loo_loglik(const DevModel *Mg, LlParams P) {
  const DevModel M = *Mg;
  __shared__ RowLds lds;
  const int tid = threadIdx.x, nb = P.p1 - P.p0, Np = M.Npad;
  const RowCols c = row_cols(M);
  double *row = P.scratch + (size_t)blockIdx.x * P.ncols;
  for (long long d = blockIdx.x; d < (long long)P.n_post * P.src.chains; d += gridDim.x) {
    const int iter = (int)(d / P.src.chains), chain = (int)(d % P.src.chains);
    const double *src = P.src.at(chain, iter), *q = src + POTUS_N_SAMPLER_COLS;
    wa_build_row(M, src, row, lds);
    double *dst = P.out + (size_t)d * nb;
    for (int i = tid; i < M.Npoll; i += 256) {
      const int s = M.pi[i], qi = M.pi[5 * Np + i];
      const bool nat = s == M.S;
      const int k = nat ? M.Ns + (qi - M.o_nn) : qi - M.o_ns;
      if (k < P.p0 || k >= P.p1) continue;
      double eta = row_poll_eta(M, c, row, M.pd + 2 * Np, i);
      eta += nat ? row[c.nat_polling_bias] : row[c.polling_bias + s];
      dst[k - P.p0] = P.lc[i] + loo_poll_ll(M.pd[i], M.pd[Np + i], eta, M.pd[3 * Np + i], q[qi], P.integrate);
    }
    __syncthreads();
  }
}

struct PsisParams {
  const double *ll;           // [NP][C][n]
  const double *r_eff;        // [NP], or null: computed
  PsisWork W;
  double *out;                // [NP][LOO_NPW]
  long long n;                // draws per chain
  int C, NP;
};

__global__ __launch_bounds__(DG_THREADS) void k_loo_psis(PsisParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long xk[];   // as k_dg_column: min(npad, DG_RUN) keys, then the indices
  __shared__ PsisLds L;
  __shared__ PsisReffLds G;
  const int tid = threadIdx.x, C = P.C;
  const long long n = P.n, S = (long long)C * n;
  const PsisPtrs Q = psis_ptrs(P.W, S, xk);
  for (int p = blockIdx.x; p < P.NP; p += gridDim.x) {
    const double *ll = P.ll + (size_t)p * S;
    double *o = P.out + (size_t)p * LOO_NPW;
    {
      int bad = 0;
      for (long long j = tid; j < S; j += DG_THREADS) bad |= !isfinite(ll[j]);
      if (__syncthreads_or(bad)) {
        if (tid == 0) { for (int k = 0; k < 4; k++) o[k] = NAN; o[4] = P.r_eff ? P.r_eff[p] : NAN; }
        continue;
      }
    }
    double mx = -INFINITY, mn = INFINITY;
    for (long long j = tid; j < S; j += DG_THREADS) { mx = fmax(mx, ll[j]); mn = fmin(mn, ll[j]); }
    mx = dg_block_max(mx, L.red);
    mn = -dg_block_max(-mn, L.red);
    const double reff = P.r_eff ? P.r_eff[p] : psis_reff([&](long long j) { return exp(ll[j] - mx); }, C, n, Q.xc, L, G);
    // ---- PSIS of the ratios r = -ll: lw = r - max r
    const double rmax = -mn;
    auto lwv = [&](long long j) { return -ll[j] - rmax + 0.0; };
    const PsisTail T = psis_tail(lwv, S, reff, Q, L);
    auto lwf = [&](long long j) { return T.lw(lwv(j), j); };
    // ---- self-normalised weights; elpd_loo_i = logsumexp(ll + lw), lpd_i = logsumexp(ll) - log S (one pass for both sums, no weights stored)
    double m1 = -INFINITY;
    for (long long j = tid; j < S; j += DG_THREADS) m1 = fmax(m1, lwf(j));
    m1 = dg_block_max(m1, L.red);
    double s1 = 0.0, s3 = 0.0;
    for (long long j = tid; j < S; j += DG_THREADS) { s1 += exp(lwf(j) - m1); s3 += exp(ll[j] - mx); }
    const double lse_w = m1 + log(dg_block_sum(s1, L.red));
    const double lpd = mx + log(dg_block_sum(s3, L.red)) - log((double)S);
    double m2 = -INFINITY;
    for (long long j = tid; j < S; j += DG_THREADS) m2 = fmax(m2, ll[j] + (lwf(j) - lse_w));
    m2 = dg_block_max(m2, L.red);
    double s2 = 0.0;
    for (long long j = tid; j < S; j += DG_THREADS) s2 += exp(ll[j] + (lwf(j) - lse_w) - m2);
    const double elpd = m2 + log(dg_block_sum(s2, L.red));
    if (tid == 0) { o[0] = elpd; o[1] = lpd - elpd; o[2] = -2.0 * elpd; o[3] = T.khat; o[4] = reff; }
    __syncthreads();
  }
}
