// potus_monitor.hpp -- the posterior summary table of any column of the output row, on the device.
//
// What a cmdstanr / rstan user reads first (fit$summary(), print(stanfit), rstan::monitor) and what the reference's scripts tabulate right after
// extract() (final_2016.R:556-705: mean_low_high of mu_b, mean +- 1.96 sd of mu_c / mu_m / mu_pop / polling_bias, the means of e_bias): per column
//   mean, sd, mad, mcse_mean, rhat, ess_bulk, ess_tail, ess_mean, then R's type-7 quantiles at the caller's probabilities,
// as us_potus_model_amd/diagnostics.py (monitor_row) states them in numpy.  rhat and ess_bulk are potus_diagnostics' (potus_diag.hpp), by the same
// device functions; ess_mean is ess_basic of the split draws themselves; ess_tail is posterior::ess_tail, the smaller ess_basic of the split
// indicators 1[x <= Q(x, 0.05)] and 1[x <= Q(x, 0.95)], the quantile taken over ALL draws.
// One workgroup per column, k_dg_column's launch shape (512 threads, at most 96 KB of dynamic LDS for a run of DG_RUN (key, index) pairs) and its
// scratch: two rows of N doubles, and the sorted runs in global memory once the pooled draws exceed DG_RUN.
//   moments   mean and sd (ddof = 1) over all C n draws, two passes, summed thread-strided and then by a DPP tree per wave: same draws, same bytes;
//   sort 1    all draws: order statistics for the quantiles, the median, the two tail quantiles, minimum and maximum (constant columns end here);
//   sort 2    |x - median| of all draws: the mad;
//             with an even number of draws per chain the split draws ARE all draws, enumerated in the split order, so that sorts 1 and 2 also rank
//             the bulk and folded draws; with an odd number the split drops each chain's middle draw (enumerated last here) and two more sorts
//             rank the split draws, exactly as k_dg_column does;
//   four ESS  normal scores (bulk), split draws (mean), the two indicators (tail): each is written to the first scratch row in turn, its chain
//             moments taken by dg_rhat_basic and Geyer's sequence run by dg_ess_basic.
#pragma once
#include "potus_diag.hpp"

#define MN_NSTATS 8           // = POTUS_MONITOR_NSTATS: slots in front of the quantiles
#define MN_MAXPROBS 16
#define MN_NORD (2 * MN_MAXPROBS + 8)   // order statistics of sort 1: two per probability, then two per tail quantile, the two middle ones, the first and the last

struct MnParams {
  const double *cols;       // [NC][C][n]
  double *zbuf;             // [grid][2][max(N, 1)] scratch rows of the split draws
  unsigned long long *rkey; // [grid][C n] sorted runs (only when C n > DG_RUN) ...
  unsigned *ridx;           // ... and their indices
  double *out;              // [NC][MN_NSTATS + n_probs]
  long long n;              // draws per chain
  int C, NC, n_probs;
  double probs[MN_MAXPROBS];
};

// draw j of ALL draws: the split array first (dg_split_value), then -- odd n -- the middle draw of every chain, which the split drops
__device__ __forceinline__ double mn_all_value(const double *x, long long n, int C, long long h, long long N, long long j) {
  return j < N ? dg_split_value(x, n, C, h, j) : x[(size_t)(j - N) * n + h] + 0.0;
}

__global__ __launch_bounds__(DG_THREADS) void k_mn_column(MnParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long xk[];   // min(npad, DG_RUN) keys, then as many indices
  __shared__ double cmean[DG_MAXCH], cvar[DG_MAXCH], rho[DG_LAGS];
  __shared__ double sc[8], ord[MN_NORD], red[DG_THREADS / 64], prob[MN_MAXPROBS];
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < MN_MAXPROBS; i++) if (tid == i) prob[i] = P.probs[i];   // (constant indices: the argument block is not copied to scratch)
  __syncthreads();
  const long long n = P.n, h = n / 2;
  const int C = P.C, C2 = 2 * C, W = MN_NSTATS + P.n_probs;
  const long long N = (long long)C2 * h, M = (long long)C * n;   // split draws, all draws
  const bool odd = (n & 1) != 0, ranked = h >= 2;                // below two draws per half there is no R-hat and no ESS
  double *z = P.zbuf + (size_t)blockIdx.x * 2 * (size_t)(N > 0 ? N : 1), *zf = z + N;
  const DgRuns R = dg_runs(xk, M, P.rkey, P.ridx);
  for (int col = blockIdx.x; col < P.NC; col += gridDim.x) {
    const double *x = P.cols + (size_t)col * C * n;
    double *o = P.out + (size_t)col * W;
    auto aval = [&](long long j) { return mn_all_value(x, n, C, h, N, j); };
    auto val = [&](long long j) { return dg_split_value(x, n, C, h, j); };
    {
      int bad = 0;                                     // a NaN or infinite draw anywhere: every slot is NaN
      for (long long j = tid; j < M; j += DG_THREADS) bad |= !isfinite(aval(j));
      if (__syncthreads_or(bad)) { for (int i = tid; i < W; i += DG_THREADS) o[i] = NAN; continue; }
    }
    // ---- moments over all draws
    double s = 0.0;
    for (long long j = tid; j < M; j += DG_THREADS) s += aval(j);
    const double mean = dg_block_sum(s, red) / (double)M;
    double q = 0.0;
    for (long long j = tid; j < M; j += DG_THREADS) { const double d = aval(j) - mean; q += d * d; }
    const double sd = sqrt(dg_block_sum(q, red) / (double)(M - 1));
    // ---- sort 1: all draws
    dg_sort_runs(aval, M, R);
    if (tid < MN_NORD) {
      long long k = -1;
      if (tid < 2 * P.n_probs) k = ps_q7_index(M, prob[tid >> 1], tid & 1);
      else if (tid >= 2 * MN_MAXPROBS && tid < 2 * MN_MAXPROBS + 4) k = ps_q7_index(M, tid < 2 * MN_MAXPROBS + 2 ? 0.05 : 0.95, tid & 1);
      else if (tid == 2 * MN_MAXPROBS + 4) k = (M - 1) / 2;          // the median: the mean of the two middle draws
      else if (tid == 2 * MN_MAXPROBS + 5) k = M / 2;
      else if (tid == 2 * MN_MAXPROBS + 6) k = 0;
      else if (tid == 2 * MN_MAXPROBS + 7) k = M - 1;
      if (k >= 0) ord[tid] = dg_order(M, k, R);
    }
    __syncthreads();
    const double *tl = ord + 2 * MN_MAXPROBS;
    const double q05 = ps_q7(M, 0.05, tl[0], tl[1]), q95 = ps_q7(M, 0.95, tl[2], tl[3]), med = 0.5 * (tl[4] + tl[5]);
    const bool constant = tl[6] == tl[7];
    if (tid < P.n_probs) o[MN_NSTATS + tid] = ps_q7(M, prob[tid], ord[2 * tid], ord[2 * tid + 1]);
    if (constant) {                                    // as `posterior`: nothing to diagnose
      if (tid == 0) { o[0] = tl[6]; o[1] = 0.0; o[2] = 0.0; for (int i = 3; i < MN_NSTATS; i++) o[i] = NAN; }
      continue;
    }
    if (ranked && !odd) dg_scores(aval, N, R, z);
    __syncthreads();
    // ---- sort 2: |x - median| of all draws
    auto afold = [&](long long j) { return fabs(aval(j) - med) + 0.0; };
    dg_sort_runs(afold, M, R);
    if (tid < 2) ord[tid] = dg_order(M, tid == 0 ? (M - 1) / 2 : M / 2, R);
    if (ranked && !odd) dg_scores(afold, N, R, zf);
    __syncthreads();
    const double mad = 1.4826 * (0.5 * (ord[0] + ord[1]));
    if (ranked && odd) {                               // the split draws on their own, with their own median: k_dg_column's two sorts
      dg_sort_runs(val, N, R);
      if (tid == 0) sc[0] = 0.5 * (dg_order(N, (N - 1) / 2, R) + dg_order(N, N / 2, R));
      dg_scores(val, N, R, z);
      __syncthreads();
      const double smed = sc[0];
      __syncthreads();
      auto fval = [&](long long j) { return fabs(dg_split_value(x, n, C, h, j) - smed) + 0.0; };
      dg_sort_runs(fval, N, R);
      dg_scores(fval, N, R, zf);
    }
    __threadfence_block();
    __syncthreads();
    double rhat = NAN, ess_bulk = NAN, ess_mean = NAN, ess_tail = NAN;
    if (ranked) {
      // ---- R-hat of the folded and the bulk scores, bulk last: its chain moments stay for the ESS
      const double rh_folded = dg_rhat_basic(zf, C2, h, cmean, cvar, sc);
      const double rh_bulk = dg_rhat_basic(z, C2, h, cmean, cvar, sc);
      rhat = dg_nanmax(rh_folded, rh_bulk);
      ess_bulk = dg_ess_basic(z, C2, h, cmean, rho, sc);
      // ---- the split draws themselves
      for (long long j = tid; j < N; j += DG_THREADS) z[j] = val(j);
      __threadfence_block();
      __syncthreads();
      (void)dg_rhat_basic(z, C2, h, cmean, cvar, sc);
      ess_mean = dg_ess_basic(z, C2, h, cmean, rho, sc);
      // ---- the two tail indicators
      double et[2];
      for (int p = 0; p < 2; p++) {
        const double thr = p == 0 ? q05 : q95;
        for (long long j = tid; j < N; j += DG_THREADS) z[j] = val(j) <= thr ? 1.0 : 0.0;
        __threadfence_block();
        __syncthreads();
        (void)dg_rhat_basic(z, C2, h, cmean, cvar, sc);
        et[p] = dg_ess_basic(z, C2, h, cmean, rho, sc);
      }
      ess_tail = (isnan(et[0]) || isnan(et[1])) ? NAN : fmin(et[0], et[1]);
    }
    if (tid == 0) {
      o[0] = mean; o[1] = sd; o[2] = mad; o[3] = sd / sqrt(ess_mean);
      o[4] = rhat; o[5] = ess_bulk; o[6] = ess_tail; o[7] = ess_mean;
    }
    __syncthreads();
  }
}
