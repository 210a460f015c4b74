// potus_crossval.hpp -- exact cross-validation: held-out polls evaluated under the posterior of the data set (fold) that did not see
// them.  DESIGN.md section 4j.
//
// A fold of K-fold cross-validation, and a run date of leave-future-out, is a data set of potus_set_datasets_ex: the polls it holds out
// stay in the design with n_two_share = 0.  The held-out log predictive density of poll k under data set d is
//   lpd[d][k] = log (1 / n) sum_draws p(y_k | n_k, draw),
// with the data set's own model (its prior and scales, the poll's measurement-noise sigma among them: on a handle of
// potus_set_datasets_grid that is the data set's, elsewhere the one given to potus_create) and the y, n and log C(n, y) of the data given to
// potus_create -- the data set's own y and n of such a poll are 0.  integrate = 1 integrates the poll's noise coordinate over its N(0,1) prior (the fold never saw
// the poll, so the prior IS its posterior there): the exact predictive density, by loo_poll_ll's Gauss-Hermite form.  integrate = 0
// evaluates at the draw's own noise coordinate (checkable to the bit against the logit_pi columns).
// Kernels:
//   k_cv_loglik   one 256-thread workgroup per post-warm-up draw, grid-strided.  A draw of a data set that holds nothing out in this
//                 block of pairs is skipped; otherwise the output row is rebuilt with the chain's model (wa_build_row, as
//                 k_write_array_ds) and loo_poll_ll (shared with k_loo_loglik) is evaluated for the held polls only, eta formed from
//                 the row with k_loo_loglik's terms in its order: on an in-sample pair the bytes are potus_log_lik_device's.
//                 out is compact, [pair][draw of the data set]: pairs ordered by data set, then by poll number as the output row numbers
//                 polls (state polls in data order, then national polls); a data set's draws in canonical order (its chains one after
//                 another, iterations within).  The held lists are per-data-set offsets into ONE index array in the model's (day-sorted)
//                 poll order.  No dense [draw][poll] block, no transpose: for K folds all but 1 / K of its cells would be unused.
//                 The stores of a draw are strided by the draw count (one cell per pair); the row costs far more than they do.
//   k_cv_reduce   one wave per pair: m = max over the data set's draws, a = sum exp(l - m), b = sum exp(2 (l - m)), lane-strided in draw
//                 order and then dpp_wave_sum -- the order is fixed by the draw count alone, no atomics, same bytes on every call.
//                 out [pair][2] = log(a / n) + m, log(b / n) + 2 m: the log predictive density, and the log mean square, from which the
//                 host has the Monte-Carlo variance of the first by the delta method, (exp(o1 - 2 o0) - 1) / n.  That variance treats
//                 the draws as INDEPENDENT: autocorrelation is not accounted for.
//                 A pair with a non-finite ll gives NaN in both slots; so does every pair of a data set with a failed chain (skip).
#pragma once
#include "potus_loo.hpp"

struct CvParams {
  RowSrc src;
  int ncols, n_post, chains_per_ds, integrate;   // post-warm-up rows src.first .. src.first + n_post - 1 of every chain
  const double *pd0;     // [4][Npad] y, n, unadjusted (and sigma, not read: the data set's own is) of the data given to potus_create, in the model's poll order
  const double *lc;      // [Npoll] log C(n, y) of that data, same order
  const int *off;        // [n_datasets + 1] offsets of the data sets' held lists
  const int *held;       // [off[n_datasets]] model poll index of every pair
  const int *skip;       // [n_datasets]: nonzero = a chain of the data set failed
  int p0, p1;            // this launch evaluates pairs [p0, p1)
  double *scratch;       // [gridDim.x][ncols]
  double *out;           // [p1 - p0][chains_per_ds * n_post]
};
__global__ __launch_bounds__(256) void k_cv_loglik(const DevModel *Mg, CvParams P) {
  __shared__ RowLds lds;
  const int tid = threadIdx.x;
  const long long n_items = (long long)P.src.chains * P.n_post, nd = (long long)P.chains_per_ds * P.n_post;
  double *row = P.scratch + (size_t)blockIdx.x * P.ncols;
  for (long long d = blockIdx.x; d < n_items; d += gridDim.x) {          // workgroup-uniform
    const int chain = (int)(d / P.n_post), iter = (int)(d % P.n_post), ds = chain / P.chains_per_ds;
    const int j0 = max(P.off[ds], P.p0), j1 = min(P.off[ds + 1], P.p1);
    if (j0 >= j1) continue;
    const long long at = (long long)(chain % P.chains_per_ds) * P.n_post + iter;
    if (P.skip[ds]) {
      for (int j = j0 + tid; j < j1; j += 256) P.out[(size_t)(j - P.p0) * nd + at] = NAN;
      continue;
    }
    const DevModel M = Mg[ds];
    const int Np = M.Npad;
    const RowCols c = row_cols(M);
    const double *src = P.src.at(chain, iter), *q = src + POTUS_N_SAMPLER_COLS;
    wa_build_row(M, src, row, lds);
    for (int j = j0 + tid; j < j1; j += 256) {
      const int i = P.held[j];
      const int s = M.pi[i], qi = M.pi[5 * Np + i];
      double eta = row_poll_eta(M, c, row, P.pd0 + 2 * Np, i);
      eta += s == M.S ? row[c.nat_polling_bias] : row[c.polling_bias + s];
      P.out[(size_t)(j - P.p0) * nd + at] = P.lc[i] + loo_poll_ll(P.pd0[i], P.pd0[Np + i], eta, M.pd[3 * Np + i], q[qi], P.integrate);
    }
    __syncthreads();
  }
}

struct CvReduceParams {
  const double *ll;      // [n_pairs][n]
  const int *pair_ds;    // [n_pairs] data set of every pair
  const int *skip;       // [n_datasets]
  int n_pairs, n;
  double *out;           // [n_pairs][2]
};
__global__ __launch_bounds__(256) void k_cv_reduce(CvReduceParams P) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long p = (long long)blockIdx.x * 4 + wave; p < P.n_pairs; p += (long long)gridDim.x * 4) {   // wave-uniform
    const double *l = P.ll + (size_t)p * P.n;
    double *o = P.out + (size_t)p * 2;
    int bad = P.skip[P.pair_ds[p]];
    double m = -INFINITY;
    if (!bad)
      for (int j = lane; j < P.n; j += 64) { const double v = l[j]; bad |= !isfinite(v); m = fmax(m, v); }
    if (__any(bad)) {
      if (lane == 0) { o[0] = NAN; o[1] = NAN; }
      continue;
    }
    for (int s = 32; s > 0; s >>= 1) m = fmax(m, __shfl_xor(m, s));
    double a = 0.0, b = 0.0;
    for (int j = lane; j < P.n; j += 64) { const double x = l[j] - m; a += exp(x); b += exp(2.0 * x); }
    a = dpp_wave_sum(a);
    b = dpp_wave_sum(b);
    if (lane == 0) { o[0] = log(a / (double)P.n) + m; o[1] = log(b / (double)P.n) + 2.0 * m; }
  }
}
