// potus_psis.hpp -- Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao, Gabry 2024; loo 2.x) for one workgroup of DG_THREADS,
// stated once for every kernel that smooths ratios: k_loo_psis (potus_loo.hpp), k_mm_psis (potus_loo_mm.hpp), k_el_pointwise, k_el_kr and
// k_el_khat (potus_eloo.hpp).  The rules live here and nowhere else:
//   psis_reff        loo::relative_eff of x = exp(ll - max ll), chains not split: Geyer's initial positive, then monotone sequence of the
//                    chain-averaged autocorrelations, lag by lag (DG_LAGS at a time) as far as the sequence reads them; tau >= 1 / log10 S
//   psis_tail_len    M = ceil(min(0.2 S, 3 sqrt(S / r_eff)));  psis_tail_varies  a tail whose spread is below DBL_EPSILON / 100 is not fitted
//   psis_gpdfit      Zhang & Stephens (2009) with loo's prior on k (10 pseudo-observations of 0.5)
//   psis_tail        the M largest log ratios by potus_diag.hpp's sorted runs, the fit, the smoothed order statistics written back over them;
//                    PsisTail::lw = the smoothed log ratio of a draw, truncated at the largest raw one (0)
//   psis_normalise   lw - logsumexp(lw) written out
// Every sum runs in a fixed order (lane-strided, then a DPP tree, then the waves in order): same ratios, same bytes, whichever kernel asks.
#pragma once
#include <float.h>
#include "potus_diag.hpp"

// The scratch of `grid` workgroups in global memory (the host's psis_work allocates it).  A workgroup's doubles are xc [S] | tail [S] | th [mmax] |
// lth [mmax], then whatever rows the kernel keeps behind them (E_loo: three of S), `stride` doubles in all.
struct PsisWork {
  double *wsd;                // [gridDim.x][stride]: centred weights, then gpdfit's sample | tail | grid of theta | profile log-likelihoods
  int *wsi;                   // [gridDim.x][S] ranks of the draws among the ratios
  unsigned long long *rkey;   // [gridDim.x][S] sorted runs when S > DG_RUN
  unsigned *ridx;
  size_t stride;
  int mmax;                   // psis_mmax(S): at least gpdfit's grid of 30 + floor(sqrt(M)) points
};
__host__ __device__ inline int psis_mmax(long long S) { return 32 + (int)sqrt(0.2 * (double)S + 1.0); }
__host__ __device__ inline size_t psis_ws_doubles(long long S, int extra_rows) { return (2 + (size_t)extra_rows) * (size_t)S + 2 * (size_t)psis_mmax(S); }

// Static LDS in two structs: what every caller needs (the reductions' slots and the two results thread 0 hands to the workgroup: r_eff and
// gpdfit's theta-hat), and what psis_reff alone needs (the chain moments, a round of autocorrelations and the state of Geyer's sequence), so
// that a kernel that is always given r_eff does not carry the latter.  (Both a multiple of 16 bytes: no padding between them.)
struct PsisLds { double red[DG_THREADS / 64], reff, thh; };
struct PsisReffLds { double cmean[DG_MAXCH / 2], cvar[DG_MAXCH / 2], rho[DG_LAGS], sc[6]; };

struct PsisPtrs {             // one workgroup's views of PsisWork and of its sorted runs; end = the kernel's own rows
  double *xc, *tail, *th, *lth, *end;
  int *rnk;
  DgRuns R;
};
__device__ __forceinline__ PsisPtrs psis_ptrs(const PsisWork &W, long long S, unsigned long long *dyn) {
  PsisPtrs p;
  p.xc = W.wsd + (size_t)blockIdx.x * W.stride;
  p.tail = p.xc + S; p.th = p.tail + S; p.lth = p.th + W.mmax; p.end = p.lth + W.mmax;
  p.rnk = W.wsi + (size_t)blockIdx.x * (size_t)S;
  p.R = dg_runs(dyn, S, W.rkey, W.ridx);
  return p;
}

// r_eff = ESS / S of x = xv(j) = exp(ll - max ll), j = chain * n + draw, chains not split.  xc [S] is overwritten.
template <class X>
__device__ __forceinline__ double psis_reff(X xv, int C, long long n, double *xc, PsisLds &L, PsisReffLds &G) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long S = (long long)C * n;
  double *sc = G.sc;
  for (long long j = tid; j < S; j += DG_THREADS) xc[j] = xv(j);
  __threadfence_block();
  __syncthreads();
  for (int c = w; c < C; c += DG_THREADS / 64) {       // one wave per chain: mean, biased autocovariance at lag 0
    double s = 0.0;
    for (long long i = lane; i < n; i += 64) s += xc[(size_t)c * n + i];
    const double m = dpp_wave_sum(s) / (double)n;
    double q = 0.0;
    for (long long i = lane; i < n; i += 64) { const double d = xc[(size_t)c * n + i] - m; q += d * d; }
    const double v = dpp_wave_sum(q) / (double)n;
    if (lane == 0) { G.cmean[c] = m; G.cvar[c] = v; }
  }
  __syncthreads();
  for (long long j = tid; j < S; j += DG_THREADS) xc[j] -= G.cmean[j / n];
  if (tid == 0) {
    double a = 0.0, mm = 0.0;
    for (int c = 0; c < C; c++) { a += G.cvar[c]; mm += G.cmean[c]; }
    const double mean_var = a / C * (double)n / (double)(n - 1);
    double var_plus = mean_var * (double)(n - 1) / (double)n;
    if (C > 1) {
      mm /= C;
      double b = 0.0;
      for (int c = 0; c < C; c++) b += (G.cmean[c] - mm) * (G.cmean[c] - mm);
      var_plus += b / (C - 1);
    }
    sc[0] = mean_var; sc[1] = var_plus;
    sc[2] = 0.0; sc[3] = 0.0; sc[4] = 0.0; sc[5] = 0.0;   // sum of rho over lags < max_t, previous pair, rho(max_t), done
  }
  __threadfence_block();
  __syncthreads();
  const double mean_var = sc[0], var_plus = sc[1];
  for (long long t0 = 0; t0 < n; t0 += DG_LAGS) {
    for (int lg = w; lg < DG_LAGS; lg += DG_THREADS / 64) {
      const long long t = t0 + lg;
      double s = 0.0;
      if (t < n)
        for (int c = 0; c < C; c++) {
          const double *xcc = xc + (size_t)c * n;
          double a = 0.0;
          for (long long i = lane; i + t < n; i += 64) a += xcc[i] * xcc[i + t];
          s += dpp_wave_sum(a) / (double)n;                // biased autocovariance of chain c at lag t
        }
      if (lane == 0) G.rho[lg] = t < n ? 1.0 - (mean_var - s / C) / var_plus : NAN;
    }
    __syncthreads();
    if (tid == 0) {
      double tsum = sc[2], prev = sc[3];
      for (int lg = 0; lg < DG_LAGS; lg += 2) {
        const long long t = t0 + lg;
        const double even = t == 0 ? 1.0 : G.rho[lg], odd = G.rho[lg + 1], pair = even + odd;
        if (t < n - 5 && pair > 0) {                   // not the last pair: kept, then made monotone
          double e = even, od = odd;
          if (t >= 2 && pair > prev) { e = prev / 2; od = e; }
          tsum += e; tsum += od;
          prev = e + od;
        } else {                                       // the last pair: max_t = t
          sc[4] = (t == 0 || pair >= 0 || even > 0) ? even : 0.0;
          sc[5] = 1.0;
          break;
        }
      }
      sc[2] = tsum; sc[3] = prev;
    }
    __syncthreads();
    if (sc[5] != 0.0) break;
  }
  if (tid == 0) {
    double tau = -1.0 + 2.0 * sc[2] + sc[4];
    tau = fmax(tau, 1.0 / log10((double)S));
    L.reff = ((double)S / tau) / (double)S;
  }
  __syncthreads();
  const double reff = L.reff;
  __syncthreads();
  return reff;
}

// the tail length, and whether an ascending tail tl [M] has a spread to fit
__device__ __forceinline__ long long psis_tail_len(long long S, double reff) { return (long long)ceil(fmin(0.2 * (double)S, 3.0 * sqrt((double)S / reff))); }
__device__ __forceinline__ bool psis_tail_varies(const double *tl, long long M) { return tl[M - 1] - tl[0] >= DBL_EPSILON / 100; }

// gpdfit of the ascending sample xs [N], already visible to the workgroup: k (NaN: +inf), sigma
__device__ __forceinline__ double psis_gpdfit(const double *xs, int N, double *th, double *lth, PsisLds &L, double *sigma_out) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int m = 30 + (int)floor(sqrt((double)N));
  const double xstar = xs[(int)floor(N / 4.0 + 0.5) - 1];
  for (int jj = w; jj < m; jj += DG_THREADS / 64) {      // one wave per grid point theta_j
    const double theta = 1.0 / xs[N - 1] + (1.0 - sqrt((double)m / (jj + 0.5))) / 3.0 / xstar;
    double a = 0.0;
    for (int i = lane; i < N; i += 64) a += log1p(-theta * xs[i]);
    const double kj = dpp_wave_sum(a) / N;
    if (lane == 0) { th[jj] = theta; lth[jj] = N * (log(-theta / kj) - kj - 1.0); }
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {                                        // theta-hat = sum_j softmax(l)_j theta_j
    double lm = -INFINITY;
    for (int jj = 0; jj < m; jj++) lm = fmax(lm, lth[jj]);
    double s = 0.0;
    for (int jj = 0; jj < m; jj++) s += exp(lth[jj] - lm);
    const double lse = lm + log(s);
    double thh = 0.0;
    for (int jj = 0; jj < m; jj++) thh += th[jj] * exp(lth[jj] - lse);
    L.thh = thh;
  }
  __syncthreads();
  const double thh = L.thh;
  double a = 0.0;
  for (int j = tid; j < N; j += DG_THREADS) a += log1p(-thh * xs[j]);
  double k = dg_block_sum(a, L.red) / N;
  *sigma_out = -k / thh;
  k = k * N / (N + 10) + 10 * 0.5 / (N + 10);          // loo's weakly informative prior
  if (isnan(k)) k = INFINITY;
  return k;
}

// What the tail step leaves: k-hat (+inf: no fit), and with `smooth` the smoothed order statistics tl [Mt] of the draws whose rank is at least S - Mt
struct PsisTail {
  double khat;
  bool smooth;
  long long S, Mt;
  const double *tl;
  const int *rnk;
  // the log ratio of draw j (raw value v): smoothed, then truncated at max lw = 0
  __device__ __forceinline__ double lw(double v, long long j) const {
    if (smooth && rnk[j] >= S - Mt) v = tl[rnk[j] - (S - Mt)];
    return fmin(v, 0.0);
  }
};
// PSIS of lwv(j) = (log ratio of draw j) - (the largest log ratio), finite or -inf, j < S
template <class F>
__device__ __forceinline__ PsisTail psis_tail(F lwv, long long S, double reff, const PsisPtrs &Q, PsisLds &L) {
  const int tid = threadIdx.x;
  const long long Mt = psis_tail_len(S, reff);
  double khat = INFINITY;
  bool smooth = false;
  double *tail = Q.tail, *tl = tail + 1;                  // tail[0] = the cutoff, tail[1 .. M] = the M largest lw, ascending
  if (Mt >= 5) {
    dg_sort_runs(lwv, S, Q.R);
    for (long long j = tid; j < S; j += DG_THREADS) {
      const double v = lwv(j);
      const long long r0 = dg_rank(v, j, S, Q.R) - 1;
      Q.rnk[j] = (int)r0;
      if (r0 >= S - Mt - 1) tail[r0 - (S - Mt - 1)] = v;
    }
    __threadfence_block();
    __syncthreads();
    if (psis_tail_varies(tl, Mt)) {
      smooth = true;
      const int N = (int)Mt;
      const double ec = exp(tail[0]);
      double *xs = Q.xc;                                  // gpdfit's sample exp(tail) - exp(cutoff), ascending
      for (int j = tid; j < N; j += DG_THREADS) xs[j] = exp(tl[j]) - ec;
      __threadfence_block();
      __syncthreads();
      double sigma;
      const double k = psis_gpdfit(xs, N, Q.th, Q.lth, L, &sigma);
      khat = k;
      if (isfinite(k))
        for (int j = tid; j < N; j += DG_THREADS) tl[j] = log(sigma * expm1(-k * log1p(-(j + 0.5) / N)) / k + ec);
      __threadfence_block();
      __syncthreads();
    }
  }
  return PsisTail{khat, smooth, S, Mt, tl, Q.rnk};
}

// the normalised log weights lw(j) - logsumexp(lw) into lwo [S], visible to the workgroup on return
template <class F>
__device__ __forceinline__ void psis_normalise(F lwv, const PsisTail &T, PsisLds &L, double *lwo) {
  const int tid = threadIdx.x;
  const long long S = T.S;
  auto lwf = [&](long long j) { return T.lw(lwv(j), j); };
  double m1 = -INFINITY;
  for (long long j = tid; j < S; j += DG_THREADS) m1 = fmax(m1, lwf(j));
  m1 = dg_block_max(m1, L.red);
  double s1 = 0.0;
  for (long long j = tid; j < S; j += DG_THREADS) s1 += exp(lwf(j) - m1);
  const double lse_w = m1 + log(dg_block_sum(s1, L.red));
  for (long long j = tid; j < S; j += DG_THREADS) lwo[j] = lwf(j) - lse_w;
  __threadfence_block();
  __syncthreads();
}
