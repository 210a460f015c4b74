// potus_timeline.hpp -- the forecast timeline: every run date of a campaign fitted as the data sets of one handle
// (potus_set_datasets_ex) and summarised per data set on the device.  DESIGN.md section 4i.
//
// What a forecaster shows from the refits of a campaign is how predicted_score of a few days -- election day above all -- moved
// from one run date to the next (final_2016.R:66-67 RUN_DATE, :708-762 intervals, :799-823 electoral votes).  Neither kernel
// builds the output row of a draw (43 360 columns for the 2016 design); potus_write_array[_device] of such a handle does, with the
// CHAIN'S model (k_write_array_ds, potus_rows.hpp):
//
//   k_tl_scores       predicted_score of the days [t0, t1) of every post-warm-up draw, straight from the saved unconstrained draw
//                     and the chain's model:  mu_b[:, t] = prior + L_T z_T + L_W (sum of the walk innovations after t).
//                     One WAVE per draw, lane = state.  Election day needs no suffix sum and no L_W product.
//                     out [n_datasets][draws_per_ds][t1 - t0][S]; a data set's draws in canonical order (its chains one after
//                     another, iterations within): the slice of one data set is the `block` of potus_outcomes_device and
//                     potus_scenario_device.
//                     VALUES: bit-equal to wa_build_row's predicted_score.  The same expressions are evaluated in the same
//                     order -- b_T[s] = prior[s] + sum_{k <= s} L_T[s,k] z_T[k] (k ascending), the suffix sums from day T - 2
//                     downwards, a = b_T[s] + sum_{k <= s} L_W[s,k] C[k] (k ascending), d_inv_logit -- and on election day
//                     C = 0, so that the product wa_build_row still walks through adds nothing (a + L * 0 = a for finite L).
//                     No re-association is declared; tests/test_gpu_timeline.py compares bytes.
//   k_tl_summary      one workgroup per (data set, day, column); columns = the S states, the weighted national vote, the
//                     Democratic electoral votes.  The column's draws (at most TL_MAX_DRAWS = 16 384, 128 KB) are summed in
//                     canonical order (thread-strided, then a tree: fixed by the number of draws alone), bitonic-sorted in LDS
//                     and the type-7 order statistics read out of LDS (ps_q7_index / ps_q7 of potus_summary.hpp).  Dynamic LDS
//                     is sized to the padded draw count, so a 2 000-draw date takes 16 KB and several workgroups share a CU;
//                     a 16 384-draw date takes 128 KB + 8 KB of reduction slots, one workgroup per CU (160 KB).
//                     state [n][nd][S][4] = low 2.5 %, high 97.5 %, mean, P(> 0.5); natl [n][nd][4] the same;
//                     ev [n][nd][5] = mean, median, high, low, P(>= ev_to_win).  A data set with a failed chain: NaN.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define TL_MAX_DRAWS PS_RUN
#define TL_THREADS PS_THREADS

struct TlScoreParams {
  RowSrc src;
  int n_post, chains_per_ds;   // post-warm-up rows src.first .. src.first + n_post - 1 of every chain
  int t0, t1;            // days [t0, t1), 0-based
  const int *skip;       // [n_datasets]: nonzero = a chain of the data set failed, its scores are NaN
  double *out;           // [chains * n_post][t1 - t0][S]  (= [n_datasets][chains_per_ds * n_post][t1 - t0][S])
};
__global__ __launch_bounds__(256) void k_tl_scores(const DevModel *Mg, TlScoreParams P) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nd = P.t1 - P.t0;
  const long long n_items = (long long)P.src.chains * P.n_post;
  for (long long item = (long long)blockIdx.x * 4 + wave; item < n_items; item += (long long)gridDim.x * 4) {   // wave-uniform
    const int chain = (int)(item / P.n_post), it = (int)(item % P.n_post), ds = chain / P.chains_per_ds;
    const DevModel &M = Mg[ds];
    const int S = M.S, T = M.T, s = lane;
    const bool act = s < S;
    double *dst = P.out + (size_t)item * nd * S;
    if (P.skip[ds]) {
      for (int i = lane; i < nd * S; i += 64) dst[i] = NAN;
      continue;
    }
    const double *q = P.src.at(chain, it) + POTUS_N_SAMPLER_COLS;
    double bT = 0.0;
    if (act) {
      bT = M.mat[M.m_prior + s];
      for (int k = 0; k <= s; k++) bT += M.mat[M.m_LT + s * S + k] * q[M.o_zT + k];
    }
    if (P.t1 == T && act) dst[(size_t)(T - 1 - P.t0) * S + s] = d_inv_logit(bT);
    const double *Lrow = M.mat + (act ? s : 0) * M.SP;
    double run = 0.0;
    for (int t = T - 2; t >= P.t0; t--) {          // every lane takes every step: the lanes read each other's sums
      run += act ? q[M.o_Z + s + S * t] : 0.0;
      if (t >= P.t1) continue;
      double a = bT;
      for (int k = 0; k < S; k++) {
        const double Ck = oc_readlane(run, k);
        if (act && k <= s) a += Lrow[k] * Ck;
      }
      if (act) dst[(size_t)(t - P.t0) * S + s] = d_inv_logit(a);
    }
  }
}

struct TlSumParams {
  const double *x;       // [n_datasets][n][nd][S]
  int n_ds, n, nd, S;
  const double *w, *ev;  // [S] normalised state weights; electoral votes
  double ev_to_win;
  const int *skip;       // [n_datasets]
  double *o_state, *o_natl, *o_ev;
};
__global__ __launch_bounds__(TL_THREADS) void k_tl_summary(TlSumParams P) {
  extern __shared__ __attribute__((aligned(16))) double tl_xs[];   // npad doubles
  __shared__ double red[2][TL_THREADS];
  __shared__ double qv[6];
  const int tid = threadIdx.x, S = P.S, n = P.n, NCOL = S + 2;
  int npad = 1;
  while (npad < n) npad <<= 1;
  const long long jobs = (long long)P.n_ds * P.nd * NCOL;
  for (long long job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int c = (int)(job % NCOL), day = (int)((job / NCOL) % P.nd), ds = (int)(job / ((long long)NCOL * P.nd));
    const int kind = c < S ? 0 : c == S ? 1 : 2;
    double *o = kind == 0 ? P.o_state + (((size_t)ds * P.nd + day) * S + c) * 4 : kind == 1 ? P.o_natl + ((size_t)ds * P.nd + day) * 4
                                                                                          : P.o_ev + ((size_t)ds * P.nd + day) * 5;
    if (P.skip[ds]) {
      if (tid < (kind == 2 ? 5 : 4)) o[tid] = NAN;
      continue;
    }
    const double thr = kind == 2 ? P.ev_to_win : 0.5;
    const double *base = P.x + ((size_t)ds * n * P.nd + day) * S;
    double sm = 0.0, ex = 0.0;
    for (int d = tid; d < npad; d += TL_THREADS) {
      double v = INFINITY;                                     // padding sorts to the end
      if (d < n) {
        const double *xr = base + (size_t)d * P.nd * S;
        if (kind == 0) v = xr[c];
        else if (kind == 1) { double a = 0.0; for (int s = 0; s < S; s++) a += P.w[s] * xr[s]; v = a; }   // as k_ps_derived sums it
        else { double b = 0.0; for (int s = 0; s < S; s++) b += xr[s] > 0.5 ? P.ev[s] : 0.0; v = b; }
        sm += v;
        ex += kind == 2 ? (v >= thr ? 1.0 : 0.0) : (v > thr ? 1.0 : 0.0);
      }
      tl_xs[d] = v;
    }
    red[0][tid] = sm; red[1][tid] = ex;
    __syncthreads();
    for (int off = TL_THREADS / 2; off > 0; off >>= 1) {
      if (tid < off) { red[0][tid] += red[0][tid + off]; red[1][tid] += red[1][tid + off]; }
      __syncthreads();
    }
    for (int k = 2; k <= npad; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < npad; i += TL_THREADS) {
          const int l = i ^ j;
          if (l > i) {
            const double a = tl_xs[i], b = tl_xs[l];
            const bool up = (i & k) == 0;
            if ((a > b) == up) { tl_xs[i] = b; tl_xs[l] = a; }
          }
        }
        __syncthreads();
      }
    if (tid < 6) {
      const double p = tid < 2 ? 0.025 : tid < 4 ? 0.975 : 0.5;
      qv[tid] = tl_xs[ps_q7_index(n, p, tid & 1)];
    }
    __syncthreads();
    if (tid == 0) {
      const double mean = red[0][0] / (double)n, prob = red[1][0] / (double)n;
      double q3[3];
      for (int j = 0; j < 3; j++) q3[j] = ps_q7(n, j == 0 ? 0.025 : j == 1 ? 0.975 : 0.5, qv[2 * j], qv[2 * j + 1]);
      if (kind == 2) { o[0] = mean; o[1] = q3[2]; o[2] = q3[1]; o[3] = q3[0]; o[4] = prob; }
      else { o[0] = q3[0]; o[1] = q3[1]; o[2] = mean; o[3] = prob; }
    }
    __syncthreads();
  }
}
