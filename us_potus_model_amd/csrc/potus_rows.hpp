// potus_rows.hpp -- the CmdStan output row of a draw, rebuilt from its unconstrained point, and what the kernels that rebuild it share
// (DESIGN.md 4m): the column blocks (RowCols), the builder (wa_build_row) with its LDS (RowLds) and source (RowSrc), the poll predictor
// (row_poll_eta), and the kernels k_write_array[_ds], k_simulate_prior, k_sbc_ranks / k_sbc_reduce.  k_loo_loglik (potus_loo.hpp) and
// k_cv_loglik (potus_crossval.hpp) build rows too.
#pragma once

// The first column of every block of a row, in CmdStan's order: 7 sampler columns, the D parameters, transformed parameters (stan:70-113),
// generated quantities (stan:134-140).  row_cols is the ONE place that knows the order and sizes of the blocks after the parameters.
struct RowCols {
  int par, mu_b, mu_c, mu_m, mu_pop, e_bias, polling_bias, nat_mu_b, nat_polling_bias, sigma_rho, logit_pi_state, logit_pi_national, predicted_score, ncols;
};
__host__ __device__ inline RowCols row_cols(int D, int S, int T, int P, int M, int Pop, int Ns, int Nn, bool full) {
  RowCols c;
  c.par = POTUS_N_SAMPLER_COLS; c.mu_b = c.par + D; c.mu_c = c.mu_b + S * T; c.mu_m = c.mu_c + P;
  c.mu_pop = c.mu_m + (full ? M : 0); c.e_bias = c.mu_pop + (full ? Pop : 0); c.polling_bias = c.e_bias + (full ? T : 0);
  c.nat_mu_b = c.polling_bias + S; c.nat_polling_bias = c.nat_mu_b + T; c.sigma_rho = c.nat_polling_bias + 1;
  c.logit_pi_state = c.sigma_rho + (full ? 1 : 0); c.logit_pi_national = c.logit_pi_state + Ns; c.predicted_score = c.logit_pi_national + Nn;
  c.ncols = c.predicted_score + T * S; return c;
}
__host__ __device__ inline RowCols row_cols(const DevModel &M) { return row_cols(M.D, M.S, M.T, M.P, M.M, M.Pop, M.Ns, M.Nn, M.full != 0); }
inline RowCols row_cols(const potus_data *d, int D) { return row_cols(D, d->S, d->T, d->P, d->M, d->Pop, d->N_state_polls, d->N_national_polls, d->variant == POTUS_VARIANT_FULL); }

struct RowLds { double bT[64], pb[64], misc[4]; };   // declared __shared__ once per kernel
struct RowSrc {
  const double *draws; // [chains][n_save_max][row]
  int chains, n_save_max, row, first;   // saved row `first` of a chain is iter 0
  __device__ const double *at(int chain, int iter) const { return draws + ((size_t)chain * n_save_max + first + iter) * row; }
};

// The prediction of model poll i (day-sorted order) from a built row, before polling bias and measurement noise are added; unadjusted = the
// [Npoll] flags of the polls, the model's own (M.pd + 2 * M.Npad) or those of other data in the same order.
__device__ __forceinline__ double row_poll_eta(const DevModel &M, const RowCols &c, const double *row, const double *unadjusted, int i) {
  const int s = M.pi[i], t = M.pi[M.Npad + i];
  double eta = (s == M.S ? row[c.nat_mu_b + t] : row[c.mu_b + s + M.S * t]) + row[c.mu_c + M.pi[2 * M.Npad + i]];
  if (M.full) eta += row[c.mu_m + M.pi[3 * M.Npad + i]] + row[c.mu_pop + M.pi[4 * M.Npad + i]] + unadjusted[i] * row[c.e_bias + t];
  return eta;
}

// One full CmdStan output row (ncols doubles) from a draw's sampler columns and unconstrained point src[0 .. 7 + D); src must not
// alias row.  Called by every thread of a workgroup of NT threads (256 in the row kernels; k_mm_pass shares its workgroup with the model pass).
template <int NT = 256>
__device__ __forceinline__ void wa_build_row(const DevModel &M, const double *src, double *row, RowLds &lds) {
  const int tid = threadIdx.x, S = M.S, T = M.T, D = M.D;
  const RowCols c = row_cols(M);
  const double *q = src + POTUS_N_SAMPLER_COLS;
  for (int i = tid; i < POTUS_N_SAMPLER_COLS + D; i += NT) row[i] = src[i];
  __syncthreads();
  double *Ct = row + c.predicted_score; // suffix sums, staged where predicted_score will go
  if (tid < S) {
    double run = 0.0;
    Ct[tid + S * (T - 1)] = 0.0;
    for (int t = T - 2; t >= 0; t--) { run += q[M.o_Z + tid + S * t]; Ct[tid + S * t] = run; }
    double bT = M.mat[M.m_prior + tid], pb = 0.0;
    for (int k = 0; k <= tid; k++) { bT += M.mat[M.m_LT + tid * S + k] * q[M.o_zT + k]; pb += M.mat[M.m_LB + tid * S + k] * q[M.o_zb + k]; }
    lds.bT[tid] = bT; lds.pb[tid] = pb; row[c.polling_bias + tid] = pb;
  }
  if (tid == 64 && M.full) {
    const double mue = 0.02 * q[M.o_mue], rho = d_inv_logit(q[M.o_rho]), srho = sqrt(1.0 - rho * rho) * M.sigma_e;
    row[c.par + M.o_mue] = mue; row[c.par + M.o_rho] = rho; row[c.sigma_rho] = srho;
    double e = q[M.o_ze] * M.sigma_e;
    row[c.e_bias] = e;
    for (int t = 1; t < T; t++) { e = mue + rho * (e - mue) + q[M.o_ze + t] * srho; row[c.e_bias + t] = e; }
  }
  for (int i = tid; i < M.P; i += NT) row[c.mu_c + i] = q[M.o_c + i] * M.sigma_c;
  if (M.full) {
    for (int i = tid; i < M.M; i += NT) row[c.mu_m + i] = q[M.o_m + i] * M.sigma_m;
    for (int i = tid; i < M.Pop; i += NT) row[c.mu_pop + i] = q[M.o_pop + i] * M.sigma_pop;
  }
  __syncthreads();
  for (int idx = tid; idx < S * T; idx += NT) {
    const int s = idx % S, t = idx / S;
    double a = lds.bT[s];
    const double *Lrow = M.mat + s * M.SP, *Cc = Ct + S * t;
    for (int k = 0; k <= s; k++) a += Lrow[k] * Cc[k];
    row[c.mu_b + idx] = a;
  }
  if (tid == 0) { double a = 0.0; for (int s = 0; s < S; s++) a += lds.pb[s] * M.mat[M.m_w + s]; lds.misc[0] = a; row[c.nat_polling_bias] = a; }
  __syncthreads();
  for (int t = tid; t < T; t += NT) {
    double a = 0.0;
    for (int s = 0; s < S; s++) a += row[c.mu_b + s + S * t] * M.mat[M.m_w + s];
    row[c.nat_mu_b + t] = a;
  }
  __syncthreads();
  for (int i = tid; i < M.Npoll; i += NT) {
    const int s = M.pi[i], qi = M.pi[5 * M.Npad + i];
    const bool nat = s == S;
    double eta = row_poll_eta(M, c, row, M.pd + 2 * M.Npad, i);
    eta += q[qi] * M.pd[3 * M.Npad + i] + (nat ? lds.misc[0] : lds.pb[s]);
    if (nat) row[c.logit_pi_national + (qi - M.o_nn)] = eta; else row[c.logit_pi_state + (qi - M.o_ns)] = eta;
  }
  __syncthreads();
  for (int idx = tid; idx < S * T; idx += NT) { // predicted_score[t,s] = inv_logit(mu_b[s,t]) (stan:135-139)
    const int t = idx % T, s = idx / T;
    row[c.predicted_score + idx] = d_inv_logit(row[c.mu_b + s + S * t]);
  }
  __syncthreads();
}

// write_array (stan:70-113 transformed parameters, stan:134-140 generated quantities) for saved draws; one 256-thread workgroup per draw
// builds the full CmdStan row in scratch and copies the requested column range.  out layout: [iter][chain][col_end - col_begin].
struct WAParams {
  RowSrc src;
  int n_saved, ncols, col_begin, col_end;
  double *scratch;     // [gridDim.x][ncols]
  double *out;         // [n_saved * chains][out_stride], the first col_end - col_begin entries of a row are written
  int out_stride;
};
// chains_per_ds = 0: every row is built with the one model *Mg; > 0: Mg = [n_datasets] models (potus_set_datasets[_ex]), chain c uses
// Mg[c / chains_per_ds] (mu_b, predicted_score and logit_pi depend on the data set's prior).  Two kernels over this one body: with the
// constant 0 the one model is read once and stays in registers; ONE kernel that read the model per row, or carried it through the loop,
// cost the 8000-row predicted_score launch of the 2016 design 5 % and 1 % (profiles/row_kernels_same_bytes.txt).
__device__ __forceinline__ void wa_write_rows(const DevModel *Mg, const WAParams &W, int chains_per_ds) {
  DevModel M = *Mg;
  __shared__ RowLds lds;
  const int tid = threadIdx.x;
  double *row = W.scratch + (size_t)blockIdx.x * W.ncols;
  for (int d = blockIdx.x; d < W.n_saved * W.src.chains; d += gridDim.x) {
    const int iter = d / W.src.chains, chain = d % W.src.chains;
    if (chains_per_ds) M = Mg[chain / chains_per_ds];
    wa_build_row(M, W.src.at(chain, iter), row, lds);
    const int nsel = W.col_end - W.col_begin;
    double *dst = W.out + (size_t)d * W.out_stride;
    for (int i = tid; i < nsel; i += 256) dst[i] = row[W.col_begin + i];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_write_array(const DevModel *Mg, WAParams W) { wa_write_rows(Mg, W, 0); }
__global__ __launch_bounds__(256) void k_write_array_ds(const DevModel *Mg, WAParams W, int chains_per_ds) { wa_write_rows(Mg, W, chains_per_ds); }

// ------------------------------------------------------------------------ prior predictive simulation and SBC ranks
// y ~ binomial(n, p) with p = inv_logit(eta), exactly: inversion (sequential search from 0) when n min(p, 1 - p) < 10, else BTRS (Hoermann
// 1993, "The generation of binomial random variates", with the exact log-ratio lgamma form of its acceptance bound).  Uniforms of attempt a
// come from Philox counter (iter a, RNG_PRIOR, aux 2 / 3, index idx): BinomCtrPrior, the default.  Another caller gives the uniforms a purpose and a
// counter of its own as Ctr: ctr(key, attempt, kind, idx), kind 2 = u, 3 = v (potus_ppc.hpp).
struct BinomCtrPrior {
  __device__ __forceinline__ double operator()(const RngKey &key, uint32_t att, uint32_t kind, uint32_t idx) const { return rng_uniform(key, att, RNG_PRIOR, kind, idx); }
};
template <class Ctr = BinomCtrPrior>
__device__ int binomial_logit_draw(const RngKey &key, uint32_t idx, int n, double eta, const Ctr ctr = Ctr()) {
  if (n <= 0) return 0;
  const double e = exp(-fabs(eta));
  const double p = e / (1.0 + e), q = 1.0 / (1.0 + e);          // p = min(pi, 1 - pi), computed without cancellation
  const bool flip = eta > 0;
  int k = 0;
  if ((double)n * p < 10.0) {
    const double s = p / q, a = (n + 1) * s, r0 = pow(q, (double)n);
    for (uint32_t att = 0; att < 64; att++) {
      double u = ctr(key, att, 2, idx), r = r0;
      int x = 0;
      while (u > r && x <= n) { u -= r; x++; r *= a / x - s; }
      k = x;
      if (x <= n) break;                                            // (x > n: the rounding of the cumulative sum ran out; draw again)
    }
    k = min(k, n);
  } else {
    const double spq = sqrt(n * p * q), b = 1.15 + 2.53 * spq, a = -0.0873 + 0.0248 * b + 0.01 * p, c = n * p + 0.5;
    const double vr = 0.92 - 4.2 / b, alpha = (2.83 + 5.1 / b) * spq, lpq = log(p / q), m = floor((n + 1) * p);
    const double h = lgamma(m + 1.0) + lgamma(n - m + 1.0);
    for (uint32_t att = 0; att < 4096; att++) {
      const double u = ctr(key, att, 2, idx) - 0.5, v0 = ctr(key, att, 3, idx);
      const double us = 0.5 - fabs(u), kk = floor((2.0 * a / us + b) * u + c);
      if (kk < 0.0 || kk > (double)n) continue;
      k = (int)kk;
      if (us >= 0.07 && v0 <= vr) break;
      const double v = log(v0 * alpha / (a / (us * us) + b));
      if (v <= h - lgamma(kk + 1.0) - lgamma(n - kk + 1.0) + (kk - m) * lpq) break;
    }
  }
  return flip ? n - k : k;
}

struct SimParams {
  double *qrow;        // [n][7 + D]: sampler columns zero, then the drawn unconstrained point
  double *scratch;     // [gridDim.x][ncols]
  int *y;              // [n][Ns + Nn]: state polls, then national polls, in the caller's order
  int n, ncols, sim_offset;
  unsigned seed_lo, seed_hi;
};
// One workgroup per simulation: theta ~ prior (stan:116-128 on the unconstrained scale), logit_pi by the row builder, y ~ binomial.
// Counters (key chain field = sim_offset + sim + 1, so a simulation's bytes do not depend on the batching) are listed in potus_hmc.h.
__global__ __launch_bounds__(256) void k_simulate_prior(const DevModel *Mg, SimParams P) {
  const DevModel M = *Mg;
  __shared__ RowLds lds;
  const int tid = threadIdx.x, D = M.D, Ns = M.Ns;
  const RowCols c = row_cols(M);
  double *row = P.scratch + (size_t)blockIdx.x * P.ncols;
  for (int sim = blockIdx.x; sim < P.n; sim += gridDim.x) {
    const RngKey key{P.seed_lo, P.seed_hi, (uint32_t)(P.sim_offset + sim + 1)};
    double *src = P.qrow + (size_t)sim * (POTUS_N_SAMPLER_COLS + D);
    double *q = src + POTUS_N_SAMPLER_COLS;
    if (tid < POTUS_N_SAMPLER_COLS) src[tid] = 0.0;
    for (int j = tid; 2 * j < D; j += 256) {
      double z0, z1;
      rng_normal_pair(key, 0, RNG_PRIOR, 0, (uint32_t)j, z0, z1);
      q[2 * j] = z0;
      if (2 * j + 1 < D) q[2 * j + 1] = z1;
    }
    __syncthreads();
    if (M.full && tid == 0) {   // rho_e_bias ~ normal(0.7, 0.1) restricted to (0, 1): rejection; P(reject) = 1.3e-3
      double rho = 0.7;
      for (uint32_t att = 0; att < 256; att++) {
        double z0, z1;
        rng_normal_pair(key, 0, RNG_PRIOR, 1, att, z0, z1);
        const double r = 0.7 + 0.1 * z0;
        if (r > 0.0 && r < 1.0) { rho = r; break; }
      }
      q[M.o_rho] = log(rho / (1.0 - rho));
    }
    __syncthreads();
    wa_build_row(M, src, row, lds);
    for (int i = tid; i < M.Npoll; i += 256) {
      const int qi = M.pi[5 * M.Npad + i];
      const bool nat = M.pi[i] == M.S;
      const int j = nat ? qi - M.o_nn : qi - M.o_ns;
      const uint32_t idx = (uint32_t)(nat ? Ns + j : j);
      P.y[(size_t)sim * M.Npoll + idx] = binomial_logit_draw(key, idx, (int)M.pd[M.Npad + i], row[nat ? c.logit_pi_national + j : c.logit_pi_state + j]);
    }
    __syncthreads();
  }
}

struct RankParams {
  RowSrc src;
  int ncols, col_begin, col_end;
  int thin, L, chains_per_ds;   // saved draws src.first, src.first + thin, ... (L of them) of every chain
  const double *truth; // [n_datasets][col_end - col_begin]
  const int *skip;     // [chains]: nonzero = the chain failed, its counts stay zero
  double *scratch;     // [gridDim.x][ncols]
  int *less, *equal;   // [chains][col_end - col_begin]
};
// One workgroup per chain: each compared draw's output row is rebuilt (wa_build_row) and compared with the truth of the chain's data
// set; a thread owns the same columns for the whole launch, so its counts are plain loads and stores.
__global__ __launch_bounds__(256) void k_sbc_ranks(const DevModel *Mg, RankParams P) {
  const DevModel M = *Mg;
  __shared__ RowLds lds;
  const int tid = threadIdx.x, nsel = P.col_end - P.col_begin;
  double *row = P.scratch + (size_t)blockIdx.x * P.ncols;
  for (int chain = blockIdx.x; chain < P.src.chains; chain += gridDim.x) {
    const double *tr = P.truth + (size_t)(chain / P.chains_per_ds) * nsel;
    int *ls = P.less + (size_t)chain * nsel, *eq = P.equal + (size_t)chain * nsel;
    for (int i = tid; i < nsel; i += 256) { ls[i] = 0; eq[i] = 0; }
    if (P.skip[chain]) continue;
    for (int j = 0; j < P.L; j++) {
      wa_build_row(M, P.src.at(chain, j * P.thin), row, lds);
      for (int i = tid; i < nsel; i += 256) {
        const double v = row[P.col_begin + i], t = tr[i];
        ls[i] += v < t ? 1 : 0;
        eq[i] += v == t ? 1 : 0;
      }
      __syncthreads();
    }
  }
}
// Counts per data set: [n_datasets][nsel] = sum over the data set's chains.
__global__ __launch_bounds__(256) void k_sbc_reduce(const int *less, const int *equal, int n_ds, int chains_per_ds, int nsel, int *less_out, int *equal_out) {
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < (long long)n_ds * nsel; k += (long long)gridDim.x * 256) {
    const int ds = (int)(k / nsel), i = (int)(k % nsel);
    int a = 0, b = 0;
    for (int c = ds * chains_per_ds; c < (ds + 1) * chains_per_ds; c++) { a += less[(size_t)c * nsel + i]; b += equal[(size_t)c * nsel + i]; }
    less_out[k] = a; equal_out[k] = b;
  }
}
