// potus_eloo.hpp -- E_loo on the device (loo's E_loo): expectations under the posterior that has not seen poll i, from the PSIS weights
// k_loo_psis computes and discards.  DESIGN.md section 4r states the definitions; tests/eloo_ref.py restates them in numpy.
//
// For poll i: r the raw log ratios (-log_lik_i), lw the normalised PSIS log weights of r (smoothed, truncated, logsumexp 0), w = exp(lw)
// (a weight of -inf is 0), rho = exp(r - max r).  For a quantity x[s]:
//   mean      sum w x;   variance  sum w (x - mean)^2 (a second pass);   sd  its square root
//   quantile  equal weights: type 7.  Otherwise x sorted ascending (ties by draw index) with w carried along, ww = cumsum(w) / sum w, j the first
//             index with ww[j] >= p: x[0] when j = 0, else x[j-1] + (x[j] - x[j-1]) (p - ww[j-1]) / (ww[j] - ww[j-1])
//   k         mean: h = x, variance and sd: h = x^2: max(k_r, k_hr); quantile, or h constant, two-valued or not finite somewhere: k_r.
//             k_r = k-hat of the right tail of rho (potus_loo's pareto_k), k_hr = the larger k-hat of the right tails of h rho and -h rho;
//             a tail = the M largest values, M = ceil(min(0.2 S, 3 sqrt(S / r_eff))), minus the value just below them, through gpdfit with
//             loo's prior; M < 5 or a spread below DBL_EPSILON / 100: +inf.
// Kernels:
//   k_el_pointwise    x with its own values per poll.  One workgroup of DG_THREADS per poll: r_eff (when not given) and PSIS of r by potus_psis.hpp
//                     (what k_loo_psis and k_mm_psis call), the moments, four sorts on potus_diag.hpp's runs (r, x, x rho, x^2 rho: one sort of
//                     h rho gives both of its tails), the weighted quantiles by a segmented scan in a fixed order.  Every sum is dg_block_sum's: a poll's bytes depend on its own row alone.
//   k_el_colmean      c[j] = the equal-weight mean of column j of X (the posterior mean), one workgroup per column.
//   k_el_shared       X shared by all polls: D1 = W (X - c), D2 = W (X - c)^2 as tiled products on v_mfma_f64_16x16x4_f64.  A workgroup of four
//                     waves owns EL_TM polls x EL_TN columns of one chunk of EL_CHUNK draws; EL_KB draws at a time are staged in LDS, the weights
//                     exponentiated and the columns centred on the way in; a wave multiplies 32 polls x 32 columns (2 x 2 operand tiles, both
//                     moments: 32 accumulator registers).  Partials [chunk][2][polls][columns]; k_el_shared_sum adds the chunks in order and
//                     writes mean = c + D1, variance = D2 - D1^2.  The chunk is a constant, a chunk's draws enter in order, an accumulator
//                     element sees its own poll and column only: an entry's bytes depend on (lw[poll], X[column]) alone.
//   k_el_ess          1 / sum w^2 per poll.
//   k_el_poll_share   per (draw, poll) the expected share E_z[p] and E_z[p^2] of the poll, k_loo_loglik's sibling.
//   k_el_kr           k_r and r_eff per poll from the raw ratios;  k_el_khat  max(k_r, k_hr) of the mean per (poll, column), one workgroup each.
#pragma once
#include "potus_loo_mm.hpp"

#define EL_NK 3          // k of the mean, of variance and sd, of the quantiles
#define EL_MAXP 16       // quantile probabilities per call
#define EL_TM 64         // polls per workgroup of k_el_shared
#define EL_TN 64         // columns per workgroup
#define EL_KB 32         // draws staged in LDS at a time
#define EL_XS (EL_KB + 2)   // LDS row stride (doubles): the operand reads of a half wave fall on distinct banks
#define EL_CHUNK 1024    // draws per partial sum
#define EL_THREADS 256

#define EL_ROWS 3         // a workgroup's rows of S doubles behind the PSIS scratch (PsisPtrs::end): lwn | xs | ws

// h constant, two-valued or not finite somewhere: its k is k_r
template <class H>
__device__ bool el_plain(H h, long long S, PsisLds &L) {
  const int tid = threadIdx.x;
  int bad = 0;
  double mx = -INFINITY, mn = INFINITY;
  for (long long j = tid; j < S; j += DG_THREADS) { const double v = h(j); bad |= !isfinite(v); mx = fmax(mx, v); mn = fmin(mn, v); }
  if (__syncthreads_or(bad)) return true;
  mx = dg_block_max(mx, L.red);
  mn = -dg_block_max(-mn, L.red);
  int other = 0;
  for (long long j = tid; j < S; j += DG_THREADS) { const double v = h(j); other |= (v != mn && v != mx); }
  return !__syncthreads_or(other);
}

// the larger k-hat of the right tails of v and of -v (v finite): one sort; the right tail of -v is the left tail of v, negated
template <class F>
__device__ double el_khat_both(F val, long long S, long long Mt, const PsisPtrs &Q, PsisLds &L) {
  if (Mt < 5) return INFINITY;
  const int tid = threadIdx.x;
  double *tr = Q.tail, *tn = Q.tail + S / 2;              // [0] = the cutoff, [1 .. M] the tail ascending (M + 1 <= 0.2 S + 2 <= S / 2 from S = 7)
  dg_sort_runs(val, S, Q.R);
  for (long long j = tid; j < S; j += DG_THREADS) {
    const double v = val(j);
    const long long r0 = dg_rank(v, j, S, Q.R) - 1;
    if (r0 >= S - Mt - 1) tr[r0 - (S - Mt - 1)] = v;
    if (r0 <= Mt) tn[Mt - r0] = -v + 0.0;
  }
  __threadfence_block();
  __syncthreads();
  double k = -INFINITY;
  for (int side = 0; side < 2; side++) {
    const double *t = side ? tn : tr;
    double ks = INFINITY;
    if (psis_tail_varies(t + 1, Mt)) {
      const int N = (int)Mt;
      for (int j = tid; j < N; j += DG_THREADS) Q.xc[j] = t[1 + j] - t[0];
      __threadfence_block();
      __syncthreads();
      double sigma;
      ks = psis_gpdfit(Q.xc, N, Q.th, Q.lth, L, &sigma);
    }
    k = fmax(k, ks);
    __syncthreads();
  }
  return k;
}

// the ratios of a poll: false (and NaN to report) when they hold a NaN or +inf, no finite value, or a -inf without a given r_eff
__device__ bool el_ratio_range(const double *r, long long S, bool given, PsisLds &L, double *rmax_, double *rmin_) {
  int bad = 0, low = 0;
  double rmax = -INFINITY, rmin = INFINITY;
  for (long long j = threadIdx.x; j < S; j += DG_THREADS) { const double v = r[j]; bad |= (isnan(v) || v == INFINITY); low |= (v == -INFINITY); rmax = fmax(rmax, v); rmin = fmin(rmin, v); }
  *rmax_ = rmax = dg_block_max(rmax, L.red);
  *rmin_ = -dg_block_max(-rmin, L.red);
  bad = __syncthreads_or(bad);
  low = __syncthreads_or(low);
  return !(bad || rmax == -INFINITY || (low && !given));
}

// r_eff (the given one, or that of exp(-r + min r) = exp(ll - max ll)) and PSIS of the finite-maximum ratios r [C][n]: the normalised log weights
// into lwo, k_r returned
__device__ __forceinline__ double el_psis(const double *r, double rmax, double rmin, const double *r_eff, int C, long long n, const PsisPtrs &Q, PsisLds &L,
                                          PsisReffLds &G, double *lwo, double *reff_out) {
  const double reff = r_eff ? *r_eff : psis_reff([&](long long j) { return exp(-r[j] + rmin); }, C, n, Q.xc, L, G);
  auto lwv = [&](long long j) { return r[j] - rmax + 0.0; };
  const PsisTail T = psis_tail(lwv, (long long)C * n, reff, Q, L);
  psis_normalise(lwv, T, L, lwo);
  *reff_out = reff;
  return T.khat;
}

// ---- the pointwise form
struct ElPwParams {
  const double *x, *r;        // [NP][C][n]
  const double *r_eff;        // [NP], or null: computed
  PsisWork W;                 // stride: psis_ws_doubles(S, EL_ROWS)
  double *out;                // [NP][3 + np]: mean, variance, sd, quantiles
  double *khat;               // [NP][EL_NK]
  double probs[EL_MAXP];
  long long n;
  int C, NP, np;
};

__global__ __launch_bounds__(DG_THREADS) void k_el_pointwise(ElPwParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long el_dyn[];   // min(npad, DG_RUN) keys, then the indices (a symbol of its own, as k_mm_psis's)
  __shared__ PsisLds L;
  __shared__ PsisReffLds G;
  __shared__ double seg[DG_THREADS + 1];
  const int tid = threadIdx.x, np = P.np;
  const long long n = P.n, S = (long long)P.C * n;
  const PsisPtrs Q = psis_ptrs(P.W, S, el_dyn);
  double *const lwn = Q.end, *const xs = lwn + S, *const ws = xs + S;
  for (int p = blockIdx.x; p < P.NP; p += gridDim.x) {
    const double *x = P.x + (size_t)p * S, *r = P.r + (size_t)p * S;
    double *o = P.out + (size_t)p * (3 + np), *ko = P.khat + (size_t)p * EL_NK;
    // a NaN or +inf ratio, no finite ratio, or a -inf ratio without a given r_eff (its r_eff is that of exp(-r)): NaN
    double rmax, rmin;
    if (!el_ratio_range(r, S, P.r_eff != nullptr, L, &rmax, &rmin)) {
      for (int k = tid; k < 3 + np; k += DG_THREADS) o[k] = NAN;
      if (tid < EL_NK) ko[tid] = NAN;
      continue;
    }
    double reff;
    const double k_r = el_psis(r, rmax, rmin, P.r_eff ? P.r_eff + p : nullptr, P.C, n, Q, L, G, lwn, &reff);
    const double *lw = lwn;
    // ---- mean, then the variance about it
    double a = 0.0, lmx = -INFINITY, lmn = INFINITY;
    for (long long j = tid; j < S; j += DG_THREADS) { const double l = lw[j]; a += exp(l) * x[j]; lmx = fmax(lmx, l); lmn = fmin(lmn, l); }
    const double mean = dg_block_sum(a, L.red);
    lmx = dg_block_max(lmx, L.red);
    lmn = -dg_block_max(-lmn, L.red);
    double q = 0.0;
    for (long long j = tid; j < S; j += DG_THREADS) { const double d = x[j] - mean; q += exp(lw[j]) * (d * d); }
    const double var = dg_block_sum(q, L.red);
    // ---- k of the mean (h = x) and of variance and sd (h = x^2)
    const long long Mt = psis_tail_len(S, reff);
    auto h1 = [&](long long j) { return x[j]; };
    auto h2 = [&](long long j) { return x[j] * x[j]; };
    auto v1 = [&](long long j) { return x[j] * exp(r[j] - rmax) + 0.0; };
    auto v2 = [&](long long j) { return x[j] * x[j] * exp(r[j] - rmax) + 0.0; };
    const double k1 = el_plain(h1, S, L) ? k_r : fmax(k_r, el_khat_both(v1, S, Mt, Q, L));
    const double k2 = el_plain(h2, S, L) ? k_r : fmax(k_r, el_khat_both(v2, S, Mt, Q, L));
    if (tid == 0) { o[0] = mean; o[1] = var; o[2] = sqrt(var); ko[0] = k1; ko[1] = k2; ko[2] = k_r; }
    // ---- quantiles: x sorted (ties by draw index), the weights carried along
    if (np > 0) {
      auto xv = [&](long long j) { return x[j] + 0.0; };
      dg_sort_runs(xv, S, Q.R);
      for (long long j = tid; j < S; j += DG_THREADS) {
        const double v = xv(j);
        const long long r0 = dg_rank(v, j, S, Q.R) - 1;
        xs[r0] = v; ws[r0] = exp(lw[j]);
      }
      __threadfence_block();
      __syncthreads();
      if (lmx == lmn) {                                   // equal weights: type 7 (numpy's linear interpolation, its two-sided form)
        if (tid < np) {
          const double hh = (double)(S - 1) * P.probs[tid], fl = floor(hh), g = hh - fl;
          const long long lo = (long long)fl, hi = lo + 1 < S ? lo + 1 : S - 1;
          const double xa = xs[lo], xb = xs[hi], d = xb - xa;
          o[3 + tid] = g >= 0.5 ? xb - d * (1.0 - g) : xa + d * g;
        }
      } else {
        // cum[j] = (the sum of the segments before j's) + (the sum within j's segment up to j), each added in index order
        const long long len = (S + DG_THREADS - 1) / DG_THREADS, j0 = (long long)tid * len, j1 = j0 + len < S ? j0 + len : S;
        double s = 0.0;
        for (long long j = j0; j < j1; j++) s += ws[j];
        seg[tid + 1] = s;
        __syncthreads();
        if (tid == 0) {
          seg[0] = 0.0;
          for (int t = 1; t <= DG_THREADS; t++) seg[t] += seg[t - 1];
        }
        __syncthreads();
        const double pre = seg[tid], tot = seg[DG_THREADS];
        double loc = 0.0, wprev = pre / tot;
        for (long long j = j0; j < j1; j++) {
          loc += ws[j];
          const double wj = (pre + loc) / tot;
          for (int i = 0; i < np; i++) {
            const double pr = P.probs[i];
            if (wj >= pr && (j == 0 || wprev < pr))
              o[3 + i] = j == 0 ? xs[0] : xs[j - 1] + (xs[j] - xs[j - 1]) * (pr - wprev) / (wj - wprev);
          }
          wprev = wj;
        }
      }
    }
    __syncthreads();
  }
}

// ---- what the model expects of a poll: k_loo_loglik's sibling (the same row rebuild, poll numbering and eta)
// Per (draw, poll) a1 = E_z[p], a2 = E_z[p^2], p = inv_logit(eta + sigma z): integrate = 0 at the draw's own noise coordinate (a2 = a1^2);
// integrate = 1 over z ~ N(0, 1) by the 16 Gauss-Hermite nodes of potus_loo.hpp centred at 0 (z = sqrt(2) x_k, weight w_k / sqrt(pi)): the
// integrand is a bounded sigmoid, not the peaked likelihood, so the rule needs no mode search (its error against quad).
struct ElShareParams {
  RowSrc src;
  int ncols, n_post;
  int p0, p1, integrate;
  double *scratch;      // [gridDim.x][ncols]
  double *a1, *a2;      // [n_post][chains][p1 - p0]
};
__global__ __launch_bounds__(256) void k_el_poll_share(const DevModel *Mg, ElShareParams P) {
  const DevModel M = *Mg;
  __shared__ RowLds lds;
  const int tid = threadIdx.x, nb = P.p1 - P.p0, Np = M.Npad;
  const RowCols c = row_cols(M);
  double *row = P.scratch + (size_t)blockIdx.x * P.ncols;
  for (long long d = blockIdx.x; d < (long long)P.n_post * P.src.chains; d += gridDim.x) {
    const int iter = (int)(d / P.src.chains), chain = (int)(d % P.src.chains);
    const double *src = P.src.at(chain, iter), *q = src + POTUS_N_SAMPLER_COLS;
    wa_build_row(M, src, row, lds);
    for (int i = tid; i < M.Npoll; i += 256) {
      const int s = M.pi[i], qi = M.pi[5 * Np + i];
      const bool nat = s == M.S;
      const int k = nat ? M.Ns + (qi - M.o_nn) : qi - M.o_ns;
      if (k < P.p0 || k >= P.p1) continue;
      double eta = row_poll_eta(M, c, row, M.pd + 2 * Np, i);
      eta += nat ? row[c.nat_polling_bias] : row[c.polling_bias + s];
      const double sig = M.pd[3 * Np + i];
      double a1, a2;
      if (!P.integrate || sig == 0.0) {
        const double p = loo_inv_logit(P.integrate ? eta : eta + sig * q[qi]);
        a1 = p; a2 = p * p;
      } else {
        a1 = 0.0; a2 = 0.0;
#pragma unroll
        for (int g = 0; g < LOO_GH; g++) {
          const double x = loo_gh_x[g], wg = exp(loo_gh_lw[g] - x * x), p = loo_inv_logit(eta + sig * 1.4142135623730951 * x);
          a1 += wg * p; a2 += wg * p * p;
        }
        a1 *= 0.56418958354775629;   // 1 / sqrt(pi)
        a2 *= 0.56418958354775629;
      }
      P.a1[(size_t)d * nb + k - P.p0] = a1;
      P.a2[(size_t)d * nb + k - P.p0] = a2;
    }
    __syncthreads();
  }
}

// ---- the shared form
// c[j] = sum_s X[j][s] / S, one workgroup per column, dg_block_sum's order
__global__ __launch_bounds__(DG_THREADS) void k_el_colmean(const double *X, double *c, long long S, int NC) {
  __shared__ double red[DG_THREADS / 64];
  for (int j = blockIdx.x; j < NC; j += gridDim.x) {
    const double *x = X + (size_t)j * S;
    double a = 0.0;
    for (long long s = threadIdx.x; s < S; s += DG_THREADS) a += x[s];
    const double t = dg_block_sum(a, red);
    if (threadIdx.x == 0) c[j] = t / (double)S;
  }
}

// the forecast columns of a handle's scores sc [draws][nd][S] (canonical order) into X [columns][Stot] at draw offset off.  full: the 2 S + 3
// columns of the one day (scores, national = sum_s w[s] x[s] in state order, indicators x > 0.5, electoral college won, electoral votes);
// otherwise column d (S + 1) + s = score s of day d, d (S + 1) + S = the national vote of day d.
struct ElColParams {
  const double *sc, *w, *ev;
  double *X;
  long long n_h, Stot, off;
  int nd, S, full;
  double ev_to_win;
};
__global__ __launch_bounds__(256) void k_el_columns(ElColParams P) {
  const long long items = P.n_h * P.nd;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < items; e += (long long)gridDim.x * 256) {
    const long long draw = e % P.n_h;
    const int d = (int)(e / P.n_h), S = P.S;
    const double *x = P.sc + ((size_t)draw * P.nd + d) * S;
    double *o = P.X + P.off + draw;
    double nat = 0.0, evs = 0.0;
    const size_t base = P.full ? 0 : (size_t)d * (S + 1);
    for (int s = 0; s < S; s++) {
      const double v = x[s], won = v > 0.5 ? 1.0 : 0.0;
      nat += P.w[s] * v;
      o[(base + s) * P.Stot] = v;
      if (P.full) { evs += P.ev[s] * won; o[(size_t)(S + 1 + s) * P.Stot] = won; }
    }
    o[(base + S) * P.Stot] = nat;
    if (P.full) { o[(size_t)(2 * S + 1) * P.Stot] = evs >= P.ev_to_win ? 1.0 : 0.0; o[(size_t)(2 * S + 2) * P.Stot] = evs; }
  }
}

struct ElShParams {
  const double *X;            // [NC][S]
  const double *lw;           // [NP][S] normalised log weights
  const double *c;            // [NC] the centres
  double *part;               // [nchunk][2][NP][NC]
  long long S;
  int NP, NC;
};
// v_mfma_f64_16x16x4_f64: D[m][n] += sum_k A[m][k] B[k][n]; lane l feeds A[l & 15][l >> 4] and B[l >> 4][l & 15], holds D[(l >> 4) + 4 v][l & 15].
// Here m = a poll, k = a draw, n = a column: A[m][k] = exp(lw[poll m][draw k]), B[k][n] = X[column n][draw k] - c[n] (second moment: its square).
__global__ __launch_bounds__(EL_THREADS) void k_el_shared(ElShParams P) {
  __shared__ double wl[EL_TM][EL_XS], xl[EL_TN][EL_XS];
  typedef double d4_t __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c0 = blockIdx.x * EL_TN, p0 = blockIdx.y * EL_TM, ch = blockIdx.z;
  const long long S = P.S, s0 = (long long)ch * EL_CHUNK, s1 = s0 + EL_CHUNK < S ? s0 + EL_CHUNK : S;
  const int wm = (w >> 1) * 32, wn = (w & 1) * 32, m = lane & 15, kq = lane >> 4;
  d4_t a1[2][2], a2[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) { a1[i][j] = d4_t{0.0, 0.0, 0.0, 0.0}; a2[i][j] = d4_t{0.0, 0.0, 0.0, 0.0}; }
  const int sk = tid & (EL_KB - 1), sr = tid / EL_KB;     // staging: consecutive threads read consecutive draws of one row
  for (long long t0 = s0; t0 < s1; t0 += EL_KB) {
    __syncthreads();
    const long long s = t0 + sk;
#pragma unroll
    for (int i = 0; i < EL_TM / (EL_THREADS / EL_KB); i++) {
      const int row = sr + (EL_THREADS / EL_KB) * i;
      double wv = 0.0, xv = 0.0;
      if (s < s1) {
        if (p0 + row < P.NP) wv = exp(P.lw[(size_t)(p0 + row) * S + s]);
        if (c0 + row < P.NC) xv = P.X[(size_t)(c0 + row) * S + s] - P.c[c0 + row];
      }
      wl[row][sk] = wv; xl[row][sk] = xv;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < EL_KB / 4; kk++) {
      double av[2], bv[2], b2[2];
#pragma unroll
      for (int i = 0; i < 2; i++) { av[i] = wl[wm + 16 * i + m][4 * kk + kq]; bv[i] = xl[wn + 16 * i + m][4 * kk + kq]; b2[i] = bv[i] * bv[i]; }
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
          a1[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], a1[i][j], 0, 0, 0);
          a2[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], b2[j], a2[i][j], 0, 0, 0);
        }
    }
  }
  // D[(l >> 4) + 4 v][l & 15]: poll p0 + wm + 16 i + kq + 4 v, column c0 + wn + 16 j + m
  const size_t PC = (size_t)P.NP * P.NC;
  double *o1 = P.part + (size_t)ch * 2 * PC, *o2 = o1 + PC;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int pl = p0 + wm + 16 * i + kq + 4 * v, cl = c0 + wn + 16 * j + m;
        if (pl < P.NP && cl < P.NC) { o1[(size_t)pl * P.NC + cl] = a1[i][j][v]; o2[(size_t)pl * P.NC + cl] = a2[i][j][v]; }
      }
}
// mean = c + sum of the chunks' D1, variance = sum of the chunks' D2 - D1^2, the chunks in order
__global__ __launch_bounds__(256) void k_el_shared_sum(const double *part, const double *c, double *mean, double *var, int nchunk, int NP, int NC) {
  const long long PC = (long long)NP * NC;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < PC; e += (long long)gridDim.x * 256) {
    double d1 = 0.0, d2 = 0.0;
    for (int k = 0; k < nchunk; k++) { d1 += part[(size_t)k * 2 * PC + e]; d2 += part[(size_t)k * 2 * PC + PC + e]; }
    mean[e] = c[e % NC] + d1;
    var[e] = d2 - d1 * d1;
  }
}
// ess[p] = 1 / sum_s w^2
__global__ __launch_bounds__(DG_THREADS) void k_el_ess(const double *lw, double *ess, long long S, int NP) {
  __shared__ double red[DG_THREADS / 64];
  for (int p = blockIdx.x; p < NP; p += gridDim.x) {
    const double *l = lw + (size_t)p * S;
    double a = 0.0;
    for (long long s = threadIdx.x; s < S; s += DG_THREADS) { const double wv = exp(l[s]); a += wv * wv; }
    const double t = dg_block_sum(a, red);
    if (threadIdx.x == 0) ess[p] = 1.0 / t;
  }
}

struct ElKParams {
  const double *X;            // [NC][S] (k_el_khat)
  const double *r;            // [NP][S] raw log ratios
  const double *r_eff;        // [NP] given, or null: computed
  PsisWork W;                 // stride: psis_ws_doubles(S, EL_ROWS)
  double *kr, *reff;          // [NP]
  double *khat;               // [NP][NC] (k_el_khat)
  long long n;
  int C, NP, NC;
};
__global__ __launch_bounds__(DG_THREADS) void k_el_kr(ElKParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long el_dyn[];
  __shared__ PsisLds L;
  __shared__ PsisReffLds G;
  const long long S = (long long)P.C * P.n;
  const PsisPtrs Q = psis_ptrs(P.W, S, el_dyn);
  for (int p = blockIdx.x; p < P.NP; p += gridDim.x) {
    const double *r = P.r + (size_t)p * S;
    double rmax, rmin;
    if (!el_ratio_range(r, S, P.r_eff != nullptr, L, &rmax, &rmin)) {
      if (threadIdx.x == 0) { P.kr[p] = NAN; P.reff[p] = NAN; }
      continue;
    }
    double reff;
    const double k = el_psis(r, rmax, rmin, P.r_eff ? P.r_eff + p : nullptr, P.C, P.n, Q, L, G, Q.end, &reff);
    if (threadIdx.x == 0) { P.kr[p] = k; P.reff[p] = reff; }
    __syncthreads();
  }
}
// khat[p][j] = k of the mean of column j under poll p's weights, after k_el_kr
__global__ __launch_bounds__(DG_THREADS) void k_el_khat(ElKParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long el_dyn[];
  __shared__ PsisLds L;
  const long long S = (long long)P.C * P.n, items = (long long)P.NP * P.NC;
  const PsisPtrs Q = psis_ptrs(P.W, S, el_dyn);
  for (long long e = blockIdx.x; e < items; e += gridDim.x) {
    const int p = (int)(e / P.NC), j = (int)(e % P.NC);
    const double *r = P.r + (size_t)p * S, *x = P.X + (size_t)j * S;
    const double k_r = P.kr[p], reff = P.reff[p];
    double k = k_r;
    if (!isnan(k_r)) {
      double rmax = -INFINITY;
      for (long long s = threadIdx.x; s < S; s += DG_THREADS) rmax = fmax(rmax, r[s]);
      rmax = dg_block_max(rmax, L.red);
      const long long Mt = psis_tail_len(S, reff);
      auto h1 = [&](long long s) { return x[s]; };
      auto v1 = [&](long long s) { return x[s] * exp(r[s] - rmax) + 0.0; };
      if (!el_plain(h1, S, L)) k = fmax(k_r, el_khat_both(v1, S, Mt, Q, L));
    }
    if (threadIdx.x == 0) P.khat[e] = k;
    __syncthreads();
  }
}
