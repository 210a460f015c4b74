// potus_loo_mm.hpp -- moment matching for PSIS-LOO on the device (Paananen, Piironen, Buerkner, Vehtari 2021; loo's loo_moment_match
// without its covariance step).  DESIGN.md section 4q; the sequential rules are potus_loo_mm_rules.hpp.
//
// Per poll b the state is a diagonal affine map T(theta) = a_b + b_b * theta of the pooled draws theta_s.  No transformed copy of the
// draws exists: the pass applies the map on load, the moments are those of the untransformed draws.
// Kernels:
//   k_mm_pass      workgroups of PT_THREADS walk the items (poll b, draw s).  Per item: the point theta, T theta or T^-1 theta = (theta - a) / b
//                  (sel[b]: MM_SEL_*; MM_SEL_SPLIT takes T at even iterations of a chain and T^-1 at odd ones) goes into the workgroup's
//                  scratch, model_pass under PlainPolicy (the device code of k_lap_lp) gives lp, wa_build_row rebuilds the output row and
//                  thread 0 evaluates poll b's eta and loo_poll_ll with k_loo_loglik's terms in its order.  Everything around the pass
//                  is out of line (mm_point, mm_after), so the pass keeps the registers it has in k_logprob_grad.  Outputs lp, ll
//                  [B][S], s = chain * n + iteration.  An item's bytes depend on (theta_s, a_b, b_b, poll) alone.
//   k_mm_moments   mu~[b][j] = sum_s w[b][s] theta[s][j], q~[b][j] = sum_s w[b][s] (theta[s][j] - m0[j])^2 for a tile of MM_BT = 16
//                  polls in one streaming pass: a workgroup owns 256 columns (one per thread, lanes on consecutive addresses) and one
//                  chunk of MM_CHUNK draws, the weights of the chunk staged in LDS MM_STAGE draws at a time; 32 FMAs per loaded double.
//                  Partials [chunk][b][2][D]; k_mm_moments_sum adds the chunks in order.  The chunk is a constant, the draws of a
//                  chunk are summed in order: an entry's bytes depend on (w[b], theta[:, j], m0[j]) alone, not on the other polls or the grid.
//   k_mm_ratio     the log ratios of a round from lp, ll and lp0: start, candidate or split (see MmRatioParams).
//   k_mm_psis      PSIS of general log ratios, one workgroup per poll: potus_psis.hpp's tail step and normalisation (k_loo_psis's, on r
//                  instead of -ll), with the normalised log weights written out.
//   k_mm_final     elpd[b] = logsumexp_s(ll[b][s] + lw[b][s]), fixed order.
#pragma once
#include "potus_loo.hpp"

enum { MM_SEL_ID = 0, MM_SEL_T = 1, MM_SEL_TINV = 2, MM_SEL_SPLIT = 3 };
#define MM_BT 16        // polls per tile of k_mm_moments
#define MM_CHUNK 512    // draws per partial sum
#define MM_STAGE 256    // draws whose weights are in LDS at a time

struct MmPassParams {
  const double *const *chain;   // [C] the first post-warm-up row of every pooled chain; rows of `row` doubles, n of them
  const double *a, *b;          // [B][D]
  const int *poll;              // [B] the model's (day-sorted) index of poll b
  const int *sel;               // [B] MM_SEL_*
  const double *lc;             // [Npoll] log C(n, y) in the model's poll order
  double *scratch;              // [gridDim.x][7 + 2 Dpad + ncols]: sampler columns and point | gradient | output row
  double *lp, *ll;              // [B][C n]
  int n, C, B, row, Dpad, ncols, integrate;
};
typedef const MmPassParams AS_C *CMmp;

__host__ __device__ inline size_t mm_scratch_doubles(int Dpad, int ncols) { return (size_t)POTUS_N_SAMPLER_COLS + 1 + 2 * (size_t)Dpad + (size_t)ncols; }

// the point of item d = b S + s into the workgroup's scratch
__device__ __noinline__ void mm_point(const DevModel *Mg, const MmPassParams *Pg, int d_) {
  CMp M = (CMp)uni_ptr(Mg);
  CMmp P = (CMmp)uni_ptr(Pg);
  const int d = (int)uni32((unsigned)d_), S = P->C * P->n, b = d / S, s = d % S, c = s / P->n, it = s % P->n, D = M->D;
  int sel = P->sel[b];
  if (sel == MM_SEL_SPLIT) sel = (it & 1) ? MM_SEL_TINV : MM_SEL_T;
  const double *src = P->chain[c] + (size_t)it * P->row;
  double *x = P->scratch + (size_t)blockIdx.x * mm_scratch_doubles(P->Dpad, P->ncols);
  const double *av = P->a + (size_t)b * D, *bv = P->b + (size_t)b * D;
  for (int i = threadIdx.x; i < POTUS_N_SAMPLER_COLS + D; i += PT_THREADS) {
    double v = src[i];
    if (i >= POTUS_N_SAMPLER_COLS && sel != MM_SEL_ID) {
      const int j = i - POTUS_N_SAMPLER_COLS;
      v = sel == MM_SEL_T ? av[j] + bv[j] * v : (v - av[j]) / bv[j];
    }
    x[i] = v;
  }
  __syncthreads();
}

// after the pass: the row of the point, poll b's log-likelihood, the two outputs
// (the row builder's LDS comes as an argument: an out-of-line function that named lds_dyn itself would put the kernel into the table of
// kernel ids the compiler keeps for such functions, and renumber k_pf_elbo and k_vi_elbo in it)
__device__ __noinline__ void mm_after(const DevModel *Mg, const MmPassParams *Pg, int d_, double lp_, RowLds *rl_) {
  CMmp P = (CMmp)uni_ptr(Pg);
  const DevModel M = *(const DevModel *)uni_ptr(Mg);
  const int d = (int)uni32((unsigned)d_), S = P->C * P->n, b = d / S;
  RowLds &rl = *uni_ptr(rl_);
  double *x = P->scratch + (size_t)blockIdx.x * mm_scratch_doubles(P->Dpad, P->ncols);
  double *row = x + POTUS_N_SAMPLER_COLS + 1 + 2 * (size_t)P->Dpad;
  wa_build_row<PT_THREADS>(M, x, row, rl);
  if (threadIdx.x == 0) {
    const RowCols c = row_cols(M);
    const int i = P->poll[b], Np = M.Npad, st = M.pi[i], qi = M.pi[5 * Np + i];
    double eta = row_poll_eta(M, c, row, M.pd + 2 * Np, i);
    eta += st == M.S ? row[c.nat_polling_bias] : row[c.polling_bias + st];
    P->ll[d] = P->lc[i] + loo_poll_ll(M.pd[i], M.pd[Np + i], eta, M.pd[3 * Np + i], x[POTUS_N_SAMPLER_COLS + qi], P->integrate);
    P->lp[d] = lp_;
  }
  __syncthreads();
}

__global__ __launch_bounds__(PT_THREADS) void k_mm_pass(const DevModel *Mg, const MmPassParams *Pg) {
  CMp M = (CMp)Mg;
  CMmp P = (CMmp)Pg;
  ldp lds = (ldp)lds_dyn;
  const PassStatic pst = model_setup_lds(M, lds);
  const int D = M->D, Dpad = P->Dpad, items = P->B * P->C * P->n;
  double *x = P->scratch + (size_t)blockIdx.x * mm_scratch_doubles(Dpad, P->ncols);
  const rsrc_t rq = make_rsrc(x + POTUS_N_SAMPLER_COLS, 8u * D), rg = make_rsrc(x + POTUS_N_SAMPLER_COLS + 1 + Dpad, 8u * D);
  for (int d = blockIdx.x; d < items; d += gridDim.x) {
    mm_point(Mg, Pg, d);
    PlainPolicy pol{rq, rg, 0u, 0u, {0}};
    const double v = model_pass(M, lds, pst, pol);
    __syncthreads();
    mm_after(Mg, Pg, d, v, (RowLds *)(lds_dyn + M->lds_doubles));
  }
}

// ---- the weighted moments
struct MmMomParams {
  const double *const *chain;   // as MmPassParams
  const double *w;              // [B][S] weights, or log weights (is_log): w = exp(.)
  const double *m0;             // [D], or null: 0
  double *part;                 // [nchunk][B][2][D]
  int n, C, B, row, D, is_log;
};
__global__ __launch_bounds__(256) void k_mm_moments(MmMomParams P) {
  __shared__ double wl[MM_STAGE][MM_BT];
  const int tid = threadIdx.x, j = blockIdx.x * 256 + tid, ch = blockIdx.y, b0 = blockIdx.z * MM_BT, S = P.C * P.n;
  const int s0 = ch * MM_CHUNK, s1 = min(s0 + MM_CHUNK, S);
  const bool live = j < P.D;
  const double m0 = (live && P.m0) ? P.m0[j] : 0.0;
  double mu[MM_BT], q[MM_BT];
#pragma unroll
  for (int k = 0; k < MM_BT; k++) { mu[k] = 0.0; q[k] = 0.0; }
  for (int t0 = s0; t0 < s1; t0 += MM_STAGE) {
    const int nt = min(MM_STAGE, s1 - t0);
    __syncthreads();
    for (int e = tid; e < MM_STAGE * MM_BT; e += 256) {
      const int k = e / MM_STAGE, t = e % MM_STAGE;        // consecutive threads read consecutive draws of one poll
      double v = 0.0;
      if (b0 + k < P.B && t < nt) { v = P.w[(size_t)(b0 + k) * S + t0 + t]; if (P.is_log) v = exp(v); }
      wl[t][k] = v;
    }
    __syncthreads();
    if (live)
      for (int t = 0; t < nt; t++) {
        const int s = t0 + t, c = s / P.n, it = s % P.n;
        const double x = P.chain[c][(size_t)it * P.row + POTUS_N_SAMPLER_COLS + j], dx = x - m0, d2 = dx * dx;
#pragma unroll
        for (int k = 0; k < MM_BT; k++) { const double wv = wl[t][k]; mu[k] = fma(wv, x, mu[k]); q[k] = fma(wv, d2, q[k]); }
      }
  }
  if (live)
#pragma unroll
    for (int k = 0; k < MM_BT; k++)
      if (b0 + k < P.B) {
        double *o = P.part + (((size_t)ch * P.B + b0 + k) * 2) * P.D;
        o[j] = mu[k]; o[P.D + j] = q[k];
      }
}
// out [B][2][D] = the chunks' partials added in order
__global__ __launch_bounds__(256) void k_mm_moments_sum(const double *part, double *out, int nchunk, long long BD2) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < BD2; e += (long long)gridDim.x * 256) {
    double s = 0.0;
    for (int c = 0; c < nchunk; c++) s += part[(size_t)c * BD2 + e];
    out[e] = s;
  }
}

// ---- the log ratios of a round
//   mode 0  start      r = -ll
//   mode 1  candidate  r = -ll + lp - lp0[s]
//   mode 2  split      x = T theta at even iterations, theta at odd ones; lp, ll come from a pass under MM_SEL_SPLIT (T theta | T^-1 theta):
//                      even: llx = ll, lpx = lp, lpi = lp0[s] - slb[b];  odd: llx = ll0[b][s], lpx = lp0[s], lpi = lp - slb[b]
//                      r = -llx + lpx - logaddexp(lpx, lpi); llx is written to llx_out
// A ratio with a term that is not finite is -inf (weight 0).
struct MmRatioParams {
  const double *lp, *ll;    // [B][S] of this round's pass
  const double *lp0;        // [S]
  const double *ll0;        // [B][S] at the untransformed draws (mode 2)
  const double *slb;        // [B] sum_j log b_j (mode 2)
  double *r, *llx_out;      // [B][S]
  int n, S, B, mode;
};
__global__ __launch_bounds__(256) void k_mm_ratio(MmRatioParams P) {
  const long long N = (long long)P.B * P.S;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < N; e += (long long)gridDim.x * 256) {
    const int b = (int)(e / P.S), s = (int)(e % P.S);
    double r;
    if (P.mode == 0) r = -P.ll[e];
    else if (P.mode == 1) {
      const double l = P.ll[e], p = P.lp[e], p0 = P.lp0[s];
      r = (isfinite(l) && isfinite(p) && isfinite(p0)) ? -l + p - p0 : -INFINITY;
    } else {
      const bool even = ((s % P.n) & 1) == 0;
      const double llx = even ? P.ll[e] : P.ll0[e], lpx = even ? P.lp[e] : P.lp0[s], lpi = (even ? P.lp0[s] : P.lp[e]) - P.slb[b];
      const double hi = fmax(lpx, lpi), lae = hi + log1p(exp(-fabs(lpx - lpi)));
      r = -llx + lpx - lae;
      if (!(isfinite(llx) && isfinite(lpx) && isfinite(r))) r = -INFINITY;
      P.llx_out[e] = llx;
    }
    P.r[e] = r;
  }
}

// ---- PSIS of general log ratios
struct PsisGenParams {
  const double *r;            // [NP][S]
  const double *r_eff;        // [NP]
  PsisWork W;
  double *lw;                 // [NP][S] normalised log weights
  double *khat;               // [NP]
  long long S;
  int NP;
};
// A NaN or +inf ratio, or no finite ratio at all: k = NaN and NaN weights (the rules reject a NaN k).
__global__ __launch_bounds__(DG_THREADS) void k_mm_psis(PsisGenParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long mk[];   // min(npad, DG_RUN) keys, then the indices (its own symbol: see DESIGN.md 4q)
  __shared__ PsisLds L;
  const int tid = threadIdx.x;
  const long long S = P.S;
  const PsisPtrs Q = psis_ptrs(P.W, S, mk);
  for (int p = blockIdx.x; p < P.NP; p += gridDim.x) {
    const double *r = P.r + (size_t)p * S;
    double *lwo = P.lw + (size_t)p * S;
    int bad = 0;
    double rmax = -INFINITY;
    for (long long j = tid; j < S; j += DG_THREADS) { const double v = r[j]; bad |= (isnan(v) || v == INFINITY); rmax = fmax(rmax, v); }
    rmax = dg_block_max(rmax, L.red);
    if (__syncthreads_or(bad) || rmax == -INFINITY) {
      for (long long j = tid; j < S; j += DG_THREADS) lwo[j] = NAN;
      if (tid == 0) P.khat[p] = NAN;
      continue;
    }
    auto lwv = [&](long long j) { return r[j] - rmax + 0.0; };
    const PsisTail T = psis_tail(lwv, S, P.r_eff[p], Q, L);
    psis_normalise(lwv, T, L, lwo);
    if (tid == 0) P.khat[p] = T.khat;
    __syncthreads();
  }
}

// elpd[p] = logsumexp_s(ll[p][s] + lw[p][s]); one workgroup per poll, the order of k_loo_psis's last sum
__global__ __launch_bounds__(DG_THREADS) void k_mm_final(const double *ll, const double *lw, double *elpd, long long S, int NP) {
  __shared__ double red[DG_THREADS / 64];
  const int tid = threadIdx.x;
  for (int p = blockIdx.x; p < NP; p += gridDim.x) {
    const double *l = ll + (size_t)p * S, *v = lw + (size_t)p * S;
    double m2 = -INFINITY;
    for (long long j = tid; j < S; j += DG_THREADS) m2 = fmax(m2, l[j] + v[j]);
    m2 = dg_block_max(m2, red);
    double s2 = 0.0;
    for (long long j = tid; j < S; j += DG_THREADS) s2 += exp(l[j] + v[j] - m2);
    const double e = m2 + log(dg_block_sum(s2, red));
    if (tid == 0) elpd[p] = e;
  }
}
