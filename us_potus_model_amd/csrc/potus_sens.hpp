// potus_sens.hpp -- prior sensitivity by refit: how far one set of draws lies from another, per column.  DESIGN.md section 4t.
//
// The settings of a grid of prior scales are the data sets of one handle (potus_set_datasets_grid); what a reader of such a grid asks is how
// far a forecast moved from the baseline's, and whether that is more than two runs of the SAME setting differ by.  k_sg_distance answers with
// three distances between the empirical distribution functions of two samples a [n_a] and b [n_b] of one column.
//
// DEFINITIONS.
//   x_1 < ... < x_m are the distinct values of the union of the two samples.
//   P_j = #{a <= x_j} / n_a.  Q_j is likewise for b.
//   Delta_j = x_{j+1} - x_j for j < m.
//   The three outputs are:
//     w1  = sum_j Delta_j |P_j - Q_j|.  This is the Wasserstein-1 distance, in the column's own units.
//     ks  = max_j |P_j - Q_j|.
//     cjs = max(c(a, b), c(-a, -b)), defined as follows.
//       c(a, b) = sqrt(max(0, C(P||Q) + C(Q||P)) / sum_j Delta_j (P_j + Q_j)).
//       C(P||Q) = sum_j Delta_j P_j log2(P_j / ((P_j + Q_j)/2)) + (1 / (2 ln 2)) sum_j Delta_j (Q_j - P_j), with 0 * log 0 = 0.
//       c = 0 when m = 1.
//       This is the cumulative Jensen-Shannon distance of Nguyen & Vemuri (2015), which Kallioinen et al. (2023) use for power-scaling
//       sensitivity.
//   A non-finite value in either sample of a column makes that column's three outputs NaN, and no other column's.
//
// WHAT THE KERNEL EVALUATES.  The two linear sums of C(P||Q) + C(Q||P) are each other's negative and are left out: the numerator is
// sum_j Delta_j (P_j log2(P_j / M_j) + Q_j log2(Q_j / M_j)), M_j = (P_j + Q_j) / 2.  For the samples -a and -b the distinct values are the
// -x_j in reverse, the gap below -x_j is Delta_j again and the distribution functions on it are 1 - P_j and 1 - Q_j, taken as the integer
// ratios (n_a - #{a <= x_j}) / n_a: the second orientation is a second pair of sums over the same sorted arrays.  -0.0 is read as 0.0.
//
// SHAPE.  One workgroup of SG_THREADS per column, grid-stride over the columns.  Both samples sit in dynamic LDS as the order-preserving keys
// of potus_summary.hpp (ps_key), a's n_a then b's n_b, (n_a + n_b) * 8 bytes, at most SG_MAX_N = 16 384 keys = 128 KB; each is sorted by a
// bitonic network whose every exchange is ascending (sg_sort), which needs no padding to a power of two -- two padded runs of 8 191 and 8 193
// would not fit.  Element i of a sorted sample that is the LAST of its run of equal keys stands for the distinct value x = key[i]: its own
// position gives the count in its sample, a binary search the count in the other; a value present in both is taken from a.  The next distinct
// value is the smaller of the two successors.  Every thread sums its elements (tid, tid + SG_THREADS, ...) in ascending order, then one tree
// over the SG_THREADS partial sums: the order is fixed by n_a and n_b alone, so a column has the same bytes alone and among a thousand, for
// any grid.  No workgroup waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SG_MAX_N PS_RUN
#define SG_THREADS PS_THREADS
#define SG_NSUM 6   // w1, numerator and denominator of c(a, b), the same of c(-a, -b), ks (a maximum)

// ascending bitonic sort of k[0, n) in LDS, any n: the merge of two sorted halves of a block of 2^p starts with the exchange i <-> i ^ (2^p - 1)
// and goes on with i <-> i ^ j, j = 2^(p-2) .. 1, the smaller key always to the lower index.  A partner at or beyond n stands for +infinity and
// is never exchanged, so the network sorts n keys as it would sort them padded.  Ends with a barrier.
__device__ __forceinline__ void sg_sort(unsigned long long *k, int n) {
  for (int blk = 2; (blk >> 1) < n; blk <<= 1)
    for (int j = blk >> 1; j > 0; j >>= 1) {
      const int mask = j == (blk >> 1) ? blk - 1 : j;
      for (int i = threadIdx.x; i < n; i += SG_THREADS) {
        const int l = i ^ mask;
        if (l > i && l < n) {
          const unsigned long long a = k[i], b = k[l];
          if (a > b) { k[i] = b; k[l] = a; }
        }
      }
      __syncthreads();
    }
}
// number of keys <= key in a sorted run
__device__ __forceinline__ int sg_upper(const unsigned long long *run, int n, unsigned long long key) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (run[mid] <= key) lo = mid + 1; else hi = mid; }
  return lo;
}
__device__ __forceinline__ double sg_plog(double p, double m) { return p > 0.0 ? p * log2(p / m) : 0.0; }

// One column: load(i) is element i of the concatenation a | b.  keys [na + nb] and red [SG_NSUM][SG_THREADS] in LDS.  out [3] = w1, ks, cjs.
// Called by every thread of the workgroup; ends with a barrier, so that the next column may overwrite keys and red.
template <class Load>
__device__ void sg_column(unsigned long long *keys, double (*red)[SG_THREADS], int na, int nb, Load load, double *out) {
  const int tid = threadIdx.x, n = na + nb;
  int bad = 0;
  for (int i = tid; i < n; i += SG_THREADS) {
    double v = load(i);
    if (!isfinite(v)) bad = 1;
    if (v == 0.0) v = 0.0;
    keys[i] = ps_key(v);
  }
  bad = __syncthreads_or(bad);
  if (bad) {
    if (tid < 3) out[tid] = NAN;
    __syncthreads();
    return;
  }
  unsigned long long *ka = keys, *kb = keys + na;
  sg_sort(ka, na);
  sg_sort(kb, nb);
  double acc[SG_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += SG_THREADS) {
    const bool in_a = i < na;
    const unsigned long long *own = in_a ? ka : kb, *oth = in_a ? kb : ka;
    const int no = in_a ? na : nb, nt = in_a ? nb : na, p = in_a ? i : i - na;
    const unsigned long long key = own[p];
    if (p + 1 < no && own[p + 1] == key) continue;          // not the last of its run
    const int co = p + 1, ct = sg_upper(oth, nt, key);
    if (!in_a && ct > 0 && oth[ct - 1] == key) continue;    // a value of both samples: a's element has it
    const int ca = in_a ? co : ct, cb = in_a ? ct : co;
    const double P = (double)ca / (double)na, Q = (double)cb / (double)nb;
    acc[5] = fmax(acc[5], fabs(P - Q));
    if (ca == na && cb == nb) continue;                     // x_m: no gap above it
    unsigned long long nx = ~0ull;
    if (ca < na) nx = ka[ca];
    if (cb < nb && kb[cb] < nx) nx = kb[cb];
    const double delta = ps_unkey(nx) - ps_unkey(key);
    const double P2 = (double)(na - ca) / (double)na, Q2 = (double)(nb - cb) / (double)nb;
    const double M = 0.5 * (P + Q), M2 = 0.5 * (P2 + Q2);
    acc[0] += delta * fabs(P - Q);
    acc[1] += delta * (sg_plog(P, M) + sg_plog(Q, M));
    acc[2] += delta * (P + Q);
    acc[3] += delta * (sg_plog(P2, M2) + sg_plog(Q2, M2));
    acc[4] += delta * (P2 + Q2);
  }
  for (int k = 0; k < SG_NSUM; k++) red[k][tid] = acc[k];
  __syncthreads();
  for (int off = SG_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) {
      for (int k = 0; k < 5; k++) red[k][tid] += red[k][tid + off];
      red[5][tid] = fmax(red[5][tid], red[5][tid + off]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double c1 = red[2][0] > 0.0 ? sqrt(fmax(0.0, red[1][0]) / red[2][0]) : 0.0;
    const double c2 = red[4][0] > 0.0 ? sqrt(fmax(0.0, red[3][0]) / red[4][0]) : 0.0;
    out[0] = red[0][0]; out[1] = red[5][0]; out[2] = fmax(c1, c2);
  }
  __syncthreads();
}

// potus_ecdf_distance_device: a [n_a][n_cols], b [n_b][n_cols], draw-major; out [n_cols][3]
__global__ __launch_bounds__(SG_THREADS) void k_sg_distance(const double *a, int na, const double *b, int nb, int n_cols, double *out) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sg_keys[];   // na + nb keys
  __shared__ double red[SG_NSUM][SG_THREADS];
  for (int col = blockIdx.x; col < n_cols; col += gridDim.x)
    sg_column(sg_keys, red, na, nb, [&](int i) { return i < na ? a[(size_t)i * n_cols + col] : b[(size_t)(i - na) * n_cols + col]; }, out + (size_t)col * 3);
}

// potus_grid_compare: every data set against data set `base`, on the scores of k_tl_scores.  One job per (data set, day, column); the columns
// are the S state scores, the weighted national vote and the Democratic electoral votes of a draw, derived as k_tl_summary derives them.
struct SgGridParams {
  const double *x;       // [n_datasets][n][nd][S]
  int n_ds, n, nd, S, base;
  const double *w, *ev;  // [S] normalised state weights; electoral votes
  const int *skip;       // [n_datasets]: a chain of the data set failed
  double *out;           // [n_datasets][nd][S + 2][3]
};
__global__ __launch_bounds__(SG_THREADS) void k_sg_grid(SgGridParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sg_keys[];   // 2 n keys
  __shared__ double red[SG_NSUM][SG_THREADS];
  const int S = P.S, n = P.n, NCOL = S + 2;
  const long long jobs = (long long)P.n_ds * P.nd * NCOL;
  for (long long job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int c = (int)(job % NCOL), day = (int)((job / NCOL) % P.nd), ds = (int)(job / ((long long)NCOL * P.nd));
    double *o = P.out + (size_t)job * 3;
    if (P.skip[ds] || P.skip[P.base]) {   // uniform over the workgroup
      if (threadIdx.x < 3) o[threadIdx.x] = NAN;
      continue;
    }
    const double *xa = P.x + ((size_t)ds * n * P.nd + day) * S, *xb = P.x + ((size_t)P.base * n * P.nd + day) * S;
    sg_column(sg_keys, red, n, n, [&](int i) {
      const double *xr = (i < n ? xa + (size_t)i * P.nd * S : xb + (size_t)(i - n) * P.nd * S);
      if (c < S) return xr[c];
      if (c == S) { double a = 0.0; for (int s = 0; s < S; s++) a += P.w[s] * xr[s]; return a; }   // as k_tl_summary sums it
      double b = 0.0; for (int s = 0; s < S; s++) b += xr[s] > 0.5 ? P.ev[s] : 0.0; return b;
    }, o);
  }
}
