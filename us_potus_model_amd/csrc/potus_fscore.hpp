// potus_fscore.hpp -- proper scoring rules of the joint forecast against the certified result, on the device.  DESIGN.md section 4u.
//
// Every other score of the library reads a marginal summary; these read the forecast DISTRIBUTION: what scoringRules gives an R user as
// crps_sample, es_sample, vs_sample and dss_sample.  The definitions are stated once, in include/potus_hmc.h.
//
// INPUT.  x [n_ds][n][nd][S]: n draws (canonical order) of nd days of predicted_score per data set -- one data set for a block of the caller's
// or a pooled posterior, the data sets of a handle for k_tl_scores' block.  actual [S + 2]; the m USED states as the ascending list uidx [m].
//
// Kernels:
//   k_fs_column        one workgroup per (data set, day, column), grid-stride; columns = the S states, the national vote and the electoral votes
//                      of a draw, derived as k_tl_summary / k_sg_grid derive them.  The column sits in dynamic LDS as ps_key keys (n * 8 bytes, at
//                      most PS_RUN = 16 384 draws), sorted by sg_sort; sums thread-strided over the SORTED column, then a tree: fixed by n alone.
//                      uni [7] = crps, pit_lo, pit_hi, dss, interval, ae_median, se_mean.
//   k_fs_variogram     one workgroup per (data set, day), thread = a pair of used states a < b: sum_i |x_ia - x_ib|^p over chunks of FS_VCHUNK
//                      draws staged in LDS, a chunk's draws in order, the chunk partials added in chunk order; the pairs' terms thread-strided,
//                      then a tree.  Also writes the day's FLAG: a used state of some draw is not finite (the three joint scores are NaN then).
//   k_fs_energy<MB>    the hot path: all pairs of a day, never stored.  The pairs are cut into square tiles of FS_TILE draws per side; only tiles on
//                      or above the diagonal are jobs (grid-stride), and a diagonal tile counts i < j.  The tile's ROW draws are centred on y
//                      and staged in LDS (FS_TILE x MB doubles, MB = m rounded up to eight, the padding zero); lane = one COLUMN draw, centred
//                      the same way, its MB values in registers; threads c and c + FS_TILE share a column and take the lower and the upper half
//                      of the rows.  A pair is MB subtractions and MB fused multiply-adds (two chains: even and odd coordinates, added at the
//                      end) and one sqrt; the row values are LDS broadcasts.  No Gram identity: coincident draws are at distance exactly 0.
//                      The single term |x_i - y| is taken on the diagonal tiles, from the same centred values.  A thread adds its distances in
//                      row order, the tile adds its threads by a tree, and writes one partial per sum: part [job][2].
//   k_fs_energy_finish one wave per (data set, day): the tile partials lane-strided in tile order, then a tree; energy = single / n - pairs / n^2.
//   k_fs_dss           one workgroup per day: the m x m Cholesky factor of the used block of scenario's two-pass covariance (k_sc_sum,
//                      k_sc_gram), the solve and the log determinant.  n <= m or a pivot that is not positive: NaN.
// No floating-point atomics; no workgroup waits for another.  The bytes of a day depend on (n, the used states, FS_TILE, FS_VCHUNK) alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "potus_summary.hpp"
#include "potus_sens.hpp"

#define FS_TILE 128                 // draws per side of a tile of pairs: a constant of the library
#define FS_ETHREADS (2 * FS_TILE)
#define FS_MAX_S 63
#define FS_VCHUNK 64                // draws per partial sum of the variogram score
#define FS_VTHREADS 256
#define FS_VPAIRS 8                 // pairs per thread: 63 * 62 / 2 = 1953 <= 8 * 256
#define FS_NUNI 7
#define FS_NMULTI 3

struct FsParams {
  const double *x;       // [n_ds][n][nd][S]
  int n_ds, n, nd, S, m;
  const double *w, *ev;  // [S] normalised state weights; electoral votes
  const double *actual;  // [S + 2]
  const int *uidx;       // [m]: the used states, ascending
  double vs_p;
  int p_mode;            // 0: pow, 1: sqrt (p = 0.5), 2: p = 1, 3: p = 2
};

// number of keys < key in a sorted run
__device__ __forceinline__ int fs_lower(const unsigned long long *run, int n, unsigned long long key) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (run[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}

// sum of red[k][0 .. PS_THREADS) into red[k][0], k < K; starts and ends with a barrier
template <int K>
__device__ __forceinline__ void fs_tree(double (*red)[PS_THREADS]) {
  __syncthreads();
  for (int off = PS_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off)
      for (int k = 0; k < K; k++) red[k][threadIdx.x] += red[k][threadIdx.x + off];
    __syncthreads();
  }
}

__global__ __launch_bounds__(PS_THREADS) void k_fs_column(FsParams P, double *uni /*[n_ds][nd][S + 2][7]*/) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long fs_keys[];   // n keys
  __shared__ double red[2][PS_THREADS];
  __shared__ int s_cnt[2];
  const int tid = threadIdx.x, S = P.S, n = P.n, NCOL = S + 2;
  const long long jobs = (long long)P.n_ds * P.nd * NCOL;
  for (long long job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int c = (int)(job % NCOL), day = (int)((job / NCOL) % P.nd), ds = (int)(job / ((long long)NCOL * P.nd));
    double *o = uni + (size_t)job * FS_NUNI;
    const double y = P.actual[c] + 0.0;                      // (-0.0 is read as 0.0)
    const double *base = P.x + ((size_t)ds * n * P.nd + day) * S;
    int bad = 0;
    for (int i = tid; i < n; i += PS_THREADS) {
      const double *xr = base + (size_t)i * P.nd * S;
      double v;
      if (c < S) v = xr[c];
      else {                                                 // as k_tl_summary sums them; a state that is not finite spoils both
        double a = 0.0, b = 0.0;
        for (int s = 0; s < S; s++) { const double xs = xr[s]; if (!isfinite(xs)) bad = 1; a += P.w[s] * xs; b += xs > 0.5 ? P.ev[s] : 0.0; }
        v = c == S ? a : b;
      }
      if (!isfinite(v)) bad = 1;
      if (v == 0.0) v = 0.0;
      fs_keys[i] = ps_key(v);
    }
    bad = __syncthreads_or(bad);
    if (bad) {                                               // uniform over the workgroup
      if (tid < FS_NUNI) o[tid] = NAN;
      continue;
    }
    sg_sort(fs_keys, n);
    const unsigned long long ky = ps_key(y);
    if (tid == 0) s_cnt[0] = fs_lower(fs_keys, n, ky);
    if (tid == 64) s_cnt[1] = sg_upper(fs_keys, n, ky);
    double s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < n; i += PS_THREADS) {
      const double x = ps_unkey(fs_keys[i]);
      s1 += x;
      s2 += (x - y) * ((y < x ? (double)n : 0.0) - (double)(i + 1) + 0.5);
    }
    red[0][tid] = s1; red[1][tid] = s2;
    fs_tree<2>(red);
    const double mean = red[0][0] / (double)n, crps_sum = red[1][0];
    __syncthreads();
    double s3 = 0.0;
    for (int i = tid; i < n; i += PS_THREADS) { const double d = ps_unkey(fs_keys[i]) - mean; s3 += d * d; }
    red[0][tid] = s3;
    fs_tree<1>(red);
    if (tid == 0) {
      const double nn = (double)n;
      const bool constant = fs_keys[0] == fs_keys[n - 1];    // every draw the same value: the variance is 0, whatever the sum rounds to
      const double var = n > 1 && !constant ? red[0][0] / (nn - 1.0) : 0.0;
      double q3[3];
      for (int j = 0; j < 3; j++) {
        const double p = j == 0 ? 0.025 : j == 1 ? 0.975 : 0.5;
        q3[j] = ps_q7(n, p, ps_unkey(fs_keys[ps_q7_index(n, p, false)]), ps_unkey(fs_keys[ps_q7_index(n, p, true)]));
      }
      const double lo = q3[0], hi = q3[1];
      o[0] = 2.0 * crps_sum / (nn * nn);
      o[1] = (double)s_cnt[0] / nn;
      o[2] = (double)s_cnt[1] / nn;
      o[3] = var > 0.0 ? log(var) + (y - mean) * (y - mean) / var : NAN;
      o[4] = (hi - lo) + 40.0 * fmax(lo - y, 0.0) + 40.0 * fmax(y - hi, 0.0);
      o[5] = fabs(q3[2] - y);
      o[6] = (mean - y) * (mean - y);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ double fs_pow(double d, double p, int mode) {
  return mode == 1 ? sqrt(d) : mode == 2 ? d : mode == 3 ? d * d : pow(d, p);
}

__global__ __launch_bounds__(FS_VTHREADS) void k_fs_variogram(FsParams P, double *multi /*[n_ds][nd][3]*/, int *flag /*[n_ds][nd]*/) {
  __shared__ double s_x[FS_VCHUNK][FS_MAX_S + 2];            // (65 doubles a row: the pairs of one draw spread over the banks)
  __shared__ double red[FS_VTHREADS];
  const int tid = threadIdx.x, S = P.S, n = P.n, m = P.m, npairs = m * (m - 1) / 2;
  int pa[FS_VPAIRS], pb[FS_VPAIRS];
#pragma unroll
  for (int t = 0; t < FS_VPAIRS; t++) {                      // pair q of the list (0,1), (0,2), ..., (m-2,m-1)
    int q = tid + FS_VTHREADS * t, a = 0;
    pa[t] = pb[t] = 0;
    if (q < npairs) {
      while (q >= m - 1 - a) { q -= m - 1 - a; a++; }
      pa[t] = a; pb[t] = a + 1 + q;
    }
  }
  const int jobs = P.n_ds * P.nd;
  for (int job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int day = job % P.nd, ds = job / P.nd;
    const double *base = P.x + ((size_t)ds * n * P.nd + day) * S;
    double tot[FS_VPAIRS];
#pragma unroll
    for (int t = 0; t < FS_VPAIRS; t++) tot[t] = 0.0;
    int bad = 0;
    for (int c0 = 0; c0 < n; c0 += FS_VCHUNK) {
      const int cn = n - c0 < FS_VCHUNK ? n - c0 : FS_VCHUNK;
      for (int idx = tid; idx < cn * m; idx += FS_VTHREADS) {
        const int i = idx / m, k = idx - i * m;
        const double v = base[(size_t)(c0 + i) * P.nd * S + P.uidx[k]];
        if (!isfinite(v)) bad = 1;
        s_x[i][k] = v;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < FS_VPAIRS; t++)
        if (tid + FS_VTHREADS * t < npairs) {
          double part = 0.0;
          for (int i = 0; i < cn; i++) part += fs_pow(fabs(s_x[i][pa[t]] - s_x[i][pb[t]]), P.vs_p, P.p_mode);
          tot[t] += part;
        }
      __syncthreads();
    }
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < FS_VPAIRS; t++)
      if (tid + FS_VTHREADS * t < npairs) {
        const double e = fs_pow(fabs(P.actual[P.uidx[pa[t]]] - P.actual[P.uidx[pb[t]]]), P.vs_p, P.p_mode) - tot[t] / (double)n;
        acc += e * e;
      }
    red[tid] = acc;
    bad = __syncthreads_or(bad);
    for (int off = FS_VTHREADS / 2; off > 0; off >>= 1) {
      if (tid < off) red[tid] += red[tid + off];
      __syncthreads();
    }
    if (tid == 0) {
      flag[job] = bad;
      multi[(size_t)job * FS_NMULTI + 1] = bad ? NAN : red[0];
    }
    __syncthreads();
  }
}

// tile t of the upper triangle of nt x nt tiles, row after row: (ti, tj), ti <= tj
__device__ __forceinline__ void fs_tile_of(int t, int nt, int *ti, int *tj) {
  int i = 0;
  while (t >= nt - i) { t -= nt - i; i++; }
  *ti = i; *tj = i + t;
}

template <int MB>
__global__ __launch_bounds__(FS_ETHREADS) void k_fs_energy(FsParams P, double *part /*[n_ds][nd][tiles][2]*/) {
  __shared__ __attribute__((aligned(16))) double rows[FS_TILE * MB];
  static_assert(FS_TILE == 128 && MB % 8 == 0 && MB >= 8 && MB <= 64, "two waves per half of the rows; the sums of a tile fit the rows' place");
  const int tid = threadIdx.x, c = tid & (FS_TILE - 1), half = tid / FS_TILE, S = P.S, n = P.n, m = P.m;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = (n + FS_TILE - 1) / FS_TILE, tiles = nt * (nt + 1) / 2;
  const long long jobs = (long long)P.n_ds * P.nd * tiles;
  const long long stride = (long long)P.nd * S;
  for (long long job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int t = (int)(job % tiles), day = (int)((job / tiles) % P.nd), ds = (int)(job / ((long long)tiles * P.nd));
    int ti, tj;
    fs_tile_of(t, nt, &ti, &tj);
    const bool diag = ti == tj;
    const double *base = P.x + ((size_t)ds * n * P.nd + day) * S;
    // the row draws, centred on y; the padding is zero and adds exactly nothing to a distance.  (Staged before the column draw is loaded:
    // both in registers at once are 4 MB of them.)
    if (half == 0 && !diag) {
      double *dst = rows + c * MB;
      const int i = ti * FS_TILE + c;                        // (i < n: only the last tile of a row of tiles is ragged, and it is a column)
      const double *xr = base + (long long)i * stride;
#pragma unroll
      for (int k = 0; k < MB; k++) {
        double v = 0.0;
        if (k < m) { const int u = P.uidx[k]; v = xr[u] - P.actual[u]; }
        dst[k] = v;
      }
    }
    // the thread's column draw j, centred the same way; on a diagonal tile the column draws are the row draws
    const int j = tj * FS_TILE + c;
    double xj[MB];
#pragma unroll
    for (int k = 0; k < MB; k++) xj[k] = 0.0;
    if (j < n) {
      const double *xr = base + (long long)j * stride;
#pragma unroll
      for (int k = 0; k < MB; k++)
        if (k < m) { const int u = P.uidx[k]; xj[k] = xr[u] - P.actual[u]; }
    }
    if (half == 0 && diag) {
      double *dst = rows + c * MB;
#pragma unroll
      for (int k = 0; k < MB; k++) dst[k] = xj[k];
    }
    __syncthreads();
    // rows [r0, r1) of the thread's half; on a diagonal tile a wave needs the rows below its last column only
    const int r0 = half * (FS_TILE / 2);
    int r1 = r0 + FS_TILE / 2;
    if (diag) { const int cmax = (wave & 1) * 64 + 63; r1 = r1 < cmax ? r1 : cmax; }
    const int i0 = ti * FS_TILE;
    double acc = 0.0;
#pragma unroll 1
    for (int r = r0; r < r1; r += 2) {
      const double *ra = rows + r * MB, *rb = ra + MB;       // (r + 1 <= FS_TILE - 1: r0 and r1 - r0 are even or the last row is 126)
      double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
#pragma unroll
      for (int k = 0; k < MB; k += 2) {
        const double da0 = ra[k] - xj[k], da1 = ra[k + 1] - xj[k + 1];
        const double db0 = rb[k] - xj[k], db1 = rb[k + 1] - xj[k + 1];
        a0 = fma(da0, da0, a0); a1 = fma(da1, da1, a1);
        b0 = fma(db0, db0, b0); b1 = fma(db1, db1, b1);
      }
      const double da = sqrt(a0 + a1), db = sqrt(b0 + b1);
      const bool va = j < n && (diag ? r < c : i0 + r < n), vb = j < n && r + 1 < r1 && (diag ? r + 1 < c : i0 + r + 1 < n);
      acc += va ? da : 0.0;
      acc += vb ? db : 0.0;
    }
    double single = 0.0;
    if (diag && half == 0 && j < n) {
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int k = 0; k < MB; k += 2) { a0 = fma(xj[k], xj[k], a0); a1 = fma(xj[k + 1], xj[k + 1], a1); }
      single = sqrt(a0 + a1);
    }
    __syncthreads();                                         // the rows are read; their place takes the threads' sums
    double *red = rows;                                      // [FS_ETHREADS] pairs, then [FS_TILE] singles: 384 <= FS_TILE * 8 doubles
    red[tid] = acc;
    if (half == 0) red[FS_ETHREADS + c] = single;
    __syncthreads();
    for (int off = FS_ETHREADS / 2; off > 0; off >>= 1) {
      if (tid < off) red[tid] += red[tid + off];
      if (off <= FS_TILE / 2 && tid < off) red[FS_ETHREADS + tid] += red[FS_ETHREADS + tid + off];
      __syncthreads();
    }
    if (tid == 0) { part[(size_t)job * 2] = red[0]; part[(size_t)job * 2 + 1] = red[FS_ETHREADS]; }
    __syncthreads();
  }
}

// grid = (data set, day), one wave each
__global__ __launch_bounds__(64) void k_fs_energy_finish(const double *part, int n, int tiles, const int *flag, double *multi /*[n_ds][nd][3]*/) {
  __shared__ double red[2][64];
  const int lane = threadIdx.x, job = blockIdx.x;
  const double *p = part + (size_t)job * tiles * 2;
  double a = 0.0, b = 0.0;
  for (int t = lane; t < tiles; t += 64) { a += p[2 * t]; b += p[2 * t + 1]; }
  red[0][lane] = a; red[1][lane] = b;
  __syncthreads();
  for (int off = 32; off > 0; off >>= 1) {
    if (lane < off) { red[0][lane] += red[0][lane + off]; red[1][lane] += red[1][lane + off]; }
    __syncthreads();
  }
  if (lane == 0) {
    const double nn = (double)n;
    multi[(size_t)job * FS_NMULTI] = flag[job] ? NAN : red[1][0] / nn - red[0][0] / (nn * nn);
  }
}

// grid = the days of ONE data set; mean [nd][S + 1] and cov [nd][S + 1][S + 1] of its draws (k_sc_finish_mean, k_sc_finish_cov); flag and multi at the
// data set's first day
__global__ __launch_bounds__(256) void k_fs_dss(FsParams P, const double *mean, const double *cov, const int *flag, double *multi) {
  __shared__ double A[FS_MAX_S][FS_MAX_S + 2];
  __shared__ int s_ok;
  const int tid = threadIdx.x, day = blockIdx.x, m = P.m, C = P.S + 1;
  double *o = multi + (size_t)day * FS_NMULTI + 2;
  if (P.n <= m || flag[day]) {                               // uniform over the workgroup
    if (tid == 0) *o = NAN;
    return;
  }
  const double *cv = cov + (size_t)day * C * C;
  for (int idx = tid; idx < m * m; idx += 256) { const int a = idx / m, b = idx - a * m; A[a][b] = cv[P.uidx[a] * C + P.uidx[b]]; }
  if (tid == 0) s_ok = 1;
  __syncthreads();
  for (int k = 0; k < m; k++) {                              // right-looking, the lower triangle
    if (tid == 0) { const double piv = A[k][k]; if (piv > 0.0) A[k][k] = sqrt(piv); else s_ok = 0; }
    __syncthreads();
    if (!s_ok) break;
    const double d = A[k][k];
    __syncthreads();
    for (int i = k + 1 + tid; i < m; i += 256) A[i][k] /= d;
    __syncthreads();
    const int r = m - 1 - k;
    for (int idx = tid; idx < r * r; idx += 256) {
      const int i = k + 1 + idx / r, jj = k + 1 + idx % r;
      if (jj <= i) A[i][jj] -= A[i][k] * A[jj][k];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  if (!s_ok) { *o = NAN; return; }
  double q = 0.0, logdet = 0.0;
  for (int i = 0; i < m; i++) {                              // L z = y - mean; the row's own z in the factor's dead upper triangle
    const int u = P.uidx[i];
    double s = P.actual[u] - mean[(size_t)day * C + u];
    for (int k = 0; k < i; k++) s -= A[i][k] * A[k][m];
    const double z = s / A[i][i];
    A[i][m] = z;
    q += z * z;
    logdet += log(A[i][i]);
  }
  *o = 2.0 * logdet + q;
}
