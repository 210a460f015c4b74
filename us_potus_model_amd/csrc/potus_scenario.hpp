// potus_scenario.hpp -- conditional forecasts and the covariance of the state scores, on the device.  DESIGN.md section 4h.
//
// final_2016.R:710-715 ("state correlation?") calls cor() on the election-day scores of the draws, the older run files cov(p[, election_day, ]);
// and the reader of a forecast asks "what if": the forecast GIVEN that the Democrat carries Florida, loses Pennsylvania, or that the national
// vote lands between 48 % and 52 %.  Both need every draw of predicted_score; neither needs it on the host.
//
// For one draw and one day the S + 1 COORDINATES are x[s] = predicted_score[t, s] (s < S) and x[S] = nat = sum_s w[s] x[s], summed
// s = 0, 1, ..., S-1 in order.  The condition reads it exactly as k_oc_count sums it (sc_nat below is that loop: a chain of fused
// multiply-adds); coordinate S of the moments is the same loop with every product and sum rounded on its own (k_sc_nat).
//   condition   given cond_day, lo[S+1], hi[S+1]: a draw is KEPT iff lo[k] < x_cond_day[k] <= hi[k] for every k (-inf / +inf: free;
//               "wins s" is lo[s] = 0.5, "does not win s" is hi[s] = 0.5 -- the strict rule of final_2016.R:817, so the two partition the draws)
//   mean        [days][S+1]       sum over the kept draws / n_kept, one division
//   cov         [days][S+1][S+1]  two-pass: sum of products of deviations from that mean / (n_kept - 1), both triangles written
//   counts      potus_outcomes' ev_hist, tipping, joint of the kept draws: k_oc_count on the compacted block, untouched
// The draws come in CANONICAL order (chain after chain as the handles are listed, iteration order inside a chain) and every floating-point
// sum runs in an order fixed by that sequence alone: chunks of SC_CHUNK kept draws, a chunk's draws dealt to the four waves of its workgroup
// in a fixed pattern, wave partials added in wave order, chunk partials in chunk order.  No floating-point atomics.
//
// Kernels:
//   k_sc_keep     one wave per draw, lane = coordinate, on the condition day's items: a byte flag per draw, a kept count per SC_KEEP_BLOCK draws
//   k_sc_scan     exclusive scan of the block counts (one wave, dpp_scan_sum on exact integers held as doubles) -> each block's first row; the total
//   k_sc_compact  copies every kept draw's [n_days][S] row to its place, order kept, coalesced
//   k_sc_nat      grid (day, chunk): lane = item; the national vote of every kept (draw, day), for k_sc_sum and k_sc_gram
//   k_sc_sum      grid (day, chunk): one wave per item, lane = coordinate; column sums of the S + 1 coordinates
//   k_sc_finish_mean  adds the chunk partials in chunk order, divides once
//   k_sc_gram<NT> grid (day, chunk): the centred Gram matrix on the fp64 matrix cores, NT = ceil((S+1)/16) operand tiles.
//                 v_mfma_f64_16x16x4_f64: D[m][n] += sum_k A[m][k] B[k][n]; lane l feeds A[l & 15][l >> 4] and B[l >> 4][l & 15], holds
//                 D[(l >> 4) + 4 v][l & 15] (potus_dense_pool.hpp).  With k = a draw of a step of four and m, n = coordinates, the A operand of
//                 tile row c and the B operand of tile column c are the SAME register: lane l holds x[draw 4b + (l >> 4)][16c + (l & 15)] - mean.
//                 A load per operand tile, straight from global memory into the lane that feeds it; no LDS staging, no shuffles.
//   k_sc_finish_cov   adds the chunk partials in chunk order, divides by n_kept - 1, mirrors the lower triangle
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "potus_dpp.hpp"
#include "potus_outcomes.hpp"

#define SC_THREADS 256
#define SC_WAVES (SC_THREADS / 64)
#define SC_KEEP_BLOCK 256          // draws per kept count (and per workgroup of k_sc_keep / k_sc_compact): 64 per wave
#define SC_CHUNK 1024              // kept draws per partial sum: a constant of the library, never derived from the device or the launch shape
#define SC_MAX_NT 4                // operand tiles of sixteen coordinates: S + 1 <= 64

typedef double sc_d4 __attribute__((ext_vector_type(4)));

// the national vote of the wave's item: lane s < S holds x[s] and w[s] (zeros beyond).  The loop of k_oc_count, same order, same contraction:
// `nat > 0.5` here and pop_win there cannot disagree.
__device__ __forceinline__ double sc_nat(double x, double my_w, int S) {
  double nat = 0.0;
  for (int j = 0; j < S; j++) {
    const double xj = oc_readlane(x, j);
    nat += oc_readlane(my_w, j) * xj;
  }
  return nat;
}

// xc: the condition day's item of draw d at xc + d * cstride.  grid = blocks of SC_KEEP_BLOCK draws; wave w of a block takes its draws 64 w .. 64 w + 63
__global__ __launch_bounds__(SC_THREADS) void k_sc_keep(const double *xc, long long cstride, long long nd, int S, const double *w, const double *lo, const double *hi,
                                                        unsigned char *flag, int *block_count) {
  __shared__ int s_cnt[SC_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool act = lane < S;
  const double my_w = act ? w[lane] : 0.0;
  const double my_lo = lane <= S ? lo[lane] : 0.0, my_hi = lane <= S ? hi[lane] : 0.0;
  const long long d0 = (long long)blockIdx.x * SC_KEEP_BLOCK + 64 * wave, d1 = d0 + 64 < nd ? d0 + 64 : nd;
  int kept = 0;
  for (long long d = d0; d < d1; d++) {
    const double x = act ? xc[d * cstride + lane] : 0.0;
    const double nat = sc_nat(x, my_w, S);
    const double v = act ? x : nat;
    const bool in = lane > S || (my_lo < v && v <= my_hi);          // (a NaN score is in no interval)
    const bool keep = __ballot(in) == ~0ull;
    if (lane == 0) flag[d] = keep ? 1 : 0;
    kept += keep ? 1 : 0;
  }
  if (lane == 0) s_cnt[wave] = kept;
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// first[b] = kept draws of the blocks before b; first[nblk] = all of them.  One wave; the counts are exact as doubles (< 2^53)
__global__ __launch_bounds__(64) void k_sc_scan(const int *block_count, long long nblk, long long *first) {
  const int lane = threadIdx.x;
  double carry = 0.0;
  for (long long base = 0; base < nblk; base += 64) {
    const double c = base + lane < nblk ? (double)block_count[base + lane] : 0.0;
    const double inc = dpp_scan_sum(c);
    if (base + lane < nblk) first[base + lane] = (long long)(carry + inc - c);
    carry += dpp_readlane_d(inc, 63);
  }
  if (lane == 0) first[nblk] = (long long)carry;
}

// grid (blocks of SC_KEEP_BLOCK draws, slices of a row); out row first[block] + (rank of the draw among the block's kept draws)
__global__ __launch_bounds__(SC_THREADS) void k_sc_compact(const double *x, long long nd, long long rowlen, const unsigned char *flag, const long long *first, double *out) {
  __shared__ int s_list[SC_KEEP_BLOCK];
  __shared__ int s_cnt[SC_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long d = (long long)blockIdx.x * SC_KEEP_BLOCK + tid;
  const bool f = d < nd && flag[d] != 0;
  const unsigned long long mask = __ballot(f);
  if (lane == 0) s_cnt[wave] = __popcll(mask);
  __syncthreads();
  int before = 0, total = 0;
  for (int k = 0; k < SC_WAVES; k++) { before += k < wave ? s_cnt[k] : 0; total += s_cnt[k]; }
  if (f) s_list[before + __popcll(mask & ((1ull << lane) - 1ull))] = tid;
  __syncthreads();
  const long long e0 = rowlen * blockIdx.y / gridDim.y, e1 = rowlen * (blockIdx.y + 1) / gridDim.y;
  const long long row0 = first[blockIdx.x];
  for (int k = 0; k < total; k++) {
    const double *src = x + ((long long)blockIdx.x * SC_KEEP_BLOCK + s_list[k]) * rowlen;
    double *dst = out + (row0 + k) * rowlen;
    for (long long e = e0 + tid; e < e1; e += SC_THREADS) dst[e] = src[e];
  }
}

struct ScParams {
  const double *x;       // [n][n_days][S]: the kept draws
  long long n;
  int n_days, S;
  int day0, nchunks;     // the launch covers days day0 .. day0 + gridDim.x - 1, blockIdx.y = chunk
  const double *w;       // [S]
  double *nat;           // [gridDim.x][n]
  double *psum;          // [gridDim.x][nchunks][S + 1]
  double *pcov;          // [gridDim.x][nchunks][S + 1][S + 1]: the upper operand tiles
  double *mean;          // [n_days][S + 1]
  double *cov;           // [n_days][S + 1][S + 1]
};

// Coordinate S of the MOMENTS: the same in-order sum with every product and every sum rounded on its own (no contraction), which is what the
// loop gives in plain C or Python on any host -- the restatement of the tests holds it bit for bit; nothing discrete hangs on it.  Lane = item:
// the chain of S dependent additions runs for 64 items at once instead of once per wave (k_oc_count's chain is what makes that kernel
// compute-bound); a lane walks its item's S contiguous scores, whose cache lines it shares with nobody and uses up within eight steps.
__global__ __launch_bounds__(SC_THREADS) void k_sc_nat(ScParams P) {
#pragma clang fp contract(off)
  const int S = P.S;
  const long long d0 = (long long)blockIdx.y * SC_CHUNK, d1 = d0 + SC_CHUNK < P.n ? d0 + SC_CHUNK : P.n;
  const long long stride = (long long)P.n_days * S;
  const double *px = P.x + (long long)(P.day0 + blockIdx.x) * S;
  double *pn = P.nat + (size_t)blockIdx.x * P.n;
  for (long long d = d0 + threadIdx.x; d < d1; d += SC_THREADS) {
    const double *row = px + d * stride;
    double nat = 0.0;
#pragma unroll 8
    for (int s = 0; s < S; s++) {                                   // (unrolled: the loads do not wait for the chain)
      const double p = P.w[s] * row[s];
      nat = nat + p;
    }
    pn[d] = nat;
  }
}

// one wave per item, lane = coordinate (lane S reads the nat of k_sc_nat); the waves take the chunk's draws in turn
__global__ __launch_bounds__(SC_THREADS) void k_sc_sum(ScParams P) {
  __shared__ double s_acc[SC_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, S = P.S;
  const int day = P.day0 + blockIdx.x;
  const long long d0 = (long long)blockIdx.y * SC_CHUNK, d1 = d0 + SC_CHUNK < P.n ? d0 + SC_CHUNK : P.n;
  // lane < S: x[d][day][lane]; lane S: nat[d]; the lanes beyond read nothing
  const long long stride = lane < S ? (long long)P.n_days * S : 1;
  const double *px = lane < S ? P.x + (long long)day * S + lane : P.nat + (size_t)blockIdx.x * P.n;
  const bool act = lane <= S;
  double acc = 0.0;
  long long d = d0 + wave;
  double xn = (d < d1 && act) ? px[d * stride] : 0.0;
  for (; d < d1; d += SC_WAVES) {
    const double x = xn;
    if (d + SC_WAVES < d1 && act) xn = px[(d + SC_WAVES) * stride];
    acc += x;
  }
  s_acc[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && lane <= S)
    P.psum[((size_t)blockIdx.x * P.nchunks + blockIdx.y) * (S + 1) + lane] = ((s_acc[0][lane] + s_acc[1][lane]) + s_acc[2][lane]) + s_acc[3][lane];
}

// grid = the days of the launch, 64 threads
__global__ __launch_bounds__(64) void k_sc_finish_mean(ScParams P) {
  const int lane = threadIdx.x, S = P.S;
  if (lane > S) return;
  double s = 0.0;
  for (int c = 0; c < P.nchunks; c++) s += P.psum[((size_t)blockIdx.x * P.nchunks + c) * (S + 1) + lane];
  P.mean[(size_t)(P.day0 + blockIdx.x) * (S + 1) + lane] = s / (double)P.n;
}

template <int NT>
__global__ __launch_bounds__(SC_THREADS) void k_sc_gram(ScParams P) {
  constexpr int NTL = NT * (NT + 1) / 2;
  __shared__ double s_acc[NTL * 4 * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), S = P.S, C = S + 1;
  const int r = lane >> 4, m = lane & 15;
  const int day = P.day0 + blockIdx.x;
  const long long d0 = (long long)blockIdx.y * SC_CHUNK, d1 = d0 + SC_CHUNK < P.n ? d0 + SC_CHUNK : P.n;
  const long long stride = (long long)P.n_days * S;
  const double *px = P.x + (long long)day * S;
  const double *pn = P.nat + (size_t)blockIdx.x * P.n;
  double mu[NT];
#pragma unroll
  for (int c = 0; c < NT; c++) mu[c] = 16 * c + m <= S ? P.mean[(size_t)day * C + 16 * c + m] : 0.0;
  // the lane's operands of the step whose four draws start at b: zero beyond column S and beyond the last draw
  auto load = [&](double (&v)[NT], long long b) {
    const long long d = b + r;
#pragma unroll
    for (int c = 0; c < NT; c++) {
      const int col = 16 * c + m;
      double t = 0.0;
      if (d < d1) {
        if (col < S) t = px[d * stride + col] - mu[c];
        else if (col == S) t = pn[d] - mu[c];
      }
      v[c] = t;
    }
  };
  sc_d4 acc[NTL];
#pragma unroll
  for (int t = 0; t < NTL; t++) acc[t] = sc_d4{0.0, 0.0, 0.0, 0.0};
  double v[NT], vn[NT];
  long long b = d0 + 4 * wave;                                       // wave-uniform: the waves take the steps of four draws in turn
  load(v, b);
  for (; b < d1; b += 4 * SC_WAVES) {
    load(vn, b + 4 * SC_WAVES);                                      // the next step's loads are in flight during this one's products
    int t = 0;
#pragma unroll
    for (int ci = 0; ci < NT; ci++)
#pragma unroll
      for (int cj = ci; cj < NT; cj++, t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[ci], v[cj], acc[t], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < NT; c++) v[c] = vn[c];
  }
  // wave 0 adds the others' accumulators in wave order
  for (int w = 1; w < SC_WAVES; w++) {
    if (wave == w) {
#pragma unroll
      for (int t = 0; t < NTL; t++)
#pragma unroll
        for (int k = 0; k < 4; k++) s_acc[(t * 4 + k) * 64 + lane] = acc[t][k];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int t = 0; t < NTL; t++)
#pragma unroll
        for (int k = 0; k < 4; k++) acc[t][k] += s_acc[(t * 4 + k) * 64 + lane];
    }
    __syncthreads();
  }
  if (wave != 0) return;
  double *pc = P.pcov + ((size_t)blockIdx.x * P.nchunks + blockIdx.y) * (size_t)C * C;
  int t = 0;
#pragma unroll
  for (int ci = 0; ci < NT; ci++)
#pragma unroll
    for (int cj = ci; cj < NT; cj++, t++)
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int row = 16 * ci + r + 4 * k, col = 16 * cj + m;
        if (row <= S && col <= S) pc[row * C + col] = acc[t][k];
      }
}

// grid = the days of the launch
__global__ __launch_bounds__(SC_THREADS) void k_sc_finish_cov(ScParams P) {
  const int S = P.S, C = S + 1;
  const double den = (double)(P.n - 1);
  double *out = P.cov + (size_t)(P.day0 + blockIdx.x) * C * C;
  for (int idx = threadIdx.x; idx < C * C; idx += SC_THREADS) {
    const int i = idx / C, j = idx - i * C;
    if (i > j) continue;
    double s = 0.0;
    for (int c = 0; c < P.nchunks; c++) s += P.pcov[((size_t)blockIdx.x * P.nchunks + c) * (size_t)C * C + idx];
    const double q = s / den;
    out[i * C + j] = q;
    out[j * C + i] = q;
  }
}
