// potus_outcomes.hpp -- joint election outcomes of the draws, counted on the device.
//
// What the reference's run scripts compute from the JOINT outcome of a draw (final_2016.R:904-920 electoral-college histogram,
// final_2012.R:809-839 / final_2008.R:813-843 tipping-point state, README.Rmd:481-502 p-values of the certified result) and the
// conditional questions asked of it, without shipping draws x T x S doubles of predicted_score to the host.  DESIGN.md section 4f.
//
// For one draw and one day, x[s] = predicted_score[t, s], ev[s] non-negative integers, W = ev_to_win, w = normalised state weights:
//   dem_ev  = sum_s ev[s] 1[x[s] > 0.5]                       (strict, final_2016.R:817,909)
//   nat     = sum_s w[s] x[s], summed s = 0, 1, ..., S-1 as k_ps_derived sums it; pop_win = nat > 0.5
//   tipping point (final_2012.R:817-839): states ordered by x descending when pop_win, ascending otherwise, equal x keeping the lower
//           state index first (dplyr's stable arrange); the first state whose cumulative ev is >= W.  The reference orders by the
//           POPULAR-vote winner, not the electoral-college winner; so does this.  No sort: state s is it iff
//           before(s) < W <= before(s) + ev[s], before(s) = the ev of the states ranked ahead of s.  sum ev < W: none (slot S).
//   indicators I_0..I_{S-1} = 1[x[s] > 0.5], I_S = 1[dem_ev >= W], I_{S+1} = pop_win
// Outputs are 64-bit COUNTS per day: exact, independent of the order in which draws arrive, the same bytes however the chains are split.
//
// Kernels:
//   k_oc_days   rows of predicted_score as write_array lays them out (cell (t, s) at t + T s) -> items [draw][day of the range][S],
//               through 64 x 64 LDS tiles (coalesced on both sides); only the days asked for are written.
//   k_oc_count  one workgroup = one day x one chunk of draws; one WAVE per (draw, day) item, lane = state.  The other states' scores come
//               from the lanes (v_readlane, the loop index is wave-uniform): one pass for nat and dem_ev, one for before(s).  Lane s keeps
//               the 64-item bit column of its indicator in a register (bit k = item k of the wave's current batch); every 64 items
//               joint[i][j] += popcount(column_i & column_j) into LDS.  Histogram, tipping and below-actual counts live in LDS / registers
//               per workgroup and go out as ONE 64-bit integer atomic add per non-zero bin per workgroup.  No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define OC_THREADS 256
#define OC_WAVES (OC_THREADS / 64)
#define OC_EV_CAP 2047            // sum of ev the LDS histogram holds (bins 0 .. OC_EV_CAP); 538 fits with room
#define OC_MAX_S 63               // lane = state
#define OC_NI (OC_MAX_S + 2)      // indicators: the states, electoral-college win, popular-vote win

// in [rows][in_stride], predicted_score cell (t, s) at t + T s  ->  out [rows][t1 - t0][S]
__global__ __launch_bounds__(256) void k_oc_days(const double *in, long long in_stride, double *out, long long rows, int T, int S, int t0, int t1) {
  __shared__ double tile[64][65];
  const int nsel = t1 - t0, tb = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 64 x 4
  for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
    const double *src = in + row * in_stride;
    for (int s = ty; s < S; s += 4) tile[s][tx] = (tb + tx < nsel) ? src[(t0 + tb + tx) + (long long)T * s] : 0.0;
    __syncthreads();
    double *dst = out + row * (long long)nsel * S;
    for (int r = ty; r < 64; r += 4)
      if (tb + r < nsel && tx < S) dst[(long long)(tb + r) * S + tx] = tile[tx][r];
    __syncthreads();
  }
}

__device__ __forceinline__ double oc_readlane(double v, int lane) {   // lane is wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ unsigned long long oc_readlane(unsigned long long v, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

struct OcParams {
  const double *x;              // [nd][n_days][S]
  long long nd, chunk;          // draws, draws per blockIdx.y
  int n_days, S, W, ev_sum;
  const double *w;              // [S]
  const int32_t *ev;            // [S]
  const double *actual;         // [S] or null
  unsigned long long *ev_hist;  // [n_days][ev_sum + 1]
  unsigned long long *tipping;  // [n_days][S + 1]
  unsigned long long *joint;    // [n_days][S + 2][S + 2]
  unsigned long long *below;    // [n_days][S]
};

// the batch of up to 64 items whose indicator columns the lanes hold -> the workgroup's joint counts.  Rows i < S hold every column;
// rows S and S + 1 only their upper triangle (the flush mirrors the rest).
__device__ __forceinline__ void oc_fold(unsigned *s_joint, int lane, int S, unsigned long long col, unsigned long long colE, unsigned long long colP) {
  const int NI = S + 2;
  for (int j = 0; j < S; j++) {
    const unsigned c = (unsigned)__popcll(col & oc_readlane(col, j));
    if (c) atomicAdd(&s_joint[lane * NI + j], c);      // (col is zero in the lanes beyond S)
  }
  const unsigned cE = (unsigned)__popcll(col & colE), cP = (unsigned)__popcll(col & colP);
  if (cE) atomicAdd(&s_joint[lane * NI + S], cE);
  if (cP) atomicAdd(&s_joint[lane * NI + S + 1], cP);
  if (lane == 0) {
    atomicAdd(&s_joint[S * NI + S], (unsigned)__popcll(colE));
    atomicAdd(&s_joint[S * NI + S + 1], (unsigned)__popcll(colE & colP));
    atomicAdd(&s_joint[(S + 1) * NI + S + 1], (unsigned)__popcll(colP));
  }
}

// grid (n_days, chunks of draws); the workgroup's counters are 32-bit (chunk <= 2^30 draws), the global ones 64-bit
__global__ __launch_bounds__(OC_THREADS) void k_oc_count(OcParams P) {
  __shared__ unsigned s_hist[OC_EV_CAP + 1];
  __shared__ unsigned s_joint[OC_NI * OC_NI];
  __shared__ unsigned s_tip[64], s_below[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, S = P.S, NI = S + 2, W = P.W;
  const int day = blockIdx.x;
  for (int i = tid; i <= OC_EV_CAP; i += OC_THREADS) s_hist[i] = 0u;
  for (int i = tid; i < OC_NI * OC_NI; i += OC_THREADS) s_joint[i] = 0u;
  if (tid < 64) { s_tip[tid] = 0u; s_below[tid] = 0u; }
  __syncthreads();
  const long long d0 = (long long)blockIdx.y * P.chunk, d1 = d0 + P.chunk < P.nd ? d0 + P.chunk : P.nd;
  const bool act = lane < S;
  const int my_ev = act ? P.ev[lane] : 0;
  const double my_w = act ? P.w[lane] : 0.0;
  const bool have_actual = P.actual != nullptr;
  const double my_actual = (have_actual && act) ? P.actual[lane] : 0.0;
  unsigned n_tip = 0u, n_below = 0u, n_none = 0u;
  unsigned long long col = 0ull, colE = 0ull, colP = 0ull;   // bit k: item k of the batch (colE, colP are wave-uniform)
  int k = 0;
  const long long stride = (long long)P.n_days * S;
  const double *px = P.x + (long long)day * S + lane;
  long long d = d0 + wave;
  double xn = (d < d1 && act) ? px[d * stride] : 0.0;
  for (; d < d1; d += OC_WAVES) {
    const double x = xn;
    if (d + OC_WAVES < d1 && act) xn = px[(d + OC_WAVES) * stride];   // the next item's load is in flight during this one's arithmetic
    double nat = 0.0;
    int dem = 0;
    for (int j = 0; j < S; j++) {                                     // s = 0 .. S-1 in order: pop_win does not depend on the launch shape
      const double xj = oc_readlane(x, j);
      nat += oc_readlane(my_w, j) * xj;
      dem += xj > 0.5 ? __builtin_amdgcn_readlane(my_ev, j) : 0;
    }
    const bool pop = nat > 0.5, ec = dem >= W;
    const double y = pop ? x : -x;                                    // descending x for a popular-vote win, ascending otherwise
    int before = 0;
    for (int j = 0; j < S; j++) {
      const double yj = oc_readlane(y, j);
      const bool ahead = yj > y || (yj == y && j < lane);             // equal scores: the lower index first
      before += ahead ? __builtin_amdgcn_readlane(my_ev, j) : 0;
    }
    const bool tip = act && before < W && W <= before + my_ev;
    n_tip += tip ? 1u : 0u;
    n_none += __ballot(tip) == 0ull ? 1u : 0u;
    n_below += (act && have_actual && x < my_actual) ? 1u : 0u;
    col |= (unsigned long long)((act && x > 0.5) ? 1 : 0) << k;
    colE |= (unsigned long long)(ec ? 1 : 0) << k;
    colP |= (unsigned long long)(pop ? 1 : 0) << k;
    if (lane == 0) atomicAdd(&s_hist[dem < OC_EV_CAP ? dem : OC_EV_CAP], 1u);
    if (++k == 64) { oc_fold(s_joint, lane, S, col, colE, colP); col = colE = colP = 0ull; k = 0; }
  }
  if (k) oc_fold(s_joint, lane, S, col, colE, colP);
  if (n_tip) atomicAdd(&s_tip[lane], n_tip);
  if (n_below) atomicAdd(&s_below[lane], n_below);
  if (lane == 0 && n_none) atomicAdd(&s_tip[S], n_none);
  __syncthreads();
  // one integer atomic add per non-zero bin per workgroup
  for (int b = tid; b <= P.ev_sum; b += OC_THREADS) {
    const unsigned v = s_hist[b];
    if (v) atomicAdd(&P.ev_hist[(long long)day * (P.ev_sum + 1) + b], (unsigned long long)v);
  }
  for (int idx = tid; idx < NI * NI; idx += OC_THREADS) {
    const int i = idx / NI, j = idx - i * NI;
    const unsigned v = (i >= S && j < i) ? s_joint[j * NI + i] : s_joint[i * NI + j];
    if (v) atomicAdd(&P.joint[(long long)day * NI * NI + idx], (unsigned long long)v);
  }
  if (tid <= S && s_tip[tid]) atomicAdd(&P.tipping[(long long)day * (S + 1) + tid], (unsigned long long)s_tip[tid]);
  if (tid < S && s_below[tid]) atomicAdd(&P.below[(long long)day * S + tid], (unsigned long long)s_below[tid]);
}
