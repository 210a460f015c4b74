// potus_advi.hpp -- mean-field ADVI on the device: cmdstanr's $variational(algorithm = "meanfield"), batched.  DESIGN.md section 4p.
// Kucukelbir, Tran, Ranganath, Gelman and Blei (2017); the rules are CmdStan 2.24's advi.hpp as include/potus_hmc.h states them.
//
// q = N(mu, diag(exp(omega))^2).  A TRACK is one stochastic-gradient ascent: the main run of a run (stage 0), or one of the five step-size
// candidates of its adaptation (stages 1 .. 5); track = stage * n_runs + run.  A track's working set in global memory is VI_NVEC vectors of
// Dpad doubles, mu | omega | s_mu | s_omega | zeta | g | a_mu | a_omega, and a ViTrack (t, eta, code, the iterations to run).  a_mu and a_omega
// hold the sums over the grad_samples draws of g and g o eps; with one draw they are the gradient itself.
//
//   k_vi_sga    one workgroup per track, model Mg_all[run / per_ds] as k_opt_lbfgs picks a path's.  Per pass: model_pass at ONE call site
//               under PlainPolicy, then vi_step, out of line: the non-finite test (the one workgroup-wide sum), the draw's share of the two
//               sums, after the last draw of an iteration the element-wise update
//                   g_mu = a_mu / M, g_om = a_om / M * exp(om) + 1;  s = g^2 (t = 1), 0.9 g^2 + 0.1 s;  x += (eta / sqrt(t)) g / (1 + sqrt(s))
//               and the next zeta = mu + exp(om) eps.  A thread owns the Box-Muller PAIRS tid, tid + PT_THREADS, ... -- coordinates 2 j and
//               2 j + 1 of every vector -- so nothing between the pass's gradient and the next pass's point needs the workgroup; eps is
//               regenerated from its counter, not stored.  The scalars live in LDS where the sampler keeps its transition state.  A track
//               whose code is set returns at once.  With P->init the kernel first sets the track's start (q0 or U(-r, r), omega = 0).
//   k_vi_elbo   item (entry e of a list of tracks, draw k) over a fixed grid: workgroup w takes the items w, w + G, ...  Each item builds
//               zeta in the workgroup's own two vectors, runs one pass and writes lp to ITS slot; draw 0 also writes sum omega (strided
//               partials, block_sum).  The mean over a track's slots is the host's, in index order.  The model's LDS block is set up
//               again only when an item's data set differs from the last item's.
//   k_vi_draws  item (run, n): the row [NaN (lp__: k_lap_lp), six NaN, zeta_n] and log q = -1/2 |eps|^2 - sum omega - 1/2 D log 2 pi.
//               lp__ is Laplace's lp-of-rows stage (k_lap_lp), launched per run with the run's model: the bytes of potus_log_prob_grad.
//   randomness  Philox4x32-10 as the sampler's, key = the handle's seed, purpose RNG_ADVI = 10, counter
//               {j, 10 | aux << 8, iter word, run_offset + run + 1}, aux = stage | draw << 4 (include/potus_hmc.h has the table).
//   determinism no atomics; every sum in a fixed order; a track writes its own working set and its own slots, so its bytes depend on
//               neither the batch nor the grid.
//   fp          the element-wise arithmetic is compiled without contraction into fused multiply-adds: tests/advi_ref.py states it in numpy,
//               operation by operation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "potus_advi_rules.hpp"

enum { RNG_ADVI = 10 };   // after RNG_PATHFINDER = 9 (potus_pathfinder.hpp)
enum { VI_V_MU = 0, VI_V_OM, VI_V_SMU, VI_V_SOM, VI_V_ZETA, VI_V_G, VI_V_AMU, VI_V_AOM, VI_NVEC };
enum { VI_AUX_ELBO = 8, VI_AUX_INIT = 14, VI_AUX_DRAW = 15 };   // the stage nibble of aux: 0 .. 5 gradient draws, 8 .. 13 ELBO draws
#define VI_MAX_SAMPLES 0xFFFFF   // a draw's number takes the 20 bits above the stage nibble

struct ViTrack { double eta; int t, code, n_iter, pad; };
struct ViParams {
  const double *q0;        // [n_runs][D] or null
  double *work;            // [n_tracks][VI_NVEC][Dpad]
  ViTrack *track;          // [n_tracks]
  const int *elbo_tracks;  // [n_et] k_vi_elbo: the tracks whose ELBO is wanted
  double *lp_slot;         // [n_et][elbo_samples]
  double *ent;             // [n_et] sum omega
  double *escr;            // [grid][2][Dpad] k_vi_elbo: zeta | g of the workgroup
  double *rows, *lq;       // k_vi_draws: [n_runs][M][7 + D], [n_runs][M]
  const int *no_draws;     // [n_runs] not 0: NaN rows
  int n_runs, per_ds, D, Dpad, grad_samples, elbo_samples, n_et, M, run_offset, draw_offset, init;
  double radius;
  unsigned seed_lo, seed_hi;
};
typedef const ViParams AS_C *CVp;

struct ViState { double eta; int t, code, m, left; };
static_assert(sizeof(ViState) <= sizeof(TS), "ADVI's scalars take the place of the sampler's transition state in LDS");

struct ViTrk { CMp M; CVp P; ldp red; ViState AS_L *st; gdp W; int D, Dpad, run, stage, tid; RngKey key; };
__device__ __forceinline__ ViTrk vi_trk(const DevModel *Mg, const ViParams *Pg, int track_) {
  ViTrk o;
  o.M = (CMp)uni_ptr(Mg); o.P = (CVp)uni_ptr(Pg);
  const int track = (int)uni32((unsigned)track_);
  ldp lds = (ldp)lds_dyn;
  o.st = (ViState AS_L *)(lds + o.M->lds_doubles); o.red = lds + o.M->l_red;
  o.D = o.M->D; o.Dpad = o.P->Dpad; o.tid = threadIdx.x;
  o.run = track % o.P->n_runs; o.stage = track / o.P->n_runs;
  o.W = as_g(o.P->work) + (size_t)track * VI_NVEC * o.Dpad;
  o.key = RngKey{o.P->seed_lo, o.P->seed_hi, (uint32_t)(o.P->run_offset + o.run + 1)};
  return o;
}

// zeta = mu + exp(omega) eps for the pair j, eps the pair of counter {j, RNG_ADVI | aux << 8, iter, run}
__device__ __forceinline__ void vi_zeta_pair(const RngKey &key, uint32_t iter, uint32_t aux, int j, int D, gcdp mu, gcdp om, gdp zeta) {
#pragma clang fp contract(off)
  double a, b;
  rng_normal_pair(key, iter, RNG_ADVI, aux, (uint32_t)j, a, b);
  const int i0 = 2 * j, i1 = i0 + 1;
  zeta[i0] = mu[i0] + exp(om[i0]) * a;
  if (i1 < D) zeta[i1] = mu[i1] + exp(om[i1]) * b;
}

// one coordinate's update; returns nothing, writes x and s
__device__ __forceinline__ void vi_update(double g, double step, int t, double &x, double &s) {
#pragma clang fp contract(off)
  const double g2 = g * g;
  s = t == 1 ? g2 : 0.9 * g2 + 0.1 * s;
  x = x + step * g / (1.0 + sqrt(s));
}

// The start of a track: mu = the run's q0 or U(-r, r), omega = 0, the step-size memory 0.
__device__ __noinline__ void vi_init(const DevModel *Mg, const ViParams *Pg, int track_) {
  const ViTrk o = vi_trk(Mg, Pg, track_);
  CVp P = o.P;
  gdp W = o.W;
  const int Dpad = o.Dpad;
  for (int i = o.tid; i < o.D; i += PT_THREADS) {
    W[(size_t)VI_V_MU * Dpad + i] = P->q0 ? as_g(P->q0)[(size_t)o.run * o.D + i]
                                          : P->radius * (2.0 * rng_uniform(o.key, 0u, RNG_ADVI, VI_AUX_INIT, (uint32_t)i) - 1.0);
    W[(size_t)VI_V_OM * Dpad + i] = 0.0; W[(size_t)VI_V_SMU * Dpad + i] = 0.0; W[(size_t)VI_V_SOM * Dpad + i] = 0.0;
  }
  __syncthreads();
}

// What follows a pass at zeta (first = 0), and what precedes the first one (first = 1).  Returns whether the track has another pass.
__device__ __noinline__ int vi_step(const DevModel *Mg, const ViParams *Pg, int track_, double lp, int first_) {
  const ViTrk o = vi_trk(Mg, Pg, track_);
  CVp P = o.P;
  ViState AS_L *st = o.st;
  const int tid = o.tid, D = o.D, Dpad = o.Dpad, Ms = P->grad_samples, first = (int)uni32((unsigned)first_);
  gdp mu = o.W + (size_t)VI_V_MU * Dpad, om = o.W + (size_t)VI_V_OM * Dpad, smu = o.W + (size_t)VI_V_SMU * Dpad, som = o.W + (size_t)VI_V_SOM * Dpad;
  gdp zeta = o.W + (size_t)VI_V_ZETA * Dpad, amu = o.W + (size_t)VI_V_AMU * Dpad, aom = o.W + (size_t)VI_V_AOM * Dpad;
  gcdp g = o.W + (size_t)VI_V_G * Dpad;
  const int t = opt_uni(st->t), m = opt_uni(st->m), left = opt_uni(st->left);
  const int npair = (D + 1) / 2;
  if (first) {
    for (int j = tid; j < npair; j += PT_THREADS) vi_zeta_pair(o.key, (uint32_t)(t + 1), (uint32_t)o.stage, j, D, gcdp(mu), gcdp(om), zeta);
    __syncthreads();
    return left > 0;
  }
  double bad[1] = {isfinite(lp) ? 0.0 : 1.0};
  for (int i = tid; i < D; i += PT_THREADS) bad[0] += isfinite(g[i]) ? 0.0 : 1.0;
  block_sum(bad, o.red, tid);
  if (opt_uni(bad[0] != 0.0 ? 1 : 0)) {                  // the run ends at its last finished iterate
    if (tid == 0) st->code = ADVI_NONFINITE;
    __syncthreads();
    return 0;
  }
  const bool last = m + 1 == Ms;
  const int t1 = last ? t + 1 : t, m1 = last ? 0 : m + 1, left1 = last ? left - 1 : left;
  const double step = st->eta / sqrt((double)(t + 1)), Md = (double)Ms;
  const uint32_t aux_now = (uint32_t)o.stage | ((uint32_t)m << 4), aux_next = (uint32_t)o.stage | ((uint32_t)m1 << 4);
  for (int j = tid; j < npair; j += PT_THREADS) {
#pragma clang fp contract(off)
    double e[2];
    rng_normal_pair(o.key, (uint32_t)(t + 1), RNG_ADVI, aux_now, (uint32_t)j, e[0], e[1]);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int i = 2 * j + h;
      if (i >= D) break;
      const double gi = g[i];
      double a = m == 0 ? gi : amu[i] + gi, w = m == 0 ? gi * e[h] : aom[i] + gi * e[h];
      if (!last) { amu[i] = a; aom[i] = w; continue; }
      double x = mu[i], s = smu[i];
      vi_update(a / Md, step, t + 1, x, s);
      mu[i] = x; smu[i] = s;
      double y = om[i], r = som[i];
      vi_update(w / Md * exp(y) + 1.0, step, t + 1, y, r);
      om[i] = y; som[i] = r;
    }
    if (left1 > 0) vi_zeta_pair(o.key, (uint32_t)(t1 + 1), aux_next, j, D, gcdp(mu), gcdp(om), zeta);
  }
  if (tid == 0) { st->t = t1; st->m = m1; st->left = left1; }
  __syncthreads();
  return left1 > 0;
}

__global__ __launch_bounds__(PT_THREADS) void k_vi_sga(const DevModel *Mg_all, const ViParams *Pg) {
  CVp P = (CVp)Pg;
  const int track = blockIdx.x, tid = threadIdx.x;
  ViTrack *tr = P->track + track;
  const int init = P->init;
  if (!init && opt_uni(as_g(tr)->code)) return;
  const DevModel *Mg = Mg_all + (track % P->n_runs) / P->per_ds;
  CMp M = (CMp)Mg;
  ldp lds = (ldp)lds_dyn;
  ViState AS_L *st = (ViState AS_L *)(lds + M->lds_doubles);
  const int n_iter = opt_uni(as_g(tr)->n_iter), Dpad = P->Dpad;
  if (init) vi_init(Mg, Pg, track);
  if (n_iter <= 0) return;
  const PassStatic pst = model_setup_lds(M, lds);
  if (tid == 0) { st->eta = as_g(tr)->eta; st->t = init ? 0 : as_g(tr)->t; st->code = 0; st->m = 0; st->left = n_iter; }
  __syncthreads();
  const rsrc_t rw = make_rsrc(P->work + (size_t)track * VI_NVEC * Dpad, (unsigned)VI_NVEC * (unsigned)Dpad * 8u);
  const long long max_pass = (long long)n_iter * P->grad_samples;
  int more = opt_uni(vi_step(Mg, Pg, track, 0.0, 1));
  for (long long pass = 0; pass < max_pass && more; pass++) {
    PlainPolicy pol{rw, rw, 8u * (unsigned)Dpad * (unsigned)VI_V_ZETA, 8u * (unsigned)Dpad * (unsigned)VI_V_G, {0}};
    const double lp = model_pass(M, lds, pst, pol);
    more = opt_uni(vi_step(Mg, Pg, track, lp, 0));
  }
  if (tid == 0) { tr->t = st->t; tr->code = st->code; }
}

// Before an ELBO item's pass: zeta of draw k of the track at its iterate t into the workgroup's vectors; draw 0 also leaves sum omega.
__device__ __noinline__ void vi_elbo_before(const DevModel *Mg, const ViParams *Pg, int e_, int k_) {
  CMp M = (CMp)uni_ptr(Mg);
  CVp P = (CVp)uni_ptr(Pg);
  const int e = (int)uni32((unsigned)e_), k = (int)uni32((unsigned)k_), track = as_c(P->elbo_tracks)[e];
  const int tid = threadIdx.x, D = M->D, Dpad = P->Dpad, run = track % P->n_runs, stage = track / P->n_runs;
  ldp red = (ldp)lds_dyn + M->l_red;
  gcdp mu = as_g(P->work) + ((size_t)track * VI_NVEC + VI_V_MU) * Dpad, om = as_g(P->work) + ((size_t)track * VI_NVEC + VI_V_OM) * Dpad;
  gdp zeta = as_g(P->escr) + (size_t)blockIdx.x * 2 * Dpad;
  const RngKey key{P->seed_lo, P->seed_hi, (uint32_t)(P->run_offset + run + 1)};
  const uint32_t t = (uint32_t)as_g(P->track)[track].t, aux = (uint32_t)(VI_AUX_ELBO + stage) | ((uint32_t)k << 4);
  for (int j = tid; j < (D + 1) / 2; j += PT_THREADS) vi_zeta_pair(key, t, aux, j, D, mu, om, zeta);
  if (k == 0) {
    double v[1] = {0.0};
    for (int i = tid; i < D; i += PT_THREADS) v[0] += om[i];
    block_sum(v, red, tid);
    if (tid == 0) P->ent[e] = v[0];
  }
  __syncthreads();
}

__global__ __launch_bounds__(PT_THREADS) void k_vi_elbo(const DevModel *Mg_all, const ViParams *Pg) {
  CVp P = (CVp)Pg;
  ldp lds = (ldp)lds_dyn;
  const int tid = threadIdx.x, Dpad = P->Dpad, K = P->elbo_samples;
  const long long n_items = (long long)P->n_et * K;
  const rsrc_t rw = make_rsrc(P->escr + (size_t)blockIdx.x * 2 * Dpad, 2u * (unsigned)Dpad * 8u);
  int ds_now = -1;
  PassStatic pst{};
  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int e = (int)(item / K), k = (int)(item % K), track = as_c(P->elbo_tracks)[e];
    if (opt_uni(as_g(P->track)[track].code)) {          // a track that has ended: no pass
      if (tid == 0) { P->lp_slot[item] = -INFINITY; if (k == 0) P->ent[e] = NAN; }
      continue;
    }
    const int ds = opt_uni((track % P->n_runs) / P->per_ds);
    const DevModel *Mg = Mg_all + ds;
    CMp M = (CMp)Mg;
    if (ds != ds_now) { pst = model_setup_lds(M, lds); ds_now = ds; }
    vi_elbo_before(Mg, Pg, e, k);
    PlainPolicy pol{rw, rw, 0u, 8u * (unsigned)Dpad, {0}};
    const double lp = model_pass(M, lds, pst, pol);
    if (tid == 0) P->lp_slot[item] = lp;
  }
}

// rows [NaN (lp__: k_lap_lp), six NaN, zeta_n] and log q of the final draws; a run without an approximation gets NaN
__global__ __launch_bounds__(PT_THREADS) void k_vi_draws(const ViParams *Pg) {
  __shared__ double red_s[PT_NW * 2];
  CVp P = (CVp)Pg;
  ldp red = (ldp)red_s;
  const int tid = threadIdx.x, D = P->D, Dpad = P->Dpad, Mn = P->M, row = POTUS_N_SAMPLER_COLS + D;
  const long long n_items = (long long)P->n_runs * Mn;
  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int run = (int)(item / Mn), n = (int)(item % Mn);
    gdp r = as_g(P->rows) + (size_t)item * row;
    if (tid < POTUS_N_SAMPLER_COLS) r[tid] = NAN;
    if (opt_uni(as_c(P->no_draws)[run])) {
      for (int i = tid; i < D; i += PT_THREADS) r[POTUS_N_SAMPLER_COLS + i] = NAN;
      if (tid == 0) P->lq[item] = NAN;
      continue;
    }
    gcdp mu = as_g(P->work) + ((size_t)run * VI_NVEC + VI_V_MU) * Dpad, om = as_g(P->work) + ((size_t)run * VI_NVEC + VI_V_OM) * Dpad;
    const RngKey key{P->seed_lo, P->seed_hi, (uint32_t)(P->run_offset + run + 1)};
    double v[2] = {0.0, 0.0};                             // |eps|^2, sum omega
    for (int j = tid; j < (D + 1) / 2; j += PT_THREADS) {
#pragma clang fp contract(off)
      double e[2];
      rng_normal_pair(key, (uint32_t)(P->draw_offset + n + 1), RNG_ADVI, VI_AUX_DRAW, (uint32_t)j, e[0], e[1]);
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int i = 2 * j + h;
        if (i >= D) break;
        r[POTUS_N_SAMPLER_COLS + i] = mu[i] + exp(om[i]) * e[h];
        v[0] += e[h] * e[h]; v[1] += om[i];
      }
    }
    block_sum(v, red, tid);
    if (tid == 0) P->lq[item] = -0.5 * v[0] - v[1] - 0.5 * (double)D * 1.8378770664093454836;
  }
}
