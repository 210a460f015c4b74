// potus_hmc.hip -- libpotus_hmc.so: C ABI (include/potus_hmc.h) over the gfx950 kernels.
//
// Host side: validates the Stan data block, builds transformed data (stan:42-55) and the
// static poll schedule, owns device memory / stream / events behind an integer handle.
// Device side: potus_model.hpp (log-density + gradient), potus_nuts.hpp (NUTS + adaptation), potus_rules.hpp (their scalar
// rules, shared with the host's dense window schedule).
#include "../../include/potus_hmc.h"
#include "potus_nuts.hpp"
#include "potus_cluster.hpp"
#include "potus_nuts_twin.hpp"
#include "potus_dense.hpp"
#include "potus_summary.hpp"
#include "potus_diag.hpp"
#include "potus_monitor.hpp"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <charconv>
#include <chrono>
#include <thread>
#include <mutex>
#include <string>
#include <vector>

// ======================================================================== kernels

__global__ __launch_bounds__(PT_THREADS) void k_logprob_grad(const DevModel *Mg, const double *q, double *lp, double *grad, int n) {
  CMp M = (CMp)Mg;
  ldp lds = (ldp)lds_dyn;
  const PassStatic pst = model_setup_lds(M, lds);
  const int D = M->D;
  for (int b = blockIdx.x; b < n; b += gridDim.x) {
    PlainPolicy pol{make_rsrc(q + (size_t)b * D, 8u * D), make_rsrc(grad + (size_t)b * D, 8u * D), 0u, 0u, {0}};
    const double v = model_pass(M, lds, pst, pol);
    if (threadIdx.x == 0) lp[b] = v;
  }
}

// (two workgroups per chain, potus_nuts_twin.hpp: side s of a chain works in block chain + s * chains of state and scalars)
__device__ __forceinline__ Chain make_chain(CMp M, CRp R, int chain, int side = 0) {
  ldp lds = (ldp)lds_dyn;
  Chain c;
  const int Dpad = R->Dpad;
  const int blk = chain + side * R->chains;
  double *state = R->state + (size_t)blk * V_COUNT * Dpad;
  c.M = M; c.lds = lds; c.ts = (ltp)(lds + M->lds_doubles);
  c.base = as_g(state);
  c.st = make_rsrc(state, (unsigned)V_COUNT * (unsigned)Dpad * 8u);
  c.sc = (gsc)(R->scal + blk);
  c.key = RngKey{R->seed_lo, R->seed_hi, (uint32_t)(R->chain_id_offset + chain + 1)};
  c.D = M->D; c.Dpad = Dpad; c.tid = (int)threadIdx.x; c.max_depth = R->max_depth; c.num_warmup = R->num_warmup;
  c.init_buffer = R->init_buffer; c.term_buffer = R->term_buffer;
  c.delta = R->delta; c.gamma = R->gamma; c.kappa = R->kappa; c.t0 = R->t0;
#ifdef POTUS_PROF
  c.prof = lds + M->l_prof;
#endif
  return c;
}

// Initial values (stan::services::util::initialize: U(-R,R), <= 100 attempts), unit metric,
// adaptation windows (windowed_adaptation), mu = log(10*stepsize), initial init_stepsize.
__device__ __forceinline__ void init_one_workgroup(CMp M, CRp R, int chain, int side, const double *q0) {
  Chain c = make_chain(M, R, chain, side);
  c.pst = model_setup_lds(M, c.lds);
  const int tid = c.tid;
  gdp Q0 = c.vec(V_QC), G0 = c.vec(V_GC), minv = c.vec(V_MINV), mean = c.vec(V_WMEAN), m2 = c.vec(V_WM2);
  for (int i = tid; i < c.D; i += PT_THREADS) { minv[i] = 1.0; mean[i] = 0.0; m2[i] = 0.0; }
  if (tid == 0) rule_reset_chain(c.sc, R->stepsize, R->init_buffer, R->window);
  __syncthreads();
  bool ok = false;
  const double radius = R->init_radius;
  for (uint32_t attempt = 0; attempt < 100 && !ok; attempt++) {
    for (int i = tid; i < c.D; i += PT_THREADS) {
      if (q0) Q0[i] = as_g(q0)[(size_t)chain * c.D + i];
      else Q0[i] = radius * (2.0 * rng_uniform(c.key, PT_ITER_PRE, RNG_INITS, attempt, (uint32_t)i) - 1.0);
    }
    __syncthreads();
    PlainPolicy pol{c.st, c.st, c.soff(V_QC), c.soff(V_GC), {0}};
    const double lp = model_pass(M, c.lds, c.pst, pol);
    double bad[1] = {0.0};
    for (int i = tid; i < c.D; i += PT_THREADS) bad[0] += isfinite(G0[i]) ? 0.0 : 1.0;
    block_sum(bad, c.red(), tid);
    ok = isfinite(lp) && bad[0] == 0.0;
    if (tid == 0 && ok) c.sc->lp_cur = lp;
    __syncthreads();
    if (q0) break;
  }
  if (!ok) { if (tid == 0) c.sc->status = POTUS_ERR_INIT; return; }
  init_stepsize(c, PT_ITER_PRE);
  if (tid == 0 && R->num_warmup == 0) rule_complete_adaptation(c.sc); // engage+disengage
}
__global__ __launch_bounds__(PT_THREADS) void k_init(const DevModel *Mg, const RunParams *Rg, const double *q0) {
  CRp R = (CRp)Rg;
  init_one_workgroup((CMp)Mg, R, blockIdx.x % R->chains, blockIdx.x / R->chains, q0);   // side 1: two workgroups per chain only
}

// The once-per-transition work is kept out of line so that the register allocator only sees the
// tree loop (leaves + merges) in the kernel body.  Arguments are re-made wave-uniform on entry.
__device__ __noinline__ void cold_transition_begin(const DevModel *Mg, const RunParams *Rg, int chain, uint32_t iter, int side = 0) {
  CMp M = (CMp)uni_ptr(Mg);
  CRp R = (CRp)uni_ptr(Rg);
  Chain c = make_chain(M, R, (int)uni32((unsigned)chain), (int)uni32((unsigned)side));
  c.pst = model_load_static(M);
  transition_begin(c, uni32(iter));
}

// The end of a transition, the pieces every diagonal sampler shares.  Thread 0: the trajectory's scalars -> ts and the
// chain's counters, from the sampler's own tree (end_trajectory) or from the state the two sides combined (end_trajectory_twin).
__device__ __forceinline__ void end_trajectory(ltp ts, gsc sc) {
  ts->accept_stat = ts->sum_metro / (double)ts->n_leap;
  ts->out_lp = ts->q_lp[ts->sample_qid];
  ts->out_h = ts->q_h[ts->sample_qid];
  sc->total_leapfrogs += ts->n_leap;
  sc->n_divergent += ts->divergent;
}
__device__ __forceinline__ void end_trajectory_twin(ltp ts, gsc sc) {
  ts->n_leap = (int)ts->tt[TT_NLEAP]; ts->divergent = (int)ts->tt[TT_DIV]; ts->depth = (int)ts->tt[TT_DEPTH];
  ts->accept_stat = ts->tt[TT_METRO] / ts->tt[TT_NLEAP];
  ts->out_lp = ts->tt[TT_SLP]; ts->out_h = ts->tt[TT_SH];
  sc->total_leapfrogs += ts->n_leap;
  sc->n_divergent += ts->divergent;
  sc->spec_limit = (int)(((unsigned)sc->spec_limit << 8) | (unsigned)ts->tw_seq);   // doublings of the last four transitions, a byte each
}
// the row of the draws array this transition is saved in, its sampler columns, and the chain's scalars once it is written
__device__ __forceinline__ gdp draw_row(CRp R, int chain, gsc sc) { return as_g(R->draws) + ((size_t)chain * R->n_save_max + sc->saved) * R->row; }
__device__ __forceinline__ void draw_row_head(gdp row, ltp ts) { rule_sampler_cols(row, ts, ts->out_lp, ts->accept_stat, ts->out_h); }
__device__ __forceinline__ void end_commit(ltp ts, gsc sc, bool saved) {
  sc->lp_cur = ts->out_lp;
  if (saved) sc->saved += 1;
}

// New sample -> chain position and draws array; warmup adaptation.
__device__ __noinline__ void cold_transition_end(const DevModel *Mg, const RunParams *Rg, int chain_, uint32_t iter) {
  CMp M = (CMp)uni_ptr(Mg);
  CRp R = (CRp)uni_ptr(Rg);
  const int chain = (int)uni32((unsigned)chain_);
  const int it = (int)uni32(iter);
  Chain c = make_chain(M, R, chain);
  c.pst = model_load_static(M);
  ltp ts = c.ts;
  const int tid = c.tid;
  if (tid == 0) end_trajectory(ts, c.sc);
  __syncthreads();
  CPROF_START(c);
  gcdp qs = c.vec(V_POOLQ + ts->sample_qid);
  gdp Q0 = c.vec(V_QC);
  const bool warm = it < R->num_warmup;
  const bool save = !warm || R->save_warmup;
  gdp row = draw_row(R, chain, c.sc);
  if (save && tid == 0) draw_row_head(row, ts);
  for (int i = tid; i < c.D; i += PT_THREADS) {
    const double v = qs[i];
    Q0[i] = v;
    if (save) row[POTUS_N_SAMPLER_COLS + i] = v;
  }
  __syncthreads();
  if (tid == 0) end_commit(ts, c.sc, save);
  CPROF_MARK(c, PF_SAVE);
  if (warm) adapt_after_transition(c, (uint32_t)it, Q0);
  CPROF_MARK(c, PF_ADAPT);
  __syncthreads();
  if (tid == 0) c.sc->iter = it + 1;
  __syncthreads();
}

// n_iter transitions per chain, adaptation during warmup, draws appended to the draws array.
__device__ __forceinline__ void run_one_workgroup(const DevModel *Mg, const RunParams *Rg, int chain, int n_iter) {
  CMp M = (CMp)Mg;
  CRp R = (CRp)Rg;
  Chain c = make_chain(M, R, chain);
  if (c.sc->status != 0) return;
  c.pst = model_setup_lds(M, c.lds);
  const int total = R->num_warmup + R->num_samples;
  for (int k = 0; k < n_iter; k++) {
    const int it = c.sc->iter;
    if (it >= total) break;
    cold_transition_begin(Mg, Rg, chain, (uint32_t)it);
    transition_tree(c, (uint32_t)it);
    cold_transition_end(Mg, Rg, chain, (uint32_t)it);
  }
#ifdef POTUS_PROF
  if (R->prof) for (int i = c.tid; i < PT_NPROF; i += PT_THREADS) as_g(R->prof)[(size_t)chain * PT_NPROF + i] += c.prof[i];
#endif
}
__global__ __launch_bounds__(PT_THREADS) void k_run(const DevModel *Mg, const RunParams *Rg, int n_iter) { run_one_workgroup(Mg, Rg, blockIdx.x, n_iter); }

// ------------------------------------------------------------------------ two workgroups per chain (potus_nuts_twin.hpp): the cold parts
// The combine of doubling d by the side that built its subtree (valid: the subtree completed without an internal U-turn or
// divergence and was not dropped).  Sets ts->tw_over when the trajectory is over.  One body for the two twin samplers; what
// differs between them comes in through `o`:
//   o.c            the chain (Chain / ClChain: same member names)
//   o.x()          the exchange handle the mailbox waits watch
//   o.UNR, o.first(), o.end()   the elements of this workgroup's share of a vector, UNR in flight per trip
//   o.leaf(ts, d)  momentum slot of the subtree's last leaf
//   o.reduce(v, first)          sum of v over the chain; every store before it is complete when it returns
//   o.publishes()  whether this workgroup writes the chain's mailbox
template <class Ops>
__device__ __forceinline__ void twin_combine(Ops &o, const Twin &t, int side, int d, int valid, uint32_t iter) {
  auto &c = o.c;
  ltp ts = c.ts;
  const int tid = c.tid;
  __syncthreads();
  if (tid == 0) c.sc->leaves_run += ts->n_leap;       // whether the subtree ends up in the trajectory or not
  // 1. the state this combine starts from: published by the combine of doubling d - 1 (or the end of the trajectory)
  if (uni_i(ts->tw_seq) < d) {
    if (tid < 64) tw_catch_up(o.x(), t, ts, d);
    __syncthreads();
  }
  if (uni_i((int)ts->tt[TT_STOP])) {                 // the trajectory ended before this doubling: the subtree is dropped
    if (tid == 0) ts->tw_over = 1;
    __syncthreads();
    return;
  }
  const int rho_side = uni_i((int)ts->tt[TT_RHOSIDE]), dirs = uni_i(ts->tw_dirs);
  int stop = 1;
  if (valid) {
    // 2. rho_top += rho_subtree and the three checks of transition() across the whole trajectory; the other end's momentum
    //    and (if the last combine was the other side's) rho_top come from the other side's state block, where they were
    //    stored write-through before that combine was published.  The subtree's last leaf becomes this side's end point.
    constexpr int UNR = Ops::UNR;
    const bool other_moved = ((side ? ~dirs : dirs) & ((1 << d) - 1)) != 0;
    const rsrc_t rA = other_moved ? t.ost : c.st, rR = rho_side == 1 - side ? t.ost : c.st;
    const int leaf = o.leaf(ts, d);
    const unsigned sM = c.soff(V_MINV), a_beg = c.soff(V_PF0 + (1 - side)), a_end = c.soff(V_PNEAR), s_rt = c.soff(V_RHOTOP);
    const unsigned b_beg = c.soff(V_POOLP + uni_i(ts->pend_beg[d])), b_end = c.soff(V_POOLP + leaf);
    const unsigned b_rho = d == 0 ? c.soff(V_POOLP + leaf) : c.soff(V_RHOLEV + d), s_pf = c.soff(V_PF0 + side);
    double v[6] = {0, 0, 0, 0, 0, 0};
    const int first = o.first(), end = o.end();
    for (int base = first; base < end; base += UNR * PT_THREADS) {
      double mi[UNR], ab[UNR], ae[UNR], ar[UNR], bb[UNR], be[UNR], br[UNR];
#pragma unroll
      for (int k = 0; k < UNR; k++) {
        const int i = base + k * PT_THREADS;
        const unsigned off = i < end ? 8u * i : PT_OOB;   // masked elements read zeros and add nothing
        mi[k] = bld(c.st, off, sM); ab[k] = bld_s(rA, off, a_beg); ae[k] = bld(c.st, off, a_end); ar[k] = bld_s(rR, off, s_rt);
        bb[k] = bld(c.st, off, b_beg); be[k] = bld(c.st, off, b_end); br[k] = bld(c.st, off, b_rho);
      }
#pragma unroll
      for (int k = 0; k < UNR; k++) {
        const int i = base + k * PT_THREADS;
        const unsigned off = i < end ? 8u * i : PT_OOB;
        const double rs = ar[k] + br[k];
        bst_s(c.st, off, s_rt, rs);
        bst_s(c.st, off, s_pf, be[k]);
        const double sab = mi[k] * ab[k], sbe = mi[k] * be[k];
        v[0] += sab * rs;                 // p#_beg . rho
        v[1] += sbe * rs;                 // p#_end . rho
        const double e1 = ar[k] + bb[k];  // rho_old + p of the subtree's first leaf
        v[2] += sab * e1;
        v[3] += mi[k] * bb[k] * e1;
        const double e2 = br[k] + ae[k];  // rho_subtree + p of the old end
        v[4] += mi[k] * ae[k] * e2;
        v[5] += sbe * e2;
      }
    }
    o.reduce(v, first);                   // also: the stores above are complete before anything is published
    const bool persist = v[0] > 0 && v[1] > 0 && v[2] > 0 && v[3] > 0 && v[4] > 0 && v[5] > 0;
    stop = (!persist || d + 1 >= c.max_depth) ? 1 : 0;
  }
  __syncthreads();
  if (tid == 0) {
    // the subtree's leaves count whether it is valid or not (base_nuts: n_leapfrog_, sum_metro_prob, divergent_)
    ts->tt[TT_METRO] += ts->sum_metro; ts->tt[TT_NLEAP] += (double)ts->n_leap;
    if (ts->divergent) ts->tt[TT_DIV] = 1.0;
    if (valid) {
      const double lsw_top = ts->tt[TT_LSW], lsw_sub = ts->pend_lsw[d];
      const int prop = ts->pend_prop[d];
      bool accept;
      if (lsw_sub > lsw_top) accept = true;
      else accept = rng_uniform(c.key, iter, RNG_TOP_ACCEPT, 0, (uint32_t)d) < exp(lsw_sub - lsw_top);
      if (accept) {
        ts->tt[TT_SSIDE] = (double)side; ts->tt[TT_SSLOT] = (double)prop; ts->tt[TT_SLP] = ts->q_lp[prop]; ts->tt[TT_SH] = ts->q_h[prop];
        ts->tw_keep = prop;
      }
      ts->tt[TT_LSW] = d_lse(lsw_top, lsw_sub);
      ts->tt[TT_DEPTH] = (double)(d + 1);
      ts->tt[TT_RHOSIDE] = (double)side;
    }
    ts->tt[TT_STOP] = (double)stop;
    ts->tw_seq = d + 1; ts->tw_over = stop;
  }
  __syncthreads();
  // 3. publish: the state after combine d, and the STOP word if the trajectory is over
  if (o.publishes() && tid < 64) {
    const double val = ts->tt[tid < TT_N ? tid : 0];
    tw_st(t, tid < TT_N ? 16u * (unsigned)(TWB_TOP + 16 * ((d + 1) & 1) + tid) : PT_OOB, val, t.ittag | (unsigned)(d + 2));
    tw_st(t, (stop && tid == 0) ? 16u * (unsigned)TWB_STOP : PT_OOB, (double)(d + 1), t.ittag);
  }
  __syncthreads();
}

// two workgroups per chain: the whole vector, the workgroup's own sum, both sides publish their combines
struct Tw1CombineOps {
  const Chain &c;
  const Xch &xw;
  static constexpr int UNR = PT_UNR;
  __device__ __forceinline__ const Xch &x() const { return xw; }
  __device__ __forceinline__ int first() const { return fresh_tid(c); }
  __device__ __forceinline__ int end() const { return c.D; }
  __device__ __forceinline__ int leaf(ltp ts, int d) const { return uni_i(ts->pend_end[d]); }
  __device__ __forceinline__ void reduce(double (&v)[6], int first) const { drain_vmem(); block_sum(v, c.red(), first); }   // (barriers in block_sum)
  __device__ __forceinline__ bool publishes() const { return true; }
};
__device__ __noinline__ void cold_twin1_combine(const DevModel *Mg, const RunParams *Rg, int chain_, int side_, unsigned launch_, uint32_t iter_,
                                                int depth_, int valid_) {
  CMp M = (CMp)uni_ptr(Mg);
  CRp R = (CRp)uni_ptr(Rg);
  const int chain = (int)uni32((unsigned)chain_), side = (int)uni32((unsigned)side_), d = (int)uni32((unsigned)depth_);
  const int valid = (int)uni32((unsigned)valid_);
  const uint32_t iter = uni32(iter_);
  Chain c = make_chain(M, R, chain, side);
  const Xch x = tw1_watch(R, chain + side * R->chains, launch_);
  const Twin t = make_twin(R, chain, side, x.launch, iter);
  Tw1CombineOps o{c, x};
  twin_combine(o, t, side, d, valid, iter);
}

// New sample -> this side's chain position (from its own pool or from the other side's QC), draws array (side 0),
// adaptation (both sides, same inputs, same bits), rendezvous with the other side.  (cl_cold_twin_end below is the cluster's; the two
// move the sample differently: here the side that holds it publishes it in V_SCR1.)
__device__ __noinline__ void cold_twin1_end(const DevModel *Mg, const RunParams *Rg, int chain_, int side_, unsigned launch_, uint32_t iter_) {
  CMp M = (CMp)uni_ptr(Mg);
  CRp R = (CRp)uni_ptr(Rg);
  const int chain = (int)uni32((unsigned)chain_), side = (int)uni32((unsigned)side_), it = (int)uni32(iter_);
  Chain c = make_chain(M, R, chain, side);
  c.pst = model_load_static(M);
  const Xch x = tw1_watch(R, chain + side * R->chains, launch_);
  const Twin t = make_twin(R, chain, side, x.launch, (uint32_t)it);
  ltp ts = c.ts;
  const int tid = c.tid;
  __syncthreads();
  if (!uni_i(ts->tw_over)) {                          // this side ran out of doublings of its own: wait for the end
    if (tid < 64) tw_catch_up(x, t, ts, -1);
    __syncthreads();
  }
  const int owner = uni_i((int)ts->tt[TT_SSIDE]), slot = uni_i((int)ts->tt[TT_SSLOT]);
  if (tid == 0) end_trajectory_twin(ts, c.sc);
  __syncthreads();
  const bool warm = it < R->num_warmup;
  const bool save = (!warm || R->save_warmup) && side == 0;
  gdp row = draw_row(R, chain, c.sc);
  if (save && tid == 0) draw_row_head(row, ts);
  const unsigned sQ = c.soff(V_QC);
  if (owner == 1 - side) {
    if (tid < 64) { double dummy; tw_wait(x, t, TWB_QC, 1, t.ittag, dummy); }
    __syncthreads();
  }
  {
    // The side that holds the sample publishes it in V_SCR1 (write-through; free until the next transition's merges, which
    // start after the rendezvous below) and keeps QC itself a plainly stored vector, as in the one-workgroup sampler: what
    // reads QC later (Welford update, the model pass of the next transition) uses plain loads.
    const bool remote = owner == 1 - side;
    const unsigned s_src = remote ? c.soff(V_SCR1) : c.soff(V_POOLQ + slot), s_pub = c.soff(V_SCR1);
    for (int i = tid; i < c.D; i += PT_THREADS) {
      const double v = remote ? bld_s(t.ost, 8u * i, s_src) : bld(c.st, 8u * i, s_src);
      bst(c.st, 8u * i, sQ, v);
      if (owner == side) bst_s(c.st, 8u * i, s_pub, v);
      if (save) row[POTUS_N_SAMPLER_COLS + i] = v;
    }
  }
  drain_vmem();
  __syncthreads();
  if (owner == side && tid < 64) tw_st(t, tid == 0 ? 16u * (unsigned)TWB_QC : PT_OOB, 1.0, t.ittag);
  if (tid == 0) end_commit(ts, c.sc, !warm || R->save_warmup);
  if (warm) adapt_after_transition(c, (uint32_t)it, c.vec(V_QC));
  __syncthreads();
  if (tid == 0) c.sc->iter = it + 1;
  // Rendezvous: nothing of this transition is read from the other side's memory after this point, and the other side
  // must have reached the same point before this side's next transition overwrites what it may still be reading.
  drain_vmem();
  __syncthreads();
  if (tid < 64) {
    tw_st(t, tid == 0 ? 16u * (unsigned)(TWB_DONE + side) : PT_OOB, 1.0, t.ittag);
    tw_wait_ge(x, t, TWB_DONE + (1 - side), t.ittag);
  }
  __syncthreads();
}

// grid = 2 * chains; block b works for chain b % chains on side b / chains.  Both sides must be resident together.
__global__ __launch_bounds__(PT_THREADS) void k_run_twin(const DevModel *Mg, const RunParams *Rg, int n_iter, unsigned launch) {
  CMp M = (CMp)Mg;
  CRp R = (CRp)Rg;
  const int chain = blockIdx.x % R->chains, side = blockIdx.x / R->chains;
  Chain c = make_chain(M, R, chain, side);
  if (c.sc->status != 0) return;
  if (R->debug_drop_member == side + 1) return;    // test hook: a side that never shows up
  if (threadIdx.x == 0) cl_dead = 0;
  c.pst = model_setup_lds(M, c.lds);
  const Xch x = tw1_watch(R, chain + side * R->chains, launch);
  const Tw1Args ta{Mg, Rg, chain, side, launch};
  const int total = R->num_warmup + R->num_samples;
  for (int k = 0; k < n_iter; k++) {
    const int it = c.sc->iter;
    if (it >= total || uni_i(cl_dead)) break;
    cold_transition_begin(Mg, Rg, chain, (uint32_t)it, side);
    transition_tree_twin(c, x, ta, (uint32_t)it);
    if (uni_i(cl_dead)) break;
    cold_twin1_end(Mg, Rg, chain, side, launch, (uint32_t)it);
  }
  if (uni_i(cl_dead) && (c.tid & 63) == 0) c.sc->status = POTUS_ERR_WATCHDOG;   // every wave that is still alive
}

// ------------------------------------------------------------------------ cluster kernels (potus_cluster.hpp)
// grid = chains * K; block b works for chain b % chains as member b / chains.
// (twin mode: side s of a chain works in block chain + s * chains of state, scalars and exchange buffers)
__device__ __forceinline__ ClChain make_clchain(CMp M, CCp CL, CRp R, int chain, int m, unsigned launch, int side = 0) {
  ldp lds = (ldp)lds_dyn;
  ClChain c;
  const int Dpad = R->Dpad, K = CL->K;
  const int blk = chain + side * R->chains;
  double *state = R->state + (size_t)blk * V_COUNT * Dpad;
  c.M = M; c.CL = CL; c.part = (cip)(CL->part + m * CP_N); c.lds = lds; c.ts = (ltp)(lds + CL->lds_doubles);
  c.st = make_rsrc(state, (unsigned)V_COUNT * (unsigned)Dpad * 8u);
  c.sc = (gsc)(R->scal + (size_t)blk * K + m);
  c.key = RngKey{R->seed_lo, R->seed_hi, (uint32_t)(R->chain_id_offset + chain + 1)};
  c.perm = as_g(CL->perm);
  c.x.xb = make_rsrc(R->xbuf + (size_t)blk * (8 * K * CL->XW + 16), 4u * (unsigned)K * (unsigned)CL->XW * 16u + 16u);   // + the watchdog word
  c.x.epoch = 0; c.x.launch = launch; c.x.x1e = 0; c.x.K = K; c.x.m = m; c.x.XW = CL->XW; c.x.local = 0;
  c.D = M->D; c.Dpad = Dpad; c.tid = (int)threadIdx.x;
  c.e0 = c.part[CP_E0]; c.e1 = c.e0 + c.part[CP_NE];
  c.max_depth = R->max_depth; c.num_warmup = R->num_warmup; c.init_buffer = R->init_buffer; c.term_buffer = R->term_buffer;
  c.delta = R->delta; c.gamma = R->gamma; c.kappa = R->kappa; c.t0 = R->t0;
#ifdef POTUS_PROF
  c.prof = lds + CL->l_prof;
#endif
  return c;
}

// Parity hook on one cluster (grid = K): q, grad in Stan order; scratch = [2][Dpad] in internal order.
template <int CL_DW>
__global__ __launch_bounds__(PT_THREADS) void k_cl_logprob_grad(const DevModel *Mg, const ClModel *CLg, const RunParams *Rg, const double *q,
                                                                double *lp, double *grad, int n, double *scratch, unsigned launch) {
  CMp M = (CMp)Mg;
  CCp CL = (CCp)CLg;
  CRp R = (CRp)Rg;
  ClChain c = make_clchain(M, CL, R, 0, blockIdx.x, launch);
  c.cst = cl_setup_lds(M, CL, c.part, c.lds);
  const int D = M->D, Dpad = R->Dpad;
  const rsrc_t rs = make_rsrc(scratch, 2u * (unsigned)Dpad * 8u);
  for (int b = 0; b < n; b++) {
    for (int i = c.e0 + c.tid; i < c.e1; i += PT_THREADS) { const int si = c.perm[i]; bst_s(rs, 8u * i, 0, si >= 0 ? as_g(q)[(size_t)b * D + si] : 0.0); }
    cl_sync(c.x, c.red());
    ClPlainPolicy pol{rs, rs, 0u, (unsigned)Dpad * 8u, {0}};
    const double v = cl_pass<CL_DW>(M, CL, c.part, c.lds, c.cst, c.x, pol);
    drain_vmem();
    __syncthreads();
    for (int i = c.e0 + c.tid; i < c.e1; i += PT_THREADS) { const int si = c.perm[i]; if (si >= 0) as_g(grad)[(size_t)b * D + si] = bld(rs, 8u * i, (unsigned)Dpad * 8u); }
    if (blockIdx.x == 0 && c.tid == 0) lp[b] = v;
    cl_sync(c.x, c.red());
  }
}

template <int CL_DW>
__global__ __launch_bounds__(PT_THREADS) void k_cl_init(const DevModel *Mg, const ClModel *CLg, const RunParams *Rg, const double *q0, unsigned launch) {
  CMp M = (CMp)Mg;
  CCp CL = (CCp)CLg;
  CRp R = (CRp)Rg;
  const int chain = blockIdx.x % R->chains, r = blockIdx.x / R->chains, m = r % CL->K, side = r / CL->K;   // side 1: twin mode only
  ClChain c = make_clchain(M, CL, R, chain, m, launch, side);
  c.cst = cl_setup_lds(M, CL, c.part, c.lds);
  const int tid = c.tid;
  const unsigned sQ = c.soff(V_QC), sG = c.soff(V_GC);
  for (int i = c.e0 + tid; i < c.e1; i += PT_THREADS) { bst(c.st, 8u * i, c.soff(V_MINV), 1.0); bst(c.st, 8u * i, c.soff(V_WMEAN), 0.0); bst(c.st, 8u * i, c.soff(V_WM2), 0.0); }
  if (tid == 0) rule_reset_chain(c.sc, R->stepsize, R->init_buffer, R->window);
  __syncthreads();
  bool ok = false;
  const double radius = R->init_radius;
  for (uint32_t attempt = 0; attempt < 100 && !ok; attempt++) {
    for (int i = c.e0 + tid; i < c.e1; i += PT_THREADS) {
      const int si = c.perm[i];                      // < 0: padding element, stays 0
      if (si >= 0) bst_s(c.st, 8u * i, sQ, q0 ? as_g(q0)[(size_t)chain * c.D + si] : radius * (2.0 * rng_uniform(c.key, PT_ITER_PRE, RNG_INITS, attempt, (uint32_t)si) - 1.0));
    }
    cl_sync(c.x, c.red());
    ClPlainPolicy pol{c.st, c.st, sQ, sG, {0}};
    const double lp = cl_pass<CL_DW>(M, CL, c.part, c.lds, c.cst, c.x, pol);
    drain_vmem();
    __syncthreads();
    double bad[1] = {0.0};
    for (int i = c.e0 + tid; i < c.e1; i += PT_THREADS) bad[0] += isfinite(bld(c.st, 8u * i, sG)) ? 0.0 : 1.0;
    cl_allreduce(bad, c.red(), c.x, tid);
    ok = isfinite(lp) && bad[0] == 0.0;
    if (tid == 0 && ok) c.sc->lp_cur = lp;
    __syncthreads();
    if (q0) break;
  }
  if (!ok) { if (tid == 0) c.sc->status = POTUS_ERR_INIT; return; }   // every member takes this branch together
  cl_init_stepsize<CL_DW>(c, PT_ITER_PRE);
  if (tid == 0 && R->num_warmup == 0) rule_complete_adaptation(c.sc);
}

// New sample -> chain position and draws array (Stan order); warmup adaptation.
template <int CL_DW>
__device__ __forceinline__ void cl_transition_end(ClChain &c, CRp R, int chain, int it) {
  ltp ts = c.ts;
  const int tid = c.tid;
  if (tid == 0) end_trajectory(ts, c.sc);
  __syncthreads();
  const bool warm = it < R->num_warmup;
  const bool save = !warm || R->save_warmup;
  gdp row = draw_row(R, chain, c.sc);
  if (save && tid == 0 && c.x.m == 0) draw_row_head(row, ts);
  const unsigned s_src = c.soff(V_POOLQ + ts->sample_qid), sQ = c.soff(V_QC);
  for (int i = c.e0 + tid; i < c.e1; i += PT_THREADS) {
    const double v = bld_s(c.st, 8u * i, s_src);   // positions are read with sc1 loads (see potus_cluster.hpp)
    bst_s(c.st, 8u * i, sQ, v);
    const int si = c.perm[i];
    if (save && si >= 0) row[POTUS_N_SAMPLER_COLS + si] = v;
  }
  cl_sync(c.x, c.red());
  if (tid == 0) end_commit(ts, c.sc, save);
  if (warm) cl_adapt_after_transition<CL_DW>(c, (uint32_t)it);
  __syncthreads();
  if (tid == 0) c.sc->iter = it + 1;
  __syncthreads();
}

// The once-per-transition parts are separate functions, as in the one-workgroup sampler (cold_transition_*): the
// kernel proper then holds one copy of the model pass (the leaf of the tree) instead of four, and the only state that
// crosses a call is the exchange counter.  Arguments of a non-inlined function arrive in vector registers; everything
// wave-uniform is rebuilt from them here.
template <int CL_DW>
__device__ __noinline__ unsigned cl_cold_transition_begin(const DevModel *Mg, const ClModel *CLg, const RunParams *Rg, int chain_, int m_, int side_,
                                                          unsigned launch_, unsigned epoch_, uint32_t iter_) {
  CMp M = (CMp)uni_ptr(Mg);
  CCp CL = (CCp)uni_ptr(CLg);
  CRp R = (CRp)uni_ptr(Rg);
  ClChain c = make_clchain(M, CL, R, (int)uni32((unsigned)chain_), (int)uni32((unsigned)m_), uni32(launch_), (int)uni32((unsigned)side_));
  c.x.epoch = uni32(epoch_); c.x.local = uni_i(cl_local);   // (what k_cl_run found out about this launch's placement)
  c.cst = cl_load_static(CL, c.part);
  CPROF_START(c);
  cl_transition_begin<CL_DW>(c, uni32(iter_));
  CPROF_MARK(c, PF_INITCOPY);
  return c.x.epoch;
}
template <int CL_DW>
__device__ __noinline__ unsigned cl_cold_transition_end(const DevModel *Mg, const ClModel *CLg, const RunParams *Rg, int chain_, int m_,
                                                        unsigned launch_, unsigned epoch_, uint32_t iter_) {
  CMp M = (CMp)uni_ptr(Mg);
  CCp CL = (CCp)uni_ptr(CLg);
  CRp R = (CRp)uni_ptr(Rg);
  const int chain = (int)uni32((unsigned)chain_);
  ClChain c = make_clchain(M, CL, R, chain, (int)uni32((unsigned)m_), uni32(launch_));
  c.x.epoch = uni32(epoch_); c.x.local = uni_i(cl_local);   // (what k_cl_run found out about this launch's placement)
  c.cst = cl_load_static(CL, c.part);
  CPROF_START(c);
  cl_transition_end<CL_DW>(c, R, chain, (int)uni32(iter_));
  CPROF_MARK(c, PF_SAVE);
  return c.x.epoch;
}

// ------------------------------------------------------------------------ twin mode (potus_cluster.hpp): the cold parts
// The combine of doubling d (twin_combine above) by the cluster that built its subtree; leaf: momentum slot of its last leaf.
// A member's share of the vector, the cluster's all-reduce (after which every member's stores are complete), member 0 publishes.
struct ClCombineOps {
  ClChain &c;
  int last_leaf;
  static constexpr int UNR = CL_UNR;
  __device__ __forceinline__ const Xch &x() const { return c.x; }
  __device__ __forceinline__ int first() const { return cl_first(c); }
  __device__ __forceinline__ int end() const { return c.e1; }
  __device__ __forceinline__ int leaf(ltp, int) const { return last_leaf; }
  __device__ __forceinline__ void reduce(double (&v)[6], int) const { cl_allreduce(v, c.red(), c.x, c.tid); }
  __device__ __forceinline__ bool publishes() const { return c.x.m == 0; }
};
template <int CL_DW>
__device__ __noinline__ unsigned cl_cold_twin_combine(const DevModel *Mg, const ClModel *CLg, const RunParams *Rg, int chain_, int m_, int side_,
                                                      unsigned launch_, unsigned epoch_, uint32_t iter_, int depth_, int valid_, int leaf_) {
  CMp M = (CMp)uni_ptr(Mg);
  CCp CL = (CCp)uni_ptr(CLg);
  CRp R = (CRp)uni_ptr(Rg);
  const int chain = (int)uni32((unsigned)chain_), side = (int)uni32((unsigned)side_), d = (int)uni32((unsigned)depth_);
  const int valid = (int)uni32((unsigned)valid_), leaf = (int)uni32((unsigned)leaf_);
  const uint32_t iter = uni32(iter_);
  ClChain c = make_clchain(M, CL, R, chain, (int)uni32((unsigned)m_), uni32(launch_), side);
  c.x.epoch = uni32(epoch_); c.x.local = uni_i(cl_local);   // (what k_cl_run found out about this launch's placement)
  const Twin t = make_twin(R, chain, side, c.x.launch, iter);
  ClCombineOps o{c, leaf};
  twin_combine(o, t, side, d, valid, iter);
  return c.x.epoch;
}

// New sample -> this side's chain position (from its own pool or from the other side's QC), draws array (side 0),
// adaptation (both sides, same inputs), rendezvous with the other side.
template <int CL_DW>
__device__ __noinline__ unsigned cl_cold_twin_end(const DevModel *Mg, const ClModel *CLg, const RunParams *Rg, int chain_, int m_, int side_,
                                                  unsigned launch_, unsigned epoch_, uint32_t iter_) {
  CMp M = (CMp)uni_ptr(Mg);
  CCp CL = (CCp)uni_ptr(CLg);
  CRp R = (CRp)uni_ptr(Rg);
  const int chain = (int)uni32((unsigned)chain_), side = (int)uni32((unsigned)side_), it = (int)uni32(iter_);
  ClChain c = make_clchain(M, CL, R, chain, (int)uni32((unsigned)m_), uni32(launch_), side);
  c.x.epoch = uni32(epoch_); c.x.local = uni_i(cl_local);   // (what k_cl_run found out about this launch's placement)
  c.cst = cl_load_static(CL, c.part);
  const Twin t = make_twin(R, chain, side, c.x.launch, (uint32_t)it);
  ltp ts = c.ts;
  const int tid = c.tid;
  CPROF_START(c);
  __syncthreads();
  if (!uni_i(ts->tw_over)) {                          // this side ran out of doublings of its own: wait for the end
    if (tid < 64) tw_catch_up(c.x, t, ts, -1);
    __syncthreads();
  }
  const int owner = uni_i((int)ts->tt[TT_SSIDE]), slot = uni_i((int)ts->tt[TT_SSLOT]);
  if (tid == 0) end_trajectory_twin(ts, c.sc);
  __syncthreads();
  const bool warm = it < R->num_warmup;
  const bool save = (!warm || R->save_warmup) && side == 0;
  gdp row = draw_row(R, chain, c.sc);
  if (save && tid == 0 && c.x.m == 0) draw_row_head(row, ts);
  const unsigned sQ = c.soff(V_QC);
  if (owner == 1 - side) {
    if (tid < 64) { double dummy; tw_wait(c.x, t, TWB_QC, 1, t.ittag, dummy); }
    __syncthreads();
  }
  {
    const rsrc_t rsrc = owner == 1 - side ? t.ost : c.st;
    const unsigned s_src = owner == 1 - side ? sQ : c.soff(V_POOLQ + slot);
    for (int i = c.e0 + tid; i < c.e1; i += PT_THREADS) {
      const double v = bld_s(rsrc, 8u * i, s_src);
      bst_s(c.st, 8u * i, sQ, v);
      const int si = c.perm[i];
      if (save && si >= 0) row[POTUS_N_SAMPLER_COLS + si] = v;
    }
  }
  cl_sync(c.x, c.red());
  if (owner == side && c.x.m == 0 && tid < 64) tw_st(t, tid == 0 ? 16u * (unsigned)TWB_QC : PT_OOB, 1.0, t.ittag);
  if (tid == 0) end_commit(ts, c.sc, !warm || R->save_warmup);
  if (warm) cl_adapt_after_transition<CL_DW>(c, (uint32_t)it);
  __syncthreads();
  if (tid == 0) c.sc->iter = it + 1;
  // Rendezvous: nothing of this transition is read from the other side's memory after this point, and the other side
  // must have reached the same point before this side's next transition overwrites what it may still be reading.
  cl_sync(c.x, c.red());
  if (c.x.m == 0 && tid < 64) tw_st(t, tid == 0 ? 16u * (unsigned)(TWB_DONE + side) : PT_OOB, 1.0, t.ittag);
  if (tid < 64) tw_wait_ge(c.x, t, TWB_DONE + (1 - side), t.ittag);
  __syncthreads();
  CPROF_MARK(c, PF_SAVE);
  return c.x.epoch;
}

template <int CL_DW, bool TWIN>
__global__ __launch_bounds__(PT_THREADS) void k_cl_run(const DevModel *Mg, const ClModel *CLg, const RunParams *Rg, int n_iter, unsigned launch) {
  CMp M = (CMp)Mg;
  CCp CL = (CCp)CLg;
  CRp R = (CRp)Rg;
  // Which cluster a block works for.  Blocks are dealt to the eight XCDs round-robin: whenever the launch has a multiple of eight clusters, the blocks of one residue
  // b % 8 -- one XCD -- form whole clusters (cluster x + 8 q, member (b / 8) % K), so that the members of a cluster share an L2 and publish their exchange words with plain
  // stores (cl_find_local checks, per launch).  With a multiple of eight chains this is the mapping of rounds 1-6 (chain = b % chains, both clusters of a chain on one XCD);
  // with four chains x two clusters the clusters of a chain sit on XCDs c and c + 4.  Otherwise: chain = b % chains, members wherever they fall, write-through stores.
  int chain, m, side;
  {
    const int C = R->chains, K = CL->K, b = (int)blockIdx.x, sides = TWIN ? 2 : 1, ncl = C * sides;
    if (ncl % 8 == 0) {
      const int x = b & 7, i = b >> 3, q = i / K, j = x + 8 * q;                      // cluster j of ncl
      m = i % K;
      if (C % 8 == 0) { chain = x + 8 * (q / sides); side = q % sides; }
      else { chain = j % C; side = j / C; }
    } else {
      const int r = b / C;
      chain = b % C; m = TWIN ? r % K : r; side = TWIN ? r / K : 0;
    }
  }
  ClChain c = make_clchain(M, CL, R, chain, m, launch, side);
  if (c.sc->status != 0) return;
  if (R->debug_drop_member == m + 1) return;       // test hook: a member that never shows up
  c.cst = cl_setup_lds(M, CL, c.part, c.lds);
  cl_find_local(c.x, c.red());                      // (one all-reduce per launch: exchange words go out as plain stores when the cluster sits on one XCD)
  if (R->debug_drop_member == -1) {                 // test hook: the write-through path whatever the placement
    if (c.tid == 0) cl_local = 0;
    __syncthreads();
    c.x.local = 0;
  }
  if (c.tid == 0) c.sc->xcd_local = c.x.local;
  const ClTwinArgs ta{Mg, CLg, Rg, chain, m, side, launch};
  const int total = R->num_warmup + R->num_samples;
  for (int k = 0; k < n_iter; k++) {
    const int it = c.sc->iter;
    if (it >= total || uni_i(cl_dead)) break;
    c.x.epoch = uni32(cl_cold_transition_begin<CL_DW>(Mg, CLg, Rg, chain, m, side, launch, c.x.epoch, (uint32_t)it));
    cl_transition_tree<CL_DW, TWIN>(c, (uint32_t)it, ta);
    if (uni_i(cl_dead)) break;
    if (TWIN) c.x.epoch = uni32(cl_cold_twin_end<CL_DW>(Mg, CLg, Rg, chain, m, side, launch, c.x.epoch, (uint32_t)it));
    else c.x.epoch = uni32(cl_cold_transition_end<CL_DW>(Mg, CLg, Rg, chain, m, launch, c.x.epoch, (uint32_t)it));
  }
  if (uni_i(cl_dead) && (c.tid & 63) == 0) c.sc->status = POTUS_ERR_WATCHDOG;   // every wave that is still alive
#ifdef POTUS_PROF
  if (R->prof) for (int i = c.tid; i < PT_NPROF; i += PT_THREADS) as_g(R->prof)[((size_t)(chain + side * R->chains) * CL->K + m) * PT_NPROF + i] += c.prof[i];
#endif
}

// ------------------------------------------------------------------------ gradient of a dense-metric round (potus_dense.hpp)
// one workgroup per chain: the position and the slot receiving the gradient come from the chain's round descriptor
__global__ __launch_bounds__(PT_THREADS) void k_dn_grad1(const DevModel *Mg, const DnParams P) {
  const int chain = blockIdx.x;
  const DnRound &rd = P.rd[chain];
  if (!rd.active) return;
  CMp M = (CMp)Mg;
  ldp lds = (ldp)lds_dyn;
  const PassStatic pst = model_setup_lds(M, lds);
  const int D = M->D;
  PlainPolicy pol{make_rsrc(dn_vec(P, chain, rd.qin), 8u * D), make_rsrc(dn_vec(P, chain, rd.gout), 8u * D), 0u, 0u, {0}};
  const double v = model_pass(M, lds, pst, pol);
  if (threadIdx.x == 0) P.lpbuf[chain] = v;
}
// one cluster per chain (models beyond one workgroup): the position goes into the cluster's internal element order
// (scratch vectors of the chain's state block), the gradient comes back in Stan's order
template <int CL_DW>
__global__ __launch_bounds__(PT_THREADS) void k_dn_gradK(const DevModel *Mg, const ClModel *CLg, const RunParams *Rg, const DnParams P, unsigned launch) {
  CMp M = (CMp)Mg;
  CCp CL = (CCp)CLg;
  CRp R = (CRp)Rg;
  const int chain = blockIdx.x % R->chains, m = blockIdx.x / R->chains;
  const DnRound &rd = P.rd[chain];
  if (!rd.active) return;                            // the whole cluster
  ClChain c = make_clchain(M, CL, R, chain, m, launch);
  c.cst = cl_setup_lds(M, CL, c.part, c.lds);
  const double *q = dn_vec(P, chain, rd.qin);
  double *grad = dn_vec(P, chain, rd.gout);
  const unsigned sQ = c.soff(V_QA1), sG = c.soff(V_GC);
  for (int i = c.e0 + c.tid; i < c.e1; i += PT_THREADS) { const int si = c.perm[i]; bst_s(c.st, 8u * i, sQ, si >= 0 ? as_g(q)[si] : 0.0); }
  cl_sync(c.x, c.red());
  ClPlainPolicy pol{c.st, c.st, sQ, sG, {0}};
  const double v = cl_pass<CL_DW>(M, CL, c.part, c.lds, c.cst, c.x, pol);
  drain_vmem();
  __syncthreads();
  for (int i = c.e0 + c.tid; i < c.e1; i += PT_THREADS) { const int si = c.perm[i]; if (si >= 0) as_g(grad)[si] = bld(c.st, 8u * i, sG); }
  if (m == 0 && c.tid == 0) P.lpbuf[chain] = v;
}
// the point found by k_init / k_cl_init (diagonal state block) -> the dense state block, Stan's order
__global__ void k_dn_import_q(const RunParams *Rg, const DnParams P, const int *perm, int Dint) {
  const int chain = blockIdx.y;
  const double *src = Rg->state + ((size_t)chain * V_COUNT + V_QC) * Rg->Dpad;
  double *dst = dn_vec(P, chain, DV_QC);
  const int n = perm ? Dint : P.D;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int si = perm ? perm[i] : i;
    if (si >= 0) dst[si] = src[i];
  }
}

#include "potus_rows.hpp"   // the output row of a draw: its column blocks, its builder and the kernels around it

// Many data sets in one handle (potus_set_datasets): Mg = [n_datasets] models that differ only in the poll outcomes (pd), chain c
// uses data set c / chains_per_ds.  One workgroup per chain, diagonal metric: the bodies of k_init / k_run with the chain's model.
__global__ __launch_bounds__(PT_THREADS) void k_init_ds(const DevModel *Mg, const RunParams *Rg, const double *q0, int chains_per_ds) {
  init_one_workgroup((CMp)(Mg + blockIdx.x / chains_per_ds), (CRp)Rg, blockIdx.x, 0, q0);
}
__global__ __launch_bounds__(PT_THREADS) void k_run_ds(const DevModel *Mg_all, const RunParams *Rg, int n_iter, int chains_per_ds) {
  run_one_workgroup(Mg_all + blockIdx.x / chains_per_ds, Rg, blockIdx.x, n_iter);
}

#include "potus_loo.hpp"   // per-poll log-likelihoods and PSIS-LOO (after potus_rows.hpp, whose row builder it shares)
#include "potus_outcomes.hpp"   // joint election outcomes: EV histogram, tipping point, joint win counts
#include "potus_scenario.hpp"   // conditional forecasts and the covariance of the state scores
#include "potus_timeline.hpp"   // run dates as the data sets of one handle: their rows, scores and summaries
#include "potus_sens.hpp"       // prior sensitivity by refit: the distance between two sets of draws, per column
#include "potus_crossval.hpp"   // exact cross-validation: held-out polls under the draws of the data set that did not see them
#include "potus_loo_mm.hpp"     // moment matching for PSIS-LOO: the pass under an affine map, weighted moments, PSIS of general ratios
#include "potus_loo_mm_rules.hpp"
#include "potus_optimize.hpp"   // the posterior mode: batched L-BFGS, one workgroup per path
#include "potus_laplace.hpp"    // the Laplace approximation at a mode: Hessian, factor, draws
#include "potus_pathfinder.hpp" // Pathfinder: a normal around every iterate of an L-BFGS path, the best ELBO, draws
#include "potus_advi.hpp"       // mean-field ADVI: stochastic-gradient tracks, the ELBO on a chip-wide grid, draws
#include "potus_eloo.hpp"       // E_loo: expectations under the leave-one-out posteriors, pointwise and as a product on the matrix cores (included last: potus_loo_mm.hpp's reason)
#include "potus_ppc.hpp"        // posterior predictive checks: replicated polls, PIT and LOO-PIT sums, group statistics (after potus_eloo.hpp: it adds kernels only)
#include "potus_fscore.hpp"     // proper scoring rules of the joint forecast: CRPS, energy, variogram, Dawid-Sebastiani (it adds kernels only)

// ======================================================================== host
namespace {

thread_local std::string g_err;
int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  g_err = buf;
  return code;
}
#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(POTUS_ERR_DEVICE, "%s failed: %s", #x, hipGetErrorString(e_)); } while (0)

struct Layout { // column blocks of one output row after the 7 sampler columns
  int D, ncols;
  int o_zT, o_Z, o_c, o_m, o_pop, o_mue, o_rho, o_ze, o_nn, o_ns, o_zb;
};
Layout make_layout(const potus_data *d) {
  Layout L{};
  const bool full = d->variant == POTUS_VARIANT_FULL;
  int o = 0;
  L.o_zT = o; o += d->S;
  L.o_Z = o; o += d->S * d->T;
  L.o_c = o; o += d->P;
  if (full) { L.o_m = o; o += d->M; L.o_pop = o; o += d->Pop; L.o_mue = o; o += 1; L.o_rho = o; o += 1; L.o_ze = o; o += d->T; }
  else L.o_m = L.o_pop = L.o_mue = L.o_rho = L.o_ze = -1;
  L.o_nn = o; o += d->N_national_polls;
  L.o_ns = o; o += d->N_state_polls;
  L.o_zb = o; o += d->S;
  L.D = o;
  L.ncols = row_cols(d, L.D).ncols;
  return L;
}

int validate(const potus_data *d) {
  if (!d) return fail(POTUS_ERR_ARG, "null data");
  if (d->variant != POTUS_VARIANT_FULL && d->variant != POTUS_VARIANT_NO_MODE) return fail(POTUS_ERR_ARG, "unknown variant %d", d->variant);
  const bool full = d->variant == POTUS_VARIANT_FULL;
  if (d->S < 1 || d->P < 1 || d->N_state_polls < 0 || d->N_national_polls < 0)
    return fail(POTUS_ERR_ARG, "bad sizes: S = %d, P = %d, N_state_polls = %d, N_national_polls = %d", d->S, d->P, d->N_state_polls, d->N_national_polls);
  if (d->T < 2) return fail(POTUS_ERR_ARG, "T = %d: the model is a random walk over days, at least two are needed", d->T);
  if (full && (d->M < 1 || d->Pop < 1)) return fail(POTUS_ERR_ARG, "bad sizes M/Pop");
  auto range = [&](const int32_t *v, int n, int lo, int hi, const char *name) {
    if (n > 0 && !v) return fail(POTUS_ERR_ARG, "%s is null", name);
    for (int i = 0; i < n; i++) if (v[i] < lo || v[i] > hi) return fail(POTUS_ERR_ARG, "%s[%d] = %d outside [%d,%d]", name, i + 1, v[i], lo, hi);
    return 0;
  };
  int rc;
  // declared bounds stan:9-17; state = S+1 is declared legal but indexes out of range at stan:97
  if ((rc = range(d->state, d->N_state_polls, 1, d->S, "state"))) return rc;
  if ((rc = range(d->day_state, d->N_state_polls, 1, d->T, "day_state"))) return rc;
  if ((rc = range(d->day_national, d->N_national_polls, 1, d->T, "day_national"))) return rc;
  if ((rc = range(d->poll_state, d->N_state_polls, 1, d->P, "poll_state"))) return rc;
  if ((rc = range(d->poll_national, d->N_national_polls, 1, d->P, "poll_national"))) return rc;
  if (full) {
    if ((rc = range(d->poll_mode_state, d->N_state_polls, 1, d->M, "poll_mode_state"))) return rc;
    if ((rc = range(d->poll_mode_national, d->N_national_polls, 1, d->M, "poll_mode_national"))) return rc;
    if ((rc = range(d->poll_pop_state, d->N_state_polls, 1, d->Pop, "poll_pop_state"))) return rc;
    if ((rc = range(d->poll_pop_national, d->N_national_polls, 1, d->Pop, "poll_pop_national"))) return rc;
    if ((d->N_state_polls && !d->unadjusted_state) || (d->N_national_polls && !d->unadjusted_national)) return fail(POTUS_ERR_ARG, "unadjusted_* is null");
    for (int i = 0; i < d->N_state_polls; i++) if (!(d->unadjusted_state[i] >= 0 && d->unadjusted_state[i] <= 1)) return fail(POTUS_ERR_ARG, "unadjusted_state outside [0,1]");
    for (int i = 0; i < d->N_national_polls; i++) if (!(d->unadjusted_national[i] >= 0 && d->unadjusted_national[i] <= 1)) return fail(POTUS_ERR_ARG, "unadjusted_national outside [0,1]");
  }
  if ((d->N_state_polls && (!d->n_democrat_state || !d->n_two_share_state)) || (d->N_national_polls && (!d->n_democrat_national || !d->n_two_share_national)))
    return fail(POTUS_ERR_ARG, "poll counts are null");
  for (int i = 0; i < d->N_state_polls; i++) if (d->n_democrat_state[i] < 0 || d->n_democrat_state[i] > d->n_two_share_state[i]) return fail(POTUS_ERR_ARG, "n_democrat_state outside [0,N]");
  for (int i = 0; i < d->N_national_polls; i++) if (d->n_democrat_national[i] < 0 || d->n_democrat_national[i] > d->n_two_share_national[i]) return fail(POTUS_ERR_ARG, "n_democrat_national outside [0,N]");
  if (!d->mu_b_prior || !d->state_weights || !d->state_covariance_0) return fail(POTUS_ERR_ARG, "null prior/weights/covariance");
  const int S = d->S;
  for (int i = 0; i < S; i++) for (int j = 0; j < i; j++) {
    const double a = d->state_covariance_0[i + (size_t)j * S], b = d->state_covariance_0[j + (size_t)i * S];
    if (std::fabs(a - b) > 1e-8 * std::max(1.0, std::max(std::fabs(a), std::fabs(b)))) return fail(POTUS_ERR_ARG, "state_covariance_0 is not symmetric");
  }
  return 0;
}

// FNV-1a over everything the posterior depends on (sizes, index vectors, counts, flags, prior, weights, covariance, scales)
unsigned long long hash_data(const potus_data *d) {
  unsigned long long h = 1469598103934665603ull;
  auto mix = [&](const void *p, size_t n) { const unsigned char *b = (const unsigned char *)p; for (size_t i = 0; p && i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } };
  const bool full = d->variant == POTUS_VARIANT_FULL;
  const int32_t dims[8] = {d->N_national_polls, d->N_state_polls, d->T, d->S, d->P, full ? d->M : 0, full ? d->Pop : 0, d->variant};
  mix(dims, sizeof dims);
  const size_t ns = (size_t)d->N_state_polls * 4, nn = (size_t)d->N_national_polls * 4;
  mix(d->state, ns); mix(d->day_state, ns); mix(d->day_national, nn); mix(d->poll_state, ns); mix(d->poll_national, nn);
  if (full) { mix(d->poll_mode_state, ns); mix(d->poll_mode_national, nn); mix(d->poll_pop_state, ns); mix(d->poll_pop_national, nn);
              mix(d->unadjusted_state, ns * 2); mix(d->unadjusted_national, nn * 2); }
  mix(d->n_democrat_national, nn); mix(d->n_two_share_national, nn); mix(d->n_democrat_state, ns); mix(d->n_two_share_state, ns);
  mix(d->mu_b_prior, (size_t)d->S * 8); mix(d->state_weights, (size_t)d->S * 8); mix(d->state_covariance_0, (size_t)d->S * d->S * 8);
  const double sc[9] = {d->sigma_c, full ? d->sigma_m : 0, full ? d->sigma_pop : 0, d->sigma_measure_noise_national, d->sigma_measure_noise_state,
                        full ? d->sigma_e_bias : 0, d->random_walk_scale, d->mu_b_T_scale, d->polling_bias_scale};
  mix(sc, sizeof sc);
  return h;
}

// lower Cholesky factor, column-major (cholesky_decompose, stan:52-54)
bool chol(const std::vector<double> &A, std::vector<double> &L, int n) {
  L.assign((size_t)n * n, 0.0);
  for (int j = 0; j < n; j++) {
    double s = A[j + (size_t)j * n];
    for (int k = 0; k < j; k++) s -= L[j + (size_t)k * n] * L[j + (size_t)k * n];
    if (!(s > 0)) return false;
    const double ljj = std::sqrt(s);
    L[j + (size_t)j * n] = ljj;
    for (int i = j + 1; i < n; i++) {
      double t = A[i + (size_t)j * n];
      for (int k = 0; k < j; k++) t -= L[i + (size_t)k * n] * L[j + (size_t)k * n];
      L[i + (size_t)j * n] = t / ljj;
    }
  }
  return true;
}

struct Sampler {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DevModel M{};
  DevModel *dM = nullptr; // device copy read by the kernels through scalar loads
  RunParams *dR = nullptr;
  RunParams R{};
  potus_opts opts{};
  Layout L{};
  std::vector<void *> allocs;
  size_t lds_bytes = 0;
  std::string k1_unsupported;   // why the one-workgroup kernels cannot run this model (empty: they can); cluster mode may still
  bool inited = false;
  double last_ms = 0;
  long long last_leapfrogs = 0;
  double warm_ms = 0, samp_ms = 0;
  std::vector<double> LB, LT, LW; // column-major host copies (transformed data)
  // cluster mode (K > 1)
  int K = 1, cl_dw = 8;
  int twin = 0;             // two clusters per chain (one per end of the trajectory): state, scalars and exchange buffers hold 2 x chains blocks
  int sides() const { return twin ? 2 : 1; }
  bool coop() const { return K > 1 || twin; }   // workgroups that wait for each other: the whole grid must be resident
  unsigned launch_id = 0;   // tags the exchange words of each launch
  ClModel CL{};
  ClModel *dCL = nullptr;
  size_t cl_lds_bytes = 0;
  std::vector<int> h_ps, h_pt, h_pp, h_pm, h_ppop, h_pq, h_dayptr, h_perm;   // day-sorted polls (host copies)
  std::vector<double> h_w;    // state_weights
  std::vector<double> h_pu;
  unsigned long long data_hash = 0;   // FNV-1a over the data block: handles that pool their draws must hold the same posterior
  // dense metric (potus_dense.hpp)
  bool dense = false;
  DnParams dn{};
  int *h_active = nullptr;                 // pinned host copy of the per-chain activity flags
  int dn_win_counter = 0, dn_win_next = 0, dn_win_size = 0, dn_wf_n = 0;   // host mirror of the warm-up window schedule
  hipEvent_t mv0 = nullptr, mv1 = nullptr;
  static constexpr int DN_AHEAD = 4;       // leaf rounds the host keeps queued beyond the one whose activity flags it has seen
  hipEvent_t rv0[DN_AHEAD] = {}, rv1[DN_AHEAD] = {}, rdone[DN_AHEAD] = {};   // per queued round: around its matrix pass, after its flag copy
  bool dn_pending = false;                 // pooled_metric = 2: a window end whose moments wait for the host (potus_dense_pool_window / _finish)
  int dn_pending_n = 0; unsigned dn_pending_iter = 0; double dn_pending_cov_ms = 0;
  int rv_launches[DN_AHEAD] = {1, 1, 1, 1};   // ... and the launches of that pass (pooled metric: one per DNP_RMAX right-hand sides)
  double mv_ms = 0;                        // time spent in the matrix passes (k_dn_symv + finish, events), their number and the bytes they loaded
  int mv_launches_pending = 0;             // matrix passes between the event pair of the last timed dense_matvec (the first pass of a transition: two)
  long long mv_calls = 0, mv_bytes = 0, dn_rounds = 0, dn_pass_bytes[2] = {0, 0};   // bytes per pass at DN_RB rows per workgroup / at the handle's DnParams::rb
  double we_cov_ms = 0, we_chol_ms = 0, we_eps_ms = 0;   // window ends: covariance, factorisation, init_stepsize (host clock around synchronised sections)
  int we_count = 0;
  // potus_set_datasets: n_ds models that differ only in the poll outcomes (0: one data set, dM)
  // potus_set_datasets_ex (ds_ex): ... in the poll outcomes and sizes, and with ds_own_prior in mu_b_prior / mu_b_T_scale (own mat, own aT)
  int n_ds = 0;
  DevModel *dMs = nullptr;
  bool ds_ex = false, ds_own_prior = false;
  std::vector<double> h_mat, h_cov, h_w_raw;   // host copies for the per-data-set models: the packed mat, state_covariance_0, state_weights as given
  double h_nsd = 0, h_rw_scale = 0, h_T_scale = 0;   // sqrt(w' cov w), random_walk_scale, mu_b_T_scale
  double h_scales[9] = {};                             // the nine scales as given to potus_create (data_scales)
  std::vector<int> h_seg_src;                          // per segment of seg_scale: the scale it holds, -1 = 1.0 (seg_scales)
  bool ds_grid = false;                                // potus_set_datasets_grid with scales: every data set has all of these of its own
  int chains_per_ds() const { return n_ds ? R.chains / n_ds : R.chains; }
  // potus_laplace: the rows [lp__, six NaN, x] of the last call's draws, [lap_modes][lap_draws][7 + D]; apart from chain state
  double *lap_rows = nullptr;
  int lap_modes = 0, lap_draws = 0;
  std::vector<int> lap_code;   // per mode: 0 = its rows are draws
  // potus_pathfinder[_path]: the same for the last call's draws, [pf_paths][pf_draws][7 + D]
  double *pf_rows = nullptr;
  int pf_paths = 0, pf_draws = 0;
  std::vector<int> pf_code;    // per path: 0 = its rows are draws
  // potus_advi: the same, [vi_runs][vi_draws][7 + D]
  double *vi_rows = nullptr;
  int vi_runs = 0, vi_draws = 0;
  std::vector<int> vi_code;    // per run: 0 = its rows are draws
};

std::mutex g_mu;
std::vector<Sampler *> g_handles;
// Cluster kernels need all their workgroups co-resident (they wait for each other): whatever launches work on a device --
// sampler runs, the parity hook, write_array, the posterior summaries, the CSV writer's row kernels -- holds that device's
// mutex from launch to completion, so host threads driving one handle per GPU run side by side while two calls on one GPU take
// turns.  potus_run_many locks the devices of its handles in ascending order.
constexpr int POTUS_MAX_DEVICES = 64;
std::mutex g_device_mu[POTUS_MAX_DEVICES];
struct DeviceLocks {
  std::vector<std::unique_lock<std::mutex>> held;
  DeviceLocks() {}
  explicit DeviceLocks(std::vector<int> devs) { take(std::move(devs)); }
  explicit DeviceLocks(int dev) { take({dev}); }
  void take(std::vector<int> devs) {
    std::sort(devs.begin(), devs.end());
    devs.erase(std::unique(devs.begin(), devs.end()), devs.end());
    for (int d : devs) held.emplace_back(g_device_mu[std::min(std::max(d, 0), POTUS_MAX_DEVICES - 1)]);
  }
};
// the caller's HIP device is put back on every return path (the library works on the handles' devices)
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// What a *_device entry point works on: a block of the caller's in the memory of GPU `device`.  Declared on the entry point's stack once every check
// that needs no device has passed; open() names the device, locks it, makes it current and refuses a pointer that is not that GPU's memory --
// a kernel handed a host pointer, or another GPU's without peer access, is a memory fault.  The lock goes and the caller's device comes back with the object.
struct DeviceBlock {
  DeviceGuard guard;
  DeviceLocks lock;
  int open(const char *what, int device, const void *ptr, const char *ptr_name = "block") {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(POTUS_ERR_DEVICE, "%s: no HIP device %d", what, device);
    lock.take({device});
    HIP_TRY(hipSetDevice(device));
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != device) {
      (void)hipGetLastError();
      return fail(POTUS_ERR_ARG, "%s: the %s is not device memory of GPU %d", what, ptr_name, device);
    }
    return 0;
  }
};

Sampler *get(int h) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (h < 0 || h >= (int)g_handles.size()) return nullptr;
  return g_handles[h];
}

// Calls that pool every chain of a handle into one posterior: a handle with several data sets holds several posteriors
int refuse_many_datasets(const Sampler *sp, const char *what) {
  if (!sp->n_ds) return 0;
  return fail(POTUS_ERR_STATE, "%s pools all chains of a handle, which holds %d data sets (potus_set_datasets): slice the chains per data set "
                               "(potus_get_draws / potus_write_array, chains d * %d .. (d + 1) * %d - 1) or use potus_sbc_ranks", what, sp->n_ds,
              sp->chains_per_ds(), sp->chains_per_ds());
}

// Calls that build rows with the handle's one model: the data sets of potus_set_datasets_ex have models of their own
int refuse_own_models(const Sampler *sp, const char *what) {
  if (!sp->ds_ex) return 0;
  return fail(POTUS_ERR_UNSUPPORTED, "%s builds its rows with the handle's own model; the %d data sets of this handle (potus_set_datasets_ex) have "
                                     "models of their own (poll sizes, mu_b_prior, mu_b_T_scale): use potus_write_array or a stand-alone handle", what, sp->n_ds);
}

// One owner for every temporary device buffer of a call: freed on every return path.
struct DevBufs {
  std::vector<void *> v;
  ~DevBufs() { for (void *p : v) (void)hipFree(p); }
  template <class T> hipError_t alloc(T **p, size_t bytes) {
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, std::max<size_t>(bytes, 8));
    if (e == hipSuccess) v.push_back(q);
    *p = static_cast<T *>(q);
    return e;
  }
  // ... for the analysis calls: a refusal that names the caller and the size
  template <class T> int get(T **p, size_t bytes, const char *what) {
    if (alloc(p, bytes) == hipSuccess) return 0;
    (void)hipGetLastError();
    return fail(POTUS_ERR_DEVICE, "%s: hipMalloc of %zu bytes (%.1f MB) failed", what, bytes, bytes / 1048576.0);
  }
};

// One pair of events around a span of a stream's work, destroyed on every return path: HIP_TRY(t.made) once, start() and stop() around the span,
// elapsed() once the stream has been synchronised.  A call that may ignore a failed reading tests elapsed(); one that may not returns elapsed_or_fail().
struct EventTimer {
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t made, err = hipSuccess;
  EventTimer() { if ((made = hipEventCreate(&a)) == hipSuccess) made = hipEventCreate(&b); }
  EventTimer(const EventTimer &) = delete;
  ~EventTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  hipError_t start(hipStream_t st) { return hipEventRecord(a, st); }
  hipError_t stop(hipStream_t st) { return hipEventRecord(b, st); }
  bool elapsed(double *ms) {   // *ms is left alone when the reading fails
    float f = 0.f;
    if ((err = hipEventElapsedTime(&f, a, b)) == hipSuccess) *ms = f;
    return err == hipSuccess;
  }
  int elapsed_or_fail(double *ms) { return elapsed(ms) ? 0 : fail(POTUS_ERR_DEVICE, "hipEventElapsedTime failed: %s", hipGetErrorString(err)); }
};

// what every *_timing getter does: the calling thread's last figures, n of them
int timing_out(const char *what, const double *src, int n, double *ms) {
  if (!ms) return fail(POTUS_ERR_ARG, "%s: null output", what);
  std::copy(src, src + n, ms);
  return 0;
}

template <class T>
int upload(Sampler *s, const std::vector<T> &v, const T **dst) {
  void *p = nullptr;
  const size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
  HIP_TRY(hipMalloc(&p, bytes));
  s->allocs.push_back(p);
  if (!v.empty()) HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *dst = static_cast<const T *>(p);
  return 0;
}

// chol((scale / nsd)^2 cov), column-major (stan:50-54)
bool scaled_chol(const std::vector<double> &cov, double nsd, double scale, int S, std::vector<double> &Lout) {
  std::vector<double> A(cov);
  const double f = (scale / nsd) * (scale / nsd);
  for (auto &x : A) x *= f;
  return chol(A, Lout, S);
}
// What mu_b_prior and mu_b_T_scale put into DevModel::mat: LT_t [k][s], LT [s][k], prior [S], prior_ext [S + 2] (prior, its weighted average, 0).
// build_model packs them; potus_set_datasets_ex rebuilds them per data set with the same code, so that the bytes are those of a stand-alone handle.
struct PriorBlocks { std::vector<double> LT, LT_t, LTr, prior, px; };
bool prior_blocks(const std::vector<double> &cov, double nsd, const std::vector<double> &w, int S, const double *mu_b_prior, double mu_b_T_scale, PriorBlocks &B) {
  if (!scaled_chol(cov, nsd, mu_b_T_scale, S, B.LT)) return false;
  B.LT_t.resize((size_t)S * S); B.LTr.resize((size_t)S * S);
  for (int s = 0; s < S; s++) for (int k = 0; k < S; k++) { B.LT_t[(size_t)k * S + s] = B.LT[s + (size_t)k * S]; B.LTr[(size_t)s * S + k] = B.LT[s + (size_t)k * S]; }
  B.prior.assign(mu_b_prior, mu_b_prior + S);
  B.px = B.prior;
  double nat = 0; for (int s = 0; s < S; s++) nat += w[s] * B.px[s];   // stan:87 applied to the prior part of mu_b
  B.px.push_back(nat); B.px.push_back(0.0);
  return true;
}

// What random_walk_scale and polling_bias_scale put into DevModel::mat: Lw_ext [SE][SP] (L_W [s][k], then the row v = L_W' w), LB_t [k][s], LB [s][k].
// build_model packs them; potus_set_datasets_grid rebuilds them per data set with the same code.  LW and LB are the column-major factors.
struct ScaleBlocks { std::vector<double> LW, LB, Lw_ext, LB_t, LBr; };
bool scale_blocks(const std::vector<double> &cov, double nsd, const std::vector<double> &w, int S, int SE, int SP, double random_walk_scale, double polling_bias_scale, ScaleBlocks &B) {
  if (!scaled_chol(cov, nsd, polling_bias_scale, S, B.LB) || !scaled_chol(cov, nsd, random_walk_scale, S, B.LW)) return false;
  auto at = [&](const std::vector<double> &Lm, int i, int j) { return Lm[i + (size_t)j * S]; };
  B.Lw_ext.assign((size_t)SE * SP, 0.0); B.LB_t.resize((size_t)S * S); B.LBr.resize((size_t)S * S);
  for (int s = 0; s < S; s++) for (int k = 0; k < S; k++) {
    B.Lw_ext[(size_t)s * SP + k] = at(B.LW, s, k);
    B.LB_t[(size_t)k * S + s] = at(B.LB, s, k); B.LBr[(size_t)s * S + k] = at(B.LB, s, k);
  }
  for (int k = 0; k < S; k++) { double v = 0; for (int s = k; s < S; s++) v += at(B.LW, s, k) * w[s]; B.Lw_ext[(size_t)S * SP + k] = v; }
  return true;
}
// The scales of a model in the order of hash_data's sc[9] (POTUS_N_SCALES, potus_hmc.h), as given: the no-mode variant never reads sc[1], sc[2], sc[5].
enum { SC_C = 0, SC_M, SC_POP, SC_NOISE_NATIONAL, SC_NOISE_STATE, SC_E_BIAS, SC_RANDOM_WALK, SC_MU_B_T, SC_POLLING_BIAS };
void data_scales(const potus_data *d, double *sc) {
  sc[SC_C] = d->sigma_c; sc[SC_M] = d->sigma_m; sc[SC_POP] = d->sigma_pop; sc[SC_NOISE_NATIONAL] = d->sigma_measure_noise_national;
  sc[SC_NOISE_STATE] = d->sigma_measure_noise_state; sc[SC_E_BIAS] = d->sigma_e_bias; sc[SC_RANDOM_WALK] = d->random_walk_scale;
  sc[SC_MU_B_T] = d->mu_b_T_scale; sc[SC_POLLING_BIAS] = d->polling_bias_scale;
}
// ... what they put into the scalar fields of DevModel
void model_scales(DevModel &M, const double *sc) {
  M.sigma_c = sc[SC_C]; M.sigma_m = sc[SC_M]; M.sigma_pop = sc[SC_POP]; M.sigma_e = sc[SC_E_BIAS];
  M.sigma_ns = sc[SC_NOISE_STATE]; M.sigma_nn = sc[SC_NOISE_NATIONAL];
  // (stan:50-52 uses square(scale): the sign of a scale does not reach the factors, chol(c^2 A) = |c| chol(A))
  M.aT = std::fabs(sc[SC_MU_B_T] / sc[SC_RANDOM_WALK]); M.aB = std::fabs(sc[SC_POLLING_BIAS] / sc[SC_RANDOM_WALK]);
}
// ... into the sigma slot of a poll in pd
double poll_sigma(const double *sc, bool national) { return sc[national ? SC_NOISE_NATIONAL : SC_NOISE_STATE]; }
// ... and into seg_scale: src names the scale of every segment (-1: none, 1.0)
std::vector<double> seg_scales(const std::vector<int> &src, const double *sc) {
  std::vector<double> v(src.size());
  for (size_t i = 0; i < src.size(); i++) v[i] = src[i] < 0 ? 1.0 : sc[src[i]];
  return v;
}

int build_model(Sampler *sp, const potus_data *d) {
  const bool full = d->variant == POTUS_VARIANT_FULL;
  const int S = d->S, T = d->T, Ns = d->N_state_polls, Nn = d->N_national_polls;
  DevModel &M = sp->M;
  const Layout &L = sp->L;
  if (S + 1 > 64) return fail(POTUS_ERR_UNSUPPORTED, "S = %d: this kernel maps states to the 64 lanes of a wave (S <= 63)", S);
  auto k1_fail = [&](const char *fmt, auto... args) { char buf[256]; std::snprintf(buf, sizeof buf, fmt, args...); if (sp->k1_unsupported.empty()) sp->k1_unsupported = buf; };
  if (T > PT_NW * PT_CH) k1_fail("T = %d: one workgroup per chain handles T <= %d days", T, PT_NW * PT_CH);
  M.S = S; M.T = T; M.P = d->P; M.M = full ? d->M : 0; M.Pop = full ? d->Pop : 0; M.Ns = Ns; M.Nn = Nn; M.Npoll = Ns + Nn;
  M.D = L.D; M.full = full;
  M.SE = S + 1; M.SP = S | 1; M.TP = T | 1;
  M.o_zT = L.o_zT; M.o_Z = L.o_Z; M.o_c = L.o_c; M.o_m = L.o_m; M.o_pop = L.o_pop; M.o_mue = L.o_mue; M.o_rho = L.o_rho;
  M.o_ze = L.o_ze; M.o_nn = L.o_nn; M.o_ns = L.o_ns; M.o_zb = L.o_zb; M.nmid = L.o_nn - L.o_c;
  double *sc = sp->h_scales;
  data_scales(d, sc);
  model_scales(M, sc);

  // transformed data (stan:42-55)
  std::vector<double> w(d->state_weights, d->state_weights + S), cov(d->state_covariance_0, d->state_covariance_0 + (size_t)S * S);
  double nsd2 = 0;
  for (int i = 0; i < S; i++) for (int j = 0; j < S; j++) nsd2 += w[i] * cov[i + (size_t)j * S] * w[j];
  const double nsd = std::sqrt(nsd2);
  PriorBlocks pb;
  ScaleBlocks sb;
  if (!scale_blocks(cov, nsd, w, S, M.SE, M.SP, d->random_walk_scale, d->polling_bias_scale, sb) || !prior_blocks(cov, nsd, w, S, d->mu_b_prior, d->mu_b_T_scale, pb))
    return fail(POTUS_ERR_ARG, "state_covariance_0 is not positive definite");
  sp->LT = pb.LT; sp->LW = sb.LW; sp->LB = sb.LB;
  sp->h_cov = cov; sp->h_w_raw = w; sp->h_nsd = nsd; sp->h_rw_scale = d->random_walk_scale; sp->h_T_scale = d->mu_b_T_scale;
  const std::vector<double> &Lw_ext = sb.Lw_ext, &LB_t = sb.LB_t, &LBr = sb.LBr;

  // polls merged and sorted by day (then state); national polls carry the pseudo-state S
  struct Poll { int s, t, p, m, pop, qidx; double y, n, unadj, sig; };
  std::vector<Poll> polls;
  for (int i = 0; i < Ns; i++)
    polls.push_back({d->state[i] - 1, d->day_state[i] - 1, d->poll_state[i] - 1, full ? d->poll_mode_state[i] - 1 : 0,
                     full ? d->poll_pop_state[i] - 1 : 0, L.o_ns + i, (double)d->n_democrat_state[i], (double)d->n_two_share_state[i],
                     full ? d->unadjusted_state[i] : 0.0, poll_sigma(sc, false)});
  for (int j = 0; j < Nn; j++)
    polls.push_back({S, d->day_national[j] - 1, d->poll_national[j] - 1, full ? d->poll_mode_national[j] - 1 : 0,
                     full ? d->poll_pop_national[j] - 1 : 0, L.o_nn + j, (double)d->n_democrat_national[j],
                     (double)d->n_two_share_national[j], full ? d->unadjusted_national[j] : 0.0, poll_sigma(sc, true)});
  std::stable_sort(polls.begin(), polls.end(), [](const Poll &a, const Poll &b) { return a.t != b.t ? a.t < b.t : a.s < b.s; });
  const int Np = (int)polls.size();
  std::vector<int> ps(Np), pt(Np), pp(Np), pm(Np), ppop(Np), pq(Np), day_ptr(T + 1, 0);
  std::vector<double> py(Np), pn(Np), pu(Np), psig(Np);
  for (int i = 0; i < Np; i++) {
    ps[i] = polls[i].s; pt[i] = polls[i].t; pp[i] = polls[i].p; pm[i] = polls[i].m; ppop[i] = polls[i].pop; pq[i] = polls[i].qidx;
    py[i] = polls[i].y; pn[i] = polls[i].n; pu[i] = polls[i].unadj; psig[i] = polls[i].sig;
    day_ptr[polls[i].t + 1]++;
  }
  for (int t = 0; t < T; t++) day_ptr[t + 1] += day_ptr[t];

  // per-day gathers: days balanced over the 8 waves (PT_NW; longest-processing-time first); each wave gets
  // the polls of its days as one contiguous entry list (index, day, state)
  std::vector<int> order, load(PT_NW, 0), npolls_w(PT_NW, 0);
  for (int t = 0; t < T; t++) if (day_ptr[t + 1] > day_ptr[t]) order.push_back(t);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return day_ptr[a + 1] - day_ptr[a] > day_ptr[b + 1] - day_ptr[b]; });
  std::vector<std::vector<int>> wt(PT_NW);
  for (int t : order) {
    int wmin = -1;   // least-loaded wave with a free day slot (64) and room for the polls (256 packed states)
    const int nt = day_ptr[t + 1] - day_ptr[t];
    for (int wv = 0; wv < PT_NW; wv++)
      if (wt[wv].size() < 64 && npolls_w[wv] + nt <= 256 && (wmin < 0 || load[wv] < load[wmin])) wmin = wv;
    if (wmin < 0) { k1_fail("poll schedule of one workgroup per chain does not fit: more than %d polls or %d polled days", 256 * PT_NW, 64 * PT_NW); break; }
    npolls_w[wmin] += nt;
    wt[wmin].push_back(t);
    load[wmin] += day_ptr[t + 1] - day_ptr[t] + 2;
  }
  std::vector<int> wd_t(PT_NW * 64, 0), wd_a(PT_NW * 64, 0), wd_b(PT_NW * 64, 0), wpk(PT_NW * 64, 0), daymask(PT_NW, 0);
  for (int wv = 0; wv < PT_NW; wv++) {
    int e = 0;
    for (size_t j = 0; j < wt[wv].size(); j++) {
      const int t = wt[wv][j];
      wd_t[wv * 64 + j] = t; wd_a[wv * 64 + j] = day_ptr[t]; wd_b[wv * 64 + j] = day_ptr[t + 1];
      for (int i = day_ptr[t]; i < day_ptr[t + 1]; i++, e++) if (e < 256) wpk[wv * 64 + e / 4] |= ps[i] << (8 * (e % 4));
    }
  }
  for (int t = 0; t < T && t < PT_NW * PT_CH; t++) if (day_ptr[t + 1] > day_ptr[t]) daymask[t / PT_CH] |= (int)(1u << (t % PT_CH));

  // two-level segment sums: level-1 tasks of <= PT_SUBLEN polls (padded with the zero slot Npoll),
  // level-2 one thread per segment
  std::vector<int> sub16, seg_ptr{0}, seg_kind, seg_index;
  std::vector<int> &seg_src = sp->h_seg_src;   // the scale of every segment (seg_scales)
  std::vector<double> sub_wt16;
  int nsub = 0;
  auto add_group = [&](int nseg, int kind, int index0, int scale, bool weighted, auto key) {
    std::vector<std::vector<int>> lists(nseg);
    for (int i = 0; i < Np; i++) { const int k = key(i); if (k >= 0) lists[k].push_back(i); }
    for (int sgi = 0; sgi < nseg; sgi++) {
      const auto &l = lists[sgi];
      for (size_t a = 0; a < l.size(); a += PT_SUBLEN) {
        for (size_t j = a; j < a + PT_SUBLEN; j++) {
          sub16.push_back(j < l.size() ? l[j] : Np);
          if (weighted) sub_wt16.push_back(j < l.size() ? pu[l[j]] : 0.0);
        }
        nsub++;
      }
      seg_ptr.push_back(nsub);
      seg_kind.push_back(kind); seg_index.push_back(index0 + sgi); seg_src.push_back(scale);
    }
  };
  add_group(d->P, 0, L.o_c, SC_C, false, [&](int i) { return pp[i]; });
  if (full) {
    add_group(d->M, 0, L.o_m, SC_M, false, [&](int i) { return pm[i]; });
    add_group(d->Pop, 0, L.o_pop, SC_POP, false, [&](int i) { return ppop[i]; });
  }
  add_group(S + 1, 1, 0, -1, false, [&](int i) { return ps[i]; });
  M.sub_weighted_begin = nsub;
  if (full) add_group(T, 2, 0, -1, true, [&](int i) { return pt[i]; });
  const std::vector<double> seg_scale = seg_scales(seg_src, sc);
  M.nsub = nsub;
  M.nseg = (int)seg_kind.size();
  seg_ptr.push_back(nsub); // so that seg_ptr[seg + 1] is loadable for every seg

  // LDS layout (doubles)
  int o = 0;
  auto take = [&](int n) { const int a = o; o += (n + 1) & ~1; return a; };
  M.l_C = take(std::max(S * M.TP, 2 * PT_NW * M.SE));
  M.l_Lw = take(M.SE * M.SP);
  M.l_X = take(std::max(2 * PT_NW * M.SE, Np + 2));
  M.l_Y = take(std::max(PT_NW * M.SE, M.nsub));
  M.l_zT = take(S + 1); M.l_zb = take(S + 1); M.l_mid = take(M.nmid + 1);
  M.l_bT = take(M.SE); M.l_pb = take(M.SE); M.l_e = take(T); M.l_gs = take(M.SE); M.l_ge = take(T);
  M.l_scal = take(SC_N); M.l_red = take(PT_NW * PT_NRED); M.l_st = take((Np + 8 + 7) / 8);
#ifdef POTUS_PROF
  M.l_prof = take(PT_NPROF);
#else
  M.l_prof = 0;
#endif
  M.lds_doubles = o;
  sp->lds_bytes = (size_t)o * 8 + sizeof(TS) + 16;
  if (sp->lds_bytes > 160 * 1024) k1_fail("one workgroup per chain needs %zu bytes of LDS (> 160 KiB): T=%d, polls=%d", sp->lds_bytes, T, Np);

  int rc;
  // pack: mat = Lw_ext | LT_t | LB_t | LT | LB | prior | w
  std::vector<double> mat(Lw_ext);
  auto app = [&](const std::vector<double> &v) { const int off = (int)mat.size(); mat.insert(mat.end(), v.begin(), v.end()); return off; };
  M.m_LTt = app(pb.LT_t); M.m_LBt = app(LB_t); M.m_LT = app(pb.LTr); M.m_LB = app(LBr);
  M.m_prior = app(pb.prior); M.m_w = app(w);
  M.m_priorx = app(pb.px);
  sp->h_mat = mat;
  M.Npad = (Np + 15) & ~15;
  std::vector<int> pi((size_t)6 * M.Npad, 0);
  std::vector<double> pdv((size_t)4 * M.Npad, 0.0);
  for (int i = 0; i < Np; i++) {
    pi[i] = ps[i]; pi[M.Npad + i] = pt[i]; pi[2 * M.Npad + i] = pp[i]; pi[3 * M.Npad + i] = pm[i]; pi[4 * M.Npad + i] = ppop[i];
    pi[5 * M.Npad + i] = pq[i];
    pdv[i] = py[i]; pdv[M.Npad + i] = pn[i]; pdv[2 * M.Npad + i] = pu[i]; pdv[3 * M.Npad + i] = psig[i];
  }
  std::vector<int> sched(wd_t);
  auto appi = [&](const std::vector<int> &v) {
    while (sched.size() % 4) sched.push_back(0);   // 16-byte aligned blocks (sub16 is read with 128-bit loads)
    const int off = (int)sched.size();
    sched.insert(sched.end(), v.begin(), v.end());
    return off;
  };
  M.c_wda = appi(wd_a); M.c_wdb = appi(wd_b); M.c_wpk = appi(wpk); M.c_mask = appi(daymask);
  M.c_sub16 = appi(sub16); M.c_segptr = appi(seg_ptr); M.c_segkind = appi(seg_kind); M.c_segidx = appi(seg_index);
  for (int k = 0; k < 8; k++) sched.push_back(0);
  if (sub_wt16.empty()) sub_wt16.assign(2, 0.0);
  if ((rc = upload(sp, mat, &M.mat)) || (rc = upload(sp, pi, &M.pi)) || (rc = upload(sp, pdv, &M.pd)) ||
      (rc = upload(sp, sched, &M.sched)) || (rc = upload(sp, seg_scale, &M.seg_scale)) || (rc = upload(sp, sub_wt16, &M.sub_wt16)))
    return rc;
  sp->h_w = w;   // weighted.mean() normalises: keep them summing to one
  { double sw = 0; for (double x : sp->h_w) sw += x; for (double &x : sp->h_w) x /= sw; }
  sp->h_ps = ps; sp->h_pt = pt; sp->h_pp = pp; sp->h_pm = pm; sp->h_ppop = ppop; sp->h_pq = pq; sp->h_dayptr = day_ptr; sp->h_pu = pu;
  void *pdm = nullptr;
  HIP_TRY(hipMalloc(&pdm, sizeof(DevModel)));
  sp->allocs.push_back(pdm);
  HIP_TRY(hipMemcpy(pdm, &M, sizeof(DevModel), hipMemcpyHostToDevice));
  sp->dM = (DevModel *)pdm;
  return 0;
}

int set_lds_attr(Sampler *sp) {
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_logprob_grad), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp->lds_bytes));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_init), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp->lds_bytes));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_run), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp->lds_bytes));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_run_twin), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp->lds_bytes));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_init_ds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp->lds_bytes));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_run_ds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp->lds_bytes));
  return 0;
}

// Cluster mode: split the days over K members (contiguous ranges balanced by days + polls), give every
// parameter one owner, lay the owners' elements out contiguously and build each member's schedule.
int build_cluster(Sampler *sp, const potus_data *d, int K) {
  const DevModel &M = sp->M;
  const Layout &L = sp->L;
  const bool full = M.full;
  const int S = M.S, T = M.T, Np = M.Npoll, P = M.P;
  if (K < 2 || K > CL_MAXK) return fail(POTUS_ERR_ARG, "cus_per_chain must be 1 or in [2,%d]", CL_MAXK);
  ClModel &C = sp->CL;
  C.K = K;
  C.NR = 2 * S + P + (full ? M.M + M.Pop + 2 : 0);
  C.NREP = 2 * S + M.nmid;
  // days per wave: 4 (at most 32 days per member) when that leaves room to balance the members by polls, else 8
  // (up to 26 days per member on average: measured with 12 chains on two clusters of 10, profiles/r02_cl_cluster_sizes.txt)
  const int dw4_max = getenv("POTUS_CL_DW4_MAXAVG") ? atoi(getenv("POTUS_CL_DW4_MAXAVG")) : CL_DW4_MAXAVG;   // development: sweeps
  const int DW = (T + K - 1) / K <= dw4_max ? 4 : 8;
  // (development: POTUS_CL_MAXDAYS caps the days of a member below what its waves hold -- partition sweeps, profiles/r05_cl_partition.txt)
  const int maxdays = getenv("POTUS_CL_MAXDAYS") ? std::max(1, std::min(PT_NW * DW, atoi(getenv("POTUS_CL_MAXDAYS")))) : PT_NW * DW;
  sp->cl_dw = DW;   // (12 once the adjoint goes to the matrix cores, below)
  C.XW = (std::max(XP_P + C.NR, XQ0 + C.NREP) + 7) & ~7;
  if (P > 65535 || M.M > 255 || M.Pop > 255) return fail(POTUS_ERR_UNSUPPORTED, "cluster mode packs pollster/mode/population indices in 16/8/8 bits");
  if (C.NREP > 2 * PT_THREADS) return fail(POTUS_ERR_UNSUPPORTED, "cluster mode: %d small parameters (> %d)", C.NREP, 2 * PT_THREADS);
  if ((C.NR + K - 1) / K > PT_THREADS - 128 - 3) return fail(POTUS_ERR_UNSUPPORTED, "cluster mode: too many pollsters for K = %d", K);
  const std::vector<int> &dp = sp->h_dayptr;

  // contiguous day ranges: minimise the largest cost (a day = S elements of vector work, a poll = a
  // 51-term dot + a gather) with at most CL_MAXDAYS days each
  // (weights measured on the 2016 posterior, scripts/micro/r02_sweep.sh: a poll costs a member about as much as a day --
  //  dot, binomial term, adjoint gather -- 20.1 us per leapfrog against 21.1 with the earlier 51 : 10)
  const int cw_day = getenv("POTUS_CW_DAY") ? atoi(getenv("POTUS_CW_DAY")) : 30, cw_poll = getenv("POTUS_CW_POLL") ? atoi(getenv("POTUS_CW_POLL")) : 45;   // (round 4, without the 51 x 51 products: 30 : 45 / 30 : 60 / 20 : 30 13.9 us against 14.1 with 30 : 30)
  auto groups_for = [&](int B, std::vector<int> *cut) {
    int g = 0, t = 0;
    if (cut) cut->assign(1, 0);
    while (t < T) {
      int nd = 0, cost = 0;
      while (t < T && nd < maxdays) {
        const int c1 = cw_day + cw_poll * (dp[t + 1] - dp[t]);
        if (nd > 0 && cost + c1 > B) break;
        cost += c1; nd++; t++;
      }
      g++;
      if (cut) cut->push_back(t);
    }
    return g;
  };
  int lo = 1, hi = cw_day * T + cw_poll * Np;
  while (lo < hi) { const int mid = (lo + hi) / 2; if (groups_for(mid, nullptr) <= K) hi = mid; else lo = mid + 1; }
  std::vector<int> cut;
  if (groups_for(lo, &cut) > K) return fail(POTUS_ERR_UNSUPPORTED, "T = %d days do not fit %d members of at most %d days", T, K, maxdays);
  while ((int)cut.size() < K + 1) cut.push_back(T);   // members without days still own a share of the small vectors

  // the adjoint product on the fp64 matrix cores (potus_cluster.hpp, cl_pass_partial): G[pseudo-state][local day], row stride
  // = 16 mod 32 doubles (the four rows a wave reads per MFMA step fall on disjoint LDS banks)
  // -- for poll-dense posteriors (more than 8 polls per day: the dense product then beats the walk over the polls, measured in
  // profiles/r03_cl_mfma_adjoint.txt; the reference's own posteriors have 4-6 and keep the walk); POTUS_CL_MFMA = 0 / 1 overrides
  // The choice by poll density is a matter of speed only: where a member is beyond what the adjoint scatter addresses (1023 polls, 63 polls
  // of one state on one day, CL_CELLS_PER_THREAD x PT_THREADS polled cells) the walk runs the same data.  Forced on (POTUS_CL_MFMA = 1), such
  // a member is refused below.
  auto scatter_holds_every_member = [&]() {
    for (int m = 0; m < K; m++) {
      const int p0 = dp[cut[m]], np = dp[cut[m + 1]] - p0;
      if (np >= 1024) return false;
      int ncell = 0;
      for (int il = 0; il < np;) {
        int j = il + 1;
        while (j < np && sp->h_pt[p0 + j] == sp->h_pt[p0 + il] && sp->h_ps[p0 + j] == sp->h_ps[p0 + il]) j++;
        if (j - il > 63 || ++ncell > CL_CELLS_PER_THREAD * PT_THREADS) return false;
        il = j;
      }
    }
    return true;
  };
  const bool mfma = DW == 4 && (getenv("POTUS_CL_MFMA") ? atoi(getenv("POTUS_CL_MFMA")) != 0 : Np > 8 * T && scatter_holds_every_member());
  const int GS = 48, GROWS = 4 * ((M.SE + 3) / 4);
  if (mfma) sp->cl_dw = 12;
  std::vector<int> part((size_t)K * CP_N, 0), sched, perm;   // perm: internal index -> Stan index, -1 for padding
  std::vector<double> wts;
  int e = 0, npmax = 0, nsubmax = 0;
  for (int m = 0; m < K; m++) {
    int *pt_ = &part[(size_t)m * CP_N];
    const int d0 = cut[m], nd = cut[m + 1] - cut[m], p0 = dp[d0], np = dp[d0 + nd] - p0;
    const int r0 = (int)((long long)C.NR * m / K), nr = (int)((long long)C.NR * (m + 1) / K) - r0;
    pt_[CP_D0] = d0; pt_[CP_ND] = nd; pt_[CP_P0] = p0; pt_[CP_NP] = np; pt_[CP_E0] = e; pt_[CP_R0] = r0; pt_[CP_NR] = nr;
    if (getenv("POTUS_CL_VERBOSE")) fprintf(stderr, "cluster member %2d: days [%3d, %3d) = %2d, polls %4d, small-vector slots %3d\n", m, d0, d0 + nd, nd, np, nr);
    npmax = std::max(npmax, np);
    // internal order: days of raw_mu_b | noise of own polls | pad | own days of raw_e_bias | share of the small
    // vectors | pad.  The two blocks start on 128-byte lines: no cache line has two writers (members sit on
    // different compute units, possibly different XCDs) or mixes plain stores (first block: read only by the owner)
    // with write-through stores (second block: read by every member).
    auto pad16 = [&]() { while (perm.size() % 16) perm.push_back(-1); };
    for (int tl = 0; tl < nd; tl++) for (int k = 0; k < S; k++) perm.push_back(L.o_Z + k + S * (d0 + tl));
    for (int il = 0; il < np; il++) perm.push_back(sp->h_pq[p0 + il]);
    pad16();
    pt_[CP_E_SH] = (int)perm.size();
    if (full) for (int tl = 0; tl < nd; tl++) perm.push_back(L.o_ze + d0 + tl);
    for (int j = 0; j < nr; j++) { const int r = r0 + j; perm.push_back(r < S ? L.o_zT + r : r < 2 * S ? L.o_zb + (r - S) : L.o_c + (r - 2 * S)); }
    pad16();
    e = (int)perm.size();
    pt_[CP_NE] = e - pt_[CP_E0];

    // the member's days are dealt to the waves as contiguous ranges of at most CL_DW days, balanced by
    // polls (a wave gathers the adjoint of the days it owns): smallest feasible bound on polls per wave
    std::vector<int> wd0(PT_NW, nd), wnd(PT_NW, 0);
    {
      auto assign = [&](int B, bool commit) {
        int tl = 0;
        for (int wv = 0; wv < PT_NW; wv++) {
          int n = 0, polls = 0;
          const int start = tl;
          while (tl < nd && n < DW) {
            const int c1 = dp[d0 + tl + 1] - dp[d0 + tl];
            // leave enough room in the remaining waves for the remaining days
            if (n > 0 && polls + c1 > B && (nd - tl) <= (PT_NW - 1 - wv) * DW) break;
            polls += c1; n++; tl++;
          }
          if (commit) { wd0[wv] = start; wnd[wv] = n; }
        }
        return tl == nd;
      };
      int lo2 = 0, hi2 = np + 1;
      auto maxpolls = [&](int B) {   // feasibility: all days placed and no wave above the bound unless forced by one day
        int tl = 0, worst = 0;
        for (int wv = 0; wv < PT_NW; wv++) {
          int n = 0, polls = 0;
          while (tl < nd && n < DW) {
            const int c1 = dp[d0 + tl + 1] - dp[d0 + tl];
            if (n > 0 && polls + c1 > B && (nd - tl) <= (PT_NW - 1 - wv) * DW) break;
            polls += c1; n++; tl++;
          }
          worst = std::max(worst, polls);
        }
        return tl == nd ? worst : 1 << 30;
      };
      int best = hi2, bestB = hi2;
      for (int B = lo2; B <= hi2; B++) { const int w_ = maxpolls(B); if (w_ < best) { best = w_; bestB = B; } }
      if (!assign(bestB, true)) return fail(POTUS_ERR_STATE, "internal: member %d: %d days do not fit %d waves", m, nd, PT_NW);
    }
    // adjoint gather: equal chunks of the member's polls per wave; program word per poll; what the owner of
    // each day reads back (last polled day <= it, chunk of that day's last poll)
    std::vector<int> ca(PT_NW), cb(PT_NW), tab(np), s2info(PT_THREADS, 0);
    for (int wv = 0; wv < PT_NW; wv++) { ca[wv] = (int)((long long)np * std::min(wv, CL_NCHUNK) / CL_NCHUNK); cb[wv] = (int)((long long)np * std::min(wv + 1, CL_NCHUNK) / CL_NCHUNK); }
    auto chunk_of = [&](int il) { int c = 0; while (c < CL_NCHUNK - 1 && il >= cb[c]) c++; return c; };
    for (int il = 0; il < np; il++) {
      const int g = p0 + il, tl = sp->h_pt[g] - d0;
      const bool dayend = il == np - 1 || sp->h_pt[g + 1] != sp->h_pt[g];
      tab[il] = sp->h_ps[g] | (tl << 8) | ((dayend ? 1 : 0) << 16);
    }
    for (int wv = 0; wv < PT_NW; wv++)
      for (int j = 0; j < wnd[wv]; j++) {
        int tl = wd0[wv] + j;
        while (tl >= 0 && dp[d0 + tl + 1] == dp[d0 + tl]) tl--;   // last day with polls at or before this one
        s2info[wv * 64 + j] = tl < 0 ? 0 : ((tl + 1) | (chunk_of(dp[d0 + tl + 1] - 1 - p0) << 8));
      }
    // adjoint on the matrix cores (4-days-per-wave build): the (state, day) cells of the member's polls -- runs of its
    // day-then-state sorted polls -- one per thread: first poll | polls << 10 | offset in G << 16
    std::vector<int> cellw((size_t)CL_CELLS_PER_THREAD * PT_THREADS, 0);
    int ncell = 0;
    if (mfma) {
      const int dump = GROWS * GS;
      if (np >= 1024) return fail(POTUS_ERR_UNSUPPORTED, "cluster mode: member %d has %d polls (the adjoint scatter addresses 1023)", m, np);
      for (auto &cw : cellw) cw = np | (1 << 10) | (dump << 16);
      for (int il = 0; il < np;) {
        int j = il + 1;
        while (j < np && sp->h_pt[p0 + j] == sp->h_pt[p0 + il] && sp->h_ps[p0 + j] == sp->h_ps[p0 + il]) j++;
        {
          if (j - il > 63) return fail(POTUS_ERR_UNSUPPORTED, "cluster mode: %d polls of one state on one day (the adjoint scatter takes 63)", j - il);
          if (ncell >= CL_CELLS_PER_THREAD * PT_THREADS) return fail(POTUS_ERR_UNSUPPORTED, "cluster mode: member %d has more than %d polled (state, day) cells", m, CL_CELLS_PER_THREAD * PT_THREADS);
          cellw[ncell++] = il | ((j - il) << 10) | ((sp->h_ps[p0 + il] * GS + (sp->h_pt[p0 + il] - d0)) << 16);
        }
        il = j;
      }
    }
    pt_[CP_NCELL] = ncell;
    std::vector<int> wdays(wd0);
    wdays.insert(wdays.end(), wnd.begin(), wnd.end());
    wdays.insert(wdays.end(), ca.begin(), ca.end());
    wdays.insert(wdays.end(), cb.begin(), cb.end());

    // two-level segment sums over the member's polls (local poll indices, padded with the zero slot np)
    std::vector<int> sub16, seg_ptr{0}, seg_kind, seg_index;
    std::vector<double> sub_wt;
    int nsub = 0;
    auto add_group = [&](int nseg, int kind, int index0, bool weighted, auto key) {
      std::vector<std::vector<int>> lists(nseg);
      for (int il = 0; il < np; il++) lists[key(p0 + il)].push_back(il);
      for (int sgi = 0; sgi < nseg; sgi++) {
        const auto &l = lists[sgi];
        if (l.empty()) continue;
        for (size_t a = 0; a < l.size(); a += PT_SUBLEN) {
          for (size_t j = a; j < a + PT_SUBLEN; j++) {
            sub16.push_back(j < l.size() ? l[j] : np);
            if (weighted) sub_wt.push_back(j < l.size() ? sp->h_pu[p0 + l[j]] : 0.0);
          }
          nsub++;
        }
        seg_ptr.push_back(nsub);
        seg_kind.push_back(kind); seg_index.push_back(index0 + sgi);
      }
    };
    add_group(P, 0, 2 * S, false, [&](int i) { return sp->h_pp[i]; });
    if (full) {
      add_group(M.M, 0, 2 * S + P, false, [&](int i) { return sp->h_pm[i]; });
      add_group(M.Pop, 0, 2 * S + P + M.M, false, [&](int i) { return sp->h_ppop[i]; });
    }
    const int wb = nsub;   // tasks from here on sum unadjusted * residual
    if (full) add_group(nd, 2, 0, false, [&](int i) { return sp->h_pt[i] - d0; });
    seg_ptr.push_back(nsub);
    if ((int)seg_kind.size() > PT_THREADS) return fail(POTUS_ERR_UNSUPPORTED, "cluster mode: member %d has %zu segments (> %d)", m, seg_kind.size(), PT_THREADS);
    pt_[CP_NSUB] = nsub; pt_[CP_NSEG] = (int)seg_kind.size(); pt_[CP_WB] = wb;
    // phase D takes the two counts and the wave's chunk bounds from spare lanes of the per-thread statics (lanes 0 .. CL_DW - 1 describe the wave's days)
    static_assert(CL_L1_LANE >= 8 && CL_L1_LANE + 2 < 64, "lanes 0-7 of s2info are the wave's days");
    if (nsub > 0xffff) return fail(POTUS_ERR_UNSUPPORTED, "cluster mode: member %d has %d level-1 tasks (> 65535)", m, nsub);
    for (int wv = 0; wv < PT_NW; wv++) {
      int *sl = &s2info[wv * 64 + CL_L1_LANE];
      sl[0] = nsub | (wb << 16); sl[1] = ca[wv]; sl[2] = cb[wv];
    }
    nsubmax = std::max(nsubmax, nsub);
    auto appi = [&](const std::vector<int> &v) {
      while (sched.size() % 4) sched.push_back(0);
      const int off = (int)sched.size();
      sched.insert(sched.end(), v.begin(), v.end());
      return off;
    };
    pt_[CP_O_WD] = appi(s2info); appi(wdays);
    pt_[CP_O_MASK] = appi(tab); pt_[CP_O_SUB] = appi(sub16); pt_[CP_O_SEGPTR] = appi(seg_ptr);
    pt_[CP_O_SEGKIND] = appi(seg_kind); pt_[CP_O_SEGIDX] = appi(seg_index);
    pt_[CP_O_CELL] = appi(cellw);
    while (wts.size() % 2) wts.push_back(0.0);
    pt_[CP_O_WT] = (int)wts.size();
    wts.insert(wts.end(), sub_wt.begin(), sub_wt.end());
  }
  const int Dint = e;   // internal length of a vector (parameters + padding)
  C.Dint = Dint;
  for (int k = 0; k < 16; k++) { sched.push_back(0); wts.push_back(0.0); }
  C.npmax = npmax; C.nsubmax = nsubmax;

  std::vector<int> iperm(L.D, -1);
  for (int i = 0; i < Dint; i++) { if (perm[i] >= L.D) return fail(POTUS_ERR_STATE, "internal: bad permutation"); if (perm[i] >= 0) iperm[perm[i]] = i; }
  for (int i = 0; i < L.D; i++) if (iperm[i] < 0) return fail(POTUS_ERR_STATE, "internal: cluster layout misses parameter %d", i);
  std::vector<int> rep_pos(C.NREP), rep_owner(C.NREP);
  for (int j = 0; j < C.NREP; j++) {
    rep_pos[j] = iperm[j < S ? L.o_zT + j : j < 2 * S ? L.o_zb + (j - S) : L.o_c + (j - 2 * S)];
    int mo = 0;
    while (mo < K - 1 && rep_pos[j] >= part[(size_t)mo * CP_N + CP_E0] + part[(size_t)mo * CP_N + CP_NE]) mo++;   // owner = member whose element range holds it
    rep_owner[j] = mo;
  }
  std::vector<double> rep_scale(C.NR, 1.0);
  for (int i = 0; i < S; i++) { rep_scale[i] = M.aT; rep_scale[S + i] = M.aB; }   // L_T = aT L_W, L_B = aB L_W (DevModel::aT)
  for (int i = 0; i < P; i++) rep_scale[2 * S + i] = d->sigma_c;
  if (full) {
    for (int i = 0; i < M.M; i++) rep_scale[2 * S + P + i] = d->sigma_m;
    for (int i = 0; i < M.Pop; i++) rep_scale[2 * S + P + M.M + i] = d->sigma_pop;
  }
  sp->h_perm = perm;

  int ndmax = 1, nemax = 0;
  for (int m = 0; m < K; m++) { ndmax = std::max(ndmax, part[(size_t)m * CP_N + CP_ND]); nemax = std::max(nemax, part[(size_t)m * CP_N + CP_NE]); }
  C.NDP = cl_ndp(ndmax);   // odd row stride of the member's C[state][local day] block, with a spare column behind the days (the dump column of the walk)
  if (M.SE * M.SP * 8 > 0x10000 || C.NDP * 8 > 0x10000) return fail(POTUS_ERR_UNSUPPORTED, "cluster mode: the gather program holds byte offsets in 16 bits");
  C.GS = GS; C.GROWS = GROWS;
  ClLay lay = cl_layout(S, M.SE, M.SP, C.NDP, npmax, nsubmax, C.NREP, C.NR, T, mfma ? GROWS * GS + CL_G_PAD : 0);
  // The builds with the layout fixed at compile time (tags 16 and 17 = full model / no_mode_adjustment variant, ClFixed): 51 states, members of
  // at most 32 days / 256 polls / 384 level-1 tasks, the walk for the adjoint.  The layout is then the same function of ClFixed's capacities -- the numbers the
  // kernel uses as immediates.
  {
    const bool fits = DW == 4 && !mfma && K <= ClFixed::KMAX && std::max(XP_P + C.NR, XQ0 + C.NREP) <= ClFixed::XW && S == ClFixed::S && M.SE == ClFixed::SE && M.SP == ClFixed::SP && ndmax <= ClFixed::NDP - 1 && npmax <= ClFixed::NPCAP &&
                      nsubmax <= ClFixed::NSUBCAP && C.NREP <= ClFixed::NREPCAP && C.NR <= ClFixed::NRCAP && T <= ClFixed::TCAP && (int)SC_N <= 8 &&
                      nemax <= ClFixed::NECAP;                // the member's resident share of a vector (ClLeapPolicyRes)
    if (fits && !(getenv("POTUS_CL_DYNAMIC") && atoi(getenv("POTUS_CL_DYNAMIC")))) {
      C.NDP = ClFixed::NDP; C.XW = ClFixed::XW;
      lay = ClFixed::L;
      sp->cl_dw = full ? 16 : 17;       // the variant is a constant of the build as well (ClTag::FULL)
    }
  }
  C.l_C = lay.l_C; C.l_G = lay.l_G; C.l_Lw = lay.l_Lw; C.l_prior = lay.l_prior; C.l_pm = lay.l_pm; C.l_py = lay.l_py; C.l_pun = lay.l_pun;
  C.l_sub = lay.l_sub; C.l_tab = lay.l_tab; C.l_ru = lay.l_ru; C.l_wide = lay.l_wide; C.l_wout = lay.l_wout; C.l_X = lay.l_X; C.l_Y = lay.l_Y;
  C.l_r = lay.l_r; C.l_rep = lay.l_rep; C.l_bT = lay.l_bT; C.l_e = lay.l_e; C.l_c1 = lay.l_c1; C.l_c2 = lay.l_c2; C.l_c3 = lay.l_c3; C.l_ge = lay.l_ge;
  C.l_P = lay.l_P; C.l_scal = lay.l_scal; C.l_red = lay.l_red; C.l_st = lay.l_st; C.l_prof = lay.l_prof; C.lds_doubles = lay.total;
  const int o = lay.total;
  sp->cl_lds_bytes = (size_t)o * 8 + sizeof(TS) + 16;
  if (sp->cl_lds_bytes > 160 * 1024 - 64) return fail(POTUS_ERR_UNSUPPORTED, "cluster mode needs %zu bytes of LDS per workgroup", sp->cl_lds_bytes);

  int rc;
  if ((rc = upload(sp, part, &C.part)) || (rc = upload(sp, sched, &C.sched)) || (rc = upload(sp, wts, &C.wt)) ||
      (rc = upload(sp, rep_pos, &C.rep_pos)) || (rc = upload(sp, rep_owner, &C.rep_owner)) || (rc = upload(sp, rep_scale, &C.rep_scale)) || (rc = upload(sp, perm, &C.perm)))
    return rc;
  void *pc = nullptr;
  HIP_TRY(hipMalloc(&pc, sizeof(ClModel)));
  sp->allocs.push_back(pc);
  HIP_TRY(hipMemcpy(pc, &C, sizeof(ClModel), hipMemcpyHostToDevice));
  sp->dCL = (ClModel *)pc;
  for (const void *f : {reinterpret_cast<const void *>(k_cl_logprob_grad<4>), reinterpret_cast<const void *>(k_cl_logprob_grad<8>), reinterpret_cast<const void *>(k_cl_logprob_grad<12>),
                        reinterpret_cast<const void *>(k_cl_logprob_grad<16>), reinterpret_cast<const void *>(k_cl_init<16>),
                        reinterpret_cast<const void *>(k_cl_run<16, false>), reinterpret_cast<const void *>(k_cl_run<16, true>),
                        reinterpret_cast<const void *>(k_cl_logprob_grad<17>), reinterpret_cast<const void *>(k_cl_init<17>),
                        reinterpret_cast<const void *>(k_cl_run<17, false>), reinterpret_cast<const void *>(k_cl_run<17, true>),
                        reinterpret_cast<const void *>(k_cl_init<4>), reinterpret_cast<const void *>(k_cl_init<8>), reinterpret_cast<const void *>(k_cl_init<12>),
                        reinterpret_cast<const void *>(k_cl_run<4, false>), reinterpret_cast<const void *>(k_cl_run<8, false>), reinterpret_cast<const void *>(k_cl_run<12, false>),
                        reinterpret_cast<const void *>(k_cl_run<4, true>), reinterpret_cast<const void *>(k_cl_run<8, true>), reinterpret_cast<const void *>(k_cl_run<12, true>)})
    HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp->cl_lds_bytes));
  sp->K = K;
  return 0;
}

// The builds of the cluster pass (template tag of potus_cluster.hpp): 4 = four days per wave, 8 = eight days per wave, 12 = four
// days per wave with the adjoint product on the fp64 matrix cores (poll-dense posteriors), 16 = four days per wave, 51 states, LDS
// layout fixed at compile time (ClFixed: the reference's posteriors on clusters of 16).
#define CL_DISPATCH(tag, CALL) do { if ((tag) == 16) { CALL(16); } else if ((tag) == 17) { CALL(17); } else if ((tag) == 4) { CALL(4); } else if ((tag) == 12) { CALL(12); } else { CALL(8); } } while (0)

// replica 0 of every chain's scalars
int read_scalars(Sampler *sp, std::vector<ChainScalars> &sc) {
  std::vector<ChainScalars> all((size_t)sp->R.chains * sp->K);
  HIP_TRY(hipMemcpy(all.data(), sp->R.scal, sizeof(ChainScalars) * all.size(), hipMemcpyDeviceToHost));
  sc.resize(sp->R.chains);
  for (int c = 0; c < sp->R.chains; c++) sc[c] = all[(size_t)c * sp->K];
  return 0;
}

// Anything that makes the chains of a handle unusable: a chain whose step-size search ran away (Stan throws there),
// a cluster launch that gave up waiting for a member (watchdog word raised by the device).
int check_chains(Sampler *sp) {
  std::vector<ChainScalars> sc;
  { const int rc_ = read_scalars(sp, sc); if (rc_) return rc_; }
  if (sp->coop()) {
    const size_t per_chain = 4 * (size_t)sp->K * sp->CL.XW + 8;   // 16-byte words: exchange slots + the watchdog line (K = 1: XW = 0)
    for (int b = 0; b < sp->R.chains * sp->sides(); b++) {
      const int c = b % sp->R.chains;
      unsigned wd = 0, wt = 0;
      HIP_TRY(hipMemcpy(&wd, (const char *)sp->R.xbuf + ((size_t)b * per_chain + 4 * (size_t)sp->K * sp->CL.XW) * 16, 4, hipMemcpyDeviceToHost));
      if (sp->twin) HIP_TRY(hipMemcpy(&wt, (const char *)sp->R.twbuf + ((size_t)c * TWB_WORDS + TWB_WD) * 16, 4, hipMemcpyDeviceToHost));
      wd |= wt;
      if (wd) return fail(POTUS_ERR_WATCHDOG, "chain %d: the %d workgroups working for it were not running together (is another process using GPU %d?); "
                                              "the launch was abandoned and this handle is no longer usable", c + 1, sp->K * sp->sides(), sp->device);
    }
  }
  for (int c = 0; c < sp->R.chains; c++) {
    // many data sets: a replicate whose chain found no start or step size is reported by potus_chain_status, the others go on
    if (sp->n_ds && (sc[c].status == POTUS_ERR_INIT || sc[c].status == POTUS_ERR_STEPSIZE)) continue;
    if (sc[c].status == POTUS_ERR_INIT) return fail(POTUS_ERR_INIT, "chain %d: no finite initial log density/gradient after 100 attempts", c + 1);
    if (sc[c].status == POTUS_ERR_STEPSIZE) return fail(POTUS_ERR_STEPSIZE, "chain %d: the step-size search left (0, 1e7) -- the posterior is improper or the gradient is wrong (Stan throws here)", c + 1);
    if (sc[c].status == POTUS_ERR_WATCHDOG) return fail(POTUS_ERR_WATCHDOG, "chain %d: cluster launch abandoned (watchdog)", c + 1);
    if (sc[c].status != 0) return fail(POTUS_ERR_STATE, "chain %d: status %d", c + 1, sc[c].status);
  }
  return 0;
}


// ======================================================================== dense metric: host side (potus_dense.hpp)
// windowed_adaptation's schedule, shared by every chain: the longest window = capacity of the draw buffer
int dense_window_capacity(int nw, int ib, int tb, int bw) {
  if (nw < 20) return 1;
  int cap = 1, n = 0, counter = 0, next = ib + bw - 1, size = bw;
  for (int it = 0; it < nw; it++) {
    const bool in = counter >= ib && counter < nw - tb && counter != nw, end = counter == next && counter != nw;
    if (in) n++;
    cap = std::max(cap, n);
    if (end) {
      const int last = nw - tb - 1;
      if (next != last) { size *= 2; next = counter + size; if (next != last && next + 2 * size >= nw - tb) next = last; }
      n = 0;
    }
    counter++;
  }
  return cap;
}

// Blocked Cholesky factorisation in place on the lower triangles of the chains' matrices, in panels of DN_PANEL block columns:
// inside a panel potrf / trsm / narrow update per block column, behind it one wide update (k_dn_syrk_wide).
void dense_cholesky_launch(hipStream_t st, const DnParams &P, int chains) {
  const int nb = (P.D + DN_NB - 1) / DN_NB;
  for (int pb = 0; pb < nb; pb += DN_PANEL) {
    const int nk = std::min(DN_PANEL, nb - pb), last = pb + nk - 1;
    for (int kb = pb; kb <= last; kb++) {
      hipLaunchKernelGGL(k_dn_potrf, dim3(chains), dim3(256), 0, st, P, kb);
      const int rem = nb - kb - 1;
      if (rem > 0) {
        hipLaunchKernelGGL(k_dn_trsm, dim3(rem, chains), dim3(256), 0, st, P, kb);
        if (last > kb) hipLaunchKernelGGL(k_dn_syrk, dim3(rem, last - kb, chains), dim3(256), 0, st, P, kb, last);
      }
    }
    const int behind = P.D - (pb + nk) * DN_NB;
    if (behind > 0) {
      const int nt = (behind + DN_WT - 1) / DN_WT;
      hipLaunchKernelGGL(k_dn_syrk_wide, dim3(nt, nt, chains), dim3(256), 0, st, P, pb, nk);
    }
  }
}

// Shape of one launch of the symmetric product: rows a workgroup takes at a time (256 for large matrices: fewer tiles per
// byte) and, by the number of chains that take part, workgroups per pair of row blocks (enough to keep 256 compute units
// busy when the active chains are few; the results do not depend on it).
void dense_launch_shape(DnParams &P, int active) {
  active = std::max(active, 1);
  P.rb = P.D >= 32 * DN_RB_MAX ? DN_RB_MAX : P.D >= 32 * DN_RB_BIG ? DN_RB_BIG : DN_RB;   // by the size of the matrix alone: a chain's numbers must not depend on its companions
  P.ntile = (P.D + DN_CT - 1) / DN_CT;
  const int pairs = ((P.D + P.rb - 1) / P.rb + 1) / 2;
  // One workgroup per compute unit at a time (DN_SYMV_LDS(2) = 90 KB of LDS with DN_RB_MAX = 512): the launch runs in waves of 256 workgroups.  Few, large workgroups are
  // best (measured: profiles/r02_dense_active_sweep.txt), so: the smallest split whose last wave is at least 90 % full.
  const int base = active * pairs;
  P.split = 1;
  if (const char *e = getenv("POTUS_DENSE_SPLIT")) { P.split = std::max(1, std::min(DN_SPLIT_MAX, atoi(e))); return; }   // development: sweeps of scripts/micro/dense_probe.py
  double best = 0.0;
  for (int s = 1; s <= DN_SPLIT_MAX; s++) {
    const int w = base * s;
    const double fill = (double)w / (((w + 255) / 256) * 256);
    if (fill > best + 1e-9) { best = fill; P.split = s; }
    if (fill >= 0.9) { P.split = s; break; }
  }
}

// bytes one pass of the symmetric product loads per chain: the tiles right of (and on) each row block's diagonal
long long dense_pass_bytes(int D, int LD, int rb) {
  long long n = 0;
  const int tile_end = std::min(LD, ((D + DN_CT - 1) / DN_CT) * DN_CT);
  for (int r0 = 0; r0 < D; r0 += rb) n += (long long)std::min(rb, D - r0) * (tile_end - (r0 / DN_CT) * DN_CT);
  return n * 8;
}

int dense_alloc(Sampler *sp) {
  DnParams &P = sp->dn;
  const int D = sp->L.D, chains = sp->R.chains;
  P.chains = chains; P.D = D; P.LD = (D + 7) & ~7; P.npart = (D + DN_FIN / 4 - 1) / (DN_FIN / 4); P.nblk = (D + DN_RB - 1) / DN_RB; P.sc_stride = sp->K; P.identity = 1;
  P.win_cap = dense_window_capacity(sp->R.num_warmup, sp->R.init_buffer, sp->R.term_buffer, sp->R.window);
  P.f32 = sp->opts.metric_storage == POTUS_STORAGE_F32 ? 1 : 0;
  P.pooled = sp->opts.pooled_metric ? 1 : 0;
  dense_launch_shape(P, chains);
  // pooled metric: ONE full symmetric matrix + ONE factor for the handle, and the partial products of the row splits.  The number of splits is a
  // function of D alone (the order in which a product is summed must not depend on who else is active): the largest one (up to DNP_SPLIT_MAX) that keeps the launch
  // within two workgroups of 256 columns per compute unit -- all resident at once, no tail --, in whole batches of DNP_KB rows.
  P.pool_split = 1; P.pool_rows = D;
  if (P.pooled) {
    const int panels = (D + DNP_COLS_OF(P.f32) - 1) / DNP_COLS_OF(P.f32);
    int s = std::max(1, std::min(DNP_SPLIT_MAX, (2 * 256) / panels));   // at most two workgroups per compute unit, all resident at once (measured: profiles/r06_dense_pooled.txt)
    if (const char *e = getenv("POTUS_POOL_SPLIT")) s = std::max(1, std::min(DNP_SPLIT_MAX, atoi(e)));   // development: sweeps
    P.pool_rows = (((D + s - 1) / s + DNP_KB - 1) / DNP_KB) * DNP_KB;
    P.pool_split = (D + P.pool_rows - 1) / P.pool_rows;
  }
  const int mchains = P.pooled ? 1 : chains;
  const size_t mat = (size_t)mchains * D * P.LD * 8 * (P.pooled ? 2 : 1) + (P.pooled ? (size_t)P.pool_split * DNP_RMAX * P.LD * 8 : 0) + (P.pooled && P.f32 ? (size_t)D * P.LD * 4 : 0), vec = (size_t)chains * DV_COUNT * P.LD * 8, win = (size_t)chains * P.win_cap * P.LD * 8;
  const size_t tp = (size_t)chains * (P.nblk + P.ntile) * 3 * P.LD * 8;   // column sums per row block + row sums per column tile
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (mat + vec + win + tp + (64u << 20) > free_b)
    return fail(POTUS_ERR_UNSUPPORTED, "dense metric: %d chains x (D^2 + %d window draws + %d vectors + %d partial vectors) x 8 bytes = %.1f GB, %.1f GB free on GPU %d "
                                       "(D = %d: %.2f GB per matrix; potus_opts.pooled_metric keeps one matrix and one factor for all chains of the handle)", chains, P.win_cap, DV_COUNT, 3 * P.nblk, (mat + vec + win + tp) / 1e9, free_b / 1e9, sp->device, D, (double)D * P.LD * 8 / 1e9);
  auto get = [&](void **q, size_t bytes) {
    if (hipMalloc(q, std::max<size_t>(bytes, 8)) != hipSuccess) return fail(POTUS_ERR_DEVICE, "hipMalloc(%zu) for the dense metric failed", bytes);
    sp->allocs.push_back(*q);
    // (on the sampler's own stream: it is a non-blocking stream, which a memset on the null stream would not order with)
    return hipMemsetAsync(*q, 0, std::max<size_t>(bytes, 8), sp->stream) == hipSuccess ? 0 : fail(POTUS_ERR_DEVICE, "hipMemset failed");
  };
  int rc;
  if ((rc = get((void **)&P.state, vec)) || (rc = get((void **)&P.A, (size_t)mchains * D * P.LD * 8)) || (rc = get((void **)&P.dg, (size_t)mchains * P.LD * 8)) || (rc = get((void **)&P.win, win)) ||
      (P.pooled && ((rc = get((void **)&P.Lf, (size_t)D * P.LD * 8)) || (rc = get((void **)&P.ypool, (size_t)P.pool_split * DNP_RMAX * P.LD * 8)) ||
                    (rc = get((void **)&P.pmean, (size_t)P.LD * 8)) || (P.f32 && (rc = get((void **)&P.A32, (size_t)D * P.LD * 4))))) ||
      (rc = get((void **)&P.tpart, (size_t)chains * P.nblk * 3 * P.LD * 8)) || (rc = get((void **)&P.srow, (size_t)chains * 3 * P.ntile * P.LD * 8)) ||
      (rc = get((void **)&P.partial, (size_t)chains * P.npart * 8)) || (rc = get((void **)&P.lpbuf, (size_t)chains * 8)) ||
      (rc = get((void **)&P.ts, (size_t)chains * sizeof(TS))) || (rc = get((void **)&P.rd, (size_t)chains * sizeof(DnRound))) ||
      (rc = get((void **)&P.active, (size_t)chains * 4)) || (rc = get((void **)&P.fail, 4)) || (rc = get((void **)&P.act_passes, 8)))
    return rc;
  HIP_TRY(hipHostMalloc((void **)&sp->h_active, (size_t)chains * sizeof(int)));
  HIP_TRY(hipEventCreate(&sp->mv0)); HIP_TRY(hipEventCreate(&sp->mv1));
  for (int k = 0; k < Sampler::DN_AHEAD; k++) { HIP_TRY(hipEventCreate(&sp->rv0[k])); HIP_TRY(hipEventCreate(&sp->rv1[k])); HIP_TRY(hipEventCreate(&sp->rdone[k])); }
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dn_symv<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DN_SYMV_LDS(1)));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dn_symv<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DN_SYMV_LDS(2)));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dn_symv<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DN_SYMV_LDS(1)));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dn_symv<2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DN_SYMV_LDS(2)));
  if (sp->K == 1) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dn_grad1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp->lds_bytes));
  else for (const void *f : {reinterpret_cast<const void *>(k_dn_gradK<4>), reinterpret_cast<const void *>(k_dn_gradK<8>), reinterpret_cast<const void *>(k_dn_gradK<12>), reinterpret_cast<const void *>(k_dn_gradK<16>), reinterpret_cast<const void *>(k_dn_gradK<17>)})
    HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp->cl_lds_bytes));
  for (const void *f : {reinterpret_cast<const void *>(k_dn_pool_mm<1>), reinterpret_cast<const void *>(k_dn_pool_mm<2>), reinterpret_cast<const void *>(k_dn_pool_mm<3>),
                        reinterpret_cast<const void *>(k_dn_pool_mm<1, true>), reinterpret_cast<const void *>(k_dn_pool_mm<2, true>), reinterpret_cast<const void *>(k_dn_pool_mm<3, true>)})
    HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DNP_LDS(3)));
  hipLaunchKernelGGL(k_dn_identity, dim3((D + 255) / 256, mchains), dim3(256), 0, sp->stream, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(sp->stream));
  sp->dn_win_counter = 0; sp->dn_win_size = sp->R.window; sp->dn_win_next = rule_first_window_end(sp->R.init_buffer, sp->R.window); sp->dn_wf_n = 0;
  sp->dn_pass_bytes[0] = dense_pass_bytes(D, P.LD, DN_RB) / (P.f32 ? 2 : 1); sp->dn_pass_bytes[1] = dense_pass_bytes(D, P.LD, P.rb) / (P.f32 ? 2 : 1);   // ([1]: at the handle's own block size)
  if (P.pooled) sp->dn_pass_bytes[0] = sp->dn_pass_bytes[1] = (long long)D * P.LD * (P.f32 ? 4 : 8);   // the whole symmetric matrix, once per pass whatever the number of chains
  return 0;
}

// M^-1 times the round's right-hand sides for the active chains: one pass over the upper triangles (two launches when
// there are three right-hand sides) and the finishing kernel
void dense_symv_launch(hipStream_t st, const DnParams &P, const DnActive &act, int nrhs) {
  if (P.pooled) {
    // one pass over the handle's ONE matrix for every right-hand side of every chain that takes part (potus_dense_pool.hpp); more than
    // DNP_RMAX of them (over sixteen chains with three each) go in several launches, whole chains at a time
    const int nact = act.n ? act.n : P.chains, per = DNP_RMAX / nrhs;
    for (int c0 = 0; c0 < nact; c0 += per) {
      DnPoolRhs R;
      const int nc = std::min(per, nact - c0);
      R.n = nc * nrhs; R.nrhs = nrhs; R.job0 = 0;
      for (int r = 0; r < DNP_RMAX; r++) R.chain[r] = (unsigned char)(r < R.n ? (act.n ? act.idx[c0 + r / nrhs] : c0 + r / nrhs) : 0);
      const dim3 grid((unsigned)((P.D + DNP_COLS_OF(P.f32) - 1) / DNP_COLS_OF(P.f32)), (unsigned)P.pool_split);
      const int nt = (R.n + 15) / 16;
      if (P.f32) {
        if (nt == 1) hipLaunchKernelGGL((k_dn_pool_mm<1, true>), grid, dim3(DNP_THREADS), DNP_LDS(1), st, P, R, P.pool_rows);
        else if (nt == 2) hipLaunchKernelGGL((k_dn_pool_mm<2, true>), grid, dim3(DNP_THREADS), DNP_LDS(2), st, P, R, P.pool_rows);
        else hipLaunchKernelGGL((k_dn_pool_mm<3, true>), grid, dim3(DNP_THREADS), DNP_LDS(3), st, P, R, P.pool_rows);
      } else if (nt == 1) hipLaunchKernelGGL(k_dn_pool_mm<1>, grid, dim3(DNP_THREADS), DNP_LDS(1), st, P, R, P.pool_rows);
      else if (nt == 2) hipLaunchKernelGGL(k_dn_pool_mm<2>, grid, dim3(DNP_THREADS), DNP_LDS(2), st, P, R, P.pool_rows);
      else hipLaunchKernelGGL(k_dn_pool_mm<3>, grid, dim3(DNP_THREADS), DNP_LDS(3), st, P, R, P.pool_rows);
      hipLaunchKernelGGL(k_dn_pool_finish, dim3((unsigned)P.npart, (unsigned)R.n), dim3(64), 0, st, P, R, P.pool_split);
    }
    return;
  }
  const int nblk = (P.D + P.rb - 1) / P.rb;
  const unsigned ny = (unsigned)(act.n ? act.n : P.chains);
  const dim3 grid((unsigned)(((nblk + 1) / 2) * P.split), ny), fin((unsigned)P.npart, ny);
  auto one = [&](int job0) {
    if (P.f32) hipLaunchKernelGGL((k_dn_symv<1, true>), grid, dim3(DN_THREADS), DN_SYMV_LDS(1), st, P, act, job0);
    else hipLaunchKernelGGL((k_dn_symv<1, false>), grid, dim3(DN_THREADS), DN_SYMV_LDS(1), st, P, act, job0);
    hipLaunchKernelGGL(k_dn_symv_finish<1>, fin, dim3(DN_FIN), 0, st, P, act, job0);
  };
  if (nrhs == 1) one(0);
  else {
    if (P.f32) hipLaunchKernelGGL((k_dn_symv<2, true>), grid, dim3(DN_THREADS), DN_SYMV_LDS(2), st, P, act, 0);
    else hipLaunchKernelGGL((k_dn_symv<2, false>), grid, dim3(DN_THREADS), DN_SYMV_LDS(2), st, P, act, 0);
    hipLaunchKernelGGL(k_dn_symv_finish<2>, fin, dim3(DN_FIN), 0, st, P, act, 0);
    if (nrhs == 3) one(2);
  }
}

inline dim3 dn_grid(const Sampler *sp) { return dim3((unsigned)std::min((sp->L.D + 255) / 256, 64), (unsigned)sp->R.chains); }

int dense_grad(Sampler *sp) {
  if (sp->K == 1)
    hipLaunchKernelGGL(k_dn_grad1, dim3(sp->R.chains), dim3(PT_THREADS), sp->lds_bytes, sp->stream, (const DevModel *)sp->dM, sp->dn);
  else {
    const unsigned lid = ++sp->launch_id;
#define POTUS_CALL(TAG) hipLaunchKernelGGL(k_dn_gradK<TAG>, dim3(sp->R.chains * sp->K), dim3(PT_THREADS), sp->cl_lds_bytes, sp->stream, (const DevModel *)sp->dM, \
                                           (const ClModel *)sp->dCL, (const RunParams *)sp->dR, sp->dn, lid)
    CL_DISPATCH(sp->cl_dw, POTUS_CALL);
#undef POTUS_CALL
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
// one pass over the matrices of the active chains; the pass is timed with events resolved at the next sync point
int dense_matvec(Sampler *sp, int nrhs, int n_active, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr, bool timed = true) {
  DnActive act;
  act.n = 0;                                              // every chain, or (from the flags of the last sync point) the active ones, compacted
  if (n_active < sp->R.chains && sp->R.chains <= DN_ACT_MAX) {
    for (int c = 0; c < sp->R.chains; c++) if (sp->h_active[c]) act.idx[act.n++] = c;
    n_active = act.n;
  }
  dense_launch_shape(sp->dn, n_active);
  sp->dn.count_passes = timed ? 1 : 0;     // potus_dense_timing: bytes and milliseconds over the same set of passes
  // (launches of the matrix pass: two for three right-hand sides per chain; pooled: one per DNP_RMAX right-hand sides)
  const int nact_launch = act.n ? act.n : sp->R.chains;   // (an empty list means everybody: dense_symv_launch)
  sp->mv_launches_pending = !timed ? 0 : sp->dn.pooled ? (nact_launch + DNP_RMAX / nrhs - 1) / (DNP_RMAX / nrhs) : (nrhs == 3 ? 2 : 1);
  // (the bytes the passes stream are counted on the device, DnParams::act_passes: the host's flags may be a few rounds old)
  HIP_TRY(hipEventRecord(e0 ? e0 : sp->mv0, sp->stream));
  dense_symv_launch(sp->stream, sp->dn, act, nrhs);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1 ? e1 : sp->mv1, sp->stream));
  return 0;
}
// sync point of a round: the activity flags come to the host; returns the number of chains still active
int dense_sync(Sampler *sp, int *n_active, bool timed_matvec) {
  HIP_TRY(hipMemcpyAsync(sp->h_active, sp->dn.active, (size_t)sp->R.chains * sizeof(int), hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  int n = 0;
  for (int c = 0; c < sp->R.chains; c++) n += sp->h_active[c] != 0;
  if (timed_matvec) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, sp->mv0, sp->mv1));
    sp->mv_ms += ms; sp->mv_calls += sp->mv_launches_pending;
  }
  *n_active = n;
  return 0;
}
// p ~ N(0, M): standard normals, then L^T p = u (nothing to solve while the metric is the unit matrix)
int dense_sample_p(Sampler *sp, unsigned iter, unsigned purpose) {
  hipLaunchKernelGGL(k_dn_normals, dn_grid(sp), dim3(256), 0, sp->stream, sp->dn, (const RunParams *)sp->dR, iter, purpose);
  HIP_TRY(hipGetLastError());
  if (!sp->dn.identity) {
    const int nb = (sp->L.D + DN_NB - 1) / DN_NB;
    for (int b = nb - 1; b >= 0; b--) {
      hipLaunchKernelGGL(k_dn_trsv_diag, dim3(sp->R.chains), dim3(64), 0, sp->stream, sp->dn, b);
      if (b > 0) hipLaunchKernelGGL(k_dn_trsv_update, dim3((b * DN_NB + 255) / 256, sp->R.chains), dim3(256), 0, sp->stream, sp->dn, b);
    }
    HIP_TRY(hipGetLastError());
  }
  return 0;
}
// base_hmc::init_stepsize for every chain of the handle (the point QC, its log density in the chain scalars)
int dense_init_stepsize(Sampler *sp, unsigned iter) {
  int rc, n_active = 0;
  const int cg = (sp->R.chains + 63) / 64;
  hipLaunchKernelGGL(k_dn_eps_arm, dim3(cg), dim3(64), 0, sp->stream, sp->dn, (const RunParams *)sp->dR);
  if ((rc = dense_grad(sp))) return rc;                                  // hamiltonian.init at the current point: gradient -> GC
  if ((rc = dense_sync(sp, &n_active, false))) return rc;
  for (int attempt = 0; n_active > 0; attempt++) {
    if (attempt > 200) return fail(POTUS_ERR_STATE, "dense init_stepsize did not terminate");
    if ((rc = dense_sample_p(sp, iter, RNG_INIT_EPS))) return rc;
    hipLaunchKernelGGL(k_dn_eps_prekick, dn_grid(sp), dim3(256), 0, sp->stream, sp->dn, (const RunParams *)sp->dR);
    if ((rc = dense_matvec(sp, 2, n_active, nullptr, nullptr, false))) return rc;
    hipLaunchKernelGGL(k_dn_eps_mid, dim3(cg), dim3(64), 0, sp->stream, sp->dn, (const RunParams *)sp->dR);
    if ((rc = dense_grad(sp))) return rc;
    hipLaunchKernelGGL(k_dn_kick, dn_grid(sp), dim3(256), 0, sp->stream, sp->dn);
    if ((rc = dense_matvec(sp, 1, n_active, nullptr, nullptr, false))) return rc;
    hipLaunchKernelGGL(k_dn_eps_step, dim3(cg), dim3(64), 0, sp->stream, sp->dn, (const RunParams *)sp->dR);
    HIP_TRY(hipGetLastError());
    if ((rc = dense_sync(sp, &n_active, false))) return rc;
  }
  return 0;
}
// the rest of a window end once M^-1 stands (pooled: once the pooled M2 stands in P.A, n_total draws behind it): factor, new step size
static double dn_now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
int dense_window_finish(Sampler *sp, int n, unsigned iter, double n_total, double cov_ms) {
  DnParams &P = sp->dn;
  const int D = sp->L.D, chains = sp->R.chains;
  if (P.pooled) {
    const double ts = dn_now();
    hipLaunchKernelGGL(k_dn_pool_scale, dim3((unsigned)std::min((D + 255) / 256, 64), (unsigned)D), dim3(256), 0, sp->stream, P, n_total);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(sp->stream));
    cov_ms += dn_now() - ts;
  }
  const double tc = dn_now();
  dense_cholesky_launch(sp->stream, P, P.pooled ? 1 : chains);   // in place on the lower triangle; the upper one keeps M^-1 (pooled: in the factor's own buffer)
  HIP_TRY(hipGetLastError());
  int failed = 0;
  HIP_TRY(hipMemcpyAsync(&failed, P.fail, 4, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  if (failed) return fail(POTUS_ERR_STATE, "the adapted covariance of a chain is not positive definite (window of %d draws)", n);
  const double t2 = dn_now();
  P.identity = 0;
  int rc;
  if ((rc = dense_init_stepsize(sp, iter))) return rc;
  sp->we_cov_ms += cov_ms; sp->we_chol_ms += t2 - tc; sp->we_eps_ms += dn_now() - t2; sp->we_count += 1;
  hipLaunchKernelGGL(k_dn_window_done, dim3((chains + 63) / 64), dim3(64), 0, sp->stream, P, (const RunParams *)sp->dR, (int)iter);
  HIP_TRY(hipGetLastError());
  return 0;
}
// covar_adaptation at the end of a window of n draws: covariance -> M^-1, Cholesky factor, new step size
int dense_window_end(Sampler *sp, int n, unsigned iter) {
  DnParams &P = sp->dn;
  const int D = sp->L.D, chains = sp->R.chains, nb = (D + DN_NB - 1) / DN_NB;
  if (n < 2) return fail(POTUS_ERR_STATE, "adaptation window of %d draws", n);
  HIP_TRY(hipStreamSynchronize(sp->stream));
  const double t0 = dn_now();
  if (P.pooled) {   // the handle's mean and M2 over the draws of every chain (potus_dense_pool.hpp)
    hipLaunchKernelGGL(k_dn_pool_center, dim3((unsigned)std::min((D + 255) / 256, 64)), dim3(256), 0, sp->stream, P, n);
    hipLaunchKernelGGL(k_dn_pool_cov, dim3(nb, nb), dim3(256), 0, sp->stream, P, n);
  } else {
    hipLaunchKernelGGL(k_dn_center, dn_grid(sp), dim3(256), 0, sp->stream, P, n);
    hipLaunchKernelGGL(k_dn_cov, dim3(nb, nb, chains), dim3(256), 0, sp->stream, P, n);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(sp->stream));
  const double t1 = dn_now();
  if (sp->opts.pooled_metric == 2) {   // the host pools further (other handles, other ranks) and calls potus_dense_pool_finish
    sp->dn_pending = true; sp->dn_pending_n = n; sp->dn_pending_iter = iter; sp->dn_pending_cov_ms = t1 - t0;
    return 0;
  }
  return dense_window_finish(sp, n, iter, (double)chains * (double)n, t1 - t0);
}
// n_iter transitions of every chain of the handle
int dense_run(Sampler *sp, int n_iter) {
  DnParams &P = sp->dn;
  const int chains = sp->R.chains, total = sp->R.num_warmup + sp->R.num_samples, cg = (chains + 63) / 64;
  const int nw = sp->R.num_warmup, ib = sp->R.init_buffer, tb = sp->R.term_buffer;
  std::vector<ChainScalars> sc;
  int rc;
  if (sp->dn_pending) return fail(POTUS_ERR_STATE, "a pooled window end is pending (pooled_metric = 2): potus_dense_pool_finish comes before the next potus_run");
  if ((rc = read_scalars(sp, sc))) return rc;
  int it = sc[0].iter;
  for (int k = 0; k < n_iter && it < total && !sp->dn_pending; k++, it++) {
    int n_active = 0;
    hipLaunchKernelGGL(k_dn_arm, dim3(cg), dim3(64), 0, sp->stream, P, (const RunParams *)sp->dR, total);
    if ((rc = dense_sample_p(sp, (unsigned)it, RNG_MOMENTUM))) return rc;
    if ((rc = dense_grad(sp))) return rc;                                // hamiltonian.init: gradient at the current point -> GC
    hipLaunchKernelGGL(k_dn_begin, dn_grid(sp), dim3(256), 0, sp->stream, P, (const RunParams *)sp->dR);
    if ((rc = dense_matvec(sp, 3, chains))) return rc;
    hipLaunchKernelGGL(k_dn_step, dim3(chains), dim3(DN_THREADS), 0, sp->stream, P, (const RunParams *)sp->dR, (unsigned)it, (int)DN_MODE_BEGIN);
    HIP_TRY(hipGetLastError());
    if ((rc = dense_sync(sp, &n_active, true))) return rc;
    // Leaf rounds.  The host does not wait for a round before it queues the next: it keeps DN_AHEAD rounds in flight and looks
    // at the activity flags of the round that left the queue (they come back with an asynchronous copy behind every round;
    // flags only ever go from 1 to 0 inside a transition).  Chains that have finished sit rounds out on the device (every
    // kernel returns at once for them), so the rounds queued past the end of the transition cost a few empty launches --
    // against a host round trip per leaf with the GPU idle (13 % of the wall time at D = 15 098 before).
    {
      constexpr int R = Sampler::DN_AHEAD;
      long long q = 0;                                  // rounds queued in this transition
      auto retire = [&](long long r) -> int {           // wait for round r; its pass time; the flags as of then (or later)
        const int k = (int)(r % R);
        HIP_TRY(hipEventSynchronize(sp->rdone[k]));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, sp->rv0[k], sp->rv1[k]));
        sp->mv_ms += ms; sp->mv_calls += sp->rv_launches[k];
        int n = 0;
        for (int c = 0; c < sp->R.chains; c++) n += sp->h_active[c] != 0;
        n_active = n;
        return 0;
      };
      long long retired = 0;
      while (n_active > 0) {
        const int k = (int)(q % R);
        if ((rc = dense_grad(sp))) return rc;
        hipLaunchKernelGGL(k_dn_kick, dn_grid(sp), dim3(256), 0, sp->stream, P);
        if ((rc = dense_matvec(sp, 2, n_active, sp->rv0[k], sp->rv1[k]))) return rc;
        sp->rv_launches[k] = sp->mv_launches_pending;
        hipLaunchKernelGGL(k_dn_step, dim3(chains), dim3(DN_THREADS), 0, sp->stream, P, (const RunParams *)sp->dR, (unsigned)it, (int)DN_MODE_LEAF);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(sp->h_active, sp->dn.active, (size_t)sp->R.chains * sizeof(int), hipMemcpyDeviceToHost, sp->stream));
        HIP_TRY(hipEventRecord(sp->rdone[k], sp->stream));
        sp->dn_rounds += 1;
        q++;
        if (q - retired >= R) { if ((rc = retire(retired))) return rc; retired++; }
      }
      while (retired < q) { if ((rc = retire(retired))) return rc; retired++; }
    }
    // adapt_dense_e_nuts::transition: the warm-up schedule is the same for every chain, so the host keeps its own copy
    const bool warm = it < nw;
    int in_window = 0, end_window = 0;
    if (warm) rule_window_flags(nw, ib, tb, sp->dn_win_counter, sp->dn_win_next, in_window, end_window);
    const int flags = in_window | end_window << 1;
    hipLaunchKernelGGL(k_dn_end, dim3(chains), dim3(DN_THREADS), 0, sp->stream, P, (const RunParams *)sp->dR, it, flags, sp->dn_wf_n, total);
    HIP_TRY(hipGetLastError());
    if (in_window) sp->dn_wf_n += 1;
    if (end_window) {
      if ((rc = dense_window_end(sp, sp->dn_wf_n, (unsigned)it))) return rc;
      rule_next_window(nw, tb, sp->dn_win_counter, sp->dn_win_next, sp->dn_win_size);
      sp->dn_wf_n = 0;
    }
    if (warm && nw >= 20) sp->dn_win_counter += 1;
  }
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}
// potus_init of a dense-metric handle: k_init / k_cl_init have found the initial points and -- the metric being the
// unit matrix, for which the diagonal and the dense sampler coincide -- the initial step sizes; the points move over
int dense_import_init(Sampler *sp) {
  if (!sp->dn.identity || sp->dn_win_counter != 0) {
    // a second potus_init: back to the unit metric and the start of the window schedule (the upper triangle is what the matrix
    // pass reads, so the whole matrix goes, not only the flag)
    DnParams &P = sp->dn;
    HIP_TRY(hipMemsetAsync(P.A, 0, (size_t)(P.pooled ? 1 : P.chains) * P.D * P.LD * 8, sp->stream));
    if (P.pooled) HIP_TRY(hipMemsetAsync(P.Lf, 0, (size_t)P.D * P.LD * 8, sp->stream));
    if (P.pooled && P.f32) HIP_TRY(hipMemsetAsync(P.A32, 0, (size_t)P.D * P.LD * 4, sp->stream));
    HIP_TRY(hipMemsetAsync(P.fail, 0, 4, sp->stream));
    hipLaunchKernelGGL(k_dn_identity, dim3((P.D + 255) / 256, P.pooled ? 1 : P.chains), dim3(256), 0, sp->stream, P);
    HIP_TRY(hipGetLastError());
    P.identity = 1;
  }
  sp->dn_pending = false;
  sp->dn_win_counter = 0; sp->dn_win_size = sp->R.window; sp->dn_win_next = rule_first_window_end(sp->R.init_buffer, sp->R.window); sp->dn_wf_n = 0;
  hipLaunchKernelGGL(k_dn_import_q, dim3(64, sp->R.chains), dim3(256), 0, sp->stream, (const RunParams *)sp->dR, sp->dn,
                     sp->K > 1 ? sp->CL.perm : (const int *)nullptr, sp->K > 1 ? sp->CL.Dint : 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------------- pooled calls
// Calls that take a list of handles and treat their chains as the chains of ONE posterior ("The pooling contract").
int saved_count(Sampler *sp, int *n_saved) {
  std::vector<ChainScalars> sc;
  { const int rc_ = read_scalars(sp, sc); if (rc_) return rc_; }
  int m = -1;   // (many data sets: over the chains that have not failed)
  for (auto &s : sc) if (!sp->n_ds || s.status == 0) m = m < 0 ? s.saved : std::min(m, s.saved);
  *n_saved = std::max(m, 0);
  return 0;
}

// warm-up rows among the first n_saved rows of a handle (save_warmup = 1): not draws from the posterior -- rstan::monitor and extract() drop them
int warm_rows(const Sampler *sp, int n_saved) { return sp->opts.save_warmup ? std::min(n_saved, sp->R.num_warmup) : 0; }

// The draws of ONE handle's data sets (one data set when potus_set_datasets[_ex] was not called): what every call that works on them per data set needs.
// of() is the part that needs no device -- the data sets, their chains, their models; ds_plan() adds the post-warm-up window and who has failed.
struct DsPlan {
  int n_ds = 1, cpd = 1, first = 0, n_post = 0;   // data sets, chains of each; saved rows [first, first + n_post) are the draws
  std::vector<int> failed, skip;                  // per chain: its status is not 0; per data set: one of its chains has failed
  const DevModel *Mg = nullptr;                   // n_ds models on the device (the handle's one model when it holds one data set)
  void of(const Sampler *sp) { n_ds = std::max(sp->n_ds, 1); cpd = sp->chains_per_ds(); Mg = sp->n_ds ? sp->dMs : sp->dM; }
};
int ds_plan(const char *what, Sampler *sp, DsPlan &pl) {   // under the device lock, before anything is allocated or launched
  pl.of(sp);
  std::vector<ChainScalars> sc;
  if (const int rc = read_scalars(sp, sc)) return rc;
  int n_saved = 0;
  if (const int rc = saved_count(sp, &n_saved)) return rc;
  pl.first = warm_rows(sp, n_saved); pl.n_post = n_saved - pl.first;
  if (pl.n_post < 1) return fail(POTUS_ERR_STATE, "%s: no post-warm-up draws saved yet (%d saved, %d of them warm-up)", what, n_saved, pl.first);
  pl.failed.assign(sp->R.chains, 0); pl.skip.assign(pl.n_ds, 0);
  for (int c = 0; c < sp->R.chains; c++) if (sc[c].status != 0) pl.failed[c] = pl.skip[c / pl.cpd] = 1;
  return 0;
}

int check_cols(const Sampler *sp, int col_begin, int col_end) {
  if (col_begin < 0 || col_end > sp->L.ncols || col_begin >= col_end) return fail(POTUS_ERR_ARG, "bad column range [%d,%d) of %d", col_begin, col_end, sp->L.ncols);
  return 0;
}

// The listed handles, resolved.  Everything down to same_posterior() needs no device and is done before the first HIP call; count() runs
// under the caller's DeviceLocks(devs), which the caller holds from there to the last synchronise of the call.
struct Pool {
  const char *what = "";
  const int *handles = nullptr;
  std::vector<Sampler *> sps;
  std::vector<int> devs, saved;   // per handle: its device; its saved rows per chain (count())
  Sampler *s0 = nullptr;          // the first handle: the pooled work runs on its GPU
  int chains = 0;                 // count(): chains of all handles
  long long draws = 0;            //          ... and the rows they have saved

  int lookup(const int *h, int n, const char *what_) {
    what = what_; handles = h;
    if (!h || n < 1) return fail(POTUS_ERR_ARG, "%s: null handle list", what);
    for (int i = 0; i < n; i++) {
      Sampler *sp = get(h[i]);
      if (!sp) return fail(POTUS_ERR_STATE, "%s: bad handle %d", what, h[i]);
      sps.push_back(sp); devs.push_back(sp->device);
    }
    s0 = sps[0];
    return 0;
  }
  int single_dataset() const {
    for (const Sampler *sp : sps) if (const int rc = refuse_many_datasets(sp, what)) return rc;
    return 0;
  }
  int distinct() const {
    for (size_t i = 0; i < sps.size(); i++)
      for (size_t j = 0; j < i; j++) if (handles[j] == handles[i]) return fail(POTUS_ERR_ARG, "%s: handle %d listed twice", what, handles[i]);
    return 0;
  }
  // what a call that pools chains starts with
  int resolve(const int *h, int n, const char *what_) {
    if (const int rc = lookup(h, n, what_)) return rc;
    if (const int rc = single_dataset()) return rc;
    return distinct();
  }
  // same columns, same variant, same data (hash_data covers the sizes, S and T among them)
  int same_posterior(const char *why) const {
    for (size_t i = 1; i < sps.size(); i++)
      if (sps[i]->L.ncols != s0->L.ncols || sps[i]->M.full != s0->M.full || sps[i]->data_hash != s0->data_hash)
        return fail(POTUS_ERR_ARG, "%s: handle %d holds another posterior than handle %d (%s)", what, handles[i], handles[0], why);
    return 0;
  }
  int count() {
    saved.assign(sps.size(), 0); chains = 0; draws = 0;
    for (size_t i = 0; i < sps.size(); i++) {
      HIP_TRY(hipSetDevice(sps[i]->device));
      if (const int rc = saved_count(sps[i], &saved[i])) return rc;
      chains += sps[i]->R.chains; draws += (long long)saved[i] * sps[i]->R.chains;
    }
    return 0;
  }
  int equal_counts() const {
    for (size_t i = 1; i < sps.size(); i++)
      if (saved[i] != saved[0]) return fail(POTUS_ERR_STATE, "%s: handle %d has saved %d draws per chain, handle %d has %d", what, handles[i], saved[i], handles[0], saved[0]);
    return 0;
  }
  // after equal_counts(): the first post-warm-up row of every handle and the draws per chain from there on
  int post_warmup(int *first, int *n_post) const {
    *first = warm_rows(s0, saved[0]); *n_post = saved[0] - *first;
    for (const Sampler *sp : sps) if (warm_rows(sp, saved[0]) != *first) return fail(POTUS_ERR_ARG, "%s: the handles saved different numbers of warm-up rows", what);
    if (*n_post < 4) return fail(POTUS_ERR_STATE, "%s needs at least four saved post-warm-up draws per chain (%d saved, %d of them warm-up)", what, saved[0], *first);
    return 0;
  }
};

// One handle's block of a pooled call: made on the handle's own GPU -- produce(out) queues the work on sp's stream, sp's device current -- and
// landed in dst on the first handle's.  On return the block is complete and s0's device is current.
template <class Produce>
int gather_block(Sampler *s0, Sampler *sp, size_t bytes, double *dst, Produce produce) {
  HIP_TRY(hipSetDevice(sp->device));
  DevBufs far;
  double *blk = dst;
  if (sp->device != s0->device) HIP_TRY(far.alloc(&blk, bytes));
  if (const int rc = produce(blk)) return rc;
  HIP_TRY(hipStreamSynchronize(sp->stream));
  if (blk != dst) {
    // (hipMemcpyPeer stages through the host when the two GPUs have no peer access; with it, the copy goes over xGMI)
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, s0->device, sp->device) == hipSuccess && can) { (void)hipSetDevice(s0->device); (void)hipDeviceEnablePeerAccess(sp->device, 0); (void)hipGetLastError(); }
    HIP_TRY(hipMemcpyPeer(dst, s0->device, blk, sp->device, bytes));
  }
  HIP_TRY(hipSetDevice(s0->device));
  return 0;
}

// blk [n][C][ncol] -> the places of chains coff .. coff + C - 1 in cols [ncol][Ctot][n]
int transpose_block(hipStream_t st, const double *blk, double *cols, long long n, int C, int ncol, int Ctot, int coff) {
  hipLaunchKernelGGL(k_dg_transpose, dim3((ncol + 63) / 64, (unsigned)((n + 63) / 64), C), dim3(256), 0, st, blk, cols, n, C, ncol, Ctot, coff);
  HIP_TRY(hipGetLastError());
  return 0;
}
// ... of one handle of a pool, on the first handle's GPU, finished on return (the caller frees blk next)
int pool_transpose(Sampler *s0, const double *blk, double *cols, int n_post, int C, int ncol, int Ctot, int coff) {
  if (const int rc = transpose_block(s0->stream, blk, cols, n_post, C, ncol, Ctot, coff)) return rc;
  HIP_TRY(hipStreamSynchronize(s0->stream));
  return 0;
}

// dynamic LDS of the kernels that sort a column of n items in runs (k_dg_column, k_mn_column, k_loo_psis): the keys and the indices of one run
size_t sorted_run_lds(long long n) {
  int npad = 1;
  while (npad < n && npad < DG_RUN) npad <<= 1;
  return (size_t)npad * 12;
}
// ... and their runs in global memory, for `grid` workgroups of N items each: above DG_RUN items only (one run stays in LDS)
size_t sorted_run_bytes(long long N) { return N > DG_RUN ? (size_t)N * 12 : 0; }
int sorted_run_scratch(DevBufs &bufs, int grid, long long N, unsigned long long **rkey, unsigned **ridx, const char *what) {
  *rkey = nullptr; *ridx = nullptr;
  if (N <= DG_RUN) return 0;
  if (const int rc = bufs.get(rkey, (size_t)grid * (size_t)N * 8, what)) return rc;
  return bufs.get(ridx, (size_t)grid * (size_t)N * 4, what);
}

// The PSIS workspace (potus_psis.hpp) of `grid` workgroups over S pooled draws, each with extra_rows rows of S doubles of the kernel's own behind
// the PSIS rows: the bytes one workgroup needs (what a budget-capped grid divides by); the buffers out of `bufs`, and the dynamic LDS of the
// kernels that will be launched on them.
size_t psis_work_bytes(long long S, int extra_rows) { return psis_ws_doubles(S, extra_rows) * 8 + (size_t)S * 4 + sorted_run_bytes(S); }
int psis_work(DevBufs &bufs, int grid, long long S, int extra_rows, PsisWork &W, const char *what, std::initializer_list<const void *> kernels) {
  W.mmax = psis_mmax(S);
  W.stride = psis_ws_doubles(S, extra_rows);
  int rc;
  if ((rc = bufs.get(&W.wsd, (size_t)grid * W.stride * 8, what)) || (rc = bufs.get(&W.wsi, (size_t)grid * S * 4, what)) ||
      (rc = sorted_run_scratch(bufs, grid, S, &W.rkey, &W.ridx, what)))
    return rc;
  for (const void *k : kernels) HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sorted_run_lds(S)));
  return 0;
}

} // namespace

// ======================================================================== C ABI
extern "C" {

const char *potus_version(void) { return "potus_hmc 0.5 (gfx950)"; }   // 0.5: potus_opts.pooled_metric (round 6), and the entry points added since without a change to potus_opts (... potus_timeline*, potus_cv_*);   // 0.4: potus_opts.metric_storage (round 3), potus_diagnostics* (round 4)

int potus_last_error(char *buf, int len) {
  if (buf && len > 0) { std::snprintf(buf, (size_t)len, "%s", g_err.c_str()); }
  return (int)g_err.size();
}

void potus_default_opts(potus_opts *o) {
  std::memset(o, 0, sizeof *o);
  o->chains = 4; o->chain_id_offset = 0; o->num_warmup = 1000; o->num_samples = 1000; o->max_depth = 10;
  o->init_buffer = 75; o->term_buffer = 50; o->window = 25;
  o->delta = 0.8; o->gamma = 0.05; o->kappa = 0.75; o->t0 = 10; o->stepsize = 1.0; o->init_radius = 2.0;
  o->seed = 1843; o->device = 0; o->save_warmup = 0; o->cus_per_chain = 0; o->metric = POTUS_METRIC_DIAG; o->twin = -1; o->pooled_metric = 0; o->reserved_ = 0; o->metric_storage = POTUS_STORAGE_F64;
}

int potus_num_params(const potus_data *d, int *D) {
  if (!d || !D) return fail(POTUS_ERR_ARG, "null argument");
  *D = make_layout(d).D;
  return 0;
}
int potus_num_columns(const potus_data *d, int *n_cols) {
  if (!d || !n_cols) return fail(POTUS_ERR_ARG, "null argument");
  *n_cols = make_layout(d).ncols;
  return 0;
}

int potus_column_name(const potus_data *d, int col, char *buf, int len) {
  if (!d || !buf || len <= 0) return fail(POTUS_ERR_ARG, "null argument");
  static const char *samp[] = {"lp__", "accept_stat__", "stepsize__", "treedepth__", "n_leapfrog__", "divergent__", "energy__"};
  if (col < 0) return fail(POTUS_ERR_ARG, "negative column");
  if (col < POTUS_N_SAMPLER_COLS) { std::snprintf(buf, (size_t)len, "%s", samp[col]); return 0; }
  const bool full = d->variant == POTUS_VARIANT_FULL;
  struct Blk { const char *name; int r, c; }; // r x c column-major; c = 0: vector of r (which may be empty), c < 0: scalar
  std::vector<Blk> b = {{"raw_mu_b_T", d->S, 0}, {"raw_mu_b", d->S, d->T}, {"raw_mu_c", d->P, 0}};
  if (full) { b.push_back({"raw_mu_m", d->M, 0}); b.push_back({"raw_mu_pop", d->Pop, 0}); b.push_back({"mu_e_bias", 1, -1});
              b.push_back({"rho_e_bias", 1, -1}); b.push_back({"raw_e_bias", d->T, 0}); }
  b.push_back({"raw_measure_noise_national", d->N_national_polls, 0}); b.push_back({"raw_measure_noise_state", d->N_state_polls, 0});
  b.push_back({"raw_polling_bias", d->S, 0});
  b.push_back({"mu_b", d->S, d->T}); b.push_back({"mu_c", d->P, 0});
  if (full) { b.push_back({"mu_m", d->M, 0}); b.push_back({"mu_pop", d->Pop, 0}); b.push_back({"e_bias", d->T, 0}); }
  b.push_back({"polling_bias", d->S, 0}); b.push_back({"national_mu_b_average", d->T, 0}); b.push_back({"national_polling_bias_average", 1, -1});
  if (full) b.push_back({"sigma_rho", 1, -1});
  b.push_back({"logit_pi_democrat_state", d->N_state_polls, 0}); b.push_back({"logit_pi_democrat_national", d->N_national_polls, 0});
  b.push_back({"predicted_score", d->T, d->S});
  int c = col - POTUS_N_SAMPLER_COLS;
  for (const Blk &k : b) {
    const int n = k.c <= 0 ? k.r : k.r * k.c;
    if (c < n) {
      if (k.c < 0) std::snprintf(buf, (size_t)len, "%s", k.name);
      else if (k.c == 0) std::snprintf(buf, (size_t)len, "%s.%d", k.name, c + 1);
      else std::snprintf(buf, (size_t)len, "%s.%d.%d", k.name, c % k.r + 1, c / k.r + 1);
      return 0;
    }
    c -= n;
  }
  return fail(POTUS_ERR_ARG, "column %d out of range", col);
}

// ---------------------------------------------------------------- how many workgroups work for a chain (pure functions)
// The first plan for cus_per_chain (potus_create may still double it when a member's polls do not fit its LDS):
// 0 = as many compute units per chain as fit the device, out of {16, 8, 4, 1}; 9-12 chains on 256 compute units get 14 / 12 /
// 11 / 10 so that a second cluster per chain fits (*lowered_for_twin = 1: back to 16 if the second cluster is not taken).
int potus_plan_cus_per_chain(int chains, int T, int n_cus, int cus_per_chain, int twin, int metric, int one_workgroup_ok, int *K_out, int *lowered_for_twin) {
  if (!K_out || !lowered_for_twin) return fail(POTUS_ERR_ARG, "potus_plan_cus_per_chain: null output");
  if (chains < 1 || n_cus < 1 || T < 1) return fail(POTUS_ERR_ARG, "potus_plan_cus_per_chain: chains, T and the number of compute units must be positive");
  int K = cus_per_chain;
  *lowered_for_twin = 0;
  if (K < 0 || K > CL_MAXK) return fail(POTUS_ERR_ARG, "cus_per_chain must be in [0,%d]", CL_MAXK);
  if (K == 0) {
    K = chains * 16 <= n_cus ? 16 : chains * 8 <= n_cus ? 8 : chains * 4 <= n_cus ? 4 : 1;
    if (K == 4 && T > 4 * CL_MAXDAYS) K = 1;      // four members hold up to 256 days
    // 9-12 chains: two clusters of 14, 12, 11 or 10 per chain (17-20 us per leapfrog on the 2016 posterior) beat one cluster
    // of 16 (21 us) -- as long as the members keep few enough days for the lighter build of the pass (4 days per wave)
    if (K == 16 && twin != 0 && metric != POTUS_METRIC_DENSE && chains * 32 > n_cus) {
      const int k2 = n_cus / (2 * chains);
      if (k2 >= 10 && (T + k2 - 1) / k2 <= CL_DW4_MAXAVG) { K = k2; *lowered_for_twin = 1; }
    }
    // models beyond the one-workgroup kernels (T > 256, > 2048 polls) need a cluster; long campaigns need more members
    if (K == 1 && !one_workgroup_ok) K = 8;
    while (K > 1 && T > K * CL_MAXDAYS && 2 * K <= CL_MAXK) K *= 2;
    if (K > 1 && chains * K > n_cus)
      return fail(POTUS_ERR_UNSUPPORTED, "%s, and %d chains x %d compute units do not fit the %d of the device",
                  one_workgroup_ok ? "T needs more members per chain" : "the model needs a cluster per chain", chains, K, n_cus);
  } else if (K == 1 && !one_workgroup_ok)
    return fail(POTUS_ERR_UNSUPPORTED, "the model is beyond the one-workgroup kernels; use cus_per_chain = 0 or >= 8");
  if (K > 1 && chains * K > n_cus) return fail(POTUS_ERR_ARG, "chains * cus_per_chain = %d exceeds the %d compute units of the device", chains * K, n_cus);
  *K_out = K;
  return 0;
}

// One or two clusters (K > 1) / workgroups (K = 1) per chain, one per end of the trajectory: two when asked for (twin = 1) or when
// the library chooses the size as well (twin < 0 and cus_per_chain = 0), the metric is diagonal and 2 * chains * K workgroups are
// resident together (resident_per_cu: workgroups of the kernel a compute unit holds).  twin = 1 that does not fit is an error.
int potus_plan_sides(int chains, int K, int n_cus, int resident_per_cu, int cus_per_chain, int twin, int metric, int *sides) {
  if (!sides) return fail(POTUS_ERR_ARG, "potus_plan_sides: null output");
  if (twin < -1 || twin > 1) return fail(POTUS_ERR_ARG, "twin must be -1 (library's choice), 0 or 1");
  const bool fits = metric != POTUS_METRIC_DENSE && resident_per_cu >= 1 &&
                    2ll * chains * K <= (long long)n_cus * (K == 1 ? resident_per_cu : 1);
  if (twin == 1 && !fits) {
    if (K == 1)
      return fail(POTUS_ERR_ARG, "twin = 1: two workgroups per chain need %d resident workgroups (the device holds %d) and the diagonal metric",
                  2 * chains, n_cus * std::max(resident_per_cu, 0));
    return fail(POTUS_ERR_ARG, "twin = 1: two clusters of %d per chain need %d compute units (the device has %d) and the diagonal metric", K, chains * 2 * K, n_cus);
  }
  *sides = ((twin == 1 || (twin < 0 && cus_per_chain == 0)) && fits) ? 2 : 1;
  return 0;
}

int potus_create(const potus_data *d, const potus_opts *o, int *handle) {
  if (!o || !handle) return fail(POTUS_ERR_ARG, "null argument");
  int rc = validate(d);
  if (rc) return rc;
  if (o->chains < 1) return fail(POTUS_ERR_ARG, "chains must be >= 1");
  if (o->max_depth < 1 || o->max_depth > PT_MAXD) return fail(POTUS_ERR_ARG, "max_depth must be in [1,%d]", PT_MAXD);
  if (o->num_warmup < 0 || o->num_samples < 0) return fail(POTUS_ERR_ARG, "negative iteration counts");
  if (o->metric != POTUS_METRIC_DIAG && o->metric != POTUS_METRIC_DENSE) return fail(POTUS_ERR_ARG, "metric must be POTUS_METRIC_DIAG or POTUS_METRIC_DENSE");
  if (o->twin < -1 || o->twin > 1) return fail(POTUS_ERR_ARG, "twin must be -1 (library's choice), 0 or 1");
  if (o->metric_storage != POTUS_STORAGE_F64 && o->metric_storage != POTUS_STORAGE_F32) return fail(POTUS_ERR_ARG, "metric_storage must be POTUS_STORAGE_F64 or POTUS_STORAGE_F32");
  if (o->pooled_metric < 0 || o->pooled_metric > 2) return fail(POTUS_ERR_ARG, "pooled_metric must be 0, 1 or 2");
  if (o->pooled_metric && o->metric != POTUS_METRIC_DENSE) return fail(POTUS_ERR_ARG, "pooled_metric applies to the dense metric (metric = POTUS_METRIC_DENSE)");
  if (o->metric_storage == POTUS_STORAGE_F32 && o->metric != POTUS_METRIC_DENSE) return fail(POTUS_ERR_ARG, "metric_storage = f32 applies to the dense metric only");
  // CmdStan 2.24's argument bounds (arg_adapt_*, arg_stepsize, arg_init); written so that a NaN fails every one of them
  if (!(o->delta > 0.0 && o->delta < 1.0)) return fail(POTUS_ERR_ARG, "delta must be in (0, 1), got %g", o->delta);
  if (!(o->gamma > 0.0 && std::isfinite(o->gamma))) return fail(POTUS_ERR_ARG, "gamma must be finite and > 0, got %g", o->gamma);
  if (!(o->kappa > 0.0 && std::isfinite(o->kappa))) return fail(POTUS_ERR_ARG, "kappa must be finite and > 0, got %g", o->kappa);
  if (!(o->t0 > 0.0 && std::isfinite(o->t0))) return fail(POTUS_ERR_ARG, "t0 must be finite and > 0, got %g", o->t0);
  if (!(o->stepsize > 0.0 && std::isfinite(o->stepsize))) return fail(POTUS_ERR_ARG, "stepsize must be finite and > 0, got %g", o->stepsize);
  if (!(o->init_radius >= 0.0 && std::isfinite(o->init_radius))) return fail(POTUS_ERR_ARG, "init_radius must be finite and >= 0, got %g", o->init_radius);
  if (o->init_buffer < 0) return fail(POTUS_ERR_ARG, "init_buffer must be >= 0, got %d", o->init_buffer);
  if (o->term_buffer < 0) return fail(POTUS_ERR_ARG, "term_buffer must be >= 0, got %d", o->term_buffer);
  if (o->window < 0) return fail(POTUS_ERR_ARG, "window must be >= 0, got %d", o->window);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(POTUS_ERR_DEVICE, "no HIP device: libpotus_hmc needs an MI355X (gfx950)");
  if (o->device < 0 || o->device >= ndev) return fail(POTUS_ERR_DEVICE, "device %d out of range (have %d)", o->device, ndev);
  HIP_TRY(hipSetDevice(o->device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, o->device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fail(POTUS_ERR_DEVICE, "device is %s; this library is built for gfx950 only", prop.gcnArchName);

  Sampler *sp = new Sampler();
  sp->device = o->device; sp->opts = *o; sp->L = make_layout(d);
  sp->data_hash = hash_data(d);
  auto bail = [&](int code) {
    for (void *p : sp->allocs) (void)hipFree(p);
    if (sp->ev0) (void)hipEventDestroy(sp->ev0);
    if (sp->ev1) (void)hipEventDestroy(sp->ev1);
    if (sp->mv0) (void)hipEventDestroy(sp->mv0);
    if (sp->mv1) (void)hipEventDestroy(sp->mv1);
    for (int k = 0; k < Sampler::DN_AHEAD; k++) { if (sp->rv0[k]) (void)hipEventDestroy(sp->rv0[k]); if (sp->rv1[k]) (void)hipEventDestroy(sp->rv1[k]); if (sp->rdone[k]) (void)hipEventDestroy(sp->rdone[k]); }
    if (sp->h_active) (void)hipHostFree(sp->h_active);
    if (sp->stream) (void)hipStreamDestroy(sp->stream);
    delete sp;
    return code;
  };
  if ((rc = build_model(sp, d))) return bail(rc);
  if (sp->k1_unsupported.empty() && (rc = set_lds_attr(sp))) return bail(rc);
  {
    // workgroups (CUs) per chain and sides: potus_plan_cus_per_chain / potus_plan_sides (pure functions, below; tested without a GPU)
    const int ncu = prop.multiProcessorCount;
    int K = 0, lowered = 0;
    if ((rc = potus_plan_cus_per_chain(o->chains, d->T, ncu, o->cus_per_chain, o->twin, o->metric, sp->k1_unsupported.empty() ? 1 : 0, &K, &lowered))) {
      if (rc == POTUS_ERR_UNSUPPORTED && !sp->k1_unsupported.empty()) {
        const std::string first = g_err;
        return bail(fail(rc, "%s (%s)", sp->k1_unsupported.c_str(), first.c_str()));
      }
      return bail(rc);
    }
    const bool k_lowered_for_twin = lowered != 0;
    if (K == 1) {
      // Two workgroups per chain, one per end of the trajectory (potus_nuts_twin.hpp): both sides of every chain wait for each
      // other, so the whole grid has to be resident at once
      int per_cu = 0, sides = 1;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(k_run_twin), PT_THREADS, sp->lds_bytes) != hipSuccess) per_cu = 0;
      if ((rc = potus_plan_sides(o->chains, 1, ncu, per_cu, o->cus_per_chain, o->twin, o->metric, &sides))) return bail(rc);
      sp->twin = sides == 2;
    }
    if (K > 1) {
      rc = build_cluster(sp, d, K);
      // chosen by the library: a member whose polls do not fit its LDS gets half of them with twice the members
      while (rc == POTUS_ERR_UNSUPPORTED && o->cus_per_chain == 0 && 2 * K <= CL_MAXK && o->chains * 2 * K <= ncu) { K *= 2; rc = build_cluster(sp, d, K); }
      if (rc) return bail(rc);
      // the members of a cluster wait for each other: the whole grid has to be resident at once
      int per_cu = 0;
      const void *kfn = sp->cl_dw == 16 ? reinterpret_cast<const void *>(k_cl_run<16, false>) : sp->cl_dw == 17 ? reinterpret_cast<const void *>(k_cl_run<17, false>) : sp->cl_dw == 4 ? reinterpret_cast<const void *>(k_cl_run<4, false>)
                        : sp->cl_dw == 12 ? reinterpret_cast<const void *>(k_cl_run<12, false>) : reinterpret_cast<const void *>(k_cl_run<8, false>);
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, PT_THREADS, sp->cl_lds_bytes) != hipSuccess || per_cu < 1)
        return bail(fail(POTUS_ERR_DEVICE, "cluster kernel cannot be resident on this device (occupancy query: %d workgroups per compute unit with %zu bytes of LDS)",
                         per_cu, sp->cl_lds_bytes));
      if ((long long)o->chains * K > (long long)ncu * per_cu)
        return bail(fail(POTUS_ERR_ARG, "chains * cus_per_chain = %d workgroups cannot be resident together (%d compute units x %d)", o->chains * K, ncu, per_cu));
      // Two clusters per chain, one per end of the trajectory (potus_cluster.hpp, twin mode), when the compute units are there:
      // asked for (twin = 1), or chosen with the cluster size (twin < 0 and cus_per_chain = 0).  Diagonal metric only.
      int sides_plan = 1;
      if ((rc = potus_plan_sides(o->chains, K, ncu, 1, o->cus_per_chain, o->twin, o->metric, &sides_plan))) return bail(rc);
      const bool twin_fits = sides_plan == 2;      // asked for or chosen, and the compute units are there
      const void *kft = sp->cl_dw == 16 ? reinterpret_cast<const void *>(k_cl_run<16, true>) : sp->cl_dw == 17 ? reinterpret_cast<const void *>(k_cl_run<17, true>) : sp->cl_dw == 4 ? reinterpret_cast<const void *>(k_cl_run<4, true>)
                        : sp->cl_dw == 12 ? reinterpret_cast<const void *>(k_cl_run<12, true>) : reinterpret_cast<const void *>(k_cl_run<8, true>);
      int per_cu_t = 0;
      if (twin_fits && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_t, kft, PT_THREADS, sp->cl_lds_bytes) == hipSuccess && per_cu_t >= 1)
        sp->twin = 1;
      else if (o->twin == 1) return bail(fail(POTUS_ERR_DEVICE, "twin = 1: the twin kernel cannot be resident on this device"));
      if (!sp->twin && k_lowered_for_twin) {   // the smaller clusters were chosen for the sake of the second one: without it, back to 16
        if ((rc = build_cluster(sp, d, 16))) return bail(rc);
      }
    }
  }
  if (hipStreamCreateWithFlags(&sp->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&sp->ev0) != hipSuccess ||
      hipEventCreate(&sp->ev1) != hipSuccess)
    return bail(fail(POTUS_ERR_DEVICE, "stream/event creation failed"));

  RunParams &R = sp->R;
  R.chains = o->chains; R.chain_id_offset = o->chain_id_offset; R.num_warmup = o->num_warmup; R.num_samples = o->num_samples;
  R.max_depth = o->max_depth; R.save_warmup = o->save_warmup;
  // windowed_adaptation::set_window_params
  int ib = o->init_buffer, tb = o->term_buffer, bw = o->window;
  rule_window_params(o->num_warmup, ib, tb, bw);
  R.init_buffer = ib; R.term_buffer = tb; R.window = bw;
  R.delta = o->delta; R.gamma = o->gamma; R.kappa = o->kappa; R.t0 = o->t0; R.stepsize = o->stepsize; R.init_radius = o->init_radius;
  R.seed_lo = (unsigned)(o->seed & 0xFFFFFFFFu); R.seed_hi = (unsigned)(o->seed >> 32);
  R.Dpad = sp->K > 1 ? ((sp->CL.Dint + 15) & ~15) : ((sp->L.D + 7) & ~7);
  R.row = POTUS_N_SAMPLER_COLS + sp->L.D;
  R.n_save_max = o->num_samples + (o->save_warmup ? o->num_warmup : 0);
  void *p = nullptr;
  const size_t nblk = (size_t)o->chains * sp->sides();      // twin mode: a block per side
  const size_t state_bytes = nblk * V_COUNT * R.Dpad * sizeof(double);
  if (hipMalloc(&p, state_bytes) != hipSuccess) return bail(fail(POTUS_ERR_DEVICE, "hipMalloc(%zu) for chain state failed", state_bytes));
  sp->allocs.push_back(p); R.state = (double *)p;
  (void)hipMemset(p, 0, state_bytes);
  if (hipMalloc(&p, sizeof(ChainScalars) * nblk * sp->K) != hipSuccess) return bail(fail(POTUS_ERR_DEVICE, "hipMalloc for chain scalars failed"));
  sp->allocs.push_back(p); R.scal = (ChainScalars *)p;
  (void)hipMemset(p, 0, sizeof(ChainScalars) * nblk * sp->K);
  R.K = sp->K; R.xbuf = nullptr; R.xcnt = nullptr; R.twin = sp->twin; R.twbuf = nullptr;
  R.debug_drop_member = getenv("POTUS_DEBUG_DROP_MEMBER") ? atoi(getenv("POTUS_DEBUG_DROP_MEMBER")) : 0;
  if (sp->coop()) {
    const size_t xb = nblk * (4 * (size_t)sp->K * sp->CL.XW + 8) * 16;   // per chain (and side): 4 exchange slots + a line for the watchdog word
    if (hipMalloc(&p, xb) != hipSuccess) return bail(fail(POTUS_ERR_DEVICE, "hipMalloc for exchange buffers failed"));
    sp->allocs.push_back(p); R.xbuf = (double *)p;
    (void)hipMemset(p, 0, xb);
    if (hipMalloc(&p, (size_t)o->chains * 64 * sizeof(unsigned)) != hipSuccess) return bail(fail(POTUS_ERR_DEVICE, "hipMalloc for exchange counters failed"));
    sp->allocs.push_back(p); R.xcnt = (unsigned *)p;
    (void)hipMemset(p, 0, (size_t)o->chains * 64 * sizeof(unsigned));
    if (sp->twin) {
      const size_t tb = (size_t)o->chains * TWB_WORDS * 16;
      if (hipMalloc(&p, tb) != hipSuccess) return bail(fail(POTUS_ERR_DEVICE, "hipMalloc for the twin mailboxes failed"));
      sp->allocs.push_back(p); R.twbuf = (double *)p;
      (void)hipMemset(p, 0, tb);
    }
  }
  const size_t draw_bytes = std::max<size_t>((size_t)o->chains * R.n_save_max * R.row, 1) * sizeof(double);
  if (hipMalloc(&p, draw_bytes) != hipSuccess) return bail(fail(POTUS_ERR_DEVICE, "hipMalloc(%zu) for draws failed", draw_bytes));
  sp->allocs.push_back(p); R.draws = (double *)p;
  (void)hipMemset(p, 0, draw_bytes);

#ifdef POTUS_PROF
  if (hipMalloc(&p, sizeof(double) * PT_NPROF * nblk * sp->K) != hipSuccess) return bail(fail(POTUS_ERR_DEVICE, "hipMalloc for profile failed"));
  sp->allocs.push_back(p); R.prof = (double *)p;
  (void)hipMemset(p, 0, sizeof(double) * PT_NPROF * nblk * sp->K);
#else
  R.prof = nullptr;
#endif
  if (hipMalloc(&p, sizeof(RunParams)) != hipSuccess) return bail(fail(POTUS_ERR_DEVICE, "hipMalloc for run parameters failed"));
  sp->allocs.push_back(p); sp->dR = (RunParams *)p;
  if (hipMemcpy(p, &R, sizeof(RunParams), hipMemcpyHostToDevice) != hipSuccess) return bail(fail(POTUS_ERR_DEVICE, "upload of run parameters failed"));
  if (o->metric == POTUS_METRIC_DENSE) {
    sp->dense = true;
    if ((rc = dense_alloc(sp))) return bail(rc);
  }
  // the buffers above were cleared on the null stream, the sampler launches on its own non-blocking stream
  if (hipDeviceSynchronize() != hipSuccess) return bail(fail(POTUS_ERR_DEVICE, "device synchronisation after the allocations failed"));
  std::lock_guard<std::mutex> lk(g_mu);
  size_t slot = 0;
  while (slot < g_handles.size() && g_handles[slot]) slot++;     // handles of destroyed samplers are reused
  if (slot == g_handles.size()) g_handles.push_back(sp); else g_handles[slot] = sp;
  *handle = (int)slot;
  return 0;
}

int potus_destroy(int handle) {
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  (void)hipSetDevice(sp->device);
  (void)hipStreamSynchronize(sp->stream);
  for (void *p : sp->allocs) (void)hipFree(p);
  if (sp->lap_rows) (void)hipFree(sp->lap_rows);
  if (sp->pf_rows) (void)hipFree(sp->pf_rows);
  if (sp->vi_rows) (void)hipFree(sp->vi_rows);
  (void)hipEventDestroy(sp->ev0); (void)hipEventDestroy(sp->ev1); (void)hipStreamDestroy(sp->stream);
  if (sp->mv0) (void)hipEventDestroy(sp->mv0);
  if (sp->mv1) (void)hipEventDestroy(sp->mv1);
  for (int k = 0; k < Sampler::DN_AHEAD; k++) { if (sp->rv0[k]) (void)hipEventDestroy(sp->rv0[k]); if (sp->rv1[k]) (void)hipEventDestroy(sp->rv1[k]); if (sp->rdone[k]) (void)hipEventDestroy(sp->rdone[k]); }
  if (sp->h_active) (void)hipHostFree(sp->h_active);
  { std::lock_guard<std::mutex> lk(g_mu); g_handles[handle] = nullptr; }
  delete sp;
  return 0;
}

int potus_cus_per_chain(int handle, int *k) {
  Sampler *sp = get(handle);
  if (!sp || !k) return fail(POTUS_ERR_STATE, "bad handle");
  *k = sp->K;
  return 0;
}

int potus_clusters_per_chain(int handle, int *n) {
  Sampler *sp = get(handle);
  if (!sp || !n) return fail(POTUS_ERR_STATE, "bad handle");
  *n = sp->sides();
  return 0;
}

int potus_log_prob_grad(int handle, const double *q, int n, double *lp, double *grad) {
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  if (n < 0 || (n > 0 && (!q || !lp || !grad))) return fail(POTUS_ERR_ARG, "null argument");
  if (n == 0) return 0;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  const size_t D = sp->L.D;
  DevBufs tmp;
  double *dq = nullptr, *dlp = nullptr, *dg = nullptr;
  HIP_TRY(tmp.alloc(&dq, n * D * 8)); HIP_TRY(tmp.alloc(&dg, n * D * 8)); HIP_TRY(tmp.alloc(&dlp, (size_t)n * 8));
  HIP_TRY(hipMemcpyAsync(dq, q, n * D * 8, hipMemcpyHostToDevice, sp->stream));
  double *dscr = nullptr;
  if (sp->K > 1) {   // the cluster's own pass, on one cluster
    HIP_TRY(tmp.alloc(&dscr, 2 * (size_t)sp->R.Dpad * 8));
    const unsigned lid = ++sp->launch_id;
#define POTUS_CALL(TAG) hipLaunchKernelGGL(k_cl_logprob_grad<TAG>, dim3(sp->K), dim3(PT_THREADS), sp->cl_lds_bytes, sp->stream, (const DevModel *)sp->dM, \
                                           (const ClModel *)sp->dCL, (const RunParams *)sp->dR, (const double *)dq, dlp, dg, n, dscr, lid)
    CL_DISPATCH(sp->cl_dw, POTUS_CALL);
#undef POTUS_CALL
  } else {
    const int grid = std::min(n, 1024);
    hipLaunchKernelGGL(k_logprob_grad, dim3(grid), dim3(PT_THREADS), sp->lds_bytes, sp->stream, (const DevModel *)sp->dM, (const double *)dq, dlp, dg, n);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(lp, dlp, (size_t)n * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipMemcpyAsync(grad, dg, n * D * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

int potus_init(int handle, const double *q0) {
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  DevBufs tmp;
  double *dq0 = nullptr;
  const size_t bytes = (size_t)sp->R.chains * sp->L.D * 8;
  if (q0) { HIP_TRY(tmp.alloc(&dq0, bytes)); HIP_TRY(hipMemcpyAsync(dq0, q0, bytes, hipMemcpyHostToDevice, sp->stream)); }
  if (sp->K > 1) {
    const unsigned lid = ++sp->launch_id;
#define POTUS_CALL(TAG) hipLaunchKernelGGL(k_cl_init<TAG>, dim3(sp->R.chains * sp->K * sp->sides()), dim3(PT_THREADS), sp->cl_lds_bytes, sp->stream, (const DevModel *)sp->dM, \
                                           (const ClModel *)sp->dCL, (const RunParams *)sp->dR, (const double *)dq0, lid)
    CL_DISPATCH(sp->cl_dw, POTUS_CALL);
#undef POTUS_CALL
  } else if (sp->n_ds)
    hipLaunchKernelGGL(k_init_ds, dim3(sp->R.chains), dim3(PT_THREADS), sp->lds_bytes, sp->stream, (const DevModel *)sp->dMs, (const RunParams *)sp->dR, (const double *)dq0,
                       sp->chains_per_ds());
  else
    hipLaunchKernelGGL(k_init, dim3(sp->R.chains * sp->sides()), dim3(PT_THREADS), sp->lds_bytes, sp->stream, (const DevModel *)sp->dM, (const RunParams *)sp->dR, (const double *)dq0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(sp->stream));
  {
    const int rc_ = check_chains(sp);
    if (rc_ == POTUS_ERR_INIT && q0) {   // a user's point is tried once: say so instead of "after 100 attempts"
      const std::string chain = g_err.substr(0, g_err.find(':'));
      return fail(POTUS_ERR_INIT, "%s: the initial point handed in has no finite log density and gradient (Stan: \"Rejecting initial value\")", chain.c_str());
    }
    if (rc_) return rc_;
  }
  if (sp->dense) { const int rc_ = dense_import_init(sp); if (rc_) return rc_; }
  sp->inited = true;
  return 0;
}

namespace {
// potus_run in two halves, so that several samplers can be in flight at once
struct RunTicket { Sampler *sp; int handle; long long before; int it0; };
int run_launch(RunTicket &t, int n_iter) {
  Sampler *sp = t.sp;
  HIP_TRY(hipSetDevice(sp->device));
  potus_total_leapfrogs(t.handle, &t.before);
  potus_iterations_done(t.handle, &t.it0);
  HIP_TRY(hipEventRecord(sp->ev0, sp->stream));
  if (sp->dense) {   // a sequence of chip-wide launches driven from here (potus_dense.hpp); it ends synchronised
    const int rc = dense_run(sp, n_iter);
    if (rc) return rc;
  } else if (sp->K > 1) {
    const unsigned lid = ++sp->launch_id;
    const dim3 grid((unsigned)(sp->R.chains * sp->K * sp->sides()));
    const DevModel *dM = sp->dM; const ClModel *dCL = sp->dCL; const RunParams *dR = sp->dR;
#define POTUS_CALL(TAG) do { if (sp->twin) hipLaunchKernelGGL((k_cl_run<TAG, true>), grid, dim3(PT_THREADS), sp->cl_lds_bytes, sp->stream, dM, dCL, dR, n_iter, lid); \
                             else hipLaunchKernelGGL((k_cl_run<TAG, false>), grid, dim3(PT_THREADS), sp->cl_lds_bytes, sp->stream, dM, dCL, dR, n_iter, lid); } while (0)
    CL_DISPATCH(sp->cl_dw, POTUS_CALL);
#undef POTUS_CALL
  } else if (sp->twin)
    hipLaunchKernelGGL(k_run_twin, dim3(2 * sp->R.chains), dim3(PT_THREADS), sp->lds_bytes, sp->stream, (const DevModel *)sp->dM, (const RunParams *)sp->dR, n_iter,
                       ++sp->launch_id);
  else if (sp->n_ds)
    hipLaunchKernelGGL(k_run_ds, dim3(sp->R.chains), dim3(PT_THREADS), sp->lds_bytes, sp->stream, (const DevModel *)sp->dMs, (const RunParams *)sp->dR, n_iter,
                       sp->chains_per_ds());
  else
    hipLaunchKernelGGL(k_run, dim3(sp->R.chains), dim3(PT_THREADS), sp->lds_bytes, sp->stream, (const DevModel *)sp->dM, (const RunParams *)sp->dR, n_iter);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(sp->ev1, sp->stream));
  return 0;
}
int run_finish(RunTicket &t) {
  Sampler *sp = t.sp;
  HIP_TRY(hipSetDevice(sp->device));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, sp->ev0, sp->ev1));
  long long after = 0;
  potus_total_leapfrogs(t.handle, &after);
  sp->last_ms = ms; sp->last_leapfrogs = after - t.before;
  int it1 = 0; potus_iterations_done(t.handle, &it1);
  // split elapsed time between warm-up and sampling in proportion to iterations (for the CSV footer)
  const int nw = sp->R.num_warmup;
  const int w_it = std::max(0, std::min(it1, nw) - std::min(t.it0, nw)), tot = std::max(1, it1 - t.it0);
  sp->warm_ms += ms * w_it / tot; sp->samp_ms += ms * (tot - w_it) / tot;
  return check_chains(sp);
}
} // namespace

int potus_run(int handle, int n_iter) {
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  if (!sp->inited) return fail(POTUS_ERR_STATE, "potus_init must be called before potus_run");
  if (n_iter <= 0) return 0;
  // launches are serialised per process: a cluster launch must find its compute units free, also of the
  // workgroups of a one-workgroup-per-chain sampler
  DeviceLocks lock(sp->device);
  RunTicket t{sp, handle, 0, 0};
  int rc = run_launch(t, n_iter);
  if (rc) return rc;
  return run_finish(t);
}

// Several samplers at once (the three backtests of BASELINE configs[3] on one GPU, or the shards of one posterior on
// the GPUs of a node, driven from a single host thread such as R's): all launches of a group are issued before any is
// waited for.  The workgroups of a cluster launch wait for each other, so every cluster launch in flight on a device
// must be resident in full: a group takes cluster samplers only while their workgroups fit the compute units of their
// device, XCD by XCD (workgroups are dealt round-robin to the eight XCDs); the rest runs in the next group.
int potus_run_many(const int *handles, int n_handles, int n_iter) {
  if (!handles || n_handles < 0) return fail(POTUS_ERR_ARG, "potus_run_many: null handle list");
  if (n_iter <= 0 || n_handles == 0) return 0;
  Pool P;   // (no chains are pooled here: handles with several data sets are welcome)
  if (const int rc_ = P.lookup(handles, n_handles, "potus_run_many")) return rc_;
  std::vector<RunTicket> todo;
  for (int i = 0; i < n_handles; i++) {
    if (!P.sps[i]->inited) return fail(POTUS_ERR_STATE, "potus_init must be called before potus_run_many");
    todo.push_back(RunTicket{P.sps[i], handles[i], 0, 0});
  }
  if (const int rc_ = P.distinct()) return rc_;
  DeviceLocks lock(P.devs);
  std::vector<char> done(todo.size(), 0);
  size_t n_done = 0;
  while (n_done < todo.size()) {
    std::vector<size_t> group;
    struct Use { int device, rows, plain; };   // XCD rows held by clusters; one-workgroup samplers in the group
    std::vector<Use> used;
    for (size_t i = 0; i < todo.size(); i++) {
      if (done[i]) continue;
      Sampler *sp = todo[i].sp;
      auto it = std::find_if(used.begin(), used.end(), [&](const Use &u) { return u.device == sp->device; });
      if (sp->dense) {   // chip-wide launches driven by the host: a group of its own
        if (!group.empty()) continue;
        group.push_back(i);
        break;
      }
      if (sp->coop()) {
        int ncu = 0;
        HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, sp->device));
        const int rows = (sp->R.chains * sp->K * sp->sides() + 7) / 8, cap = ncu / 8;
        if (it != used.end() && (it->plain > 0 || it->rows + rows > cap)) continue;   // next group (a sampler alone always fits: checked at create)
        if (it == used.end()) used.push_back({sp->device, rows, 0}); else it->rows += rows;
      } else {
        // a one-workgroup-per-chain launch may hold every compute unit for seconds: never beside a cluster
        if (it != used.end() && it->rows > 0) continue;
        if (it == used.end()) used.push_back({sp->device, 0, 1}); else it->plain += 1;
      }
      group.push_back(i);
    }
    int rc = 0;
    size_t launched = 0;
    for (; launched < group.size() && !rc; launched++) rc = run_launch(todo[group[launched]], n_iter);
    for (size_t k = 0; k < launched; k++) { const int r2 = run_finish(todo[group[k]]); if (!rc) rc = r2; }
    if (rc) return rc;
    for (size_t gi : group) { done[gi] = 1; n_done++; }
  }
  return 0;
}

int potus_iterations_done(int handle, int *n) {
  Sampler *sp = get(handle);
  if (!sp || !n) return fail(POTUS_ERR_STATE, "bad handle");
  HIP_TRY(hipSetDevice(sp->device));
  std::vector<ChainScalars> sc;
  { const int rc_ = read_scalars(sp, sc); if (rc_) return rc_; }
  int m = -1;   // (many data sets: over the chains that have not failed)
  for (auto &s : sc) if (!sp->n_ds || s.status == 0) m = m < 0 ? s.iter : std::min(m, s.iter);
  *n = std::max(m, 0);
  return 0;
}

int potus_total_leapfrogs(int handle, long long *n) {
  Sampler *sp = get(handle);
  if (!sp || !n) return fail(POTUS_ERR_STATE, "bad handle");
  HIP_TRY(hipSetDevice(sp->device));
  std::vector<ChainScalars> sc;
  { const int rc_ = read_scalars(sp, sc); if (rc_) return rc_; }
  long long t = 0;
  for (auto &s : sc) t += s.total_leapfrogs;
  *n = t;
  return 0;
}

int potus_twin_stats(int handle, long long *counted, long long *run_backward, long long *run_forward) {
  Sampler *sp = get(handle);
  if (!sp || !counted || !run_backward || !run_forward) return fail(POTUS_ERR_STATE, "bad handle");
  if (!sp->twin) return fail(POTUS_ERR_STATE, "potus_twin_stats: the handle runs one cluster per chain");
  HIP_TRY(hipSetDevice(sp->device));
  std::vector<ChainScalars> all((size_t)sp->R.chains * sp->K * 2);
  HIP_TRY(hipMemcpy(all.data(), sp->R.scal, sizeof(ChainScalars) * all.size(), hipMemcpyDeviceToHost));
  *counted = *run_backward = *run_forward = 0;
  for (int c = 0; c < sp->R.chains; c++) {
    *counted += all[(size_t)c * sp->K].total_leapfrogs;
    *run_backward += all[(size_t)c * sp->K].leaves_run;
    *run_forward += all[((size_t)sp->R.chains + c) * sp->K].leaves_run;
  }
  return 0;
}

int potus_chain_status(int handle, int *status, int *n_divergent) {
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  HIP_TRY(hipSetDevice(sp->device));
  std::vector<ChainScalars> sc;
  { const int rc_ = read_scalars(sp, sc); if (rc_) return rc_; }
  for (int c = 0; c < sp->R.chains; c++) { if (status) status[c] = sc[c].status; if (n_divergent) n_divergent[c] = sc[c].n_divergent; }
  return 0;
}

int potus_get_adaptation(int handle, double *stepsize, double *inv_metric) {
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  HIP_TRY(hipSetDevice(sp->device));
  std::vector<ChainScalars> sc;
  { const int rc_ = read_scalars(sp, sc); if (rc_) return rc_; }
  for (int c = 0; c < sp->R.chains; c++) {
    if (stepsize) stepsize[c] = sc[c].nom_eps;
    if (inv_metric && sp->dense) {   // the diagonal of the dense inverse metric
      HIP_TRY(hipMemcpy(inv_metric + (size_t)c * sp->L.D, dn_diag(sp->dn, c), (size_t)sp->L.D * 8, hipMemcpyDeviceToHost));   // (pooled: the one diagonal for every chain)
    } else if (inv_metric) {
      double *dst = inv_metric + (size_t)c * sp->L.D;
      if (sp->K == 1) HIP_TRY(hipMemcpy(dst, sp->R.state + ((size_t)c * V_COUNT + V_MINV) * sp->R.Dpad, (size_t)sp->L.D * 8, hipMemcpyDeviceToHost));
      if (sp->K > 1) {   // the cluster keeps its vectors in internal order (with padding)
        std::vector<double> tmp(sp->CL.Dint);
        HIP_TRY(hipMemcpy(tmp.data(), sp->R.state + ((size_t)c * V_COUNT + V_MINV) * sp->R.Dpad, (size_t)sp->CL.Dint * 8, hipMemcpyDeviceToHost));
        for (int i = 0; i < sp->CL.Dint; i++) if (sp->h_perm[i] >= 0) dst[sp->h_perm[i]] = tmp[i];
      }
    }
  }
  return 0;
}

int potus_get_dense_metric(int handle, int chain, double *inv_metric) {
  Sampler *sp = get(handle);
  if (!sp || !inv_metric) return fail(POTUS_ERR_STATE, "bad handle or null output");
  if (chain < 0 || chain >= sp->R.chains) return fail(POTUS_ERR_ARG, "chain %d out of range", chain);
  if (!sp->dense) return fail(POTUS_ERR_STATE, "the handle runs the diagonal metric: use potus_get_adaptation");
  HIP_TRY(hipSetDevice(sp->device));
  const size_t D = sp->L.D;
  // the strict upper triangle of the chain's matrix is M^-1's (the lower one holds its Cholesky factor), the diagonal a vector
  if (sp->dn.f32 && !sp->dn.pooled) {   // the upper triangle lives as floats in the second half of each row (dn_f32_row); pooled: A holds the rounded values as doubles
    const size_t LD = sp->dn.LD, rows_at_once = 256;
    std::vector<double> buf(rows_at_once * LD);
    for (size_t r0 = 0; r0 < D; r0 += rows_at_once) {
      const size_t nr = std::min(rows_at_once, D - r0);
      HIP_TRY(hipMemcpy(buf.data(), sp->dn.A + ((size_t)chain * D + r0) * LD, nr * LD * 8, hipMemcpyDeviceToHost));
      for (size_t r = 0; r < nr; r++) {
        const float *f = dn_f32_row(buf.data(), (int)LD, (int)r);
        for (size_t j = r0 + r + 1; j < D; j++) inv_metric[(r0 + r) * D + j] = (double)f[j];
      }
    }
  } else
  HIP_TRY(hipMemcpy2D(inv_metric, D * 8, dn_mat(sp->dn, chain), (size_t)sp->dn.LD * 8, D * 8, D, hipMemcpyDeviceToHost));   // (pooled: every chain's is the handle's one)
  std::vector<double> dg(D);
  HIP_TRY(hipMemcpy(dg.data(), dn_diag(sp->dn, chain), D * 8, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < D; i++) {
    inv_metric[i * D + i] = dg[i];
    for (size_t j = 0; j < i; j++) inv_metric[i * D + j] = inv_metric[j * D + i];
  }
  return 0;
}

// Dense metric: time spent in the matrix passes (k_dn_symv + k_dn_symv_finish, HIP events on the sampler's stream), their number and
// the bytes of matrix they loaded (active chains x the upper-triangle tiles, about 4 D^2 per pass), since the handle was created.
int potus_dense_timing(int handle, double *matvec_ms, long long *passes, long long *bytes, long long *rounds) {
  Sampler *sp = get(handle);
  if (!sp || !sp->dense) return fail(POTUS_ERR_STATE, "bad handle or not a dense-metric sampler");
  if (matvec_ms) *matvec_ms = sp->mv_ms;
  if (passes) *passes = sp->mv_calls;
  if (bytes) {   // (chain, pass) pairs counted by the timed passes themselves x the bytes a pass loads per chain
    unsigned long long np_ = 0;
    DeviceGuard guard;
    DeviceLocks lock(sp->device);
    HIP_TRY(hipSetDevice(sp->device));
    HIP_TRY(hipMemcpy(&np_, sp->dn.act_passes, 8, hipMemcpyDeviceToHost));
    *bytes = (long long)np_ * sp->dn_pass_bytes[sp->dn.rb == DN_RB ? 0 : 1];
  }
  if (rounds) *rounds = sp->dn_rounds;
  return 0;
}

// Dense metric: what the window ends of the warm-up have cost so far -- milliseconds in the covariance, in the blocked Cholesky
// factorisation and in the init_stepsize that follows (host clock around synchronised sections), and their number.
int potus_dense_adapt_timing(int handle, double *cov_ms, double *chol_ms, double *init_stepsize_ms, int *window_ends) {
  Sampler *sp = get(handle);
  if (!sp || !sp->dense) return fail(POTUS_ERR_STATE, "bad handle or not a dense-metric sampler");
  if (cov_ms) *cov_ms = sp->we_cov_ms;
  if (chol_ms) *chol_ms = sp->we_chol_ms;
  if (init_stepsize_ms) *init_stepsize_ms = sp->we_eps_ms;
  if (window_ends) *window_ends = sp->we_count;
  return 0;
}

// pooled_metric = 2: the window end in two halves, so that the host can pool over handles and ranks in between.  potus_run stops after the transition that ends
// a window (potus_iterations_done says where); *pending = 1 then, *count = the draws behind the handle's moments (chains x window length), *mean_dev /
// *m2_dev = DEVICE pointers to the handle's mean [D] and M2 = sum of centred outer products [D rows of *ld doubles, both triangles] -- the host replaces M2 by the
// pooled one (Chan's update: M2 += count (mean - pooled mean)(mean - pooled mean)', then the sum over everybody; us_potus_model_amd/parallel.py) and calls
// potus_dense_pool_finish with the pooled count: M^-1 = N/(N+5) M2/(N-1) + 1e-3 5/(N+5) I, its factor, init_stepsize.  With one handle and nothing in between,
// finish(count) is exactly pooled_metric = 1.
int potus_dense_pool_window(int handle, int *pending, double *count, void **mean_dev, void **m2_dev, long long *ld) {
  Sampler *sp = get(handle);
  if (!sp || !pending) return fail(POTUS_ERR_STATE, "bad handle or null output");
  if (!sp->dense || !sp->dn.pooled) return fail(POTUS_ERR_STATE, "potus_dense_pool_window: the handle does not run a pooled dense metric");
  *pending = sp->dn_pending ? 1 : 0;
  if (count) *count = sp->dn_pending ? (double)sp->R.chains * (double)sp->dn_pending_n : 0.0;
  if (mean_dev) *mean_dev = sp->dn.pmean;
  if (m2_dev) *m2_dev = sp->dn.A;
  if (ld) *ld = sp->dn.LD;
  return 0;
}
int potus_dense_pool_finish(int handle, double n_total) {
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  if (!sp->dense || !sp->dn.pooled || !sp->dn_pending) return fail(POTUS_ERR_STATE, "potus_dense_pool_finish: no pooled window end is pending on this handle");
  if (!(n_total >= (double)sp->R.chains * (double)sp->dn_pending_n)) return fail(POTUS_ERR_ARG, "potus_dense_pool_finish: the pooled count cannot be below the handle's own %d x %d draws", sp->R.chains, sp->dn_pending_n);
  DeviceGuard guard;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  sp->dn_pending = false;
  const int rc = dense_window_finish(sp, sp->dn_pending_n, sp->dn_pending_iter, n_total, sp->dn_pending_cov_ms);   // (the time between the halves is the host's)
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return check_chains(sp);
}

// Dense metric, verification hook (like potus_log_prob_grad): is the factor in the lower triangle the factor of the metric the
// leapfrog multiplies with?  For n_probe standard-normal vectors x: M^-1 x by the sampler's own matrix pass (upper triangle +
// diagonal, fp64 or fp32 storage) against L (L' x) by plain kernels over the lower triangle; and the momentum draw's own blocked
// back substitution L' p = u, checked by multiplying back.  out[0] = max ||L L' x - M^-1 x|| / ||M^-1 x||, out[1] = ||L' p - u|| / ||u||.
int potus_dense_check(int handle, int chain, int n_probe, double *out) {
  Sampler *sp = get(handle);
  if (!sp || !out) return fail(POTUS_ERR_STATE, "bad handle or null output");
  if (!sp->dense) return fail(POTUS_ERR_STATE, "the handle runs the diagonal metric");
  if (chain < 0 || chain >= sp->R.chains || n_probe < 1) return fail(POTUS_ERR_ARG, "potus_dense_check: bad chain or probe count");
  if (!sp->inited) return fail(POTUS_ERR_STATE, "potus_dense_check: call potus_init first (the check runs the sampler's kernels on the chain's state block)");
  DeviceGuard guard;                                   // the caller's device comes back
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  {
    int failed = 0;
    HIP_TRY(hipMemcpy(&failed, sp->dn.fail, 4, hipMemcpyDeviceToHost));
    if (failed) return fail(POTUS_ERR_STATE, "potus_dense_check: the last window end did not produce a factor (the adapted covariance was not positive definite)");
  }
  DnParams &P = sp->dn;
  P.count_passes = 0;                                  // verification passes are not part of potus_dense_timing's set
  const int D = P.D, chains = P.chains;
  std::vector<DnRound> rds(chains);
  for (int c = 0; c < chains; c++) { std::memset(&rds[c], 0, sizeof(DnRound)); rds[c].active = c == chain; }
  rds[chain].job[0] = DnJob{DV_TMPP, DV_SCR1, -1, -1, -1, 0, 0.0};              // SCR1 = M^-1 TMPP
  HIP_TRY(hipMemcpyAsync(P.rd, rds.data(), rds.size() * sizeof(DnRound), hipMemcpyHostToDevice, sp->stream));
  for (int c = 0; c < chains; c++) sp->h_active[c] = c == chain;
  std::vector<double> a(D), b(D);
  auto fetch = [&](int slot, std::vector<double> &v) {
    return hipMemcpyAsync(v.data(), P.state + ((size_t)chain * DV_COUNT + slot) * P.LD, (size_t)D * 8, hipMemcpyDeviceToHost, sp->stream);
  };
  out[0] = out[1] = 0.0;
  for (int k = 0; k <= n_probe; k++) {
    // standard normals -> P0; the last round solves L' p = u with the sampler's kernels and multiplies back
    const bool solve = k == n_probe;
    rds[chain].aux = k;
    HIP_TRY(hipMemcpyAsync(&P.rd[chain].aux, &rds[chain].aux, sizeof(int), hipMemcpyHostToDevice, sp->stream));
    const int id0 = P.identity;
    if (!solve) P.identity = 1;                                                  // (dense_sample_p: normals only)
    const int rc = dense_sample_p(sp, 0x7ffffff0u, RNG_INIT_EPS);
    P.identity = id0;
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(P.state + ((size_t)chain * DV_COUNT + DV_TMPP) * P.LD, P.state + ((size_t)chain * DV_COUNT + DV_P0) * P.LD, (size_t)D * 8,
                           hipMemcpyDeviceToDevice, sp->stream));
    hipLaunchKernelGGL(k_dn_chk_ltx, dim3((D + 255) / 256), dim3(256), 0, sp->stream, P, chain, (int)DV_TMPP, (int)DV_TMPQ);   // TMPQ = L' TMPP
    if (solve) {
      P.identity = 1;
      const int rc2 = dense_sample_p(sp, 0x7ffffff0u, RNG_INIT_EPS);            // the same normals again: u
      P.identity = id0;
      if (rc2) return rc2;
      HIP_TRY(fetch(DV_TMPQ, a)); HIP_TRY(fetch(DV_P0, b));
    } else {
      hipLaunchKernelGGL(k_dn_chk_lx, dim3(D), dim3(256), 0, sp->stream, P, chain, (int)DV_TMPQ, (int)DV_SCR0);                 // SCR0 = L L' x
      DnActive act; act.n = 1; act.idx[0] = chain;
      dense_launch_shape(P, 1);
      dense_symv_launch(sp->stream, P, act, 1);
      HIP_TRY(fetch(DV_SCR0, a)); HIP_TRY(fetch(DV_SCR1, b));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(sp->stream));
    double num = 0, den = 0;
    for (int i = 0; i < D; i++) { num += (a[i] - b[i]) * (a[i] - b[i]); den += b[i] * b[i]; }
    const double rel = std::sqrt(num / std::max(den, 1e-300));
    if (solve) out[1] = rel; else out[0] = std::max(out[0], rel);
  }
  return 0;
}

int potus_get_draws(int handle, double *out, int *n_saved) {
  Sampler *sp = get(handle);
  if (!sp || !n_saved) return fail(POTUS_ERR_STATE, "bad handle");
  HIP_TRY(hipSetDevice(sp->device));
  int rc = saved_count(sp, n_saved);
  if (rc) return rc;
  if (out) {
    for (int c = 0; c < sp->R.chains; c++)
      HIP_TRY(hipMemcpy(out + (size_t)c * *n_saved * sp->R.row, sp->R.draws + (size_t)c * sp->R.n_save_max * sp->R.row,
                        (size_t)*n_saved * sp->R.row * 8, hipMemcpyDeviceToHost));
  }
  return 0;
}

int potus_draws_device_ptr(int handle, void **dptr, long long *n_doubles) {
  Sampler *sp = get(handle);
  if (!sp || !dptr) return fail(POTUS_ERR_STATE, "bad handle");
  *dptr = sp->R.draws;
  if (n_doubles) *n_doubles = (long long)sp->R.chains * sp->R.n_save_max * sp->R.row;
  return 0;
}

static RowSrc row_src(const Sampler *sp, int first) { return RowSrc{sp->R.draws, sp->R.chains, sp->R.n_save_max, sp->R.row, first}; }   // a handle's saved draws
// One row-builder launch on the sampler's stream: the W.n_saved x W.src.chains rows of W.src.  The CALLER chooses the kernel: per_ds = 0 builds every row
// with the one model M (k_write_array), per_ds > 0 builds chain c's rows with M[c / per_ds] (k_write_array_ds).  The grid and W.scratch are owned here;
// W.out is the caller's or, when null, comes from tmp too.  Allocations fail by the name `what` (DevBufs::get), or with what = null as HIP calls fail.
static int launch_rows(Sampler *sp, DevBufs &tmp, const char *what, const DevModel *M, int per_ds, WAParams &W) {
  const int n = W.n_saved * W.src.chains, nsel = W.col_end - W.col_begin, grid = std::min(n, 512);
  double *scratch = nullptr, *dout = W.out;
  if (what) {
    if (const int rc_ = tmp.get(&scratch, (size_t)grid * sp->L.ncols * 8, what)) return rc_;
    if (!dout) if (const int rc_ = tmp.get(&dout, (size_t)n * nsel * 8, what)) return rc_;
  } else {
    HIP_TRY(tmp.alloc(&scratch, (size_t)grid * sp->L.ncols * 8));
    if (!dout) HIP_TRY(tmp.alloc(&dout, (size_t)n * nsel * 8));
  }
  W.scratch = scratch; W.out = dout;
  if (per_ds) hipLaunchKernelGGL(k_write_array_ds, dim3(grid), dim3(256), 0, sp->stream, M, W, per_ds);
  else hipLaunchKernelGGL(k_write_array, dim3(grid), dim3(256), 0, sp->stream, M, W);
  HIP_TRY(hipGetLastError());
  return 0;
}

// out: host buffer, or (device_out) a device buffer of the sampler's GPU that receives the rows directly
static int write_array_range(Sampler *sp, int n_saved, int col_begin, int col_end, double *out, bool device_out = false, int out_stride = 0) {
  const int nsel = col_end - col_begin;
  if (out_stride <= 0) out_stride = nsel;
  const int ndraw = n_saved * sp->R.chains;
  if (ndraw == 0) return 0;
  DevBufs tmp;
  WAParams W{row_src(sp, 0), n_saved, sp->L.ncols, col_begin, col_end, nullptr, device_out ? out : nullptr, out_stride};
  if (const int rc_ = launch_rows(sp, tmp, "potus_write_array", sp->ds_ex ? sp->dMs : sp->dM, sp->ds_ex ? sp->chains_per_ds() : 0, W)) return rc_;   // ds_ex: the chain's own model
  if (!device_out) HIP_TRY(hipMemcpyAsync(out, W.out, (size_t)ndraw * nsel * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

int potus_write_array(int handle, int col_begin, int col_end, double *out) {
  Sampler *sp = get(handle);
  if (!sp || !out) return fail(POTUS_ERR_STATE, "bad handle or null output");
  if (const int rc_ = check_cols(sp, col_begin, col_end)) return rc_;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  int n_saved = 0, rc = saved_count(sp, &n_saved);
  if (rc) return rc;
  return write_array_range(sp, n_saved, col_begin, col_end, out);
}

// rstan::extract(out, pars)[[1]] as R stores it, in ONE pass and in place: `out` is a column-major matrix [rows, col_end - col_begin] whose row
// chain_global * n_saved + iteration holds a draw -- chains merged chain after chain, the handles' chains in the order listed (R/potus_sampling.R deals
// consecutive chain ids to consecutive handles).  *rows_out = the rows the listed handles hold (call with out = NULL to size the result); rows must equal it.
// What R's .Call() wrapper (R/src/potus_call.c) fills an allocVector'ed result with: no second copy in R, long vectors welcome (the .C() path hands R
// [iteration][chain][column] rows, which the shim then permutes -- two more copies of 0.83 GB for predicted_score of 8 x 1000 draws, final_2016.R:708).
__global__ __launch_bounds__(256) void k_rows_to_r_matrix(const double *in, double *out, int n_saved, int chains, int ncol) {
  // in [iteration][chain][column] -> out [column][chain][iteration]; tiles of 32 x 32 through LDS
  __shared__ double tile[32][33];
  const long long nrow = (long long)n_saved * chains;
  const long long r0 = (long long)blockIdx.x * 32;
  const int c0 = (int)blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const long long r = r0 + k;
    tile[k][tx] = (r < nrow && c0 + tx < ncol) ? in[r * ncol + c0 + tx] : 0.0;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const long long r = r0 + tx;                                   // source row = iteration * chains + chain
    if (r < nrow && c0 + k < ncol) {
      const long long it = r / chains, ch = r % chains;
      out[(long long)(c0 + k) * nrow + ch * n_saved + it] = tile[tx][k];
    }
  }
}
int potus_extract_matrix(const int *handles, int n_handles, int col_begin, int col_end, double *out, long long rows, long long *rows_out) {
  Pool P;
  if (const int rc_ = P.resolve(handles, n_handles, "potus_extract_matrix")) return rc_;
  for (const Sampler *sp : P.sps)   // (the columns alone: weaker than Pool::same_posterior)
    if (sp->L.ncols != P.s0->L.ncols) return fail(POTUS_ERR_ARG, "potus_extract_matrix: the handles hold different posteriors");
  if (const int rc_ = check_cols(P.s0, col_begin, col_end)) return rc_;
  DeviceGuard guard;
  DeviceLocks lock(P.devs);
  if (const int rc_ = P.count()) return rc_;
  if (const int rc_ = P.equal_counts()) return rc_;
  const std::vector<Sampler *> &sps = P.sps;
  const std::vector<int> &saved = P.saved;
  const long long total = P.draws;
  if (rows_out) *rows_out = total;
  if (!out) return 0;
  if (rows != total) return fail(POTUS_ERR_ARG, "potus_extract_matrix: the result has %lld rows, the handles hold %lld draws", rows, total);
  const int nsel = col_end - col_begin;
  long long off = 0;
  for (int i = 0; i < n_handles; i++) {
    Sampler *sp = sps[i];
    const long long nrow = (long long)saved[i] * sp->R.chains;
    if (nrow == 0) continue;
    HIP_TRY(hipSetDevice(sp->device));
    DevBufs tmp;
    double *rowsd = nullptr, *colsd = nullptr;
    int rc;
    if ((rc = tmp.get(&rowsd, (size_t)nrow * nsel * 8, P.what)) || (rc = tmp.get(&colsd, (size_t)nrow * nsel * 8, P.what))) return rc;
    if ((rc = write_array_range(sp, saved[i], col_begin, col_end, rowsd, true))) return rc;
    hipLaunchKernelGGL(k_rows_to_r_matrix, dim3((unsigned)((nrow + 31) / 32), (unsigned)((nsel + 31) / 32)), dim3(256), 0, sp->stream, rowsd, colsd, saved[i], sp->R.chains, nsel);
    HIP_TRY(hipGetLastError());
    // column k of this handle's block -> rows [off, off + nrow) of column k of the result
    HIP_TRY(hipMemcpy2DAsync(out + off, (size_t)total * 8, colsd, (size_t)nrow * 8, (size_t)nrow * 8, (size_t)nsel, hipMemcpyDeviceToHost, sp->stream));
    HIP_TRY(hipStreamSynchronize(sp->stream));
    off += nrow;
  }
  return 0;
}

// The same rows written straight into a DEVICE buffer of the sampler's GPU (e.g. a torch tensor's data_ptr()): what
// the RCCL all-gather of the draws-of-interest sends, without a trip through host memory.
int potus_write_array_device(int handle, int col_begin, int col_end, void *out_device) {
  Sampler *sp = get(handle);
  if (!sp || !out_device) return fail(POTUS_ERR_STATE, "bad handle or null output");
  if (const int rc_ = check_cols(sp, col_begin, col_end)) return rc_;
  DeviceBlock dev;
  if (const int rc_ = dev.open("potus_write_array_device", sp->device, out_device, "output")) return rc_;
  int n_saved = 0, rc = saved_count(sp, &n_saved);
  if (rc) return rc;
  return write_array_range(sp, n_saved, col_begin, col_end, (double *)out_device, true);
}

// Pooled over every saved draw of every listed sampler (the chains of one posterior may sit in several handles, on one
// GPU or several: PotusModel.sample(devices=...), potus_sampling.R gpus=...).  The work runs on the first handle's GPU;
// predicted_score blocks of other GPUs are brought over with a peer copy.  Any number of draws (potus_summary.hpp).
int potus_posterior_summary_many(const int *handles, int n_handles, const double *ev, double *state_out, double *natl_out, double *ev_out) {
  if (!handles || n_handles < 1 || !ev || !state_out || !natl_out || !ev_out) return fail(POTUS_ERR_ARG, "potus_posterior_summary: null argument");
  Pool P;
  if (const int rc_ = P.resolve(handles, n_handles, "potus_posterior_summary")) return rc_;
  // (the first handle's state weights are the ones the national vote is taken with)
  if (const int rc_ = P.same_posterior("pooled summaries are for the chains of one")) return rc_;
  DeviceGuard guard;                                   // whatever happens below, the caller's device comes back
  DeviceLocks lock(P.devs);
  if (const int rc_ = P.count()) return rc_;           // (the handles may have saved different numbers of draws: every one of them is pooled)
  Sampler *s0 = P.s0;
  const long long nd = P.draws;
  const int S = s0->M.S, T = s0->M.T, TS = S * T, NC = TS + 2 * T;
  if (nd < 2) return fail(POTUS_ERR_STATE, "posterior summaries need at least two saved draws");
  const int col_end = s0->L.ncols, col_begin = row_cols(s0->M).predicted_score;   // the generated-quantities block
  HIP_TRY(hipSetDevice(s0->device));
  DevBufs tmp;
  double *full = nullptr, *cols = nullptr, *dw = nullptr, *dev_ = nullptr, *dout = nullptr, *scr = nullptr;
  int rc;
  if ((rc = tmp.get(&full, (size_t)nd * NC * 8, P.what)) || (rc = tmp.get(&cols, (size_t)nd * NC * 8, P.what))) return rc;
  if ((rc = tmp.get(&dw, (size_t)S * 8, P.what)) || (rc = tmp.get(&dev_, (size_t)S * 8, P.what))) return rc;
  if ((rc = tmp.get(&dout, ((size_t)TS * 4 + (size_t)T * 9) * 8, P.what))) return rc;
  long long row0 = 0;
  for (int i = 0; i < n_handles; i++) {
    Sampler *sp = P.sps[i];
    const int n_saved = P.saved[i];
    const long long rows = (long long)n_saved * sp->R.chains;
    if (rows == 0) continue;
    if ((rc = gather_block(s0, sp, (size_t)rows * NC * 8, full + (size_t)row0 * NC,
                           [&](double *out) { return write_array_range(sp, n_saved, col_begin, col_end, out, true, NC); }))) return rc;
    row0 += rows;
  }
  HIP_TRY(hipMemcpyAsync(dw, s0->h_w.data(), (size_t)S * 8, hipMemcpyHostToDevice, s0->stream));
  HIP_TRY(hipMemcpyAsync(dev_, ev, (size_t)S * 8, hipMemcpyHostToDevice, s0->stream));
  hipLaunchKernelGGL(k_ps_derived, dim3((unsigned)std::min<long long>((nd * T + 255) / 256, 65535)), dim3(256), 0, s0->stream, full, nd, T, S,
                     (const double *)dw, (const double *)dev_);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_ps_transpose, dim3((NC + 63) / 64, (unsigned)((nd + 63) / 64)), dim3(256), 0, s0->stream, (const double *)full, cols, nd, NC);
  HIP_TRY(hipGetLastError());
  int npad = 1;
  while (npad < nd && npad < PS_RUN) npad <<= 1;
  const size_t lds = (size_t)npad * 8;
  const int grid = std::min(NC, 1024);
  if (nd > PS_RUN && (rc = tmp.get(&scr, (size_t)grid * (size_t)nd * 8, P.what))) return rc;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_col_summary), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  double *o_state = dout, *o_natl = dout + (size_t)TS * 4, *o_ev = o_natl + (size_t)T * 4;
  hipLaunchKernelGGL(k_col_summary, dim3(grid), dim3(PS_THREADS), lds, s0->stream, (const double *)cols, scr, nd, T, S, o_state, o_natl, o_ev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(state_out, o_state, (size_t)TS * 4 * 8, hipMemcpyDeviceToHost, s0->stream));
  HIP_TRY(hipMemcpyAsync(natl_out, o_natl, (size_t)T * 4 * 8, hipMemcpyDeviceToHost, s0->stream));
  HIP_TRY(hipMemcpyAsync(ev_out, o_ev, (size_t)T * 5 * 8, hipMemcpyDeviceToHost, s0->stream));
  HIP_TRY(hipStreamSynchronize(s0->stream));
  return 0;
}

int potus_posterior_summary(int handle, const double *ev, double *state_out, double *natl_out, double *ev_out) {
  return potus_posterior_summary_many(&handle, 1, ev, state_out, natl_out, ev_out);
}

// ---------------------------------------------------------------------------------------------- diagnostics (potus_diag.hpp)
namespace {
// cols [NC][C][n] on the current device -> rhat / bulk ESS per column (host arrays)
int diagnostics_of_columns(hipStream_t stream, const double *cols, long long n, int C, int NC, double *rhat_out, double *ess_out) {
  const char *what = "potus_diagnostics";
  if (2 * C > DG_MAXCH) return fail(POTUS_ERR_UNSUPPORTED, "%s: %d chains pooled (at most %d)", what, C, DG_MAXCH / 2);
  const long long N = 2ll * C * (n / 2);
  DevBufs tmp;
  double *zbuf = nullptr, *dout = nullptr;
  unsigned long long *rkey;
  unsigned *ridx;
  // a workgroup's scratch: two rank-normalised copies of the column, and the sorted runs when they do not fit LDS; the grid is
  // capped so that the scratch of a call stays within 768 MB whatever the number of pooled draws (a workgroup loops over columns)
  const long long per_wg = std::max<long long>(N, 1) * 16 + (long long)sorted_run_bytes(N);
  const int grid = (int)std::max<long long>(1, std::min<long long>(std::min(NC, 1024), (768ll << 20) / per_wg));
  int rc;
  if ((rc = tmp.get(&zbuf, (size_t)grid * 2 * (size_t)std::max<long long>(N, 1) * 8, what))) return rc;
  if ((rc = sorted_run_scratch(tmp, grid, N, &rkey, &ridx, what)) || (rc = tmp.get(&dout, (size_t)NC * 2 * 8, what))) return rc;
  const size_t lds = sorted_run_lds(N);                // keys + split indices
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dg_column), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  DgParams P{cols, zbuf, rkey, ridx, dout, dout + NC, n, C, NC};
  hipLaunchKernelGGL(k_dg_column, dim3(grid), dim3(DG_THREADS), lds, stream, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(rhat_out, dout, (size_t)NC * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(ess_out, dout + NC, (size_t)NC * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}
} // namespace

int potus_diagnostics_device(int device, const void *block, long long n_draws, int n_chains, int n_cols, double *rhat_out, double *ess_bulk_out) {
  if (!block || !rhat_out || !ess_bulk_out || n_draws < 1 || n_chains < 1 || n_cols < 1) return fail(POTUS_ERR_ARG, "potus_diagnostics_device: bad argument");
  if (2 * n_chains > DG_MAXCH) return fail(POTUS_ERR_UNSUPPORTED, "potus_diagnostics_device: %d chains pooled (at most %d)", n_chains, DG_MAXCH / 2);   // before anything is allocated
  DeviceBlock dev;
  if (const int rc_ = dev.open("potus_diagnostics_device", device, block)) return rc_;
  DevBufs tmp;
  double *cols = nullptr;
  if (const int rc_ = tmp.get(&cols, (size_t)n_draws * n_chains * n_cols * 8, "potus_diagnostics_device")) return rc_;
  if (const int rc_ = transpose_block(0, (const double *)block, cols, n_draws, n_chains, n_cols, n_chains, 0)) return rc_;
  return diagnostics_of_columns(0, cols, n_draws, n_chains, n_cols, rhat_out, ess_bulk_out);
}

// Columns [col_begin, col_end) of the post-warm-up draws of a counted pool, gathered handle by handle and transposed into cols [NC][chains][n_post] on
// the first handle's GPU (its device current on return)
static int gather_columns(const Pool &P, int col_begin, int col_end, int n_warm_rows, int n_post, double *cols) {
  Sampler *s0 = P.s0;
  const int Ctot = P.chains, n_saved = P.saved[0], NC = col_end - col_begin;
  int coff = 0;
  for (Sampler *sp : P.sps) {
    const int C = sp->R.chains;
    const size_t bytes = (size_t)n_saved * C * NC * 8;
    DevBufs blkbuf;
    double *blk = nullptr;
    int rc;
    if ((rc = blkbuf.get(&blk, bytes, P.what))) return rc;
    if ((rc = gather_block(s0, sp, bytes, blk, [&](double *out) { return write_array_range(sp, n_saved, col_begin, col_end, out, true, NC); }))) return rc;
    if ((rc = pool_transpose(s0, blk + (size_t)n_warm_rows * C * NC, cols, n_post, C, NC, Ctot, coff))) return rc;
    coff += C;
  }
  return 0;
}

// Days [day_begin, day_end) of predicted_score over the post-warm-up draws of a resolved pool of one posterior (Pool::same_posterior), counted here under
// the caller's locks: gathered handle by handle and cut into items [nd][n_days][S] on the first handle's GPU (its device current on return).  The handles may
// have saved different numbers of draws: every one of them is pooled.  Row order: as the handles saved them (row = saved draw x chain), one k_oc_days launch
// per handle; or (by_chain) CANONICAL, chain after chain in the order the handles are listed, each chain's draws in iteration order (the row order of
// potus_extract_matrix) -- one launch per chain.  extra_day >= 0: that day too, as a one-day block extra [nd][1][S] in the same order.
struct DayItems {
  DevBufs bufs;
  double *items = nullptr, *extra = nullptr;
  long long nd = 0;
  double gather_ms = 0.0, reshape_ms = 0.0;   // gather + produce, day-range reshape: summed over the handles
};
static int gather_days(Pool &P, int day_begin, int day_end, bool by_chain, int extra_day, DayItems &g) {
  Sampler *s0 = P.s0;
  const int S = s0->M.S, T = s0->M.T, TS = S * T, n_days = day_end - day_begin;
  if (day_begin < 0 || day_end > T || day_begin >= day_end) return fail(POTUS_ERR_ARG, "%s: days [%d, %d) of %d", P.what, day_begin, day_end, T);
  int rc;
  if ((rc = P.count())) return rc;
  std::vector<int> first(P.sps.size());
  for (size_t i = 0; i < P.sps.size(); i++) {
    first[i] = warm_rows(P.sps[i], P.saved[i]);
    g.nd += (long long)(P.saved[i] - first[i]) * P.sps[i]->R.chains;
  }
  if (g.nd < 1) return fail(POTUS_ERR_STATE, "%s needs at least one saved post-warm-up draw (%lld rows saved, all of them warm-up)", P.what, P.draws);
  const int col_end = s0->L.ncols, col_begin = row_cols(s0->M).predicted_score;   // the generated-quantities block
  HIP_TRY(hipSetDevice(s0->device));
  if ((rc = g.bufs.get(&g.items, (size_t)g.nd * n_days * S * 8, P.what))) return rc;
  if (extra_day >= 0 && (rc = g.bufs.get(&g.extra, (size_t)g.nd * S * 8, P.what))) return rc;
  long long row0 = 0;
  for (size_t i = 0; i < P.sps.size(); i++) {
    Sampler *sp = P.sps[i];
    const int n_saved = P.saved[i], C = sp->R.chains, nsplit = by_chain ? C : 1;
    const long long rows = (long long)(n_saved - first[i]) * C / nsplit;   // per launch
    if (rows == 0) continue;
    const size_t bytes = (size_t)n_saved * C * TS * 8;
    DevBufs blkbuf;
    double *blk = nullptr;
    if ((rc = blkbuf.get(&blk, bytes, P.what))) return rc;
    const double t0 = dn_now();
    if ((rc = gather_block(s0, sp, bytes, blk, [&](double *out) { return write_array_range(sp, n_saved, col_begin, col_end, out, true, TS); }))) return rc;
    const double t1 = dn_now();
    // launch c: the handle's post-warm-up rows (row = saved draw x chain) from row c on, nsplit rows apart -- all of them, or those of chain c
    for (int c = 0; c < nsplit; c++, row0 += rows) {
      const double *src = blk + ((size_t)first[i] * C + c) * TS;
      const unsigned gy = (unsigned)std::min<long long>(rows, 32768);
      hipLaunchKernelGGL(k_oc_days, dim3((n_days + 63) / 64, gy), dim3(256), 0, s0->stream, src, (long long)nsplit * TS, g.items + (size_t)row0 * n_days * S, rows, T, S, day_begin, day_end);
      HIP_TRY(hipGetLastError());
      if (g.extra) {
        hipLaunchKernelGGL(k_oc_days, dim3(1, gy), dim3(256), 0, s0->stream, src, (long long)nsplit * TS, g.extra + (size_t)row0 * S, rows, T, S, extra_day, extra_day + 1);
        HIP_TRY(hipGetLastError());
      }
    }
    HIP_TRY(hipStreamSynchronize(s0->stream));
    g.gather_ms += t1 - t0; g.reshape_ms += dn_now() - t1;
  }
  return 0;
}

// R-hat / bulk ESS of columns [col_begin, col_end) over the pooled post-warm-up draws of a counted pool, under the caller's locks
static int diagnostics_pooled(const Pool &P, int col_begin, int col_end, double *rhat_out, double *ess_bulk_out) {
  Sampler *s0 = P.s0;
  const int Ctot = P.chains, NC = col_end - col_begin;
  if (2 * Ctot > DG_MAXCH) return fail(POTUS_ERR_UNSUPPORTED, "potus_diagnostics: %d chains pooled (at most %d)", Ctot, DG_MAXCH / 2);
  int n_warm_rows = 0, n_post = 0;
  if (const int rc_ = P.post_warmup(&n_warm_rows, &n_post)) return rc_;
  HIP_TRY(hipSetDevice(s0->device));
  DevBufs tmp;
  double *cols = nullptr;
  if (const int rc_ = tmp.get(&cols, (size_t)n_post * Ctot * NC * 8, P.what)) return rc_;
  if (const int rc_ = gather_columns(P, col_begin, col_end, n_warm_rows, n_post, cols)) return rc_;
  return diagnostics_of_columns(s0->stream, cols, n_post, Ctot, NC, rhat_out, ess_bulk_out);
}

int potus_diagnostics(const int *handles, int n_handles, int col_begin, int col_end, double *rhat_out, double *ess_bulk_out) {
  if (!handles || n_handles < 1 || !rhat_out || !ess_bulk_out) return fail(POTUS_ERR_ARG, "potus_diagnostics: null argument");
  Pool P;
  if (const int rc_ = P.resolve(handles, n_handles, "potus_diagnostics")) return rc_;
  if (col_begin < 0 || col_end > P.s0->L.ncols || col_begin >= col_end) return fail(POTUS_ERR_ARG, "potus_diagnostics: columns [%d, %d) of %d", col_begin, col_end, P.s0->L.ncols);
  if (const int rc_ = P.same_posterior("R-hat / ESS pool the chains of one")) return rc_;
  DeviceGuard guard;
  DeviceLocks lock(P.devs);
  if (const int rc_ = P.count()) return rc_;
  if (const int rc_ = P.equal_counts()) return rc_;
  return diagnostics_pooled(P, col_begin, col_end, rhat_out, ess_bulk_out);
}

// ---------------------------------------------------------------------------------------------- PSIS-LOO (potus_loo.hpp)
namespace {
constexpr size_t LOO_BLOCK_BUDGET = 256ull << 20;   // a call's log-likelihood blocks (half) and PSIS scratch (half)
constexpr size_t LOO_ROW_BUDGET = 64ull << 20;      // k_loo_loglik's rebuilt output rows, per handle

// per handle: log C(n, y) of its polls in the model's order, and the row scratch of k_loo_loglik
struct LooRows { double *lc = nullptr, *scratch = nullptr; int grid = 1; };
int loo_rows_setup(Sampler *sp, long long ndraw, DevBufs &keep, LooRows &r, const char *what) {
  HIP_TRY(hipSetDevice(sp->device));
  const int Np = sp->M.Npoll, Npad = sp->M.Npad;
  std::vector<double> pd((size_t)2 * Npad), lc(std::max(Np, 1), 0.0);
  HIP_TRY(hipMemcpy(pd.data(), sp->M.pd, pd.size() * 8, hipMemcpyDeviceToHost));
  for (int i = 0; i < Np; i++) {
    const long double y = pd[i], n = pd[Npad + i];
    lc[i] = (double)(lgammal(n + 1) - lgammal(y + 1) - lgammal(n - y + 1));
  }
  int rc;
  if ((rc = keep.get(&r.lc, lc.size() * 8, what))) return rc;
  HIP_TRY(hipMemcpy(r.lc, lc.data(), lc.size() * 8, hipMemcpyHostToDevice));
  r.grid = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(ndraw, 512), (long long)(LOO_ROW_BUDGET / ((size_t)sp->L.ncols * 8))));
  return keep.get(&r.scratch, (size_t)r.grid * sp->L.ncols * 8, what);
}

// log-likelihoods of polls [b0, b1) of the handle's post-warm-up draws -> out [n_post][chains][b1 - b0], on the handle's device and stream
int loo_loglik(Sampler *sp, const LooRows &r, int first, int n_post, int b0, int b1, int integrate, double *out) {
  LlParams P{row_src(sp, first), sp->L.ncols, n_post, b0, b1, integrate, r.lc, r.scratch, out};
  hipLaunchKernelGGL(k_loo_loglik, dim3(r.grid), dim3(256), 0, sp->stream, (const DevModel *)sp->dM, P);
  HIP_TRY(hipGetLastError());
  return 0;
}

// polls per block: blocks of bytes_per_poll each within half the budget
int loo_block_polls(size_t bytes_per_poll, int n) {
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)n, LOO_BLOCK_BUDGET / 2 / std::max<size_t>(bytes_per_poll, 1)));
}

// PSIS-LOO of ll [NP][C][n] on the current device -> pointwise [NP][LOO_NPW] on the host (r_eff: host [NP] or null)
int loo_psis(hipStream_t st, const double *ll, int NP, int C, long long n, const double *r_eff, double *pw, const char *what) {
  const long long S = (long long)C * n;
  const int grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(NP, 1024), LOO_BLOCK_BUDGET / 2 / psis_work_bytes(S, 0)));
  DevBufs tmp;
  PsisWork W;
  double *dre = nullptr, *dout = nullptr;
  int rc;
  if ((rc = psis_work(tmp, grid, S, 0, W, what, {reinterpret_cast<const void *>(k_loo_psis)})) || (rc = tmp.get(&dout, (size_t)NP * LOO_NPW * 8, what))) return rc;
  if (r_eff) {
    if ((rc = tmp.get(&dre, (size_t)NP * 8, what))) return rc;
    HIP_TRY(hipMemcpyAsync(dre, r_eff, (size_t)NP * 8, hipMemcpyHostToDevice, st));
  }
  PsisParams P{ll, dre, W, dout, n, C, NP};
  hipLaunchKernelGGL(k_loo_psis, dim3(grid), dim3(DG_THREADS), sorted_run_lds(S), st, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(pw, dout, (size_t)NP * LOO_NPW * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

// [3][2] = (elpd_loo, p_loo, looic) x (sum, sqrt(N) sd) over the polls, in poll order
void loo_estimates(const double *pw, int N, double *est) {
  for (int k = 0; k < 3; k++) {
    double s = 0.0, q = 0.0;
    for (int i = 0; i < N; i++) s += pw[(size_t)i * LOO_NPW + k];
    const double m = s / N;
    for (int i = 0; i < N; i++) { const double d = pw[(size_t)i * LOO_NPW + k] - m; q += d * d; }
    est[2 * k] = s;
    est[2 * k + 1] = std::sqrt((double)N) * std::sqrt(q / (N - 1));
  }
}

int loo_check_r_eff(const double *r_eff, int n, const char *what) {
  for (int i = 0; r_eff && i < n; i++)
    if (!(std::isfinite(r_eff[i]) && r_eff[i] > 0)) return fail(POTUS_ERR_ARG, "%s: r_eff[%d] = %g (finite and > 0 expected)", what, i, r_eff[i]);
  return 0;
}
} // namespace

int potus_log_lik_device(int handle, int poll_begin, int poll_end, int integrate, void *out_device) {
  Sampler *sp = get(handle);
  if (!sp || !out_device) return fail(POTUS_ERR_STATE, "bad handle or null output");
  if (const int rc_ = refuse_many_datasets(sp, "potus_log_lik_device")) return rc_;
  if (integrate != 0 && integrate != 1) return fail(POTUS_ERR_ARG, "potus_log_lik_device: integrate = %d (0: plain, 1: noise coordinate integrated out)", integrate);
  const int Np = sp->M.Npoll;
  if (poll_begin < 0 || poll_end > Np || poll_begin >= poll_end) return fail(POTUS_ERR_ARG, "potus_log_lik_device: polls [%d, %d) of %d", poll_begin, poll_end, Np);
  DeviceBlock dev;
  if (const int rc_ = dev.open("potus_log_lik_device", sp->device, out_device, "output")) return rc_;
  int n_saved = 0, rc = saved_count(sp, &n_saved);
  if (rc) return rc;
  const int first = warm_rows(sp, n_saved), n_post = n_saved - first, C = sp->R.chains;
  if (n_post < 1) return fail(POTUS_ERR_STATE, "potus_log_lik_device: no post-warm-up draws saved (%d saved, %d of them warm-up)", n_saved, first);
  DevBufs keep;
  LooRows r;
  if ((rc = loo_rows_setup(sp, (long long)n_post * C, keep, r, "potus_log_lik_device"))) return rc;
  const int nb = loo_block_polls((size_t)n_post * C * 8, poll_end - poll_begin);
  double *blk = nullptr, *out = (double *)out_device;
  if ((rc = keep.get(&blk, (size_t)n_post * C * nb * 8, "potus_log_lik_device"))) return rc;
  for (int b0 = poll_begin; b0 < poll_end; b0 += nb) {
    const int b1 = std::min(b0 + nb, poll_end);
    if ((rc = loo_loglik(sp, r, first, n_post, b0, b1, integrate, blk))) return rc;
    if ((rc = transpose_block(sp->stream, blk, out + (size_t)(b0 - poll_begin) * C * n_post, n_post, C, b1 - b0, C, 0))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

int potus_loo_device(int device, const void *log_lik, int n_polls, int n_chains, long long n_draws, const double *r_eff, double *pointwise_out,
                     double *estimates_out) {
  if (!log_lik || !pointwise_out || !estimates_out || n_polls < 1 || n_chains < 1) return fail(POTUS_ERR_ARG, "potus_loo_device: bad argument");
  if (n_draws < 4) return fail(POTUS_ERR_ARG, "potus_loo_device: %lld draws per chain (at least 4)", n_draws);
  if (2 * n_chains > DG_MAXCH) return fail(POTUS_ERR_UNSUPPORTED, "potus_loo_device: %d chains pooled (at most %d)", n_chains, DG_MAXCH / 2);
  if ((long long)n_chains * n_draws > 0x7fffffffll) return fail(POTUS_ERR_UNSUPPORTED, "potus_loo_device: %lld draws per poll (at most 2^31 - 1)", (long long)n_chains * n_draws);
  if (const int rc_ = loo_check_r_eff(r_eff, n_polls, "potus_loo_device")) return rc_;
  DeviceBlock dev;
  if (const int rc_ = dev.open("potus_loo_device", device, log_lik)) return rc_;
  const int rc = loo_psis(0, (const double *)log_lik, n_polls, n_chains, n_draws, r_eff, pointwise_out, "potus_loo_device");
  if (rc) return rc;
  loo_estimates(pointwise_out, n_polls, estimates_out);
  return 0;
}

int potus_loo(const int *handles, int n_handles, int integrate, const double *r_eff, double *pointwise_out, double *estimates_out) {
  if (!handles || n_handles < 1 || !pointwise_out || !estimates_out) return fail(POTUS_ERR_ARG, "potus_loo: null argument");
  Pool P;
  if (const int rc_ = P.resolve(handles, n_handles, "potus_loo")) return rc_;
  if (const int rc_ = P.same_posterior("LOO pools the chains of one")) return rc_;
  const std::vector<Sampler *> &sps = P.sps;
  Sampler *s0 = P.s0;
  const int Np = s0->M.Npoll;
  if (integrate != 0 && integrate != 1) return fail(POTUS_ERR_ARG, "potus_loo: integrate = %d (0: plain, 1: noise coordinate integrated out)", integrate);
  if (Np < 1) return fail(POTUS_ERR_ARG, "potus_loo: the data hold no polls");
  if (const int rc_ = loo_check_r_eff(r_eff, Np, "potus_loo")) return rc_;
  DeviceGuard guard;
  DeviceLocks lock(P.devs);
  if (const int rc_ = P.count()) return rc_;
  if (const int rc_ = P.equal_counts()) return rc_;
  const int Ctot = P.chains;
  if (2 * Ctot > DG_MAXCH) return fail(POTUS_ERR_UNSUPPORTED, "potus_loo: %d chains pooled (at most %d)", Ctot, DG_MAXCH / 2);
  int first = 0, n_post = 0;
  if (const int rc_ = P.post_warmup(&first, &n_post)) return rc_;
  DevBufs keep;
  std::vector<LooRows> rows(sps.size());
  int rc;
  for (size_t i = 0; i < sps.size(); i++)
    if ((rc = loo_rows_setup(sps[i], (long long)n_post * sps[i]->R.chains, keep, rows[i], "potus_loo"))) return rc;
  const long long S = (long long)n_post * Ctot;
  const int nb = loo_block_polls((size_t)S * 16, Np);    // the pooled block, and one handle's block before its transpose
  HIP_TRY(hipSetDevice(s0->device));
  double *cols = nullptr;
  if ((rc = keep.get(&cols, (size_t)S * nb * 8, "potus_loo"))) return rc;
  for (int b0 = 0; b0 < Np; b0 += nb) {
    const int b1 = std::min(b0 + nb, Np), nbk = b1 - b0;
    int coff = 0;
    for (size_t i = 0; i < sps.size(); i++) {
      Sampler *sp = sps[i];
      const int C = sp->R.chains;
      const size_t bytes = (size_t)n_post * C * nbk * 8;
      DevBufs blkbuf;
      double *blk = nullptr;
      if ((rc = blkbuf.get(&blk, bytes, "potus_loo"))) return rc;
      if ((rc = gather_block(s0, sp, bytes, blk, [&](double *out) { return loo_loglik(sp, rows[i], first, n_post, b0, b1, integrate, out); }))) return rc;
      if ((rc = pool_transpose(s0, blk, cols, n_post, C, nbk, Ctot, coff))) return rc;
      coff += C;
    }
    if ((rc = loo_psis(s0->stream, cols, nbk, Ctot, n_post, r_eff ? r_eff + b0 : nullptr, pointwise_out + (size_t)b0 * LOO_NPW, "potus_loo"))) return rc;
  }
  loo_estimates(pointwise_out, Np, estimates_out);
  return 0;
}

// ---------------------------------------------------------------------------------------------- moment matching (potus_loo_mm.hpp)
extern "C++" {   // (a template and a function that returns a vector)
namespace {
constexpr size_t MM_PART_BUDGET = 128ull << 20;   // the chunk partials of one k_mm_moments launch
thread_local double g_mm_ms[4] = {0.0, 0.0, 0.0, 0.0};   // the calling thread's last call: passes, moments, PSIS, final (HIP events)

// What the stages work with: the model (a handle of one workgroup per chain), the pooled chains on its device, the scratch of the kernels.
struct MmCtx {
  const char *what = "";
  Sampler *mp = nullptr;
  hipStream_t st = nullptr;
  int C = 0, n = 0, D = 0, Dpad = 0, row = 0, ncols = 0, S = 0, pass_grid = 1, psis_grid = 1, maxB = 1;
  DevBufs keep;
  const double **dchain = nullptr;
  double *lc = nullptr, *scratch = nullptr, *part = nullptr, *mom = nullptr, *dre = nullptr, *dk = nullptr, *da = nullptr, *db = nullptr, *dm0 = nullptr;
  int *dpoll = nullptr, *dsel = nullptr;
  PsisWork psis{};
  MmPassParams *dP = nullptr;
  std::vector<int> model_index;   // poll as the output row numbers it -> the model's (day-sorted) index
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
  int nchunk() const { return (S + MM_CHUNK - 1) / MM_CHUNK; }
};

// the wording of potus_optimize / potus_cv_lpd for a handle that cannot run the one-workgroup pass
int mm_check_model(const char *what, const Sampler *mp) {
  if (mp->dense) return fail(POTUS_ERR_UNSUPPORTED, "%s: the dense metric is not supported (metric = POTUS_METRIC_DIAG only)", what);
  if (mp->K != 1 || mp->twin) return fail(POTUS_ERR_UNSUPPORTED, "%s: needs one workgroup per chain (cus_per_chain = 1, twin = 0); this handle runs %d x %d", what, mp->K, mp->sides());
  if (!mp->k1_unsupported.empty()) return fail(POTUS_ERR_UNSUPPORTED, "%s: %s", what, mp->k1_unsupported.c_str());
  if (mp->lds_bytes + sizeof(RowLds) > 160 * 1024) return fail(POTUS_ERR_UNSUPPORTED, "%s: the pass and the row builder need %zu bytes of LDS (> 160 KiB)", what, mp->lds_bytes + sizeof(RowLds));
  return refuse_many_datasets(mp, what);
}
int mm_check_sizes(const char *what, long long C, long long n, long long maxB) {
  if (C < 1 || n < 4) return fail(POTUS_ERR_ARG, "%s: %lld chains of %lld draws (at least one chain, four draws per chain)", what, C, n);
  if (2 * C > DG_MAXCH) return fail(POTUS_ERR_UNSUPPORTED, "%s: %lld chains pooled (at most %d)", what, C, DG_MAXCH / 2);
  // (k_mm_pass walks its items with an int that a stride of up to 2^16 workgroups must not overflow; k_mm_moments has one grid row per chunk of draws)
  if (C * n * std::max<long long>(maxB, 1) > 0x7fffffffll - 65536) return fail(POTUS_ERR_UNSUPPORTED, "%s: %lld polls x %lld draws in one launch (at most 2^31 - 2^16 items)", what, maxB, C * n);
  if ((C * n + MM_CHUNK - 1) / MM_CHUNK > 65535) return fail(POTUS_ERR_UNSUPPORTED, "%s: %lld pooled draws (at most %d: one grid row per %d draws)", what, C * n, 65535 * MM_CHUNK, MM_CHUNK);
  return 0;
}

// under the device lock, the model's device current: chains = the first post-warm-up row of every pooled chain (device pointers)
int mm_setup(MmCtx &x, const char *what, Sampler *mp, const std::vector<const double *> &chains, int n, int maxB) {
  x.what = what; x.mp = mp; x.st = mp->stream;
  x.C = (int)chains.size(); x.n = n; x.S = x.C * n; x.D = mp->L.D; x.Dpad = (x.D + 7) & ~7; x.row = POTUS_N_SAMPLER_COLS + x.D; x.ncols = mp->L.ncols;
  x.maxB = std::max(maxB, 1);
  int rc;
  LooRows lr;
  if ((rc = loo_rows_setup(mp, 1, x.keep, lr, what))) return rc;
  x.lc = lr.lc;
  const int Np = mp->M.Npoll, Npad = mp->M.Npad;
  std::vector<int> pi((size_t)6 * Npad);
  HIP_TRY(hipMemcpy(pi.data(), mp->M.pi, pi.size() * 4, hipMemcpyDeviceToHost));
  x.model_index.assign(Np, -1);
  for (int i = 0; i < Np; i++) {
    const int s = pi[i], qi = pi[(size_t)5 * Npad + i];
    const int k = s == mp->M.S ? mp->M.Ns + (qi - mp->M.o_nn) : qi - mp->M.o_ns;
    if (k >= 0 && k < Np) x.model_index[k] = i;
  }
  int ncu = 256;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, mp->device) == hipSuccess) ncu = std::max(1, prop.multiProcessorCount);
  x.pass_grid = (int)std::max<long long>(1, std::min<long long>((long long)x.maxB * x.S, 2ll * ncu));
  x.psis_grid = std::min(x.maxB, 1024);
  const size_t BD = (size_t)x.maxB * x.D;
  if ((rc = x.keep.get(&x.dchain, chains.size() * sizeof(double *), what)) || (rc = x.keep.get(&x.scratch, (size_t)x.pass_grid * mm_scratch_doubles(x.Dpad, x.ncols) * 8, what)) ||
      (rc = x.keep.get(&x.dP, sizeof(MmPassParams), what)) || (rc = x.keep.get(&x.da, BD * 8, what)) || (rc = x.keep.get(&x.db, BD * 8, what)) ||
      (rc = x.keep.get(&x.dm0, (size_t)x.D * 8, what)) || (rc = x.keep.get(&x.dpoll, (size_t)x.maxB * 4, what)) || (rc = x.keep.get(&x.dsel, (size_t)x.maxB * 4, what)) ||
      (rc = x.keep.get(&x.part, (size_t)x.nchunk() * BD * 2 * 8, what)) || (rc = x.keep.get(&x.mom, BD * 2 * 8, what)) ||
      (rc = psis_work(x.keep, x.psis_grid, x.S, 0, x.psis, what, {reinterpret_cast<const void *>(k_mm_psis)})) || (rc = x.keep.get(&x.dre, (size_t)x.maxB * 8, what)) || (rc = x.keep.get(&x.dk, (size_t)x.maxB * 8, what)))
    return rc;
  HIP_TRY(hipMemcpy(x.dchain, chains.data(), chains.size() * sizeof(double *), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(x.scratch, 0, (size_t)x.pass_grid * mm_scratch_doubles(x.Dpad, x.ncols) * 8));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mm_pass), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(mp->M.lds_doubles * 8 + sizeof(RowLds))));
  return 0;
}

// one stage's launches between two events; the stream is idle on return
template <class Launch>
int mm_timed(MmCtx &x, int stage, Launch launch) {
  EventTimer t;
  HIP_TRY(t.made);
  HIP_TRY(t.start(x.st));
  if (const int rc = launch()) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(t.stop(x.st));
  HIP_TRY(hipStreamSynchronize(x.st));
  double ms = 0.0;
  if (t.elapsed(&ms)) x.ms[stage] += ms;
  return 0;
}

// lp, ll [B][S] (device) of the polls (output numbering) at theta, T theta or T^-1 theta; a, b host [B][D]
int mm_pass(MmCtx &x, int B, const double *a, const double *b, const int *polls, const int *sel, int integrate, double *lp, double *ll) {
  std::vector<int> mi(B);
  for (int k = 0; k < B; k++) mi[k] = x.model_index[polls[k]];
  HIP_TRY(hipMemcpyAsync(x.da, a, (size_t)B * x.D * 8, hipMemcpyHostToDevice, x.st));
  HIP_TRY(hipMemcpyAsync(x.db, b, (size_t)B * x.D * 8, hipMemcpyHostToDevice, x.st));
  HIP_TRY(hipMemcpyAsync(x.dpoll, mi.data(), (size_t)B * 4, hipMemcpyHostToDevice, x.st));
  HIP_TRY(hipMemcpyAsync(x.dsel, sel, (size_t)B * 4, hipMemcpyHostToDevice, x.st));
  const MmPassParams P{x.dchain, x.da, x.db, x.dpoll, x.dsel, x.lc, x.scratch, lp, ll, x.n, x.C, B, x.row, x.Dpad, x.ncols, integrate};
  HIP_TRY(hipMemcpyAsync(x.dP, &P, sizeof P, hipMemcpyHostToDevice, x.st));
  HIP_TRY(hipStreamSynchronize(x.st));   // (the host arrays above are the caller's stack)
  const int grid = (int)std::min<long long>(x.pass_grid, (long long)B * x.S);
  return mm_timed(x, 0, [&] {
    hipLaunchKernelGGL(k_mm_pass, dim3(grid), dim3(PT_THREADS), x.mp->M.lds_doubles * 8 + sizeof(RowLds), x.st, (const DevModel *)x.mp->dM, (const MmPassParams *)x.dP);
    return 0;
  });
}

// mu~, q~ -> host mu, q [B][D]; w device [B][S] (log weights when is_log); m0 host [D] or null
int mm_moments(MmCtx &x, int B, const double *w, int is_log, const double *m0, double *mu, double *q) {
  if (m0) HIP_TRY(hipMemcpyAsync(x.dm0, m0, (size_t)x.D * 8, hipMemcpyHostToDevice, x.st));
  const MmMomParams P{x.dchain, w, m0 ? x.dm0 : nullptr, x.part, x.n, x.C, B, x.row, x.D, is_log};
  const long long BD2 = (long long)B * 2 * x.D;
  if (const int rc = mm_timed(x, 1, [&] {
        hipLaunchKernelGGL(k_mm_moments, dim3((x.D + 255) / 256, x.nchunk(), (B + MM_BT - 1) / MM_BT), dim3(256), 0, x.st, P);
        hipLaunchKernelGGL(k_mm_moments_sum, dim3((unsigned)std::min<long long>((BD2 + 255) / 256, 65535)), dim3(256), 0, x.st, (const double *)x.part, x.mom, x.nchunk(), BD2);
        return 0;
      })) return rc;
  std::vector<double> h((size_t)BD2);
  HIP_TRY(hipMemcpy(h.data(), x.mom, h.size() * 8, hipMemcpyDeviceToHost));
  for (int k = 0; k < B; k++) {
    std::copy(h.begin() + (size_t)k * 2 * x.D, h.begin() + (size_t)k * 2 * x.D + x.D, mu + (size_t)k * x.D);
    std::copy(h.begin() + (size_t)k * 2 * x.D + x.D, h.begin() + (size_t)(k + 1) * 2 * x.D, q + (size_t)k * x.D);
  }
  return 0;
}

// PSIS of r [B][S] (device) -> lw [B][S] (device), k (host [B]); r_eff host [B]
int mm_psis(MmCtx &x, int B, const double *r, const double *r_eff, double *lw, double *k) {
  HIP_TRY(hipMemcpyAsync(x.dre, r_eff, (size_t)B * 8, hipMemcpyHostToDevice, x.st));
  const PsisGenParams P{r, x.dre, x.psis, lw, x.dk, (long long)x.S, B};
  if (const int rc = mm_timed(x, 2, [&] {
        hipLaunchKernelGGL(k_mm_psis, dim3(std::min(B, x.psis_grid)), dim3(DG_THREADS), sorted_run_lds(x.S), x.st, P);
        return 0;
      })) return rc;
  HIP_TRY(hipMemcpy(k, x.dk, (size_t)B * 8, hipMemcpyDeviceToHost));
  return 0;
}

int mm_ratio(MmCtx &x, int B, int mode, const double *lp, const double *ll, const double *lp0, const double *ll0, const double *slb, double *r, double *llx) {
  const MmRatioParams P{lp, ll, lp0, ll0, slb, r, llx, x.n, x.S, B, mode};
  hipLaunchKernelGGL(k_mm_ratio, dim3((unsigned)std::min<long long>(((long long)B * x.S + 255) / 256, 65535)), dim3(256), 0, x.st, P);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mm_check_r_eff(const char *what, const double *r_eff, int n) {
  if (!r_eff) return fail(POTUS_ERR_ARG, "%s: null r_eff", what);
  return loo_check_r_eff(r_eff, n, what);
}

// a further block of an entry point whose DeviceBlock is open on `device`
int mm_also_device(const char *what, int device, const void *ptr, const char *ptr_name) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, ptr) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != device) {
    (void)hipGetLastError();
    return fail(POTUS_ERR_ARG, "%s: the %s is not device memory of GPU %d", what, ptr_name, device);
  }
  return 0;
}

// the chains of a device block [C][n][row]
std::vector<const double *> mm_block_chains(const void *draws, int C, int n, int row) {
  std::vector<const double *> ch(C);
  for (int c = 0; c < C; c++) ch[c] = (const double *)draws + (size_t)c * n * row;
  return ch;
}
} // namespace
} // extern "C++"

void potus_default_loo_mm_opts(potus_loo_mm_opts *o) {
  if (!o) return;
  o->integrate = 1; o->max_iters = 30; o->split = 1; o->cov = 0; o->k_threshold = 0.0;
}

int potus_loo_mm_timing(double *ms) {
  return timing_out("potus_loo_mm_timing", g_mm_ms, 4, ms);
}

int potus_psis_device(int device, const void *log_ratios, int n_polls, int n_chains, long long n_draws, const double *r_eff, void *log_weights_out, double *khat_out) {
  const char *what = "potus_psis_device";
  if (!log_ratios || !log_weights_out || !khat_out || n_polls < 1) return fail(POTUS_ERR_ARG, "%s: bad argument", what);
  if (const int rc_ = mm_check_sizes(what, n_chains, n_draws, 1)) return rc_;
  if (const int rc_ = mm_check_r_eff(what, r_eff, n_polls)) return rc_;
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, device, log_ratios)) return rc_;
  if (const int rc_ = mm_also_device(what, device, log_weights_out, "output")) return rc_;
  // (no model: the PSIS scratch alone)
  const long long S = (long long)n_chains * n_draws;
  const int grid = std::min(n_polls, 1024);
  DevBufs tmp;
  PsisWork W;
  double *dre = nullptr, *dk = nullptr;
  int rc;
  if ((rc = psis_work(tmp, grid, S, 0, W, what, {reinterpret_cast<const void *>(k_mm_psis)})) || (rc = tmp.get(&dre, (size_t)n_polls * 8, what)) ||
      (rc = tmp.get(&dk, (size_t)n_polls * 8, what)))
    return rc;
  HIP_TRY(hipMemcpy(dre, r_eff, (size_t)n_polls * 8, hipMemcpyHostToDevice));
  const PsisGenParams P{(const double *)log_ratios, dre, W, (double *)log_weights_out, dk, S, n_polls};
  hipLaunchKernelGGL(k_mm_psis, dim3(grid), dim3(DG_THREADS), sorted_run_lds(S), 0, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(khat_out, dk, (size_t)n_polls * 8, hipMemcpyDeviceToHost));
  return 0;
}

int potus_loo_mm_moments_device(int device, const void *draws, int n_chains, int n_draws, int D, const void *weights, int n_polls, int is_log, const double *m0,
                                double *mu_out, double *q_out) {
  const char *what = "potus_loo_mm_moments_device";
  if (!draws || !weights || !mu_out || !q_out || n_polls < 1 || D < 1) return fail(POTUS_ERR_ARG, "%s: bad argument", what);
  if (n_polls > 65535 * MM_BT) return fail(POTUS_ERR_UNSUPPORTED, "%s: %d polls (at most %d)", what, n_polls, 65535 * MM_BT);
  if (const int rc_ = mm_check_sizes(what, n_chains, n_draws, 1)) return rc_;
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, device, draws, "block of draws")) return rc_;
  if (const int rc_ = mm_also_device(what, device, weights, "block of weights")) return rc_;
  const int row = POTUS_N_SAMPLER_COLS + D, S = n_chains * n_draws, nchunk = (S + MM_CHUNK - 1) / MM_CHUNK;
  const std::vector<const double *> ch = mm_block_chains(draws, n_chains, n_draws, row);
  DevBufs tmp;
  const double **dchain = nullptr;
  double *part = nullptr, *mom = nullptr, *dm0 = nullptr;
  const long long BD2 = (long long)n_polls * 2 * D;
  int rc;
  if ((rc = tmp.get(&dchain, ch.size() * sizeof(double *), what)) || (rc = tmp.get(&part, (size_t)nchunk * BD2 * 8, what)) || (rc = tmp.get(&mom, (size_t)BD2 * 8, what)) ||
      (rc = tmp.get(&dm0, (size_t)D * 8, what)))
    return rc;
  HIP_TRY(hipMemcpy(dchain, ch.data(), ch.size() * sizeof(double *), hipMemcpyHostToDevice));
  if (m0) HIP_TRY(hipMemcpy(dm0, m0, (size_t)D * 8, hipMemcpyHostToDevice));
  const MmMomParams P{dchain, (const double *)weights, m0 ? dm0 : nullptr, part, n_draws, n_chains, n_polls, row, D, is_log ? 1 : 0};
  hipLaunchKernelGGL(k_mm_moments, dim3((D + 255) / 256, nchunk, (n_polls + MM_BT - 1) / MM_BT), dim3(256), 0, 0, P);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_mm_moments_sum, dim3((unsigned)std::min<long long>((BD2 + 255) / 256, 65535)), dim3(256), 0, 0, (const double *)part, mom, nchunk, BD2);
  HIP_TRY(hipGetLastError());
  std::vector<double> h((size_t)BD2);
  HIP_TRY(hipMemcpy(h.data(), mom, h.size() * 8, hipMemcpyDeviceToHost));
  for (int k = 0; k < n_polls; k++) {
    std::copy(h.begin() + (size_t)k * 2 * D, h.begin() + (size_t)k * 2 * D + D, mu_out + (size_t)k * D);
    std::copy(h.begin() + (size_t)k * 2 * D + D, h.begin() + (size_t)(k + 1) * 2 * D, q_out + (size_t)k * D);
  }
  return 0;
}

int potus_loo_mm_ratios_device(int model_handle, const void *draws, int n_chains, int n_draws, const double *a, const double *b, const int32_t *polls, const int32_t *sel,
                               int n_polls, int integrate, void *lp_out, void *ll_out, void *lp0_out) {
  const char *what = "potus_loo_mm_ratios_device";
  Sampler *mp = get(model_handle);
  if (!mp) return fail(POTUS_ERR_STATE, "%s: bad handle %d", what, model_handle);
  if (!draws || !a || !b || !polls || !sel || !lp_out || !ll_out || n_polls < 1) return fail(POTUS_ERR_ARG, "%s: bad argument", what);
  if (integrate != 0 && integrate != 1) return fail(POTUS_ERR_ARG, "%s: integrate = %d (0: plain, 1: noise coordinate integrated out)", what, integrate);
  if (const int rc_ = mm_check_model(what, mp)) return rc_;
  if (const int rc_ = mm_check_sizes(what, n_chains, n_draws, n_polls)) return rc_;
  for (int k = 0; k < n_polls; k++) {
    if (polls[k] < 0 || polls[k] >= mp->M.Npoll) return fail(POTUS_ERR_ARG, "%s: polls[%d] = %d of %d polls", what, k, polls[k], mp->M.Npoll);
    if (sel[k] < MM_SEL_ID || sel[k] > MM_SEL_SPLIT) return fail(POTUS_ERR_ARG, "%s: sel[%d] = %d (0: theta, 1: T theta, 2: T^-1 theta, 3: split)", what, k, sel[k]);
  }
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, mp->device, draws, "block of draws")) return rc_;
  if (const int rc_ = mm_also_device(what, mp->device, lp_out, "lp output")) return rc_;
  if (const int rc_ = mm_also_device(what, mp->device, ll_out, "ll output")) return rc_;
  if (lp0_out) if (const int rc_ = mm_also_device(what, mp->device, lp0_out, "lp0 output")) return rc_;
  MmCtx x;
  int rc;
  if ((rc = mm_setup(x, what, mp, mm_block_chains(draws, n_chains, n_draws, POTUS_N_SAMPLER_COLS + mp->L.D), n_draws, n_polls))) return rc;
  std::vector<int> pl(polls, polls + n_polls), sl(sel, sel + n_polls);
  if (lp0_out) {
    DevBufs tmp;
    double *ll_tmp = nullptr;
    if ((rc = tmp.get(&ll_tmp, (size_t)x.S * 8, what))) return rc;
    const int id = MM_SEL_ID;
    if ((rc = mm_pass(x, 1, a, b, pl.data(), &id, integrate, (double *)lp0_out, ll_tmp))) return rc;
  }
  return mm_pass(x, n_polls, a, b, pl.data(), sl.data(), integrate, (double *)lp_out, (double *)ll_out);
}

int potus_loo_moment_match(int model_handle, const int *handles, int n_handles, const potus_loo_mm_opts *opts, const int32_t *polls, int n_polls, double *pointwise,
                           double *estimates_out, int32_t *info_out, double *k_path_out, double *map_out) {
  const char *what = "potus_loo_moment_match";
  potus_loo_mm_opts o;
  potus_default_loo_mm_opts(&o);
  if (opts) o = *opts;
  if (!handles || n_handles < 1 || !pointwise || !estimates_out) return fail(POTUS_ERR_ARG, "%s: null argument", what);
  if (o.cov) return fail(POTUS_ERR_UNSUPPORTED, "%s: cov = 1 (loo's third step, a D x D weighted covariance) is not supported: with fewer pooled draws than the D "
                                                "coordinates the weighted covariance is singular; the maps stay diagonal", what);
  if (o.integrate != 0 && o.integrate != 1) return fail(POTUS_ERR_ARG, "%s: integrate = %d (0: plain, 1: noise coordinate integrated out)", what, o.integrate);
  if (o.max_iters < 0 || o.max_iters > 10000) return fail(POTUS_ERR_ARG, "%s: max_iters = %d (0 to 10000)", what, o.max_iters);
  if (std::isnan(o.k_threshold)) return fail(POTUS_ERR_ARG, "%s: k_threshold is NaN", what);
  if (map_out && !polls) return fail(POTUS_ERR_ARG, "%s: map_out [n_polls][2][D] follows the order of polls, which is null", what);
  Sampler *mp = get(model_handle);
  if (!mp) return fail(POTUS_ERR_STATE, "%s: bad model handle %d", what, model_handle);
  if (const int rc_ = mm_check_model(what, mp)) return rc_;
  Pool P;
  if (const int rc_ = P.resolve(handles, n_handles, what)) return rc_;
  if (const int rc_ = P.same_posterior("moment matching pools the chains of one")) return rc_;
  Sampler *s0 = P.s0;
  if (mp->L.D != s0->L.D || mp->L.ncols != s0->L.ncols || mp->M.full != s0->M.full || mp->data_hash != s0->data_hash)
    return fail(POTUS_ERR_ARG, "%s: model handle %d holds another model than handle %d (D, the polls or other data differ): the log density must be the fit's", what, model_handle, handles[0]);
  for (size_t i = 0; i < P.sps.size(); i++)
    if (P.sps[i]->device != mp->device) return fail(POTUS_ERR_UNSUPPORTED, "%s: handle %d is on GPU %d, the model handle on GPU %d (one device in this version)", what, handles[i], P.sps[i]->device, mp->device);
  const int Np = mp->M.Npoll, D = mp->L.D;
  if (Np < 1) return fail(POTUS_ERR_ARG, "%s: the data hold no polls", what);
  if (polls) {
    if (n_polls < 1) return fail(POTUS_ERR_ARG, "%s: n_polls = %d", what, n_polls);
    for (int k = 0; k < n_polls; k++) {
      if (polls[k] < 0 || polls[k] >= Np) return fail(POTUS_ERR_ARG, "%s: polls[%d] = %d of %d polls", what, k, polls[k], Np);
      for (int j = 0; j < k; j++) if (polls[j] == polls[k]) return fail(POTUS_ERR_ARG, "%s: poll %d listed twice", what, polls[k]);
    }
  }
  for (int i = 0; i < Np; i++) {
    const double re = pointwise[(size_t)i * LOO_NPW + 4];
    if (!(std::isfinite(re) && re > 0)) return fail(POTUS_ERR_ARG, "%s: pointwise[%d] holds r_eff = %g (the rows of potus_loo expected)", what, i, re);
  }
  std::vector<int> devs = P.devs;
  devs.push_back(mp->device);
  DeviceGuard guard;
  DeviceLocks lock(devs);
  if (const int rc_ = P.count()) return rc_;
  if (const int rc_ = P.equal_counts()) return rc_;
  int first = 0, n_post = 0;
  if (const int rc_ = P.post_warmup(&first, &n_post)) return rc_;
  const int Ctot = P.chains;
  const long long S = (long long)Ctot * n_post;
  const double thr = o.k_threshold == 0.0 ? lmm_default_threshold(S) : o.k_threshold;
  const int kp = o.max_iters + 2;
  std::fill(g_mm_ms, g_mm_ms + 4, 0.0);
  // the rules decide who enters the loop, before any kernel runs
  std::vector<int> cand;
  if (polls) cand.assign(polls, polls + n_polls);
  else for (int i = 0; i < Np; i++) cand.push_back(i);
  std::vector<LmmPoll> ru(Np);
  std::vector<int> work;
  if (info_out) std::fill(info_out, info_out + (size_t)Np * LMM_NINFO, 0);
  if (k_path_out) std::fill(k_path_out, k_path_out + (size_t)Np * kp, std::numeric_limits<double>::quiet_NaN());
  if (map_out) for (int k = 0; k < n_polls; k++) { std::fill(map_out + (size_t)k * 2 * D, map_out + (size_t)k * 2 * D + D, 0.0); std::fill(map_out + (size_t)k * 2 * D + D, map_out + (size_t)(k + 1) * 2 * D, 1.0); }
  for (int i : cand) {
    if (ru[i].start(pointwise[(size_t)i * LOO_NPW + 3], thr, o.max_iters) != LMM_NONE) work.push_back(i);
    if (info_out) info_out[(size_t)i * LMM_NINFO + 4] = ru[i].stop;
  }
  std::sort(work.begin(), work.end());
  if (work.empty()) { loo_estimates(pointwise, Np, estimates_out); return 0; }
  if (const int rc_ = mm_check_sizes(what, Ctot, n_post, 1)) return rc_;
  const int nchunk = (int)((S + MM_CHUNK - 1) / MM_CHUNK);
  int maxB = (int)std::max<size_t>(1, std::min<size_t>(64, MM_PART_BUDGET / ((size_t)nchunk * 2 * D * 8)));
  if (maxB >= MM_BT) maxB -= maxB % MM_BT;
  maxB = std::min<int>(maxB, (int)work.size());
  maxB = (int)std::min<long long>(maxB, std::max<long long>(1, 0x7fffffffll / S));

  HIP_TRY(hipSetDevice(mp->device));
  std::vector<const double *> chains;
  for (Sampler *sp : P.sps) {
    HIP_TRY(hipStreamSynchronize(sp->stream));
    for (int c = 0; c < sp->R.chains; c++) chains.push_back(sp->R.draws + ((size_t)c * sp->R.n_save_max + first) * sp->R.row);
  }
  MmCtx x;
  int rc;
  if ((rc = mm_setup(x, what, mp, chains, n_post, maxB))) return rc;
  const size_t BS = (size_t)maxB * S;
  double *lp = nullptr, *ll = nullptr, *ll0 = nullptr, *llc = nullptr, *r = nullptr, *lwc = nullptr, *lwn = nullptr, *lp0 = nullptr, *wuni = nullptr, *gA = nullptr, *gB = nullptr, *dslb = nullptr, *delpd = nullptr;
  if ((rc = x.keep.get(&lp, BS * 8, what)) || (rc = x.keep.get(&ll, BS * 8, what)) || (rc = x.keep.get(&ll0, BS * 8, what)) || (rc = x.keep.get(&llc, BS * 8, what)) ||
      (rc = x.keep.get(&r, BS * 8, what)) || (rc = x.keep.get(&lwc, BS * 8, what)) || (rc = x.keep.get(&lwn, BS * 8, what)) || (rc = x.keep.get(&lp0, (size_t)S * 8, what)) ||
      (rc = x.keep.get(&wuni, (size_t)S * 8, what)) || (rc = x.keep.get(&gA, BS * 8, what)) || (rc = x.keep.get(&gB, BS * 8, what)) || (rc = x.keep.get(&dslb, (size_t)maxB * 8, what)) ||
      (rc = x.keep.get(&delpd, (size_t)maxB * 8, what)))
    return rc;
  auto finish = [&](int code) { std::copy(x.ms, x.ms + 4, g_mm_ms); return code; };
  const size_t rowS = (size_t)S * 8;
  // base moments: m0 = mean, v0 = variance (S - 1), two passes of the moments kernel under uniform weights
  std::vector<double> m0(D), v0(D), tmpq(D);
  {
    std::vector<double> wu((size_t)S, 1.0 / (double)S);
    HIP_TRY(hipMemcpy(wuni, wu.data(), rowS, hipMemcpyHostToDevice));
    if ((rc = mm_moments(x, 1, wuni, 0, nullptr, m0.data(), tmpq.data()))) return finish(rc);
    if ((rc = mm_moments(x, 1, wuni, 0, m0.data(), tmpq.data(), v0.data()))) return finish(rc);
    for (int j = 0; j < D; j++) v0[j] *= (double)S / (double)(S - 1);
  }
  bool have_lp0 = false;
  std::vector<double> rows_new(pointwise, pointwise + (size_t)Np * LOO_NPW);   // the caller's rows change once, when every batch is through: a call that fails leaves them alone
  for (size_t w0 = 0; w0 < work.size(); w0 += maxB) {
    const int B = (int)std::min<size_t>(maxB, work.size() - w0);
    const int *pb = work.data() + w0;
    std::vector<double> a((size_t)B * D, 0.0), b((size_t)B * D, 1.0), a1((size_t)B * D), b1((size_t)B * D), mu((size_t)B * D), q((size_t)B * D), reff(B), kk(B);
    std::vector<int> sel(B, MM_SEL_ID), idx(B), pa(B);
    std::vector<std::vector<double>> path(B);
    for (int k = 0; k < B; k++) reff[k] = pointwise[(size_t)pb[k] * LOO_NPW + 4];
    // ---- start: lp0 and ll0 by the kernel of the candidates, PSIS of -ll0
    if ((rc = mm_pass(x, B, a.data(), b.data(), pb, sel.data(), o.integrate, lp, ll0))) return finish(rc);
    if (!have_lp0) { HIP_TRY(hipMemcpy(lp0, lp, rowS, hipMemcpyDeviceToDevice)); have_lp0 = true; }
    HIP_TRY(hipMemcpy(llc, ll0, (size_t)B * rowS, hipMemcpyDeviceToDevice));
    if ((rc = mm_ratio(x, B, 0, lp, ll0, lp0, nullptr, nullptr, r, nullptr)) || (rc = mm_psis(x, B, r, reff.data(), lwc, kk.data()))) return finish(rc);
    for (int k = 0; k < B; k++) {
      const double kpw = pointwise[(size_t)pb[k] * LOO_NPW + 3];
      const bool same = kk[k] == kpw || std::fabs(kk[k] - kpw) <= 1e-12 * std::max(1.0, std::fabs(kpw));   // (both NaN never enters: the rules stop there)
      if (!same) return finish(fail(POTUS_ERR_ARG, "%s: poll %d: PSIS of the fit's draws gives k = %.17g, pointwise holds %.17g: the rows are not potus_loo's of these handles with integrate = %d",
                                    what, pb[k], kk[k], kpw, o.integrate));
      ru[pb[k]].start(kk[k], thr, o.max_iters);
      path[k].push_back(kk[k]);
    }
    // ---- rounds: one candidate per active poll
    for (;;) {
      int nA = 0;
      for (int k = 0; k < B; k++) if (ru[pb[k]].next != LMM_NONE) idx[nA++] = k;
      if (nA == 0) break;
      for (int u = 0; u < nA; u++) HIP_TRY(hipMemcpyAsync(gA + (size_t)u * S, lwc + (size_t)idx[u] * S, rowS, hipMemcpyDeviceToDevice, x.st));
      if ((rc = mm_moments(x, nA, gA, 1, m0.data(), mu.data(), q.data()))) return finish(rc);
      for (int u = 0; u < nA; u++) {
        const int k = idx[u];
        const double *ak = a.data() + (size_t)k * D, *bk = b.data() + (size_t)k * D, *mk = mu.data() + (size_t)u * D, *qk = q.data() + (size_t)u * D;
        double *an = a1.data() + (size_t)u * D, *bn = b1.data() + (size_t)u * D;
        const bool t1 = ru[pb[k]].next == LMM_T1;
        for (int j = 0; j < D; j++) {
          const double m = ak[j] + bk[j] * m0[j], muw = ak[j] + bk[j] * mk[j];
          if (t1) { an[j] = ak[j] + (muw - m); bn[j] = bk[j]; continue; }
          const double dm = mk[j] - m0[j], s2w = bk[j] * bk[j] * (qk[j] - dm * dm) * (double)S / (double)(S - 1);
          double rho = std::sqrt(s2w / (bk[j] * bk[j] * v0[j]));
          if (!(std::isfinite(rho) && rho > 0.0)) rho = 1.0;
          bn[j] = rho * bk[j];
          an[j] = muw - rho * bk[j] * m0[j];
        }
        pa[u] = pb[k]; sel[u] = MM_SEL_T;
      }
      if ((rc = mm_pass(x, nA, a1.data(), b1.data(), pa.data(), sel.data(), o.integrate, lp, ll))) return finish(rc);
      std::vector<double> re(nA), kn(nA);
      for (int u = 0; u < nA; u++) re[u] = reff[idx[u]];
      if ((rc = mm_ratio(x, nA, 1, lp, ll, lp0, nullptr, nullptr, r, nullptr)) || (rc = mm_psis(x, nA, r, re.data(), lwn, kn.data()))) return finish(rc);
      for (int u = 0; u < nA; u++) {
        const int k = idx[u];
        if (!ru[pb[k]].feed(kn[u], thr, o.max_iters)) continue;
        std::copy(a1.begin() + (size_t)u * D, a1.begin() + (size_t)(u + 1) * D, a.begin() + (size_t)k * D);
        std::copy(b1.begin() + (size_t)u * D, b1.begin() + (size_t)(u + 1) * D, b.begin() + (size_t)k * D);
        HIP_TRY(hipMemcpyAsync(lwc + (size_t)k * S, lwn + (size_t)u * S, rowS, hipMemcpyDeviceToDevice, x.st));
        HIP_TRY(hipMemcpyAsync(llc + (size_t)k * S, ll + (size_t)u * S, rowS, hipMemcpyDeviceToDevice, x.st));
        path[k].push_back(kn[u]);
      }
      HIP_TRY(hipStreamSynchronize(x.st));
    }
    // ---- split: half of every chain's draws transformed, the mixture of the posterior and its push-forward as the proposal
    int nS = 0;
    for (int k = 0; k < B; k++) if (o.split && ru[pb[k]].accepted() > 0) idx[nS++] = k;
    if (nS > 0) {
      std::vector<double> slb(nS), re(nS), kn(nS);
      for (int u = 0; u < nS; u++) {
        const int k = idx[u];
        std::copy(a.begin() + (size_t)k * D, a.begin() + (size_t)(k + 1) * D, a1.begin() + (size_t)u * D);
        std::copy(b.begin() + (size_t)k * D, b.begin() + (size_t)(k + 1) * D, b1.begin() + (size_t)u * D);
        double s = 0.0;
        for (int j = 0; j < D; j++) s += std::log(b[(size_t)k * D + j]);
        slb[u] = s; re[u] = reff[k]; pa[u] = pb[k]; sel[u] = MM_SEL_SPLIT;
        HIP_TRY(hipMemcpyAsync(gA + (size_t)u * S, ll0 + (size_t)k * S, rowS, hipMemcpyDeviceToDevice, x.st));
      }
      HIP_TRY(hipMemcpyAsync(dslb, slb.data(), (size_t)nS * 8, hipMemcpyHostToDevice, x.st));
      if ((rc = mm_pass(x, nS, a1.data(), b1.data(), pa.data(), sel.data(), o.integrate, lp, ll))) return finish(rc);
      if ((rc = mm_ratio(x, nS, 2, lp, ll, lp0, gA, dslb, r, gB)) || (rc = mm_psis(x, nS, r, re.data(), lwn, kn.data()))) return finish(rc);
      for (int u = 0; u < nS; u++) {
        const int k = idx[u];
        HIP_TRY(hipMemcpyAsync(lwc + (size_t)k * S, lwn + (size_t)u * S, rowS, hipMemcpyDeviceToDevice, x.st));
        HIP_TRY(hipMemcpyAsync(llc + (size_t)k * S, gB + (size_t)u * S, rowS, hipMemcpyDeviceToDevice, x.st));
        ru[pb[k]].k = kn[u];
        path[k].push_back(kn[u]);
      }
      HIP_TRY(hipStreamSynchronize(x.st));
    }
    // ---- the result rows
    std::vector<double> elpd(B);
    if ((rc = mm_timed(x, 3, [&] { hipLaunchKernelGGL(k_mm_final, dim3(B), dim3(DG_THREADS), 0, x.st, (const double *)llc, (const double *)lwc, delpd, S, B); return 0; }))) return finish(rc);
    HIP_TRY(hipMemcpy(elpd.data(), delpd, (size_t)B * 8, hipMemcpyDeviceToHost));
    for (int k = 0; k < B; k++) {
      const int i = pb[k];
      const LmmPoll &u = ru[i];
      const bool split_done = o.split && u.accepted() > 0;
      if (info_out) { int32_t *io = info_out + (size_t)i * LMM_NINFO; io[0] = u.n_t1; io[1] = u.n_t2; io[2] = u.rounds; io[3] = split_done; io[4] = u.stop; io[5] = 0; }
      if (k_path_out) for (size_t t = 0; t < path[k].size() && t < (size_t)kp; t++) k_path_out[(size_t)i * kp + t] = path[k][t];
      if (map_out)
        for (int t = 0; t < n_polls; t++)
          if (polls[t] == i) { std::copy(a.begin() + (size_t)k * D, a.begin() + (size_t)(k + 1) * D, map_out + (size_t)t * 2 * D); std::copy(b.begin() + (size_t)k * D, b.begin() + (size_t)(k + 1) * D, map_out + (size_t)t * 2 * D + D); }
      if (u.accepted() == 0) continue;                       // the row keeps its bytes
      double *pw = rows_new.data() + (size_t)i * LOO_NPW;
      const double lpd = pw[0] + pw[1];
      pw[0] = elpd[k]; pw[1] = lpd - elpd[k]; pw[2] = -2.0 * elpd[k]; pw[3] = u.k;
    }
  }
  std::copy(rows_new.begin(), rows_new.end(), pointwise);
  loo_estimates(pointwise, Np, estimates_out);
  return finish(0);
}

// ---------------------------------------------------------------------------------------------- E_loo (potus_eloo.hpp)
namespace {
constexpr size_t EL_PART_BUDGET = 128ull << 20;   // the chunk partials of one k_el_shared launch
thread_local double g_el_ms[4] = {0.0, 0.0, 0.0, 0.0};   // the calling thread's last call: pointwise form, column means and product, chunk sum and ess, diagnostic

int el_check_sizes(const char *what, long long C, long long n) {
  if (C < 1 || n < 4) return fail(POTUS_ERR_ARG, "%s: %lld chains of %lld draws (at least one chain, four draws per chain)", what, C, n);
  if (2 * C > DG_MAXCH) return fail(POTUS_ERR_UNSUPPORTED, "%s: %lld chains pooled (at most %d)", what, C, DG_MAXCH / 2);
  if (C * n > 0x7fffffffll) return fail(POTUS_ERR_UNSUPPORTED, "%s: %lld draws per poll (at most 2^31 - 1)", what, C * n);
  if ((C * n + EL_CHUNK - 1) / EL_CHUNK > 65535) return fail(POTUS_ERR_UNSUPPORTED, "%s: %lld pooled draws (at most %d: one grid plane per %d draws)", what, C * n, 65535 * EL_CHUNK, EL_CHUNK);
  return 0;
}
// the span between two recorded events of an idle stream, added to ms[stage]
int el_span(EventTimer &t, hipStream_t st, double *ms, int stage) {
  HIP_TRY(hipGetLastError());
  HIP_TRY(t.stop(st));
  HIP_TRY(hipStreamSynchronize(st));
  double v = 0.0;
  if (t.elapsed(&v)) ms[stage] += v;
  return 0;
}
} // namespace

int potus_e_loo_timing(double *ms) {
  return timing_out("potus_e_loo_timing", g_el_ms, 4, ms);
}

int potus_poll_share_device(int handle, int poll_begin, int poll_end, int integrate, void *a1_out_device, void *a2_out_device) {
  const char *what = "potus_poll_share_device";
  Sampler *sp = get(handle);
  if (!sp || !a1_out_device || !a2_out_device) return fail(POTUS_ERR_STATE, "bad handle or null output");
  if (const int rc_ = refuse_many_datasets(sp, what)) return rc_;
  if (integrate != 0 && integrate != 1) return fail(POTUS_ERR_ARG, "%s: integrate = %d (0: at the draw's noise coordinate, 1: noise coordinate integrated out)", what, integrate);
  const int Np = sp->M.Npoll;
  if (poll_begin < 0 || poll_end > Np || poll_begin >= poll_end) return fail(POTUS_ERR_ARG, "%s: polls [%d, %d) of %d", what, poll_begin, poll_end, Np);
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, sp->device, a1_out_device, "a1 output")) return rc_;
  if (const int rc_ = mm_also_device(what, sp->device, a2_out_device, "a2 output")) return rc_;
  int n_saved = 0, rc = saved_count(sp, &n_saved);
  if (rc) return rc;
  const int first = warm_rows(sp, n_saved), n_post = n_saved - first, C = sp->R.chains;
  if (n_post < 1) return fail(POTUS_ERR_STATE, "%s: no post-warm-up draws saved (%d saved, %d of them warm-up)", what, n_saved, first);
  DevBufs keep;
  LooRows r;
  if ((rc = loo_rows_setup(sp, (long long)n_post * C, keep, r, what))) return rc;
  const int nb = loo_block_polls((size_t)n_post * C * 16, poll_end - poll_begin);
  double *b1 = nullptr, *b2 = nullptr;
  if ((rc = keep.get(&b1, (size_t)n_post * C * nb * 8, what)) || (rc = keep.get(&b2, (size_t)n_post * C * nb * 8, what))) return rc;
  for (int b0 = poll_begin; b0 < poll_end; b0 += nb) {
    const int e1 = std::min(b0 + nb, poll_end);
    ElShareParams P{row_src(sp, first), sp->L.ncols, n_post, b0, e1, integrate, r.scratch, b1, b2};
    hipLaunchKernelGGL(k_el_poll_share, dim3(r.grid), dim3(256), 0, sp->stream, (const DevModel *)sp->dM, P);
    HIP_TRY(hipGetLastError());
    if ((rc = transpose_block(sp->stream, b1, (double *)a1_out_device + (size_t)(b0 - poll_begin) * C * n_post, n_post, C, e1 - b0, C, 0))) return rc;
    if ((rc = transpose_block(sp->stream, b2, (double *)a2_out_device + (size_t)(b0 - poll_begin) * C * n_post, n_post, C, e1 - b0, C, 0))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

int potus_e_loo_device(int device, const void *x, const void *log_ratios, int n_polls, int n_chains, long long n_draws, const double *r_eff, const double *probs,
                       int n_probs, double *out, double *khat_out) {
  const char *what = "potus_e_loo_device";
  if (!x || !log_ratios || !out || !khat_out || n_polls < 1 || n_probs < 0 || (n_probs > 0 && !probs)) return fail(POTUS_ERR_ARG, "%s: bad argument", what);
  if (n_probs > EL_MAXP) return fail(POTUS_ERR_UNSUPPORTED, "%s: %d quantile probabilities (at most %d per call)", what, n_probs, EL_MAXP);
  for (int i = 0; i < n_probs; i++)
    if (!(probs[i] > 0.0 && probs[i] < 1.0)) return fail(POTUS_ERR_ARG, "%s: probs[%d] = %g (inside (0, 1) expected)", what, i, probs[i]);
  if (const int rc_ = el_check_sizes(what, n_chains, n_draws)) return rc_;
  if (const int rc_ = loo_check_r_eff(r_eff, n_polls, what)) return rc_;
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, device, x, "block of x")) return rc_;
  if (const int rc_ = mm_also_device(what, device, log_ratios, "block of log ratios")) return rc_;
  std::fill(g_el_ms, g_el_ms + 4, 0.0);
  const long long S = (long long)n_chains * n_draws;
  const int grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(n_polls, 1024), LOO_BLOCK_BUDGET / 2 / psis_work_bytes(S, EL_ROWS)));
  DevBufs tmp;
  ElPwParams P{};
  double *dre = nullptr, *dout = nullptr, *dk = nullptr;
  int rc;
  if ((rc = psis_work(tmp, grid, S, EL_ROWS, P.W, what, {reinterpret_cast<const void *>(k_el_pointwise)})) || (rc = tmp.get(&dout, (size_t)n_polls * (3 + n_probs) * 8, what)) || (rc = tmp.get(&dk, (size_t)n_polls * EL_NK * 8, what))) return rc;
  if (r_eff) {
    if ((rc = tmp.get(&dre, (size_t)n_polls * 8, what))) return rc;
    HIP_TRY(hipMemcpy(dre, r_eff, (size_t)n_polls * 8, hipMemcpyHostToDevice));
  }
  P.x = (const double *)x; P.r = (const double *)log_ratios; P.r_eff = dre; P.out = dout; P.khat = dk;
  for (int i = 0; i < n_probs; i++) P.probs[i] = probs[i];
  P.n = n_draws; P.C = n_chains; P.NP = n_polls; P.np = n_probs;
  const size_t lds = sorted_run_lds(S);
  EventTimer t;
  HIP_TRY(t.made);
  HIP_TRY(t.start(0));
  hipLaunchKernelGGL(k_el_pointwise, dim3(grid), dim3(DG_THREADS), lds, 0, P);
  if ((rc = el_span(t, 0, g_el_ms, 0))) return rc;
  HIP_TRY(hipMemcpy(out, dout, (size_t)n_polls * (3 + n_probs) * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(khat_out, dk, (size_t)n_polls * EL_NK * 8, hipMemcpyDeviceToHost));
  return 0;
}

int potus_e_loo_shared_device(int device, const void *X, int n_cols, const void *log_weights, int n_polls, int n_chains, long long n_draws, const void *log_ratios,
                              const double *r_eff, int diag, double *mean_out, double *var_out, double *ess_out, double *khat_out) {
  const char *what = "potus_e_loo_shared_device";
  if (!X || !log_weights || !mean_out || !var_out || !ess_out || n_polls < 1 || n_cols < 1) return fail(POTUS_ERR_ARG, "%s: bad argument", what);
  if (diag != 0 && diag != 1) return fail(POTUS_ERR_ARG, "%s: diag = %d (0: k of the ratios per poll, 1: k of every mean)", what, diag);
  if (diag && !log_ratios) return fail(POTUS_ERR_ARG, "%s: diag = 1 needs the raw log ratios", what);
  if (log_ratios && !khat_out) return fail(POTUS_ERR_ARG, "%s: log ratios without an output for their k", what);
  if (const int rc_ = el_check_sizes(what, n_chains, n_draws)) return rc_;
  if (const int rc_ = loo_check_r_eff(r_eff, n_polls, what)) return rc_;
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, device, X, "block of columns")) return rc_;
  if (const int rc_ = mm_also_device(what, device, log_weights, "block of log weights")) return rc_;
  if (log_ratios) if (const int rc_ = mm_also_device(what, device, log_ratios, "block of log ratios")) return rc_;
  std::fill(g_el_ms, g_el_ms + 4, 0.0);
  const long long S = (long long)n_chains * n_draws;
  const int nchunk = (int)((S + EL_CHUNK - 1) / EL_CHUNK);
  // polls per launch: whole tiles whose chunk partials stay within the budget (at least one tile)
  const size_t per_tile = (size_t)nchunk * 2 * EL_TM * (size_t)n_cols * 8;
  const int pb = (int)std::min<size_t>((size_t)(n_polls + EL_TM - 1) / EL_TM, std::max<size_t>(1, EL_PART_BUDGET / per_tile)) * EL_TM;
  const int pmax = std::min(pb, n_polls);
  DevBufs tmp;
  double *cm = nullptr, *part = nullptr, *dmean = nullptr, *dvar = nullptr, *dess = nullptr;
  int rc;
  if ((rc = tmp.get(&cm, (size_t)n_cols * 8, what)) || (rc = tmp.get(&part, (size_t)nchunk * 2 * pmax * (size_t)n_cols * 8, what)) ||
      (rc = tmp.get(&dmean, (size_t)pmax * n_cols * 8, what)) || (rc = tmp.get(&dvar, (size_t)pmax * n_cols * 8, what)) || (rc = tmp.get(&dess, (size_t)n_polls * 8, what)))
    return rc;
  EventTimer t;
  HIP_TRY(t.made);
  const double *Xd = (const double *)X, *lw = (const double *)log_weights;
  HIP_TRY(t.start(0));
  hipLaunchKernelGGL(k_el_colmean, dim3(std::min(n_cols, 65535)), dim3(DG_THREADS), 0, 0, Xd, cm, S, n_cols);
  if ((rc = el_span(t, 0, g_el_ms, 1))) return rc;
  for (int p0 = 0; p0 < n_polls; p0 += pb) {
    const int np = std::min(pb, n_polls - p0);
    const ElShParams P{Xd, lw + (size_t)p0 * S, cm, part, S, np, n_cols};
    HIP_TRY(t.start(0));
    hipLaunchKernelGGL(k_el_shared, dim3((n_cols + EL_TN - 1) / EL_TN, (np + EL_TM - 1) / EL_TM, nchunk), dim3(EL_THREADS), 0, 0, P);
    if ((rc = el_span(t, 0, g_el_ms, 1))) return rc;
    const long long PC = (long long)np * n_cols;
    HIP_TRY(t.start(0));
    hipLaunchKernelGGL(k_el_shared_sum, dim3((unsigned)std::min<long long>((PC + 255) / 256, 65535)), dim3(256), 0, 0, (const double *)part, (const double *)cm, dmean, dvar, nchunk, np, n_cols);
    if ((rc = el_span(t, 0, g_el_ms, 2))) return rc;
    HIP_TRY(hipMemcpy(mean_out + (size_t)p0 * n_cols, dmean, (size_t)PC * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(var_out + (size_t)p0 * n_cols, dvar, (size_t)PC * 8, hipMemcpyDeviceToHost));
  }
  HIP_TRY(t.start(0));
  hipLaunchKernelGGL(k_el_ess, dim3(std::min(n_polls, 65535)), dim3(DG_THREADS), 0, 0, lw, dess, S, n_polls);
  if ((rc = el_span(t, 0, g_el_ms, 2))) return rc;
  HIP_TRY(hipMemcpy(ess_out, dess, (size_t)n_polls * 8, hipMemcpyDeviceToHost));
  if (!log_ratios) return 0;
  // ---- the diagnostic: k_r (and r_eff) per poll, then with diag = 1 the k of every mean
  const long long items = diag ? (long long)n_polls * n_cols : n_polls;
  const int grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min<long long>(items, 1024), LOO_BLOCK_BUDGET / 2 / psis_work_bytes(S, EL_ROWS)));
  ElKParams K{};
  double *dre = nullptr, *dkr = nullptr, *dreff = nullptr, *dkh = nullptr;
  if ((rc = psis_work(tmp, grid, S, EL_ROWS, K.W, what, {reinterpret_cast<const void *>(k_el_kr), reinterpret_cast<const void *>(k_el_khat)})) || (rc = tmp.get(&dkr, (size_t)n_polls * 8, what)) || (rc = tmp.get(&dreff, (size_t)n_polls * 8, what))) return rc;
  if (r_eff) {
    if ((rc = tmp.get(&dre, (size_t)n_polls * 8, what))) return rc;
    HIP_TRY(hipMemcpy(dre, r_eff, (size_t)n_polls * 8, hipMemcpyHostToDevice));
  }
  if (diag && (rc = tmp.get(&dkh, (size_t)items * 8, what))) return rc;
  K.X = Xd; K.r = (const double *)log_ratios; K.r_eff = dre; K.kr = dkr; K.reff = dreff; K.khat = dkh;
  K.n = n_draws; K.C = n_chains; K.NP = n_polls; K.NC = n_cols;
  const size_t lds = sorted_run_lds(S);
  HIP_TRY(t.start(0));
  hipLaunchKernelGGL(k_el_kr, dim3(std::min(n_polls, grid)), dim3(DG_THREADS), lds, 0, K);
  if (diag) hipLaunchKernelGGL(k_el_khat, dim3(grid), dim3(DG_THREADS), lds, 0, K);
  if ((rc = el_span(t, 0, g_el_ms, 3))) return rc;
  HIP_TRY(hipMemcpy(khat_out, diag ? dkh : dkr, (size_t)items * 8, hipMemcpyDeviceToHost));
  return 0;
}

// ---------------------------------------------------------------------------------------------- summary table (potus_monitor.hpp)
namespace {
// the gathered rows of one handle plus the transposed columns of one block of a potus_monitor call (POTUS_MONITOR_BLOCK_BUDGET, bytes: tests)
constexpr size_t MONITOR_BLOCK_BUDGET = 256ull << 20;

// what needs no device: the probabilities, the output, the pooled sizes
int monitor_check(const char *what, const double *probs, int n_probs, const double *out, long long n, long long C) {
  if (n_probs < 0 || n_probs > MN_MAXPROBS) return fail(POTUS_ERR_ARG, "%s: n_probs = %d (0 to %d)", what, n_probs, MN_MAXPROBS);
  if (n_probs > 0 && !probs) return fail(POTUS_ERR_ARG, "%s: null probs", what);
  for (int i = 0; i < n_probs; i++) if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) return fail(POTUS_ERR_ARG, "%s: probs[%d] = %g outside [0, 1]", what, i, probs[i]);
  if (!out) return fail(POTUS_ERR_ARG, "%s: null out", what);
  if (2 * C > DG_MAXCH) return fail(POTUS_ERR_UNSUPPORTED, "%s: %lld chains pooled (at most %d)", what, C, DG_MAXCH / 2);
  if (C * n > 0x7fffffffll) return fail(POTUS_ERR_UNSUPPORTED, "%s: %lld pooled draws (the sort's indices have 32 bits)", what, C * n);
  return 0;
}

// cols [NC][C][n] on the current device -> out [NC][MN_NSTATS + n_probs] (host)
int monitor_of_columns(hipStream_t stream, const double *cols, long long n, int C, int NC, const double *probs, int n_probs, double *out, const char *what) {
  const long long N = std::max<long long>(2ll * C * (n / 2), 1), M = (long long)C * n;
  const int W = MN_NSTATS + n_probs;
  DevBufs tmp;
  MnParams P{};
  int rc;
  // k_dg_column's scratch per workgroup (its runs hold the C middle draws too when n is odd) and its cap on the grid
  const long long per_wg = N * 16 + (long long)sorted_run_bytes(M);
  const int grid = (int)std::max<long long>(1, std::min<long long>(std::min(NC, 1024), (768ll << 20) / per_wg));
  if ((rc = tmp.get(&P.zbuf, (size_t)grid * 2 * (size_t)N * 8, what))) return rc;
  if ((rc = sorted_run_scratch(tmp, grid, M, &P.rkey, &P.ridx, what)) || (rc = tmp.get(&P.out, (size_t)NC * W * 8, what))) return rc;
  const size_t lds = sorted_run_lds(M);                // keys + indices
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mn_column), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  P.cols = cols; P.n = n; P.C = C; P.NC = NC; P.n_probs = n_probs;
  for (int i = 0; i < n_probs; i++) P.probs[i] = probs[i];
  hipLaunchKernelGGL(k_mn_column, dim3(grid), dim3(DG_THREADS), lds, stream, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, P.out, (size_t)NC * W * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}
} // namespace

int potus_monitor_device(int device, const void *block, long long n_draws, int n_chains, int n_cols, const double *probs, int n_probs, double *out) {
  if (!block || n_draws < 1 || n_chains < 1 || n_cols < 1) return fail(POTUS_ERR_ARG, "potus_monitor_device: bad argument");
  if (const int rc_ = monitor_check("potus_monitor_device", probs, n_probs, out, n_draws, n_chains)) return rc_;   // before anything is allocated
  DeviceBlock dev;
  if (const int rc_ = dev.open("potus_monitor_device", device, block)) return rc_;
  DevBufs tmp;
  double *cols = nullptr;
  if (const int rc_ = tmp.get(&cols, (size_t)n_draws * n_chains * n_cols * 8, "potus_monitor_device")) return rc_;
  if (const int rc_ = transpose_block(0, (const double *)block, cols, n_draws, n_chains, n_cols, n_chains, 0)) return rc_;
  return monitor_of_columns(0, cols, n_draws, n_chains, n_cols, probs, n_probs, out, "potus_monitor_device");
}

int potus_monitor(const int *handles, int n_handles, int col_begin, int col_end, const double *probs, int n_probs, double *out) {
  if (const int rc_ = monitor_check("potus_monitor", probs, n_probs, out, 0, 0)) return rc_;
  if (col_begin < 0 || col_begin >= col_end) return fail(POTUS_ERR_ARG, "potus_monitor: columns [%d, %d)", col_begin, col_end);
  Pool P;
  if (const int rc_ = P.resolve(handles, n_handles, "potus_monitor")) return rc_;
  if (col_end > P.s0->L.ncols) return fail(POTUS_ERR_ARG, "potus_monitor: columns [%d, %d) of %d", col_begin, col_end, P.s0->L.ncols);
  if (const int rc_ = P.same_posterior("the table pools the chains of one")) return rc_;
  long long Ctot = 0;
  for (const Sampler *sp : P.sps) Ctot += sp->R.chains;
  if (const int rc_ = monitor_check("potus_monitor", probs, n_probs, out, 0, Ctot)) return rc_;
  DeviceGuard guard;
  DeviceLocks lock(P.devs);
  if (const int rc_ = P.count()) return rc_;
  if (const int rc_ = P.equal_counts()) return rc_;
  int n_warm_rows = 0, n_post = 0;
  if (const int rc_ = P.post_warmup(&n_warm_rows, &n_post)) return rc_;
  if (const int rc_ = monitor_check("potus_monitor", probs, n_probs, out, n_post, Ctot)) return rc_;
  Sampler *s0 = P.s0;
  HIP_TRY(hipSetDevice(s0->device));
  // columns per block: one handle's gathered rows (at most all chains, warm-up rows included) and the block's transposed columns
  size_t budget = MONITOR_BLOCK_BUDGET;
  if (const char *e = getenv("POTUS_MONITOR_BLOCK_BUDGET")) budget = std::max<size_t>(1, (size_t)atoll(e));
  const size_t per_col = ((size_t)P.saved[0] + (size_t)n_post) * (size_t)Ctot * 8;
  const int nb = (int)std::max<size_t>(1, std::min<size_t>((size_t)(col_end - col_begin), budget / per_col));
  const int W = MN_NSTATS + n_probs;
  DevBufs tmp;
  double *cols = nullptr;
  if (const int rc_ = tmp.get(&cols, (size_t)n_post * Ctot * nb * 8, "potus_monitor")) return rc_;
  for (int b0 = col_begin; b0 < col_end; b0 += nb) {
    const int b1 = std::min(b0 + nb, col_end);
    if (const int rc_ = gather_columns(P, b0, b1, n_warm_rows, n_post, cols)) return rc_;
    if (const int rc_ = monitor_of_columns(s0->stream, cols, n_post, (int)Ctot, b1 - b0, probs, n_probs, out + (size_t)(b0 - col_begin) * W, "potus_monitor")) return rc_;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------- joint outcomes (potus_outcomes.hpp)
namespace {
thread_local double g_oc_ms[3] = {0.0, 0.0, 0.0};   // the last call of this thread: gather + produce, day-range reshape, counting kernel
static_assert(sizeof(long long) == sizeof(unsigned long long), "the counts are copied out as they are");

struct OcOut { long long *ev_hist, *tipping, *joint, *below_actual, *n_draws; };

// everything about ev, ev_to_win and actual: no device needed
int oc_check(const char *what, int S, const int32_t *ev, int ev_to_win, const double *actual, int *ev_sum) {
  if (S < 1 || S > OC_MAX_S) return fail(POTUS_ERR_UNSUPPORTED, "%s: S = %d (the kernel maps states to the lanes of a wave: 1 .. %d)", what, S, OC_MAX_S);
  if (!ev) return fail(POTUS_ERR_ARG, "%s: ev is null", what);
  long long sum = 0;
  for (int s = 0; s < S; s++) {
    if (ev[s] < 0) return fail(POTUS_ERR_ARG, "%s: ev[%d] = %d is negative", what, s, ev[s]);
    sum += ev[s];
  }
  if (sum > OC_EV_CAP) return fail(POTUS_ERR_UNSUPPORTED, "%s: the electoral votes sum to %lld, the histogram holds at most %d", what, sum, OC_EV_CAP);
  if (ev_to_win < 1) return fail(POTUS_ERR_ARG, "%s: ev_to_win = %d (at least 1)", what, ev_to_win);
  if (actual)
    for (int s = 0; s < S; s++)
      if (!(actual[s] >= 0.0 && actual[s] <= 1.0)) return fail(POTUS_ERR_ARG, "%s: actual[%d] = %g outside [0, 1]", what, s, actual[s]);
  *ev_sum = (int)sum;
  return 0;
}

// items [nd][n_days][S] on the current device -> the counts, in the caller's host arrays (any of them may be null); *kernel_ms = the counting kernel's time
int oc_count(const char *what, hipStream_t st, const double *items, long long nd, int n_days, int S, const double *w, const int32_t *ev, int ev_to_win,
             const double *actual, int ev_sum, const OcOut &o, double *kernel_ms) {
  const size_t n_hist = (size_t)n_days * (ev_sum + 1), n_tip = (size_t)n_days * (S + 1), n_joint = (size_t)n_days * (S + 2) * (S + 2),
               n_below = (size_t)n_days * S;
  DevBufs tmp;
  double *dw = nullptr, *dact = nullptr;
  int32_t *dev_ = nullptr;
  unsigned long long *dout = nullptr;
  int rc;
  if ((rc = tmp.get(&dw, (size_t)S * 8, what)) || (rc = tmp.get(&dev_, (size_t)S * 4, what))) return rc;
  if ((rc = tmp.get(&dout, (n_hist + n_tip + n_joint + n_below) * 8, what))) return rc;
  HIP_TRY(hipMemcpyAsync(dw, w, (size_t)S * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(dev_, ev, (size_t)S * 4, hipMemcpyHostToDevice, st));
  if (actual) { if ((rc = tmp.get(&dact, (size_t)S * 8, what))) return rc; HIP_TRY(hipMemcpyAsync(dact, actual, (size_t)S * 8, hipMemcpyHostToDevice, st)); }
  HIP_TRY(hipMemsetAsync(dout, 0, (n_hist + n_tip + n_joint + n_below) * 8, st));
  // about 2048 workgroups over days x chunks of draws; a workgroup's own counters have 32 bits
  long long chunks = std::min<long long>(std::max(1, 2048 / n_days), (nd + 63) / 64);
  chunks = std::max(chunks, (nd + (1ll << 30) - 1) >> 30);
  const long long chunk = (nd + chunks - 1) / chunks;
  chunks = (nd + chunk - 1) / chunk;
  OcParams P{items, nd, chunk, n_days, S, ev_to_win, ev_sum, dw, dev_, dact, dout, dout + n_hist, dout + n_hist + n_tip, dout + n_hist + n_tip + n_joint};
  EventTimer e;
  HIP_TRY(e.made);
  HIP_TRY(e.start(st));
  hipLaunchKernelGGL(k_oc_count, dim3((unsigned)n_days, (unsigned)chunks), dim3(OC_THREADS), 0, st, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(e.stop(st));
  if (o.ev_hist) HIP_TRY(hipMemcpyAsync(o.ev_hist, P.ev_hist, n_hist * 8, hipMemcpyDeviceToHost, st));
  if (o.tipping) HIP_TRY(hipMemcpyAsync(o.tipping, P.tipping, n_tip * 8, hipMemcpyDeviceToHost, st));
  if (o.joint) HIP_TRY(hipMemcpyAsync(o.joint, P.joint, n_joint * 8, hipMemcpyDeviceToHost, st));
  if (o.below_actual && actual) HIP_TRY(hipMemcpyAsync(o.below_actual, P.below, n_below * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  (void)e.elapsed(kernel_ms);
  if (o.n_draws) *o.n_draws = nd;
  return 0;
}
} // namespace

int potus_outcomes_device(int device, const void *block, long long n_draws, int n_days, int S, const double *w, const int32_t *ev, int ev_to_win,
                          const double *actual, long long *ev_hist, long long *tipping, long long *joint, long long *below_actual, long long *n_draws_out) {
  const char *what = "potus_outcomes_device";
  if (!block || !w) return fail(POTUS_ERR_ARG, "%s: null block or weights", what);
  if (n_draws < 1) return fail(POTUS_ERR_ARG, "%s: %lld draws (at least one)", what, n_draws);
  if (n_draws > (1ll << 40)) return fail(POTUS_ERR_UNSUPPORTED, "%s: %lld draws (at most 2^40)", what, n_draws);
  if (n_days < 1) return fail(POTUS_ERR_ARG, "%s: %d days (at least one)", what, n_days);
  int ev_sum = 0;
  if (const int rc_ = oc_check(what, S, ev, ev_to_win, actual, &ev_sum)) return rc_;
  for (int s = 0; s < S; s++) if (!std::isfinite(w[s])) return fail(POTUS_ERR_ARG, "%s: w[%d] is not finite", what, s);
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, device, block)) return rc_;
  g_oc_ms[0] = g_oc_ms[1] = g_oc_ms[2] = 0.0;
  return oc_count(what, 0, (const double *)block, n_draws, n_days, S, w, ev, ev_to_win, actual, ev_sum, OcOut{ev_hist, tipping, joint, below_actual, n_draws_out}, &g_oc_ms[2]);
}

// Pooled over the post-warm-up draws of every listed sampler (the rules of potus_posterior_summary_many for what may be pooled, of potus_loo for
// the warm-up rows); the counting runs on the first handle's GPU, predicted_score blocks of other GPUs come over by peer copies.
int potus_outcomes(const int *handles, int n_handles, int day_begin, int day_end, const int32_t *ev, int ev_to_win, const double *actual,
                   long long *ev_hist, long long *tipping, long long *joint, long long *below_actual, long long *n_draws_out) {
  const char *what = "potus_outcomes";
  if (!handles || n_handles < 1) return fail(POTUS_ERR_ARG, "%s: null handle list", what);
  Pool P;
  if (const int rc_ = P.resolve(handles, n_handles, what)) return rc_;
  if (const int rc_ = P.same_posterior("joint outcomes pool the chains of one")) return rc_;
  Sampler *s0 = P.s0;
  const int S = s0->M.S;
  int ev_sum = 0;
  if (const int rc_ = oc_check(what, S, ev, ev_to_win, actual, &ev_sum)) return rc_;
  DeviceGuard guard;
  DeviceLocks lock(P.devs);
  DayItems g;
  if (const int rc_ = gather_days(P, day_begin, day_end, false, -1, g)) return rc_;
  g_oc_ms[0] = g.gather_ms; g_oc_ms[1] = g.reshape_ms; g_oc_ms[2] = 0.0;
  return oc_count(what, s0->stream, g.items, g.nd, day_end - day_begin, S, s0->h_w.data(), ev, ev_to_win, actual, ev_sum,
                  OcOut{ev_hist, tipping, joint, below_actual, n_draws_out}, &g_oc_ms[2]);
}

int potus_outcomes_timing(double *ms) {
  return timing_out("potus_outcomes_timing", g_oc_ms, 3, ms);
}

// ---------------------------------------------------------------------------------------------- conditional forecasts (potus_scenario.hpp)
namespace {
thread_local double g_sc_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // the last call of this thread (potus_scenario_timing)
constexpr size_t SC_SCRATCH_BUDGET = (size_t)256 << 20;        // nat and the chunk partials of one block of days (POTUS_SCENARIO_SCRATCH_BUDGET, bytes: tests)

struct ScOut { long long *n_kept; double *mean, *cov; long long *ev_hist, *tipping, *joint; };

// everything about the bounds, ev and ev_to_win: no device needed
int sc_check(const char *what, int S, const double *lo, const double *hi, const int32_t *ev, int ev_to_win, const ScOut &o, int *ev_sum) {
  if (S < 1 || S > OC_MAX_S) return fail(POTUS_ERR_UNSUPPORTED, "%s: S = %d (the kernels map the coordinates to the lanes of a wave: 1 .. %d)", what, S, OC_MAX_S);
  if ((lo == nullptr) != (hi == nullptr)) return fail(POTUS_ERR_ARG, "%s: lo and hi are given together or not at all", what);
  if (lo)
    for (int k = 0; k <= S; k++) {
      if (std::isnan(lo[k]) || std::isnan(hi[k])) return fail(POTUS_ERR_ARG, "%s: the bounds of coordinate %d hold a NaN", what, k);
      if (lo[k] >= hi[k]) return fail(POTUS_ERR_ARG, "%s: lo[%d] = %g is not below hi[%d] = %g (the interval is empty)", what, k, lo[k], k, hi[k]);
    }
  *ev_sum = 0;
  if (!ev) {
    if (o.ev_hist || o.tipping || o.joint) return fail(POTUS_ERR_ARG, "%s: ev is null, but a count output is asked for", what);
    return 0;
  }
  return oc_check(what, S, ev, ev_to_win, nullptr, ev_sum);
}

// The two-pass moments of the S + 1 coordinates of x [n][n_days][S] (w [S] on the device), in blocks of days that fit the scratch budget:
// *dmean [n_days][S + 1] and (want_cov) *dcov [n_days][S + 1][S + 1] on the device, owned by tmp; span times the kernels.  Queued on st, not waited for.
int sc_moments(const char *what, hipStream_t st, DevBufs &tmp, const double *x, long long n, int n_days, int S, const double *dw, bool want_cov, EventTimer &span,
               double **dmean_out, double **dcov_out) {
  const int C = S + 1;
  const size_t n_mean = (size_t)n_days * C, n_cov = (size_t)n_days * C * C;
  if (n > 65535ll * SC_CHUNK) return fail(POTUS_ERR_UNSUPPORTED, "%s: %lld kept draws (the moments take at most %lld)", what, n, 65535ll * SC_CHUNK);
  const int nchunks = (int)((n + SC_CHUNK - 1) / SC_CHUNK);
  const size_t per_day = ((size_t)n + (size_t)nchunks * (C + (want_cov ? (size_t)C * C : 0))) * 8;
  size_t budget = SC_SCRATCH_BUDGET;
  if (const char *e = getenv("POTUS_SCENARIO_SCRATCH_BUDGET")) budget = std::max<size_t>(1, (size_t)atoll(e));
  const int dblk = (int)std::min<size_t>((size_t)n_days, std::max<size_t>(1, budget / per_day));
  double *scratch = nullptr, *dmean = nullptr, *dcov = nullptr;
  if (const int rc_ = tmp.get(&scratch, per_day * dblk, what)) return rc_;
  if (const int rc_ = tmp.get(&dmean, n_mean * 8, what)) return rc_;
  if (want_cov) if (const int rc_ = tmp.get(&dcov, n_cov * 8, what)) return rc_;
  ScParams P{x, n, n_days, S, 0, nchunks, dw, scratch, scratch + (size_t)dblk * n, scratch + (size_t)dblk * n + (size_t)dblk * nchunks * C, dmean, dcov};
  const int NT = (C + 15) / 16;
  HIP_TRY(span.start(st));
  for (int d0 = 0; d0 < n_days; d0 += dblk) {
    P.day0 = d0;
    const dim3 grid((unsigned)std::min(dblk, n_days - d0), (unsigned)nchunks);
    hipLaunchKernelGGL(k_sc_nat, grid, dim3(SC_THREADS), 0, st, P);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sc_sum, grid, dim3(SC_THREADS), 0, st, P);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sc_finish_mean, dim3(grid.x), dim3(64), 0, st, P);
    HIP_TRY(hipGetLastError());
    if (!want_cov) continue;
    switch (NT) {
      case 1: hipLaunchKernelGGL(k_sc_gram<1>, grid, dim3(SC_THREADS), 0, st, P); break;
      case 2: hipLaunchKernelGGL(k_sc_gram<2>, grid, dim3(SC_THREADS), 0, st, P); break;
      case 3: hipLaunchKernelGGL(k_sc_gram<3>, grid, dim3(SC_THREADS), 0, st, P); break;
      default: hipLaunchKernelGGL(k_sc_gram<4>, grid, dim3(SC_THREADS), 0, st, P); break;
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sc_finish_cov, dim3(grid.x), dim3(SC_THREADS), 0, st, P);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(span.stop(st));
  *dmean_out = dmean; *dcov_out = dcov;
  return 0;
}

// items [nd][n_days][S] on the current device, in canonical order; the condition day's item of draw d at cond + d * cstride.
// Everything the call returns, in the caller's host arrays (any of them may be null).
int sc_compute(const char *what, hipStream_t st, const double *items, long long nd, int n_days, int S, const double *cond, long long cstride, const double *w,
               const double *lo, const double *hi, const int32_t *ev, int ev_to_win, int ev_sum, const ScOut &o) {
  const int C = S + 1;
  const long long rowlen = (long long)n_days * S;
  DevBufs tmp;
  EventTimer e;
  HIP_TRY(e.made);
  double *dw = nullptr;
  if (const int rc_ = tmp.get(&dw, (size_t)S * 8, what)) return rc_;
  HIP_TRY(hipMemcpyAsync(dw, w, (size_t)S * 8, hipMemcpyHostToDevice, st));
  // ---- keep + compact
  const double t0 = dn_now();
  const double *kept = items;
  long long n = nd;
  if (lo) {
    const long long nblk = (nd + SC_KEEP_BLOCK - 1) / SC_KEEP_BLOCK;
    double *dlh = nullptr;
    unsigned char *flag = nullptr;
    int *cnt = nullptr;
    long long *first = nullptr;
    if (const int rc_ = tmp.get(&dlh, (size_t)2 * C * 8, what)) return rc_;
    if (const int rc_ = tmp.get(&flag, (size_t)nd, what)) return rc_;
    if (const int rc_ = tmp.get(&cnt, (size_t)nblk * 4, what)) return rc_;
    if (const int rc_ = tmp.get(&first, (size_t)(nblk + 1) * 8, what)) return rc_;
    HIP_TRY(hipMemcpyAsync(dlh, lo, (size_t)C * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dlh + C, hi, (size_t)C * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sc_keep, dim3((unsigned)nblk), dim3(SC_THREADS), 0, st, cond, cstride, nd, S, (const double *)dw, (const double *)dlh, (const double *)(dlh + C), flag, cnt);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sc_scan, dim3(1), dim3(64), 0, st, (const int *)cnt, nblk, first);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&n, first + nblk, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n < 0 || n > nd) return fail(POTUS_ERR_DEVICE, "%s: the kept count %lld of %lld draws is out of range", what, n, nd);
    if (n > 0 && n < nd) {
      double *comp = nullptr;
      if (const int rc_ = tmp.get(&comp, (size_t)n * rowlen * 8, what)) return rc_;
      const unsigned slices = (unsigned)std::min<long long>(std::max<long long>(1, rowlen / 512), 64);
      hipLaunchKernelGGL(k_sc_compact, dim3((unsigned)nblk, slices), dim3(SC_THREADS), 0, st, items, nd, rowlen, (const unsigned char *)flag, (const long long *)first, comp);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(st));
      kept = comp;
    }
    g_sc_ms[2] = dn_now() - t0;
  }
  if (o.n_kept) *o.n_kept = n;
  // ---- moments
  const size_t n_mean = (size_t)n_days * C, n_cov = (size_t)n_days * C * C;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const bool want_mean = o.mean && n >= 1, want_cov = o.cov && n >= 2;
  if (o.mean && !want_mean) std::fill(o.mean, o.mean + n_mean, nan);
  if (o.cov && !want_cov) std::fill(o.cov, o.cov + n_cov, nan);
  if (want_mean || want_cov) {
    double *dmean = nullptr, *dcov = nullptr;
    if (const int rc_ = sc_moments(what, st, tmp, kept, n, n_days, S, dw, want_cov, e, &dmean, &dcov)) return rc_;
    if (want_mean) HIP_TRY(hipMemcpyAsync(o.mean, dmean, n_mean * 8, hipMemcpyDeviceToHost, st));
    if (want_cov) HIP_TRY(hipMemcpyAsync(o.cov, dcov, n_cov * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    (void)e.elapsed(&g_sc_ms[3]);
  }
  // ---- counts: potus_outcomes' own counting of the kept draws
  if (o.ev_hist || o.tipping || o.joint) {
    if (n == 0) {
      if (o.ev_hist) std::fill(o.ev_hist, o.ev_hist + (size_t)n_days * (ev_sum + 1), 0ll);
      if (o.tipping) std::fill(o.tipping, o.tipping + (size_t)n_days * (S + 1), 0ll);
      if (o.joint) std::fill(o.joint, o.joint + (size_t)n_days * (S + 2) * (S + 2), 0ll);
    } else {
      // (its time is the scenario's: potus_outcomes_timing keeps speaking of the last potus_outcomes call)
      return oc_count(what, st, kept, n, n_days, S, w, ev, ev_to_win, nullptr, ev_sum, OcOut{o.ev_hist, o.tipping, o.joint, nullptr, nullptr}, &g_sc_ms[4]);
    }
  }
  return 0;
}
} // namespace

int potus_scenario_device(int device, const void *block, long long n_draws, int n_days, int S, const double *w, int cond_day, const double *lo, const double *hi,
                          const int32_t *ev, int ev_to_win, long long *n_kept, double *mean, double *cov, long long *ev_hist, long long *tipping, long long *joint) {
  const char *what = "potus_scenario_device";
  if (!block || !w) return fail(POTUS_ERR_ARG, "%s: null block or weights", what);
  if (n_draws < 1) return fail(POTUS_ERR_ARG, "%s: %lld draws (at least one)", what, n_draws);
  if (n_draws > (1ll << 40)) return fail(POTUS_ERR_UNSUPPORTED, "%s: %lld draws (at most 2^40)", what, n_draws);
  if (n_days < 1) return fail(POTUS_ERR_ARG, "%s: %d days (at least one)", what, n_days);
  if (cond_day < 0 || cond_day >= n_days) return fail(POTUS_ERR_ARG, "%s: condition day %d of %d days", what, cond_day, n_days);
  const ScOut o{n_kept, mean, cov, ev_hist, tipping, joint};
  int ev_sum = 0;
  if (const int rc_ = sc_check(what, S, lo, hi, ev, ev_to_win, o, &ev_sum)) return rc_;
  for (int s = 0; s < S; s++) if (!std::isfinite(w[s])) return fail(POTUS_ERR_ARG, "%s: w[%d] is not finite", what, s);
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, device, block)) return rc_;
  for (double &x : g_sc_ms) x = 0.0;
  const double *items = (const double *)block;
  return sc_compute(what, 0, items, n_draws, n_days, S, items + (size_t)cond_day * S, (long long)n_days * S, w, lo, hi, ev, ev_to_win, ev_sum, o);
}

// Pooled over the post-warm-up draws of every listed sampler, as potus_outcomes pools them, but in CANONICAL order: chain after chain in the
// order the handles are listed, each chain's draws in iteration order (the row order of potus_extract_matrix) -- one k_oc_days launch per chain.
int potus_scenario(const int *handles, int n_handles, int cond_day, const double *lo, const double *hi, int day_begin, int day_end, const int32_t *ev, int ev_to_win,
                   long long *n_kept, long long *n_draws, double *mean, double *cov, long long *ev_hist, long long *tipping, long long *joint) {
  const char *what = "potus_scenario";
  if (!handles || n_handles < 1) return fail(POTUS_ERR_ARG, "%s: null handle list", what);
  Pool P;
  if (const int rc_ = P.resolve(handles, n_handles, what)) return rc_;
  if (const int rc_ = P.same_posterior("a scenario pools the chains of one")) return rc_;
  Sampler *s0 = P.s0;
  const int S = s0->M.S, T = s0->M.T;
  if (cond_day < 0 || cond_day >= T) return fail(POTUS_ERR_ARG, "%s: condition day %d of %d days", what, cond_day, T);
  const ScOut o{n_kept, mean, cov, ev_hist, tipping, joint};
  int ev_sum = 0;
  if (const int rc_ = sc_check(what, S, lo, hi, ev, ev_to_win, o, &ev_sum)) return rc_;
  DeviceGuard guard;
  DeviceLocks lock(P.devs);
  const bool cond_apart = lo && (cond_day < day_begin || cond_day >= day_end);   // the condition day as a one-day block of its own
  const int n_days = day_end - day_begin;
  DayItems g;
  if (const int rc_ = gather_days(P, day_begin, day_end, true, cond_apart ? cond_day : -1, g)) return rc_;
  for (double &x : g_sc_ms) x = 0.0;
  g_sc_ms[0] = g.gather_ms; g_sc_ms[1] = g.reshape_ms;
  if (n_draws) *n_draws = g.nd;
  const double *cond = cond_apart ? g.extra : g.items + (size_t)(cond_day - day_begin) * S;
  return sc_compute(what, s0->stream, g.items, g.nd, n_days, S, lo ? cond : nullptr, cond_apart ? (long long)S : (long long)n_days * S, s0->h_w.data(), lo, hi, ev,
                    ev_to_win, ev_sum, o);
}

int potus_scenario_timing(double *ms) {
  return timing_out("potus_scenario_timing", g_sc_ms, 5, ms);
}

// SURVEY 8(f4), "online R-hat-based early stop": the diagnostics of lp__ and mu_b[:, T] (the columns bench.py's ESS / s is defined on;
// predicted_score[T, :] is their inverse logit) over the post-warm-up draws saved SO FAR by the pooled chains of the handles.  The host loop
// that advances the sampler in chunks of `refresh` transitions may stop once *converged is set; nothing the sampler does depends on it (same
// draws up to that point as an uninterrupted run).  A deviation from Stan, which always runs num_samples iterations: off unless the host asks.
int potus_check_convergence(const int *handles, int n_handles, double rhat_below, double ess_at_least, int *converged, double *rhat_max, double *ess_bulk_min) {
  if (!handles || n_handles < 1 || !converged || !rhat_max || !ess_bulk_min) return fail(POTUS_ERR_ARG, "potus_check_convergence: null argument");
  Pool P;
  if (const int rc_ = P.lookup(handles, n_handles, "potus_check_convergence")) return rc_;
  if (const int rc_ = P.single_dataset()) return rc_;
  Sampler *s0 = P.s0;
  DeviceGuard guard;
  DeviceLocks lock(P.devs);                          // one set of locks for the count and both column ranges: no run on another host thread adds draws between them
  const int S = s0->M.S, T = s0->M.T, a_mu = POTUS_N_SAMPLER_COLS + s0->L.D + S * (T - 1);
  std::vector<double> rh(1 + S), es(1 + S);
  *converged = 0; *rhat_max = NAN; *ess_bulk_min = NAN;
  int rc;
  if ((rc = P.count())) return rc;
  if (P.saved[0] - warm_rows(s0, P.saved[0]) < 4) return 0;      // too early to say anything: not converged, no error (the list is looked at once there is something to say)
  if ((rc = P.distinct()) || (rc = P.same_posterior("R-hat / ESS pool the chains of one")) || (rc = P.equal_counts())) return rc;
  if ((rc = diagnostics_pooled(P, 0, 1, rh.data(), es.data()))) return rc;
  if ((rc = diagnostics_pooled(P, a_mu, a_mu + S, rh.data() + 1, es.data() + 1))) return rc;
  double r = -INFINITY, e = INFINITY;
  bool bad = false;
  for (int i = 0; i <= S; i++) { bad = bad || std::isnan(rh[i]) || std::isnan(es[i]); r = std::max(r, rh[i]); e = std::min(e, es[i]); }
  *rhat_max = bad ? NAN : r; *ess_bulk_min = bad ? NAN : e;
  *converged = (!bad && r < rhat_below && e >= ess_at_least) ? 1 : 0;
  return 0;
}

// The backtest scores of final_2016.R:925-945 (final_2012.R:918-931, final_2008.R:922-935) from the state summaries:
// with p_s = P(score > 0.5) of state s on `day` (1-based; 0 = the last day) and won_s the actual outcome,
//   out[0] = weighted.mean((won - p)^2, ev / sum(ev)), out[1] = mean((won - p)^2), out[2] = sum(round(p) == won)
// (R's round(): half to even).  Pure host arithmetic on the output of potus_posterior_summary.
int potus_backtest_scores(const double *state_out, int T, int S, int day, const double *ev, const int *won, double *out) {
  if (!state_out || !ev || !won || !out || T < 1 || S < 1 || day < 0 || day > T) return fail(POTUS_ERR_ARG, "potus_backtest_scores: bad argument");
  const int t = day == 0 ? T - 1 : day - 1;
  double evsum = 0, a = 0, b = 0;
  int correct = 0;
  for (int s = 0; s < S; s++) evsum += ev[s];
  if (!(evsum > 0)) return fail(POTUS_ERR_ARG, "potus_backtest_scores: electoral votes sum to %g", evsum);
  for (int s = 0; s < S; s++) {
    const double p = state_out[((size_t)t + (size_t)T * s) * 4 + 3], d = (double)won[s] - p;
    a += ev[s] / evsum * d * d;
    b += d * d;
    correct += (int)std::nearbyint(p) == won[s];
  }
  out[0] = a; out[1] = b / S; out[2] = correct;
  return 0;
}

int potus_last_run_timing(int handle, double *ms, long long *leapfrogs) {
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  if (ms) *ms = sp->last_ms;
  if (leapfrogs) *leapfrogs = sp->last_leapfrogs;
  return 0;
}

// CmdStan-format CSV, one file per chain (what rstan::read_stan_csv consumes, final_2016.R:543)
int potus_write_stan_csv(int handle, const char *dir, const char *basename) {
  Sampler *sp = get(handle);
  if (!sp || !dir || !basename) return fail(POTUS_ERR_STATE, "bad handle or null path");
  if (const int rc_ = refuse_many_datasets(sp, "potus_write_stan_csv")) return rc_;
  int n_saved = 0, rc = 0;
  { DeviceLocks lock0(sp->device); HIP_TRY(hipSetDevice(sp->device)); rc = saved_count(sp, &n_saved); }
  if (rc) return rc;
  const int chains = sp->R.chains, ncols = sp->L.ncols, D = sp->L.D;
  std::vector<double> eps(chains), minv((size_t)chains * D);
  if ((rc = potus_get_adaptation(handle, eps.data(), minv.data()))) return rc;
  // reconstruct a potus_data shell for the column names
  potus_data dd{}; dd.S = sp->M.S; dd.T = sp->M.T; dd.P = sp->M.P; dd.M = sp->M.M; dd.Pop = sp->M.Pop;
  dd.N_state_polls = sp->M.Ns; dd.N_national_polls = sp->M.Nn; dd.variant = sp->M.full ? POTUS_VARIANT_FULL : POTUS_VARIANT_NO_MODE;
  std::vector<FILE *> fp(chains, nullptr);
  auto close_all = [&]() { for (FILE *f : fp) if (f) fclose(f); };
  for (int c = 0; c < chains; c++) {
    const std::string path = std::string(dir) + "/" + basename + "-" + std::to_string(sp->R.chain_id_offset + c + 1) + ".csv";
    fp[c] = fopen(path.c_str(), "w");
    if (!fp[c]) { close_all(); return fail(POTUS_ERR_IO, "cannot open %s", path.c_str()); }
    FILE *f = fp[c];
    const potus_opts &o = sp->opts;
    fprintf(f, "# stan_version_major = 2\n# stan_version_minor = 24\n# stan_version_patch = 1\n");
    fprintf(f, "# model = %s\n", sp->M.full ? "poll_model_2020_model" : "poll_model_2020_no_mode_adjustment_model");
    fprintf(f, "# method = sample (Default)\n#   sample\n#     num_samples = %d\n#     num_warmup = %d\n#     save_warmup = %d\n#     thin = 1 (Default)\n",
            o.num_samples, o.num_warmup, o.save_warmup);
    fprintf(f, "#     adapt\n#       engaged = 1 (Default)\n#       gamma = %g\n#       delta = %g\n#       kappa = %g\n#       t0 = %g\n#       init_buffer = %d\n#       term_buffer = %d\n#       window = %d\n",
            o.gamma, o.delta, o.kappa, o.t0, sp->R.init_buffer, sp->R.term_buffer, sp->R.window);
    fprintf(f, "#     algorithm = hmc (Default)\n#       hmc\n#         engine = nuts (Default)\n#           nuts\n#             max_depth = %d\n#         metric = %s\n#         metric_file =  (Default)\n#         stepsize = %g\n#         stepsize_jitter = 0 (Default)\n",
            o.max_depth, sp->dense ? "dense_e" : "diag_e (Default)", o.stepsize);
    fprintf(f, "# id = %d\n# data\n#   file = (in-memory)\n# init = %g\n# random\n#   seed = %llu\n# output\n#   file = %s\n#   diagnostic_file =  (Default)\n#   refresh = 100 (Default)\n",
            sp->R.chain_id_offset + c + 1, o.init_radius, (unsigned long long)o.seed, path.c_str());
    // (not CmdStan's: what the library resolved cus_per_chain = 0 / twin = -1 to -- draws are reproducible bit for bit for a given pair)
    fprintf(f, "# potus_hmc\n#   cus_per_chain = %d\n#   clusters_per_chain = %d\n#   metric_storage = %s\n#   pooled_metric = %d\n", sp->K, sp->sides(), sp->dense && sp->dn.f32 ? "f32" : "f64",
            sp->dense && sp->dn.pooled ? 1 : 0);
    char name[96];
    for (int k = 0; k < ncols; k++) { potus_column_name(&dd, k, name, sizeof name); fprintf(f, k ? ",%s" : "%s", name); }
    fprintf(f, "\n");
  }
  // CmdStan writes the adaptation block when warm-up ends: straight after the header without save_warmup, after the
  // warm-up rows with it.  The text is prepared here, on the calling thread (the dense metric comes off the device), so that
  // the writer threads below only copy it.  dense_e: "# Elements of inverse mass matrix:" and D rows of D values, as CmdStan --
  // up to 2048 parameters; beyond that the matrix is left out TOGETHER WITH its header line (a reader that has seen the
  // header expects D rows; rstan keeps the block as text, potus_get_dense_metric returns the matrix).
  std::vector<std::string> adapt_txt(chains);
  for (int c = 0; c < chains; c++) {
    std::string &t = adapt_txt[c];
    char num[64];
    std::snprintf(num, sizeof num, "# Adaptation terminated\n# Step size = %.6g\n", eps[c]);
    t = num;
    auto put_row = [&](const double *v, int n) {
      t += "# ";
      for (int j = 0; j < n; j++) { std::snprintf(num, sizeof num, j ? ", %.6g" : "%.6g", v[j]); t += num; }
      t += "\n";
    };
    if (sp->dense) {
      if (D <= 2048) {
        std::vector<double> mm((size_t)D * D);
        if ((rc = potus_get_dense_metric(handle, c, mm.data()))) { close_all(); return rc; }
        t += "# Elements of inverse mass matrix:\n";
        for (int i = 0; i < D; i++) put_row(mm.data() + (size_t)i * D, D);
      } else {
        std::snprintf(num, sizeof num, "# (dense inverse metric, %d x %d", D, D);
        t += num;
        t += ": left out of the CSV, see potus_get_dense_metric)\n";
      }
    } else {
      t += "# Diagonal elements of inverse mass matrix:\n";
      put_row(minv.data() + (size_t)c * D, D);
    }
  }
  auto adaptation_block = [&](int c) { fwrite(adapt_txt[c].data(), 1, adapt_txt[c].size(), fp[c]); };
  const int n_warm_rows = warm_rows(sp, n_saved);
  if (n_warm_rows == 0) for (int c = 0; c < chains; c++) adaptation_block(c);
  // stream the rows in blocks of draws: rows come back as [iter][chain][ncols]
  const int blk = 32;
  std::vector<double> rows((size_t)blk * chains * ncols);
  Sampler view = *sp; // shallow copy to address a sub-range of iterations
  for (int i0 = 0; i0 < n_saved; i0 += blk) {
    const int nb = std::min(blk, n_saved - i0);
    view.R.draws = sp->R.draws + (size_t)i0 * sp->R.row;
    { DeviceLocks lockb(sp->device); rc = write_array_range(&view, nb, 0, ncols, rows.data()); }
    if (rc) { close_all(); return rc; }
    // one host thread per chain (up to the cores there are) turns its rows into text: "%.6g" through std::to_chars -- the same
    // characters as printf, a third faster, and the 347 M numbers of the 2016 fit (8 x 1000 x 43 360) no longer go through
    // one thread
    const int nthr = std::max(1, std::min(chains, (int)std::thread::hardware_concurrency()));
    std::vector<int> io_err(nthr, 0);
    auto work = [&](int j) {
      std::vector<char> txt((size_t)ncols * 26 + 2);
      for (int c = j; c < chains; c += nthr)
        for (int i = 0; i < nb; i++) {
          const double *r = rows.data() + ((size_t)i * chains + c) * ncols;
          char *q = txt.data();
          for (int k = 0; k < ncols; k++) {
            if (k) *q++ = ',';
            q = std::to_chars(q, q + 25, r[k], std::chars_format::general, 6).ptr;
          }
          *q++ = '\n';
          if (fwrite(txt.data(), 1, (size_t)(q - txt.data()), fp[c]) != (size_t)(q - txt.data())) io_err[j] = 1;
          if (n_warm_rows > 0 && i0 + i == n_warm_rows - 1) adaptation_block(c);
        }
    };
    std::vector<std::thread> pool;
    for (int j = 1; j < nthr; j++) pool.emplace_back(work, j);
    work(0);
    for (auto &t : pool) t.join();
    for (int e : io_err) if (e) { close_all(); return fail(POTUS_ERR_IO, "write to %s/%s-*.csv failed", dir, basename); }
  }
  for (int c = 0; c < chains; c++)
    fprintf(fp[c], "# \n#  Elapsed Time: %.3f seconds (Warm-up)\n#                %.3f seconds (Sampling)\n#                %.3f seconds (Total)\n# \n",
            sp->warm_ms * 1e-3, sp->samp_ms * 1e-3, (sp->warm_ms + sp->samp_ms) * 1e-3);
  close_all();
  return 0;
}

// ------------------------------------------------------------------------ simulation-based calibration (DESIGN.md "Simulation-based calibration")
// potus_set_datasets, potus_set_datasets_ex (ex: the four arrays may be null, the poll sizes and the prior may differ per data set, ds_ex is set)
// and potus_set_datasets_grid (ex with scales [n][POTUS_N_SCALES]: every piece of the model that a scale reaches is the data set's own)
static const char *const kScaleNames[POTUS_N_SCALES] = {"sigma_c", "sigma_m", "sigma_pop", "sigma_measure_noise_national", "sigma_measure_noise_state",
                                                        "sigma_e_bias", "random_walk_scale", "mu_b_T_scale", "polling_bias_scale"};
static int set_datasets_impl(const char *what, Sampler *sp, int n_datasets, const int32_t *y_state, const int32_t *y_national, const int32_t *n_state,
                             const int32_t *n_national, const double *mu_b_prior, const double *mu_b_T_scale, bool ex, const double *scales = nullptr) {
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  const int Ns = sp->M.Ns, Nn = sp->M.Nn, Np = Ns + Nn, Npad = sp->M.Npad, S = sp->M.S;
  if (n_datasets < 1) return fail(POTUS_ERR_ARG, "%s: n_datasets = %d, at least 1", what, n_datasets);
  if (scales && mu_b_T_scale) return fail(POTUS_ERR_ARG, "%s: both mu_b_T_scale[] and scales are given: scales[][%d] is mu_b_T_scale, pass one of the two", what, (int)SC_MU_B_T);
  if (!ex && ((Ns && !y_state) || (Nn && !y_national))) return fail(POTUS_ERR_ARG, "%s: null outcome array", what);
  if (sp->inited) return fail(POTUS_ERR_STATE, "%s: the handle is already initialised (call it between potus_create and potus_init)", what);
  if (sp->n_ds) return fail(POTUS_ERR_STATE, "%s: the handle already holds %d data sets", what, sp->n_ds);
  if (sp->dense) return fail(POTUS_ERR_UNSUPPORTED, "%s: the dense metric is not supported (metric = POTUS_METRIC_DIAG only)", what);
  if (sp->K != 1 || sp->twin) return fail(POTUS_ERR_UNSUPPORTED, "%s: needs one workgroup per chain (cus_per_chain = 1, twin = 0); this handle runs %d x %d", what, sp->K, sp->sides());
  if (sp->R.chains % n_datasets) return fail(POTUS_ERR_ARG, "%s: chains = %d is not a multiple of n_datasets = %d", what, sp->R.chains, n_datasets);
  if (mu_b_prior) for (size_t i = 0; i < (size_t)n_datasets * S; i++) if (!std::isfinite(mu_b_prior[i])) return fail(POTUS_ERR_ARG, "%s: data set %d: mu_b_prior is not finite", what, (int)(i / S) + 1);
  if (mu_b_T_scale) for (int k = 0; k < n_datasets; k++) if (!(mu_b_T_scale[k] > 0) || !std::isfinite(mu_b_T_scale[k])) return fail(POTUS_ERR_ARG, "%s: data set %d: mu_b_T_scale = %g, must be positive and finite", what, k + 1, mu_b_T_scale[k]);
  // the scales of every data set: the no-mode variant keeps the handle's own where it reads none (potus_create ignores them there).  potus_create
  // itself tests a scale only through the factorisation below; a grid names the data set and the scale before that
  std::vector<double> scs;
  if (scales) {
    scs.assign(scales, scales + (size_t)n_datasets * POTUS_N_SCALES);
    for (int k = 0; k < n_datasets; k++)
      for (int j = 0; j < POTUS_N_SCALES; j++) {
        double &v = scs[(size_t)k * POTUS_N_SCALES + j];
        if (!sp->M.full && (j == SC_M || j == SC_POP || j == SC_E_BIAS)) { v = sp->h_scales[j]; continue; }
        if (!(v > 0) || !std::isfinite(v)) return fail(POTUS_ERR_ARG, "%s: data set %d: %s = %g, must be positive and finite", what, k + 1, kScaleNames[j], v);
      }
  }
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  std::vector<double> base((size_t)4 * Npad);
  HIP_TRY(hipMemcpy(base.data(), sp->M.pd, base.size() * 8, hipMemcpyDeviceToHost));
  std::vector<double> pd((size_t)n_datasets * 4 * Npad);
  for (int k = 0; k < n_datasets; k++) {
    double *blk = pd.data() + (size_t)k * 4 * Npad;
    std::copy(base.begin(), base.end(), blk);
    for (int i = 0; i < Np; i++) {   // day-sorted poll i is state poll qidx - o_ns or national poll qidx - o_nn (build_model)
      const int qi = sp->h_pq[i];
      const bool nat = sp->h_ps[i] == S;
      const int j = nat ? qi - sp->M.o_nn : qi - sp->M.o_ns;
      const int32_t *ya = nat ? y_national : y_state, *na = nat ? n_national : n_state;
      const size_t at = (size_t)k * (nat ? Nn : Ns) + j;
      const double n = na ? (double)na[at] : base[(size_t)Npad + i], y = ya ? (double)ya[at] : base[i];
      if (ex && n < 0) return fail(POTUS_ERR_ARG, "%s: data set %d: n_two_share_%s[%d] = %d is negative", what, k + 1, nat ? "national" : "state", j + 1, (int)n);
      if (y < 0 || y > n) return fail(POTUS_ERR_ARG, "%s: data set %d: n_democrat_%s[%d] = %d outside [0,%d]", what, k + 1, nat ? "national" : "state", j + 1, (int)y, (int)n);
      blk[i] = y; blk[(size_t)Npad + i] = n;
      if (scales) blk[(size_t)3 * Npad + i] = poll_sigma(&scs[(size_t)k * POTUS_N_SCALES], nat);
    }
  }
  const double *dpd = nullptr;
  if (const int rc = upload(sp, pd, &dpd)) return rc;
  std::vector<DevModel> ms(n_datasets, sp->M);
  for (int k = 0; k < n_datasets; k++) ms[k].pd = dpd + (size_t)k * 4 * Npad;
  if (scales) {   // own sigma fields, aT, aB and seg_scale, by build_model's code.  Sizes, offsets, the LDS layout and the schedule are the handle's: no scale reaches them
    const size_t nseg = sp->h_seg_src.size();
    if ((int)nseg != sp->M.nseg) return fail(POTUS_ERR_STATE, "%s: internal: %zu segment scales for %d segments", what, nseg, sp->M.nseg);
    std::vector<double> segs;
    for (int k = 0; k < n_datasets; k++) {
      const double *sc = &scs[(size_t)k * POTUS_N_SCALES];
      const DevModel before = ms[k];
      model_scales(ms[k], sc);
      const std::vector<double> one = seg_scales(sp->h_seg_src, sc);
      segs.insert(segs.end(), one.begin(), one.end());
      DevModel same = ms[k];   // everything but the eight scalars is untouched
      same.sigma_c = before.sigma_c; same.sigma_m = before.sigma_m; same.sigma_pop = before.sigma_pop; same.sigma_e = before.sigma_e;
      same.sigma_ns = before.sigma_ns; same.sigma_nn = before.sigma_nn; same.aT = before.aT; same.aB = before.aB;
      if (std::memcmp(&same, &before, sizeof(DevModel)) != 0) return fail(POTUS_ERR_STATE, "%s: internal: a scale changed the layout of data set %d", what, k + 1);
    }
    const double *dseg = nullptr;
    if (const int rc = upload(sp, segs, &dseg)) return rc;
    for (int k = 0; k < n_datasets; k++) ms[k].seg_scale = dseg + (size_t)k * nseg;
  }
  if (mu_b_prior || mu_b_T_scale || scales) {   // own mat and aT: the blocks build_model derives from the prior and the scales, by its code
    const size_t nm = sp->h_mat.size();
    std::vector<double> mats((size_t)n_datasets * nm);
    for (int k = 0; k < n_datasets; k++) {
      double *m = mats.data() + (size_t)k * nm;
      std::copy(sp->h_mat.begin(), sp->h_mat.end(), m);
      PriorBlocks pb;
      const double *sc = scales ? &scs[(size_t)k * POTUS_N_SCALES] : nullptr;
      const double scale = sc ? sc[SC_MU_B_T] : mu_b_T_scale ? mu_b_T_scale[k] : sp->h_T_scale;
      const double *prior = mu_b_prior ? mu_b_prior + (size_t)k * S : sp->h_mat.data() + sp->M.m_prior;
      if (!prior_blocks(sp->h_cov, sp->h_nsd, sp->h_w_raw, S, prior, scale, pb)) return fail(POTUS_ERR_ARG, "%s: data set %d: the covariance scaled by mu_b_T_scale = %g is not positive definite", what, k + 1, scale);
      std::copy(pb.LT_t.begin(), pb.LT_t.end(), m + sp->M.m_LTt);
      std::copy(pb.LTr.begin(), pb.LTr.end(), m + sp->M.m_LT);
      if (!sc) ms[k].aT = std::fabs(scale / sp->h_rw_scale);
      std::copy(pb.prior.begin(), pb.prior.end(), m + sp->M.m_prior);
      std::copy(pb.px.begin(), pb.px.end(), m + sp->M.m_priorx);
      if (sc) {   // Lw_ext (mat starts with it), LB_t and LB
        ScaleBlocks sb;
        if (!scale_blocks(sp->h_cov, sp->h_nsd, sp->h_w_raw, S, sp->M.SE, sp->M.SP, sc[SC_RANDOM_WALK], sc[SC_POLLING_BIAS], sb))
          return fail(POTUS_ERR_ARG, "%s: data set %d: the covariance scaled by random_walk_scale = %g or polling_bias_scale = %g is not positive definite", what, k + 1, sc[SC_RANDOM_WALK], sc[SC_POLLING_BIAS]);
        if (sb.Lw_ext.size() > (size_t)sp->M.m_LTt || sp->M.m_LBt + sb.LB_t.size() > nm || sp->M.m_LB + sb.LBr.size() > nm)
          return fail(POTUS_ERR_STATE, "%s: internal: the blocks of data set %d do not fit the handle's mat", what, k + 1);
        std::copy(sb.Lw_ext.begin(), sb.Lw_ext.end(), m);
        std::copy(sb.LB_t.begin(), sb.LB_t.end(), m + sp->M.m_LBt);
        std::copy(sb.LBr.begin(), sb.LBr.end(), m + sp->M.m_LB);
      }
    }
    const double *dmat = nullptr;
    if (const int rc = upload(sp, mats, &dmat)) return rc;
    for (int k = 0; k < n_datasets; k++) ms[k].mat = dmat + (size_t)k * nm;
    sp->ds_own_prior = true;
  }
  const DevModel *dms = nullptr;
  if (const int rc = upload(sp, ms, &dms)) return rc;
  sp->dMs = const_cast<DevModel *>(dms);
  sp->n_ds = n_datasets;
  if (ex) sp->ds_ex = true;
  if (scales) sp->ds_grid = true;
  return 0;
}

int potus_set_datasets(int handle, int n_datasets, const int32_t *n_democrat_state, const int32_t *n_democrat_national) {
  return set_datasets_impl("potus_set_datasets", get(handle), n_datasets, n_democrat_state, n_democrat_national, nullptr, nullptr, nullptr, nullptr, false);
}

// Run dates as data sets: every data set may have its own poll sizes (0 = it has not seen the poll), prior and scale.
int potus_set_datasets_ex(int handle, int n_datasets, const int32_t *n_democrat_state, const int32_t *n_democrat_national,
                          const int32_t *n_two_share_state, const int32_t *n_two_share_national, const double *mu_b_prior, const double *mu_b_T_scale) {
  return set_datasets_impl("potus_set_datasets_ex", get(handle), n_datasets, n_democrat_state, n_democrat_national, n_two_share_state, n_two_share_national,
                           mu_b_prior, mu_b_T_scale, true);
}

// Prior settings as data sets: potus_set_datasets_ex, and every data set with the nine scales of its own.
int potus_set_datasets_grid(int handle, int n_datasets, const int32_t *n_democrat_state, const int32_t *n_democrat_national,
                            const int32_t *n_two_share_state, const int32_t *n_two_share_national, const double *mu_b_prior, const double *mu_b_T_scale,
                            const double *scales) {
  return set_datasets_impl("potus_set_datasets_grid", get(handle), n_datasets, n_democrat_state, n_democrat_national, n_two_share_state, n_two_share_national,
                           mu_b_prior, mu_b_T_scale, true, scales);
}

namespace {
thread_local double g_tl_ms[2] = {0.0, 0.0};   // the last call of this thread: k_tl_scores, k_tl_summary (HIP events)

struct TlPlan : DsPlan { int nd = 0; };
// everything potus_timeline[_scores_device] checks before a kernel runs; the argument tests come before the first HIP call
int tl_check_args(const char *what, Sampler *sp, int day_begin, int day_end, TlPlan &pl) {
  pl.of(sp); pl.nd = day_end - day_begin;
  if (day_begin < 0 || day_end > sp->M.T || day_begin >= day_end) return fail(POTUS_ERR_ARG, "%s: bad day range [%d,%d) of %d days", what, day_begin, day_end, sp->M.T);
  if ((long long)pl.cpd * sp->R.num_samples > TL_MAX_DRAWS)
    return fail(POTUS_ERR_UNSUPPORTED, "%s: %d chains x %d draws per data set: a data set's draws are sorted in LDS, at most %d", what, pl.cpd, sp->R.num_samples, TL_MAX_DRAWS);
  if (sp->K != 1 || sp->twin || sp->dense) return fail(POTUS_ERR_UNSUPPORTED, "%s: needs one workgroup per chain and the diagonal metric (the handles potus_set_datasets[_ex] take)", what);
  return 0;
}
int tl_scores(Sampler *sp, const TlPlan &pl, int day_begin, int day_end, const int *dskip, double *out) {
  const long long items = (long long)sp->R.chains * pl.n_post;
  TlScoreParams P{row_src(sp, pl.first), pl.n_post, pl.cpd, day_begin, day_end, dskip, out};
  hipLaunchKernelGGL(k_tl_scores, dim3((unsigned)std::min<long long>((items + 3) / 4, 65535)), dim3(256), 0, sp->stream, pl.Mg, P);
  HIP_TRY(hipGetLastError());
  return 0;
}
} // namespace

int potus_timeline_scores_device(int handle, int day_begin, int day_end, void *out_device) {
  const char *what = "potus_timeline_scores_device";
  Sampler *sp = get(handle);
  if (!sp || !out_device) return fail(POTUS_ERR_STATE, "bad handle or null output");
  TlPlan pl;
  if (const int rc_ = tl_check_args(what, sp, day_begin, day_end, pl)) return rc_;
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, sp->device, out_device, "output")) return rc_;
  if (const int rc_ = ds_plan(what, sp, pl)) return rc_;
  DevBufs tmp;
  int *dskip = nullptr;
  if (const int rc_ = tmp.get(&dskip, (size_t)pl.n_ds * 4, what)) return rc_;
  HIP_TRY(hipMemcpyAsync(dskip, pl.skip.data(), (size_t)pl.n_ds * 4, hipMemcpyHostToDevice, sp->stream));
  if (const int rc_ = tl_scores(sp, pl, day_begin, day_end, dskip, (double *)out_device)) return rc_;
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

int potus_timeline(int handle, int day_begin, int day_end, const double *ev, int ev_to_win, double *state_out, double *natl_out, double *ev_out, int32_t *n_draws_out) {
  const char *what = "potus_timeline";
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  if (!ev || !state_out || !natl_out || !ev_out || !n_draws_out) return fail(POTUS_ERR_ARG, "%s: null argument", what);
  TlPlan pl;
  if (const int rc_ = tl_check_args(what, sp, day_begin, day_end, pl)) return rc_;
  DeviceGuard guard;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  if (const int rc_ = ds_plan(what, sp, pl)) return rc_;
  const int S = sp->M.S, nd = pl.nd, n = pl.cpd * pl.n_post, n_ds = pl.n_ds;
  DevBufs tmp;
  EventTimer e0, e1;
  HIP_TRY(e0.made); HIP_TRY(e1.made);
  double *x = nullptr, *dw = nullptr, *dev_ = nullptr, *dout = nullptr;
  int *dskip = nullptr;
  int rc;
  const size_t n_out = (size_t)n_ds * nd * ((size_t)S * 4 + 9);
  if ((rc = tmp.get(&x, (size_t)n_ds * n * nd * S * 8, what)) || (rc = tmp.get(&dw, (size_t)S * 8, what)) || (rc = tmp.get(&dev_, (size_t)S * 8, what)) ||
      (rc = tmp.get(&dout, n_out * 8, what)) || (rc = tmp.get(&dskip, (size_t)n_ds * 4, what))) return rc;
  HIP_TRY(hipMemcpyAsync(dskip, pl.skip.data(), (size_t)n_ds * 4, hipMemcpyHostToDevice, sp->stream));
  HIP_TRY(hipMemcpyAsync(dw, sp->h_w.data(), (size_t)S * 8, hipMemcpyHostToDevice, sp->stream));
  HIP_TRY(hipMemcpyAsync(dev_, ev, (size_t)S * 8, hipMemcpyHostToDevice, sp->stream));
  HIP_TRY(e0.start(sp->stream));
  if ((rc = tl_scores(sp, pl, day_begin, day_end, dskip, x))) return rc;
  HIP_TRY(e0.stop(sp->stream));
  int npad = 1;
  while (npad < n) npad <<= 1;
  const size_t lds = (size_t)npad * 8;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_tl_summary), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  double *o_state = dout, *o_natl = o_state + (size_t)n_ds * nd * S * 4, *o_ev = o_natl + (size_t)n_ds * nd * 4;
  TlSumParams Q{x, n_ds, n, nd, S, dw, dev_, (double)ev_to_win, dskip, o_state, o_natl, o_ev};
  HIP_TRY(e1.start(sp->stream));
  hipLaunchKernelGGL(k_tl_summary, dim3((unsigned)std::min<long long>((long long)n_ds * nd * (S + 2), 65535)), dim3(TL_THREADS), lds, sp->stream, Q);
  HIP_TRY(hipGetLastError());
  HIP_TRY(e1.stop(sp->stream));
  HIP_TRY(hipMemcpyAsync(state_out, o_state, (size_t)n_ds * nd * S * 4 * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipMemcpyAsync(natl_out, o_natl, (size_t)n_ds * nd * 4 * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipMemcpyAsync(ev_out, o_ev, (size_t)n_ds * nd * 5 * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  double ms0 = 0, ms1 = 0;
  if ((rc = e0.elapsed_or_fail(&ms0)) || (rc = e1.elapsed_or_fail(&ms1))) return rc;
  g_tl_ms[0] = ms0; g_tl_ms[1] = ms1;
  for (int k = 0; k < n_ds; k++) n_draws_out[k] = pl.skip[k] ? 0 : n;
  return 0;
}

int potus_timeline_timing(double *ms) {
  return timing_out("potus_timeline_timing", g_tl_ms, 2, ms);
}

// ---------------------------------------------------------------------------------------------- prior sensitivity by refit (potus_sens.hpp)
namespace {
thread_local double g_sg_ms[2] = {0.0, 0.0};   // the last call of this thread: k_tl_scores, k_sg_distance / k_sg_grid (HIP events)
constexpr int SG_MAX_GRID = 512;               // workgroups of a launch: with the largest samples one is resident per CU, more columns are grid-strided

int sg_check_sizes(const char *what, long long n_a, long long n_b) {
  if (n_a < 1 || n_b < 1) return fail(POTUS_ERR_ARG, "%s: n_a = %lld, n_b = %lld, at least one draw each", what, n_a, n_b);
  if (n_a + n_b > SG_MAX_N)
    return fail(POTUS_ERR_UNSUPPORTED, "%s: n_a + n_b = %lld + %lld = %lld: both samples of a column are sorted in LDS, at most %d draws together", what, n_a, n_b,
                n_a + n_b, SG_MAX_N);
  return 0;
}
} // namespace

int potus_ecdf_distance_device(int device, const void *a, int n_a, const void *b, int n_b, int n_cols, double *out) {
  const char *what = "potus_ecdf_distance_device";
  if (!a || !b || !out || n_cols < 1) return fail(POTUS_ERR_ARG, "%s: bad argument", what);
  if (const int rc_ = sg_check_sizes(what, n_a, n_b)) return rc_;
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, device, a, "block a")) return rc_;
  if (const int rc_ = mm_also_device(what, device, b, "block b")) return rc_;
  DevBufs tmp;
  double *dout = nullptr;
  if (const int rc_ = tmp.get(&dout, (size_t)n_cols * 3 * 8, what)) return rc_;
  const size_t lds = (size_t)(n_a + n_b) * 8;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sg_distance), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  EventTimer t;
  HIP_TRY(t.made);
  HIP_TRY(t.start(0));
  hipLaunchKernelGGL(k_sg_distance, dim3((unsigned)std::min(n_cols, SG_MAX_GRID)), dim3(SG_THREADS), lds, 0, (const double *)a, n_a, (const double *)b, n_b, n_cols, dout);
  HIP_TRY(hipGetLastError());
  HIP_TRY(t.stop(0));
  HIP_TRY(hipMemcpy(out, dout, (size_t)n_cols * 3 * 8, hipMemcpyDeviceToHost));
  double ms = 0;
  if (const int rc_ = t.elapsed_or_fail(&ms)) return rc_;
  g_sg_ms[0] = 0.0; g_sg_ms[1] = ms;
  return 0;
}

int potus_grid_compare(int handle, int base, int day_begin, int day_end, const double *ev, int ev_to_win, double *out, int32_t *n_draws_out) {
  const char *what = "potus_grid_compare";
  (void)ev_to_win;   // the electoral votes of a draw are compared as a count; the threshold is part of potus_timeline's summary only
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  if (!ev || !out || !n_draws_out) return fail(POTUS_ERR_ARG, "%s: null argument", what);
  TlPlan pl;
  if (const int rc_ = tl_check_args(what, sp, day_begin, day_end, pl)) return rc_;
  if (base < 0 || base >= pl.n_ds) return fail(POTUS_ERR_ARG, "%s: base = %d outside the handle's %d data sets", what, base, pl.n_ds);
  DeviceGuard guard;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  if (const int rc_ = ds_plan(what, sp, pl)) return rc_;
  const int S = sp->M.S, nd = pl.nd, n = pl.cpd * pl.n_post, n_ds = pl.n_ds;
  if (const int rc_ = sg_check_sizes(what, n, n)) return rc_;
  DevBufs tmp;
  EventTimer e0, e1;
  HIP_TRY(e0.made); HIP_TRY(e1.made);
  double *x = nullptr, *dw = nullptr, *dev_ = nullptr, *dout = nullptr;
  int *dskip = nullptr;
  int rc;
  const size_t n_out = (size_t)n_ds * nd * (S + 2) * 3;
  if ((rc = tmp.get(&x, (size_t)n_ds * n * nd * S * 8, what)) || (rc = tmp.get(&dw, (size_t)S * 8, what)) || (rc = tmp.get(&dev_, (size_t)S * 8, what)) ||
      (rc = tmp.get(&dout, n_out * 8, what)) || (rc = tmp.get(&dskip, (size_t)n_ds * 4, what))) return rc;
  HIP_TRY(hipMemcpyAsync(dskip, pl.skip.data(), (size_t)n_ds * 4, hipMemcpyHostToDevice, sp->stream));
  HIP_TRY(hipMemcpyAsync(dw, sp->h_w.data(), (size_t)S * 8, hipMemcpyHostToDevice, sp->stream));
  HIP_TRY(hipMemcpyAsync(dev_, ev, (size_t)S * 8, hipMemcpyHostToDevice, sp->stream));
  HIP_TRY(e0.start(sp->stream));
  if ((rc = tl_scores(sp, pl, day_begin, day_end, dskip, x))) return rc;
  HIP_TRY(e0.stop(sp->stream));
  const size_t lds = (size_t)2 * n * 8;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sg_grid), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  SgGridParams Q{x, n_ds, n, nd, S, base, dw, dev_, dskip, dout};
  HIP_TRY(e1.start(sp->stream));
  hipLaunchKernelGGL(k_sg_grid, dim3((unsigned)std::min<long long>((long long)n_ds * nd * (S + 2), SG_MAX_GRID)), dim3(SG_THREADS), lds, sp->stream, Q);
  HIP_TRY(hipGetLastError());
  HIP_TRY(e1.stop(sp->stream));
  HIP_TRY(hipMemcpyAsync(out, dout, n_out * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  double ms0 = 0, ms1 = 0;
  if ((rc = e0.elapsed_or_fail(&ms0)) || (rc = e1.elapsed_or_fail(&ms1))) return rc;
  g_sg_ms[0] = ms0; g_sg_ms[1] = ms1;
  for (int k = 0; k < n_ds; k++) n_draws_out[k] = pl.skip[k] || pl.skip[base] ? 0 : n;
  return 0;
}

int potus_grid_timing(double *ms) {
  return timing_out("potus_grid_timing", g_sg_ms, 2, ms);
}

// ---------------------------------------------------------------------------------------------- scoring rules of the joint forecast (potus_fscore.hpp)
namespace {
thread_local double g_fs_ms[4] = {0.0, 0.0, 0.0, 0.0};   // the last call of this thread: columns, energy, variogram, joint DSS (HIP events)
constexpr int FS_MAX_GRID = 4096;                        // workgroups of the tile launch; more tiles are grid-strided

// everything about S, ev, actual, use and vs_p: no device needed.  used = the used states, ascending
int fs_check(const char *what, int S, const double *ev, const double *actual, const int32_t *use, double vs_p, std::vector<int> &used) {
  if (S < 1 || S > FS_MAX_S) return fail(POTUS_ERR_UNSUPPORTED, "%s: S = %d (the used states of a draw sit in the registers of a lane: 1 .. %d)", what, S, FS_MAX_S);
  if (!ev || !actual || !use) return fail(POTUS_ERR_ARG, "%s: null ev, actual or use", what);
  for (int s = 0; s < S; s++) if (!std::isfinite(ev[s])) return fail(POTUS_ERR_ARG, "%s: ev[%d] is not finite", what, s);
  for (int c = 0; c < S + 2; c++) {
    if (!std::isfinite(actual[c])) return fail(POTUS_ERR_ARG, "%s: actual[%d] is not finite", what, c);
    if (c <= S && !(actual[c] >= 0.0 && actual[c] <= 1.0)) return fail(POTUS_ERR_ARG, "%s: actual[%d] = %g outside [0, 1]", what, c, actual[c]);
  }
  used.clear();
  for (int s = 0; s < S; s++) {
    if (use[s] != 0 && use[s] != 1) return fail(POTUS_ERR_ARG, "%s: use[%d] = %d (0 or 1)", what, s, use[s]);
    if (use[s]) used.push_back(s);
  }
  if (used.empty()) return fail(POTUS_ERR_ARG, "%s: use is all zero (no state enters the multivariate scores)", what);
  if (!(vs_p > 0.0 && vs_p <= 2.0)) return fail(POTUS_ERR_ARG, "%s: vs_p = %g outside (0, 2]", what, vs_p);
  return 0;
}
int fs_check_draws(const char *what, long long n) {
  if (n < 1) return fail(POTUS_ERR_ARG, "%s: %lld draws (at least one)", what, n);
  if (n > PS_RUN) return fail(POTUS_ERR_UNSUPPORTED, "%s: %lld draws: a column's draws are sorted in LDS, at most %d", what, n, PS_RUN);
  return 0;
}

// x [n_ds][n][nd][S] on the current device, every data set's draws in canonical order -> uni_out [n_ds][nd][S + 2][7], multi_out [n_ds][nd][3] on the host
int fs_compute(const char *what, hipStream_t st, const double *x, int n_ds, int n, int nd, int S, const double *w, const double *ev, const double *actual,
               const std::vector<int> &used, double vs_p, double *uni_out, double *multi_out) {
  const int m = (int)used.size();
  const long long days = (long long)n_ds * nd;
  const int nt = (n + FS_TILE - 1) / FS_TILE, tiles = nt * (nt + 1) / 2;
  if (days * tiles > (1ll << 31) || days > (1 << 24)) return fail(POTUS_ERR_UNSUPPORTED, "%s: %lld days of %d tiles of pairs (at most 2^31 tiles)", what, days, tiles);
  const size_t n_uni = (size_t)days * (S + 2) * FS_NUNI, n_multi = (size_t)days * FS_NMULTI;
  DevBufs tmp;
  EventTimer e[3];   // the columns, the energy score, the variogram score
  for (EventTimer &t : e) HIP_TRY(t.made);
  double *dw = nullptr, *dev_ = nullptr, *dact = nullptr, *duni = nullptr, *dmulti = nullptr, *part = nullptr;
  int *duidx = nullptr, *dflag = nullptr;
  int rc;
  if ((rc = tmp.get(&dw, (size_t)S * 8, what)) || (rc = tmp.get(&dev_, (size_t)S * 8, what)) || (rc = tmp.get(&dact, (size_t)(S + 2) * 8, what)) ||
      (rc = tmp.get(&duidx, (size_t)m * 4, what)) || (rc = tmp.get(&duni, n_uni * 8, what)) || (rc = tmp.get(&dmulti, n_multi * 8, what)) ||
      (rc = tmp.get(&dflag, (size_t)days * 4, what)) || (rc = tmp.get(&part, (size_t)days * tiles * 2 * 8, what))) return rc;
  HIP_TRY(hipMemcpyAsync(dw, w, (size_t)S * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(dev_, ev, (size_t)S * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(dact, actual, (size_t)(S + 2) * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(duidx, used.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
  const FsParams P{x, n_ds, n, nd, S, m, dw, dev_, dact, duidx, vs_p, vs_p == 0.5 ? 1 : vs_p == 1.0 ? 2 : vs_p == 2.0 ? 3 : 0};
  // ---- the columns
  const size_t lds = (size_t)n * 8;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fs_column), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HIP_TRY(e[0].start(st));
  hipLaunchKernelGGL(k_fs_column, dim3((unsigned)std::min<long long>(days * (S + 2), 65535)), dim3(PS_THREADS), lds, st, P, duni);
  HIP_TRY(hipGetLastError());
  HIP_TRY(e[0].stop(st));
  // ---- the variogram score, and the flag of every day
  HIP_TRY(e[2].start(st));
  hipLaunchKernelGGL(k_fs_variogram, dim3((unsigned)std::min<long long>(days, 65535)), dim3(FS_VTHREADS), 0, st, P, dmulti, dflag);
  HIP_TRY(hipGetLastError());
  HIP_TRY(e[2].stop(st));
  // ---- the energy score: the tiles, then their partials in tile order
  const unsigned grid = (unsigned)std::min<long long>(days * tiles, FS_MAX_GRID);
  HIP_TRY(e[1].start(st));
  switch ((m + 7) / 8) {   // the used states of a draw, padded to a multiple of eight, are the registers of a lane
    case 1: hipLaunchKernelGGL(k_fs_energy<8>, dim3(grid), dim3(FS_ETHREADS), 0, st, P, part); break;
    case 2: hipLaunchKernelGGL(k_fs_energy<16>, dim3(grid), dim3(FS_ETHREADS), 0, st, P, part); break;
    case 3: hipLaunchKernelGGL(k_fs_energy<24>, dim3(grid), dim3(FS_ETHREADS), 0, st, P, part); break;
    case 4: hipLaunchKernelGGL(k_fs_energy<32>, dim3(grid), dim3(FS_ETHREADS), 0, st, P, part); break;
    case 5: hipLaunchKernelGGL(k_fs_energy<40>, dim3(grid), dim3(FS_ETHREADS), 0, st, P, part); break;
    case 6: hipLaunchKernelGGL(k_fs_energy<48>, dim3(grid), dim3(FS_ETHREADS), 0, st, P, part); break;
    case 7: hipLaunchKernelGGL(k_fs_energy<56>, dim3(grid), dim3(FS_ETHREADS), 0, st, P, part); break;
    default: hipLaunchKernelGGL(k_fs_energy<64>, dim3(grid), dim3(FS_ETHREADS), 0, st, P, part); break;
  }
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_fs_energy_finish, dim3((unsigned)days), dim3(64), 0, st, (const double *)part, n, tiles, (const int *)dflag, dmulti);
  HIP_TRY(hipGetLastError());
  HIP_TRY(e[1].stop(st));
  // ---- the joint Dawid-Sebastiani score, data set after data set: scenario's two-pass moments, then one workgroup per day.  The moments'
  // scratch (up to SC_SCRATCH_BUDGET), mean and covariance are one data set's at a time: given back before the next one takes its own.
  // (n <= m: no covariance of full rank, the score is NaN whatever the draws are)
  std::vector<std::unique_ptr<EventTimer>> ed;   // per data set: its moments, its factor and solve
  for (int k = 0; k < n_ds && n > m; k++) {
    for (int j = 0; j < 2; j++) { ed.emplace_back(new EventTimer()); HIP_TRY(ed.back()->made); }
    EventTimer &e_mom = *ed[2 * k], &e_fac = *ed[2 * k + 1];
    double *dmean = nullptr, *dcov = nullptr;
    DevBufs own;
    FsParams Pk = P;
    Pk.x = x + (size_t)k * n * nd * S;
    if ((rc = sc_moments(what, st, own, Pk.x, n, nd, S, dw, true, e_mom, &dmean, &dcov))) return rc;
    HIP_TRY(e_fac.start(st));
    hipLaunchKernelGGL(k_fs_dss, dim3((unsigned)nd), dim3(256), 0, st, Pk, (const double *)dmean, (const double *)dcov, (const int *)(dflag + (size_t)k * nd),
                       dmulti + (size_t)k * nd * FS_NMULTI);
    HIP_TRY(hipGetLastError());
    HIP_TRY(e_fac.stop(st));
    HIP_TRY(hipStreamSynchronize(st));   // before `own` frees what the kernels read
  }
  HIP_TRY(hipMemcpyAsync(uni_out, duni, n_uni * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(multi_out, dmulti, n_multi * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (n <= m) for (long long d = 0; d < days; d++) multi_out[d * FS_NMULTI + 2] = std::numeric_limits<double>::quiet_NaN();
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < 3; k++) if ((rc = e[k].elapsed_or_fail(&ms[k]))) return rc;
  for (auto &t : ed) { double v = 0.0; if ((rc = t->elapsed_or_fail(&v))) return rc; ms[3] += v; }
  std::copy(ms, ms + 4, g_fs_ms);
  return 0;
}
} // namespace

int potus_forecast_scores_device(int device, const void *block, long long n_draws, int n_days, int S, const double *w, const double *ev, int ev_to_win,
                                 const double *actual, const int32_t *use, double vs_p, double *uni_out, double *multi_out) {
  const char *what = "potus_forecast_scores_device";
  (void)ev_to_win;   // the electoral votes of a draw are scored as a count
  if (!block || !w || !uni_out || !multi_out) return fail(POTUS_ERR_ARG, "%s: null block, weights or output", what);
  if (n_days < 1) return fail(POTUS_ERR_ARG, "%s: %d days (at least one): a bad day range", what, n_days);
  std::vector<int> used;
  if (const int rc_ = fs_check(what, S, ev, actual, use, vs_p, used)) return rc_;
  if (const int rc_ = fs_check_draws(what, n_draws)) return rc_;
  for (int s = 0; s < S; s++) if (!std::isfinite(w[s])) return fail(POTUS_ERR_ARG, "%s: w[%d] is not finite", what, s);
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, device, block)) return rc_;
  return fs_compute(what, 0, (const double *)block, 1, (int)n_draws, n_days, S, w, ev, actual, used, vs_p, uni_out, multi_out);
}

// Pooled over the post-warm-up draws of every listed sampler in CANONICAL order, exactly as potus_scenario pools them.
int potus_forecast_scores(const int *handles, int n_handles, int day_begin, int day_end, const double *ev, int ev_to_win, const double *actual,
                          const int32_t *use, double vs_p, double *uni_out, double *multi_out, long long *n_draws_out) {
  const char *what = "potus_forecast_scores";
  (void)ev_to_win;
  if (!handles || n_handles < 1) return fail(POTUS_ERR_ARG, "%s: null handle list", what);
  if (!uni_out || !multi_out) return fail(POTUS_ERR_ARG, "%s: null output", what);
  Pool P;
  if (const int rc_ = P.resolve(handles, n_handles, what)) return rc_;
  if (const int rc_ = P.same_posterior("the scores pool the chains of one")) return rc_;
  Sampler *s0 = P.s0;
  const int S = s0->M.S, T = s0->M.T;
  std::vector<int> used;
  if (const int rc_ = fs_check(what, S, ev, actual, use, vs_p, used)) return rc_;
  if (day_begin < 0 || day_end > T || day_begin >= day_end) return fail(POTUS_ERR_ARG, "%s: bad day range [%d,%d) of %d days", what, day_begin, day_end, T);
  long long most = 0;
  for (const Sampler *sp : P.sps) most += (long long)sp->R.chains * sp->R.num_samples;
  if (const int rc_ = fs_check_draws(what, std::max<long long>(most, 1))) return rc_;
  DeviceGuard guard;
  DeviceLocks lock(P.devs);
  DayItems g;
  if (const int rc_ = gather_days(P, day_begin, day_end, true, -1, g)) return rc_;
  if (const int rc_ = fs_check_draws(what, g.nd)) return rc_;
  if (n_draws_out) *n_draws_out = g.nd;
  return fs_compute(what, s0->stream, g.items, 1, (int)g.nd, day_end - day_begin, S, s0->h_w.data(), ev, actual, used, vs_p, uni_out, multi_out);
}

// Every data set of one handle, on k_tl_scores' block, in one launch of every kernel.
int potus_forecast_scores_datasets(int handle, int day_begin, int day_end, const double *ev, int ev_to_win, const double *actual, const int32_t *use,
                                   double vs_p, double *uni_out, double *multi_out, int32_t *n_draws_out) {
  const char *what = "potus_forecast_scores_datasets";
  (void)ev_to_win;
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  if (!uni_out || !multi_out || !n_draws_out) return fail(POTUS_ERR_ARG, "%s: null output", what);
  std::vector<int> used;
  if (const int rc_ = fs_check(what, sp->M.S, ev, actual, use, vs_p, used)) return rc_;
  TlPlan pl;
  if (const int rc_ = tl_check_args(what, sp, day_begin, day_end, pl)) return rc_;
  DeviceGuard guard;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  if (const int rc_ = ds_plan(what, sp, pl)) return rc_;
  const int S = sp->M.S, nd = pl.nd, n = pl.cpd * pl.n_post, n_ds = pl.n_ds;
  DevBufs tmp;
  double *x = nullptr;
  int *dskip = nullptr;
  int rc;
  if ((rc = tmp.get(&x, (size_t)n_ds * n * nd * S * 8, what)) || (rc = tmp.get(&dskip, (size_t)n_ds * 4, what))) return rc;
  HIP_TRY(hipMemcpyAsync(dskip, pl.skip.data(), (size_t)n_ds * 4, hipMemcpyHostToDevice, sp->stream));
  if ((rc = tl_scores(sp, pl, day_begin, day_end, dskip, x))) return rc;   // NaN scores for a data set with a failed chain: every score of it is NaN
  if ((rc = fs_compute(what, sp->stream, x, n_ds, n, nd, S, sp->h_w.data(), ev, actual, used, vs_p, uni_out, multi_out))) return rc;
  for (int k = 0; k < n_ds; k++) n_draws_out[k] = pl.skip[k] ? 0 : n;
  return 0;
}

int potus_forecast_scores_timing(double *ms) {
  return timing_out("potus_forecast_scores_timing", g_fs_ms, 4, ms);
}

// ---------------------------------------------------------------------------------------------- exact cross-validation (potus_crossval.hpp)
namespace {
constexpr size_t CV_BLOCK_BUDGET = 256ull << 20;   // the ll block of one round of potus_cv_lpd (POTUS_CV_BLOCK_BUDGET, bytes: tests)
thread_local double g_cv_ms[2] = {0.0, 0.0};       // the calling thread's last potus_cv_lpd: k_cv_loglik, k_cv_reduce (HIP events, summed over the blocks)

struct CvPlan : DsPlan {
  int Np = 0;
  std::vector<int> off, held, pair_ds, pair_k;   // pairs by data set, then by poll number; held = the pair's poll in the model's order
  long long n_pairs() const { return (long long)held.size(); }
};
// every refusal that needs no device, and the held lists in the model's poll order (the qi mapping k_loo_loglik inverts)
int cv_check_args(const char *what, Sampler *sp, const int32_t *held_state, const int32_t *held_national, int integrate, CvPlan &pl) {
  const int Ns = sp->M.Ns, Nn = sp->M.Nn, Np = Ns + Nn, S = sp->M.S;
  if ((Ns && !held_state) || (Nn && !held_national)) return fail(POTUS_ERR_ARG, "%s: null mask", what);
  if (integrate != 0 && integrate != 1) return fail(POTUS_ERR_ARG, "%s: integrate = %d (0: the draw's noise coordinate, 1: integrated out)", what, integrate);
  if (sp->dense) return fail(POTUS_ERR_UNSUPPORTED, "%s: the dense metric is not supported (metric = POTUS_METRIC_DIAG only)", what);
  if (!sp->inited) return fail(POTUS_ERR_STATE, "%s: the handle is not initialised (potus_init, then potus_run)", what);
  pl.of(sp); pl.Np = Np;
  std::vector<int> model_of(Np, -1);
  for (int i = 0; i < Np; i++) {   // day-sorted poll i is state poll qidx - o_ns or national poll qidx - o_nn (build_model)
    const int qi = sp->h_pq[i];
    model_of[sp->h_ps[i] == S ? Ns + (qi - sp->M.o_nn) : qi - sp->M.o_ns] = i;
  }
  pl.off.assign(1, 0);
  for (int d = 0; d < pl.n_ds; d++) {
    for (int k = 0; k < Np; k++)
      if (k < Ns ? held_state[(size_t)d * Ns + k] : held_national[(size_t)d * Nn + (k - Ns)]) { pl.held.push_back(model_of[k]); pl.pair_ds.push_back(d); pl.pair_k.push_back(k); }
    pl.off.push_back((int)pl.held.size());
  }
  return 0;
}
struct CvDev { LooRows rows; int *off = nullptr, *held = nullptr, *pair_ds = nullptr, *skip = nullptr; };
int cv_upload(const char *what, Sampler *sp, const CvPlan &pl, DevBufs &keep, CvDev &d) {
  int rc;
  if ((rc = loo_rows_setup(sp, (long long)pl.n_post * sp->R.chains, keep, d.rows, what))) return rc;
  const size_t np = (size_t)pl.n_pairs();
  if ((rc = keep.get(&d.off, pl.off.size() * 4, what)) || (rc = keep.get(&d.held, np * 4, what)) || (rc = keep.get(&d.pair_ds, np * 4, what)) ||
      (rc = keep.get(&d.skip, (size_t)pl.n_ds * 4, what))) return rc;
  HIP_TRY(hipMemcpyAsync(d.off, pl.off.data(), pl.off.size() * 4, hipMemcpyHostToDevice, sp->stream));
  HIP_TRY(hipMemcpyAsync(d.held, pl.held.data(), np * 4, hipMemcpyHostToDevice, sp->stream));
  HIP_TRY(hipMemcpyAsync(d.pair_ds, pl.pair_ds.data(), np * 4, hipMemcpyHostToDevice, sp->stream));
  HIP_TRY(hipMemcpyAsync(d.skip, pl.skip.data(), (size_t)pl.n_ds * 4, hipMemcpyHostToDevice, sp->stream));
  return 0;
}
// ll of pairs [p0, p1) -> out [p1 - p0][draws per data set], on the handle's stream
int cv_loglik(Sampler *sp, const CvPlan &pl, const CvDev &d, int p0, int p1, int integrate, double *out) {
  CvParams P{row_src(sp, pl.first), sp->L.ncols, pl.n_post, pl.cpd, integrate,
             sp->M.pd, d.rows.lc, d.off, d.held, d.skip, p0, p1, d.rows.scratch, out};
  hipLaunchKernelGGL(k_cv_loglik, dim3(d.rows.grid), dim3(256), 0, sp->stream, pl.Mg, P);
  HIP_TRY(hipGetLastError());
  return 0;
}
} // namespace

int potus_cv_log_lik_device(int handle, const int32_t *held_state, const int32_t *held_national, int integrate, void *out_device, long long *n_pairs) {
  const char *what = "potus_cv_log_lik_device";
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  if (!out_device && !n_pairs) return fail(POTUS_ERR_ARG, "%s: null output", what);
  CvPlan pl;
  if (const int rc_ = cv_check_args(what, sp, held_state, held_national, integrate, pl)) return rc_;
  if (n_pairs) *n_pairs = pl.n_pairs();
  if (!out_device) return 0;
  if (pl.n_pairs() == 0) {   // nothing to write: only the state of the handle is left to check
    DeviceGuard guard;
    DeviceLocks lock(sp->device);
    HIP_TRY(hipSetDevice(sp->device));
    return ds_plan(what, sp, pl);
  }
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, sp->device, out_device, "output")) return rc_;
  if (const int rc_ = ds_plan(what, sp, pl)) return rc_;
  DevBufs keep;
  CvDev d;
  if (const int rc_ = cv_upload(what, sp, pl, keep, d)) return rc_;
  if (const int rc_ = cv_loglik(sp, pl, d, 0, (int)pl.n_pairs(), integrate, (double *)out_device)) return rc_;
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

int potus_cv_lpd(int handle, const int32_t *held_state, const int32_t *held_national, int integrate, double *lpd_out, int32_t *n_draws_out) {
  const char *what = "potus_cv_lpd";
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  if (!lpd_out || !n_draws_out) return fail(POTUS_ERR_ARG, "%s: null output", what);
  CvPlan pl;
  if (const int rc_ = cv_check_args(what, sp, held_state, held_national, integrate, pl)) return rc_;
  DeviceGuard guard;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  if (const int rc_ = ds_plan(what, sp, pl)) return rc_;
  const long long nd = (long long)pl.cpd * pl.n_post;
  const int np = (int)pl.n_pairs();
  for (size_t i = 0; i < (size_t)pl.n_ds * pl.Np * 2; i++) lpd_out[i] = std::numeric_limits<double>::quiet_NaN();
  for (int k = 0; k < pl.n_ds; k++) n_draws_out[k] = pl.skip[k] ? 0 : (int32_t)nd;
  g_cv_ms[0] = g_cv_ms[1] = 0.0;
  if (np == 0) return 0;
  size_t budget = CV_BLOCK_BUDGET;
  if (const char *e = getenv("POTUS_CV_BLOCK_BUDGET")) budget = std::max<size_t>(1, (size_t)atoll(e));
  const int nb = (int)std::max<size_t>(1, std::min<size_t>((size_t)np, budget / ((size_t)nd * 8)));   // pairs per block
  DevBufs keep;
  CvDev d;
  int rc;
  if ((rc = cv_upload(what, sp, pl, keep, d))) return rc;
  double *blk = nullptr, *dout = nullptr;
  if ((rc = keep.get(&blk, (size_t)nb * nd * 8, what)) || (rc = keep.get(&dout, (size_t)np * 2 * 8, what))) return rc;
  const int n_blocks = (np + nb - 1) / nb;
  std::vector<EventTimer> e0(n_blocks), e1(n_blocks);
  for (int b = 0; b < n_blocks; b++) {
    const int p0 = b * nb, p1 = std::min(p0 + nb, np);
    HIP_TRY(e0[b].made); HIP_TRY(e1[b].made);
    HIP_TRY(e0[b].start(sp->stream));
    if ((rc = cv_loglik(sp, pl, d, p0, p1, integrate, blk))) return rc;
    HIP_TRY(e0[b].stop(sp->stream));
    CvReduceParams Q{blk, d.pair_ds + p0, d.skip, p1 - p0, (int)nd, dout + (size_t)p0 * 2};
    HIP_TRY(e1[b].start(sp->stream));
    hipLaunchKernelGGL(k_cv_reduce, dim3((unsigned)std::min((p1 - p0 + 3) / 4, 65535)), dim3(256), 0, sp->stream, Q);
    HIP_TRY(hipGetLastError());
    HIP_TRY(e1[b].stop(sp->stream));
  }
  std::vector<double> h((size_t)np * 2);
  HIP_TRY(hipMemcpyAsync(h.data(), dout, h.size() * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  for (int b = 0; b < n_blocks; b++) {
    double ms0 = 0, ms1 = 0;
    if ((rc = e0[b].elapsed_or_fail(&ms0)) || (rc = e1[b].elapsed_or_fail(&ms1))) return rc;
    g_cv_ms[0] += ms0; g_cv_ms[1] += ms1;
  }
  for (int p = 0; p < np; p++) {
    double *o = lpd_out + ((size_t)pl.pair_ds[p] * pl.Np + pl.pair_k[p]) * 2;
    o[0] = h[(size_t)p * 2]; o[1] = h[(size_t)p * 2 + 1];
  }
  return 0;
}

int potus_cv_timing(double *ms) {
  return timing_out("potus_cv_timing", g_cv_ms, 2, ms);
}

// ---------------------------------------------------------------------------------------------- the posterior mode (potus_optimize.hpp)
namespace {
thread_local double g_opt_ms = 0.0;   // the calling thread's last potus_optimize: k_opt_lbfgs (HIP events)
}

void potus_default_optimize_opts(potus_optimize_opts *o) {
  if (!o) return;
  o->jacobian = 0; o->history_size = 5; o->iter = 2000; o->path_offset = 0;
  o->init_alpha = 1e-3; o->tol_obj = 1e-12; o->tol_rel_obj = 1e4; o->tol_grad = 1e-8; o->tol_rel_grad = 1e7; o->tol_param = 1e-8;
}

namespace {
// what every call that deals paths to a handle's data sets refuses first: the handle's layout, then the number of paths
int paths_check(const Sampler *sp, const char *what, int n_paths, const char *noun = "n_paths") {
  // a model beyond the one-workgroup kernels first: "cus_per_chain = 1" is no advice for it, that handle cannot be created
  if (!sp->k1_unsupported.empty()) return fail(POTUS_ERR_UNSUPPORTED, "%s: %s", what, sp->k1_unsupported.c_str());
  if (sp->K != 1) return fail(POTUS_ERR_UNSUPPORTED, "%s: needs one workgroup per chain (cus_per_chain = 1); this handle runs %d per chain", what, sp->K);
  if (sp->dense) return fail(POTUS_ERR_UNSUPPORTED, "%s: the dense metric is not supported (metric = POTUS_METRIC_DIAG only)", what);
  if (n_paths <= 0) return fail(POTUS_ERR_ARG, "%s: %s = %d, at least 1", what, noun, n_paths);
  if (sp->n_ds && n_paths % sp->n_ds) return fail(POTUS_ERR_ARG, "%s: %s = %d is not a multiple of the handle's %d data sets", what, noun, n_paths, sp->n_ds);
  return 0;
}
// what potus_optimize and potus_pathfinder refuse alike, before any kernel runs
int opt_check(const Sampler *sp, const char *what, const potus_optimize_opts &o, int n_paths, const char *null_outputs) {
  if (const int rc_ = paths_check(sp, what, n_paths)) return rc_;
  if (null_outputs) return fail(POTUS_ERR_ARG, "%s: null output (%s are required)", what, null_outputs);
  if (o.history_size < 1 || o.history_size > OPT_MAX_HISTORY) return fail(POTUS_ERR_ARG, "%s: history_size = %d outside 1..%d", what, o.history_size, OPT_MAX_HISTORY);
  if (o.iter < 1) return fail(POTUS_ERR_ARG, "%s: iter = %d, at least 1", what, o.iter);
  const double tols[5] = {o.tol_obj, o.tol_rel_obj, o.tol_grad, o.tol_rel_grad, o.tol_param};
  static const char *const tol_names[5] = {"tol_obj", "tol_rel_obj", "tol_grad", "tol_rel_grad", "tol_param"};
  for (int k = 0; k < 5; k++) if (!(tols[k] >= 0.0)) return fail(POTUS_ERR_ARG, "%s: %s = %g, must be >= 0 (0 switches the rule off)", what, tol_names[k], tols[k]);
  if (!(o.init_alpha > 0.0) || !std::isfinite(o.init_alpha)) return fail(POTUS_ERR_ARG, "%s: init_alpha = %g, must be positive and finite", what, o.init_alpha);
  if (o.jacobian != 0 && o.jacobian != 1) return fail(POTUS_ERR_ARG, "%s: jacobian = %d, 0 or 1", what, o.jacobian);
  if (o.path_offset < 0 || (long long)o.path_offset + n_paths >= 0xFFFFFFFFll) return fail(POTUS_ERR_ARG, "%s: path_offset = %d with %d paths", what, o.path_offset, n_paths);
  const int D = sp->L.D, Dpad = (D + 7) & ~7, nvec = 2 * o.history_size + 5;
  if ((unsigned long long)nvec * Dpad * 8ull >= 0x7fffffffull) return fail(POTUS_ERR_UNSUPPORTED, "%s: D = %d with history_size = %d: a path's working set must stay below 2 GB", what, D, o.history_size);
  return 0;
}

// One k_opt_lbfgs launch on the handle's stream, under the caller's device lock: the working set comes from `tmp`, the event pair is around the
// kernel.  traj_x, traj_g [n_paths][traj_rows][Dpad] (or null): the accepted points and gradients of every path (potus_pathfinder).
struct OptRun { double *rows = nullptr, *dlp = nullptr, *dgn = nullptr; int *dinfo = nullptr; int per_ds = 1; const DevModel *Mg = nullptr; };
int opt_launch(Sampler *sp, const char *what, const potus_optimize_opts &o, const double *q0, int n_paths, DevBufs &tmp,
               double *traj_x, double *traj_g, int traj_rows, EventTimer &ev, OptRun &r) {
  const int D = sp->L.D, row = POTUS_N_SAMPLER_COLS + D, Dpad = (D + 7) & ~7, nvec = 2 * o.history_size + 5;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_opt_lbfgs), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp->lds_bytes));
  double *dq0 = nullptr, *work = nullptr;
  int rc;
  if ((rc = tmp.get(&work, (size_t)n_paths * nvec * Dpad * 8, what)) || (rc = tmp.get(&r.rows, (size_t)n_paths * row * 8, what)) ||
      (rc = tmp.get(&r.dlp, (size_t)n_paths * 8, what)) || (rc = tmp.get(&r.dgn, (size_t)n_paths * 8, what)) || (rc = tmp.get(&r.dinfo, (size_t)n_paths * 3 * 4, what))) return rc;
  if (q0) {
    if ((rc = tmp.get(&dq0, (size_t)n_paths * D * 8, what))) return rc;
    HIP_TRY(hipMemcpyAsync(dq0, q0, (size_t)n_paths * D * 8, hipMemcpyHostToDevice, sp->stream));
  }
  HIP_TRY(ev.made);
  DsPlan pl;   // the models of the handle's data sets; the paths are dealt to them as chains are
  pl.of(sp);
  r.per_ds = n_paths / pl.n_ds;
  r.Mg = pl.Mg;
  OptParams P{dq0, work, r.rows, r.dlp, r.dgn, r.dinfo, r.per_ds, o.history_size, o.iter, o.jacobian, o.path_offset, Dpad,
              o.init_alpha, o.tol_obj, o.tol_rel_obj, o.tol_grad, o.tol_rel_grad, o.tol_param, sp->R.init_radius, sp->R.seed_lo, sp->R.seed_hi,
              traj_x, traj_g, traj_rows};
  OptParams *dP = nullptr;
  if ((rc = tmp.get(&dP, sizeof(OptParams), what))) return rc;
  HIP_TRY(hipMemcpyAsync(dP, &P, sizeof(OptParams), hipMemcpyHostToDevice, sp->stream));
  HIP_TRY(ev.start(sp->stream));
  hipLaunchKernelGGL(k_opt_lbfgs, dim3(n_paths), dim3(PT_THREADS), sp->lds_bytes, sp->stream, r.Mg, (const OptParams *)dP);
  HIP_TRY(hipGetLastError());
  HIP_TRY(ev.stop(sp->stream));
  return 0;
}
} // namespace

int potus_optimize(int handle, const potus_optimize_opts *opts, const double *q0, int n_paths, double *q_out, double *lp_out, double *gnorm_out,
                   int32_t *info_out, int col_begin, int col_end, double *row_out) {
  const char *what = "potus_optimize";
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  potus_optimize_opts o;
  potus_default_optimize_opts(&o);
  if (opts) o = *opts;
  if (const int rc_ = opt_check(sp, what, o, n_paths, q_out && lp_out && info_out ? nullptr : "q_out, lp_out and info_out")) return rc_;
  if (row_out) if (const int rc_ = check_cols(sp, col_begin, col_end)) return rc_;
  const int D = sp->L.D, row = POTUS_N_SAMPLER_COLS + D;
  DeviceGuard guard;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  DevBufs tmp;   // the working set is the call's own: the sampler's chain state is not touched
  EventTimer ev;
  OptRun r;
  int rc;
  if ((rc = opt_launch(sp, what, o, q0, n_paths, tmp, nullptr, nullptr, 0, ev, r))) return rc;
  double *rows = r.rows;
  std::vector<double> hrows((size_t)n_paths * row);
  HIP_TRY(hipMemcpyAsync(hrows.data(), rows, hrows.size() * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipMemcpyAsync(lp_out, r.dlp, (size_t)n_paths * 8, hipMemcpyDeviceToHost, sp->stream));
  if (gnorm_out) HIP_TRY(hipMemcpyAsync(gnorm_out, r.dgn, (size_t)n_paths * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipMemcpyAsync(info_out, r.dinfo, (size_t)n_paths * 3 * 4, hipMemcpyDeviceToHost, sp->stream));
  if (row_out) {   // the CmdStan row of every path's point, built with the path's own model
    const int nsel = col_end - col_begin;
    WAParams W{RowSrc{rows, n_paths, 1, row, 0}, 1, sp->L.ncols, col_begin, col_end, nullptr, nullptr, nsel};   // one saved draw of n_paths chains
    if ((rc = launch_rows(sp, tmp, what, r.Mg, sp->n_ds ? r.per_ds : 0, W))) return rc;
    HIP_TRY(hipMemcpyAsync(row_out, W.out, (size_t)n_paths * nsel * 8, hipMemcpyDeviceToHost, sp->stream));
  }
  HIP_TRY(hipStreamSynchronize(sp->stream));
  if ((rc = ev.elapsed_or_fail(&g_opt_ms))) return rc;
  for (int i = 0; i < n_paths; i++) std::copy(hrows.begin() + (size_t)i * row + POTUS_N_SAMPLER_COLS, hrows.begin() + (size_t)(i + 1) * row, q_out + (size_t)i * D);
  return 0;
}

int potus_optimize_timing(double *ms) {
  return timing_out("potus_optimize_timing", &g_opt_ms, 1, ms);
}

// ---------------------------------------------------------------------------------------------- the Laplace approximation (potus_laplace.hpp)
namespace {
constexpr size_t LAP_MATRIX_BUDGET = 16ull << 30;   // D x LD matrices in flight (POTUS_LAPLACE_MATRIX_BUDGET, bytes: tests)
thread_local double g_lap_ms[4] = {0.0, 0.0, 0.0, 0.0};   // the calling thread's last potus_laplace: Hessian, factor, solve, lp__ (HIP events, summed)

// the timed spans of one stage of a call: as many event pairs as the stage has spans, summed once the stream is synchronised
struct LapSpans {
  std::vector<std::unique_ptr<EventTimer>> v;
  int begin(hipStream_t st) {
    v.emplace_back(new EventTimer());
    HIP_TRY(v.back()->made);
    HIP_TRY(v.back()->start(st));
    return 0;
  }
  int end(hipStream_t st) { HIP_TRY(v.back()->stop(st)); return 0; }
  int sum(double *ms) {
    *ms = 0.0;
    for (auto &e : v) { double x = 0; if (const int rc = e->elapsed_or_fail(&x)) return rc; *ms += x; }
    return 0;
  }
};

// The rows [lp__, six NaN, x] a handle keeps of its last potus_laplace (groups = modes) or potus_pathfinder[_path] (groups = paths): what the
// three accessors of either read.  ONE body per accessor takes this view.
struct KeptRows {
  const char *missing;           // what to say when there are none
  const char *group;             // "mode" or "path"
  double *rows; int groups, draws; const std::vector<int> *code;
  int n() const { return groups * draws; }
  int per_ds(const Sampler *sp) const { return groups / std::max(sp->n_ds, 1) * draws; }   // rows per data set, group-major
};
enum { KEPT_LAPLACE = 0, KEPT_PATHFINDER = 1, KEPT_ADVI = 2 };
KeptRows kept_rows(const Sampler *sp, int which) {
  if (which == KEPT_ADVI) return KeptRows{"no ADVI draws on this handle (potus_advi with output_samples >= 1 first)", "run", sp->vi_rows, sp->vi_runs, sp->vi_draws, &sp->vi_code};
  if (which == KEPT_PATHFINDER) return KeptRows{"no Pathfinder draws on this handle (potus_pathfinder or potus_pathfinder_path with num_draws >= 1 first)", "path", sp->pf_rows, sp->pf_paths, sp->pf_draws, &sp->pf_code};
  return KeptRows{"no Laplace draws on this handle (potus_laplace with n_draws >= 1 first)", "mode", sp->lap_rows, sp->lap_modes, sp->lap_draws, &sp->lap_code};
}
// what the three accessors check first: a successful call with draws on this handle
int kept_have_rows(const char *what, const KeptRows &kr) {
  if (!kr.rows || kr.draws < 1) return fail(POTUS_ERR_STATE, "%s: %s", what, kr.missing);
  return 0;
}
} // namespace

void potus_default_laplace_opts(potus_laplace_opts *o) {
  if (!o) return;
  o->jacobian = 1; o->draw_offset = 0; o->pad0 = 0; o->pad1 = 0; o->h = 1e-4;
}

int potus_laplace(int handle, const potus_laplace_opts *opts, const double *mode, int n_modes, const double *u, int n_draws,
                  double *q_out, double *lp_out, double *lp_approx_out, double *info_out, double *precision_out) {
  const char *what = "potus_laplace";
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  potus_laplace_opts o;
  potus_default_laplace_opts(&o);
  if (opts) o = *opts;
  if (sp->K != 1) return fail(POTUS_ERR_UNSUPPORTED, "%s: needs one workgroup per chain (cus_per_chain = 1); this handle runs %d per chain", what, sp->K);
  if (sp->dense) return fail(POTUS_ERR_UNSUPPORTED, "%s: the dense metric is not supported (metric = POTUS_METRIC_DIAG only)", what);
  if (!sp->k1_unsupported.empty()) return fail(POTUS_ERR_UNSUPPORTED, "%s: %s", what, sp->k1_unsupported.c_str());
  if (n_modes <= 0) return fail(POTUS_ERR_ARG, "%s: n_modes = %d, at least 1", what, n_modes);
  if (sp->n_ds && n_modes % sp->n_ds) return fail(POTUS_ERR_ARG, "%s: n_modes = %d is not a multiple of the handle's %d data sets", what, n_modes, sp->n_ds);
  if (n_draws < 0) return fail(POTUS_ERR_ARG, "%s: n_draws = %d", what, n_draws);
  if (!(o.h > 0.0) || !std::isfinite(o.h)) return fail(POTUS_ERR_ARG, "%s: h = %g, must be positive and finite", what, o.h);
  if (o.jacobian != 0 && o.jacobian != 1) return fail(POTUS_ERR_ARG, "%s: jacobian = %d, 0 or 1", what, o.jacobian);
  if (o.draw_offset < 0 || (long long)o.draw_offset + n_draws >= 0xFFFFFFFFll) return fail(POTUS_ERR_ARG, "%s: draw_offset = %d with %d draws", what, o.draw_offset, n_draws);
  if (!mode || !info_out) return fail(POTUS_ERR_ARG, "%s: null argument (mode and info_out are required)", what);
  const int D = sp->L.D, row = POTUS_N_SAMPLER_COLS + D, Dpad = (D + 7) & ~7, LD = Dpad;
  const size_t mat = (size_t)D * LD, rows_total = (size_t)n_modes * n_draws;
  if (3ull * Dpad * 8ull >= 0x7fffffffull) return fail(POTUS_ERR_UNSUPPORTED, "%s: D = %d: a workgroup's working set must stay below 2 GB", what, D);
  if (rows_total * row >= (1ull << 40)) return fail(POTUS_ERR_ARG, "%s: %d modes x %d draws of %d coordinates", what, n_modes, n_draws, D);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  // the modes that are finite go through the kernels, in blocks of as many matrices as the budget holds
  std::vector<int> live, code(n_modes, LAP_OK);
  for (int m = 0; m < n_modes; m++) {
    bool fin = true;
    for (int i = 0; i < D && fin; i++) fin = std::isfinite(mode[(size_t)m * D + i]);
    if (fin) live.push_back(m); else code[m] = LAP_NOT_FINITE;
  }
  size_t budget = LAP_MATRIX_BUDGET;
  if (const char *e = getenv("POTUS_LAPLACE_MATRIX_BUDGET")) budget = std::max<size_t>(1, (size_t)atoll(e));
  const int nlive = (int)live.size(), nmat = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(nlive, 1), budget / (mat * 8)));
  int G = std::max(1, std::min(D, 512 / std::min(nmat, 512)));   // workgroups per mode: the chip's 256 compute units twice over
  if (const char *e = getenv("POTUS_LAPLACE_G")) G = std::max(1, std::min(D, atoi(e)));   // tests: the rows do not depend on it

  DeviceGuard guard;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lap_hess), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp->lds_bytes));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lap_lp), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp->lds_bytes));
  hipStream_t st = sp->stream;
  DsPlan pl;
  pl.of(sp);
  const int per_ds = n_modes / pl.n_ds;
  // the handle's rows of the last call go first: a call that fails leaves none behind
  HIP_TRY(hipStreamSynchronize(st));
  if (sp->lap_rows) { (void)hipFree(sp->lap_rows); sp->lap_rows = nullptr; }
  sp->lap_modes = sp->lap_draws = 0; sp->lap_code.clear();
  DevBufs tmp;
  int rc;
  double *rows = nullptr;
  if (n_draws > 0) {
    void *p = nullptr;
    if (hipMalloc(&p, rows_total * row * 8) != hipSuccess) { (void)hipGetLastError(); return fail(POTUS_ERR_DEVICE, "%s: hipMalloc of %zu bytes for the rows failed", what, rows_total * row * 8); }
    rows = static_cast<double *>(p);
  }
  struct RowsOwner { double *p; ~RowsOwner() { if (p) (void)hipFree(p); } } owner{rows};   // until the call has succeeded
  double *H = nullptr, *work = nullptr, *dmode = nullptr, *dgn = nullptr, *dinfo = nullptr, *U = nullptr, *dlp = nullptr, *dla = nullptr, *gscr = nullptr;
  int *dds = nullptr, *dfail = nullptr;
  LapHessParams *dP = nullptr;
  const int lp_grid = std::max(1, std::min(n_draws, 1024));
  if ((rc = tmp.get(&H, (size_t)nmat * mat * 8, what)) || (rc = tmp.get(&work, (size_t)nmat * G * 3 * Dpad * 8, what)) ||
      (rc = tmp.get(&dmode, (size_t)n_modes * D * 8, what)) || (rc = tmp.get(&dgn, (size_t)n_modes * 8, what)) ||
      (rc = tmp.get(&dinfo, (size_t)nmat * 4 * 8, what)) || (rc = tmp.get(&dds, (size_t)n_modes * 4, what)) ||
      (rc = tmp.get(&dfail, (size_t)n_modes * 4, what)) || (rc = tmp.get(&dP, sizeof(LapHessParams), what))) return rc;
  if (n_draws > 0 && ((rc = tmp.get(&U, (size_t)n_draws * LD * 8, what)) || (rc = tmp.get(&dlp, rows_total * 8, what)) ||
                      (rc = tmp.get(&dla, rows_total * 8, what)) || (rc = tmp.get(&gscr, (size_t)lp_grid * Dpad * 8, what)))) return rc;
  // (live modes compacted: entry k of dmode / dds / dgn / dfail is mode live[k])
  std::vector<double> hmode((size_t)std::max(nlive, 1) * D);
  std::vector<int> hds(std::max(nlive, 1), 0);
  for (int k = 0; k < nlive; k++) {
    std::copy(mode + (size_t)live[k] * D, mode + (size_t)(live[k] + 1) * D, hmode.begin() + (size_t)k * D);
    hds[k] = live[k] / per_ds;
  }
  HIP_TRY(hipMemcpyAsync(dmode, hmode.data(), (size_t)std::max(nlive, 1) * D * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(dds, hds.data(), (size_t)std::max(nlive, 1) * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(dfail, 0, (size_t)n_modes * 4, st));
  std::vector<double> hinfo((size_t)std::max(nlive, 1) * 4, nan), hgn(std::max(nlive, 1), nan);
  std::vector<int> hfail(std::max(nlive, 1), 0);
  LapSpans t_hess, t_fac, t_solve, t_lp;
  const int nbk = (D + DN_NB - 1) / DN_NB;
  for (int k0 = 0; k0 < nlive; k0 += nmat) {
    const int nk = std::min(nmat, nlive - k0);
    LapHessParams P{dmode + (size_t)k0 * D, dds + k0, work, H, dgn + k0, G, Dpad, LD, o.jacobian, o.h};
    HIP_TRY(hipMemcpyAsync(dP, &P, sizeof(P), hipMemcpyHostToDevice, st));   // (pageable source: copied before the call returns)
    if ((rc = t_hess.begin(st))) return rc;
    hipLaunchKernelGGL(k_lap_hess, dim3(G, nk), dim3(PT_THREADS), sp->lds_bytes, st, pl.Mg, (const LapHessParams *)dP);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_lap_sym, dim3(nbk, nbk, nk), dim3(256), 0, st, H, D, LD);
    HIP_TRY(hipGetLastError());
    if ((rc = t_hess.end(st))) return rc;
    if (precision_out)
      for (int k = 0; k < nk; k++)
        HIP_TRY(hipMemcpy2DAsync(precision_out + (size_t)live[k0 + k] * D * D, (size_t)D * 8, H + (size_t)k * mat, (size_t)LD * 8, (size_t)D * 8, D, hipMemcpyDeviceToHost, st));
    if ((rc = t_fac.begin(st))) return rc;
    for (int k = 0; k < nk; k++) {   // one matrix per launch set: its own fail word
      DnParams F{};
      F.chains = 1; F.D = D; F.LD = LD; F.A = H + (size_t)k * mat; F.fail = dfail + k0 + k;
      dense_cholesky_launch(st, F, 1);
      HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_lap_diag, dim3(nk), dim3(256), 0, st, (const double *)H, D, LD, dinfo);
    HIP_TRY(hipGetLastError());
    if ((rc = t_fac.end(st))) return rc;
    HIP_TRY(hipMemcpyAsync(hinfo.data() + (size_t)k0 * 4, dinfo, (size_t)nk * 4 * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hfail.data() + k0, dfail + k0, (size_t)nk * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // who has a factor decides what the draws of the block become
    for (int k = 0; k < nk && n_draws > 0; k++) {
      const int m = live[k0 + k], ok = hfail[k0 + k] == 0;
      const double *Lk = H + (size_t)k * mat;
      double *mrows = rows + (size_t)m * n_draws * row, *mlp = dlp + (size_t)m * n_draws, *mla = dla + (size_t)m * n_draws;
      const int dgrid = std::min(n_draws, 4096), nt = (n_draws + DN_NB - 1) / DN_NB;
      if ((rc = t_solve.begin(st))) return rc;
      if (ok) {
        if (u) HIP_TRY(hipMemcpy2DAsync(U, (size_t)LD * 8, u + (size_t)m * n_draws * D, (size_t)D * 8, (size_t)D * 8, n_draws, hipMemcpyHostToDevice, st));
        else {
          hipLaunchKernelGGL(k_lap_normals, dim3((unsigned)std::min<long long>(((long long)n_draws * ((D + 1) / 2) + 255) / 256, 65535)), dim3(256), 0, st,
                             U, n_draws, D, LD, o.draw_offset, sp->R.seed_lo, sp->R.seed_hi);
          HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_lap_norm, dim3(dgrid), dim3(256), 0, st, (const double *)U, n_draws, D, LD, mla);
        HIP_TRY(hipGetLastError());
        for (int pe = nbk; pe > 0;) {                       // the panel of blocks [pb, pe), last panel first
          const int pb = std::max(0, pe - LAP_PANEL);
          for (int b = pe - 1; b >= pb; b--) {
            hipLaunchKernelGGL(k_lap_solve_diag, dim3(nt), dim3(256), 0, st, Lk, U, D, LD, n_draws, b);
            if (b > pb) hipLaunchKernelGGL(k_lap_solve_update, dim3(b - pb, nt), dim3(256), 0, st, Lk, U, D, LD, n_draws, b, b + 1, pb);
          }
          if (pb > 0) hipLaunchKernelGGL(k_lap_solve_update, dim3(pb, nt), dim3(256), 0, st, Lk, U, D, LD, n_draws, pb, pe, 0);
          pe = pb;
        }
        HIP_TRY(hipGetLastError());
      }
      hipLaunchKernelGGL(k_lap_rows, dim3(dgrid), dim3(256), 0, st, (const double *)U, (const double *)(dmode + (size_t)(k0 + k) * D), n_draws, D, LD, ok, mrows, mlp, mla);
      HIP_TRY(hipGetLastError());
      if ((rc = t_solve.end(st))) return rc;
      if (ok) {
        if ((rc = t_lp.begin(st))) return rc;
        hipLaunchKernelGGL(k_lap_lp, dim3(lp_grid), dim3(PT_THREADS), sp->lds_bytes, st, pl.Mg + hds[k0 + k], mrows, n_draws, gscr, Dpad, mlp);
        HIP_TRY(hipGetLastError());
        if ((rc = t_lp.end(st))) return rc;
      }
    }
  }
  if (nlive) HIP_TRY(hipMemcpyAsync(hgn.data(), dgn, (size_t)nlive * 8, hipMemcpyDeviceToHost, st));
  if (n_draws > 0) {
    for (int m = 0; m < n_modes; m++) if (code[m] == LAP_NOT_FINITE) {   // no kernel has written these rows
      hipLaunchKernelGGL(k_lap_rows, dim3(std::min(n_draws, 4096)), dim3(256), 0, st, (const double *)U, (const double *)dmode, n_draws, D, LD, 0,
                         rows + (size_t)m * n_draws * row, dlp + (size_t)m * n_draws, dla + (size_t)m * n_draws);
      HIP_TRY(hipGetLastError());
    }
    if (q_out) HIP_TRY(hipMemcpy2DAsync(q_out, (size_t)D * 8, rows + POTUS_N_SAMPLER_COLS, (size_t)row * 8, (size_t)D * 8, rows_total, hipMemcpyDeviceToHost, st));
    if (lp_out) HIP_TRY(hipMemcpyAsync(lp_out, dlp, rows_total * 8, hipMemcpyDeviceToHost, st));
    if (lp_approx_out) HIP_TRY(hipMemcpyAsync(lp_approx_out, dla, rows_total * 8, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  double ms[4];
  if ((rc = t_hess.sum(&ms[0])) || (rc = t_fac.sum(&ms[1])) || (rc = t_solve.sum(&ms[2])) || (rc = t_lp.sum(&ms[3]))) return rc;
  std::copy(ms, ms + 4, g_lap_ms);
  for (int m = 0; m < n_modes; m++) for (int i = 0; i < 4; i++) info_out[(size_t)m * 4 + i] = i == 0 ? (double)LAP_NOT_FINITE : nan;
  for (int k = 0; k < nlive; k++) {
    const int m = live[k];
    code[m] = hfail[k] ? LAP_NOT_PD : LAP_OK;
    double *io = info_out + (size_t)m * 4;
    io[0] = code[m]; io[1] = hfail[k] ? nan : hinfo[(size_t)k * 4 + 1]; io[2] = hgn[k]; io[3] = hfail[k] ? nan : hinfo[(size_t)k * 4 + 3];
  }
  if (precision_out)
    for (int m = 0; m < n_modes; m++) if (code[m] == LAP_NOT_FINITE) std::fill(precision_out + (size_t)m * D * D, precision_out + (size_t)(m + 1) * D * D, nan);
  if (n_draws > 0) { sp->lap_rows = rows; owner.p = nullptr; sp->lap_modes = n_modes; sp->lap_draws = n_draws; sp->lap_code = code; }
  return 0;
}

namespace {
int kept_write_array_device(const char *what, int which, int handle, int col_begin, int col_end, void *out_device) {
  Sampler *sp = get(handle);
  if (!sp || !out_device) return fail(POTUS_ERR_STATE, "bad handle or null output");
  const KeptRows kr = kept_rows(sp, which);
  if (const int rc_ = kept_have_rows(what, kr)) return rc_;
  if (const int rc_ = check_cols(sp, col_begin, col_end)) return rc_;
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, sp->device, out_device, "output")) return rc_;
  DevBufs tmp;
  const int n = kr.n(), nsel = col_end - col_begin;
  DsPlan pl;
  pl.of(sp);
  WAParams W{RowSrc{kr.rows, n, 1, POTUS_N_SAMPLER_COLS + sp->L.D, 0}, 1, sp->L.ncols, col_begin, col_end, nullptr, (double *)out_device, nsel};   // one saved draw of n chains
  if (const int rc_ = launch_rows(sp, tmp, what, pl.Mg, sp->n_ds ? kr.per_ds(sp) : 0, W)) return rc_;
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

int lap_scores(Sampler *sp, const KeptRows &kr, int day_begin, int day_end, const int *dskip, double *out) {
  const int n = kr.n();
  DsPlan pl;
  pl.of(sp);
  TlScoreParams P{RowSrc{kr.rows, n, 1, POTUS_N_SAMPLER_COLS + sp->L.D, 0}, 1, kr.per_ds(sp), day_begin, day_end, dskip, out};
  hipLaunchKernelGGL(k_tl_scores, dim3((unsigned)std::min<long long>(((long long)n + 3) / 4, 65535)), dim3(256), 0, sp->stream, pl.Mg, P);
  HIP_TRY(hipGetLastError());
  return 0;
}
int lap_check_days(const char *what, const Sampler *sp, int day_begin, int day_end) {
  if (day_begin < 0 || day_end > sp->M.T || day_begin >= day_end) return fail(POTUS_ERR_ARG, "%s: bad day range [%d,%d) of %d days", what, day_begin, day_end, sp->M.T);
  return 0;
}

int kept_scores_device(const char *what, int which, int handle, int day_begin, int day_end, void *out_device) {
  Sampler *sp = get(handle);
  if (!sp || !out_device) return fail(POTUS_ERR_STATE, "bad handle or null output");
  const KeptRows kr = kept_rows(sp, which);
  if (const int rc_ = kept_have_rows(what, kr)) return rc_;
  if (const int rc_ = lap_check_days(what, sp, day_begin, day_end)) return rc_;
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, sp->device, out_device, "output")) return rc_;
  DevBufs tmp;
  int *dskip = nullptr;
  const int n_ds = std::max(sp->n_ds, 1);
  if (const int rc_ = tmp.get(&dskip, (size_t)n_ds * 4, what)) return rc_;
  HIP_TRY(hipMemsetAsync(dskip, 0, (size_t)n_ds * 4, sp->stream));   // (a mode without a factor has NaN rows: its scores are NaN without a flag)
  if (const int rc_ = lap_scores(sp, kr, day_begin, day_end, dskip, (double *)out_device)) return rc_;
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

int kept_summary(const char *what, int which, int handle, int day_begin, int day_end, const double *ev, int ev_to_win, double *state_out, double *natl_out, double *ev_out, int32_t *n_draws_out) {
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  if (!ev || !state_out || !natl_out || !ev_out || !n_draws_out) return fail(POTUS_ERR_ARG, "%s: null argument", what);
  const KeptRows kr = kept_rows(sp, which);
  if (const int rc_ = kept_have_rows(what, kr)) return rc_;
  if (const int rc_ = lap_check_days(what, sp, day_begin, day_end)) return rc_;
  if (kr.draws > TL_MAX_DRAWS) return fail(POTUS_ERR_UNSUPPORTED, "%s: %d draws per %s: a %s's draws are sorted in LDS, at most %d", what, kr.draws, kr.group, kr.group, TL_MAX_DRAWS);
  DeviceGuard guard;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  const int S = sp->M.S, nd = day_end - day_begin, n = kr.draws, nm = kr.groups, n_ds = std::max(sp->n_ds, 1);
  DevBufs tmp;
  double *x = nullptr, *dw = nullptr, *dev_ = nullptr, *dout = nullptr;
  int *dskip = nullptr, *dzero = nullptr;
  int rc;
  const size_t n_out = (size_t)nm * nd * ((size_t)S * 4 + 9);
  if ((rc = tmp.get(&x, (size_t)nm * n * nd * S * 8, what)) || (rc = tmp.get(&dw, (size_t)S * 8, what)) || (rc = tmp.get(&dev_, (size_t)S * 8, what)) ||
      (rc = tmp.get(&dout, n_out * 8, what)) || (rc = tmp.get(&dskip, (size_t)nm * 4, what)) || (rc = tmp.get(&dzero, (size_t)n_ds * 4, what))) return rc;
  HIP_TRY(hipMemcpyAsync(dskip, kr.code->data(), (size_t)nm * 4, hipMemcpyHostToDevice, sp->stream));   // per mode: a code that is not 0 gives NaN
  HIP_TRY(hipMemsetAsync(dzero, 0, (size_t)n_ds * 4, sp->stream));
  HIP_TRY(hipMemcpyAsync(dw, sp->h_w.data(), (size_t)S * 8, hipMemcpyHostToDevice, sp->stream));
  HIP_TRY(hipMemcpyAsync(dev_, ev, (size_t)S * 8, hipMemcpyHostToDevice, sp->stream));
  if ((rc = lap_scores(sp, kr, day_begin, day_end, dzero, x))) return rc;
  int npad = 1;
  while (npad < n) npad <<= 1;
  const size_t lds = (size_t)npad * 8;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_tl_summary), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  double *o_state = dout, *o_natl = o_state + (size_t)nm * nd * S * 4, *o_ev = o_natl + (size_t)nm * nd * 4;
  TlSumParams Q{x, nm, n, nd, S, dw, dev_, (double)ev_to_win, dskip, o_state, o_natl, o_ev};
  hipLaunchKernelGGL(k_tl_summary, dim3((unsigned)std::min<long long>((long long)nm * nd * (S + 2), 65535)), dim3(TL_THREADS), lds, sp->stream, Q);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(state_out, o_state, (size_t)nm * nd * S * 4 * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipMemcpyAsync(natl_out, o_natl, (size_t)nm * nd * 4 * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipMemcpyAsync(ev_out, o_ev, (size_t)nm * nd * 5 * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  for (int m = 0; m < nm; m++) n_draws_out[m] = (*kr.code)[m] ? 0 : n;
  return 0;
}
} // namespace

int potus_laplace_write_array_device(int handle, int col_begin, int col_end, void *out_device) {
  return kept_write_array_device("potus_laplace_write_array_device", KEPT_LAPLACE, handle, col_begin, col_end, out_device);
}
int potus_laplace_scores_device(int handle, int day_begin, int day_end, void *out_device) {
  return kept_scores_device("potus_laplace_scores_device", KEPT_LAPLACE, handle, day_begin, day_end, out_device);
}
int potus_laplace_summary(int handle, int day_begin, int day_end, const double *ev, int ev_to_win, double *state_out, double *natl_out, double *ev_out, int32_t *n_draws_out) {
  return kept_summary("potus_laplace_summary", KEPT_LAPLACE, handle, day_begin, day_end, ev, ev_to_win, state_out, natl_out, ev_out, n_draws_out);
}
int potus_pathfinder_write_array_device(int handle, int col_begin, int col_end, void *out_device) {
  return kept_write_array_device("potus_pathfinder_write_array_device", KEPT_PATHFINDER, handle, col_begin, col_end, out_device);
}
int potus_pathfinder_scores_device(int handle, int day_begin, int day_end, void *out_device) {
  return kept_scores_device("potus_pathfinder_scores_device", KEPT_PATHFINDER, handle, day_begin, day_end, out_device);
}
int potus_pathfinder_summary(int handle, int day_begin, int day_end, const double *ev, int ev_to_win, double *state_out, double *natl_out, double *ev_out, int32_t *n_draws_out) {
  return kept_summary("potus_pathfinder_summary", KEPT_PATHFINDER, handle, day_begin, day_end, ev, ev_to_win, state_out, natl_out, ev_out, n_draws_out);
}

int potus_laplace_timing(double *ms) {
  return timing_out("potus_laplace_timing", g_lap_ms, 4, ms);
}

// ---------------------------------------------------------------------------------------------- Pathfinder (potus_pathfinder.hpp)
namespace {
thread_local double g_pf_ms[4] = {0.0, 0.0, 0.0, 0.0};   // the calling thread's last potus_pathfinder[_path]: L-BFGS, alpha, ELBO, draws (HIP events)

struct PfOut {
  int32_t *info; double *elbo; int32_t *kept; double *q, *lp, *lq, *mu, *alpha, *logdet, *phi, *lqw, *qtq;
};

int pf_check(const Sampler *sp, const char *what, const potus_pathfinder_opts &o, int n_paths) {
  if (const int rc_ = paths_check(sp, what, n_paths)) return rc_;
  if (o.history_size < 1 || o.history_size > PF_MAX_J) return fail(POTUS_ERR_ARG, "%s: history_size = %d outside 1..%d", what, o.history_size, PF_MAX_J);
  if (o.num_elbo_draws < 1 || o.num_elbo_draws > PF_MAX_K) return fail(POTUS_ERR_ARG, "%s: num_elbo_draws = %d outside 1..%d", what, o.num_elbo_draws, PF_MAX_K);
  if (o.num_draws < 0) return fail(POTUS_ERR_ARG, "%s: num_draws = %d", what, o.num_draws);
  if (o.draw_offset < 0 || (long long)o.draw_offset + o.num_draws >= 0xFFFFFFFFll) return fail(POTUS_ERR_ARG, "%s: draw_offset = %d with %d draws", what, o.draw_offset, o.num_draws);
  if (o.path_offset < 0 || (long long)o.path_offset + n_paths >= 0xFFFFFFFFll) return fail(POTUS_ERR_ARG, "%s: path_offset = %d with %d paths", what, o.path_offset, n_paths);
  const int D = sp->L.D, Dpad = (D + 7) & ~7;
  if ((unsigned long long)(2 * o.history_size + 4) * Dpad * 8ull >= 0x7fffffffull) return fail(POTUS_ERR_UNSUPPORTED, "%s: D = %d: a workgroup's working set must stay below 2 GB", what, D);
  if ((unsigned long long)n_paths * std::max(o.num_draws, 1) * (POTUS_N_SAMPLER_COLS + D) >= (1ull << 40)) return fail(POTUS_ERR_ARG, "%s: %d paths x %d draws of %d coordinates", what, n_paths, o.num_draws, D);
  return 0;
}

// From a trajectory on the device (dX, dG [n_paths][rows][Dpad], hL its lengths) to the outputs, under the caller's device lock.
int pf_core(Sampler *sp, const char *what, const potus_pathfinder_opts &o, DevBufs &tmp, const double *dX, const double *dG, const std::vector<int> &hL, int rows,
            int n_paths, const double *u_elbo, const double *u_draws, const int32_t *want_l, const int *opt_code, const PfOut &out, double *ms /*[3]*/) {
  const int D = sp->L.D, row = POTUS_N_SAMPLER_COLS + D, Dpad = (D + 7) & ~7, J = o.history_size, K = o.num_elbo_draws, Mn = o.num_draws;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  hipStream_t st = sp->stream;
  int G = 0;
  HIP_TRY(hipDeviceGetAttribute(&G, hipDeviceAttributeMultiprocessorCount, sp->device));
  G = std::max(G, 1);
  if (const char *e = getenv("POTUS_PATHFINDER_G")) G = std::max(1, atoi(e));   // tests: no output depends on it
  const size_t lds = sp->lds_bytes;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_pf_elbo), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_pf_draws), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  DsPlan pl;
  pl.of(sp);
  // the handle's rows of the last call go first: a call that fails leaves none behind
  HIP_TRY(hipStreamSynchronize(st));
  if (sp->pf_rows) { (void)hipFree(sp->pf_rows); sp->pf_rows = nullptr; }
  sp->pf_paths = sp->pf_draws = 0; sp->pf_code.clear();
  int rc;
  double *drows = nullptr;
  const size_t rows_total = (size_t)n_paths * Mn;
  if (Mn > 0) {
    void *p = nullptr;
    if (hipMalloc(&p, rows_total * row * 8) != hipSuccess) { (void)hipGetLastError(); return fail(POTUS_ERR_DEVICE, "%s: hipMalloc of %zu bytes for the rows failed", what, rows_total * row * 8); }
    drows = static_cast<double *>(p);
  }
  struct RowsOwner { double *p; ~RowsOwner() { if (p) (void)hipFree(p); } } owner{drows};   // until the call has succeeded
  const size_t nl = (size_t)n_paths * rows;
  double *alpha = nullptr, *abc = nullptr, *work = nullptr, *delbo = nullptr, *due = nullptr, *dud = nullptr, *dmu = nullptr, *dld = nullptr, *dlp = nullptr, *dlq = nullptr;
  int *dkept = nullptr, *dL = nullptr, *dsel = nullptr, *dwant = nullptr;
  PfParams *dP = nullptr, *dP2 = nullptr;
  PfSmall *dsmall = nullptr;
  double *dphi = nullptr, *dlqw = nullptr, *dqtq = nullptr;
  const bool want_draws = want_l && Mn > 0 && (out.phi || out.lqw || out.qtq);
  if ((rc = tmp.get(&alpha, nl * Dpad * 8, what)) || (rc = tmp.get(&abc, nl * 3 * 8, what)) || (rc = tmp.get(&work, (size_t)G * (2 * J + 4) * Dpad * 8, what)) ||
      (rc = tmp.get(&delbo, nl * 8, what)) || (rc = tmp.get(&dkept, nl * 4, what)) || (rc = tmp.get(&dL, (size_t)n_paths * 4, what)) ||
      (rc = tmp.get(&dsel, (size_t)n_paths * 4, what)) || (rc = tmp.get(&dwant, (size_t)n_paths * 4, what)) || (rc = tmp.get(&dmu, (size_t)n_paths * D * 8, what)) ||
      (rc = tmp.get(&dld, (size_t)n_paths * 8, what)) || (rc = tmp.get(&dlp, std::max<size_t>(rows_total, 1) * 8, what)) ||
      (rc = tmp.get(&dlq, std::max<size_t>(rows_total, 1) * 8, what)) || (rc = tmp.get(&dP, sizeof(PfParams), what)) || (rc = tmp.get(&dP2, sizeof(PfParams), what)) ||
      (rc = tmp.get(&dsmall, (size_t)G * sizeof(PfSmall), what))) return rc;
  if (u_elbo) {
    const size_t nb = (size_t)n_paths * (rows - 1) * K * D * 8;
    if ((rc = tmp.get(&due, nb, what))) return rc;
    HIP_TRY(hipMemcpyAsync(due, u_elbo, nb, hipMemcpyHostToDevice, st));
  }
  if (u_draws && Mn > 0) {
    if ((rc = tmp.get(&dud, rows_total * D * 8, what))) return rc;
    HIP_TRY(hipMemcpyAsync(dud, u_draws, rows_total * D * 8, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipMemcpyAsync(dL, hL.data(), (size_t)n_paths * 4, hipMemcpyHostToDevice, st));
  std::vector<int> hwant(n_paths, -1);
  if (want_l) for (int p = 0; p < n_paths; p++) hwant[p] = want_l[p];
  HIP_TRY(hipMemcpyAsync(dwant, hwant.data(), (size_t)n_paths * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(dmu, 0xFF, (size_t)n_paths * D * 8, st));   // (NaN: an iterate nobody asked for, or outside 1 .. L)
  HIP_TRY(hipMemsetAsync(dld, 0xFF, (size_t)n_paths * 8, st));
  if (want_draws) {
    if ((rc = tmp.get(&dphi, rows_total * D * 8, what)) || (rc = tmp.get(&dlqw, rows_total * 8, what)) || (rc = tmp.get(&dqtq, (size_t)n_paths * PF_MAX_N * PF_MAX_N * 8, what))) return rc;
    HIP_TRY(hipMemsetAsync(dphi, 0xFF, rows_total * D * 8, st));
    HIP_TRY(hipMemsetAsync(dlqw, 0xFF, rows_total * 8, st));
    HIP_TRY(hipMemsetAsync(dqtq, 0xFF, (size_t)n_paths * PF_MAX_N * PF_MAX_N * 8, st));
  }
  PfParams P{dX, dG, dL, alpha, dkept, abc, work, dsmall, delbo, due, dud, dsel, want_l ? dwant : nullptr, dmu, dld, drows, dlp, dlq, dphi, dlqw, dqtq,
             n_paths, rows, n_paths / pl.n_ds, J, K, Mn, 1, D, Dpad, o.path_offset, o.draw_offset, sp->R.seed_lo, sp->R.seed_hi};
  HIP_TRY(hipMemcpyAsync(dP, &P, sizeof(P), hipMemcpyHostToDevice, st));
  EventTimer t_alpha, t_elbo, t_draws;
  HIP_TRY(t_alpha.made); HIP_TRY(t_elbo.made); HIP_TRY(t_draws.made);
  HIP_TRY(t_alpha.start(st));
  hipLaunchKernelGGL(k_pf_alpha, dim3(n_paths), dim3(PT_THREADS), 0, st, (const PfParams *)dP);
  HIP_TRY(hipGetLastError());
  HIP_TRY(t_alpha.stop(st));
  const long long n_items = (long long)n_paths * (rows - 1);
  HIP_TRY(t_elbo.start(st));
  if (n_items > 0) {
    hipLaunchKernelGGL(k_pf_elbo, dim3((unsigned)std::min<long long>(G, n_items)), dim3(PT_THREADS), lds, st, pl.Mg, (const PfParams *)dP);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(t_elbo.stop(st));
  std::vector<double> helbo(nl, nan);
  std::vector<int> hkept(nl, 0);
  HIP_TRY(hipMemcpyAsync(helbo.data(), delbo, nl * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hkept.data(), dkept, nl * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));   // the ELBOs decide which iterate the draws come from
  std::vector<int> hsel(n_paths, 0), code(n_paths, PF_NO_ELBO);
  for (int p = 0; p < n_paths; p++) {
    double best = -std::numeric_limits<double>::infinity();
    for (int l = 0; l < rows; l++) {
      double &e = helbo[(size_t)p * rows + l];
      if (l < 1 || l > hL[p]) { e = nan; hkept[(size_t)p * rows + l] = 0; continue; }
      if (std::isfinite(e) && e > best) { best = e; hsel[p] = l; }   // (strict: the lowest l on ties)
    }
    if (hsel[p]) code[p] = PF_OK;
  }
  HIP_TRY(t_draws.start(st));
  if (Mn > 0) {
    const int nchunk = std::max(1, std::min(Mn, G / n_paths));
    P.chunk = (Mn + nchunk - 1) / nchunk;
    const long long d_items = (long long)n_paths * ((Mn + P.chunk - 1) / P.chunk);
    HIP_TRY(hipMemcpyAsync(dsel, hsel.data(), (size_t)n_paths * 4, hipMemcpyHostToDevice, st));
    P.want_l = nullptr;
    HIP_TRY(hipMemcpyAsync(dP2, &P, sizeof(P), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pf_draws, dim3((unsigned)std::min<long long>(G, d_items)), dim3(PT_THREADS), lds, st, pl.Mg, (const PfParams *)dP2);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(t_draws.stop(st));
  if (Mn > 0) {
    if (out.q) HIP_TRY(hipMemcpy2DAsync(out.q, (size_t)D * 8, drows + POTUS_N_SAMPLER_COLS, (size_t)row * 8, (size_t)D * 8, rows_total, hipMemcpyDeviceToHost, st));
    if (out.lp) HIP_TRY(hipMemcpyAsync(out.lp, dlp, rows_total * 8, hipMemcpyDeviceToHost, st));
    if (out.lq) HIP_TRY(hipMemcpyAsync(out.lq, dlq, rows_total * 8, hipMemcpyDeviceToHost, st));
  }
  if (out.mu) HIP_TRY(hipMemcpyAsync(out.mu, dmu, (size_t)n_paths * D * 8, hipMemcpyDeviceToHost, st));
  if (out.logdet) HIP_TRY(hipMemcpyAsync(out.logdet, dld, (size_t)n_paths * 8, hipMemcpyDeviceToHost, st));
  if (want_draws) {
    if (out.phi) HIP_TRY(hipMemcpyAsync(out.phi, dphi, rows_total * D * 8, hipMemcpyDeviceToHost, st));
    if (out.lqw) HIP_TRY(hipMemcpyAsync(out.lqw, dlqw, rows_total * 8, hipMemcpyDeviceToHost, st));
    if (out.qtq) HIP_TRY(hipMemcpyAsync(out.qtq, dqtq, (size_t)n_paths * PF_MAX_N * PF_MAX_N * 8, hipMemcpyDeviceToHost, st));
  }
  if (out.alpha)
    for (int p = 0; p < n_paths; p++) {
      const int l = hwant[p];
      if (l >= 0 && l <= hL[p]) HIP_TRY(hipMemcpyAsync(out.alpha + (size_t)p * D, alpha + ((size_t)p * rows + l) * Dpad, (size_t)D * 8, hipMemcpyDeviceToHost, st));
      else std::fill(out.alpha + (size_t)p * D, out.alpha + (size_t)(p + 1) * D, nan);
    }
  HIP_TRY(hipStreamSynchronize(st));
  if ((rc = t_alpha.elapsed_or_fail(&ms[0])) || (rc = t_elbo.elapsed_or_fail(&ms[1])) || (rc = t_draws.elapsed_or_fail(&ms[2]))) return rc;
  for (int p = 0; p < n_paths; p++) {
    int32_t *io = out.info + (size_t)p * 4;
    io[0] = code[p]; io[1] = hL[p]; io[2] = hsel[p]; io[3] = opt_code ? opt_code[p] : 0;
  }
  if (out.elbo) std::copy(helbo.begin(), helbo.end(), out.elbo);
  if (out.kept) std::copy(hkept.begin(), hkept.end(), out.kept);
  if (Mn > 0) { sp->pf_rows = drows; owner.p = nullptr; sp->pf_paths = n_paths; sp->pf_draws = Mn; sp->pf_code = code; }
  return 0;
}
} // namespace

void potus_default_pathfinder_opts(potus_pathfinder_opts *o) {
  if (!o) return;
  potus_default_optimize_opts(&o->opt);
  o->opt.jacobian = 1; o->opt.iter = 1000;
  o->history_size = 6; o->num_elbo_draws = 25; o->num_draws = 1000; o->draw_offset = 0; o->path_offset = 0; o->pad0 = 0;
}

int potus_pathfinder(int handle, const potus_pathfinder_opts *opts, const double *q0, int n_paths, int32_t *info_out, double *elbo_out, int32_t *kept_out,
                     double *q_out, double *lp_out, double *lq_out, double *traj_x_out, double *traj_g_out) {
  const char *what = "potus_pathfinder";
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  potus_pathfinder_opts o;
  potus_default_pathfinder_opts(&o);
  if (opts) o = *opts;
  o.opt.jacobian = 1; o.opt.path_offset = o.path_offset;   // the density the sampler draws from; one offset for the starts and the normals
  if (const int rc_ = pf_check(sp, what, o, n_paths)) return rc_;
  if (const int rc_ = opt_check(sp, what, o.opt, n_paths, info_out ? nullptr : "info_out")) return rc_;
  const int D = sp->L.D, Dpad = (D + 7) & ~7, rows = o.opt.iter + 1;
  DeviceGuard guard;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  DevBufs tmp;
  double *dX = nullptr, *dG = nullptr;
  int rc;
  if ((rc = tmp.get(&dX, (size_t)n_paths * rows * Dpad * 8, what)) || (rc = tmp.get(&dG, (size_t)n_paths * rows * Dpad * 8, what))) return rc;
  EventTimer ev;
  OptRun r;
  if ((rc = opt_launch(sp, what, o.opt, q0, n_paths, tmp, dX, dG, rows, ev, r))) return rc;
  std::vector<int> hinfo((size_t)n_paths * 3), hL(n_paths), ocode(n_paths);
  HIP_TRY(hipMemcpyAsync(hinfo.data(), r.dinfo, hinfo.size() * 4, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  for (int p = 0; p < n_paths; p++) { ocode[p] = hinfo[(size_t)p * 3]; hL[p] = ocode[p] == OPT_INIT ? 0 : std::min(hinfo[(size_t)p * 3 + 1], rows - 1); }
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
  if ((rc = ev.elapsed_or_fail(&ms[0]))) return rc;
  const PfOut out{info_out, elbo_out, kept_out, q_out, lp_out, lq_out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if ((rc = pf_core(sp, what, o, tmp, dX, dG, hL, rows, n_paths, nullptr, nullptr, nullptr, ocode.data(), out, ms + 1))) return rc;
  for (int k = 0; k < 2; k++) if (double *t = k ? traj_g_out : traj_x_out)
    HIP_TRY(hipMemcpy2D(t, (size_t)D * 8, k ? dG : dX, (size_t)Dpad * 8, (size_t)D * 8, (size_t)n_paths * rows, hipMemcpyDeviceToHost));
  if (traj_x_out || traj_g_out) {   // rows behind a path's end were never written
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int p = 0; p < n_paths; p++) {
      const int first = ocode[p] == OPT_INIT ? 0 : hL[p] + 1;
      for (double *t : {traj_x_out, traj_g_out}) if (t) std::fill(t + ((size_t)p * rows + first) * D, t + (size_t)(p + 1) * rows * D, nan);
    }
  }
  std::copy(ms, ms + 4, g_pf_ms);
  return 0;
}

int potus_pathfinder_path(int handle, const potus_pathfinder_opts *opts, const double *x, const double *g, const int32_t *L, int rows, int n_paths,
                          const double *u_elbo, const double *u_draws, const int32_t *want_l, int32_t *info_out, double *elbo_out, int32_t *kept_out,
                          double *q_out, double *lp_out, double *lq_out, double *mu_out, double *alpha_out, double *logdet_out,
                          double *phi_out, double *lqw_out, double *qtq_out) {
  const char *what = "potus_pathfinder_path";
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  potus_pathfinder_opts o;
  potus_default_pathfinder_opts(&o);
  if (opts) o = *opts;
  if (const int rc_ = pf_check(sp, what, o, n_paths)) return rc_;
  if (!x || !g || !L || !info_out) return fail(POTUS_ERR_ARG, "%s: null argument (x, g, L and info_out are required)", what);
  if (rows < 2) return fail(POTUS_ERR_ARG, "%s: rows = %d: a trajectory has at least the rows 0 and 1", what, rows);
  std::vector<int> hL(n_paths);
  for (int p = 0; p < n_paths; p++) {
    if (L[p] < 0 || L[p] > rows - 1) return fail(POTUS_ERR_ARG, "%s: L[%d] = %d outside 0..%d", what, p, L[p], rows - 1);
    hL[p] = L[p];
  }
  const int D = sp->L.D, Dpad = (D + 7) & ~7;
  DeviceGuard guard;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  DevBufs tmp;
  double *dX = nullptr, *dG = nullptr;
  int rc;
  if ((rc = tmp.get(&dX, (size_t)n_paths * rows * Dpad * 8, what)) || (rc = tmp.get(&dG, (size_t)n_paths * rows * Dpad * 8, what))) return rc;
  HIP_TRY(hipMemcpy2DAsync(dX, (size_t)Dpad * 8, x, (size_t)D * 8, (size_t)D * 8, (size_t)n_paths * rows, hipMemcpyHostToDevice, sp->stream));
  HIP_TRY(hipMemcpy2DAsync(dG, (size_t)Dpad * 8, g, (size_t)D * 8, (size_t)D * 8, (size_t)n_paths * rows, hipMemcpyHostToDevice, sp->stream));
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
  const PfOut out{info_out, elbo_out, kept_out, q_out, lp_out, lq_out, mu_out, alpha_out, logdet_out, phi_out, lqw_out, qtq_out};
  if ((rc = pf_core(sp, what, o, tmp, dX, dG, hL, rows, n_paths, u_elbo, u_draws, want_l, nullptr, out, ms + 1))) return rc;
  std::copy(ms, ms + 4, g_pf_ms);
  return 0;
}

int potus_pathfinder_timing(double *ms) {
  return timing_out("potus_pathfinder_timing", g_pf_ms, 4, ms);
}

// ---------------------------------------------------------------------------------------------- mean-field ADVI (potus_advi.hpp)
namespace {
thread_local double g_vi_ms[4] = {0.0, 0.0, 0.0, 0.0};   // the calling thread's last potus_advi: adaptation, gradient segments, ELBO, draws (HIP events, summed)
}

void potus_default_advi_opts(potus_advi_opts *o) {
  if (!o) return;
  o->algorithm = POTUS_ADVI_MEANFIELD; o->iter = 10000; o->grad_samples = 1; o->elbo_samples = 100; o->eval_elbo = 100; o->adapt_engaged = 1;
  o->adapt_iter = 50; o->output_samples = 1000; o->draw_offset = 0; o->run_offset = 0; o->eta = 1.0; o->tol_rel_obj = 0.01; o->elbo_offset = 0.0;
}

int potus_advi(int handle, const potus_advi_opts *opts, const double *q0, int n_runs, int32_t *info_out, double *mu_out, double *omega_out,
               double *elbo_out, double *adapt_elbo_out, double *q_out, double *lp_out, double *lq_out) {
  const char *what = "potus_advi";
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  potus_advi_opts o;
  potus_default_advi_opts(&o);
  if (opts) o = *opts;
  if (const int rc_ = paths_check(sp, what, n_runs, "n_runs")) return rc_;
  if (o.algorithm == POTUS_ADVI_FULLRANK) return fail(POTUS_ERR_UNSUPPORTED, "%s: algorithm = fullrank is not built (a D x D factor updated every iteration); meanfield only", what);
  if (o.algorithm != POTUS_ADVI_MEANFIELD) return fail(POTUS_ERR_ARG, "%s: algorithm = %d, 0 (meanfield)", what, o.algorithm);
  if (!info_out) return fail(POTUS_ERR_ARG, "%s: null output (info_out is required)", what);
  if (o.iter < 1) return fail(POTUS_ERR_ARG, "%s: iter = %d, at least 1", what, o.iter);
  if (o.grad_samples < 1 || o.grad_samples > VI_MAX_SAMPLES) return fail(POTUS_ERR_ARG, "%s: grad_samples = %d outside 1..%d", what, o.grad_samples, VI_MAX_SAMPLES);
  if (o.elbo_samples < 1 || o.elbo_samples > VI_MAX_SAMPLES) return fail(POTUS_ERR_ARG, "%s: elbo_samples = %d outside 1..%d", what, o.elbo_samples, VI_MAX_SAMPLES);
  if (o.eval_elbo < 1) return fail(POTUS_ERR_ARG, "%s: eval_elbo = %d, at least 1", what, o.eval_elbo);
  if (o.adapt_engaged != 0 && o.adapt_engaged != 1) return fail(POTUS_ERR_ARG, "%s: adapt_engaged = %d, 0 or 1", what, o.adapt_engaged);
  if (o.adapt_iter < 1) return fail(POTUS_ERR_ARG, "%s: adapt_iter = %d, at least 1", what, o.adapt_iter);
  if (o.output_samples < 0) return fail(POTUS_ERR_ARG, "%s: output_samples = %d", what, o.output_samples);
  if (!(o.eta > 0.0) || !std::isfinite(o.eta)) return fail(POTUS_ERR_ARG, "%s: eta = %g, must be positive and finite", what, o.eta);
  if (!(o.tol_rel_obj >= 0.0) || !std::isfinite(o.tol_rel_obj)) return fail(POTUS_ERR_ARG, "%s: tol_rel_obj = %g, must be finite and not negative", what, o.tol_rel_obj);
  if (!std::isfinite(o.elbo_offset)) return fail(POTUS_ERR_ARG, "%s: elbo_offset = %g, must be finite", what, o.elbo_offset);
  if (o.draw_offset < 0 || (long long)o.draw_offset + o.output_samples >= 0xFFFFFFFFll) return fail(POTUS_ERR_ARG, "%s: draw_offset = %d with %d draws", what, o.draw_offset, o.output_samples);
  if (o.run_offset < 0 || (long long)o.run_offset + n_runs >= 0xFFFFFFFFll) return fail(POTUS_ERR_ARG, "%s: run_offset = %d with %d runs", what, o.run_offset, n_runs);
  const int D = sp->L.D, row = POTUS_N_SAMPLER_COLS + D, Dpad = (D + 7) & ~7, K = o.elbo_samples, Mn = o.output_samples;
  const int n_stage = o.adapt_engaged ? 1 + ADVI_N_ETA : 1, n_tracks = n_stage * n_runs, trace = o.iter / o.eval_elbo + 1;
  if ((unsigned long long)VI_NVEC * Dpad * 8ull >= 0x7fffffffull) return fail(POTUS_ERR_UNSUPPORTED, "%s: D = %d: a track's working set must stay below 2 GB", what, D);
  if ((unsigned long long)n_runs * std::max(Mn, 1) * row >= (1ull << 40) || (unsigned long long)n_tracks * K >= (1ull << 31))
    return fail(POTUS_ERR_ARG, "%s: %d runs x %d draws of %d coordinates, %d ELBO draws", what, n_runs, Mn, D, K);
  const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
  DeviceGuard guard;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  hipStream_t st = sp->stream;
  int G = 0;
  HIP_TRY(hipDeviceGetAttribute(&G, hipDeviceAttributeMultiprocessorCount, sp->device));
  G = std::max(G, 1);
  if (const char *e = getenv("POTUS_ADVI_G")) G = std::max(1, atoi(e));   // tests and scripts/variational.py: no output depends on it
  const size_t lds = sp->lds_bytes;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_vi_sga), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_vi_elbo), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lap_lp), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  DsPlan pl;
  pl.of(sp);
  const int per_ds = n_runs / pl.n_ds;
  // the handle's rows of the last call go first: a call that fails leaves none behind
  HIP_TRY(hipStreamSynchronize(st));
  if (sp->vi_rows) { (void)hipFree(sp->vi_rows); sp->vi_rows = nullptr; }
  sp->vi_runs = sp->vi_draws = 0; sp->vi_code.clear();
  int rc;
  double *drows = nullptr;
  const size_t rows_total = (size_t)n_runs * Mn;
  if (Mn > 0) {
    void *p = nullptr;
    if (hipMalloc(&p, rows_total * row * 8) != hipSuccess) { (void)hipGetLastError(); return fail(POTUS_ERR_DEVICE, "%s: hipMalloc of %zu bytes for the rows failed", what, rows_total * row * 8); }
    drows = static_cast<double *>(p);
  }
  struct RowsOwner { double *p; ~RowsOwner() { if (p) (void)hipFree(p); } } owner{drows};   // until the call has succeeded
  DevBufs tmp;   // the working set is the call's own: the sampler's chain state is not touched
  const int lp_grid = std::max(1, std::min(Mn, 1024));
  double *dq0 = nullptr, *work = nullptr, *dslot = nullptr, *dent = nullptr, *escr = nullptr, *dlq = nullptr, *dlp = nullptr, *gscr = nullptr;
  ViTrack *dtrack = nullptr;
  int *det = nullptr, *dno = nullptr;
  ViParams *dP = nullptr;
  if ((rc = tmp.get(&work, (size_t)n_tracks * VI_NVEC * Dpad * 8, what)) || (rc = tmp.get(&dtrack, (size_t)n_tracks * sizeof(ViTrack), what)) ||
      (rc = tmp.get(&det, (size_t)n_tracks * 4, what)) || (rc = tmp.get(&dslot, (size_t)n_tracks * K * 8, what)) || (rc = tmp.get(&dent, (size_t)n_tracks * 8, what)) ||
      (rc = tmp.get(&escr, (size_t)G * 2 * Dpad * 8, what)) || (rc = tmp.get(&dlq, std::max<size_t>(rows_total, 1) * 8, what)) ||
      (rc = tmp.get(&dlp, std::max<size_t>(rows_total, 1) * 8, what)) || (rc = tmp.get(&gscr, (size_t)lp_grid * Dpad * 8, what)) ||
      (rc = tmp.get(&dno, (size_t)n_runs * 4, what)) || (rc = tmp.get(&dP, sizeof(ViParams), what))) return rc;
  if (q0) {
    if ((rc = tmp.get(&dq0, (size_t)n_runs * D * 8, what))) return rc;
    HIP_TRY(hipMemcpyAsync(dq0, q0, (size_t)n_runs * D * 8, hipMemcpyHostToDevice, st));
  }
  std::vector<ViTrack> hT(n_tracks);
  for (int k = 0; k < n_tracks; k++) {
    const int stage = k / n_runs;
    hT[k] = ViTrack{stage ? advi_eta(stage - 1) : o.eta, 0, 0, stage ? o.adapt_iter : 0, 0};
  }
  ViParams P{dq0, work, dtrack, det, dslot, dent, escr, drows, dlq, dno, n_runs, per_ds, D, Dpad, o.grad_samples, K, 0, Mn, o.run_offset, o.draw_offset, 1,
             sp->R.init_radius, sp->R.seed_lo, sp->R.seed_hi};
  LapSpans t_adapt, t_grad, t_elbo, t_draws;
  // n_blocks tracks from 0 on, each for its own n_iter iterations (a track whose code is set returns at once)
  auto sga = [&](int n_blocks, int init, LapSpans &span) -> int {
    P.init = init;
    HIP_TRY(hipMemcpyAsync(dtrack, hT.data(), (size_t)n_blocks * sizeof(ViTrack), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dP, &P, sizeof(P), hipMemcpyHostToDevice, st));   // (pageable sources: copied before the calls return)
    if (const int r_ = span.begin(st)) return r_;
    hipLaunchKernelGGL(k_vi_sga, dim3(n_blocks), dim3(PT_THREADS), lds, st, pl.Mg, (const ViParams *)dP);
    HIP_TRY(hipGetLastError());
    return span.end(st);
  };
  // the ELBO of the listed tracks at their iterates: one launch, one synchronisation; the mean over a track's slots in index order
  std::vector<double> hslot((size_t)n_tracks * K), hent(n_tracks);
  const double entropy0 = 0.5 * (double)D * (1.0 + 1.8378770664093454836);
  auto elbo_of = [&](const std::vector<int> &tracks, std::vector<double> &out) -> int {
    const int n_et = (int)tracks.size();
    const long long n_items = (long long)n_et * K;
    P.n_et = n_et;
    HIP_TRY(hipMemcpyAsync(det, tracks.data(), (size_t)n_et * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dP, &P, sizeof(P), hipMemcpyHostToDevice, st));
    if (const int r_ = t_elbo.begin(st)) return r_;
    hipLaunchKernelGGL(k_vi_elbo, dim3((unsigned)std::min<long long>(G, n_items)), dim3(PT_THREADS), lds, st, pl.Mg, (const ViParams *)dP);
    HIP_TRY(hipGetLastError());
    if (const int r_ = t_elbo.end(st)) return r_;
    HIP_TRY(hipMemcpyAsync(hslot.data(), dslot, (size_t)n_items * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hent.data(), dent, (size_t)n_et * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hT.data(), dtrack, (size_t)n_tracks * sizeof(ViTrack), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out.assign(n_et, ninf);
    for (int e = 0; e < n_et; e++) {
      double acc = 0.0;
      bool bad = false;
      for (int k = 0; k < K; k++) { const double v = hslot[(size_t)e * K + k]; bad = bad || !std::isfinite(v); acc += v; }
      if (!bad) out[e] = acc / (double)K + entropy0 + hent[e] + o.elbo_offset;
    }
    return 0;
  };

  // ---- the starts, the five candidates of every run at once, the initial ELBO and theirs, the sequential rule on the five numbers
  std::vector<int> code(n_runs, 0), flags(n_runs, 0), eta_index(n_runs, -1), iters(n_runs, 0);
  std::vector<long long> passes(n_runs, 0);
  std::vector<double> htrace((size_t)n_runs * trace, nan), hadapt((size_t)n_runs * ADVI_N_ETA, nan), e0;
  if ((rc = sga(n_tracks, 1, t_adapt))) return rc;
  {
    std::vector<int> all(n_tracks);
    for (int k = 0; k < n_tracks; k++) all[k] = k;
    if ((rc = elbo_of(all, e0))) return rc;
  }
  for (int r = 0; r < n_runs; r++) {
    htrace[(size_t)r * trace] = e0[r];
    passes[r] += K;
    double eta = o.eta;
    if (!std::isfinite(e0[r])) code[r] = ADVI_INIT;
    if (o.adapt_engaged) {
      double cand[ADVI_N_ETA];
      for (int k = 0; k < ADVI_N_ETA; k++) {
        const ViTrack &tk = hT[(size_t)(k + 1) * n_runs + r];
        cand[k] = tk.code ? ninf : e0[(size_t)(k + 1) * n_runs + r];
        hadapt[(size_t)r * ADVI_N_ETA + k] = cand[k];
        passes[r] += (long long)tk.t * o.grad_samples + (tk.code ? 1 : K);
      }
      if (!code[r]) {
        eta_index[r] = advi_pick_eta(e0[r], cand, nullptr);
        if (eta_index[r] < 0) code[r] = ADVI_ADAPT_FAILED; else eta = advi_eta(eta_index[r]);
      }
    }
    hT[r] = ViTrack{eta, 0, code[r], 0, 0};
  }

  // ---- the main runs: segments of eval_elbo iterations, one synchronisation each
  std::vector<AdviConv> conv(n_runs, AdviConv(o.iter, o.eval_elbo));
  std::vector<int> live;
  std::vector<double> e1;
  for (int t_now = 0;;) {
    live.clear();
    for (int r = 0; r < n_runs; r++) if (!code[r]) live.push_back(r);
    if (live.empty()) break;
    const int seg = std::min(o.eval_elbo, o.iter - t_now);
    for (int r : live) hT[r].n_iter = seg;
    if ((rc = sga(n_runs, 0, t_grad))) return rc;
    t_now += seg;
    const bool eval = t_now % o.eval_elbo == 0;
    if (eval) { if ((rc = elbo_of(live, e1))) return rc; }
    else {
      HIP_TRY(hipMemcpyAsync(hT.data(), dtrack, (size_t)n_runs * sizeof(ViTrack), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    for (size_t e = 0; e < live.size(); e++) {
      const int r = live[e];
      if (hT[r].code == ADVI_NONFINITE) code[r] = ADVI_NONFINITE;     // found by the track itself: it stands at its last finished iterate
      else if (eval) {
        htrace[(size_t)r * trace + t_now / o.eval_elbo] = e1[e];
        passes[r] += K;
        code[r] = conv[r].push(e1[e], t_now, o.iter, o.eval_elbo, o.tol_rel_obj, &flags[r]);
      } else code[r] = ADVI_MAXIT;                                      // iter is no multiple of eval_elbo: the tail has no evaluation
      hT[r].code = code[r];
    }
  }
  for (int r = 0; r < n_runs; r++) {
    iters[r] = hT[r].t;
    passes[r] += (long long)hT[r].t * o.grad_samples + (code[r] == ADVI_NONFINITE ? 1 : 0);
  }

  // ---- the draws, and what goes back
  std::vector<int> no_draws(n_runs);
  for (int r = 0; r < n_runs; r++) no_draws[r] = code[r] == ADVI_INIT || code[r] == ADVI_ADAPT_FAILED;
  if (Mn > 0) {
    HIP_TRY(hipMemcpyAsync(dno, no_draws.data(), (size_t)n_runs * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dP, &P, sizeof(P), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dlp, 0xFF, rows_total * 8, st));   // (NaN: a run without an approximation)
    if ((rc = t_draws.begin(st))) return rc;
    hipLaunchKernelGGL(k_vi_draws, dim3((unsigned)std::min<size_t>(rows_total, 65535)), dim3(PT_THREADS), 0, st, (const ViParams *)dP);
    HIP_TRY(hipGetLastError());
    for (int r = 0; r < n_runs; r++) if (!no_draws[r]) {   // lp__ with the run's model: Laplace's stage, the bytes of potus_log_prob_grad
      hipLaunchKernelGGL(k_lap_lp, dim3(lp_grid), dim3(PT_THREADS), lds, st, pl.Mg + r / per_ds, drows + (size_t)r * Mn * row, Mn, gscr, Dpad, dlp + (size_t)r * Mn);
      HIP_TRY(hipGetLastError());
      passes[r] += Mn;
    }
    if ((rc = t_draws.end(st))) return rc;
    if (q_out) HIP_TRY(hipMemcpy2DAsync(q_out, (size_t)D * 8, drows + POTUS_N_SAMPLER_COLS, (size_t)row * 8, (size_t)D * 8, rows_total, hipMemcpyDeviceToHost, st));
    if (lp_out) HIP_TRY(hipMemcpyAsync(lp_out, dlp, rows_total * 8, hipMemcpyDeviceToHost, st));
    if (lq_out) HIP_TRY(hipMemcpyAsync(lq_out, dlq, rows_total * 8, hipMemcpyDeviceToHost, st));
  }
  const size_t wpitch = (size_t)VI_NVEC * Dpad * 8;   // the main tracks are the first n_runs
  if (mu_out) HIP_TRY(hipMemcpy2DAsync(mu_out, (size_t)D * 8, work + (size_t)VI_V_MU * Dpad, wpitch, (size_t)D * 8, n_runs, hipMemcpyDeviceToHost, st));
  if (omega_out) HIP_TRY(hipMemcpy2DAsync(omega_out, (size_t)D * 8, work + (size_t)VI_V_OM * Dpad, wpitch, (size_t)D * 8, n_runs, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  double ms[4];
  if ((rc = t_adapt.sum(&ms[0])) || (rc = t_grad.sum(&ms[1])) || (rc = t_elbo.sum(&ms[2])) || (rc = t_draws.sum(&ms[3]))) return rc;
  std::copy(ms, ms + 4, g_vi_ms);
  for (int r = 0; r < n_runs; r++) {
    int32_t *io = info_out + (size_t)r * 6;
    io[0] = code[r]; io[1] = flags[r]; io[2] = iters[r]; io[3] = eta_index[r]; io[4] = (int32_t)std::min<long long>(passes[r], 0x7fffffffll); io[5] = 0;
    for (int k = 1; k < trace; k++) if (!std::isnan(htrace[(size_t)r * trace + k])) io[5] = k;   // evaluations of the main run
    if (no_draws[r]) for (double *v : {mu_out, omega_out}) if (v) std::fill(v + (size_t)r * D, v + (size_t)(r + 1) * D, nan);
  }
  if (elbo_out) std::copy(htrace.begin(), htrace.end(), elbo_out);
  if (adapt_elbo_out) std::copy(hadapt.begin(), hadapt.end(), adapt_elbo_out);
  if (Mn > 0) { sp->vi_rows = drows; owner.p = nullptr; sp->vi_runs = n_runs; sp->vi_draws = Mn; sp->vi_code = no_draws; }
  return 0;
}

int potus_advi_write_array_device(int handle, int col_begin, int col_end, void *out_device) {
  return kept_write_array_device("potus_advi_write_array_device", KEPT_ADVI, handle, col_begin, col_end, out_device);
}
int potus_advi_scores_device(int handle, int day_begin, int day_end, void *out_device) {
  return kept_scores_device("potus_advi_scores_device", KEPT_ADVI, handle, day_begin, day_end, out_device);
}
int potus_advi_summary(int handle, int day_begin, int day_end, const double *ev, int ev_to_win, double *state_out, double *natl_out, double *ev_out, int32_t *n_draws_out) {
  return kept_summary("potus_advi_summary", KEPT_ADVI, handle, day_begin, day_end, ev, ev_to_win, state_out, natl_out, ev_out, n_draws_out);
}
int potus_advi_timing(double *ms) {
  return timing_out("potus_advi_timing", g_vi_ms, 4, ms);
}

int potus_simulate_prior(int handle, uint64_t seed, int n_sims, int sim_offset, double *q_out, int32_t *n_democrat_state_out, int32_t *n_democrat_national_out) {
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  if (const int rc_ = refuse_own_models(sp, "potus_simulate_prior")) return rc_;
  if (n_sims < 0 || sim_offset < 0 || (long long)sim_offset + n_sims >= 0xFFFFFFFFll) return fail(POTUS_ERR_ARG, "potus_simulate_prior: n_sims = %d, sim_offset = %d", n_sims, sim_offset);
  if (n_sims == 0) return 0;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  const int D = sp->L.D, row = POTUS_N_SAMPLER_COLS + D, Ns = sp->M.Ns, Np = sp->M.Npoll;
  const int grid = std::min(n_sims, 512);
  DevBufs tmp;
  double *qrow = nullptr, *scratch = nullptr;
  int *y = nullptr;
  HIP_TRY(tmp.alloc(&qrow, (size_t)n_sims * row * 8)); HIP_TRY(tmp.alloc(&scratch, (size_t)grid * sp->L.ncols * 8));
  HIP_TRY(tmp.alloc(&y, (size_t)n_sims * std::max(Np, 1) * 4));
  SimParams P{qrow, scratch, y, n_sims, sp->L.ncols, sim_offset, (unsigned)(seed & 0xFFFFFFFFu), (unsigned)(seed >> 32)};
  hipLaunchKernelGGL(k_simulate_prior, dim3(grid), dim3(256), 0, sp->stream, (const DevModel *)sp->dM, P);
  HIP_TRY(hipGetLastError());
  std::vector<double> hq((size_t)n_sims * row);
  std::vector<int32_t> hy((size_t)n_sims * Np);
  HIP_TRY(hipMemcpyAsync(hq.data(), qrow, hq.size() * 8, hipMemcpyDeviceToHost, sp->stream));
  if (Np) HIP_TRY(hipMemcpyAsync(hy.data(), y, hy.size() * 4, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  for (int i = 0; i < n_sims; i++) {
    if (q_out) std::copy(hq.begin() + (size_t)i * row + POTUS_N_SAMPLER_COLS, hq.begin() + (size_t)(i + 1) * row, q_out + (size_t)i * D);
    if (n_democrat_state_out) std::copy(hy.begin() + (size_t)i * Np, hy.begin() + (size_t)i * Np + Ns, n_democrat_state_out + (size_t)i * Ns);
    if (n_democrat_national_out) std::copy(hy.begin() + (size_t)i * Np + Ns, hy.begin() + (size_t)(i + 1) * Np, n_democrat_national_out + (size_t)i * (Np - Ns));
  }
  return 0;
}

int potus_constrain(int handle, const double *q, int n, int col_begin, int col_end, double *out) {
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  if (const int rc_ = refuse_own_models(sp, "potus_constrain")) return rc_;
  if (n < 0 || (n > 0 && (!q || !out))) return fail(POTUS_ERR_ARG, "potus_constrain: null argument");
  if (const int rc_ = check_cols(sp, col_begin, col_end)) return rc_;
  if (n == 0) return 0;
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  const int D = sp->L.D, row = POTUS_N_SAMPLER_COLS + D, nsel = col_end - col_begin;
  std::vector<double> blk((size_t)n * row, NAN);   // the sampler columns of these rows are NaN
  for (int i = 0; i < n; i++) std::copy(q + (size_t)i * D, q + (size_t)(i + 1) * D, blk.begin() + (size_t)i * row + POTUS_N_SAMPLER_COLS);
  DevBufs tmp;
  double *dblk = nullptr;
  HIP_TRY(tmp.alloc(&dblk, blk.size() * 8));
  HIP_TRY(hipMemcpyAsync(dblk, blk.data(), blk.size() * 8, hipMemcpyHostToDevice, sp->stream));
  WAParams W{RowSrc{dblk, 1, n, row, 0}, n, sp->L.ncols, col_begin, col_end, nullptr, nullptr, nsel};   // n draws of one chain
  if (const int rc_ = launch_rows(sp, tmp, nullptr, sp->dM, 0, W)) return rc_;
  HIP_TRY(hipMemcpyAsync(out, W.out, (size_t)n * nsel * 8, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

int potus_sbc_ranks(int handle, const double *truth, int col_begin, int col_end, int thin, int32_t *less, int32_t *equal, int *L) {
  Sampler *sp = get(handle);
  if (!sp) return fail(POTUS_ERR_STATE, "bad handle");
  if (const int rc_ = refuse_own_models(sp, "potus_sbc_ranks")) return rc_;
  if (!truth || !less || !equal || !L) return fail(POTUS_ERR_ARG, "potus_sbc_ranks: null argument");
  if (col_begin < POTUS_N_SAMPLER_COLS || col_end > sp->L.ncols || col_begin >= col_end)
    return fail(POTUS_ERR_ARG, "potus_sbc_ranks: bad column range [%d,%d) (columns %d .. %d)", col_begin, col_end, POTUS_N_SAMPLER_COLS, sp->L.ncols);
  if (thin < 1) return fail(POTUS_ERR_ARG, "potus_sbc_ranks: thin = %d, at least 1", thin);
  DeviceLocks lock(sp->device);
  HIP_TRY(hipSetDevice(sp->device));
  DsPlan pl;
  if (const int rc = ds_plan("potus_sbc_ranks", sp, pl)) return rc;
  const int nL = (pl.n_post + thin - 1) / thin, chains = sp->R.chains, n_ds = pl.n_ds, cpd = pl.cpd, nsel = col_end - col_begin;
  const int grid = std::min(chains, 1024);
  DevBufs tmp;
  double *dtruth = nullptr, *scratch = nullptr;
  int *dskip = nullptr, *cl = nullptr, *ce = nullptr, *dl = nullptr, *de = nullptr;
  HIP_TRY(tmp.alloc(&dtruth, (size_t)n_ds * nsel * 8)); HIP_TRY(tmp.alloc(&scratch, (size_t)grid * sp->L.ncols * 8)); HIP_TRY(tmp.alloc(&dskip, (size_t)chains * 4));
  HIP_TRY(tmp.alloc(&cl, (size_t)chains * nsel * 4)); HIP_TRY(tmp.alloc(&ce, (size_t)chains * nsel * 4));
  HIP_TRY(tmp.alloc(&dl, (size_t)n_ds * nsel * 4)); HIP_TRY(tmp.alloc(&de, (size_t)n_ds * nsel * 4));
  HIP_TRY(hipMemcpyAsync(dtruth, truth, (size_t)n_ds * nsel * 8, hipMemcpyHostToDevice, sp->stream));
  HIP_TRY(hipMemcpyAsync(dskip, pl.failed.data(), (size_t)chains * 4, hipMemcpyHostToDevice, sp->stream));   // per chain: what k_sbc_ranks takes
  RankParams P{row_src(sp, pl.first), sp->L.ncols, col_begin, col_end, thin, nL, cpd, dtruth, dskip, scratch, cl, ce};
  hipLaunchKernelGGL(k_sbc_ranks, dim3(grid), dim3(256), 0, sp->stream, (const DevModel *)sp->dM, P);
  HIP_TRY(hipGetLastError());
  const int rgrid = (int)std::min<long long>(((long long)n_ds * nsel + 255) / 256, 1024);
  hipLaunchKernelGGL(k_sbc_reduce, dim3(rgrid), dim3(256), 0, sp->stream, (const int *)cl, (const int *)ce, n_ds, cpd, nsel, dl, de);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(less, dl, (size_t)n_ds * nsel * 4, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipMemcpyAsync(equal, de, (size_t)n_ds * nsel * 4, hipMemcpyDeviceToHost, sp->stream));
  HIP_TRY(hipStreamSynchronize(sp->stream));
  *L = nL * cpd;
  return 0;
}

// Development aid (POTUS_PROF builds only; not part of include/potus_hmc.h): per-chain cycle
// counters of the kernel phases.  Returns the number of slots written per chain, 0 otherwise.
int potus_debug_profile(int handle, double *out) {
  Sampler *sp = get(handle);
  if (!sp || !sp->R.prof || !out) return 0;
  (void)hipSetDevice(sp->device);
  if (hipMemcpy(out, sp->R.prof, sizeof(double) * PT_NPROF * sp->R.chains * sp->K * sp->sides(), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return PT_NPROF;
}

// What the last cluster launch found about its placement, per chain and side: 1 = the cluster's members on one XCD (exchange words published with plain stores).
int potus_debug_xcd_local(int handle, int *out) {
  Sampler *sp = get(handle);
  if (!sp || !out || sp->K <= 1) return -1;
  (void)hipSetDevice(sp->device);
  const int blocks = sp->R.chains * sp->sides();
  std::vector<ChainScalars> all((size_t)blocks * sp->K);
  if (hipMemcpy(all.data(), sp->R.scal, sizeof(ChainScalars) * all.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  for (int b = 0; b < blocks; b++) out[b] = all[(size_t)b * sp->K].xcd_local;
  return blocks;
}

// Which build of the cluster pass a handle runs (template tag of potus_cluster.hpp: 4, 8, 12, 16, 17), 0 for one workgroup per chain.
int potus_debug_build_tag(int handle) {
  Sampler *sp = get(handle);
  return sp ? (sp->K > 1 ? sp->cl_dw : 0) : -1;
}

// The per-poll scalar arithmetic on caller data (tests/test_gpu_poll_terms.py): one thread per item calls loo_poll_ll, one thread per draw
// calls binomial_logit_draw with key chain field item + 1 and the draw number as the counter index.  Nothing else runs in these kernels.
namespace {
__global__ __launch_bounds__(256) void k_poll_ll_probe(int n_items, const double *y, const double *n, const double *eta, const double *sigma, const double *z,
                                                       int integrate, double *out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_items) out[i] = loo_poll_ll(y[i], n[i], eta[i], sigma[i], z[i], integrate);
}
__global__ __launch_bounds__(256) void k_binomial_draw_probe(unsigned seed_lo, unsigned seed_hi, int n_items, const int *n, const double *eta, int draws, int *out) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= (long long)n_items * draws) return;
  const int item = (int)(j / draws), d = (int)(j % draws);
  const RngKey key{seed_lo, seed_hi, (uint32_t)(item + 1)};
  out[j] = binomial_logit_draw(key, (uint32_t)d, n[item], eta[item]);
}
}

int potus_poll_ll_probe(int device, int n_items, const double *y, const double *n, const double *eta, const double *sigma, const double *z, int integrate,
                        double *out) {
  if (n_items < 1 || !y || !n || !eta || !sigma || !z || !out) return fail(POTUS_ERR_ARG, "potus_poll_ll_probe: bad arguments");
  HIP_TRY(hipSetDevice(device));
  DevBufs bufs;
  const size_t nb = (size_t)n_items * 8;
  double *d[6];
  const double *src[5] = {y, n, eta, sigma, z};
  for (int k = 0; k < 6; k++) HIP_TRY(bufs.alloc(&d[k], nb));
  for (int k = 0; k < 5; k++) HIP_TRY(hipMemcpy(d[k], src[k], nb, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_poll_ll_probe, dim3((n_items + 255) / 256), dim3(256), 0, 0, n_items, d[0], d[1], d[2], d[3], d[4], integrate, d[5]);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d[5], nb, hipMemcpyDeviceToHost));
  return 0;
}

int potus_binomial_draw_probe(int device, unsigned long long seed, int n_items, const int *n, const double *eta, int draws_per_item, int *out) {
  if (n_items < 1 || draws_per_item < 1 || !n || !eta || !out || (long long)n_items * draws_per_item > (1LL << 28))
    return fail(POTUS_ERR_ARG, "potus_binomial_draw_probe: bad arguments");
  HIP_TRY(hipSetDevice(device));
  DevBufs bufs;
  const size_t total = (size_t)n_items * draws_per_item;
  int *dn, *dout;
  double *deta;
  HIP_TRY(bufs.alloc(&dn, (size_t)n_items * 4)); HIP_TRY(bufs.alloc(&deta, (size_t)n_items * 8)); HIP_TRY(bufs.alloc(&dout, total * 4));
  HIP_TRY(hipMemcpy(dn, n, (size_t)n_items * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(deta, eta, (size_t)n_items * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_binomial_draw_probe, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, (unsigned)(seed & 0xFFFFFFFFu), (unsigned)(seed >> 32), n_items,
                     (const int *)dn, (const double *)deta, draws_per_item, dout);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, dout, total * 4, hipMemcpyDeviceToHost));
  return 0;
}

// Development entry points (not in include/potus_hmc.h) that run single pieces of the dense-metric path on caller data,
// so that each can be checked against numpy and timed on its own (tests/test_gpu_dense.py, scripts/micro/dense_probe.py).
namespace {
struct DenseProbe {   // a DnParams with every chain active, owned buffers
  DnParams P{};
  DevBufs bufs;
  int init(int device, int chains, int D, int win_cap, bool pooled = false) {
    HIP_TRY(hipSetDevice(device));
    P.chains = chains; P.D = D; P.LD = (D + 7) & ~7; P.npart = (D + DN_FIN / 4 - 1) / (DN_FIN / 4); P.nblk = (D + DN_RB - 1) / DN_RB; P.sc_stride = 1; P.win_cap = win_cap; P.identity = 0;
    P.pooled = pooled ? 1 : 0;
    const size_t mat = (size_t)(pooled ? 1 : chains) * D * P.LD * 8;
    HIP_TRY(bufs.alloc(&P.state, (size_t)chains * DV_COUNT * P.LD * 8)); HIP_TRY(bufs.alloc(&P.A, mat)); HIP_TRY(bufs.alloc(&P.dg, (size_t)chains * P.LD * 8));
    P.pool_split = 1; P.pool_rows = D;
    // development: POTUS_PROBE_F32 = 1 -- every piece with metric_storage = f32 (per chain: the floats in the rows' free halves, dn_f32_row; pooled: A32)
    P.f32 = getenv("POTUS_PROBE_F32") && atoi(getenv("POTUS_PROBE_F32")) ? 1 : 0;
    if (pooled) {   // (as dense_alloc)
      const int panels = (D + DNP_COLS_OF(P.f32) - 1) / DNP_COLS_OF(P.f32);
      int s = std::max(1, std::min(DNP_SPLIT_MAX, (2 * 256) / panels));   // at most two workgroups per compute unit, all resident at once (measured: profiles/r06_dense_pooled.txt)
      if (const char *e = getenv("POTUS_POOL_SPLIT")) s = std::max(1, std::min(DNP_SPLIT_MAX, atoi(e)));
      P.pool_rows = (((D + s - 1) / s + DNP_KB - 1) / DNP_KB) * DNP_KB;
      P.pool_split = (D + P.pool_rows - 1) / P.pool_rows;
      HIP_TRY(bufs.alloc(&P.Lf, mat)); HIP_TRY(hipMemset(P.Lf, 0, mat));
      HIP_TRY(bufs.alloc(&P.ypool, (size_t)P.pool_split * DNP_RMAX * P.LD * 8)); HIP_TRY(bufs.alloc(&P.pmean, (size_t)P.LD * 8));
      if (P.f32) { HIP_TRY(bufs.alloc(&P.A32, mat / 2)); HIP_TRY(hipMemset(P.A32, 0, mat / 2)); }
      for (const void *f : {reinterpret_cast<const void *>(k_dn_pool_mm<1>), reinterpret_cast<const void *>(k_dn_pool_mm<2>), reinterpret_cast<const void *>(k_dn_pool_mm<3>),
                            reinterpret_cast<const void *>(k_dn_pool_mm<1, true>), reinterpret_cast<const void *>(k_dn_pool_mm<2, true>), reinterpret_cast<const void *>(k_dn_pool_mm<3, true>)})
        HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DNP_LDS(3)));
    }
    dense_launch_shape(P, chains);
    HIP_TRY(bufs.alloc(&P.tpart, (size_t)chains * P.nblk * 3 * P.LD * 8)); HIP_TRY(bufs.alloc(&P.srow, (size_t)chains * 3 * P.ntile * P.LD * 8));
    HIP_TRY(bufs.alloc(&P.win, (size_t)chains * std::max(win_cap, 1) * P.LD * 8)); HIP_TRY(bufs.alloc(&P.partial, (size_t)chains * P.npart * 8));
    HIP_TRY(bufs.alloc(&P.lpbuf, (size_t)chains * 8)); HIP_TRY(bufs.alloc(&P.ts, (size_t)chains * sizeof(TS)));
    HIP_TRY(bufs.alloc(&P.rd, (size_t)chains * sizeof(DnRound))); HIP_TRY(bufs.alloc(&P.active, (size_t)chains * 4)); HIP_TRY(bufs.alloc(&P.fail, 4));
    HIP_TRY(hipMemset(P.state, 0, (size_t)chains * DV_COUNT * P.LD * 8)); HIP_TRY(hipMemset(P.A, 0, mat)); HIP_TRY(hipMemset(P.dg, 0, (size_t)chains * P.LD * 8));
    HIP_TRY(hipMemset(P.fail, 0, 4));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dn_symv<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DN_SYMV_LDS(1)));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dn_symv<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DN_SYMV_LDS(2)));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dn_symv<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DN_SYMV_LDS(1)));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dn_symv<2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DN_SYMV_LDS(2)));
    return 0;
  }
  int set_rounds(const std::vector<DnRound> &r) { HIP_TRY(hipMemcpy(P.rd, r.data(), r.size() * sizeof(DnRound), hipMemcpyHostToDevice)); return 0; }
};
}

// y_r = M^-1 x_r (r < nrhs <= 3) for `chains` dense inverse metrics of size D x D (symmetric; the device keeps the strict
// upper triangle and the diagonal).  Minv_host == NULL: the matrices are generated on the device (k_dn_fill) -- for rates
// at sizes whose matrices would take seconds to upload.  Runs the product `reps` times; x_host / y_host are
// [chains][nrhs][D]; dot_host [chains] receives x_0 . M^-1 x_0; *ms the average time of a pass (HIP events); *pass_bytes
// the bytes of matrix one pass loads per chain.  POTUS_PROBE_F32 = 1: metric_storage = f32 -- the caller's matrix is rounded to fp32 on the way in
// (upper triangle as floats in the rows' free halves, the diagonal vector as doubles) and k_dn_symv<NRHS, true> runs.
static int dense_matvec_probe_impl(bool pooled, int device, int chains, int D, int nrhs, const double *Minv_host, const double *x_host, double *y_host, double *dot_host, int reps,
                                   double *ms, long long *pass_bytes) {
  if (chains < 1 || D < 1 || nrhs < 1 || nrhs > 3 || !x_host || !y_host || reps < 1) return fail(POTUS_ERR_ARG, "potus_dense_matvec_probe: bad arguments");
  DenseProbe pr;
  int rc = pr.init(device, chains, D, 1, pooled);
  if (rc) return rc;
  DnParams &P = pr.P;
  if (pooled) {   // ONE full symmetric matrix for every chain (generated: chain 0's of k_dn_fill, mirrored)
    if (Minv_host) {
      HIP_TRY(hipMemcpy2D(P.A, (size_t)P.LD * 8, Minv_host, (size_t)D * 8, (size_t)D * 8, (size_t)D, hipMemcpyHostToDevice));
      if (P.f32) hipLaunchKernelGGL(k_dn_pool_round32, dim3(4096), dim3(256), 0, 0, P);
    } else hipLaunchKernelGGL(k_dn_pool_fill, dim3(4096), dim3(256), 0, 0, P);
  } else if (Minv_host) {
    std::vector<double> dg((size_t)chains * P.LD, 0.0);
    if (P.f32) {
      // fp32 storage as the sampler keeps it: row i holds the caller's lower triangle as doubles [0, i] (not the metric's: the factor's place) and
      // element (i, j), j > i, rounded to fp32 in its free half (dn_f32_row); the diagonal vector holds the rounded values as doubles
      std::vector<double> rows((size_t)D * P.LD);
      for (int c = 0; c < chains; c++) {
        std::fill(rows.begin(), rows.end(), 0.0);
        const double *Mc = Minv_host + (size_t)c * D * D;
        for (int i = 0; i < D; i++) {
          for (int j = 0; j <= i; j++) rows[(size_t)i * P.LD + j] = Mc[(size_t)i * D + j];
          float *f = dn_f32_row(rows.data(), P.LD, i);
          for (int j = i + 1; j < D; j++) f[j] = (float)Mc[(size_t)i * D + j];
          dg[(size_t)c * P.LD + i] = (double)(float)Mc[(size_t)i * D + i];
        }
        HIP_TRY(hipMemcpy(P.A + (size_t)c * D * P.LD, rows.data(), rows.size() * 8, hipMemcpyHostToDevice));
      }
    } else {
      HIP_TRY(hipMemcpy2D(P.A, (size_t)P.LD * 8, Minv_host, (size_t)D * 8, (size_t)D * 8, (size_t)chains * D, hipMemcpyHostToDevice));   // the lower half is ignored
      for (int c = 0; c < chains; c++) for (int i = 0; i < D; i++) dg[(size_t)c * P.LD + i] = Minv_host[((size_t)c * D + i) * D + i];
    }
    HIP_TRY(hipMemcpy(P.dg, dg.data(), dg.size() * 8, hipMemcpyHostToDevice));
  } else hipLaunchKernelGGL(k_dn_fill, dim3(4096), dim3(256), 0, 0, P);   // (POTUS_PROBE_F32 = 1: the floats of the generated matrix)
  std::vector<DnRound> rds(chains);
  // development: a launch with idle companions (POTUS_PROBE_ACTIVE = n: the first n chains take part; or a list "2,7,11")
  std::vector<int> act_flag(chains, 1);
  int n_act = chains;
  if (const char *e = getenv("POTUS_PROBE_ACTIVE")) {
    std::fill(act_flag.begin(), act_flag.end(), 0);
    if (strchr(e, ',')) { for (const char *q = e; q && *q; q = strchr(q, ',') ? strchr(q, ',') + 1 : nullptr) { const int c = atoi(q); if (c >= 0 && c < chains) act_flag[c] = 1; } }
    else for (int c = 0; c < std::min(chains, std::max(1, atoi(e))); c++) act_flag[c] = 1;
    n_act = (int)std::count(act_flag.begin(), act_flag.end(), 1);
  }
  dense_launch_shape(P, n_act);
  for (int c = 0; c < chains; c++) {
    DnRound &r = rds[c];
    std::memset(&r, 0, sizeof r);
    r.active = act_flag[c];
    for (int k = 0; k < 3; k++) r.job[k] = DnJob{DV_POOLP + k, DV_POOLPS + k, -1, -1, k == 0 ? DV_POOLP : -1, 0, 0.0};
    for (int k = 0; k < nrhs; k++)
      HIP_TRY(hipMemcpy(P.state + ((size_t)c * DV_COUNT + DV_POOLP + k) * P.LD, x_host + ((size_t)c * nrhs + k) * D, (size_t)D * 8, hipMemcpyHostToDevice));
  }
  if ((rc = pr.set_rounds(rds))) return rc;
  EventTimer e;
  HIP_TRY(e.made);
  DnActive act;
  act.n = 0;
  if (n_act < chains && chains <= DN_ACT_MAX && !getenv("POTUS_PROBE_NO_COMPACTION")) for (int c = 0; c < chains; c++) if (act_flag[c]) act.idx[act.n++] = c;
  dense_symv_launch(0, P, act, nrhs);   // warm-up
  (void)e.start(0);
  for (int r = 0; r < reps; r++) dense_symv_launch(0, P, act, nrhs);
  (void)e.stop(0);
  const bool ok = hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
  double t = 0; (void)e.elapsed(&t);
  if (!ok) return fail(POTUS_ERR_DEVICE, "k_dn_symv failed");
  if (ms) *ms = t / reps;
  if (pass_bytes) *pass_bytes = pooled ? (long long)D * P.LD * (P.f32 ? 4 : 8) * ((n_act * nrhs + DNP_RMAX - 1) / DNP_RMAX)
                                       : dense_pass_bytes(D, P.LD, P.rb) * (nrhs == 3 ? 2 : 1) / (P.f32 ? 2 : 1);
  for (int c = 0; c < chains; c++) {
    for (int k = 0; k < nrhs; k++)
      HIP_TRY(hipMemcpy(y_host + ((size_t)c * nrhs + k) * D, P.state + ((size_t)c * DV_COUNT + DV_POOLPS + k) * P.LD, (size_t)D * 8, hipMemcpyDeviceToHost));
    if (dot_host) {
      std::vector<double> part(P.npart);
      HIP_TRY(hipMemcpy(part.data(), P.partial + (size_t)c * P.npart, (size_t)P.npart * 8, hipMemcpyDeviceToHost));
      double t2 = 0; for (double v : part) t2 += v;
      dot_host[c] = t2;
    }
  }
  return 0;
}

int potus_dense_matvec_probe(int device, int chains, int D, int nrhs, const double *Minv_host, const double *x_host, double *y_host, double *dot_host, int reps,
                             double *ms, long long *pass_bytes) {
  return dense_matvec_probe_impl(false, device, chains, D, nrhs, Minv_host, x_host, y_host, dot_host, reps, ms, pass_bytes);
}
// the same for the POOLED metric (potus_opts.pooled_metric): ONE D x D matrix Minv_host for all chains (NULL: generated), every right-hand side of every
// chain in one pass (k_dn_pool_mm); *pass_bytes = the whole matrix per pass
int potus_dense_pool_matvec_probe(int device, int chains, int D, int nrhs, const double *Minv_host, const double *x_host, double *y_host, double *dot_host, int reps,
                                  double *ms, long long *pass_bytes) {
  return dense_matvec_probe_impl(true, device, chains, D, nrhs, Minv_host, x_host, y_host, dot_host, reps, ms, pass_bytes);
}

// covar_adaptation on caller data: draws [chains][n][D] -> M^-1 (covariance of the window, regularised), its lower
// Cholesky factor (in place, in the lower triangle of the same matrix), and p = L^-T u for u [chains][D] (the momentum
// draw's triangular solve).  Outputs [chains][D][D] (M^-1 rebuilt from the upper triangle and the diagonal vector; L the
// lower triangle, zeros above) / [chains][D]; ms[3] = covariance, factorisation, solve (milliseconds).
// POTUS_PROBE_F32 = 1: metric_storage = f32 -- M^-1 comes back from the floats in the rows' free halves (dn_f32_row), read AFTER the factorisation.
static int dense_factor_probe_impl(bool pooled, int device, int chains, int D, int n, const double *draws_host, const double *u_host, double *Minv_host, double *L_host,
                                   double *p_host, double *ms) {
  if (chains < 1 || D < 1 || n < 2 || !draws_host) return fail(POTUS_ERR_ARG, "potus_dense_factor_probe: bad arguments");
  DenseProbe pr;
  int rc = pr.init(device, chains, D, n, pooled);
  if (rc) return rc;
  DnParams &P = pr.P;
  HIP_TRY(hipMemcpy2D(P.win, (size_t)P.LD * 8, draws_host, (size_t)D * 8, (size_t)D * 8, (size_t)chains * n, hipMemcpyHostToDevice));
  std::vector<DnRound> rds(chains);
  for (auto &r : rds) { std::memset(&r, 0, sizeof r); r.active = 1; }
  if ((rc = pr.set_rounds(rds))) return rc;
  hipEvent_t ev[4];
  for (auto &e : ev) HIP_TRY(hipEventCreate(&e));
  const int nb = (D + DN_NB - 1) / DN_NB;
  const dim3 eg((unsigned)std::min((D + 255) / 256, 64), (unsigned)chains);
  (void)hipEventRecord(ev[0], 0);
  if (pooled) {
    hipLaunchKernelGGL(k_dn_pool_center, dim3(eg.x), dim3(256), 0, 0, P, n);
    hipLaunchKernelGGL(k_dn_pool_cov, dim3(nb, nb), dim3(256), 0, 0, P, n);
    hipLaunchKernelGGL(k_dn_pool_scale, dim3(eg.x, (unsigned)D), dim3(256), 0, 0, P, (double)chains * (double)n);
  } else {
    hipLaunchKernelGGL(k_dn_center, eg, dim3(256), 0, 0, P, n);
    hipLaunchKernelGGL(k_dn_cov, dim3(nb, nb, chains), dim3(256), 0, 0, P, n);
  }
  (void)hipEventRecord(ev[1], 0);
  dense_cholesky_launch(0, P, pooled ? 1 : chains);
  (void)hipEventRecord(ev[2], 0);
  if (u_host && p_host) {
    for (int c = 0; c < chains; c++) HIP_TRY(hipMemcpy(P.state + ((size_t)c * DV_COUNT + DV_P0) * P.LD, u_host + (size_t)c * D, (size_t)D * 8, hipMemcpyHostToDevice));
    for (int b = nb - 1; b >= 0; b--) {
      hipLaunchKernelGGL(k_dn_trsv_diag, dim3(chains), dim3(64), 0, 0, P, b);
      if (b > 0) hipLaunchKernelGGL(k_dn_trsv_update, dim3((b * DN_NB + 255) / 256, chains), dim3(256), 0, 0, P, b);
    }
  }
  (void)hipEventRecord(ev[3], 0);
  const bool ok = hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
  if (ms) for (int k = 0; k < 3; k++) { float t = 0; (void)hipEventElapsedTime(&t, ev[k], ev[k + 1]); ms[k] = t; }
  for (auto &e : ev) (void)hipEventDestroy(e);
  if (!ok) return fail(POTUS_ERR_DEVICE, "dense factor kernels failed");
  int failed = 0;
  HIP_TRY(hipMemcpy(&failed, P.fail, 4, hipMemcpyDeviceToHost));
  if (failed) return fail(POTUS_ERR_STATE, "covariance not positive definite");
  if (Minv_host || L_host) {
    std::vector<double> buf((size_t)D * D), dg(D), lbuf, rows;
    const bool halves = !pooled && P.f32;               // per chain with fp32 storage: the metric above the diagonal is the floats in the rows' free halves
    for (int c = 0; c < (pooled ? 1 : chains); c++) {   // (pooled: ONE matrix and ONE factor come back)
      HIP_TRY(hipMemcpy2D(buf.data(), (size_t)D * 8, dn_mat(P, c), (size_t)P.LD * 8, (size_t)D * 8, (size_t)D, hipMemcpyDeviceToHost));
      if (halves) { rows.resize((size_t)D * P.LD); HIP_TRY(hipMemcpy(rows.data(), dn_mat(P, c), rows.size() * 8, hipMemcpyDeviceToHost)); }
      auto upper = [&](size_t i, size_t j) { return halves ? (double)dn_f32_row(rows.data(), P.LD, (int)i)[j] : buf[i * D + j]; };   // i < j
      HIP_TRY(hipMemcpy(dg.data(), dn_diag(P, c), (size_t)D * 8, hipMemcpyDeviceToHost));
      if (pooled) { lbuf.resize((size_t)D * D); HIP_TRY(hipMemcpy2D(lbuf.data(), (size_t)D * 8, P.Lf, (size_t)P.LD * 8, (size_t)D * 8, (size_t)D, hipMemcpyDeviceToHost)); }
      const std::vector<double> &lb = pooled ? lbuf : buf;
      for (size_t i = 0; i < (size_t)D; i++)
        for (size_t j = 0; j < (size_t)D; j++) {
          if (Minv_host) Minv_host[((size_t)c * D + i) * D + j] = pooled ? buf[i * D + j] : (i == j ? dg[i] : (i < j ? upper(i, j) : upper(j, i)));
          if (L_host) L_host[((size_t)c * D + i) * D + j] = j <= i ? lb[i * D + j] : 0.0;
        }
    }
  }
  if (u_host && p_host)
    for (int c = 0; c < chains; c++) HIP_TRY(hipMemcpy(p_host + (size_t)c * D, P.state + ((size_t)c * DV_COUNT + DV_P0) * P.LD, (size_t)D * 8, hipMemcpyDeviceToHost));
  return 0;
}
int potus_dense_factor_probe(int device, int chains, int D, int n, const double *draws_host, const double *u_host, double *Minv_host, double *L_host,
                             double *p_host, double *ms) {
  return dense_factor_probe_impl(false, device, chains, D, n, draws_host, u_host, Minv_host, L_host, p_host, ms);
}
// the POOLED window end: ONE regularised covariance of all chains x n draws -> Minv_host [D][D] (as the device holds it: the full symmetric matrix),
// ONE factor L_host [D][D], and p = L^-T u for every chain's u
int potus_dense_pool_factor_probe(int device, int chains, int D, int n, const double *draws_host, const double *u_host, double *Minv_host, double *L_host,
                                  double *p_host, double *ms) {
  return dense_factor_probe_impl(true, device, chains, D, n, draws_host, u_host, Minv_host, L_host, p_host, ms);
}

// Development aid: the whole state block [chains][V_COUNT][Dpad] (internal element order) and every replica of the
// chain scalars as raw bytes.  which = 0: sizes only (out[0] = V_COUNT, out[1] = Dpad, out[2] = sizeof scalars * replicas).
int potus_debug_state(int handle, int which, double *out, unsigned char *scal) {
  Sampler *sp = get(handle);
  if (!sp || !out) return 0;
  (void)hipSetDevice(sp->device);
  const size_t nblk = (size_t)sp->R.chains * sp->sides();   // (two clusters / workgroups per chain: side 1's blocks follow side 0's)
  if (which == 0) { out[0] = V_COUNT; out[1] = sp->R.Dpad; out[2] = (double)(sizeof(ChainScalars) * nblk * sp->K); return 1; }
  if (hipMemcpy(out, sp->R.state, sizeof(double) * V_COUNT * sp->R.Dpad * nblk, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  if (scal && hipMemcpy(scal, sp->R.scal, sizeof(ChainScalars) * nblk * sp->K, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return 1;
}

// ---------------------------------------------------------------------------------------------- E_loo on a fit's handles (potus_eloo.hpp)
// Pools as potus_loo pools: the polls in blocks whose temporaries stay within LOO_BLOCK_BUDGET, every handle's block made on its own GPU and
// brought to the first handle's (gather_block).  Per block: log-likelihoods -> potus_loo's k-hat and r_eff (loo_psis) -> ratios -> under no
// lock of its own the device forms (potus_psis_device, potus_e_loo_shared_device / potus_e_loo_device take the device's lock themselves).
// The scores (k_tl_scores) and the log-likelihoods (k_loo_loglik) both walk a handle's draws chain after chain, iterations within, and the
// handles are placed at their chain offset in the order listed: column s of X and weight s of a poll are the same draw.
int potus_e_loo(const int *handles, int n_handles, int integrate, int what, const double *ev, int ev_to_win, int day, int day_begin, int day_end, int diag,
                double *out, double *var_out, double *post_out, double *pareto_k_out, double *ess_out, double *khat_out, double *days_out, double *days_post_out) {
  const char *nm = "potus_e_loo";
  if (!out || !pareto_k_out) return fail(POTUS_ERR_ARG, "%s: null output", nm);
  if (what != POTUS_ELOO_PREDICT && what != POTUS_ELOO_INFLUENCE) return fail(POTUS_ERR_ARG, "%s: what = %d (0: predict, 1: influence)", nm, what);
  if (integrate != 0 && integrate != 1) return fail(POTUS_ERR_ARG, "%s: integrate = %d (0: plain, 1: noise coordinate integrated out)", nm, integrate);
  if (diag != 0 && diag != 1) return fail(POTUS_ERR_ARG, "%s: diag = %d", nm, diag);
  Pool P;
  if (const int rc_ = P.resolve(handles, n_handles, nm)) return rc_;
  if (const int rc_ = P.same_posterior("E_loo pools the chains of one")) return rc_;
  const std::vector<Sampler *> &sps = P.sps;
  Sampler *s0 = P.s0;
  const int Np = s0->M.Npoll, S = s0->M.S, T = s0->M.T;
  if (Np < 1) return fail(POTUS_ERR_ARG, "%s: the data hold no polls", nm);
  const bool infl = what == POTUS_ELOO_INFLUENCE;
  const int t = day < 0 ? T - 1 : day, nday = infl && day_end > day_begin ? day_end - day_begin : 0, NC = 2 * S + 3;
  std::vector<TlPlan> plans(sps.size());
  if (infl) {
    if (!ev || !var_out || !post_out || !ess_out || (diag && !khat_out)) return fail(POTUS_ERR_ARG, "%s: influence needs ev and the outputs var, post, ess (and khat with diag)", nm);
    if (nday && (!days_out || !days_post_out)) return fail(POTUS_ERR_ARG, "%s: a day range without its outputs", nm);
    for (size_t i = 0; i < sps.size(); i++) {
      if (const int rc_ = tl_check_args(nm, sps[i], t, t + 1, plans[i])) return rc_;
      if (nday) if (const int rc_ = tl_check_args(nm, sps[i], day_begin, day_end, plans[i])) return rc_;
    }
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  DevBufs keep;
  double *cols = nullptr, *rr = nullptr, *lw = nullptr, *b1 = nullptr, *b2 = nullptr, *X = nullptr, *Xd = nullptr, *cm = nullptr;
  int Ctot = 0, n_post = 0, first = 0, nb = 0;
  long long Stot = 0;
  std::vector<LooRows> rows(sps.size());
  {
    DeviceGuard guard;
    DeviceLocks lock(P.devs);
    if (const int rc_ = P.count()) return rc_;
    if (const int rc_ = P.equal_counts()) return rc_;
    Ctot = P.chains;
    if (2 * Ctot > DG_MAXCH) return fail(POTUS_ERR_UNSUPPORTED, "%s: %d chains pooled (at most %d)", nm, Ctot, DG_MAXCH / 2);
    if (const int rc_ = P.post_warmup(&first, &n_post)) return rc_;
    Stot = (long long)n_post * Ctot;
    if (const int rc_ = el_check_sizes(nm, Ctot, n_post)) return rc_;
    int rc;
    for (size_t i = 0; i < sps.size(); i++)
      if ((rc = loo_rows_setup(sps[i], (long long)n_post * sps[i]->R.chains, keep, rows[i], nm))) return rc;
    nb = loo_block_polls((size_t)Stot * 8 * (infl ? 4 : 6), Np);
    if (const char *e = getenv("POTUS_ELOO_BLOCK_POLLS")) nb = std::max(1, std::min(nb, atoi(e)));   // (tests: several blocks on a small fit)
    HIP_TRY(hipSetDevice(s0->device));
    if ((rc = keep.get(&cols, (size_t)Stot * nb * 8, nm)) || (rc = keep.get(&rr, (size_t)Stot * nb * 8, nm)) || (rc = keep.get(&lw, (size_t)Stot * nb * 8, nm))) return rc;
    if (!infl && ((rc = keep.get(&b1, (size_t)Stot * nb * 8, nm)) || (rc = keep.get(&b2, (size_t)Stot * nb * 8, nm)) || (rc = keep.get(&cm, (size_t)nb * 8, nm)))) return rc;
    if (infl) {
      // ---- the forecast columns, shared by all polls
      const int ncd = nday * (S + 1);
      double *dw = nullptr, *dev_ev = nullptr;
      if ((rc = keep.get(&X, (size_t)NC * Stot * 8, nm)) || (rc = keep.get(&cm, (size_t)std::max(NC, ncd) * 8, nm)) || (rc = keep.get(&dw, (size_t)S * 8, nm)) ||
          (rc = keep.get(&dev_ev, (size_t)S * 8, nm)) || (nday && (rc = keep.get(&Xd, (size_t)ncd * Stot * 8, nm))))
        return rc;
      HIP_TRY(hipMemcpy(dw, s0->h_w.data(), (size_t)S * 8, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(dev_ev, ev, (size_t)S * 8, hipMemcpyHostToDevice));
      for (int pass = 0; pass < (nday ? 2 : 1); pass++) {
        const int d0 = pass ? day_begin : t, d1 = pass ? day_end : t + 1, nd = d1 - d0;
        long long off = 0;
        for (size_t i = 0; i < sps.size(); i++) {
          Sampler *sp = sps[i];
          const long long n_h = (long long)sp->R.chains * n_post;
          const size_t bytes = (size_t)n_h * nd * S * 8;
          DevBufs blkbuf;
          double *blk = nullptr;
          if ((rc = blkbuf.get(&blk, bytes, nm))) return rc;
          TlPlan &pl = plans[i];
          if ((rc = gather_block(s0, sp, bytes, blk, [&](double *o) {
                 if (const int r_ = ds_plan(nm, sp, pl)) return r_;
                 DevBufs tmp;
                 int *dskip = nullptr;
                 if (const int r_ = tmp.get(&dskip, 4, nm)) return r_;
                 const int zero = 0;
                 HIP_TRY(hipMemcpyAsync(dskip, &zero, 4, hipMemcpyHostToDevice, sp->stream));
                 if (const int r_ = tl_scores(sp, pl, d0, d1, dskip, o)) return r_;
                 HIP_TRY(hipStreamSynchronize(sp->stream));
                 return 0;
               }))) return rc;
          const ElColParams Q{blk, dw, dev_ev, pass ? Xd : X, n_h, Stot, off, nd, S, pass ? 0 : 1, (double)ev_to_win};
          hipLaunchKernelGGL(k_el_columns, dim3((unsigned)std::min<long long>((n_h * nd + 255) / 256, 65535)), dim3(256), 0, s0->stream, Q);
          HIP_TRY(hipGetLastError());
          HIP_TRY(hipStreamSynchronize(s0->stream));
          off += n_h;
        }
        const int nc = pass ? ncd : NC;
        hipLaunchKernelGGL(k_el_colmean, dim3(std::min(nc, 65535)), dim3(DG_THREADS), 0, s0->stream, (const double *)(pass ? Xd : X), cm, Stot, nc);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(pass ? days_post_out : post_out, cm, (size_t)nc * 8, hipMemcpyDeviceToHost, s0->stream));
        HIP_TRY(hipStreamSynchronize(s0->stream));
      }
    }
  }
  std::vector<double> pw((size_t)nb * LOO_NPW), re(nb), kk(nb), o3((size_t)nb * 3), k3((size_t)nb * EL_NK), e2(nb), ins(nb);
  for (int b0 = 0; b0 < Np; b0 += nb) {
    const int e1 = std::min(b0 + nb, Np), nbk = e1 - b0;
    {
      DeviceGuard guard;
      DeviceLocks lock(P.devs);
      int rc, coff = 0;
      HIP_TRY(hipSetDevice(s0->device));
      for (size_t i = 0; i < sps.size(); i++) {
        Sampler *sp = sps[i];
        const int C = sp->R.chains;
        const size_t bytes = (size_t)n_post * C * nbk * 8;
        DevBufs blkbuf;
        double *blk = nullptr, *blk2 = nullptr;
        if ((rc = blkbuf.get(&blk, bytes, nm))) return rc;
        if ((rc = gather_block(s0, sp, bytes, blk, [&](double *o) { return loo_loglik(sp, rows[i], first, n_post, b0, e1, integrate, o); }))) return rc;
        if ((rc = pool_transpose(s0, blk, cols, n_post, C, nbk, Ctot, coff))) return rc;
        if (!infl) {
          // (a1 and a2 come from one launch: both blocks are made on the handle's GPU, then brought over one after the other)
          HIP_TRY(hipSetDevice(sp->device));
          DevBufs far;
          double *f1 = nullptr, *f2 = nullptr;
          if ((rc = far.get(&f1, bytes, nm)) || (rc = far.get(&f2, bytes, nm))) return rc;
          ElShareParams Q{row_src(sp, first), sp->L.ncols, n_post, b0, e1, integrate, rows[i].scratch, f1, f2};
          hipLaunchKernelGGL(k_el_poll_share, dim3(rows[i].grid), dim3(256), 0, sp->stream, (const DevModel *)sp->dM, Q);
          HIP_TRY(hipGetLastError());
          HIP_TRY(hipStreamSynchronize(sp->stream));
          HIP_TRY(hipSetDevice(s0->device));
          const double *g1 = f1, *g2 = f2;
          if (sp->device != s0->device) {      // (on one device the transposes read the blocks where they are: a copy there is not ordered with s0's stream)
            if ((rc = blkbuf.get(&blk2, bytes, nm))) return rc;
            HIP_TRY(hipMemcpyPeer(blk, s0->device, f1, sp->device, bytes));
            HIP_TRY(hipMemcpyPeer(blk2, s0->device, f2, sp->device, bytes));
            HIP_TRY(hipDeviceSynchronize());
            g1 = blk; g2 = blk2;
          }
          if ((rc = pool_transpose(s0, g1, b1, n_post, C, nbk, Ctot, coff)) || (rc = pool_transpose(s0, g2, b2, n_post, C, nbk, Ctot, coff))) return rc;
        }
        coff += C;
      }
      if ((rc = loo_psis(s0->stream, cols, nbk, Ctot, n_post, nullptr, pw.data(), nm))) return rc;
      const MmRatioParams R{nullptr, cols, nullptr, nullptr, nullptr, rr, nullptr, n_post, (int)Stot, nbk, 0};
      hipLaunchKernelGGL(k_mm_ratio, dim3((unsigned)std::min<long long>(((long long)nbk * Stot + 255) / 256, 65535)), dim3(256), 0, s0->stream, R);
      HIP_TRY(hipGetLastError());
      if (!infl) {
        hipLaunchKernelGGL(k_el_colmean, dim3(std::min(nbk, 65535)), dim3(DG_THREADS), 0, s0->stream, (const double *)b1, cm, Stot, nbk);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(ins.data(), cm, (size_t)nbk * 8, hipMemcpyDeviceToHost, s0->stream));
      }
      HIP_TRY(hipStreamSynchronize(s0->stream));
    }
    for (int k = 0; k < nbk; k++) { pareto_k_out[b0 + k] = pw[(size_t)k * LOO_NPW + 3]; re[k] = pw[(size_t)k * LOO_NPW + 4]; }
    // a poll with identical log-likelihoods has no r_eff (NaN): any value gives its flat tail no fit
    for (int k = 0; k < nbk; k++) if (!(std::isfinite(re[k]) && re[k] > 0)) re[k] = 1.0;
    int rc;
    if (infl) {
      if ((rc = potus_psis_device(s0->device, rr, nbk, Ctot, n_post, re.data(), lw, kk.data()))) return rc;
      if ((rc = potus_e_loo_shared_device(s0->device, X, NC, lw, nbk, Ctot, n_post, rr, re.data(), diag, out + (size_t)b0 * NC, var_out + (size_t)b0 * NC, ess_out + b0,
                                          diag ? khat_out + (size_t)b0 * NC : kk.data())))
        return rc;
      for (int k = 0; k < 4; k++) acc[k] += g_el_ms[k];
      if (nday) {
        const int ncd = nday * (S + 1);
        std::vector<double> dvar((size_t)nbk * ncd);
        if ((rc = potus_e_loo_shared_device(s0->device, Xd, ncd, lw, nbk, Ctot, n_post, nullptr, nullptr, 0, days_out + (size_t)b0 * ncd, dvar.data(), e2.data(), nullptr))) return rc;
        for (int k = 0; k < 4; k++) acc[k] += g_el_ms[k];
      }
    } else {
      if ((rc = potus_e_loo_device(s0->device, b2, rr, nbk, Ctot, n_post, re.data(), nullptr, 0, o3.data(), k3.data()))) return rc;
      for (int k = 0; k < nbk; k++) e2[k] = o3[(size_t)k * 3];
      for (int k = 0; k < 4; k++) acc[k] += g_el_ms[k];
      if ((rc = potus_e_loo_device(s0->device, b1, rr, nbk, Ctot, n_post, re.data(), nullptr, 0, o3.data(), k3.data()))) return rc;
      for (int k = 0; k < 4; k++) acc[k] += g_el_ms[k];
      std::vector<double> nn((size_t)2 * s0->M.Npad);
      { DeviceGuard guard; HIP_TRY(hipSetDevice(s0->device)); HIP_TRY(hipMemcpy(nn.data(), s0->M.pd, nn.size() * 8, hipMemcpyDeviceToHost)); }
      std::vector<int> pi((size_t)6 * s0->M.Npad);
      { DeviceGuard guard; HIP_TRY(hipSetDevice(s0->device)); HIP_TRY(hipMemcpy(pi.data(), s0->M.pi, pi.size() * 4, hipMemcpyDeviceToHost)); }
      for (int i = 0; i < Np; i++) {          // the model's (day-sorted) poll i is poll k of the output numbering
        const int st = pi[i], qi = pi[(size_t)5 * s0->M.Npad + i], k = (st == S ? s0->M.Ns + (qi - s0->M.o_nn) : qi - s0->M.o_ns) - b0;
        if (k < 0 || k >= nbk) continue;
        const double n = nn[(size_t)s0->M.Npad + i], m1 = o3[(size_t)k * 3], var = m1 / n + (1.0 - 1.0 / n) * e2[k] - m1 * m1;
        double *o = out + (size_t)(b0 + k) * 5;
        o[0] = m1; o[1] = var; o[2] = std::sqrt(std::max(var, 0.0)); o[3] = k3[(size_t)k * EL_NK]; o[4] = ins[k];
      }
    }
  }
  std::copy(acc, acc + 4, g_el_ms);
  return 0;
}

// ---------------------------------------------------------------------------------------------- posterior predictive checks (potus_ppc.hpp)
namespace {
constexpr size_t PPC_BLOCK_BUDGET = 256ull << 20;   // the pooled per-poll blocks of one round of potus_ppc (POTUS_PPC_BLOCK_BUDGET, bytes: tests)
thread_local double g_ppc_ms[4] = {0.0, 0.0, 0.0, 0.0};   // the calling thread's last call: log-likelihood and PSIS, shares and replicate, PIT, groups

// y_rep of polls [b0, b1) of the handle's post-warm-up draws -> out [n_post][chains][b1 - b0], on the handle's device and stream
int ppc_rep(Sampler *sp, const LooRows &r, int first, int n_post, int b0, int b1, int integrate, int rep, double *out) {
  PpcRepParams P{row_src(sp, first), sp->L.ncols, n_post, b0, b1, integrate, rep, sp->R.chain_id_offset, sp->R.seed_lo, sp->R.seed_hi, r.scratch, out};
  hipLaunchKernelGGL(k_ppc_rep, dim3(r.grid), dim3(256), 0, sp->stream, (const DevModel *)sp->dM, P);
  HIP_TRY(hipGetLastError());
  return 0;
}

// lo, eq of NP polls (blocks on the current device, whose lock the caller holds) -> out [NP] rows of `stride` doubles on the host; ms += the kernel's time
int ppc_pit(hipStream_t st, const double *yrep, const double *y, const double *lw, int NP, long long S, double *out, int stride, double *ms, const char *what) {
  DevBufs tmp;
  double *dy = nullptr, *dout = nullptr;
  int rc;
  if ((rc = tmp.get(&dy, (size_t)NP * 8, what)) || (rc = tmp.get(&dout, (size_t)NP * 16, what))) return rc;
  HIP_TRY(hipMemcpyAsync(dy, y, (size_t)NP * 8, hipMemcpyHostToDevice, st));
  EventTimer t;
  HIP_TRY(t.made);
  HIP_TRY(t.start(st));
  hipLaunchKernelGGL(k_ppc_pit, dim3(std::min(NP, 65535)), dim3(DG_THREADS), 0, st, yrep, (const double *)dy, lw, dout, S, NP);
  if ((rc = el_span(t, st, ms, 2))) return rc;
  std::vector<double> h((size_t)NP * 2);
  HIP_TRY(hipMemcpy(h.data(), dout, h.size() * 8, hipMemcpyDeviceToHost));
  for (int k = 0; k < NP; k++) { out[(size_t)k * stride] = h[2 * k]; out[(size_t)k * stride + 1] = h[2 * k + 1]; }
  return 0;
}

// the polls of a block join their groups' sums: acc [G][3][2][S] on the current device, count [G] on the host (polls with n > 0 so far)
int ppc_groups_add(hipStream_t st, const double *yrep, const double *a1, const double *a2, const double *y, const double *n, const int32_t *labels, int G, int NP, long long S,
                   double *acc, long long *count, double *ms, const char *what) {
  std::vector<int> goff(G + 1, 0), gpoll;
  for (int k = 0; k < NP; k++) if (labels[k] >= 0 && n[k] > 0) goff[labels[k] + 1]++;
  for (int g = 0; g < G; g++) { count[g] += goff[g + 1]; goff[g + 1] += goff[g]; }
  gpoll.assign(std::max(goff[G], 1), 0);
  {
    std::vector<int> at(goff.begin(), goff.end() - 1);
    for (int k = 0; k < NP; k++) if (labels[k] >= 0 && n[k] > 0) gpoll[at[labels[k]]++] = k;   // ascending poll number within a group
  }
  if (goff[G] == 0) return 0;
  DevBufs tmp;
  double *dy = nullptr, *dn = nullptr;
  int *doff = nullptr, *dpoll = nullptr;
  int rc;
  if ((rc = tmp.get(&dy, (size_t)NP * 8, what)) || (rc = tmp.get(&dn, (size_t)NP * 8, what)) || (rc = tmp.get(&doff, goff.size() * 4, what)) ||
      (rc = tmp.get(&dpoll, gpoll.size() * 4, what)))
    return rc;
  HIP_TRY(hipMemcpyAsync(dy, y, (size_t)NP * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(dn, n, (size_t)NP * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(doff, goff.data(), goff.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(dpoll, gpoll.data(), gpoll.size() * 4, hipMemcpyHostToDevice, st));
  const PpcGroupParams P{yrep, a1, a2, dy, dn, doff, dpoll, acc, S, G};
  EventTimer t;
  HIP_TRY(t.made);
  HIP_TRY(t.start(st));
  hipLaunchKernelGGL(k_ppc_groups, dim3((unsigned)std::min<long long>(((long long)G * S + 255) / 256, 65535)), dim3(256), 0, st, P);
  return el_span(t, st, ms, 3);
}

// out [G][3][6] on the host from acc
int ppc_groups_finish(hipStream_t st, const double *acc, const long long *count, int G, long long S, double *out, double *ms, const char *what) {
  DevBufs tmp;
  long long *dc = nullptr;
  double *dout = nullptr;
  int rc;
  if ((rc = tmp.get(&dc, (size_t)G * 8, what)) || (rc = tmp.get(&dout, (size_t)G * PPC_NSTAT * PPC_NOUT * 8, what))) return rc;
  HIP_TRY(hipMemcpyAsync(dc, count, (size_t)G * 8, hipMemcpyHostToDevice, st));
  EventTimer t;
  HIP_TRY(t.made);
  HIP_TRY(t.start(st));
  hipLaunchKernelGGL(k_ppc_group_stats, dim3(std::min(G * PPC_NSTAT, 65535)), dim3(DG_THREADS), 0, st, acc, (const long long *)dc, dout, S, G);
  if ((rc = el_span(t, st, ms, 3))) return rc;
  HIP_TRY(hipMemcpy(out, dout, (size_t)G * PPC_NSTAT * PPC_NOUT * 8, hipMemcpyDeviceToHost));
  return 0;
}

int ppc_check_labels(const char *what, const int32_t *labels, long long N, int G, int grouping) {
  if (G < 1) return fail(POTUS_ERR_ARG, "%s: grouping %d has %d groups", what, grouping, G);
  for (long long k = 0; k < N; k++)
    if (labels[k] < -1 || labels[k] >= G) return fail(POTUS_ERR_ARG, "%s: poll %lld of grouping %d has label %d (-1: in no group, or 0 .. %d)", what, k, grouping, labels[k], G - 1);
  return 0;
}
int ppc_check_modes(const char *what, int integrate, int rep) {
  if (integrate != 0 && integrate != 1) return fail(POTUS_ERR_ARG, "%s: integrate = %d (0: the draw's noise coordinate, 1: a fresh one)", what, integrate);
  if (rep < 0 || rep > PPC_MAX_REP) return fail(POTUS_ERR_ARG, "%s: rep = %d (0 .. %d)", what, rep, PPC_MAX_REP);
  return 0;
}
} // namespace

int potus_ppc_timing(double *ms) {
  return timing_out("potus_ppc_timing", g_ppc_ms, 4, ms);
}

int potus_poll_rep_device(int handle, int poll_begin, int poll_end, int integrate, int rep, void *yrep_out_device) {
  const char *what = "potus_poll_rep_device";
  Sampler *sp = get(handle);
  if (!sp || !yrep_out_device) return fail(POTUS_ERR_STATE, "bad handle or null output");
  if (const int rc_ = refuse_many_datasets(sp, what)) return rc_;
  if (const int rc_ = ppc_check_modes(what, integrate, rep)) return rc_;
  const int Np = sp->M.Npoll;
  if (poll_begin < 0 || poll_end > Np || poll_begin >= poll_end) return fail(POTUS_ERR_ARG, "%s: polls [%d, %d) of %d", what, poll_begin, poll_end, Np);
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, sp->device, yrep_out_device, "output")) return rc_;
  int n_saved = 0, rc = saved_count(sp, &n_saved);
  if (rc) return rc;
  const int first = warm_rows(sp, n_saved), n_post = n_saved - first, C = sp->R.chains;
  if (n_post < 1) return fail(POTUS_ERR_STATE, "%s: no post-warm-up draws saved (%d saved, %d of them warm-up)", what, n_saved, first);
  std::fill(g_ppc_ms, g_ppc_ms + 4, 0.0);
  DevBufs keep;
  LooRows r;
  if ((rc = loo_rows_setup(sp, (long long)n_post * C, keep, r, what))) return rc;
  const int nb = loo_block_polls((size_t)n_post * C * 8, poll_end - poll_begin);
  double *blk = nullptr, *out = (double *)yrep_out_device;
  if ((rc = keep.get(&blk, (size_t)n_post * C * nb * 8, what))) return rc;
  EventTimer t;
  HIP_TRY(t.made);
  for (int b0 = poll_begin; b0 < poll_end; b0 += nb) {
    const int b1 = std::min(b0 + nb, poll_end);
    HIP_TRY(t.start(sp->stream));
    if ((rc = ppc_rep(sp, r, first, n_post, b0, b1, integrate, rep, blk))) return rc;
    if ((rc = el_span(t, sp->stream, g_ppc_ms, 1))) return rc;
    if ((rc = transpose_block(sp->stream, blk, out + (size_t)(b0 - poll_begin) * C * n_post, n_post, C, b1 - b0, C, 0))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(sp->stream));
  return 0;
}

int potus_ppc_pit_device(int device, const void *yrep, const double *y, const void *log_weights, int n_polls, int n_chains, long long n_draws, double *out) {
  const char *what = "potus_ppc_pit_device";
  if (!yrep || !y || !out || n_polls < 1) return fail(POTUS_ERR_ARG, "%s: bad argument", what);
  if (const int rc_ = el_check_sizes(what, n_chains, n_draws)) return rc_;
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, device, yrep, "block of y_rep")) return rc_;
  if (log_weights) if (const int rc_ = mm_also_device(what, device, log_weights, "block of log weights")) return rc_;
  std::fill(g_ppc_ms, g_ppc_ms + 4, 0.0);
  return ppc_pit(0, (const double *)yrep, y, (const double *)log_weights, n_polls, (long long)n_chains * n_draws, out, 2, g_ppc_ms, what);
}

int potus_ppc_groups_device(int device, const void *yrep, const void *a1, const void *a2, const double *y, const double *n, const int32_t *groups, int n_groups,
                            int n_polls, int n_chains, long long n_draws, void *acc_device, int flags, double *group_out, long long *n_in_group) {
  const char *what = "potus_ppc_groups_device";
  if (!yrep || !a1 || !a2 || !y || !n || !groups || !n_in_group || n_polls < 1) return fail(POTUS_ERR_ARG, "%s: bad argument", what);
  if (flags < 0 || flags > (POTUS_PPC_BEGIN | POTUS_PPC_FINISH)) return fail(POTUS_ERR_ARG, "%s: flags = %d", what, flags);
  const bool begin = flags & POTUS_PPC_BEGIN, finish = flags & POTUS_PPC_FINISH;
  if (finish && !group_out) return fail(POTUS_ERR_ARG, "%s: POTUS_PPC_FINISH without group_out", what);
  if (!acc_device && !(begin && finish)) return fail(POTUS_ERR_ARG, "%s: without acc_device the call is the first and the last block (flags = 3)", what);
  if (const int rc_ = ppc_check_labels(what, groups, n_polls, n_groups, 0)) return rc_;
  if (const int rc_ = el_check_sizes(what, n_chains, n_draws)) return rc_;
  DeviceBlock dev;
  if (const int rc_ = dev.open(what, device, yrep, "block of y_rep")) return rc_;
  if (const int rc_ = mm_also_device(what, device, a1, "block of a1")) return rc_;
  if (const int rc_ = mm_also_device(what, device, a2, "block of a2")) return rc_;
  if (acc_device) if (const int rc_ = mm_also_device(what, device, acc_device, "block of accumulators")) return rc_;
  std::fill(g_ppc_ms, g_ppc_ms + 4, 0.0);
  const long long S = (long long)n_chains * n_draws;
  const size_t acc_bytes = (size_t)n_groups * PPC_NSTAT * 2 * S * 8;
  DevBufs tmp;
  double *acc = (double *)acc_device;
  int rc;
  if (!acc && (rc = tmp.get(&acc, acc_bytes, what))) return rc;
  if (begin) {
    HIP_TRY(hipMemset(acc, 0, acc_bytes));
    std::fill(n_in_group, n_in_group + n_groups, 0ll);
  }
  if ((rc = ppc_groups_add(0, (const double *)yrep, (const double *)a1, (const double *)a2, y, n, groups, n_groups, n_polls, S, acc, n_in_group, g_ppc_ms, what))) return rc;
  if (finish && (rc = ppc_groups_finish(0, acc, n_in_group, n_groups, S, group_out, g_ppc_ms, what))) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

// Pools as potus_e_loo pools.  Per poll block: every handle's log-likelihoods, shares and replicates made on its own GPU and brought to the first
// handle's; there potus_loo's k-hat and r_eff (loo_psis), the ratios, the PSIS weights (potus_psis_device, under its own lock), the PIT and
// LOO-PIT sums and the groups' accumulators, which stay on the device from the first block to the last.
int potus_ppc(const int *handles, int n_handles, int integrate, int rep, const int32_t *groups, int n_groupings, const int32_t *n_groups, double *pit_out,
              double *pareto_k_out, double *group_out, long long *n_in_group_out) {
  const char *nm = "potus_ppc";
  if (!pit_out || !pareto_k_out) return fail(POTUS_ERR_ARG, "%s: null output", nm);
  if (n_groupings < 0 || (n_groupings > 0 && (!groups || !n_groups || !group_out || !n_in_group_out))) return fail(POTUS_ERR_ARG, "%s: %d groupings without their labels or outputs", nm, n_groupings);
  if (const int rc_ = ppc_check_modes(nm, integrate, rep)) return rc_;
  Pool P;
  if (const int rc_ = P.resolve(handles, n_handles, nm)) return rc_;
  if (const int rc_ = P.same_posterior("a posterior predictive check pools the chains of one")) return rc_;
  const std::vector<Sampler *> &sps = P.sps;
  Sampler *s0 = P.s0;
  const int Np = s0->M.Npoll, Sst = s0->M.S, Npad = s0->M.Npad;
  if (Np < 1) return fail(POTUS_ERR_ARG, "%s: the data hold no polls", nm);
  std::vector<size_t> goff(n_groupings + 1, 0);
  for (int j = 0; j < n_groupings; j++) {
    if (const int rc_ = ppc_check_labels(nm, groups + (size_t)j * Np, Np, n_groups[j], j)) return rc_;
    goff[j + 1] = goff[j] + (size_t)n_groups[j];
  }
  size_t budget = PPC_BLOCK_BUDGET;
  if (const char *e = getenv("POTUS_PPC_BLOCK_BUDGET")) budget = std::max<size_t>(1, (size_t)atoll(e));
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
  DevBufs keep;
  double *cols = nullptr, *rr = nullptr, *lw = nullptr, *b1 = nullptr, *b2 = nullptr, *yr = nullptr, *acc = nullptr;
  int Ctot = 0, n_post = 0, first = 0, nb = 0;
  long long Stot = 0;
  std::vector<LooRows> rows(sps.size());
  std::vector<double> y(Np), n(Np);
  {
    DeviceGuard guard;
    DeviceLocks lock(P.devs);
    if (const int rc_ = P.count()) return rc_;
    if (const int rc_ = P.equal_counts()) return rc_;
    Ctot = P.chains;
    if (const int rc_ = P.post_warmup(&first, &n_post)) return rc_;
    Stot = (long long)n_post * Ctot;
    if (const int rc_ = el_check_sizes(nm, Ctot, n_post)) return rc_;
    int rc;
    for (size_t i = 0; i < sps.size(); i++)
      if ((rc = loo_rows_setup(sps[i], (long long)n_post * sps[i]->R.chains, keep, rows[i], nm))) return rc;
    // six pooled blocks (log-likelihoods, ratios, weights, a1, a2, y_rep) and a handle's block before its transpose
    nb = (int)std::max<size_t>(1, std::min<size_t>((size_t)Np, budget / ((size_t)Stot * 8 * 7)));
    HIP_TRY(hipSetDevice(s0->device));
    const size_t blk_bytes = (size_t)Stot * nb * 8;
    if ((rc = keep.get(&cols, blk_bytes, nm)) || (rc = keep.get(&rr, blk_bytes, nm)) || (rc = keep.get(&lw, blk_bytes, nm)) || (rc = keep.get(&b1, blk_bytes, nm)) ||
        (rc = keep.get(&b2, blk_bytes, nm)) || (rc = keep.get(&yr, blk_bytes, nm)))
      return rc;
    if (n_groupings) {
      const size_t acc_bytes = goff[n_groupings] * PPC_NSTAT * 2 * (size_t)Stot * 8;
      if ((rc = keep.get(&acc, acc_bytes, nm))) return rc;
      HIP_TRY(hipMemset(acc, 0, acc_bytes));
      std::fill(n_in_group_out, n_in_group_out + goff[n_groupings], 0ll);
    }
    std::vector<double> pd((size_t)2 * Npad);
    std::vector<int> pi((size_t)6 * Npad);
    HIP_TRY(hipMemcpy(pd.data(), s0->M.pd, pd.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pi.data(), s0->M.pi, pi.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < Np; i++) {          // the model's (day-sorted) poll i is poll k of the output numbering
      const int st = pi[i], qi = pi[(size_t)5 * Npad + i], k = st == Sst ? s0->M.Ns + (qi - s0->M.o_nn) : qi - s0->M.o_ns;
      y[k] = pd[i]; n[k] = pd[(size_t)Npad + i];
    }
  }
  std::vector<double> pw((size_t)nb * LOO_NPW), re(nb), kk(nb);
  for (int b0 = 0; b0 < Np; b0 += nb) {
    const int e1 = std::min(b0 + nb, Np), nbk = e1 - b0;
    {
      DeviceGuard guard;
      DeviceLocks lock(P.devs);
      int rc, coff = 0;
      HIP_TRY(hipSetDevice(s0->device));
      for (size_t i = 0; i < sps.size(); i++) {
        Sampler *sp = sps[i];
        const int C = sp->R.chains;
        const size_t bytes = (size_t)n_post * C * nbk * 8;
        DevBufs blkbuf;
        double *blk = nullptr;
        if ((rc = blkbuf.get(&blk, bytes, nm))) return rc;
        // (one block at a time: made on the handle's GPU, brought over, transposed into its chains' places)
        for (int which = 0; which < 3; which++) {          // log-likelihoods; a1 (a2 comes from the same launch, into a block of its own: f2); y_rep
          double *dst = which == 0 ? cols : which == 1 ? b1 : yr;
          DevBufs far2;
          double *f2 = nullptr, *g2 = nullptr;
          if (which == 1) {
            HIP_TRY(hipSetDevice(sp->device));
            if ((rc = far2.get(&f2, bytes, nm))) return rc;
            HIP_TRY(hipSetDevice(s0->device));
          }
          if ((rc = gather_block(s0, sp, bytes, blk, [&](double *o) {
                 EventTimer t;
                 HIP_TRY(t.made);
                 HIP_TRY(t.start(sp->stream));
                 if (which == 0) { if (const int r_ = loo_loglik(sp, rows[i], first, n_post, b0, e1, integrate, o)) return r_; }
                 else if (which == 1) {
                   ElShareParams Q{row_src(sp, first), sp->L.ncols, n_post, b0, e1, integrate, rows[i].scratch, o, f2};
                   hipLaunchKernelGGL(k_el_poll_share, dim3(rows[i].grid), dim3(256), 0, sp->stream, (const DevModel *)sp->dM, Q);
                 } else if (const int r_ = ppc_rep(sp, rows[i], first, n_post, b0, e1, integrate, rep, o)) return r_;
                 return el_span(t, sp->stream, ms, which == 0 ? 0 : 1);
               }))) return rc;
          if ((rc = pool_transpose(s0, blk, dst, n_post, C, nbk, Ctot, coff))) return rc;
          if (which == 1) {
            const double *src2 = f2;
            DevBufs near2;
            if (sp->device != s0->device) {
              if ((rc = near2.get(&g2, bytes, nm))) return rc;
              HIP_TRY(hipMemcpyPeer(g2, s0->device, f2, sp->device, bytes));
              HIP_TRY(hipDeviceSynchronize());
              src2 = g2;
            }
            if ((rc = pool_transpose(s0, src2, b2, n_post, C, nbk, Ctot, coff))) return rc;
          }
        }
        coff += C;
      }
      EventTimer t;
      HIP_TRY(t.made);
      HIP_TRY(t.start(s0->stream));
      if ((rc = loo_psis(s0->stream, cols, nbk, Ctot, n_post, nullptr, pw.data(), nm))) return rc;
      const MmRatioParams R{nullptr, cols, nullptr, nullptr, nullptr, rr, nullptr, n_post, (int)Stot, nbk, 0};
      hipLaunchKernelGGL(k_mm_ratio, dim3((unsigned)std::min<long long>(((long long)nbk * Stot + 255) / 256, 65535)), dim3(256), 0, s0->stream, R);
      if ((rc = el_span(t, s0->stream, ms, 0))) return rc;
    }
    for (int k = 0; k < nbk; k++) { pareto_k_out[b0 + k] = pw[(size_t)k * LOO_NPW + 3]; re[k] = pw[(size_t)k * LOO_NPW + 4]; }
    // a poll with identical log-likelihoods has no r_eff (NaN): any value gives its flat tail no fit (potus_e_loo's rule)
    for (int k = 0; k < nbk; k++) if (!(std::isfinite(re[k]) && re[k] > 0)) re[k] = 1.0;
    {
      DeviceGuard guard;
      HIP_TRY(hipSetDevice(s0->device));
      EventTimer t;
      HIP_TRY(t.made);
      HIP_TRY(t.start(0));
      if (const int rc = potus_psis_device(s0->device, rr, nbk, Ctot, n_post, re.data(), lw, kk.data())) return rc;
      if (const int rc = el_span(t, 0, ms, 0)) return rc;
    }
    {
      DeviceGuard guard;
      DeviceLocks lock(P.devs);
      int rc;
      HIP_TRY(hipSetDevice(s0->device));
      if ((rc = ppc_pit(s0->stream, yr, y.data() + b0, nullptr, nbk, Stot, pit_out + (size_t)b0 * 4, 4, ms, nm))) return rc;
      if ((rc = ppc_pit(s0->stream, yr, y.data() + b0, lw, nbk, Stot, pit_out + (size_t)b0 * 4 + 2, 4, ms, nm))) return rc;
      for (int k = b0; k < e1; k++) if (!(n[k] > 0)) for (int c = 0; c < 4; c++) pit_out[(size_t)k * 4 + c] = NAN;
      for (int j = 0; j < n_groupings; j++)
        if ((rc = ppc_groups_add(s0->stream, yr, b1, b2, y.data() + b0, n.data() + b0, groups + (size_t)j * Np + b0, n_groups[j], nbk, Stot,
                                 acc + goff[j] * PPC_NSTAT * 2 * (size_t)Stot, n_in_group_out + goff[j], ms, nm)))
          return rc;
    }
  }
  {
    DeviceGuard guard;
    DeviceLocks lock(P.devs);
    HIP_TRY(hipSetDevice(s0->device));
    for (int j = 0; j < n_groupings; j++)
      if (const int rc = ppc_groups_finish(s0->stream, acc + goff[j] * PPC_NSTAT * 2 * (size_t)Stot, n_in_group_out + goff[j], n_groups[j], Stot,
                                           group_out + goff[j] * PPC_NSTAT * PPC_NOUT, ms, nm))
        return rc;
  }
  std::copy(ms, ms + 4, g_ppc_ms);
  return 0;
}

// ---------------------------------------------------------------- .C() wrappers
void potus_R_create(int *dims, int *state, int *day_state, int *day_national, int *poll_state, int *poll_national,
                    int *poll_mode_state, int *poll_mode_national, int *poll_pop_state, int *poll_pop_national,
                    int *n_democrat_national, int *n_two_share_national, int *n_democrat_state, int *n_two_share_state,
                    double *unadjusted_national, double *unadjusted_state, double *mu_b_prior, double *state_weights,
                    double *scalars, double *state_covariance_0, int *iopts, double *dopts, int *handle, int *status) {
  potus_data d{};
  d.N_national_polls = dims[0]; d.N_state_polls = dims[1]; d.T = dims[2]; d.S = dims[3]; d.P = dims[4]; d.M = dims[5]; d.Pop = dims[6];
  d.variant = dims[7];
  d.state = state; d.day_state = day_state; d.day_national = day_national; d.poll_state = poll_state; d.poll_national = poll_national;
  d.poll_mode_state = poll_mode_state; d.poll_mode_national = poll_mode_national; d.poll_pop_state = poll_pop_state;
  d.poll_pop_national = poll_pop_national; d.n_democrat_national = n_democrat_national; d.n_two_share_national = n_two_share_national;
  d.n_democrat_state = n_democrat_state; d.n_two_share_state = n_two_share_state; d.unadjusted_national = unadjusted_national;
  d.unadjusted_state = unadjusted_state; d.mu_b_prior = mu_b_prior; d.state_weights = state_weights;
  d.sigma_c = scalars[0]; d.sigma_m = scalars[1]; d.sigma_pop = scalars[2]; d.sigma_measure_noise_national = scalars[3];
  d.sigma_measure_noise_state = scalars[4]; d.sigma_e_bias = scalars[5]; d.random_walk_scale = scalars[6]; d.mu_b_T_scale = scalars[7];
  d.polling_bias_scale = scalars[8]; d.state_covariance_0 = state_covariance_0;
  potus_opts o; potus_default_opts(&o);
  o.chains = iopts[0]; o.chain_id_offset = iopts[1]; o.num_warmup = iopts[2]; o.num_samples = iopts[3]; o.max_depth = iopts[4];
  o.device = iopts[5]; o.save_warmup = iopts[6]; o.cus_per_chain = iopts[7]; o.metric = iopts[8]; o.twin = iopts[9]; o.metric_storage = iopts[10]; o.pooled_metric = iopts[11];
  o.delta = dopts[0]; o.gamma = dopts[1]; o.kappa = dopts[2]; o.t0 = dopts[3]; o.stepsize = dopts[4]; o.init_radius = dopts[5];
  if (!(dopts[6] >= 0) || dopts[6] > 9007199254740992.0 || dopts[6] != std::floor(dopts[6])) { *status = fail(POTUS_ERR_ARG, "seed must be a non-negative integer below 2^53"); return; }
  o.seed = (uint64_t)dopts[6];   // R integers are 32 bits wide: the seed travels as a double (exact to 2^53)
  *status = potus_create(&d, &o, handle);
}
void potus_R_init(int *handle, int *status) { *status = potus_init(*handle, nullptr); }
void potus_R_run(int *handle, int *n_iter, int *status) { *status = potus_run(*handle, *n_iter); }
void potus_R_run_many(int *handles, int *n_handles, int *n_iter, int *status) { *status = potus_run_many(handles, *n_handles, *n_iter); }
void potus_R_num_columns(int *handle, int *D, int *n_cols, int *status) {
  Sampler *sp = get(*handle);
  if (!sp) { *status = fail(POTUS_ERR_STATE, "bad handle"); return; }
  *D = sp->L.D; *n_cols = sp->L.ncols; *status = 0;
}
void potus_R_write_array(int *handle, int *col_begin, int *col_end, double *out, int *status) { *status = potus_write_array(*handle, *col_begin, *col_end, out); }
void potus_R_write_stan_csv(int *handle, char **dir, char **basename, int *status) { *status = potus_write_stan_csv(*handle, dir[0], basename[0]); }
void potus_R_posterior_summary(int *handles, int *n_handles, double *ev, double *state_out, double *natl_out, double *ev_out, int *status) {
  *status = potus_posterior_summary_many(handles, *n_handles, ev, state_out, natl_out, ev_out);
}
void potus_R_diagnostics(int *handles, int *n_handles, int *cols /*[2]: col_begin, col_end*/, double *rhat_out, double *ess_bulk_out, int *status) {
  *status = potus_diagnostics(handles, *n_handles, cols[0], cols[1], rhat_out, ess_bulk_out);
}
void potus_R_check_convergence(int *handles, int *n_handles, double *limits /*[2]: rhat_below, ess_at_least*/, int *converged, double *out /*[2]: rhat_max, ess_bulk_min*/, int *status) {
  *status = potus_check_convergence(handles, *n_handles, limits[0], limits[1], converged, out, out + 1);
}
void potus_R_backtest_scores(double *state_out, int *dims /*[3]: T, S, day*/, double *ev, int *won, double *out, int *status) {
  *status = potus_backtest_scores(state_out, dims[0], dims[1], dims[2], ev, won, out);
}
void potus_R_saved_count(int *handle, int *n_saved, int *status) { *status = potus_get_draws(*handle, nullptr, n_saved); }
void potus_R_last_error(char **buf, int *len) { potus_last_error(buf[0], *len); }
void potus_R_destroy(int *handle, int *status) { *status = potus_destroy(*handle); }
void potus_R_set_datasets_ex(int *handle, int *n_datasets, int *n_democrat_state, int *n_democrat_national, int *n_two_share_state, int *n_two_share_national,
                             int *has_prior, double *mu_b_prior, int *has_scale, double *mu_b_T_scale, int *status) {
  *status = potus_set_datasets_ex(*handle, *n_datasets, n_democrat_state, n_democrat_national, n_two_share_state, n_two_share_national,
                                  *has_prior ? mu_b_prior : nullptr, *has_scale ? mu_b_T_scale : nullptr);
}
void potus_R_set_datasets_grid(int *handle, int *n_datasets, int *n_democrat_state, int *n_democrat_national, int *n_two_share_state, int *n_two_share_national,
                               int *has /*[3]: mu_b_prior, mu_b_T_scale, scales given*/, double *mu_b_prior, double *mu_b_T_scale, double *scales, int *status) {
  *status = potus_set_datasets_grid(*handle, *n_datasets, n_democrat_state, n_democrat_national, n_two_share_state, n_two_share_national,
                                    has[0] ? mu_b_prior : nullptr, has[1] ? mu_b_T_scale : nullptr, has[2] ? scales : nullptr);
}
void potus_R_grid_compare(int *handle, int *iargs /*[4]: base, day_begin, day_end, ev_to_win*/, double *ev, double *out, int *n_draws_out, int *status) {
  *status = potus_grid_compare(*handle, iargs[0], iargs[1], iargs[2], ev, iargs[3], out, n_draws_out);
}
void potus_R_timeline(int *handle, int *day_begin, int *day_end, double *ev, int *ev_to_win, double *state_out, double *natl_out, double *ev_out, int *n_draws_out, int *status) {
  *status = potus_timeline(*handle, *day_begin, *day_end, ev, *ev_to_win, state_out, natl_out, ev_out, n_draws_out);
}
void potus_R_cv_lpd(int *handle, int *held_state, int *held_national, int *integrate, double *lpd_out, int *n_draws_out, int *status) {
  *status = potus_cv_lpd(*handle, held_state, held_national, *integrate, lpd_out, n_draws_out);
}
void potus_R_optimize(int *handle, int *iopts /*[7]: jacobian, history_size, iter, path_offset, n_paths, q0 given, rows wanted*/,
                      double *dopts /*[6]: init_alpha, tol_obj, tol_rel_obj, tol_grad, tol_rel_grad, tol_param*/, double *q0, double *q_out, double *lp_out,
                      double *gnorm_out, int *info_out, int *cols /*[2]: col_begin, col_end*/, double *row_out, int *status) {
  potus_optimize_opts o;
  o.jacobian = iopts[0]; o.history_size = iopts[1]; o.iter = iopts[2]; o.path_offset = iopts[3];
  o.init_alpha = dopts[0]; o.tol_obj = dopts[1]; o.tol_rel_obj = dopts[2]; o.tol_grad = dopts[3]; o.tol_rel_grad = dopts[4]; o.tol_param = dopts[5];
  *status = potus_optimize(*handle, &o, iopts[5] ? q0 : nullptr, iopts[4], q_out, lp_out, gnorm_out, info_out, cols[0], cols[1], iopts[6] ? row_out : nullptr);
}
void potus_R_laplace(int *handle, int *iopts /*[6]: jacobian, draw_offset, n_modes, n_draws, u given, precision wanted*/, double *h, double *mode, double *u,
                     double *q_out, double *lp_out, double *lp_approx_out, double *info_out, double *precision_out, int *status) {
  potus_laplace_opts o;
  potus_default_laplace_opts(&o);
  o.jacobian = iopts[0]; o.draw_offset = iopts[1]; o.h = *h;
  const bool draws = iopts[3] > 0;
  *status = potus_laplace(*handle, &o, mode, iopts[2], iopts[4] ? u : nullptr, iopts[3], draws ? q_out : nullptr, draws ? lp_out : nullptr,
                          draws ? lp_approx_out : nullptr, info_out, iopts[5] ? precision_out : nullptr);
}
void potus_R_pathfinder(int *handle, int *iopts /*[9]: history_size, num_elbo_draws, num_draws, draw_offset, path_offset, max_lbfgs_iters, L-BFGS history, n_paths, q0 given*/,
                        double *dopts /*[6]: init_alpha, tol_obj, tol_rel_obj, tol_grad, tol_rel_grad, tol_param*/, double *q0, int *info_out, double *elbo_out,
                        int *kept_out, double *q_out, double *lp_out, double *lq_out, int *status) {
  potus_pathfinder_opts o;
  potus_default_pathfinder_opts(&o);
  o.history_size = iopts[0]; o.num_elbo_draws = iopts[1]; o.num_draws = iopts[2]; o.draw_offset = iopts[3]; o.path_offset = iopts[4];
  o.opt.iter = iopts[5]; o.opt.history_size = iopts[6];
  o.opt.init_alpha = dopts[0]; o.opt.tol_obj = dopts[1]; o.opt.tol_rel_obj = dopts[2]; o.opt.tol_grad = dopts[3]; o.opt.tol_rel_grad = dopts[4]; o.opt.tol_param = dopts[5];
  const bool draws = iopts[2] > 0;
  *status = potus_pathfinder(*handle, &o, iopts[8] ? q0 : nullptr, iopts[7], info_out, elbo_out, kept_out, draws ? q_out : nullptr, draws ? lp_out : nullptr,
                             draws ? lq_out : nullptr, nullptr, nullptr);
}
void potus_R_variational(int *handle, int *iopts /*[11]: iter, grad_samples, elbo_samples, eval_elbo, adapt_engaged, adapt_iter, output_samples, draw_offset, run_offset, n_runs, q0 given*/,
                         double *dopts /*[3]: eta, tol_rel_obj, elbo_offset*/, double *q0, int *info_out, double *mu_out, double *omega_out, double *elbo_out,
                         double *adapt_elbo_out, double *q_out, double *lp_out, double *lq_out, int *status) {
  potus_advi_opts o;
  potus_default_advi_opts(&o);
  o.iter = iopts[0]; o.grad_samples = iopts[1]; o.elbo_samples = iopts[2]; o.eval_elbo = iopts[3]; o.adapt_engaged = iopts[4]; o.adapt_iter = iopts[5];
  o.output_samples = iopts[6]; o.draw_offset = iopts[7]; o.run_offset = iopts[8];
  o.eta = dopts[0]; o.tol_rel_obj = dopts[1]; o.elbo_offset = dopts[2];
  const bool draws = iopts[6] > 0;
  *status = potus_advi(*handle, &o, iopts[10] ? q0 : nullptr, iopts[9], info_out, mu_out, omega_out, elbo_out, adapt_elbo_out, draws ? q_out : nullptr,
                       draws ? lp_out : nullptr, draws ? lq_out : nullptr);
}
void potus_R_set_datasets(int *handle, int *n_datasets, int *n_democrat_state, int *n_democrat_national, int *status) {
  *status = potus_set_datasets(*handle, *n_datasets, n_democrat_state, n_democrat_national);
}
void potus_R_simulate_prior(int *handle, double *seed, int *dims /*[2]: n_sims, sim_offset*/, double *q_out, int *n_democrat_state_out, int *n_democrat_national_out,
                            int *status) {
  if (!(seed[0] >= 0) || seed[0] > 9007199254740992.0 || seed[0] != std::floor(seed[0])) { *status = fail(POTUS_ERR_ARG, "seed must be a non-negative integer below 2^53"); return; }
  *status = potus_simulate_prior(*handle, (uint64_t)seed[0], dims[0], dims[1], q_out, n_democrat_state_out, n_democrat_national_out);
}
void potus_R_sbc_ranks(int *handle, double *truth, int *cols /*[3]: col_begin, col_end, thin*/, int *less, int *equal, int *L, int *status) {
  *status = potus_sbc_ranks(*handle, truth, cols[0], cols[1], cols[2], less, equal, L);
}
void potus_R_constrain(int *handle, double *q, int *n, int *cols /*[2]: col_begin, col_end*/, double *out, int *status) {
  *status = potus_constrain(*handle, q, *n, cols[0], cols[1], out);
}
void potus_R_monitor(int *handles, int *n_handles, int *cols /*[2]: col_begin, col_end*/, double *probs, int *n_probs, double *out, int *status) {
  *status = potus_monitor(handles, *n_handles, cols[0], cols[1], probs, *n_probs, out);
}
void potus_R_loo(int *handles, int *n_handles, int *iopts /*[2]: integrate, r_eff given*/, double *r_eff, double *pointwise_out, double *estimates_out,
                 int *status) {
  *status = potus_loo(handles, *n_handles, iopts[0], iopts[1] ? r_eff : nullptr, pointwise_out, estimates_out);
}
// E_loo on a fit: influence (iopts: integrate, ev_to_win, day (-1: election day), diag) and predict; the outputs of potus_e_loo
void potus_R_loo_influence(int *handles, int *n_handles, int *iopts /*[4]*/, double *ev, double *loo_mean, double *var_out, double *post_out, double *pareto_k,
                           double *ess, double *khat, int *status) {
  *status = potus_e_loo(handles, *n_handles, iopts[0], POTUS_ELOO_INFLUENCE, ev, iopts[1], iopts[2], 0, 0, iopts[3], loo_mean, var_out, post_out, pareto_k, ess, khat, nullptr, nullptr);
}
void potus_R_loo_predict(int *handles, int *n_handles, int *integrate, double *out /*[N][5]*/, double *pareto_k, int *status) {
  *status = potus_e_loo(handles, *n_handles, *integrate, POTUS_ELOO_PREDICT, nullptr, 0, -1, 0, 0, 0, out, nullptr, nullptr, pareto_k, nullptr, nullptr, nullptr, nullptr);
}
void potus_R_ppc(int *handles, int *n_handles, int *iopts /*[3]: integrate, rep, n_groupings*/, int *groups, int *n_groups, double *pit_out, double *pareto_k,
                 double *group_out, double *n_in_group, int *status) {
  size_t tot = 0;
  for (int j = 0; j < iopts[2]; j++) tot += (size_t)std::max(n_groups[j], 0);
  std::vector<long long> cnt(std::max<size_t>(tot, 1), 0);
  *status = potus_ppc(handles, *n_handles, iopts[0], iopts[1], groups, iopts[2], n_groups, pit_out, pareto_k, group_out, cnt.data());
  if (*status == 0) for (size_t g = 0; g < tot; g++) n_in_group[g] = (double)cnt[g];
}
void potus_R_loo_moment_match(int *model_handle, int *handles, int *n_handles, int *iopts /*[5]: integrate, max_iters, split, cov, n_polls (0: every poll)*/,
                              double *k_threshold, int *polls, double *pointwise, double *estimates_out, int *info_out, int *status) {
  const potus_loo_mm_opts o{iopts[0], iopts[1], iopts[2], iopts[3], *k_threshold};
  *status = potus_loo_moment_match(*model_handle, handles, *n_handles, &o, iopts[4] > 0 ? polls : nullptr, iopts[4], pointwise, estimates_out, info_out, nullptr, nullptr);
}
// counts come back as doubles (exact below 2^53); below_actual is written only when actual is given
void potus_R_outcomes(int *handles, int *n_handles, int *iopts /*[4]: day_begin, day_end, ev_to_win, actual given*/, int *ev, double *actual,
                      double *ev_hist, double *tipping, double *joint, double *below_actual, double *n_draws, int *status) {
  Sampler *sp = (handles && *n_handles >= 1) ? get(handles[0]) : nullptr;
  if (!sp || !ev) { *status = fail(POTUS_ERR_STATE, "potus_R_outcomes: bad handle or null ev"); return; }
  const int S = sp->M.S;
  const size_t days = iopts[1] > iopts[0] ? (size_t)(iopts[1] - iopts[0]) : 0;
  long long sum = 0;
  for (int s = 0; s < S; s++) sum += ev[s] > 0 ? ev[s] : 0;
  // (a refused call writes nothing: the sizes below only matter for the arguments potus_outcomes accepts)
  std::vector<long long> h(days * (size_t)(sum <= OC_EV_CAP ? sum + 1 : 0)), t(days * (size_t)(S + 1)), j(days * (size_t)(S + 2) * (S + 2)), b(days * (size_t)S);
  long long n = 0;
  *status = potus_outcomes(handles, *n_handles, iopts[0], iopts[1], ev, iopts[2], iopts[3] ? actual : nullptr, h.data(), t.data(), j.data(), b.data(), &n);
  if (*status) return;
  for (size_t i = 0; i < h.size(); i++) ev_hist[i] = (double)h[i];
  for (size_t i = 0; i < t.size(); i++) tipping[i] = (double)t[i];
  for (size_t i = 0; i < j.size(); i++) joint[i] = (double)j[i];
  if (iopts[3]) for (size_t i = 0; i < b.size(); i++) below_actual[i] = (double)b[i];
  *n_draws = (double)n;
}

// counts come back as doubles; n[2] = n_kept, n_draws.  iopts[5], [6] say which outputs are wanted: the others are left alone
void potus_R_scenario(int *handles, int *n_handles, int *iopts /*[7]: cond_day, day_begin, day_end, ev_to_win, bounds given, moments wanted, counts wanted*/,
                      double *lo, double *hi, int *ev, double *n, double *mean, double *cov, double *ev_hist, double *tipping, double *joint, int *status) {
  Sampler *sp = (handles && *n_handles >= 1) ? get(handles[0]) : nullptr;
  if (!sp) { *status = fail(POTUS_ERR_STATE, "potus_R_scenario: bad handle"); return; }
  const int S = sp->M.S;
  const bool counts = iopts[6] != 0 && ev != nullptr;
  if (iopts[6] && !ev) { *status = fail(POTUS_ERR_ARG, "potus_R_scenario: ev is null, but the counts are asked for"); return; }
  const size_t days = iopts[2] > iopts[1] ? (size_t)(iopts[2] - iopts[1]) : 0;
  long long sum = 0;
  if (counts) for (int s = 0; s < S; s++) sum += ev[s] > 0 ? ev[s] : 0;
  std::vector<long long> h, t, j;
  if (counts) { h.resize(days * (size_t)(sum <= OC_EV_CAP ? sum + 1 : 0)); t.resize(days * (size_t)(S + 1)); j.resize(days * (size_t)(S + 2) * (S + 2)); }
  long long nk = 0, nd = 0;
  *status = potus_scenario(handles, *n_handles, iopts[0], iopts[4] ? lo : nullptr, iopts[4] ? hi : nullptr, iopts[1], iopts[2], counts ? ev : nullptr, iopts[3], &nk, &nd,
                           iopts[5] ? mean : nullptr, iopts[5] ? cov : nullptr, counts ? h.data() : nullptr, counts ? t.data() : nullptr, counts ? j.data() : nullptr);
  if (*status) return;
  for (size_t i = 0; i < h.size(); i++) ev_hist[i] = (double)h[i];
  for (size_t i = 0; i < t.size(); i++) tipping[i] = (double)t[i];
  for (size_t i = 0; i < j.size(); i++) joint[i] = (double)j[i];
  n[0] = (double)nk; n[1] = (double)nd;
}

void potus_R_forecast_scores(int *handles, int *n_handles, int *iopts /*[3]: day_begin, day_end, ev_to_win*/, double *ev, double *actual, int *use, double *vs_p,
                             double *uni_out, double *multi_out, double *n_draws, int *status) {
  if (!handles || !n_handles || !iopts || !vs_p || !n_draws) { *status = fail(POTUS_ERR_ARG, "potus_R_forecast_scores: null argument"); return; }
  long long nd = 0;
  *status = potus_forecast_scores(handles, *n_handles, iopts[0], iopts[1], ev, iopts[2], actual, use, *vs_p, uni_out, multi_out, &nd);
  if (!*status) *n_draws = (double)nd;
}

} // extern "C"
