// potus_rules.hpp -- the scalar rules of Stan 2.24's NUTS and warm-up adaptation, stated once for every sampler.
//
// One workgroup per chain (potus_nuts.hpp), two workgroups per chain (potus_nuts_twin.hpp), a cluster per chain
// (potus_cluster.hpp), the dense metric (potus_dense.hpp) and the host's window schedule of the dense sampler all run the same
// algorithm on different carriers.  What does not depend on the carrier is here: each rule works on the scalars it is handed
// and nothing else -- no thread index, no barrier, no vector.  Where a rule takes the transition state `ts` or the chain
// scalars `sc` it is a template on the pointer type: the diagonal samplers pass address-space pointers (ltp, gsc), the dense
// kernels plain ones.  Uniforms come in as a callable, so that a rule draws only the ones upstream would draw.
// The header compiles on its own with a C++ compiler (tests/test_rules_host.py): no HIP header is needed.
// Upstream, by file name: stepsize_adaptation.hpp, windowed_adaptation.hpp, base_hmc.hpp::init_stepsize,
// base_nuts.hpp::transition / build_tree.
#pragma once
#include <math.h>
#include "../../include/potus_hmc.h"

#ifndef __HIPCC__
#define __host__
#define __device__
#ifndef __forceinline__
#define __forceinline__ inline __attribute__((always_inline))
#endif
#endif
#define POTUS_RULE __host__ __device__ __forceinline__

// ---------------------------------------------------------------- log weights and the slot pools
POTUS_RULE double d_lse(double a, double b) {
  if (a == -INFINITY) return b;
  if (a == INFINITY && b == INFINITY) return INFINITY;
  return a > b ? a + log1p(exp(b - a)) : b + log1p(exp(a - b));
}
POTUS_RULE int pool_alloc(unsigned &mask, int n) {
  for (int i = 0; i < n; i++) if (!(mask & (1u << i))) { mask |= 1u << i; return i; }
  return n - 1; // cannot happen: pools are sized for PT_MAXD
}
POTUS_RULE void pool_free(unsigned &mask, int i) { if (i >= 0) mask &= ~(1u << i); }

// ---------------------------------------------------------------- the warm-up schedule (windowed_adaptation)
// the constructor: buffers that do not fit the warm-up become 15 % | rest | 10 %
POTUS_RULE void rule_window_params(int num_warmup, int &init_buffer, int &term_buffer, int &window) {
  if (num_warmup >= 20 && (long long)init_buffer + window + term_buffer > num_warmup) {
    init_buffer = (int)(0.15 * num_warmup); term_buffer = (int)(0.1 * num_warmup); window = num_warmup - (init_buffer + term_buffer);
  }
}
POTUS_RULE int rule_first_window_end(int init_buffer, int window) { return init_buffer + window - 1; }
// warm-up iteration wc (the chain's win_counter): does its draw join the variance window, does the window end with it
POTUS_RULE void rule_window_flags(int nw, int ib, int tb, int wc, int win_next, int &in_window, int &end_window) {
  int fa = 0, fb = 0;
  if (nw >= 20) {
    fa = wc >= ib && wc < nw - tb && wc != nw;
    fb = wc == win_next && wc != nw;
  }
  in_window = fa; end_window = fb;
}
// compute_next_window, at the end of a window: the next one is twice as long and is stretched to the terminal buffer when
// the one after it would not fit
POTUS_RULE void rule_next_window(int nw, int tb, int wc, int &win_next, int &win_size) {
  const int last = nw - tb - 1;
  int wn = win_next, wsz = win_size;
  if (wn != last) {
    wsz *= 2;
    wn = wc + wsz;
    if (wn != last) {
      const int boundary = wn + 2 * wsz;
      if (boundary >= nw - tb) wn = last;
    }
  }
  win_next = wn; win_size = wsz;
}

// ---------------------------------------------------------------- step-size adaptation (stepsize_adaptation)
template <class SC>
POTUS_RULE void rule_learn_stepsize(SC sc, double accept_stat, double delta, double gamma, double kappa, double t0) {
  const double cnt = sc->ad_counter + 1;
  sc->ad_counter = cnt;
  const double as = accept_stat > 1 ? 1.0 : accept_stat;
  const double eta = 1.0 / (cnt + t0);
  // (1 - eta) s_bar + eta (delta - as), and x_bar below: the fused forms are written out.  Left to the compiler, which of the two
  // products is fused depends on the code around the call, and the samplers' bytes with it.  These are the forms the compiler had
  // chosen in every copy this rule replaced, read from their disassembly (k_dn_end, cold_transition_end, cold_twin1_end, every
  // cl_cold_transition_end / cl_cold_twin_end): 1 - eta feeds a v_fmac, 1 - x_eta a v_mul
  // (profiles/rules_once_same_device_code.txt).
  const double s_bar = fma(1.0 - eta, sc->s_bar, eta * (delta - as));
  sc->s_bar = s_bar;
  const double x = sc->mu - s_bar * sqrt(cnt) / gamma;
  const double x_eta = pow(cnt, -kappa);
  sc->x_bar = fma(x_eta, x, (1.0 - x_eta) * sc->x_bar);
  sc->nom_eps = exp(x);
}
// after a metric update and its init_stepsize: dual averaging starts again around the new step
template <class SC> POTUS_RULE void rule_restart_stepsize(SC sc) { sc->mu = log(10.0 * sc->nom_eps); sc->s_bar = 0; sc->x_bar = 0; sc->ad_counter = 0; }
template <class SC> POTUS_RULE void rule_complete_adaptation(SC sc) { sc->nom_eps = exp(sc->x_bar); }

// the chain's scalars at potus_init: services' set_mu(log(10 * stepsize)), the first window of the schedule
template <class SC>
POTUS_RULE void rule_reset_chain(SC sc, double stepsize, int init_buffer, int window) {
  sc->nom_eps = stepsize; sc->mu = log(10.0 * stepsize); sc->s_bar = 0; sc->x_bar = 0; sc->ad_counter = 0;
  sc->wf_n = 0; sc->total_leapfrogs = 0; sc->iter = 0; sc->status = 0; sc->n_divergent = 0; sc->saved = 0; sc->leaves_run = 0; sc->spec_limit = 0x7f7f7f7f;
  sc->win_counter = 0; sc->win_size = window; sc->win_next = rule_first_window_end(init_buffer, window);
}

// ---------------------------------------------------------------- base_hmc::init_stepsize: the verdict of one attempt
// kin = p.M^-1.p and lpv = log density after one leapfrog of eps from a point of Hamiltonian H0.  The first attempt fixes
// the direction (ts->direction); a later one either ends the search (ts->done = 1) or doubles / halves sc->nom_eps.
template <class T, class SC>
POTUS_RULE void rule_init_stepsize_verdict(T ts, SC sc, bool first, double H0, double kin, double lpv, double eps) {
  double h = 0.5 * kin - lpv;
  if (isnan(h)) h = INFINITY;
  const double delta_H = H0 - h, thr = log(0.8);
  if (first) ts->direction = delta_H > thr ? 1 : -1;
  else {
    const int dirn = ts->direction;
    if (dirn == 1 && !(delta_H > thr)) ts->done = 1;
    else if (dirn == -1 && !(delta_H < thr)) ts->done = 1;
    else {
      const double ne = dirn == 1 ? 2.0 * eps : 0.5 * eps;
      sc->nom_eps = ne;
      if (ne > 1e7 || ne == 0) { ts->done = 1; sc->status = POTUS_ERR_STEPSIZE; } // upstream throws here
    }
  }
}

// ---------------------------------------------------------------- base_nuts::build_tree
// A leaf: its Hamiltonian h (kin = p.M^-1.p, lpv = log density), the divergence latch, its metropolis term, the leapfrog
// count.  Returns the leaf's log weight H0 - h.
template <class T>
POTUS_RULE double rule_leaf(T ts, double kin, double lpv, double &h_out) {
  const double H0 = ts->H0;
  double h = 0.5 * kin - lpv;
  if (isnan(h)) h = INFINITY;
  const int div = (h - H0 > 1000.0) ? 1 : ts->divergent;
  ts->divergent = div;
  const double wgt = H0 - h;
  ts->sum_metro += wgt > 0 ? 1.0 : exp(wgt);
  ts->n_leap += 1;
  h_out = h;
  return wgt;
}
// Level j of the cascade after a leaf: the pending subtree [ib, ie] and the current one [cb, ce] (momentum-pool slots) become
// the current subtree; its proposal is the final one's with probability exp(cur_lsw - lsw_sub) (u() draws the uniform);
// persist: the merged subtree passed its U-turn checks.
template <class T, class U>
POTUS_RULE void rule_merge_step(T ts, int j, int ib, int ie, int cb, int ce, bool persist, U u) {
  const double cur_lsw = ts->cur_lsw;
  const double lsw_sub = d_lse(ts->pend_lsw[j - 1], cur_lsw);
  bool take_final;
  if (cur_lsw > lsw_sub) take_final = true;
  else take_final = u() < exp(cur_lsw - lsw_sub);
  unsigned qm = ts->qmask, pm = ts->pmask;
  if (take_final) pool_free(qm, ts->pend_prop[j - 1]);
  else { pool_free(qm, ts->cur_prop); ts->cur_prop = ts->pend_prop[j - 1]; }
  if (ie != ib) pool_free(pm, ie);
  if (cb != ce) pool_free(pm, cb);
  ts->qmask = qm; ts->pmask = pm;
  ts->cur_beg = ib;
  ts->cur_lsw = lsw_sub;
  ts->abort = !persist;
}
// base_nuts::transition after doubling `depth`: the new subtree's proposal replaces the sample with probability
// exp(lsw_sub - lsw); persist: the whole trajectory passed its U-turn checks.
template <class T, class U>
POTUS_RULE void rule_top_accept(T ts, int depth, bool persist, U u) {
  ts->depth = depth + 1;
  const double lsw_sub = ts->pend_lsw[depth], lsw = ts->lsw;
  bool accept;
  if (lsw_sub > lsw) accept = true;
  else accept = u() < exp(lsw_sub - lsw);
  unsigned qm = ts->qmask;
  if (accept) { pool_free(qm, ts->sample_qid); ts->sample_qid = ts->pend_prop[depth]; }
  else pool_free(qm, ts->pend_prop[depth]);
  ts->qmask = qm;
  ts->lsw = d_lse(lsw, lsw_sub);
  if (!persist) ts->stop = 1;
}

// ---------------------------------------------------------------- the end of a transition
// the sampler columns of a saved row: lp__, accept_stat__, stepsize__, treedepth__, n_leapfrog__, divergent__, energy__
template <class ROW, class T>
POTUS_RULE void rule_sampler_cols(ROW row, T ts, double lp, double accept_stat, double energy) {
  row[0] = lp; row[1] = accept_stat; row[2] = ts->eps; row[3] = ts->depth; row[4] = ts->n_leap;
  row[5] = ts->divergent; row[6] = energy;
}
