// potus_advi_rules.hpp -- the scalar rules of mean-field ADVI (potus_advi.hpp, potus_advi in potus_hmc.hip), stated once for the host.
//
// CmdStan 2.24's advi.hpp, as include/potus_hmc.h states it: which of the five step sizes the adaptation keeps (adapt_eta), and when the
// main run stops (the circular buffer of relative ELBO differences, calc_ELBO's callers in stochastic_gradient_ascent).  Each rule works
// on the scalars it is handed and nothing else; the header compiles on its own with a C++ compiler (tests/test_advi_host.py): no HIP
// header is needed.  tests/advi_ref.py restates both rules in Python; the tests hold the two against each other.
#pragma once
#include <math.h>
#include <algorithm>
#include <vector>

enum { ADVI_MEAN_CONVERGED = 1, ADVI_MEDIAN_CONVERGED = 2, ADVI_MAXIT = 3, ADVI_NONFINITE = 4, ADVI_INIT = 5, ADVI_ADAPT_FAILED = 6 };
enum { ADVI_FLAG_DIVERGING = 1 };   // Stan's "the algorithm may be diverging" message, a bit of the info word
#define ADVI_N_ETA 5
inline double advi_eta(int k) { const double e[ADVI_N_ETA] = {100.0, 10.0, 1.0, 0.1, 0.01}; return e[k]; }

// The step size the SEQUENTIAL search keeps, from the ELBOs of all five candidates (a candidate that ended NONFINITE comes in as -inf):
//   if elbo < best and best > elbo_init: stop;  else if elbo > best: best = elbo, eta* = eta;
//   after the last candidate: its elbo <= elbo_init is a failure.
// Returns the index of eta*, or -1 (ADAPT_FAILED).  *n_seen: how many candidates the sequential search would have run.
inline int advi_pick_eta(double elbo_init, const double *elbo /*[ADVI_N_ETA]*/, int *n_seen) {
  double best = -INFINITY;
  int pick = -1, k = 0;
  for (; k < ADVI_N_ETA; k++) {
    if (elbo[k] < best && best > elbo_init) break;
    if (elbo[k] > best) { best = elbo[k]; pick = k; }
    if (k == ADVI_N_ETA - 1 && !(elbo[k] > elbo_init)) pick = -1;
  }
  if (n_seen) *n_seen = k < ADVI_N_ETA ? k + 1 : ADVI_N_ETA;
  return pick;
}

// The main run's stop.  Every eval_elbo iterations: prev = elbo (the variable starts at 0, so the first relative difference is 1),
// elbo = the new ELBO, delta = |(elbo - prev) / elbo| goes into a circular buffer of max(floor(0.1 iter / eval_elbo), 2) entries.
// mean: the sum of the entries, oldest first, over their number.  median: Stan's circ_buff_median, nth_element at n / 2 -- the UPPER
// of the two middle entries when their number is even.  MEAN_CONVERGED when mean < tol_rel_obj, else MEDIAN_CONVERGED when median <
// tol_rel_obj, else MAXIT at t = iter; the DIVERGING bit when t > 10 eval_elbo and mean or median > 0.5.
struct AdviConv {
  std::vector<double> buf;   // the ring: entry (head + k) % size is the k-th oldest once it is full
  size_t cap, head = 0;
  double elbo = 0.0, delta = 0.0, mean = 0.0, median = 0.0;
  AdviConv(int iter, int eval_elbo) : cap((size_t)std::max(0.1 * iter / eval_elbo, 2.0)) {}
  int push(double elbo_new, int t, int iter, int eval_elbo, double tol_rel_obj, int *flags) {
    const double prev = elbo;
    elbo = elbo_new;
    delta = fabs((elbo - prev) / elbo);
    if (buf.size() < cap) buf.push_back(delta);
    else { buf[head] = delta; head = (head + 1) % cap; }
    const size_t n = buf.size();
    double s = 0.0;
    for (size_t k = 0; k < n; k++) s += buf[(head + k) % n];
    mean = s / (double)n;
    std::vector<double> v(buf);
    if (s != s) median = s;   // (an entry that is NaN -- an ELBO of -inf after a finite one -- has no place in an order: neither rule fires)
    else { std::nth_element(v.begin(), v.begin() + n / 2, v.end()); median = v[n / 2]; }
    if (flags && t > 10 * eval_elbo && (mean > 0.5 || median > 0.5)) *flags |= ADVI_FLAG_DIVERGING;
    if (mean < tol_rel_obj) return ADVI_MEAN_CONVERGED;
    if (median < tol_rel_obj) return ADVI_MEDIAN_CONVERGED;
    return t >= iter ? ADVI_MAXIT : 0;
  }
};
