// potus_loo_mm_rules.hpp -- the sequential rules of moment matching for PSIS-LOO (potus_loo_mm.hpp, potus_loo_moment_match in
// potus_hmc.hip), stated once for the host.  DESIGN.md section 4q.
//
// Paananen, Piironen, Buerkner, Vehtari (2021), as loo's loo_moment_match runs it without its covariance step.  Per poll: while
// k > k_threshold and fewer than max_iters steps have been accepted, try T1 (match the mean); if it is rejected try T2 (match mean and
// marginal variance); if that is rejected too, stop.  A candidate is accepted iff its k' < k, so a NaN k' is rejected and any finite k'
// is accepted after k = inf.  The polls of a call advance in lockstep rounds, one candidate per active poll and round; each poll's
// decisions depend on its own k's alone.  The header compiles on its own with a C++ compiler (tests/test_loo_mm_host.py): no HIP header is
// needed.  tests/loo_mm_ref.py restates the loop in Python; the tests hold the two against each other.
#pragma once
#include <math.h>

enum { LMM_NONE = 0, LMM_T1 = 1, LMM_T2 = 2 };                                       // the candidate a poll evaluates next
enum { LMM_RUNNING = 0, LMM_BELOW = 1, LMM_MAXIT = 2, LMM_REJECTED = 3 };             // why a poll stopped (info_out[.][4])
#define LMM_NINFO 6   // info_out per poll: accepted T1, accepted T2, rounds evaluated, split done, stop reason, reserved

// loo's default: k-hat up to min(1 - 1 / log10 S, 0.7) is good
inline double lmm_default_threshold(long long S) { return fmin(1.0 - 1.0 / log10((double)S), 0.7); }

struct LmmPoll {
  double k = NAN;        // the k of the accepted map so far
  int n_t1 = 0, n_t2 = 0, rounds = 0, stop = LMM_RUNNING, next = LMM_NONE;
  int accepted() const { return n_t1 + n_t2; }
  // what the loop's head decides: the next candidate, or the reason to stop
  void head(double thr, int max_iters) {
    if (!(k > thr)) { stop = LMM_BELOW; next = LMM_NONE; }
    else if (accepted() >= max_iters) { stop = LMM_MAXIT; next = LMM_NONE; }
    else next = LMM_T1;
  }
  // k0: the k of plain PSIS.  Returns the first candidate (LMM_NONE: the poll does not enter the loop).
  int start(double k0, double thr, int max_iters) {
    k = k0; n_t1 = n_t2 = rounds = 0; stop = LMM_RUNNING;
    head(thr, max_iters);
    return next;
  }
  // k_new: the k of the candidate `next`.  Returns 1 when it is accepted (the caller keeps its map and weights), 0 otherwise; `next` is
  // the candidate of the following round, LMM_NONE when the poll has stopped.
  int feed(double k_new, double thr, int max_iters) {
    rounds++;
    if (k_new < k) {
      if (next == LMM_T1) n_t1++; else n_t2++;
      k = k_new;
      head(thr, max_iters);
      return 1;
    }
    if (next == LMM_T1) next = LMM_T2;
    else { stop = LMM_REJECTED; next = LMM_NONE; }
    return 0;
  }
};
