// potus_optimize.hpp -- the posterior mode on the device: batched L-BFGS, one workgroup per path.  DESIGN.md section 4k.
//
// cmdstanr's $optimize(): the mode of log_prob<jacobian = true> (the MAP point on the unconstrained scale) or, with jacobian = 0 --
// CmdStan's default for optimisation -- of log_prob<jacobian = false> (the penalised MLE).  Every scale of this model is data and every
// prior a standard normal on the non-centred coordinates, so the no-mode variant is strictly log-concave (-Hessian >= I) and the full
// variant adds the two AR(1) scalars only.  The device's advantage is the batch: the run dates of a timeline, the folds of a
// cross-validation, the simulated data sets of an SBC are the chains of one handle, and k_opt_lbfgs gives each of them -- or several
// starts of each -- its mode in ONE launch, with no host round trip per iteration.
//
//   k_opt_lbfgs   path p = workgroup p of PT_THREADS; model Mg_all[p / per_ds] as k_run_ds picks a chain's model.  The objective is
//                 model_pass under PlainPolicy, the device code of the leapfrog; it has ONE call site, inside a bounded loop, and the
//                 line search and the iteration are a state machine around it (its state lives in LDS while the pass runs, so the
//                 pass keeps the registers it has in k_logprob_grad).  jacobian = 0 takes the Jacobian out AFTER the pass: it lives in
//                 one coordinate, lp -= log(0.02) + log(rho) + log1p(-rho), g[rho] -= 1 - 2 rho (potus_model.hpp phase B).
//   L-BFGS        history m (1..20), two-loop recursion, initial scaling s'y / y'y of the newest pair; a pair with s'y <= 0 is skipped;
//                 a direction that is no ascent direction resets the history to steepest ascent.  Working set of a path in global
//                 memory, (2 m + 5) vectors of Dpad doubles: x g | x g (current and trial, swapped on acceptance) | direction | s[m] | y[m].
//   line search   strong Wolfe (c1 = 1e-4, c2 = 0.9): bracketing with secant extrapolation of the directional derivative (between 1.1
//                 and 10 times the last step), then zoom with the secant of the two end derivatives kept inside the middle 80 % of the
//                 bracket, bisection where that fails; a non-finite trial becomes the bracket's far end, i.e. shrinks the step.  First
//                 trial of the first iteration init_alpha, afterwards 1.  At most OPT_LS_MAX evaluations per search; a search that fails
//                 with a history is repeated once along the gradient (so an iteration takes at most 2 OPT_LS_MAX), a search that fails
//                 along the gradient ends the path (LSFAIL) at the last accepted point -- every accepted step increases the objective,
//                 so that is the best point seen.
//   termination   CmdStan 2.24's rules after each accepted step, strict <, in the order of the codes (a tolerance of 0 switches a rule
//                 off).  The loop runs at most 100 + 21 iter passes whatever the data: 100 start attempts, one pass for the start,
//                 20 per iteration with one search; a path that has used them -- iterations that repeat their search can, before
//                 `iter` iterations are done -- ends MAXIT.
//   determinism   every dot product is a thread-strided partial sum followed by block_sum (fixed order, no atomics), and no path reads
//                 what another writes: a path's bytes are a function of (model, start, options) alone.
//   starts        q0 [n][D] tried once (non-finite value or gradient: INIT for that path alone), else U(-r, r) with the handle's
//                 init_radius, up to 100 attempts as k_init retries.  Philox4x32-10 as the sampler's, counter = {coordinate,
//                 RNG_OPT_INITS | attempt << 8, PT_ITER_PRE, path_offset + p + 1}, key = the handle's seed: the purpose is new, so no
//                 stream of the sampler is reused, and path_offset makes a path's bytes independent of the batching.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum { RNG_OPT_INITS = 7 };   // after RNG_PRIOR = 6 (potus_nuts.hpp)
enum { OPT_ABSF = 1, OPT_RELF, OPT_ABSGRAD, OPT_RELGRAD, OPT_ABSX, OPT_MAXIT, OPT_LSFAIL, OPT_INIT };
#define OPT_MAX_HISTORY 20
#define OPT_LS_MAX 20
#define OPT_INIT_ATTEMPTS 100
enum { OPT_V_DIR = 4, OPT_V_S = 5 };   // vector slots after the two (x, g) pairs; y[m] follows s[m]

struct OptParams {
  const double *q0;      // [n_paths][D] or null
  double *work;          // [n_paths][2 m + 5][Dpad]
  double *rows;          // [n_paths][7 + D]: lp__, six NaN, the point (the `draws` block of k_write_array[_ds])
  double *lp, *gnorm;    // [n_paths]
  int *info;             // [n_paths][3]: code, iterations, gradient evaluations
  int per_ds;            // paths per data set (n_paths on a plain handle)
  int m, iter, jacobian, path_offset, Dpad;
  double init_alpha, tol_obj, tol_rel_obj, tol_grad, tol_rel_grad, tol_param, radius;
  unsigned seed_lo, seed_hi;
  double *traj_x, *traj_g;   // [n_paths][traj_rows][Dpad] or null: the accepted (x_l, g_l), l = 0 .. iterations (potus_pathfinder.hpp)
  int traj_rows;
};

// The state machine's memory, in the LDS that the sampler kernels use for their transition state (after DevModel::lds_doubles).
// stage 0: the pass evaluates a start; 1: a trial step of the line search.  (lo, hi): the bracket of the search, lo its best point so far.
#define OPT_FIELDS_D(X) X(f) X(f0) X(gd0) X(alpha) X(gamma) X(gnorm) X(a_lo) X(h_lo) X(d_lo) X(a_hi) X(h_hi) X(d_hi)
#define OPT_FIELDS_I(X) X(stage) X(it) X(nev) X(ls_ev) X(hn) X(head) X(cur) X(hi_ok) X(zoom) X(retried) X(attempt)
struct OptScal {
#define X(n) double n;
  OPT_FIELDS_D(X)
#undef X
#define X(n) int n;
  OPT_FIELDS_I(X)
#undef X
};
struct OptState {
  OptScal s;
  double rho[OPT_MAX_HISTORY], al[OPT_MAX_HISTORY];   // 1 / s'y of the pairs; the two-loop recursion's coefficients
};
static_assert(sizeof(OptState) <= sizeof(TS), "the optimiser's state takes the place of the sampler's transition state in LDS");
__device__ __forceinline__ OptScal opt_load(const OptState AS_L *st) {
  OptScal s;
#define X(n) s.n = st->s.n;
  OPT_FIELDS_D(X) OPT_FIELDS_I(X)
#undef X
  return s;
}
__device__ __forceinline__ void opt_store(OptState AS_L *st, const OptScal &s) {   // by thread 0, followed by a barrier
#define X(n) st->s.n = s.n;
  OPT_FIELDS_D(X) OPT_FIELDS_I(X)
#undef X
}

__device__ __forceinline__ int opt_uni(int v) { return (int)__builtin_amdgcn_readfirstlane((unsigned)v); }

// dot products of a path's vectors: thread-strided partials, then block_sum
template <int N>
__device__ __forceinline__ void opt_dots(gcdp a, gcdp (&b)[N], int D, ldp red, int tid, double (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = 0.0;
  for (int i = tid; i < D; i += PT_THREADS) {
    const double ai = a[i];
#pragma unroll
    for (int k = 0; k < N; k++) v[k] += ai * b[k][i];
  }
  block_sum(v, red, tid);
}

// direction = H g by the two-loop recursion over the hn newest pairs (slot head - 1 is the newest); returns g . direction.
// Every thread owns the elements tid, tid + PT_THREADS, ... of every vector, so only the sums need the workgroup.
__device__ __forceinline__ double opt_direction(gdp W, int Dpad, int D, int m, int g_slot, OptState AS_L *st, int hn, int head, double gamma, ldp red, int tid) {
  gdp dir = W + (size_t)OPT_V_DIR * Dpad;
  gcdp g = W + (size_t)g_slot * Dpad;
  for (int i = tid; i < D; i += PT_THREADS) dir[i] = g[i];
  for (int k = 0; k < hn; k++) {                      // newest to oldest
    const int idx = (head - 1 - k + 2 * m) % m;
    gcdp s = W + (size_t)(OPT_V_S + idx) * Dpad, y = W + (size_t)(OPT_V_S + m + idx) * Dpad;
    gcdp bs[1] = {s};
    double v[1];
    opt_dots(gcdp(dir), bs, D, red, tid, v);
    const double a = st->rho[idx] * v[0];
    if (tid == 0) st->al[idx] = a;
    for (int i = tid; i < D; i += PT_THREADS) dir[i] -= a * y[i];
  }
  if (hn > 0) for (int i = tid; i < D; i += PT_THREADS) dir[i] *= gamma;
  for (int j = 0; j < hn; j++) {                      // oldest to newest (al[] was written before the block_sum barriers in between)
    const int idx = (head - hn + j + 2 * m) % m;
    gcdp s = W + (size_t)(OPT_V_S + idx) * Dpad, y = W + (size_t)(OPT_V_S + m + idx) * Dpad;
    gcdp by[1] = {y};
    double v[1];
    opt_dots(gcdp(dir), by, D, red, tid, v);
    const double c = st->al[idx] - st->rho[idx] * v[0];
    for (int i = tid; i < D; i += PT_THREADS) dir[i] += c * s[i];
  }
  gcdp bg[1] = {g};
  double v[1];
  opt_dots(gcdp(dir), bg, D, red, tid, v);
  return v[0];
}

typedef const OptParams AS_C *COp;   // read through scalar loads, like the model descriptor

struct OptPath { CMp M; ldp lds; OptState AS_L *st; ldp red; gdp W; double *Wp; int D, Dpad, m; RngKey key; };
__device__ __forceinline__ OptPath opt_path(CMp M, COp P, int p) {
  OptPath o;
  o.M = M; o.lds = (ldp)lds_dyn; o.st = (OptState AS_L *)(o.lds + M->lds_doubles); o.red = o.lds + M->l_red;
  o.D = M->D; o.Dpad = P->Dpad; o.m = P->m;
  o.Wp = P->work + (size_t)p * (2 * o.m + 5) * o.Dpad;
  o.W = as_g(o.Wp);
  o.key = RngKey{P->seed_lo, P->seed_hi, (uint32_t)(P->path_offset + p + 1)};
  return o;
}

// What follows a pass: the state machine's step.  Kept out of line, as the sampler keeps its once-per-transition work, so that the register
// allocator sees the pass alone in the kernel's loop.  lp: the pass's value at the trial point.  Returns 0 to go on, else the path's code.
__device__ __noinline__ int opt_step(const DevModel *Mg, const OptParams *Pg, int p_, double lp) {
  CMp M = (CMp)uni_ptr(Mg);
  COp P = (COp)uni_ptr(Pg);
  const OptPath o = opt_path(M, P, (int)uni32((unsigned)p_));
  ldp lds = o.lds, red = o.red;
  OptState AS_L *st = o.st;
  gdp W = o.W;
  const RngKey key = o.key;
  const int tid = threadIdx.x, D = o.D, Dpad = o.Dpad, m = o.m;
  const bool own_start = P->q0 != nullptr;
  const int cur = opt_uni(st->s.cur);
  const int x_slot = 2 * cur, g_slot = 2 * cur + 1, xt_slot = 2 * (1 - cur), gt_slot = xt_slot + 1;
  gdp x = W + (size_t)x_slot * Dpad, g = W + (size_t)g_slot * Dpad, xt = W + (size_t)xt_slot * Dpad, gt = W + (size_t)gt_slot * Dpad;
  gdp dir = W + (size_t)OPT_V_DIR * Dpad;
  if (!P->jacobian && M->full) {                       // log_prob<jacobian = false>: the Jacobian terms of stan:62-63 taken out again
    const double rho = (lds + M->l_scal)[SC_RHO];
    lp -= log(0.02) + log(rho) + log1p(-rho);
    if (tid == 0) gt[M->o_rho] -= 1.0 - 2.0 * rho;
    __syncthreads();
  }
  const int stage = opt_uni(st->s.stage);
  double v[3] = {0.0, 0.0, 0.0};                      // g_t . d, g_t . g_t, non-finite entries of g_t
  for (int i = tid; i < D; i += PT_THREADS) {
    const double gi = gt[i];
    v[0] += stage ? gi * dir[i] : 0.0;
    v[1] += gi * gi;
    v[2] += isfinite(gi) ? 0.0 : 1.0;
  }
  block_sum(v, red, tid);
  const double dh = v[0], gg = v[1];
  const bool fin = isfinite(lp) && v[2] == 0.0 && isfinite(dh);
  OptScal s = opt_load(st);                           // every thread takes the same decisions from the same numbers
  __syncthreads();
  s.nev += 1;
  // what to do next: 0 = another trial at s.alpha, 1 = accept the trial, 2 = the search failed; 3 = the start is good, 4 = another start,
  // 5 = no finite start, 6 = the start has a zero gradient; 7 = the search failed for good
  int act = 0;
  if (stage == 0) {
    if (fin) act = gg > 0.0 ? 3 : 6;
    else act = (own_start || s.attempt + 1 >= OPT_INIT_ATTEMPTS) ? 5 : 4;
  } else {
    const double alpha = s.alpha;
    const bool armijo_fails = lp < s.f0 + 1e-4 * alpha * s.gd0;
    const bool wolfe = fabs(dh) <= 0.9 * s.gd0;
    bool expand = false;
    if (!s.zoom) {
      if (!fin) { s.a_hi = alpha; s.hi_ok = 0; s.zoom = 1; }
      else if (armijo_fails || (s.ls_ev > 0 && lp <= s.h_lo)) { s.a_hi = alpha; s.h_hi = lp; s.d_hi = dh; s.hi_ok = 1; s.zoom = 1; }
      else if (wolfe) act = 1;
      else if (dh <= 0.0) {
        s.a_hi = s.a_lo; s.h_hi = s.h_lo; s.d_hi = s.d_lo; s.hi_ok = 1;
        s.a_lo = alpha; s.h_lo = lp; s.d_lo = dh; s.zoom = 1;
      } else {                                        // still rising: go further out
        double an = s.d_lo > dh ? alpha + (alpha - s.a_lo) * dh / (s.d_lo - dh) : 10.0 * alpha;
        an = fmin(fmax(an, 1.1 * alpha), 10.0 * alpha);
        s.a_lo = alpha; s.h_lo = lp; s.d_lo = dh;
        s.alpha = an;
        expand = true;
      }
    } else {
      if (!fin) { s.a_hi = alpha; s.hi_ok = 0; }
      else if (armijo_fails || lp <= s.h_lo) { s.a_hi = alpha; s.h_hi = lp; s.d_hi = dh; s.hi_ok = 1; }
      else if (wolfe) act = 1;
      else {
        if (dh * (s.a_hi - s.a_lo) <= 0.0) { s.a_hi = s.a_lo; s.h_hi = s.h_lo; s.d_hi = s.d_lo; s.hi_ok = 1; }
        s.a_lo = alpha; s.h_lo = lp; s.d_lo = dh;
      }
    }
    s.ls_ev += 1;
    if (act == 0 && s.ls_ev >= OPT_LS_MAX) act = (s.hn > 0 && !s.retried) ? 2 : 7;
    if (act == 0 && !expand) {                        // next trial inside the bracket
      const double w = s.a_hi - s.a_lo;
      double t = 0.5;
      if (s.hi_ok && (s.d_lo - s.d_hi) * w > 0.0) {
        const double ts = s.d_lo / (s.d_lo - s.d_hi);
        if (ts > 0.0) t = fmin(fmax(ts, 0.1), 0.9);
      }
      s.alpha = s.a_lo + t * w;
    }
  }
  act = opt_uni(act);                                 // (the same in every thread: branches with barriers inside are taken on a scalar)
  if (act == 5) return OPT_INIT;
  if (act == 7) return OPT_LSFAIL;

  bool new_search = false;                            // begin a line search along dir from the current point
  if (act == 4) {
    s.attempt += 1;
    for (int i = tid; i < D; i += PT_THREADS) xt[i] = P->radius * (2.0 * rng_uniform(key, PT_ITER_PRE, RNG_OPT_INITS, (uint32_t)s.attempt, (uint32_t)i) - 1.0);
  } else if (act == 6) {
    s.cur = 1 - cur; s.f = lp; s.gnorm = 0.0;
    if (tid == 0) opt_store(st, s);
    __syncthreads();
    return OPT_ABSGRAD;
  } else if (act == 3) {                              // the start becomes the current point; first direction: the gradient
    s.cur = 1 - cur; s.f = lp; s.gnorm = sqrt(gg); s.stage = 1; s.hn = 0; s.head = 0;
    for (int i = tid; i < D; i += PT_THREADS) dir[i] = gt[i];
    s.gd0 = gg; s.alpha = P->init_alpha;
    new_search = true;
  } else if (act == 2) {                              // once more, along the gradient
    s.hn = 0; s.retried = 1;
    gcdp bg[1] = {gcdp(g)};
    double w1[1];
    opt_dots(gcdp(g), bg, D, red, tid, w1);
    for (int i = tid; i < D; i += PT_THREADS) dir[i] = g[i];
    s.gd0 = w1[0]; s.alpha = s.it > 0 ? 1.0 : P->init_alpha;
    new_search = true;
  } else if (act == 1) {
    double w3[3] = {0.0, 0.0, 0.0};                   // s'y, y'y, s's with s = x_t - x, y = g - g_t (the pair of -f)
    for (int i = tid; i < D; i += PT_THREADS) {
      const double si = xt[i] - x[i], yi = g[i] - gt[i];
      w3[0] += si * yi; w3[1] += yi * yi; w3[2] += si * si;
    }
    block_sum(w3, red, tid);
    if (w3[0] > 0.0) {                                 // (a skipped pair leaves the oldest one in its slot)
      gdp sv = W + (size_t)(OPT_V_S + s.head) * Dpad, yv = W + (size_t)(OPT_V_S + m + s.head) * Dpad;
      for (int i = tid; i < D; i += PT_THREADS) { sv[i] = xt[i] - x[i]; yv[i] = g[i] - gt[i]; }
      if (tid == 0) st->rho[s.head] = 1.0 / w3[0];
      s.gamma = w3[0] / w3[1];
      s.head = (s.head + 1) % m; s.hn = min(s.hn + 1, m);
    }
    const double df = fabs(lp - s.f), fprev = s.f, dx = sqrt(w3[2]);
    s.f = lp; s.cur = 1 - cur; s.it += 1; s.gnorm = sqrt(gg); s.retried = 0;
    double gd = opt_direction(W, Dpad, D, m, gt_slot, st, opt_uni(s.hn), opt_uni(s.head), s.gamma, red, tid);
    if (!(gd > 0.0) || !isfinite(gd)) {               // no ascent direction: steepest ascent, empty history
      s.hn = 0;
      for (int i = tid; i < D; i += PT_THREADS) dir[i] = gt[i];
      gd = gg;
    }
    const double eps = 2.220446049250313e-16;
    int c = 0;
    if (df < P->tol_obj) c = OPT_ABSF;
    else if (df / fmax(fmax(fabs(s.f), fabs(fprev)), P->tol_obj) < P->tol_rel_obj * eps) c = OPT_RELF;
    else if (s.gnorm < P->tol_grad) c = OPT_ABSGRAD;
    else if (gd / fmax(fabs(s.f), P->tol_obj) < P->tol_rel_grad * eps) c = OPT_RELGRAD;
    else if (dx < P->tol_param) c = OPT_ABSX;
    else if (s.it >= P->iter) c = OPT_MAXIT;
    c = opt_uni(c);
    if (c) { if (tid == 0) opt_store(st, s); __syncthreads(); return c; }
    s.gd0 = gd; s.alpha = 1.0;
    new_search = true;
  }
  if (new_search) {
    s.f0 = s.f; s.a_lo = 0.0; s.h_lo = s.f; s.d_lo = s.gd0; s.a_hi = 0.0; s.h_hi = 0.0; s.d_hi = 0.0;
    s.hi_ok = 0; s.zoom = 0; s.ls_ev = 0;
  }
  if (act != 4) {                                     // the next trial point: current + alpha * direction, into the other pair
    const int c2 = opt_uni(s.cur);
    gcdp xc = W + (size_t)(2 * c2) * Dpad;
    gdp xn = W + (size_t)(2 * (1 - c2)) * Dpad;
    const double a = s.alpha;
    for (int i = tid; i < D; i += PT_THREADS) xn[i] = xc[i] + a * dir[i];
  }
  if (tid == 0) opt_store(st, s);
  __syncthreads();
  return 0;
}

// The trajectory, for a caller that gave buffers for it: a step that accepted a point (the start included) has flipped `cur` and left the
// point in the current pair; it becomes row `it` of the path.  Out of line and behind a scalar test, so potus_optimize's loop is the pass and opt_step.
__device__ __noinline__ void opt_record(const DevModel *Mg, const OptParams *Pg, int p_, int cur_before_) {
  CMp M = (CMp)uni_ptr(Mg);
  COp P = (COp)uni_ptr(Pg);
  const int p = (int)uni32((unsigned)p_), cur_before = (int)uni32((unsigned)cur_before_);
  const OptPath o = opt_path(M, P, p);
  const int cur = opt_uni(o.st->s.cur), l = opt_uni(o.st->s.it), tid = threadIdx.x, D = o.D, Dpad = o.Dpad;
  if (cur == cur_before || l >= P->traj_rows) return;
  gcdp x = o.W + (size_t)(2 * cur) * Dpad, g = x + Dpad;
  const size_t at = ((size_t)p * P->traj_rows + l) * Dpad;
  gdp tx = as_g(P->traj_x) + at, tg = as_g(P->traj_g) + at;
  for (int i = tid; i < D; i += PT_THREADS) { tx[i] = x[i]; tg[i] = g[i]; }
}

__global__ __launch_bounds__(PT_THREADS) void k_opt_lbfgs(const DevModel *Mg_all, const OptParams *Pg) {
  COp P = (COp)Pg;
  const int p = blockIdx.x;
  const DevModel *Mg = Mg_all + p / P->per_ds;
  CMp M = (CMp)Mg;
  const OptPath o = opt_path(M, P, p);
  ldp lds = o.lds;
  const PassStatic pst = model_setup_lds(M, lds);
  OptState AS_L *st = o.st;
  gdp W = o.W;
  const int tid = threadIdx.x, D = o.D, Dpad = o.Dpad;
  const rsrc_t rw = make_rsrc(o.Wp, (unsigned)(2 * o.m + 5) * (unsigned)Dpad * 8u);

  if (tid == 0) opt_store(st, OptScal{});
  for (int i = tid; i < D; i += PT_THREADS)            // cur = 0: the trial pair is slots 2, 3
    W[(size_t)2 * Dpad + i] = P->q0 ? as_g(P->q0)[(size_t)p * D + i] : P->radius * (2.0 * rng_uniform(o.key, PT_ITER_PRE, RNG_OPT_INITS, 0u, (uint32_t)i) - 1.0);
  __syncthreads();

  int code = 0;
  const long long max_pass = (long long)OPT_INIT_ATTEMPTS + (long long)(OPT_LS_MAX + 1) * P->iter;
  for (long long pass = 0; pass < max_pass && !code; pass++) {
    const int xt_slot = 2 * (1 - opt_uni(st->s.cur));
    PlainPolicy pol{rw, rw, 8u * (unsigned)Dpad * (unsigned)xt_slot, 8u * (unsigned)Dpad * (unsigned)(xt_slot + 1), {0}};
    const double lp = model_pass(M, lds, pst, pol);
    code = opt_uni(opt_step(Mg, Pg, p, lp));
    if (P->traj_x) opt_record(Mg, Pg, p, 1 - xt_slot / 2);
  }
  if (!code) code = OPT_MAXIT;                          // every pass is used up

  // ---- results: the current point (INIT: NaN), as the row k_write_array[_ds] reads
  const int cur = opt_uni(st->s.cur), nev = st->s.nev, it = st->s.it;
  const bool none = code == OPT_INIT;
  const bool uncounted = none || code == OPT_LSFAIL;    // opt_step returns these two before it stores the pass it has just counted
  gcdp xf = W + (size_t)(2 * cur) * Dpad;
  double *row = P->rows + (size_t)p * (POTUS_N_SAMPLER_COLS + D);
  const double lpf = none ? NAN : st->s.f;
  for (int i = tid; i < D; i += PT_THREADS) row[POTUS_N_SAMPLER_COLS + i] = none ? NAN : xf[i];
  if (tid < POTUS_N_SAMPLER_COLS) row[tid] = tid == 0 ? lpf : NAN;
  if (tid == 0) {
    P->lp[p] = lpf; P->gnorm[p] = none ? NAN : st->s.gnorm;
    P->info[3 * p] = code; P->info[3 * p + 1] = it; P->info[3 * p + 2] = uncounted ? nev + 1 : nev;
  }
}
