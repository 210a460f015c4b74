// potus_pathfinder.hpp -- Pathfinder on the device: a normal around every iterate of an L-BFGS path, the one with the highest ELBO, draws.
// DESIGN.md section 4o.  Zhang, Carpenter, Gelman and Vehtari (2022), cmdstanr's $pathfinder() with psis_resample = FALSE.
//
// The path is the trajectory k_opt_lbfgs records (potus_optimize.hpp, opt_record) or the caller's: accepted points x_l and gradients
// g_l = grad log p(x_l), l = 0 .. L, rows of [n_paths][rows][Dpad].  s_l = x_l - x_{l-1}, z_l = g_{l-1} - g_l are recomputed from the rows
// wherever they are needed: the history is a list of row numbers, not a copy of vectors.
//
//   k_pf_alpha   one workgroup per path walks l = 1 .. L.  Pair l is kept when s'z > 0 and z'z <= 1e12 s'z; then, with a = z'diag(alpha)z,
//                b = z's, c = s'diag(alpha)^-1 s at alpha_{l-1}, alpha_l = 1 / (a / (b alpha) + z^2 / b - a s^2 / (b c alpha^2)) elementwise;
//                otherwise alpha_l = alpha_{l-1}; alpha_0 = 1.  A thread owns the coordinates tid, tid + 512, ... of every row, the four sums
//                of a pair are one block_sum.  Writes alpha [n_paths][rows][Dpad], the kept flags and (a, b, c).
//   k_pf_elbo    item (path, l), l = 1 .. L; workgroup w of a fixed grid G takes the items w, w + G, ...  Per item: model_setup_lds for the
//                path's model (Mg_all[p / per_ds], as k_opt_lbfgs picks it), pf_fit, then K times pf_before (u, phi, log q), ONE model_pass
//                call site under PlainPolicy, pf_after (the sum of log p - log q).  Everything around the pass is out of line.
//   pf_fit       the history: the last min(J, kept so far) kept pairs up to l, oldest first (S, Z: D x j).  Gram sums S'Z and
//                Z'diag(alpha)Z (one block_sum of 2 j values per column); R = triu(S'Z), E = diag(S'Z),
//                gamma = [[0, -R^-1], [-R^-T, R^-T (E + Z'diag(alpha)Z) R^-1]] (2 j x 2 j); the thin QR of diag(alpha^-1/2) beta,
//                beta = [diag(alpha) Z, S], by modified Gram-Schmidt with one re-orthogonalisation (Q in the workgroup's global working
//                set, R~ in PfSmall; a column whose remainder is below 1e-14 of its norm gives a zero column of Q); L~ = chol(I + R~ gamma R~');
//                mu = x_l + alpha g_l + beta gamma beta' g_l.  A pivot that is not positive and finite: no fit, ELBO_l = -inf.
//   draw         phi = mu + alpha^1/2 (u + Q (L~ - I) Q'u),  log q = -1/2 (sum log alpha + 2 sum log L~_ii + u'u + D log 2 pi).
//   k_pf_draws   item (path, chunk of draws) with l = l* of the path (chosen on the host from the ELBOs: argmax, lowest l on ties): pf_fit
//                once per chunk, then per draw the same pf_before, pass, pf_after, which writes the row [lp__, six NaN, phi], lp and log q.
//                A path without l* (NO_ELBO) gets NaN rows.
//   small state  PfState, in LDS where OptState lives (static_assert against sizeof(TS)): the scalars and the history.  The small matrices do
//                not fit there (16 KB against 1.1 KB; the 2016 design's block leaves 6 KB of the 160 KiB), so they are PfSmall, per workgroup
//                in GLOBAL memory: S'Z, Z'diag(alpha)Z, R^-1, gamma, R~, a product, L~, Q'u and (L~ - I) Q'u, written and read between
//                barriers by the workgroup that owns them.  Sums of more than PT_NRED values go through the model's reduction slots eight at a
//                time (pf_sum).  The kernels are launched with the sampler's LDS size: every design the sampler takes, Pathfinder takes.
//   randomness   Philox4x32-10 as the sampler's, purpose RNG_PATHFINDER = 9, key = the handle's seed.  ELBO draw k of iterate l of path p:
//                counter {i, 9 | k << 8, l, path_offset + p + 1}; final draw n: {i, 9 | 0xFF << 8, draw_offset + n + 1, path_offset + p + 1};
//                coordinates 2 i and 2 i + 1 are the Box-Muller pair.
//   determinism  every length-D sum is a thread-strided partial followed by block_sum, no atomics; an item reads the trajectory, alpha and
//                the flags of its path and writes its own outputs: its bytes depend on neither G nor the other items.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum { RNG_PATHFINDER = 9 };   // after RNG_LAPLACE = 8 (potus_laplace.hpp)
enum { PF_OK = 0, PF_NO_ELBO = 1 };
#define PF_MAX_J 10
#define PF_MAX_N (2 * PF_MAX_J)
#define PF_MAX_K 255

struct PfSmall;
struct PfParams {
  const double *x, *g;     // [n_paths][rows][Dpad] the trajectory
  const int *L;            // [n_paths] its length: rows 0 .. L
  double *alpha;           // [n_paths][rows][Dpad]
  int *kept;               // [n_paths][rows]
  double *abc;             // [n_paths][rows][3]
  double *work;            // [grid][2 J + 4][Dpad]: Q | mu | u | phi | gradient of the pass
  PfSmall *small;          // [grid]
  double *elbo;            // [n_paths][rows], entry l
  const double *u_elbo;    // [n_paths][rows - 1][K][D] or null: the library's normals
  const double *u_draws;   // [n_paths][M][D] or null
  const int *lsel;         // [n_paths] k_pf_draws: l* or 0
  const int *want_l;       // [n_paths] or null: k_pf_elbo also writes mu and log det Sigma of this iterate
  double *mu_out;          // [n_paths][D]
  double *logdet_out;      // [n_paths]
  double *rows_out;        // [n_paths][M][7 + D]
  double *lp, *lq;         // [n_paths][M]
  double *phi_out, *lqw_out, *qtq_out;   // with want_l: [n_paths][M][D], [n_paths][M] the draws of that iterate, [n_paths][PF_MAX_N][PF_MAX_N] Q'Q
  int n_paths, rows, per_ds, J, K, M, chunk, D, Dpad, path_offset, draw_offset;
  unsigned seed_lo, seed_hi;
};
typedef const PfParams AS_C *CPp;

struct PfState {
  double acc, sum_log_alpha, logdet_l, lq;
  int j, bad, ok, fin;
  int p, l, n, n_end;                      // the item and its next draw: what pf_before and pf_after work on (the kernel's loop keeps none of it)
  int hist[PF_MAX_J];                      // newest first: column k of S and Z (oldest first) is pair hist[j - 1 - k]
};
// The small matrices, per workgroup in global memory (the 2016 design leaves 6 KB of the 160 KiB of LDS): written and read between
// barriers by the workgroup that owns them.
struct PfSmall {
  double Lt[PF_MAX_N * PF_MAX_N];          // L~, row stride PF_MAX_N
  double c[PF_MAX_N], d[PF_MAX_N];
  double G1[PF_MAX_J * PF_MAX_J], G2[PF_MAX_J * PF_MAX_J], Rinv[PF_MAX_J * PF_MAX_J];   // S'Z, Z'diag(alpha)Z, R^-1; row stride PF_MAX_J
  double gam[PF_MAX_N * PF_MAX_N], Rt[PF_MAX_N * PF_MAX_N], tmp[PF_MAX_N * PF_MAX_N];   // gamma, R~, a product; row stride PF_MAX_N
};
static_assert(sizeof(PfState) <= sizeof(TS), "Pathfinder's state takes the place of the sampler's transition state in LDS");

// block_sum of N values through the model's PT_NRED reduction slots, eight at a time: the same order of additions as one block_sum<N>
template <int N>
__device__ __forceinline__ void pf_sum(double (&v)[N], ldp red, int tid) {
#pragma unroll
  for (int c = 0; c < N; c += PT_NRED) {
    double w[PT_NRED];
#pragma unroll
    for (int k = 0; k < PT_NRED; k++) w[k] = c + k < N ? v[c + k] : 0.0;
    block_sum(w, red, tid);
#pragma unroll
    for (int k = 0; k < PT_NRED; k++) if (c + k < N) v[c + k] = w[k];
  }
}

struct PfItem {
  CMp M; CPp P; ldp lds, red; PfState AS_L *st;
  gcdp X, Gd, A;         // the path's trajectory rows and alpha_l
  gdp Q, mu, u, phi;
  int D, Dpad, j, tid;
};
__device__ __forceinline__ PfItem pf_item(const DevModel *Mg, const PfParams *Pg, int p_, int l_) {
  PfItem o;
  o.M = (CMp)uni_ptr(Mg); o.P = (CPp)uni_ptr(Pg);
  const int p = (int)uni32((unsigned)p_), l = (int)uni32((unsigned)l_);
  o.lds = (ldp)lds_dyn; o.st = (PfState AS_L *)(o.lds + o.M->lds_doubles); o.red = o.lds + o.M->l_red;
  o.D = o.M->D; o.Dpad = o.P->Dpad; o.tid = threadIdx.x;
  const size_t path = (size_t)p * o.P->rows * o.Dpad;
  o.X = as_g(o.P->x) + path; o.Gd = as_g(o.P->g) + path; o.A = as_g(o.P->alpha) + path + (size_t)l * o.Dpad;
  o.Q = as_g(o.P->work) + (size_t)blockIdx.x * (2 * o.P->J + 4) * o.Dpad;
  o.mu = o.Q + (size_t)(2 * o.P->J) * o.Dpad; o.u = o.mu + o.Dpad; o.phi = o.u + o.Dpad;
  o.j = 0;
  return o;
}

// element i of column k of diag(alpha^-1/2) beta: sqrt(alpha) z for k < j, s / sqrt(alpha) behind
__device__ __forceinline__ double pf_w(const PfItem &o, bool is_z, int h, int i) {   // h: the column's pair
  const double ra = sqrt(o.A[i]);
  gcdp a = (is_z ? o.Gd : o.X) + (size_t)(h - 1) * o.Dpad, b = a + o.Dpad;
  return is_z ? ra * (a[i] - b[i]) : (b[i] - a[i]) / ra;
}

// The normal of iterate l of path p: Q, mu in the workgroup's working set, L~ in LDS, the rest of the small matrices in PfSmall.  Returns 1 when there is one.
__device__ __noinline__ int pf_fit(const DevModel *Mg, const PfParams *Pg, int p_, int l_) {
  const PfItem o = pf_item(Mg, Pg, p_, l_);
  CPp P = o.P;
  PfState AS_L *st = o.st;
  const int p = (int)uni32((unsigned)p_), l = (int)uni32((unsigned)l_);
  const int tid = o.tid, D = o.D, Dpad = o.Dpad, J = P->J;
  ldp red = o.red;
  gcdp X = o.X, Gd = o.Gd, A = o.A;
  PfSmall AS_G *sm = as_g(P->small) + blockIdx.x;
  if (tid == 0) {
    const int AS_G *kept = as_g(P->kept) + (size_t)p * P->rows;
    int cnt = 0;
    for (int i = l; i >= 1 && cnt < J; i--) if (kept[i]) st->hist[cnt++] = i;
    st->j = cnt; st->acc = 0.0; st->bad = 0; st->ok = 1;
  }
  for (int e = tid; e < PF_MAX_N * PF_MAX_N; e += PT_THREADS) sm->Rt[e] = 0.0;
  __syncthreads();
  const int j = opt_uni(st->j), n = 2 * j;
  int hr[PF_MAX_J];                                     // the pairs, oldest first
#pragma unroll
  for (int a = 0; a < PF_MAX_J; a++) hr[a] = a < j ? st->hist[j - 1 - a] : 1;
  {
    double v[1] = {0.0};
    for (int i = tid; i < D; i += PT_THREADS) v[0] += log(A[i]);
    block_sum(v, red, tid);
    if (tid == 0) st->sum_log_alpha = v[0];
  }
  // ---- Gram sums, a column at a time: G1[a][b] = s_a . z_b, G2[a][b] = z_a . alpha z_b
  for (int b = 0; b < j; b++) {
    const int hb = opt_uni(st->hist[j - 1 - b]);
    gcdp gb0 = Gd + (size_t)(hb - 1) * Dpad, gb1 = gb0 + Dpad;
    double v[2 * PF_MAX_J];
#pragma unroll
    for (int a = 0; a < 2 * PF_MAX_J; a++) v[a] = 0.0;
    for (int i = tid; i < D; i += PT_THREADS) {
      const double zb = gb0[i] - gb1[i], azb = A[i] * zb;
#pragma unroll
      for (int a = 0; a < PF_MAX_J; a++) if (a < j) {
        const size_t r0 = (size_t)(hr[a] - 1) * Dpad + i, r1 = r0 + Dpad;
        v[a] += (X[r1] - X[r0]) * zb;
        v[PF_MAX_J + a] += (Gd[r0] - Gd[r1]) * azb;
      }
    }
    pf_sum(v, red, tid);
    if (tid == 0) {
#pragma unroll
      for (int a = 0; a < PF_MAX_J; a++) if (a < j) { sm->G1[a * PF_MAX_J + b] = v[a]; sm->G2[a * PF_MAX_J + b] = v[PF_MAX_J + a]; }
    }
  }
  __syncthreads();
  // ---- R^-1 (upper triangle of S'Z, back substitution) and gamma
  if (tid == 0) {
    for (int c = 0; c < j; c++) {
      for (int r = 0; r < j; r++) sm->Rinv[r * PF_MAX_J + c] = 0.0;
      sm->Rinv[c * PF_MAX_J + c] = 1.0 / sm->G1[c * PF_MAX_J + c];
      for (int r = c - 1; r >= 0; r--) {
        double s = 0.0;
        for (int k = r + 1; k <= c; k++) s += sm->G1[r * PF_MAX_J + k] * sm->Rinv[k * PF_MAX_J + c];
        sm->Rinv[r * PF_MAX_J + c] = -s / sm->G1[r * PF_MAX_J + r];
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < n * n; e += PT_THREADS) {
    const int r = e / n, c = e % n;
    double v = 0.0;
    if (r < j && c >= j) v = -sm->Rinv[r * PF_MAX_J + c - j];
    else if (r >= j && c < j) v = -sm->Rinv[c * PF_MAX_J + r - j];
    else if (r >= j) {
      const int rr = r - j, cc = c - j;
      for (int a = 0; a <= rr; a++)
        for (int b = 0; b <= cc; b++) {
          const double m = sm->G2[min(a, b) * PF_MAX_J + max(a, b)] + (a == b ? sm->G1[a * PF_MAX_J + a] : 0.0);
          v += sm->Rinv[a * PF_MAX_J + rr] * m * sm->Rinv[b * PF_MAX_J + cc];
        }
    }
    sm->gam[r * PF_MAX_N + c] = v;
  }
  __syncthreads();
  // ---- thin QR of W = diag(alpha^-1/2) beta: modified Gram-Schmidt, every column orthogonalised twice against the columns before it
  for (int k = 0; k < n; k++) {
    gdp qk = o.Q + (size_t)k * Dpad;
    const int hk = opt_uni(st->hist[j - 1 - (k < j ? k : k - j)]);
    double w0[1] = {0.0};
    for (int i = tid; i < D; i += PT_THREADS) { const double w = pf_w(o, k < j, hk, i); qk[i] = w; w0[0] += w * w; }
    block_sum(w0, red, tid);
    for (int pass = 0; pass < 2; pass++)
      for (int c = 0; c < k; c++) {
        gcdp qc = o.Q + (size_t)c * Dpad;
        double r[1] = {0.0};
        for (int i = tid; i < D; i += PT_THREADS) r[0] += qc[i] * qk[i];
        block_sum(r, red, tid);
        for (int i = tid; i < D; i += PT_THREADS) qk[i] -= r[0] * qc[i];
        if (tid == 0) sm->Rt[c * PF_MAX_N + k] += r[0];
      }
    double w1[1] = {0.0};
    for (int i = tid; i < D; i += PT_THREADS) w1[0] += qk[i] * qk[i];
    block_sum(w1, red, tid);
    const bool dep = !(w1[0] > 1e-28 * w0[0]);          // the column lies in the span of those before it
    const double nrm = dep ? 0.0 : sqrt(w1[0]), inv = dep ? 0.0 : 1.0 / nrm;
    for (int i = tid; i < D; i += PT_THREADS) qk[i] = dep ? 0.0 : qk[i] * inv;
    if (tid == 0) sm->Rt[k * PF_MAX_N + k] = nrm;
  }
  __syncthreads();
  // ---- L~ = chol(I + R~ gamma R~')
  for (int e = tid; e < n * n; e += PT_THREADS) {
    const int r = e / n, c = e % n;
    double v = 0.0;
    for (int m = r; m < n; m++) v += sm->Rt[r * PF_MAX_N + m] * sm->gam[m * PF_MAX_N + c];
    sm->tmp[r * PF_MAX_N + c] = v;
  }
  __syncthreads();
  for (int e = tid; e < n * n; e += PT_THREADS) {
    const int r = e / n, c = e % n;
    double v = r == c ? 1.0 : 0.0;
    for (int m = c; m < n; m++) v += sm->tmp[r * PF_MAX_N + m] * sm->Rt[c * PF_MAX_N + m];
    sm->Lt[r * PF_MAX_N + c] = v;
  }
  __syncthreads();
  if (tid == 0) {
    int ok = 1;
    double ld = 0.0;
    for (int c = 0; c < n && ok; c++) {
      double dg = sm->Lt[c * PF_MAX_N + c];
      for (int k = 0; k < c; k++) dg -= sm->Lt[c * PF_MAX_N + k] * sm->Lt[c * PF_MAX_N + k];
      if (!(dg > 0.0) || !isfinite(dg)) { ok = 0; break; }
      const double piv = sqrt(dg);
      sm->Lt[c * PF_MAX_N + c] = piv;
      ld += log(piv);
      for (int r = c + 1; r < n; r++) {
        double s = sm->Lt[r * PF_MAX_N + c];
        for (int k = 0; k < c; k++) s -= sm->Lt[r * PF_MAX_N + k] * sm->Lt[c * PF_MAX_N + k];
        sm->Lt[r * PF_MAX_N + c] = s / piv;
      }
    }
    if (!isfinite(st->sum_log_alpha)) ok = 0;
    st->ok = ok; st->logdet_l = 2.0 * ld;
  }
  // ---- mu = x + alpha g + beta gamma beta'g
  gcdp xl = X + (size_t)l * Dpad, gl = Gd + (size_t)l * Dpad;
  {
    double v[PF_MAX_N];
#pragma unroll
    for (int a = 0; a < PF_MAX_N; a++) v[a] = 0.0;
    for (int i = tid; i < D; i += PT_THREADS) {
      const double gi = gl[i], agi = A[i] * gi;
#pragma unroll
      for (int a = 0; a < PF_MAX_J; a++) if (a < j) {
        const size_t r0 = (size_t)(hr[a] - 1) * Dpad + i, r1 = r0 + Dpad;
        v[a] += (Gd[r0] - Gd[r1]) * agi;
        v[PF_MAX_J + a] += (X[r1] - X[r0]) * gi;
      }
    }
    pf_sum(v, red, tid);
    if (tid == 0) {
#pragma unroll
      for (int a = 0; a < PF_MAX_J; a++) if (a < j) { sm->c[a] = v[a]; sm->c[j + a] = v[PF_MAX_J + a]; }
    }
  }
  __syncthreads();
  if (tid < n) {
    double s = 0.0;
    for (int m = 0; m < n; m++) s += sm->gam[tid * PF_MAX_N + m] * sm->c[m];
    sm->d[tid] = s;
  }
  __syncthreads();
  {
    double dz[PF_MAX_J], ds[PF_MAX_J];
#pragma unroll
    for (int a = 0; a < PF_MAX_J; a++) { dz[a] = a < j ? sm->d[a] : 0.0; ds[a] = a < j ? sm->d[j + a] : 0.0; }
    for (int i = tid; i < D; i += PT_THREADS) {
      const double ai = A[i];
      double m = xl[i] + ai * gl[i];
#pragma unroll
      for (int a = 0; a < PF_MAX_J; a++) if (a < j) {
        const size_t r0 = (size_t)(hr[a] - 1) * Dpad + i, r1 = r0 + Dpad;
        m += ai * (Gd[r0] - Gd[r1]) * dz[a] + (X[r1] - X[r0]) * ds[a];
      }
      o.mu[i] = m;
    }
  }
  __syncthreads();
  const int ok = opt_uni(st->ok);
  if (P->want_l && as_c(P->want_l)[p] == l) {
    gdp mo = as_g(P->mu_out) + (size_t)p * D;
    for (int i = tid; i < D; i += PT_THREADS) mo[i] = ok ? o.mu[i] : NAN;
    if (tid == 0) P->logdet_out[p] = ok ? st->sum_log_alpha + st->logdet_l : NAN;
  }
  return ok;
}

// Before a pass: draw `n` of the item (ELBO draw k = n of iterate l, or final draw n): u, phi in the working set, log q in the state.
__device__ __noinline__ void pf_before(const DevModel *Mg, const PfParams *Pg) {
  PfState AS_L *st0 = (PfState AS_L *)((ldp)lds_dyn + ((CMp)uni_ptr(Mg))->lds_doubles);
  const int p = opt_uni(st0->p), l = opt_uni(st0->l), nd = opt_uni(st0->n), fin = opt_uni(st0->fin);
  const PfItem o = pf_item(Mg, Pg, p, l);
  CPp P = o.P;
  PfState AS_L *st = o.st;
  const int tid = o.tid, D = o.D, Dpad = o.Dpad, nq = 2 * opt_uni(st->j);
  PfSmall AS_G *sm = as_g(P->small) + blockIdx.x;
  const double *us = fin ? P->u_draws : P->u_elbo;
  if (us) {
    gcdp src = as_g(us) + (fin ? (size_t)p * P->M + nd : ((size_t)p * (P->rows - 1) + (l - 1)) * P->K + nd) * (size_t)D;
    for (int i = tid; i < D; i += PT_THREADS) o.u[i] = src[i];
  } else {
    const RngKey key{P->seed_lo, P->seed_hi, (uint32_t)(P->path_offset + p + 1)};
    const uint32_t iter = fin ? (uint32_t)(P->draw_offset + nd + 1) : (uint32_t)l, aux = fin ? 0xFFu : (uint32_t)nd;
    for (int i = tid; i < (D + 1) / 2; i += PT_THREADS) {
      double a, b;
      rng_normal_pair(key, iter, RNG_PATHFINDER, aux, (uint32_t)i, a, b);
      o.u[2 * i] = a;
      if (2 * i + 1 < D) o.u[2 * i + 1] = b;
    }
  }
  __syncthreads();
  double v[PF_MAX_N + 1];                               // Q'u and u'u
#pragma unroll
  for (int k = 0; k <= PF_MAX_N; k++) v[k] = 0.0;
  for (int i = tid; i < D; i += PT_THREADS) {
    const double ui = o.u[i];
#pragma unroll
    for (int k = 0; k < PF_MAX_N; k++) if (k < nq) v[k] += o.Q[(size_t)k * Dpad + i] * ui;
    v[PF_MAX_N] += ui * ui;
  }
  pf_sum(v, o.red, tid);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < PF_MAX_N; k++) if (k < nq) sm->c[k] = v[k];
    st->lq = -0.5 * (st->sum_log_alpha + st->logdet_l + v[PF_MAX_N] + (double)D * 1.8378770664093454836);
  }
  __syncthreads();
  if (tid < nq) {                                       // (L~ - I) Q'u
    double s = -sm->c[tid];
    for (int m = 0; m <= tid; m++) s += sm->Lt[tid * PF_MAX_N + m] * sm->c[m];
    sm->d[tid] = s;
  }
  __syncthreads();
  double t[PF_MAX_N];
#pragma unroll
  for (int k = 0; k < PF_MAX_N; k++) t[k] = k < nq ? sm->d[k] : 0.0;
  for (int i = tid; i < D; i += PT_THREADS) {
    double s = o.u[i];
#pragma unroll
    for (int k = 0; k < PF_MAX_N; k++) if (k < nq) s += o.Q[(size_t)k * Dpad + i] * t[k];
    o.phi[i] = o.mu[i] + sqrt(o.A[i]) * s;
  }
  __syncthreads();
}

// After the pass at phi: the ELBO's term, or the draw's row.  Returns whether the item has another draw.
__device__ __noinline__ int pf_after(const DevModel *Mg, const PfParams *Pg, double lp) {
  PfState AS_L *st0 = (PfState AS_L *)((ldp)lds_dyn + ((CMp)uni_ptr(Mg))->lds_doubles);
  const int p = opt_uni(st0->p), l = opt_uni(st0->l), nd = opt_uni(st0->n), fin = opt_uni(st0->fin), n_end = opt_uni(st0->n_end);
  const PfItem o = pf_item(Mg, Pg, p, l);
  CPp P = o.P;
  PfState AS_L *st = o.st;
  const int tid = o.tid, D = o.D;
  if (!fin) {
    if (tid == 0) { if (isfinite(lp)) st->acc += lp - st->lq; else st->bad = 1; }
  } else {
    const size_t at = (size_t)p * P->M + nd;
    gdp row = as_g(P->rows_out) + at * (size_t)(POTUS_N_SAMPLER_COLS + D);
    for (int i = tid; i < D; i += PT_THREADS) row[POTUS_N_SAMPLER_COLS + i] = o.phi[i];
    if (tid < POTUS_N_SAMPLER_COLS) row[tid] = tid == 0 ? lp : NAN;
    if (tid == 0) { P->lp[at] = lp; P->lq[at] = st->lq; }
  }
  __syncthreads();
  if (tid == 0) st->n = nd + 1;
  __syncthreads();
  return nd + 1 < n_end;
}

// For the iterate a caller asked about (want_l), after its ELBO: Q'Q of the fit, and phi and log q of the M draws the iterate would give from the
// caller's (or the library's) final normals -- no model pass.
__device__ __noinline__ void pf_want(const DevModel *Mg, const PfParams *Pg, int p_, int l_) {
  const PfItem o = pf_item(Mg, Pg, p_, l_);
  CPp P = o.P;
  PfState AS_L *st = o.st;
  const int p = (int)uni32((unsigned)p_), tid = o.tid, D = o.D, Dpad = o.Dpad, nq = 2 * opt_uni(st->j), Mn = P->M;
  gdp qq = as_g(P->qtq_out) + (size_t)p * PF_MAX_N * PF_MAX_N;
  for (int a = 0; a < nq; a++) {
    double v[PF_MAX_N];
#pragma unroll
    for (int k = 0; k < PF_MAX_N; k++) v[k] = 0.0;
    for (int i = tid; i < D; i += PT_THREADS) {
      const double qa = o.Q[(size_t)a * Dpad + i];
#pragma unroll
      for (int k = 0; k < PF_MAX_N; k++) if (k < nq) v[k] += o.Q[(size_t)k * Dpad + i] * qa;
    }
    pf_sum(v, o.red, tid);
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < PF_MAX_N; k++) if (k < nq) qq[a * PF_MAX_N + k] = v[k];
    }
  }
  for (int n = 0; n < Mn; n++) {
    if (tid == 0) { st->n = n; st->fin = 1; }
    __syncthreads();
    pf_before(Mg, Pg);
    gdp out = as_g(P->phi_out) + ((size_t)p * Mn + n) * (size_t)D;
    for (int i = tid; i < D; i += PT_THREADS) out[i] = o.phi[i];
    if (tid == 0) P->lqw_out[(size_t)p * Mn + n] = st->lq;
    __syncthreads();
  }
}

__global__ __launch_bounds__(PT_THREADS) void k_pf_alpha(const PfParams *Pg) {
  __shared__ double red_s[PT_NW * 4];
  CPp P = (CPp)Pg;
  ldp red = (ldp)red_s;
  const int p = blockIdx.x, tid = threadIdx.x, D = P->D, Dpad = P->Dpad, rows = P->rows, L = as_c(P->L)[p];
  const size_t path = (size_t)p * rows * Dpad;
  gcdp X = as_g(P->x) + path, Gd = as_g(P->g) + path;
  gdp A = as_g(P->alpha) + path;
  for (int i = tid; i < D; i += PT_THREADS) A[i] = 1.0;
  if (tid == 0) { P->kept[(size_t)p * rows] = 0; for (int k = 0; k < 3; k++) P->abc[(size_t)p * rows * 3 + k] = NAN; }
  for (int l = 1; l <= L; l++) {
    gcdp x0 = X + (size_t)(l - 1) * Dpad, x1 = x0 + Dpad, g0 = Gd + (size_t)(l - 1) * Dpad, g1 = g0 + Dpad;
    gdp a0 = A + (size_t)(l - 1) * Dpad, a1 = a0 + Dpad;
    double v[4] = {0.0, 0.0, 0.0, 0.0};                 // a = z'alpha z, b = z's, c = s's / alpha, z'z
    for (int i = tid; i < D; i += PT_THREADS) {
      const double s = x1[i] - x0[i], z = g0[i] - g1[i], al = a0[i];
      v[0] += z * z * al; v[1] += z * s; v[2] += s * s / al; v[3] += z * z;
    }
    block_sum(v, red, tid);
    const double a = v[0], b = v[1], c = v[2];
    const int keep = opt_uni((b > 0.0 && v[3] <= 1e12 * b) ? 1 : 0);
    for (int i = tid; i < D; i += PT_THREADS) {
      const double s = x1[i] - x0[i], z = g0[i] - g1[i], al = a0[i];
      a1[i] = keep ? 1.0 / (a / (b * al) + z * z / b - a * s * s / (b * c * al * al)) : al;
    }
    if (tid == 0) {
      P->kept[(size_t)p * rows + l] = keep;
      double *o = P->abc + ((size_t)p * rows + l) * 3;
      o[0] = a; o[1] = b; o[2] = c;
    }
  }
}

// The items of a workgroup.  DRAWS = false: item (p, l), l = 1 .. L_p, K ELBO draws.  DRAWS = true: item (p, chunk), draws of l*.
template <bool DRAWS>
__device__ __forceinline__ void pf_items(const DevModel *Mg_all, const PfParams *Pg) {
  CPp P = (CPp)Pg;
  ldp lds = (ldp)lds_dyn;
  const int tid = threadIdx.x, Dpad = P->Dpad, J = P->J, rows = P->rows, Mn = P->M;
  const int per = DRAWS ? (Mn + P->chunk - 1) / P->chunk : rows - 1;
  const long long n_items = (long long)P->n_paths * per;
  double *wk = P->work + (size_t)blockIdx.x * (2 * J + 4) * Dpad;
  const rsrc_t rw = make_rsrc(wk, (unsigned)(2 * J + 4) * (unsigned)Dpad * 8u);
  const unsigned s_phi = 8u * (unsigned)Dpad * (unsigned)(2 * J + 2), s_g = s_phi + 8u * (unsigned)Dpad;
  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int p = (int)(item / per), r = (int)(item % per);
    const int l = DRAWS ? as_c(P->lsel)[p] : r + 1;
    const int n0 = DRAWS ? r * P->chunk : 0, n1 = DRAWS ? min(Mn, n0 + P->chunk) : P->K;
    if (!DRAWS && l > as_c(P->L)[p]) continue;
    const DevModel *Mg = Mg_all + p / P->per_ds;
    CMp M = (CMp)Mg;
    int ok = 0;
    PassStatic pst = model_setup_lds(M, lds);
    if (l >= 1) ok = opt_uni(pf_fit(Mg, Pg, p, l));
    if (!ok) {
      if (DRAWS) {
        const int row = POTUS_N_SAMPLER_COLS + M->D;
        for (int n = n0; n < n1; n++) {
          const size_t at = (size_t)p * Mn + n;
          for (int i = tid; i < row; i += PT_THREADS) P->rows_out[at * row + i] = NAN;
          if (tid == 0) { P->lp[at] = NAN; P->lq[at] = NAN; }
        }
      } else if (tid == 0) P->elbo[(size_t)p * rows + l] = -INFINITY;
      __syncthreads();
      continue;
    }
    if (tid == 0) {
      PfState AS_L *st = (PfState AS_L *)(lds + M->lds_doubles);
      st->p = p; st->l = l; st->n = n0; st->n_end = n1; st->fin = DRAWS ? 1 : 0;
    }
    __syncthreads();
    for (int more = n0 < n1; more;) {
      pf_before(Mg, Pg);
      PlainPolicy pol{rw, rw, s_phi, s_g, {0}};
      const double lp = model_pass(M, lds, pst, pol);
      __syncthreads();
      more = opt_uni(pf_after(Mg, Pg, lp));
    }
    if (!DRAWS && tid == 0) {
      const PfState AS_L *st = (const PfState AS_L *)(lds + M->lds_doubles);
      P->elbo[(size_t)p * rows + l] = st->bad ? -INFINITY : st->acc / (double)P->K;
    }
    __syncthreads();
    if (!DRAWS && P->want_l && P->phi_out && as_c(P->want_l)[p] == l) pf_want(Mg, Pg, p, l);
  }
}

__global__ __launch_bounds__(PT_THREADS) void k_pf_elbo(const DevModel *Mg_all, const PfParams *Pg) { pf_items<false>(Mg_all, Pg); }
__global__ __launch_bounds__(PT_THREADS) void k_pf_draws(const DevModel *Mg_all, const PfParams *Pg) { pf_items<true>(Mg_all, Pg); }
