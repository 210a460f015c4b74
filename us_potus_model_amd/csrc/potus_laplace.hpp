// potus_laplace.hpp -- the Laplace approximation on the device: Hessian at a mode, its Cholesky factor, draws.  DESIGN.md section 4n.
//
// cmdstanr's $laplace(mode =, draws =, jacobian =): the normal approximation N(q^, P^-1) around a mode q^ of log_prob<jacobian>, with
// P = -Hessian.  Draws are x = q^ + L^-T u with P = L L' and u standard normal, so that lp_approx(x) = -1/2 |u|^2 up to the constant
// 1/2 log det P - D/2 log 2 pi, and lp(x) - lp(q^) - lp_approx(x) is the log importance ratio of the draw.
//
//   k_lap_hess     minus the Hessian by central differences of the gradient.  Workgroup w of a mode's G takes the coordinates w, w + G, ...;
//                  per coordinate two model_pass calls under PlainPolicy (the device code of the leapfrog and of k_opt_lbfgs) at
//                  q^ +- h_j e_j, h_j = h max(1, |q^_j|).  Default h = 1e-4, chosen from the 2016 table of profiles/laplace_2016.txt: the identity
//                  (x - q^).(-H)(x - q^) = |u|^2 holds to 4.1e-11, 1.8e-12, 3.2e-11, 3.6e-10 for h = 1e-3 .. 1e-6 (gradient rounding at
//                  lp = -1.17e6 takes over below 1e-4; on the small design, against autograd, 1e-5 is still marginally better).  ONE call site inside a loop of 2 x (the workgroup's coordinates) trips -- plus,
//                  for workgroup 0, one trip at q^ itself for |g|_2 -- and everything after a pass is out of line (lap_after), so the pass
//                  keeps the registers it has in k_logprob_grad.  Row j of Hraw = -(g+ - g-) / (x+ - x-) with the divisor as stored.
//                  jacobian = 0 takes the Jacobian out of each gradient after the pass, as potus_optimize.hpp does.  Working set of a
//                  workgroup: x, g+, g- of Dpad doubles.  Every row is written once, by one workgroup: the bytes do not depend on G.
//   k_lap_sym      P[i][j] = P[j][i] = (Hraw[i][j] + Hraw[j][i]) / 2 in place, one workgroup per pair of 64 x 64 tiles.
//   factor         dense_cholesky_launch (potus_dense.hpp) on a DnParams that describes the mode's own D x LD buffer, its own fail word.
//   k_lap_diag     log det P = 2 sum log L_ii and the smallest pivot min L_ii^2, thread-strided partials and a fixed tree.
//   k_lap_normals  u from Philox4x32-10, purpose RNG_LAPLACE = 8: coordinates 2 i, 2 i + 1 of draw n are the Box-Muller pair of counter
//                  {i, 8, 0, draw_offset + n + 1}, key = the handle's seed (the pairing of potus_simulate_prior).
//   k_lap_norm     lp_approx = -1/2 |u|^2 per draw: thread-strided partials over the coordinates, then a fixed tree.
//   k_lap_solve_*  L' X = U for all draws of a mode, right-looking from the last block of DN_NB = 64 rows up, in panels of LAP_PANEL = 4 blocks:
//                  k_lap_solve_diag back-substitutes the block's rows with L_bb in LDS (one thread per draw), k_lap_solve_update subtracts
//                  X_b L[b rows, columns] from the columns left of the block on v_mfma_f64_16x16x4_f64 (operand layout as in k_dn_cov) --
//                  inside the panel after every block, left of the panel once per panel with the panel's 256 rows (measured against one block
//                  at a time: DESIGN.md section 4n).  A workgroup owns 64 draws x 64 columns, a row of the MFMA's A operand is one draw.  Every sum of a draw runs over k
//                  in a fixed order and an output row of an MFMA depends on its own row of A alone, so a draw's bytes depend on
//                  (matrix, u of the draw) only -- not on the number of draws, draw_offset or the tile the draw lands in.
//   k_lap_rows     rows [lp__ (k_lap_lp), six NaN, q^ + X]: the layout k_write_array and k_tl_scores read.
//   k_lap_lp       lp__ of every row: model_pass under PlainPolicy, Jacobian on -- the device code and bytes of potus_log_prob_grad.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum { RNG_LAPLACE = 8 };   // after RNG_OPT_INITS = 7 (potus_optimize.hpp)
enum { LAP_OK = 0, LAP_NOT_PD = 1, LAP_NOT_FINITE = 2 };

struct LapHessParams {
  const double *mode;    // [n][D] the modes of this launch (blockIdx.y)
  const int *ds;         // [n] the data set of each
  double *work;          // [n][G][3][Dpad]: x, g+, g-
  double *H;             // [n][D][LD]
  double *gnorm;         // [n]
  int G, Dpad, LD, jacobian;
  double h;
};
typedef const LapHessParams AS_C *CLp;

// What follows a pass.  t = 2 c + s: coordinate j = w + c G, s = 0 the pass was at x+ (gradient in slot 1), s = 1 at x- (slot 2): the row is
// written and x[j] restored.  j >= D: the pass was at q^ itself (workgroup 0's last trip): |g|_2.  Then x is set up for trip t + 1.
__device__ __noinline__ void lap_after(const DevModel *Mg, const LapHessParams *Pg, int t_, int ntrip_) {
  CMp M = (CMp)uni_ptr(Mg);
  CLp P = (CLp)uni_ptr(Pg);
  const int t = (int)uni32((unsigned)t_), ntrip = (int)uni32((unsigned)ntrip_);
  const int w = blockIdx.x, mi = blockIdx.y, tid = threadIdx.x, D = M->D, Dpad = P->Dpad, G = P->G;
  ldp lds = (ldp)lds_dyn;
  ldp red = lds + M->l_red;
  gdp x = as_g(P->work) + ((size_t)mi * G + w) * 3 * (size_t)Dpad, gp = x + Dpad, gm = gp + Dpad;
  gcdp q = as_g(P->mode) + (size_t)mi * D;
  const int j = w + (t >> 1) * G, s = t & 1;
  gdp gt = (j < D && s) ? gm : gp;
  if (t >= 0 && !P->jacobian && M->full) {             // log_prob<jacobian = false>: potus_optimize.hpp's removal, at the evaluated point
    const double rho = (lds + M->l_scal)[SC_RHO];
    if (tid == 0) gt[M->o_rho] -= 1.0 - 2.0 * rho;
    __syncthreads();
  }
  if (t >= 0 && j >= D) {
    double v[1] = {0.0};
    for (int i = tid; i < D; i += PT_THREADS) { const double gi = gp[i]; v[0] += gi * gi; }
    block_sum(v, red, tid);
    if (tid == 0) P->gnorm[mi] = sqrt(v[0]);
  } else if (t >= 0 && s) {
    const double qj = q[j], hj = P->h * fmax(1.0, fabs(qj));
    const double xp = qj + hj, xm = qj - hj, den = xp - xm;
    gdp row = as_g(P->H) + ((size_t)mi * D + j) * (size_t)P->LD;
    for (int i = tid; i < D; i += PT_THREADS) row[i] = -(gp[i] - gm[i]) / den;
    if (tid == 0) x[j] = qj;
  }
  const int tn = t + 1;                                  // the point of the next trip
  if (tn < ntrip && tid == 0) {
    const int jn = w + (tn >> 1) * G;
    if (jn < D) {
      const double qj = q[jn], hj = P->h * fmax(1.0, fabs(qj));
      x[jn] = (tn & 1) ? qj - hj : qj + hj;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(PT_THREADS) void k_lap_hess(const DevModel *Mg_all, const LapHessParams *Pg) {
  CLp P = (CLp)Pg;
  const int w = blockIdx.x, mi = blockIdx.y;
  const DevModel *Mg = Mg_all + as_c(P->ds)[mi];
  CMp M = (CMp)Mg;
  ldp lds = (ldp)lds_dyn;
  const PassStatic pst = model_setup_lds(M, lds);
  const int tid = threadIdx.x, D = M->D, Dpad = P->Dpad, G = P->G;
  double *xw = P->work + ((size_t)mi * G + w) * 3 * (size_t)Dpad;
  gdp x = as_g(xw);
  gcdp q = as_g(P->mode) + (size_t)mi * D;
  const rsrc_t rw = make_rsrc(xw, 3u * (unsigned)Dpad * 8u);
  for (int i = tid; i < D; i += PT_THREADS) x[i] = q[i];
  __syncthreads();
  const int ncol = w < D ? (D - w + G - 1) / G : 0;
  const int ntrip = 2 * ncol + (w == 0 ? 1 : 0);        // (workgroup 0's extra trip has j = w + ncol G >= D)
  lap_after(Mg, Pg, -1, ntrip);
  for (int t = 0; t < ntrip; t++) {
    const int j = w + (t >> 1) * G;
    const unsigned slot = (j < D && (t & 1)) ? 2u : 1u;
    PlainPolicy pol{rw, rw, 0u, uni32(8u * (unsigned)Dpad * slot), {0}};   // (the loop counter lives in a vector register across lap_after)
    (void)model_pass(M, lds, pst, pol);
    __syncthreads();
    lap_after(Mg, Pg, t, ntrip);
  }
}

// P = (Hraw + Hraw') / 2 in place: tile pair (I, J), I >= J, by one workgroup.  Both triangles end up with the same bytes.
__global__ __launch_bounds__(256) void k_lap_sym(double *H, int D, int LD) {
  __shared__ double a[DN_NB][DN_NB + 1], b[DN_NB][DN_NB + 1];
  const int I = blockIdx.x, J = blockIdx.y, tid = threadIdx.x;
  if (J > I) return;
  double *A = H + (size_t)blockIdx.z * (size_t)D * (size_t)LD;
  for (int e = tid; e < DN_NB * DN_NB; e += 256) {
    const int i = e >> 6, j = e & 63;
    const int r = I * DN_NB + i, c = J * DN_NB + j, r2 = J * DN_NB + i, c2 = I * DN_NB + j;
    a[i][j] = (r < D && c < D) ? A[(size_t)r * LD + c] : 0.0;        // tile (I, J)
    b[i][j] = (r2 < D && c2 < D) ? A[(size_t)r2 * LD + c2] : 0.0;    // tile (J, I)
  }
  __syncthreads();
  for (int e = tid; e < DN_NB * DN_NB; e += 256) {
    const int i = e >> 6, j = e & 63;
    const int r = I * DN_NB + i, c = J * DN_NB + j, r2 = J * DN_NB + i, c2 = I * DN_NB + j;
    if (r < D && c < D) A[(size_t)r * LD + c] = 0.5 * (a[i][j] + b[j][i]);
    if (I != J && r2 < D && c2 < D) A[(size_t)r2 * LD + c2] = 0.5 * (a[j][i] + b[i][j]);
  }
}

// info[1] = log det P = 2 sum_i log L_ii, info[3] = min_i L_ii^2; one workgroup per matrix, fixed order
__global__ __launch_bounds__(256) void k_lap_diag(const double *Lall, int D, int LD, double *info) {
  __shared__ double rs[256], rm[256];
  const int tid = threadIdx.x;
  const double *L = Lall + (size_t)blockIdx.x * (size_t)D * (size_t)LD;
  double s = 0.0, mn = INFINITY;
  for (int i = tid; i < D; i += 256) { const double d = L[(size_t)i * LD + i]; s += log(d); mn = fmin(mn, d * d); }
  rs[tid] = s; rm[tid] = mn;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) { rs[tid] += rs[tid + h]; rm[tid] = fmin(rm[tid], rm[tid + h]); }
    __syncthreads();
  }
  if (tid == 0) { info[4 * blockIdx.x + 1] = 2.0 * rs[0]; info[4 * blockIdx.x + 3] = rm[0]; }
}

// U [n_draws][LD]: standard normals of draws draw_offset .. draw_offset + n_draws - 1
__global__ __launch_bounds__(256) void k_lap_normals(double *U, int n_draws, int D, int LD, int draw_offset, unsigned seed_lo, unsigned seed_hi) {
  const int npair = (D + 1) / 2;
  const long long total = (long long)n_draws * npair;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int n = (int)(e / npair), i = (int)(e % npair);
    const RngKey key{seed_lo, seed_hi, (uint32_t)(draw_offset + n + 1)};
    double a, b;
    rng_normal_pair(key, 0u, RNG_LAPLACE, 0u, (uint32_t)i, a, b);
    double *u = U + (size_t)n * LD;
    u[2 * i] = a;
    if (2 * i + 1 < D) u[2 * i + 1] = b;
  }
}

// lp_approx[n] = -1/2 |u_n|^2: workgroup per draw, thread t sums coordinates t, t + 256, ..., then a tree -- fixed by D alone
__global__ __launch_bounds__(256) void k_lap_norm(const double *U, int n_draws, int D, int LD, double *lp_approx) {
  __shared__ double rs[256];
  const int tid = threadIdx.x;
  for (int n = blockIdx.x; n < n_draws; n += gridDim.x) {
    const double *u = U + (size_t)n * LD;
    double s = 0.0;
    for (int i = tid; i < D; i += 256) s += u[i] * u[i];
    __syncthreads();
    rs[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) { if (tid < h) rs[tid] += rs[tid + h]; __syncthreads(); }
    if (tid == 0) lp_approx[n] = -0.5 * rs[0];
  }
}

// Block b of L' X = U: x_i = (u_i - sum_{k > i, in the block} L[k][i] x_k) / L[i][i], k descending from the block's last row.
// 64 draws per workgroup, staged in LDS; thread n < 64 solves draw n.  X overwrites U.
__global__ __launch_bounds__(256) void k_lap_solve_diag(const double *L, double *U, int D, int LD, int n_draws, int b) {
  __shared__ double lk[DN_NB][DN_NB + 1], x[DN_NB][DN_NB + 1];
  const int tid = threadIdx.x, r0 = b * DN_NB, nb = min(DN_NB, D - r0), n0 = blockIdx.x * DN_NB;
  for (int e = tid; e < DN_NB * DN_NB; e += 256) {
    const int i = e >> 6, j = e & 63;
    lk[i][j] = (i < nb && j <= i) ? L[(size_t)(r0 + i) * LD + r0 + j] : 0.0;
    x[i][j] = (n0 + i < n_draws && j < nb) ? U[(size_t)(n0 + i) * LD + r0 + j] : 0.0;
  }
  __syncthreads();
  if (tid < DN_NB) {
    const int n = tid;
    for (int i = nb - 1; i >= 0; i--) {
      double s = x[n][i];
      for (int k = nb - 1; k > i; k--) s -= lk[k][i] * x[n][k];
      x[n][i] = s / lk[i][i];
    }
  }
  __syncthreads();
  for (int e = tid; e < DN_NB * DN_NB; e += 256) { const int i = e >> 6, j = e & 63; if (n0 + i < n_draws && j < nb) U[(size_t)(n0 + i) * LD + r0 + j] = x[i][j]; }
}

// U[:, 64 J : 64 J + 64] -= X[:, rows] L[rows, 64 J : 64 J + 64] for the rows of the blocks [b0, b1) -- already solved -- the block columns
// J = cb0 + blockIdx.x left of them and 64 draws (blockIdx.y).  Inside a panel of LAP_PANEL blocks the update after each block stops at the
// panel's left edge (b1 = b0 + 1); everything left of the panel gets the whole panel at once (up to 256 k per element, 64 at a time
// through LDS): U left of a panel is read and written once per panel, not once per block.  Four waves; wave w owns draws 16 w .. 16 w + 15 of the
// tile and the four 16-column blocks.  MFMA: lane l feeds A[l & 15][l >> 4] = X[draw 16 w + (l & 15)][k] and B[l >> 4][l & 15] = L[row k][column],
// and holds D[(l >> 4) + 4 v][l & 15].  Rows beyond D and draws beyond n_draws enter as zeros.
#define LAP_PANEL 4
__global__ __launch_bounds__(256) void k_lap_solve_update(const double *L, double *U, int D, int LD, int n_draws, int b0, int b1, int cb0) {
  __shared__ double xa[DN_NB][DN_NB + 1], lb[DN_NB][DN_NB + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, m = lane & 15, kk = lane >> 4;
  const int c0 = (cb0 + (int)blockIdx.x) * DN_NB, n0 = (int)blockIdx.y * DN_NB;
  dn_d4 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; cb++) acc[cb] = dn_d4{0.0, 0.0, 0.0, 0.0};
  for (int b = b0; b < b1; b++) {                          // k ascending: a fixed order for every draw
    const int r0 = b * DN_NB, nb = min(DN_NB, D - r0);
    __syncthreads();
    for (int e = tid; e < DN_NB * DN_NB; e += 256) {
      const int i = e >> 6, j = e & 63;
      xa[i][j] = (n0 + i < n_draws && j < nb) ? U[(size_t)(n0 + i) * LD + r0 + j] : 0.0;   // [draw][k]
      lb[i][j] = i < nb ? L[(size_t)(r0 + i) * LD + c0 + j] : 0.0;                         // [k][column]: c0 + j < 64 b0 <= D
    }
    __syncthreads();
#pragma unroll 4
    for (int t0 = 0; t0 < DN_NB; t0 += 4) {
      const double av = xa[16 * w + m][t0 + kk];
#pragma unroll
      for (int cb = 0; cb < 4; cb++) acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, lb[t0 + kk][16 * cb + m], acc[cb], 0, 0, 0);
    }
  }
#pragma unroll
  for (int cb = 0; cb < 4; cb++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int n = n0 + 16 * w + kk + 4 * v, j = c0 + 16 * cb + m;
      if (n < n_draws) U[(size_t)n * LD + j] -= acc[cb][v];
    }
}

// rows[n] = [NaN (lp__: k_lap_lp), six NaN, q^ + X_n]; ok = 0: the mode has no factor, every entry NaN
__global__ __launch_bounds__(256) void k_lap_rows(const double *X, const double *mode, int n_draws, int D, int LD, int ok, double *rows, double *lp, double *lp_approx) {
  const int row = POTUS_N_SAMPLER_COLS + D;
  for (int n = blockIdx.x; n < n_draws; n += gridDim.x) {
    double *r = rows + (size_t)n * row;
    const double *x = X + (size_t)n * LD;
    for (int i = threadIdx.x; i < row; i += 256) r[i] = (i < POTUS_N_SAMPLER_COLS || !ok) ? NAN : mode[i - POTUS_N_SAMPLER_COLS] + x[i - POTUS_N_SAMPLER_COLS];
    if (!ok && threadIdx.x == 0) { lp[n] = NAN; lp_approx[n] = NAN; }
  }
}

// lp__ of the rows of one mode, with the mode's model: k_logprob_grad's pass on a row's point; the gradient goes to the workgroup's scratch
__global__ __launch_bounds__(PT_THREADS) void k_lap_lp(const DevModel *Mg, double *rows, int n_draws, double *gscratch, int Dpad, double *lp) {
  CMp M = (CMp)Mg;
  ldp lds = (ldp)lds_dyn;
  const PassStatic pst = model_setup_lds(M, lds);
  const int D = M->D, row = POTUS_N_SAMPLER_COLS + D;
  const rsrc_t rg = make_rsrc(gscratch + (size_t)blockIdx.x * Dpad, 8u * D);
  for (int n = blockIdx.x; n < n_draws; n += gridDim.x) {
    PlainPolicy pol{make_rsrc(rows + (size_t)n * row + POTUS_N_SAMPLER_COLS, 8u * D), rg, 0u, 0u, {0}};
    const double v = model_pass(M, lds, pst, pol);
    if (threadIdx.x == 0) { rows[(size_t)n * row] = v; lp[n] = v; }
    __syncthreads();
  }
}
