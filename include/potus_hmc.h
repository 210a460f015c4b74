/*
 * potus_hmc.h -- C ABI of libpotus_hmc.so, the MI355X-native HMC/NUTS sampler for the
 * posterior defined by scripts/model/poll_model_2020.stan (and the
 * poll_model_2020_no_mode_adjustment.stan variant) of TheEconomist/us-potus-model.
 *
 * What each entry point replaces in the reference
 * -----------------------------------------------
 * The reference has no FFI: the R scripts hand the `data` list to CmdStan through
 * files and a process boundary:
 *
 *   scripts/model/final_2016.R:475-514   data <- list(...)            -> potus_data
 *   scripts/model/final_2016.R:532       cmdstan_model(..., compile)  -> potus_create
 *   scripts/model/final_2016.R:533-541   model$sample(data, seed, chains, iter_warmup,
 *                                        iter_sampling, refresh)      -> potus_run (chunked)
 *   scripts/model/final_2016.R:543       rstan::read_stan_csv(files)  -> potus_get_draws /
 *                                                                        potus_write_array /
 *                                                                        potus_write_stan_csv
 *   scripts/model/final_2016.R:556,...   rstan::extract(out, pars=)   -> potus_write_array
 *   (same call sites: final_2012.R:558-569, final_2008.R:562-573; the commented rstan
 *    surface at final_2016.R:525-529 and scripts/deprecated/R/Refactored/poll_run_v9.R:387-390)
 *
 * Conventions
 * -----------
 *  - plain C, no C++/torch types; every function returns an int status (0 = ok) and
 *    the message of the last failure is available from potus_last_error().
 *  - the caller owns every buffer it passes; inputs are copied at potus_create and no
 *    caller pointer is retained.  Device memory, streams and kernels live behind the
 *    integer handle.
 *  - indices inside potus_data are 1-based int32 exactly as in the Stan `data{}` block
 *    (poll_model_2020.stan:1-41); matrices are column-major.
 *  - all arithmetic is fp64.
 *  - the `_R` entry points take only int* / double* / char** so that R's .C() can call
 *    them (R passes every argument by pointer and ignores return values, so they also
 *    write *status).
 */
#ifndef POTUS_HMC_H
#define POTUS_HMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POTUS_VARIANT_FULL 0    /* scripts/model/poll_model_2020.stan */
#define POTUS_VARIANT_NO_MODE 1 /* scripts/model/poll_model_2020_no_mode_adjustment.stan */

/* status codes */
#define POTUS_OK 0
#define POTUS_ERR_ARG 1      /* bad argument / Stan data-block constraint violated */
#define POTUS_ERR_DEVICE 2   /* HIP runtime failure or no gfx950 device */
#define POTUS_ERR_INIT 3     /* no finite initial point after 100 attempts, or a user's initial point without a finite
                                log density and gradient (it is tried once; Stan: "Rejecting initial value") */
#define POTUS_ERR_STATE 4    /* call order / handle state */
#define POTUS_ERR_IO 5
#define POTUS_ERR_UNSUPPORTED 6
#define POTUS_ERR_STEPSIZE 7 /* base_hmc::init_stepsize ran the step size to 0 or beyond 1e7 (Stan throws there) */
#define POTUS_ERR_WATCHDOG 8 /* the workgroups of a chain's cluster were not resident together (GPU shared with
                                another process?): the launch gave up instead of hanging; the handle is dead */

/* The Stan data block (poll_model_2020.stan:1-41) as a C struct.  For the no-mode
 * variant the four poll_mode_* / poll_pop_* pointers, M, Pop, sigma_m, sigma_pop and
 * sigma_e_bias and the unadjusted_* vectors are ignored (as Stan ignores extra list
 * entries) and may be NULL / 0. */
typedef struct potus_data {
  int32_t N_national_polls, N_state_polls, T, S, P, M, Pop;
  const int32_t *state;               /* [N_state_polls]    1..S   (stan:9)  */
  const int32_t *day_state;           /* [N_state_polls]    1..T   (stan:10) */
  const int32_t *day_national;        /* [N_national_polls] 1..T   (stan:11) */
  const int32_t *poll_state;          /* [N_state_polls]    1..P   (stan:12) */
  const int32_t *poll_national;       /* [N_national_polls] 1..P   (stan:13) */
  const int32_t *poll_mode_state;     /* 1..M    (stan:14) */
  const int32_t *poll_mode_national;  /* 1..M    (stan:15) */
  const int32_t *poll_pop_state;      /* 1..Pop  (stan:16) */
  const int32_t *poll_pop_national;   /* 1..Pop  (stan:17) */
  const int32_t *n_democrat_national; /* (stan:18) */
  const int32_t *n_two_share_national;
  const int32_t *n_democrat_state;
  const int32_t *n_two_share_state;
  const double *unadjusted_national;  /* in [0,1] (stan:22) */
  const double *unadjusted_state;     /* in [0,1] (stan:23) */
  const double *mu_b_prior;           /* [S] (stan:28) */
  const double *state_weights;        /* [S] (stan:29) */
  double sigma_c, sigma_m, sigma_pop;
  double sigma_measure_noise_national, sigma_measure_noise_state, sigma_e_bias;
  const double *state_covariance_0;   /* [S*S] column-major, symmetric PD (stan:37) */
  double random_walk_scale, mu_b_T_scale, polling_bias_scale;
  int32_t variant;                    /* POTUS_VARIANT_* */
} potus_data;

/* Sampler options: the argument surface of cmdstanr's $sample() as used at
 * final_2016.R:533-541 plus the CmdStan 2.24 defaults it implies.
 * ALWAYS start from potus_default_opts(): fields are appended over time (metric_storage came with library version 0.4 in what used
 * to be tail padding, pooled_metric with 0.5), and a struct filled field by field by a caller built against an older header leaves them undefined;
 * potus_version() names the version the header must match. */
typedef struct potus_opts {
  int32_t chains;          /* chains run by THIS handle                                  */
  int32_t chain_id_offset; /* global id of this handle's first chain minus 1; chain c of
                              the handle uses RNG stream chain_id_offset + c + 1, so the
                              draws do not depend on how chains are split over GPUs       */
  int32_t num_warmup;      /* iter_warmup   (final_2016.R:538) */
  int32_t num_samples;     /* iter_sampling (final_2016.R:539) */
  int32_t max_depth;       /* 10 */
  int32_t init_buffer, term_buffer, window; /* 75, 50, 25; each >= 0 (rescaled to 15 % / 75 % / 10 % of num_warmup when
                                               20 <= num_warmup < their sum, as windowed_adaptation does) */
  double delta, gamma, kappa, t0;           /* 0.8, 0.05, 0.75, 10; 0 < delta < 1, the other three finite and > 0 */
  double stepsize;         /* 1.0; finite and > 0 */
  double init_radius;      /* 2.0 : inits ~ U(-2,2) on the unconstrained scale; finite and >= 0.
                              potus_create refuses a value outside these ranges (CmdStan 2.24's argument bounds) with
                              POTUS_ERR_ARG, before it touches the device. */
  uint64_t seed;           /* 1843 (final_2016.R:535) */
  int32_t device;          /* HIP device ordinal */
  int32_t save_warmup;     /* 0 */
  int32_t cus_per_chain;   /* compute units (workgroups) cooperating on one chain: 1 = one workgroup per
                              chain (best throughput with >= 64 chains), 2..32 = a cluster per chain
                              (lowest latency with few chains; chains * cus_per_chain <= CUs of the device),
                              0 = choose from {16, 8, 4, 1} by what fits (10-14 for
                              9-12 chains, as two clusters each, and 1 with two workgroups per chain for 65-128 chains: see twin).  Draws are reproducible bit for bit
                              for a given value; different values differ in floating-point summation order. */
  int32_t metric;          /* POTUS_METRIC_DIAG (CmdStan's default, what final_2016.R:533-541 runs) or
                              POTUS_METRIC_DENSE (metric = "dense_e": stan::mcmc::dense_e_metric + covar_adaptation,
                              BASELINE configs[4]) */
  int32_t twin;            /* cluster mode, diagonal metric: 1 = TWO clusters of cus_per_chain workgroups per chain, one per
                              end of the NUTS trajectory -- the doublings that go forward and those that go backward are
                              integrated at the same time (2 * chains * cus_per_chain <= CUs of the device); 0 = one
                              cluster; -1 = the library decides when it also chooses the cluster size (cus_per_chain = 0):
                              two clusters if they fit.  Same algorithm, RNG streams and arithmetic: the draws are the
                              same bytes as with one cluster of the same size.  With cus_per_chain = 1 the "cluster" is one
                              workgroup: two workgroups per chain (2 * chains <= resident workgroups of the device; what
                              the library picks for 65-128 chains on 256 compute units).  Every form with more than one
                              workgroup per chain needs ALL its workgroups resident together, i.e. the GPU to itself: beside
                              another process the launch ends with POTUS_ERR_WATCHDOG after ~1-3 s and the handle is dead (ask
                              for twin = 0, cus_per_chain = 1 on a shared GPU). */
  int32_t metric_storage;  /* dense metric only: POTUS_STORAGE_F64 (Stan's) or POTUS_STORAGE_F32 -- the adapted covariance is
                              rounded to fp32 and THAT matrix is the metric: its Cholesky factor (fp64) draws the momenta, the
                              leapfrog multiplies with it (fp64 accumulation), so the sampler stays exact while the matrix pass
                              of every leapfrog streams 2 D^2 bytes instead of 4 D^2.  A declared deviation from Stan, which
                              keeps the covariance in fp64; same memory per chain.  With pooled_metric
                              the handle's ONE matrix is kept in fp32 beside its fp64 factor and the pooled pass streams 4 D^2
                              bytes per round instead of 8 D^2. */
  int32_t pooled_metric;   /* dense metric only, 0 (Stan's: every chain adapts its own covariance), 1 or 2 (as 1, but every window end is finished by
                              the host, which may pool over several handles and GPUs first: potus_dense_pool_window).  1: at every window end the draws of ALL
                              chains of the handle form ONE regularised covariance -- covar_adaptation::learn_covariance applied to the
                              pooled sample of chains x n draws -- and ONE Cholesky factor (library version 0.5).  A leaf round then streams
                              one D x D matrix once for every chain (M^-1 times a D x (chains x right-hand sides) block on the fp64 matrix
                              cores) instead of one triangle per chain, and the handle keeps two matrices instead of one per chain.  A
                              declared deviation from Stan / CmdStan, whose chains are separate processes and cannot pool (SURVEY.md
                              section 7.3-5, section 8 f4); the sampler stays exact for the metric it uses.  fp64 storage only. */
  int32_t reserved_;       /* (keeps the struct a multiple of 8 bytes; set by potus_default_opts) */
} potus_opts;
#define POTUS_METRIC_DIAG 0
#define POTUS_METRIC_DENSE 1
#define POTUS_STORAGE_F64 0
#define POTUS_STORAGE_F32 1

/* per-draw sampler columns, in CmdStan order */
#define POTUS_N_SAMPLER_COLS 7 /* lp__,accept_stat__,stepsize__,treedepth__,n_leapfrog__,divergent__,energy__ */

const char *potus_version(void);
int potus_last_error(char *buf, int len);
void potus_default_opts(potus_opts *o);

/* Number of unconstrained parameters D and of columns of one full output row
 * (7 sampler + D constrained parameters + transformed parameters + generated
 * quantities; 43 360 for the 2016 data). Pure host arithmetic, no device needed. */
int potus_num_params(const potus_data *d, int *D);
int potus_num_columns(const potus_data *d, int *n_cols);
/* Column names in CmdStan CSV order ("raw_mu_b.3.17" style, column-major).  Writes at
 * most n_names pointers into a caller array of char[name_len] rows. */
int potus_column_name(const potus_data *d, int col, char *buf, int len);

/* Validate data (Stan's declared bounds), build the three scaled Cholesky factors
 * (transformed data, stan:42-55), upload everything, allocate chain state. */
int potus_create(const potus_data *d, const potus_opts *o, int *handle);
int potus_destroy(int handle);
/* Compute units (workgroups) per chain the handle actually runs with (cus_per_chain = 0 resolved). */
int potus_cus_per_chain(int handle, int *k);
/* clusters per chain of the handle: 2 when it runs the two ends of the trajectory on a cluster each (potus_opts.twin),
 * 1 otherwise */
int potus_clusters_per_chain(int handle, int *n);
/* How potus_create resolves cus_per_chain = 0 and twin = -1, as pure functions of the sizes (no device needed; the reference has
 * no counterpart: CmdStan runs one process per chain, scripts/model/final_2016.R:533-541 `parallel_chains`).
 * potus_plan_cus_per_chain: the first plan for the workgroups per chain (potus_create may still double it when a member's polls
 * do not fit its LDS); one_workgroup_ok = 0 for models beyond the one-workgroup kernels (T > 256 or > 2 048 polls);
 * *lowered_for_twin = 1 when 10-14 was chosen instead of 16 so that a second cluster per chain fits.
 * potus_plan_sides: 1 or 2 clusters (K > 1) / workgroups (K = 1) per chain; resident_per_cu = workgroups of the kernel a compute
 * unit holds (1 for these kernels on gfx950). */
int potus_plan_cus_per_chain(int chains, int T, int n_cus, int cus_per_chain, int twin, int metric, int one_workgroup_ok, int *K, int *lowered_for_twin);
int potus_plan_sides(int chains, int K, int n_cus, int resident_per_cu, int cus_per_chain, int twin, int metric, int *sides);
/* twin mode: leapfrogs counted in the trajectories (n_leapfrog__ summed, = potus_total_leapfrogs) and leaves each side has
 * integrated, those of speculative subtrees that were dropped included -- what the second cluster costs and buys */
int potus_twin_stats(int handle, long long *counted, long long *run_backward, long long *run_forward);

/* Parity hook: log-density (with Jacobians, constants dropped as `~` does) and its
 * gradient for n points of the unconstrained space, evaluated by the same device
 * code the leapfrog uses.  q: [n][D], lp: [n], grad: [n][D] (host pointers). */
int potus_log_prob_grad(int handle, const double *q, int n, double *lp, double *grad);

/* Initial values ~ U(-r,r) with retry (CmdStan semantics), then the initial
 * step-size search.  Must be called once before potus_run. Optional user inits:
 * q0 [chains][D] or NULL; a row of q0 whose log density or gradient is not finite
 * ends the call with POTUS_ERR_INIT. */
int potus_init(int handle, const double *q0);

/* Advance every chain by n_iter NUTS transitions (warmup transitions adapt).
 * Blocks until done.  R calls this in chunks of `refresh` iterations. */
int potus_run(int handle, int n_iter);

/* The same for several handles at once: all launches are issued before any is waited for, so the
 * handles of different GPUs (shards of one posterior, BASELINE configs[2]) or of different posteriors on
 * one GPU (the 2008 / 2012 / 2016 backtests, configs[3]) run concurrently under a single host thread --
 * R has only one.  No reference counterpart: cmdstanr gets its concurrency from one OS process per chain
 * (final_2016.R:536 parallel_chains).  Handles that cannot be co-resident on their device run in turn. */
int potus_run_many(const int *handles, int n_handles, int n_iter);

/* Progress / accounting. */
int potus_iterations_done(int handle, int *n);
int potus_total_leapfrogs(int handle, long long *n); /* sum over chains and iterations so far */
int potus_chain_status(int handle, int *status /*[chains]*/, int *n_divergent /*[chains]*/);

/* Adaptation result per chain: step size and diagonal inverse metric (dense metric: its diagonal). */
int potus_get_adaptation(int handle, double *stepsize /*[chains]*/, double *inv_metric /*[chains][D]*/);
/* Dense metric only: the D x D inverse metric of one chain of the handle (row-major = column-major, it is symmetric). */
int potus_get_dense_metric(int handle, int chain, double *inv_metric /*[D][D]*/);

/* Saved draws on the unconstrained scale: out[chain][iter][7 + D] (host pointer).
 * n_saved = num_samples (+ num_warmup when save_warmup). */
int potus_get_draws(int handle, double *out, int *n_saved);

/* Device pointer of the same array (for RCCL all-gather through torch); the buffer
 * stays owned by the handle. */
int potus_draws_device_ptr(int handle, void **dptr, long long *n_doubles);

/* write_array: constrained parameters, transformed parameters (stan:70-113) and
 * generated quantities (stan:134-140) for every saved draw, restricted to the columns
 * [col_begin, col_end) of the full CmdStan row (0-based, including the 7 sampler
 * columns).  out[iter][chain][col_end-col_begin] -- the as.array(stanfit) layout. */
int potus_write_array(int handle, int col_begin, int col_end, double *out);
/* The same rows written into DEVICE memory of the handle's GPU (e.g. the data_ptr() of a torch tensor that an RCCL
 * all-gather then sends: the draws-of-interest never visit the host). */
int potus_write_array_device(int handle, int col_begin, int col_end, void *out_device);
/* rstan::extract(out, pars)[[1]] (final_2016.R:556, :708) as R stores it, filled in place in ONE pass: `out` = a column-major matrix
 * [rows, col_end - col_begin] whose row chain_global * n_saved + iteration holds a draw -- chains merged chain after chain, the handles' chains in the order
 * listed.  out = NULL: only *rows_out (the draws the handles hold) is set, to size the result; otherwise rows must equal it.  This is what the .Call()
 * wrapper R/src/potus_call.c hands an allocMatrix'ed result to (long vectors welcome); the .C() path returns [iteration][chain][column] rows that the R shim
 * must permute -- two more copies of the block. */
int potus_extract_matrix(const int *handles, int n_handles, int col_begin, int col_end, double *out, long long rows, long long *rows_out);

/* One CmdStan-format CSV per chain (<dir>/<basename>-<chain>.csv) readable by
 * rstan::read_stan_csv (final_2016.R:543). */
int potus_write_stan_csv(int handle, const char *dir, const char *basename);

/* Posterior summaries the run scripts build from extract(out, "predicted_score") (final_2016.R:708-762 state and
 * national intervals, :799-823 electoral-college simulation), computed on the device from the saved draws of
 * all chains of the handle (pooled; any number of draws).  Cell order of state_out: t + T*s (CmdStan's column-major
 * predicted_score[T,S]); quantiles are R's default (type 7); the national vote is weighted.mean(score, state_weights).
 *   state_out [T*S][4] = low (2.5 %), high (97.5 %), mean, P(score > 0.5)
 *   natl_out  [T][4]   = the same for the state_weights-weighted national vote of each draw
 *   ev_out    [T][5]   = mean, median, high, low, P(>= 270) of sum_s ev[s] 1[score > 0.5]      (ev: [S]) */
int potus_posterior_summary(int handle, const double *ev, double *state_out, double *natl_out, double *ev_out);
/* The same over the pooled draws of several handles of one posterior (its chains spread over several samplers or
 * GPUs: potus_run_many); runs on the first handle's GPU. */
int potus_posterior_summary_many(const int *handles, int n_handles, const double *ev, double *state_out, double *natl_out,
                                 double *ev_out);
/* Backtest scores of final_2016.R:925-945 (final_2012.R:918-931, final_2008.R:922-935) from state_out: with p_s =
 * P(score > 0.5) of state s on `day` (1-based; 0 = last day) and won[s] in {0,1} the outcome,
 * out[3] = EV-weighted Brier score, unweighted Brier score, states called correctly (round(p) == won). */
int potus_backtest_scores(const double *state_out, int T, int S, int day, const double *ev, const int *won, double *out);

/* Cross-chain diagnostics on the device: rank-normalised split R-hat and bulk ESS (Vehtari et al. 2021; the definitions bench.py's
 * ESS/s uses) of the columns [col_begin, col_end) of the output row, over the pooled chains of several handles of ONE posterior
 * (equal numbers of saved draws).  The reference has no counterpart (final_2016.R:543-556 never looks at a diagnostic); the
 * all-gather of BASELINE.json's north_star exists "to pool draws for R-hat / ESS".  rhat_out, ess_bulk_out: [col_end - col_begin].
 * Warm-up rows saved with save_warmup = 1 are left out, as rstan::monitor / extract() leave them out; at most 512 chains pooled; a
 * column that holds a NaN or an infinite draw gets NaN for both, a constant column NaN as in `posterior`. */
int potus_diagnostics(const int *handles, int n_handles, int col_begin, int col_end, double *rhat_out, double *ess_bulk_out);
/* The same for a block that already sits in DEVICE memory of GPU `device`: block[draw][chain][column] -- the layout
 * potus_write_array_device produces and an RCCL all-gather of it keeps.  rhat_out, ess_bulk_out: host arrays [n_cols]. */
int potus_diagnostics_device(int device, const void *block, long long n_draws, int n_chains, int n_cols, double *rhat_out, double *ess_bulk_out);

/* ---- the posterior summary table: what fit$summary() / print(stanfit) / rstan::monitor show, for any column ----
 * What the run scripts tabulate right after extract() (final_2016.R:556-705: mean_low_high of mu_b, mean +- 1.96 sd of mu_c, mu_m, mu_pop and
 * polling_bias, the means of e_bias), without the draws visiting the host.  Per column of [col_begin, col_end) a row of
 * POTUS_MONITOR_NSTATS + n_probs doubles over the pooled post-warm-up draws:
 *   0 mean   1 sd (ddof = 1)   2 mad = 1.4826 median|x - median(x)|   3 mcse_mean = sd / sqrt(ess_mean)
 *   4 rhat and 5 ess_bulk, exactly potus_diagnostics' values   6 ess_tail (posterior::ess_tail: the smaller ESS of the split indicators
 *   1[x <= Q(x, 0.05)], 1[x <= Q(x, 0.95)])   7 ess_mean (Geyer's ESS of the split draws, not rank-normalised)   8... R's type-7 quantiles at probs.
 * mean, sd, mad and the quantiles are over ALL draws; slots 4-7 over the split draws (an odd number of draws per chain drops each chain's middle
 * one).  A column with a NaN or an infinite draw: NaN in every slot.  A constant column: mean and quantiles the value, sd = mad = 0, slots 3-7
 * NaN.  Fewer than four draws per half chain: the three ESS and mcse_mean NaN.  n_probs is 0 to 16, every prob finite and in [0, 1].
 * potus_monitor pools as potus_diagnostics does (one posterior, equal counts, warm-up rows left out, at least four post-warm-up draws per chain, at
 * most 512 chains, handles of other GPUs by peer copies) and works the column range in blocks whose gathered rows and transposed columns stay
 * within 256 MB, so the whole output row can be asked for in one call.  Sums run in a fixed order: the same draws give the same bytes however
 * the chains are spread over handles or the range over blocks. */
#define POTUS_MONITOR_NSTATS 8
int potus_monitor(const int *handles, int n_handles, int col_begin, int col_end, const double *probs, int n_probs,
                  double *out /*[col_end - col_begin][POTUS_MONITOR_NSTATS + n_probs]*/);
/* The same for a block [draw][chain][column] that already sits in DEVICE memory of GPU `device` (every row counts); out: host, [n_cols][8 + n_probs]. */
int potus_monitor_device(int device, const void *block, long long n_draws, int n_chains, int n_cols, const double *probs, int n_probs, double *out);

/* Online convergence check for a host loop that advances the sampler in chunks ("online R-hat-based early
 * stop"): rank-normalised split R-hat and bulk ESS of lp__ and mu_b[:, T] (what predicted_score[T, :], the quantity the scripts report, is a
 * monotone map of: final_2016.R:708-762) over the post-warm-up draws saved so far by the pooled chains of the handles.  *converged = 1 when
 * every R-hat is below rhat_below and every bulk ESS is at least ess_at_least (fewer than four draws: 0, no error).  The sampler itself never
 * looks at the flag: the draws up to that point are those of an uninterrupted run.  Stopping on it is a DEVIATION from Stan / the reference,
 * which always run iter_sampling iterations (final_2016.R:539): the host has to ask (argument rhat_stop of the R shim's and the
 * Python host's sample functions). */
int potus_check_convergence(const int *handles, int n_handles, double rhat_below, double ess_at_least, int *converged, double *rhat_max, double *ess_bulk_min);

/* Kernel timing of the most recent potus_run, measured with HIP events on the
 * sampler's own stream: elapsed milliseconds and leapfrogs executed in it. */
int potus_last_run_timing(int handle, double *ms, long long *leapfrogs);

/* Dense metric only: milliseconds spent in the matrix passes (k_dn_matvec: M^-1 times the momenta of a leaf, HIP events on
 * the sampler's stream), their number, the bytes of matrix they streamed (active chains x D x LD x 8 each) and the
 * number of leaf rounds, since potus_create. */
int potus_dense_timing(int handle, double *matvec_ms, long long *passes, long long *bytes, long long *rounds);
/* Dense metric only: what the window ends of the warm-up (covar_adaptation::learn_covariance, then base_hmc::init_stepsize) have
 * cost since potus_create: milliseconds in the covariance, in the blocked Cholesky factorisation and in the step-size search,
 * and the number of window ends. */
int potus_dense_adapt_timing(int handle, double *cov_ms, double *chol_ms, double *init_stepsize_ms, int *window_ends);
/* potus_opts.pooled_metric = 2: the pooled window end in two halves, so that the HOST can pool further -- over the handles of a process, and through an
 * all-reduce (RCCL) over the GPUs of a node (us_potus_model_amd/parallel.py: pool_window_moments, sampler.run_pooled).
 * potus_run / potus_run_many stop after the transition that ends a window (potus_iterations_done says where; a further potus_run before the finish is
 * POTUS_ERR_STATE).  potus_dense_pool_window: *pending = 1 then; *count = the draws behind the handle's moments (chains x window length); *mean_dev and
 * *m2_dev = DEVICE pointers to the handle's mean [D] and M2 = sum of the centred outer products [D rows of *ld doubles, both triangles].  The host
 * replaces M2 by the pooled one (Chan's update: M2 += count (mean - pooled mean)(mean - pooled mean)', then the sum over all handles and ranks) and
 * calls potus_dense_pool_finish with the pooled count N: M^-1 = N/(N+5) M2/(N-1) + 1e-3 5/(N+5) I, its Cholesky factor, base_hmc::init_stepsize.
 * With one handle and nothing done in between, finish(count) is exactly pooled_metric = 1. */
int potus_dense_pool_window(int handle, int *pending, double *count, void **mean_dev, void **m2_dev, long long *ld);
int potus_dense_pool_finish(int handle, double n_total);
/* Dense metric only, verification hook (as potus_log_prob_grad is for the gradient): is the factor L the momentum draw solves
 * with the Cholesky factor of the inverse metric the leapfrog multiplies with?  For n_probe standard-normal vectors x,
 * M^-1 x by the sampler's own matrix pass against L (L' x) by plain kernels over the factor, and the momentum draw's blocked
 * back substitution L' p = u multiplied back:
 *   out[0] = max ||L L' x - M^-1 x|| / ||M^-1 x||,   out[1] = ||L' p - u|| / ||u||.
 * Only BETWEEN runs of an initialised handle whose last window end succeeded (POTUS_ERR_STATE otherwise): the check uses the
 * sampler's own scratch vectors (momentum, temporaries) and round descriptors of every chain, which the next potus_run re-arms;
 * its passes are not part of potus_dense_timing's counts. */
int potus_dense_check(int handle, int chain, int n_probe, double *out /*[2]*/);

/* ---- simulation-based calibration (Talts et al. 2018; DESIGN.md "Simulation-based calibration") ----
 * Many data sets in one handle: after potus_create and before potus_init, give n_datasets outcome vectors of the handle's polls
 * ([n][N_state_polls] and [n][N_national_polls], caller's order, 0 <= y <= n_two_share); everything else in the data is shared
 * (the data sets' models differ only in `pd` -- except on the handles of potus_set_datasets_ex below, whose data sets may also
 * have poll sizes, a mu_b_prior and a mu_b_T_scale of their own).
 * Chain c fits data set c / (chains / n_datasets).  Needs chains % n_datasets == 0, one workgroup per chain (cus_per_chain = 1,
 * twin = 0) and the diagonal metric.  Per-chain calls (potus_get_draws, potus_write_array[_device], potus_chain_status,
 * potus_get_adaptation, potus_draws_device_ptr) work unchanged; calls that pool all chains (potus_posterior_summary[_many],
 * potus_diagnostics, potus_check_convergence, potus_extract_matrix, potus_write_stan_csv, potus_loo, potus_log_lik_device, potus_outcomes, potus_monitor, potus_scenario) refuse with
 * POTUS_ERR_STATE.  A chain
 * whose initialisation or step-size search fails does not fail potus_init / potus_run: potus_chain_status reports it, the
 * iteration and saved-draw counts are those of the other chains. */
int potus_set_datasets(int handle, int n_datasets, const int32_t *n_democrat_state, const int32_t *n_democrat_national);
/* ---- the forecast timeline: the run dates of a campaign as the data sets of one handle ----
 * potus_set_datasets with more that may differ between the data sets: the poll outcomes AND sizes ([n][N_state_polls], [n][N_national_polls];
 * a NULL array = the handle's own values for every data set; n_two_share = 0 = this data set has not seen the poll: it adds 0 to the log
 * density, its noise coordinate keeps its N(0,1) prior), mu_b_prior [n][S] and mu_b_T_scale [n] (> 0), each or both NULL = the handle's.
 * Preconditions and refusals are potus_set_datasets': between potus_create and potus_init, one workgroup per chain, diagonal metric,
 * chains % n_datasets == 0, 0 <= n_democrat <= n_two_share per data set.  Every data set gets a model of its own; with a prior or a scale
 * given also its own transformed data, built by the code potus_create uses: chain c of the handle holds the bytes of a stand-alone handle on
 * that data set's data with chain_id_offset = c.  potus_write_array[_device] build every row with the chain's own model.
 * potus_sbc_ranks, potus_constrain and potus_simulate_prior work with the handle's one model and return POTUS_ERR_UNSUPPORTED on such a
 * handle; the pooled calls refuse it as they refuse potus_set_datasets'. */
int potus_set_datasets_ex(int handle, int n_datasets, const int32_t *n_democrat_state, const int32_t *n_democrat_national,
                          const int32_t *n_two_share_state, const int32_t *n_two_share_national,
                          const double *mu_b_prior /*[n][S] or NULL*/, const double *mu_b_T_scale /*[n] or NULL*/);
/* ---- prior sensitivity by refit: the settings of a grid of prior scales as the data sets of one handle ----
 * potus_set_datasets_ex with one more thing that may differ between the data sets: the nine hand-set scales of potus_data, scales
 * [n][POTUS_N_SCALES] in the order sigma_c, sigma_m, sigma_pop, sigma_measure_noise_national, sigma_measure_noise_state, sigma_e_bias,
 * random_walk_scale, mu_b_T_scale, polling_bias_scale; NULL = potus_set_datasets_ex.  It is a superset of that call, so one handle can hold
 * run dates x settings.  Giving both mu_b_T_scale[] and scales is refused (POTUS_ERR_ARG): scales[][7] is that scale.  Every scale must be
 * positive and finite (POTUS_ERR_ARG, naming the data set and the scale), and the covariance scaled by it must factor, as for potus_create;
 * for the no-mode variant sigma_m, sigma_pop and sigma_e_bias are ignored, as potus_create ignores them.  Preconditions and refusals are
 * potus_set_datasets_ex's.  With scales every data set gets, besides what potus_set_datasets_ex gives it, its own sigma fields, the sigma
 * of every poll, the scales of the pollster / mode / population segments, L_W with its row L_W' w, L_T, L_B and the ratios of the three
 * factors, all built by the code potus_create uses; sizes, offsets, the LDS layout and the schedule do not depend on a scale and stay the
 * handle's (checked, not assumed).  The contract is the timeline's: chain c of the handle holds the bytes of a stand-alone handle created on
 * that data set's data with chain_id_offset = c.  Every call that takes a handle of potus_set_datasets_ex takes this one and works with the
 * chain's or the data set's model: potus_write_array[_device], potus_timeline*, potus_cv_*, potus_optimize, potus_laplace, potus_pathfinder,
 * potus_advi.  potus_sbc_ranks, potus_constrain and potus_simulate_prior refuse it as they refuse potus_set_datasets_ex's; so do the pooled
 * calls. */
#define POTUS_N_SCALES 9
int potus_set_datasets_grid(int handle, int n_datasets, const int32_t *n_democrat_state, const int32_t *n_democrat_national,
                            const int32_t *n_two_share_state, const int32_t *n_two_share_national,
                            const double *mu_b_prior /*[n][S] or NULL*/, const double *mu_b_T_scale /*[n] or NULL*/,
                            const double *scales /*[n][POTUS_N_SCALES] or NULL*/);
/* The distance between two sets of draws, per column (potus_sens.hpp, k_sg_distance).  a [n_a][n_cols] and b [n_b][n_cols] are blocks in the
 * memory of GPU `device`, draw-major: the layout of a data set's slice of potus_timeline_scores_device.  out [n_cols][3] (host) = w1, ks, cjs:
 *   x_1 < ... < x_m are the distinct values of the union of the two samples.
 *   P_j = #{a <= x_j} / n_a.  Q_j is likewise for b.
 *   Delta_j = x_{j+1} - x_j for j < m.
 *   w1  = sum_j Delta_j |P_j - Q_j|.  This is the Wasserstein-1 distance, in the column's own units.
 *   ks  = max_j |P_j - Q_j|.
 *   cjs = max(c(a, b), c(-a, -b)), defined as follows.
 *     c(a, b) = sqrt(max(0, C(P||Q) + C(Q||P)) / sum_j Delta_j (P_j + Q_j)).
 *     C(P||Q) = sum_j Delta_j P_j log2(P_j / ((P_j + Q_j)/2)) + (1 / (2 ln 2)) sum_j Delta_j (Q_j - P_j), with 0 * log 0 = 0.
 *     c = 0 when m = 1.
 *     This is the cumulative Jensen-Shannon distance of Nguyen & Vemuri (2015), which Kallioinen et al. (2023) use for power-scaling
 *     sensitivity.
 *   A non-finite value in either sample of a column makes that column's three outputs NaN, and no other column's.
 * Both samples of a column are sorted in LDS: n_a + n_b <= 16 384, more is refused with POTUS_ERR_UNSUPPORTED before the device is touched.
 * Every sum runs in an order fixed by n_a and n_b: a column has the same bytes alone and among any number of others. */
int potus_ecdf_distance_device(int device, const void *a, int n_a, const void *b, int n_b, int n_cols, double *out /*[n_cols][3]*/);
/* Every data set of a handle against data set `base` (0-based), over the post-warm-up draws and per day of [day_begin, day_end): the three
 * distances above for S + 2 columns -- the S state scores (predicted_score), the state_weights-weighted national vote and the Democratic
 * electoral votes sum_s ev[s] 1[score > 0.5] of a draw.  out [n_datasets][days][S + 2][3]; n_draws_out [n_datasets] as potus_timeline's.
 * Row `base` is 0, 0, 0.  A data set with a failed chain gets NaN, and so does every row if `base` failed; the others are unaffected.
 * Equal to potus_ecdf_distance_device on the slices of potus_timeline_scores_device.  Refusals are potus_timeline's, and base outside
 * [0, n_datasets) (POTUS_ERR_ARG); 2 x draws per data set <= 16 384. */
int potus_grid_compare(int handle, int base, int day_begin, int day_end, const double *ev /*[S]*/, int ev_to_win,
                       double *out, int32_t *n_draws_out);
/* Milliseconds (HIP events) of the calling thread's last potus_grid_compare: the scores kernel, the distance kernel; after
 * potus_ecdf_distance_device: 0, the distance kernel. */
int potus_grid_timing(double *ms /*[2]*/);
/* Per data set of a handle (of potus_set_datasets or potus_set_datasets_ex; a handle without either is one data set) and per day of
 * [day_begin, day_end) (0-based), over the data set's post-warm-up draws (warm-up rows of save_warmup = 1 are left out):
 *   state_out [n][days][S][4]   low 2.5 %, high 97.5 %, mean, P(> 0.5) of predicted_score; quantiles are R's type 7
 *   natl_out  [n][days][4]      the same for the state_weights-weighted national vote
 *   ev_out    [n][days][5]      Democratic electoral votes sum_s ev[s] 1[score > 0.5]: mean, median, high, low, P(>= ev_to_win)
 *   n_draws_out [n]             the draws summarised (chains per data set x post-warm-up draws)
 * A data set with a chain whose potus_chain_status is non-zero gets n_draws_out = 0 and NaN everywhere; the others are unaffected.  Sums run
 * in the canonical order of the draws (the data set's chains one after another, iterations within).  At most 16 384 post-warm-up draws per
 * data set (chains per data set x num_samples; more is refused with POTUS_ERR_UNSUPPORTED before the device is touched).  No output row
 * is built: election day costs prior + L_T z_T per draw, earlier days a suffix sum of the walk innovations on top. */
int potus_timeline(int handle, int day_begin, int day_end, const double *ev /*[S]*/, int ev_to_win,
                   double *state_out, double *natl_out, double *ev_out, int32_t *n_draws_out);
/* predicted_score of those days into DEVICE memory of the handle's GPU: [n][draws per data set][days][S], a data set's draws in canonical
 * order -- the slice of data set d is the `block` potus_outcomes_device and potus_scenario_device take.  The values are bit-equal to the
 * predicted_score columns of potus_write_array.  The scores of a data set with a failed chain are NaN. */
int potus_timeline_scores_device(int handle, int day_begin, int day_end, void *out_device);
/* Milliseconds (HIP events) of the calling thread's last potus_timeline: the scores kernel, the summary kernel. */
int potus_timeline_timing(double *ms /*[2]*/);
/* ---- exact cross-validation: held-out polls under the draws of the data set that did not see them ----
 * A fold of K-fold cross-validation, or a run date of leave-future-out, is a data set of potus_set_datasets_ex whose held-out polls have
 * n_two_share = 0.  For every (data set, poll) pair the masks name, the calls evaluate log p(y | n, draw) on the data set's post-warm-up draws
 * (warm-up rows of save_warmup = 1 are left out) with the data set's own model -- its prior and scales -- and the y and n of the data
 * given to potus_create.  The poll's measurement-noise sigma is the data set's own: on a handle of potus_set_datasets_grid the one of its
 * scales, on every other handle the one given to potus_create.  integrate = 1: the poll's noise coordinate integrated over its N(0,1) prior, the exact predictive density of a poll
 * the data set has not seen; integrate = 0: at the draw's own noise coordinate.  Handles of potus_set_datasets[_ex], and a plain handle,
 * which counts as one data set (in-sample values: those of potus_log_lik_device, byte for byte).  Refused before any kernel runs: a NULL mask or
 * output (POTUS_ERR_ARG; out_device = NULL is the exception below), a handle that is not initialised or has no post-warm-up draw saved
 * (POTUS_ERR_STATE), the dense metric (POTUS_ERR_UNSUPPORTED).  All-zero masks are no error: n_pairs = 0 and every output cell is NaN.
 * The same handle and masks give the same bytes on every call.
 * held_state [n_datasets][N_state_polls], held_national [n_datasets][N_national_polls]: nonzero = evaluate this poll under this
 * data set's draws (caller's poll order).  out_device [n_pairs][draws per data set]; out_device = NULL: only *n_pairs.
 * Pairs are ordered by data set, then state polls in data order, then national polls; a data set's draws in canonical order (its chains
 * one after another, iterations within).  The pairs of a data set with a failed chain (potus_chain_status) are NaN. */
int potus_cv_log_lik_device(int handle, const int32_t *held_state, const int32_t *held_national, int integrate,
                            void *out_device, long long *n_pairs);
/* lpd_out [n_datasets][N_state_polls + N_national_polls][2] = log mean p, log mean p^2 over the data set's post-warm-up draws;
 * NaN where the pair was not asked for; n_draws_out [n_datasets] (0 for a data set with a failed chain).  The Monte-Carlo variance of the
 * first slot is (exp(slot1 - 2 slot0) - 1) / n_draws by the delta method, with the draws taken as independent.  The pairs are worked in
 * blocks whose log-likelihood buffer stays within 256 MB (environment variable POTUS_CV_BLOCK_BUDGET, bytes: tests); the results do not
 * depend on the blocking. */
int potus_cv_lpd(int handle, const int32_t *held_state, const int32_t *held_national, int integrate,
                 double *lpd_out, int32_t *n_draws_out);
int potus_cv_timing(double *ms /*[2]: k_cv_loglik, k_cv_reduce, HIP events, calling thread's last potus_cv_lpd*/);
/* ---- the posterior mode: cmdstanr's $optimize(), batched -- one workgroup per path, every path in ONE launch ----
 * L-BFGS (history_size pairs, two-loop recursion, initial scaling s'y / y'y; a pair with s'y <= 0 is skipped, a direction that is no ascent
 * direction resets the history) with a strong-Wolfe line search (c1 = 1e-4, c2 = 0.9; first trial step of the first iteration init_alpha,
 * afterwards 1; at most 20 evaluations per search, a search that fails with a history is repeated once along the gradient with the history
 * emptied, so at most 40 per iteration; a non-finite trial shrinks the step) on log_prob<jacobian> of the unconstrained
 * coordinates: jacobian = 1 is the mode of the density the sampler draws from, jacobian = 0 (CmdStan's default for optimisation) the
 * penalised maximum-likelihood point.  The no-mode variant has no constrained parameter: both settings are the same computation there.
 * Stopping rules are CmdStan 2.24's, tested after each accepted step with strict <, so a tolerance of 0 switches a rule off; eps = 2^-52:
 *   1 ABSF     |f_k - f_{k-1}| < tol_obj                                    5 ABSX    ||x_k - x_{k-1}||_2 < tol_param
 *   2 RELF     |f_k - f_{k-1}| / max(|f_k|, |f_{k-1}|, tol_obj) < tol_rel_obj eps     6 MAXIT   iter iterations done
 *   3 ABSGRAD  ||g||_2 < tol_grad                                           7 LSFAIL  the line search failed; the last accepted point is returned
 *   4 RELGRAD  g' H g / max(|f|, tol_obj) < tol_rel_grad eps                8 INIT    no finite start; q, lp and the gradient norm of the path are NaN
 * (H the L-BFGS inverse-Hessian approximation with the newest pair in it, the identity after a reset).  A launch ends after at most
 * 100 + 21 iter model passes per path whatever the data: a path whose iterations repeat their search can use them up before iter iterations
 * and then ends MAXIT too.  info_out's gradient evaluations count every pass of the path, those of a failed search included.
 * Path p of a handle with data sets (potus_set_datasets[_ex]) uses the model of data set p / (n_paths / n_datasets), as the sampler picks a
 * chain's; on a plain handle every path uses the handle's model.  Starts: q0 [n_paths][D] is tried once per path; q0 = NULL draws
 * U(-init_radius, init_radius) starts, up to 100 attempts per path, from Philox4x32-10 as the sampler's (counter = {index, purpose | aux << 8,
 * iter, chain}, key = the handle's seed) with the NEW purpose 7:
 *   coordinate i of attempt a of path p   uniform of (index i, purpose 7, aux a, iter 0xFFFFFFFF, chain path_offset + p + 1)
 * so the bytes of a path do not depend on how paths are batched, and no stream of the sampler is reused.  Every sum runs in a fixed order
 * without atomics: the same (model, start, options) give the same bytes on every call and in every batch.
 * Callable any time after potus_create, before or after potus_init / potus_run: the call reads the models, works in buffers of its own and
 * touches no chain state -- a run continued afterwards gives the bytes of an uninterrupted run.  opts = NULL: the defaults.
 * Refused before any kernel runs: cus_per_chain > 1 or the dense metric (POTUS_ERR_UNSUPPORTED); n_paths <= 0 or, on a handle with data sets,
 * no multiple of their number; NULL q_out, lp_out or info_out; history_size outside 1..20; iter < 1; a negative or NaN tolerance; init_alpha
 * not finite and > 0; jacobian not 0 or 1; row_out with a bad column range (POTUS_ERR_ARG).  A path that ends INIT or LSFAIL does not fail
 * the call.  gnorm_out may be NULL.
 * row_out [n_paths][col_end - col_begin] (or NULL): the CmdStan output row of q_out[p], built on the device with the PATH'S OWN model by
 * the row builder of potus_write_array; column 0 (lp__) is lp_out[p], the sampler columns 1-6 are NaN as potus_constrain leaves them.  It is
 * what gives the constrained point on potus_set_datasets_ex handles, which potus_constrain refuses. */
typedef struct potus_optimize_opts {
  int32_t jacobian, history_size, iter, path_offset;
  double init_alpha, tol_obj, tol_rel_obj, tol_grad, tol_rel_grad, tol_param;
} potus_optimize_opts;   /* 64 bytes */
void potus_default_optimize_opts(potus_optimize_opts *o);   /* 0, 5, 2000, 0, 1e-3, 1e-12, 1e4, 1e-8, 1e7, 1e-8 */
int potus_optimize(int handle, const potus_optimize_opts *o, const double *q0 /*[n_paths][D] or NULL*/, int n_paths, double *q_out /*[n_paths][D]*/,
                   double *lp_out /*[n_paths]*/, double *gnorm_out /*[n_paths]*/, int32_t *info_out /*[n_paths][3]: code, iterations, gradient evaluations*/,
                   int col_begin, int col_end, double *row_out /*[n_paths][col_end - col_begin] or NULL*/);
int potus_optimize_timing(double *ms /*[1]: k_opt_lbfgs, HIP events, calling thread's last potus_optimize*/);
/* ---- the Laplace approximation: cmdstanr's $laplace(mode =, draws =, jacobian =) ----
 * For each of n_modes points: P = minus the Hessian of log_prob<jacobian> by central differences of the device gradient (step
 * h_j = h max(1, |mode_j|)), symmetrised; its Cholesky factor P = L L' on the matrix cores; n_draws draws x = mode + L^-T u with u standard
 * normal -- the caller's u, or Philox4x32-10 with purpose 8: coordinates 2 i and 2 i + 1 of draw n are the Box-Muller pair of counter
 * {i, 8, 0, draw_offset + n + 1}, key = the handle's seed.  A draw's bytes depend on (matrix, u of that draw) alone: not on n_draws, not on
 * draw_offset, not on the other modes of the call, not on the memory budget (POTUS_LAPLACE_MATRIX_BUDGET, bytes; default 16 GiB of D x D
 * matrices in flight).  lp_out is log_prob<jacobian = true> of the draw with the bytes of potus_log_prob_grad; lp_approx_out = -1/2 |u|^2, so
 * lp - lp(mode) - lp_approx is the draw's log importance ratio up to a constant.
 * Modes per handle as paths in potus_optimize: on a handle with data sets n_modes is a multiple of their number and mode m uses data set
 * m / (n_modes / n_datasets).  info_out [n_modes][4]: code (0 ok; 1 NOT_PD: a non-positive pivot, the mode's draws, log det and pivot are NaN;
 * 2: the mode is not finite, everything of it is NaN), log det P, |g|_2 at the mode (of log_prob<jacobian>), the smallest pivot min L_ii^2.
 * A mode that fails does not fail the call.  n_draws = 0 with precision_out is the Hessian alone.  The call needs cus_per_chain = 1 and the
 * diagonal metric, is possible any time after potus_create and touches no chain state.  The rows [lp__, six NaN, x] of the last call stay
 * on the handle for the three accessors below (replaced by the next call, freed by potus_destroy):
 *   potus_laplace_write_array_device  [n_modes * n_draws][col_end - col_begin] CmdStan columns of every draw, built with the mode's model
 *   potus_laplace_scores_device       [n_modes][n_draws][days][S] predicted_score: a mode's block is what potus_outcomes_device takes
 *   potus_laplace_summary             potus_timeline's outputs with a mode in the place of a data set (at most 16 384 draws per mode);
 *                                     a mode whose code is not 0 gives NaN and n_draws_out = 0 */
typedef struct potus_laplace_opts { int32_t jacobian, draw_offset, pad0, pad1; double h; } potus_laplace_opts;   /* 24 bytes */
void potus_default_laplace_opts(potus_laplace_opts *o);   /* 1, 0, 0, 0, 1e-4 (h: the best step on the 2016 design, profiles/laplace_2016.txt) */
int potus_laplace(int handle, const potus_laplace_opts *o, const double *mode /*[n_modes][D]*/, int n_modes,
                  const double *u /*[n_modes][n_draws][D] or NULL*/, int n_draws,
                  double *q_out /*[n_modes][n_draws][D] or NULL*/, double *lp_out, double *lp_approx_out /*[n_modes][n_draws] or NULL*/,
                  double *info_out /*[n_modes][4]*/, double *precision_out /*[n_modes][D][D] or NULL*/);
int potus_laplace_write_array_device(int handle, int col_begin, int col_end, void *out_device);
int potus_laplace_scores_device(int handle, int day_begin, int day_end, void *out_device);
int potus_laplace_summary(int handle, int day_begin, int day_end, const double *ev, int ev_to_win,
                          double *state_out, double *natl_out, double *ev_out, int32_t *n_draws_out);
int potus_laplace_timing(double *ms /*[4]: Hessian, factor, solve, lp__; HIP events, calling thread's last potus_laplace*/);
/* ---- Pathfinder: cmdstanr's $pathfinder(psis_resample = FALSE), Zhang, Carpenter, Gelman and Vehtari (2022) ----
 * Along an L-BFGS path x_0 .. x_L of log_prob<jacobian = true> with gradients g_l, s_l = x_l - x_{l-1}, z_l = g_{l-1} - g_l: pair l is kept
 * when s'z > 0 and z'z <= 1e12 s'z; alpha_0 = 1 and a kept pair updates the diagonal, with a = z'diag(alpha)z, b = z's, c = s'diag(alpha)^-1 s
 * at alpha_{l-1}, to alpha_l = 1 / (a / (b alpha) + z^2 / b - a s^2 / (b c alpha^2)) elementwise.  With S, Z the last min(history_size, kept so
 * far) kept pairs up to l (oldest first), R = triu(S'Z), E = diag(S'Z), beta = [diag(alpha_l) Z, S],
 * gamma = [[0, -R^-1], [-R^-T, R^-T (E + Z'diag(alpha_l)Z) R^-1]]: Sigma_l = diag(alpha_l) + beta gamma beta', mu_l = x_l + Sigma_l g_l.
 * Draws: thin QR diag(alpha_l^-1/2) beta = Q R~, L~ = chol(I + R~ gamma R~'), phi = mu_l + alpha_l^1/2 (u + Q (L~ - I) Q'u),
 * log q(phi) = -1/2 (sum log alpha_l + 2 sum log L~_ii + u'u + D log 2 pi).  ELBO_l, l = 1 .. L: the mean over num_elbo_draws draws of
 * log p(phi) - log q(phi); a non-finite log p in any of them, or a Sigma_l that is not positive definite, makes it -inf.  l* = argmax, the
 * lowest l on ties; the path's num_draws draws come from (mu_l*, Sigma_l*).  Every ELBO -inf: the path's code is 1 (NO_ELBO), its draws are
 * NaN, the call does not fail.  There is no D x D matrix: a fit costs O(D history_size^2), a draw O(D history_size) and one model pass.
 * Normals, when the caller gives none: Philox4x32-10 as the sampler's, key = the handle's seed, the NEW purpose 9; coordinates 2 i, 2 i + 1 are
 * the Box-Muller pair of counter
 *   ELBO draw k of iterate l of path p    {i, 9 | k << 8, l, path_offset + p + 1}
 *   final draw n of path p                {i, 9 | 0xFF << 8, draw_offset + n + 1, path_offset + p + 1}
 * so a path's bytes depend on neither the batch, nor the number of draws asked for, nor the number of workgroups (environment variable
 * POTUS_PATHFINDER_G, default: the compute units; tests).  Paths per handle as in potus_optimize: path p uses data set p / (n_paths / n_datasets).
 * potus_pathfinder runs k_opt_lbfgs first (opt: potus_optimize's options; opt.jacobian is taken as 1 and opt.path_offset as path_offset;
 * opt.iter is CmdStan's max_lbfgs_iters) and takes the accepted points as the path; potus_pathfinder_path takes the caller's x, g
 * [n_paths][rows][D] with lengths L[p] <= rows - 1, and with u_elbo [n_paths][rows - 1][num_elbo_draws][D] / u_draws [n_paths][num_draws][D]
 * the caller's normals; for want_l[p] it also returns mu, alpha and log det Sigma of that iterate (NaN outside 1 .. L; alpha from 0), the
 * draws phi_out and their log q lqw_out that THAT iterate gives from the final normals (no model pass), and Q'Q of its thin QR (2j x 2j of a
 * 20 x 20 block, NaN elsewhere).
 * Outputs: info_out [n_paths][4] = code, L, l*, the optimiser's return code (0 from potus_pathfinder_path); elbo_out, kept_out
 * [n_paths][rows] indexed by l (rows = opt.iter + 1 in potus_pathfinder; NaN / 0 outside 1 .. L); q_out [n_paths][num_draws][D]; lp_out: log_prob of
 * the draw with the bytes of potus_log_prob_grad; lq_out: log q.  Any output but info_out may be NULL.  traj_x_out, traj_g_out
 * [n_paths][opt.iter + 1][D] or NULL: the path itself, NaN behind its end.  The rows [lp__, six NaN, phi] of the last call stay on the handle for
 * the three accessors, which are potus_laplace's with a path in the place of a mode.  Refused before any kernel runs, as in potus_optimize:
 * cus_per_chain > 1, the dense metric (POTUS_ERR_UNSUPPORTED); history_size outside 1..10,
 * num_elbo_draws outside 1..255, negative num_draws or offsets, n_paths no multiple of the data sets (POTUS_ERR_ARG).  No chain state is touched. */
typedef struct potus_pathfinder_opts {
  potus_optimize_opts opt;
  int32_t history_size, num_elbo_draws, num_draws, draw_offset, path_offset, pad0;
} potus_pathfinder_opts;   /* 88 bytes */
void potus_default_pathfinder_opts(potus_pathfinder_opts *o);   /* opt: potus_optimize's with jacobian 1, iter 1000; 6, 25, 1000, 0, 0 */
int potus_pathfinder(int handle, const potus_pathfinder_opts *o, const double *q0 /*[n_paths][D] or NULL*/, int n_paths, int32_t *info_out,
                     double *elbo_out, int32_t *kept_out, double *q_out, double *lp_out, double *lq_out, double *traj_x_out, double *traj_g_out);
int potus_pathfinder_path(int handle, const potus_pathfinder_opts *o, const double *x, const double *g, const int32_t *L, int rows, int n_paths,
                          const double *u_elbo, const double *u_draws, const int32_t *want_l, int32_t *info_out, double *elbo_out,
                          int32_t *kept_out, double *q_out, double *lp_out, double *lq_out, double *mu_out /*[n_paths][D]*/,
                          double *alpha_out /*[n_paths][D]*/, double *logdet_out /*[n_paths]*/, double *phi_out /*[n_paths][num_draws][D]*/,
                          double *lqw_out /*[n_paths][num_draws]*/, double *qtq_out /*[n_paths][20][20]*/);
int potus_pathfinder_write_array_device(int handle, int col_begin, int col_end, void *out_device);
int potus_pathfinder_scores_device(int handle, int day_begin, int day_end, void *out_device);
int potus_pathfinder_summary(int handle, int day_begin, int day_end, const double *ev, int ev_to_win,
                             double *state_out, double *natl_out, double *ev_out, int32_t *n_draws_out);
int potus_pathfinder_timing(double *ms /*[4]: L-BFGS, alpha, ELBO, draws; HIP events, calling thread's last potus_pathfinder[_path]*/);
/* ---- mean-field ADVI: cmdstanr's $variational(algorithm = "meanfield"), batched; the rules of CmdStan 2.24's advi.hpp ----
 * q = N(mu, diag(exp(omega))^2) on the unconstrained scale.  Start: mu_0 = q0 or U(-r, r) with the handle's init_radius, omega_0 = 0.
 * Gradient step t = 1, 2, ...: for m = 1 .. grad_samples, eps_m ~ N(0, I), zeta = mu + exp(omega) o eps_m, (lp, g) = log_prob_grad<jacobian = true>
 * (zeta); g_mu = mean g, g_omega = mean(g o eps) o exp(omega) + 1; for mu and omega alike s = g^2 at t = 1, afterwards s <- 0.9 g^2 + 0.1 s, and
 * theta <- theta + (eta / sqrt(t)) g / (1 + sqrt(s)).  A non-finite lp or gradient entry ends the run (NONFINITE) at the last finished iterate.
 * ELBO(mu, omega) = mean over elbo_samples draws of lp(zeta_k) + 1/2 D (1 + log 2 pi) + sum omega + elbo_offset.
 *   Deviation 1: Stan redraws a non-finite lp up to elbo_samples times; here any non-finite lp makes that ELBO -inf (Pathfinder's rule in this
 *   library: fixed counters cannot redraw).  Deviation 2: lp is the library's lp__, constants dropped, where Stan uses log_prob<propto = false>;
 *   elbo_offset adds the constant for a caller who wants it: it enters the relative differences below and nothing else.
 * Adaptation (adapt_engaged): elbo_init = ELBO(mu_0, omega_0), not finite: INIT.  Each eta of (100, 10, 1, 0.1, 0.01) runs adapt_iter steps from
 * (mu_0, omega_0) with s reset, then its ELBO (a NONFINITE candidate counts as -inf).  In sequence order: if elbo < best and best > elbo_init,
 * stop; else if elbo > best, best = elbo and eta* = eta; after the last candidate, its elbo <= elbo_init is ADAPT_FAILED.  The five candidates
 * are independent and run at once; the sequential rule is applied to the five ELBOs afterwards and gives the sequential algorithm's result.
 * Main run from (mu_0, omega_0), s reset, eta* (eta as given with adapt_engaged = 0).  Every eval_elbo iterations: prev = elbo (starts at 0, so
 * the first relative difference is 1), elbo = ELBO, delta = |(elbo - prev) / elbo| into a circular buffer of max(floor(0.1 iter / eval_elbo), 2)
 * entries; the run ends MEAN_CONVERGED when mean(buffer) < tol_rel_obj, else MEDIAN_CONVERGED when median(buffer) < tol_rel_obj (Stan's
 * circ_buff_median: nth_element at n / 2, the UPPER middle entry of an even number), else MAXIT at t = iter (iter < eval_elbo: no evaluation).
 * Flag bit 1 of the info word: t > 10 eval_elbo and mean or median > 0.5 (Stan's "may be diverging").
 * Codes: 1 MEAN_CONVERGED, 2 MEDIAN_CONVERGED, 3 MAXIT, 4 NONFINITE, 5 INIT, 6 ADAPT_FAILED.  INIT and ADAPT_FAILED leave no approximation:
 * mu, omega and the run's draws are NaN; a code fails its run alone, never the call.
 * Normals: Philox4x32-10 as the sampler's, key = the handle's seed, the NEW purpose 10; coordinates 2 j, 2 j + 1 are the Box-Muller pair of counter
 * {j, 10 | aux << 8, iter word, run_offset + r + 1} with aux = stage | draw << 4:
 *   gradient draw m of step t, main run                 stage 0,      draw m, iter word t
 *   gradient draw m of step t, adaptation candidate c   stage 1 + c,  draw m, iter word t          (c = 0 .. 4)
 *   ELBO draw k at iterate t (t = 0: the initial ELBO)  stage 8 (main) or 9 + c, draw k, iter word t
 *   library start, coordinate i (a uniform)             {i, 10 | 14 << 8, 0, run_offset + r + 1}
 *   final draw n                                        stage 15,     draw 0, iter word draw_offset + n + 1
 * so a run's bytes depend on neither the batch, nor the number of workgroups of the ELBO grid (environment variable POTUS_ADVI_G, default: the
 * compute units; tests), nor output_samples, nor draw_offset.  Runs per handle as in potus_optimize: run r uses data set r / (n_runs / n_datasets).
 * Outputs: info_out [n_runs][6] = code, flag bits, iterations, index of eta* (-1: none), model passes, ELBO evaluations of the main run;
 * mu_out, omega_out [n_runs][D]; elbo_out [n_runs][iter / eval_elbo + 1]: the initial ELBO at 0, entry j the ELBO at t = j eval_elbo, NaN behind
 * the end; adapt_elbo_out [n_runs][5] (NaN with adapt_engaged = 0); q_out [n_runs][output_samples][D]: zeta_n = mu + exp(omega) o eps_n; lp_out:
 * log_prob of the draw with the bytes of potus_log_prob_grad; lq_out = -1/2 |eps|^2 - sum omega - 1/2 D log 2 pi.  Any output but info_out may be
 * NULL.  The rows [lp__, six NaN, zeta] of the last call stay on the handle for the three accessors, which are potus_laplace's with a run in the
 * place of a mode.  Refused before any kernel runs, as in potus_optimize: cus_per_chain > 1, the dense metric, algorithm = fullrank
 * (POTUS_ERR_UNSUPPORTED); n_runs no multiple of the data sets, iter / eval_elbo / adapt_iter < 1, grad_samples or elbo_samples outside
 * 1..1048575, eta not positive, negative tol_rel_obj, output_samples or offsets (POTUS_ERR_ARG).  No chain state is touched. */
#define POTUS_ADVI_MEANFIELD 0
#define POTUS_ADVI_FULLRANK 1
typedef struct potus_advi_opts {
  int32_t algorithm, iter, grad_samples, elbo_samples, eval_elbo, adapt_engaged, adapt_iter, output_samples, draw_offset, run_offset;
  double eta, tol_rel_obj, elbo_offset;
} potus_advi_opts;   /* 64 bytes */
void potus_default_advi_opts(potus_advi_opts *o);   /* meanfield, 10000, 1, 100, 100, adapt on / 50, 1000 draws, offsets 0; 1.0, 0.01, 0 */
int potus_advi(int handle, const potus_advi_opts *o, const double *q0 /*[n_runs][D] or NULL*/, int n_runs, int32_t *info_out, double *mu_out,
               double *omega_out, double *elbo_out, double *adapt_elbo_out, double *q_out, double *lp_out, double *lq_out);
int potus_advi_write_array_device(int handle, int col_begin, int col_end, void *out_device);
int potus_advi_scores_device(int handle, int day_begin, int day_end, void *out_device);
int potus_advi_summary(int handle, int day_begin, int day_end, const double *ev, int ev_to_win,
                       double *state_out, double *natl_out, double *ev_out, int32_t *n_draws_out);
int potus_advi_timing(double *ms /*[4]: adaptation, gradient segments, ELBO, draws; HIP events, calling thread's last potus_advi*/);
/* Prior predictive simulation: n_sims draws theta ~ prior (poll_model_2020.stan:116-128) on the unconstrained scale (q_out [n_sims][D];
 * rho_e_bias ~ normal(0.7, 0.1) restricted to (0, 1), stored as logit(rho)) and y ~ binomial(n_two_share, inv_logit(logit_pi(theta)))
 * (stan:85-113; exact sampler: inversion when n min(p, 1 - p) < 10, BTRS above) in the caller's poll order.  Any output may be null.
 * Philox4x32-10 as the sampler's (counter = {index, purpose | aux << 8, iter, chain}, key = seed), purpose 6, chain = sim_offset + i + 1
 * for simulation i, so a simulation's bytes do not depend on how simulations are batched:
 *   standard normals   coordinates 2j, 2j+1 = the Box-Muller pair of (iter 0, aux 0, index j)
 *   rho_e_bias         attempt a = 0, 1, ...: z = first normal of (iter 0, aux 1, index a), accepted when 0 < 0.7 + 0.1 z < 1
 *                      (replaces coordinate rho_e_bias of the line above)
 *   outcome of poll k  (k = state poll index, or N_state_polls + national poll index) attempt a: u = uniform (iter a, aux 2, index k);
 *                      BTRS also v = uniform (iter a, aux 3, index k) */
int potus_simulate_prior(int handle, uint64_t seed, int n_sims, int sim_offset, double *q_out /*[n_sims][D]*/,
                         int32_t *n_democrat_state_out /*[n_sims][N_state_polls]*/, int32_t *n_democrat_national_out /*[n_sims][N_national_polls]*/);
/* CmdStan output rows of arbitrary unconstrained points (rstan's constrain_pars): out [n][col_end - col_begin]; the sampler columns
 * 0-6 of these rows are NaN. */
int potus_constrain(int handle, const double *q /*[n][D]*/, int n, int col_begin, int col_end, double *out);
/* SBC ranks on the device: for every data set d (a handle without potus_set_datasets is one) and column k of [col_begin, col_end)
 * (col_begin >= POTUS_N_SAMPLER_COLS), less[d][k] / equal[d][k] = how many of the compared draws are below / equal to truth[d][k];
 * the compared draws are every thin-th post-warm-up saved draw (the first, the (thin+1)-th, ...) of every chain of the data set, *L of
 * them per data set.  Chains that failed (potus_chain_status != 0) add nothing.  No draws x columns block is built. */
int potus_sbc_ranks(int handle, const double *truth /*[n_datasets][ncols]*/, int col_begin, int col_end, int thin, int32_t *less /*[n_datasets][ncols]*/,
                    int32_t *equal, int *L);

/* ---- PSIS-LOO (Vehtari, Gelman, Gabry 2017): what fit$loo() computes from a log_lik generated quantity ----
 * Polls are numbered as the output row numbers them: state polls in data order, then national polls.  integrate = 0: the plain
 * binomial_logit_lpmf(y | n, logit_pi) of each poll at the draw (log C(n, y) included); integrate = 1: the poll's own noise coordinate
 * raw_measure_noise_* integrated out of its likelihood, log int Binomial(y | n, inv_logit(eta + sigma z)) phi(z) dz (adaptive Gauss-Hermite,
 * 16 nodes), where plain PSIS-LOO meets high Pareto k because every poll has a parameter of its own.  Warm-up rows (save_warmup = 1) are left out. */
/* per-poll log-likelihood of the saved post-warm-up draws, on the handle's device: out_device [poll_end - poll_begin][chains][n_post] */
int potus_log_lik_device(int handle, int poll_begin, int poll_end, int integrate, void *out_device);
/* PSIS-LOO of a [n_polls][n_chains][n_draws] log-likelihood block already on `device`; r_eff [n_polls] or NULL (computed);
 * pointwise_out [n_polls][5] = elpd_loo, p_loo, looic, pareto_k, r_eff; estimates_out [3][2] = (elpd_loo, p_loo, looic) x (estimate, se) */
int potus_loo_device(int device, const void *log_lik, int n_polls, int n_chains, long long n_draws, const double *r_eff,
                     double *pointwise_out, double *estimates_out);
/* the same over the pooled post-warm-up draws of handles that hold one posterior (the pooling rules of potus_diagnostics; at least four
 * post-warm-up draws per chain); handles on other GPUs are brought to the first handle's by peer copies.  Polls go in blocks whose
 * temporaries stay within 256 MB; r_eff as loo::relative_eff (not split) when NULL. */
int potus_loo(const int *handles, int n_handles, int integrate, const double *r_eff, double *pointwise_out, double *estimates_out);

/* ---- moment matching for PSIS-LOO (Paananen, Piironen, Buerkner, Vehtari 2021): loo(..., moment_match = TRUE) ----
 * For the polls whose k-hat is above k_threshold, a diagonal affine map T(theta) = a + b * theta of the pooled draws is adapted step by step
 * (T1: match the mean under the PSIS weights; T2: mean and marginal variance), each candidate accepted iff its k-hat falls; the log density
 * and the poll's log-likelihood are evaluated at the mapped draws by the model pass.  With split = 1 the map is then applied to the draws
 * at even iterations of every chain only and the mixture of the posterior and its push-forward is the proposal.  Departures from loo: the
 * split halves (loo: the first half of the rows), the exact inverse (x - a) / b, no covariance step (cov = 1 is refused with
 * POTUS_ERR_UNSUPPORTED: with S < D the weighted covariance is singular), the fit and the model handle on one device.
 *   model_handle  supplies the model of the pass: one workgroup per chain (cus_per_chain = 1, twin = 0), diagonal metric, no data sets, the
 *                 data of the fit.  It may be one of `handles`.
 *   handles       the fit, pooled as potus_loo pools (any layout), on the model handle's device.
 *   polls         [n_polls] poll numbers as potus_loo numbers them, or NULL: every poll.  Only polls above the threshold are worked on.
 *   pointwise     in: potus_loo's [N][5] of these handles with the same integrate; out: the rows of the polls with an accepted step updated
 *                 (elpd_loo, p_loo = lpd - elpd_loo with the old lpd, looic, pareto_k; r_eff stays); every other row keeps its bytes.
 *                 The call recomputes each worked poll's k from the draws and refuses rows it cannot reproduce to 1e-12 (rows of the other
 *                 form or of another fit).  A call that fails leaves pointwise and estimates_out as they were (the optional outputs not).
 *   info_out      optional [N][6]: accepted T1 steps, accepted T2 steps, candidates evaluated, split done, stop reason (1: k <= threshold,
 *                 2: max_iters accepted, 3: both candidates rejected; 0: the poll was not listed), reserved.
 *   k_path_out    optional [N][max_iters + 2]: k of plain PSIS, k after every accepted step, k after the split; NaN beyond.
 *   map_out       optional, needs polls: [n_polls][2][D], a then b of every listed poll (0 and 1 where no step was accepted).
 * A poll's outputs depend on neither the other polls of the call nor the grid.  Refused before any kernel runs: cov = 1, a model handle that
 * is not one workgroup per chain with the diagonal metric (POTUS_ERR_UNSUPPORTED), handles with data sets (POTUS_ERR_STATE), a model
 * handle with other data than the fit (POTUS_ERR_ARG), handles on another device (POTUS_ERR_UNSUPPORTED). */
typedef struct potus_loo_mm_opts { int32_t integrate, max_iters, split, cov; double k_threshold; } potus_loo_mm_opts;   /* 24 bytes */
void potus_default_loo_mm_opts(potus_loo_mm_opts *o);   /* 1, 30, 1, 0, 0 (k_threshold = 0: min(1 - 1 / log10 S, 0.7)) */
int potus_loo_moment_match(int model_handle, const int *handles, int n_handles, const potus_loo_mm_opts *opts, const int32_t *polls, int n_polls,
                           double *pointwise /*[N][5]*/, double *estimates_out /*[3][2]*/, int32_t *info_out, double *k_path_out, double *map_out);
int potus_loo_mm_timing(double *ms /*[4]: passes, moments, PSIS, final; HIP events, calling thread's last potus_loo_moment_match*/);
/* The stages on device blocks.  draws [n_chains][n_draws][7 + D] are rows as potus_get_draws returns them (canonical order).
 * ratios: lp_out, ll_out [n_polls][n_chains][n_draws] = the log density and poll polls[k]'s log-likelihood at theta (sel[k] = 0), a_k + b_k *
 * theta (1), (theta - a_k) / b_k (2), or (3) the first at even and the second at odd iterations; a, b host [n_polls][D]; lp0_out optional
 * [n_chains][n_draws]: the log density at theta by the same kernel.
 * moments: mu_out[k][j] = sum_s w[k][s] theta[s][j], q_out[k][j] = sum_s w[k][s] (theta[s][j] - m0[j])^2 (m0 NULL: 0); weights [n_polls][S]
 * on the device, log weights when is_log.
 * psis: PSIS of general log ratios [n_polls][n_chains][n_draws] (-inf: weight 0; a NaN or +inf entry, or no finite one: k = NaN and NaN
 * weights): normalised log weights to log_weights_out (device, same shape), k-hat to khat_out (host). */
int potus_loo_mm_ratios_device(int model_handle, const void *draws, int n_chains, int n_draws, const double *a, const double *b, const int32_t *polls,
                               const int32_t *sel, int n_polls, int integrate, void *lp_out, void *ll_out, void *lp0_out);
int potus_loo_mm_moments_device(int device, const void *draws, int n_chains, int n_draws, int D, const void *weights, int n_polls, int is_log,
                                const double *m0, double *mu_out /*[n_polls][D]*/, double *q_out);
int potus_psis_device(int device, const void *log_ratios, int n_polls, int n_chains, long long n_draws, const double *r_eff /*[n_polls]*/,
                      void *log_weights_out, double *khat_out);

/* ---- E_loo (loo::E_loo): expectations under the posterior that has not seen poll i, from the PSIS weights ----
 * For poll i: r = the raw log ratios (from a fit: -log_lik_i), lw = the normalised log weights potus_psis_device gives for r, w = exp(lw) (a
 * weight of -inf is 0), rho = exp(r - max r).  For a quantity x[s]:
 *   mean = sum w x;  variance = sum w (x - mean)^2;  sd = its square root;
 *   quantile(p): type 7 when all weights are equal; otherwise x sorted ascending (ties by draw index) with w carried along, ww = cumsum(w) /
 *     sum w, j the first index with ww[j] >= p: x[0] when j = 0, else x[j-1] + (x[j] - x[j-1]) (p - ww[j-1]) / (ww[j] - ww[j-1]);
 *   Pareto k of the estimate: mean: h = x, variance and sd: h = x^2: max(k_r, k_hr); quantile: k_r; also k_r when h is constant, takes exactly
 *     two values or is not finite somewhere.  k_r = the k-hat of the right tail of rho (potus_loo's pareto_k of the poll), k_hr = the larger of
 *     the k-hats of the right tails of h rho and -h rho; a tail = the M largest values, M = ceil(min(0.2 S, 3 sqrt(S / r_eff))), minus the value
 *     just below them, fitted by gpdfit with loo's prior; M < 5 or a tail spread below DBL_EPSILON / 100: +inf.
 * pointwise form: x and log_ratios [n_polls][n_chains][n_draws] on `device` (x has its own values per poll); r_eff [n_polls] or NULL (computed
 * from -log_ratios as potus_loo computes it); probs [n_probs] inside (0, 1), at most 16.  out [n_polls][3 + n_probs] = mean, variance, sd,
 * quantiles; khat_out [n_polls][3] = k of the mean, of variance and sd, of the quantiles.  A poll whose ratios hold a NaN or +inf, no finite
 * value, or a -inf while r_eff is NULL gets NaN.  A poll's bytes depend on its own rows alone.
 * shared form: X [n_cols][n_chains][n_draws] quantities common to all polls, log_weights [n_polls][n_chains][n_draws] normalised log weights,
 * both on `device`: mean_out, var_out [n_polls][n_cols], ess_out [n_polls] = 1 / sum w^2 (host).  The products run on the fp64 matrix cores
 * about c[j] = the equal-weight mean of column j: mean = c + sum w (x - c), variance = sum w (x - c)^2 - (sum w (x - c))^2; the draws are summed
 * in chunks of 1024, the chunks added in order: an entry's bytes depend on its poll's weights and its column alone.  log_ratios (optional, device,
 * the shape of log_weights) and r_eff ([n_polls] or NULL: computed) give the diagnostic: diag = 0: khat_out [n_polls] = k_r; diag = 1: khat_out
 * [n_polls][n_cols] = the k of every mean.
 * Refused before any kernel runs (POTUS_ERR_ARG): fewer than four draws per chain, probs outside (0, 1), r_eff not finite and positive, blocks that
 * are not memory of `device`. */
int potus_e_loo_device(int device, const void *x, const void *log_ratios, int n_polls, int n_chains, long long n_draws, const double *r_eff,
                       const double *probs, int n_probs, double *out, double *khat_out);
int potus_e_loo_shared_device(int device, const void *X, int n_cols, const void *log_weights, int n_polls, int n_chains, long long n_draws,
                              const void *log_ratios, const double *r_eff, int diag, double *mean_out, double *var_out, double *ess_out, double *khat_out);
/* What the model expects of each poll at every post-warm-up draw (k_el_poll_share, the sibling of potus_log_lik_device: same polls, same
 * eta): a1 = E_z[p], a2 = E_z[p^2], p = inv_logit(eta + sigma z); integrate = 0: at the draw's own noise coordinate (a2 = a1^2); integrate = 1:
 * over z ~ N(0, 1), 16 Gauss-Hermite nodes centred at 0.  a1_out, a2_out: device [poll_end - poll_begin][chains][n_post].  With E_loo of a1 and
 * a2 the leave-one-out predictive mean of the observed share y / n is E[a1], its variance E[a1] / n + (1 - 1 / n) E[a2] - E[a1]^2. */
int potus_poll_share_device(int handle, int poll_begin, int poll_end, int integrate, void *a1_out_device, void *a2_out_device);
/* E_loo on a fit's handles, pooled as potus_loo pools (one posterior; polls in blocks whose temporaries stay within 256 MB; blocks of other GPUs
 * brought to the first handle's by peer copies): log-likelihood -> potus_loo's k-hat and r_eff -> ratios -> PSIS weights -> the forms above.
 * The weights are the plain PSIS weights, not moment-matched ones.  pareto_k_out [N] is potus_loo's pareto_k.
 *   what = POTUS_ELOO_PREDICT: out [N][5] = the leave-one-out predictive mean of the poll's share y / n (E_loo[a1]), its variance E_loo[a1] / n +
 *     (1 - 1 / n) E_loo[a2] - E_loo[a1]^2, its sd, the k of the a1 mean, the in-sample (equal-weight) mean of a1.  The other arguments are ignored.
 *   what = POTUS_ELOO_INFLUENCE: the 2 S + 3 forecast columns of `day` (0-based; negative: election day): the S state scores, the national vote
 *     (normalised state_weights . scores), the S indicators score > 0.5, electoral college won (sum ev won >= ev_to_win), electoral votes.
 *     out, var_out [N][2 S + 3] = leave-one-out mean and variance, post_out [2 S + 3] the posterior means (influence = out - post_out), ess_out
 *     [N], khat_out [N][2 S + 3] the k of every mean when diag = 1.  With day_begin < day_end also the score and national columns of those days:
 *     days_out [N][days][S + 1], days_post_out [days][S + 1].  Needs handles of one workgroup per chain with the diagonal metric.
 * Refused before any kernel runs: handles with data sets (POTUS_ERR_STATE), handles of another posterior or listed twice (POTUS_ERR_ARG), fewer
 * than four post-warm-up draws per chain (POTUS_ERR_STATE, potus_loo's refusal), bad integrate / what / day.  potus_e_loo_timing: the stages summed. */
enum { POTUS_ELOO_PREDICT = 0, POTUS_ELOO_INFLUENCE = 1 };
int potus_e_loo(const int *handles, int n_handles, int integrate, int what, const double *ev /*[S]*/, int ev_to_win, int day, int day_begin, int day_end, int diag,
                double *out, double *var_out, double *post_out, double *pareto_k_out, double *ess_out, double *khat_out, double *days_out, double *days_post_out);
int potus_e_loo_timing(double *ms /*[4]: pointwise form; column means and products; chunk sums and ess; diagnostic.  HIP events, calling thread's last call*/);

/* ---- posterior predictive checks: could the fitted model have produced the polls it was fitted to? ----
 * Polls are numbered as potus_loo numbers them: state polls in data order, then national polls.  For poll i (outcome y_i of n_i) and post-warm-up
 * draw s (S of them over all chains): eta_is = the predictor without the poll's noise term, exactly as potus_log_lik_device forms it, sigma_i the
 * poll's noise scale, z_is the draw's own noise coordinate.
 *   replicate   integrate = 0: x = eta_is + sigma_i z_is (the same poll repeated);  integrate = 1: x = eta_is + sigma_i z', z' ~ N(0, 1) fresh (a new
 *               poll of the same pollster, mode, population, state and day: the replicate that belongs with the integrated log-likelihood, since
 *               under leave-one-out the poll's noise coordinate has its prior);  sigma_i = 0: as integrate = 0.
 *               y_rep_is ~ Binomial(n_i, inv_logit(x)) by the prior simulator's exact sampler: inversion below n min(p, 1 - p) = 10, BTRS above.
 *               n_i = 0: y_rep = 0, NaN PIT values, and the poll is in no group sum.
 *   randomness  Philox4x32-10, purpose RNG_PPC = 11.  Key = the handle's seed; counter words
 *                 c0 = poll number;  c1 = 11 | kind << 8 | attempt << 10 | rep << 22;  c2 = post-warm-up iteration (0-based);
 *                 c3 = the chain's global id, chain_id_offset + c + 1
 *               kind 1 = the fresh normal z' (attempt 0; the first normal of the Box-Muller pair of the block), kind 2 = u and kind 3 = v of the
 *               sampler's attempt (< 4096, 12 bits); rep in [0, 1023], rep + 1 an independent second replicate.  A cell's y_rep depends on seed,
 *               chain id, iteration, poll and rep, and on nothing else: not on the poll block, the grid, or how the chains are split over handles
 *               or GPUs.
 *   moments     a1, a2 = potus_poll_share_device's blocks with the same integrate;  m = n a1;  v = n a1 (1 - a1) + n (n - 1) max(a2 - a1^2, 0);
 *               r(k) = (k - m) / sqrt(v) for v > 0, else 0.  Every operation is rounded on its own (no fused multiply-adds), evaluated as
 *               ((n a1) (1 - a1)) + ((n (n - 1)) max(a2 - (a1 a1), 0)).
 *   groups      for group g and draw s, over the group's polls with n > 0 in ascending poll number, added one after the other from 0:
 *               bias B = sum r(.), dispersion X = sum r(.)^2, count N = sum (.), each at y_i (realised, T_obs) and at y_rep_is (replicated, T_rep).
 *               Per (group, statistic) six numbers: mean_s T_obs, mean_s T_rep, the exact counts #{T_rep > T_obs}, #{=}, #{<} (whole numbers),
 *               p = (gt + eq / 2) / S.  A group without polls: NaN, NaN, 0, 0, 0, NaN.
 *   PIT         lo_i = sum_s w_is 1[y_rep_is < y_i], eq_i = sum_s w_is 1[y_rep_is = y_i], summed in a fixed order.  Without weights (w = 1 / S, the
 *               posterior PIT) the exact counts divided by S; with log_weights w = exp(lw), lw = the normalised PSIS log weights potus_psis_device
 *               gives for r = -log_lik_i with the same integrate (the LOO-PIT); a weight of -inf counts as 0, NaN weights give NaN.  The
 *               randomised PIT lo + v eq, the non-randomised histogram (Czado, Gneiting, Held 2009) and the coverage are formed on the host.
 * potus_poll_rep_device: the sibling of potus_log_lik_device / potus_poll_share_device (same polls, same eta): y_rep of polls [poll_begin, poll_end)
 *   as doubles, device [polls][chains][n_post]: it feeds potus_e_loo_device unchanged.
 * potus_ppc_pit_device: yrep (and log_weights, or NULL) device [n_polls][n_chains][n_draws], y host [n_polls]; out host [n_polls][2] = lo, eq.
 * potus_ppc_groups_device: yrep, a1, a2 device [n_polls][n_chains][n_draws]; y, n, groups host [n_polls] (a label in [0, n_groups), or -1: in no
 *   group).  acc_device [n_groups][3][2][n_chains][n_draws] (statistic, then realised / replicated) holds T per draw; flags: POTUS_PPC_BEGIN zeroes
 *   it and n_in_group first, POTUS_PPC_FINISH writes group_out [n_groups][3][6] afterwards; between them the poll blocks of one fit are added in
 *   ascending order, and the bytes do not depend on where the blocks are cut.  acc_device may be NULL when both flags are set.
 *   n_in_group [n_groups] (host) counts the polls with n > 0 added so far.
 * potus_ppc: the whole check on a fit's handles, pooled as potus_e_loo pools (and refusing what it refuses).  Per poll block: log-likelihood ->
 *   potus_loo's k-hat and r_eff -> PSIS weights -> shares -> replicate -> PIT -> group accumulation.  groups [n_groupings][N] labels, n_groups
 *   [n_groupings]; pit_out [N][4] = lo, eq, loo_lo, loo_eq; pareto_k_out [N] = potus_loo's pareto_k; group_out [sum n_groups][3][6];
 *   n_in_group_out [sum n_groups].  n_groupings may be 0.  The poll blocks stay within 256 MB (POTUS_PPC_BLOCK_BUDGET, bytes, overrides it: tests).
 * Refused before any kernel runs: handles with data sets (POTUS_ERR_STATE), fewer than four post-warm-up draws per chain, integrate not 0 or 1,
 * rep outside [0, 1023], a label >= its n_groups or < -1, NULL outputs, blocks that are not memory of `device`. */
enum { POTUS_PPC_BEGIN = 1, POTUS_PPC_FINISH = 2 };
int potus_poll_rep_device(int handle, int poll_begin, int poll_end, int integrate, int rep, void *yrep_out_device);
int potus_ppc_pit_device(int device, const void *yrep, const double *y, const void *log_weights, int n_polls, int n_chains, long long n_draws, double *out);
int potus_ppc_groups_device(int device, const void *yrep, const void *a1, const void *a2, const double *y, const double *n, const int32_t *groups, int n_groups,
                            int n_polls, int n_chains, long long n_draws, void *acc_device, int flags, double *group_out, long long *n_in_group);
int potus_ppc(const int *handles, int n_handles, int integrate, int rep, const int32_t *groups, int n_groupings, const int32_t *n_groups, double *pit_out,
              double *pareto_k_out, double *group_out, long long *n_in_group_out);
int potus_ppc_timing(double *ms /*[4]: log-likelihood and PSIS; shares and replicate; PIT; groups.  HIP events, calling thread's last call*/);

/* ---- joint election outcomes: what the run scripts compute from the JOINT outcome of a draw ----
 * final_2016.R:904-920 (final_2012.R, final_2008.R, README.Rmd "Final electoral college histogram") the distribution of Democratic electoral
 * votes; final_2012.R:809-839, final_2008.R:813-843 the tipping-point state; README.Rmd:481-502, :1638-1672 the p-value of the certified
 * result among the draws; and the joint / conditional win probabilities none of the marginal tables can give.  For one draw and one day,
 * x[s] = predicted_score[t, s], ev[s] non-negative integers, W = ev_to_win, w = the handle's normalised state weights:
 *   dem_ev = sum_s ev[s] 1[x[s] > 0.5];  nat = sum_s w[s] x[s] (summed s = 0 .. S-1 in order);  pop_win = nat > 0.5
 *   tipping point: states ordered by x descending when pop_win, ascending otherwise, equal x keeping the lower index first; the first state
 *     whose cumulative ev is >= W (none when sum ev < W).  As in the reference the order follows the POPULAR-vote winner, not the
 *     electoral-college winner.
 *   indicators I_0..I_{S-1} = 1[x[s] > 0.5], I_S = 1[dem_ev >= W], I_{S+1} = pop_win
 * Outputs are COUNTS over the draws, per day of [day_begin, day_end) (0-based), exact and independent of how the chains are split:
 *   ev_hist      [days][sum(ev) + 1]   draws with dem_ev == k
 *   tipping      [days][S + 1]         draws whose tipping point is state s; last slot: none
 *   joint        [days][S + 2][S + 2]  draws with I_i and I_j (symmetric; the diagonal holds the marginal counts)
 *   below_actual [days][S]             draws with x[s] < actual[s]; written only when actual is given
 *   n_draws                            the draws counted
 * Any output pointer may be NULL.  sum(ev) may be at most 2047 (the kernel's histogram), S at most 63.
 * potus_outcomes pools the post-warm-up draws of handles that hold one posterior (they may have saved different numbers of draws); the
 * counting runs on the first handle's GPU, blocks of other GPUs come over by peer copies.  Warm-up rows saved with save_warmup = 1 are LEFT
 * OUT, as potus_loo and potus_diagnostics leave them out -- potus_posterior_summary pools every saved row, so the two agree only for
 * save_warmup = 0.  predicted_score never visits the host. */
int potus_outcomes(const int *handles, int n_handles, int day_begin, int day_end, const int32_t *ev, int ev_to_win, const double *actual /*[S] or NULL*/,
                   long long *ev_hist, long long *tipping, long long *joint, long long *below_actual, long long *n_draws);
/* The same for a block [n_draws][n_days][S] of doubles that already sits in DEVICE memory of GPU `device` (what a multi-rank job holds after its
 * all-gather); w [S]: the weights of the national vote, used as given (normalise them to sum to one). */
int potus_outcomes_device(int device, const void *block, long long n_draws, int n_days, int S, const double *w, const int32_t *ev, int ev_to_win,
                          const double *actual /*[S] or NULL*/, long long *ev_hist, long long *tipping, long long *joint, long long *below_actual,
                          long long *n_draws_out);
/* Milliseconds of the calling thread's last potus_outcomes[_device]: ms[3] = producing and gathering predicted_score (host clock), cutting the
 * day range out of it (host clock), the counting kernel (HIP events). */
int potus_outcomes_timing(double *ms /*[3]*/);

/* ---- conditional forecasts and the covariance of the state scores ----
 * final_2016.R:710-715 calls cor() on the election-day scores of the draws (the older run files cov(p[, election_day, ])); and the reader of a
 * forecast asks for it GIVEN an event: the Democrat carries Florida, loses Pennsylvania, the national vote lands between 48 % and 52 %.
 * For one draw and one day the S + 1 COORDINATES are x[s] = predicted_score[t, s] (s < S) and x[S] = nat = sum_s w[s] x[s], summed
 * s = 0 .. S-1 in order with the handle's normalised weights.  The CONDITION reads nat exactly as potus_outcomes sums it (each step one fused
 * multiply-add), so that `nat > 0.5` here and pop_win there can never disagree; coordinate S of mean and cov is the same in-order sum with every
 * product and every sum rounded on its own -- what the loop gives in plain C on any host, so a host restatement holds it bit for bit.
 *   Condition: given cond_day, lo[S+1] and hi[S+1], a draw is KEPT iff lo[k] < x_cond_day[k] <= hi[k] for every k.  -inf / +inf leave a
 *     coordinate free; "wins s" is lo[s] = 0.5, "does not win s" is hi[s] = 0.5 (the strict rule of final_2016.R:817: complementary
 *     conditions partition the draws); lo = hi = NULL keeps every draw.  A NaN bound or lo[k] >= hi[k] is refused (POTUS_ERR_ARG) before
 *     the device is touched.
 *   Outputs, per day of [day_begin, day_end) (0-based), over the kept draws only:
 *     n_kept, n_draws                    P(condition) = n_kept / n_draws
 *     mean    [days][S + 1]              sum / n_kept, one division
 *     cov     [days][S + 1][S + 1]       two-pass: products of deviations from that mean, ddof 1; symmetric, both triangles written
 *     ev_hist, tipping, joint            potus_outcomes' counts of the kept draws, same shapes and meaning
 *   n_kept = 0: mean and cov NaN, counts zero, status OK.  n_kept = 1: mean is the draw, cov NaN.  Any output pointer may be NULL; ev may be
 *   NULL when all three count outputs are.  The limits are potus_outcomes': S <= 63, sum(ev) <= 2047.
 * The draws are taken in CANONICAL order -- chain after chain in the order the handles are listed, each chain's post-warm-up draws in iteration
 * order: the row order of potus_extract_matrix -- and every floating-point sum runs in an order fixed by that sequence alone (chunks of 1024
 * kept draws, chunk partials added in chunk order, no floating-point atomics): two handles of two chains give the bytes of one handle of
 * four.  Warm-up rows of save_warmup = 1 are left out; handles with potus_set_datasets are refused (POTUS_ERR_STATE).  cond_day may lie
 * outside [day_begin, day_end).  predicted_score never visits the host. */
int potus_scenario(const int *handles, int n_handles, int cond_day, const double *lo /*[S+1] or NULL*/, const double *hi /*[S+1] or NULL*/,
                   int day_begin, int day_end, const int32_t *ev, int ev_to_win,
                   long long *n_kept, long long *n_draws, double *mean, double *cov,
                   long long *ev_hist, long long *tipping, long long *joint);
/* The same for a block [n_draws][n_days][S] of doubles in DEVICE memory of GPU `device`, its draws in the order they are to be summed in;
 * w [S] as in potus_outcomes_device; cond_day indexes the block's days; the outputs cover all of them. */
int potus_scenario_device(int device, const void *block /*[n_draws][n_days][S]*/, long long n_draws, int n_days, int S, const double *w,
                          int cond_day, const double *lo, const double *hi, const int32_t *ev, int ev_to_win,
                          long long *n_kept, double *mean, double *cov, long long *ev_hist, long long *tipping, long long *joint);
/* Milliseconds of the calling thread's last potus_scenario[_device]: producing and gathering predicted_score (host clock), cutting the days
 * out of it (host clock), keeping and compacting (host clock), the moments (HIP events), the counting kernel (HIP events). */
int potus_scenario_timing(double *ms /*[5]*/);

/* ---- proper scoring rules of the joint forecast against the result ----
 * What scoringRules gives an R user as crps_sample, es_sample, vs_sample and dss_sample, for the n draws of predicted_score of every day.
 * INPUT: a block x [n_draws][n_days][S], draws in canonical order (the block of potus_outcomes_device and potus_scenario_device); w [S] the
 *   normalised national weights and ev [S] the electoral votes; actual [S + 2] = the certified two-party share per state, the national share,
 *   the Democratic electoral votes; use [S] of 0 / 1: the m states that enter the multivariate scores; vs_p in (0, 2].
 * UNIVARIATE, uni_out [days][S + 2][7], per day and column c -- the S states, the national vote sum_s w[s] x[s] and the electoral votes
 *   sum_s ev[s] 1[x[s] > 0.5] of a draw (ev_to_win is taken for symmetry with potus_timeline and not used: the votes are scored as a count) -- over the
 *   column's draws sorted ascending, x_(1..n), y = actual[c]:
 *     [0] crps       (2 / n^2) sum_i (x_(i) - y)(n 1[y < x_(i)] - i + 1/2)  =  mean|x - y| - sum_i sum_j |x_i - x_j| / (2 n^2)   (crps_sample, edf)
 *     [1] pit_lo     #{x < y} / n
 *     [2] pit_hi     #{x <= y} / n
 *     [3] dss        log v + (y - mean)^2 / v, v the variance (ddof 1, two passes); NaN when v = 0 (every draw the same value) or n = 1
 *     [4] interval   (u - l) + 40 (l - y)+ + 40 (y - u)+, l and u the type-7 quantiles at 0.025 and 0.975
 *     [5] ae_median  |median - y|, the type-7 median
 *     [6] se_mean    (mean - y)^2
 * MULTIVARIATE, multi_out [days][3], per day over the m used states, x_i and y in R^m:
 *     [0] energy     (1 / n) sum_i |x_i - y| - (1 / (2 n^2)) sum_i sum_j |x_i - x_j|, Euclidean norm, every pair by direct differences
 *     [1] variogram  sum_{a < b} (|y_a - y_b|^p - (1 / n) sum_i |x_ia - x_ib|^p)^2, p = vs_p; 0 when m = 1
 *     [2] dss        log det Sigma + (y - mu)' Sigma^-1 (y - mu), Sigma the ddof-1 covariance by two passes (potus_scenario's); NaN when n <= m or
 *                    a Cholesky pivot is not positive, with status OK
 * NOT FINITE: a value that is not finite in a column makes that (day, column)'s seven outputs NaN; in a state it also makes that day's national and
 *   electoral-vote rows NaN and, if the state is used, that day's three multivariate outputs.  No other day is affected.
 * Every sum runs in an order fixed by (n, the used states) and two constants of the library (tiles of 128 draws, chunks of 64): a day has the same
 *   bytes alone and inside a range, for any launch shape.  No floating-point atomics.
 * REFUSED before the device is touched: S > 63 and more than 16 384 draws per block or data set (POTUS_ERR_UNSUPPORTED); an actual that is not
 *   finite or a share outside [0, 1], use all zero, vs_p outside (0, 2], a bad day range, a null argument (POTUS_ERR_ARG). */
int potus_forecast_scores_device(int device, const void *block /*[n_draws][n_days][S]*/, long long n_draws, int n_days, int S, const double *w,
                                 const double *ev, int ev_to_win, const double *actual /*[S + 2]*/, const int32_t *use /*[S]*/, double vs_p,
                                 double *uni_out, double *multi_out);
/* The same over the pooled post-warm-up draws of handles that hold one posterior, pooled exactly as potus_scenario pools them (canonical
 * order, warm-up rows left out, handles with data sets refused with POTUS_ERR_STATE), days [day_begin, day_end). */
int potus_forecast_scores(const int *handles, int n_handles, int day_begin, int day_end, const double *ev, int ev_to_win,
                          const double *actual, const int32_t *use, double vs_p, double *uni_out, double *multi_out, long long *n_draws_out);
/* The same for every data set of one handle (run dates, prior settings) in one call, on potus_timeline's scores: the columns, the energy and
 * the variogram score of all data sets in one launch each; the joint dss data set after data set (its moments are potus_scenario's kernels, which
 * take one block of draws).  uni_out [n][days][S + 2][7], multi_out [n][days][3], n_draws_out [n].  A data set with a failed chain gets NaN and
 * n_draws_out = 0. */
int potus_forecast_scores_datasets(int handle, int day_begin, int day_end, const double *ev, int ev_to_win, const double *actual,
                                   const int32_t *use, double vs_p, double *uni_out, double *multi_out, int32_t *n_draws_out);
/* Milliseconds (HIP events) of the calling thread's last potus_forecast_scores[_device|_datasets]: the columns, the energy score, the variogram
 * score, the joint DSS (moments, factor and solve). */
int potus_forecast_scores_timing(double *ms /*[4]*/);

/* ---- .C()-callable wrappers (int* / double* / char** only) ---- */
void potus_R_create(int *dims /*[8]: N_nat,N_state,T,S,P,M,Pop,variant*/,
                    int *state, int *day_state, int *day_national, int *poll_state,
                    int *poll_national, int *poll_mode_state, int *poll_mode_national,
                    int *poll_pop_state, int *poll_pop_national, int *n_democrat_national,
                    int *n_two_share_national, int *n_democrat_state, int *n_two_share_state,
                    double *unadjusted_national, double *unadjusted_state, double *mu_b_prior,
                    double *state_weights, double *scalars /*[9]: sigma_c,sigma_m,sigma_pop,
                    sigma_noise_nat,sigma_noise_state,sigma_e_bias,random_walk_scale,
                    mu_b_T_scale,polling_bias_scale*/,
                    double *state_covariance_0,
                    int *iopts /*[12]: chains,chain_id_offset,num_warmup,num_samples,max_depth,
                    device,save_warmup,cus_per_chain,metric,twin,metric_storage,pooled_metric*/,
                    double *dopts /*[7]: delta,gamma,kappa,t0,stepsize,init_radius,seed (an integer < 2^53:
                    R's own integers have 32 bits)*/,
                    int *handle, int *status);
void potus_R_init(int *handle, int *status);
void potus_R_run(int *handle, int *n_iter, int *status);
void potus_R_run_many(int *handles, int *n_handles, int *n_iter, int *status);
void potus_R_num_columns(int *handle, int *D, int *n_cols, int *status);
void potus_R_write_array(int *handle, int *col_begin, int *col_end, double *out, int *status);
void potus_R_write_stan_csv(int *handle, char **dir, char **basename, int *status);
void potus_R_saved_count(int *handle, int *n_saved, int *status);
void potus_R_posterior_summary(int *handles, int *n_handles, double *ev, double *state_out, double *natl_out, double *ev_out, int *status);
void potus_R_diagnostics(int *handles, int *n_handles, int *cols /*[2]: col_begin, col_end*/, double *rhat_out, double *ess_bulk_out, int *status);
void potus_R_monitor(int *handles, int *n_handles, int *cols /*[2]: col_begin, col_end*/, double *probs, int *n_probs, double *out, int *status);
void potus_R_check_convergence(int *handles, int *n_handles, double *limits /*[2]: rhat_below, ess_at_least*/, int *converged, double *out /*[2]: rhat_max, ess_bulk_min*/,
                                int *status);
void potus_R_backtest_scores(double *state_out, int *dims /*[3]: T, S, day*/, double *ev, int *won, double *out /*[3]*/, int *status);
void potus_R_last_error(char **buf, int *len);
void potus_R_destroy(int *handle, int *status);
void potus_R_set_datasets(int *handle, int *n_datasets, int *n_democrat_state, int *n_democrat_national, int *status);
void potus_R_set_datasets_ex(int *handle, int *n_datasets, int *n_democrat_state, int *n_democrat_national, int *n_two_share_state, int *n_two_share_national,
                             int *has_prior, double *mu_b_prior, int *has_scale, double *mu_b_T_scale, int *status);
void potus_R_timeline(int *handle, int *day_begin, int *day_end, double *ev, int *ev_to_win, double *state_out, double *natl_out, double *ev_out,
                      int *n_draws_out, int *status);
void potus_R_set_datasets_grid(int *handle, int *n_datasets, int *n_democrat_state, int *n_democrat_national, int *n_two_share_state, int *n_two_share_national,
                               int *has /*[3]: mu_b_prior, mu_b_T_scale, scales given*/, double *mu_b_prior, double *mu_b_T_scale, double *scales /*[n][9]*/,
                               int *status);
void potus_R_grid_compare(int *handle, int *iargs /*[4]: base (0-based), day_begin, day_end, ev_to_win*/, double *ev, double *out /*[n][days][S + 2][3]*/,
                          int *n_draws_out, int *status);
void potus_R_cv_lpd(int *handle, int *held_state, int *held_national, int *integrate, double *lpd_out, int *n_draws_out, int *status);
void potus_R_optimize(int *handle, int *iopts /*[7]: jacobian, history_size, iter, path_offset, n_paths, q0 given, rows wanted*/,
                      double *dopts /*[6]: init_alpha, tol_obj, tol_rel_obj, tol_grad, tol_rel_grad, tol_param*/, double *q0, double *q_out, double *lp_out,
                      double *gnorm_out, int *info_out, int *cols /*[2]: col_begin, col_end*/, double *row_out, int *status);
void potus_R_pathfinder(int *handle, int *iopts /*[9]: history_size, num_elbo_draws, num_draws, draw_offset, path_offset, max_lbfgs_iters, L-BFGS history, n_paths, q0 given*/,
                        double *dopts /*[6]: init_alpha, tol_obj, tol_rel_obj, tol_grad, tol_rel_grad, tol_param*/, double *q0, int *info_out /*[n_paths][4]*/,
                        double *elbo_out, int *kept_out /*[n_paths][max_lbfgs_iters + 1]*/, double *q_out, double *lp_out, double *lq_out, int *status);
void potus_R_variational(int *handle, int *iopts /*[11]: iter, grad_samples, elbo_samples, eval_elbo, adapt_engaged, adapt_iter, output_samples, draw_offset, run_offset, n_runs, q0 given*/,
                         double *dopts /*[3]: eta, tol_rel_obj, elbo_offset*/, double *q0, int *info_out /*[n_runs][6]*/, double *mu_out, double *omega_out,
                         double *elbo_out /*[n_runs][iter / eval_elbo + 1]*/, double *adapt_elbo_out /*[n_runs][5]*/, double *q_out, double *lp_out,
                         double *lq_out, int *status);
void potus_R_laplace(int *handle, int *iopts /*[6]: jacobian, draw_offset, n_modes, n_draws, u given, precision wanted*/, double *h, double *mode, double *u,
                     double *q_out, double *lp_out, double *lp_approx_out, double *info_out, double *precision_out, int *status);
void potus_R_simulate_prior(int *handle, double *seed, int *dims /*[2]: n_sims, sim_offset*/, double *q_out, int *n_democrat_state_out,
                            int *n_democrat_national_out, int *status);
void potus_R_sbc_ranks(int *handle, double *truth, int *cols /*[3]: col_begin, col_end, thin*/, int *less, int *equal, int *L, int *status);
void potus_R_constrain(int *handle, double *q, int *n, int *cols /*[2]: col_begin, col_end*/, double *out, int *status);
void potus_R_loo_influence(int *handles, int *n_handles, int *iopts /*[4]: integrate, ev_to_win, day (0-based; -1: election day), diag*/, double *ev,
                           double *loo_mean /*[N][2S+3]*/, double *var_out, double *post_out /*[2S+3]*/, double *pareto_k /*[N]*/, double *ess, double *khat,
                           int *status);
void potus_R_loo_predict(int *handles, int *n_handles, int *integrate, double *out /*[N][5]*/, double *pareto_k /*[N]*/, int *status);
/* potus_ppc; the counts of n_in_group as doubles */
void potus_R_ppc(int *handles, int *n_handles, int *iopts /*[3]: integrate, rep, n_groupings*/, int *groups /*[n_groupings][N]*/, int *n_groups /*[n_groupings]*/,
                 double *pit_out /*[N][4]*/, double *pareto_k /*[N]*/, double *group_out /*[sum n_groups][3][6]*/, double *n_in_group /*[sum n_groups]*/, int *status);
void potus_R_loo_moment_match(int *model_handle, int *handles, int *n_handles, int *iopts /*[5]: integrate, max_iters, split, cov, n_polls (0: every poll)*/,
                              double *k_threshold, int *polls, double *pointwise /*[n_polls of the data][5], in and out*/, double *estimates_out,
                              int *info_out /*[n_polls of the data][6]*/, int *status);
void potus_R_loo(int *handles, int *n_handles, int *iopts /*[2]: integrate, r_eff given*/, double *r_eff, double *pointwise_out /*[n_polls][5]*/,
                 double *estimates_out /*[3][2]*/, int *status);
void potus_R_outcomes(int *handles, int *n_handles, int *iopts /*[4]: day_begin, day_end, ev_to_win, actual given*/, int *ev, double *actual,
                      double *ev_hist, double *tipping, double *joint, double *below_actual, double *n_draws, int *status);
/* counts as doubles, like potus_R_outcomes; n [2] = n_kept, n_draws; mean and cov are written when iopts[5], the counts when iopts[6] */
void potus_R_scenario(int *handles, int *n_handles, int *iopts /*[7]: cond_day, day_begin, day_end, ev_to_win, bounds given, moments wanted, counts wanted*/,
                      double *lo, double *hi, int *ev, double *n /*[2]*/, double *mean, double *cov, double *ev_hist, double *tipping, double *joint, int *status);
/* potus_forecast_scores; n_draws as a double */
void potus_R_forecast_scores(int *handles, int *n_handles, int *iopts /*[3]: day_begin, day_end, ev_to_win*/, double *ev, double *actual /*[S + 2]*/,
                             int *use, double *vs_p, double *uni_out, double *multi_out, double *n_draws, int *status);

#ifdef __cplusplus
}
#endif
#endif /* POTUS_HMC_H */
