# potus_sampling.R -- R host shim over libpotus_hmc.so: plain .C() everywhere (no Rcpp, no Rinternals.h needed), and -- where R/src/potus_call.c has been
# built (R CMD SHLIB) and loaded -- .Call() for the calls that return draws: the result is then allocated once and filled in place (long vectors welcome),
# where .C() copies every argument in and out and the shim permutes the block once more.
#
# Drop-in for the sampler call of the reference scripts:
#
#   scripts/model/final_2016.R:532-543
#     model <- cmdstanr::cmdstan_model("scripts/model/poll_model_2020.stan", compile=TRUE, force=TRUE)
#     fit   <- model$sample(data = data, seed = 1843, parallel_chains = n_cores, chains = n_chains,
#                           iter_warmup = n_warmup, iter_sampling = n_sampling, refresh = n_refresh)
#     out   <- rstan::read_stan_csv(fit$output_files())
#
# becomes
#
#   source("R/potus_sampling.R"); potus_load("us_potus_model_amd/libpotus_hmc.so")
#   fit <- potus_sample(data, variant = "full", seed = 1843, chains = n_chains,
#                       iter_warmup = n_warmup, iter_sampling = n_sampling, refresh = n_refresh)
#   mu_b <- potus_extract(fit, "mu_b")             # = rstan::extract(out, pars = "mu_b")[[1]]
#   out  <- rstan::read_stan_csv(potus_output_files(fit, tempdir()))   # the literal plumbing, if a stanfit is needed
#
# NOTE: R is not installed in the build image, so this file itself has never run; every .C() call below is
# replayed argument for argument (int* / double* / char** only, outputs through the same buffers) by
# tests/test_gpu_boundary.py::test_r_entry_points_replay_the_shim with ctypes.

# path: libpotus_hmc.so; call_path: R/src/potus_call.so (optional: without it every call goes through .C())
potus_load <- function(path, call_path = NULL) {
  dyn.load(path, local = FALSE)                  # (global: potus_call.so resolves the C ABI against it)
  if (!is.null(call_path)) dyn.load(call_path)
  invisible(is.loaded("potus_call_extract"))
}

.potus_check <- function(status) {
  if (status != 0L) {
    msg <- .C("potus_R_last_error", buf = paste(rep(" ", 512), collapse = ""), len = 512L)$buf
    stop(sprintf("libpotus_hmc error %d: %s", status, trimws(msg)), call. = FALSE)
  }
}

# potus_R_create on an R data list; iopts / dopts as in include/potus_hmc.h.  Returns the .C() result (handle, status).
.potus_create <- function(data, variant, iopts, dopts) {
  full <- variant == "full"
  iv <- function(x, n) if (is.null(x)) integer(max(n, 1)) else as.integer(x)
  dv <- function(x, n) if (is.null(x)) double(max(n, 1)) else as.double(x)
  Ns <- as.integer(data$N_state_polls); Nn <- as.integer(data$N_national_polls)
  dims <- as.integer(c(Nn, Ns, data$T, data$S, data$P, if (full) data$M else 0L, if (full) data$Pop else 0L,
                       if (full) 0L else 1L))
  scalars <- as.double(c(data$sigma_c, if (full) data$sigma_m else 0, if (full) data$sigma_pop else 0,
                         data$sigma_measure_noise_national, data$sigma_measure_noise_state,
                         if (full) data$sigma_e_bias else 0, data$random_walk_scale, data$mu_b_T_scale,
                         data$polling_bias_scale))
  .C("potus_R_create", dims,
     iv(data$state, Ns), iv(data$day_state, Ns), iv(data$day_national, Nn), iv(data$poll_state, Ns),
     iv(data$poll_national, Nn), iv(data$poll_mode_state, Ns), iv(data$poll_mode_national, Nn),
     iv(data$poll_pop_state, Ns), iv(data$poll_pop_national, Nn),
     iv(data$n_democrat_national, Nn), iv(data$n_two_share_national, Nn),
     iv(data$n_democrat_state, Ns), iv(data$n_two_share_state, Ns),
     dv(data$unadjusted_national, Nn), dv(data$unadjusted_state, Ns),
     as.double(data$mu_b_prior), as.double(data$state_weights), scalars,
     as.double(data$state_covariance_0),           # column-major, as R stores it
     as.integer(iopts), as.double(dopts), handle = integer(1), status = integer(1))
}

# gpus: device ids; the chains are dealt to them in contiguous blocks (chain ids, hence RNG streams and draws, do not
# depend on the number of GPUs) and all devices advance together under potus_R_run_many.
potus_sample <- function(data, variant = c("full", "no_mode_adjustment"), seed = 1843, chains = 4,
                         parallel_chains = chains, iter_warmup = 1000, iter_sampling = 1000, refresh = 100,
                         adapt_delta = 0.8, max_treedepth = 10, init = 2, device = 0, chain_id_offset = 0,
                         save_warmup = FALSE, gpus = device, cus_per_chain = 0, metric = c("diag_e", "dense_e"), twin = -1,
                         metric_storage = c("f64", "f32"), rhat_stop = NULL, ess_stop = 400, pooled_metric = FALSE) {
  # pooled_metric (off by default; metric = "dense_e" only; a DEVIATION from Stan / CmdStan, whose chains are separate processes): ONE inverse metric
  # per GPU, adapted at every window end from the draws of all chains on it (potus_opts.pooled_metric, include/potus_hmc.h).
  # rhat_stop (off by default; a DEVIATION from Stan / the reference, which always run iter_sampling iterations, final_2016.R:539): after every
  # `refresh` transitions of the sampling phase the pooled chains' rank-normalised split R-hat / bulk ESS of lp__ and mu_b[, T] are taken on the
  # device (potus_R_check_convergence) and sampling ends once every R-hat < rhat_stop and every bulk ESS >= ess_stop; the draws up to that point
  # are those of the uninterrupted run.
  metric_storage <- match.arg(metric_storage)
  metric <- match.arg(metric)
  variant <- match.arg(variant)
  full <- variant == "full"
  gpus <- as.integer(gpus)
  per <- rep(chains %/% length(gpus), length(gpus)) + (seq_along(gpus) <= chains %% length(gpus))   # chains per device
  first <- cumsum(c(0L, per))[seq_along(per)]
  handles <- integer(0); counts <- integer(0)
  for (g in seq_along(gpus)) {
    if (per[g] == 0L) next
    res <- .potus_create(data, variant,
                         as.integer(c(per[g], chain_id_offset + first[g], iter_warmup, iter_sampling, max_treedepth, gpus[g],
                                      as.integer(save_warmup), cus_per_chain, if (metric == "dense_e") 1L else 0L, twin,
                                      if (metric_storage == "f32") 1L else 0L, if (isTRUE(pooled_metric)) 1L else 0L)),
                         as.double(c(adapt_delta, 0.05, 0.75, 10, 1, init, seed)))   # the seed as a double: exact to 2^53
    .potus_check(res$status)
    .potus_check(.C("potus_R_init", res$handle, status = integer(1))$status)
    handles <- c(handles, res$handle); counts <- c(counts, per[g])
  }
  total <- iter_warmup + iter_sampling
  done <- 0L
  chunk <- if (is.null(refresh) || refresh <= 0) total else as.integer(refresh)
  convergence <- NULL
  while (done < total) {                     # chunked so that R can print progress / be interrupted
    n <- min(chunk, total - done)
    if (done < iter_warmup) n <- min(n, iter_warmup - done)
    .potus_check(.C("potus_R_run_many", as.integer(handles), length(handles), as.integer(n), status = integer(1))$status)
    done <- done + n
    message(sprintf("Iteration: %5d / %d [%3d%%]  (%s)", done, total, as.integer(100 * done / total),
                    if (done <= iter_warmup) "Warmup" else "Sampling"))
    if (!is.null(rhat_stop) && done > iter_warmup && done < total) {
      cv <- .C("potus_R_check_convergence", as.integer(handles), length(handles), as.double(c(rhat_stop, ess_stop)), converged = integer(1), out = double(2),
               status = integer(1))
      .potus_check(cv$status)
      convergence <- rbind(convergence, data.frame(iterations = done, rhat_max = cv$out[1], ess_bulk_min = cv$out[2], converged = cv$converged == 1L))
      if (cv$converged == 1L) {
        message(sprintf("Stopped after %d sampling iterations: R-hat %.4f < %g, bulk ESS %.0f >= %g", done - iter_warmup, cv$out[1], rhat_stop, cv$out[2], ess_stop))
        break
      }
    }
  }
  info <- .C("potus_R_num_columns", handles[1], D = integer(1), n_cols = integer(1), status = integer(1))
  .potus_check(info$status)
  saved <- .C("potus_R_saved_count", handles[1], n_saved = integer(1), status = integer(1))   # what the library holds, not what was asked for
  .potus_check(saved$status)
  structure(list(handle = handles[1], handles = handles, chains_per_handle = counts, D = info$D, n_cols = info$n_cols, chains = chains,
                 n_saved = saved$n_saved, data = data, variant = variant, convergence = convergence,
                 model_name = if (full) "poll_model_2020_model" else "poll_model_2020_no_mode_adjustment_model"),
            class = "potus_fit")
}

# rstan::sampling() surface (final_2016.R:525-529, scripts/deprecated/R/Refactored/poll_run_v9.R:387-390): `iter` counts
# warm-up + sampling, `warmup` defaults to iter / 2, control = list(adapt_delta =, max_treedepth =).
potus_sampling <- function(data, variant = c("full", "no_mode_adjustment"), chains = 4, iter = 2000, warmup = floor(iter / 2),
                           seed = 1843, refresh = max(iter %/% 10, 1), init = 2, control = list(), gpus = 0L, ...) {
  potus_sample(data, variant = match.arg(variant), seed = seed, chains = chains, iter_warmup = warmup, iter_sampling = iter - warmup,
               refresh = refresh, init = if (is.numeric(init)) init else 2,
               adapt_delta = if (is.null(control$adapt_delta)) 0.8 else control$adapt_delta,
               max_treedepth = if (is.null(control$max_treedepth)) 10 else control$max_treedepth, gpus = gpus, ...)
}

# column ranges of the CmdStan row, 0-based [begin, end): same arithmetic as _abi.column_layout
.potus_layout <- function(fit) {
  d <- fit$data; full <- fit$variant == "full"
  S <- d$S; T <- d$T; P <- d$P; Ns <- d$N_state_polls; Nn <- d$N_national_polls
  blocks <- list(raw_mu_b_T = S, raw_mu_b = c(S, T), raw_mu_c = P)
  if (full) blocks <- c(blocks, list(raw_mu_m = d$M, raw_mu_pop = d$Pop, mu_e_bias = integer(0), rho_e_bias = integer(0), raw_e_bias = T))
  blocks <- c(blocks, list(raw_measure_noise_national = Nn, raw_measure_noise_state = Ns, raw_polling_bias = S,
                           mu_b = c(S, T), mu_c = P))
  if (full) blocks <- c(blocks, list(mu_m = d$M, mu_pop = d$Pop, e_bias = T))
  blocks <- c(blocks, list(polling_bias = S, national_mu_b_average = T, national_polling_bias_average = integer(0)))
  if (full) blocks <- c(blocks, list(sigma_rho = integer(0)))
  blocks <- c(blocks, list(logit_pi_democrat_state = Ns, logit_pi_democrat_national = Nn, predicted_score = c(T, S)))
  col <- 7L; out <- list()
  for (nm in names(blocks)) { n <- as.integer(prod(blocks[[nm]])); out[[nm]] <- list(begin = col, end = col + n, dims = blocks[[nm]]); col <- col + n }
  out
}

# rstan::extract(out, pars = name)[[1]] : array [draws, dims...], chains merged (chain-major)
potus_extract <- function(fit, name) {
  b <- .potus_layout(fit)[[name]]
  if (is.null(b)) stop("unknown parameter ", name)
  n <- b$end - b$begin
  if (is.loaded("potus_call_extract")) {          # .Call(): ONE allocation, filled in place in R's own order [draws, columns] (R/src/potus_call.c)
    a <- .Call("potus_call_extract", as.integer(fit$handles), as.integer(b$begin), as.integer(b$end))
    return(if (length(b$dims)) { dim(a) <- c(nrow(a), b$dims); a } else as.vector(a))
  }
  parts <- lapply(seq_along(fit$handles), function(g) {
    ch <- fit$chains_per_handle[g]
    res <- .C("potus_R_write_array", fit$handles[g], as.integer(b$begin), as.integer(b$end),
              out = double(fit$n_saved * ch * n), status = integer(1))
    .potus_check(res$status)
    a <- aperm(array(res$out, c(n, ch, fit$n_saved)), c(3, 2, 1))         # [iter, chain, col]
    matrix(a, fit$n_saved * ch, n)                                          # chain-major merge of this device's chains
  })
  a <- do.call(rbind, parts)                                                # devices hold consecutive chain ids
  if (length(b$dims)) array(a, c(nrow(a), b$dims)) else as.vector(a)
}

potus_output_files <- function(fit, dir, basename = "poll_model_2020") {
  for (h in fit$handles) .potus_check(.C("potus_R_write_stan_csv", h, as.character(dir), as.character(basename), status = integer(1))$status)
  file.path(dir, sprintf("%s-%d.csv", basename, seq_len(fit$chains)))       # files are numbered by chain id
}

# Posterior summaries of predicted_score computed on the device (replaces final_2016.R:708-762 and :799-823:
# no 8000 x 12954 array ever reaches R), pooled over every chain of the fit whatever the number of GPUs.
# ev: electoral votes per state in state order (states2012$ev).
# Returns list(state = array [T, S, 4] (low, high, mean, prob), national = [T, 4],
#              electoral_votes = [T, 5] (mean, median, high, low, prob >= 270)).
potus_summary <- function(fit, ev) {
  S <- fit$data$S; T <- fit$data$T
  r <- .C("potus_R_posterior_summary", as.integer(fit$handles), length(fit$handles), as.double(ev), state = double(T * S * 4),
          natl = double(T * 4), ev_out = double(T * 5), status = integer(1))
  .potus_check(r$status)
  list(state = aperm(array(r$state, c(4, T, S)), c(2, 3, 1)),       # C order [s][t][4] -> [t, s, 4]
       national = t(matrix(r$natl, nrow = 4)), electoral_votes = t(matrix(r$ev_out, nrow = 5)),
       state_raw = r$state)
}

# Rank-normalised split R-hat and bulk ESS (Vehtari et al. 2021) of the columns `pars` names, over every chain of the fit, computed on
# the device (the reference never inspects a diagnostic, final_2016.R:543-556; rstan::monitor would need the draws in R).
# Returns data.frame(column, rhat, ess_bulk); columns are 0-based positions in the CmdStan row, as in potus_extract.
potus_diagnostics <- function(fit, col_begin, col_end) {
  n <- col_end - col_begin
  if (is.loaded("potus_call_diagnostics")) {
    m <- .Call("potus_call_diagnostics", as.integer(fit$handles), as.integer(col_begin), as.integer(col_end))
    return(data.frame(column = seq(col_begin, col_end - 1L), rhat = m[, 1], ess_bulk = m[, 2]))
  }
  r <- .C("potus_R_diagnostics", as.integer(fit$handles), length(fit$handles), as.integer(c(col_begin, col_end)), rhat = double(n), ess = double(n),
          status = integer(1))
  .potus_check(r$status)
  data.frame(column = seq(col_begin, col_end - 1L), rhat = r$rhat, ess_bulk = r$ess)
}

# The posterior summary table -- rstan::summary(out, pars, probs)$summary / rstan::monitor -- formed on the device over every chain of the fit
# (post-warm-up draws): what final_2016.R:556-705 tabulates right after extract() (mean_low_high of mu_b, mean +- 1.96 sd of mu_c, mu_m, mu_pop
# and polling_bias, the means of e_bias) without the draws reaching R.  pars: names of the CmdStan row's blocks or "lp__"; NULL = the whole row.
# Returns a matrix [columns, 8 + length(probs)] with rstan-style dimnames: rows "mu_c[1]", "mu_b[1,1]", ...; columns mean, sd, mad, se_mean,
# Rhat, n_eff (bulk ESS), tail_eff, ess_mean, then "2.5%", ...  (us_potus_model_amd/monitor.py is the same in Python; DESIGN.md section 4g.)
potus_monitor <- function(fit, pars = NULL, probs = c(.025, .25, .5, .75, .975)) {
  lay <- .potus_layout(fit)
  ncols <- max(sapply(lay, function(b) b$end))
  sampler <- c("lp__", "accept_stat__", "stepsize__", "treedepth__", "n_leapfrog__", "divergent__", "energy__")
  if (is.null(pars)) {
    ranges <- list(list(begin = 0L, end = ncols))
    pars <- c(sampler, names(lay))
  } else {
    ranges <- lapply(pars, function(nm) {
      if (nm %in% sampler) return(list(begin = match(nm, sampler) - 1L, end = match(nm, sampler)))
      if (is.null(lay[[nm]])) stop("unknown parameter ", nm)
      lay[[nm]]
    })
  }
  rn <- unlist(lapply(pars, function(nm) {
    d <- lay[[nm]]$dims
    if (nm %in% sampler || length(d) == 0) return(nm)
    idx <- as.matrix(expand.grid(lapply(d, seq_len)))                       # first index fastest: CmdStan's column-major order
    paste0(nm, "[", apply(idx, 1, paste, collapse = ","), "]")
  }))
  w <- 8L + length(probs)
  rows <- lapply(ranges, function(b) {
    n <- b$end - b$begin
    r <- .C("potus_R_monitor", as.integer(fit$handles), length(fit$handles), as.integer(c(b$begin, b$end)), as.double(probs), length(probs),
            out = double(n * w), status = integer(1))
    .potus_check(r$status)
    matrix(r$out, n, w, byrow = TRUE)
  })
  m <- do.call(rbind, rows)
  dimnames(m) <- list(rn, c("mean", "sd", "mad", "se_mean", "Rhat", "n_eff", "tail_eff", "ess_mean", paste0(sapply(100 * probs, format), "%")))
  m
}

# Backtest scores of final_2016.R:925-945: EV-weighted Brier, unweighted Brier, states called correctly on `day`
# (1-based; 0 = the last day).  won: 1 where the Democrat carried the state, in state order.
potus_backtest_scores <- function(fit, summary, ev, won, day = 0L) {
  r <- .C("potus_R_backtest_scores", summary$state_raw, as.integer(c(fit$data$T, fit$data$S, day)), as.double(ev), as.integer(won),
          out = double(3), status = integer(1))
  .potus_check(r$status)
  c(ev_wtd_brier = r$out[1], unwtd_brier = r$out[2], states_correct = r$out[3])
}

potus_free <- function(fit) invisible(lapply(fit$handles, function(h) .C("potus_R_destroy", h, status = integer(1))))

# ---- simulation-based calibration (us_potus_model_amd/sbc.py is the same workflow in Python) ----
# Prior predictive simulation of `data`'s design: list(q = [n_sims, D] unconstrained draws, n_democrat_state = [n_sims, N_state_polls],
# n_democrat_national = [n_sims, N_national_polls]); simulation i is the same whatever n_sims / sim_offset it is asked with.
potus_simulate_prior <- function(data, variant = c("full", "no_mode_adjustment"), n_sims = 100, seed = 1843, sim_offset = 0, device = 0) {
  variant <- match.arg(variant)
  res <- .potus_create(data, variant, c(1L, 0L, 0L, 0L, 10L, as.integer(device), 0L, 0L, 0L, -1L, 0L, 0L), c(0.8, 0.05, 0.75, 10, 1, 2, seed))
  .potus_check(res$status)
  on.exit(.C("potus_R_destroy", res$handle, status = integer(1)))
  info <- .C("potus_R_num_columns", res$handle, D = integer(1), n_cols = integer(1), status = integer(1))
  .potus_check(info$status)
  Ns <- as.integer(data$N_state_polls); Nn <- as.integer(data$N_national_polls)
  r <- .C("potus_R_simulate_prior", res$handle, as.double(seed), as.integer(c(n_sims, sim_offset)), q = double(n_sims * info$D),
          ys = integer(max(n_sims * Ns, 1)), yn = integer(max(n_sims * Nn, 1)), status = integer(1))
  .potus_check(r$status)
  list(q = matrix(r$q, n_sims, info$D, byrow = TRUE), n_democrat_state = matrix(r$ys[seq_len(n_sims * Ns)], n_sims, Ns, byrow = TRUE),
       n_democrat_national = matrix(r$yn[seq_len(n_sims * Nn)], n_sims, Nn, byrow = TRUE), D = info$D, n_cols = info$n_cols)
}

# SBC (Talts et al. 2018): n_sims replicates simulated from the prior, fitted as chains_per_sim chains each of ONE handle (one workgroup per
# chain, diagonal metric), ranked on the device.  columns: 0-based output-row columns (>= 7), e.g. .potus_layout(fit)$mu_b$begin + ...
# Returns list(ranks [n_sims, columns] (ties broken uniformly with R's RNG), L, failed [n_sims]: every count zero, i.e. no draw kept; with one
# column a truth below every draw looks the same) -- test the ranks of the other replicates for uniformity, e.g. with chisq.test.
potus_sbc <- function(data, variant = c("full", "no_mode_adjustment"), columns, n_sims = 100, chains_per_sim = 2, iter_warmup = 1000,
                      iter_sampling = 1000, thin = 10, seed = 1843, device = 0) {
  variant <- match.arg(variant)
  sims <- potus_simulate_prior(data, variant, n_sims, seed, 0, device)
  a <- min(columns); e <- max(columns) + 1L
  cr <- .potus_create(data, variant, c(1L, 0L, 0L, 0L, 10L, as.integer(device), 0L, 0L, 0L, -1L, 0L, 0L), c(0.8, 0.05, 0.75, 10, 1, 2, seed))
  .potus_check(cr$status)
  tr <- .C("potus_R_constrain", cr$handle, as.double(t(sims$q)), as.integer(n_sims), as.integer(c(a, e)), out = double(n_sims * (e - a)), status = integer(1))
  .C("potus_R_destroy", cr$handle, status = integer(1))
  .potus_check(tr$status)
  res <- .potus_create(data, variant, c(n_sims * chains_per_sim, 0L, iter_warmup, iter_sampling, 10L, as.integer(device), 0L, 1L, 0L, 0L, 0L, 0L),
                       c(0.8, 0.05, 0.75, 10, 1, 2, seed))
  .potus_check(res$status)
  on.exit(.C("potus_R_destroy", res$handle, status = integer(1)))
  .potus_check(.C("potus_R_set_datasets", res$handle, as.integer(n_sims), as.integer(t(sims$n_democrat_state)),
                  as.integer(t(sims$n_democrat_national)), status = integer(1))$status)
  .potus_check(.C("potus_R_init", res$handle, status = integer(1))$status)
  .potus_check(.C("potus_R_run", res$handle, as.integer(iter_warmup + iter_sampling), status = integer(1))$status)
  rk <- .C("potus_R_sbc_ranks", res$handle, tr$out, as.integer(c(a, e, thin)), less = integer(n_sims * (e - a)), equal = integer(n_sims * (e - a)),
           L = integer(1), status = integer(1))
  .potus_check(rk$status)
  less <- matrix(rk$less, n_sims, e - a, byrow = TRUE)[, columns - a + 1L, drop = FALSE]
  equal <- matrix(rk$equal, n_sims, e - a, byrow = TRUE)[, columns - a + 1L, drop = FALSE]
  # a replicate whose chains failed (step-size search, initialisation) adds no draws: all its counts are zero
  failed <- rowSums(less + equal) == 0
  list(ranks = less + floor(runif(length(less)) * (equal + 1)), L = rk$L, failed = failed)
}

# ---- the forecast timeline (us_potus_model_amd/timeline.py is the same in Python; DESIGN.md section 4i) ----
# Every run date of a campaign fitted as chains of ONE handle and summarised per date on the device.  `data`: the data list of the LAST run date;
# keep_state [n, N_state_polls] / keep_national [n, N_national_polls]: logical, the polls each run date has seen (the others get n_two_share = 0);
# mu_b_prior [n, S] and mu_b_T_scale [n]: per run date, or NULL for the data list's.  days: c(first, last), 1-based, default election day alone.
# Returns list(state = [n, days, S, 4] (low, high, mean, prob), national = [n, days, 4], electoral_votes = [n, days, 5] (mean, median, high, low,
# P(>= ev_to_win)), n_draws = [n]; a run date with a failed chain has n_draws = 0 and NaN).
potus_timeline <- function(data, keep_state, keep_national, ev, mu_b_prior = NULL, mu_b_T_scale = NULL, variant = c("full", "no_mode_adjustment"),
                           chains_per_date = 4, iter_warmup = 1000, iter_sampling = 1000, days = NULL, ev_to_win = 270L, seed = 1843, device = 0) {
  variant <- match.arg(variant)
  keep_state <- matrix(as.logical(keep_state), ncol = as.integer(data$N_state_polls)); n <- nrow(keep_state)
  keep_national <- matrix(as.logical(keep_national), nrow = n)
  S <- as.integer(data$S); T <- as.integer(data$T)
  days <- if (is.null(days)) c(T, T) else as.integer(days)
  nd <- days[2] - days[1] + 1L
  counts <- function(v, keep) as.integer(t(keep * matrix(as.integer(v), n, length(v), byrow = TRUE)))   # [n][polls], row-major
  res <- .potus_create(data, variant, c(n * chains_per_date, 0L, iter_warmup, iter_sampling, 10L, as.integer(device), 0L, 1L, 0L, 0L, 0L, 0L),
                       c(0.8, 0.05, 0.75, 10, 1, 2, seed))
  .potus_check(res$status)
  on.exit(.C("potus_R_destroy", res$handle, status = integer(1)))
  .potus_check(.C("potus_R_set_datasets_ex", res$handle, n, counts(data$n_democrat_state, keep_state), counts(data$n_democrat_national, keep_national),
                  counts(data$n_two_share_state, keep_state), counts(data$n_two_share_national, keep_national),
                  as.integer(!is.null(mu_b_prior)), if (is.null(mu_b_prior)) double(1) else as.double(t(matrix(mu_b_prior, n, S))),
                  as.integer(!is.null(mu_b_T_scale)), if (is.null(mu_b_T_scale)) double(1) else as.double(mu_b_T_scale), status = integer(1))$status)
  .potus_check(.C("potus_R_init", res$handle, status = integer(1))$status)
  .potus_check(.C("potus_R_run", res$handle, as.integer(iter_warmup + iter_sampling), status = integer(1))$status)
  r <- .C("potus_R_timeline", res$handle, days[1] - 1L, days[2], as.double(ev), as.integer(ev_to_win), state = double(n * nd * S * 4),
          national = double(n * nd * 4), ev = double(n * nd * 5), n_draws = integer(n), status = integer(1))
  .potus_check(r$status)
  list(state = aperm(array(r$state, c(4, S, nd, n)), 4:1), national = aperm(array(r$national, c(4, nd, n)), 3:1),
       electoral_votes = aperm(array(r$ev, c(5, nd, n)), 3:1), n_draws = r$n_draws)
}

# ---- prior sensitivity by refit (us_potus_model_amd/sensitivity.py is the same in Python; DESIGN.md section 4t) ----
# A grid of prior scales fitted as chains of ONE handle and compared with the baseline on the device.  scales: a named list of factor vectors,
# list(sigma_c = c(0.5, 2), mu_b_T_scale = 3): the data list's own value of the scale times each factor.  Setting 1 is the data as given; with
# null = TRUE setting 2 is a second copy of it with other chains (its distance to setting 1 is the Monte-Carlo floor); then one setting per
# (scale, factor), or with product = TRUE the full factorial of the factor vectors.  days: c(first, last), 1-based, default election day alone.
# Returns list(labels, scales = [n, 9], factors = [n, 9], distance = [n, days, S + 2, 3] (w1, ks, cjs of the S state scores, the national vote
# and the electoral votes of a draw, against setting 1), n_draws = [n], and potus_timeline's state, national and electoral_votes per setting).
.potus_scale_names <- c("sigma_c", "sigma_m", "sigma_pop", "sigma_measure_noise_national", "sigma_measure_noise_state", "sigma_e_bias",
                        "random_walk_scale", "mu_b_T_scale", "polling_bias_scale")
potus_prior_grid <- function(data, scales, ev, product = FALSE, null = TRUE, variant = c("full", "no_mode_adjustment"), chains_per_setting = 4,
                             iter_warmup = 1000, iter_sampling = 1000, days = NULL, ev_to_win = 270L, seed = 1843, device = 0) {
  variant <- match.arg(variant)
  stopifnot(all(names(scales) %in% .potus_scale_names), all(is.finite(unlist(scales))), all(unlist(scales) > 0))
  base <- vapply(.potus_scale_names, function(nm) if (is.null(data[[nm]])) 0 else as.double(data[[nm]]), double(1))
  rows <- list(rep(1, 9)); labels <- "baseline"
  if (null) { rows <- c(rows, list(rep(1, 9))); labels <- c(labels, "null copy") }
  one <- function(nms, vals) { f <- rep(1, 9); f[match(nms, .potus_scale_names)] <- vals; f }
  if (product) {
    combos <- expand.grid(rev(scales))[, rev(seq_along(scales)), drop = FALSE]      # the first scale varies slowest
    for (i in seq_len(nrow(combos))) {
      rows <- c(rows, list(one(names(scales), as.double(combos[i, ]))))
      labels <- c(labels, paste(sprintf("%s x %g", names(scales), as.double(combos[i, ])), collapse = ", "))
    }
  } else for (nm in names(scales)) for (v in scales[[nm]]) { rows <- c(rows, list(one(nm, v))); labels <- c(labels, sprintf("%s x %g", nm, v)) }
  factors <- do.call(rbind, rows); n <- nrow(factors)
  sc <- sweep(factors, 2, base, `*`)
  S <- as.integer(data$S); T <- as.integer(data$T)
  days <- if (is.null(days)) c(T, T) else as.integer(days)
  nd <- days[2] - days[1] + 1L
  counts <- function(v) as.integer(rep(as.integer(v), n))                            # [n][polls], row-major: every setting sees every poll
  res <- .potus_create(data, variant, c(n * chains_per_setting, 0L, iter_warmup, iter_sampling, 10L, as.integer(device), 0L, 1L, 0L, 0L, 0L, 0L),
                       c(0.8, 0.05, 0.75, 10, 1, 2, seed))
  .potus_check(res$status)
  on.exit(.C("potus_R_destroy", res$handle, status = integer(1)))
  .potus_check(.C("potus_R_set_datasets_grid", res$handle, n, counts(data$n_democrat_state), counts(data$n_democrat_national),
                  counts(data$n_two_share_state), counts(data$n_two_share_national), c(0L, 0L, 1L), double(1), double(1), as.double(t(sc)),
                  status = integer(1))$status)
  .potus_check(.C("potus_R_init", res$handle, status = integer(1))$status)
  .potus_check(.C("potus_R_run", res$handle, as.integer(iter_warmup + iter_sampling), status = integer(1))$status)
  g <- .C("potus_R_grid_compare", res$handle, c(0L, days[1] - 1L, days[2], as.integer(ev_to_win)), as.double(ev), out = double(n * nd * (S + 2) * 3),
          n_draws = integer(n), status = integer(1))
  .potus_check(g$status)
  r <- .C("potus_R_timeline", res$handle, days[1] - 1L, days[2], as.double(ev), as.integer(ev_to_win), state = double(n * nd * S * 4),
          national = double(n * nd * 4), ev = double(n * nd * 5), n_draws = integer(n), status = integer(1))
  .potus_check(r$status)
  list(labels = labels, scales = sc, factors = factors, distance = aperm(array(g$out, c(3, S + 2, nd, n)), 4:1), n_draws = g$n_draws,
       state = aperm(array(r$state, c(4, S, nd, n)), 4:1), national = aperm(array(r$national, c(4, nd, n)), 3:1),
       electoral_votes = aperm(array(r$ev, c(5, nd, n)), 3:1))
}

# ---- PSIS-LOO (us_potus_model_amd/loo.py is the same in Python; DESIGN.md section 4e) ----
# What fit$loo() gives a cmdstanr user with a log_lik generated quantity, computed on the device over every chain of the fit (post-warm-up
# draws).  integrate = TRUE integrates each poll's own noise coordinate out of its likelihood (plain PSIS-LOO meets high Pareto k there, since
# every poll has a parameter of its own).  r_eff: one value per poll, or NULL (computed as loo::relative_eff does).
# Returns list(estimates = [3, 2] (elpd_loo, p_loo, looic) x (Estimate, SE), pointwise = [polls, 5], diagnostics = list(pareto_k)); polls are
# numbered state polls first, then national polls.
potus_loo <- function(fit, integrate = TRUE, r_eff = NULL) {
  N <- as.integer(fit$data$N_state_polls) + as.integer(fit$data$N_national_polls)
  r <- .C("potus_R_loo", as.integer(fit$handles), length(fit$handles), as.integer(c(isTRUE(integrate), !is.null(r_eff))),
          as.double(if (is.null(r_eff)) 0 else r_eff), pointwise = double(N * 5), estimates = double(6), status = integer(1))
  .potus_check(r$status)
  pw <- matrix(r$pointwise, N, 5, byrow = TRUE, dimnames = list(NULL, c("elpd_loo", "p_loo", "looic", "pareto_k", "r_eff")))
  est <- matrix(r$estimates, 3, 2, byrow = TRUE, dimnames = list(c("elpd_loo", "p_loo", "looic"), c("Estimate", "SE")))
  structure(list(estimates = est, pointwise = pw, diagnostics = list(pareto_k = pw[, "pareto_k"]),
                 y = c(fit$data$n_democrat_state, fit$data$n_democrat_national), n = c(fit$data$n_two_share_state, fit$data$n_two_share_national)),
            class = "potus_loo")
}

# Which polls move the forecast (DESIGN.md section 4r; us_potus_model_amd/loo.py influence is the same in Python): for every poll the
# leave-one-out expectation of the forecast of `day` (1-based; NULL: election day) minus its posterior mean, from one fit: potus_e_loo.  ev:
# electoral votes per state.  Columns: the S state scores, the national vote, the S indicators score > 0.5, electoral college won, electoral
# votes.  Returns delta, loo_mean, sd [polls, 2 S + 3], post_mean, pareto_k (potus_loo's; read it first: the weights are the plain PSIS
# weights), khat (the k of every mean, when diag), ess.  The fit must run one workgroup per chain.  Like the rest of this file: not run under R here.
potus_loo_influence <- function(fit, ev, day = NULL, ev_to_win = 270, integrate = TRUE, diag = TRUE) {
  N <- as.integer(fit$data$N_state_polls) + as.integer(fit$data$N_national_polls)
  S <- as.integer(fit$data$S)
  NC <- 2L * S + 3L
  r <- .C("potus_R_loo_influence", as.integer(fit$handles), length(fit$handles),
          as.integer(c(isTRUE(integrate), ev_to_win, if (is.null(day)) -1L else as.integer(day) - 1L, isTRUE(diag))), as.double(ev),
          loo_mean = double(N * NC), var = double(N * NC), post = double(NC), pareto_k = double(N), ess = double(N), khat = double(N * NC),
          status = integer(1))
  .potus_check(r$status)
  cols <- c(paste0("score_", seq_len(S)), "national", paste0("win_", seq_len(S)), "ec_win", "ev")
  m <- function(v) matrix(v, N, NC, byrow = TRUE, dimnames = list(NULL, cols))
  loo_mean <- m(r$loo_mean)
  list(delta = sweep(loo_mean, 2, r$post), loo_mean = loo_mean, sd = sqrt(pmax(m(r$var), 0)), post_mean = setNames(r$post, cols),
       pareto_k = r$pareto_k, khat = if (isTRUE(diag)) m(r$khat) else NULL, ess = r$ess)
}

# What the model expected of each poll before it saw it: the leave-one-out predictive mean and sd of its share y / n (potus_e_loo, predict),
# with the k of the mean, the in-sample mean, residual = y / n - mean and z = residual / sd.  Plain PSIS weights.  Not run under R here.
potus_loo_predict <- function(fit, integrate = TRUE) {
  N <- as.integer(fit$data$N_state_polls) + as.integer(fit$data$N_national_polls)
  r <- .C("potus_R_loo_predict", as.integer(fit$handles), length(fit$handles), as.integer(isTRUE(integrate)), out = double(N * 5),
          pareto_k = double(N), status = integer(1))
  .potus_check(r$status)
  o <- matrix(r$out, N, 5, byrow = TRUE, dimnames = list(NULL, c("mean", "variance", "sd", "pareto_k", "in_sample_mean")))
  share <- c(fit$data$n_democrat_state, fit$data$n_democrat_national) / c(fit$data$n_two_share_state, fit$data$n_two_share_national)
  data.frame(o, share = share, residual = share - o[, "mean"], z = (share - o[, "mean"]) / o[, "sd"],
             pollster = c(fit$data$poll_state, fit$data$poll_national))
}

# Posterior predictive checks (DESIGN.md section 4s; us_potus_model_amd/ppc.py check is the same in Python): could the fitted model have
# produced its polls?  Per poll the PIT and LOO-PIT sums lo = P(y_rep < y), eq = P(y_rep = y) (randomised PIT: lo + runif(N) * eq) with
# potus_loo's pareto_k; per group of `by` the realised and replicated bias, dispersion and count with their posterior predictive p-values
# (gt + eq / 2) / draws.  integrate = TRUE replicates a new poll of the same pollster, mode, population, state and day.  National polls get
# state S + 1; the no-mode variant has no mode and no population.  Plain PSIS weights.  Like the rest of this file: not run under R here.
potus_ppc <- function(fit, by = c("pollster", "mode", "population", "state"), integrate = TRUE, rep = 0L) {
  d <- fit$data
  N <- as.integer(d$N_state_polls) + as.integer(d$N_national_polls)
  full <- !is.null(d$poll_mode_state)
  if (!full) by <- setdiff(by, c("mode", "population"))
  labels <- list(pollster = c(d$poll_state, d$poll_national), mode = c(d$poll_mode_state, d$poll_mode_national),
                 population = c(d$poll_pop_state, d$poll_pop_national), state = c(d$state, rep.int(as.integer(d$S) + 1L, as.integer(d$N_national_polls))))
  sizes <- c(pollster = as.integer(d$P), mode = as.integer(d$M), population = as.integer(d$Pop), state = as.integer(d$S) + 1L)
  groups <- unlist(lapply(by, function(b) as.integer(labels[[b]]) - 1L))
  ng <- as.integer(sizes[by])
  tot <- sum(ng)
  r <- .C("potus_R_ppc", as.integer(fit$handles), length(fit$handles), as.integer(c(isTRUE(integrate), rep, length(by))), as.integer(groups), ng,
          pit = double(N * 4), pareto_k = double(N), group = double(tot * 18), n_in_group = double(tot), status = integer(1))
  .potus_check(r$status)
  pit <- matrix(r$pit, N, 4, byrow = TRUE, dimnames = list(NULL, c("lo", "eq", "loo_lo", "loo_eq")))
  g <- aperm(array(r$group, c(6, 3, tot)), c(3, 2, 1))
  dimnames(g) <- list(NULL, c("bias", "dispersion", "count"), c("T_obs", "T_rep", "gt", "eq", "lt", "p"))
  tabs <- list()
  o <- 0L
  for (k in seq_along(by)) {
    i <- o + seq_len(ng[k])
    tabs[[by[k]]] <- data.frame(label = seq_len(ng[k]), n_polls = r$n_in_group[i], T_obs = g[i, , "T_obs"], T_rep = g[i, , "T_rep"],
                                p_bias = g[i, "bias", "p"], p_dispersion = g[i, "dispersion", "p"], p_count = g[i, "count", "p"])
    o <- o + ng[k]
  }
  list(pit = pit, pareto_k = r$pareto_k, groups = tabs)
}

# loo::loo_moment_match for the polls of `loo` (a potus_loo of this fit with the same `integrate`) whose Pareto k is above k_threshold
# (0: min(1 - 1 / log10 S, 0.7)): potus_loo_moment_match (DESIGN.md section 4q; us_potus_model_amd/loo.py moment_match is the same in Python).
# polls: poll numbers from 1 (state polls first, then national polls), or NULL for every poll.  model_handle: a handle of the fit's data that
# runs one workgroup per chain with the diagonal metric (cus_per_chain = 1, twin = 0); NULL takes the fit's first handle, which a fit sampled
# with other settings does not satisfy -- the library then says so.  cov = TRUE (loo's covariance step) is refused by the library.
# Returns the potus_loo with the matched rows updated, plus k_before and mm_info [polls, 6] (accepted T1, accepted T2, candidates
# evaluated, split done, stop reason, reserved); potus_loo_compare takes it.  Like the rest of this file: not run under R here.
potus_loo_moment_match <- function(fit, loo, integrate = TRUE, polls = NULL, model_handle = NULL, max_iters = 30, split = TRUE, cov = FALSE,
                                   k_threshold = 0) {
  N <- nrow(loo$pointwise)
  mh <- if (is.null(model_handle)) fit$handles[1] else model_handle
  r <- .C("potus_R_loo_moment_match", as.integer(mh), as.integer(fit$handles), length(fit$handles),
          as.integer(c(isTRUE(integrate), max_iters, isTRUE(split), isTRUE(cov), length(polls))), as.double(k_threshold),
          as.integer(if (is.null(polls)) 0 else polls - 1), pointwise = as.double(t(loo$pointwise)), estimates = double(6), info = integer(N * 6),
          status = integer(1))
  .potus_check(r$status)
  pw <- matrix(r$pointwise, N, 5, byrow = TRUE, dimnames = dimnames(loo$pointwise))
  out <- loo
  out$pointwise <- pw
  out$estimates <- matrix(r$estimates, 3, 2, byrow = TRUE, dimnames = dimnames(loo$estimates))
  out$diagnostics <- list(pareto_k = pw[, "pareto_k"])
  out$k_before <- loo$pointwise[, "pareto_k"]
  out$mm_info <- matrix(r$info, N, 6, byrow = TRUE,
                        dimnames = list(NULL, c("accepted_t1", "accepted_t2", "rounds", "split_done", "stop", "reserved")))
  out
}

# loo::loo_compare: rows sorted by elpd_loo, elpd_diff against the best and se_diff = sqrt(N) sd(pointwise differences).  The fits must be
# of the same polls (e.g. potus_loo_compare(full = potus_loo(fit_full), no_mode = potus_loo(fit_no_mode))).
potus_loo_compare <- function(...) {
  loos <- list(...)
  nm <- names(loos)
  if (is.null(nm) || any(nm == "")) nm <- paste0("model", seq_along(loos))
  N <- nrow(loos[[1]]$pointwise)
  for (l in loos[-1])
    if (nrow(l$pointwise) != N || !identical(as.numeric(l$y), as.numeric(loos[[1]]$y)) || !identical(as.numeric(l$n), as.numeric(loos[[1]]$n)))
      stop("potus_loo_compare: the fits were not fitted to the same polls")
  ord <- order(sapply(loos, function(l) l$estimates["elpd_loo", "Estimate"]), decreasing = TRUE)
  best <- loos[[ord[1]]]$pointwise[, "elpd_loo"]
  out <- t(sapply(seq_along(ord), function(r) {
    l <- loos[[ord[r]]]
    d <- l$pointwise[, "elpd_loo"] - best
    c(elpd_diff = sum(d), se_diff = if (r == 1) 0 else sqrt(N) * sd(d), elpd_loo = l$estimates[1, 1], se_elpd_loo = l$estimates[1, 2],
      p_loo = l$estimates[2, 1], se_p_loo = l$estimates[2, 2], looic = l$estimates[3, 1], se_looic = l$estimates[3, 2])
  }))
  rownames(out) <- nm[ord]
  out
}

# ---- exact K-fold cross-validation (us_potus_model_amd/crossval.py is the same in Python; DESIGN.md section 4j) ----
# Every fold refitted, all folds as the chains of ONE launch: fold k is a data set in which the polls with fold == k keep their place in the design with
# n_two_share = 0, and potus_cv_lpd evaluates each of them under the draws of the fold that did not see it (real y and n; integrate = TRUE: the poll's
# noise coordinate integrated over its N(0,1) prior, the exact predictive density).  fold: one number in 1..K per poll, state polls then national
# polls (e.g. sample(rep_len(1:K, N)), or one number per pollster for leave-pollster-out).
# Returns list(pointwise = [N, 2] (elpd, mcse: delta method, draws taken as independent), elpd_kfold, se = sqrt(N) sd(elpd), fold, n_draws [K]);
# a fold with a failed chain is an error.
potus_kfold <- function(data, fold, variant = c("full", "no_mode_adjustment"), chains_per_fold = 4, iter_warmup = 1000, iter_sampling = 1000,
                        integrate = TRUE, seed = 1843, device = 0) {
  variant <- match.arg(variant)
  Ns <- as.integer(data$N_state_polls); Nn <- as.integer(data$N_national_polls); N <- Ns + Nn
  fold <- as.integer(fold); K <- max(fold)
  if (length(fold) != N || min(fold) < 1L) stop("potus_kfold: fold must hold one number in 1..K per poll (state polls, then national polls)")
  held <- outer(seq_len(K), fold, "==")                                                    # [K, N]
  counts <- function(v, keep) as.integer(t(keep * matrix(as.integer(v), K, length(v), byrow = TRUE)))   # [K][polls], row-major
  res <- .potus_create(data, variant, c(K * chains_per_fold, 0L, iter_warmup, iter_sampling, 10L, as.integer(device), 0L, 1L, 0L, 0L, 0L, 0L),
                       c(0.8, 0.05, 0.75, 10, 1, 2, seed))
  .potus_check(res$status)
  on.exit(.C("potus_R_destroy", res$handle, status = integer(1)))
  ks <- !held[, seq_len(Ns), drop = FALSE]; kn <- !held[, Ns + seq_len(Nn), drop = FALSE]
  .potus_check(.C("potus_R_set_datasets_ex", res$handle, K, counts(data$n_democrat_state, ks), counts(data$n_democrat_national, kn),
                  counts(data$n_two_share_state, ks), counts(data$n_two_share_national, kn), 0L, double(1), 0L, double(1), status = integer(1))$status)
  .potus_check(.C("potus_R_init", res$handle, status = integer(1))$status)
  .potus_check(.C("potus_R_run", res$handle, as.integer(iter_warmup + iter_sampling), status = integer(1))$status)
  if (is.loaded("potus_call_cv_lpd")) {
    v <- .Call("potus_call_cv_lpd", res$handle, as.integer(t(!ks)), as.integer(t(!kn)), K, as.integer(isTRUE(integrate)))
    r <- list(lpd = v[seq_len(K * N * 2)], n_draws = as.integer(v[K * N * 2 + seq_len(K)]))
  } else {
    r <- .C("potus_R_cv_lpd", res$handle, as.integer(t(!ks)), as.integer(t(!kn)), as.integer(isTRUE(integrate)), lpd = double(K * N * 2),
            n_draws = integer(K), status = integer(1))
    .potus_check(r$status)
  }
  if (any(r$n_draws == 0L)) stop(sprintf("potus_kfold: fold %d: a chain of its fit failed", which(r$n_draws == 0L)[1]))
  lpd <- aperm(array(r$lpd, c(2, N, K)), 3:1)                                              # [K, N, 2]
  at <- cbind(fold, seq_len(N))
  elpd <- lpd[, , 1][at]
  mcse <- sqrt(pmax(expm1(lpd[, , 2][at] - 2 * elpd), 0) / r$n_draws[fold])
  list(pointwise = cbind(elpd = elpd, mcse = mcse), elpd_kfold = sum(elpd), se = sqrt(N) * sd(elpd), fold = fold, n_draws = r$n_draws)
}

# ---- the posterior mode (PotusModel.optimize is the same in Python; DESIGN.md section 4k) ----
# cmdstanr's model$optimize(data, jacobian = FALSE, algorithm = "lbfgs"): batched L-BFGS on the device, `paths` starts in one launch.
# init: the radius of the uniform starts, or a matrix [paths, D] of unconstrained starting points.  pars: 0-based output-row columns
# c(begin, end) whose constrained values are wanted (NULL: none).  Returns list(q [paths, D], lp, grad_norm, return_code (1 ABSF, 2 RELF,
# 3 ABSGRAD, 4 RELGRAD, 5 ABSX, 6 MAXIT, 7 LSFAIL, 8 INIT), iterations, grad_evals [paths], best, rows [paths, end - begin] or NULL).
potus_optimize <- function(data, variant = c("full", "no_mode_adjustment"), jacobian = FALSE, init = 2, paths = 1, seed = 1843, iter = 2000,
                           history_size = 5, init_alpha = 1e-3, tol_obj = 1e-12, tol_rel_obj = 1e4, tol_grad = 1e-8, tol_rel_grad = 1e7,
                           tol_param = 1e-8, path_offset = 0, pars = NULL, device = 0) {
  variant <- match.arg(variant)
  own <- is.matrix(init)
  if (own) paths <- nrow(init)
  res <- .potus_create(data, variant, c(1L, 0L, 0L, 0L, 10L, as.integer(device), 0L, 1L, 0L, 0L, 0L, 0L),
                       c(0.8, 0.05, 0.75, 10, 1, if (own) 2 else init, seed))
  .potus_check(res$status)
  on.exit(.C("potus_R_destroy", res$handle, status = integer(1)))
  info <- .C("potus_R_num_columns", res$handle, D = integer(1), n_cols = integer(1), status = integer(1))
  .potus_check(info$status)
  D <- info$D
  cols <- if (is.null(pars)) c(0L, 1L) else as.integer(pars)
  nsel <- cols[2] - cols[1]
  r <- .C("potus_R_optimize", res$handle, as.integer(c(isTRUE(jacobian), history_size, iter, path_offset, paths, own, !is.null(pars))),
          as.double(c(init_alpha, tol_obj, tol_rel_obj, tol_grad, tol_rel_grad, tol_param)), if (own) as.double(t(init)) else double(1),
          q = double(paths * D), lp = double(paths), grad_norm = double(paths), info = integer(3 * paths), cols,
          rows = double(max(paths * nsel, 1)), status = integer(1))
  .potus_check(r$status)
  info3 <- matrix(r$info, paths, 3, byrow = TRUE)
  ok <- info3[, 1] >= 1 & info3[, 1] <= 5
  pool <- if (any(ok)) ok else is.finite(r$lp)
  list(q = matrix(r$q, paths, D, byrow = TRUE), lp = r$lp, grad_norm = r$grad_norm, return_code = info3[, 1], iterations = info3[, 2],
       grad_evals = info3[, 3], best = which(pool)[which.max(r$lp[pool])],
       rows = if (is.null(pars)) NULL else matrix(r$rows[seq_len(paths * nsel)], paths, nsel, byrow = TRUE))
}

# ---- the Laplace approximation (Handle.laplace is the same in Python; DESIGN.md section 4n) ----
# cmdstanr's model$laplace(data, mode =, draws =, jacobian = TRUE): minus the Hessian of log_prob<jacobian> at `mode` (a vector of D unconstrained
# coordinates, or a matrix [modes, D]; e.g. potus_optimize(..., jacobian = TRUE)$q) by central differences on the device, its Cholesky factor, and
# `draws` draws mode + L^-T u.  u: NULL for the library's normals (Philox, purpose 8) or an array [D, draws, modes] (column-major: u[, n, m] is draw n).
# Returns list(q [modes * draws, D], lp, lp_approx, log_ratio = lp - lp_approx up to lp(mode), return_code (0 ok, 1 NOT_PD, 2 mode not finite),
# log_det, grad_norm, min_pivot [modes], precision [D, D, modes] or NULL).
potus_laplace <- function(data, mode, variant = c("full", "no_mode_adjustment"), draws = 1000, jacobian = TRUE, seed = 1843, h = 1e-4, u = NULL,
                          draw_offset = 0, precision = FALSE, device = 0) {
  variant <- match.arg(variant)
  if (!is.matrix(mode)) mode <- matrix(mode, 1)
  modes <- nrow(mode)
  res <- .potus_create(data, variant, c(1L, 0L, 0L, 0L, 10L, as.integer(device), 0L, 1L, 0L, 0L, 0L, 0L), c(0.8, 0.05, 0.75, 10, 1, 2, seed))
  .potus_check(res$status)
  on.exit(.C("potus_R_destroy", res$handle, status = integer(1)))
  D <- ncol(mode)
  n <- modes * draws
  r <- .C("potus_R_laplace", res$handle, as.integer(c(isTRUE(jacobian), draw_offset, modes, draws, !is.null(u), isTRUE(precision))), as.double(h),
          as.double(t(mode)), if (is.null(u)) double(1) else as.double(u), q = double(max(n * D, 1)), lp = double(max(n, 1)), lp_approx = double(max(n, 1)),
          info = double(4 * modes), precision = double(if (isTRUE(precision)) modes * D * D else 1), status = integer(1))
  .potus_check(r$status)
  info4 <- matrix(r$info, modes, 4, byrow = TRUE)
  list(q = matrix(r$q[seq_len(n * D)], n, D, byrow = TRUE), lp = r$lp[seq_len(n)], lp_approx = r$lp_approx[seq_len(n)],
       log_ratio = r$lp[seq_len(n)] - r$lp_approx[seq_len(n)], return_code = info4[, 1], log_det = info4[, 2], grad_norm = info4[, 3],
       min_pivot = info4[, 4], precision = if (isTRUE(precision)) array(r$precision, c(D, D, modes)) else NULL)
}

# ---- Pathfinder (DESIGN.md section 4o): cmdstanr's model$pathfinder(data, num_paths = 4, draws = 1000, psis_resample = FALSE) ----
# `paths` L-BFGS paths from init (a radius, or a matrix [paths, D] of unconstrained starts), a normal approximation around every iterate, the
# ELBO of each from num_elbo_draws draws, and ceiling(draws / paths) draws per path from the path's best iterate.  Returns q [paths * draws per
# path, D] (path-major), lp, lq, log_ratio = lp - lq, and per path return_code (0 ok, 1 NO_ELBO: NaN draws), iterations, best_iteration,
# optimize_code, elbo [paths, max_lbfgs_iters + 1] indexed by the iterate (column l + 1 is iterate l) and kept, the pairs the history may use.
potus_pathfinder <- function(data, variant = c("full", "no_mode_adjustment"), paths = 4, draws = 1000, init = 2, seed = 1843, history_size = 6,
                             num_elbo_draws = 25, max_lbfgs_iters = 1000, lbfgs_history_size = 5, init_alpha = 1e-3, tol_obj = 1e-12, tol_rel_obj = 1e4,
                             tol_grad = 1e-8, tol_rel_grad = 1e7, tol_param = 1e-8, draw_offset = 0, path_offset = 0, device = 0) {
  variant <- match.arg(variant)
  q0 <- if (is.matrix(init)) init else NULL
  if (!is.null(q0)) paths <- nrow(q0)
  radius <- if (is.null(q0)) init else 2
  res <- .potus_create(data, variant, c(1L, 0L, 0L, 0L, 10L, as.integer(device), 0L, 1L, 0L, 0L, 0L, 0L), c(0.8, 0.05, 0.75, 10, 1, radius, seed))
  .potus_check(res$status)
  on.exit(.C("potus_R_destroy", res$handle, status = integer(1)))
  D <- .C("potus_R_num_columns", res$handle, D = integer(1), n_cols = integer(1), status = integer(1))$D
  m <- as.integer(ceiling(draws / paths)); n <- paths * m; rows <- as.integer(max_lbfgs_iters) + 1L
  r <- .C("potus_R_pathfinder", res$handle,
          as.integer(c(history_size, num_elbo_draws, m, draw_offset, path_offset, max_lbfgs_iters, lbfgs_history_size, paths, !is.null(q0))),
          as.double(c(init_alpha, tol_obj, tol_rel_obj, tol_grad, tol_rel_grad, tol_param)), if (is.null(q0)) double(1) else as.double(t(q0)),
          info = integer(4 * paths), elbo = double(paths * rows), kept = integer(paths * rows), q = double(max(n * D, 1)), lp = double(max(n, 1)),
          lq = double(max(n, 1)), status = integer(1))
  .potus_check(r$status)
  info4 <- matrix(r$info, paths, 4, byrow = TRUE)
  list(q = matrix(r$q[seq_len(n * D)], n, D, byrow = TRUE), lp = r$lp[seq_len(n)], lq = r$lq[seq_len(n)], log_ratio = r$lp[seq_len(n)] - r$lq[seq_len(n)],
       return_code = info4[, 1], iterations = info4[, 2], best_iteration = info4[, 3], optimize_code = info4[, 4],
       elbo = matrix(r$elbo, paths, rows, byrow = TRUE), kept = matrix(r$kept, paths, rows, byrow = TRUE))
}

# ---- mean-field ADVI (DESIGN.md section 4p): cmdstanr's model$variational(data, algorithm = "meanfield", ...) with its argument names ----
# `runs` independent runs in one call (cmdstanr runs one) from init (a radius, or a matrix [runs, D] of unconstrained starts), output_samples
# draws per run.  Returns mean, sd = exp(omega) [runs, D], q [runs * output_samples, D] (run-major), lp, lq, log_ratio = lp - lq, and per run
# return_code (1 MEAN_CONVERGED, 2 MEDIAN_CONVERGED, 3 MAXIT, 4 NONFINITE, 5 INIT, 6 ADAPT_FAILED; 5 and 6: NaN draws), flags (1: may be
# diverging), iterations, eta, elbo [runs, iter %/% eval_elbo + 1] (column 1 the initial ELBO, NaN behind the end), adapt_elbo [runs, 5].
potus_variational <- function(data, variant = c("full", "no_mode_adjustment"), runs = 1, init = 2, seed = 1843, algorithm = "meanfield", iter = 10000,
                              grad_samples = 1, elbo_samples = 100, eta = 1, adapt_engaged = TRUE, adapt_iter = 50, tol_rel_obj = 0.01, eval_elbo = 100,
                              output_samples = 1000, elbo_offset = 0, draw_offset = 0, run_offset = 0, device = 0) {
  variant <- match.arg(variant)
  if (!identical(algorithm, "meanfield")) stop("potus_variational: algorithm = \"", algorithm, "\" is not built (meanfield only)")
  q0 <- if (is.matrix(init)) init else NULL
  if (!is.null(q0)) runs <- nrow(q0)
  radius <- if (is.null(q0)) init else 2
  res <- .potus_create(data, variant, c(1L, 0L, 0L, 0L, 10L, as.integer(device), 0L, 1L, 0L, 0L, 0L, 0L), c(0.8, 0.05, 0.75, 10, 1, radius, seed))
  .potus_check(res$status)
  on.exit(.C("potus_R_destroy", res$handle, status = integer(1)))
  D <- .C("potus_R_num_columns", res$handle, D = integer(1), n_cols = integer(1), status = integer(1))$D
  m <- as.integer(output_samples); n <- runs * m; trace <- as.integer(iter) %/% as.integer(eval_elbo) + 1L
  r <- .C("potus_R_variational", res$handle,
          as.integer(c(iter, grad_samples, elbo_samples, eval_elbo, isTRUE(adapt_engaged), adapt_iter, m, draw_offset, run_offset, runs, !is.null(q0))),
          as.double(c(eta, tol_rel_obj, elbo_offset)), if (is.null(q0)) double(1) else as.double(t(q0)),
          info = integer(6 * runs), mu = double(runs * D), omega = double(runs * D), elbo = double(runs * trace), adapt_elbo = double(runs * 5),
          q = double(max(n * D, 1)), lp = double(max(n, 1)), lq = double(max(n, 1)), status = integer(1))
  .potus_check(r$status)
  info6 <- matrix(r$info, runs, 6, byrow = TRUE)
  etas <- c(100, 10, 1, 0.1, 0.01)
  list(mean = matrix(r$mu, runs, D, byrow = TRUE), sd = exp(matrix(r$omega, runs, D, byrow = TRUE)),
       q = matrix(r$q[seq_len(n * D)], n, D, byrow = TRUE), lp = r$lp[seq_len(n)], lq = r$lq[seq_len(n)], log_ratio = r$lp[seq_len(n)] - r$lq[seq_len(n)],
       return_code = info6[, 1], flags = info6[, 2], iterations = info6[, 3],
       eta = ifelse(info6[, 4] >= 0, etas[pmax(info6[, 4], 0) + 1], if (isTRUE(adapt_engaged)) NA_real_ else eta),
       elbo = matrix(r$elbo, runs, trace, byrow = TRUE), adapt_elbo = matrix(r$adapt_elbo, runs, 5, byrow = TRUE))
}

# ---- joint election outcomes (us_potus_model_amd/outcomes.py is the same in Python; DESIGN.md section 4f) ----
# What the run scripts compute from the JOINT outcome of a draw, counted on the device over the post-warm-up draws of every chain of the fit:
# the distribution of Democratic electoral votes (final_2016.R:904-920), the tipping-point state (final_2012.R:809-843), how often states i and j
# are won together, and -- with `actual`, the certified two-party share per state -- how many draws fall below it (README.Rmd:481-502).
# ev: integer electoral votes in state order; days: c(first, last) 1-based, NULL = every day.  Returns counts (exact doubles):
# ev_hist [days, sum(ev) + 1], tipping [days, S + 1] (last column: no tipping point), joint [days, S + 2, S + 2] over the indicators
# (state won ..., electoral-college win, popular-vote win), below_actual [days, S], n_draws, and p_value = (2 below + 1) / (2 n + 2).
potus_outcomes <- function(fit, ev, actual = NULL, days = NULL, ev_to_win = 270L) {
  S <- as.integer(fit$data$S); nT <- as.integer(fit$data$T)
  if (any(ev != round(ev))) stop("potus_outcomes: electoral votes must be integers")
  if (is.null(days)) days <- c(1L, nT)
  n <- as.integer(days[2] - days[1] + 1L); K <- as.integer(sum(ev))
  r <- .C("potus_R_outcomes", as.integer(fit$handles), length(fit$handles), as.integer(c(days[1] - 1L, days[2], ev_to_win, !is.null(actual))),
          as.integer(ev), as.double(if (is.null(actual)) rep(0, S) else actual), ev_hist = double(max(n, 1L) * (K + 1L)),
          tipping = double(max(n, 1L) * (S + 1L)), joint = double(max(n, 1L) * (S + 2L)^2), below = double(max(n, 1L) * S), n_draws = double(1),
          status = integer(1))
  .potus_check(r$status)
  out <- list(ev_hist = matrix(r$ev_hist, n, K + 1L, byrow = TRUE), tipping = matrix(r$tipping, n, S + 1L, byrow = TRUE),
              joint = aperm(array(r$joint, c(S + 2L, S + 2L, n)), c(3, 2, 1)), n_draws = r$n_draws, days = days, ev = ev, ev_to_win = ev_to_win)
  if (!is.null(actual)) {
    out$below_actual <- matrix(r$below, n, S, byrow = TRUE)
    out$p_value <- (2 * out$below_actual + 1) / (2 * r$n_draws + 2)
  }
  out
}

# The tipping-point table of final_2012.R:836-843 on `day` of the range (default: its last day): state, prop, sorted by prop; states that
# never tip are left out.
potus_tipping_point <- function(outcomes, states = NULL, day = nrow(outcomes$tipping)) {
  S <- ncol(outcomes$tipping) - 1L
  cnt <- outcomes$tipping[day, seq_len(S)]
  if (is.null(states)) states <- seq_len(S)
  d <- data.frame(state = states, prop = cnt / sum(cnt))
  d <- d[cnt > 0, , drop = FALSE]
  d[order(-d$prop), , drop = FALSE]
}

# ---- conditional forecasts and the covariance of the state scores (us_potus_model_amd/scenario.py is the same in Python; DESIGN.md section 4h) ----
# cor() of the election-day scores of the draws (final_2016.R:710-715) without the draws on the host, and the forecast GIVEN an event:
# given = list(FL = "win", PA = "lose", national = c(0.48, 0.52)) -- names are state names (`states`, in state order), 1-based state indices
# as strings ("3") or "national"; an interval is lo < x <= hi, "win" is (0.5, Inf], "lose" is (-Inf, 0.5].  day: the day the condition is
# read on (1-based, default election day); days: c(first, last) of the outputs, 1-based, NULL = every day; ev: integer electoral votes or
# NULL for the moments alone.  Returns n_kept, n_draws, probability, mean [days, S + 1], cov [days, S + 1, S + 1] (coordinate S + 1: the
# national vote) and, with ev, potus_outcomes' ev_hist, tipping and joint of the kept draws (n_draws of that list = n_kept).
potus_scenario <- function(fit, given = NULL, ev = NULL, day = NULL, days = NULL, ev_to_win = 270L, states = NULL) {
  S <- as.integer(fit$data$S); nT <- as.integer(fit$data$T)
  if (!is.null(ev) && any(ev != round(ev))) stop("potus_scenario: electoral votes must be integers")
  if (is.null(days)) days <- c(1L, nT)
  if (is.null(day)) day <- nT
  lo <- rep(-Inf, S + 1L); hi <- rep(Inf, S + 1L)
  for (nm in names(given)) {
    k <- if (nm == "national") S + 1L else if (!is.null(states) && nm %in% states) match(nm, states) else suppressWarnings(as.integer(nm))
    if (is.na(k) || k < 1L || k > S + 1L) stop("potus_scenario: '", nm, "' is no state name, state index or \"national\"")
    g <- given[[nm]]
    if (identical(g, "win")) lo[k] <- 0.5
    else if (identical(g, "lose")) hi[k] <- 0.5
    else if (is.numeric(g) && length(g) == 2L) { lo[k] <- g[1]; hi[k] <- g[2] }
    else stop("potus_scenario: a condition is \"win\", \"lose\" or c(lo, hi)")
  }
  n <- as.integer(days[2] - days[1] + 1L); K <- if (is.null(ev)) 0L else as.integer(sum(ev)); m <- max(n, 1L)
  r <- .C("potus_R_scenario", as.integer(fit$handles), length(fit$handles),
          as.integer(c(day - 1L, days[1] - 1L, days[2], ev_to_win, length(given) > 0L, 1L, !is.null(ev))), as.double(lo), as.double(hi),
          as.integer(if (is.null(ev)) rep(0L, S) else ev), n = double(2), mean = double(m * (S + 1L)), cov = double(m * (S + 1L)^2),
          ev_hist = double(m * (K + 1L)), tipping = double(m * (S + 1L)), joint = double(m * (S + 2L)^2), status = integer(1))
  .potus_check(r$status)
  out <- list(n_kept = r$n[1], n_draws = r$n[2], probability = r$n[1] / r$n[2], mean = matrix(r$mean, n, S + 1L, byrow = TRUE),
              cov = aperm(array(r$cov, c(S + 1L, S + 1L, n)), c(3, 2, 1)), days = days, day = day, given = given)
  if (!is.null(ev))
    out$outcomes <- list(ev_hist = matrix(r$ev_hist, n, K + 1L, byrow = TRUE), tipping = matrix(r$tipping, n, S + 1L, byrow = TRUE),
                         joint = aperm(array(r$joint, c(S + 2L, S + 2L, n)), c(3, 2, 1)), n_draws = r$n[1], days = days, ev = ev, ev_to_win = ev_to_win)
  out
}

# cov2cor of one day of a potus_scenario() result (default: its last day); NaN where a variance is zero
potus_scenario_cor <- function(scenario, day = dim(scenario$cov)[1]) {
  v <- scenario$cov[day, , ]
  s <- ifelse(diag(v) > 0, 1 / sqrt(diag(v)), NaN)
  v * outer(s, s)
}

# ---- proper scoring rules of the joint forecast against the result (us_potus_model_amd/scoring.py is the same in Python; DESIGN.md section 4u) ----
# What scoringRules gives as crps_sample, es_sample, vs_sample and dss_sample, on the device over the post-warm-up draws of every chain of the fit.
# actual: the certified two-party share per state; the national share and the Democratic electoral votes of the result are derived with the
# fit's normalised state weights and ev unless given.  use: logical [S], the states of the multivariate scores (NULL: all); days: c(first, last)
# 1-based, NULL = election day alone.  Returns crps, pit_lo, pit_hi, dss, interval, ae_median, se_mean [days, S + 2] (columns: the states, the
# national vote, the electoral votes), energy, variogram, dss_joint [days], rmse (root mean se_mean of the used states on the last day), n_draws.
potus_forecast_scores <- function(fit, actual, ev, use = NULL, vs_p = 0.5, days = NULL, actual_national = NULL, actual_ev = NULL, ev_to_win = 270L) {
  S <- as.integer(fit$data$S); nT <- as.integer(fit$data$T)
  if (length(actual) != S || length(ev) != S) stop("potus_forecast_scores: actual and ev have one entry per state")
  if (is.null(use)) use <- rep(TRUE, S)
  if (is.null(days)) days <- c(nT, nT)
  w <- fit$data$state_weights / sum(fit$data$state_weights)
  if (is.null(actual_national)) actual_national <- sum(w * actual)
  if (is.null(actual_ev)) actual_ev <- sum(ev[actual > 0.5])
  n <- as.integer(days[2] - days[1] + 1L)
  r <- .C("potus_R_forecast_scores", as.integer(fit$handles), length(fit$handles), as.integer(c(days[1] - 1L, days[2], ev_to_win)), as.double(ev),
          as.double(c(actual, actual_national, actual_ev)), as.integer(use), as.double(vs_p), uni = double(max(n, 1L) * (S + 2L) * 7L),
          multi = double(max(n, 1L) * 3L), n_draws = double(1), status = integer(1))
  .potus_check(r$status)
  uni <- aperm(array(r$uni, c(7L, S + 2L, n)), c(3, 2, 1))
  multi <- matrix(r$multi, n, 3L, byrow = TRUE)
  out <- list(n_draws = r$n_draws, days = days, use = as.logical(use), vs_p = vs_p, energy = multi[, 1], variogram = multi[, 2], dss_joint = multi[, 3])
  for (k in 1:7) out[[c("crps", "pit_lo", "pit_hi", "dss", "interval", "ae_median", "se_mean")[k]]] <- matrix(uni[, , k], n, S + 2L)
  out$rmse <- sqrt(mean(out$se_mean[n, seq_len(S)][as.logical(use)]))
  out
}
