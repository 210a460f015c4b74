"""Exact cross-validation of the poll models on the GPU: K-fold (random, leave-pollster-out, leave-state-out) and, on a fitted timeline,
leave-future-out (timeline.Timeline.lfo).  DESIGN.md section 4j.

PSIS-LOO (loo.py) approximates leaving one poll out by importance sampling and says itself where that stops (Pareto k).  Here every fold IS
refitted: a fold is a data set of one handle (potus_set_datasets_ex) in which the held-out polls keep their place in the design with
n_two_share = 0, so the K refits are the chains of one launch (timeline.fit), and potus_cv_lpd evaluates every held-out poll under the
draws of the fold that did not see it -- with the real y and n, and the poll's noise coordinate integrated over the N(0,1) prior it kept.

    kf = crossval.kfold(data, "full", K=10, by="pollster", chains_per_fold=4, num_warmup=1000, num_samples=1000)
    kf.elpd_kfold, kf.se
    loo.loo_compare(kf.as_loo(), crossval.kfold(data, "no_mode_adjustment", K=10, by="pollster").as_loo())
"""
from __future__ import annotations

import numpy as np

from . import timeline
from .loo import Loo, poll_vectors
from .sampler import PotusError

BY = ("random", "pollster", "state")


def _balanced(groups, K):
    """Whole groups to folds: the groups by descending size (ties: the lower group first), each to the currently smallest fold (ties: the
    lower fold).  groups: one group number per poll."""
    sizes = np.bincount(groups)
    fold_of, load = np.zeros(sizes.size, dtype=np.int64), np.zeros(K, dtype=np.int64)
    for g in sorted(range(sizes.size), key=lambda g: (-sizes[g], g)):
        if sizes[g] == 0:
            continue
        f = int(np.argmin(load))                       # the first of the smallest
        fold_of[g] = f
        load[f] += sizes[g]
    return fold_of[groups]


def poll_groups(data, by):
    """One group number per poll (state polls, then national polls): the pollster (0-based), or the state with the national polls as a
    group of their own (number S)."""
    if by == "pollster":
        return np.concatenate([np.asarray(data["poll_state"]), np.asarray(data["poll_national"])]).astype(np.int64) - 1
    if by == "state":
        return np.concatenate([np.asarray(data["state"]).astype(np.int64) - 1, np.full(int(data["N_national_polls"]), int(data["S"]), np.int64)])
    raise ValueError(f"poll_groups: by = {by!r} (pollster or state)")


def folds(data, K, by="random", seed=0):
    """One fold number (0 .. K - 1) per poll, state polls then national polls, one numbering over both.
    random: the ranks of default_rng(seed).permutation(N) modulo K.  pollster / state: the polls of a pollster / of a state (the national
    polls form one group) stay together; see _balanced."""
    N, K = int(data["N_state_polls"]) + int(data["N_national_polls"]), int(K)
    if not 2 <= K <= N:
        raise ValueError(f"folds: K = {K} for {N} polls")
    if by == "random":
        return (np.random.default_rng(seed).permutation(N) % K).astype(np.int64)
    if by not in BY:
        raise ValueError(f"folds: by = {by!r} (one of {BY})")
    return _balanced(poll_groups(data, by), K)


def held_masks(data, fold):
    """(held_state [K, N_state_polls], held_national [K, N_national_polls]): fold d holds out the polls numbered d."""
    fold = np.asarray(fold)
    Ns = int(data["N_state_polls"])
    held = fold[None, :] == np.arange(int(fold.max()) + 1)[:, None]
    return held[:, :Ns], held[:, Ns:]


def design(data, fold):
    """The timeline design of a fold assignment: data set d keeps the polls whose fold is not d; no prior or scale of its own."""
    hs, hn = held_masks(data, fold)
    return timeline.design_of(data, ~hs, ~hn)


class Kfold:
    """Exact K-fold cross-validation of one model: pointwise elpd [N] (the held-out log predictive density of every poll under the fold that did
    not see it) and its Monte-Carlo standard error mcse [N] (delta method, draws taken as independent), fold [N], n_draws [K], and per fold
    rhat_max / ess_bulk_min of the fit as the timeline reports them."""

    def __init__(self, elpd, mcse, fold, n_draws, rhat_max=None, ess_bulk_min=None, name=None, y=None, n=None, integrate=None, wall_s=None, timing=None):
        self.elpd, self.mcse = np.asarray(elpd, dtype=np.float64), np.asarray(mcse, dtype=np.float64)
        self.fold, self.n_draws = np.asarray(fold), np.asarray(n_draws)
        self.rhat_max, self.ess_bulk_min = rhat_max, ess_bulk_min
        self.name, self.integrate, self.wall_s, self.timing = name, integrate, wall_s, timing
        self.y = None if y is None else np.asarray(y)
        self.n = None if n is None else np.asarray(n)

    @property
    def elpd_kfold(self):
        return float(self.elpd.sum())

    @property
    def se(self):
        """sqrt(N var(elpd_i)), n - 1 in the variance: loo's standard error of a sum of pointwise values."""
        N = self.elpd.size
        return float(np.sqrt(N * np.var(self.elpd, ddof=1)))

    def as_loo(self):
        """A loo.Loo that loo_compare takes unchanged: column 0 = elpd, column 2 = -2 elpd, the other columns NaN; estimates rows 0 and 2."""
        pw = np.full((self.elpd.size, 5), np.nan)
        pw[:, 0], pw[:, 2] = self.elpd, -2.0 * self.elpd
        est = np.full((3, 2), np.nan)
        est[0], est[2] = (self.elpd_kfold, self.se), (-2.0 * self.elpd_kfold, 2.0 * self.se)
        return Loo(pw, est, int(np.min(self.n_draws)) if np.size(self.n_draws) else 0, self.name, self.y, self.n, self.integrate)

    def against(self, loo, mcse_loo=None):
        """elpd_kfold_i - elpd_loo_i against a PSIS-LOO of the same polls: dict(diff [N], all = dict(n, mean, max_abs, outside), high_k = the
        same over the polls whose Pareto k is above loo.k_threshold()).  outside counts |diff| > 4 combined standard errors,
        sqrt(mcse_kfold^2 + mcse_loo^2); mcse_loo [N] is the caller's (a Loo does not carry one; None: 0)."""
        if loo.pointwise.shape[0] != self.elpd.size:
            raise ValueError("Kfold.against: the PSIS-LOO is of another number of polls")
        d = self.elpd - loo.pointwise[:, 0]
        se = np.sqrt(self.mcse ** 2 + (0.0 if mcse_loo is None else np.asarray(mcse_loo, dtype=np.float64) ** 2))
        high = loo.pareto_k > loo.k_threshold()

        def table(m):
            if not m.any():
                return dict(n=0, mean=np.nan, max_abs=np.nan, outside=0)
            return dict(n=int(m.sum()), mean=float(d[m].mean()), max_abs=float(np.abs(d[m]).max()), outside=int((np.abs(d[m]) > 4.0 * se[m]).sum()))
        return dict(diff=d, all=table(np.ones(d.size, bool)), high_k=table(high))

    def __str__(self):
        return f"elpd_kfold {self.elpd_kfold:.1f} +- {self.se:.1f} ({int(self.fold.max()) + 1} folds, {self.elpd.size} polls)"


def of_lpd(lpd, n_draws, fold, **kw):
    """The Kfold of potus_cv_lpd's output [K, N, 2] for held[d] = fold == d.  A fold with a failed chain raises PotusError naming it."""
    fold, n_draws = np.asarray(fold), np.asarray(n_draws)
    for d in range(n_draws.size):
        if n_draws[d] == 0:
            raise PotusError(f"kfold: fold {d}: a chain of its fit failed (chain_status)")
    i = np.arange(fold.size)
    o0, o1 = lpd[fold, i, 0], lpd[fold, i, 1]
    var = np.expm1(o1 - 2.0 * o0) / n_draws[fold]
    return Kfold(o0, np.sqrt(np.maximum(var, 0.0)), fold, n_draws, **kw)


def kfold(data, variant="full", K=10, by="random", chains_per_fold=4, fold_seed=0, integrate=True, diagnostics=True, **opts):
    """Fit the K folds as the data sets of one launch (timeline.fit) and evaluate every poll under the fold that held it out (potus_cv_lpd).
    opts: the sampler options of Handle (num_warmup, num_samples, seed, ...)."""
    fold = folds(data, K, by, fold_seed)
    tl = timeline.fit(design(data, fold), variant, chains_per_date=chains_per_fold, **opts)
    try:
        hs, hn = held_masks(data, fold)
        lpd, cnt = tl.handle.cv_lpd(hs, hn, integrate)
        timing = tl.handle.cv_timing()
        rh, es = tl.diagnostics(n_draws=cnt) if diagnostics else (None, None)
    finally:
        tl.close()
    y, n = poll_vectors(data)
    return of_lpd(lpd, cnt, fold, rhat_max=rh, ess_bulk_min=es, name=variant, y=y, n=n, integrate=bool(integrate), wall_s=tl.wall_s, timing=timing)
