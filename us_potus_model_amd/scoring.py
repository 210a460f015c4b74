"""Proper scoring rules of the joint forecast against the certified result, on the GPU (potus_fscore.hpp): what
scoringRules gives an R user as crps_sample, es_sample, vs_sample and dss_sample.

    score(handles, ev, actual)        the pooled post-warm-up draws of one posterior, pooled as scenario() pools them
    score_of_block(block, w, ev, actual)   a torch tensor [draws, days, S] of predicted scores on the GPU
    score_datasets(handle, ev, actual)     every data set of one handle (run dates, prior settings) in one launch

Per day and COLUMN -- the S states, the national vote, the Democratic electoral votes of a draw -- crps, pit, dss, interval (95 %), ae_median
and se_mean; per day over the USED states the energy score, the variogram score of order vs_p and the joint Dawid-Sebastiani score.  All of
them are negatively oriented: smaller is better.  The definitions are in include/potus_hmc.h.  predicted_score never visits the host.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .outcomes import _national_weights
from .sampler import _check, _device_block, _dp, _handle_ids, _ip, load_library

MAX_S = 63
MAX_DRAWS = 16384
UNI = ("crps", "pit_lo", "pit_hi", "dss", "interval", "ae_median", "se_mean")
MULTI = ("energy", "variogram", "dss_joint")
SCORES = ("crps", "dss", "interval", "ae_median", "se_mean") + MULTI        # what against() differences


def check_args(S, ev, actual, use=None, vs_p=0.5, actual_national=None, actual_ev=None, w=None):
    """The arguments as the library takes them: (ev [S] float64, actual [S + 2], use [S] int32, vs_p).  Refuses what the library refuses, with
    the same words; the national share and the electoral votes of the result are derived as sum(w y) and sum(ev 1[y > 0.5]) when not given."""
    S = int(S)
    if not 1 <= S <= MAX_S:
        raise ValueError(f"score: S = {S} (1 .. {MAX_S})")
    e = np.ascontiguousarray(ev, dtype=np.float64)
    if e.shape != (S,):
        raise ValueError(f"score: ev has shape {e.shape}, ({S},) expected")
    if not np.isfinite(e).all():
        raise ValueError("score: ev is not finite")
    y = np.asarray(actual, dtype=np.float64)
    if y.shape == (S,):
        if (actual_national is None or actual_ev is None) and not np.isfinite(y).all():
            raise ValueError("score: actual is not finite")
        if actual_national is None:
            if w is None:
                raise ValueError("score: actual_national is not given and there are no weights to derive it with")
            nat = 0.0
            for s in range(S):
                nat = nat + float(w[s]) * float(y[s])
            actual_national = nat
        if actual_ev is None:
            actual_ev = float(e[y > 0.5].sum())
        y = np.concatenate([y, [float(actual_national), float(actual_ev)]])
    elif y.shape != (S + 2,):
        raise ValueError(f"score: actual has shape {y.shape}, ({S},) or ({S + 2},) expected")
    elif actual_national is not None or actual_ev is not None:
        raise ValueError(f"score: actual has all {S + 2} entries, and actual_national / actual_ev are given too")
    y = np.ascontiguousarray(y)
    if not np.isfinite(y).all():
        raise ValueError("score: actual is not finite")
    if not ((y[:S + 1] >= 0) & (y[:S + 1] <= 1)).all():
        raise ValueError("score: a share of actual lies outside [0, 1]")
    u = np.ones(S, np.int32) if use is None else np.ascontiguousarray(np.asarray(use) != 0, dtype=np.int32)
    if u.shape != (S,):
        raise ValueError(f"score: use has shape {u.shape}, ({S},) expected")
    if not u.any():
        raise ValueError("score: use selects no state")
    p = float(vs_p)
    if not 0.0 < p <= 2.0:
        raise ValueError(f"score: vs_p = {vs_p} outside (0, 2]")
    return e, y, u, p


class ForecastScores:
    """uni [..., days, S + 2, 7] and multi [..., days, 3] as the library writes them (leading axes: the data sets of a timeline or grid).
    Attributes crps, dss, interval, ae_median, se_mean [..., days, S + 2]; pit [..., days, S + 2, 2] = (#{x < y}, #{x <= y}) / n; energy,
    variogram, dss_joint [..., days].  Column S is the national vote, column S + 1 the electoral votes."""

    def __init__(self, uni, multi, n_draws, use, actual, days=None, vs_p=0.5, states=None):
        self.uni, self.multi = np.asarray(uni, dtype=np.float64), np.asarray(multi, dtype=np.float64)
        if self.uni.shape[-1] != len(UNI) or self.multi.shape[-1] != len(MULTI) or self.uni.shape[:-2] != self.multi.shape[:-1]:
            raise ValueError(f"ForecastScores: uni {self.uni.shape} and multi {self.multi.shape} do not belong together")
        self.S = self.uni.shape[-2] - 2
        self.n_draws = n_draws
        self.use = np.asarray(use) != 0
        if self.use.shape != (self.S,):
            raise ValueError(f"ForecastScores: use has shape {self.use.shape}, ({self.S},) expected")
        self.actual = np.asarray(actual, dtype=np.float64)
        n = self.uni.shape[-3]
        self.days = (0, n) if days is None else (int(days[0]), int(days[1]))
        self.vs_p = float(vs_p)
        self.states = None if states is None else list(states)

    crps = property(lambda self: self.uni[..., 0])
    pit = property(lambda self: self.uni[..., 1:3])
    dss = property(lambda self: self.uni[..., 3])
    interval = property(lambda self: self.uni[..., 4])
    ae_median = property(lambda self: self.uni[..., 5])
    se_mean = property(lambda self: self.uni[..., 6])
    energy = property(lambda self: self.multi[..., 0])
    variogram = property(lambda self: self.multi[..., 1])
    dss_joint = property(lambda self: self.multi[..., 2])

    def rmse(self, day=-1):
        """Root of the mean se_mean over the used states on `day` of the range: the reference's RMSE of the state means (DC left out by `use`)."""
        return np.sqrt(self.se_mean[..., day, :self.S][..., self.use].mean(axis=-1))

    def table(self, day=-1):
        """dict(columns = names, crps, pit_lo, ..., se_mean [..., S + 2], energy, variogram, dss_joint, rmse) of `day` of the range."""
        names = list(self.states) if self.states is not None else [str(s) for s in range(self.S)]
        out = dict(columns=names + ["national", "electoral_votes"])
        for k, name in enumerate(UNI):
            out[name] = self.uni[..., day, :, k]
        for k, name in enumerate(MULTI):
            out[name] = self.multi[..., day, k]
        out["rmse"] = self.rmse(day)
        return out

    def against(self, other):
        """This minus other, score by score (negative: this forecast is the better one): dict of crps, dss, interval, ae_median, se_mean
        [..., days, S + 2] and energy, variogram, dss_joint [..., days].  Both must score the same days, states and result."""
        if self.days != other.days or self.S != other.S or not np.array_equal(self.use, other.use) or self.vs_p != other.vs_p:
            raise ValueError("against: the two results do not score the same days, states or order")
        if not np.array_equal(self.actual, other.actual):
            raise ValueError("against: the two results are scored against different outcomes")
        return {k: getattr(self, k) - getattr(other, k) for k in SCORES}


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def score(handles, ev, actual, days=None, use=None, vs_p=0.5, actual_national=None, actual_ev=None, ev_to_win=270, states=None):
    """potus_forecast_scores over the pooled post-warm-up draws of the listed handles (one posterior, one GPU or several), chain after chain.
    actual: the certified share per state [S] (the national share and the electoral votes derived, or given), or all S + 2; days: (begin, end),
    0-based, None = election day alone, as for every scoring call here and in R (the energy score is all pairs of draws per day: ask for more
    days by naming them); use: the states of the multivariate scores and of rmse(), None = all."""
    hs, ids = _handle_ids(handles)
    h0 = hs[0]
    S, T = int(h0.data["S"]), int(h0.data["T"])
    e, y, u, p = check_args(S, ev, actual, use, vs_p, actual_national, actual_ev, _national_weights(h0.data["state_weights"], S))
    d0, d1 = (T - 1, T) if days is None else (int(days[0]), int(days[1]))
    if not (0 <= d0 < d1 <= T):
        raise ValueError(f"score: days [{d0}, {d1}) of {T}")
    n = d1 - d0
    uni, multi = np.zeros((n, S + 2, len(UNI))), np.zeros((n, len(MULTI)))
    nd = C.c_longlong(0)
    _check(h0.L, h0.L.potus_forecast_scores(ids, len(hs), d0, d1, _dp(e), int(ev_to_win), _dp(y), _i32(u), p, _dp(uni), _dp(multi), C.byref(nd)))
    return ForecastScores(uni, multi, nd.value, u, y, (d0, d1), p, states)


def score_of_block(block, w, ev, actual, use=None, vs_p=0.5, actual_national=None, actual_ev=None, ev_to_win=270, states=None, days=None):
    """potus_forecast_scores_device on a torch tensor [draws, days, S] (float64, contiguous, on a GPU) of predicted scores, its draws in
    canonical order.  w: the weights of the national vote (normalised here, in index order).  days: the (begin, end) of the design that the
    block's days are, kept on the result so that against() can tell whether two results score the same days; None = (0, the block's days)."""
    _device_block(block, "score_of_block", ("draws", "days", "S"))
    L = load_library()
    n_draws, n, S = (int(x) for x in block.shape)
    if days is not None and int(days[1]) - int(days[0]) != n:
        raise ValueError(f"score_of_block: days = {tuple(days)} for a block of {n} days")
    w = _national_weights(w, S)
    e, y, u, p = check_args(S, ev, actual, use, vs_p, actual_national, actual_ev, w)
    uni, multi = np.zeros((n, S + 2, len(UNI))), np.zeros((n, len(MULTI)))
    _check(L, L.potus_forecast_scores_device(int(block.device.index or 0), C.c_void_p(block.data_ptr()), n_draws, n, S, _dp(w), _dp(e), int(ev_to_win),
                                             _dp(y), _i32(u), p, _dp(uni), _dp(multi)))
    return ForecastScores(uni, multi, n_draws, u, y, (0, n) if days is None else days, p, states)


def score_datasets(handle, ev, actual, days=None, use=None, vs_p=0.5, actual_national=None, actual_ev=None, ev_to_win=270, states=None):
    """potus_forecast_scores_datasets: every data set of one handle (potus_set_datasets[_ex|_grid]) scored in one launch; the leading axis of
    every score is the data set, n_draws [data sets] (0 and NaN scores for a data set with a failed chain).  days default: election day alone."""
    h = handle
    S, T = int(h.data["S"]), int(h.data["T"])
    e, y, u, p = check_args(S, ev, actual, use, vs_p, actual_national, actual_ev, _national_weights(h.data["state_weights"], S))
    d0, d1 = (T - 1, T) if days is None else (int(days[0]), int(days[1]))
    if not (0 <= d0 < d1 <= T):
        raise ValueError(f"score: days [{d0}, {d1}) of {T}")
    n_ds, n = max(int(getattr(h, "n_datasets", 1) or 1), 1), d1 - d0
    uni, multi, cnt = np.zeros((n_ds, n, S + 2, len(UNI))), np.zeros((n_ds, n, len(MULTI))), np.zeros(n_ds, np.int32)
    _check(h.L, h.L.potus_forecast_scores_datasets(h.h, d0, d1, _dp(e), int(ev_to_win), _dp(y), _i32(u), p, _dp(uni), _dp(multi), _ip(cnt)))
    return ForecastScores(uni, multi, cnt, u, y, (d0, d1), p, states)


def last_timing():
    """(columns, energy score, variogram score, joint DSS) in ms of this thread's last scoring call (potus_forecast_scores_timing)."""
    L = load_library()
    ms = np.zeros(4)
    _check(L, L.potus_forecast_scores_timing(_dp(ms)))
    return tuple(float(x) for x in ms)
