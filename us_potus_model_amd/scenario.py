"""Conditional forecasts and the covariance of the state scores, on the GPU (potus_scenario.hpp).

    cor() / cov        final_2016.R:710-715 ("state correlation?": cor() of the election-day scores of the draws), cov(p[, election_day, ])
    scenario(given=)   the forecast GIVEN that the Democrat wins or loses some states, or that a vote share lands in an interval: the
                       probability of the condition, and mean, covariance, electoral-vote histogram, tipping point and joint win counts of
                       the draws that meet it

The S + 1 coordinates of a draw and a day are the S state scores and the national vote (the weighted mean of outcomes.py).  A condition is a
half-open interval lo < x <= hi per coordinate on ONE day: "win" is (0.5, inf], "lose" is (-inf, 0.5] -- the strict rule of
final_2016.R:817, so the two partition the draws.  predicted_score never visits the host; warm-up rows of save_warmup = 1 are left out.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .outcomes import Outcomes, _I32P, _integer_ev, _llp, _national_weights
from .sampler import _check, _device_block, _dp, _handle_ids, load_library


def parse_given(given, S, states=None):
    """`given`: {state name | state index | "national": "win" | "lose" | (lo, hi)} -> (lo [S + 1], hi [S + 1]), or (None, None) when nothing is
    given.  A bound of None leaves that side free.  Checked here as the library checks it: no NaN, lo < hi."""
    if not given:
        return None, None
    lo, hi = np.full(S + 1, -np.inf), np.full(S + 1, np.inf)
    seen = set()
    for key, what in dict(given).items():
        if isinstance(key, str):
            if key == "national":
                k = S
            elif states is not None and key in list(states):
                k = list(states).index(key)
            else:
                raise KeyError(f"scenario: {key!r} is neither \"national\" nor one of the state names" + ("" if states is not None else " (no names were given)"))
        elif isinstance(key, (int, np.integer)) and not isinstance(key, bool):
            k = int(key)
            if not 0 <= k < S:
                raise KeyError(f"scenario: state index {k} outside 0 .. {S - 1}")
        else:
            raise KeyError(f"scenario: {key!r} is no state name, state index or \"national\"")
        if k in seen:
            raise ValueError(f"scenario: coordinate {k} is conditioned on twice")
        seen.add(k)
        if isinstance(what, str):
            if what == "win":
                lo[k] = 0.5
            elif what == "lose":
                hi[k] = 0.5
            else:
                raise ValueError(f"scenario: {what!r} is neither \"win\" nor \"lose\" nor an interval (lo, hi)")
        else:
            try:
                a, b = what
            except (TypeError, ValueError):
                raise ValueError(f"scenario: {what!r} is neither \"win\" nor \"lose\" nor an interval (lo, hi)") from None
            lo[k] = -np.inf if a is None else float(a)
            hi[k] = np.inf if b is None else float(b)
        if np.isnan(lo[k]) or np.isnan(hi[k]):
            raise ValueError(f"scenario: a bound of {key!r} is NaN")
        if not lo[k] < hi[k]:
            raise ValueError(f"scenario: the interval ({lo[k]}, {hi[k]}] of {key!r} is empty")
    return lo, hi


def cov2cor(cov):
    """R's cov2cor on the last two axes; NaN in the rows and columns of a zero (or NaN) variance."""
    cov = np.asarray(cov, dtype=np.float64)
    v = np.diagonal(cov, axis1=-2, axis2=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(v > 0, 1.0 / np.sqrt(v), np.nan)
        r = cov * s[..., :, None] * s[..., None, :]
    i = np.arange(cov.shape[-1])
    r[..., i, i] = np.where(v > 0, 1.0, np.nan)                          # (as cov2cor sets it)
    return r


class Scenario:
    """Per day of the range `days` = (begin, end), 0-based, over the draws that meet the condition: mean [days, S + 1], cov [days, S + 1, S + 1]
    (coordinate S: the national vote) and -- when electoral votes were given -- `outcomes`, an Outcomes of the conditional counts whose n_draws
    is n_kept (so ev_distribution, ev_summary, tipping_point, conditional and win_probability are conditional on the event).  n_kept of the
    n_draws draws met the condition: probability = n_kept / n_draws."""

    def __init__(self, n_kept, n_draws, mean, cov, outcomes=None, days=None, cond_day=None, given=None, states=None):
        self.n_kept, self.n_draws = int(n_kept), int(n_draws)
        self.mean = np.asarray(mean, dtype=np.float64)
        self.cov = np.asarray(cov, dtype=np.float64)
        self.outcomes = outcomes
        self.S = self.mean.shape[1] - 1
        self.days = (0, self.mean.shape[0]) if days is None else (int(days[0]), int(days[1]))
        self.cond_day = cond_day
        self.given = given
        self.states = None if states is None else list(states)

    @property
    def probability(self):
        """P(condition) = n_kept / n_draws."""
        return self.n_kept / self.n_draws if self.n_draws else float("nan")

    def sd(self, day=-1):
        """Standard deviation of the S + 1 coordinates on `day` of the range."""
        return np.sqrt(np.diagonal(self.cov[day]))

    def cor(self, day=-1):
        """Correlation matrix [S + 1, S + 1] on `day` of the range (cov2cor; NaN where a variance is zero)."""
        return cov2cor(self.cov[day])

    def index(self, which):
        """Coordinate of a state index / name or "national"."""
        if which == "national":
            return self.S
        if isinstance(which, str):
            if self.states is None:
                raise KeyError(f"no state names were given: {which!r}")
            return self.states.index(which)
        return int(which)


def _counts(n, S, e):
    if e is None:
        return None, None, None
    return np.zeros((n, int(e.sum()) + 1), np.int64), np.zeros((n, S + 1), np.int64), np.zeros((n, S + 2, S + 2), np.int64)


def _llp_or_none(a):
    return None if a is None else _llp(a)


def scenario(handles, ev=None, given=None, day=-1, days=None, ev_to_win=270, states=None):
    """potus_scenario over the pooled post-warm-up draws of the listed handles (one posterior, one GPU or several), taken chain after chain.
    ev: integer electoral votes per state, or None for the moments alone; given: see parse_given; day: the condition day, 0-based, -1 =
    election day; days: (begin, end) of the outputs, 0-based, None = all days."""
    hs, ids = _handle_ids(handles)
    h0 = hs[0]
    S, T = int(h0.data["S"]), int(h0.data["T"])
    e = None if ev is None else _integer_ev(ev, S)
    if int(ev_to_win) < 1:
        raise ValueError("scenario: ev_to_win must be at least 1")
    d0, d1 = (0, T) if days is None else (int(days[0]), int(days[1]))
    if not (0 <= d0 < d1 <= T):
        raise ValueError(f"scenario: days [{d0}, {d1}) of {T}")
    cd = T + int(day) if int(day) < 0 else int(day)
    if not 0 <= cd < T:
        raise ValueError(f"scenario: condition day {day} of {T}")
    lo, hi = parse_given(given, S, states)
    n = d1 - d0
    mean, cov = np.zeros((n, S + 1)), np.zeros((n, S + 1, S + 1))
    hist, tip, joint = _counts(n, S, e)
    nk, nd = C.c_longlong(0), C.c_longlong(0)
    _check(h0.L, h0.L.potus_scenario(ids, len(hs), cd, None if lo is None else _dp(lo), None if hi is None else _dp(hi), d0, d1,
                                     None if e is None else e.ctypes.data_as(_I32P), int(ev_to_win), C.byref(nk), C.byref(nd), _dp(mean), _dp(cov),
                                     _llp_or_none(hist), _llp_or_none(tip), _llp_or_none(joint)))
    o = None if e is None else Outcomes(hist, tip, joint, None, nk.value, e, ev_to_win, (d0, d1), None, states)
    return Scenario(nk.value, nd.value, mean, cov, o, (d0, d1), cd, given, states)


def scenario_of_block(block, w, ev=None, given=None, day=-1, ev_to_win=270, states=None):
    """potus_scenario_device on a torch tensor [draws, days, S] (float64, contiguous, on a GPU) of predicted scores, its draws in the order
    they are to be summed in.  w: the weights of the national vote (normalised here, in index order); day indexes the block's days."""
    _device_block(block, "scenario_of_block", ("draws", "days", "S"))
    L = load_library()
    nd_, n, S = (int(x) for x in block.shape)
    e = None if ev is None else _integer_ev(ev, S)
    w = _national_weights(w, S)
    cd = n + int(day) if int(day) < 0 else int(day)
    if not 0 <= cd < n:
        raise ValueError(f"scenario_of_block: condition day {day} of {n}")
    lo, hi = parse_given(given, S, states)
    mean, cov = np.zeros((n, S + 1)), np.zeros((n, S + 1, S + 1))
    hist, tip, joint = _counts(n, S, e)
    nk = C.c_longlong(0)
    _check(L, L.potus_scenario_device(int(block.device.index or 0), C.c_void_p(block.data_ptr()), nd_, n, S, _dp(w), cd,
                                      None if lo is None else _dp(lo), None if hi is None else _dp(hi), None if e is None else e.ctypes.data_as(_I32P),
                                      int(ev_to_win), C.byref(nk), _dp(mean), _dp(cov), _llp_or_none(hist), _llp_or_none(tip), _llp_or_none(joint)))
    o = None if e is None else Outcomes(hist, tip, joint, None, nk.value, e, ev_to_win, (0, n), None, states)
    return Scenario(nk.value, nd_, mean, cov, o, (0, n), cd, given, states)


def last_timing():
    """(produce + gather, day cut, keep + compact, moments, counting kernel) in ms of this thread's last scenario call (potus_scenario_timing)."""
    L = load_library()
    ms = np.zeros(5)
    _check(L, L.potus_scenario_timing(_dp(ms)))
    return tuple(float(x) for x in ms)
