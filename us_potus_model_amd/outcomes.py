"""Joint election outcomes of the draws, counted on the GPU (potus_outcomes.hpp): what the reference's run scripts
compute from the JOINT outcome of a draw and no marginal table can give.

    ev_distribution     final_2016.R:904-920, README.Rmd "Final electoral college histogram"
    tipping_point       final_2012.R:809-843, final_2008.R:813-843
    p_values            README.Rmd:481-502 (2008; 2012 and 2016 likewise): (2 #(draw < actual) + 1) / (2 n + 2)
    conditional, popular_vote_split, joint counts: P(state i and state j), P(win | state j), P(popular-vote win and electoral-college loss)

Everything the device returns is a COUNT (int64) per day; the derivations below are host arithmetic on those counts.  predicted_score never
visits the host.  Warm-up rows of save_warmup = 1 are left out (posterior_summary pools them in: the two agree for save_warmup = 0).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .sampler import _check, _device_block, _dp, _handle_ids, load_library

EV_CAP = 2047          # the kernel's histogram: sum(ev) at most this
_LLP = C.POINTER(C.c_longlong)
_I32P = C.POINTER(C.c_int32)


def _llp(a):
    return a.ctypes.data_as(_LLP)


def _integer_ev(ev, S):
    e = np.asarray(ev)
    if e.shape != (S,):
        raise ValueError(f"ev has shape {e.shape}, ({S},) expected")
    r = np.rint(np.asarray(e, dtype=np.float64))
    if not np.array_equal(r, np.asarray(e, dtype=np.float64)):
        raise ValueError("outcomes: electoral votes must be integers (the counts are exact only then)")
    if (r < 0).any():
        raise ValueError("outcomes: electoral votes must not be negative")
    if r.sum() > EV_CAP:
        raise ValueError(f"outcomes: the electoral votes sum to {int(r.sum())}, at most {EV_CAP} supported")
    return np.ascontiguousarray(r, dtype=np.int32)


def _actual(actual, S):
    if actual is None:
        return None
    a = np.ascontiguousarray(actual, dtype=np.float64)
    if a.shape != (S,):
        raise ValueError(f"actual has shape {a.shape}, ({S},) expected")
    if not ((a >= 0) & (a <= 1)).all():
        raise ValueError("outcomes: actual must lie in [0, 1]")
    return a


def _national_weights(w, S):
    """The weights of the national vote, normalised to sum to one: summed in index order as Python floats, so that every caller divides by
    the same bits."""
    w = np.asarray(w, dtype=np.float64)
    if w.shape != (S,):
        raise ValueError(f"w has shape {w.shape}, ({S},) expected")
    sw = 0.0
    for x in w:
        sw += float(x)
    return np.ascontiguousarray(w / sw)


class Outcomes:
    """Counts per day of the range `days` = (begin, end), 0-based: ev_hist [days, sum(ev) + 1], tipping [days, S + 1] (last slot: no tipping
    point, sum(ev) < ev_to_win), joint [days, S + 2, S + 2] over the indicators (state s won, ..., electoral-college win, popular-vote win),
    below_actual [days, S] or None, n_draws.  `day` arguments index the range (-1: its last day, election day for the whole range)."""

    def __init__(self, ev_hist, tipping, joint, below_actual, n_draws, ev, ev_to_win=270, days=None, actual=None, states=None):
        self.ev_hist = np.asarray(ev_hist, dtype=np.int64)
        self.tipping = np.asarray(tipping, dtype=np.int64)
        self.joint = np.asarray(joint, dtype=np.int64)
        self.below_actual = None if below_actual is None else np.asarray(below_actual, dtype=np.int64)
        self.n_draws = int(n_draws)
        self.ev = np.asarray(ev, dtype=np.int64)
        self.ev_to_win = int(ev_to_win)
        self.S = self.tipping.shape[1] - 1
        self.days = (0, self.tipping.shape[0]) if days is None else (int(days[0]), int(days[1]))
        self.actual = None if actual is None else np.asarray(actual, dtype=np.float64)
        self.states = None if states is None else list(states)

    # ---- electoral votes
    def ev_distribution(self, day=-1):
        """P(dem_ev == k), k = 0 .. sum(ev)."""
        return self.ev_hist[day] / self.n_draws

    def ev_summary(self, day=-1):
        """mean, median, 2.5 % and 97.5 % quantiles (R's default, type 7) and P(>= ev_to_win) of the Democratic electoral votes: the five
        numbers posterior_summary()["electoral_votes"] holds, read off the histogram."""
        h = self.ev_hist[day]
        k = np.arange(h.size)
        cum = np.cumsum(h)

        def quantile(p):
            pos = (self.n_draws - 1) * p
            lo = int(np.floor(pos))
            a = int(np.searchsorted(cum, lo + 1, side="left"))                            # order statistic lo (0-based)
            b = int(np.searchsorted(cum, min(lo + 2, self.n_draws), side="left"))
            return a + (pos - lo) * (b - a)
        return dict(mean=float((k * h).sum() / self.n_draws), median=quantile(0.5), low=quantile(0.025), high=quantile(0.975),
                    prob=float(h[self.ev_to_win:].sum() / self.n_draws))

    def win_probability(self):
        """P(dem_ev >= ev_to_win) per day of the range: the series the reference plots."""
        S = self.S
        return self.joint[:, S, S] / self.n_draws

    # ---- tipping point
    def tipping_point(self, day=-1, states=None):
        """[(state name or index, share)] sorted by share, largest first (as final_2012.R:836-843 prints it); states that never tip are left
        out, as are the draws without a tipping point (their share: tipping[day, S] / n_draws)."""
        names = states if states is not None else self.states
        cnt = self.tipping[day, :self.S]
        tot = cnt.sum()
        order = sorted(range(self.S), key=lambda s: (-cnt[s], s))
        return [((names[s] if names is not None else s), float(cnt[s] / tot)) for s in order if cnt[s] > 0]

    # ---- joint and conditional
    def index(self, which):
        """Indicator index of a state index / name, "ec" (electoral-college win) or "popular" (popular-vote win)."""
        if which == "ec":
            return self.S
        if which == "popular":
            return self.S + 1
        if isinstance(which, str):
            if self.states is None:
                raise KeyError(f"no state names were given: {which!r}")
            return self.states.index(which)
        return int(which)

    def conditional(self, given, day=-1):
        """P(I_i | I_given) for every indicator i (S states, electoral-college win, popular-vote win); NaN where the condition never happens."""
        g = self.index(given)
        den = self.joint[day, g, g]
        num = self.joint[day, :, g].astype(np.float64)
        return num / den if den > 0 else np.full(num.shape, np.nan)

    def popular_vote_split(self, day=-1):
        """(P(popular-vote win and electoral-college loss), P(popular-vote loss and electoral-college win))."""
        S, J, n = self.S, self.joint[day], self.n_draws
        both = J[S, S + 1]
        return float((J[S + 1, S + 1] - both) / n), float((J[S, S] - both) / n)

    # ---- the certified result among the draws
    def p_values(self, day=-1):
        """(2 #(draw < actual) + 1) / (2 n + 2) per state (README.Rmd:493-495; the DC filter of README.Rmd:1645 belongs to the plot)."""
        if self.below_actual is None:
            raise ValueError("p_values: outcomes() was called without `actual`")
        return (2.0 * self.below_actual[day] + 1.0) / (2.0 * self.n_draws + 2.0)

    def outside_ci(self, summary, day=-1):
        """README.Rmd:502: actual > high | actual < low against the 95 % interval of a posterior_summary() result (its `state` block is
        [T, S, 4] = low, high, mean, prob over ALL days: `day` of the range is mapped to the summary's day)."""
        if self.actual is None:
            raise ValueError("outside_ci: outcomes() was called without `actual`")
        n = self.days[1] - self.days[0]
        t = self.days[0] + (day if day >= 0 else n + day)
        st = np.asarray(summary["state"])[t]
        return (self.actual > st[:, 1]) | (self.actual < st[:, 0])


def outcomes(handles, ev, actual=None, days=None, ev_to_win=270, states=None):
    """potus_outcomes over the pooled post-warm-up draws of the listed handles (one posterior, one GPU or several).  ev: integer electoral
    votes per state; actual: certified two-party share per state, or None; days: (begin, end) 0-based, None = all days."""
    hs, ids = _handle_ids(handles)
    h0 = hs[0]
    S, T = int(h0.data["S"]), int(h0.data["T"])
    e = _integer_ev(ev, S)
    a = _actual(actual, S)
    if int(ev_to_win) < 1:
        raise ValueError("outcomes: ev_to_win must be at least 1")
    d0, d1 = (0, T) if days is None else (int(days[0]), int(days[1]))
    if not (0 <= d0 < d1 <= T):
        raise ValueError(f"outcomes: days [{d0}, {d1}) of {T}")
    n, K = d1 - d0, int(e.sum())
    hist, tip, joint = np.zeros((n, K + 1), np.int64), np.zeros((n, S + 1), np.int64), np.zeros((n, S + 2, S + 2), np.int64)
    below = None if a is None else np.zeros((n, S), np.int64)
    nd = C.c_longlong(0)
    _check(h0.L, h0.L.potus_outcomes(ids, len(hs), d0, d1, e.ctypes.data_as(_I32P), int(ev_to_win), None if a is None else _dp(a),
                                     _llp(hist), _llp(tip), _llp(joint), None if below is None else _llp(below), C.byref(nd)))
    return Outcomes(hist, tip, joint, below, nd.value, e, ev_to_win, (d0, d1), a, states)


def outcomes_of_block(block, w, ev, actual=None, ev_to_win=270, states=None):
    """potus_outcomes_device on a torch tensor [draws, days, S] (float64, contiguous, on a GPU) of predicted scores -- e.g. the all-gathered
    blocks of a multi-rank job.  w: the weights of the national vote (normalised here to sum to one, in index order)."""
    _device_block(block, "outcomes_of_block", ("draws", "days", "S"))
    L = load_library()
    nd_, n, S = (int(x) for x in block.shape)
    e = _integer_ev(ev, S)
    a = _actual(actual, S)
    w = _national_weights(w, S)
    K = int(e.sum())
    hist, tip, joint = np.zeros((n, K + 1), np.int64), np.zeros((n, S + 1), np.int64), np.zeros((n, S + 2, S + 2), np.int64)
    below = None if a is None else np.zeros((n, S), np.int64)
    nd = C.c_longlong(0)
    _check(L, L.potus_outcomes_device(int(block.device.index or 0), C.c_void_p(block.data_ptr()), nd_, n, S, _dp(w), e.ctypes.data_as(_I32P),
                                      int(ev_to_win), None if a is None else _dp(a), _llp(hist), _llp(tip), _llp(joint),
                                      None if below is None else _llp(below), C.byref(nd)))
    return Outcomes(hist, tip, joint, below, nd.value, e, ev_to_win, (0, n), a, states)


def last_timing():
    """(produce + gather ms, day-range reshape ms, counting-kernel ms) of this thread's last outcomes call (potus_outcomes_timing)."""
    L = load_library()
    ms = np.zeros(3)
    _check(L, L.potus_outcomes_timing(_dp(ms)))
    return tuple(float(x) for x in ms)
