"""Numpy / plain-Python restatement of potus_scenario -- TEST INFRASTRUCTURE ONLY.

For one draw and one day the S + 1 coordinates are x[s] = predicted_score[t, s] and x[S] = nat = sum_s w[s] x[s], summed s = 0 .. S-1 in order
(the loop of outcomes_ref.item).  A draw is kept iff lo[k] < x_cond_day[k] <= hi[k] for every k.  Over the kept draws, per day:

    counts   outcomes_ref.outcomes on the kept draws
    mean     the exactly rounded sum (math.fsum) divided by n
    cov      two-pass: products of the float64 deviations from that mean, summed in long double, / (n - 1)
"""
import math

import numpy as np

import outcomes_ref


def nat_of(items, w):
    """items [n, S] -> nat [n], by the in-order loop of outcomes_ref.item."""
    w = [float(v) for v in w]
    out = np.zeros(len(items))
    for i, row in enumerate(np.asarray(items, dtype=np.float64)):
        out[i] = outcomes_ref.item([float(v) for v in row], w, [0] * len(w), 1)[1]
    return out


def keep_mask(items, w, lo, hi):
    """items [n, S] of the condition day -> (mask [n], nat [n]); lo = hi = None keeps every draw."""
    items = np.asarray(items, dtype=np.float64)
    nat = nat_of(items, w)
    if lo is None:
        return np.ones(len(items), bool), nat
    x = np.concatenate([items, nat[:, None]], axis=1)
    return ((np.asarray(lo)[None, :] < x) & (x <= np.asarray(hi)[None, :])).all(axis=1), nat


def moments(x):
    """x [n, days, C] -> mean [days, C], cov [days, C, C]; NaN where there are too few draws."""
    n, ndays, C = x.shape
    mean, cov = np.full((ndays, C), np.nan), np.full((ndays, C, C), np.nan)
    if n == 0:
        return mean, cov
    for t in range(ndays):
        for c in range(C):
            mean[t, c] = math.fsum(x[:, t, c]) / n
        if n >= 2:
            d = (x[:, t, :] - mean[t][None, :]).astype(np.longdouble)
            cov[t] = ((d.T @ d) / np.longdouble(n - 1)).astype(np.float64)
    return mean, cov


def scenario(ps, w, cond_day, lo=None, hi=None, ev=None, ev_to_win=270, cond_items=None):
    """ps [draws, days, S] in canonical order; the condition is read on day `cond_day` of ps, or on cond_items [draws, S] when given.
    Returns dict: keep, nat_cond, n_kept, n_draws, mean, cov, nat (of the kept draws, [n_kept, days]), and -- with ev -- ev_hist, tipping, joint."""
    ps = np.asarray(ps, dtype=np.float64)
    nd, ndays, S = ps.shape
    keep, nat_cond = keep_mask(ps[:, cond_day, :] if cond_items is None else cond_items, w, lo, hi)
    kept = ps[keep]
    n = len(kept)
    out = dict(keep=keep, nat_cond=nat_cond, n_kept=n, n_draws=nd)
    e = [0] * S if ev is None else ev
    oc = outcomes_ref.outcomes(kept, w, e, ev_to_win)
    if ev is not None:
        out.update(ev_hist=oc["ev_hist"], tipping=oc["tipping"], joint=oc["joint"])
    out["nat"] = oc["nat"]
    out["mean"], out["cov"] = moments(np.concatenate([kept, oc["nat"][:, :, None]], axis=2))
    return out
