"""Numpy / plain-Python restatement of the joint election outcomes (potus_outcomes) -- TEST INFRASTRUCTURE ONLY.

A literal transcription of the definitions, one draw and one day at a time, with an explicit stable sort:

    dem_ev  = sum_s ev[s] 1[x[s] > 0.5]                                  (final_2016.R:817,909: strict)
    nat     = sum_s w[s] x[s], s = 0, 1, ..., S-1 in that order; pop_win = nat > 0.5
    tipping point (final_2012.R:817-839): arrange(desc(x)) when pop_win, arrange(x) otherwise -- dplyr's arrange is stable, so equal x keep
            the lower state index first --, cumsum(ev), the first state with cumulative ev >= W; none (slot S) when sum ev < W
    indicators I_0..I_{S-1} = 1[x[s] > 0.5], I_S = 1[dem_ev >= W], I_{S+1} = pop_win
    below_actual[s] counts x[s] < actual[s]; p-value (README.Rmd:493-495) = (2 below + 1) / (2 n + 2)

`outcomes_vectorised` is the same over all draws at once (what a host user would write after pulling predicted_score off the device); the CPU
tests hold the two equal.
"""
import numpy as np


def normalised_weights(state_weights):
    """weighted.mean's weights: w / sum(w), the sum taken in index order (as the library does)."""
    w = [float(x) for x in np.asarray(state_weights, dtype=np.float64)]
    sw = 0.0
    for x in w:
        sw += x
    return np.array([x / sw for x in w])


def item(x, w, ev, W):
    """One (draw, day): (dem_ev, nat, pop_win, tipping-point state or S)."""
    S = len(x)
    dem = 0
    nat = 0.0
    for s in range(S):
        nat += w[s] * x[s]
        if x[s] > 0.5:
            dem += ev[s]
    pop = nat > 0.5
    order = sorted(range(S), key=lambda s: ((-x[s] if pop else x[s]), s))      # equal scores: the lower index first
    cum, tip = 0, S
    for s in order:
        cum += ev[s]
        if cum >= W:
            tip = s
            break
    return dem, nat, pop, tip


def outcomes(ps, w, ev, ev_to_win=270, actual=None):
    """ps [draws, days, S]; w [S] (normalised); ev [S] non-negative integers.  Returns dict of int64 counts: ev_hist [days, sum(ev) + 1],
    tipping [days, S + 1], joint [days, S + 2, S + 2], below_actual [days, S] (None without actual), n_draws; and nat [draws, days]."""
    ps = np.asarray(ps, dtype=np.float64)
    nd, ndays, S = ps.shape
    ev = [int(e) for e in ev]
    assert all(e >= 0 for e in ev) and len(ev) == S
    w = [float(v) for v in w]
    K = sum(ev)
    hist = np.zeros((ndays, K + 1), np.int64)
    tipping = np.zeros((ndays, S + 1), np.int64)
    joint = np.zeros((ndays, S + 2, S + 2), np.int64)
    below = None if actual is None else np.zeros((ndays, S), np.int64)
    nat_all = np.zeros((nd, ndays))
    for d in range(nd):
        for t in range(ndays):
            x = [float(v) for v in ps[d, t]]
            dem, nat, pop, tip = item(x, w, ev, ev_to_win)
            nat_all[d, t] = nat
            hist[t, dem] += 1
            tipping[t, tip] += 1
            ind = [x[s] > 0.5 for s in range(S)] + [dem >= ev_to_win, pop]
            on = [i for i in range(S + 2) if ind[i]]
            for i in on:
                for j in on:
                    joint[t, i, j] += 1
            if actual is not None:
                for s in range(S):
                    if x[s] < actual[s]:
                        below[t, s] += 1
    return dict(ev_hist=hist, tipping=tipping, joint=joint, below_actual=below, n_draws=nd, nat=nat_all)


def outcomes_vectorised(ps, w, ev, ev_to_win=270, actual=None):
    """The same counts (no `nat`), vectorised over the draws of each day."""
    ps = np.asarray(ps, dtype=np.float64)
    nd, ndays, S = ps.shape
    ev = np.asarray(ev, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64)
    K = int(ev.sum())
    hist = np.zeros((ndays, K + 1), np.int64)
    tipping = np.zeros((ndays, S + 1), np.int64)
    joint = np.zeros((ndays, S + 2, S + 2), np.int64)
    below = None if actual is None else np.zeros((ndays, S), np.int64)
    for t in range(ndays):
        x = ps[:, t, :]
        nat = np.zeros(nd)
        for s in range(S):                                   # the documented order
            nat += w[s] * x[:, s]
        win = x > 0.5
        dem = (win * ev).sum(axis=1)
        pop = nat > 0.5
        order = np.argsort(np.where(pop[:, None], -x, x), axis=1, kind="stable")
        cum = np.cumsum(ev[order], axis=1)
        reached = cum >= ev_to_win
        first = reached.argmax(axis=1)
        tip = np.where(reached.any(axis=1), order[np.arange(nd), first], S)
        hist[t] = np.bincount(dem, minlength=K + 1)
        tipping[t] = np.bincount(tip, minlength=S + 1)
        ind = np.concatenate([win, (dem >= ev_to_win)[:, None], pop[:, None]], axis=1).astype(np.int64)
        joint[t] = ind.T @ ind
        if actual is not None:
            below[t] = (x < np.asarray(actual)[None, :]).sum(axis=0)
    return dict(ev_hist=hist, tipping=tipping, joint=joint, below_actual=below, n_draws=nd)


def p_values(below, n):
    return (2.0 * np.asarray(below, dtype=np.float64) + 1.0) / (2.0 * n + 2.0)
