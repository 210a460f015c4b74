"""A numpy restatement of potus_timeline's summary, for the tests: R's type-7 quantiles, the state_weights-weighted national vote, the
Democratic electoral votes.  x: predicted scores [draws, days, S] of ONE data set, draws in canonical order (chains one after another)."""
from fractions import Fraction

import numpy as np


def quantile7(x, p):
    """R's default quantile of the columns of x [n, ...]: with h = (n - 1) p it is x_(floor h) + (h - floor h) (x_(floor h + 1) - x_(floor h)).
    The formula is evaluated in exact rational arithmetic on the doubles x and p and rounded once: in floating point the rounding of h alone
    (half an ulp of h, 7e-15 for 100 draws) times a gap of 70 electoral votes between two order statistics is 5e-13."""
    xs = np.sort(np.asarray(x, dtype=np.float64), axis=0)
    n = xs.shape[0]
    h = Fraction(n - 1) * Fraction(float(p))
    lo = int(h // 1)
    hi = min(lo + 1, n - 1)
    frac = h - lo
    a, b = xs[lo], xs[hi]
    if frac == 0:
        return a.copy()
    out = np.array([float(Fraction(float(u)) + frac * (Fraction(float(v)) - Fraction(float(u)))) for u, v in zip(a.ravel(), b.ravel())])
    return out.reshape(a.shape)


def national(x, w):
    """sum_s w[s] x[..., s], added s = 0, 1, ... as the kernels add it; w normalised to sum to one (summed in index order)."""
    w = np.asarray(w, dtype=np.float64)
    sw = 0.0
    for v in w:
        sw += float(v)
    w = w / sw
    a = np.zeros(x.shape[:-1])
    for s in range(x.shape[-1]):
        a = a + w[s] * x[..., s]
    return a


def electoral_votes(x, ev):
    """sum_s ev[s] 1[x[..., s] > 0.5] (strict)."""
    return ((np.asarray(x) > 0.5) * np.asarray(ev, dtype=np.float64)).sum(-1)


def summary(x, w, ev, ev_to_win=270):
    """dict(state [days, S, 4] = low 2.5 %, high 97.5 %, mean, P(> 0.5); national [days, 4] the same; electoral_votes [days, 5] = mean,
    median, high, low, P(>= ev_to_win))."""
    x = np.asarray(x, dtype=np.float64)

    def four(v):
        return np.stack([quantile7(v, 0.025), quantile7(v, 0.975), v.mean(0), (v > 0.5).mean(0)], axis=-1)
    e = electoral_votes(x, ev)
    evs = np.stack([e.mean(0), quantile7(e, 0.5), quantile7(e, 0.975), quantile7(e, 0.025), (e >= ev_to_win).mean(0)], axis=-1)
    return dict(state=four(x), national=four(national(x, w)), electoral_votes=evs)
