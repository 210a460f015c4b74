"""The posterior predictive check of DESIGN.md section 4s restated in numpy, operation by operation (every product, sum and quotient rounded on
its own, as the device code is compiled): the residuals, the group sums in ascending poll number, the counts, the PIT sums, the non-randomised
PIT histogram (Czado, Gneiting, Held 2009) and the coverage.  Blocks are [polls, S] (S = chains x draws, flattened)."""
import numpy as np


def moments(n, a1, a2):
    """m = n a1 and sd = sqrt(v), v = n a1 (1 - a1) + n (n - 1) max(a2 - a1^2, 0); sd = 0 unless v > 0.  n [polls], a1, a2 [polls, S]."""
    n = np.asarray(n, dtype=np.float64)[:, None]
    m = n * a1
    d = a2 - a1 * a1
    v = (n * a1) * (1.0 - a1) + (n * (n - 1.0)) * np.where(d > 0.0, d, 0.0)
    with np.errstate(invalid="ignore"):
        sd = np.where(v > 0.0, np.sqrt(np.where(v > 0.0, v, 1.0)), 0.0)
    return m, sd


def resid(k, m, sd):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(sd > 0.0, (k - m) / np.where(sd > 0.0, sd, 1.0), 0.0)


def group_sums(yrep, a1, a2, y, n, labels, G):
    """T [G, 3, 2, S] (bias, dispersion, count) x (realised, replicated) and n_in_group [G]: the polls with n > 0 of each group added one after
    the other in ascending poll number, from 0."""
    y, n, labels = np.asarray(y, dtype=np.float64), np.asarray(n, dtype=np.float64), np.asarray(labels)
    S = yrep.shape[1]
    T, cnt = np.zeros((G, 3, 2, S)), np.zeros(G, np.int64)
    m, sd = moments(n, a1, a2)
    for i in range(len(y)):
        g = int(labels[i])
        if g < 0 or not n[i] > 0:
            continue
        ro, rr = resid(np.full(S, y[i]), m[i], sd[i]), resid(yrep[i], m[i], sd[i])
        T[g, 0, 0] = T[g, 0, 0] + ro
        T[g, 0, 1] = T[g, 0, 1] + rr
        T[g, 1, 0] = T[g, 1, 0] + ro * ro
        T[g, 1, 1] = T[g, 1, 1] + rr * rr
        T[g, 2, 0] = T[g, 2, 0] + y[i]
        T[g, 2, 1] = T[g, 2, 1] + yrep[i]
        cnt[g] += 1
    return T, cnt


def group_table(T, cnt):
    """[G, 3, 6]: mean T_obs, mean T_rep, #{T_rep > T_obs}, #{=}, #{<}, p = (gt + eq / 2) / S; a group without polls: NaN, NaN, 0, 0, 0, NaN."""
    G, S = T.shape[0], T.shape[3]
    out = np.zeros((G, 3, 6))
    for g in range(G):
        for k in range(3):
            if cnt[g] == 0:
                out[g, k] = (np.nan, np.nan, 0, 0, 0, np.nan)
                continue
            o, r = T[g, k, 0], T[g, k, 1]
            gt, eq, lt = int((r > o).sum()), int((r == o).sum()), int((r < o).sum())
            out[g, k] = (o.sum() / S, r.sum() / S, gt, eq, lt, (gt + 0.5 * eq) / S)
    return out


def near_ties(T, rel=1e-9):
    """[G, 3] the number of draws where T_rep and T_obs are within rel (1 + |T_obs|) of each other without being equal: the cells in which a
    last-place difference of the sums may move a draw between gt, eq and lt."""
    o, r = T[:, :, 0], T[:, :, 1]
    return ((np.abs(r - o) <= rel * (1.0 + np.abs(o))) & (r != o)).sum(axis=-1)


def pit_sums(yrep, y, lw=None):
    """lo [polls] = sum_s w [y_rep < y], eq = sum_s w [y_rep = y]; w = exp(lw) (a weight of -inf is 0, NaN gives NaN), or 1 / S: the counts over S."""
    y = np.asarray(y, dtype=np.float64)[:, None]
    S = yrep.shape[1]
    if lw is None:
        return (yrep < y).sum(axis=1) / S, (yrep == y).sum(axis=1) / S
    w = np.exp(lw)
    return (w * (yrep < y)).sum(axis=1), (w * (yrep == y)).sum(axis=1)


def pit_cdf(lo, eq, u):
    """The mean over the polls of F_i(u): 0 up to lo_i, linear to 1 at lo_i + eq_i, F_i(0) = 0; polls with NaN sums left out."""
    lo, eq = np.asarray(lo, dtype=np.float64), np.asarray(eq, dtype=np.float64)
    ok = np.isfinite(lo) & np.isfinite(eq)
    out = []
    for uu in np.atleast_1d(u):
        tot = 0.0
        for l, e in zip(lo[ok], eq[ok]):
            h = min(l + e, 1.0)
            tot += 0.0 if uu <= 0.0 else 1.0 if uu >= h else 0.0 if uu <= l else (uu - l) / (h - l)
        out.append(tot / ok.sum())
    return np.array(out)


def pit_hist(lo, eq, bins=10):
    return np.diff(pit_cdf(lo, eq, np.linspace(0.0, 1.0, bins + 1)))


def coverage(lo, eq, level=0.95):
    a, b = pit_cdf(lo, eq, [(1.0 - level) / 2.0, (1.0 + level) / 2.0])
    return float(b - a)


def randomised(lo, eq, seed=0):
    return lo + np.random.default_rng(seed).random(np.shape(lo)) * eq
