"""A numpy restatement of the scoring rules of include/potus_hmc.h (potus_forecast_scores): the pairwise forms taken literally, O(n^2),
sums in np.longdouble, numpy.linalg for the joint Dawid-Sebastiani score.  tests/test_scoring_host.py earns it its trust."""
import numpy as np

LD = np.longdouble
UNI = ("crps", "pit_lo", "pit_hi", "dss", "interval", "ae_median", "se_mean")


def _sum(a):
    return np.sum(np.asarray(a, dtype=LD), dtype=LD)


def crps_pairwise(x, y):
    """mean|x - y| - sum_i sum_j |x_i - x_j| / (2 n^2)"""
    x = np.asarray(x, dtype=LD)
    n = x.size
    return float(_sum(np.abs(x - LD(y))) / n - _sum(np.abs(x[:, None] - x[None, :])) / (2 * LD(n) * n))


def crps_sorted(x, y):
    """(2 / n^2) sum_i (x_(i) - y)(n 1[y < x_(i)] - i + 1/2)"""
    x = np.sort(np.asarray(x, dtype=LD))
    n = x.size
    i = np.arange(1, n + 1, dtype=LD)
    return float(2 * _sum((x - LD(y)) * (n * (LD(y) < x) - i + LD(0.5))) / (LD(n) * n))


def variance(x):
    """ddof 1, two passes; exactly 0 for a constant sample, NaN for n = 1"""
    x = np.asarray(x, dtype=LD)
    if x.size < 2:
        return float("nan")
    if x.min() == x.max():
        return 0.0
    m = _sum(x) / x.size
    return float(_sum((x - m) ** 2) / (x.size - 1))


def column(x, y):
    """The seven univariate scores of one column x [n] against y, in the order of UNI."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    if not np.isfinite(x).all():
        return np.full(len(UNI), np.nan)
    m = float(_sum(x) / n)
    v = variance(x)
    lo, med, hi = (float(q) for q in np.quantile(x, [0.025, 0.5, 0.975]))     # numpy's default is R's type 7
    dss = np.log(v) + (y - m) ** 2 / v if v > 0 else np.nan
    return np.array([crps_pairwise(x, y), (x < y).sum() / n, (x <= y).sum() / n, dss,
                     (hi - lo) + 40.0 * max(lo - y, 0.0) + 40.0 * max(y - hi, 0.0), abs(med - y), (m - y) ** 2])


def energy(x, y):
    """x [n, m], y [m]: (1 / n) sum_i |x_i - y| - (1 / (2 n^2)) sum_i sum_j |x_i - x_j|, every pair by direct differences"""
    x, y = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    n = x.shape[0]
    single = _sum(np.sqrt(((x - y[None, :]) ** 2).sum(axis=1, dtype=LD)))
    pairs = LD(0)
    for i in range(n):
        pairs += _sum(np.sqrt(((x - x[i][None, :]) ** 2).sum(axis=1, dtype=LD)))
    return float(single / n - pairs / (2 * LD(n) * n))


def variogram(x, y, p=0.5):
    """sum_{a < b} (|y_a - y_b|^p - (1 / n) sum_i |x_ia - x_ib|^p)^2; 0 when m = 1"""
    x, y = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    n, m = x.shape
    tot = LD(0)
    for a in range(m):
        for b in range(a + 1, m):
            tot += (np.abs(y[a] - y[b]) ** LD(p) - _sum(np.abs(x[:, a] - x[:, b]) ** LD(p)) / n) ** 2
    return float(tot)


def dss_joint(x, y):
    """log det Sigma + (y - mu)' Sigma^-1 (y - mu), Sigma of ddof 1; NaN when n <= m or Sigma is not positive definite"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, m = x.shape
    if n <= m or not np.isfinite(x).all():
        return float("nan")
    mu = x.mean(axis=0)
    d = x - mu
    cov = d.T @ d / (n - 1)
    try:
        L = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        return float("nan")
    z = np.linalg.solve(L, y - mu)
    return float(2.0 * np.log(np.diagonal(L)).sum() + z @ z)


def derived(x, w, ev):
    """x [n, S] -> [n, S + 2]: the states, the national vote (summed in index order) and the electoral votes of every draw"""
    x = np.asarray(x, dtype=np.float64)
    nat = np.zeros(x.shape[0])
    for s in range(x.shape[1]):
        nat = nat + w[s] * x[:, s]
    with np.errstate(invalid="ignore"):
        votes = ((x > 0.5) * np.asarray(ev, dtype=np.float64)[None, :]).sum(axis=1)
    return np.concatenate([x, nat[:, None], votes[:, None]], axis=1)


def full_actual(y, w, ev):
    """actual [S] -> [S + 2] as scoring.check_args derives it"""
    y = np.asarray(y, dtype=np.float64)
    nat = 0.0
    for s in range(y.size):
        nat = nat + float(w[s]) * float(y[s])
    return np.concatenate([y, [nat, float(np.asarray(ev, dtype=np.float64)[y > 0.5].sum())]])


def scores(ps, w, ev, actual, use=None, vs_p=0.5):
    """ps [n, days, S], actual [S + 2] -> (uni [days, S + 2, 7], multi [days, 3]) with the rule for values that are not finite."""
    ps = np.asarray(ps, dtype=np.float64)
    n, nd, S = ps.shape
    u = np.ones(S, bool) if use is None else np.asarray(use) != 0
    uni, multi = np.zeros((nd, S + 2, len(UNI))), np.zeros((nd, 3))
    for t in range(nd):
        x = ps[:, t]
        cols = derived(x, w, ev)
        fin = np.isfinite(x).all(axis=0)
        for c in range(S + 2):
            uni[t, c] = column(cols[:, c], actual[c]) if (fin[c] if c < S else fin.all()) else np.nan
        if not fin[u].all():
            multi[t] = np.nan
            continue
        xu, yu = x[:, u], np.asarray(actual)[:S][u]
        multi[t] = energy(xu, yu), variogram(xu, yu, vs_p), dss_joint(xu, yu)
    return uni, multi
