"""numpy / scipy restatement of PSIS-LOO as the loo R package (2.x) computes it: relative_eff(), psis() with gpdfit(), the pointwise and
total estimates, and the integrated per-poll likelihood by adaptive Gauss-Hermite quadrature.  The GPU tests compare
potus_loo / potus_log_lik_device with this file; DESIGN.md section 4e states the same definitions."""
from __future__ import annotations

import numpy as np
from scipy.special import gammaln, logsumexp

GH_NODES = 16             # Q of the device's quadrature (potus_loo.hpp LOO_GH)
MODE_CAP = 100            # most trips of the mode search (potus_loo.hpp LOO_MODE_CAP)


def ess_rfun(x):
    """loo's ess_rfun of x [n, C] (draws of C chains, not split): ESS from Geyer's initial positive, then monotone sequence."""
    x = np.asarray(x, dtype=np.float64)
    n, C = x.shape
    xc = x - x.mean(axis=0)
    acov = np.empty((n, C))
    for c in range(C):                                 # biased autocovariance, sum / n
        v = xc[:, c]
        acov[:, c] = np.correlate(v, v, mode="full")[n - 1:] / n
    chain_mean = x.mean(axis=0)
    mean_var = acov[0].mean() * n / (n - 1)
    var_plus = mean_var * (n - 1) / n
    if C > 1:
        var_plus += np.var(chain_mean, ddof=1)
    rho = np.zeros(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        def rho_at(t):
            return 1.0 - (mean_var - acov[t].mean()) / var_plus
        t = 0
        even, odd = 1.0, rho_at(1)
        rho[0], rho[1] = even, odd
        while t < n - 5 and not np.isnan(even + odd) and even + odd > 0:
            t += 2
            even, odd = rho_at(t), rho_at(t + 1)
            if even + odd >= 0:
                rho[t], rho[t + 1] = even, odd
        max_t = t
        if even > 0:
            rho[max_t] = even
        t = 0
        while t <= max_t - 4:
            t += 2
            if rho[t] + rho[t + 1] > rho[t - 2] + rho[t - 1]:
                rho[t] = (rho[t - 2] + rho[t - 1]) / 2
                rho[t + 1] = rho[t]
        S = C * n
        tau = -1.0 + 2.0 * rho[:max_t].sum() + rho[max_t]
        tau = max(tau, 1.0 / np.log10(S))
    return S / tau


def relative_eff(ll):
    """r_eff of one poll's log-likelihoods ll [C, n]: ESS / S of exp(ll - max ll)."""
    ll = np.asarray(ll, dtype=np.float64)
    x = np.exp(ll - ll.max())
    return ess_rfun(x.T) / ll.size


def gpdfit(x):
    """Zhang & Stephens (2009) with loo's weakly informative prior on k; x sorted ascending.  Returns (k, sigma)."""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    m = 30 + int(np.floor(np.sqrt(N)))
    jj = np.arange(1, m + 1)
    xstar = x[int(np.floor(N / 4 + 0.5)) - 1]
    theta = 1.0 / x[N - 1] + (1.0 - np.sqrt(m / (jj - 0.5))) / 3.0 / xstar
    with np.errstate(invalid="ignore", divide="ignore"):
        kj = np.array([np.mean(np.log1p(-t * x)) for t in theta])
        l_theta = N * (np.log(-theta / kj) - kj - 1.0)
        w = np.exp(l_theta - logsumexp(l_theta))
        theta_hat = np.sum(theta * w)
        k = np.mean(np.log1p(-theta_hat * x))
        sigma = -k / theta_hat
        k = k * N / (N + 10) + 10 * 0.5 / (N + 10)
    if np.isnan(k):
        k = np.inf
    return k, sigma


def tail_length(r_eff, S):
    return int(np.ceil(min(0.2 * S, 3.0 * np.sqrt(S / r_eff))))


def psis(ll, r_eff):
    """Normalised PSIS log weights of the leave-one-out ratios -ll (any shape, S draws) and k-hat."""
    r = -np.asarray(ll, dtype=np.float64).reshape(-1)
    S = r.size
    lw = r - r.max()
    k = np.inf
    M = tail_length(r_eff, S)
    if M >= 5:
        order = np.argsort(lw, kind="stable")
        tail_ids = order[S - M:]
        tail = lw[tail_ids]
        if abs(tail[-1] - tail[0]) >= np.finfo(float).eps / 100:
            cutoff = lw[order[S - M - 1]]
            k, sigma = gpdfit(np.exp(tail) - np.exp(cutoff))
            if np.isfinite(k):
                p = (np.arange(1, M + 1) - 0.5) / M
                with np.errstate(invalid="ignore", divide="ignore"):
                    tail = np.log(sigma * np.expm1(-k * np.log1p(-p)) / k + np.exp(cutoff))
            lw[tail_ids] = tail
    lw = np.minimum(lw, 0.0)
    return lw - logsumexp(lw), k


def loo_pointwise(ll, r_eff=None):
    """ll [N_polls, C, n] -> pointwise [N_polls, 5] = elpd_loo, p_loo, looic, pareto_k, r_eff (the layout of potus_loo)."""
    ll = np.asarray(ll, dtype=np.float64)
    out = np.zeros((ll.shape[0], 5))
    for i in range(ll.shape[0]):
        re = relative_eff(ll[i]) if r_eff is None else float(r_eff[i])
        lw, k = psis(ll[i], re)
        x = ll[i].reshape(-1)
        elpd = logsumexp(x + lw)
        lpd = logsumexp(x) - np.log(x.size)
        out[i] = elpd, lpd - elpd, -2.0 * elpd, k, re
    return out


def estimates(pointwise):
    """[3, 2] = (elpd_loo, p_loo, looic) x (estimate, se); se = sqrt(N) sd."""
    pw = np.asarray(pointwise)[:, :3]
    N = pw.shape[0]
    return np.stack([pw.sum(axis=0), np.sqrt(N) * pw.std(axis=0, ddof=1)], axis=1)


# ---- per-poll likelihoods
def lchoose(n, y):
    return gammaln(np.asarray(n, float) + 1) - gammaln(np.asarray(y, float) + 1) - gammaln(np.asarray(n, float) - y + 1)


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def binom_term(y, n, x):
    """y log inv_logit(x) + (n - y) log inv_logit(-x) = y x - n softplus(x), in the form without cancellation that loo_poll_ll uses."""
    return y * np.minimum(x, 0.0) - (n - y) * np.maximum(x, 0.0) - n * np.log1p(np.exp(-np.abs(x)))


def log_lik_plain(y, n, x):
    """binomial_logit_lpmf(y | n, x), with log C(n, y)."""
    return lchoose(n, y) + binom_term(y, n, x)


def _expit(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def integrand_mode(y, n, eta, sigma, cap=MODE_CAP):
    """The mode of f(z) = y x - n softplus(x) - z^2 / 2, x = eta + sigma z, as loo_poll_ll finds it: f'(z) = sigma (y - n p(x)) - z is strictly
    decreasing with its root in [sigma (y - n), sigma y]; Newton steps from 0, the bracket narrowed by the sign of every f', a step that does not
    land strictly inside it replaced by the midpoint; an element stops when a step no longer moves it.  Broadcasts."""
    y, n, eta, sigma = (np.asarray(a, dtype=np.float64) for a in np.broadcast_arrays(y, n, eta, sigma))
    z, lo, hi = np.zeros_like(eta), sigma * (y - n), sigma * y
    live = np.ones(z.shape, bool)
    for _ in range(cap):
        p = _expit(eta + sigma * z)
        g = sigma * (y - n * p) - z
        live = live & (g != 0)
        lo, hi = np.where(live & (g > 0), z, lo), np.where(live & (g < 0), z, hi)
        zn = z - g / (-sigma * sigma * n * p * (1 - p) - 1.0)
        live = live & (zn != z)
        zn = np.where((zn > lo) & (zn < hi), zn, 0.5 * (lo + hi))
        live = live & (zn != z)
        if not live.any():
            break
        z = np.where(live, zn, z)
    return z


def log_lik_integrated(y, n, eta, sigma, Q=GH_NODES):
    """log int Binomial(y | n, inv_logit(eta + sigma z)) phi(z) dz by adaptive Gauss-Hermite quadrature: the mode of the strictly concave
    f(z) = y x - n softplus(x) - z^2 / 2 (x = eta + sigma z) by integrand_mode, nodes scaled by sqrt(2 / -f''(mode)).  Broadcasts."""
    y, n, eta, sigma = (np.asarray(a, dtype=np.float64) for a in np.broadcast_arrays(y, n, eta, sigma))
    z = integrand_mode(y, n, eta, sigma)
    p = _expit(eta + sigma * z)
    s = np.sqrt(2.0 / (sigma * sigma * n * p * (1 - p) + 1.0))
    xk, wk = np.polynomial.hermite.hermgauss(Q)
    zk = z[..., None] + s[..., None] * xk
    xx = eta[..., None] + sigma[..., None] * zk
    f = binom_term(y[..., None], n[..., None], xx) - 0.5 * zk * zk + xk * xk + np.log(wk)
    out = lchoose(n, y) + logsumexp(f, axis=-1) + np.log(s) - 0.5 * np.log(2 * np.pi)
    return np.where(sigma == 0, log_lik_plain(y, n, eta), out)


def log_lik_quad(y, n, eta, sigma):
    """The same integral by scipy.integrate.quad around the mode (the independent check): the mode is the root of the strictly decreasing
    f'(z) = sigma (y - n p) - z, bracketed by [sigma (y - n), sigma y], by scipy.optimize.brentq."""
    from scipy import integrate, optimize
    y, n, eta, sigma = float(y), float(n), float(eta), float(sigma)
    if sigma == 0.0:
        return float(log_lik_plain(y, n, eta))

    def df(u):
        return sigma * (y - n * float(_expit(eta + sigma * u))) - u

    a, b = sigma * (y - n), sigma * y
    z = a if a == b else optimize.brentq(df, a, b, xtol=1e-300, rtol=4 * np.finfo(float).eps, maxiter=500)
    p = float(_expit(eta + sigma * z))
    sd = 1.0 / np.sqrt(sigma * sigma * n * p * (1 - p) + 1.0)

    def f(u):
        x = eta + sigma * u
        return binom_term(y, n, x) - 0.5 * u * u

    f0 = f(z)
    val, _ = integrate.quad(lambda u: np.exp(f(u) - f0), z - 40 * sd, z + 40 * sd, epsabs=0, epsrel=1e-13, limit=400, points=[z])
    return float(lchoose(n, y) + f0 + np.log(val) - 0.5 * np.log(2 * np.pi))
