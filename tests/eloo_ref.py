"""numpy restatement of E_loo as DESIGN.md section 4r defines it (loo's E_loo with the Pareto k of the estimate): weighted mean, centred
variance, sd, weighted quantiles and their k-hat, the shared form (quantities common to all polls) and predict's variance formula.  Built on
psis_ref (gpdfit, tail_length, psis) and loo_mm_ref.psis_general; the GPU tests hold potus_e_loo_device / potus_e_loo_shared_device against
this file, tests/test_eloo_host.py holds this file against cases with a known answer."""
from __future__ import annotations

import numpy as np

import psis_ref
from loo_mm_ref import psis_general
from psis_ref import gpdfit, tail_length


def weights(r, r_eff):
    """(w, k_r) of the raw log ratios r [S]: w = exp of psis_general's normalised log weights (a weight of -inf is 0)."""
    lw, k = psis_general(r, r_eff)
    return np.exp(lw), k


def r_eff_of(r):
    """the r_eff potus_loo computes for a poll with log-likelihoods -r [C, n]"""
    return psis_ref.relative_eff(-np.asarray(r, dtype=np.float64))


def tail_khat(v, M):
    """k-hat of the right tail of v: the M largest values minus the value just below them, through gpdfit with its prior term."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if M < 5:
        return np.inf
    s = np.sort(v)
    tail, cutoff = s[v.size - M:], s[v.size - M - 1]
    if abs(tail[-1] - tail[0]) < np.finfo(float).eps / 100:
        return np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        return gpdfit(tail - cutoff)[0]


def is_plain(h):
    """h constant, taking exactly two distinct values, or not finite somewhere: its k is k_r."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    return (not np.isfinite(h).all()) or np.unique(h).size <= 2


def khat(h, r, r_eff, k_r):
    """max(k_r, k_hr), k_hr the larger k-hat of the right tails of h rho and -h rho (rho = exp(r - max r)); k_r when h is None or plain."""
    if h is None or is_plain(h):
        return k_r
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    v = np.asarray(h, dtype=np.float64).reshape(-1) * np.exp(r - r.max()) + 0.0
    M = tail_length(r_eff, r.size)
    return max(k_r, tail_khat(v, M), tail_khat(-v + 0.0, M))


def wquantile(x, w, probs):
    """The weighted quantiles of the definition: type 7 (numpy's default) when all weights are equal."""
    x, w = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(w, dtype=np.float64).reshape(-1)
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if np.all(w == w[0]):
        return np.quantile(x, probs)
    order = np.argsort(x + 0.0, kind="stable")          # ties by draw index
    xs, ws = x[order], w[order]
    ww = np.cumsum(ws) / ws.sum()
    out = np.empty(probs.size)
    for i, p in enumerate(probs):
        j = int(np.argmax(ww >= p))
        out[i] = xs[0] if j == 0 else xs[j - 1] + (xs[j] - xs[j - 1]) * (p - ww[j - 1]) / (ww[j] - ww[j - 1])
    return out


def moments(x, w):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    mean = np.sum(w * x)
    var = np.sum(w * (x - mean) ** 2)
    return mean, var


def e_loo(x, r, probs=(), r_eff=None):
    """x, r [polls, C, n] -> out [polls, 3 + len(probs)] = mean, variance, sd, quantiles; khat [polls, 3] = k of the mean, of variance and
    sd, of the quantiles (the layout of potus_e_loo_device)."""
    x, r = np.asarray(x, dtype=np.float64), np.asarray(r, dtype=np.float64)
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    out, kh = np.zeros((x.shape[0], 3 + probs.size)), np.zeros((x.shape[0], 3))
    for i in range(x.shape[0]):
        re = r_eff_of(r[i]) if r_eff is None else float(r_eff[i])
        w, k_r = weights(r[i], re)
        xi = x[i].reshape(-1)
        mean, var = moments(xi, w)
        out[i, :3] = mean, var, np.sqrt(var)
        if probs.size:
            out[i, 3:] = wquantile(xi, w, probs)
        kh[i] = khat(xi, r[i], re, k_r), khat(xi * xi, r[i], re, k_r), k_r
    return out, kh


def e_loo_shared(X, lw, r=None, r_eff=None, diag=False):
    """X [cols, C, n], lw [polls, C, n] normalised log weights -> mean, var [polls, cols], ess [polls] = 1 / sum w^2, and khat: None
    without r, k_r [polls] with diag False, the k of every mean [polls, cols] with diag True."""
    X, lw = np.asarray(X, dtype=np.float64), np.asarray(lw, dtype=np.float64)
    Xf, W = X.reshape(X.shape[0], -1), np.exp(lw.reshape(lw.shape[0], -1))
    mean = W @ Xf.T
    var = np.stack([(W * (Xf[j][None, :] - mean[:, j][:, None]) ** 2).sum(axis=1) for j in range(Xf.shape[0])], axis=1)
    ess = 1.0 / (W * W).sum(axis=1)
    kh = None
    if r is not None:
        r = np.asarray(r, dtype=np.float64)
        res = [r_eff_of(r[i]) if r_eff is None else float(r_eff[i]) for i in range(r.shape[0])]
        k_r = np.array([psis_general(r[i], res[i])[1] for i in range(r.shape[0])])
        kh = k_r if not diag else np.array([[khat(Xf[j], r[i], res[i], k_r[i]) for j in range(Xf.shape[0])] for i in range(r.shape[0])])
    return mean, var, ess, kh


def predict_var(e_a1, e_a2, n):
    """LOO predictive variance of a poll's observed share y / n, y ~ Binomial(n, p): E[a1] / n + (1 - 1 / n) E[a2] - E[a1]^2 with a1 = E_z[p],
    a2 = E_z[p^2] under the leave-one-out posterior."""
    return e_a1 / n + (1.0 - 1.0 / n) * e_a2 - e_a1 ** 2


def poll_share(eta, sigma, z, integrate, Q=16):
    """(a1, a2) = E_z[p], E_z[p^2] with p = inv_logit(eta + sigma z): at the given z (integrate False), or over z ~ N(0, 1) by Q Gauss-Hermite
    nodes centred at 0 (k_el_poll_share).  Broadcasts."""
    eta, sigma, z = np.broadcast_arrays(np.asarray(eta, float), np.asarray(sigma, float), np.asarray(z, float))
    if not integrate:
        p = 1.0 / (1.0 + np.exp(-(eta + sigma * z)))
        return p, p * p
    xk, wk = np.polynomial.hermite.hermgauss(Q)
    p = 1.0 / (1.0 + np.exp(-(eta[..., None] + sigma[..., None] * np.sqrt(2.0) * xk)))
    return (p * wk).sum(axis=-1) / np.sqrt(np.pi), (p * p * wk).sum(axis=-1) / np.sqrt(np.pi)


def poll_share_quad(eta, sigma):
    """the same two integrals by scipy.integrate.quad (the independent check of the rule)"""
    from scipy import integrate
    f = lambda u, k: (1.0 / (1.0 + np.exp(-(eta + sigma * u)))) ** k * np.exp(-0.5 * u * u) / np.sqrt(2 * np.pi)
    return tuple(integrate.quad(f, -12, 12, args=(k,), epsabs=0, epsrel=1e-13, limit=400)[0] for k in (1, 2))
