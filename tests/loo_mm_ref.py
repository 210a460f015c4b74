"""numpy restatement of moment matching for PSIS-LOO (Paananen, Piironen, Buerkner, Vehtari 2021) as potus_loo_moment_match runs it:
DESIGN.md section 4q states the same definitions.  Generic over two callables, log_prob(theta [S, D]) -> [S] (the log density, Jacobian in,
constants dropped) and log_lik(theta [S, D]) -> [S] (the left-out observation's log-likelihood).  The map of a poll stays diagonal-affine,
T(theta) = a + b * theta; no covariance step.  moment_match() records every candidate and every k, so that the host rules
(csrc/potus_loo_mm_rules.hpp) and the device call can be held against it decision by decision."""
from __future__ import annotations

import numpy as np
from scipy.special import logsumexp

from psis_ref import gpdfit, tail_length

T1, T2 = 1, 2
RUNNING, BELOW, MAXIT, REJECTED = 0, 1, 2, 3


def default_threshold(S):
    return min(1.0 - 1.0 / np.log10(S), 0.7)


def psis_general(r, r_eff):
    """Normalised PSIS log weights of general log ratios r [S] and k-hat: psis_ref.psis on r instead of -ll.  -inf entries are legal (weight
    0); a NaN or +inf entry, or no finite entry at all, gives (all NaN, NaN): the candidate is rejected."""
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    S = r.size
    if np.isnan(r).any() or (r == np.inf).any() or not np.isfinite(r).any():
        return np.full(S, np.nan), np.nan
    lw = r - r.max() + 0.0
    k = np.inf
    M = tail_length(r_eff, S)
    if M >= 5:
        order = np.argsort(lw, kind="stable")
        tail_ids = order[S - M:]
        tail = lw[tail_ids]
        if abs(tail[-1] - tail[0]) >= np.finfo(float).eps / 100:
            cutoff = lw[order[S - M - 1]]
            with np.errstate(invalid="ignore", divide="ignore"):
                k, sigma = gpdfit(np.exp(tail) - np.exp(cutoff))
                if np.isfinite(k):
                    p = (np.arange(1, M + 1) - 0.5) / M
                    tail = np.log(sigma * np.expm1(-k * np.log1p(-p)) / k + np.exp(cutoff))
            lw[tail_ids] = tail
    lw = np.minimum(lw, 0.0)
    return lw - logsumexp(lw), k


def ratios(ll, lp, lp0):
    """r = -ll + lp - lp0, -inf where a term is not finite."""
    with np.errstate(invalid="ignore"):
        r = -ll + lp - lp0
    return np.where(np.isfinite(ll) & np.isfinite(lp) & np.isfinite(lp0), r, -np.inf)


def weighted_moments(theta, m0, lw):
    """mu~ = sum w theta, q~ = sum w (theta - m0)^2 under w = exp(lw)."""
    w = np.exp(lw)[:, None]
    return (w * theta).sum(axis=0), (w * (theta - m0) ** 2).sum(axis=0)


def current_moments(a, b, m0, mu_t, q_t, S):
    """(m, mu_w, sigma2_w) of the sample T(theta) from the moments of theta: its mean, weighted mean and weighted variance."""
    return a + b * m0, a + b * mu_t, b * b * (q_t - (mu_t - m0) ** 2) * S / (S - 1)


def candidate(which, a, b, m0, v0, mu_t, q_t, S):
    m, mu_w, s2_w = current_moments(a, b, m0, mu_t, q_t, S)
    if which == T1:
        return a + (mu_w - m), b.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.sqrt(s2_w / (b * b * v0))
    rho = np.where(np.isfinite(rho) & (rho > 0), rho, 1.0)
    return mu_w - rho * b * m0, rho * b


def inverse(x, a, b):
    return (x - a) / b


class Rules:
    """potus_loo_mm_rules.hpp's LmmPoll."""

    def __init__(self, k0, thr, max_iters):
        self.k, self.thr, self.max_iters = k0, thr, max_iters
        self.n_t1 = self.n_t2 = self.rounds = 0
        self.stop, self.next = RUNNING, 0
        self._head()

    def accepted(self):
        return self.n_t1 + self.n_t2

    def _head(self):
        if not self.k > self.thr:
            self.stop, self.next = BELOW, 0
        elif self.accepted() >= self.max_iters:
            self.stop, self.next = MAXIT, 0
        else:
            self.next = T1

    def feed(self, k_new):
        self.rounds += 1
        if k_new < self.k:
            if self.next == T1:
                self.n_t1 += 1
            else:
                self.n_t2 += 1
            self.k = k_new
            self._head()
            return True
        if self.next == T1:
            self.next = T2
        else:
            self.stop, self.next = REJECTED, 0
        return False

    def info(self):
        return (self.n_t1, self.n_t2, self.rounds, self.stop)


def decisions(ks, thr, max_iters):
    """The rules fed a recorded sequence k0, k'1, k'2, ...: [(candidate, accepted)] and the final info; stops when the rules stop."""
    ru, out = Rules(ks[0], thr, max_iters), []
    for k in ks[1:]:
        if not ru.next:
            break
        c = ru.next
        out.append((c, ru.feed(k)))
    return out, ru.info()


def moment_match(theta, n_per_chain, log_prob, log_lik, r_eff, k_threshold=None, max_iters=30, split=True):
    """theta [S, D] pooled draws in canonical order ([chain][iteration], n_per_chain iterations each).  Returns a dict: elpd, k, a, b,
    steps [(candidate, k', accepted)], k_path (k0 then every k' evaluated, the split's last), info (n_t1, n_t2, rounds, stop), split_done,
    k0, elpd0, k_loop and elpd_loop (before the split), lw (final normalised log weights) and ll (the log-likelihood at the points the
    weights belong to)."""
    theta = np.asarray(theta, dtype=np.float64)
    S, D = theta.shape
    thr = default_threshold(S) if k_threshold is None else k_threshold
    m0, v0 = theta.mean(axis=0), theta.var(axis=0, ddof=1)
    lp0, ll0 = log_prob(theta), log_lik(theta)
    lw, k = psis_general(-ll0, r_eff)
    a, b = np.zeros(D), np.ones(D)
    ll, k_path, steps = ll0, [k], []
    elpd0 = logsumexp(ll0 + lw)
    ru = Rules(k, thr, max_iters)
    while ru.next:
        mu_t, q_t = weighted_moments(theta, m0, lw)
        a1, b1 = candidate(ru.next, a, b, m0, v0, mu_t, q_t, S)
        x = a1 + b1 * theta
        ll1 = log_lik(x)
        lw1, k1 = psis_general(ratios(ll1, log_prob(x), lp0), r_eff)
        k_path.append(k1)
        c = ru.next
        ok = ru.feed(k1)
        steps.append((c, k1, ok))
        if ok:
            a, b, lw, ll, k = a1, b1, lw1, ll1, k1
    k_loop, elpd_loop = k, logsumexp(ll + lw)                 # what a call with split off ends with
    split_done = bool(split and ru.accepted() > 0)
    if split_done:
        it = np.arange(S) % n_per_chain
        H = it % 2 == 0
        x = np.where(H[:, None], a + b * theta, theta)
        xinv = inverse(x, a, b)
        lpx, ll = log_prob(x), log_lik(x)
        lpi = np.where(H, lp0, log_prob(xinv)) - np.log(b).sum()
        with np.errstate(invalid="ignore"):
            r = -ll + lpx - np.logaddexp(lpx, lpi)
        r = np.where(np.isfinite(ll) & np.isfinite(lpx) & np.isfinite(r), r, -np.inf)
        lw, k = psis_general(r, r_eff)
        k_path.append(k)
    return dict(elpd=logsumexp(ll + lw), k=k, a=a, b=b, steps=steps, k_path=k_path, info=ru.info(), split_done=split_done, k0=k_path[0],
                elpd0=elpd0, lw=lw, ll=ll, k_loop=k_loop, elpd_loop=elpd_loop)
