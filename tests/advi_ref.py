"""CPU reference for mean-field ADVI (tests of potus_advi), numpy written from the rules include/potus_hmc.h states: the stochastic-gradient
step with its step-size memory, the ELBO, the step-size selection and the stop of the main run.  Every element-wise expression is written
operation by operation in the order csrc/potus_advi.hpp evaluates it (no fused multiply-add there), and every sum that the library takes in
index order is taken in index order here.

log_prob_grad is any callable q -> (lp, g): OracleModel.log_prob_grad for the poll models, a closed form for the Gaussian target of
tests/test_advi_host.py.  normals(stage, draw, it) -> eps [D] supplies the standard normals: library_normals restates the library's Philox
streams with the oracle's generator, as pathfinder_ref.library_normals does; numpy_normals gives numpy's own."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

RNG_ADVI = 10
ETAS = (100.0, 10.0, 1.0, 0.1, 0.01)
MEAN_CONVERGED, MEDIAN_CONVERGED, MAXIT, NONFINITE, INIT, ADAPT_FAILED = 1, 2, 3, 4, 5, 6
FLAG_DIVERGING = 1
LOG_2PI = 1.8378770664093454836
STAGE_ELBO, STAGE_DRAW = 8, 15


def library_normals(seed, run):
    """normals(stage, draw, it) of run `run` (run_offset + r) under the handle's seed: the Box-Muller pairs of counter
    {j, 10 | (stage | draw << 4) << 8, it, run + 1}."""
    from oracle_lib import lib as oracle_lib
    Lo = oracle_lib()
    a, b = C.c_double(), C.c_double()

    def normals(stage, draw, it, D):
        out = np.zeros(2 * ((D + 1) // 2))
        aux = int(stage) | (int(draw) << 4)
        for j in range((D + 1) // 2):
            Lo.oracle_rng_normal_pair(int(seed), run + 1, int(it), RNG_ADVI, aux, j, C.byref(a), C.byref(b))
            out[2 * j], out[2 * j + 1] = a.value, b.value
        return out[:D]
    return normals


def numpy_normals(seed):
    """normals(stage, draw, it) from numpy: a generator per counter, so the draws do not depend on the order they are asked for in."""
    def normals(stage, draw, it, D):
        return np.random.default_rng([int(seed), int(stage), int(draw), int(it)]).standard_normal(D)
    return normals


def _update(g, step, t, x, s):
    g2 = g * g
    s = g2 if t == 1 else 0.9 * g2 + 0.1 * s
    return x + step * g / (1.0 + np.sqrt(s)), s


def sga(log_prob_grad, mu0, om0, eta, n_iter, normals, stage=0, grad_samples=1, t0=0, s=None, record=None):
    """n_iter gradient steps t0 + 1 .. t0 + n_iter.  Returns dict(mu, omega, s = (s_mu, s_omega), t, code): code NONFINITE at the last
    finished iterate when a pass gave a non-finite lp or gradient entry, else 0.  record(t, zeta, s_mu, mu, omega) is called with every
    pass's point and, after the step, its results (mu, omega None for all draws but an iteration's last)."""
    mu, om = np.array(mu0, dtype=np.float64), np.array(om0, dtype=np.float64)
    D = mu.size
    s_mu, s_om = (np.zeros(D), np.zeros(D)) if s is None else (s[0].copy(), s[1].copy())
    t = int(t0)
    with np.errstate(all="ignore"):
        for _ in range(int(n_iter)):
            a_mu = a_om = None
            zetas = []
            for m in range(int(grad_samples)):
                eps = normals(stage, m, t + 1, D)
                zeta = mu + np.exp(om) * eps
                lp, g = log_prob_grad(zeta)
                g = np.asarray(g, dtype=np.float64)
                if not (np.isfinite(lp) and np.isfinite(g).all()):
                    return dict(mu=mu, omega=om, s=(s_mu, s_om), t=t, code=NONFINITE)
                a_mu, a_om = (g, g * eps) if m == 0 else (a_mu + g, a_om + g * eps)
                zetas.append(zeta)
            M = float(grad_samples)
            step = eta / math.sqrt(float(t + 1))
            g_mu, g_om = a_mu / M, a_om / M * np.exp(om) + 1.0
            s_mu_before = s_mu
            mu, s_mu = _update(g_mu, step, t + 1, mu, s_mu)
            om, s_om = _update(g_om, step, t + 1, om, s_om)
            t += 1
            if record is not None:
                record(t, zetas, step, s_mu_before, s_mu, mu.copy(), om.copy())
    return dict(mu=mu, omega=om, s=(s_mu, s_om), t=t, code=0)


def elbo(log_prob_grad, mu, om, normals, stage, t, elbo_samples, elbo_offset=0.0, points=None):
    """ELBO at (mu, omega), the iterate t of the track `stage` (0 main, 1 .. 5 the candidates): the mean in index order, -inf when any lp is
    not finite.  points: a list the zeta_k are appended to."""
    D = mu.size
    acc, bad = 0.0, False
    with np.errstate(all="ignore"):
        for k in range(int(elbo_samples)):
            zeta = mu + np.exp(om) * normals(STAGE_ELBO + stage, k, t, D)
            if points is not None:
                points.append(zeta)
            lp = float(log_prob_grad(zeta)[0])
            bad = bad or not math.isfinite(lp)
            acc += lp
    if bad:
        return -math.inf
    ent = 0.0
    for w in om:                                          # (the device sums in another order: DEPTH eps sum|omega| in the tests' bound)
        ent += float(w)
    return acc / float(elbo_samples) + 0.5 * float(D) * (1.0 + LOG_2PI) + ent + float(elbo_offset)


def pick_eta(elbo_init, cand):
    """The sequential rule on the five candidates' ELBOs (-inf for a NONFINITE one): (index of eta* or -1 for ADAPT_FAILED, candidates seen)."""
    best, pick = -math.inf, -1
    for k, e in enumerate(cand):
        if e < best and best > elbo_init:
            return pick, k + 1
        if e > best:
            best, pick = e, k
        if k == len(cand) - 1 and not e > elbo_init:
            pick = -1
    return pick, len(cand)


class Conv:
    """The main run's stop: push(elbo, t) -> code (0: go on).  The buffer holds max(floor(0.1 iter / eval_elbo), 2) relative differences; mean =
    their sum, oldest first, over their number; median = Stan's circ_buff_median, the entry at n // 2 of the sorted ones (the UPPER middle one of
    an even number); a NaN among them makes both NaN."""

    def __init__(self, iter, eval_elbo, tol_rel_obj):
        self.iter, self.eval_elbo, self.tol = int(iter), int(eval_elbo), float(tol_rel_obj)
        self.cap = int(max(0.1 * self.iter / self.eval_elbo, 2.0))
        self.buf, self.elbo, self.flags = [], 0.0, 0
        self.delta = self.mean = self.median = math.nan

    def push(self, elbo_new, t):
        prev, self.elbo = self.elbo, float(elbo_new)
        with np.errstate(all="ignore"):
            self.delta = float(np.abs((np.float64(self.elbo) - np.float64(prev)) / np.float64(self.elbo)))
        self.buf.append(self.delta)
        self.buf = self.buf[-self.cap:]
        s = 0.0
        for d in self.buf:
            s += d
        n = len(self.buf)
        self.mean = s / n
        self.median = s if s != s else sorted(self.buf)[n // 2]
        if t > 10 * self.eval_elbo and (self.mean > 0.5 or self.median > 0.5):
            self.flags |= FLAG_DIVERGING
        if self.mean < self.tol:
            return MEAN_CONVERGED
        if self.median < self.tol:
            return MEDIAN_CONVERGED
        return MAXIT if t >= self.iter else 0


def run(log_prob_grad, mu0, normals, iter=10000, grad_samples=1, elbo_samples=100, eta=1.0, adapt_engaged=True, adapt_iter=50, tol_rel_obj=0.01,
        eval_elbo=100, elbo_offset=0.0):
    """The whole algorithm of one run from mu0 (omega_0 = 0).  dict(code, flags, iterations, eta_index, eta, mu, omega, elbo [iter // eval_elbo + 1]
    (NaN behind the end), adapt_elbo [5], deltas, means, medians: what the buffer held after every evaluation)."""
    mu0 = np.array(mu0, dtype=np.float64)
    om0 = np.zeros(mu0.size)
    trace = np.full(iter // eval_elbo + 1, np.nan)
    out = dict(code=0, flags=0, iterations=0, eta_index=-1, eta=float(eta), mu=mu0, omega=om0, elbo=trace, adapt_elbo=np.full(5, np.nan),
               deltas=[], means=[], medians=[])
    trace[0] = elbo(log_prob_grad, mu0, om0, normals, 0, 0, elbo_samples, elbo_offset)
    if not math.isfinite(trace[0]):
        out["code"] = INIT
        return out
    if adapt_engaged:
        for k, e in enumerate(ETAS):
            r = sga(log_prob_grad, mu0, om0, e, adapt_iter, normals, stage=1 + k, grad_samples=grad_samples)
            out["adapt_elbo"][k] = -math.inf if r["code"] else elbo(log_prob_grad, r["mu"], r["omega"], normals, 1 + k, r["t"], elbo_samples, elbo_offset)
        out["eta_index"], _ = pick_eta(trace[0], out["adapt_elbo"])
        if out["eta_index"] < 0:
            out["code"] = ADAPT_FAILED
            return out
        out["eta"] = ETAS[out["eta_index"]]
    conv = Conv(iter, eval_elbo, tol_rel_obj)
    st = dict(mu=mu0, omega=om0, s=None, t=0)
    while not out["code"]:
        seg = min(eval_elbo, iter - st["t"])
        st = sga(log_prob_grad, st["mu"], st["omega"], out["eta"], seg, normals, stage=0, grad_samples=grad_samples, t0=st["t"], s=st["s"])
        if st["code"]:
            out["code"] = NONFINITE
        elif st["t"] % eval_elbo == 0:
            e = elbo(log_prob_grad, st["mu"], st["omega"], normals, 0, st["t"], elbo_samples, elbo_offset)
            trace[st["t"] // eval_elbo] = e
            out["code"] = conv.push(e, st["t"])
            out["deltas"].append(conv.delta); out["means"].append(conv.mean); out["medians"].append(conv.median)
        else:
            out["code"] = MAXIT
    out.update(mu=st["mu"], omega=st["omega"], iterations=st["t"], flags=conv.flags)
    return out
