"""CPU reference for the posterior mode (tests of potus_optimize): scipy L-BFGS on the oracle's log density with the Jacobian
removed as potus_optimize removes it, polished by Newton-CG steps whose Hessian-vector products are central differences of the
oracle gradient; and the smallest eigenvalue of minus the Hessian there, from central differences (small designs only)."""
from __future__ import annotations

import functools

import numpy as np

from oracle_lib import OracleModel
from us_potus_model_amd import _abi

LOG_002 = float(np.log(0.02))


def rho_index(data, variant):
    """Position of the rho_e_bias coordinate in the unconstrained vector (None for the no-mode variant): the only coordinate
    with a Jacobian whose gradient is not constant."""
    if variant != "full":
        return None
    layout, _ = _abi.column_layout(data, variant)
    return layout["rho_e_bias"][0] - _abi.N_SAMPLER_COLS


def remove_jacobian(lp, g, q, irho):
    """(lp, g) of log_prob<jacobian = true> -> those of log_prob<jacobian = false> (stan:62-63: mu_e_bias = 0.02 raw, rho = inv_logit(raw))."""
    if irho is None:
        return lp, g
    x = q[irho]
    rho = 1.0 / (1.0 + np.exp(-x)) if x >= 0 else np.exp(x) / (1.0 + np.exp(x))
    g = g.copy()
    g[irho] -= 1.0 - 2.0 * rho
    return lp - (LOG_002 + np.log(rho) + np.log1p(-rho)), g


class Objective:
    """log density and gradient of one design on the CPU oracle, with or without the Jacobian."""

    def __init__(self, data, variant, jacobian=False):
        self.m = OracleModel(data, variant)
        self.D = self.m.D
        self.irho = rho_index(data, variant)
        self.jacobian = bool(jacobian)

    def __call__(self, q):
        q = np.ascontiguousarray(q, dtype=np.float64)
        lp, g = self.m.log_prob_grad(q)
        return (lp, g) if self.jacobian else remove_jacobian(lp, g, q, self.irho)

    def neg(self, q):
        lp, g = self(q)
        return -lp, -g

    def grad(self, q):
        return self(q)[1]

    def hess_vec(self, q, v, h=1e-5):
        """(-Hessian) v by central differences of the gradient along v (relative step h)."""
        nv = np.linalg.norm(v)
        if nv == 0:
            return np.zeros_like(v)
        e = h * max(1.0, np.linalg.norm(q)) / nv
        return -(self.grad(q + e * v) - self.grad(q - e * v)) / (2 * e)


def scipy_lbfgs(obj, q0, history=5, maxiter=20000):
    from scipy.optimize import minimize
    r = minimize(obj.neg, np.asarray(q0, dtype=np.float64), jac=True, method="L-BFGS-B",
                 options=dict(maxcor=history, maxiter=maxiter, maxfun=4 * maxiter, ftol=0.0, gtol=0.0))
    return r.x, int(r.nit), int(r.nfev)


def newton_polish(obj, q, steps=3, cg_tol=1e-13, cg_max=400):
    """Newton steps on the gradient equation, each solved by conjugate gradients on finite-difference products with -Hessian (positive definite)."""
    q = np.array(q, dtype=np.float64)
    for _ in range(steps):
        g = obj.grad(q)
        x, r = np.zeros_like(g), g.copy()
        p, rr = r.copy(), float(r @ r)
        r0 = np.sqrt(rr)
        for _ in range(cg_max):
            if np.sqrt(rr) <= cg_tol * max(r0, 1e-300):
                break
            Ap = obj.hess_vec(q, p)
            a = rr / float(p @ Ap)
            x += a * p
            r -= a * Ap
            rr2 = float(r @ r)
            p = r + (rr2 / rr) * p
            rr = rr2
        cand = q + x
        if np.linalg.norm(obj.grad(cand)) >= np.linalg.norm(g):
            break                                           # at the rounding floor of the gradient: keep the better point
        q = cand
    return q


def reference_mode(obj, q0=None, history=5, polish=3):
    """(q, ||g||_2 at q, L-BFGS iterations, gradient evaluations)."""
    q0 = np.zeros(obj.D) if q0 is None else q0
    q, nit, nfev = scipy_lbfgs(obj, q0, history)
    if polish:
        q = newton_polish(obj, q, polish)
    return q, float(np.linalg.norm(obj.grad(q))), nit, nfev


def lambda_min(obj, q, h=1e-5):
    """Smallest eigenvalue of -Hessian at q: dense central differences of the gradient, symmetrised (D of a few hundred)."""
    D = obj.D
    H = np.zeros((D, D))
    for i in range(D):
        e = np.zeros(D)
        e[i] = h
        H[:, i] = -(obj.grad(q + e) - obj.grad(q - e)) / (2 * h)
    return float(np.linalg.eigvalsh(0.5 * (H + H.T))[0])


@functools.lru_cache(maxsize=None)
def small_reference(variant, jacobian):
    """The shared reference of the small synthetic design: computed once per (variant, Jacobian setting), treated as read-only."""
    from us_potus_model_amd import synthetic
    data = synthetic.small(variant)
    obj = Objective(data, variant, jacobian)
    q, gn, nit, nfev = reference_mode(obj)
    q.setflags(write=False)
    return dict(data=data, obj=obj, q=q, gnorm=gn, lambda_min=lambda_min(obj, q), iterations=nit, grad_evals=nfev)
