"""CPU reference for the Laplace approximation (tests of potus_laplace): minus the Hessian of the log density at the shared mode of
tests/optimize_ref.small_reference by torch autograd on the literal Stan transcription, the oracle's own central-difference matrix with
potus_laplace's step rule (its truncation error is the yardstick of the device's), and the library's normals restated with the oracle's Philox."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch

import optimize_ref
import stan_transcription
from oracle_lib import lib as oracle_lib

RNG_LAPLACE = 8


def precision_autograd(data, variant, jacobian, q):
    """P_ref = -(H + H') / 2, H the autograd Hessian of log_prob<jacobian> at q (jacobian = False: optimize_ref.remove_jacobian's term inside)."""
    irho = optimize_ref.rho_index(data, variant)

    def f(x):
        lp = stan_transcription.log_prob(data, x, variant)[0]
        if not jacobian and irho is not None:
            rho = torch.sigmoid(x[irho])
            lp = lp - (optimize_ref.LOG_002 + torch.log(rho) + torch.log1p(-rho))
        return lp
    H = torch.autograd.functional.hessian(f, torch.tensor(np.array(q, dtype=np.float64))).numpy()
    return -0.5 * (H + H.T)


def precision_fd(obj, q, h):
    """The oracle's central-difference matrix with potus_laplace's rule: h_j = h max(1, |q_j|), row j = -(g+ - g-) / (x+ - x-), symmetrised."""
    D = obj.D
    H = np.zeros((D, D))
    for j in range(D):
        hj = h * max(1.0, abs(q[j]))
        xp, xm = np.array(q, dtype=np.float64), np.array(q, dtype=np.float64)
        xp[j], xm[j] = q[j] + hj, q[j] - hj
        H[j] = -(obj.grad(xp) - obj.grad(xm)) / (xp[j] - xm[j])
    return 0.5 * (H + H.T)


@functools.lru_cache(maxsize=None)
def small_precision(variant, jacobian):
    """The shared reference at the read-only mode of optimize_ref.small_reference: computed once, treated as read-only."""
    r = optimize_ref.small_reference(variant, jacobian)
    P = precision_autograd(r["data"], variant, jacobian, r["q"])
    P.setflags(write=False)
    return dict(data=r["data"], obj=r["obj"], q=r["q"], P=P)


@functools.lru_cache(maxsize=None)
def small_precision_fd(variant, jacobian, h):
    r = small_precision(variant, jacobian)
    P = precision_fd(r["obj"], r["q"], h)
    P.setflags(write=False)
    return P


def library_normals(seed, draw, D):
    """u of library draw `draw` (draw_offset + n): coordinates 2 i, 2 i + 1 are the Box-Muller pair of counter {i, 8, 0, draw + 1}, key = seed."""
    L = oracle_lib()
    a, b = C.c_double(), C.c_double()
    out = np.zeros(2 * ((D + 1) // 2))
    for i in range((D + 1) // 2):
        L.oracle_rng_normal_pair(int(seed), draw + 1, 0, RNG_LAPLACE, 0, i, C.byref(a), C.byref(b))
        out[2 * i], out[2 * i + 1] = a.value, b.value
    return out[:D]


def log_ratio(obj_jac, q_mode, P, u):
    """x = q^ + L^-T u with P = L L' (numpy / scipy), and lp(x) - lp(q^) + |u|^2 / 2 under the oracle's log_prob<jacobian = true>."""
    from scipy.linalg import solve_triangular
    L = np.linalg.cholesky(P)
    X = solve_triangular(L.T, np.asarray(u).T, lower=False).T
    lp0 = obj_jac.m.log_prob_grad(np.ascontiguousarray(q_mode))[0]
    lp = np.array([obj_jac.m.log_prob_grad(np.ascontiguousarray(q_mode + x))[0] for x in X])
    return lp - lp0 + 0.5 * (np.asarray(u) ** 2).sum(1), X
