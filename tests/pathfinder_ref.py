"""CPU reference for Pathfinder (tests of potus_pathfinder / potus_pathfinder_path), numpy written from the formulas of Zhang, Carpenter,
Gelman and Vehtari (2022) as include/potus_hmc.h states them.

dense():    the DENSE form.  Sigma_l is built as a D x D matrix, mu = x + Sigma g, log det comes from slogdet and log q is the
            multivariate-normal density of phi (a solve with Sigma).  A draw is phi = mu + A u with a D x D matrix A, A A' = Sigma; of the many
            square roots the formulas fix A = diag(alpha^1/2)(I + Q (L~ - I) Q'), and dense_draw builds it from Sigma itself:
            L~ = chol(Q' C Q) with C = diag(alpha^-1/2) Sigma diag(alpha^-1/2) and Q an orthonormal basis of its low-rank part.
low_rank(): the second form: thin QR, L~ = chol(I + R~ gamma R~'), phi and log q without any D x D matrix, with numpy's Householder QR.
The spread between the two on a trajectory is the reference's own error e_ref (tests/test_pathfinder_host.py, test_gpu_pathfinder.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

RNG_PATHFINDER = 9
LOG_2PI = float(np.log(2.0 * np.pi))


def alphas(x, g):
    """alpha_l, l = 0 .. L, the kept flags and (a, b, c) per pair along the path x, g [L + 1, D]."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    L, D = x.shape[0] - 1, x.shape[1]
    al = np.ones((L + 1, D))
    kept = np.zeros(L + 1, dtype=bool)
    abc = np.full((L + 1, 3), np.nan)
    for l in range(1, L + 1):
        s, z, a0 = x[l] - x[l - 1], g[l - 1] - g[l], al[l - 1]
        with np.errstate(all="ignore"):
            a, b, c = float(z @ (a0 * z)), float(z @ s), float(s @ (s / a0))
            abc[l] = a, b, c
            kept[l] = b > 0 and float(z @ z) <= 1e12 * b
            al[l] = 1.0 / (a / (b * a0) + z * z / b - a * s * s / (b * c * a0 * a0)) if kept[l] else a0
    return al, kept, abc


def history(kept, l, J):
    """The pairs of the history at iterate l: the last min(J, kept so far) kept ones up to l, oldest first."""
    return [int(i) for i in np.flatnonzero(kept[:l + 1])[-J:]]


def _beta_gamma(x, g, al, hist):
    S = np.stack([x[i] - x[i - 1] for i in hist], 1)
    Z = np.stack([g[i - 1] - g[i] for i in hist], 1)
    j = len(hist)
    StZ = S.T @ Z
    R, E = np.triu(StZ), np.diag(np.diag(StZ))
    Ri = np.linalg.inv(R)
    beta = np.concatenate([al[:, None] * Z, S], 1)
    gamma = np.zeros((2 * j, 2 * j))
    gamma[:j, j:] = -Ri
    gamma[j:, :j] = -Ri.T
    gamma[j:, j:] = Ri.T @ (E + Z.T @ (al[:, None] * Z)) @ Ri
    return beta, gamma, S, Z


def dense(x, g, l, J, u=None, al_kept=None):
    """Iterate l in the dense form: dict(alpha, hist, Sigma, mu, log_det and, with u [n, D], phi, lq)."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    al_all, kept, _ = al_kept if al_kept is not None else alphas(x, g)
    al, hist, D = al_all[l], history(kept, l, J), x.shape[1]
    Sigma = np.diag(al)
    if hist:
        beta, gamma, _, _ = _beta_gamma(x, g, al, hist)
        Sigma = Sigma + beta @ gamma @ beta.T
    Sigma = 0.5 * (Sigma + Sigma.T)
    mu = x[l] + Sigma @ g[l]
    sign, log_det = np.linalg.slogdet(Sigma)
    out = dict(alpha=al, hist=hist, Sigma=Sigma, mu=mu, log_det=float(log_det) if sign > 0 else np.nan)
    if u is not None:
        phi = dense_draw(al, Sigma, hist, x, g, mu, np.atleast_2d(u))
        d = phi - mu
        out["phi"] = phi
        out["lq"] = -0.5 * (log_det + np.einsum("ni,ni->n", d, np.linalg.solve(Sigma, d.T).T) + D * LOG_2PI)
    return out


def dense_draw(al, Sigma, hist, x, g, mu, u):
    """phi = mu + A u with the D x D matrix A = diag(alpha^1/2) (I + Q (L~ - I) Q'), Q and L~ from the dense
    C = diag(alpha^-1/2) Sigma diag(alpha^-1/2) = I + W gamma W': Q spans W's columns (SVD, dense), L~ = chol(Q' C Q)."""
    D = al.size
    if not hist:
        return mu + np.sqrt(al) * u
    beta, gamma, _, _ = _beta_gamma(x, g, al, hist)
    Wm = beta / np.sqrt(al)[:, None]
    Q, Rt = np.linalg.qr(Wm)
    sgn = np.sign(np.diag(Rt))
    sgn[sgn == 0] = 1.0
    Q = Q * sgn                                                   # the QR with a positive diagonal, as Gram-Schmidt gives it
    Cm = Sigma / np.sqrt(al)[:, None] / np.sqrt(al)[None, :]
    Lt = np.linalg.cholesky(Q.T @ Cm @ Q)
    A = np.sqrt(al)[:, None] * (np.eye(D) + Q @ (Lt - np.eye(Lt.shape[0])) @ Q.T)
    return mu + u @ A.T


def low_rank(x, g, l, J, u=None, al_kept=None):
    """Iterate l without a D x D matrix: dict(alpha, hist, mu, log_det and, with u [n, D], phi, lq)."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    al_all, kept, _ = al_kept if al_kept is not None else alphas(x, g)
    al, hist, D = al_all[l], history(kept, l, J), x.shape[1]
    ra = np.sqrt(al)
    if hist:
        beta, gamma, _, _ = _beta_gamma(x, g, al, hist)
        mu = x[l] + al * g[l] + beta @ (gamma @ (beta.T @ g[l]))
        Q, Rt = np.linalg.qr(beta / ra[:, None])
        sgn = np.sign(np.diag(Rt))
        sgn[sgn == 0] = 1.0
        Q, Rt = Q * sgn, Rt * sgn[:, None]
        Mm = np.eye(Rt.shape[0]) + Rt @ gamma @ Rt.T
        try:
            Lt = np.linalg.cholesky(0.5 * (Mm + Mm.T))
        except np.linalg.LinAlgError:
            return dict(alpha=al, hist=hist, mu=mu, log_det=np.nan)
        log_det = float(np.log(al).sum() + 2.0 * np.log(np.diag(Lt)).sum())
    else:
        mu, log_det, Q, Lt = x[l] + al * g[l], float(np.log(al).sum()), None, None
    out = dict(alpha=al, hist=hist, mu=mu, log_det=log_det, Q=Q, Lt=Lt)
    if u is not None:
        u = np.atleast_2d(u)
        w = u if Q is None else u + (u @ Q) @ (Lt - np.eye(Lt.shape[0])).T @ Q.T
        out["phi"] = mu + ra * w
        out["lq"] = -0.5 * (log_det + (u * u).sum(1) + D * LOG_2PI)
    return out


def phi_rounding(r, u, depth, eps=2.0 ** -52):
    """First-order bound on what rounding can move phi = mu + alpha^1/2 (u + Q (L~ - I) Q'u) by, for r = low_rank(...), when each of the 2 j sums
    Q'u of D terms passes through `depth` additions: |d(Q'u)_m| <= depth eps sum_i |Q_im u_i|, carried through |L~ - I| and |Q|, plus
    (2 j + 4) eps for the 2 j + 3 terms of an entry itself.  [n] -> the largest over entries and draws."""
    u = np.atleast_2d(u)
    own = (2 * len(r["hist"]) + 4) * eps * np.abs(r["phi"]).max()
    if r["Q"] is None:
        return own
    T = np.abs(r["Lt"] - np.eye(r["Lt"].shape[0]))
    dc = depth * eps * (np.abs(u) @ np.abs(r["Q"]))
    return float((np.sqrt(r["alpha"]) * ((dc @ T.T) @ np.abs(r["Q"]).T)).max()) + own


def elbo(form, log_p, x, g, J, u):
    """ELBO_l, l = 1 .. L (entry 0 NaN), of `form` (dense or low_rank) with u [L, K, D] and log_p(phi) -> float; -inf where any log p is not finite."""
    L = np.asarray(x).shape[0] - 1
    ak = alphas(x, g)
    out = np.full(L + 1, np.nan)
    for l in range(1, L + 1):
        r = form(x, g, l, J, u=u[l - 1], al_kept=ak)
        if "phi" not in r:
            out[l] = -np.inf
            continue
        lp = np.array([log_p(p) for p in r["phi"]])
        out[l] = np.mean(lp - r["lq"]) if np.isfinite(lp).all() else -np.inf
    return out


def best(e):
    """l* = argmax over the finite ELBOs, the lowest l on ties; 0: none."""
    e = np.where(np.isfinite(e), e, -np.inf)
    e[0] = -np.inf
    return int(np.argmax(e)) if np.isfinite(e).any() else 0


def library_normals(seed, path, D, l=None, k=None, draw=None):
    """The library's u restated with the oracle's Philox: ELBO draw k of iterate l of path `path` (path_offset + p) is the Box-Muller pairs of
    counter {i, 9 | k << 8, l, path + 1}; final draw `draw` (draw_offset + n) those of {i, 9 | 0xFF << 8, draw + 1, path + 1}; key = seed."""
    from oracle_lib import lib as oracle_lib
    Lo = oracle_lib()
    a, b = C.c_double(), C.c_double()
    it, aux = (int(l), int(k)) if draw is None else (int(draw) + 1, 0xFF)
    out = np.zeros(2 * ((D + 1) // 2))
    for i in range((D + 1) // 2):
        Lo.oracle_rng_normal_pair(int(seed), path + 1, it, RNG_PATHFINDER, aux, i, C.byref(a), C.byref(b))
        out[2 * i], out[2 * i + 1] = a.value, b.value
    return out[:D]


def quadratic_path(rng, D, L, cond=100.0, reject=None, repeat=None):
    """A path on the strongly concave quadratic log p = -1/2 (x - m)' H (x - m): steepest ascent steps with exact line search from a random
    start.  reject: a pair index whose gradient row is replaced so that s'z < 0; repeat: an index whose point repeats the one before."""
    A = rng.standard_normal((D, D))
    Qm, _ = np.linalg.qr(A)
    H = (Qm * np.geomspace(1.0, cond, D)) @ Qm.T
    H = 0.5 * (H + H.T)
    m = rng.standard_normal(D)
    x = np.zeros((L + 1, D))
    x[0] = m + 3.0 * rng.standard_normal(D)
    for l in range(1, L + 1):
        gr = -H @ (x[l - 1] - m)
        d = gr + 0.3 * np.linalg.norm(gr) * rng.standard_normal(D) / np.sqrt(D)     # (not the exact gradient: the pairs stay independent)
        t = (gr @ d) / (d @ H @ d)
        x[l] = x[l - 1] if repeat == l else x[l - 1] + 0.7 * t * d
    g = -(x - m) @ H
    if reject is not None:
        g[reject] = g[reject - 1] + (g[reject - 1] - g[reject])                      # z -> -z for pair `reject` (and changes pair reject + 1)
    return dict(x=x, g=g, H=H, m=m, log_p=lambda p: float(-0.5 * (p - m) @ H @ (p - m)))
