"""numpy restatement of the three distances between two samples of one column (include/potus_hmc.h, potus_ecdf_distance_device), written
from the definitions there and sharing nothing with the kernel:

  x_1 < ... < x_m the distinct values of the union, P_j = #{a <= x_j} / n_a, Q_j likewise, Delta_j = x_{j+1} - x_j (j < m);
  w1 = sum Delta_j |P_j - Q_j|;  ks = max_j |P_j - Q_j|;  cjs = max(c(a, b), c(-a, -b)),
  c = sqrt(max(0, C(P||Q) + C(Q||P)) / sum Delta_j (P_j + Q_j)),
  C(P||Q) = sum Delta_j P_j log2(P_j / ((P_j + Q_j) / 2)) + (1 / (2 ln 2)) sum Delta_j (Q_j - P_j), 0 log 0 = 0, c = 0 when m = 1.
"""
import numpy as np


def ecdfs(a, b):
    """(x [m], P [m], Q [m]) of two finite samples."""
    a, b = np.sort(np.asarray(a, dtype=np.float64)), np.sort(np.asarray(b, dtype=np.float64))
    x = np.unique(np.concatenate([a, b]))
    P = np.searchsorted(a, x, side="right") / a.size
    Q = np.searchsorted(b, x, side="right") / b.size
    return x, P, Q


def _c_one_sided(delta, P, Q):
    """C(P||Q) over the gaps."""
    M = 0.5 * (P + Q)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(P > 0, P * np.log2(np.where(P > 0, P, 1.0) / np.where(M > 0, M, 1.0)), 0.0)
    return float(np.sum(delta * t) + np.sum(delta * (Q - P)) / (2.0 * np.log(2.0)))


def cjs2_oriented(a, b):
    """c(a, b) squared (the square root near 0 magnifies rounding: compare squares)."""
    x, P, Q = ecdfs(a, b)
    if x.size == 1:
        return 0.0
    delta = np.diff(x)
    P, Q = P[:-1], Q[:-1]
    den = float(np.sum(delta * (P + Q)))
    return max(0.0, _c_one_sided(delta, P, Q) + _c_one_sided(delta, Q, P)) / den


def distance(a, b):
    """(w1, ks, cjs^2) of two samples; NaN, NaN, NaN when either holds a non-finite value."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return np.nan, np.nan, np.nan
    x, P, Q = ecdfs(a, b)
    w1 = float(np.sum(np.diff(x) * np.abs(P - Q)[:-1]))
    ks = float(np.max(np.abs(P - Q)))
    return w1, ks, max(cjs2_oriented(a, b), cjs2_oriented(-a, -b))


def distance_columns(a, b):
    """[n_cols, 3] = (w1, ks, cjs^2) of the columns of a [n_a, n_cols] and b [n_b, n_cols]."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array([distance(a[:, j], b[:, j]) for j in range(a.shape[1])])
