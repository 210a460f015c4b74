"""Sizes at the edges of the tiles and panels of the dense-metric kernels (csrc/potus_dense.hpp, csrc/potus_dense_pool.hpp) with their inputs
and high-precision references, shared by tests/test_gpu_dense_edges.py (the kernels, through the four probes of include/potus_hmc_debug.h)
and tests/test_dense_edges_host.py (the references against float64 numpy, the conditioning of every window-end case, the constants against
the headers' text).  Every builder is seeded by its shape, cached, and hands out read-only arrays."""
import functools

import numpy as np

# ---- the constants the kernels cut their work by (test_dense_edges_host.py holds them to the headers)
DN_NB = 64                                  # rows per block of the factorisation and the triangular solve; k_dn_cov reads this many draws at a time
DN_PANEL = 4                                # block columns per panel: 256 columns
DN_WT = 128                                 # tile of the wide trailing update
DN_RB, DN_RB_BIG, DN_RB_MAX = 128, 256, 512   # rows per workgroup of the per-chain product ...
RB_BIG_FROM, RB_MAX_FROM = 32 * DN_RB_BIG, 32 * DN_RB_MAX   # ... by D (dense_launch_shape): 8192 and 16 384
DN_CT = 512                                 # columns per tile of it
DNP_COLS, DNP_COLS_F32 = 256, 512           # columns per panel of the pooled product
DNP_KB, DNP_KB_TILES = 32, 16               # rows per batch: one operand tile / two or three
DNP_RMAX = 48                               # right-hand sides per pooled launch, in operand tiles of 16
PANEL = DN_NB * DN_PANEL
EPS = 2.0 ** -52
LONGDOUBLE_UP_TO = 1024                     # references in np.longdouble up to this D, float64 beyond
FORWARD_BOUND = 1e-6                        # 8 D eps kappa_2 of every window-end case stays at or below this

# ---- per-chain product: k_dn_symv + k_dn_symv_finish
# one row block and less, 128 +- 1 (two blocks), 256 +- 1, 384 +- 1 (three blocks: the middle one once), 512 +- 1 (one column tile exactly);
# 513 .. 517: a last column tile of 1 .. 5 columns -- an fp32 load carries four, so the right-edge mask cuts inside a load
SYMV_D = (1, 2, 7, 8, 9, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 514, 515, 517)
SYMV_NRHS = (1, 2, 3)
# one chain, two right-hand sides: rb 128 -> 256 (8193: a last block of one row) and 256 -> 512
SYMV_BIG_D = (RB_BIG_FROM - 1, RB_BIG_FROM, RB_BIG_FROM + 1, RB_MAX_FROM - 1, RB_MAX_FROM)
SYMV_BIG_CHAINS, SYMV_BIG_NRHS = 1, 2


def symv_chains(D, nrhs):
    """two or three chains, in turn"""
    return 2 + (D + nrhs) % 2


# ---- pooled product: k_dn_pool_mm<NT, F32> + k_dn_pool_finish
POOL_D = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1025)
POOL_RHS = ((16, 1), (17, 1), (16, 2), (11, 3), (16, 3), (17, 3), (25, 2))   # (chains, nrhs): R = 16, 17, 32, 33, 48, 51, 50
POOL_SPLIT_D = (33, 257)                    # POTUS_POOL_SPLIT = 8: the last row split has one row
POOL_SPLITS = (8, 3, 1)                     # 8: the library's own choice up to D = 16 384, stated; 3: other row counts, a ragged last split; 1: no split at all
POOL_IDLE = (17, 1)                         # the idle-companion check: chains 0 and 16 of 17 run alone

# ---- window end: k_dn_center, k_dn_cov, dense_cholesky_launch, k_dn_trsv_* (and the pooled k_dn_pool_center / _cov / _scale)
# below one block; one block +- 1; two blocks; one panel +- 1; 320 +- 1: a second panel of one block, of one block and a row; 384 +- 1: 127, 128, 129
# rows behind the first panel (one wide tile, one exactly, two); two panels +- 1; 769: a fourth panel of one row
WINDOW_D = (1, 2, 63, 64, 65, 128, 255, 256, 257, 319, 320, 321, 383, 384, 385, 511, 512, 513, 769)
WINDOW_N_DEFAULT = 40
WINDOW_N = (2, 3, 63, 64, 65, 128, 129)     # the legal minimum; the 64 draws k_dn_cov reads at a time, +- 1; twice that, + 1
WINDOW_N_D = (65, 257)
WINDOW_CHAINS = 2
POOL_WINDOW_D = (1, 2, 63, 64, 65, 255, 256, 257, 320, 321, 383, 384, 385, 512, 513, 769)   # every edge once
POOL_WINDOW_CHAINS = 3
POOL_WINDOW_N = ((65, 2), (65, 21), (65, 22), (257, 43))    # (D, n per chain): N = 6; 63 and 66 pooled draws in chains of less than 64; 129


def window_cases():
    """(D, n) of the per-chain window end"""
    return [(D, WINDOW_N_DEFAULT) for D in WINDOW_D] + [(D, n) for D in WINDOW_N_D for n in WINDOW_N]


def pool_window_cases():
    """(D, n per chain) of the pooled window end"""
    return [(D, WINDOW_N_DEFAULT // 2) for D in POOL_WINDOW_D] + list(POOL_WINDOW_N)


# ---- helpers
def round32(a):
    """to fp32 (round to nearest even) and back: what metric_storage = f32 keeps"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def ref_dtype(D):
    return np.longdouble if D <= LONGDOUBLE_UP_TO else np.float64


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- products
@functools.lru_cache(maxsize=8)
def symv_matrices(chains, D):
    """[chains, D, D] symmetric positive definite: rank 8 plus the unit diagonal, one matmul per chain"""
    rng = np.random.default_rng(100 * D + chains)
    B = rng.standard_normal((chains, D, 8))
    M = np.matmul(B, np.transpose(B, (0, 2, 1)))
    M /= 8.0
    M[:, np.arange(D), np.arange(D)] += 1.0
    return _frozen(M)


def poisoned(M):
    """the matrix as the device is handed it: NaN below the diagonal (the factor's place; the product selects, it does not multiply by zero)"""
    D = M.shape[-1]
    return np.where(np.tri(D, D, -1, dtype=bool), np.nan, M)


@functools.lru_cache(maxsize=None)
def symv_rhs(chains, nrhs, D):
    return _frozen(np.random.default_rng(7 * D + 10 * chains + nrhs).standard_normal((chains, nrhs, D)))


def symv_reference(M, x, dtype):
    """y [chains, nrhs, D] = M x and x_0 . M x_0 per chain, accumulated in dtype (M: [chains, D, D] or one [D, D] for every chain)"""
    xl = np.asarray(x, dtype=dtype)
    if M.ndim == 2:
        y = np.matmul(xl, np.asarray(M, dtype=dtype).T)
    else:
        y = np.stack([np.matmul(xl[c], np.asarray(M[c], dtype=dtype).T) for c in range(M.shape[0])])
    return y, (xl[:, 0] * y[:, 0]).sum(axis=1)


@functools.lru_cache(maxsize=None)
def symv_case(D, nrhs, f32):
    """-> (x, y_ref, dot_ref) of the small per-chain sizes for symv_matrices(symv_chains(D, nrhs), D); f32: the reference uses the rounded matrix"""
    chains = symv_chains(D, nrhs)
    M, x = symv_matrices(chains, D), symv_rhs(chains, nrhs, D)
    y, dot = symv_reference(round32(M) if f32 else M, x, ref_dtype(D))
    return (x,) + _frozen(y, dot)


@functools.lru_cache(maxsize=1)
def big_symv_matrix(D):
    """[1, D, D] of the sizes where the row-block size changes (2 GB at D = 16 384: one at a time)"""
    return symv_matrices.__wrapped__(SYMV_BIG_CHAINS, D)


@functools.lru_cache(maxsize=None)
def pool_matrix(D):
    return symv_matrices.__wrapped__(1, D)[0]


@functools.lru_cache(maxsize=None)
def pool_case(D, chains, nrhs, f32):
    """-> (x, y_ref, dot_ref) for pool_matrix(D)"""
    M, x = pool_matrix(D), symv_rhs(chains, nrhs, D)
    y, dot = symv_reference(round32(M) if f32 else M, x, ref_dtype(D))
    return (x,) + _frozen(y, dot)


# ---- window end
def draw_scale(D):
    """With fewer draws than dimensions the regulariser 1e-3 * 5 / (n + 5) is the smallest eigenvalue and the largest grows like scale^2 * D / 5e-3:
    the draws shrink with D so that 8 D eps kappa_2 stays under FORWARD_BOUND (test_dense_edges_host.py checks every case)."""
    return 1.0 if D <= 128 else 0.5 if D <= 400 else 0.25


@functools.lru_cache(maxsize=None)
def window_draws(chains, n, D):
    """[chains, n, D] draws, every chain its own: per-coordinate scales over a factor of three, a location of order one that the centring has to
    take out, and a small offset per chain (the pooled estimate sees it as variance); u [chains, D]"""
    rng = np.random.default_rng(1000 * D + 10 * n + chains)
    s = draw_scale(D) * rng.uniform(0.4, 1.2, (1, 1, D))
    draws = rng.standard_normal((chains, n, D)) * s + rng.standard_normal((1, 1, D)) + 0.5 * s * rng.standard_normal((chains, 1, D))
    return _frozen(draws, rng.standard_normal((chains, D)))


def learn_covariance(x, dtype=np.float64):
    """covar_adaptation::learn_covariance of the draws x [n, D]: n / (n + 5) * cov + 1e-3 * 5 / (n + 5) * I, accumulated in dtype"""
    xl = np.asarray(x, dtype=dtype)
    n, D = xl.shape
    c = xl - xl.sum(axis=0) / dtype(n)
    S = np.matmul(c.T, c)
    return (dtype(n) / dtype(n + 5)) * (S / dtype(n - 1)) + dtype(1e-3) * (dtype(5) / dtype(n + 5)) * np.eye(D, dtype=dtype)


@functools.lru_cache(maxsize=None)
def window_reference(chains, n, D, pooled):
    """the regularised covariance as float64, rounded once from ref_dtype(D): [chains, D, D], or one [D, D] over the chains x n pooled draws"""
    draws, _ = window_draws(chains, n, D)
    dt = ref_dtype(D)
    if pooled:
        return _frozen(np.asarray(learn_covariance(draws.reshape(chains * n, D), dt), dtype=np.float64))
    return _frozen(np.stack([np.asarray(learn_covariance(draws[c], dt), dtype=np.float64) for c in range(chains)]))


def forward_bound(M):
    """8 D eps kappa_2(M): the relative forward error allowed to a backward-stable Cholesky factor and triangular solve (tests/test_gpu_laplace.py, check_draws)"""
    ev = np.linalg.eigvalsh(M)
    return 8.0 * M.shape[0] * EPS * (ev[-1] / ev[0]), ev
