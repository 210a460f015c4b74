"""Inputs at the edges of the sorted runs (DG_RUN = 8192 pairs in potus_diag.hpp, PS_RUN = 16384 doubles in potus_summary.hpp), shared by
tests/test_gpu_sorted_runs.py (the kernels against the restatements) and tests/test_sorted_runs_host.py (the restatements against numpy
and scipy).  Every builder is seeded by its shape, cached, and hands out read-only arrays."""
import functools

import numpy as np
from scipy.signal import lfilter

DG_RUN, PS_RUN = 8192, 16384
MONITOR_PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)
# (draws per chain n, chains C): N = 2 C (n // 2) split draws, M = C n draws
COLUMN_SHAPES = ((1024, 8),    # N = M = 8192: exactly one full run, sorted and read in LDS
                 (8190, 1),    # two padding slots in a full-size sort
                 (8191, 1),    # N = 8190, M = 8191: odd n just below the edge
                 (8193, 1),    # N = 8192 stays in LDS, M = 8193 has a last run of ONE element
                 (2049, 4),    # N = 8192, M = 8196: the monitor's mixed case, a last run of four
                 (8194, 1),    # N = M = 8194: a last run of two
                 (2048, 8))    # N = M = 16384: two full runs, no partial one
PSIS_SHAPES = ((8, 1024), (3, 2731), (2, 4097), (8, 2048))   # (chains, draws): S = 8192, 8193, 8194, 16384
COLUMNS = ("ar1 -0.5", "ar1 0.3", "ar1 0.95", "rounded", "minus zero", "wide range")
ROUNDED, MINUS_ZERO, WIDE = 3, 4, 5
WIDE_SLOTS = (2, 4, 5, 6, 8, 9, 10, 11, 12)   # of the monitor's row for the wide-range column: mad, R-hat, bulk ESS, tail ESS, the quantiles
# more work items than workgroups: the grid of every sorted-run kernel is capped at 1024
MANY_DRAWS, MANY_CHAINS, GRID_CAP, N_EARLY = 64, 2, 1024, 76
N_MANY = GRID_CAP + N_EARLY
OTHERS = tuple(int(v) for v in np.linspace(N_EARLY, GRID_CAP - 1, 16))   # ordinary items no early exit comes before or after


def _ar1(rng, n, C, rho):
    """test_gpu_monitor._ar1_block's recursion: x[0] = e[0], x[t] = rho x[t - 1] + sqrt(1 - rho^2) e[t], per chain"""
    u = np.sqrt(1.0 - rho * rho) * rng.standard_normal((n, C))
    u[0] /= np.sqrt(1.0 - rho * rho)
    return lfilter([1.0], [1.0, -rho], u, axis=0)


@functools.lru_cache(maxsize=None)
def column_block(n, C):
    """[n draws, C chains, 6 columns]: AR(1) with rho = -0.5, 0.3, 0.95; the rho = 0.3 column rounded to one decimal (hundreds of ties that
    straddle the run boundary); a column whose every 7th draw is -0.0; the first column with every 11th draw times 1e-310 (subnormal) and
    every 13th times 1e100 (the first and the last steps of the 64-bit key bisection)."""
    rng = np.random.default_rng(1000 * C + n)
    blk = np.zeros((n, C, len(COLUMNS)))
    for j, rho in enumerate((-0.5, 0.3, 0.95)):
        blk[:, :, j] = _ar1(rng, n, C, rho)
    blk[:, :, ROUNDED] = np.round(blk[:, :, 1], 1)
    blk[:, :, MINUS_ZERO] = rng.standard_normal((n, C))
    blk[::7, :, MINUS_ZERO] = -0.0
    blk[:, :, WIDE] = blk[:, :, 0]
    blk[::11, :, WIDE] *= 1e-310
    blk[::13, :, WIDE] *= 1e100
    blk.setflags(write=False)
    return blk


def chains_first(blk):
    """[draws, chains, columns] -> [chains, draws, columns]: what diagnostics.py takes column by column"""
    return np.transpose(blk, (1, 0, 2))


def _log_lik(rng, shape):
    """the generator of test_psis_branches_on_built_blocks"""
    return rng.normal(-3, 0.7, shape) + 0.3 * rng.standard_t(3, shape)


def _tie_largest_ratios(ll, share=0.3):
    """the largest `share` of the ratios -ll become one value (in place, ll of one poll)"""
    v = ll.reshape(-1)
    v[v < np.quantile(v, share)] = np.quantile(v, share)


@functools.lru_cache(maxsize=None)
def log_lik_block(chains, draws):
    """[3 polls, chains, draws] log-likelihoods; poll 1 has its largest 30 % of ratios tied, so the tail cut falls inside a tie"""
    ll = _log_lik(np.random.default_rng(chains * draws), (3, chains, draws))
    _tie_largest_ratios(ll[1])
    ll.setflags(write=False)
    return ll


GENERAL_R_EFF = (1.0, 0.6, 0.3)


@functools.lru_cache(maxsize=None)
def ratio_block(chains, draws):
    """[3 polls, chains, draws] general log ratios as test_psis_of_general_ratios_matches_the_restatement builds them: poll 1 rounded to one
    decimal (ties everywhere: which of the tied draws belong to the tail is decided by their index, across runs), poll 2 with its
    largest tenth tied"""
    rng = np.random.default_rng(chains * draws + 1)
    r = rng.normal(0, 1.5, (3, chains, draws)) + 0.5 * rng.standard_t(3, (3, chains, draws))
    r[1] = np.round(r[1], 1)
    v = r[2].reshape(-1)
    v[v > np.quantile(v, 0.9)] = np.quantile(v, 0.9)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def quantity_block(chains, draws, kind):
    """[3 polls, chains, draws] of test_gpu_eloo._quantities' continuous kind, or the same rounded to one decimal (ties in x)"""
    rng = np.random.default_rng(chains * draws + 2)
    x = rng.normal(0.3, 1.0, (3, chains, draws)) + np.arange(3)[:, None, None]
    if kind == "rounded":
        x = np.round(x, 1)
    x.setflags(write=False)
    return x


# ---- more work items than workgroups
@functools.lru_cache(maxsize=None)
def many_columns(n=MANY_DRAWS, C=MANY_CHAINS):
    """[n, C, 1100]: AR(1) columns of every rho from -0.6 to 0.95; the first 76 take the kernels' early exits in turn -- a NaN, an inf,
    a constant, a constant of +0.0 and -0.0 -- so that the workgroup that left item j early goes on to the ordinary item j + 1024."""
    rng = np.random.default_rng(n * C)
    rho = np.linspace(-0.6, 0.95, N_MANY)[rng.permutation(N_MANY)]
    e = rng.standard_normal((n, C, N_MANY))
    blk = np.zeros((n, C, N_MANY))
    blk[0] = e[0]
    for t in range(1, n):
        blk[t] = rho * blk[t - 1] + np.sqrt(1.0 - rho * rho) * e[t]
    for j in range(N_EARLY):
        kind = j % 4
        if kind == 0:
            blk[(7 * j) % n, j % C, j] = np.nan
        elif kind == 1:
            blk[(5 * j) % n, j % C, j] = np.inf if j % 8 == 1 else -np.inf
        elif kind == 2:
            blk[:, :, j] = 0.25 * j - 3.0
        else:
            blk[:, :, j] = np.where(rng.random((n, C)) < 0.5, 0.0, -0.0)
    blk.setflags(write=False)
    return blk


EARLY_RATIO_KINDS = ("nan", "plus inf", "no finite ratio", "identical", "identical +-0.0", "tied tail")


@functools.lru_cache(maxsize=None)
def many_ratios(n=MANY_DRAWS, C=MANY_CHAINS):
    """[1100 polls, C, n] raw log ratios (the log-likelihoods of the PSIS-LOO entry are their negatives): the first 76 take the early exits
    of the three PSIS kernels in turn -- a NaN, a +inf ratio, no finite ratio, identical ratios (a tail of one value: no fit), identical
    ratios of +0.0 and -0.0, and a tail tied beyond the cut."""
    rng = np.random.default_rng(n * C + 1)
    r = -_log_lik(rng, (N_MANY, C, n))
    for j in range(N_EARLY):
        kind = EARLY_RATIO_KINDS[j % len(EARLY_RATIO_KINDS)]
        if kind == "nan":
            r[j, j % C, (7 * j) % n] = np.nan
        elif kind == "plus inf":
            r[j, j % C, (5 * j) % n] = np.inf
        elif kind == "no finite ratio":
            r[j] = -np.inf
        elif kind == "identical":
            r[j] = 1.25 - 0.01 * j
        elif kind == "identical +-0.0":
            r[j] = np.where(rng.random((C, n)) < 0.5, 0.0, -0.0)
        else:
            ll = -r[j]
            _tie_largest_ratios(ll)
            r[j] = -ll
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def many_quantities(n=MANY_DRAWS, C=MANY_CHAINS):
    """[1100 polls, C, n] of x for E_loo: ordinary, except that among the first 76 every fifth is constant, every fifth (shifted) two-valued
    and every fifth (shifted again) holds a NaN -- the three ways el_plain leaves early, out of step with the six kinds of ratios"""
    rng = np.random.default_rng(n * C + 2)
    x = rng.normal(0.3, 1.0, (N_MANY, C, n))
    for j in range(N_EARLY):
        if j % 5 == 1:
            x[j] = 0.37
        elif j % 5 == 2:
            x[j] = (rng.random((C, n)) < 0.4).astype(float)
        elif j % 5 == 3:
            x[j, j % C, (3 * j) % n] = np.nan
    x.setflags(write=False)
    return x
