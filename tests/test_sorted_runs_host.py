"""The restatements the sorted-run kernels are held to (us_potus_model_amd/diagnostics.py, tests/psis_ref.py) against code the project
did not write -- scipy's rankdata and norm.ppf, numpy's quantile and median, a lag-by-lag autocovariance, loo's tail rule written out --
on the inputs of tests/test_gpu_sorted_runs.py (tests/sorted_run_cases.py): the shapes at the edges of the LDS runs, the tied, the -0.0 and
the wide-range column.  No GPU."""
import numpy as np
import pytest
from scipy import special, stats

import psis_ref
import sorted_run_cases as cases
from us_potus_model_amd import diagnostics as dg

HARD_COLUMNS = (cases.ROUNDED, cases.MINUS_ZERO, cases.WIDE)


def _columns(n, C):
    x = cases.chains_first(cases.column_block(n, C))
    return [(cases.COLUMNS[j], x[:, :, j]) for j in HARD_COLUMNS]


@pytest.mark.parametrize("n,C", cases.COLUMN_SHAPES)
def test_rank_normalisation_is_scipys_ordinal_ranks_through_the_normal_quantile(n, C):
    """ranks: ties in the order of the split array, -0.0 tied with 0.0; z = Phi^-1((r - 3/8) / (N + 1/4)), for the bulk and the folded draws"""
    for name, x in _columns(n, C):
        xs = dg._split(x)
        N = xs.size
        assert N == 2 * C * (n // 2)
        for what, v in (("bulk", xs), ("folded", np.abs(xs - np.median(xs)))):
            z = dg._rank_normalise(v)
            r = stats.rankdata(v.reshape(-1), method="ordinal")
            assert np.array_equal(np.rint(special.ndtr(z.reshape(-1)) * (N + 0.25) + 0.375), r), (name, what)
            assert np.allclose(z.reshape(-1), stats.norm.ppf((r - 0.375) / (N + 0.25)), rtol=1e-14, atol=0), (name, what)
        if name == "rounded" and N > cases.DG_RUN:                       # the draws of the later runs are tied with draws of the first
            flat = xs.reshape(-1)
            assert np.isin(flat[cases.DG_RUN:], flat[:cases.DG_RUN]).mean() > 0.99 and np.unique(flat).size < 100


@pytest.mark.parametrize("n,C", cases.COLUMN_SHAPES)
def test_quantiles_and_median_are_numpys(n, C):
    """(the median of the wide-range column is subnormal, where doubles are 2^-1074 apart whatever their size: two roundings of the
    interpolation there may differ by that spacing each)"""
    tiny = 2 * 2.0 ** -1074
    for name, x in _columns(n, C):
        for p in cases.MONITOR_PROBS + (0.05, 0.95):
            assert np.isclose(dg.quantile7(x, p), np.quantile(x, p), rtol=1e-14, atol=tiny), (name, p)
            assert np.array_equal(x <= dg.quantile7(x, p), x <= np.quantile(x, p)), (name, p)       # the indicator of ess_tail
        assert dg.quantile7(x, 0.0) == x.min() and dg.quantile7(x, 1.0) == x.max()
        s = np.sort(x.reshape(-1))
        M = s.size
        assert 0.5 * (s[(M - 1) // 2] + s[M // 2]) == np.median(x), name                            # the form the kernels state
        assert np.isclose(dg.quantile7(x, 0.5), np.median(x), rtol=1e-15, atol=tiny), name
        assert np.isclose(dg.mad(x), 1.4826 * np.median(np.abs(x - np.median(x))), rtol=1e-15, atol=0), name


@pytest.mark.parametrize("n,C", [(2049, 4), (8194, 1)])
def test_fft_autocovariance_is_the_lag_by_lag_sum(n, C):
    """the autocovariances ess_bulk reads (normal scores of the split draws of the rho = 0.95 column): the first 64 lags"""
    z = dg._rank_normalise(dg._split(cases.chains_first(cases.column_block(n, C))[:, :, 2]))
    h = z.shape[1]
    zc = z - z.mean(axis=1, keepdims=True)
    direct = np.array([[np.dot(zc[c, :h - t], zc[c, t:]) / h for t in range(64)] for c in range(z.shape[0])])
    ac = dg._autocov(z)[:, :64]
    err = np.abs(ac - direct).max() / direct[:, 0].max()
    print(f"n = {n}, C = {C}: largest |FFT - direct| / acov(0) = {err:.2e}")
    assert err <= 1e-13


@pytest.mark.parametrize("n,C", cases.COLUMN_SHAPES)
def test_the_restatement_is_finite_wherever_the_device_is_held_to_it(n, C):
    """diagnostics.monitor_row on the six columns: every slot of the five ordinary columns, and the slots compared for the wide-range column
    (its mean, sd, MCSE and mean ESS are left out: the FFT autocovariance of draws spread over 400 decades has no relative accuracy)"""
    x = cases.chains_first(cases.column_block(n, C))
    ref = np.array([dg.monitor_row(x[:, :, j], cases.MONITOR_PROBS) for j in range(x.shape[2])])
    assert ref.shape == (6, 13)
    assert np.isfinite(np.delete(ref, cases.WIDE, axis=0)).all()
    assert np.isfinite(ref[cases.WIDE, list(cases.WIDE_SLOTS)]).all()
    assert np.isfinite([dg.rhat(x[:, :, j]) for j in range(6)]).all() and np.isfinite([dg.ess_bulk(x[:, :, j]) for j in range(6)]).all()
    w = np.abs(x[:, :, cases.WIDE])
    assert 0 < w[w > 0].min() < 2.3e-308 and w.max() > 1e99                                       # subnormal and huge draws are both there


@pytest.mark.parametrize("chains,draws", cases.PSIS_SHAPES)
def test_tail_length_and_the_position_of_the_tail_cut(chains, draws):
    """loo::psis: M = ceiling(min(S / 5, 3 sqrt(S / r_eff))) and the tail = the M largest ratios, ties by draw index; the draw just below them
    is the cutoff and keeps its weight.  Seen from outside: a draw psis_ref.psis moved away from its raw weight belongs to the tail."""
    S = chains * draws
    want = {8192: (1639, 272, 496), 8193: (1639, 272, 496), 8194: (1639, 272, 496), 16384: (3277, 384, 702)}[S]
    for re, m in zip((1e-6, 1.0, 0.3), want):
        assert psis_ref.tail_length(re, S) == int(np.ceil(min(S / 5, 3 * np.sqrt(S / re)))) == m
    r = cases.ratio_block(chains, draws)
    for p, re in enumerate(cases.GENERAL_R_EFF[:2]):                      # continuous ratios, and rounded ones: the cut falls inside a tie
        raw = r[p].reshape(-1) - r[p].max()
        lw, k = psis_ref.psis(-r[p], re)
        assert np.isfinite(k)
        M = psis_ref.tail_length(re, S)
        order = np.lexsort((np.arange(S), raw))                            # by value, then by draw index
        tail, body = order[S - M:], order[:S - M]
        if p == 1:
            assert raw[tail[0]] == raw[body[-1]]                           # a tie across the cut
        shift = lw[order[0]] - raw[order[0]]                               # -logsumexp of the smoothed weights
        moved = np.abs(lw - raw - shift) > 1e-9
        assert not moved[body].any()
        assert moved[tail[:-1]].mean() > 0.99                              # (the largest one is truncated at 0, where it began)
        if p == 1:
            assert moved[tail[:3]].all()                                   # of the draws tied at the cut, the later ones are smoothed
