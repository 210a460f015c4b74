"""potus_monitor / potus_monitor_device (csrc/potus_monitor.hpp) against the numpy restatement diagnostics.monitor_row: built blocks through the
_device entry, edge columns, and one short synthetic fit pooled over two handles."""
import ctypes as C

import numpy as np
import pytest

from us_potus_model_amd import Handle, diagnostics as dg, monitor as mn, sampler

DP = C.POINTER(C.c_double)
PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)


def _dp(a):
    return a.ctypes.data_as(DP)


def _device_block(block):
    """a host array copied to device memory through the HIP runtime (no torch): returns (pointer, free)"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), block.nbytes) == 0
    assert hip.hipMemcpy(p, block.ctypes.data_as(C.c_void_p), block.nbytes, 1) == 0     # hipMemcpyHostToDevice
    return p, lambda: hip.hipFree(p)


def _restatement(block, probs):
    """diagnostics.monitor_row column by column: block [draws, chains, columns] -> [columns, 8 + len(probs)]"""
    x = np.transpose(block, (1, 0, 2))
    return np.array([dg.monitor_row(x[:, :, j], probs) for j in range(x.shape[2])])


def _assert_table(got, ref):
    """the project's own tolerances (1e-12 for summaries; rtol 1e-10 for R-hat / ESS)"""
    mean, sd = ref[:, 0], np.where(np.isfinite(ref[:, 1]), ref[:, 1], 0.0)
    d = np.abs(got[:, 0] - mean)
    with np.errstate(invalid="ignore", divide="ignore"):                                  # the figures first, then the assertions
        print("mean: max |d| / (|mean| + sd) =", np.nanmax(d / (np.abs(mean) + sd), initial=0.0),
              " sd, mad: max rel =", np.nanmax(np.abs(got[:, 1:3] / ref[:, 1:3] - 1), initial=0.0),
              " slots 3-7: max rel =", np.nanmax(np.abs(got[:, 3:8] / ref[:, 3:8] - 1), initial=0.0),
              " quantiles: max rel =", np.nanmax(np.abs(got[:, 8:] / ref[:, 8:] - 1), initial=0.0))
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert (d[np.isfinite(mean)] <= 1e-12 * (np.abs(mean) + sd)[np.isfinite(mean)]).all()
    assert np.allclose(got[:, 1:3], ref[:, 1:3], rtol=1e-12, atol=0, equal_nan=True)
    assert np.allclose(got[:, 8:], ref[:, 8:], rtol=1e-12, atol=0, equal_nan=True)
    assert np.allclose(got[:, 3:8], ref[:, 3:8], rtol=1e-10, atol=0, equal_nan=True)


def _ar1_block(draws, chains, ncols):
    """the columns of test_device_diagnostics_match_the_numpy_restatement: AR(1) from -0.6 to 0.98, disagreeing chains, runs of ties, rounded values"""
    rng = np.random.default_rng(draws + chains)
    blk = np.zeros((draws, chains, ncols))
    for j in range(ncols):
        rho = np.linspace(-0.6, 0.98, ncols)[j]
        e = rng.standard_normal((draws, chains))
        x = np.zeros((draws, chains))
        x[0] = e[0]
        for t in range(1, draws):
            x[t] = rho * x[t - 1] + np.sqrt(1 - rho * rho) * e[t]
        if j % 5 == 1:
            x = x * (1.0 + 0.5 * np.arange(chains)) + 0.7 * np.arange(chains)            # chains that disagree
        if j % 5 == 2:
            x = np.repeat(x[::3], 3, axis=0)[:draws]                                      # every draw three times in a row: ties
        if j % 5 == 3:
            x = np.round(x, 1)                                                            # heavy ties across chains too
        blk[:, :, j] = x
    return blk


@pytest.mark.gpu
@pytest.mark.parametrize("draws,chains,ncols", [(301, 4, 37), (500, 40, 3), (8, 2, 5), (9, 3, 5)])
def test_device_table_matches_the_numpy_restatement(draws, chains, ncols):
    """potus_monitor_device against diagnostics.monitor_row: an odd number of draws per chain (the split drops a draw the moments keep), 20 000
    pooled draws (more than one LDS run: order statistics across runs), the smallest n with an ESS (8) and an odd one beside it.  R-hat and
    bulk ESS are the very doubles potus_diagnostics_device returns for the block.  (On the two larger shapes the restatement's ess_tail is
    finite everywhere; on the two smallest the tied column's 95 % quantile is its maximum, the indicator constant and ess_tail NaN on both
    sides.  The type-7 indicator equals np.quantile's for every draw of every column.)"""
    blk = _ar1_block(draws, chains, ncols)
    x = np.transpose(blk, (1, 0, 2))
    for j in range(ncols):
        for p in (0.05, 0.95):
            assert np.array_equal(x[:, :, j] <= dg.quantile7(x[:, :, j], p), x[:, :, j] <= np.quantile(x[:, :, j], p))
    ref = _restatement(blk, PROBS)
    if draws > 100:
        assert np.isfinite(ref).all()
    L = sampler.load_library()
    p, free = _device_block(blk)
    probs = np.array(PROBS)
    got = np.zeros((ncols, 8 + len(PROBS)))
    rhat, ess = np.zeros(ncols), np.zeros(ncols)
    rc = L.potus_monitor_device(0, p, draws, chains, ncols, _dp(probs), len(PROBS), _dp(got))
    rc2 = L.potus_diagnostics_device(0, p, draws, chains, ncols, _dp(rhat), _dp(ess))
    free()
    assert rc == 0 and rc2 == 0
    _assert_table(got, ref)
    assert np.array_equal(got[:, 4], rhat, equal_nan=True) and np.array_equal(got[:, 5], ess, equal_nan=True)


@pytest.mark.gpu
def test_edge_columns_in_one_block():
    """A constant column (mean and quantiles the value, sd = mad = 0, slots 3-7 NaN), a column of +0.0 and -0.0 (constant too), a column with
    one NaN and one with an inf (every slot NaN), -0.0 among ordinary draws, probs 0 and 1 (minimum and maximum exactly), n_probs = 0, and
    600 pooled chains refused before anything is allocated."""
    rng = np.random.default_rng(17)
    draws, chains = 50, 3
    blk = rng.standard_normal((draws, chains, 6))
    blk[:, :, 1] = -3.25
    blk[:, :, 2] = np.where(rng.random((draws, chains)) < 0.5, 0.0, -0.0)
    blk[17, 2, 3] = np.nan
    blk[5, 0, 4] = -np.inf
    blk[::4, :, 5] = -0.0
    L = sampler.load_library()
    p, free = _device_block(blk)
    probs = np.array([0.0, 1.0, 0.5])
    got, got0 = np.zeros((6, 11)), np.full((6, 8), -1.0)
    assert L.potus_monitor_device(0, p, draws, chains, 6, _dp(probs), 3, _dp(got)) == 0
    assert L.potus_monitor_device(0, p, draws, chains, 6, None, 0, _dp(got0)) == 0
    assert L.potus_monitor_device(0, p, 2, 600, 1, _dp(probs), 3, _dp(got)) != 0        # 600 chains pooled: refused up front
    free()
    ref = _restatement(blk, probs)
    _assert_table(got, ref)
    assert np.array_equal(got[:, :8], got0, equal_nan=True)                             # the quantiles change nothing in front of them
    assert got[1, :3].tolist() == [-3.25, 0.0, 0.0] and np.isnan(got[1, 3:8]).all() and got[1, 8:].tolist() == [-3.25] * 3
    assert got[2, :3].tolist() == [0.0, 0.0, 0.0] and np.isnan(got[2, 3:8]).all() and got[2, 8:].tolist() == [0.0] * 3
    assert np.isnan(got[3]).all() and np.isnan(got[4]).all()
    for j in (0, 5):
        assert got[j, 8] == blk[:, :, j].min() and got[j, 9] == blk[:, :, j].max()
        assert np.isfinite(got[j]).all()


@pytest.mark.gpu
def test_fitted_posterior_pooled_over_two_handles(cases, monkeypatch):
    """synthetic.small, chains 1-3 and 4-5 of one posterior on two handles that save their warm-up rows (40 warm-up + 30 draws; pooled handles
    must have saved equal numbers of rows), and ONE handle that holds the five chains and saves none: the
    table of lp__, mu_c, polling_bias, e_bias and a block of mu_b columns against the restatement on the rows fetched with write_array, warm-up
    rows dropped; byte for byte the table of ONE handle holding the five chains; mean_low_high; a range cut into several internal blocks gives
    the bytes of separate calls; potus_R_monitor; a handle with potus_set_datasets is refused."""
    from conftest import second_device
    data, variant = cases["small_full"]
    kw = dict(num_warmup=40, num_samples=30, seed=11, cus_per_chain=1, twin=0)          # one workgroup per chain: the draws do not depend on the split
    hs = [Handle(data, variant, chains=3, chain_id_offset=0, save_warmup=1, device=0, **kw),
          Handle(data, variant, chains=2, chain_id_offset=3, save_warmup=1, device=second_device(), **kw)]
    one = Handle(data, variant, chains=5, save_warmup=0, **kw)
    for h in hs + [one]:
        h.init()
        h.run(70)
    pars = ["lp__", "mu_c", "polling_bias", "e_bias"]
    m = mn.monitor(hs, pars=pars)
    assert m.n_chains == 5 and m.n_draws == 30 and m.probs == PROBS

    def fetched(a, b):                                                                    # [30 draws, 5 chains, b - a]
        return np.concatenate([h.write_array(a, b, 70)[40:] for h in hs], axis=1)
    ranges = [(0, 1)] + [hs[0].layout[n][:2] for n in pars[1:]]
    ref = np.concatenate([_restatement(fetched(a, b), PROBS) for a, b in ranges])
    _assert_table(m.table, ref)
    assert m.names[0] == "lp__" and m.names[1] == "mu_c.1" and m.par("mu_c").shape == (int(data["P"]), 13) and m.par("e_bias").shape == (int(data["T"]), 13)
    a = hs[0].layout["mu_b"][0]
    mb = mn.monitor(hs, cols=(a, a + 40))
    _assert_table(mb.table, _restatement(fetched(a, a + 40), PROBS))
    assert mb.names[0] == "mu_b.1.1"
    # the same chains in one handle: the same bytes
    assert np.array_equal(one.monitor(pars=pars).table, m.table, equal_nan=True)
    assert np.array_equal(mn.monitor([one], cols=(a, a + 40)).table, mb.table, equal_nan=True)
    # mean +- 1.96 sd of the fetched draws (final_2016.R:578-582)
    b0, b1, _ = hs[0].layout["mu_c"]
    d = fetched(b0, b1).reshape(-1, b1 - b0)
    want = np.stack([d.mean(0), d.mean(0) - 1.96 * d.std(0, ddof=1), d.mean(0) + 1.96 * d.std(0, ddof=1)], axis=1)
    assert np.allclose(m.mean_low_high("mu_c"), want, rtol=1e-12, atol=1e-12 * np.abs(d).max())
    # a range worked in several internal blocks: 7 columns per block here ((70 + 30) rows x 5 chains x 8 bytes = 4000 bytes per column)
    monkeypatch.setenv("POTUS_MONITOR_BLOCK_BUDGET", "28000")
    cut = mn.monitor(hs, cols=(a, a + 40))
    monkeypatch.delenv("POTUS_MONITOR_BLOCK_BUDGET")
    assert np.array_equal(cut.table, mb.table, equal_nan=True)
    two = np.concatenate([mn.monitor(hs, cols=(a, a + 7)).table, mn.monitor(hs, cols=(a + 7, a + 40)).table])
    assert np.array_equal(two, mb.table, equal_nan=True)
    # the .C() wrapper
    L = hs[0].L
    out, st, probs = np.zeros((40, 13)), C.c_int(-1), np.array(PROBS)
    ids = (C.c_int * 2)(hs[0].h, hs[1].h)
    L.potus_R_monitor(ids, C.byref(C.c_int(2)), (C.c_int * 2)(a, a + 40), _dp(probs), C.byref(C.c_int(5)), _dp(out), C.byref(st))
    assert st.value == 0 and np.array_equal(out, mb.table, equal_nan=True)
    for h in hs + [one]:
        h.close()
    # many data sets in one handle: the pooled table is refused
    many = Handle(data, variant, chains=2, num_warmup=5, num_samples=5, seed=3, cus_per_chain=1, twin=0)
    many.set_datasets(np.stack([np.asarray(data["n_democrat_state"])] * 2), np.stack([np.asarray(data["n_democrat_national"])] * 2))
    with pytest.raises(sampler.PotusError, match="error 4.*potus_monitor pools all chains"):
        many.monitor(pars=["lp__"])
    many.close()
