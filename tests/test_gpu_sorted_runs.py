"""The seven kernels that bitonic-sort a column in LDS in runs (k_dg_column, k_mn_column, k_loo_psis, k_mm_psis, k_el_pointwise: runs of
DG_RUN = 8192 (key, index) pairs; k_col_summary: PS_RUN = 16384 doubles; k_tl_summary: one run of at most TL_MAX_DRAWS = PS_RUN) at the edges
of their runs, and with more work items than workgroups.  Each leg holds an entry point to the numpy restatement its own test file uses,
at that file's tolerance, on the inputs of tests/sorted_run_cases.py (tests/test_sorted_runs_host.py holds the restatements to numpy and
scipy on the same inputs); every call is made twice and must repeat its bytes; every leg prints its worst deviation before it asserts.

  A  potus_diagnostics_device   R-hat, bulk ESS                       diagnostics.rhat / ess_bulk            rtol 1e-10
  B  potus_monitor_device       the summary row                       diagnostics.monitor_row                test_gpu_monitor._assert_table
  C  loo.loo_of_block           PSIS-LOO pointwise and totals         psis_ref.loo_pointwise / estimates     test_gpu_loo._close, 1e-8
  D  potus_psis_device          weights and k of general ratios       psis_ref.psis                          the same
  E  loo.e_loo                  mean, variance, quantiles, their k    eloo_ref.e_loo                         the same
  F  posterior_summary          of fitted handles                     oracle/posterior_summary_ref.py        rtol = atol = 1e-12
  G  Handle.laplace_summary     at TL_MAX_DRAWS and one below         timeline_ref.summary                   test_gpu_laplace's
  H  legs A-E with 1024 + 76 work items: item j, which leaves its kernel early, and item j + 1024 share a workgroup

Measured on an MI355X (largest deviation over the shapes of a leg): A 2e-16 (R-hat), 7e-15 (bulk ESS); B 2e-14, the subnormal median of the
wide-range column 6e-13; C 1e-13; D 8e-14; E 2e-13; F 1e-13 absolute, win frequencies equal; G 5e-15 (means), 1e-16 (quantiles); H 4e-15.
The fits of leg F take 0.4 to 0.6 s each at max_depth 3 (0.2 s at 1); the 44 cases take 15 s together, none more than 0.8 s.
"""
import ctypes as C
import sys
import time

import numpy as np
import pytest

import eloo_ref
import psis_ref
import sorted_run_cases as cases
import timeline_ref
from conftest import ROOT
from test_gpu_loo import _close
from test_gpu_monitor import _assert_table, _device_block, _restatement
from us_potus_model_amd import Handle, diagnostics as dg, loo as loo_mod, posterior_summary, sampler, synthetic

pytestmark = pytest.mark.gpu
DP = C.POINTER(C.c_double)
PROBS = cases.MONITOR_PROBS
E_PROBS = (0.05, 0.5, 0.95)
N_STATS = 8


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def _dp(a):
    return a.ctypes.data_as(DP)


def _dev(a):
    import torch
    return torch.tensor(np.array(a, dtype=np.float64), device="cuda:0")


# ---- the entries, each called twice
def _diagnostics(blk):
    """potus_diagnostics_device of blk [draws, chains, columns] -> (rhat, ess_bulk)"""
    blk = np.ascontiguousarray(blk)
    n, ch, nc = blk.shape
    L = sampler.load_library()
    p, free = _device_block(blk)
    out = [(np.zeros(nc), np.zeros(nc)) for _ in range(2)]
    rcs = [L.potus_diagnostics_device(0, p, n, ch, nc, _dp(r), _dp(e)) for r, e in out]
    free()
    assert rcs == [0, 0]
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    return out[0]


def _monitor(blk, probs=PROBS):
    """potus_monitor_device of blk [draws, chains, columns] -> [columns, 8 + len(probs)]"""
    blk = np.ascontiguousarray(blk)
    n, ch, nc = blk.shape
    L = sampler.load_library()
    p, free = _device_block(blk)
    pr = np.array(probs, dtype=np.float64)
    out = [np.zeros((nc, N_STATS + len(probs))) for _ in range(2)]
    rcs = [L.potus_monitor_device(0, p, n, ch, nc, _dp(pr), len(probs), _dp(o)) for o in out]
    free()
    assert rcs == [0, 0] and out[0].tobytes() == out[1].tobytes()
    return out[0]


def _loo(ll, r_eff=None):
    """loo.loo_of_block of ll [polls, chains, draws] -> (pointwise [polls, 5], estimates [3, 2])"""
    t = _dev(ll)
    a, b = loo_mod.loo_of_block(t, r_eff=r_eff), loo_mod.loo_of_block(t, r_eff=r_eff)
    assert a.pointwise.tobytes() == b.pointwise.tobytes() and a.estimates.tobytes() == b.estimates.tobytes()
    return a.pointwise, a.estimates


def _psis(r, r_eff):
    """potus_psis_device of r [polls, chains, draws] -> (lw [polls, S], k [polls])"""
    t = _dev(r)
    out = [loo_mod.psis_weights(t, r_eff) for _ in range(2)]
    lw = [o[0].cpu().numpy().reshape(r.shape[0], -1) for o in out]
    assert lw[0].tobytes() == lw[1].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    return lw[0], out[0][1]


def _e_loo(x, r, type="quantile", probs=E_PROBS, r_eff=None):
    """loo.e_loo -> (out [polls, 3 + len(probs)] = mean, variance, sd, quantiles; khat [polls, 3])"""
    xd, rd = _dev(x), _dev(r)
    got = [loo_mod.e_loo(xd, rd, type, probs, r_eff) for _ in range(2)]
    out = [np.concatenate([g.mean[:, None], g.variance[:, None], g.sd[:, None], g.quantiles], axis=1) for g in got]
    assert out[0].tobytes() == out[1].tobytes() and got[0].khat.tobytes() == got[1].khat.tobytes()
    return out[0], got[0].khat


def _rel(a, b):
    """largest |a - b| / max(1, |b|) over the finite entries of b: what _close bounds"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b)
    return float((np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))).max()) if fin.any() else 0.0


def _close_k(a, b):
    """_close, which has nothing to take a maximum of when every k is infinite"""
    if np.isfinite(b).any():
        _close(a, b)
    else:
        assert np.array_equal(a, b)


def _numpy_diagnostics(blk):
    x = cases.chains_first(blk)
    return (np.array([dg.rhat(x[:, :, j]) for j in range(x.shape[2])]), np.array([dg.ess_bulk(x[:, :, j]) for j in range(x.shape[2])]))


# ------------------------------------------------------------------------------------------------ legs A and B
@pytest.mark.parametrize("n,C", cases.COLUMN_SHAPES)
def test_leg_a_diagnostics_at_the_edges_of_a_run(n, C):
    """potus_diagnostics_device on the six columns (the tied, the -0.0 and the wide-range one among them: R-hat and bulk ESS are functions
    of ranks alone, so every column is held to the same bar).  The split draws number N = 2 C (n // 2): 8190, 8192 (the single-run path at
    its largest), 8194 (a last run of two) and 16384 (two full runs)."""
    blk = cases.column_block(n, C)
    rhat, ess = _diagnostics(blk)
    r_ref, e_ref = _numpy_diagnostics(blk)
    assert np.isfinite(r_ref).all() and np.isfinite(e_ref).all()
    print(f"leg A n = {n}, C = {C}: R-hat max rel = {np.abs(rhat / r_ref - 1).max():.2e}, bulk ESS max rel = {np.abs(ess / e_ref - 1).max():.2e}")
    assert np.allclose(rhat, r_ref, rtol=1e-10, atol=0)
    assert np.allclose(ess, e_ref, rtol=1e-10, atol=0)


@pytest.mark.parametrize("n,C", cases.COLUMN_SHAPES)
def test_leg_b_monitor_at_the_edges_of_a_run(n, C):
    """potus_monitor_device sorts M = C n draws (sorts 1 and 2) and, with an odd n, the N split draws on their own: (8193, 1) has a last
    run of ONE element, (2049, 4) sends M = 8196 through the global runs and N = 8192 through LDS with the same arguments.  Slots 4 and 5 are
    the doubles of leg A; probs 0 and 1 the exact minimum and maximum.  Of the wide-range column the mean, sd, MCSE and mean ESS are not
    compared (the restatement's FFT autocovariance has no relative accuracy over 400 decades); everything else of every column is.
    (The median of that column is subnormal, about 1e-311, where doubles lie 2^-1074 apart: at (1024, 8) device and restatement differ by
    that one step, 5.8e-13 relative; every other quantile of every column agrees to 2e-14, slots 3-7 to 7e-15.)"""
    blk = cases.column_block(n, C)
    got = _monitor(blk)
    ref = _restatement(blk, PROBS)
    rest = [j for j in range(len(cases.COLUMNS)) if j != cases.WIDE]
    assert np.isfinite(ref[rest]).all() and np.isfinite(ref[cases.WIDE, list(cases.WIDE_SLOTS)]).all()
    print(f"leg B n = {n}, C = {C}:")
    _assert_table(got[rest], ref[rest])
    w, wr = got[cases.WIDE], ref[cases.WIDE]
    print(f"  wide-range column: mad rel = {abs(w[2] / wr[2] - 1):.2e}, slots 4-6 max rel = {np.abs(w[4:7] / wr[4:7] - 1).max():.2e},"
          f" quantiles max rel = {np.abs(w[8:] / wr[8:] - 1).max():.2e}, median {w[10]!r} against {wr[10]!r}")
    assert np.allclose(w[2], wr[2], rtol=1e-12, atol=0) and np.allclose(w[8:], wr[8:], rtol=1e-12, atol=0)
    assert np.allclose(w[4:7], wr[4:7], rtol=1e-10, atol=0)
    rhat, ess = _diagnostics(blk)
    assert got[:, 4].tobytes() == rhat.tobytes() and got[:, 5].tobytes() == ess.tobytes()
    flat = blk.reshape(-1, blk.shape[2])
    assert np.array_equal(got[:, 8], flat.min(axis=0)) and np.array_equal(got[:, 12], flat.max(axis=0))


# ------------------------------------------------------------------------------------------------ legs C, D, E
@pytest.mark.parametrize("tail", ["computed", "tail_0.2S"])
@pytest.mark.parametrize("chains,draws", cases.PSIS_SHAPES)
def test_leg_c_psis_loo_at_the_edges_of_a_run(chains, draws, tail):
    """k_loo_psis with S = 8192 (ranks and tail out of LDS), 8193 and 8194 (a last run of one and of two ratios), 16384 (two full runs);
    poll 1 has its largest 30 % of ratios tied, so the tail cut falls inside a tie (k = inf: nothing to fit)."""
    ll = cases.log_lik_block(chains, draws)
    re = None if tail == "computed" else np.full(3, 1e-6)
    ref = psis_ref.loo_pointwise(ll, re)
    assert np.isfinite(ref[[0, 2]]).all() and np.isinf(ref[1, 3]) and np.isfinite(np.delete(ref[1], 3)).all()
    if re is not None:
        assert psis_ref.tail_length(1e-6, chains * draws) == int(np.ceil(0.2 * chains * draws))
    pw, est = _loo(ll, re)
    print(f"leg C S = {chains * draws} ({chains} x {draws}), r_eff {tail}: pointwise max rel = {_rel(pw, ref):.2e}, estimates max rel = {_rel(est, psis_ref.estimates(ref)):.2e}")
    _close(pw, ref)
    _close(est, psis_ref.estimates(ref))


@pytest.mark.parametrize("chains,draws", cases.PSIS_SHAPES)
def test_leg_d_psis_of_general_ratios_at_the_edges_of_a_run(chains, draws):
    """k_mm_psis through potus_psis_device: continuous ratios, ratios rounded to one decimal (which of the tied draws are smoothed is decided
    by their index, across runs) and ratios whose largest tenth is one value (k = inf)."""
    r = cases.ratio_block(chains, draws)
    re = np.array(cases.GENERAL_R_EFF)
    lw, k = _psis(r, re)
    want = [psis_ref.psis(-r[p], re[p]) for p in range(3)]
    lw_ref, k_ref = np.stack([w[0] for w in want]), np.array([w[1] for w in want])
    assert np.isfinite(lw_ref).all() and np.isfinite(k_ref[:2]).all() and np.isinf(k_ref[2])
    print(f"leg D S = {chains * draws} ({chains} x {draws}): log weights max rel = {_rel(lw, lw_ref):.2e}, k max rel = {_rel(k, k_ref):.2e}")
    _close(lw, lw_ref)
    _close(k, k_ref)


def _entry_case(which):
    """(log-likelihoods, x, given r_eff) of test_leg_d_the_psis_entries_agree_in_bytes"""
    if which == "many_ratios":       # the tied tails and the polls without a finite ratio (all -inf) among the early exits
        sel = [j for j in range(cases.N_EARLY) if _early_kind(j) in ("tied tail", "no finite ratio")]
        return -cases.many_ratios()[sel], cases.many_quantities()[sel], np.array(cases.GENERAL_R_EFF)[np.arange(len(sel)) % 3]
    chains, draws = which
    return cases.log_lik_block(chains, draws), cases.quantity_block(chains, draws, "continuous"), np.array(cases.GENERAL_R_EFF)


@pytest.mark.parametrize("which", [(1, 25), (2, 10), (3, 2731), (8, 1024), "many_ratios"], ids=str)
def test_leg_d_the_psis_entries_agree_in_bytes(which):
    """PSIS is stated once (potus_psis.hpp), so for the same ratios and the same given r_eff the k-hat of loo_of_block (k_loo_psis), of
    psis_weights on -ll (k_mm_psis) and e_loo(...).khat[:, 2] (k_el_pointwise) are the same bytes, NaN and inf included: S = 25 (Mt = 5, the
    smallest fitted tail), 20 (Mt = 4: nothing fitted), 8193 (a last run of one) and 8192, and the tied tails and all -inf ratios of many_ratios.
    r_eff: e_loo does not return the r_eff it computes, so what is compared is e_loo under loo_of_block's computed r_eff with e_loo under its
    own -- every output, in bytes."""
    ll, x, re = _entry_case(which)
    pw, _ = _loo(ll, re)
    _, k = _psis(-ll, re)
    out, khat = _e_loo(x, -ll, r_eff=re)
    print(f"leg D entries {which}: max |k psis_weights - k loo| = {_rel(k, pw[:, 3]):.2e}, max |k e_loo - k loo| = {_rel(khat[:, 2], pw[:, 3]):.2e}")
    assert k.tobytes() == np.ascontiguousarray(pw[:, 3]).tobytes()
    assert np.ascontiguousarray(khat[:, 2]).tobytes() == np.ascontiguousarray(pw[:, 3]).tobytes()
    pw_c, _ = _loo(ll)
    fin = np.isfinite(pw_c[:, 4])               # (no finite ratio: loo_of_block reports a NaN r_eff, which e_loo would refuse as a given one)
    assert fin.any() and (which != "many_ratios" or not fin.all())
    own, under = _e_loo(x[fin], -ll[fin]), _e_loo(x[fin], -ll[fin], r_eff=pw_c[fin, 4])
    assert own[0].tobytes() == under[0].tobytes() and own[1].tobytes() == under[1].tobytes()


@pytest.mark.parametrize("kind", ["continuous", "rounded"])
@pytest.mark.parametrize("chains,draws", cases.PSIS_SHAPES)
def test_leg_e_e_loo_at_the_edges_of_a_run(chains, draws, kind):
    """k_el_pointwise sorts the ratios, x rho and x^2 rho (both tails of each) and x itself: mean, variance and quantiles with their k, for x
    continuous and x rounded to one decimal (ties in x: the weighted quantile walks them in draw order)."""
    r = -cases.log_lik_block(chains, draws)
    x = cases.quantity_block(chains, draws, kind)
    ref, kh = eloo_ref.e_loo(x, r, E_PROBS, None)
    assert np.isfinite(ref).all() and not np.isnan(kh).any()
    out, khat = _e_loo(x, r)
    print(f"leg E S = {chains * draws} ({chains} x {draws}), x {kind}: mean, variance, sd, quantiles max rel = {_rel(out, ref):.2e}, k max rel = {_rel(khat, kh):.2e}")
    _close(out, ref)
    _close_k(khat, kh)
    for type, cols, kcol in (("mean", [0], 0), ("variance", [1], 1)):       # the calls without quantiles: the same doubles
        o, k = _e_loo(x, r, type, None)
        assert o[:, cols].tobytes() == out[:, cols].tobytes() and k.tobytes() == khat.tobytes()
        _close(o[:, cols], ref[:, cols])


# ------------------------------------------------------------------------------------------------ leg F
EV_SMALL = np.array([100, 90, 80, 70, 60, 138], dtype=np.float64)
FIT_DEPTH = 3


@pytest.mark.parametrize("chains,ns", [(4, 4096), (5, 3277), (8, 4096)])
def test_leg_f_posterior_summary_at_the_edges_of_a_run(chains, ns):
    """k_col_summary with nd = 16384 (exactly one run, out of LDS), 16385 (a last run of one draw) and 32768 (two full runs) pooled draws of
    fits with short trees: the summary does not care whether the chains have converged."""
    sys.path.insert(0, str(ROOT / "oracle"))
    from posterior_summary_ref import posterior_summary as ref_summary
    data, variant = synthetic.small("full"), "full"
    S, T = int(data["S"]), int(data["T"])
    t0 = time.perf_counter()
    h = Handle(data, variant, chains=chains, num_warmup=20, num_samples=ns, seed=5, max_depth=FIT_DEPTH)
    h.init()
    h.run(20 + ns)
    t1 = time.perf_counter()
    got, again = posterior_summary([h], EV_SMALL), posterior_summary([h], EV_SMALL)
    a, b, _ = h.layout["predicted_score"]
    ps = h.write_array(a, b, ns).reshape(-1, S, T).transpose(0, 2, 1)      # [draw, T, S]
    h.close()
    assert ps.shape[0] == chains * ns and np.isfinite(ps).all()
    ref = ref_summary(ps, data["state_weights"], EV_SMALL)
    print(f"leg F nd = {chains * ns} ({chains} x {ns}): fit {t1 - t0:.2f} s; " +
          ", ".join(f"{k} max |d| = {np.abs(got[k] - ref[k]).max():.2e}" for k in ("state", "national", "electoral_votes")))
    for k in ("state", "national", "electoral_votes"):
        assert got[k].tobytes() == again[k].tobytes()
        assert np.allclose(got[k], ref[k], rtol=1e-12, atol=1e-12), (k, np.abs(got[k] - ref[k]).max())
    assert np.array_equal(got["state"][..., 3], ref["state"][..., 3])


# ------------------------------------------------------------------------------------------------ leg G
@pytest.fixture(scope="module")
def laplace_handle():
    data = synthetic.small("full")
    h = Handle(data, "full", chains=1, seed=1843, cus_per_chain=1, twin=0)
    mode = h.optimize(np.zeros((1, h.D)), jacobian=1, tol_obj=0.0, tol_rel_obj=0.0, tol_grad=1e-4, tol_rel_grad=0.0, tol_param=0.0, iter=5000)["q"][0]
    yield data, h, mode
    h.close()


@pytest.mark.parametrize("draws", [16384, 16383])
def test_leg_g_timeline_summary_at_its_limit(laplace_handle, draws):
    """k_tl_summary sorts a column in ONE run: TL_MAX_DRAWS = 16384 draws are accepted and fill it, 16383 leave one padding slot."""
    data, h, mode = laplace_handle
    T = int(data["T"])
    res = h.laplace(mode, draws)
    assert res["return_code"][0] == 0 and np.isfinite(res["lp"]).all()
    out, again = h.laplace_summary(EV_SMALL, (T - 3, T), ev_to_win=200), h.laplace_summary(EV_SMALL, (T - 3, T), ev_to_win=200)
    x = h.laplace_scores((T - 3, T)).cpu().numpy()[0]                      # [draws, 3 days, S]
    assert x.shape == (draws, 3, int(data["S"])) and out["n_draws"].tolist() == [draws]
    want = timeline_ref.summary(x, data["state_weights"], EV_SMALL, ev_to_win=200)
    worst = {}
    for key, mean_col in (("state", 2), ("national", 2), ("electoral_votes", None)):   # test_gpu_timeline._compare's tolerances
        assert out[key].tobytes() == again[key].tobytes()
        err = np.abs(out[key][0] - np.asarray(want[key]))
        worst[key] = [float(err[..., j].max()) for j in range(err.shape[-1])]
    print(f"leg G {draws} draws: max |d| per slot = {worst}")
    for key, mean_col in (("state", 2), ("national", 2), ("electoral_votes", None)):
        for j, e in enumerate(worst[key]):
            assert e <= (1e-12 if j == mean_col else 1e-15), (key, j, e)


# ------------------------------------------------------------------------------------------------ leg H
SUCCESSORS = tuple(range(cases.GRID_CAP, cases.N_MANY))
ALONE = SUCCESSORS + cases.OTHERS
EARLY = np.arange(cases.N_EARLY)


def test_leg_h_diagnostics_and_monitor_with_more_columns_than_workgroups():
    """1100 columns of 64 x 2 draws on a grid of 1024 workgroups: the workgroup of column j < 76 leaves it early (a NaN, an inf: every slot
    NaN; a constant, a constant of +-0.0: the monitor's `continue` after sort 1, while k_dg_column ranks the ties by position as the
    restatement does) and goes on to column j + 1024.  Every one of the 76 successors and 16 other columns has the bytes of a call of its
    own; the 16 agree with the restatement."""
    blk = cases.many_columns()
    rhat, ess = _diagnostics(blk)
    table = _monitor(blk)
    kind = EARLY % 4
    assert np.isnan(rhat[EARLY[kind < 2]]).all() and np.isnan(ess[EARLY[kind < 2]]).all()
    assert np.isnan(table[EARLY[kind < 2]]).all()
    r_c, e_c = _numpy_diagnostics(blk[:, :, EARLY[kind >= 2]])            # k_dg_column has no exit for a constant: ties ranked by position
    assert np.allclose(rhat[EARLY[kind >= 2]], r_c, rtol=1e-10, atol=0) and np.allclose(ess[EARLY[kind >= 2]], e_c, rtol=1e-10, atol=0)
    const = table[EARLY[kind >= 2]]
    assert (const[:, 1:3] == 0).all() and np.isnan(const[:, 3:8]).all() and (const[:, 8:] == const[:, :1]).all()
    assert np.array_equal(table[EARLY[kind == 2], 0], 0.25 * EARLY[kind == 2] - 3.0) and (table[EARLY[kind == 3], 0] == 0).all()
    assert np.isfinite(rhat[cases.N_EARLY:]).all() and np.isfinite(ess[cases.N_EARLY:]).all() and np.isfinite(table[cases.N_EARLY:, :6]).all()
    assert table[cases.N_EARLY:, 4].tobytes() == rhat[cases.N_EARLY:].tobytes() and table[cases.N_EARLY:, 5].tobytes() == ess[cases.N_EARLY:].tobytes()
    for j in ALONE:
        r1, e1 = _diagnostics(blk[:, :, j:j + 1])
        assert r1.tobytes() == rhat[j:j + 1].tobytes() and e1.tobytes() == ess[j:j + 1].tobytes(), j
        assert _monitor(blk[:, :, j:j + 1]).tobytes() == table[j:j + 1].tobytes(), j
    sub = blk[:, :, list(cases.OTHERS)]
    r_ref, e_ref = _numpy_diagnostics(sub)
    o = list(cases.OTHERS)
    print(f"leg H, 1100 columns of 64 x 2: R-hat max rel = {np.abs(rhat[o] / r_ref - 1).max():.2e}, bulk ESS max rel = {np.abs(ess[o] / e_ref - 1).max():.2e}")
    assert np.allclose(rhat[o], r_ref, rtol=1e-10, atol=0) and np.allclose(ess[o], e_ref, rtol=1e-10, atol=0)
    _assert_table(table[o], _restatement(sub, PROBS))


def test_leg_h_fewer_than_two_draws_per_half():
    """one chain of n = 3 draws (h = 1): k_dg_column leaves every column at once, k_mn_column gives moments, mad and quantiles and no R-hat or
    ESS; 1100 columns, so that a workgroup leaves two in a row"""
    blk = np.random.default_rng(3).standard_normal((3, 1, cases.N_MANY))
    rhat, ess = _diagnostics(blk)
    assert np.isnan(rhat).all() and np.isnan(ess).all()
    table = _monitor(blk)
    ref = _restatement(blk, PROBS)
    assert np.isfinite(ref[:, :3]).all() and np.isnan(ref[:, 3:8]).all() and np.isfinite(ref[:, 8:]).all()
    print("leg H, 1100 columns of 3 x 1:")
    _assert_table(table, ref)
    for j in (0, 75, 1024, 1099):
        assert _monitor(blk[:, :, j:j + 1]).tobytes() == table[j:j + 1].tobytes(), j


def _early_kind(j):
    return cases.EARLY_RATIO_KINDS[j % len(cases.EARLY_RATIO_KINDS)]


def test_leg_h_psis_loo_with_more_polls_than_workgroups():
    """k_loo_psis takes log-likelihoods: a NaN, an infinite one (either sign) leave the poll at once with NaN; identical ones, +-0.0 and a
    tied tail go through the sort and fit nothing (k = inf)."""
    r = cases.many_ratios()
    ll = -r
    pw, _ = _loo(ll)
    for j in range(cases.N_EARLY):
        if _early_kind(j) in ("nan", "plus inf", "no finite ratio"):
            assert np.isnan(pw[j]).all(), j
        else:
            assert np.isinf(pw[j, 3]) and np.isfinite(np.delete(pw[j], 3)).all(), j
    assert np.isfinite(pw[cases.N_EARLY:]).all()
    for j in ALONE:
        assert _loo(ll[j:j + 1])[0].tobytes() == pw[j:j + 1].tobytes(), j
    o = list(cases.OTHERS)
    ref = psis_ref.loo_pointwise(ll[o])
    print(f"leg H, 1100 polls of 2 x 64 (k_loo_psis): pointwise max rel = {_rel(pw[o], ref):.2e}")
    _close(pw[o], ref)


def test_leg_h_psis_of_general_ratios_with_more_polls_than_workgroups():
    """k_mm_psis: a NaN, a +inf ratio and no finite ratio leave the poll with NaN weights and k; identical ratios and a tied tail fit nothing"""
    r = cases.many_ratios()
    re = np.array(cases.GENERAL_R_EFF)[np.arange(cases.N_MANY) % 3]
    lw, k = _psis(r, re)
    for j in range(cases.N_EARLY):
        if _early_kind(j) in ("nan", "plus inf", "no finite ratio"):
            assert np.isnan(k[j]) and np.isnan(lw[j]).all(), j
        else:
            assert np.isinf(k[j]) and np.isfinite(lw[j]).all(), j
    assert np.isfinite(k[cases.N_EARLY:]).all() and np.isfinite(lw[cases.N_EARLY:]).all()
    for j in ALONE:
        l1, k1 = _psis(r[j:j + 1], re[j:j + 1])
        assert l1.tobytes() == lw[j:j + 1].tobytes() and k1.tobytes() == k[j:j + 1].tobytes(), j
    o = list(cases.OTHERS)
    want = [psis_ref.psis(-r[j], re[j]) for j in o]
    lw_ref, k_ref = np.stack([w[0] for w in want]), np.array([w[1] for w in want])
    print(f"leg H, 1100 polls of 2 x 64 (k_mm_psis): log weights max rel = {_rel(lw[o], lw_ref):.2e}, k max rel = {_rel(k[o], k_ref):.2e}")
    _close(lw[o], lw_ref)
    _close(k[o], k_ref)


def test_leg_h_e_loo_with_more_polls_than_workgroups():
    """k_el_pointwise: a NaN, a +inf ratio, no finite ratio (and, r_eff being computed, a -inf ratio) leave the poll with NaN; among the
    first 76 polls x is also constant, two-valued or holds a NaN (el_plain leaves early: the k of the ratios)."""
    r, x = cases.many_ratios(), cases.many_quantities()
    out, khat = _e_loo(x, r)
    for j in range(cases.N_EARLY):
        if _early_kind(j) in ("nan", "plus inf", "no finite ratio"):
            assert np.isnan(out[j]).all() and np.isnan(khat[j]).all(), j
        else:
            assert np.isinf(khat[j]).all() and (np.isnan(out[j, :3]).all() if j % 5 == 3 else np.isfinite(out[j]).all()), j
    assert np.isfinite(out[cases.N_EARLY:]).all() and np.isfinite(khat[cases.N_EARLY:]).all()
    for j in ALONE:
        o1, k1 = _e_loo(x[j:j + 1], r[j:j + 1])
        assert o1.tobytes() == out[j:j + 1].tobytes() and k1.tobytes() == khat[j:j + 1].tobytes(), j
    o = list(cases.OTHERS)
    ref, kh = eloo_ref.e_loo(x[o], r[o], E_PROBS, None)
    print(f"leg H, 1100 polls of 2 x 64 (k_el_pointwise): mean, variance, sd, quantiles max rel = {_rel(out[o], ref):.2e}, k max rel = {_rel(khat[o], kh):.2e}")
    _close(out[o], ref)
    _close(khat[o], kh)
