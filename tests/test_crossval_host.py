"""CPU tests of exact cross-validation (us_potus_model_amd.crossval, timeline.lfo_masks): the fold assignments, the designs and held masks
made from them, the leave-future-out masks on the committed timeline fixture, the Kfold arithmetic, and the names of the new entry points in
the header, sampler.EXPORTS and the R shim."""
import re
from pathlib import Path

import numpy as np
import pytest

from us_potus_model_amd import crossval, dataprep, loo as loo_mod, sampler, synthetic, timeline

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def data():
    return synthetic.small("full")


def _n(data):
    return int(data["N_state_polls"]) + int(data["N_national_polls"])


@pytest.mark.parametrize("K", [2, 3, 10])
@pytest.mark.parametrize("by", ["random", "pollster", "state"])
def test_folds_partition_the_polls(data, K, by):
    f = crossval.folds(data, K, by)
    assert f.shape == (_n(data),) and f.min() >= 0 and f.max() < K
    sizes = np.bincount(f, minlength=K)
    assert sizes.sum() == _n(data)
    if by == "random":
        assert sizes.max() - sizes.min() <= 1 and np.array_equal(f, np.random.default_rng(0).permutation(_n(data)) % K)
        return
    g = crossval.poll_groups(data, by)
    for grp in np.unique(g):
        assert np.unique(f[g == grp]).size == 1, (by, grp)                      # every group whole
    # greedy on descending sizes: the folds differ by no more than the largest group
    assert sizes.max() - sizes.min() <= np.bincount(g).max(), (sizes, np.bincount(g).max())
    if np.unique(g).size >= K:
        assert (sizes > 0).all()


def test_folds_by_state_keep_the_national_polls_together(data):
    g = crossval.poll_groups(data, "state")
    Ns = int(data["N_state_polls"])
    assert (g[Ns:] == int(data["S"])).all() and g[:Ns].max() < int(data["S"])
    f = crossval.folds(data, 3, "state")
    assert np.unique(f[Ns:]).size == 1


def test_folds_are_deterministic_in_the_seed(data):
    a, b, c = crossval.folds(data, 5, "random", seed=3), crossval.folds(data, 5, "random", seed=3), crossval.folds(data, 5, "random", seed=4)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(crossval.folds(data, 3, "pollster", seed=1), crossval.folds(data, 3, "pollster", seed=2))
    for bad in (1, _n(data) + 1):
        with pytest.raises(ValueError):
            crossval.folds(data, bad)
    with pytest.raises(ValueError):
        crossval.folds(data, 3, "mode")


def test_balanced_assignment_rule():
    # groups of sizes 5, 3, 3, 2, 1 (groups 0..4) into 2 folds: 5 -> fold 0; 3 -> fold 1; 3 -> fold 1 (3 < 5); 2 -> fold 0 (5 < 6); 1 -> fold 1 (6 < 7)
    groups = np.repeat(np.arange(5), [5, 3, 3, 2, 1])
    f = crossval._balanced(groups, 2)
    assert [int(f[groups == g][0]) for g in range(5)] == [0, 1, 1, 0, 1]
    # ties: equal sizes go in group order to the lower fold first
    f = crossval._balanced(np.repeat(np.arange(4), 2), 4)
    assert f.tolist() == [0, 0, 1, 1, 2, 2, 3, 3]


def test_design_masks_are_the_complement_of_the_held_masks(data):
    f = crossval.folds(data, 3, "pollster")
    d = crossval.design(data, f)
    hs, hn = crossval.held_masks(data, f)
    Ns = int(data["N_state_polls"])
    assert d["keep_state"].shape == hs.shape == (3, Ns) and d["keep_national"].shape == hn.shape == (3, int(data["N_national_polls"]))
    assert np.array_equal(d["keep_state"], ~hs) and np.array_equal(d["keep_national"], ~hn)
    assert d["mu_b_prior"] is None and d["mu_b_T_scale"] is None
    held = np.concatenate([hs, hn], axis=1)
    assert (held.sum(0) == 1).all() and np.array_equal(held.argmax(0), f)      # every poll held out by exactly its fold
    m = timeline.data_of(d, 1)
    assert (np.asarray(m["n_two_share_state"])[hs[1]] == 0).all() and (np.asarray(m["n_two_share_state"])[~hs[1]] > 0).all()


def test_lfo_masks_on_the_committed_timeline():
    d = dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")["data"]
    design = timeline.load_fixture(ROOT / "tests" / "golden" / "timeline_2016.npz", d)
    hs, hn = timeline.lfo_masks(design)
    for held, keep in ((hs, design["keep_state"]), (hn, design["keep_national"])):
        assert held.shape == keep.shape and not held[-1].any()
        assert keep[-1].all()
        # every poll of the last date is held out exactly once -- by the date before it arrived -- or never, if the first date already saw it
        assert np.array_equal(held.sum(0), (~keep[0]).astype(int))
        assert not (held & keep).any()                                          # a date never scores a poll it was fitted to
        for dte in range(keep.shape[0] - 1):
            assert np.array_equal(held[dte], keep[dte + 1] & ~keep[dte])
    assert hs.sum() + hn.sum() > 0


def test_kfold_arithmetic_as_loo_and_against():
    rng = np.random.default_rng(5)
    N, K, n = 12, 3, 40
    fold = np.arange(N) % K
    p = rng.uniform(0.01, 0.2, (K, N, n))                                       # made-up predictive densities per draw
    lpd = np.full((K, N, 2), np.nan)
    for i in range(N):
        lpd[fold[i], i] = np.log(p[fold[i], i].mean()), np.log((p[fold[i], i] ** 2).mean())
    y, nn = np.arange(N), np.arange(N) + 5
    kf = crossval.of_lpd(lpd, np.full(K, n), fold, name="a", y=y, n=nn)
    want = np.array([np.log(p[fold[i], i].mean()) for i in range(N)])
    assert np.allclose(kf.elpd, want, rtol=0, atol=1e-15)
    # delta method: var(log mean p) = var(p) / (n mean(p)^2), the population variance
    mc = np.array([p[fold[i], i].std() / (np.sqrt(n) * p[fold[i], i].mean()) for i in range(N)])
    assert np.allclose(kf.mcse, mc, rtol=1e-10)
    assert kf.elpd_kfold == pytest.approx(want.sum(), abs=1e-13) and kf.se == pytest.approx(np.sqrt(N) * want.std(ddof=1), rel=1e-13)
    lo = kf.as_loo()
    assert isinstance(lo, loo_mod.Loo) and np.array_equal(lo.pointwise[:, 0], kf.elpd) and np.array_equal(lo.pointwise[:, 2], -2 * kf.elpd)
    assert np.isnan(lo.pointwise[:, [1, 3, 4]]).all() and np.isnan(lo.estimates[1]).all()
    assert lo.estimates[0].tolist() == [kf.elpd_kfold, kf.se] and lo.estimates[2].tolist() == [-2 * kf.elpd_kfold, 2 * kf.se]
    assert np.array_equal(lo.y, y) and np.array_equal(lo.n, nn) and lo.n_draws == n
    other = crossval.of_lpd(lpd - 0.25, np.full(K, n), fold, name="b", y=y, n=nn)
    rows = loo_mod.loo_compare(lo, other.as_loo())
    assert rows[0]["name"] == "a" and rows[0]["elpd_diff"] == 0.0 and rows[1]["elpd_diff"] == pytest.approx(-0.25 * N)
    assert rows[1]["se_diff"] == pytest.approx(0.0, abs=1e-12)
    with pytest.raises(ValueError, match="same polls"):
        loo_mod.loo_compare(lo, crossval.of_lpd(lpd, np.full(K, n), fold, y=y + 1, n=nn).as_loo())
    # against(): a PSIS-LOO that is off by a known amount at known polls
    pw = np.zeros((N, 5))
    pw[:, 0] = kf.elpd - np.where(np.arange(N) < 2, 1.0, 0.0)                   # k-fold minus LOO = 1 at polls 0 and 1, 0 elsewhere
    pw[:, 3] = np.where(np.arange(N) % 4 == 0, 0.9, 0.1)                        # polls 0, 4, 8 above the threshold
    t = kf.against(loo_mod.Loo(pw, np.zeros((3, 2)), 4000))
    assert np.allclose(t["diff"][:2], 1.0) and np.allclose(t["diff"][2:], 0.0)
    assert t["all"]["n"] == N and t["all"]["mean"] == pytest.approx(2.0 / N) and t["all"]["max_abs"] == pytest.approx(1.0) and t["all"]["outside"] == 2
    assert t["high_k"]["n"] == 3 and t["high_k"]["mean"] == pytest.approx(1.0 / 3) and t["high_k"]["outside"] == 1
    assert kf.against(loo_mod.Loo(pw, np.zeros((3, 2)), 4000), mcse_loo=np.full(N, 1.0))["all"]["outside"] == 0
    with pytest.raises(sampler.PotusError, match="fold 1"):
        crossval.of_lpd(lpd, np.array([n, 0, n]), fold)


def test_entry_points_are_declared_everywhere():
    hdr = (ROOT / "include" / "potus_hmc.h").read_text()
    new = {"potus_cv_log_lik_device", "potus_cv_lpd", "potus_cv_timing", "potus_R_cv_lpd"}
    assert new <= set(re.findall(r"\b(potus_[A-Za-z_0-9]+)\s*\(", hdr))
    assert new <= set(sampler.EXPORTS)
    for name in ("cv_lpd", "cv_log_lik_device", "cv_timing"):
        assert callable(getattr(sampler.Handle, name))
    r = (ROOT / "R" / "potus_sampling.R").read_text()
    assert "potus_R_cv_lpd" in r and "potus_kfold <- function" in r and '.Call("potus_call_cv_lpd"' in r
    assert "SEXP potus_call_cv_lpd(" in (ROOT / "R" / "src" / "potus_call.c").read_text()
    L = sampler.load_library()
    assert L.potus_cv_timing(None) != 0                  # an argument refusal: no device needed
    assert L.potus_cv_lpd(12345, None, None, 1, None, None) != 0                # no such handle
