"""CPU tests of the PSIS-LOO layer: the numpy restatement (tests/psis_ref.py) on closed cases, its quadrature against scipy, loo_compare's
arithmetic and refusal, and the names of the new entry points in the header, the R shim and sampler.EXPORTS."""
import re
from pathlib import Path

import numpy as np
import pytest
from scipy import stats

import psis_ref
from us_potus_model_amd import loo, sampler

ROOT = Path(__file__).resolve().parent.parent


def test_identical_log_likelihoods_give_elpd_ll_and_no_p_loo():
    ll = np.full((3, 4, 100), -2.5)
    pw = psis_ref.loo_pointwise(ll)
    assert np.allclose(pw[:, 0], -2.5, atol=1e-12) and np.allclose(pw[:, 1], 0.0, atol=1e-12)
    assert np.isinf(pw[:, 3]).all()                       # a tail of equal values: no fit


def test_short_tail_means_no_smoothing():
    rng = np.random.default_rng(1)
    ll = rng.normal(-3, 1, (2, 250))
    S = ll.size
    assert psis_ref.tail_length(S, S) < 5
    lw, k = psis_ref.psis(ll, r_eff=float(S))
    raw = np.minimum(-ll.reshape(-1) + ll.min(), 0.0)
    assert np.isinf(k) and np.allclose(lw, raw - np.log(np.exp(raw).sum()), atol=1e-13)


def test_equal_tail_values_give_infinite_k():
    rng = np.random.default_rng(2)
    ll = rng.normal(-3, 1, 1000)
    ll[ll < np.quantile(ll, 0.3)] = np.quantile(ll, 0.3)   # the largest ratios -ll are one value
    lw, k = psis_ref.psis(ll, r_eff=1.0)
    assert np.isinf(k)


@pytest.mark.parametrize("k_true", [0.3, 0.8])
def test_khat_of_exact_generalized_pareto_ratios(k_true):
    x = stats.genpareto.rvs(c=k_true, size=100_000, random_state=np.random.default_rng(3))
    _, k = psis_ref.psis(-np.log(x), r_eff=1.0)        # ratios exp(-ll) = x
    assert abs(k - k_true) < 0.15, k


def test_relative_eff_of_independent_draws_is_near_one():
    ll = np.random.default_rng(4).normal(-3, 0.3, (4, 1000))
    assert 0.85 < psis_ref.relative_eff(ll) < 1.15


def test_quadrature_equals_scipy_quad():
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(200):
        n = float(rng.choice([1, 20, 100, 660, 3000, 60000]))
        y = float(rng.integers(0, n + 1))
        eta, sig = rng.normal(0, 1), float(rng.choice([0.02, 0.04, 0.1, 0.3]))
        worst = max(worst, abs(psis_ref.log_lik_integrated(y, n, eta, sig) - psis_ref.log_lik_quad(y, n, eta, sig)))
    print(f"largest |Gauss-Hermite({psis_ref.GH_NODES}) - quad| = {worst:.2e}")
    assert worst < 1e-10
    assert psis_ref.log_lik_integrated(7, 20, 0.3, 0.0) == psis_ref.log_lik_plain(7, 20, 0.3)


def _fake(elpd_i, name, y=None):
    pw = np.zeros((len(elpd_i), 5))
    pw[:, 0] = elpd_i
    pw[:, 2] = -2 * pw[:, 0]
    est = psis_ref.estimates(pw)
    yy = np.arange(len(elpd_i)) if y is None else y
    return loo.Loo(pw, est, 4000, name, yy, yy + 10)


def test_loo_compare_arithmetic_and_refusal():
    rng = np.random.default_rng(6)
    a = rng.normal(-4, 1, 50)
    b = a - rng.gamma(2.0, 0.2, 50)
    rows = loo.loo_compare(_fake(b, "worse"), _fake(a, "better"))
    assert [r["name"] for r in rows] == ["better", "worse"]
    assert rows[0]["elpd_diff"] == 0 and rows[0]["se_diff"] == 0
    d = b - a
    assert rows[1]["elpd_diff"] == pytest.approx(d.sum()) and rows[1]["se_diff"] == pytest.approx(np.sqrt(50) * d.std(ddof=1))
    assert rows[1]["elpd_loo"] == pytest.approx(b.sum())
    assert "elpd_diff" in loo.format_compare(rows)
    with pytest.raises(ValueError, match="same polls"):
        loo.loo_compare(_fake(a, "x"), _fake(b, "y", y=np.arange(50) + 1))
    with pytest.raises(ValueError, match="same polls"):
        loo.loo_compare(_fake(a, "x"), _fake(b[:40], "y"))


def test_pareto_k_table_thresholds():
    lo = _fake(np.zeros(5), "m")
    lo.pointwise[:, 3] = [0.1, 0.69, 0.8, 1.5, np.inf]
    assert lo.k_threshold() == pytest.approx(min(1 - 1 / np.log10(4000), 0.7))
    assert lo.pareto_k_table() == {"good": 2, "bad": 1, "very bad": 2}
    assert "Pareto k" in str(lo)


def test_new_names_are_declared_exported_and_wrapped():
    new = {"potus_log_lik_device", "potus_loo_device", "potus_loo", "potus_R_loo"}
    hdr = (ROOT / "include" / "potus_hmc.h").read_text()
    assert new <= set(re.findall(r"\b(potus_[A-Za-z_0-9]+)\s*\(", hdr))
    assert new <= set(sampler.EXPORTS)
    r = (ROOT / "R" / "potus_sampling.R").read_text()
    assert '"potus_R_loo"' in r and "potus_loo <- function" in r and "potus_loo_compare <- function" in r
    L = sampler.load_library()
    assert all(hasattr(L, nm) for nm in new)
