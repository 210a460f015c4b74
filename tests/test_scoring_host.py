"""The numpy restatement of the scoring rules (tests/scoring_ref.py) earns its trust before the device is held to it, and the parts of
us_potus_model_amd/scoring.py that need no device: the argument checks, rmse, against."""
import numpy as np
import pytest

import scoring_ref as ref
from us_potus_model_amd import scoring as fs


def test_the_sorted_and_the_pairwise_crps_agree():
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 17, 200, 1001):
        x = rng.normal(0.5, 0.03, n)
        x[::5] = x[0]                                                      # ties
        for y in (0.45, float(x[0]), float(x.min()), float(x.max()), 0.9):
            assert abs(ref.crps_sorted(x, y) - ref.crps_pairwise(x, y)) <= 1e-13, (n, y)


def test_the_energy_score_of_one_coordinate_is_the_crps():
    rng = np.random.default_rng(2)
    for n in (1, 2, 50, 333):
        x = rng.normal(0.5, 0.05, n)
        for y in (0.4, float(x[n // 2])):
            assert abs(ref.energy(x[:, None], [y]) - ref.crps_pairwise(x, y)) <= 1e-13
    assert ref.variogram(rng.normal(size=(20, 1)), [0.3]) == 0.0


def test_degenerate_samples():
    # n = 1: |x - y| and the Euclidean distance
    assert ref.crps_pairwise([0.25], 0.75) == 0.5 == ref.crps_sorted([0.25], 0.75)
    assert ref.energy([[0.0, 0.0]], [3.0, 4.0]) == 5.0
    c = ref.column(np.array([0.25]), 0.75)
    assert c[0] == 0.5 and np.isnan(c[3]) and c[5] == 0.5 and c[6] == 0.25 and (c[1], c[2]) == (1.0, 1.0)
    # two points a < b: crps = (|a - y| + |b - y|) / 2 - (b - a) / 4
    a, b = 0.25, 0.75
    for y in (0.0, 0.25, 0.5, 1.0):
        want = (abs(a - y) + abs(b - y)) / 2 - (b - a) / 4
        assert abs(ref.crps_pairwise([a, b], y) - want) <= 1e-16 and abs(ref.crps_sorted([b, a], y) - want) <= 1e-16
    # ... and in the plane: (|p - y| + |q - y|) / 2 - |p - q| / 4
    p, q, y = np.array([0.0, 0.0]), np.array([3.0, 4.0]), np.array([3.0, 0.0])
    assert abs(ref.energy([p, q], y) - ((3.0 + 4.0) / 2 - 5.0 / 4)) <= 1e-15
    # a constant column: no variance, crps = |x - y|
    c = ref.column(np.full(9, 0.3), 0.5)
    assert abs(c[0] - 0.2) <= 1e-16 and np.isnan(c[3]) and (c[1], c[2]) == (1.0, 1.0)
    assert np.isnan(ref.dss_joint(np.zeros((3, 3)), np.zeros(3)))         # n <= m


def test_shifting_the_draws_and_the_result_changes_nothing():
    rng = np.random.default_rng(3)
    x, y = rng.integers(0, 1 << 20, (60, 4)) / 2.0 ** 22, rng.integers(0, 1 << 20, 4) / 2.0 ** 22
    s = 0.5                                                                # every sum x + s is exact
    for f in (ref.energy, ref.variogram, ref.dss_joint):
        a, b = f(x, y), f(x + s, y + s)
        assert abs(a - b) <= 1e-9 * max(1.0, abs(a)), f.__name__
    ca, cb = ref.column(x[:, 0], y[0]), ref.column(x[:, 0] + s, y[0] + s)
    assert np.allclose(ca, cb, rtol=1e-9, atol=1e-14) and ca[1] == cb[1] and ca[2] == cb[2]


def _paired(diff):
    return diff.mean() / (diff.std(ddof=1) / np.sqrt(diff.size))


def test_the_true_law_scores_best_in_the_gaussian_toy():
    """m = 6, sd 0.03, correlation 0.8, 200 draws a forecast, 400 outcomes: the true law has the lower mean energy and variogram score than the
    law with three times the sd and than the law without the correlation, each paired mean difference by at least 5 of its standard errors
    (measured in numpy: 33 and 13 for the energy score, 42 and 28 for the variogram score; the 5 is a floor, not a measurement)."""
    rng = np.random.default_rng(20161108)
    m, sd, rho, n, reps = 6, 0.03, 0.8, 200, 400
    cov = sd * sd * (rho * np.ones((m, m)) + (1 - rho) * np.eye(m))
    L = np.linalg.cholesky(cov)
    mu = np.full(m, 0.5)
    es, vs = np.zeros((reps, 3)), np.zeros((reps, 3))
    for r in range(reps):
        y = mu + L @ rng.normal(size=m)
        z = rng.normal(size=(n, m))
        laws = (mu + z @ L.T, mu + 3.0 * (z @ L.T), mu + sd * z)          # the truth, three times the sd, the correlation removed
        for k, x in enumerate(laws):
            es[r, k], vs[r, k] = _energy64(x, y), _variogram64(x, y)
    for name, sc in (("energy", es), ("variogram", vs)):
        for k, alt in ((1, "three times the sd"), (2, "correlation removed")):
            t = _paired(sc[:, k] - sc[:, 0])
            print(f"{name} score, {alt}: paired mean difference / standard error = {t:.1f}")
            assert t >= 5.0, (name, alt, t)
    # the float64 forms used in the loop are the restatement's
    assert abs(_energy64(laws[0], y) - ref.energy(laws[0], y)) <= 1e-13 and abs(_variogram64(laws[0], y) - ref.variogram(laws[0], y)) <= 1e-13


def _energy64(x, y):
    n = x.shape[0]
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    return np.sqrt(((x - y) ** 2).sum(-1)).mean() - d.sum() / (2.0 * n * n)


def _variogram64(x, y, p=0.5):
    a, b = np.triu_indices(x.shape[1], 1)
    return ((np.abs(y[a] - y[b]) ** p - (np.abs(x[:, a] - x[:, b]) ** p).mean(0)) ** 2).sum()


def test_numpy_linalg_is_good_to_the_tolerance_at_correlation_0_9():
    """The joint Dawid-Sebastiani score of the restatement is numpy.linalg in float64; at a correlation of 0.9 between 63 states it agrees with
    mpmath at 50 digits far inside the 1e-9 the device is held to (checked where mpmath imports)."""
    mp = pytest.importorskip("mpmath")
    rng = np.random.default_rng(5)
    m, n = 63, 200
    L = np.linalg.cholesky(0.9 * np.ones((m, m)) + 0.1 * np.eye(m))
    x, y = 0.5 + 0.03 * rng.normal(size=(n, m)) @ L.T, 0.5 + 0.03 * L @ rng.normal(size=m)
    mp.mp.dps = 50
    X = mp.matrix(x.tolist())
    mu = [mp.fsum(X[i, j] for i in range(n)) / n for j in range(m)]
    D = mp.matrix(n, m)
    for i in range(n):
        for j in range(m):
            D[i, j] = X[i, j] - mu[j]
    cov = (D.T * D) / (n - 1)
    Lc = mp.cholesky(cov)
    z = mp.lu_solve(Lc, mp.matrix([mp.mpf(float(y[j])) - mu[j] for j in range(m)]))
    want = 2 * mp.fsum(mp.log(Lc[j, j]) for j in range(m)) + mp.fsum(v * v for v in z)
    got = ref.dss_joint(x, y)
    print(f"numpy.linalg against mpmath: {got!r} / {float(want)!r}")
    assert abs(got - float(want)) <= 1e-12 + 1e-11 * abs(float(want)), (got, float(want))           # a hundredth of the device's tolerance


def test_the_boundary_declares_the_calls_and_the_r_shim_uses_its_entry():
    from pathlib import Path
    from us_potus_model_amd import sampler
    root = Path(__file__).resolve().parent.parent
    new = {"potus_forecast_scores", "potus_forecast_scores_device", "potus_forecast_scores_datasets", "potus_forecast_scores_timing", "potus_R_forecast_scores"}
    hdr = (root / "include" / "potus_hmc.h").read_text()
    assert new <= set(sampler.EXPORTS) and all(f"{name}(" in hdr for name in new)
    r = (root / "R" / "potus_sampling.R").read_text()
    assert '.C("potus_R_forecast_scores"' in r and "potus_forecast_scores <- function(fit, actual, ev" in r
    # a refusal of the .C() entry comes back as a status, before any device call
    import ctypes as C
    L = sampler.load_library()
    st, x = C.c_int(-1), np.zeros(64)
    dp = x.ctypes.data_as(C.POINTER(C.c_double))
    L.potus_R_forecast_scores((C.c_int * 1)(12345), C.byref(C.c_int(1)), (C.c_int * 3)(0, 1, 270), dp, dp, (C.c_int * 4)(1, 1, 1, 1), C.byref(C.c_double(0.5)), dp, dp, dp,
                              C.byref(st))
    assert st.value != 0
    buf = C.create_string_buffer(256)
    L.potus_last_error(buf, 256)
    assert b"potus_forecast_scores" in buf.value and b"handle" in buf.value


# ---- scoring.py without a device
def _result(rng, lead=()):
    S, nd = 5, 2
    uni, multi = rng.uniform(0.1, 1.0, lead + (nd, S + 2, 7)), rng.uniform(0.1, 1.0, lead + (nd, 3))
    return fs.ForecastScores(uni, multi, 100, [1, 1, 0, 1, 1], np.linspace(0.3, 0.7, S + 2), (3, 5)), uni, multi


def test_rmse_against_and_table():
    rng = np.random.default_rng(6)
    a, uni, multi = _result(rng)
    b, uni_b, multi_b = _result(rng)
    use = np.array([1, 1, 0, 1, 1], bool)
    assert a.rmse() == np.sqrt(uni[-1, :5, 6][use].mean()) and a.rmse(0) == np.sqrt(uni[0, :5, 6][use].mean())
    assert np.array_equal(a.crps, uni[..., 0]) and np.array_equal(a.pit, uni[..., 1:3]) and np.array_equal(a.dss_joint, multi[..., 2])
    d = a.against(b)
    assert set(d) == set(fs.SCORES)
    assert np.array_equal(d["crps"], uni[..., 0] - uni_b[..., 0]) and np.array_equal(d["energy"], multi[..., 0] - multi_b[..., 0])
    assert np.array_equal(d["se_mean"], uni[..., 6] - uni_b[..., 6]) and np.array_equal(d["variogram"], multi[..., 1] - multi_b[..., 1])
    t = a.table()
    assert t["columns"][-2:] == ["national", "electoral_votes"] and np.array_equal(t["interval"], uni[-1, :, 4]) and t["rmse"] == a.rmse()
    other = fs.ForecastScores(uni, multi, 100, [1, 1, 1, 1, 1], a.actual, (3, 5))
    with pytest.raises(ValueError, match="same days, states"):
        a.against(other)
    with pytest.raises(ValueError, match="different outcomes"):
        a.against(fs.ForecastScores(uni, multi, 100, a.use, a.actual + 0.01, (3, 5)))
    # a timeline's result: the leading axis is the run date
    g, uni_g, _ = _result(rng, (4,))
    assert g.rmse().shape == (4,) and g.rmse()[2] == np.sqrt(uni_g[2, -1, :5, 6][use].mean()) and g.energy.shape == (4, 2)


def test_check_args():
    S = 4
    ev, w, y = np.array([3.0, 10.0, 20.0, 5.0]), np.array([0.1, 0.4, 0.3, 0.2]), np.array([0.4, 0.6, 0.55, 0.3])
    e, a, u, p = fs.check_args(S, ev, y, w=w)
    assert a.shape == (S + 2,) and a[S + 1] == 30.0 and a[S] == ref.full_actual(y, w, ev)[S] and u.tolist() == [1] * S and p == 0.5
    assert np.array_equal(a, ref.full_actual(y, w, ev))
    e, a, u, p = fs.check_args(S, ev, y, use=[1, 0, 0, 1], vs_p=1, actual_national=0.51, actual_ev=232, w=w)
    assert a[S] == 0.51 and a[S + 1] == 232.0 and u.dtype == np.int32 and u.tolist() == [1, 0, 0, 1] and p == 1.0
    assert np.array_equal(fs.check_args(S, ev, np.append(y, [0.5, 7.0]))[1], np.append(y, [0.5, 7.0]))
    for kw, msg in ((dict(use=[0, 0, 0, 0]), "use selects no state"), (dict(vs_p=0.0), "vs_p"), (dict(vs_p=2.5), "vs_p"),
                    (dict(vs_p=float("nan")), "vs_p"), (dict(use=[1, 1]), "use has shape"), (dict(actual_national=1.5), "outside"),
                    (dict(actual_ev=float("inf")), "not finite")):
        with pytest.raises(ValueError, match=msg):
            fs.check_args(S, ev, y, w=w, **kw)
    bad = y.copy()
    bad[1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        fs.check_args(S, ev, bad, w=w)
    bad[1] = 1.25
    with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
        fs.check_args(S, ev, bad, w=w)
    with pytest.raises(ValueError, match="actual has shape"):
        fs.check_args(S, ev, y[:3], w=w)
    with pytest.raises(ValueError, match="ev has shape"):
        fs.check_args(S, ev[:3], y, w=w)
    with pytest.raises(ValueError, match="S = 64"):
        fs.check_args(64, np.ones(64), np.full(64, 0.5), w=np.full(64, 1 / 64))
    with pytest.raises(ValueError, match="given too"):                     # nothing is ignored in silence
        fs.check_args(S, ev, np.append(y, [0.5, 7.0]), actual_ev=10.0)
    with pytest.raises(ValueError, match="no weights"):
        fs.check_args(S, ev, y)
