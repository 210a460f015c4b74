"""CPU tests of the per-poll binomial terms against tests/golden/poll_terms.npz (scripts/make_golden_poll_terms.py: mpmath at 40 - 60 digits): the
oracle on the tail designs (|eta| from 0 to 800, y = 0, y = n, n = 0, n = 2 000 000), which yields e_orc, the one number the device's tolerance in
tests/test_gpu_poll_terms.py comes from; the numpy restatements of the integrated log-likelihood over the whole grid; and, where mpmath is
installed, a sample of the fixture recomputed."""
import numpy as np
import pytest

import poll_terms_ref as ptr
import psis_ref
from oracle_lib import OracleModel


def test_fixture_covers_the_grid_and_the_edge_counts():
    F, g = ptr.fixture(), ptr.gen()
    sigma, n, y, eta, off = g.ll_cells()
    for k, v in (("ll_sigma", sigma), ("ll_n", n), ("ll_y", y), ("ll_eta", eta), ("ll_off", off)):
        assert np.array_equal(F[k], v), k
    assert len(sigma) == 720 and F["ll_integrated"].shape == (720,) and F["ll_plain"].shape == (720, 3)
    assert all(np.array_equal(F[k], v) for k, v in zip(("tail_n", "tail_y", "tail_eta"), g.tail_cells()))
    assert np.isfinite(F["ll_integrated"]).all() and np.isfinite(F["ll_plain"]).all() and np.isfinite(F["tail_plain"]).all()
    for name in ptr.design_names():
        data, variant, q, lp, gr, A_lp, A = ptr.design(name)
        T = int(data["T"])
        for kind in ("state", "national"):
            nn, yy, day = (np.asarray(data[f"{k}_{kind}"]) for k in ("n_two_share", "n_democrat", "day"))
            for d in (1, T):
                on = day == d
                assert ((yy == 0) & (nn > 0) & on).any() and ((yy == nn) & (nn > 0) & on).any() and ((nn == 0) & on).any()
                assert ((nn == 2_000_000) & on).any() and ((nn == 61_771) & on).any()
        mags = [g.magnitudes(data, variant, q[i]) for i in range(len(q))]
        g.check_buckets(name, np.array([m[2] for m in mags]), mags[0][3], mags[0][4])
        for i, m in enumerate(mags):                                   # the magnitudes are doubles of this machine: equal to rounding
            assert abs(m[0] - A_lp[i]) <= 1e-12 * A_lp[i] and np.all(np.abs(m[1] - A[i]) <= 1e-9 * A[i])


def test_oracle_matches_the_60_digit_values_on_the_tail_designs():
    """Both forms of the oracle at every tail point; the largest scaled error is e_orc (poll_terms_ref.py)."""
    e_lp = e_g = 0.0
    for name in ptr.design_names():
        data, variant, q, lp, g, A_lp, A = ptr.design(name)
        m = OracleModel(data, variant)
        for fast in (False, True):
            for i in range(len(q)):
                lpo, go = m.log_prob_grad(q[i], fast=fast)
                a, b = ptr.scaled_errors(lpo, go, lp[i], g[i], A_lp[i], A[i])
                e_lp, e_g = max(e_lp, a), max(e_g, b)
    print(f"e_orc: lp {e_lp:.3e}, gradient {e_g:.3e}")
    assert e_lp <= ptr.E_ORC_LP and e_g <= ptr.E_ORC_GRAD
    assert e_g >= ptr.E_ORC_GRAD / 4                                   # the recorded figure is the measured one, not a loose ceiling


def test_numpy_integrated_forms_match_the_40_digit_grid():
    """psis_ref.log_lik_integrated restates the device formula (bracketed mode search, 16 nodes); log_lik_quad is the independent check the GPU
    tests use (brentq, scipy quad).  The first to rounding, the second within the GPU tests' 1e-9 of the 40-digit values, cells 3 and 6 logits off included."""
    F = ptr.fixture()
    y, n, eta, sigma, ref = F["ll_y"], F["ll_n"], F["ll_eta"], F["ll_sigma"], F["ll_integrated"]
    lc = psis_ref.lchoose(n, y)
    err = np.abs(psis_ref.log_lik_integrated(y, n, eta, sigma) - lc - ref) / np.maximum(1.0, np.abs(ref))
    print("log_lik_integrated: worst", err.max(), "at cell", int(err.argmax()))
    assert err.max() <= 1e-13                                          # measured 6.4e-15: rounding; 16 nodes leave no truncation error at this level
    hard = np.flatnonzero((np.abs(F["ll_off"]) >= 2.5) & (sigma * sigma * n >= 8))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in list(hard[::5]) + list(range(0, 720, 29)):
            v = psis_ref.log_lik_quad(y[i], n[i], eta[i], sigma[i]) - lc[i]
            assert abs(v - ref[i]) <= 1e-9 * max(1.0, abs(ref[i])), (i, v, ref[i])
    # the iteration the device used to run (eight undamped Newton steps from 0) is off by orders on the hard cells: the fixture would have caught it
    z = np.zeros(len(hard))
    for _ in range(8):
        p = psis_ref._expit(eta[hard] + sigma[hard] * z)
        z = z - (sigma[hard] * (y[hard] - n[hard] * p) - z) / (-sigma[hard] ** 2 * n[hard] * p * (1 - p) - 1.0)
    assert (np.abs(z - psis_ref.integrand_mode(y[hard], n[hard], eta[hard], sigma[hard])) > 1.0).any()


def test_a_sample_of_the_fixture_recomputes():
    """The fixture is what the generator computes today (two values that are both good to 40 digits round to the same double or to neighbours)."""
    pytest.importorskip("mpmath")
    F, g = ptr.fixture(), ptr.gen()
    same = lambda a, b: abs(a - b) <= 4e-16 * max(1.0, abs(b))
    for i in range(5, 720, 41):
        v = float(g.mp_integrated(F["ll_y"][i], F["ll_n"][i], F["ll_eta"][i], F["ll_sigma"][i]))
        assert same(v, F["ll_integrated"][i]), i
        for k, z in enumerate(F["ll_z"]):
            x = g._mp(40).mpf(float(F["ll_eta"][i])) + g._mp(40).mpf(float(F["ll_sigma"][i])) * g._mp(40).mpf(float(z))
            assert same(float(g.mp_plain(F["ll_y"][i], F["ll_n"][i], x)), F["ll_plain"][i, k])
    for i in range(0, len(F["tail_eta"]), 5):
        assert same(float(g.mp_plain(F["tail_y"][i], F["tail_n"][i], F["tail_eta"][i])), F["tail_plain"][i])
    for name, point in (("s6_full", 1), ("s1_nomode", 4)):
        data, variant, q, lp, gr, A_lp, A = ptr.design(name)
        m = g.MpModel(data, variant)
        assert same(float(m.log_prob(q[point])), lp[point])
        lay, D = g.layout(data, variant)
        coords = [0, lay["raw_mu_b"][0] + 7, lay["raw_measure_noise_national"][0] + 3, lay["raw_measure_noise_state"][0] + 5, D - 1]
        if variant == "full":
            coords += [lay["mu_e_bias"][0], lay["rho_e_bias"][0]]
        got = np.array([float(v) for v in m.grad(q[point], coords=coords)])
        assert all(same(a, b) for a, b in zip(got, gr[point][coords]))
