"""E_loo's numpy restatement (tests/eloo_ref.py) against cases with a known answer: a conjugate normal model whose
leave-one-out posterior is analytic, numpy's own quantile, hand-built weighted quantiles, the rule for constant and two-valued quantities, and
predict's variance formula against a direct simulation.  The GPU tests (test_gpu_eloo.py) hold the device against the restatement."""
import numpy as np
from scipy import stats

import eloo_ref as ref
import psis_ref

PROBS = (0.05, 0.5, 0.95)


def test_conjugate_normal_leave_one_out_posterior():
    """y_i ~ N(theta, sigma^2), theta ~ N(m0, s0^2), exact iid posterior draws.  Without y_i the posterior is normal with precision
    1 / s0^2 + (N - 1) / sigma^2.  Every estimate within 4 standard errors, the standard error = the analytic LOO sd / sqrt(1 / sum w^2)."""
    rng = np.random.default_rng(12)                      # (a seed at which the restatement itself passes: all polls share one set of draws, so
    N, sigma, m0, s0, C, n = 8, 1.5, 0.3, 2.0, 4, 1000   #  a sample whose own mean is 3 standard errors off fails every poll at once)
    y = rng.normal(0.8, sigma, N)
    prec = 1.0 / s0 ** 2 + N / sigma ** 2
    theta = rng.normal((m0 / s0 ** 2 + y.sum() / sigma ** 2) / prec, prec ** -0.5, (C, n))
    r = -stats.norm.logpdf(y[:, None, None], theta[None], sigma)
    x = np.broadcast_to(theta, r.shape)
    out, kh = ref.e_loo(x, r, PROBS, r_eff=np.ones(N))
    assert (kh < 0.7).all(), kh.max()                    # every estimate is in the regime where PSIS is reliable
    for i in range(N):
        pl = 1.0 / s0 ** 2 + (N - 1) / sigma ** 2
        ml, sl = (m0 / s0 ** 2 + (y.sum() - y[i]) / sigma ** 2) / pl, pl ** -0.5
        w, _ = ref.weights(r[i], 1.0)
        se = sl / np.sqrt(1.0 / np.sum(w * w))
        want = np.concatenate([[ml, sl], stats.norm.ppf(PROBS, ml, sl)])
        got = np.concatenate([[out[i, 0], out[i, 2]], out[i, 3:]])
        assert (np.abs(got - want) < 4 * se).all(), (i, got, want, se)
        assert abs(out[i, 1] - out[i, 2] ** 2) < 1e-15
    # the weights do move the estimate: the outlying observation's LOO mean differs from the posterior mean by many standard errors
    far = int(np.argmax(np.abs(y - y.mean())))
    w, _ = ref.weights(r[far], 1.0)
    assert abs(out[far, 0] - theta.mean()) > 8 * prec ** -0.5 / np.sqrt(1.0 / np.sum(w * w))


def test_equal_weights_give_numpy_quantile_exactly():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(1, 3, 37))
    r = np.full((1, 3, 37), -2.5)                        # identical ratios: no tail to fit, equal weights
    out, kh = ref.e_loo(x, r, PROBS, r_eff=np.ones(1))
    assert out[0, 3:].tobytes() == np.quantile(x.reshape(-1), PROBS).tobytes()
    assert np.isinf(kh).all()
    assert abs(out[0, 0] - x.mean()) < 1e-15 and abs(out[0, 1] - x.var()) < 1e-15


def test_hand_built_weighted_quantiles():
    x = np.array([3.0, 1.0, 2.0, 4.0])
    w = np.array([0.1, 0.4, 0.3, 0.2])                   # sorted: x 1 2 3 4, w .4 .3 .1 .2, ww .4 .7 .8 1
    q = ref.wquantile(x, w, [0.2, 0.4, 0.55, 0.9])
    assert q[0] == 1.0 and q[1] == 1.0                   # j = 0: x[0], also when ww[0] = p exactly
    assert abs(q[2] - (1.0 + (0.55 - 0.4) / 0.3)) < 1e-15
    assert abs(q[3] - (3.0 + (0.9 - 0.8) / (1.0 - 0.8))) < 1e-14
    # ties in x are ordered by draw index: the weight of the first of two equal values is met first
    xt, wt = np.array([2.0, 1.0, 2.0, 5.0]), np.array([0.5, 0.1, 0.2, 0.2])   # sorted: 1 2(draw 0) 2(draw 2) 5, ww .1 .6 .8 1
    qt = ref.wquantile(xt, wt, [0.35, 0.7, 0.9])
    assert abs(qt[0] - (1.0 + (0.35 - 0.1) / 0.5)) < 1e-15 and qt[1] == 2.0 and abs(qt[2] - (2.0 + 3.0 * (0.9 - 0.8) / 0.2)) < 1e-14
    # a zero-weight draw changes nothing where it is not a neighbour, and is a valid neighbour where it is
    xz, wz = np.array([1.0, 2.5, 3.0]), np.array([0.5, 0.0, 0.5])             # ww .5 .5 1
    qz = ref.wquantile(xz, wz, [0.25, 0.75])
    assert qz[0] == 1.0 and abs(qz[1] - (2.5 + 0.5 * (0.75 - 0.5) / 0.5)) < 1e-15
    # unnormalised weights are normalised
    assert abs(ref.wquantile(x, 7.0 * w, [0.55])[0] - q[2]) < 1e-15


def test_constant_and_two_valued_quantities_take_the_k_of_the_ratios():
    rng = np.random.default_rng(11)
    r = rng.normal(0, 1.0, (3, 4, 250)) + 0.5 * rng.standard_t(3, (3, 4, 250))
    x = np.stack([np.full((4, 250), 0.37), (rng.random((4, 250)) < 0.4).astype(float), rng.normal(size=(4, 250))])
    out, kh = ref.e_loo(x, r, PROBS)
    k_r = psis_ref.loo_pointwise(-r)[:, 3]
    assert np.array_equal(kh[:, 2], k_r) and np.isfinite(k_r).all()
    assert np.array_equal(kh[0], np.repeat(k_r[0], 3)) and np.array_equal(kh[1], np.repeat(k_r[1], 3))
    assert (kh[2, :2] >= k_r[2]).all()
    assert abs(out[0, 0] - 0.37) < 1e-15 and out[0, 1] < 1e-30
    # a quantity that is not finite somewhere: k_r too
    xn = x[2].copy()
    xn[0, 0] = np.inf
    assert ref.khat(xn.reshape(-1), r[2], 1.0, k_r[2]) == k_r[2]


def test_a_heavy_tail_of_h_times_rho_raises_k_above_the_k_of_the_ratios():
    rng = np.random.default_rng(2)
    r = rng.normal(0, 0.3, (1, 4, 500))
    x = stats.pareto.rvs(1.2, size=(1, 4, 500), random_state=rng)            # a quantity whose own tail is heavy (k = 1 / 1.2)
    _, kh = ref.e_loo(x, r, (), r_eff=np.ones(1))
    assert kh[0, 2] < 0.3 and kh[0, 0] > 0.5 and kh[0, 1] > kh[0, 0]


def test_predict_variance_against_a_direct_simulation():
    """y / n with y ~ Binomial(n, p), p = inv_logit(eta + sigma z), (eta, z) under a weighted posterior: the formula from E[a1], E[a2] against
    the variance of simulated shares, within 4 simulation standard errors."""
    rng = np.random.default_rng(7)
    S, n, sig, R = 400, 37, 0.6, 4000
    eta = rng.normal(0.2, 0.3, S)
    w = rng.dirichlet(np.full(S, 0.5))
    xk, wk = np.polynomial.hermite.hermgauss(16)
    p = 1.0 / (1.0 + np.exp(-(eta[:, None] + sig * np.sqrt(2.0) * xk)))
    a1, a2 = (p * wk).sum(axis=1) / np.sqrt(np.pi), (p * p * wk).sum(axis=1) / np.sqrt(np.pi)
    e1, e2 = np.sum(w * a1), np.sum(w * a2)
    var = ref.predict_var(e1, e2, n)
    s = rng.choice(S, size=(R, 200), p=w)
    ps = 1.0 / (1.0 + np.exp(-(eta[s] + sig * rng.normal(size=s.shape))))
    share = rng.binomial(n, ps) / n
    m = share.size
    d = share - e1
    se_var = np.sqrt((np.mean(d ** 4) - np.mean(d ** 2) ** 2) / m)
    assert abs(share.mean() - e1) < 4 * np.sqrt(var / m)
    assert abs(np.mean(d ** 2) - var) < 4 * se_var, (np.mean(d ** 2), var, se_var)


def test_shared_form_equals_the_pointwise_form_column_by_column():
    rng = np.random.default_rng(13)
    r = rng.normal(0, 0.8, (3, 2, 60))
    X = rng.normal(size=(4, 2, 60))
    lw = np.stack([psis_ref.psis(-r[i], 1.0)[0].reshape(2, 60) for i in range(3)])
    mean, var, ess, kh = ref.e_loo_shared(X, lw, r, np.ones(3), diag=True)
    for j in range(4):
        out, k = ref.e_loo(np.broadcast_to(X[j], r.shape), r, (), r_eff=np.ones(3))
        assert np.allclose(mean[:, j], out[:, 0], rtol=0, atol=1e-14) and np.allclose(var[:, j], out[:, 1], rtol=0, atol=1e-14)
        assert np.array_equal(kh[:, j], k[:, 0])
    assert np.allclose(ess, 1.0 / np.exp(2 * lw).reshape(3, -1).sum(axis=1))


def test_gauss_hermite_rule_of_the_poll_share_against_quad():
    """16 nodes centred at 0 against scipy.integrate.quad over the sigma and eta range of the designs (sigma <= 0.3 is what the reference's
    designs use; eta within +-3 logits covers every poll): the figures DESIGN.md section 4r states."""
    worst = {}
    for sig in (0.02, 0.1, 0.3, 0.6, 1.0):
        w = 0.0
        for eta in np.linspace(-3.0, 3.0, 13):
            a = ref.poll_share(eta, sig, 0.0, True)
            q = ref.poll_share_quad(float(eta), sig)
            w = max(w, abs(a[0] - q[0]), abs(a[1] - q[1]))
        worst[sig] = w
    print({k: f"{v:.1e}" for k, v in worst.items()})
    # (quad itself is asked for 1e-13 relative; the rule degrades as sigma widens the sigmoid's curvature over the nodes)
    assert worst[0.02] < 1e-13 and worst[0.1] < 1e-13 and worst[0.3] < 1e-13 and worst[0.6] < 1e-10 and worst[1.0] < 1e-6
    a1, a2 = ref.poll_share(0.4, 0.0, 0.0, True)
    assert abs(a1 - 1 / (1 + np.exp(-0.4))) < 1e-15 and abs(a2 - a1 * a1) < 1e-15
