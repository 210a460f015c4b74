"""Moment matching for PSIS-LOO without a GPU: the reference on a conjugate toy, the host rules against the reference, the algebra of the
moments.

tests/loo_mm_ref.py restates DESIGN.md section 4q in numpy; the GPU tests hold potus_loo_moment_match against it.  Here the reference
itself is held against a case with an analytic answer, csrc/potus_loo_mm_rules.hpp (compiled alone, as test_advi_host.py compiles the
ADVI rules) is held against the reference's rules on recorded k sequences, and the identities that let the device work from the moments of
the untransformed draws are checked against the materialised transformed sample."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import loo_mm_ref as ref

ROOT = Path(__file__).resolve().parent.parent
INF, NAN = math.inf, math.nan


# ---------------------------------------------------------------------------------------------- the conjugate toy
def toy(seed, S=4000, shift=10.0, nobs=(6, 5, 8), tau=10.0, sigma=1.0):
    """Three independent coordinates theta_j ~ N(0, tau^2), observations y_ji ~ N(theta_j, sigma^2); observation 0 of coordinate 0 is moved
    `shift` sigma from the mean of its neighbours.  Draws from the exact posterior; the exact leave-one-out predictive density of the
    outlier is normal."""
    rng = np.random.default_rng(seed)
    truth = np.array([0.5, -1.0, 2.0])
    ys = [truth[j] + sigma * rng.standard_normal(n) for j, n in enumerate(nobs)]
    ys[0][0] = ys[0][1:].mean() + shift * sigma
    prec = np.array([1 / tau**2 + n / sigma**2 for n in nobs])
    mean = np.array([y.sum() / sigma**2 for y in ys]) / prec
    theta = mean + rng.standard_normal((S, len(nobs))) / np.sqrt(prec)

    def log_prob(t):
        out = -0.5 * (t**2).sum(axis=1) / tau**2
        for j, y in enumerate(ys):
            out = out - 0.5 * ((y[None, :] - t[:, j:j + 1])**2).sum(axis=1) / sigma**2
        return out

    y0 = ys[0][0]

    def log_lik(t):
        return -0.5 * np.log(2 * np.pi * sigma**2) - 0.5 * (y0 - t[:, 0])**2 / sigma**2

    p1 = 1 / tau**2 + (nobs[0] - 1) / sigma**2
    m1 = ys[0][1:].sum() / sigma**2 / p1
    var = sigma**2 + 1 / p1
    return theta, log_prob, log_lik, -0.5 * np.log(2 * np.pi * var) - 0.5 * (y0 - m1)**2 / var


TOY_BOUND = 3 * 0.0941   # three times the worst of the 20 seeds below


@pytest.mark.parametrize("seed", range(20))
def test_reference_on_the_conjugate_toy(seed):
    """|elpd_mm - analytic| of the planted outlier, seeds 0 .. 19, measured with this file on the CPU (S = 4000 as 4 chains of 1000, r_eff = 1):
    0.0136 0.0175 0.0817 0.0847 0.0538 0.0401 0.0356 0.0312 0.0227 0.0137 0.0685 0.0603 0.0322 0.0490 0.0082 0.0143 0.0941 0.0815 0.0196 0.0087
    (plain PSIS: 0.40 to 1.39, k-hat 1.08 to 1.46; after moment matching k-hat 0.28 to 0.52).  Every seed accepts one T1 step and splits."""
    theta, lp, ll, exact = toy(seed)
    out = ref.moment_match(theta, 1000, lp, ll, 1.0)
    thr = ref.default_threshold(theta.shape[0])
    assert thr == 0.7
    assert out["k0"] > 0.7, out["k0"]
    assert out["k"] < thr, out["k"]
    assert out["info"][0] + out["info"][1] >= 1 and out["split_done"]
    err_mm, err_psis = abs(out["elpd"] - exact), abs(out["elpd0"] - exact)
    assert err_mm < err_psis, (err_mm, err_psis)
    assert err_mm <= TOY_BOUND, err_mm


def test_psis_general_on_minus_ll_is_psis():
    import psis_ref
    rng = np.random.default_rng(3)
    ll = -np.abs(rng.standard_normal(700)) * 3
    lw, k = psis_ref.psis(ll, 0.8)
    lw2, k2 = ref.psis_general(-ll, 0.8)
    assert k == k2 and np.array_equal(lw, lw2)
    r = -ll.copy()
    r[::7] = -INF
    lw3, k3 = ref.psis_general(r, 0.8)
    assert np.isfinite(k3) and np.all(lw3[::7] == -INF) and abs(np.exp(lw3).sum() - 1) < 1e-12
    assert np.isnan(ref.psis_general(np.full(50, -INF), 1.0)[1])
    r[3] = NAN
    assert np.isnan(ref.psis_general(r, 0.8)[1])


# ---------------------------------------------------------------------------------------------- the host rules
PROGRAM = r"""
#include "potus_loo_mm_rules.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
static double num(const char *s) { return !strcmp(s, "-inf") ? -INFINITY : !strcmp(s, "inf") ? INFINITY : !strcmp(s, "nan") ? NAN : atof(s); }
// thr max_iters k0 k'1 k'2 ...  -> per candidate evaluated "candidate accepted", then "info n_t1 n_t2 rounds stop"
int main(int argc, char **argv) {
  if (argc < 4) return 2;
  const double thr = num(argv[1]);
  const int max_iters = atoi(argv[2]);
  LmmPoll p;
  int next = p.start(num(argv[3]), thr, max_iters);
  for (int a = 4; a < argc && next != LMM_NONE; a++) {
    const int ok = p.feed(num(argv[a]), thr, max_iters);
    printf("%d %d\n", next, ok);
    next = p.next;
  }
  printf("info %d %d %d %d\n", p.n_t1, p.n_t2, p.rounds, p.stop);
  return 0;
}
"""

# (threshold, max_iters, k0 then the k' of every candidate in the order they are evaluated)
SEQS = {
    "t1_rejected_t2_accepted": (0.7, 30, (1.2, 1.3, 0.9, 0.5)),
    "both_rejected": (0.7, 30, (1.2, 1.25, 1.2, 0.1)),                 # k' = k is no improvement; the 0.1 is never evaluated
    "max_iters_reached": (0.7, 2, (1.5, 1.4, 1.3, 1.2)),
    "max_iters_zero": (0.7, 0, (1.5, 0.1)),
    "already_below": (0.7, 30, (0.5, 0.1)),
    "exactly_at_the_threshold": (0.7, 30, (0.7, 0.1)),                 # the loop runs while k > threshold
    "nan_candidates": (0.7, 30, (1.2, NAN, NAN, 0.1)),
    "nan_then_accepted": (0.7, 30, (1.2, NAN, 1.1, 0.9, 0.69)),
    "from_infinity": (0.7, 30, (INF, 2.0, INF, 1.9, 0.3)),
    "nan_start": (0.7, 30, (NAN, 0.1)),
    "negative_threshold": (-1.0, 3, (0.2, 0.1, 0.3, 0.05, 0.04, 0.01)),  # k_threshold = -1: every poll enters the loop
}


def fmt(x):
    return "nan" if x != x else "-inf" if x == -INF else "inf" if x == INF else repr(float(x))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile potus_loo_mm_rules.hpp on its own"
    tmp = tmp_path_factory.mktemp("loo_mm_rules")
    (tmp / "mm_main.cpp").write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "us_potus_model_amd" / "csrc"), str(tmp / "mm_main.cpp"),
                    "-o", str(tmp / "mm_main")], check=True)
    return lambda *a: subprocess.run([str(tmp / "mm_main"), *a], check=True, capture_output=True, text=True).stdout.splitlines()


@pytest.mark.parametrize("name", sorted(SEQS))
def test_the_decisions_are_the_reference_s(program, name):
    thr, max_iters, ks = SEQS[name]
    lines = program(fmt(thr), str(max_iters), *[fmt(k) for k in ks])
    got = [tuple(int(v) for v in ln.split()) for ln in lines[:-1]]
    info = tuple(int(v) for v in lines[-1].split()[1:])
    want, want_info = ref.decisions(ks, thr, max_iters)
    assert got == [(c, int(ok)) for c, ok in want]
    assert info == want_info


def test_the_sequences_cover_what_they_are_meant_to():
    got = {k: ref.decisions(v[2], v[0], v[1]) for k, v in SEQS.items()}
    T1, T2 = ref.T1, ref.T2
    assert got["t1_rejected_t2_accepted"] == ([(T1, False), (T2, True), (T1, True)], (1, 1, 3, ref.BELOW))
    assert got["both_rejected"] == ([(T1, False), (T2, False)], (0, 0, 2, ref.REJECTED))
    assert got["max_iters_reached"] == ([(T1, True), (T1, True)], (2, 0, 2, ref.MAXIT))
    assert got["max_iters_zero"] == ([], (0, 0, 0, ref.MAXIT))
    assert got["already_below"] == ([], (0, 0, 0, ref.BELOW))
    assert got["exactly_at_the_threshold"] == ([], (0, 0, 0, ref.BELOW))
    assert got["nan_candidates"] == ([(T1, False), (T2, False)], (0, 0, 2, ref.REJECTED))
    assert got["nan_then_accepted"] == ([(T1, False), (T2, True), (T1, True), (T1, True)], (2, 1, 4, ref.BELOW))
    assert got["from_infinity"] == ([(T1, True), (T1, False), (T2, True), (T1, True)], (2, 1, 4, ref.BELOW))
    assert got["nan_start"] == ([], (0, 0, 0, ref.BELOW))
    assert got["negative_threshold"] == ([(T1, True), (T1, False), (T2, True), (T1, True)], (2, 1, 4, ref.MAXIT))


# ---------------------------------------------------------------------------------------------- the algebra
@pytest.mark.parametrize("seed", range(4))
def test_moments_of_the_transformed_sample_from_those_of_the_draws(seed):
    """mu_w and sigma^2_w from (m0, mu~, q~) against the weighted moments of the materialised a + b theta.  Both sides sum S products; each
    is within S 2^-53 sum |terms| of the exact sum, so they agree to S 2^-52 sum |terms| (the terms of the variance: w b^2 (theta - m0)^2)."""
    rng = np.random.default_rng(seed)
    S, D = 1501, 7
    theta = rng.standard_normal((S, D)) * rng.uniform(0.1, 30, D) + rng.uniform(-50, 50, D)
    a, b = rng.uniform(-3, 3, D), rng.uniform(0.5, 2, D)
    lw = rng.standard_normal(S) * 3
    lw -= np.log(np.exp(lw).sum())
    w = np.exp(lw)
    m0 = theta.mean(axis=0)
    mu_t, q_t = ref.weighted_moments(theta, m0, lw)
    m, mu_w, s2_w = ref.current_moments(a, b, m0, mu_t, q_t, S)
    x = a + b * theta
    sw = w.sum()
    direct_mu = (w[:, None] * x).sum(axis=0) / sw
    direct_s2 = (w[:, None] * (x - direct_mu) ** 2).sum(axis=0) / sw * S / (S - 1)
    tol_mu = S * 2.0**-52 * (w[:, None] * np.abs(x)).sum(axis=0) + S * 2.0**-52 * np.abs(a)
    tol_s2 = S * 2.0**-52 * ((w[:, None] * (b * (theta - m0)) ** 2).sum(axis=0) + (b * (mu_t - m0)) ** 2) * S / (S - 1)
    assert np.all(np.abs(mu_w - direct_mu) <= tol_mu), np.abs(mu_w - direct_mu) / tol_mu
    assert np.all(np.abs(s2_w - direct_s2) <= tol_s2), np.abs(s2_w - direct_s2) / tol_s2
    assert np.all(np.abs(m - x.mean(axis=0)) <= S * 2.0**-52 * np.abs(x).mean(axis=0))
    # T1 then T2 compose to a diagonal-affine map whose sample has the weighted mean and variance it was asked for
    v0 = theta.var(axis=0, ddof=1)
    a2, b2 = ref.candidate(ref.T2, a, b, m0, v0, mu_t, q_t, S)
    x2 = a2 + b2 * theta
    assert np.allclose(x2.mean(axis=0), mu_w, rtol=1e-12, atol=1e-12) and np.allclose(x2.var(axis=0, ddof=1), s2_w, rtol=1e-11)
    a1, b1 = ref.candidate(ref.T1, a, b, m0, v0, mu_t, q_t, S)
    assert np.array_equal(b1, b) and np.allclose((a1 + b1 * theta).mean(axis=0), mu_w, rtol=1e-12, atol=1e-12)


def test_the_exact_inverse_undoes_the_map():
    rng = np.random.default_rng(11)
    theta = rng.standard_normal((4000, 9)) * 10.0 ** rng.integers(-3, 4, 9)
    a, b = rng.uniform(-3, 3, 9) * 0, rng.uniform(0.5, 2, 9)
    back = ref.inverse(a + b * theta, a, b)
    assert np.all(np.abs(back - theta) <= 4 * np.spacing(np.abs(theta)))
    # with a shift the sum a + b theta is rounded at the size of a + b theta: 4 ulp of max(|theta|, |a / b|, |x / b|)
    a = rng.uniform(-3, 3, 9)
    x = a + b * theta
    back = ref.inverse(x, a, b)
    scale = np.maximum(np.abs(theta), np.maximum(np.abs(a / b), np.abs(x / b)))
    assert np.all(np.abs(back - theta) <= 4 * np.spacing(scale))
