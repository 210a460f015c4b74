"""ADVI's host rules and its reference, without a GPU.

csrc/potus_advi_rules.hpp states the step-size selection and the main run's stop for potus_advi's host code; it compiles with a plain C++
compiler.  A stand-alone program drives both rules on the ELBO sequences below and prints what they decide; that must be exactly what
tests/advi_ref.py -- the restatement the GPU tests check the device against -- decides on the same numbers.  Then the reference itself: on a
diagonal Gaussian target mean-field ADVI is exact, so it must recover the target's mean and standard deviations."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import advi_ref as ref

ROOT = Path(__file__).resolve().parent.parent
INF = math.inf

PROGRAM = r"""
#include "potus_advi_rules.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
static double num(const char *s) { return !strcmp(s, "-inf") ? -INFINITY : !strcmp(s, "inf") ? INFINITY : !strcmp(s, "nan") ? NAN : atof(s); }
// pick elbo_init e0 .. e4                      -> "index seen"
// conv iter eval_elbo tol e(1) e(2) ...        -> per evaluation "t code flags delta mean median" until a code is set
int main(int argc, char **argv) {
  if (argc >= 8 && !strcmp(argv[1], "pick")) {
    double c[ADVI_N_ETA];
    for (int k = 0; k < ADVI_N_ETA; k++) c[k] = num(argv[3 + k]);
    int seen = 0;
    const int pick = advi_pick_eta(num(argv[2]), c, &seen);
    printf("%d %d\n", pick, seen);
    return 0;
  }
  if (argc >= 5 && !strcmp(argv[1], "conv")) {
    const int iter = atoi(argv[2]), eval_elbo = atoi(argv[3]);
    const double tol = atof(argv[4]);
    AdviConv cv(iter, eval_elbo);
    int flags = 0;
    for (int a = 5, t = eval_elbo; a < argc; a++, t += eval_elbo) {
      const int code = cv.push(num(argv[a]), t, iter, eval_elbo, tol, &flags);
      printf("%d %d %d %.17g %.17g %.17g\n", t, code, flags, cv.delta, cv.mean, cv.median);
      if (code) break;
    }
    return 0;
  }
  return 2;
}
"""

# (elbo_init, the five candidates): what each case is there for
PICKS = {
    "minus_inf_first": (-60000.0, (-INF, -79234.0, -52275.0, -52643.0, -58000.0)),      # the issue's full-variant numbers: eta* = 1, stop at the fourth
    "maximum_in_the_middle": (-100.0, (-90.0, -50.0, -20.0, -30.0, -10.0)),             # stops at -30: the later -10 is never seen
    "monotone_to_the_last": (-100.0, (-90.0, -80.0, -70.0, -60.0, -50.0)),
    "all_below_init": (-10.0, (-90.0, -80.0, -70.0, -60.0, -50.0)),                     # ADAPT_FAILED
    "all_minus_inf": (-10.0, (-INF, -INF, -INF, -INF, -INF)),                           # ADAPT_FAILED, nothing ever chosen
    "last_equals_init": (-50.0, (-90.0, -80.0, -70.0, -60.0, -50.0)),                   # <= elbo_init fails
    "best_below_init_goes_on": (-10.0, (-50.0, -60.0, -70.0, -5.0, -6.0)),              # a drop while best <= elbo_init does not stop the search
    "first_is_best": (-100.0, (-20.0, -30.0, -5.0, -1.0, -1.0)),                        # stops at the second
}
# (iter, eval_elbo, tol, the ELBOs at t = eval_elbo, 2 eval_elbo, ...)
CONVS = {
    "buffer_2_mean": (2000, 100, 0.01, (-52000.0, -51980.0, -51965.0, -51960.0)),                         # delta = 1, 4e-4, 3e-4: MEAN at t = 300
    "buffer_2_maxit": (300, 100, 1e-9, (-5.0, -4.0, -3.5)),                                                # nothing converges: MAXIT at t = iter
    "buffer_10_median_first": (10000, 100, 0.01, (-100.0, -100.5, -100.2, -100.4, -100.3, -100.35, -100.3)),  # the 1 keeps the mean up: MEDIAN
    "buffer_10_rolls_over": (10000, 100, 1e-12, tuple(-1000.0 + 50.0 * math.sin(k) for k in range(14))),  # more pushes than entries
    "diverging_flag": (3000, 100, 1e-9, tuple(-(10.0 ** (k % 2)) * 7.0 for k in range(13))),              # big swings beyond t = 10 eval_elbo
    "minus_inf_after_finite": (2000, 100, 0.01, (-5.0, -INF, -5.0, -5.0, -5.0)),                          # NaN differences fire no rule
}


def fmt(x):
    return "-inf" if x == -INF else "inf" if x == INF else repr(float(x))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile potus_advi_rules.hpp on its own"
    tmp = tmp_path_factory.mktemp("advi_rules")
    (tmp / "advi_main.cpp").write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "us_potus_model_amd" / "csrc"), str(tmp / "advi_main.cpp"),
                    "-o", str(tmp / "advi_main")], check=True)
    return lambda *a: subprocess.run([str(tmp / "advi_main"), *a], check=True, capture_output=True, text=True).stdout.splitlines()


@pytest.mark.parametrize("name", sorted(PICKS))
def test_step_size_choice_is_the_reference_s(program, name):
    e0, cand = PICKS[name]
    got = tuple(int(v) for v in program("pick", fmt(e0), *[fmt(c) for c in cand])[0].split())
    assert got == ref.pick_eta(e0, cand)


def test_the_step_size_cases_cover_what_they_are_meant_to():
    want = dict(minus_inf_first=(2, 4), maximum_in_the_middle=(2, 4), monotone_to_the_last=(4, 5), all_below_init=(-1, 5), all_minus_inf=(-1, 5),
                last_equals_init=(-1, 5), best_below_init_goes_on=(3, 5), first_is_best=(0, 2))
    assert {k: ref.pick_eta(*v) for k, v in PICKS.items()} == want


def _ref_conv(iter, eval_elbo, tol, elbos):
    cv, rows = ref.Conv(iter, eval_elbo, tol), []
    for k, e in enumerate(elbos):
        t = (k + 1) * eval_elbo
        code = cv.push(e, t)
        rows.append((t, code, cv.flags, cv.delta, cv.mean, cv.median))
        if code:
            break
    return rows


@pytest.mark.parametrize("name", sorted(CONVS))
def test_the_stop_is_the_reference_s(program, name):
    iter, eval_elbo, tol, elbos = CONVS[name]
    got = [ln.split() for ln in program("conv", str(iter), str(eval_elbo), repr(tol), *[fmt(e) for e in elbos])]
    want = _ref_conv(iter, eval_elbo, tol, elbos)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert tuple(int(v) for v in g[:3]) == w[:3], (g, w)
        for a, b in zip(g[3:], w[3:]):                        # the same IEEE operations in the same order: equal, or NaN on both sides
            assert float(a) == b or (math.isnan(float(a)) and math.isnan(b)), (g, w)


def test_the_stop_cases_cover_what_they_are_meant_to():
    r = {k: _ref_conv(*v) for k, v in CONVS.items()}
    assert ref.Conv(2000, 100, 0.01).cap == 2 and ref.Conv(10000, 100, 0.01).cap == 10 and ref.Conv(100, 100, 0.01).cap == 2
    assert r["buffer_2_mean"][0][3] == 1.0 and all(v[0][3] == 1.0 for v in r.values())                  # the first delta is 1
    assert [(t, c) for t, c, *_ in r["buffer_2_mean"]] == [(100, 0), (200, 0), (300, ref.MEAN_CONVERGED)]
    assert r["buffer_2_maxit"][-1][:2] == (300, ref.MAXIT)
    last = r["buffer_10_median_first"][-1]
    assert last[1] == ref.MEDIAN_CONVERGED and last[4] >= 0.01 > last[5]                                # median before the mean
    assert len(r["buffer_10_rolls_over"]) == 14 and r["buffer_10_rolls_over"][-1][1] == 0
    assert r["diverging_flag"][9][2] == 0 and r["diverging_flag"][10][2] == ref.FLAG_DIVERGING          # t = 1100 > 10 eval_elbo
    assert math.isnan(r["minus_inf_after_finite"][1][4]) and r["minus_inf_after_finite"][1][1] == 0
    assert r["minus_inf_after_finite"][-1][:2] == (500, ref.MEAN_CONVERGED)                              # once the NaNs have left the buffer
    # an even number of entries: the UPPER middle one
    cv = ref.Conv(2000, 100, 0.01)
    cv.push(-1.0, 100); cv.push(-2.0, 200)
    assert cv.buf == [1.0, 0.5] and cv.median == 1.0 and cv.mean == 0.75


def test_the_three_kernels_are_in_the_code_object_within_the_optimiser_s_budget():
    """scripts/kernel_resources.py on the built library: k_vi_sga, k_vi_elbo and k_vi_draws are there, and the track kernel -- the pass and one
    out-of-line call, as k_opt_lbfgs is -- spills no more vector registers and takes no more scratch than k_opt_lbfgs does."""
    import importlib.util
    import __graft_entry__ as g
    g.build()
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "scripts" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = {r["name"]: r for r in kr.resources(ROOT / "us_potus_model_amd" / "libpotus_hmc.so")}
    pick = lambda stem: next(v for k, v in res.items() if stem in k)
    sga, elbo, draws, opt = pick("k_vi_sga"), pick("k_vi_elbo"), pick("k_vi_draws"), pick("k_opt_lbfgs")
    assert int(sga["vspill"]) <= int(opt["vspill"]) and int(sga["scratch"]) <= int(opt["scratch"]), (sga, opt)
    assert int(draws["vspill"]) == 0 and int(draws["scratch"]) == 0 and int(elbo["vgpr"]) <= 256


def test_the_reference_recovers_a_diagonal_gaussian():
    """log p = -1/2 sum ((x - m) / sd)^2: q* = N(m, diag(sd^2)) exactly.  From omega = 0, with decaying steps and one gradient draw, mu comes
    within a few stochastic-gradient standard errors and omega within a few per cent."""
    D = 12
    rng = np.random.default_rng(5)
    m, sd = rng.uniform(-3.0, 3.0, D), np.exp(rng.uniform(-1.5, 1.0, D))
    lpg = lambda x: (float(-0.5 * (((x - m) / sd) ** 2).sum()), -(x - m) / sd ** 2)
    out = ref.run(lpg, np.zeros(D), ref.numpy_normals(11), iter=4000, grad_samples=5, elbo_samples=50, tol_rel_obj=1e-5, eval_elbo=200)
    assert out["code"] in (ref.MEAN_CONVERGED, ref.MEDIAN_CONVERGED, ref.MAXIT) and out["eta_index"] >= 0
    assert np.isfinite(out["elbo"][:out["iterations"] // 200 + 1]).all()
    assert np.abs((out["mu"] - m) / sd).max() < 0.15, (out["mu"] - m) / sd
    assert np.abs(out["omega"] - np.log(sd)).max() < 0.1, out["omega"] - np.log(sd)
    # the ELBO of the exact q is the log normaliser sum log sd + D/2 log 2 pi, whatever the draws: lp + entropy is constant in eps
    e = ref.elbo(lpg, m, np.log(sd), ref.numpy_normals(3), 0, 0, 7)
    # mean of -1/2 |eps|^2 over 7 draws + D/2 (1 + log 2 pi) + sum log sd
    eps = [ref.numpy_normals(3)(ref.STAGE_ELBO, k, 0, D) for k in range(7)]
    want = np.mean([-0.5 * (v * v).sum() for v in eps]) + 0.5 * D * (1.0 + ref.LOG_2PI) + np.log(sd).sum()
    assert abs(e - want) < 1e-12 * abs(want)
    # a start whose log density is not finite: INIT; a target that overflows at once: NONFINITE or ADAPT_FAILED, never an exception
    bad = ref.run(lambda x: (math.nan, np.zeros(D)), np.zeros(D), ref.numpy_normals(1), iter=100, elbo_samples=2)
    assert bad["code"] == ref.INIT
