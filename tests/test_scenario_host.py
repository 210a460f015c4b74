"""CPU tests of the scenario layer: the restatement (tests/scenario_ref.py) against brute force in exact rational arithmetic on tiny inputs,
the parsing of `given`, cor() on a zero variance, an Outcomes built from conditional counts, and the names of the new entry points in the
header, the R shim and sampler.EXPORTS."""
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import outcomes_ref
import scenario_ref as ref
from us_potus_model_amd import outcomes as oc, sampler, scenario as sc

ROOT = Path(__file__).resolve().parent.parent
INF = float("inf")


def test_new_names_are_declared_exported_and_wrapped():
    new = {"potus_scenario", "potus_scenario_device", "potus_scenario_timing", "potus_R_scenario"}
    hdr = (ROOT / "include" / "potus_hmc.h").read_text()
    assert new <= set(re.findall(r"\b(potus_[A-Za-z_0-9]+)\s*\(", hdr))
    assert new <= set(sampler.EXPORTS)
    r = (ROOT / "R" / "potus_sampling.R").read_text()
    assert '"potus_R_scenario"' in r and "potus_scenario <- function" in r
    L = sampler.load_library()
    assert all(hasattr(L, nm) for nm in new)
    import us_potus_model_amd as pkg
    assert pkg.scenario is sc and pkg.conditional_forecast is sc.scenario and pkg.scenario_of_block is sc.scenario_of_block and pkg.Scenario is sc.Scenario
    assert hasattr(sampler.Handle, "scenario") and hasattr(sampler.StanFit, "scenario")
    assert re.search(r"calls that pool all chains \([^)]*potus_scenario[^)]*\) refuse", hdr.replace("\n *", ""))


def test_timing_getter_refuses_a_null_output_by_its_own_name():
    import ctypes as C
    L = sampler.load_library()
    assert L.potus_scenario_timing(None) == 1              # POTUS_ERR_ARG: no device needed
    buf = C.create_string_buffer(512)
    L.potus_last_error(buf, 512)
    assert buf.value.decode().startswith("potus_scenario_timing:")


# ---- the restatement against brute force, exact
def _brute(ps, w, cond_day, lo, hi):
    """Every number as a Fraction of the float64 inputs: keep mask, mean and covariance of the S + 1 coordinates, no rounding anywhere."""
    nd, ndays, S = ps.shape
    fw = [Fraction(float(v)) for v in w]
    rows = [[[Fraction(float(v)) for v in ps[d, t]] for t in range(ndays)] for d in range(nd)]
    for d in range(nd):
        for t in range(ndays):
            rows[d][t].append(sum((fw[s] * rows[d][t][s] for s in range(S)), Fraction(0)))
    keep = []
    for d in range(nd):
        x = rows[d][cond_day]
        keep.append(lo is None or all((lo[k] == -INF or Fraction(float(lo[k])) < x[k]) and (hi[k] == INF or x[k] <= Fraction(float(hi[k])))
                                      for k in range(S + 1)))
    kept = [rows[d] for d in range(nd) if keep[d]]
    n = len(kept)
    mean = [[sum((r[t][c] for r in kept), Fraction(0)) / n for c in range(S + 1)] for t in range(ndays)] if n else None
    cov = None
    if n >= 2:
        cov = [[[sum(((r[t][i] - mean[t][i]) * (r[t][j] - mean[t][j]) for r in kept), Fraction(0)) / (n - 1) for j in range(S + 1)]
                for i in range(S + 1)] for t in range(ndays)]
    return keep, mean, cov


@pytest.mark.parametrize("seed,S,nd,ndays,cond", [(1, 3, 40, 2, "tight"), (2, 4, 25, 1, "loose"), (3, 2, 12, 3, None)])
def test_restatement_equals_brute_force(seed, S, nd, ndays, cond):
    rng = np.random.default_rng(seed)
    ps = rng.integers(0, 65, (nd, ndays, S)) / 64.0                      # a grid: every sum below is exact in float64 as well
    ps[::5, :, 0] = 0.5                                                   # draws exactly on the bound of "win" / "lose"
    w = (rng.multinomial(64 - S, np.full(S, 1.0 / S)) + 1) / 64.0
    lo = hi = None
    if cond:
        lo, hi = np.full(S + 1, -INF), np.full(S + 1, INF)
        lo[0] = 0.5
        if cond == "tight":
            hi[1] = 0.5
            lo[S], hi[S] = 0.375, 0.625
    cd = ndays - 1
    got = ref.scenario(ps, w, cd, lo, hi, ev=[3, 4, 5, 6][:S], ev_to_win=7)
    keep, mean, cov = _brute(ps, w, cd, lo, hi)
    assert list(got["keep"]) == keep and got["n_kept"] == sum(keep) and got["n_draws"] == nd
    assert 2 <= got["n_kept"] <= nd and (cond is None) == (got["n_kept"] == nd)
    if cond:                                                              # the half-open rule: a draw on lo is dropped
        assert not got["keep"][::5].any()
    assert np.array_equal(got["mean"], np.array([[float(v) for v in row] for row in mean]))      # exactly rounded on both sides
    c = np.array([[[float(v) for v in row] for row in day] for day in cov])
    assert np.abs(got["cov"] - c).max() <= 4 * 2.0 ** -53 * np.abs(c).max()
    assert np.array_equal(got["cov"], got["cov"].transpose(0, 2, 1))
    want = outcomes_ref.outcomes(ps[np.array(keep)], w, [3, 4, 5, 6][:S], 7)
    for k in ("ev_hist", "tipping", "joint"):
        assert np.array_equal(got[k], want[k]), k


def test_restatement_complementary_conditions_partition_the_draws():
    rng = np.random.default_rng(11)
    S, nd = 3, 200
    ps = rng.integers(0, 9, (nd, 1, S)) / 8.0
    w = np.array([0.25, 0.25, 0.5])
    lo, hi = np.full(S + 1, -INF), np.full(S + 1, INF)
    win, lose = lo.copy(), hi.copy()
    win[1] = 0.5
    lose[1] = 0.5
    a, b = ref.keep_mask(ps[:, 0], w, win, hi)[0], ref.keep_mask(ps[:, 0], w, lo, lose)[0]
    assert (a ^ b).all() and (ps[:, 0, 1] == 0.5).any()
    assert np.array_equal(a, ps[:, 0, 1] > 0.5)


def test_restatement_degenerate_keeps():
    ps = np.array([[[0.25, 0.75]], [[0.5, 0.5]], [[0.75, 0.25]]])
    w = [0.5, 0.5]
    none = ref.scenario(ps, w, 0, [0.9, -INF, -INF], [INF, INF, INF], ev=[1, 2], ev_to_win=2)
    assert none["n_kept"] == 0 and np.isnan(none["mean"]).all() and np.isnan(none["cov"]).all()
    assert not none["ev_hist"].any() and not none["tipping"].any() and not none["joint"].any()
    one = ref.scenario(ps, w, 0, [0.5, -INF, -INF], [INF, INF, INF])
    assert one["n_kept"] == 1 and np.array_equal(one["mean"], [[0.75, 0.25, 0.5]]) and np.isnan(one["cov"]).all()
    assert "joint" not in one


# ---- `given`
STATES = ["AL", "CA", "FL", "PA"]


def test_given_win_lose_interval_names_and_national():
    lo, hi = sc.parse_given({"FL": "win", "PA": "lose", "national": (0.48, 0.52), 0: (None, 0.4), 1: (0.6, None)}, 4, STATES)
    assert np.array_equal(lo, [-INF, 0.6, 0.5, -INF, 0.48]) and np.array_equal(hi, [0.4, INF, INF, 0.5, 0.52])
    assert lo.dtype == np.float64 and lo.flags.c_contiguous and hi.flags.c_contiguous
    assert sc.parse_given(None, 4) == (None, None) and sc.parse_given({}, 4, STATES) == (None, None)
    lo, hi = sc.parse_given({np.int64(3): "win"}, 4)
    assert lo[3] == 0.5 and np.isinf(hi).all()


@pytest.mark.parametrize("given,err", [
    ({"TX": "win"}, KeyError),                     # not a name of the list
    ({"FL": "win", 2: "lose"}, ValueError),        # the same coordinate twice
    ({4: "win"}, KeyError),                        # the national vote is "national", not index S
    ({-1: "win"}, KeyError),
    ({1.5: "win"}, KeyError),
    ({True: "win"}, KeyError),
    ({"FL": "tie"}, ValueError),
    ({"FL": 0.5}, ValueError),
    ({"FL": (0.6, 0.4)}, ValueError),              # lo >= hi
    ({"FL": (0.5, 0.5)}, ValueError),
    ({"FL": (float("nan"), 0.6)}, ValueError),
    ({"FL": (0.1, 0.2, 0.3)}, ValueError),
])
def test_given_refuses(given, err):
    with pytest.raises(err):
        sc.parse_given(given, 4, STATES)


def test_given_names_need_the_list():
    with pytest.raises(KeyError, match="no names"):
        sc.parse_given({"FL": "win"}, 4)
    assert sc.parse_given({"national": "win"}, 4)[0][4] == 0.5           # "national" needs none


# ---- the result object
def test_cor_on_a_zero_variance_is_nan_there_and_right_elsewhere():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(50, 3))
    x[:, 1] = 0.25                                                        # a coordinate that never moves
    cov = np.cov(x, rowvar=False)[None]
    s = sc.Scenario(50, 80, x.mean(0)[None], cov)
    r = s.cor()
    assert np.isnan(r[1]).all() and np.isnan(r[:, 1]).all()
    assert r[0, 0] == 1.0 and r[2, 2] == 1.0
    assert abs(r[0, 2] - np.corrcoef(x[:, 0], x[:, 2])[0, 1]) < 1e-15 and r[0, 2] == r[2, 0]
    assert np.array_equal(s.sd(), np.sqrt(np.diagonal(cov[0]))) and s.sd()[1] == 0.0
    assert s.probability == 50 / 80 and s.S == 2 and s.days == (0, 1)
    assert s.index("national") == 2 and s.index(1) == 1
    nan = sc.Scenario(0, 80, np.full((1, 3), np.nan), np.full((1, 3, 3), np.nan))
    assert nan.probability == 0.0 and np.isnan(nan.cor()).all()


def test_outcomes_of_conditional_counts_divide_by_the_kept_draws():
    rng = np.random.default_rng(21)
    S, nd = 3, 300
    ps = rng.integers(0, 65, (nd, 2, S)) / 64.0
    w, ev = np.array([0.25, 0.25, 0.5]), np.array([3, 4, 5])
    lo, hi = np.full(S + 1, -INF), np.full(S + 1, INF)
    lo[0] = 0.5
    r = ref.scenario(ps, w, 1, lo, hi, ev=ev, ev_to_win=7)
    n = r["n_kept"]
    assert 0 < n < nd
    o = oc.Outcomes(r["ev_hist"], r["tipping"], r["joint"], None, n, ev, 7, (0, 2))
    kept = ps[r["keep"]]
    dem = ((kept > 0.5) * ev).sum(2)
    assert np.array_equal(o.win_probability(), (dem >= 7).sum(0) / n)
    assert o.ev_distribution().sum() == pytest.approx(1.0) and o.n_draws == n
    assert o.conditional(0)[0] == 1.0                                     # the condition itself, on the condition day
    # ... and equals what potus_outcomes' conditional() says from the unconditional pair counts
    full = outcomes_ref.outcomes(ps, w, ev, 7)
    u = oc.Outcomes(full["ev_hist"], full["tipping"], full["joint"], None, nd, ev, 7, (0, 2))
    assert np.array_equal(np.diagonal(o.joint[1]) / n, u.conditional(0, day=1))
