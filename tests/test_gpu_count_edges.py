"""The counting and moment kernels at the edges of their batches (csrc/potus_outcomes.hpp, csrc/potus_scenario.hpp, oc_count and sc_compute in
csrc/potus_hmc.hip), through outcomes_of_block / potus_outcomes_device and scenario_of_block / potus_scenario_device on the blocks of
tests/count_edge_cases.py (tests/test_count_edges_host.py holds their structure: the items of the busiest wave, the blocks and scan rounds,
the slices, the kept counts and the planted keep patterns).

  A  the 64-item fold of k_oc_count   a wave with 63, 64, 65, 128 and 129 items, S = 3 and 63, one chunk and three
  B  k_sc_keep / k_sc_scan / k_sc_compact   one block, two, 64, 65 (a last block of one draw) and 130 blocks: one, two and three scan rounds
  C  the slices of k_sc_compact       rows of 511, 1024, 1025, 1537 and 32 900 doubles: 1, 2, 2, 3 and 64 slices
  D  chunk and step tails of the moments   2 .. 5, 15 .. 17, 1023 .. 1025, 2048, 2049 kept draws; S + 1 = 2, 3, 17, 32, 33, 49 coordinates
  E  non-finite scores                a NaN score is in no interval; +inf under hi = +inf is kept, -inf over lo = -inf is not
  F  the day-block loop of sc_compute POTUS_SCENARIO_SCRATCH_BUDGET set to one day and to two days of scratch: launches with day0 > 0

The tolerances are those of tests/test_gpu_scenario.py, with its own helpers: counts and n_kept EQUAL; means bit-equal (the scores lie on
the grid); covariances within 2 (n + 2) 2^-53 sqrt(v_i v_j) of the np.longdouble restatement and symmetric bit for bit.  Every call is made
twice and gives the same bytes; every case prints its worst covariance ratio before it asserts.

Measured on an MI355X (profiles/count_edges.txt): the worst covariance is 0.19 of its bound (three kept draws), 0.05 at most from 15 kept
draws on; the 41 cases take 5 s together after the first use of the device, none more than 0.9 s (S = 63 x 1025 days: a block of 133 MB).
The same file names what fails when the reset after the fold, the carry of the scan or the day of the mean is taken out of the kernels."""
import numpy as np
import pytest

import count_edge_cases as cases
from test_gpu_outcomes import KEYS, _assert_equal
from test_gpu_scenario import COUNTS, LOOSE, _assert_counts, _assert_cov, _bytes, _cov_bound
from us_potus_model_amd import outcomes as oc, scenario as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def _block(ps):
    import torch
    return torch.tensor(np.asarray(ps), device="cuda:0")


def _scenario_twice(ps, w, ev, given=None, day=-1):
    """scenario_of_block, twice on one device block: the same bytes"""
    blk = _block(ps)
    got = sc.scenario_of_block(blk, w, ev, given=given, day=day, ev_to_win=cases.W270)
    again = sc.scenario_of_block(blk, w, ev, given=given, day=day, ev_to_win=cases.W270)
    assert _bytes(again) == _bytes(got)
    return got


def _assert_scenario(got, want, what):
    _assert_counts(got, want, what)
    assert got.mean.tobytes() == want["mean"].tobytes(), (what, float(np.abs(got.mean - want["mean"]).max()))
    _assert_cov(got, want, what)


# ---------------------------------------------------------------------------------------------------- A. the fold of k_oc_count
@pytest.mark.parametrize("S,nd,n_days", cases.FOLD_CASES)
def test_fold_of_the_indicator_columns(S, nd, n_days):
    """A wave of k_oc_count keeps one bit per item and folds 64 of them into the workgroup's joint counts: the shift by k = 63, the reset, no
    remainder after an exact multiple, LDS counters that take a second and a third fold.  The fold feeds `joint` alone; the histogram, the
    tipping point and below_actual of the same items are compared with it."""
    chunks, chunk, busiest = cases.oc_chunks(nd, n_days)
    assert busiest == cases.FOLD_BUSIEST[nd] >= cases.OC_FOLD
    ps, w, ev, actual = cases.fold_case(S, nd, n_days)
    want = cases.fold_reference(S, nd, n_days)
    blk = _block(ps)
    got = oc.outcomes_of_block(blk, w, ev, actual=actual, ev_to_win=cases.W270)
    what = f"S={S} nd={nd} days={n_days}: {chunks} chunk(s) of {chunk}, busiest wave {busiest} items"
    print(what)
    _assert_equal(got, want, what)
    assert (np.diagonal(got.joint, axis1=1, axis2=2)[:, :S] <= nd).all() and (got.ev_hist.sum(1) == nd).all() and (got.tipping.sum(1) == nd).all()
    again = oc.outcomes_of_block(blk, w, ev, actual=actual, ev_to_win=cases.W270)
    assert all(getattr(got, k).tobytes() == getattr(again, k).tobytes() for k in KEYS)


# ---------------------------------------------------------------------------------------------------- B. keep, scan and compact
@pytest.mark.parametrize("nd", cases.SCAN_ND)
def test_keep_scan_and_compact_over_the_scan_rounds(nd):
    """ "State 0 wins" with the scores of state 0 set by hand: a first block that keeps nothing, a block that keeps all 256, a wave that keeps
    nothing inside a block that keeps others, a whole block of the second scan round that keeps nothing, and the last draw kept -- so the
    carry of k_sc_scan into its second and third round is not zero and the last block's first row is the last row."""
    nblk, rounds, last = cases.keep_blocks(nd)
    assert (nblk, rounds, last) == cases.SCAN_BLOCKS[nd]
    ps, w, ev, keep = cases.scan_case(nd)
    want = cases.scan_reference(nd)
    assert want["n_kept"] == int(keep.sum())
    got = _scenario_twice(ps, w, ev, cases.SCAN_GIVEN)
    _assert_scenario(got, want, f"nd={nd}: {nblk} blocks, {rounds} scan round(s), last block {last}")
    assert np.array_equal(got.mean[0, :cases.SCAN_S], ps[keep, 0].sum(0) / want["n_kept"])      # the rows that were copied are the kept ones


# ---------------------------------------------------------------------------------------------------- C. the slices of k_sc_compact
@pytest.mark.parametrize("n_days,S", cases.SLICE_CASES)
def test_compaction_in_slices_of_a_row(n_days, S):
    """Compaction shows in every output: the means (bit-equal) and the counts of the kept draws, every day."""
    rowlen, slices = cases.SLICE_ROWLEN[(n_days, S)]
    assert cases.compact_slices(n_days * S)[0] == slices
    ps, w, ev = cases.slice_case(n_days, S)
    want = cases.slice_reference(n_days, S)
    got = _scenario_twice(ps, w, ev, LOOSE)
    what = f"days={n_days} S={S}: rows of {rowlen} doubles in {slices} slice(s), kept {want['n_kept']} of {cases.SLICE_ND}"
    print(what)
    _assert_counts(got, want, what)
    assert got.mean.tobytes() == want["mean"].tobytes(), (what, float(np.abs(got.mean - want["mean"]).max()))
    assert np.array_equal(got.cov, got.cov.transpose(0, 2, 1)) and np.isfinite(got.cov).all()


# ---------------------------------------------------------------------------------------------------- D. chunk and step tails of the moments
@pytest.mark.parametrize("nd", cases.TAIL_ND)
def test_moment_tails_without_a_condition(nd):
    ps, w, ev = cases.tail_case(nd)
    want = cases.tail_reference(nd)
    assert want["n_kept"] == nd
    got = _scenario_twice(ps, w, ev)
    _assert_scenario(got, want, f"S={cases.TAIL_S} n_kept={nd}")


@pytest.mark.parametrize("n_kept", cases.TAIL_KEPT)
def test_a_chunk_edge_behind_a_compaction(n_kept):
    ps, w, ev, keep = cases.tail_kept_case(n_kept)
    want = cases.tail_kept_reference(n_kept)
    assert want["n_kept"] == n_kept
    got = _scenario_twice(ps, w, ev, cases.SCAN_GIVEN)
    _assert_scenario(got, want, f"S={cases.TAIL_S} kept {n_kept} of {cases.TAIL_KEPT_ND}")


@pytest.mark.parametrize("S", cases.TRIPLE_S)
def test_coordinate_counts_at_the_operand_tile_edges(S):
    """S + 1 = 2, 3, 17, 32, 33, 49 coordinates: at 17, 33 and 49 the national column sits alone in its operand tile of k_sc_gram."""
    ps, w, ev = cases.triple_case(S)
    for name, given in cases.triple_givens(S):
        want = cases.triple_reference(S, name)
        assert want["n_kept"] >= 2
        got = _scenario_twice(ps, w, ev, given)
        _assert_scenario(got, want, f"S={S} nd={cases.TRIPLE_ND} days={cases.TRIPLE_DAYS} {name}")


# ---------------------------------------------------------------------------------------------------- E. non-finite scores
def _assert_cov_where_finite(got, want, what):
    """NaN in exactly the restatement's entries; everything else within the bound of _assert_cov"""
    nan = np.isnan(want["cov"])
    assert np.array_equal(np.isnan(got.cov), nan), what
    with np.errstate(invalid="ignore"):
        err, bound = np.abs(got.cov - want["cov"]), _cov_bound(want)
    assert np.isfinite(bound[~nan]).all() and (bound[~nan] > 0).all()
    print(f"{what}: n_kept {want['n_kept']}, {int(nan.sum())} NaN entries, max |cov - ref| / bound elsewhere {float((err[~nan] / bound[~nan]).max()):.3f}")
    assert (err[~nan] <= bound[~nan]).all(), what
    assert np.array_equal(got.cov, got.cov.transpose(0, 2, 1), equal_nan=True), what


def test_non_finite_scores_under_a_condition():
    """On the condition day: a NaN in a conditioned state and a NaN in a free state drop their draws (a NaN score is in no interval), +inf in a
    state bounded by hi = +inf keeps its draw, -inf in a state bounded by lo = -inf drops it.  The kept set is the restatement's: n_kept,
    the counts, and the means of the kept draws (+inf in the coordinate of the kept infinite score and in the national vote)."""
    cond, _, w, ev = cases.nonfinite_case()
    want = cases.nonfinite_reference(True)
    got = _scenario_twice(cond, w, ev, cases.NF_GIVEN, day=cases.NF_COND_DAY)
    _assert_counts(got, want, "non-finite, conditioned")
    assert np.array_equal(got.mean, want["mean"]) and np.isinf(got.mean).sum() == 2
    _assert_cov_where_finite(got, want, "non-finite, conditioned")


def test_one_nan_score_without_a_condition():
    """One NaN on the other day: mean and covariance are NaN in that coordinate's and the national vote's row and column on that day only;
    every other entry stays within the bound; the counts are equal (the NaN state is not won, and the tipping point does not hang on it)."""
    _, free, w, ev = cases.nonfinite_case()
    want = cases.nonfinite_reference(False)
    got = _scenario_twice(free, w, ev, None, day=cases.NF_COND_DAY)
    _assert_counts(got, want, "one NaN, no condition")
    assert np.array_equal(np.isnan(got.mean), np.isnan(want["mean"])) and np.isnan(got.mean).sum() == 2
    assert np.array_equal(got.mean, want["mean"], equal_nan=True)
    _assert_cov_where_finite(got, want, "one NaN, no condition")
    o = oc.outcomes_of_block(_block(free), w, ev, ev_to_win=cases.W270)
    for k in COUNTS:
        assert np.array_equal(getattr(got.outcomes, k), getattr(o, k)), k


# ---------------------------------------------------------------------------------------------------- F. the day blocks of sc_compute
def test_day_blocks_give_the_bytes_of_the_unsplit_call(monkeypatch):
    """S = 33, five days, 1500 draws under the loose condition.  With the scratch budget at one day and at two days of scratch the moments
    run in launches of 1, 1, 1, 1, 1 and of 2, 2, 1 days: nat, psum and pcov are indexed by the launch-local day, x, mean and cov by the
    global one.  Both give the bytes of the unsplit call, which agrees with the restatement."""
    monkeypatch.delenv("POTUS_SCENARIO_SCRATCH_BUDGET", raising=False)
    ps, w, ev = cases.dayblock_case()
    want = cases.dayblock_reference()
    per_day = cases.scratch_per_day(want["n_kept"], cases.DAYBLOCK_S)
    whole = _scenario_twice(ps, w, ev, LOOSE)
    _assert_scenario(whole, want, f"S={cases.DAYBLOCK_S} days={cases.DAYBLOCK_DAYS} unsplit")
    for budget, launches in ((per_day, [1, 1, 1, 1, 1]), (2 * per_day, [2, 2, 1])):
        assert cases.day_blocks(cases.DAYBLOCK_DAYS, per_day, budget) == launches
        monkeypatch.setenv("POTUS_SCENARIO_SCRATCH_BUDGET", str(budget))
        split = _scenario_twice(ps, w, ev, LOOSE)
        assert split.n_kept == whole.n_kept and split.mean.tobytes() == whole.mean.tobytes(), launches
        assert split.cov.tobytes() == whole.cov.tobytes(), (launches, float(np.abs(split.cov - whole.cov).max()))
        assert _bytes(split) == _bytes(whole), launches
