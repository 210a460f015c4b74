"""The machinery of tests/test_gpu_count_edges.py without a GPU (tests/count_edge_cases.py): the constants and the restated launch rules
(oc_count's chunks, k_sc_compact's slices, sc_compute's scratch per day and day blocks) against the text of csrc/potus_outcomes.hpp,
csrc/potus_scenario.hpp and csrc/potus_hmc.hip; the structure every case is there for -- items of the busiest wave, blocks and scan rounds,
slices, kept counts, the planted keep pattern -- on the restatement's own numbers; the vectorised restatement of the counts and the fast
restatement of a scenario against the literal ones; scenario_ref.keep_mask on the non-finite scores against a direct numpy statement; and
that no shape of the existing GPU tests gives a wave of k_oc_count 64 items, which is why the fold in its loop needed cases of its own."""
import numpy as np
import pytest

import count_edge_cases as cases
import outcomes_ref
import scenario_ref as ref
import test_gpu_outcomes
import test_gpu_scenario
from conftest import ROOT

CSRC = ROOT / "us_potus_model_amd" / "csrc"
INF = float("inf")


def _sources():
    return (CSRC / "potus_outcomes.hpp").read_text(), (CSRC / "potus_scenario.hpp").read_text(), (CSRC / "potus_hmc.hip").read_text()


def test_the_constants_are_the_headers():
    oc, sc, hip = _sources()
    for text, lines in ((oc, (f"#define OC_THREADS {cases.OC_THREADS}", "#define OC_WAVES (OC_THREADS / 64)", f"#define OC_MAX_S {cases.OC_MAX_S} ")),
                        (sc, (f"#define SC_THREADS {cases.SC_THREADS}", f"#define SC_KEEP_BLOCK {cases.SC_KEEP_BLOCK} ", f"#define SC_CHUNK {cases.SC_CHUNK} "))):
        for ln in lines:
            assert text.count(ln) == 1, ln
    assert cases.OC_WAVES == 4 and cases.SC_KEEP_BLOCK == cases.SC_THREADS
    # the fold, the deal of a chunk's draws to the waves, the scan rounds, the steps of the Gram matrix
    assert oc.count(f"if (++k == {cases.OC_FOLD}) {{ oc_fold(s_joint, lane, S, col, colE, colP); col = colE = colP = 0ull; k = 0; }}") == 1
    assert "if (k) oc_fold(s_joint, lane, S, col, colE, colP);" in oc and "for (; d < d1; d += OC_WAVES) {" in oc and "long long d = d0 + wave;" in oc
    assert f"for (long long base = 0; base < nblk; base += {cases.SC_SCAN_ROUND}) {{" in sc
    assert "if (base + lane < nblk) first[base + lane] = (long long)(carry + inc - c);" in sc
    assert "const long long e0 = rowlen * blockIdx.y / gridDim.y, e1 = rowlen * (blockIdx.y + 1) / gridDim.y;" in sc
    assert "long long b = d0 + 4 * wave;" in sc and "for (; b < d1; b += 4 * SC_WAVES) {" in sc
    # the launch code
    assert "const long long nblk = (nd + SC_KEEP_BLOCK - 1) / SC_KEEP_BLOCK;" in hip
    assert f"const unsigned slices = (unsigned)std::min<long long>(std::max<long long>(1, rowlen / {cases.SC_SLICE}), {cases.SC_MAX_SLICES});" in hip
    assert "constexpr size_t SC_SCRATCH_BUDGET = (size_t)256 << 20;" in hip and cases.SC_SCRATCH_BUDGET == 256 * 1024 * 1024
    assert "const int nchunks = (int)((n + SC_CHUNK - 1) / SC_CHUNK);" in hip
    assert "const size_t per_day = ((size_t)n + (size_t)nchunks * (C + (want_cov ? (size_t)C * C : 0))) * 8;" in hip
    assert 'if (const char *e = getenv("POTUS_SCENARIO_SCRATCH_BUDGET")) budget = std::max<size_t>(1, (size_t)atoll(e));' in hip
    assert "const int dblk = (int)std::min<size_t>((size_t)n_days, std::max<size_t>(1, budget / per_day));" in hip
    assert "POTUS_SCENARIO_SCRATCH_BUDGET" in (ROOT / "DESIGN.md").read_text()


def test_the_chunk_rule_is_oc_counts():
    hip = _sources()[2]
    at = hip.index(f"long long chunks = std::min<long long>(std::max(1, {cases.OC_WORKGROUPS} / n_days), (nd + 63) / 64);")
    body = [ln.strip() for ln in hip[at:].splitlines()[:4]]
    assert body[1:] == ["chunks = std::max(chunks, (nd + (1ll << 30) - 1) >> 30);", "const long long chunk = (nd + chunks - 1) / chunks;",
                        "chunks = (nd + chunk - 1) / chunk;"]
    # the busiest wave is wave 0 of a full chunk: against the deal itself, over every chunk and wave
    rng = np.random.default_rng(1)
    for nd, n_days in [(1, 1), (63, 1), (64, 1), (65, 1), (770, 600), (8000, 254), (513, 1025), (100000, 3)] + [tuple(int(v) for v in rng.integers(1, 3000, 2)) for _ in range(200)]:
        chunks, chunk, busiest = cases.oc_chunks(nd, n_days)
        sizes = [min(chunk, nd - c * chunk) for c in range(chunks)]
        assert sum(sizes) == nd and min(sizes) >= 1 and chunks * n_days <= max(cases.OC_WORKGROUPS, n_days)
        assert busiest == max(max(cases.wave_items(s)) for s in sizes), (nd, n_days)
    assert cases.oc_chunks(8000, 254) == (8, 1000, 250)                  # the 2016 run over all days: three folds and a remainder
    assert cases.oc_chunks((1 << 31) + 5, 2048)[0] == 3                  # a workgroup's counters have 32 bits


def _existing_shapes():
    """(draws the counting kernel is handed, days) of the built blocks and fits of tests/test_gpu_outcomes.py and tests/test_gpu_scenario.py"""
    out = [(nd, ndays) for _, nd, ndays, _, _ in test_gpu_outcomes.test_built_blocks_equal_the_restatement.pytestmark[0].args[1]]
    out += [(20011, 1), (600, 254), (160, 254), (320, 254), (100, 254), (20, 254)]      # test_more_than_16384_draws; chains x draws of the fits, at the most days any design has
    for (_, nd, ndays), kept in test_gpu_scenario.KEPT.items():
        out += [(n, ndays) for n in (nd,) + tuple(kept)]
    out += [(300, 2), (700, 2), (1, 2), (1500, 3)]
    return out


def test_no_existing_shape_reaches_the_fold():
    table = {(1000, 1): 16, (777, 5): 15, (37, 254): 10, (20011, 1): 16, (4099, 2): 16, (600, 254): 19}
    shapes = _existing_shapes()
    assert set(table) <= set(shapes)
    for nd, n_days in shapes:
        busiest = cases.oc_chunks(nd, n_days)[2]
        assert busiest < cases.OC_FOLD, (nd, n_days, busiest)
        assert table.get((nd, n_days), busiest) == busiest, (nd, n_days, busiest)
    # neither do the built scenario blocks reach a second scan round (17 blocks at the most), a second slice (rows of 255 doubles) or a second launch
    assert max(cases.keep_blocks(nd)[0] for _, nd, _ in test_gpu_scenario.KEPT) == 17
    assert max(cases.compact_slices(ndays * S)[0] for S, _, ndays in test_gpu_scenario.KEPT) == 1
    assert max(ndays * cases.scratch_per_day(nd, S) for S, nd, ndays in test_gpu_scenario.KEPT) < cases.SC_SCRATCH_BUDGET // 1000


def test_fold_cases_reach_what_they_are_there_for():
    assert [c[1] for c in cases.FOLD_CASES] == [255, 256, 257, 512, 513, 257, 770] and max(c[0] for c in cases.FOLD_CASES) == cases.OC_MAX_S
    for S, nd, n_days in cases.FOLD_CASES:
        chunks, chunk, busiest = cases.oc_chunks(nd, n_days)
        assert busiest == cases.FOLD_BUSIEST[nd] >= cases.OC_FOLD
        if n_days == cases.FOLD_DAYS:
            assert 1025 <= n_days <= 2048 and (chunks, chunk) == (1, nd)
    assert cases.wave_items(255) == [64, 64, 64, 63] and cases.wave_items(256) == [64] * 4 and cases.wave_items(257) == [65, 64, 64, 64]
    assert cases.wave_items(512) == [128] * 4 and cases.wave_items(513) == [129, 128, 128, 128]
    chunks, chunk, _ = cases.oc_chunks(770, 600)
    assert (chunks, chunk) == (3, 257) and [min(chunk, 770 - c * chunk) for c in range(chunks)] == [257, 257, 256]
    S, nd, n_days = cases.FOLD_CASES[2]
    ps, w, ev, actual = cases.fold_case(S, nd, n_days)
    assert ps.shape == (nd, n_days, S) and not ps.flags.writeable and w.sum() == 1.0 and ev.sum() == 538
    assert np.array_equal(ps * 1024, np.round(ps * 1024)) and np.array_equal(actual * 1024, np.round(actual * 1024))


def test_the_vectorised_counts_are_the_literal_ones_on_a_fold_case():
    """the GPU test takes outcomes_vectorised for the cases of a thousand days: 257 draws x 1025 days x 3 states, `actual` included"""
    S, nd, n_days = cases.FOLD_CASES[2]
    ps, w, ev, actual = cases.fold_case(S, nd, n_days)
    fast, literal = cases.fold_reference(S, nd, n_days), outcomes_ref.outcomes(ps, w, ev, cases.W270, actual)
    for k in ("ev_hist", "tipping", "joint", "below_actual"):
        assert fast[k].dtype == np.int64 and np.array_equal(fast[k], literal[k]), k
    assert (literal["nat"] == 0.5).any() and fast["below_actual"].any() and (fast["joint"][:, S, S] > 0).all()


@pytest.mark.parametrize("nd", cases.SCAN_ND)
def test_scan_cases_hold_the_planted_pattern(nd):
    B = cases.SC_KEEP_BLOCK
    ps, w, ev, planted = cases.scan_case(nd)
    want = cases.scan_reference(nd)
    keep = want["keep"]
    assert np.array_equal(keep, planted) and want["n_kept"] == int(planted.sum())
    nblk, rounds, last = cases.keep_blocks(nd)
    assert (nblk, rounds, last) == cases.SCAN_BLOCKS[nd]
    counts = [int(keep[b * B:(b + 1) * B].sum()) for b in range(nblk)]
    assert keep[nd - 1] and 0 < want["n_kept"] < nd                       # the last kept draw is the last draw; there is something to compact
    wb = cases.idle_wave_block(nd)
    assert not keep[wb * B + 128:wb * B + 192].any() and counts[wb] > 0   # a wave that keeps nothing inside a block that keeps others
    if nblk >= 3:
        assert counts[0] == 0 and counts[1] == B                          # the first block keeps nothing, one block keeps all
    if rounds >= 2:
        assert sum(counts[:cases.SC_SCAN_ROUND]) > 0                      # the carry into the second round is not zero
    if nblk > cases.SCAN_EMPTY_BLOCK:
        assert cases.SC_SCAN_ROUND <= cases.SCAN_EMPTY_BLOCK < 2 * cases.SC_SCAN_ROUND and counts[cases.SCAN_EMPTY_BLOCK] == 0
        assert sum(counts[2 * cases.SC_SCAN_ROUND:]) > 0                  # and the third round places draws
    x0 = ps[:, 0, 0]
    assert (x0[~keep] == 0.5).any() and (x0[~keep] < 0.5).any() and (x0[keep] > 0.5).all()       # a draw on the bound is not kept
    assert (np.diagonal(want["cov"], axis1=1, axis2=2) > 0).all()                                # no coordinate of the kept draws is constant


def test_slice_cases_cut_their_rows_as_stated():
    for n_days, S in cases.SLICE_CASES:
        rowlen, slices = cases.SLICE_ROWLEN[(n_days, S)]
        n, cuts = cases.compact_slices(rowlen)
        assert n_days * S == rowlen and n == slices and cuts[0][0] == 0 and cuts[-1][1] == rowlen
        assert all(a[1] == b[0] for a, b in zip(cuts, cuts[1:])) and all(e1 > e0 for e0, e1 in cuts)
        want = cases.slice_reference(n_days, S)
        assert 0.35 < want["n_kept"] / cases.SLICE_ND < 0.65, want["n_kept"]
    assert [cases.SLICE_ROWLEN[c][0] for c in cases.SLICE_CASES] == [511, 1024, 1025, 1537, 32900]
    assert cases.compact_slices(1537)[1] == [(0, 512), (512, 1024), (1024, 1537)]                # a row length that is no multiple of the slice count
    assert cases.compact_slices(32900)[0] == cases.SC_MAX_SLICES and 32900 >= 32768 and 32900 % 64 != 0


def test_tail_cases_have_the_kept_counts_they_name():
    C4, W = cases.SC_CHUNK, 4
    assert set(cases.TAIL_ND) == {2, 3, 4, 5, 4 * W - 1, 4 * W, 4 * W + 1, C4 - 1, C4, C4 + 1, 2 * C4, 2 * C4 + 1}
    for nd in cases.TAIL_ND:
        want = cases.tail_reference(nd)
        assert want["n_kept"] == nd and want["mean"].shape == (cases.TAIL_DAYS, cases.TAIL_S + 1)
        v = np.diagonal(want["cov"], axis1=1, axis2=2)
        assert (v > 0).all(), nd                                         # no coordinate is constant: every bound is positive
    for n in cases.TAIL_KEPT:
        ps, w, ev, keep = cases.tail_kept_case(n)
        want = cases.tail_kept_reference(n)
        assert want["n_kept"] == n == int(keep.sum()) and np.array_equal(want["keep"], keep) and len(ps) == cases.TAIL_KEPT_ND
        assert (np.diagonal(want["cov"], axis1=1, axis2=2) > 0).all()
    assert {S + 1 for S in cases.TRIPLE_S} == {2, 3, 17, 32, 33, 49} and [(S + 1) % 16 for S in (16, 32, 48)] == [1, 1, 1]
    for S in cases.TRIPLE_S:
        givens = dict(cases.triple_givens(S))
        assert set(givens) == {"tight", "loose", "none"} and (set(givens["tight"]) == {0, 1, "national"} if S > 1 else set(givens["tight"]) == {0, "national"})
        kept = {name: cases.triple_reference(S, name)["n_kept"] for name in givens}
        print(f"S = {S}: kept {kept}")
        assert 2 <= kept["tight"] < kept["loose"] < kept["none"] == cases.TRIPLE_ND, (S, kept)


def test_the_fast_restatement_is_the_literal_one():
    for ps, w, ev, cond_day, given in ((*cases.scan_case(257)[:3], 0, cases.SCAN_GIVEN), (*cases.triple_case(16), 2, test_gpu_scenario.TIGHT),
                                       (*cases.tail_case(17), 1, None)):
        lo, hi = cases.bounds(given, ps.shape[2])
        fast, literal = cases.restate(ps, w, cond_day, lo, hi, ev=ev), ref.scenario(ps, w, cond_day, lo, hi, ev=ev)
        assert fast["n_kept"] == literal["n_kept"] and np.array_equal(fast["keep"], literal["keep"])
        for k in ("ev_hist", "tipping", "joint", "nat", "mean", "cov"):
            assert fast[k].tobytes() == literal[k].tobytes(), k
        assert cases.restate(ps, w, cond_day, lo, hi, ev=ev, want_cov=False)["mean"].tobytes() == literal["mean"].tobytes()


def test_keep_mask_on_non_finite_scores_is_the_direct_statement():
    cond, free, w, ev = cases.nonfinite_case()
    S = cases.NF_S
    lo, hi = cases.bounds(cases.NF_GIVEN, S)
    assert lo.tolist() == [0.5, 0.25, -INF, -INF, -INF, -INF] and hi.tolist() == [INF, INF, 0.75, INF, INF, INF]
    want = cases.nonfinite_reference(True)
    x = cond[:, cases.NF_COND_DAY]
    with np.errstate(invalid="ignore"):
        xn = np.concatenate([x, (x * w[None, :]).sum(axis=1)[:, None]], axis=1)
        direct = np.array([all(lo[k] < row[k] <= hi[k] for k in range(S + 1)) for row in xn])
    assert np.array_equal(want["keep"], direct) and np.array_equal(ref.keep_mask(x, w, lo, hi)[0], direct)
    for d, s, v, kept in cases.NF_PLANTED:
        assert direct[d] == kept and (np.isnan(x[d, s]) if np.isnan(v) else x[d, s] == v), (d, s)
        x_finite = np.where(np.arange(S) == s, 0.75 if s == 0 else 0.5, x[d])
        assert all(lo[k] < x_finite[k] <= hi[k] for k in range(S))        # the planted value alone decides
    assert 20 < want["n_kept"] < cases.NF_ND - 20
    # the kept draw with +inf: mean +inf and covariance NaN in its coordinate and the national vote, on the condition day only
    t, o = cases.NF_COND_DAY, cases.NF_OTHER_DAY
    assert want["mean"][t, 1] == INF == want["mean"][t, S] and np.isfinite(np.delete(want["mean"][t], [1, S])).all() and np.isfinite(want["mean"][o]).all()
    nan = np.zeros((S + 1, S + 1), bool)
    nan[[1, S], :] = nan[:, [1, S]] = True
    assert np.array_equal(np.isnan(want["cov"][t]), nan) and np.isfinite(want["cov"][o]).all()
    # no condition, one NaN on the other day: that coordinate's and the national vote's row and column, on that day only
    free_want = cases.nonfinite_reference(False)
    d, s = cases.NF_FREE_NAN
    assert np.isnan(free[d, o, s]) and np.isfinite(free).sum() == free.size - 1
    assert free_want["n_kept"] == cases.NF_ND
    nan = np.zeros((S + 1, S + 1), bool)
    nan[[s, S], :] = nan[:, [s, S]] = True
    assert np.array_equal(np.isnan(free_want["cov"][o]), nan) and np.isfinite(free_want["cov"][t]).all()
    assert np.array_equal(np.isnan(free_want["mean"]), np.isin(np.arange(2 * (S + 1)).reshape(2, S + 1), [o * (S + 1) + s, o * (S + 1) + S]))
    # the tipping point does not hang on where a NaN score is ranked: the other states reach the bar without it (the kernel ranks it nowhere,
    # the vectorised restatement last, and a literal sort has no order for it)
    assert ev.sum() - ev[s] >= cases.W270 and ev[s] < cases.W270
    assert free_want["tipping"][:, S].sum() == 0 and (free_want["tipping"].sum(1) == cases.NF_ND).all()


def test_the_day_block_case_splits_as_stated():
    want = cases.dayblock_reference()
    n, S, T = want["n_kept"], cases.DAYBLOCK_S, cases.DAYBLOCK_DAYS
    assert 100 < n < cases.SC_CHUNK and (S + 1 + 15) // 16 == 3
    per_day = cases.scratch_per_day(n, S)
    assert per_day == (n + 34 + 34 * 34) * 8
    assert cases.day_blocks(T, per_day, cases.SC_SCRATCH_BUDGET) == [5]
    assert cases.day_blocks(T, per_day, per_day) == [1] * 5 and cases.day_blocks(T, per_day, 2 * per_day) == [2, 2, 1]
    assert cases.day_blocks(T, per_day, 2 * per_day - 1) == [1] * 5 and cases.day_blocks(T, per_day, 1) == [1] * 5
    m = want["mean"]
    assert all(not np.array_equal(m[t], m[0]) for t in range(1, T))       # a launch that read another day's mean would show
