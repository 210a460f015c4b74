"""Shapes at the edges of the batches of the counting and moment kernels (csrc/potus_outcomes.hpp, csrc/potus_scenario.hpp and their launch
code oc_count / sc_compute in csrc/potus_hmc.hip) with their inputs and restatements, shared by tests/test_gpu_count_edges.py (the kernels,
through outcomes_of_block and scenario_of_block) and tests/test_count_edges_host.py (the constants and the restated launch rules against the
sources' text, the preconditions of every case, the fast restatement against the literal one).  The blocks are those of the existing tests
(_built_block, _grid_weights, _integer_ev): scores and weights are multiples of 2^-10, so the national vote is exact in any order and the
means are bit-equal.  Every builder is seeded by its shape, cached, and hands out read-only arrays."""
import functools
import math

import numpy as np

import outcomes_ref
import scenario_ref as ref
from test_gpu_scenario import LOOSE, TIGHT, _built_block, _grid_weights, _integer_ev

# ---- the constants the kernels cut their work by (test_count_edges_host.py holds them to the headers)
OC_THREADS = 256
OC_WAVES = OC_THREADS // 64                 # k_oc_count: one wave per (draw, day) item, the waves of a workgroup take a chunk's draws in turn
OC_FOLD = 64                                # items whose indicator bits a wave holds before it folds them into the workgroup's joint counts
OC_MAX_S = 63
OC_WORKGROUPS = 2048                        # oc_count aims at this many workgroups over days x chunks
SC_THREADS = 256
SC_KEEP_BLOCK = 256                         # draws per kept count, per workgroup of k_sc_keep / k_sc_compact
SC_SCAN_ROUND = 64                          # block counts k_sc_scan takes per round (one wave)
SC_CHUNK = 1024                             # kept draws per partial sum of the moments
SC_SLICE = 512                              # doubles of a row per slice of k_sc_compact, ...
SC_MAX_SLICES = 64                          # ... at most this many slices
SC_SCRATCH_BUDGET = 256 << 20               # bytes of nat and chunk partials per launch of the moments (POTUS_SCENARIO_SCRATCH_BUDGET overrides)
W270 = 270


# ---- the launch rules, restated
def oc_chunks(nd, n_days):
    """oc_count's chunk rule -> (chunks, draws per chunk, items of the busiest wave): wave 0 of the first chunk, every fourth of its draws"""
    chunks = min(max(1, OC_WORKGROUPS // n_days), (nd + 63) // 64)
    chunks = max(chunks, (nd + (1 << 30) - 1) >> 30)
    chunk = (nd + chunks - 1) // chunks
    chunks = (nd + chunk - 1) // chunk
    return chunks, chunk, (min(chunk, nd) + OC_WAVES - 1) // OC_WAVES


def wave_items(chunk_draws):
    """items of waves 0 .. 3 of a workgroup of k_oc_count whose chunk holds this many draws"""
    return [len(range(w, chunk_draws, OC_WAVES)) for w in range(OC_WAVES)]


def keep_blocks(nd):
    """-> (blocks of SC_KEEP_BLOCK draws, rounds of k_sc_scan, draws of the last block)"""
    nblk = (nd + SC_KEEP_BLOCK - 1) // SC_KEEP_BLOCK
    return nblk, (nblk + SC_SCAN_ROUND - 1) // SC_SCAN_ROUND, nd - (nblk - 1) * SC_KEEP_BLOCK


def compact_slices(rowlen):
    """-> (slices of k_sc_compact, [(e0, e1) of every slice])"""
    n = min(max(1, rowlen // SC_SLICE), SC_MAX_SLICES)
    return n, [(rowlen * y // n, rowlen * (y + 1) // n) for y in range(n)]


def scratch_per_day(n_kept, S, want_cov=True):
    """bytes of sc_compute's scratch per day of a launch: nat of every kept draw and the chunk partials of the sums and the Gram matrix"""
    C = S + 1
    nchunks = (n_kept + SC_CHUNK - 1) // SC_CHUNK
    return (n_kept + nchunks * (C + (C * C if want_cov else 0))) * 8


def day_blocks(n_days, per_day, budget):
    """days of every launch of the moments under a scratch budget"""
    dblk = min(n_days, max(1, budget // per_day))
    return [min(dblk, n_days - d0) for d0 in range(0, n_days, dblk)]


# ---- helpers
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def restate(ps, w, cond_day, lo=None, hi=None, ev=None, want_cov=True):
    """scenario_ref.scenario with the counts of outcomes_ref.outcomes_vectorised instead of the literal loop over (draw, day) -- for the
    cases with many days or draws (test_count_edges_host.py holds the two equal) and for the non-finite scores, whose place in the
    tipping-point order the vectorised form defines (last) and the literal sort does not.  The keep mask is scenario_ref.keep_mask, the
    national vote the in-order sum with every product and sum rounded on its own, the mean math.fsum / n, the covariance
    scenario_ref.moments (np.longdouble); want_cov = False leaves it out."""
    ps = np.asarray(ps, dtype=np.float64)
    nd, ndays, S = ps.shape
    with np.errstate(invalid="ignore"):
        keep, nat_cond = ref.keep_mask(ps[:, cond_day, :], w, lo, hi)
        kept = ps[keep]
        n = len(kept)
        out = dict(keep=keep, nat_cond=nat_cond, n_kept=n, n_draws=nd)
        oc = outcomes_ref.outcomes_vectorised(kept, w, [0] * S if ev is None else ev, W270)
        if ev is not None:
            out.update(ev_hist=oc["ev_hist"], tipping=oc["tipping"], joint=oc["joint"])
        nat = np.zeros((n, ndays))
        for s in range(S):
            nat = nat + float(w[s]) * kept[:, :, s]
        out["nat"] = nat
        x = np.concatenate([kept, nat[:, :, None]], axis=2)
        if want_cov:
            out["mean"], out["cov"] = ref.moments(x)
        else:
            out["mean"] = np.array([[math.fsum(x[:, t, c]) / n for c in range(S + 1)] for t in range(ndays)]) if n else np.full((ndays, S + 1), np.nan)
            out["cov"] = None
    return out


def bounds(given, S):
    from us_potus_model_amd import scenario as sc
    return sc.parse_given(given, S)


# ---- 1. the 64-item fold of k_oc_count
# n_days in 1025 .. 2048: one chunk, so a workgroup takes all nd draws and wave w every fourth from w on
FOLD_DAYS = 1025
FOLD_CASES = (                              # (S, nd, n_days): what the busiest wave reaches
    (3, 255, FOLD_DAYS),                    # 64, 64, 64, 63 items: wave 3 one short of a fold, its bit 63 never set
    (3, 256, FOLD_DAYS),                    # every wave exactly 64: the fold in the loop, no remainder (`if (k)` after the reset)
    (3, 257, FOLD_DAYS),                    # wave 0 has 65: a remainder of one item after the reset
    (3, 512, FOLD_DAYS),                    # exactly two folds: the LDS counters take a second one
    (3, 513, FOLD_DAYS),                    # wave 0 has 129
    (OC_MAX_S, 257, FOLD_DAYS),             # every lane a state
    (3, 770, 600),                          # three chunks of 257, 257 and 256 draws
)
FOLD_BUSIEST = {255: 64, 256: 64, 257: 65, 512: 128, 513: 129, 770: 65}


@functools.lru_cache(maxsize=2)
def fold_case(S, nd, n_days):
    """-> (ps [nd, n_days, S], w, ev, actual)"""
    rng = np.random.default_rng(100000 * S + 1000 * nd + n_days)
    ps, w, ev = _built_block(rng, nd, n_days, S), _grid_weights(rng, S), _integer_ev(rng, S, 538)
    actual = rng.integers(0, 1025, S) / 1024.0          # on the grid: `x < actual` meets equality
    return _frozen(ps, w, ev, actual)


@functools.lru_cache(maxsize=None)
def fold_reference(S, nd, n_days):
    ps, w, ev, actual = fold_case(S, nd, n_days)
    return outcomes_ref.outcomes_vectorised(ps, w, ev, W270, actual)


# ---- 2. keep, scan and compact: S = 3, one day, "state 0 wins" with the scores of state 0 set by hand
SCAN_S = 3
SCAN_ND = (255, 256, 257, 16384, 16385, 33025)
SCAN_BLOCKS = {255: (1, 1, 255), 256: (1, 1, 256), 257: (2, 1, 1), 16384: (64, 1, 256), 16385: (65, 2, 1), 33025: (130, 3, 1)}
SCAN_EMPTY_BLOCK = 70                       # a whole block of the second scan round that keeps nothing (where there are that many blocks)
SCAN_GIVEN = {0: "win"}


def planted_keep(nd, rng):
    """About half the draws, and by hand: with three blocks or more the first block keeps nothing and the second all 256; wave 2 (draws 128 .. 191)
    of a block that keeps others keeps nothing; block SCAN_EMPTY_BLOCK keeps nothing; the last draw is kept."""
    B = SC_KEEP_BLOCK
    nblk = keep_blocks(nd)[0]
    keep = rng.random(nd) < 0.5
    if nblk >= 3:
        keep[:B] = False
        keep[B:2 * B] = True
    wb = idle_wave_block(nd)
    keep[wb * B + 128:wb * B + 192] = False
    if nblk > SCAN_EMPTY_BLOCK:
        keep[SCAN_EMPTY_BLOCK * B:(SCAN_EMPTY_BLOCK + 1) * B] = False
    keep[nd - 1] = True
    return keep


def idle_wave_block(nd):
    return 2 if keep_blocks(nd)[0] >= 3 else 0


def planted_scores(keep, rng):
    """scores of state 0 on the grid that "state 0 wins" keeps exactly where `keep` says: above one half there, elsewhere below it and --
    every third draw -- exactly on the bound, which the strict rule leaves out"""
    n = len(keep)
    return np.where(keep, rng.integers(513, 1025, n), np.where(np.arange(n) % 3 == 0, 512, rng.integers(0, 512, n))) / 1024.0


@functools.lru_cache(maxsize=None)
def scan_case(nd):
    """-> (ps [nd, 1, 3], w, ev, planted keep)"""
    rng = np.random.default_rng(7000 + nd)
    ps, w, ev = _built_block(rng, nd, 1, SCAN_S), _grid_weights(rng, SCAN_S), _integer_ev(rng, SCAN_S, 538)
    keep = planted_keep(nd, rng)
    ps[:, 0, 0] = planted_scores(keep, rng)
    return _frozen(ps, w, ev, keep)


@functools.lru_cache(maxsize=None)
def scan_reference(nd):
    ps, w, ev, _ = scan_case(nd)
    return restate(ps, w, 0, *bounds(SCAN_GIVEN, SCAN_S), ev=ev)


# ---- 3. the slices of k_sc_compact: rowlen = n_days * S
SLICE_ND = 300
SLICE_CASES = ((73, 7), (64, 16), (41, 25), (53, 29), (700, 47))        # (n_days, S)
SLICE_ROWLEN = {(73, 7): (511, 1), (64, 16): (1024, 2), (41, 25): (1025, 2), (53, 29): (1537, 3), (700, 47): (32900, 64)}   # rowlen, slices


@functools.lru_cache(maxsize=2)
def slice_case(n_days, S):
    rng = np.random.default_rng(3000 * S + n_days)
    return _frozen(_built_block(rng, SLICE_ND, n_days, S), _grid_weights(rng, S), _integer_ev(rng, S, 538))


@functools.lru_cache(maxsize=None)
def slice_reference(n_days, S):
    """the loose condition on the last day; means and counts (compaction shows in every output)"""
    ps, w, ev = slice_case(n_days, S)
    return restate(ps, w, n_days - 1, *bounds(LOOSE, S), ev=ev, want_cov=False)


# ---- 4. chunk and step tails of the moments
TAIL_S, TAIL_DAYS = 17, 2                   # S + 1 = 18: the national column in the second operand tile
# k_sc_gram: steps of four draws dealt to four waves -- 2 .. 5: waves 1 - 3 have no step (5: wave 1 one draw); 15, 16, 17: one round of the waves
# less a draw, exactly, and a draw; SC_CHUNK - 1, SC_CHUNK, SC_CHUNK + 1 (a second chunk of one draw), two chunks, two and a draw
TAIL_ND = (2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 2048, 2049)
TAIL_KEPT = (1024, 1025)                    # the same chunk edge behind a compaction: kept draws chosen by hand among TAIL_KEPT_ND
TAIL_KEPT_ND = 3000
TRIPLE_S = (1, 2, 16, 31, 32, 48)           # S + 1 = 2, 3, 17, 32, 33, 49: at 17, 33 and 49 the national column sits alone in its operand tile
TRIPLE_ND, TRIPLE_DAYS = 515, 3


@functools.lru_cache(maxsize=None)
def tail_case(nd):
    rng = np.random.default_rng(4000 + nd)
    return _frozen(_built_block(rng, nd, TAIL_DAYS, TAIL_S), _grid_weights(rng, TAIL_S), _integer_ev(rng, TAIL_S, 538))


@functools.lru_cache(maxsize=None)
def tail_reference(nd):
    ps, w, ev = tail_case(nd)
    return ref.scenario(ps, w, TAIL_DAYS - 1, None, None, ev=ev)


@functools.lru_cache(maxsize=None)
def tail_kept_case(n_kept):
    """-> (ps [3000, 2, 17], w, ev, keep): exactly n_kept draws, chosen by the generator, have state 0 above one half on the last day"""
    rng = np.random.default_rng(5000 + n_kept)
    ps, w, ev = _built_block(rng, TAIL_KEPT_ND, TAIL_DAYS, TAIL_S), _grid_weights(rng, TAIL_S), _integer_ev(rng, TAIL_S, 538)
    keep = np.zeros(TAIL_KEPT_ND, bool)
    keep[rng.choice(TAIL_KEPT_ND, n_kept, replace=False)] = True
    ps[:, TAIL_DAYS - 1, 0] = planted_scores(keep, rng)
    return _frozen(ps, w, ev, keep)


@functools.lru_cache(maxsize=None)
def tail_kept_reference(n_kept):
    ps, w, ev, _ = tail_kept_case(n_kept)
    return ref.scenario(ps, w, TAIL_DAYS - 1, *bounds(SCAN_GIVEN, TAIL_S), ev=ev)


def triple_givens(S):
    """the tight, loose and no-condition triple of tests/test_gpu_scenario.py; one state: the tight condition is the state and the national bound"""
    tight = TIGHT if S > 1 else {k: v for k, v in TIGHT.items() if k != 1}
    return (("tight", tight), ("loose", LOOSE), ("none", None))


@functools.lru_cache(maxsize=None)
def triple_case(S):
    rng = np.random.default_rng(6000 + S)
    return _frozen(_built_block(rng, TRIPLE_ND, TRIPLE_DAYS, S), _grid_weights(rng, S), _integer_ev(rng, S, 538))


@functools.lru_cache(maxsize=None)
def triple_reference(S, name):
    ps, w, ev = triple_case(S)
    return ref.scenario(ps, w, TRIPLE_DAYS - 1, *bounds(dict(triple_givens(S))[name], S), ev=ev)


# ---- 5. non-finite scores: S = 5, 300 draws, two days, the condition on the last
NF_S, NF_ND, NF_DAYS, NF_COND_DAY, NF_OTHER_DAY = 5, 300, 2, 1, 0
NF_GIVEN = {0: "win", 1: (0.25, None), 2: (None, 0.75)}                 # states 3 and 4 and the national vote are free
# (draw, state, value, kept): every planted draw meets the condition in its other coordinates, so the planted value alone decides
NF_PLANTED = ((10, 0, np.nan, False),       # a NaN in a conditioned state
              (20, 4, np.nan, False),       # a NaN in a free state: it is in no interval, (-inf, +inf] among them
              (30, 1, np.inf, True),        # +inf under hi = +inf: lo < x <= hi holds
              (40, 2, -np.inf, False))      # -inf over lo = -inf: the lower bound is strict
NF_FREE_NAN = (50, 3)                       # (draw, state) of the one NaN on the other day of the unconditioned block


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    """-> (conditioned block, unconditioned block, w, ev): the first holds NF_PLANTED on the condition day, the second one NaN on the other day"""
    rng = np.random.default_rng(55)
    base, w, ev = _built_block(rng, NF_ND, NF_DAYS, NF_S), _grid_weights(rng, NF_S), _integer_ev(rng, NF_S, 538)
    cond = base.copy()
    for d, s, v, _ in NF_PLANTED:
        cond[d, NF_COND_DAY, :3] = (0.75, 0.5, 0.5)
        cond[d, NF_COND_DAY, s] = v
    free = base.copy()
    free[NF_FREE_NAN[0], NF_OTHER_DAY, NF_FREE_NAN[1]] = np.nan
    return _frozen(cond, free, w, ev)


@functools.lru_cache(maxsize=None)
def nonfinite_reference(conditioned):
    cond, free, w, ev = nonfinite_case()
    if conditioned:
        return restate(cond, w, NF_COND_DAY, *bounds(NF_GIVEN, NF_S), ev=ev)
    return restate(free, w, NF_COND_DAY, None, None, ev=ev)


# ---- 6. the day-block loop of sc_compute
DAYBLOCK_S, DAYBLOCK_DAYS, DAYBLOCK_ND = 33, 5, 1500


@functools.lru_cache(maxsize=None)
def dayblock_case():
    rng = np.random.default_rng(66)
    return _frozen(_built_block(rng, DAYBLOCK_ND, DAYBLOCK_DAYS, DAYBLOCK_S), _grid_weights(rng, DAYBLOCK_S), _integer_ev(rng, DAYBLOCK_S, 538))


@functools.lru_cache(maxsize=None)
def dayblock_reference():
    ps, w, ev = dayblock_case()
    return ref.scenario(ps, w, DAYBLOCK_DAYS - 1, *bounds(LOOSE, DAYBLOCK_S), ev=ev)
